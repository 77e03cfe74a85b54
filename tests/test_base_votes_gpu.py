"""Per-base calls on the card (csrc/base_votes.hpp through the C ABI) against ``base_votes.vote_host``, byte for byte and without a
tolerance: every launch shape and edge of the vote, the recipe batch, a whole round through the shipped checkpoint, and the calls of
whole reads in base coordinates.  Forged tables are tested on the CPU only (tests/test_base_votes_replay.py)."""
import numpy as np
import pytest

from catfish_amd import base_votes as bv
from catfish_amd import device_validation as dv
from catfish_amd import labelling
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from test_base_votes_host import (RECIPE_THRESHOLDS, SHAPE_THRESHOLDS, assert_recipe_is_not_vacuous, recipe_batch, shape_batch, vote_of)

pytestmark = pytest.mark.gpu


def on_device(vset, selection, packed, thresholds, max_bases):
    import torch
    got = bv.vote_device(torch.from_numpy(packed).to("cuda:0"), vset, selection, thresholds, max_bases)
    torch.cuda.synchronize()
    sums, state, confusion, runs = (t.cpu().numpy() for t in got)
    return sums.view(np.uint64), state, confusion, runs


def assert_same_bytes(got, want):
    for name, a, b in zip(("sums", "state", "base_confusion", "base_vote_runs"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


@pytest.fixture(scope="module")
def shapes():
    """The shape batch and its reference, computed once: 17 thresholds (two launch groups) at 32 bins."""
    vset, selection, packed = shape_batch()
    return vset, selection, packed, vote_of(vset, selection, packed, SHAPE_THRESHOLDS, 32)


def lumped(runs, max_bases):
    """A [..., 33] run table at fewer bins: the upper bins lumped into the last."""
    return np.concatenate((runs[..., :max_bases], runs[..., max_bases:].sum(axis=-1, keepdims=True)), axis=-1)


@pytest.mark.parametrize("k", (1, 16, 17))
def test_the_shape_batch_equals_the_host_statement(shapes, k):
    """Bases of 1, 2, 63, 64, 65 and 4097 samples and the neighbours of the long-base constant, a read of one base, stretches that start
    and end mid-event and on a border, one that holds no whole event, two neighbours of one read, called runs at both ends of a
    stretch, every letter class, NaN / -1 / 2 / inf and means exactly at a threshold; K = 17 is two launch groups."""
    vset, selection, packed, (sums, state, confusion, runs) = shapes
    got = on_device(vset, selection, packed, SHAPE_THRESHOLDS[:k], 32)
    print("voted bases:", int(np.count_nonzero(got[1][0] & bv.VOTED)), "confusion at 0.5:", got[2][0].sum(axis=0).tolist())
    assert_same_bytes(got, (sums, state[:k], confusion[:k], runs[:k]))
    assert vset.uploads == 1


@pytest.mark.parametrize("max_bases", (32, 1))
def test_a_run_of_33_bases_at_both_ends_of_the_bin_range(shapes, max_bases):
    vset, selection, packed, (sums, state, confusion, runs) = shapes
    got = on_device(vset, selection, packed, SHAPE_THRESHOLDS[:2], max_bases)
    assert_same_bytes(got, (sums, state[:2], confusion[:2], lumped(runs[:2], max_bases)))
    assert got[3][0, 0, :, 3, max_bases].sum() >= 1 and got[3][0, 1, :, 3, max_bases].sum() >= 1          # the 33 T, true and called


def test_the_recipe_batch_equals_the_host_statement_twice():
    vset, selection, packed, _reads = recipe_batch()
    want = vote_of(vset, selection, packed, RECIPE_THRESHOLDS, 16)
    assert_recipe_is_not_vacuous(want[2], want[3])
    first = on_device(vset, selection, packed, RECIPE_THRESHOLDS, 16)
    print("confusion:", first[2].sum(axis=1).tolist(), "states:", first[3].sum(axis=(3, 4)).tolist())
    assert_same_bytes(first, want)
    assert_same_bytes(on_device(vset, selection, packed, RECIPE_THRESHOLDS, 16), first)                  # two calls give equal bytes


def test_a_whole_round_and_whole_reads_through_the_shipped_checkpoint(hp, ckpt_weights):
    """``base_confusion`` and ``base_vote_runs`` of score_validation_device are vote_host of the round's own probabilities; everything
    else is the bits of the round without them, which returns a tuple of today's length and allocates nothing new; the calls of whole
    reads equal ``call_bases_host`` on the same probabilities."""
    from catfish_amd.resnet_class import ResNetRNN
    _vset, selection, _packed, reads = recipe_batch()
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in reads])
    resident = DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5)
    assert resident.uploads == 1 and resident.bases.n_bases == batch.n_events
    net = ResNetRNN(**hp)
    net.set_weights(ckpt_weights)
    plain = net.score_validation_device(resident, selection, (0.3, 0.5), vote_bases=None)
    assert len(plain) == 3 and plain.base_confusion is None and plain.base_vote_runs is None
    assert sorted(net.validation_buffers["capacity"]) == ["reads", "samples", "slots", "thresholds"]
    assert sorted(net.validation_buffers["tensors"]) == ["logits", "out", "partials", "probs", "table", "x", "y"]
    got = net.score_validation_device(resident, selection, (0.3, 0.5), vote_bases=16)
    allocations = net.validation_buffers["allocations"]
    assert len(got) == 5 and got.base_confusion is got[3] and got.base_vote_runs is got[4]
    for a, b in zip(plain, got[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    bounds, _tails = dv.layout(selection[2], 35)
    total = int(bounds[-1])
    probs = net.validation_buffers["tensors"]["probs"][:total].cpu().numpy()
    _sums, _state, confusion, runs = vote_of(resident, selection, probs, (0.3, 0.5), 16)
    print("voted bases:", int(confusion[0].sum()), "confusion:", confusion.sum(axis=1).tolist())
    assert got.base_confusion.dtype == np.int64 and np.array_equal(got.base_confusion, confusion) and confusion[0].sum() == 973
    assert got.base_vote_runs.dtype == np.int64 and np.array_equal(got.base_vote_runs, runs) and runs[:, 0].sum() > 0
    again = net.score_validation_device(resident, selection, (0.3, 0.5), vote_bases=16)
    assert net.validation_buffers["allocations"] == allocations and resident.uploads == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    # the sweep's rows carry the table and the per-base rates
    rows = tv.threshold_sweep(net, resident, (0.3, 0.5), 0, vote_bases=16)
    whole = net.score_validation_device(resident, resident.select(35, 0, "complete", 856), (0.3, 0.5), vote_bases=16)
    for k, row in enumerate(rows):
        assert row["base_confusion"] == whole.base_confusion[k].tolist() and row["voted_bases"] == batch.n_events
        assert row["base_recall"] == bv.base_vote_rates(whole.base_confusion[k])["base_recall"] and len(row["base_f1_by_base"]) == 5
        assert row["vote_runs"] == dv.run_base_rates(whole.base_vote_runs[k])
    # whole reads, in base coordinates
    calls = net.call_bases_device(resident, 0.5)
    complete = resident.select(35, 0, "complete", 856)
    bounds, _tails = dv.layout(complete[2], 35)
    probs = net.validation_buffers["tensors"]["probs"][:int(bounds[-1])].cpu().numpy()
    per_read = [probs[b0:b0 + n] for b0, n in zip(bounds[:-1].tolist(), complete[2].tolist())]
    want = bv.call_bases_host(per_read, [bases for _raw, bases, _l in reads], [lengths for _raw, _b, lengths in reads], 0.5)
    print("calls per read:", [len(c) for c in calls])
    assert calls == want and len(calls) == 3
    # sets without a base table are refused before anything is launched
    labels = resident.labels
    bare = DeviceValidationSet.from_arrays([raw for raw, _b, _l in reads], [labels[a:b] for a, b in zip(batch.sample_offsets, batch.sample_offsets[1:])])
    for call in (lambda: net.score_validation_device(bare, selection, (0.5,), vote_bases=16), lambda: net.call_bases_device(bare)):
        with pytest.raises(ValueError, match="from_events / from_moves"):
            call()
    net.engine.close()


def test_refusals_arrive_as_value_errors():
    """Argument errors only, refused on the host before any launch."""
    import ctypes as C
    import torch
    from catfish_amd import _native as N
    vset, selection, packed, _reads = recipe_batch()
    probs = torch.from_numpy(packed).to("cuda:0")
    for bad in (0, 33, True, 16.0):
        with pytest.raises(ValueError):
            bv.vote_device(probs, vset, selection, (0.5,), bad)
    with pytest.raises(ValueError):
        bv.vote_device(probs, vset, selection, (), 16)
    with pytest.raises(ValueError):
        bv.vote_device(probs[:100], vset, selection, (0.5,), 16)
    with pytest.raises(ValueError):
        bv.vote_device(probs.double(), vset, selection, (0.5,), 16)
    lib = N.lib()
    one = (C.c_double * 1)(0.5)
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
    p = C.c_void_p(buf.data_ptr())
    good = [None, p, 64, p, p, 64, p, 8, p, p, p, p, 1, 8, one, 1, 16, p, p, p, 4096 * 8, None]
    assert lib.cf_base_votes(*good) == 0
    for position, value in ([(i, None) for i in (1, 3, 4, 6, 8, 9, 10, 11, 14, 17, 18, 19)]
                            + [(2, -1), (2, 2 ** 31), (5, -1), (5, 2 ** 31), (7, -1), (7, 2 ** 31), (12, -1), (12, 2 ** 31), (15, 0), (15, 17),
                               (16, 0), (16, 33), (20, 8 * 9 - 1)]):
        args = list(good)
        args[position] = value
        with pytest.raises(ValueError):
            N.check(lib.cf_base_votes(*args))
    for position in (2, 5, 7, 12):                         # zero voted work is fine: the zeroed tables
        args = list(good)
        args[position] = 0
        buf.fill_(-1)
        assert lib.cf_base_votes(*args) == 0
        torch.cuda.synchronize()
        assert not buf[:20].any()
    torch.cuda.synchronize()


def test_the_report_line_of_a_training_run(tmp_path, monkeypatch):
    """CATFISH_VALIDATION_VOTES appends one JSON line per checkpoint round and leaves both .txt reports as they are without it."""
    import json
    import os
    for name, seeds in (("train", (70, 71)), ("val", (50, 51, 52))):
        (tmp_path / name).mkdir()
        for i, seed in enumerate(seeds):
            raw, bases, lengths = labelling.synthetic_event_read(12000 if name == "train" else 3000 + 36 * i, seed, hp_fraction=0.2)
            np.savez(tmp_path / name / ("e%d.npz" % i), raw=raw, event_base=bases, event_length=lengths)
    real_build = tv.build_model

    def seeded(kind, **kw):                                # main() draws its weights and its dropout from the clock: pin both
        network = real_build(kind, **dict(kw, train_seed=0))
        init = network.initialize_network
        network.initialize_network = lambda seed=None: init(seed=4)
        return network

    monkeypatch.setattr(tv, "build_model", seeded)
    monkeypatch.setenv("CATFISH_SHIPPED_HPARAMS", "1")
    monkeypatch.setenv("CATFISH_LABEL_KMER", "5")
    for name in ("CATFISH_DEVICE_DB", "CATFISH_NATIVE_TRAINING", "CATFISH_TRAINING_PRECISION", "CATFISH_VALIDATION_RUNS", "CATFISH_VALIDATION_BASES",
                 "CATFISH_VALIDATION_BORDERS", "CATFISH_VALIDATION_CURVE", "CATFISH_VALIDATION_BRIDGE", "CATFISH_DEVICE_VALIDATION", "CATFISH_LABEL_MOVES"):
        monkeypatch.delenv(name, raising=False)
    argv = ["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"]
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CATFISH_VALIDATION_VOTES", "1")
    with pytest.raises(ValueError, match="CATFISH_VALIDATION_VOTES needs"):            # the reads must live on the card
        tv.main(argv)
    monkeypatch.setenv("CATFISH_DEVICE_VALIDATION", "1")
    reports = {}
    for switch in ("0", "12"):
        (tmp_path / switch).mkdir()
        monkeypatch.chdir(tmp_path / switch)
        monkeypatch.setenv("CATFISH_VALIDATION_VOTES", switch)
        tv.main(argv)
        (model_dir,) = [d for d in (tmp_path / switch).iterdir() if d.is_dir()]
        with open(str(model_dir) + ".txt") as fh:
            model_report = fh.read()
        with open(model_dir.name + ".txt") as fh:
            reports[switch] = (model_report, fh.read())
        lines_at = str(model_dir) + "_base_votes.jsonl"
        if switch == "0":
            assert not os.path.exists(lines_at)
            continue
        with open(lines_at) as fh:
            (line,) = fh.read().splitlines()
        record = json.loads(line)
        assert record["step"] == 20 and record["threshold"] == 0.5 and record["max_bases"] == 12
        assert record["classes"] == ["A", "C", "G", "T", "other"] and record["states"] == ["complete", "incomplete", "absent"]
        confusion = np.array(record["base_confusion"])
        assert confusion.shape == (5, 2, 2) and confusion.sum() == record["voted_bases"] > 0 and confusion[:4, 1].sum() > 0
        assert record["base_recall"] == bv.base_vote_rates(confusion)["base_recall"] and len(record["base_precision_by_base"]) == 5
        runs = np.stack((np.array(record["hp_vote_runs"]), np.array(record["called_vote_runs"])))
        assert runs.shape == (2, 3, 5, 13) and runs[0].sum() > 0 and record["recall_by_base"] == dv.run_base_rates(runs)["recall_by_base"]
    assert "Saved checkpoint at step 20" in reports["0"][0] and "---NEXT ROUND OF VALIDATION---" in reports["0"][1]
    assert reports["0"] == reports["12"]
