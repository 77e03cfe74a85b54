"""The base step on the card (csrc/validation_bases.hpp through the C ABI) against ``device_validation.run_bases_host``: planted
runs and base maps straight into the kernel, a whole round through a real model on reads labelled on the card, the sweep and the
per-round JSON line, and the host-side refusals."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import labelling
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from test_run_bases_replay import lumped, pack_base_stretches, planted_base_stretches, set_base_map

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.5, 0.3, 0.7, 0.1, float(np.float32(0.1)), 0.9, float(np.float32(0.9)), 0.0, 1.0, 0.5 + 1e-12, 0.5 - 1e-12,
              float(np.nextafter(np.float32(0.5), np.float32(1.0))), float(np.nextafter(np.float32(0.5), np.float32(0.0))), 0.25, 0.75, 0.6)


@pytest.fixture(scope="module")
def engine(ckpt_weights):
    from catfish_amd.engine import HipEngine
    eng = HipEngine(ckpt_weights)
    yield eng
    eng.close()


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


@pytest.fixture(scope="module")
def planted(engine):
    """The planted batch, packed as a round packs it, with the base map as a set keeps it (every stretch starts mid-read), and its
    reference (computed once: 16 thresholds at 32 bins; fewer bins lump the upper ones -- tests/test_run_bases_host.py)."""
    piece = int(engine._lib.cf_validation_run_piece())
    assert piece >= 4096 and piece % 64 == 0
    stretches = planted_base_stretches(piece)
    probs, y, packed_map, bounds, lengths = pack_base_stretches(stretches)
    set_map, src_first = set_base_map(stretches)
    for r in (0, len(stretches) // 2, len(stretches) - 1):         # the set's map holds what the packed one holds, further in
        b0, s0, n = int(bounds[r]), int(src_first[r]), int(lengths[r])
        assert s0 > 0 and np.array_equal(set_map[s0:s0 + n], packed_map[b0:b0 + n])
    want = dv.run_bases_host(probs, y, packed_map, bounds, lengths, THRESHOLDS, 32)
    assert want[0].sum(axis=-1).min() >= 1 and want[0].sum(axis=(0, 1, 2)).min() >= 1      # every (kind, state, class) and every bin at 0.5
    assert lumped(want, 16)[0].sum(axis=(0, 1, 2)).min() >= 1
    return {"probs": _dev(probs), "y": _dev(y), "basemap": _dev(set_map), "src_first": _dev(src_first), "bounds": _dev(bounds),
            "length": _dev(lengths), "total": int(bounds[-1]), "longest": int(np.diff(bounds).max()), "want": want,
            "host": (probs, y, packed_map, bounds, lengths), "set_map": set_map}


def run_bases_on_device(engine, case, thresholds, max_bases, min_run=15, max_gap=0, longest=None):
    import torch
    k = len(thresholds)
    counts = torch.full((k * 2 * 3 * 5 * (max_bases + 1),), -1, dtype=torch.int64, device="cuda:0")
    work = torch.full((max(engine.run_states_work_bytes(case["total"], k), 1),), 7, dtype=torch.uint8, device="cuda:0")
    engine.run_bases_validation(case["probs"], case["y"], case["basemap"], case["src_first"], case["bounds"], case["length"], case["total"],
                                case["longest"] if longest is None else longest, thresholds, max_bases, counts, work, min_run=min_run,
                                max_gap=max_gap)
    torch.cuda.synchronize()
    engine.check_error()
    return counts.cpu().numpy().reshape(k, 2, 3, 5, max_bases + 1)


@pytest.mark.parametrize("k", (1, 16))
@pytest.mark.parametrize("max_bases", (1, 16, 32))
def test_planted_runs_equal_the_host_statement(engine, planted, k, max_bases):
    """Bit-equal to run_bases_host, twice, whatever the grid hint."""
    want = lumped(planted["want"][:k], max_bases)
    first = run_bases_on_device(engine, planted, THRESHOLDS[:k], max_bases)
    print("runs per (kind, state, class) at 0.5:", first[0].sum(axis=-1).tolist())
    assert np.array_equal(first, want)
    assert np.array_equal(run_bases_on_device(engine, planted, THRESHOLDS[:k], max_bases, longest=0), first)


def test_other_run_rules_single_and_empty_stretches(engine, planted):
    probs, y, packed_map, bounds, lengths = planted["host"]
    for min_run, max_gap in ((1, 5), (1, 0), (15, 5), (65, 0)):
        want = dv.run_bases_host(probs, y, packed_map, bounds, lengths, (0.5,), 16, min_run, max_gap)
        assert np.array_equal(run_bases_on_device(engine, planted, (0.5,), 16, min_run=min_run, max_gap=max_gap), want), (min_run, max_gap)
    r = int(np.argmax(lengths))
    a, n = int(bounds[r]), int(lengths[r])
    one = {"probs": _dev(probs[a:a + n]), "y": _dev(y[a:a + n]), "basemap": _dev(packed_map[a:a + n]), "src_first": _dev(np.int64([0])),
           "bounds": _dev(np.int64([0, n])), "length": _dev(np.int64([n])), "total": n, "longest": n}
    want = dv.run_bases_host(probs[a:a + n], y[a:a + n], packed_map[a:a + n], [0, n], [n], (0.5, 0.95), 5)
    assert np.array_equal(run_bases_on_device(engine, one, (0.5, 0.95), 5), want)
    empty = {"probs": _dev(np.zeros(1, np.float32)), "y": _dev(np.zeros(1, np.uint8)), "basemap": _dev(np.zeros(1, np.uint8)),
             "src_first": _dev(np.int64([0, 0])), "bounds": _dev(np.int64([0, 0, 0])), "length": _dev(np.int64([0, 0])), "total": 0, "longest": 0}
    assert not run_bases_on_device(engine, empty, (0.5,), 16).any()


def test_a_base_map_that_ends_early_holds_no_base_behind_its_end(engine, planted):
    """Every index is checked against the size of the base map: the samples behind it count as samples without a base."""
    probs, y, packed_map, bounds, lengths = planted["host"]
    src_first = planted["src_first"].cpu().numpy()
    keep = int(planted["set_map"].size) // 2
    cut = packed_map.copy()
    for b0, s0, n in zip(bounds[:-1].tolist(), src_first.tolist(), lengths.tolist()):
        cut[b0 + max(0, min(n, keep - s0)):b0 + n] = 0
    want = dv.run_bases_host(probs, y, cut, bounds, lengths, (0.5,), 16)
    assert not np.array_equal(want, lumped(planted["want"][:1], 16))
    short = dict(planted, basemap=planted["basemap"][:keep].clone())
    assert np.array_equal(run_bases_on_device(engine, short, (0.5,), 16), want)


def _event_reads(count=6, size=3000):
    return [labelling.synthetic_event_read(size + 36 * i, seed=80 + i, hp_fraction=0.2) for i in range(count)]


def test_a_whole_round_through_a_real_model(hp):
    """``run_bases`` of score_validation_device is run_bases_host of the round's own probabilities and of the base map made on the
    card; it sums to the round's run states; everything else is the bits of the round without it; a second round allocates nothing."""
    from catfish_amd.resnet_class import ResNetRNN
    reads = _event_reads()
    batch = labelling.EventBatch.from_reads([(bases, lengths, (3, 2)) for _raw, bases, lengths in reads])
    resident = DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5)
    labels, basemap = batch.label_host(5, base_map=True)
    assert resident.uploads == 1 and np.array_equal(resident.basemap, basemap) and np.array_equal(resident.labels, labels)
    selection = (np.int64([0, 2, 3, 5]), np.int64([0, 700, 35, 1]), np.int64([3000, 2000, 3001, 3000 + 36 * 5 - 1]))     # two start mid-read
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    plain = net.score_validation_device(resident, selection, (0.3, 0.5), run_edges=())
    bounds, _tails = dv.layout(selection[2], 35)
    total = int(bounds[-1])
    middle = np.sort(net.validation_buffers["tensors"]["probs"][:total].cpu().numpy())
    thresholds = (0.3, 0.5, float(middle[int(0.5 * (total - 1))]), float(middle[int(0.8 * (total - 1))]))      # ... and scores the model really gives
    plain = net.score_validation_device(resident, selection, thresholds, run_edges=())
    got = net.score_validation_device(resident, selection, thresholds, run_edges=(), max_bases=16)
    allocations = net.validation_buffers["allocations"]
    assert len(plain) == 4 and len(got) == 5 and got.run_bases is got[4] and plain.run_bases is None
    for a, b in zip(plain, got[:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    t = net.validation_buffers["tensors"]
    want = dv.run_bases_host(t["probs"][:total].cpu().numpy(), t["y"][:total].cpu().numpy(), resident.pack_basemap(selection, 35), bounds,
                             selection[2], thresholds, 16)
    print("true runs by base:", want[:, 0].sum(axis=(1, 3)).tolist(), "called runs by base:", want[:, 1].sum(axis=(1, 3)).tolist())
    assert got.run_bases.dtype == np.int64 and np.array_equal(got.run_bases, want)
    assert np.array_equal(got.run_bases.sum(axis=(3, 4)), got.run_states[:, :, 0, :])
    assert want[:, 0, :, :4].sum() > 0 and want[:, 1].sum() > 0          # pure true homopolymers, and something is called
    again = net.score_validation_device(resident, selection, thresholds, run_edges=(), max_bases=16)
    assert net.validation_buffers["allocations"] == allocations and resident.uploads == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    # the sweep's rows carry the tables and the rates
    rows = tv.threshold_sweep(net, resident, thresholds, 0, max_bases=16)
    whole = net.score_validation_device(resident, resident.select(35, 0, "complete", 856), thresholds, max_bases=16).run_bases
    before = tv.threshold_sweep(net, resident, thresholds, 0)
    for k, (row, old) in enumerate(zip(rows, before)):
        assert {key: row[key] for key in old} == old
        assert sorted(set(row) - set(old)) == ["called_bases", "called_pure", "complete_by_base", "complete_by_length", "hp_bases",
                                               "recall_by_base", "recall_by_length"]
        assert row["hp_bases"] == whole[k, 0].tolist() and row["called_bases"] == whole[k, 1].tolist()
        assert row["recall_by_base"] == dv.run_base_rates(whole[k])["recall_by_base"] and len(row["recall_by_length"]) == 17
    # sets without a base map are refused before anything is launched
    for bare in (DeviceValidationSet.from_arrays([raw for raw, _b, _l in reads], [labels[a:b] for a, b in zip(batch.sample_offsets, batch.sample_offsets[1:])]),):
        with pytest.raises(ValueError, match="base map"):
            net.score_validation_device(bare, selection, thresholds, max_bases=16)
    net.engine.close()


def test_a_set_from_labelled_files_has_no_base_map(hp, tmp_path):
    from catfish_amd.resnet_class import ResNetRNN
    paths = []
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(700, seed=50 + i)
        paths.append(str(tmp_path / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    for bare in (DeviceValidationSet.from_npz(paths), DeviceValidationSet.from_arrays([np.zeros(700)], [np.zeros(700, np.uint8)])):
        with pytest.raises(ValueError, match="base map"):
            net.score_validation_device(bare, bare.select(35, 0, "complete", 856), (0.5,), max_bases=16)
        with pytest.raises(ValueError, match="base map"):
            tv.threshold_sweep(net, bare, [0.5], 0, max_bases=16)
    net.engine.close()


def test_the_report_line_of_a_training_run(tmp_path, monkeypatch):
    """CATFISH_VALIDATION_BASES appends one JSON line per checkpoint round and leaves both .txt reports as they are without it."""
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
    for name in ("CATFISH_DEVICE_DB", "CATFISH_NATIVE_TRAINING", "CATFISH_TRAINING_PRECISION", "CATFISH_VALIDATION_RUNS",
                 "CATFISH_VALIDATION_BORDERS", "CATFISH_VALIDATION_CURVE", "CATFISH_VALIDATION_BRIDGE", "CATFISH_DEVICE_VALIDATION"):
        monkeypatch.delenv(name, raising=False)
    argv = ["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"]
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CATFISH_VALIDATION_BASES", "1")
    with pytest.raises(ValueError, match="CATFISH_VALIDATION_BASES needs"):            # the reads must live on the card
        tv.main(argv)
    monkeypatch.setenv("CATFISH_DEVICE_VALIDATION", "1")
    monkeypatch.delenv("CATFISH_LABEL_KMER")
    with pytest.raises(ValueError, match="CATFISH_VALIDATION_BASES needs"):            # ... and come with their event tables
        tv.main(argv)
    monkeypatch.setenv("CATFISH_LABEL_KMER", "5")
    reports = {}
    for switch in ("0", "12"):
        (tmp_path / switch).mkdir()
        monkeypatch.chdir(tmp_path / switch)
        monkeypatch.setenv("CATFISH_VALIDATION_BASES", switch)
        tv.main(argv)
        (model_dir,) = [d for d in (tmp_path / switch).iterdir() if d.is_dir()]
        with open(str(model_dir) + ".txt") as fh:
            model_report = fh.read()
        with open(model_dir.name + ".txt") as fh:
            reports[switch] = (model_report, fh.read())
        lines_at = str(model_dir) + "_hp_bases.jsonl"
        if switch == "0":
            assert not os.path.exists(lines_at)
            continue
        with open(lines_at) as fh:
            (line,) = fh.read().splitlines()
        record = json.loads(line)
        assert record["step"] == 20 and record["threshold"] == 0.5 and record["max_bases"] == 12
        assert record["classes"] == ["A", "C", "G", "T", "other"] and record["states"] == ["complete", "incomplete", "absent"]
        hp_bases, called_bases = np.array(record["hp_bases"]), np.array(record["called_bases"])
        assert hp_bases.shape == called_bases.shape == (3, 5, 13) and hp_bases[:, :4].sum() > 0
        assert record["recall_by_base"] == dv.run_base_rates(np.stack((hp_bases, called_bases)))["recall_by_base"]
        assert len(record["recall_by_length"]) == 13 and 0 <= record["called_pure"] <= 1
    assert "Saved checkpoint at step 20" in reports["0"][0] and "---NEXT ROUND OF VALIDATION---" in reports["0"][1]
    assert reports["0"] == reports["12"]


def test_refusals_arrive_as_value_errors(engine, planted):
    """Argument errors only, refused on the host before any launch; the engine stays usable."""
    import ctypes as C
    import torch
    from catfish_amd import _native as N

    def call(case=planted, work=None, counts=None, max_bases=16, thresholds=(0.5,)):
        k = max(len(thresholds), 1)
        counts = torch.zeros(k * 2 * 3 * 5 * 33, dtype=torch.int64, device="cuda:0") if counts is None else counts
        work = torch.zeros(max(engine.run_states_work_bytes(case["total"], k), 1), dtype=torch.uint8, device="cuda:0") if work is None else work
        engine.run_bases_validation(case["probs"], case["y"], case["basemap"], case["src_first"], case["bounds"], case["length"],
                                    case["total"], case["longest"], thresholds, max_bases, counts, work)

    for bad in (0, 33, -1, True, 16.0):
        with pytest.raises(ValueError):
            call(max_bases=bad)
    with pytest.raises(ValueError):                        # too small a table: one cell short
        call(counts=torch.zeros(2 * 3 * 5 * 17 - 1, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError):                        # an empty base map (a null pointer)
        call(case=dict(planted, basemap=torch.zeros(0, dtype=torch.uint8, device="cuda:0")))
    with pytest.raises(ValueError):                        # a base map of another type
        call(case=dict(planted, basemap=planted["basemap"].to(torch.int8)))
    with pytest.raises(ValueError):                        # a start for every stretch
        call(case=dict(planted, src_first=planted["src_first"][:-1]))
    with pytest.raises(ValueError):                        # a work buffer one byte short
        call(work=torch.zeros(engine.run_states_work_bytes(planted["total"], 1) - 1, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        call(thresholds=())
    with pytest.raises(ValueError):
        call(thresholds=THRESHOLDS + (0.125,))
    lib = engine._lib                                       # null pointers and sizes, straight at the C entry
    one = (C.c_double * 1)(0.5)
    buf = torch.zeros(1024, dtype=torch.int64, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    good = [None, p(planted["probs"]), p(planted["y"]), p(planted["basemap"]), 64, p(planted["src_first"]), p(planted["bounds"]),
            p(planted["length"]), 1, 64, 64, one, 1, 16, 0, 15, p(buf), p(buf), 2048, None]
    for position, value in ((1, None), (2, None), (3, None), (5, None), (6, None), (7, None), (11, None), (16, None), (17, None),
                            (4, 0), (4, -1), (4, 2 ** 31), (13, 0), (13, 33), (15, 0), (14, 60)):
        args = list(good)
        args[position] = value
        with pytest.raises(ValueError):
            N.check(lib.cf_validation_run_bases(*args))
    assert np.array_equal(run_bases_on_device(engine, planted, (0.5,), 16), lumped(planted["want"][:1], 16))
