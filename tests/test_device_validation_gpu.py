"""Validation rounds on the card (csrc/validation.hpp through the C ABI): cf_validation_gather against DeviceValidationSet.pack,
cf_validation_score against score_host, and ``validate`` on a DeviceValidationSet against ``validate`` on the paths."""
import os
import random

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from test_device_validation import (CASES, case_ids, case_selection, check_golden_round, golden_reads, stub, write_golden_npz)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(ckpt_weights):
    from catfish_amd.engine import HipEngine
    eng = HipEngine(ckpt_weights)
    assert int(eng._lib.cf_validation_score_chunk()) == dv.SCORE_CHUNK
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def vset():
    return DeviceValidationSet.from_arrays(*golden_reads())


def _longest(bounds):
    return int(np.diff(bounds).max()) if len(bounds) > 1 else 0


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


def gather_on_device(engine, vset, selection, bounds):
    """cf_validation_gather for ``selection`` laid out by ``bounds`` -> (x, y) device tensors."""
    import torch
    read_index, first, length = selection
    total = int(bounds[-1])
    signal, labels = vset.device_arrays("cuda:0")
    x = torch.full((total,), 7.0, dtype=torch.float32, device="cuda:0")          # stale values the kernel must overwrite
    y = torch.full((total,), 9, dtype=torch.uint8, device="cuda:0")
    engine.gather_validation(signal, labels, _dev(vset.offsets[read_index] + first), _dev(length), _dev(bounds), total,
                             _longest(bounds), x, y)
    return x, y


def score_on_device(engine, probs, logits, y, bounds, thresholds):
    """cf_validation_score -> (right, ce_sum, counts [K, 4]) numpy; ``probs`` / ``logits`` / ``y`` are device tensors."""
    import torch
    n, k, total = len(bounds) - 1, len(thresholds), int(bounds[-1])
    right = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    ce_sum = torch.full((n,), -1.0, dtype=torch.float64, device="cuda:0")
    counts = torch.full((4 * k,), -1, dtype=torch.int64, device="cuda:0")
    partials = torch.empty(total // dv.SCORE_CHUNK + n, dtype=torch.float64, device="cuda:0")
    engine.score_validation(probs, logits, y, _dev(bounds), total, _longest(bounds), _dev(np.asarray(thresholds, np.float64)),
                            right, ce_sum, counts, partials)
    torch.cuda.synchronize()
    engine.check_error()
    return right.cpu().numpy(), ce_sum.cpu().numpy(), counts.cpu().numpy().reshape(k, 4)


class DeviceStubNetwork(object):
    """The closed-form network of tests/golden/validate_stub.py between the two DEVICE kernels."""
    window, n_inputs, n_outputs, model_type = 35, 1, 1, "ResNet-RNN"

    def __init__(self, engine, a, b, counters=(0, 0, 0, 0)):
        self.engine, self.a, self.b = engine, a, b
        self.tp, self.fp, self.tn, self.fn = counters

    def score_validation_device(self, vset, selection, thresholds=(0.5,)):
        bounds, _tails = vset.layout(selection[2], self.window)
        x, y = gather_on_device(self.engine, vset, selection, bounds)
        logits = stub.stub_logits(x.cpu().numpy(), self.a, self.b)
        return score_on_device(self.engine, _dev(stub.stub_probs(logits)), _dev(logits), y, bounds, thresholds)


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_gather_and_score_reproduce_the_golden_round(case, engine, vset, tmp_path, monkeypatch, capsys):
    """gather == pack bit for bit; score == score_host on the stub's outputs (counts exact, float32 acc / loss / counts equal to
    score_validation_batch's); a stub-backed ``validate`` over the device kernels writes the reference's report."""
    selection = case_selection(vset, case)
    wx, wy, bounds, tails = vset.pack(selection, 35)
    x, y = gather_on_device(engine, vset, selection, bounds)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), wx.reshape(-1).view(np.uint32)) and np.array_equal(y.cpu().numpy(), wy)
    logits = stub.stub_logits(wx.reshape(-1), case["a"], case["b"])
    probs = stub.stub_probs(logits)
    right, ce_sum, counts = score_on_device(engine, _dev(probs), _dev(logits), y, bounds, (0.5,))
    want_right, want_ce, want_counts = vset.score_host(probs, logits, wy, bounds, (0.5,))
    assert np.array_equal(right, want_right) and np.array_equal(counts, want_counts)
    np.testing.assert_allclose(ce_sum, want_ce, rtol=1e-11, atol=0)
    acc, loss, got = vset.finish(right, ce_sum, counts[0], bounds, tails)
    want = tv.score_validation_batch(probs, logits, wy.astype(np.float64), bounds, tails)
    assert np.array_equal(acc, want[0]) and np.array_equal(loss, want[1]) and got == want[2]
    monkeypatch.chdir(tmp_path)
    check_golden_round(case, DeviceStubNetwork(engine, case["a"], case["b"], case["counters_before"]), vset, capsys)


def test_chunk_boundaries_determinism_and_raw_sums(engine):
    """Reads that straddle the scoring chunk, saturated logits, 16 thresholds with 0, 1 and exact probabilities, one label 2."""
    c = dv.SCORE_CHUNK
    last = 3 * c + 17 if 6 * c + 52 <= 20000 else 2 * c + 17
    lengths = np.array([1, 34, c - 1, c, c + 1, last], dtype=np.int64)
    assert lengths.sum() <= 20000
    rng = np.random.default_rng(8)
    raws = [rng.normal(size=int(n)) for n in lengths]
    labs = [rng.integers(0, 2, size=int(n)) for n in lengths]
    labs[4][c // 2] = 2
    vs = DeviceValidationSet.from_arrays(raws, labs)
    selection = vs.select(35, 0, "complete", 856)
    assert np.array_equal(selection[2], lengths)
    for window in (35, 1):                    # window 1: no tails, so the packed reads are EXACTLY 1, 34, c - 1, c, c + 1, ... long
        wx, wy, bounds, _tails = vs.pack(selection, window)
        x, y = gather_on_device(engine, vs, selection, bounds)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), wx.reshape(-1).view(np.uint32)) and np.array_equal(y.cpu().numpy(), wy)
        total = int(bounds[-1])
        logits = rng.uniform(-30.0, 30.0, size=total).astype(np.float32)
        logits[rng.choice(total, size=8, replace=False)] = np.float32([100, -100, 100, -100, 100, -100, 100, -100])
        probs = stub.stub_probs(logits)
        thresholds = [0.0, 1.0, 0.5, 0.25, 0.75, 1e-9, 1.0 - 1e-9] + [float(v) for v in probs[rng.choice(total, size=9, replace=False)]]
        assert len(thresholds) == 16
        want_right, want_ce, want_counts = dv.score_host(probs, logits, wy, bounds, thresholds)
        runs = [score_on_device(engine, _dev(probs), _dev(logits), y, bounds, thresholds) for _ in range(2)]
        for right, ce_sum, counts in runs:
            assert np.array_equal(right, want_right) and np.array_equal(counts, want_counts)
            np.testing.assert_allclose(ce_sum, want_ce, rtol=1e-11, atol=0)
        assert runs[0][1].tobytes() == runs[1][1].tobytes()                     # two launches: the same bits
        assert counts.sum(axis=1).tolist() == [total] * 16
    # refused on the host, and the engine stays usable
    import torch
    dp, dl = _dev(probs), _dev(logits)
    with pytest.raises(ValueError):
        score_on_device(engine, dp, dl, y, bounds, thresholds + [0.125])       # K = 17
    with pytest.raises(ValueError):
        score_on_device(engine, dp, dl, y, bounds, [])                          # K = 0
    with pytest.raises(ValueError):
        score_on_device(engine, dp, dl, y, bounds[:1], thresholds)              # n = 0
    with pytest.raises(ValueError):
        gather_on_device(engine, vs, tuple(a[:0] for a in selection), bounds[:1])
    with pytest.raises(ValueError):
        engine.score_validation(dp.double(), dl, y, _dev(bounds), total, c, _dev(np.float64([0.5])), torch.empty(6, dtype=torch.int64, device="cuda:0"),
                                torch.empty(6, dtype=torch.float64, device="cuda:0"), torch.empty(4, dtype=torch.int64, device="cuda:0"),
                                torch.empty(64, dtype=torch.float64, device="cuda:0"))
    again = score_on_device(engine, dp, dl, y, bounds, thresholds)
    assert np.array_equal(again[0], want_right) and again[1].tobytes() == runs[0][1].tobytes() and np.array_equal(again[2], want_counts)


def _both_routes(net, vset, paths, tmp_path, monkeypatch, stretch, start, most, seed):
    out = []
    for name, source in (("device", vset), ("host", paths)):
        os.makedirs(str(tmp_path / name), exist_ok=True)
        monkeypatch.chdir(tmp_path / name)
        if seed is not None:
            random.seed(seed)
        got = tv.validate(net, source, stretch, "some/dir/round", start, most)
        with open("round.txt", "rb") as fh:
            out.append((fh.read(), got, random.getstate()))
        os.remove("round.txt")
    return out


def test_the_real_network_scores_the_same_on_both_routes(hp, ckpt_weights, vset, tmp_path, monkeypatch):
    from catfish_amd.resnet_class import ResNetRNN
    paths = write_golden_npz(tmp_path)
    net = ResNetRNN(**hp)
    net.set_weights(ckpt_weights)
    for stretch, start, most, seed in ((0, "complete", 856, None), (700, "random", 856, 5), (700, "random", 4, 6)):
        device, host = _both_routes(net, vset, paths, tmp_path, monkeypatch, stretch, start, most, seed)
        assert device[0] == host[0] and device[1] == host[1] and device[2] == host[2]
    rows = tv.threshold_sweep(net, vset, [0.3, 0.5], 0)                          # the 0.5 row is the round's own counts
    probs, _logits = net.score_windows(vset.pack(vset.select(35, 0, "complete", 856), 35)[0])
    assert rows[1]["tp"] + rows[1]["fp"] == int(np.count_nonzero(probs.astype(np.float64) >= 0.5))
    assert rows[0]["tp"] + rows[0]["fp"] == int(np.count_nonzero(probs.astype(np.float64) >= 0.3))
    net.engine.close()
    small = ResNetRNN(**dict(hp, layer_size=16, layer_size_res=16))              # an any-size geometry
    small.initialize_network(seed=3)
    device, host = _both_routes(small, vset, paths, tmp_path, monkeypatch, 0, "complete", 856, None)
    assert device[0] == host[0] and device[1] == host[1]
    small.engine.close()


def test_rounds_score_the_weights_just_trained_and_keep_their_buffers(hp, tmp_path, monkeypatch):
    pytest.importorskip("torch")
    from catfish_amd import device_db as ddb
    val_dir = tmp_path / "val"
    val_dir.mkdir()
    paths = []
    for i in range(3):
        raw, lab = tv.synthetic_labelled_read(3000 + 35 * i + i, seed=50 + i)
        paths.append(str(val_dir / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    resident = DeviceValidationSet.from_npz(paths)
    reports = {}
    for name, source in (("device", resident), ("host", paths)):
        (tmp_path / name).mkdir()
        monkeypatch.chdir(tmp_path / name)
        net = tv.build_model("ResNetRNN", save=True, **dict(hp, batch_size=32, train_seed=0))
        net.initialize_network(seed=4)
        db = ddb.synthetic_device_db(n_reads=2, read_len=12000, seed=2)
        random.seed(9)
        acc = tv.train_and_validate(net, db, 3 * 32, source, 2000, net.model_path, "random", 856)
        with open(net.model_path + ".txt") as fh:
            model_report = fh.read()
        with open(os.path.basename(net.model_path) + ".txt") as fh:
            reports[name] = (model_report, fh.read(), acc)
        assert "---NEXT ROUND OF VALIDATION---" in reports[name][1] and "Saved checkpoint at step 3" in model_report
        if name == "device":
            book = net.validation_buffers
            assert (resident.uploads, book["allocations"], book["selection_uploads"], book["threshold_uploads"]) == (1, 1, 1, 1)
            kept = {key: t.data_ptr() for key, t in book["tensors"].items()}
            first = tv.validate(net, resident, 2000, "again", 0, 856)
            assert tv.validate(net, resident, 2000, "again", 0, 856) == first
            tv.validate(net, resident, 1000, "again", "random", 2)               # a smaller round: nothing regrows
            # nothing but the selection went to the card again, and the buffers are the ones of the first round
            assert (resident.uploads, book["allocations"], book["selection_uploads"], book["threshold_uploads"]) == (1, 1, 4, 1)
            assert {key: t.data_ptr() for key, t in book["tensors"].items()} == kept
            tv.validate(net, resident, 0, "again", "complete", 856)              # a larger one does, once
            assert (resident.uploads, book["allocations"], book["selection_uploads"]) == (1, 2, 5)
        net.engine.close()
    assert reports["device"] == reports["host"]


def test_a_round_names_its_results_and_lays_them_out_as_before(hp):
    """Every combination of the three optional results over three reads with a tail each and two thresholds: the named fields are
    the items at the positions the docstring of ``score_validation_device`` states, the round with everything asked for holds the
    bytes of the rounds that ask for one thing, and the buffers are allocated again only when a capacity grows."""
    import itertools
    from catfish_amd.resnet_class import ResNetRNN
    reads = [tv.synthetic_labelled_read(3000 + 36 * i, seed=50 + i) for i in range(3)]
    resident = DeviceValidationSet.from_arrays([raw for raw, _lab in reads], [lab for _raw, lab in reads])
    selection = resident.select(35, 0, "complete", 856)
    assert selection[2].tolist() == [3000, 3036, 3072] and all(dv.layout(selection[2], 35)[1] > 0)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    try:
        book = net.validation_buffers
        rounds = {}
        for asked in itertools.product((False, True), repeat=3):
            runs, borders, curve = asked
            before, allocations = dict(book["capacity"]), book["allocations"]
            got = net.score_validation_device(resident, selection, (0.3, 0.5), run_edges=(35,) if runs else None,
                                              border_reach=32 if borders else None, curve_shift=14 if curve else None)
            grown = [key for key, value in book["capacity"].items() if value > before.get(key, 0)]
            assert book["allocations"] == allocations + bool(grown)
            assert grown or book["capacity"] == before
            assert isinstance(got, tuple) and len(got) == 3 + sum(asked)
            assert got.right is got[0] and got.ce_sum is got[1] and got.counts is got[2]
            assert got.right.shape == (3,) and got.ce_sum.dtype == np.float64 and got.counts.shape == (2, 4)
            assert got.run_states is (got[3] if runs else None) and got.run_borders is (got[3 + runs] if borders else None)
            assert got.curve is (got[-1] if curve else None)
            if runs:
                assert got.run_states.shape == (2, 2, 2, 3)
            if borders:
                assert got.run_borders.shape == (2, 2, 5 * 32 + 3)
            if curve:
                assert got.curve.shape == (3, dv.curve_bins(14)) and int(got.curve.sum()) == int(selection[2].sum())
            assert got.counts.sum(axis=1).tolist() == [int(dv.layout(selection[2], 35)[0][-1])] * 2
            rounds[asked] = got
        assert book["selection_uploads"] == 8 and book["threshold_uploads"] == 1
        everything, allocations = rounds[(True, True, True)], book["allocations"]
        again = net.score_validation_device(resident, selection, (0.3, 0.5), run_edges=(35,), border_reach=32, curve_shift=14)
        assert book["allocations"] == allocations and all(a.tobytes() == b.tobytes() for a, b in zip(again, everything))
        for got in rounds.values():                            # the per-sample results do not depend on what else is asked for
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], everything[:3]))
        assert everything.run_states.tobytes() == rounds[(True, False, False)].run_states.tobytes()
        assert everything.run_borders.tobytes() == rounds[(False, True, False)].run_borders.tobytes()
        assert everything.curve.tobytes() == rounds[(False, False, True)].curve.tobytes()
        assert everything.run_states.sum() > 0 and everything.run_borders.sum() > 0
    finally:
        net.engine.close()
