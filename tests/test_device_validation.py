"""Device-resident validation set, host side (catfish_amd/device_validation.py): the selection is the host route's selection,
the normative numpy scorer reproduces the reference's own reports (tests/golden/validate_golden.json, made by executing the
reference's ``validate``), and the error paths -- no GPU needed."""
import json
import os
import random
import sys

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(__file__))
from golden import validate_stub as stub      # noqa: E402


def golden_cases():
    with open(os.path.join(GOLDEN, "validate_golden.json")) as fh:
        return json.load(fh)["cases"]


def golden_reads():
    """The 12 reads of the golden: ([raw], [labels])."""
    with np.load(os.path.join(GOLDEN, "validate_golden_reads.npz")) as z:
        n = len(z.files) // 2
        return [z["raw_%02d" % i] for i in range(n)], [z["labels_%02d" % i] for i in range(n)]


def write_golden_npz(directory):
    paths = []
    for i, (raw, lab) in enumerate(zip(*golden_reads())):
        paths.append(os.path.join(str(directory), "read_%02d.npz" % i))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    return paths


def case_selection(vset, case):
    if case["random_seed"] is not None:
        random.seed(case["random_seed"])
    return vset.select(35, case["max_seq_length"], case["validation_start"], case["max_number"])


class HostStubNetwork(object):
    """The closed-form 'network' of tests/golden/validate_stub.py behind ``score_validation_device``: pack -> stub -> score_host."""
    window, n_inputs, n_outputs, model_type = 35, 1, 1, "ResNet-RNN"

    def __init__(self, a, b, counters=(0, 0, 0, 0)):
        self.a, self.b = a, b
        self.tp, self.fp, self.tn, self.fn = counters
        self.forwards = 0

    def forward(self, x):
        self.forwards += 1
        logits = stub.stub_logits(np.asarray(x).reshape(-1), self.a, self.b)
        return stub.stub_probs(logits), logits

    def score_validation_device(self, vset, selection, thresholds=(0.5,)):
        x, y, bounds, _tails = vset.pack(selection, self.window)
        probs, logits = self.forward(x)
        return vset.score_host(probs, logits, y, bounds, thresholds)


def check_golden_round(case, net, vset, capsys):
    """``validate(net, vset, ...)`` in the current directory against everything the golden case recorded."""
    if case["random_seed"] is not None:
        random.seed(case["random_seed"])
    capsys.readouterr()
    got = tv.validate(net, vset, case["max_seq_length"], "some/dir/" + case["name"], case["validation_start"], case["max_number"])
    assert capsys.readouterr().out == case["printed"]
    with open(case["name"] + ".txt") as fh:
        assert fh.read() == case["report"]
    assert [float(v) for v in got] == case["returned"]
    assert [net.tp, net.fp, net.tn, net.fn] == case["counters_after"] == [0, 0, 0, 0]


@pytest.fixture(scope="module")
def vset():
    return DeviceValidationSet.from_arrays(*golden_reads())


@pytest.fixture()
def golden_paths(tmp_path):
    return write_golden_npz(tmp_path)


CASES = golden_cases()
case_ids = lambda c: c["name"]      # noqa: E731


def test_the_set_holds_what_the_host_route_packs(golden_paths):
    raws, labs = golden_reads()
    vs = DeviceValidationSet.from_npz(golden_paths)
    assert vs.signal.dtype == np.float32 and vs.labels.dtype == np.uint8 and vs.offsets.dtype == np.int64
    assert vs.lengths.tolist() == [len(r) for r in raws] and vs.offsets.tolist() == np.concatenate(([0], np.cumsum(vs.lengths))).tolist()
    assert np.array_equal(vs.signal, np.concatenate(raws).astype(np.float32)) and np.array_equal(vs.labels, np.concatenate(labs))
    served = []
    mem = DeviceValidationSet.from_npz(["a", "b"], loader=lambda path: served.append(path) or (raws[0], labs[0]))
    assert served == ["a", "b"] and mem.n_reads == 2 and mem._dev is None and mem.uploads == 0


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_selection_is_the_host_routes_selection(case, vset, golden_paths):
    if case["random_seed"] is not None:
        random.seed(case["random_seed"])
    signals, labels = tv.select_validation_stretches(golden_paths, 35, case["max_seq_length"], case["validation_start"], case["max_number"])
    want_state = random.getstate()
    wx, wy, wbounds, wtails = tv.pack_validation_windows(signals, labels, 35)
    selection = case_selection(vset, case)
    assert random.getstate() == want_state                                      # the same draws, none more
    assert all(a.dtype == np.int64 for a in selection) and len(selection[0]) == len(signals)
    x, y, bounds, tails = vset.pack(selection, 35)
    assert x.dtype == np.float32 and x.shape == wx.shape and np.array_equal(x.view(np.uint32), wx.view(np.uint32))
    assert y.dtype == np.uint8 and np.array_equal(y, wy)
    assert bounds.dtype == np.int64 and np.array_equal(bounds, wbounds) and np.array_equal(tails, wtails)
    assert int(selection[2].sum()) == sum(len(s) for s in signals)


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_the_normative_scorer_reproduces_the_reference_report(case, vset, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    net = HostStubNetwork(case["a"], case["b"], case["counters_before"])
    check_golden_round(case, net, vset, capsys)
    assert net.forwards == 1


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_score_host_and_finish_are_score_validation_batch(case, vset):
    selection = case_selection(vset, case)
    x, y, bounds, tails = vset.pack(selection, 35)
    logits = stub.stub_logits(x.reshape(-1), case["a"], case["b"])
    probs = stub.stub_probs(logits)
    for planted in (False, True):
        if planted:                                                             # the y != 1 / y != 0 branches
            y = y.copy()
            y[[0, len(y) // 3, len(y) // 2]] = (2, 255, 2)
        want_acc, want_loss, want_counts = tv.score_validation_batch(probs, logits, y.astype(np.float64), bounds, tails)
        right, ce_sum, counts = vset.score_host(probs, logits, y, bounds, (0.5,))
        assert right.dtype == np.int64 and ce_sum.dtype == np.float64 and counts.dtype == np.int64 and counts.shape == (1, 4)
        acc, loss, got_counts = vset.finish(right, ce_sum, counts[0], bounds, tails)
        assert acc.dtype == np.float32 and loss.dtype == np.float32
        assert np.array_equal(acc, want_acc) and np.array_equal(loss, want_loss) and got_counts == want_counts


@pytest.mark.parametrize("thresholds", [[k / 10.0 for k in range(11)], [k / 19.0 for k in range(20)]], ids=["11", "20"])
def test_threshold_sweep_counts_every_threshold_from_one_forward(thresholds, vset):
    net = HostStubNetwork(0.75, -0.375)
    rows = tv.threshold_sweep(net, vset, thresholds, 0)
    assert net.forwards == 1 and [row["threshold"] for row in rows] == thresholds
    selection = vset.select(35, 0, "complete", 856)
    x, y, _bounds, tails = vset.pack(selection, 35)
    logits = stub.stub_logits(x.reshape(-1), 0.75, -0.375)
    p = stub.stub_probs(logits).astype(np.float64)
    from catfish_amd import metrics
    for row, t in zip(rows, thresholds):
        called = p >= t
        tp, fp = int(np.sum(called & (y == 1))), int(np.sum(called & (y != 1)))
        tn, fn = int(np.sum(~called & (y == 0))) - int(tails.sum()), int(np.sum(~called & (y != 0)))
        precision, recall = metrics.precision_recall(tp, fp, fn)
        assert row == {"threshold": t, "tp": tp, "fp": fp, "tn": tn, "fn": fn, "precision": precision, "recall": recall,
                       "f1": metrics.f1(precision, recall)}
    assert rows[0]["tn"] == -int(tails.sum()) and rows[0]["fn"] == 0            # t = 0 calls everything, tails included


def test_threshold_sweep_limits_the_reads_like_validate(vset):
    net = HostStubNetwork(1.5, -0.5)
    random.seed(11)
    rows = tv.threshold_sweep(net, vset, [0.5], 735, "random", 3)
    random.seed(11)
    selection = vset.select(35, 735, "random", 3)
    assert len(selection[0]) == 3 and sum(rows[0][k] for k in ("tp", "fp", "tn", "fn")) == int(selection[2].sum())


def test_error_paths_raise_before_anything_is_uploaded(vset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    raws, labs = golden_reads()
    for bad in (256, 0.5, -1, float("nan")):
        lab = labs[0].astype(np.float64)
        lab[3] = bad
        with pytest.raises(ValueError):
            DeviceValidationSet.from_arrays(raws[:1], [lab])
    with pytest.raises(ValueError):
        DeviceValidationSet.from_arrays(raws[:1], [labs[0][:-1]])              # signal / label length mismatch
    with pytest.raises(ValueError):
        DeviceValidationSet.from_arrays(raws[:2], labs[:1])
    net = HostStubNetwork(1.0, 0.0)
    with pytest.raises(ValueError):
        tv.validate(net, vset, 350, "m", "middle", 856)
    with pytest.raises(ValueError):
        vset.select(35, 350, 1.0, 856)
    with pytest.raises(ZeroDivisionError):                                      # every read too short
        tv.validate(net, vset, 35000, "m", 0, 856)
    with pytest.raises(ZeroDivisionError):
        tv.threshold_sweep(net, vset, [0.5], 35000, 0)
    with pytest.raises(ValueError):
        vset.check_selection((np.array([0]), np.array([690]), np.array([35])))    # past the end of read 0
    with pytest.raises(ValueError):
        vset.check_selection((np.array([12]), np.array([0]), np.array([35])))
    assert not os.path.exists("m.txt") and net.forwards == 0
    assert vset._dev is None and vset.uploads == 0


def test_score_chunk_is_exported():
    assert isinstance(dv.SCORE_CHUNK, int) and dv.SCORE_CHUNK > 0 and dv.MAX_THRESHOLDS == 16
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "catfish_amd", "csrc", "validation.hpp")) as fh:
        text = fh.read()
    assert "#define CF_SCORE_CHUNK %d\n" % dv.SCORE_CHUNK in text and "#define CF_SCORE_MAX_K %d\n" % dv.MAX_THRESHOLDS in text
