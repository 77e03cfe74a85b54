"""The validation curves on the CPU: the bin rule of csrc/validation_curve_bin.hpp (compiled with g++ through
tests/native/validation_curve_bin_shim.cpp) against its numpy statement and against ``p >= t``; ``curve_host`` against plain loops;
``curves_from_histogram`` against ``score_host``, against pairwise counts and, where it is installed, against scikit-learn."""
import contextlib
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = (10, 14, 22)
ONE = 0x3F800000
# +-0, the smallest and the largest subnormal, the smallest normal, 1.0 and its neighbours, +-inf, both NaN signs, a negative value
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, ONE - 1, ONE, ONE + 1, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0xFFC00000, 0x7F800001, 0xBF000000, 0x80000001, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("validation_curve_bin") / "libvalidation_curve_bin.so")
    build = subprocess.run(["g++", "-std=c++17", "-O3", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "validation_curve_bin_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    dll = ctypes.CDLL(lib)
    U, LL = ctypes.c_uint, ctypes.c_longlong
    for name, res, args in (("shim_shift_ok", ctypes.c_int, [ctypes.c_int]), ("shim_bins", U, [ctypes.c_int]), ("shim_bin", U, [U, ctypes.c_int]),
                            ("shim_key", U, [U, U, ctypes.c_int]), ("shim_bin_many", None, [ctypes.c_void_p, LL, ctypes.c_int, ctypes.c_void_p]),
                            ("shim_sweep", None, [ctypes.c_int, ctypes.POINTER(LL)])):
        getattr(dll, name).restype, getattr(dll, name).argtypes = res, args
    return dll


def shim_bins_of(shim, bits, shift):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    out = np.empty(bits.size, dtype=np.uint32)
    shim.shim_bin_many(bits.ctypes.data, bits.size, shift, out.ctypes.data)
    return out.astype(np.int64)


def test_shifts_and_bin_counts(shim):
    assert dv.curve_bins() == dv.curve_bins(14) == 65025
    for shift in range(10, 23):
        assert shim.shim_shift_ok(shift) == 1 and shim.shim_bins(shift) == dv.curve_bins(shift) == (ONE >> shift) + 1
        edges = dv.curve_thresholds(shift)
        assert edges.dtype == np.float32 and edges.shape == (dv.curve_bins(shift),) and edges[0] == 0.0 and edges[-1] == 1.0
        assert np.all(np.diff(edges) > 0)
    for bad in (9, 23, -1, 0, 14.0, True, "14", None):
        with pytest.raises(ValueError):
            dv.curve_bins(bad)
    assert shim.shim_shift_ok(9) == 0 and shim.shim_shift_ok(23) == 0


@pytest.mark.parametrize("shift", SHIFTS)
def test_every_bit_pattern_lands_inside_the_table(shim, shift):
    """All 2^32 patterns: the bin lies in [0, NB), does not fall as p rises over [0, 1] and is bits >> shift there, everything above
    1.0 goes to the top bin, everything with the sign bit to bin 0."""
    out = (ctypes.c_longlong * 5)(*([-1] * 5))
    shim.shim_sweep(shift, out)
    assert list(out) == [0, 0, 0, 0, 0]


@pytest.mark.parametrize("shift", SHIFTS)
def test_bin_at_least_b_is_p_at_least_the_edge(shim, shift):
    """bin(p) >= b  <=>  p >= t_b, at every bin edge and one ulp either side, for the header and for numpy."""
    nb = dv.curve_bins(shift)
    edges = dv.curve_thresholds(shift)
    b = np.arange(nb, dtype=np.int64)
    for step in (-1, 0, 1):
        bits = (b << shift) + step
        keep = bits >= 0                                   # there is nothing below +0.0 among the non-negative patterns
        p = bits[keep].astype(np.uint32).view(np.float32)
        for other in (0, -1, 1):                           # against its own edge and against the neighbouring edges
            against = b[keep] + other
            ok = (against >= 0) & (against < nb)
            want = p[ok] >= edges[against[ok]]
            assert np.array_equal(shim_bins_of(shim, bits[keep][ok], shift) >= against[ok], want), (shift, step, other)
            assert np.array_equal(dv.curve_bin(bits[keep][ok], shift) >= against[ok], want), (shift, step, other)
    rng = np.random.default_rng(shift)
    bits = rng.integers(0, ONE + 1, size=200000, dtype=np.int64)                             # any p in [0, 1] against any edge
    against = rng.integers(0, nb, size=bits.size)
    assert np.array_equal(shim_bins_of(shim, bits, shift) >= against, bits.astype(np.uint32).view(np.float32) >= edges[against])


@pytest.mark.parametrize("shift", SHIFTS)
def test_numpy_bin_is_the_headers(shim, shift):
    rng = np.random.default_rng(100 + shift)
    bits = np.concatenate((rng.integers(0, 2 ** 32, size=10 ** 6, dtype=np.int64).astype(np.uint32), SPECIALS))
    got = dv.curve_bin(bits, shift)
    assert got.dtype == np.int64 and np.array_equal(got, shim_bins_of(shim, bits, shift))
    top = dv.curve_bins(shift) - 1
    special = dict(zip(SPECIALS.tolist(), dv.curve_bin(SPECIALS, shift).tolist()))
    assert special[0] == special[0x80000000] == special[0xFF800000] == special[0xFFC00000] == special[0xBF000000] == 0
    assert special[ONE] == special[ONE + 1] == special[0x7F800000] == special[0x7FC00000] == top and special[ONE - 1] == top - 1
    assert special[1] == special[0x80000001] == 0 and special[0x007FFFFF] == 0x007FFFFF >> shift and special[0x00800000] == 0x00800000 >> shift
    assert int(dv.curve_bin(np.float32(1.0).view(np.uint32), shift)) == top                  # a scalar works too
    nb = dv.curve_bins(shift)
    for pattern in SPECIALS.tolist():
        for label, row in ((1, 0), (0, 1), (2, 2), (255, 2)):
            assert shim.shim_key(pattern, label, shift) == row * nb + special[pattern] < 3 * nb


# ---------------------------------------------------------------------------------------------------------------- curve_host
LENGTHS = (0, 1, 34, 35, 36, 0, 71, 140)


def planted_batch(seed, lengths=LENGTHS, tail_p=0.9, window=35):
    """A packed batch with labels in {0, 1, 2, 255}; the tails hold ``tail_p`` and label 0, so a tail taken for a sample shows."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    bounds, tails = dv.layout(lengths, window)
    probs = np.full(int(bounds[-1]), tail_p, dtype=np.float32)
    y = np.zeros(int(bounds[-1]), dtype=np.uint8)
    for b0, n in zip(bounds[:-1].tolist(), lengths.tolist()):
        p = rng.random(n).astype(np.float32)
        p[rng.random(n) < 0.1] = 0.0
        p[rng.random(n) < 0.1] = 1.0
        probs[b0:b0 + n] = p
        y[b0:b0 + n] = rng.choice(np.uint8([0, 0, 0, 1, 1, 1, 2, 255]), size=n)
    return probs, y, bounds, lengths, tails


@pytest.mark.parametrize("shift", SHIFTS)
def test_curve_host_is_the_plain_loop(shift):
    probs, y, bounds, lengths, tails = planted_batch(1)
    assert tails.sum() > 0
    nb = dv.curve_bins(shift)
    want = np.zeros((3, nb), dtype=np.int64)
    for r, n in enumerate(lengths.tolist()):
        for i in range(int(bounds[r]), int(bounds[r]) + n):
            bits = int(probs[i:i + 1].view(np.uint32)[0])
            signed = bits - 2 ** 32 if bits >= 2 ** 31 else bits
            want[{1: 0, 0: 1}.get(int(y[i]), 2), min(max(signed, 0) >> shift, nb - 1)] += 1
    got = dv.curve_host(probs, y, bounds, lengths, shift)
    assert got.dtype == np.int64 and got.shape == (3, nb) and np.array_equal(got, want)
    assert got.sum() == lengths.sum() and (got.sum(axis=1) > 0).all()
    assert dv.curve_host(probs, y, bounds, lengths).shape == (3, 65025)
    # the tails are absent: whatever they hold, the table stays
    other = probs.copy()
    for r, n in enumerate(lengths.tolist()):
        other[int(bounds[r]) + n:int(bounds[r + 1])] = 0.25
    assert np.array_equal(dv.curve_host(other, y, bounds, lengths, shift), got)
    assert np.array_equal(dv.DeviceValidationSet.curve_host(probs, y, bounds, lengths, shift), got)
    with pytest.raises(ValueError):
        dv.curve_host(probs, y, bounds, lengths, 9)


# ---------------------------------------------------------------------------------------------------------------- the curves
@pytest.mark.parametrize("shift", SHIFTS)
def test_counts_at_a_bin_edge_are_score_hosts(shift):
    """tp / fp / tn / fn at bin-edge thresholds equal score_host + finish, labels other than 0 / 1 included.  The tails hold p = 0.0
    and label 0 as after a gather of zeros scored 0: uncalled at every edge above 0.0, so finish's subtraction removes exactly them;
    the batch without tails is compared at 0.0 too."""
    nb = dv.curve_bins(shift)
    for lengths, tail_p, first in ((LENGTHS, 0.0, 1), ((35, 70, 0, 140, 35), 0.9, 0)):
        probs, y, bounds, lengths, tails = planted_batch(2, lengths, tail_p)
        curves = dv.curves_from_histogram(dv.curve_host(probs, y, bounds, lengths, shift), shift)
        occupied = np.unique(dv.curve_bin(probs.view(np.uint32), shift))
        at = sorted(set([first, 1, 2, nb // 2, nb - 2, nb - 1] + occupied[occupied >= first][::7].tolist()))
        thresholds = dv.curve_thresholds(shift)[at]
        _right, _ce, counts = dv.score_host(probs, np.zeros_like(probs), y, bounds, thresholds)
        for k, b in enumerate(at):
            _acc, _loss, want = dv.finish(np.zeros(len(lengths)), np.zeros(len(lengths)), counts[k], bounds, tails)
            assert (int(curves["tp"][b]), int(curves["fp"][b]), int(curves["tn"][b]), int(curves["fn"][b])) == want, (shift, b)
        assert curves["n_other"] == int(np.count_nonzero(y > 1)) > 0
        assert curves["n_pos"] + curves["n_neg"] + curves["n_other"] == lengths.sum()
        for key in ("tp", "fp", "tn", "fn"):
            assert curves[key].dtype == np.int64 and curves[key].shape == (nb,)
        assert np.all(curves["tp"] + curves["fp"] + curves["tn"] + curves["fn"] == lengths.sum())


def binary_samples(seed, n, shift):
    """Scores with saturated 0.0 and 1.0 and many near-ties, binary labels that the scores partly explain."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.4).astype(np.uint8)
    p = np.clip(rng.normal(0.35 + 0.3 * y, 0.25), 0.0, 1.0).astype(np.float32)
    p[rng.random(n) < 0.05] = 0.0
    p[rng.random(n) < 0.05] = 1.0
    hist = dv.curve_host(p, y, [0, n], [n], shift)
    quantised = dv.curve_thresholds(shift)[dv.curve_bin(p.view(np.uint32), shift)]
    return p, quantised, y, hist


def pairwise_auc(scores, y):
    """O(n^2): the share of (positive, negative) pairs the score orders rightly, ties one half."""
    pos, neg = scores[y == 1].astype(np.float64), scores[y == 0].astype(np.float64)
    wins = np.count_nonzero(pos[:, None] > neg[None, :]) + 0.5 * np.count_nonzero(pos[:, None] == neg[None, :])
    return wins / (pos.size * neg.size)


@pytest.mark.parametrize("shift", SHIFTS)
def test_roc_auc_is_the_pairwise_count_of_the_quantised_scores(shift):
    for seed, n in ((1, 2000), (2, 333), (3, 2)):
        p, quantised, y, hist = binary_samples(seed, n, shift)
        if n == 2:
            p, y = np.float32([0.25, 0.75]), np.uint8([0, 1])
            hist = dv.curve_host(p, y, [0, 2], [2], shift)
            quantised = dv.curve_thresholds(shift)[dv.curve_bin(p.view(np.uint32), shift)]
        curves = dv.curves_from_histogram(hist, shift)
        exact, raw = pairwise_auc(quantised, y), pairwise_auc(p, y)
        print("shift %d n %d: roc_auc %.12f pairwise %.12f unquantised %.12f slack %.3g" % (shift, n, curves["roc_auc"], exact, raw,
                                                                                            curves["roc_auc_slack"]))
        assert abs(curves["roc_auc"] - exact) <= 1e-9      # float64 rounding of at most 2^20 additions of terms <= 1
        # exact in real numbers; 1e-12 covers the float64 rounding of the three quotients
        assert abs(raw - curves["roc_auc"]) <= curves["roc_auc_slack"] + 1e-12
        assert 0 <= curves["roc_auc_slack"] <= 0.5
        assert np.allclose(curves["tpr"], curves["tp"] / curves["n_pos"], rtol=0, atol=0)
        assert curves["fpr"][0] == curves["tpr"][0] == 1.0 and np.all(np.diff(curves["tpr"]) <= 0) and np.all(np.diff(curves["fpr"]) <= 0)


def pr_points(scores, y):
    """precision_recall_curve's points from the samples themselves: one per distinct score, ascending, then (precision 1, recall 0)."""
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    s, hit = scores[order], (y[order] == 1)
    last = np.flatnonzero(np.diff(s) != 0).tolist() + [len(s) - 1]                          # last sample of every distinct score
    tps, called = np.cumsum(hit)[last], np.asarray(last) + 1
    precision, recall = tps / called, tps / tps[-1]
    return np.concatenate((precision[::-1], [1.0])), np.concatenate((recall[::-1], [0.0]))


@pytest.mark.parametrize("shift", SHIFTS)
def test_pr_auc_is_the_trapezoid_over_the_distinct_quantised_scores(shift):
    p, quantised, y, hist = binary_samples(4, 2000, shift)
    curves = dv.curves_from_histogram(hist, shift)
    precision, recall = pr_points(quantised, y)
    want = -float(np.sum(np.diff(recall) * (precision[:-1] + precision[1:]) / 2.0))
    assert abs(curves["pr_auc"] - want) <= 1e-9
    occupied = np.flatnonzero(hist.sum(axis=0))
    assert np.array_equal(curves["precision"][occupied], precision[:-1]) and np.array_equal(curves["recall"][occupied], recall[:-1])


@pytest.mark.parametrize("shift", SHIFTS)
def test_curves_are_scikit_learns_on_the_quantised_scores(shift):
    sk = pytest.importorskip("sklearn.metrics")
    for seed, n in ((5, 2000), (6, 5000), (7, 400000 if shift == 14 else 50000)):
        p, quantised, y, hist = binary_samples(seed, n, shift)
        curves = dv.curves_from_histogram(hist, shift)
        precision, recall, thresholds = sk.precision_recall_curve(y, quantised)
        assert abs(curves["roc_auc"] - sk.roc_auc_score(y, quantised)) <= 1e-9
        assert abs(curves["pr_auc"] - sk.auc(recall, precision)) <= 1e-9
        assert abs(sk.roc_auc_score(y, p) - curves["roc_auc"]) <= curves["roc_auc_slack"] + 1e-12
        occupied = np.flatnonzero(hist.sum(axis=0))
        keep = np.isin(dv.curve_thresholds(shift)[occupied], thresholds)                      # (older releases stop at full recall)
        assert keep.sum() == len(thresholds) and keep[-1]
        assert np.array_equal(curves["precision"][occupied][keep], precision[:-1])
        assert np.array_equal(curves["recall"][occupied][keep], recall[:-1])
        fpr, tpr, _ = sk.roc_curve(y, quantised, drop_intermediate=False)
        assert np.array_equal(curves["tpr"][occupied][::-1], tpr[1:]) and np.array_equal(curves["fpr"][occupied][::-1], fpr[1:])


def test_an_empty_class_gives_nan_and_the_counts_stay():
    for label in (0, 1):
        y = np.full(50, label, dtype=np.uint8)
        p = np.linspace(0, 1, 50, dtype=np.float32)
        curves = dv.curves_from_histogram(dv.curve_host(p, y, [0, 50], [50], 22), 22)
        assert np.isnan(curves["roc_auc"]) and np.isnan(curves["roc_auc_slack"]) and np.isnan(curves["pr_auc"])
        assert (curves["n_pos"], curves["n_neg"], curves["n_other"]) == ((50, 0, 0) if label else (0, 50, 0))
        assert np.isnan(curves["fpr" if label else "tpr"]).all() and not np.isnan(curves["tpr" if label else "fpr"]).any()
        assert curves["tp"][0] == (50 if label else 0) and curves["fp"][0] == (0 if label else 50)
        assert curves["best_f1"]["f1"] == (1.0 if label else 0.0)
    empty = dv.curves_from_histogram(np.zeros((3, dv.curve_bins(22)), dtype=np.int64), 22)
    assert np.isnan(empty["roc_auc"]) and empty["best_f1"] == {"threshold": 0.0, "f1": 0.0, "precision": 0.0, "recall": 0.0}
    others = dv.curves_from_histogram(dv.curve_host(np.float32([0.2, 0.7, 0.9]), np.uint8([0, 1, 7]), [0, 3], [3], 22), 22)
    assert others["n_other"] == 1 and others["roc_auc"] == 1.0 and others["roc_auc_slack"] == 0.0
    with pytest.raises(ValueError):
        dv.curves_from_histogram(np.zeros((3, 5), dtype=np.int64), 22)


@pytest.mark.parametrize("shift", (14, 22))
def test_best_f1_is_the_arg_max_of_metrics_f1(shift):
    probs, y, bounds, lengths, _tails = planted_batch(8, (700, 36, 1300))
    curves = dv.curves_from_histogram(dv.curve_host(probs, y, bounds, lengths, shift), shift)
    edges = dv.curve_thresholds(shift)
    best = None
    with contextlib.redirect_stdout(io.StringIO()):          # (metrics prints when a denominator is empty)
        for b in range(dv.curve_bins(shift)):
            precision, recall = metrics.precision_recall(int(curves["tp"][b]), int(curves["fp"][b]), int(curves["fn"][b]))
            assert precision == curves["precision"][b] and recall == curves["recall"][b]
            score = metrics.f1(precision, recall)
            if best is None or score > best["f1"]:
                best = {"threshold": float(edges[b]), "f1": score, "precision": precision, "recall": recall}
    assert curves["best_f1"] == best and 0 < best["f1"] < 1
