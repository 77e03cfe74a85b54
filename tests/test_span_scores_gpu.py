"""``cf_span_scores`` on the card against ``span_scores.span_scores_host`` and exact sums: the planted batch of
tests/test_span_scores_host.py (8 reads, fewer than 20 000 samples; the kernel sees only probabilities, signal and the read table, so
the probabilities are planted), thresholds 0.5 and 0.9, min_run 1, 15, 64 and 65 (65 takes the two older span kernels).  Positions
and extremes bit for bit; every sum within ``n * 2**-53 * fsum(|values|)`` of ``math.fsum(values)``, the any-order bound of a float64
sum (derived in ``check_rows``, not measured).  Then end to end with the bundled checkpoint."""
import math
import os

import numpy as np
import pytest

from catfish_amd import infer
from catfish_amd.span_scores import SCORE_COLUMNS, span_score_summary, span_scores_host, summary_rows
from oracle import catfish_oracle as oracle
from test_span_scores_host import MIN_RUNS, THRESHOLDS, brute_force, check_rows, planted_batch
from test_span_scores_replay import check_hostile_rows, hostile_starts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = -7777
U = 2.0 ** -53


@pytest.fixture(scope="module")
def model(hp):
    from catfish_amd.resnet_class import ResNetRNN
    m = ResNetRNN(**hp)
    with np.load(os.path.join(GOLDEN, "ckpnt-30000-inference.npz")) as z:
        m.set_weights({k: z[k] for k in z.files})
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def engine(model):
    return model.engine


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


@pytest.fixture(scope="module")
def planted():
    """The planted batch on the card, and per (threshold, min_run) the host statement and the brute-force rows, computed once."""
    host = planted_batch()
    case = {"host": host, "probs": _dev(host[0]), "signal": _dev(host[1]), "offsets": _dev(host[2]), "lengths": _dev(host[3]), "want": {}}
    for t in THRESHOLDS:
        for m in MIN_RUNS:
            case["want"][(t, m)] = (span_scores_host(*host, t, m), brute_force(*host, t, m))
    return case


def device_rows(engine, case, threshold, starts, count, signal=True):
    """cf_span_scores over a start list and a count of the caller's -> (ends_paired, sums, extremes) numpy, sentinel-filled before."""
    import torch
    m = len(starts)
    out = (torch.full((m,), SENTINEL, dtype=torch.int64, device="cuda:0"), torch.full((m, 3), float(SENTINEL), dtype=torch.float64, device="cuda:0"),
           torch.full((m, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0"))
    counts = _dev(np.array([count, count], dtype=np.int64))
    engine.span_scores_device(case["probs"], case["signal"] if signal else None, case["offsets"], case["lengths"],
                              _dev(np.asarray(starts, dtype=np.int64)), counts, threshold, out=out)
    torch.cuda.synchronize()
    engine.check_error()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("min_run", MIN_RUNS)
def test_planted_batch_through_the_engine(engine, planted, threshold, min_run):
    want, brute = planted["want"][(threshold, min_run)]
    starts, ends, got = engine.postprocess_spans_device(planted["probs"], planted["offsets"], planted["lengths"], threshold, min_run,
                                                        scores=True, signal=planted["signal"])
    assert np.array_equal(starts, want["start"]) and np.array_equal(ends, want["end"])
    check_rows(got, brute)
    for key in ("start", "end", "read", "min_p", "max_p"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    # scores off: the two lists alone, as before
    plain = engine.postprocess_spans_device(planted["probs"], planted["offsets"], planted["lengths"], threshold, min_run)
    assert len(plain) == 2 and np.array_equal(plain[0], starts) and np.array_equal(plain[1], ends)


def test_two_calls_give_the_same_bits_and_rows_above_the_count_stay(engine, planted):
    want, _brute = planted["want"][(0.5, 15)]
    n = len(want["start"])
    starts = np.concatenate((want["start"][::-1], [0, 100, 200, 300]))      # unsorted, and four rows above the count
    a = device_rows(engine, planted, 0.5, starts, n)
    b = device_rows(engine, planted, 0.5, starts, n)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    ends, sums, extremes = a
    assert (ends[n:] == SENTINEL).all() and (sums[n:] == SENTINEL).all() and (extremes[n:] == SENTINEL).all()
    assert np.array_equal(ends[:n], want["end"][::-1]) and extremes[:n, 0].tobytes() == want["min_p"][::-1].tobytes()
    # a count of 0: nothing is written at all
    ends, sums, extremes = device_rows(engine, planted, 0.5, starts, 0)
    assert (ends == SENTINEL).all() and (sums == SENTINEL).all() and (extremes == SENTINEL).all()


def test_fewer_rows_than_runs_and_the_wrappers_retry(engine, planted):
    want, brute = planted["want"][(0.5, 15)]
    n = len(want["start"])
    assert n > 8
    ends, sums, extremes = device_rows(engine, planted, 0.5, want["start"][:5], n)       # the count says n, the lists hold 5
    assert np.array_equal(ends, want["end"][:5]) and extremes[:, 1].tobytes() == want["max_p"][:5].tobytes()
    starts, ends, got = engine.postprocess_spans_device(planted["probs"], planted["offsets"], planted["lengths"], 0.5, 15, max_runs=3,
                                                        scores=True, signal=planted["signal"])
    assert len(starts) == n and np.array_equal(ends, want["end"])
    check_rows(got, brute)


def test_without_the_signal_the_level_columns_are_not_written(engine, planted):
    want, brute = planted["want"][(0.9, 15)]
    n = len(want["start"])
    ends, sums, extremes = device_rows(engine, planted, 0.9, want["start"], n, signal=False)
    assert (sums[:, 1:] == SENTINEL).all() and np.array_equal(ends, want["end"])
    assert extremes[:, 0].tobytes() == want["min_p"].tobytes() and extremes[:, 1].tobytes() == want["max_p"].tobytes()
    _s, _e, got = engine.postprocess_spans_device(planted["probs"], planted["offsets"], planted["lengths"], 0.9, 15, scores=True)
    check_rows(got, brute, signal=False)
    assert np.isnan(got["sum_x"]).all() and np.isnan(got["sum_x2"]).all()


def test_hostile_start_lists(engine, planted):
    starts, expect = hostile_starts(planted["host"])
    ends, sums, extremes = device_rows(engine, planted, 0.5, starts, len(starts))
    check_hostile_rows(planted["host"], starts, expect, ends, sums, extremes)
    ends, sums, extremes = device_rows(engine, planted, 0.5, starts[:5], 1 << 40)        # a count larger than max_runs
    check_hostile_rows(planted["host"], starts[:5], expect[:5], ends, sums, extremes)
    ends, sums, extremes = device_rows(engine, planted, 0.5, starts, len(starts), signal=False)
    check_hostile_rows(planted["host"], starts, expect, ends, sums, extremes, with_signal=False)
    engine.check_error()


def summary_tolerances(flat, probs, signal):
    """How far two summaries of the same runs may differ when each of their sums lies within the any-order bound b = n u sum |v|
    (u = 2**-53) of the exact one, so that two sums differ by at most 2 b; every division and root adds a rounding of u relative:
      mean_p:  2 b_p / n + 2 u |mean|            level L:  t_L = 2 b_x / n + 2 u |L|
      variance V = s2 / n - L**2:  t_V = 2 b_x2 / n + (2 |L| + t_L) t_L + 4 u (s2 / n + L**2)
      spread = sqrt(V):  |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= t_V / spread, or sqrt(t_V) where the spread is 0."""
    s = span_score_summary(flat)
    tol = {"mean_p": [], "level": [], "spread": []}
    for k, (a, e) in enumerate(zip(flat["start"].tolist(), flat["end"].tolist())):
        n = e - a
        p, x = probs[a:e].astype(np.float64), signal[a:e].astype(np.float64)
        b_p, b_x, b_x2 = (n * U * math.fsum(np.abs(v).tolist()) for v in (p, x, x * x))
        level = abs(float(s["level"][k]))
        t_l = 2 * b_x / n + 2 * U * level
        t_v = 2 * b_x2 / n + (2 * level + t_l) * t_l + 4 * U * (float(flat["sum_x2"][k]) / n + level * level)
        spread = float(s["spread"][k])
        tol["mean_p"].append(2 * b_p / n + 2 * U * abs(float(s["mean_p"][k])))
        tol["level"].append(t_l)
        tol["spread"].append(t_v / spread + 2 * U * spread if spread > 0 else math.sqrt(t_v))
    return s, {k: np.array(v) for k, v in tol.items()}


def check_summary_rows(rows, flat, probs, signal):
    """``rows`` [n_runs, 6] against the summary of the host statement ``flat``: n, min_p and max_p exactly, the rest within
    ``summary_tolerances``."""
    s, tol = summary_tolerances(flat, probs, signal)
    want = summary_rows(s)
    assert rows.dtype == np.float64 and rows.shape == want.shape
    for c, name in enumerate(SCORE_COLUMNS):
        if name in tol:
            assert (np.abs(rows[:, c] - want[:, c]) <= tol[name]).all(), (name, np.abs(rows[:, c] - want[:, c]).max(), tol[name].min())
        else:
            assert np.array_equal(rows[:, c], want[:, c]), name


def test_infer_class_from_raw_with_scores(model):
    dac = oracle.synthetic_dac(1, 4096, seed=1)[0]
    sig = oracle.normalize_raw_signal(dac)
    spans, length = infer.infer_class_from_raw(sig, model)
    spans2, length2, rows = infer.infer_class_from_raw(sig, model, scores=True)
    assert (spans2, length2) == (spans, length) and length == 4096 and len(spans) >= 1
    pad = infer.padding_size_for(4096)
    raw_in = infer.reshape_input(np.hstack((sig, np.zeros(pad))), 35, 1)
    probs = model.infer(raw_in).astype(np.float32)
    x = raw_in.astype(np.float32).reshape(-1)
    flat = span_scores_host(probs, x, [0, len(x)], [4096])
    assert [[int(a) - 11, int(b) + 16] for a, b in zip(flat["start"], flat["end"])] == spans
    check_summary_rows(rows, flat, probs, x)


def test_the_pipeline_with_scores(model):
    import torch
    from catfish_amd.pipeline import ReadPipeline, StreamingPipeline
    assert StreamingPipeline is ReadPipeline
    dacs = [oracle.synthetic_dac(1, n, seed=40 + i)[0] for i, n in enumerate((34, 35, 4096))]
    plain = ReadPipeline(model.engine, 12000)
    want_lists = plain.collect(plain.submit(dacs))
    want_flat = plain.collect(plain.submit(dacs), as_lists=False)
    assert all(len(r) == 2 for r in want_lists) and len(want_flat) == 4 and sum(len(r[0]) for r in want_lists) >= 1
    pipe = ReadPipeline(model.engine, 12000, scores=True)
    for as_lists in (True, False):
        t = pipe.submit(dacs)
        t.done.synchronize()
        x, probs = t.keep[2].cpu().numpy().reshape(-1), t.keep[3].cpu().numpy()      # what the batch's kernels saw
        flat = span_scores_host(probs, x, t.s_off, t.lengths)
        got = pipe.collect(t, as_lists=as_lists)
        if as_lists:
            assert [r[:2] for r in got] == want_lists and all(len(r) == 3 for r in got)
            assert [len(r[2]) for r in got] == [len(r[0]) for r in got]
            check_summary_rows(np.concatenate([r[2] for r in got]), flat, probs, x)
        else:
            assert len(got) == 5 and all(np.array_equal(a, b) for a, b in zip(got[:4], want_flat))
            assert np.array_equal(got[4]["read"], got[0]) and np.array_equal(got[4]["start"], flat["start"])
            check_summary_rows(summary_rows(got[4]), flat, probs, x)
    # min_run > 64 takes the two older span kernels: the scores ride behind them all the same
    wide = ReadPipeline(model.engine, 12000, min_run=65, scores=True)
    t = wide.submit(dacs)
    t.done.synchronize()
    x, probs = t.keep[2].cpu().numpy().reshape(-1), t.keep[3].cpu().numpy()
    flat = span_scores_host(probs, x, t.s_off, t.lengths, 0.5, 65)
    got = wide.collect(t)
    assert sum(len(r[0]) for r in got) == len(flat["start"])
    if len(flat["start"]):
        check_summary_rows(np.concatenate([r[2] for r in got]), flat, probs, x)
    torch.cuda.synchronize()
    model.engine.check_error()
