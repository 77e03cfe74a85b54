"""``span_scores.span_scores_host`` -- the definition of the per-call scores -- against a brute-force loop over the reads built from
the reference's own post-processing steps (``infer.class_from_threshold``, ``correct_short``, ``hp_in_pred(..., 0, 0)``) and
``math.fsum``: on the planted batch that the replay and the GPU tests use as well (they import it from here) and on 200 random
batches."""
import math

import numpy as np
import pytest

from catfish_amd import infer
from catfish_amd.batching import scores_from_runs, spans_from_runs
from catfish_amd.span_scores import SCORE_COLUMNS, span_score_summary, span_scores_host, summary_rows

THRESHOLDS = (0.5, 0.9)
MIN_RUNS = (1, 15, 64, 65)
RUN_LENGTHS = (63, 64, 65, 127, 128, 129)                  # around one and two steps of the walk


def planted_batch():
    """(probs float32, signal float32, sample_offsets int64 [9], lengths int64 [8]): 8 reads, fewer than 20 000 samples.  Calm
    samples lie below 0.45, run samples at or above 0.9 unless said, and every padding sample is 0.99: padding that is taken for
    a sample shows."""
    rng = np.random.default_rng(11)
    reads = []                                             # (probabilities of the real part, allocated samples)

    def calm(n):
        return (rng.random(n) * 0.45).astype(np.float32)

    def sure(n):
        return (0.9 + rng.random(n) * 0.0999).astype(np.float32)

    # read 0: a run at sample 0; runs of min_run - 1 and min_run samples for every min_run swept (0 / 1, 14 / 15, 63 / 64, 64 / 65)
    # and of 127 .. 129; a run that ends on the last real sample, padding behind it
    p = calm(3000)
    p[0:40] = sure(40)
    at = 50
    for n in (1, 14, 15) + RUN_LENGTHS:
        p[at:at + n] = sure(n)
        at += n + 7
    p[2950:3000] = sure(50)
    reads.append((p, 3045))
    # reads 1 and 2: packed without padding, positive on both sides of the boundary -- two runs
    p = calm(700)
    p[670:700] = sure(30)
    reads.append((p, 700))
    p = calm(350)
    p[0:25] = sure(25)
    reads.append((p, 385))
    # read 3: the same lengths started at packed positions 64 k - 1, 64 k and 64 k + 1
    base = sum(alloc for _p, alloc in reads)
    p = calm(4200)
    at = 10
    for n in RUN_LENGTHS:
        for delta in (-1, 0, 1):
            k = (base + at + 1 + 63) // 64
            first = 64 * k + delta - base
            assert first >= at
            p[first:first + n] = sure(n)
            at = first + n + 3
    assert at < 4200
    reads.append((p, 4235))
    # read 4: one run of 5 000 samples
    p = calm(5200)
    p[100:5100] = sure(5000)
    reads.append((p, 5215))
    # read 5: a NaN inside a run (it splits); values equal to either threshold at a run's first, last and inner samples (inside);
    # a run whose middle lies between the thresholds (one run at 0.5, two at 0.9)
    p = calm(600)
    p[20:100] = sure(80)
    p[50] = np.nan
    p[150:190] = sure(40)
    p[[150, 170, 189]] = np.float32(0.5)
    p[250:290] = sure(40)
    p[[250, 260, 289]] = np.float32(0.9)
    p[350:450] = sure(100)
    p[390:410] = (0.6 + rng.random(20) * 0.2).astype(np.float32)
    reads.append((p, 630))
    # read 6: no run; read 7: one sample
    reads.append((calm(300), 315))
    reads.append((sure(1), 35))
    lengths = np.array([len(p) for p, _alloc in reads], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum([alloc for _p, alloc in reads]))).astype(np.int64)
    probs = np.full(int(offsets[-1]), 0.99, dtype=np.float32)
    for o, (p, _alloc) in zip(offsets[:-1].tolist(), reads):
        probs[o:o + len(p)] = p
    signal = rng.standard_normal(probs.shape[0]).astype(np.float32) * np.float32(1.5) + np.float32(0.25)
    assert len(reads) == 8 and probs.shape[0] < 20000
    return probs, signal, offsets, lengths


def brute_force(probs, signal, offsets, lengths, threshold, min_run):
    """One dict per kept run, read by read, from the reference's post-processing steps and exact sums."""
    rows = []
    for r, (o, n) in enumerate(zip(offsets[:-1].tolist(), lengths.tolist())):
        p = probs[o:o + n]
        with np.errstate(invalid="ignore"):
            labels = infer.correct_short(infer.class_from_threshold(p, np.float32(threshold)), min_run)
        for s, e in infer.hp_in_pred(labels, 0, 0):
            ps = [float(v) for v in p[s:e]]
            xs = [float(v) for v in signal[o + s:o + e]]
            rows.append({"read": r, "start": o + s, "end": o + e, "p": ps, "x": xs, "x2": [v * v for v in xs],
                         "min_p": p[s:e].min(), "max_p": p[s:e].max()})
    return rows


def check_rows(got, want, signal=True):
    """``got``: a flat score dict sorted by start; ``want``: brute_force's rows.  Positions and extremes bit for bit, every sum within
    n * 2**-53 * sum |v| of the exact one: the bound of a float64 sum of n values taken in ANY order (each of the n - 1 additions
    rounds a partial sum no larger than sum |v| by at most 2**-53 of it)."""
    assert got["start"].dtype == got["end"].dtype == got["read"].dtype == np.int64
    assert got["min_p"].dtype == got["max_p"].dtype == np.float32
    assert got["sum_p"].dtype == got["sum_x"].dtype == got["sum_x2"].dtype == np.float64
    assert got["start"].tolist() == [w["start"] for w in want]
    assert got["end"].tolist() == [w["end"] for w in want]
    assert got["read"].tolist() == [w["read"] for w in want]
    assert got["min_p"].tobytes() == np.array([w["min_p"] for w in want], np.float32).tobytes()
    assert got["max_p"].tobytes() == np.array([w["max_p"] for w in want], np.float32).tobytes()
    for key, vals in (("sum_p", "p"),) + ((("sum_x", "x"), ("sum_x2", "x2")) if signal else ()):
        for k, w in enumerate(want):
            v = w[vals]
            bound = len(v) * 2.0 ** -53 * math.fsum(abs(t) for t in v)
            assert abs(float(got[key][k]) - math.fsum(v)) <= bound, (key, k, float(got[key][k]), math.fsum(v), bound)


@pytest.fixture(scope="module")
def planted():
    return planted_batch()


def test_the_planted_batch_holds_what_it_says(planted):
    probs, signal, offsets, lengths = planted
    got = span_scores_host(probs, signal, offsets, lengths, 0.5, 15)
    n = (got["end"] - got["start"]).tolist()
    assert got["start"][0] == 0 and 5000 in n and all(v in n for v in (15,) + RUN_LENGTHS) and 14 not in n
    assert n.count(63) >= 4 and n.count(129) >= 4
    for delta in (63, 0, 1):                               # starts at 64 k - 1, 64 k, 64 k + 1 in read 3
        assert sum(1 for s, r in zip(got["start"].tolist(), got["read"].tolist()) if r == 3 and s % 64 == delta) >= 6
    assert offsets[1] + lengths[1] in got["end"].tolist() and offsets[2] in got["start"].tolist() and offsets[2] in got["end"].tolist()
    assert offsets[0] + lengths[0] in got["end"].tolist()  # ends on the last real sample, not in the padding
    assert 6 not in got["read"].tolist() and 7 not in got["read"].tolist()
    one = span_scores_host(probs, signal, offsets, lengths, 0.5, 1)
    assert 7 in one["read"].tolist() and 1 in (one["end"] - one["start"]).tolist()
    assert {30, 49} <= set((got["end"] - got["start"])[got["read"] == 5].tolist())      # the NaN splits its run
    assert (got["min_p"][got["read"] == 5] == np.float32(0.5)).sum() == 1               # values equal to the threshold are inside
    nine = span_scores_host(probs, signal, offsets, lengths, 0.9, 15)
    assert (nine["min_p"][nine["read"] == 5] == np.float32(0.9)).sum() == 1
    assert len(nine["start"]) > len(got["start"]) - 2


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("min_run", MIN_RUNS)
def test_planted_batch_against_the_brute_force_loop(planted, threshold, min_run):
    probs, signal, offsets, lengths = planted
    got = span_scores_host(probs, signal, offsets, lengths, threshold, min_run)
    want = brute_force(probs, signal, offsets, lengths, threshold, min_run)
    assert len(want) > 5
    check_rows(got, want)
    # start and end are what spans_from_runs inverts: the per-read [start - 11, end + 16] lists of hp_in_pred
    spans = spans_from_runs(got["start"], got["end"], offsets, len(lengths))
    for r, (o, n) in enumerate(zip(offsets[:-1].tolist(), lengths.tolist())):
        with np.errstate(invalid="ignore"):
            labels = infer.correct_short(infer.class_from_threshold(probs[o:o + n], np.float32(threshold)), min_run)
        assert spans[r] == infer.hp_in_pred(labels)
    none = span_scores_host(probs, None, offsets, lengths, threshold, min_run)
    check_rows(none, want, signal=False)
    assert np.isnan(none["sum_x"]).all() and np.isnan(none["sum_x2"]).all()


def random_batch(rng):
    n_reads = int(rng.integers(1, 6))
    lengths = rng.integers(1, 300, n_reads).astype(np.int64)
    pads = rng.integers(0, 40, n_reads) * (rng.random(n_reads) < 0.7)
    offsets = np.concatenate(([0], np.cumsum(lengths + pads))).astype(np.int64)
    total = int(offsets[-1])
    flips = np.cumsum(rng.random(total) < 0.06) & 1         # streaks of ~ 16 samples
    probs = np.where(flips == 1, 0.5 + 0.5 * rng.random(total), 0.5 * rng.random(total)).astype(np.float32)
    probs[rng.random(total) < 0.01] = np.nan
    probs[rng.random(total) < 0.02] = np.float32(0.5)
    probs[rng.random(total) < 0.02] = np.float32(0.9)
    signal = (rng.standard_normal(total) * 2.0).astype(np.float32)
    return probs, signal, offsets, lengths


def test_200_random_batches_against_the_brute_force_loop():
    rng = np.random.default_rng(2024)
    runs = 0
    for _ in range(200):
        batch = random_batch(rng)
        threshold = float(rng.choice([0.5, 0.9, 0.3, 0.75]))
        min_run = int(rng.choice([1, 2, 5, 15, 20, 64, 65]))
        got = span_scores_host(*batch, threshold, min_run)
        want = brute_force(*batch, threshold, min_run)
        check_rows(got, want)
        runs += len(want)
    assert runs > 1000


def test_summary_columns_and_the_per_read_split(planted):
    probs, signal, offsets, lengths = planted
    flat = span_scores_host(probs, signal, offsets, lengths)
    s = span_score_summary(flat)
    n = (flat["end"] - flat["start"]).astype(np.float64)
    assert all(s[c].dtype == np.float64 for c in SCORE_COLUMNS)
    assert np.array_equal(s["n"], n) and np.array_equal(s["mean_p"], flat["sum_p"] / n)
    assert np.array_equal(s["level"], flat["sum_x"] / n)
    assert np.array_equal(s["spread"], np.sqrt(np.maximum(0.0, flat["sum_x2"] / n - (flat["sum_x"] / n) ** 2)))
    assert np.array_equal(s["min_p"], flat["min_p"].astype(np.float64)) and np.array_equal(s["max_p"], flat["max_p"].astype(np.float64))
    k = int(np.argmax(n))                                  # the run of 5 000: mean and spread of the signal under it
    x = signal[flat["start"][k]:flat["end"][k]].astype(np.float64)
    assert abs(s["level"][k] - x.mean()) < 1e-12 and abs(s["spread"][k] - x.std()) < 1e-12
    rows = summary_rows(s)
    per_read = scores_from_runs(flat, len(lengths))
    spans = spans_from_runs(flat["start"], flat["end"], offsets, len(lengths))
    assert [len(a) for a in per_read] == [len(b) for b in spans] and per_read[6].shape == (0, 6)
    assert np.array_equal(np.concatenate(per_read), rows)
    empty = span_scores_host(np.zeros(70, np.float32), np.zeros(70, np.float32), [0, 70], [60])
    assert len(empty["start"]) == 0 and summary_rows(span_score_summary(empty)).shape == (0, 6)
    assert [a.shape for a in scores_from_runs(empty, 1)] == [(0, 6)]


class _HostModel(object):
    """A model without an engine: probabilities planted per window."""

    def __init__(self, probs):
        self.probs = probs

    def infer(self, raw_in):
        assert raw_in.shape[1:] == (35, 1)
        return self.probs[:raw_in.shape[0] * 35].astype(float)


def test_infer_class_from_raw_with_scores_on_a_model_without_an_engine():
    rng = np.random.default_rng(5)
    raw = rng.standard_normal(1000)
    probs = np.full(1015, 0.99, dtype=np.float32)
    probs[:1000] = (rng.random(1000) * 0.4).astype(np.float32)
    probs[100:160] = 0.93
    probs[400:414] = 0.93                                  # 14: dropped by correct_short
    probs[950:1000] = 0.71
    model = _HostModel(probs)
    spans, length = infer.infer_class_from_raw(raw, model)
    spans2, length2, rows = infer.infer_class_from_raw(raw, model, scores=True)
    assert (spans2, length2) == (spans, length) == ([[89, 176], [939, 1016]], 1000)
    assert rows.shape == (2, 6) and rows.dtype == np.float64
    assert rows[:, 0].tolist() == [60.0, 50.0]
    assert np.allclose(rows[:, 1], [np.float32(0.93), np.float32(0.71)], rtol=0, atol=1e-12)
    x = raw.astype(np.float32).astype(np.float64)
    assert abs(rows[0, 4] - x[100:160].mean()) < 1e-12 and abs(rows[1, 5] - x[950:1000].std()) < 1e-12
