"""Per-call scores of homopolymer calls: how sure the network was of a called run, at what current level the stretch sits and
how flat it is.

``span_scores_host`` is the definition in numpy; ``cf_span_scores`` (csrc/span_scores.hpp, over the index rules of
csrc/span_scores_rule.hpp) computes the same rows on the card for the runs ``cf_postprocess_spans`` reports, and
tests/native/span_scores_replay.cpp states the kernel's body serially.  A kept run is a maximal streak of ``p >= threshold``
(float32 compare, NaN is false) of at least ``min_run`` samples inside the real part of ONE read: the run definition of
``cf_postprocess_spans``, the cut between reads packed without padding included.
"""
from __future__ import annotations

import numpy as np

SCORE_COLUMNS = ("n", "mean_p", "min_p", "max_p", "level", "spread")      # the columns of a per-read score array, in order


def empty_scores():
    return {"read": np.zeros(0, np.int64), "start": np.zeros(0, np.int64), "end": np.zeros(0, np.int64),
            "sum_p": np.zeros(0, np.float64), "sum_x": np.zeros(0, np.float64), "sum_x2": np.zeros(0, np.float64),
            "min_p": np.zeros(0, np.float32), "max_p": np.zeros(0, np.float32)}


def span_scores_host(probs, signal, sample_offsets, lengths, threshold=0.5, min_run=15):
    """Packed float32 probabilities and normalised signal (what the network saw; None: no level sums, ``sum_x`` / ``sum_x2`` are
    NaN) -> dict of arrays, one entry per kept run, sorted by ``start``:

    read (int64)  start, end (int64, packed positions, end exclusive)  sum_p, sum_x, sum_x2 (float64: sums of the float32
    values widened to double, x * x formed in double)  min_p, max_p (float32)."""
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float32).reshape(-1))
    x = None if signal is None else np.ascontiguousarray(np.asarray(signal, dtype=np.float32).reshape(-1))
    if x is not None and x.shape[0] != p.shape[0]:
        raise ValueError("signal must have as many samples as probs")
    off = np.asarray(sample_offsets, dtype=np.int64).reshape(-1)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    n_reads, total = int(lengths.shape[0]), int(p.shape[0])
    if min_run < 1:
        raise ValueError("min_run must be >= 1")
    with np.errstate(invalid="ignore"):
        hit = p >= np.float32(threshold)
    real = np.zeros(total, dtype=bool)
    first = np.zeros(total + 1, dtype=bool)                # a read begins here: runs are cut
    for r in range(n_reads):
        beg = int(off[r])
        end = min(beg + int(lengths[r]), int(off[r + 1]) if r + 1 < off.shape[0] else total, total)
        if end > beg:
            real[beg:end] = True
            first[beg] = True
    hit &= real
    before = np.concatenate(([False], hit[:-1])) if total else hit
    after = np.concatenate((hit[1:], [False])) if total else hit
    starts = np.flatnonzero(hit & (~before | first[:total]))
    ends = np.flatnonzero(hit & (~after | first[1:total + 1])) + 1
    keep = ends - starts >= int(min_run)
    starts, ends = starts[keep].astype(np.int64), ends[keep].astype(np.int64)
    return scores_of_runs(p, x, starts, ends, off, n_reads)


def scores_of_runs(p, x, starts, ends, sample_offsets, n_reads):
    """The rows of given runs [starts[k], ends[k]) of packed float32 ``p`` (and ``x``, or None), starts ascending."""
    starts, ends = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    off = np.asarray(sample_offsets, dtype=np.int64)
    k = starts.shape[0]
    runs = list(zip(starts.tolist(), ends.tolist()))
    out = empty_scores()
    out["start"], out["end"] = starts, ends
    out["read"] = (np.searchsorted(off[:n_reads], starts, side="right") - 1).astype(np.int64)
    pd = p.astype(np.float64)
    # (numpy sums in an order of its own, the device in another: both lie within the any-order bound of float64 summation)
    out["sum_p"] = np.array([pd[s:e].sum() for s, e in runs], dtype=np.float64).reshape(k)
    out["min_p"] = np.array([p[s:e].min() for s, e in runs], dtype=np.float32).reshape(k)
    out["max_p"] = np.array([p[s:e].max() for s, e in runs], dtype=np.float32).reshape(k)
    if x is None:
        out["sum_x"] = np.full(k, np.nan)
        out["sum_x2"] = np.full(k, np.nan)
    else:
        xd = x.astype(np.float64)
        out["sum_x"] = np.array([xd[s:e].sum() for s, e in runs], dtype=np.float64).reshape(k)
        out["sum_x2"] = np.array([(xd[s:e] * xd[s:e]).sum() for s, e in runs], dtype=np.float64).reshape(k)
    return out


def span_score_summary(scores):
    """The flat score dict -> the per-run columns a user reads, all float64 except ``read``, ``start`` and ``end``:
    n, mean_p, min_p, max_p, level = sum_x / n, spread = sqrt(max(0, sum_x2 / n - level**2))."""
    n = (np.asarray(scores["end"], dtype=np.int64) - np.asarray(scores["start"], dtype=np.int64)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        level = np.asarray(scores["sum_x"], dtype=np.float64) / n
        spread = np.sqrt(np.maximum(0.0, np.asarray(scores["sum_x2"], dtype=np.float64) / n - level * level))
        mean_p = np.asarray(scores["sum_p"], dtype=np.float64) / n
    return {"read": np.asarray(scores["read"], dtype=np.int64), "start": np.asarray(scores["start"], dtype=np.int64),
            "end": np.asarray(scores["end"], dtype=np.int64), "n": n, "mean_p": mean_p,
            "min_p": np.asarray(scores["min_p"], dtype=np.float64), "max_p": np.asarray(scores["max_p"], dtype=np.float64),
            "level": level, "spread": spread}


def summary_rows(summary):
    """The summary dict as one float64 array [n_runs, 6]: columns ``SCORE_COLUMNS``."""
    if len(summary["n"]) == 0:
        return np.zeros((0, len(SCORE_COLUMNS)), dtype=np.float64)
    return np.stack([np.asarray(summary[c], dtype=np.float64) for c in SCORE_COLUMNS], axis=1)


def scores_from_device_rows(starts, ends_paired, sums, extremes, sample_offsets, n_reads, with_signal=True):
    """What ``cf_span_scores`` wrote next to the (unsorted) starts -> the flat dict sorted by start.  -> (dict, order): ``order`` is
    the stable argsort of the starts that the rows went through."""
    starts = np.asarray(starts, dtype=np.int64)
    order = np.argsort(starts, kind="stable")
    off = np.asarray(sample_offsets, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)[order]
    extremes = np.asarray(extremes, dtype=np.float32).reshape(-1, 2)[order]
    k = starts.shape[0]
    out = {"start": starts[order], "end": np.asarray(ends_paired, dtype=np.int64)[order]}
    out["read"] = (np.searchsorted(off[:n_reads], out["start"], side="right") - 1).astype(np.int64)
    out["sum_p"] = sums[:, 0].copy()
    out["sum_x"] = sums[:, 1].copy() if with_signal else np.full(k, np.nan)
    out["sum_x2"] = sums[:, 2].copy() if with_signal else np.full(k, np.nan)
    out["min_p"], out["max_p"] = extremes[:, 0].copy(), extremes[:, 1].copy()
    return out, order
