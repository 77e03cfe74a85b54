"""Shifted-window voting: the same reads through the network in several tilings, merged per sample.  This module is the definition
(numpy, host); ``cf_retile_windows`` and ``cf_vote_tilings`` (csrc/tilings.hpp, index rules in csrc/tilings_rule.hpp) compute the
same bits on the card.

A read is cut into independent 35-sample windows at one fixed phase: window k covers samples 35 k .. 35 k + 34 (the reference's rule).
Tiling j shifts every read right by ``phases[j]`` samples before it is cut, so that its window borders fall elsewhere; the network
sees all tilings as one larger batch, and the per-sample results are merged by a weighted mean.

Base layout (what the pipeline and the validation round use): ``offsets`` int64 [n + 1], multiples of 35; ``lengths`` int64 [n];
read r owns packed samples ``offsets[r] .. offsets[r + 1]``, the first ``lengths[r]`` real and the rest zero; ``total = offsets[n]``.
Tiling j >= 1 gives every read one window more, in one contiguous buffer of ``tiling_size`` samples behind the base region:

    T_j = total + (j - 1) * (total + 35 n)                                   (T_0 = 0: the base region itself)
    retiled[T_j + offsets[r] + 35 r + phases[j] + i] = base[offsets[r] + i]      for 0 <= i < lengths[r]; every other sample is 0

Whether voting improves the calls on real reads is not known: ``train_validate.tiling_sweep`` is the tool to find out.
"""
from __future__ import annotations

import numpy as np

WINDOW_SIZE = 35
MAX_PHASES = 8
WEIGHTS = ("mean", "centre")


def check_phases(phases):
    """``phases`` as a tuple of ints, or a ValueError that names the rule broken: ints, strictly ascending, the first one 0, every one
    in 0 .. 34, between one and eight of them.  ``(0,)`` -- and None -- is one tiling: today's behaviour."""
    if phases is None:
        return (0,)
    if isinstance(phases, (str, bytes)) or not hasattr(phases, "__iter__"):
        raise ValueError("phases must be a sequence of ints, got %r" % (phases,))
    phases = list(phases)
    for p in phases:
        if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, np.integer)):
            raise ValueError("phases must be ints, got %r" % (p,))
    phases = tuple(int(p) for p in phases)
    if not 1 <= len(phases) <= MAX_PHASES:
        raise ValueError("phases: between 1 and %d tilings, got %d" % (MAX_PHASES, len(phases)))
    if phases[0] != 0:
        raise ValueError("phases: the first phase must be 0 (the base tiling), got %d" % phases[0])
    for a, b in zip(phases, phases[1:]):
        if b <= a:
            raise ValueError("phases must be strictly ascending, got %r" % (phases,))
    if phases[-1] >= WINDOW_SIZE:
        raise ValueError("phases: every phase must be in 0 .. %d, got %d" % (WINDOW_SIZE - 1, phases[-1]))
    return phases


def check_weight(weight):
    """``weight`` as the int the C ABI takes (0 mean, 1 centre); ValueError for anything else."""
    if weight is None:
        return 0
    if isinstance(weight, str) and weight in WEIGHTS:
        return WEIGHTS.index(weight)
    raise ValueError("vote weight must be one of %s, got %r" % (" / ".join(repr(w) for w in WEIGHTS), weight))


def window_weight(weight, t):
    """w(t) for positions ``t`` (array) of the window: 1 (mean), or min(t + 1, 35 - t) (centre: 1 at both ends, 18 in the middle)."""
    t = np.asarray(t, dtype=np.int64)
    if check_weight(weight) == 0:
        return np.ones(t.shape, dtype=np.float64)
    return np.minimum(t + 1, WINDOW_SIZE - t).astype(np.float64)


def phases_from_env(value):
    """``CATFISH_TILINGS``: comma-separated phases, e.g. ``0,12,23``; unset (None) or empty means ``(0,)``."""
    if value is None or not value.strip():
        return (0,)
    try:
        phases = [int(v.strip()) for v in value.split(",")]
    except ValueError:
        raise ValueError("CATFISH_TILINGS must be comma-separated ints such as 0,12,23, got %r" % (value,))
    return check_phases(phases)


def weight_from_env(value):
    """``CATFISH_TILING_WEIGHT``: ``mean`` or ``centre``; unset (None) or empty means ``mean``."""
    if value is None or not value.strip():
        return "mean"
    value = value.strip()
    check_weight(value)
    return value


def region_size(total, n_reads):
    """Samples of one tiling j >= 1: every read one window longer than in the base layout."""
    return int(total) + WINDOW_SIZE * int(n_reads)


def tiling_start(j, total, n_reads):
    """T_j: the first sample of tiling j in the one buffer."""
    return 0 if j <= 0 else int(total) + (int(j) - 1) * region_size(total, n_reads)


def tiling_size(total, n_reads, n_phases):
    """Samples of the one buffer that holds the base region and the ``n_phases - 1`` tilings behind it (a multiple of 35)."""
    return tiling_start(int(n_phases), total, n_reads)


def _sound(o0, o1, length, total):
    """What the layout promises of one read's entries (csrc/tilings_rule.hpp: tl_sound); a read that breaks it is all zero in the
    tilings and keeps its base values in the vote."""
    return 0 <= o0 <= o1 <= total and o0 % WINDOW_SIZE == 0 and o1 % WINDOW_SIZE == 0 and 0 <= length <= o1 - o0


def _tables(offsets, lengths, total):
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if len(offsets) != len(lengths) + 1:
        raise ValueError("offsets must have n_reads + 1 entries")
    total = int(offsets[-1]) if total is None else int(total)
    if total < 0 or total % WINDOW_SIZE != 0:
        raise ValueError("total must be a non-negative multiple of %d, got %d" % (WINDOW_SIZE, total))
    return offsets, lengths, total


def retile_host(base, offsets, lengths, phases, total=None):
    """The one buffer, float32 [tiling_size]: ``base[:total]`` followed by tilings 1 .. K - 1 of it (the module's rule).  ``total``
    defaults to ``offsets[-1]``."""
    phases = check_phases(phases)
    offsets, lengths, total = _tables(offsets, lengths, total)
    base = np.asarray(base, dtype=np.float32).reshape(-1)
    if len(base) < total:
        raise ValueError("base holds %d samples, the layout %d" % (len(base), total))
    n = len(lengths)
    out = np.zeros(tiling_size(total, n, len(phases)), dtype=np.float32)
    out[:total] = base[:total]
    for j in range(1, len(phases)):
        t_j = tiling_start(j, total, n)
        for r in range(n):
            o0, o1, ln = int(offsets[r]), int(offsets[r + 1]), int(lengths[r])
            if _sound(o0, o1, ln, total) and ln:
                d = t_j + o0 + WINDOW_SIZE * r + phases[j]
                out[d:d + ln] = base[o0:o0 + ln]
    return out


def vote_host(values_all, offsets, lengths, phases, weight="mean", total=None):
    """The vote over one float32 array [tiling_size] of per-sample values (probabilities -- or logits: the voted logit is the weighted
    mean of the logits, NOT the logit of the voted probability) -> float32 [total]:

        voted[offsets[r] + i] = float32((sum_j w(t_j) * double(p_j)) / (sum_j w(t_j))),   t_j = (i + phases[j]) % 35

    for 0 <= i < lengths[r], both sums in double in the order j = 0 .. K - 1; samples of the zero tails keep the base value.  With
    one phase the output is the input, bit for bit."""
    phases = check_phases(phases)
    check_weight(weight)
    offsets, lengths, total = _tables(offsets, lengths, total)
    n = len(lengths)
    values_all = np.asarray(values_all, dtype=np.float32).reshape(-1)
    if len(values_all) < tiling_size(total, n, len(phases)):
        raise ValueError("values hold %d samples, the tilings %d" % (len(values_all), tiling_size(total, n, len(phases))))
    out = values_all[:total].copy()
    if len(phases) == 1:
        return out
    for r in range(n):
        o0, o1, ln = int(offsets[r]), int(offsets[r + 1]), int(lengths[r])
        if not _sound(o0, o1, ln, total) or ln == 0:
            continue
        i = np.arange(ln, dtype=np.int64)
        num, den = np.zeros(ln, dtype=np.float64), np.zeros(ln, dtype=np.float64)
        for j, phi in enumerate(phases):
            w = window_weight(weight, (i + phi) % WINDOW_SIZE)
            first = tiling_start(j, total, n) + o0 + (WINDOW_SIZE * r + phi if j else 0)
            num = num + w * values_all[first:first + ln].astype(np.float64)
            den = den + w
        out[o0:o0 + ln] = (num / den).astype(np.float32)
    return out


def voted_probs_of_read(raw_in, infer_fn, length, phases, weight="mean"):
    """One read, already padded and windowed as ``infer.infer_class_from_raw`` does it (``raw_in``: [n_windows, 35, 1] or anything
    of n_windows * 35 values): every tiling goes through ``infer_fn`` ([m, 35, 1] -> m * 35 probabilities, ``model.infer``) on its own,
    and the votes come back as float32 [n_windows * 35].  With one phase: ``infer_fn(raw_in)`` as float32."""
    phases = check_phases(phases)
    base = np.asarray(raw_in, dtype=np.float64).reshape(-1)
    total, length = len(base), int(length)
    offsets, lengths = np.array([0, total], dtype=np.int64), np.array([length], dtype=np.int64)
    if total % WINDOW_SIZE != 0 or not 0 <= length <= total:
        raise ValueError("a padded read of %d samples cannot hold %d real ones in windows of %d" % (total, length, WINDOW_SIZE))
    parts = [np.asarray(infer_fn(np.asarray(raw_in)), dtype=np.float32).reshape(-1)]
    for phi in phases[1:]:
        shifted = np.zeros(total + WINDOW_SIZE, dtype=base.dtype)
        shifted[phi:phi + length] = base[:length]
        parts.append(np.asarray(infer_fn(shifted.reshape(-1, WINDOW_SIZE, 1)), dtype=np.float32).reshape(-1))
    if len(phases) == 1:
        return parts[0]
    return vote_host(np.concatenate(parts), offsets, lengths, phases, weight, total=total)
