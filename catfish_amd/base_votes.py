"""Per-base calls: the samples of every base vote on it, and the voted bases are scored by base.

The reference's author sketched this step and marked it ``### NOT FINISHED ###``: ``networks/correct_output.py:correct_events`` walks a
resquiggled read's events, averages the scores of the samples that belong to each event and rounds that average to a class per base
("majority voting by measurements belong to that event").  Everything else here lives on the sample axis; this module puts the answer
on the base axis -- for a corrector or re-basecaller that works in base coordinates, and for an evaluation that does not weight a base
by how long the pore dwelt on it.

The numpy statements in this module are normative; ``cf_base_votes`` (csrc/base_votes.hpp, rules in csrc/base_votes_rule.hpp) computes
the same bits on the card:

``BaseTable``   which samples of a ``DeviceValidationSet`` belong to which base (``edges``) and which bases to which read.
``q_of``        the fixed point of a probability: ``floor(double(p) * 2^32)``, NaN and ``p < 0`` as 0, ``p > 1`` as 1 -- all sums are
                exact integers, so equal inputs give equal bits for any grid or reduction shape.
``vote_host``   one round's packed probabilities -> ``(sums, state, base_confusion, base_vote_runs)``.
``calls_of``    the called runs in base coordinates, per read.

The module is numpy only and usable without a GPU; torch is imported inside ``vote_device``."""
from __future__ import annotations

import numpy as np

from . import device_validation as dv

MAX_THRESHOLDS = 16         # thresholds per launch group (BV_MAX_K, csrc/base_votes_rule.hpp)
LONG_BASE = 256             # a base of more samples is summed by its whole wave (BV_LONG_BASE); no result depends on it
ONE = 1 << 32               # q(1.0)
CALLED, TRUTH, VOTED = 0x01, 0x02, 0x80                    # bits of a state byte; bits 2..4 hold the class
CONFUSION_CELLS = len(dv.BASE_CLASSES) * 4                 # one threshold's [5, 2, 2] table
VOTE_RESULTS = ("base_confusion", "base_vote_runs")        # a round's two tables, after ``validation_round.EXTRA_RESULTS``
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def q_of(p):
    """uint64 fixed point of float32 probabilities: NaN or ``p < 0`` -> 0, ``p > 1`` -> 2^32, else ``floor(double(p) * 2^32)`` (the
    product is exact).  ``q_of(0.5) == 2^31``, ``q_of(1) == 2^32``."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        clean = np.where(p >= 0, np.minimum(p, np.float32(1.0)), np.float32(0.0)).astype(np.float64)     # NaN fails p >= 0
    return np.floor(clean * float(ONE)).astype(np.uint64)


def base_classes(base_bytes):
    """Class per base byte (bit 7 ignored): 0..3 for upper-case ``A C G T``, 4 for anything else (``dv.BASE_CLASSES``)."""
    b = np.asarray(base_bytes, dtype=np.uint8) & 0x7f
    cls = np.full(b.shape, 4, dtype=np.int64)
    for c, letter in enumerate(_LETTERS):
        cls[b == letter] = c
    return cls


def check_vote_bases(vote_bases):
    """``vote_bases`` as an int in 1 .. 32 -- the ``max_bases`` of the vote-run table (``dv.check_max_bases``'s rule)."""
    try:
        return dv.check_max_bases(vote_bases)
    except ValueError:
        raise ValueError("vote_bases must be an int in 1 .. %d, got %r" % (dv.MAX_BASES_LIMIT, vote_bases))


class BaseTable(object):
    """Which samples belong to which base: ``edges`` int64 [n_bases + 1], strictly increasing from 0 to the set's total samples --
    base e owns samples ``edges[e] .. edges[e + 1] - 1`` of the set's concatenated arrays -- and ``base_offsets`` int64
    [n_reads + 1]: read r owns bases ``base_offsets[r] .. base_offsets[r + 1] - 1``.  Truth and base letter are not stored: they are
    ``labels[edges[e]] == 1`` and ``basemap[edges[e]] & 0x7f`` of the set.  A table that breaks a rule is a ValueError."""

    def __init__(self, edges, base_offsets):
        edges, base_offsets = np.asarray(edges), np.asarray(base_offsets)
        for name, a in (("edges", edges), ("base_offsets", base_offsets)):
            if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("%s must be a non-empty 1-d integer array" % name)
        edges, base_offsets = edges.astype(np.int64), base_offsets.astype(np.int64)
        if edges[0] != 0:
            raise ValueError("edges must begin at 0, got %d" % edges[0])
        if np.any(np.diff(edges) <= 0):
            raise ValueError("edges must be strictly increasing: every base owns at least one sample")
        if edges.size - 1 >= 2 ** 31 or edges[-1] >= 2 ** 31:
            raise ValueError("a table of 2^31 or more bases or samples")
        if base_offsets[0] != 0 or base_offsets[-1] != edges.size - 1 or np.any(np.diff(base_offsets) < 0):
            raise ValueError("base_offsets must ascend from 0 to the number of bases (%d)" % (edges.size - 1))
        self.edges, self.base_offsets = edges, base_offsets

    n_bases = property(lambda self: int(self.edges.size - 1))
    n_reads = property(lambda self: int(self.base_offsets.size - 1))
    total = property(lambda self: int(self.edges[-1]))

    def check_set(self, offsets):
        """ValueError unless the table belongs to a set with these read ``offsets``: ``edges[-1]`` is its total and
        ``edges[base_offsets[r]] == offsets[r]``."""
        offsets = np.asarray(offsets, dtype=np.int64)
        if offsets.size != self.base_offsets.size or self.total != int(offsets[-1]):
            raise ValueError("the base table covers %d reads and %d samples, the set has %d and %d"
                             % (self.n_reads, self.total, offsets.size - 1, int(offsets[-1])))
        if not np.array_equal(self.edges[self.base_offsets], offsets):
            raise ValueError("a read does not begin at a base border: edges[base_offsets[r]] must equal offsets[r]")
        return self

    @classmethod
    def from_batch(cls, batch):
        """The table of a ``labelling.EventBatch`` (a base per event) or ``labelling.MoveBatch`` (a base per merged event that kept a
        sample): the batch's own ``base_edges``."""
        return cls(*batch.base_edges()).check_set(batch.sample_offsets)

    from_events = from_moves = from_batch


def event_ranges(edges, src, length):
    """The host's part of a vote: per stretch ``(a, b)`` int64 -- ``a`` the first base with ``edges[e] >= src``, ``b`` the last with
    ``edges[e] <= src + length`` (never below ``a``); the voted bases are ``a .. b - 1``, the events that lie wholly inside the stretch,
    as the reference's loop takes them.  ValueError when two stretches share a voted base (a base has one sum)."""
    edges = np.asarray(edges, dtype=np.int64)
    src, length = np.asarray(src, dtype=np.int64), np.asarray(length, dtype=np.int64)
    a = np.searchsorted(edges, src, side="left").astype(np.int64)
    b = np.maximum(np.searchsorted(edges, src + length, side="right").astype(np.int64) - 1, a)
    order = np.argsort(a, kind="stable")
    held = order[(b > a)[order]]
    if held.size > 1 and np.any(a[held][1:] < b[held][:-1]):
        raise ValueError("two stretches share a voted base: every base is voted by one stretch of a round")
    return a, b


def _voted_span(edges, n_bases, e, src, length, bound, total, set_total):
    """bv_span: (first sample, packed place, samples) of base e when its stretch votes it, else None."""
    limit = 2 ** 31 - 1
    if not 0 <= e < n_bases or not (0 <= src <= limit and 0 <= length <= limit and 0 <= bound <= limit):
        return None
    first, end = int(edges[e]), int(edges[e + 1])
    if first < src or end <= first or end > src + length or end > set_total:
        return None
    at = bound + first - src
    if at + end - first > total:
        return None
    return first, at, end - first


def vote_host(probs, edges, labels, basemap, src, length, bounds, thresholds, max_bases=dv.MAX_BASES, ranges=None):
    """What ``cf_base_votes`` returns, in numpy: ``(sums uint64 [n_bases], state uint8 [K, n_bases], base_confusion int64 [K, 5, 2, 2],
    base_vote_runs int64 [K, 2, 3, 5, max_bases + 1])``.

    ``probs`` float32: a round's packed probabilities; stretch r is ``length[r]`` samples from sample ``src[r]`` of the set, packed at
    ``bounds[r]``.  ``edges`` is a ``BaseTable``'s, ``labels`` / ``basemap`` the set's uint8 arrays.  ``ranges`` = ``event_ranges``
    unless given.  Per voted base of ``n`` samples: ``S = sum q_of(p)`` over them; ``called_k = S >= q_of(float32(t_k)) * n`` (so a
    mean exactly at the threshold is called); ``truth = labels[edges[e]] == 1``; class = ``base_classes(basemap[edges[e]])``.
    ``state`` bit 0 called, bit 1 truth, bits 2..4 class, bit 7 voted; sums and states of a base no stretch votes are 0.
    ``base_confusion[k, class, truth, called]`` counts the voted bases.  ``base_vote_runs`` has ``run_bases_host``'s axes: a run is a
    maximal streak of consecutive voted bases of ONE stretch with truth (kind 0) or called (kind 1) set, judged against the other bit
    -- complete when it is set on every base, absent when on none, incomplete otherwise (``dv.RUN_STATES``); class 0..3 when every
    base of the run has it, else 4; bin ``min(bases, max_bases)``.  No last-sample rule on this axis.

    Tables that are not sound (the card does not trust them): a range is clamped to ``[0, n_bases]``, and a base whose samples are
    not ``src <= edges[e] < edges[e + 1] <= src + length``, inside the set and inside ``probs`` is unvoted."""
    max_bases = dv.check_max_bases(max_bases)
    probs = np.ascontiguousarray(np.asarray(probs, dtype=np.float32).reshape(-1))
    edges = np.asarray(edges, dtype=np.int64)
    labels, basemap = np.asarray(labels).reshape(-1), np.asarray(basemap).reshape(-1)
    src, length, bounds = (np.asarray(a, dtype=np.int64) for a in (src, length, bounds))
    a, b = event_ranges(edges, src, length) if ranges is None else (np.asarray(x, dtype=np.int64) for x in ranges)
    n_bases, total, set_total = int(edges.size - 1), int(probs.size), int(min(labels.size, basemap.size))
    thresholds = [float(t) for t in thresholds]
    qt = [int(v) for v in q_of(np.asarray(thresholds, dtype=np.float64).astype(np.float32))]
    k_all = len(thresholds)
    sums, state = np.zeros(n_bases, dtype=np.uint64), np.zeros((k_all, n_bases), dtype=np.uint8)
    confusion = np.zeros((k_all, len(dv.BASE_CLASSES), 2, 2), dtype=np.int64)
    runs = np.zeros((k_all, 2, 3, len(dv.BASE_CLASSES), max_bases + 1), dtype=np.int64)
    q_run = np.concatenate(([0], np.cumsum(q_of(probs), dtype=np.uint64))).astype(np.uint64)
    clamp = lambda v: min(max(int(v), 0), n_bases)          # noqa: E731
    spans = []
    for r in range(src.size):
        lo, hi = clamp(a[r]), clamp(b[r])
        mine = np.zeros(max(hi - lo, 0), dtype=bool)       # the bases of the range that THIS stretch votes
        spans.append((lo, hi, mine))
        for e in range(lo, hi):
            span = _voted_span(edges, n_bases, e, int(src[r]), int(length[r]), int(bounds[r]), total, set_total)
            if span is None:
                continue
            mine[e - lo] = True
            first, at, n = span
            s = int(q_run[at + n]) - int(q_run[at])
            sums[e] = s
            truth, cls = int(labels[first] == 1), int(base_classes(basemap[first]))
            for k in range(k_all):
                called = int(s >= qt[k] * n)
                state[k, e] = VOTED | called | (truth << 1) | (cls << 2)
    for k in range(k_all):
        for lo, hi, mine in spans:                         # (sound ranges share no base, so every voted base is counted once)
            st = np.where(mine, state[k, lo:hi], 0).astype(np.int64)
            voted, cls = (st & VOTED) != 0, (st >> 2) & 7
            np.add.at(confusion[k], (cls[voted], (st[voted] >> 1) & 1, st[voted] & 1), 1)
            for kind, (mine, other) in enumerate(((TRUTH, CALLED), (CALLED, TRUTH))):
                mask = voted & ((st & mine) != 0)
                step = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
                for s0, s1 in zip(np.flatnonzero(step == 1).tolist(), np.flatnonzero(step == -1).tolist()):
                    with_other = int(np.count_nonzero(st[s0:s1] & other))
                    run_state = 0 if with_other == s1 - s0 else (2 if with_other == 0 else 1)
                    run_cls = int(cls[s0]) if np.all(cls[s0:s1] == cls[s0]) else 4
                    runs[k, kind, run_state, run_cls, min(s1 - s0, max_bases)] += 1
    return sums, state, confusion, runs


def mean_p(sums, edges):
    """float64 [n_bases]: ``double(S[e]) / (n * 2^32)`` -- the mean probability of every base (0 where it was not voted)."""
    return np.asarray(sums, dtype=np.uint64).astype(np.float64) / (np.diff(np.asarray(edges, dtype=np.int64)) * float(ONE))


def base_vote_rates(confusion_k):
    """One threshold's [5, 2, 2] confusion table (class, truth, called) -> dict: ``base_precision`` / ``base_recall`` / ``base_f1`` over
    all voted bases and ``base_precision_by_base`` / ``base_recall_by_base`` / ``base_f1_by_base`` [5] per class of
    ``dv.BASE_CLASSES`` -- ``metrics.precision_recall`` and ``metrics.f1`` on base counts (0 for an empty denominator) -- and
    ``voted_bases``, how many bases the table holds."""
    table = np.asarray(confusion_k)
    if table.shape != (len(dv.BASE_CLASSES), 2, 2):
        raise ValueError("one threshold's base confusion table is [5, 2, 2], got %s" % (table.shape,))

    def rates(t):                                          # (the formulas of metrics.py, without its messages: empty classes are usual here)
        tp, fp, fn = int(t[1, 1]), int(t[0, 1]), int(t[1, 0])
        precision, recall = tp / (tp + fp) if tp + fp else 0, tp / (tp + fn) if tp + fn else 0
        return precision, recall, 2 * (precision * recall) / (precision + recall) if precision + recall else 0

    overall, by_base = rates(table.sum(axis=0)), [rates(t) for t in table]
    return {"voted_bases": int(table.sum()), "base_precision": overall[0], "base_recall": overall[1], "base_f1": overall[2],
            "base_precision_by_base": [r[0] for r in by_base], "base_recall_by_base": [r[1] for r in by_base],
            "base_f1_by_base": [r[2] for r in by_base]}


def calls_of(sums, state_k, table):
    """The calls in base coordinates, per read: a list of ``(first_base_in_read, n_bases, letter, mean)`` for every kind-1 run of one
    threshold's states -- a maximal streak of voted, called bases inside one read; ``letter`` is the run's base, or "N" when its bases
    differ or are not ``A C G T``; ``mean`` is the mean of the bases' ``mean_p``.  Host numpy."""
    state_k = np.asarray(state_k, dtype=np.uint8).reshape(-1)
    if state_k.size != table.n_bases or np.asarray(sums).size != table.n_bases:
        raise ValueError("calls_of: sums and state_k need one entry per base (%d)" % table.n_bases)
    mean = mean_p(sums, table.edges)
    cls = (state_k.astype(np.int64) >> 2) & 7
    out = []
    for lo, hi in zip(table.base_offsets[:-1].tolist(), table.base_offsets[1:].tolist()):
        mask = (state_k[lo:hi] & (VOTED | CALLED)) == (VOTED | CALLED)
        step = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
        calls = []
        for s0, s1 in zip(np.flatnonzero(step == 1).tolist(), np.flatnonzero(step == -1).tolist()):
            c = cls[lo + s0:lo + s1]
            letter = "ACGT"[int(c[0])] if c[0] < 4 and np.all(c == c[0]) else "N"
            calls.append((s0, s1 - s0, letter, float(np.mean(mean[lo + s0:lo + s1]))))
        out.append(calls)
    return out


def call_bases_host(probs, bases, lengths, threshold=0.5):
    """``RNN.call_bases_device`` for a model without an engine: ``probs[r]`` are read r's per-sample probabilities (float32, at least
    as many as its events cover), ``bases[r]`` / ``lengths[r]`` its event table -> the calls of ``calls_of`` over whole reads."""
    from .labelling import EventBatch
    batch = EventBatch.from_reads(list(zip(bases, lengths)))
    table = BaseTable.from_events(batch)
    if len(probs) != batch.n_reads:
        raise ValueError("%d probability arrays but %d event tables" % (len(probs), batch.n_reads))
    packed = np.zeros(batch.total, dtype=np.float32)
    for r, p in enumerate(probs):
        o, n = int(batch.sample_offsets[r]), int(batch.sample_offsets[r + 1] - batch.sample_offsets[r])
        p = np.asarray(p, dtype=np.float32).reshape(-1)
        if p.size < n:
            raise ValueError("read %d: the events cover %d samples, there are %d probabilities" % (r, n, p.size))
        packed[o:o + n] = p[:n]
    basemap = np.repeat(batch.bases, batch.lengths)
    sums, state, _confusion, _runs = vote_host(packed, table.edges, np.zeros(batch.total, np.uint8), basemap, batch.sample_offsets[:-1],
                                               np.diff(batch.sample_offsets), batch.sample_offsets[:-1], (threshold,), 1)
    return calls_of(sums, state[0], table)


# ---------------------------------------------------------------------------------------------------------------------- the card's side
def launch(lib, handle, probs, total, labels, basemap, edges, n_bases, src_first, length, bounds, ranges, longest_range, thresholds,
           max_bases, confusion_out, runs_out, work, stream):
    """``cf_base_votes`` on CUDA tensors that the caller has checked (``HipEngine.base_votes_validation`` and ``vote_device`` do)."""
    import ctypes as C
    from . import _native as N
    from ._native import _p as p
    thresholds = [float(t) for t in thresholds]
    k = len(thresholds)
    N.check(lib.cf_base_votes(handle, p(probs), int(total), p(labels), p(basemap), int(min(labels.numel(), basemap.numel())), p(edges),
                              int(n_bases), p(src_first), p(length), p(bounds), p(ranges), int(src_first.numel()), int(longest_range),
                              (C.c_double * max(k, 1))(*thresholds), k, int(max_bases), p(confusion_out), p(runs_out), p(work),
                              int(work.numel()), N.stream_ptr(stream)))


def work_bytes(n_bases, n_thresholds):
    """Bytes of ``cf_base_votes``' work buffer: uint64 sums [n_bases] | uint8 state [K, n_bases], rounded up to 16, never 0."""
    return max((8 + int(n_thresholds)) * int(n_bases), 1) + 15 & ~15


def vote_device(probs, vset, selection, thresholds, max_bases=dv.MAX_BASES, window=35):
    """The stand-alone op: ``vote_host`` on the card.  ``probs`` is a float32 CUDA tensor with a round's packed probabilities (stretch
    r at ``dv.layout(length, window)[0][r]``), ``vset`` a ``DeviceValidationSet`` with a base table (``from_events`` /
    ``from_moves``), ``selection`` its ``(read_index, first, length)`` -> ``(sums uint64-as-int64 [n_bases], state uint8 [K, n_bases],
    base_confusion int64 [K, 5, 2, 2], base_vote_runs int64 [K, 2, 3, 5, max_bases + 1])`` as CUDA tensors (the sums' int64 cells hold
    the uint64 bits; none reaches 2^63).  More than 16 thresholds go in groups of 16.  Asynchronous on torch's current stream."""
    import torch
    from . import _native as N
    max_bases = dv.check_max_bases(max_bases)
    thresholds = tuple(float(t) for t in thresholds)
    if not thresholds:
        raise ValueError("vote_device: no threshold given")
    table = vset.base_table("vote_device")
    if not isinstance(probs, torch.Tensor) or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous():
        raise ValueError("vote_device: probs must be a contiguous float32 CUDA tensor")
    read_index, first, length = vset.check_selection(selection)
    bounds, _tails = dv.layout(length, window)
    if int(probs.numel()) < int(bounds[-1]):
        raise ValueError("vote_device: probs needs %d elements" % int(bounds[-1]))
    device, n, k_all, n_bases = probs.device, int(length.size), len(thresholds), table.n_bases
    _signal, labels = vset.device_arrays(device)
    basemap, edges = vset.device_basemap(device), vset.device_edges(device)
    src = vset.offsets[read_index] + first
    a, b = event_ranges(table.edges, src, length)
    host = np.concatenate((src, length, bounds, a, b)).astype(np.int64)
    tab = torch.from_numpy(host).to(device)
    src_d, len_d, bounds_d, ranges_d = tab[:n], tab[n:2 * n], tab[2 * n:3 * n + 1], tab[3 * n + 1:]
    run_cells = 2 * 3 * len(dv.BASE_CLASSES) * (max_bases + 1)
    sums = torch.zeros(max(n_bases, 1), dtype=torch.int64, device=device)
    state = torch.zeros((k_all, n_bases), dtype=torch.uint8, device=device)
    confusion = torch.zeros(k_all * CONFUSION_CELLS, dtype=torch.int64, device=device)
    runs = torch.zeros(k_all * run_cells, dtype=torch.int64, device=device)
    stream = torch.cuda.current_stream(device)
    for k0 in range(0, k_all, MAX_THRESHOLDS):
        k1 = min(k_all, k0 + MAX_THRESHOLDS)
        work = torch.empty(work_bytes(n_bases, k1 - k0) // 8, dtype=torch.int64, device=device).view(torch.uint8)
        launch(N.lib(), None, probs, int(bounds[-1]), labels, basemap, edges, n_bases, src_d, len_d, bounds_d, ranges_d,
               int((b - a).max()) if n else 0, thresholds[k0:k1], max_bases, confusion[CONFUSION_CELLS * k0:], runs[run_cells * k0:], work, stream)
        if n_bases:
            sums[:n_bases].copy_(work[:8 * n_bases].view(torch.int64))
            state[k0:k1].copy_(work[8 * n_bases:(8 + k1 - k0) * n_bases].view(k1 - k0, n_bases))
    return (sums[:n_bases], state, confusion.view(k_all, len(dv.BASE_CLASSES), 2, 2),
            runs.view(k_all, 2, 3, len(dv.BASE_CLASSES), max_bases + 1))
