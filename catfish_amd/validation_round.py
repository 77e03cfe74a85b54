"""One validation round on the card, stated on the host: what was asked for (``RoundSpec``), the sizes and the layout of the one
result buffer that follow from it (``RoundPlan``), the results by name (``RoundResult``), and the two device steps
``RNN.score_validation_device`` is made of -- the grow-only buffers (``grow``) and the launch walk (``walk``).

Spec, plan and result are ints and numpy only and usable without a GPU; torch is imported inside ``grow`` and ``walk``.  The numpy
statements of what every launch computes stay in ``device_validation``."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import base_votes
from . import device_validation as dv
from .calling import CallRule
from .tilings import tiling_size

RESULTS = ("right", "ce_sum", "counts", "run_states", "run_borders", "curve")     # the order in the result buffer and in the tuple
EXTRA_RESULTS = ("run_bases",)          # ... and after them, with keys in ``offset`` / ``cells`` / ``need`` only when asked for
VOTE_RESULTS = base_votes.VOTE_RESULTS  # ... then the two per-base tables of ``vote_bases``, under the same rule
SCORE_RESULTS = ("run_scores",)         # ... and last the scores under runs of ``score_shift``, under the same rule


class RoundSpec(namedtuple("RoundSpec", "thresholds run_edges border_reach curve_shift rule max_bases vote_bases score_shift",
                           defaults=(None, None, None))):
    """The options of a round, checked: ``thresholds`` (a tuple of floats, at least one), ``run_edges`` / ``border_reach`` /
    ``curve_shift`` / ``max_bases`` / ``vote_bases`` / ``score_shift`` (None: that result is not asked for; ``vote_bases`` is the
    ``max_bases`` of the per-base vote-run table, ``score_shift`` the bin shift of the scores under runs) and the ``calling.CallRule`` that carries ``bridge_gap`` (``max_gap``), ``phases`` and ``vote_weight``.
    Build one with ``RoundSpec.of``."""
    __slots__ = ()

    @classmethod
    def of(cls, thresholds=(0.5,), run_edges=None, border_reach=None, curve_shift=None, bridge_gap=0, phases=(0,), vote_weight="mean",
           max_bases=None, vote_bases=None, score_shift=None):
        """The checked spec, or the ValueError of the first of ``CallRule.of``, the thresholds, ``check_run_edges``, ``curve_bins``,
        ``check_border_reach``, ``check_max_bases``, ``base_votes.check_vote_bases``, ``check_score_shift`` that refuses."""
        rule = CallRule.of(max_gap=bridge_gap, phases=phases, vote_weight=vote_weight)
        thresholds = tuple(float(t) for t in thresholds)
        if not thresholds:
            raise ValueError("score_validation_device: no threshold given")
        if run_edges is not None:
            run_edges = dv.check_run_edges(run_edges)
        if curve_shift is not None:
            dv.curve_bins(curve_shift)
            curve_shift = int(curve_shift)
        if border_reach is not None:
            border_reach = dv.check_border_reach(border_reach)
        if max_bases is not None:
            max_bases = dv.check_max_bases(max_bases)
        if vote_bases is not None:
            vote_bases = base_votes.check_vote_bases(vote_bases)
        if score_shift is not None:
            score_shift = dv.check_score_shift(score_shift)
        return cls(thresholds, run_edges, border_reach, curve_shift, rule, max_bases, vote_bases, score_shift)

    @property
    def k_all(self):
        return len(self.thresholds)

    @property
    def groups(self):
        """``(k0, k1)`` of every launch group: at most ``MAX_THRESHOLDS`` thresholds each, over the same forward pass."""
        return [(k0, min(self.k_all, k0 + dv.MAX_THRESHOLDS)) for k0 in range(0, self.k_all, dv.MAX_THRESHOLDS)]


class RoundResult(tuple):
    """What ``RNN.score_validation_device`` returns: the tuple ``(right, ce_sum, counts[, run_states][, run_borders][, curve]
    [, run_bases][, base_confusion, base_vote_runs][, run_scores])`` -- only the results asked for, in that order -- with every result as an
    attribute of that name too (None when not asked for)."""

    def __new__(cls, right, ce_sum, counts, run_states=None, run_borders=None, curve=None, run_bases=None, base_confusion=None,
                base_vote_runs=None, run_scores=None):
        fields = (right, ce_sum, counts, run_states, run_borders, curve, run_bases, base_confusion, base_vote_runs, run_scores)
        self = super().__new__(cls, (item for item in fields if item is not None))
        for name, item in zip(RESULTS + EXTRA_RESULTS + VOTE_RESULTS + SCORE_RESULTS, fields):
            setattr(self, name, item)
        return self


class RoundPlan(object):
    """Sizes and layout of one round of ``spec`` over stretches of ``length`` samples packed at ``window``: ``n``, ``bounds``,
    ``tails`` (``device_validation.layout``), ``total``, ``longest``; ``need``, the capacity every grow-only buffer must have (a key
    is there only when its result is asked for); ``run_work``, the bytes of corrected labels one threshold group writes
    (``cf_validation_run_work_bytes`` = ``cf_validation_run_borders_work_bytes``, never below 1); and the one int64 result buffer:
    ``cells[name]`` cells from ``offset[name]`` for every name of ``RESULTS`` (0 cells for a result not asked for), then those of
    ``EXTRA_RESULTS`` that are asked for (``run_bases``: ``k_all * 2 * 3 * 5 * (max_bases + 1)`` cells after the curve,
    ``need["base_cells"]``; a round that does not ask has no such key anywhere), then those of ``VOTE_RESULTS`` under the same rule
    (``base_confusion``: ``k_all * 20`` cells, ``base_vote_runs``: ``k_all * 2 * 3 * 5 * (vote_bases + 1)``; ``need["vote_cells"]`` is
    their sum and ``need["vote_work"]`` the bytes of per-base sums and states one threshold group writes, for the set's ``n_bases``),
    then those of ``SCORE_RESULTS`` (``run_scores``: ``k_all * score_cells(score_shift)`` cells, ``need["score_cells"]``; such a round
    paints behind its labels, so its ``run_work`` and ``need["run_work"]`` are ``cf_validation_run_scores_work_bytes``, twice the
    labels), ``out_cells`` in all."""

    def __init__(self, spec, length, window, n_bases=None):
        self.spec = spec
        self.length = np.asarray(length, dtype=np.int64)
        self.n = n = int(self.length.size)
        self.bounds, self.tails = dv.layout(self.length, window)
        self.total = total = int(self.bounds[-1])
        self.longest = int(np.diff(self.bounds).max())
        k_all = spec.k_all
        self.run_work = max(min(k_all, dv.MAX_THRESHOLDS) * ((total + 63) // 64 * 64), 1)
        self.cells = {"right": n, "ce_sum": n, "counts": 4 * k_all,
                      "run_states": 0 if spec.run_edges is None else k_all * 2 * (len(spec.run_edges) + 1) * 3,
                      "run_borders": 0 if spec.border_reach is None else k_all * 2 * dv.border_cells(spec.border_reach),
                      "curve": 0 if spec.curve_shift is None else 3 * dv.curve_bins(spec.curve_shift)}
        self.offset, self.out_cells = {}, 0
        for name in RESULTS:
            self.offset[name] = self.out_cells
            self.out_cells += self.cells[name]
        if spec.max_bases is not None:
            self.cells["run_bases"] = k_all * 2 * 3 * len(dv.BASE_CLASSES) * (spec.max_bases + 1)
            self.offset["run_bases"] = self.out_cells
            self.out_cells += self.cells["run_bases"]
        if spec.vote_bases is not None:
            if n_bases is None:
                raise ValueError("RoundPlan: a round with vote_bases needs the set's n_bases")
            for name, per_k in zip(VOTE_RESULTS, (base_votes.CONFUSION_CELLS, 2 * 3 * len(dv.BASE_CLASSES) * (spec.vote_bases + 1))):
                self.cells[name] = k_all * per_k
                self.offset[name] = self.out_cells
                self.out_cells += self.cells[name]
        if spec.score_shift is not None:
            self.run_work = 2 * self.run_work
            self.cells["run_scores"] = k_all * dv.score_cells(spec.score_shift)
            self.offset["run_scores"] = self.out_cells
            self.out_cells += self.cells["run_scores"]
        self.need = {"samples": max(total, 1), "reads": n, "slots": total // dv.SCORE_CHUNK + n, "thresholds": k_all}
        if spec.run_edges is not None:
            self.need.update({"run_cells": self.cells["run_states"], "run_work": self.run_work})
        if spec.border_reach is not None:
            self.need.update({"border_cells": self.cells["run_borders"], "run_work": self.run_work})
        if spec.curve_shift is not None:
            self.need["curve_cells"] = self.cells["curve"]
        if spec.max_bases is not None:
            self.need.update({"base_cells": self.cells["run_bases"], "run_work": self.run_work})
        if spec.vote_bases is not None:
            self.need.update({"vote_cells": sum(self.cells[name] for name in VOTE_RESULTS),
                              "vote_work": base_votes.work_bytes(n_bases, min(k_all, dv.MAX_THRESHOLDS))})
        if spec.score_shift is not None:
            self.need.update({"score_cells": self.cells["run_scores"], "run_work": self.run_work})
        if spec.rule.voted:
            self.need["tiling_samples"] = tiling_size(total, n, spec.rule.n_tilings)

    def cut(self, buffer, name):
        """The cells of result ``name`` in a result buffer (a host array or a device tensor of at least ``out_cells`` elements)."""
        return buffer[self.offset[name]:self.offset[name] + self.cells[name]]

    def table(self, set_offsets, read_index, first):
        """The int64 [3, n + 1] selection table a round uploads: where every stretch starts in the set's arrays | its length |
        ``bounds`` (the first two rows have n entries and a zero after them)."""
        table = np.zeros((3, self.n + 1), dtype=np.int64)
        table[0, :self.n] = np.asarray(set_offsets)[read_index] + first
        table[1, :self.n] = self.length
        table[2] = self.bounds
        return table

    def results(self, back):
        """The copied-back result buffer (host int64, ``out_cells`` elements) -> ``RoundResult``: right int64 [n], ce_sum float64 [n]
        (the cells hold the doubles' bits), counts int64 [K, 4], run states int64 [K, 2, len(run_edges) + 1, 3], borders int64
        [K, 2, 5 * border_reach + 3], curve histogram int64 [3, curve_bins(curve_shift)], run bases int64
        [K, 2, 3, 5, max_bases + 1], base confusion int64 [K, 5, 2, 2], base vote runs int64 [K, 2, 3, 5, vote_bases + 1], run scores
        int64 [K, 2, 3, curve_bins(score_shift) + 1]; every item its own copy."""
        spec, k_all = self.spec, self.spec.k_all
        return RoundResult(
            self.cut(back, "right").copy(), self.cut(back, "ce_sum").view(np.float64).copy(),
            self.cut(back, "counts").reshape(k_all, 4).copy(),
            None if spec.run_edges is None else self.cut(back, "run_states").reshape(k_all, 2, len(spec.run_edges) + 1, 3).copy(),
            None if spec.border_reach is None else self.cut(back, "run_borders").reshape(k_all, 2, -1).copy(),
            None if spec.curve_shift is None else self.cut(back, "curve").reshape(3, -1).copy(),
            None if spec.max_bases is None else
            self.cut(back, "run_bases").reshape(k_all, 2, 3, len(dv.BASE_CLASSES), spec.max_bases + 1).copy(),
            None if spec.vote_bases is None else self.cut(back, "base_confusion").reshape(k_all, len(dv.BASE_CLASSES), 2, 2).copy(),
            None if spec.vote_bases is None else
            self.cut(back, "base_vote_runs").reshape(k_all, 2, 3, len(dv.BASE_CLASSES), spec.vote_bases + 1).copy(),
            None if spec.score_shift is None else self.cut(back, "run_scores").reshape(k_all, 2, 3, -1).copy())


def grow(book, need, device):
    """The grow-only rule of ``RNN.validation_buffers``: when any capacity of ``need`` exceeds ``book["capacity"]`` every tensor is
    allocated again at the larger of the two (``book["allocations"]`` counts how often); -> ``book["tensors"]``."""
    import torch
    have = book["capacity"]
    if any(have.get(key, 0) < value for key, value in need.items()):
        cap = {key: max(have.get(key, 0), value) for key, value in need.items()}
        f32 = lambda count: torch.empty(count, dtype=torch.float32, device=device)     # noqa: E731
        book["tensors"] = {"x": f32(cap["samples"]), "probs": f32(cap["samples"]), "logits": f32(cap["samples"]),
                           "y": torch.empty(cap["samples"], dtype=torch.uint8, device=device),
                           "table": torch.empty(3 * (cap["reads"] + 1), dtype=torch.int64, device=device),
                           "partials": torch.empty(cap["slots"], dtype=torch.float64, device=device),
                           # right [reads] | ce_sum [reads], double bits | counts [4 per threshold] | run states | borders |
                           # curve histogram | run bases | base confusion | base vote runs | run scores: one copy back
                           "out": torch.empty(2 * cap["reads"] + 4 * cap["thresholds"] + cap.get("run_cells", 0)
                                              + cap.get("border_cells", 0) + cap.get("curve_cells", 0) + cap.get("base_cells", 0)
                                              + cap.get("vote_cells", 0) + cap.get("score_cells", 0), dtype=torch.int64, device=device)}
        if "run_work" in cap:                                     # corrected labels (and paint), one array per threshold of a group
            book["tensors"]["run_work"] = torch.empty(cap["run_work"], dtype=torch.uint8, device=device)
        if "vote_work" in cap:                                                   # per-base sums and states (8-byte aligned), and every
            book["tensors"]["vote_work"] = torch.empty(cap["vote_work"] // 8, dtype=torch.int64, device=device).view(torch.uint8)
            book["tensors"]["vote_ranges"] = torch.empty(2 * cap["reads"], dtype=torch.int64, device=device)     # stretch's base range
        if "tiling_samples" in cap:                                              # every tiling's input, probabilities and logits
            book["tensors"].update({key: f32(cap["tiling_samples"]) for key in ("tilings_x", "tilings_probs", "tilings_logits")})
        book["capacity"] = cap
        book["allocations"] += 1
    return book["tensors"]


def walk(engine, plan, t, thresholds_d, signal, labels, window, basemap=None, edges=None, longest_range=0):
    """Every launch of a round, on the current stream, over the buffers ``t`` (``grow``) with the selection table uploaded: gather,
    (retile,) forward pass, (vote,) then per threshold group score, run states, borders, run bases, base votes, run scores, and the
    curve histogram last.  ``thresholds_d``: the thresholds as a float64 CUDA tensor; ``basemap``: the set's base map on the card, which a
    round with ``max_bases`` or ``vote_bases`` reads in place; ``edges``: the set's base table on the card and ``longest_range`` the
    widest stretch in bases, for a round with ``vote_bases`` (its ranges are in ``t["vote_ranges"]`` already).  -> the result
    buffer's ``plan.out_cells`` cells, still on the card."""
    import torch
    spec, rule, n, total, longest = plan.spec, plan.spec.rule, plan.n, plan.total, plan.longest
    src_d, len_d, bounds_d = (t["table"][i * (n + 1):i * (n + 1) + count] for i, count in ((0, n), (1, n), (2, n + 1)))
    x, y, probs, logits = t["x"][:total], t["y"][:total], t["probs"][:total], t["logits"][:total]
    out = t["out"][:plan.out_cells]
    right_d, ce_d, counts_d = plan.cut(out, "right"), plan.cut(out, "ce_sum").view(torch.float64), plan.cut(out, "counts")
    runs_d, borders_d, curve_d = plan.cut(out, "run_states"), plan.cut(out, "run_borders"), plan.cut(out, "curve")
    if rule.voted:
        size = plan.need["tiling_samples"]
        x_all, probs_all, logits_all = t["tilings_x"][:size], t["tilings_probs"][:size], t["tilings_logits"][:size]
        engine.gather_validation(signal, labels, src_d, len_d, bounds_d, total, longest, x_all[:total], y)
        engine.retile_device(x_all, bounds_d, len_d, total, rule.phases)
        engine.infer_device(x_all.view(-1, window), out=probs_all, logits=logits_all)
        engine.vote_device(probs_all, bounds_d, len_d, total, rule.phases, rule.vote_weight, logits_all=logits_all, out=probs, logits_out=logits)
    else:
        engine.gather_validation(signal, labels, src_d, len_d, bounds_d, total, longest, x, y)
        engine.infer_device(x.view(-1, window), out=probs, logits=logits)
    run_per_k, border_per_k = plan.cells["run_states"] // spec.k_all, plan.cells["run_borders"] // spec.k_all
    if spec.max_bases is not None:
        bases_d, base_per_k = plan.cut(out, "run_bases"), plan.cells["run_bases"] // spec.k_all
    if spec.vote_bases is not None:
        confusion_d, vote_runs_d = plan.cut(out, "base_confusion"), plan.cut(out, "base_vote_runs")
        confusion_per_k, vote_per_k = plan.cells["base_confusion"] // spec.k_all, plan.cells["base_vote_runs"] // spec.k_all
    if spec.score_shift is not None:
        scores_d, score_per_k = plan.cut(out, "run_scores"), plan.cells["run_scores"] // spec.k_all
    for k0, k1 in spec.groups:
        engine.score_validation(probs, logits, y, bounds_d, total, longest, thresholds_d[k0:k1], right_d, ce_d, counts_d[4 * k0:4 * k1],
                                t["partials"])
        if spec.run_edges is not None:
            engine.run_states_validation(probs, y, bounds_d, len_d, total, longest, spec.thresholds[k0:k1], spec.run_edges,
                                         runs_d[run_per_k * k0:run_per_k * k1], t["run_work"], min_run=rule.min_run, max_gap=rule.max_gap)
        if spec.border_reach is not None:
            engine.run_borders_validation(probs, y, bounds_d, len_d, total, longest, spec.thresholds[k0:k1], spec.border_reach,
                                          borders_d[border_per_k * k0:border_per_k * k1], t["run_work"], min_run=rule.min_run, max_gap=rule.max_gap)
        if spec.max_bases is not None:
            engine.run_bases_validation(probs, y, basemap, src_d, bounds_d, len_d, total, longest, spec.thresholds[k0:k1], spec.max_bases,
                                        bases_d[base_per_k * k0:base_per_k * k1], t["run_work"], min_run=rule.min_run, max_gap=rule.max_gap)
        if spec.vote_bases is not None:
            engine.base_votes_validation(probs, labels, basemap, edges, src_d, bounds_d, len_d, t["vote_ranges"][:2 * n], total, longest_range,
                                         spec.thresholds[k0:k1], spec.vote_bases, confusion_d[confusion_per_k * k0:confusion_per_k * k1],
                                         vote_runs_d[vote_per_k * k0:vote_per_k * k1], t["vote_work"])
        if spec.score_shift is not None:
            engine.run_scores_validation(probs, y, bounds_d, len_d, total, longest, spec.thresholds[k0:k1], spec.score_shift,
                                         scores_d[score_per_k * k0:score_per_k * k1], t["run_work"], min_run=rule.min_run, max_gap=rule.max_gap)
    if spec.curve_shift is not None:
        engine.curve_validation(probs, y, bounds_d, len_d, total, longest, spec.curve_shift, curve_d)
    return out
