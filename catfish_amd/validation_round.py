"""One validation round on the card, stated on the host: what was asked for (``RoundSpec``), the sizes and the layout of the one
result buffer that follow from it (``RoundPlan``), the results by name (``RoundResult``), and the two device steps
``RNN.score_validation_device`` is made of -- the grow-only buffers (``grow``) and the launch walk (``walk``).

Spec, plan and result are ints and numpy only and usable without a GPU; torch is imported inside ``grow`` and ``walk``.  The numpy
statements of what every launch computes stay in ``device_validation``."""
from __future__ import annotations

import math
from collections import namedtuple
from operator import attrgetter

import numpy as np

from . import base_votes
from . import device_validation as dv
from .calling import CallRule
from .tilings import tiling_size


# ------------------------------------------------------------------ what the rows of ``OPTIONS`` below name: checks and launches
def _checked_curve_shift(shift):
    dv.curve_bins(shift)
    return int(shift)


def _needs_binary_labels(vset):
    if not vset.labels_binary:
        raise ValueError("score_validation_device: border_reach needs a set whose labels are all 0 or 1")


def _needs_base_map(vset):
    if vset.basemap is None:
        raise ValueError("score_validation_device: max_bases needs a set with a base map (DeviceValidationSet.from_events)")


def _needs_base_table(vset):
    vset.base_table("score_validation_device: vote_bases")


def _run_step(method):
    """The launch of a step that corrects the thresholded prediction in the label work space and counts its runs."""
    def launch(engine, plan, on, thresholds, value, outs):
        rule = plan.spec.rule
        getattr(engine, method)(on.probs, on.y, on.bounds, on.length, plan.total, plan.longest, thresholds, value, outs[0], on.t["run_work"],
                                min_run=rule.min_run, max_gap=rule.max_gap)
    return launch


def _run_bases(engine, plan, on, thresholds, value, outs):
    rule = plan.spec.rule
    engine.run_bases_validation(on.probs, on.y, on.basemap, on.src, on.bounds, on.length, plan.total, plan.longest, thresholds, value, outs[0],
                                on.t["run_work"], min_run=rule.min_run, max_gap=rule.max_gap)


def _base_votes(engine, plan, on, thresholds, value, outs):
    engine.base_votes_validation(on.probs, on.labels, on.basemap, on.edges, on.src, on.bounds, on.length, on.t["vote_ranges"][:2 * plan.n],
                                 plan.total, on.longest_range, thresholds, value, outs[0], outs[1], on.t["vote_work"])


def _curve(engine, plan, on, thresholds, value, outs):
    engine.curve_validation(on.probs, on.y, on.bounds, on.length, plan.total, plan.longest, value, outs[0])


class Option(namedtuple("Option", "option check results need_key launch run_work bridged per_threshold listed work needs basemap",
                        defaults=(True, False, None, None, False))):
    """One optional result of a round (two for ``vote_bases``), stated once:

    ``option``         the ``RoundSpec`` field and keyword; None there: not asked for
    ``check``          value -> the checked value, or ValueError
    ``results``        ``(name, shape)`` per result, ``shape(value)`` being one threshold's (the whole result's when not
                       ``per_threshold``); its cells in the result buffer are the product of the shape, per threshold
    ``need_key``       where ``RoundPlan.need`` states the cells of all its results
    ``launch``         ``(engine, plan, on, thresholds of the group, value, the group's cells of every result)``: its ``HipEngine`` call
    ``run_work``       label-sized arrays it uses per threshold of a group in the shared work space ``run_work``: 0 none, 1 the corrected
                       labels, 2 labels and paint behind them; the round's work space is the largest of these
    ``bridged``        ``bridge_gap`` changes it
    ``per_threshold``  launched once per threshold group after ``score_validation``, a leading K axis; otherwise once after the groups
    ``listed``         history, pinned by the host tests: the results that existed when ``RoundPlan`` was written have their ``offset`` and
                       ``cells`` keys (0 cells) in a round that does not ask for them; the later ones have no key then
    ``work``           ``(need key, bytes(n_bases, thresholds of a group))`` of a work space of its own that depends on the set's bases
    ``needs``          vset -> ValueError when the set lacks what the result is counted from
    ``basemap``        reads the set's base map on the card"""
    __slots__ = ()

    @property
    def names(self):
        return tuple(name for name, _shape in self.results)

    def shapes(self, value, k_all):
        """``[(name, shape)]`` of its results in a round of ``k_all`` thresholds."""
        lead = (k_all,) if self.per_threshold else ()
        return [(name, lead + tuple(shape(value))) for name, shape in self.results]


_BASES = len(dv.BASE_CLASSES)
OPTIONS = (                                                         # in the order of the result buffer
    Option("run_edges", dv.check_run_edges, (("run_states", lambda edges: (2, len(edges) + 1, 3)),), "run_cells",
           _run_step("run_states_validation"), run_work=1, bridged=True, listed=True),
    Option("border_reach", dv.check_border_reach, (("run_borders", lambda reach: (2, dv.border_cells(reach))),), "border_cells",
           _run_step("run_borders_validation"), run_work=1, bridged=True, listed=True, needs=_needs_binary_labels),
    Option("curve_shift", _checked_curve_shift, (("curve", lambda shift: (3, dv.curve_bins(shift))),), "curve_cells",
           _curve, run_work=0, bridged=False, per_threshold=False, listed=True),
    Option("max_bases", dv.check_max_bases, (("run_bases", lambda most: (2, 3, _BASES, most + 1)),), "base_cells",
           _run_bases, run_work=1, bridged=True, needs=_needs_base_map, basemap=True),
    Option("vote_bases", base_votes.check_vote_bases,
           (("base_confusion", lambda most: (_BASES, 2, 2)), ("base_vote_runs", lambda most: (2, 3, _BASES, most + 1))), "vote_cells",
           _base_votes, run_work=0, bridged=False, work=("vote_work", base_votes.work_bytes), needs=_needs_base_table, basemap=True),
    Option("score_shift", dv.check_score_shift, (("run_scores", lambda shift: (2, 3, dv.curve_bins(shift) + 1)),), "score_cells",
           _run_step("run_scores_validation"), run_work=2, bridged=True))
# history: the curve was the second option to exist, so its check still refuses before the borders' when both values are wrong
CHECK_ORDER = tuple(sorted(OPTIONS, key=lambda row: row.option not in ("run_edges", "curve_shift")))

FIXED_RESULTS = ("right", "ce_sum", "counts")
# the tiers the results were added in; all of them, in the order of the result buffer and of the tuple, are ``ALL_RESULTS``
RESULTS = FIXED_RESULTS + tuple(name for row in OPTIONS if row.listed for name in row.names)
EXTRA_RESULTS, VOTE_RESULTS, SCORE_RESULTS = (row.names for row in OPTIONS if not row.listed)
ALL_RESULTS = FIXED_RESULTS + tuple(name for row in OPTIONS for name in row.names)
assert VOTE_RESULTS == base_votes.VOTE_RESULTS and base_votes.CONFUSION_CELLS == _BASES * 2 * 2


class RoundSpec(namedtuple("RoundSpec", "thresholds run_edges border_reach curve_shift rule max_bases vote_bases score_shift",
                           defaults=(None, None, None))):
    """The options of a round, checked: ``thresholds`` (a tuple of floats, at least one), one field per row of ``OPTIONS`` (None: that
    result is not asked for) and the ``calling.CallRule`` that carries ``bridge_gap`` (``max_gap``), ``phases`` and ``vote_weight``.
    Build one with ``RoundSpec.of``."""
    __slots__ = ()

    @classmethod
    def of(cls, thresholds=(0.5,), run_edges=None, border_reach=None, curve_shift=None, bridge_gap=0, phases=(0,), vote_weight="mean",
           max_bases=None, vote_bases=None, score_shift=None):
        """The checked spec, or the ValueError of the first of ``CallRule.of``, the thresholds, ``check_run_edges``, ``curve_bins``,
        ``check_border_reach``, ``check_max_bases``, ``base_votes.check_vote_bases``, ``check_score_shift`` that refuses."""
        given = dict(run_edges=run_edges, border_reach=border_reach, curve_shift=curve_shift, max_bases=max_bases, vote_bases=vote_bases,
                     score_shift=score_shift)
        rule = CallRule.of(max_gap=bridge_gap, phases=phases, vote_weight=vote_weight)
        thresholds = tuple(float(t) for t in thresholds)
        if not thresholds:
            raise ValueError("score_validation_device: no threshold given")
        for row in CHECK_ORDER:
            if given[row.option] is not None:
                given[row.option] = row.check(given[row.option])
        return cls(thresholds=thresholds, rule=rule, **given)

    @property
    def k_all(self):
        return len(self.thresholds)

    @property
    def groups(self):
        """``(k0, k1)`` of every launch group: at most ``MAX_THRESHOLDS`` thresholds each, over the same forward pass."""
        return [(k0, min(self.k_all, k0 + dv.MAX_THRESHOLDS)) for k0 in range(0, self.k_all, dv.MAX_THRESHOLDS)]

    @property
    def rows(self):
        """``(row, value)`` for every row of ``OPTIONS``, the value None where the option is not asked for."""
        return zip(OPTIONS, _VALUES(self))

    @property
    def asked(self):
        """``[(row, value)]`` of the options asked for, in the order of ``OPTIONS``."""
        return [(row, value) for row, value in zip(OPTIONS, _VALUES(self)) if value is not None]


_VALUES = attrgetter(*(row.option for row in OPTIONS))


class RoundResult(tuple):
    """What ``RNN.score_validation_device`` returns: the tuple ``(right, ce_sum, counts[, run_states][, run_borders][, curve]
    [, run_bases][, base_confusion, base_vote_runs][, run_scores])`` -- only the results asked for, in the order of ``ALL_RESULTS`` -- with
    every result as an attribute of that name too (None when not asked for)."""

    def __new__(cls, right, ce_sum, counts, *optional, **named):
        named.update(zip(ALL_RESULTS[3:], optional))
        fields = (right, ce_sum, counts) + tuple(named.pop(name, None) for name in ALL_RESULTS[3:])
        if named:
            raise TypeError("RoundResult has no result %s" % ", ".join(sorted(named)))
        self = super().__new__(cls, (item for item in fields if item is not None))
        for name, item in zip(ALL_RESULTS, fields):
            setattr(self, name, item)
        return self


class RoundPlan(object):
    """Sizes and layout of one round of ``spec`` over stretches of ``length`` samples packed at ``window``: ``n``, ``bounds``,
    ``tails`` (``device_validation.layout``), ``total``, ``longest``; ``need``, the capacity every grow-only buffer must have;
    ``run_work``, the bytes of the label work space one threshold group writes; and the one int64 result buffer of ``out_cells``
    cells: ``cells[name]`` cells from ``offset[name]``, the three fixed results first and then, row by row of ``OPTIONS``, the results
    asked for -- ``k_all`` times the product of the row's shape (the curve: once).

    ``need``: ``samples``, ``reads``, ``slots``, ``thresholds`` always; per row asked for its ``need_key`` (the cells of its results),
    ``run_work`` when it uses the label work space, and its own ``work`` entry (``vote_work``: the per-base sums and states one group
    writes, for the set's ``n_bases``); ``tiling_samples`` for a voted round.  A key is there only when something asks for it.
    ``run_work``: ``min(k_all, 16)`` label arrays of ``total`` rounded up to 64 (``cf_validation_run_work_bytes`` =
    ``cf_validation_run_borders_work_bytes``, never below 1), twice that in a round with the scores, which paint behind their labels
    (``cf_validation_run_scores_work_bytes``).  A ``listed`` row that is not asked for keeps its keys in ``cells`` (0) and ``offset``."""

    def __init__(self, spec, length, window, n_bases=None):
        self.spec = spec
        self.length = np.asarray(length, dtype=np.int64)
        self.n = n = int(self.length.size)
        self.bounds, self.tails = dv.layout(self.length, window)
        self.total = total = int(self.bounds[-1])
        self.longest = int(np.diff(self.bounds).max())
        k_all, k_group = spec.k_all, min(spec.k_all, dv.MAX_THRESHOLDS)
        self.run_work = max(k_group * ((total + 63) // 64 * 64), 1) * max([1] + [row.run_work for row, _value in spec.asked])
        self.cells = {"right": n, "ce_sum": n, "counts": 4 * k_all}
        self.need = {"samples": max(total, 1), "reads": n, "slots": total // dv.SCORE_CHUNK + n, "thresholds": k_all}
        for row, value in spec.rows:
            if value is None:
                if row.listed:
                    self.cells.update(dict.fromkeys(row.names, 0))
                continue
            self.cells.update((name, math.prod(shape)) for name, shape in row.shapes(value, k_all))
            self.need[row.need_key] = sum(self.cells[name] for name in row.names)
            if row.run_work:
                self.need["run_work"] = self.run_work
            if row.work:
                if n_bases is None:
                    raise ValueError("RoundPlan: a round with %s needs the set's n_bases" % row.option)
                self.need[row.work[0]] = row.work[1](n_bases, k_group)
        self.offset, self.out_cells = {}, 0
        for name, cells in self.cells.items():
            self.offset[name] = self.out_cells
            self.out_cells += cells
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
        (the cells hold the doubles' bits), counts int64 [K, 4], and every result asked for as int64 of its row's ``Option.shapes``;
        every item its own copy."""
        k_all = self.spec.k_all
        return RoundResult(self.cut(back, "right").copy(), self.cut(back, "ce_sum").view(np.float64).copy(),
                           self.cut(back, "counts").reshape(k_all, 4).copy(),
                           **{name: self.cut(back, name).reshape(shape).copy()
                              for row, value in self.spec.asked for name, shape in row.shapes(value, k_all)})


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
                           # right [reads] | ce_sum [reads], double bits | counts [4 per threshold] | the cells of every row of
                           # ``OPTIONS`` that a round has asked for: one copy back
                           "out": torch.empty(2 * cap["reads"] + 4 * cap["thresholds"] + sum(cap.get(row.need_key, 0) for row in OPTIONS),
                                              dtype=torch.int64, device=device)}
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


Round = namedtuple("Round", "t probs y labels basemap edges src bounds length longest_range")      # what the rows' launches read


def walk(engine, plan, t, thresholds_d, signal, labels, window, basemap=None, edges=None, longest_range=0):
    """Every launch of a round, on the current stream, over the buffers ``t`` (``grow``) with the selection table uploaded: gather,
    (retile,) forward pass, (vote,) then per threshold group ``score_validation`` and the ``per_threshold`` rows of ``OPTIONS`` that are
    asked for, in their order, and after the groups the other rows (the curve histogram).  ``thresholds_d``: the thresholds as a float64
    CUDA tensor; ``basemap``: the set's base map on the card, which a row with ``basemap`` reads in place; ``edges``: the set's base
    table on the card and ``longest_range`` the widest stretch in bases, for a round with ``vote_bases`` (its ranges are in
    ``t["vote_ranges"]`` already).  -> the result buffer's ``plan.out_cells`` cells, still on the card."""
    import torch
    spec, rule, n, total, longest = plan.spec, plan.spec.rule, plan.n, plan.total, plan.longest
    src_d, len_d, bounds_d = (t["table"][i * (n + 1):i * (n + 1) + count] for i, count in ((0, n), (1, n), (2, n + 1)))
    x, y, probs, logits = t["x"][:total], t["y"][:total], t["probs"][:total], t["logits"][:total]
    out = t["out"][:plan.out_cells]
    right_d, ce_d, counts_d = plan.cut(out, "right"), plan.cut(out, "ce_sum").view(torch.float64), plan.cut(out, "counts")
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
    on = Round(t, probs, y, labels, basemap, edges, src_d, bounds_d, len_d, longest_range)
    steps = [(row, value, [(plan.cut(out, name), plan.cells[name] // spec.k_all) for name in row.names]) for row, value in spec.asked]
    for k0, k1 in spec.groups:
        engine.score_validation(probs, logits, y, bounds_d, total, longest, thresholds_d[k0:k1], right_d, ce_d, counts_d[4 * k0:4 * k1],
                                t["partials"])
        for row, value, outs in steps:
            if row.per_threshold:
                row.launch(engine, plan, on, spec.thresholds[k0:k1], value, [cells[per_k * k0:per_k * k1] for cells, per_k in outs])
    for row, value, outs in steps:
        if not row.per_threshold:
            row.launch(engine, plan, on, None, value, [cells for cells, _per_k in outs])
    return out
