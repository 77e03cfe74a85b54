"""The calling chain "windows in, homopolymer spans out", written once: the rule a caller asks for (``CallRule``) and the steps every
route shares -- the buffer of the K tilings, "forward, voted" and its steps, the run lists of a synchronous route, and runs ->
per-read results.
``ReadPipeline``, ``batching.infer_*`` and ``infer.infer_class_from_raw`` are built from these; the definitions they must agree with
stay where they were (``infer.bridge_gaps``, ``tilings.vote_host``, ``span_scores.span_scores_host``)."""
from __future__ import annotations

from collections import namedtuple

from .batching import scores_from_runs, spans_from_runs
from .infer import WINDOW_SIZE, check_bridge
from .tilings import check_phases, check_weight, tiling_size


class CallRule(namedtuple("CallRule", "threshold min_run max_gap phases vote_weight scores")):
    """What is called a homopolymer, checked: ``threshold`` and ``min_run`` (``infer.correct_short``), ``max_gap``
    (``infer.bridge_gaps``; 0: none), ``phases`` / ``vote_weight`` (shifted-window voting, ``tilings.py``; ``(0,)``: one tiling) and
    whether per-call ``scores`` are wanted (``span_scores.py``).  Build one with ``CallRule.of``."""
    __slots__ = ()

    @classmethod
    def of(cls, threshold=0.5, min_run=15, max_gap=0, phases=(0,), vote_weight="mean", scores=False):
        """The checked rule, or the ValueError of the first of ``check_bridge``, ``check_phases``, ``check_weight`` that refuses."""
        min_run = int(min_run)
        max_gap = check_bridge(max_gap, min_run)
        phases = check_phases(phases)
        check_weight(vote_weight)
        return cls(float(threshold), min_run, max_gap, phases, "mean" if vote_weight is None else vote_weight, bool(scores))

    @property
    def n_tilings(self):
        return len(self.phases)

    @property
    def voted(self):
        return len(self.phases) > 1

    @property
    def bridged(self):
        return self.max_gap > 0

    @property
    def scores_by_labels(self):
        """Bridged runs hold samples below the threshold: their scores follow the labels, which are written only then."""
        return self.scores and self.max_gap > 0

    def max_runs(self, total):
        """Room for the run list of ``total`` packed samples: no two kept runs are closer than ``min_run`` samples."""
        return int(total) // max(1, self.min_run) + 16


def tiling_buffer(rule, n_windows, n_reads, device):
    """-> (x_all, x): the float32 CUDA buffer [windows of all tilings, 35] the forward pass reads and its base layout
    ``x = x_all[:n_windows]``, which the caller fills.  One tiling: ``x_all is x``."""
    import torch
    if not rule.voted:
        x = torch.empty(n_windows, WINDOW_SIZE, dtype=torch.float32, device=device)
        return x, x
    x_all = torch.empty(tiling_size(n_windows * WINDOW_SIZE, n_reads, rule.n_tilings) // WINDOW_SIZE, WINDOW_SIZE, dtype=torch.float32,
                        device=device)
    return x_all, x_all[:n_windows]


def retile_tilings(engine, rule, x_all, offsets, lengths, total, stream=None):
    """Lay out the tilings behind the filled base layout of ``x_all`` (``cf_retile_windows``); one tiling: nothing is launched."""
    if rule.voted:
        engine.retile_device(x_all, offsets, lengths, total, rule.phases, stream=stream)


def vote_tilings(engine, rule, probs_all, offsets, lengths, total, stream=None):
    """The probabilities of the base layout that everything after the forward pass sees: voted over the tilings of ``probs_all``
    (``cf_vote_tilings``, a new tensor [total]); one tiling: ``probs_all`` itself, nothing is launched."""
    if not rule.voted:
        return probs_all
    return engine.vote_device(probs_all, offsets, lengths, total, rule.phases, rule.vote_weight, stream=stream)


def forward_voted(engine, rule, x_all, offsets, lengths, total):
    """``retile_tilings``, ONE forward pass over every tiling, ``vote_tilings``, all on the current stream -> (probs, probs_all).
    ``offsets`` / ``lengths``: the int64 CUDA tables of the base layout, ``total`` its samples.  (``ReadPipeline`` issues the same
    three steps one by one, each on its own stream, inside the stream contexts and between the events it has anyway.)"""
    retile_tilings(engine, rule, x_all, offsets, lengths, total)
    probs_all = engine.infer_device(x_all)
    return vote_tilings(engine, rule, probs_all, offsets, lengths, total), probs_all


def device_runs(engine, rule, probs, offsets, lengths):
    """Sorted packed run boundaries (starts, ends) on a synchronous route: bridged, the one launch of
    ``engine.postprocess_spans_device``; else the two launches ``cf_postprocess`` + ``cf_spans``."""
    if rule.bridged:
        return engine.postprocess_spans_device(probs, offsets, lengths, threshold=rule.threshold, min_run=rule.min_run, max_gap=rule.max_gap)
    return engine.spans_device(engine.postprocess_device(probs, offsets, lengths, threshold=rule.threshold, min_run=rule.min_run))


def results_of_runs(starts, ends, sample_offsets, lengths, flat=None):
    """Sorted packed run boundaries -> per read ``(spans, read length)``, spans ``[start - 11, end + 16]`` (``infer.hp_in_pred``); with
    the flat score dict of the same runs (``flat``) ``(spans, read length, rows)``, rows float64 [n_spans, 6]."""
    n = len(lengths)
    spans = spans_from_runs(starts, ends, sample_offsets, n)
    if flat is None:
        return [(spans[i], int(lengths[i])) for i in range(n)]
    rows = scores_from_runs(flat, n)
    return [(spans[i], int(lengths[i]), rows[i]) for i in range(n)]


def spans_of_batch(engine, rule, x_all, d_offsets, d_lengths, sample_offsets, lengths):
    """The synchronous chain over a filled base layout (``tiling_buffer``) -> (``results_of_runs``, the probabilities that were
    thresholded, float32 CUDA [total])."""
    probs, _probs_all = forward_voted(engine, rule, x_all, d_offsets, d_lengths, int(sample_offsets[-1]))
    starts, ends = device_runs(engine, rule, probs, d_offsets, d_lengths)
    return results_of_runs(starts, ends, sample_offsets, lengths), probs
