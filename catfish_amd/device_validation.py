"""Device-resident validation set: the reads of a run's checkpoint rounds, uploaded once, packed and scored on the card.

``train_validate.validate`` on a list of NPZ paths re-opens every file per round, packs the stretches in numpy, copies the batch
to the card, copies probabilities and logits back and scores them in numpy.  ``DeviceValidationSet`` keeps all reads on the
card (float32 signal, uint8 labels); a round then uploads three short int64 arrays (which stretch of which read), and two HIP
launches around the forward pass do the rest (csrc/validation.hpp): ``cf_validation_gather`` packs the window-major batch,
``cf_validation_score`` returns raw integer counts and double sums, and the host finishes with the divisions
``train_validate.score_validation_batch`` uses.

Every random draw stays on the host, on Python's global generator and in the reference's order
(networks/train_validate.py:214-249), so a seeded round selects the stretches the host route selects.

This module states both device steps in numpy and those statements are normative: ``DeviceValidationSet.pack`` is what the
gather kernel writes (bit for bit), ``score_host`` what the scoring kernel returns (counts exactly; the double sums up to the
summation order), ``run_states_host`` what the run-state step returns (``cf_validation_run_states``, csrc/validation_runs.hpp:
how many homopolymers a round found, bit for bit), ``run_borders_host`` what the border step returns
(``cf_validation_run_borders``, csrc/validation_borders.hpp: how far the called borders miss and the interruptions, bit for bit),
``run_bases_host`` what the base step returns (``cf_validation_run_bases``, csrc/validation_bases.hpp: the same runs by base and by
length in bases, from the set's base map, bit for bit), ``curve_host`` what the curve step returns (``cf_validation_curve``,
csrc/validation_curve.hpp: the round's probabilities binned at every threshold step, bit for bit; ``curves_from_histogram`` turns
that table into the whole ROC and precision-recall curves, their areas and the best F1), ``run_scores_host`` what the score step
returns (``cf_validation_run_scores``, csrc/validation_scores.hpp: the probabilities under the runs of every state, bit for bit;
``run_score_summary`` gives their count, mean and quartiles).  The object is host-only until ``device_arrays`` is called and usable without a GPU.
What a round on the card decides before its first launch -- the checked options, the buffer sizes, the layout of the result buffer and
the named results -- is ``validation_round`` (host-only too).
"""
from __future__ import annotations

import random

import numpy as np

SCORE_CHUNK = 2048          # samples one workgroup of the scoring kernel reduces (CF_SCORE_CHUNK, csrc/validation.hpp)
MAX_THRESHOLDS = 16         # thresholds per scoring launch (CF_SCORE_MAX_K)


def _as_labels(labels):
    """uint8 label values; anything that is not an integer in 0..255 is an error, not a wrap-around."""
    lab = np.asarray(labels)
    if lab.ndim != 1:
        lab = lab.reshape(-1)
    if lab.dtype == np.uint8:
        return lab
    if lab.dtype == np.bool_:
        return lab.astype(np.uint8)
    if not np.issubdtype(lab.dtype, np.number) or np.issubdtype(lab.dtype, np.complexfloating):
        raise ValueError("labels must be numbers, got dtype %s" % lab.dtype)
    if lab.size and not np.issubdtype(lab.dtype, np.integer) and not np.all(lab == np.rint(lab)):      # NaN fails too
        raise ValueError("labels must be integers")
    if lab.size and (lab.min() < 0 or lab.max() > 255):
        raise ValueError("labels must lie in 0..255")
    return lab.astype(np.uint8)


def layout(lengths, window):
    """Where the stretches sit in the packed batch: (bounds int64 [n + 1], tails int64 [n]) -- every stretch is followed by
    its zero tail up to the next multiple of the window (``train_validate.padding``: an exact multiple gets none)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_win = -(-lengths // int(window))
    tails = n_win * int(window) - lengths
    bounds = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(n_win * int(window), out=bounds[1:])
    return bounds, tails


def score_host(probs, logits, y, bounds, thresholds):
    """What ``cf_validation_score`` returns, in numpy: (right int64 [n], ce_sum float64 [n], counts int64 [K, 4]).

    With ``p``, ``z`` promoted to double and ``y`` the label value: ``right[r]`` counts read r's samples with
    ``round_half_even(p) == y``; ``ce_sum[r]`` sums ``max(z, 0) - z*y + log1p(exp(-|z|))`` over them; ``counts[k]`` =
    (tp, fp, tn_raw, fn) over ALL samples at ``thresholds[k]``: a sample is called when ``p >= t``, a called one is a true
    positive when its label is 1 and a false positive otherwise, an un-called one a true negative when its label is 0 and a
    false negative otherwise.  ``tn_raw`` still holds the zero tails (``finish`` takes them out)."""
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    z = np.asarray(logits, dtype=np.float64).reshape(-1)
    y = np.asarray(y).reshape(-1).astype(np.float64)
    bounds = np.asarray(bounds, dtype=np.int64)
    right_run = np.concatenate(([0], np.cumsum(np.round(p) == y))).astype(np.int64)
    right = right_run[bounds[1:]] - right_run[bounds[:-1]]
    ce = np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))
    ce_sum = np.array([np.sum(ce[a:b]) for a, b in zip(bounds[:-1].tolist(), bounds[1:].tolist())], dtype=np.float64)
    counts = np.zeros((len(thresholds), 4), dtype=np.int64)
    for k, t in enumerate(thresholds):
        called = p >= float(t)
        counts[k] = (np.count_nonzero(called & (y == 1)), np.count_nonzero(called & (y != 1)),
                     np.count_nonzero(~called & (y == 0)), np.count_nonzero(~called & (y != 0)))
    return right, ce_sum, counts


MAX_RUN_EDGES = 7           # length-bin edges per run-state call (CF_RUN_MAX_EDGES, csrc/validation_runs_word.hpp)
RUN_STATES = ("complete", "incomplete", "absent")          # check_hp's states, in the order of the table's last axis


def check_run_edges(edges):
    """``edges`` as a tuple of ints: at most 7, positive, strictly ascending (ValueError otherwise)."""
    out = []
    for e in edges:
        if isinstance(e, bool) or int(e) != e:
            raise ValueError("run edges must be integers, got %r" % (e,))
        out.append(int(e))
    if len(out) > MAX_RUN_EDGES:
        raise ValueError("at most %d run edges, got %d" % (MAX_RUN_EDGES, len(out)))
    if any(e < 1 for e in out) or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("run edges must be positive and ascending, got %r" % (tuple(out),))
    return tuple(out)


def _runs_of(mask):
    """(starts, ends) of the runs of a boolean array, ends inclusive, with ``hp_loc_dict``'s rule
    (networks/process_output.py:633-636): an open run is closed AT the last index whatever that sample holds."""
    m = np.array(mask, dtype=bool)
    if m.size >= 2 and m[-2]:
        m[-1] = True
    step = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    return np.flatnonzero(step == 1), np.flatnonzero(step == -1) - 1


def _states_of(starts, ends, other):
    """``check_hp``'s state of every run against ``other``: 0 complete (all 1), 2 absent (all 0), 1 incomplete."""
    ones = np.concatenate(([0], np.cumsum(other == 1)))
    zeros = np.concatenate(([0], np.cumsum(other == 0)))
    size = ends - starts + 1
    return np.where(ones[ends + 1] - ones[starts] == size, 0, np.where(zeros[ends + 1] - zeros[starts] == size, 2, 1))


def _stretch_predictions(probs, y, bounds, lengths, thresholds, min_run, max_gap):
    """What ``run_states_host``, ``run_bases_host`` and ``run_borders_host`` share.  At the call: the checks of ``min_run`` /
    ``max_gap`` and the arrays as they are read.  Returned: an iterator over the non-empty stretches, ``(b0, n, truth, preds)`` --
    ``truth`` = ``y`` over the stretch alone and ``preds`` the list of ``(k, pred)`` of every threshold, ``pred`` = the corrected
    prediction over the stretch alone, int64 0 / 1."""
    from .infer import bridge_gaps, check_bridge, correct_short
    if int(min_run) < 1:
        raise ValueError("min_run must be >= 1")
    max_gap = check_bridge(max_gap, min_run)
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    y = np.asarray(y).reshape(-1)
    bounds = np.asarray(bounds, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)

    def stretches():
        for b0, n in zip(bounds[:len(lengths)].tolist(), lengths.tolist()):
            if n > 0:
                called = [(p[b0:b0 + n] >= float(t)).astype(np.int64) for t in thresholds]
                yield b0, n, y[b0:b0 + n], [(k, np.asarray(correct_short(bridge_gaps(c, max_gap), int(min_run)))) for k, c in enumerate(called)]

    return stretches()


def _kinds(truth, pred):
    """``(kind, mask, other)``: kind 0, the runs of ``truth == 1`` judged against ``pred``; kind 1, those of ``pred == 1`` against ``truth``."""
    return ((0, truth == 1, pred), (1, pred == 1, truth))


def run_states_host(probs, y, bounds, lengths, thresholds, edges=(), min_run=15, max_gap=0):
    """What ``cf_validation_run_states`` returns, in numpy: int64 [K, 2, B, 3] -- per threshold, kind, length bin and state how
    many runs (the reference's offline networks/process_output.py:235-273).

    Stretch r is the ``lengths[r]`` packed samples from ``bounds[r]``; its zero tail is not part of it.  Per threshold t the
    prediction is ``infer.correct_short((double)p >= t, min_run)`` over the stretch alone.  A run is a maximal run of ones, plus
    ``hp_loc_dict``'s rule: a run whose last one sits at n - 2 ends at n - 1 (only the run mask changes, never the array a run is
    judged against).  Kind 0: the runs of ``y == 1`` judged against the prediction; kind 1: the runs of the prediction judged
    against ``y``.  State (``check_hp``) 0 = complete, the other array is 1 over the whole run; 2 = absent, it is 0 over the whole
    run; 1 = incomplete, anything else (so a label other than 0 / 1 inside a run makes it incomplete).  A run of L samples falls
    into bin ``searchsorted(edges, L, side="right")``; B = len(edges) + 1.

    ``max_gap > 0`` (``cf_validation_run_states_bridged``): the prediction is ``correct_short(infer.bridge_gaps((double)p >= t,
    max_gap), min_run)`` over the stretch alone; ValueError for ``min_run + max_gap > 64``."""
    edges = np.asarray(check_run_edges(edges), dtype=np.int64)
    stretches = _stretch_predictions(probs, y, bounds, lengths, thresholds, min_run, max_gap)
    out = np.zeros((len(thresholds), 2, len(edges) + 1, 3), dtype=np.int64)
    for _b0, _n, truth, preds in stretches:
        for k, pred in preds:
            for kind, mask, other in _kinds(truth, pred):
                starts, ends = _runs_of(mask)
                bins = np.searchsorted(edges, ends - starts + 1, side="right")
                np.add.at(out[k, kind], (bins, _states_of(starts, ends, other)), 1)
    return out


def run_state_rates(table):
    """The three rates of one threshold's [2, B, 3] table: (hp_complete, hp_found, called_absent) = complete / all true runs,
    (complete + incomplete) / all true runs, absent / all called runs; 0 for an empty denominator (``metrics.precision_recall``)."""
    true_runs, called = np.asarray(table)[0].sum(axis=0), np.asarray(table)[1].sum(axis=0)
    n_true, n_called = int(true_runs.sum()), int(called.sum())
    return (int(true_runs[0]) / n_true if n_true else 0, int(true_runs[0] + true_runs[1]) / n_true if n_true else 0,
            int(called[2]) / n_called if n_called else 0)


MAX_BASES_LIMIT = 32        # the most length bins in bases (VBS_MAX_BASES, csrc/validation_bases_word.hpp)
MAX_BASES = 16
BASE_CLASSES = ("A", "C", "G", "T", "other")               # the fourth axis of a run-bases table
BASE_MARK = 0x80            # the base map's "new base" bit (labelling.MARK)


def check_max_bases(max_bases):
    """``max_bases`` as an int in 1 .. 32 (ValueError otherwise; no bool, no fraction)."""
    if isinstance(max_bases, (bool, np.bool_)) or not isinstance(max_bases, (int, np.integer)) or not 1 <= max_bases <= MAX_BASES_LIMIT:
        raise ValueError("max_bases must be an int in 1 .. %d, got %r" % (MAX_BASES_LIMIT, max_bases))
    return int(max_bases)


def _bases_of(starts, ends, bmap, max_bases):
    """(class, bin) of every run [s, e] over one stretch's base map: the marked samples inside the run are its bases
    (``get_bases``); class 0..3 when there is one and all are that upper-case letter, else 4; bin = min(how many, max_bases)."""
    marked = (bmap & BASE_MARK) != 0
    count = np.concatenate(([0], np.cumsum(marked)))
    nb = count[ends + 1] - count[starts]
    cls = np.full(starts.size, 4, dtype=np.int64)
    for c, letter in enumerate(b"ACGT"):
        same = np.concatenate(([0], np.cumsum(marked & ((bmap & 0x7f) == letter))))
        cls[(nb >= 1) & (same[ends + 1] - same[starts] == nb)] = c
    return cls, np.minimum(nb, max_bases)


def run_bases_host(probs, y, basemap, bounds, lengths, thresholds, max_bases=MAX_BASES, min_run=15, max_gap=0):
    """What ``cf_validation_run_bases`` returns, in numpy: int64 [K, 2, 3, 5, max_bases + 1] -- per threshold, kind, state, base
    class and length in BASES how many runs (the reference's offline networks/process_output.py: ``prediction_information`` ->
    ``base_count_dict`` / ``get_bases`` / ``get_prevalence`` over the runs of ``hp_loc_dict`` and the states of ``check_hp``).

    Stretches, thresholds, the corrected prediction, runs (``_runs_of``, the last-sample rule included), kinds and states are
    ``run_states_host``'s.  ``basemap`` is packed like ``y`` (sample ``bounds[r] + i``; the zero tails are ignored): the event's
    base byte with bit 7 on the event's centre sample (``labelling.base_map_host``).  The bases of a run [s, e] are
    ``basemap[i] & 0x7f`` at the positions i in [s, e] with ``basemap[i] & 0x80``, in order; ``nb`` = how many -- the sample the
    last-sample rule adds counts.  Class 0..3 (``BASE_CLASSES``): ``nb >= 1`` and every one of them is that upper-case letter (a byte
    comparison); class 4, "other": anything else -- mixed, ``N``, lower case, or no base at all.  Bin = ``min(nb, max_bases)``.
    Summed over class and bin the table is ``run_states_host(..., edges=())`` with its axes as [K, 2, 3]."""
    max_bases = check_max_bases(max_bases)
    stretches = _stretch_predictions(probs, y, bounds, lengths, thresholds, min_run, max_gap)
    basemap = np.asarray(basemap, dtype=np.uint8).reshape(-1)
    out = np.zeros((len(thresholds), 2, 3, len(BASE_CLASSES), max_bases + 1), dtype=np.int64)
    for b0, n, truth, preds in stretches:
        for k, pred in preds:
            for kind, mask, other in _kinds(truth, pred):
                starts, ends = _runs_of(mask)
                cls, bins = _bases_of(starts, ends, basemap[b0:b0 + n], max_bases)
                np.add.at(out[k, kind], (_states_of(starts, ends, other), cls, bins), 1)
    return out


def run_base_rates(table_k):
    """One threshold's [2, 3, 5, B] table -> dict: ``recall_by_base`` [5] and ``recall_by_length`` [B] = (complete + incomplete) /
    all true runs of that class or bin; ``complete_by_base`` / ``complete_by_length`` = complete / all of them; ``called_pure`` =
    the share of called runs with a class below 4.  A share over nothing is 0 (``run_state_rates``)."""
    table = np.asarray(table_k)
    if table.ndim != 4 or table.shape[:3] != (2, 3, len(BASE_CLASSES)):
        raise ValueError("one threshold's run-bases table is [2, 3, 5, B], got %s" % (table.shape,))
    share = lambda part, whole: [int(a) / int(b) if b else 0 for a, b in zip(part.tolist(), whole.tolist())]     # noqa: E731
    by_base, by_length = table[0].sum(axis=2), table[0].sum(axis=1)               # [3, 5], [3, B]
    n_called = int(table[1].sum())
    return {"recall_by_base": share(by_base[0] + by_base[1], by_base.sum(axis=0)),
            "recall_by_length": share(by_length[0] + by_length[1], by_length.sum(axis=0)),
            "complete_by_base": share(by_base[0], by_base.sum(axis=0)),
            "complete_by_length": share(by_length[0], by_length.sum(axis=0)),
            "called_pure": int(table[1][:, :4].sum()) / n_called if n_called else 0}


MAX_BORDER_REACH = 128      # the widest offset / interruption histogram (VB_MAX_REACH, csrc/validation_borders_word.hpp)
BORDER_REACH = 64


def check_border_reach(reach):
    """``reach`` as an int in 1 .. 128 (ValueError otherwise; no bool, no fraction)."""
    if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or not 1 <= reach <= MAX_BORDER_REACH:
        raise ValueError("border reach must be an int in 1 .. %d, got %r" % (MAX_BORDER_REACH, reach))
    return int(reach)


def border_cells(reach):
    """Cells of one (threshold, kind) row of a border table: ``5 * reach + 3``."""
    return 5 * check_border_reach(reach) + 3


def _streak(mask):
    """How many consecutive True values end at every index (inclusive), int64."""
    at = np.arange(1, mask.size + 1, dtype=np.int64)
    return at - np.maximum.accumulate(np.where(mask, 0, at))


def _borders_of(mask, other, reach, row):
    """Add the non-absent runs of ``mask`` (bool), judged against ``other`` (bool: the other array is 1), to one row."""
    starts, ends = _runs_of(mask)
    if not starts.size:
        return
    ones = np.concatenate(([0], np.cumsum(other)))
    judged = ones[ends + 1] - ones[starts] > 0
    starts, ends = starts[judged], ends[judged]
    inner = other.copy()
    inner[0] = False                                       # check_hp: `not position <= 0` -- position 0 never counts
    ones_to = np.concatenate(([0], _streak(inner)))        # [i]: ones ending at i - 1, position 0 left out
    zeros_to, zeros_from = _streak(~other), _streak(~other[::-1])[::-1]
    ones_from = np.concatenate((_streak(other[::-1])[::-1], [0]))
    left = np.where(other[starts], -ones_to[starts], zeros_from[starts])
    right = np.where(other[ends], ones_from[ends + 1], -zeros_to[ends])
    np.add.at(row, np.clip(left, -reach, reach) + reach, 1)
    np.add.at(row, 2 * reach + 1 + np.clip(right, -reach, reach) + reach, 1)
    step = np.diff(np.concatenate(([0], (~other).astype(np.int8), [0])))
    hole_starts, hole_ends = np.flatnonzero(step == 1), np.flatnonzero(step == -1) - 1
    run = np.searchsorted(starts, hole_starts, side="right") - 1          # the judged run a hole could lie in
    inside = run >= 0
    inside[inside] = (hole_starts[inside] > starts[run[inside]]) & (hole_ends[inside] < ends[run[inside]])
    np.add.at(row, 4 * reach + 2 + np.minimum(hole_ends[inside] - hole_starts[inside] + 1, reach) - 1, 1)
    row[5 * reach + 2] += np.unique(run[inside]).size


def run_borders_host(probs, y, bounds, lengths, thresholds, reach=BORDER_REACH, min_run=15, max_gap=0):
    """What ``cf_validation_run_borders`` returns, in numpy: int64 [K, 2, 5 * reach + 3] -- the rest of what the reference's
    ``check_hp`` says about a run (networks/process_output.py:814-895): how far the other array's ones reach beyond its borders
    or fall short of them, and the interruptions inside it.

    Stretches, prediction, runs (``_runs_of``, the last-sample rule included) and kinds are ``run_states_host``'s; labels must be 0
    or 1 inside every stretch (ValueError).  Per run [s, e] that is not absent, with ``o`` the other array and n the stretch length:
    left ``l`` = minus the ones of ``o`` immediately before s, position 0 never counted (``check_hp`` tests ``not position <= 0``),
    when ``o[s] == 1``, else the zeros of ``o`` from s to its first one; right ``r`` = the ones of ``o`` after e (up to n - 1) when
    ``o[e] == 1``, else minus the zeros of ``o`` from e down to its last one; interruptions = the maximal runs of zeros of ``o``
    inside [s, e] that touch neither end.  ``l < 0`` / ``r > 0``: the other array's ones reach beyond the run; ``l > 0`` /
    ``r < 0``: they start late / stop early.  Cells of a row, R = reach: [0, 2R+1) histogram of ``clip(l, -R, R) + R``; [2R+1, 4R+2)
    of ``clip(r, -R, R) + R``; [4R+2, 5R+2) of ``min(g, R) - 1`` over the interruption lengths g; [5R+2] runs with an interruption.

    ``max_gap > 0`` (``cf_validation_run_borders_bridged``): the bridged prediction of ``run_states_host``."""
    reach = check_border_reach(reach)
    stretches = _stretch_predictions(probs, y, bounds, lengths, thresholds, min_run, max_gap)
    out = np.zeros((len(thresholds), 2, 5 * reach + 3), dtype=np.int64)
    for _b0, _n, truth, preds in stretches:
        if np.any((truth != 0) & (truth != 1)):
            raise ValueError("run borders need labels of 0 or 1, got %r" % (truth[(truth != 0) & (truth != 1)][0],))
        for k, pred in preds:
            for kind, mask, other in _kinds(truth, pred):
                _borders_of(mask, other == 1, reach, out[k, kind])
    return out


def split_run_borders(table, reach):
    """The four parts of a border table ``[..., 5 * reach + 3]`` as views: {"left": [..., 2R+1], "right": [..., 2R+1],
    "gaps": [..., R], "interrupted": [...]}."""
    r = check_border_reach(reach)
    table = np.asarray(table)
    if table.shape[-1] != 5 * r + 3:
        raise ValueError("a border table at reach %d has %d cells per row, got %d" % (r, 5 * r + 3, table.shape[-1]))
    return {"left": table[..., :2 * r + 1], "right": table[..., 2 * r + 1:4 * r + 2], "gaps": table[..., 4 * r + 2:5 * r + 2],
            "interrupted": table[..., 5 * r + 2]}


def _lower_median(hist, reach):
    """The lower median offset of a ``clip(v, -R, R) + R`` histogram; None when it is empty or the median lies in a clip bin."""
    total = int(hist.sum())
    if not total:
        return None
    at = int(np.searchsorted(np.cumsum(hist), (total + 1) // 2))
    return None if at in (0, 2 * reach) else at - reach


def run_border_summary(row, reach):
    """One threshold's ``[2, 5 * reach + 3]`` row -> per kind a dict: ``judged`` (runs that are not absent), ``exact_left`` /
    ``exact_right`` (share at offset 0), ``median_left`` / ``median_right`` (lower median from the histogram; None in a clip bin
    or without runs), ``clipped`` (share of runs in the four end bins), ``interrupted`` (share of judged runs), ``gaps`` (number of
    interruptions).  A share over nothing is 0 (``metrics.precision_recall``)."""
    r = check_border_reach(reach)
    row = np.asarray(row)
    if row.shape != (2, 5 * r + 3):
        raise ValueError("one threshold's border row at reach %d is [2, %d], got %s" % (r, 5 * r + 3, row.shape))
    out = []
    for kind in range(2):
        part = split_run_borders(row[kind], r)
        left, right = part["left"], part["right"]
        judged = int(left.sum())
        share = lambda count: int(count) / judged if judged else 0            # noqa: E731
        out.append({"judged": judged, "exact_left": share(left[r]), "exact_right": share(right[r]),
                    "median_left": _lower_median(left, r), "median_right": _lower_median(right, r),
                    "clipped": share(left[0] + left[2 * r] + right[0] + right[2 * r]), "interrupted": share(part["interrupted"]),
                    "gaps": int(part["gaps"].sum())})
    return out


CURVE_ONE_BITS = 0x3F800000                                # float32 1.0 (VC_ONE_BITS, csrc/validation_curve_bin.hpp)
CURVE_SHIFT_MIN, CURVE_SHIFT_MAX, CURVE_SHIFT = 10, 22, 14


def curve_bins(shift=CURVE_SHIFT):
    """Bins of a curve histogram: ``(0x3F800000 >> shift) + 1`` -- 65 025 at shift 14.  ``shift`` is an int in 10 .. 22."""
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not CURVE_SHIFT_MIN <= shift <= CURVE_SHIFT_MAX:
        raise ValueError("curve shift must be an int in %d .. %d, got %r" % (CURVE_SHIFT_MIN, CURVE_SHIFT_MAX, shift))
    return (CURVE_ONE_BITS >> int(shift)) + 1


def curve_bin(bits, shift=CURVE_SHIFT):
    """The bin of float32 probabilities given by their bit patterns (any integer array or scalar; only the low 32 bits count): read
    as signed int32, negatives clamped to 0, shifted right, clamped to the top bin -> int64.  Non-negative floats order as their
    bits do, so for every p in [0, 1]: ``p >= curve_thresholds(shift)[b]``  <=>  ``curve_bin(p) >= b``.  The top bin holds exactly
    p == 1.0 plus what is clamped into it (1 + ulp, +inf, positive NaN); -0.0, negative values and negative NaN go to bin 0."""
    top = curve_bins(shift) - 1
    signed = (np.asarray(bits).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
    return np.minimum(np.maximum(signed, 0) >> int(shift), top)


def curve_thresholds(shift=CURVE_SHIFT):
    """float32 [NB]: the lower edge of every bin, the float whose bits are ``b << shift`` (0.0 first, exactly 1.0 last)."""
    return (np.arange(curve_bins(shift), dtype=np.uint32) << np.uint32(shift)).view(np.float32)


def curve_host(probs, y, bounds, lengths, shift=CURVE_SHIFT):
    """What ``cf_validation_curve`` returns, in numpy: int64 [3, NB] -- how many samples of label 1 (row 0), label 0 (row 1) and
    any other label (row 2) fall into every bin of ``curve_bin``.  Only the ``lengths[r]`` real samples from ``bounds[r]`` are
    counted; the zero tails are not part of it, as in ``run_states_host``."""
    nb = curve_bins(shift)
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float32).reshape(-1))
    y = np.asarray(y).reshape(-1)
    bounds = np.asarray(bounds, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    hist = np.zeros((3, nb), dtype=np.int64)
    for b0, size, n in zip(bounds[:len(lengths)].tolist(), np.diff(bounds)[:len(lengths)].tolist(), lengths.tolist()):
        n = min(n, size, p.size - b0)
        if n <= 0:
            continue
        bins = curve_bin(p[b0:b0 + n].view(np.uint32), shift)
        label = y[b0:b0 + n]
        rows = np.where(label == 1, 0, np.where(label == 0, 1, 2))
        hist += np.bincount(rows * nb + bins, minlength=3 * nb).reshape(3, nb)
    return hist


def curves_from_histogram(hist, shift=CURVE_SHIFT):
    """The whole ROC and precision-recall curves of a ``curve_host`` histogram (the reference computes them offline from dumps of
    every score: networks/metrics.py:66-94, networks/precision_recall_ROC.py:14-82).  Entry b of every array belongs to the
    threshold ``curve_thresholds(shift)[b]``; a sample is called there when its bin is >= b.  -> dict:

    ``tp``, ``fp``, ``tn``, ``fn`` int64 [NB]: ``score_host``'s rules without the tails -- called & label 1, called & any other
    label, not called & label 0, not called & any label but 0 (so they equal ``score_host`` + ``finish`` wherever no tail sample is
    called and no probability is NaN).  ``n_pos``, ``n_neg``, ``n_other``: samples of label 1, 0 and neither.
    ``tpr``, ``fpr`` float64 [NB]: called label-1 samples / n_pos and called label-0 samples / n_neg (nan for an empty class).
    ``precision``, ``recall`` float64 [NB]: ``metrics.precision_recall(tp, fp, fn)``, 0 for an empty denominator.
    ``roc_auc``: the trapezoid under (fpr, tpr) over the bins, = sum_b neg_b (2 tp_above_b + pos_b) / (2 P N): the AUC of the
    scores quantised to their bin edge (sklearn's ``roc_auc_score`` of them, ties counted one half).
    ``roc_auc_slack`` = sum_b pos_b neg_b / (2 P N): only pairs that share a bin can order differently before quantisation, and
    each is counted one half, so the AUC of the unquantised scores lies within ``roc_auc`` +- ``roc_auc_slack``.
    ``pr_auc``: ``sklearn.metrics.auc(recall, precision)`` in ``precision_recall_curve``'s convention -- one point per OCCUPIED bin
    (precision = tp / (tp + fp), recall = tp / n_pos there) and the final point (recall 0, precision 1), trapezoids between.
    ``best_f1``: {threshold, f1, precision, recall} of the first bin with the largest ``metrics.f1(precision, recall)``.
    ``roc_auc``, ``roc_auc_slack`` and ``pr_auc`` are nan when n_pos or n_neg is 0."""
    nb = curve_bins(shift)
    hist = np.asarray(hist, dtype=np.int64)
    if hist.shape != (3, nb):
        raise ValueError("a curve histogram at shift %d is int64 [3, %d], got %s" % (shift, nb, hist.shape))
    pos, neg, other = hist[0], hist[1], hist[2]
    n_pos, n_neg, n_other = int(pos.sum()), int(neg.sum()), int(other.sum())
    from_top = lambda row: np.cumsum(row[::-1])[::-1]                                # noqa: E731   bins >= b
    below = lambda row: np.concatenate(([0], np.cumsum(row)[:-1]))                   # noqa: E731   bins < b
    tp, called_neg = from_top(pos), from_top(neg)
    fp = called_neg + from_top(other)
    tn, fn = below(neg), below(pos + other)
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr = tp / np.float64(n_pos) if n_pos else np.full(nb, np.nan)
        fpr = called_neg / np.float64(n_neg) if n_neg else np.full(nb, np.nan)
        precision = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1), 0.0)          # int / int in double, as Python divides them
        recall = np.where(tp + fn > 0, tp / np.maximum(tp + fn, 1), 0.0)
        f1 = np.where(precision + recall > 0, 2 * (precision * recall) / (precision + recall), 0.0)
    roc_auc = roc_auc_slack = pr_auc = float("nan")
    if n_pos and n_neg:
        at = np.flatnonzero(neg)
        above = tp[at] - pos[at]                                                     # label-1 samples in the bins above b
        if 2 * n_pos * n_neg < 2 ** 62:                                              # exact in int64
            area, shared = int(np.sum(neg[at] * (2 * above + pos[at]))), int(np.sum(neg[at] * pos[at]))
        else:
            area = float(np.sum(neg[at].astype(np.float64) * (2.0 * above + pos[at])))
            shared = float(np.sum(neg[at].astype(np.float64) * pos[at]))
        roc_auc, roc_auc_slack = area / (2 * n_pos * n_neg), shared / (2 * n_pos * n_neg)
        occupied = np.flatnonzero(pos + neg + other)
        r = np.concatenate((tp[occupied] / np.float64(n_pos), [0.0]))
        p = np.concatenate((tp[occupied] / (tp[occupied] + fp[occupied]).astype(np.float64), [1.0]))
        pr_auc = float(np.sum((r[:-1] - r[1:]) * (p[:-1] + p[1:]) / 2.0))
    best = int(np.argmax(f1))
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fn, "n_pos": n_pos, "n_neg": n_neg, "n_other": n_other, "tpr": tpr, "fpr": fpr,
            "precision": precision, "recall": recall, "roc_auc": roc_auc, "roc_auc_slack": roc_auc_slack, "pr_auc": pr_auc,
            "best_f1": {"threshold": float(curve_thresholds(shift)[best]), "f1": float(f1[best]), "precision": float(precision[best]),
                        "recall": float(recall[best])}}


SCORE_SHIFT_MIN, SCORE_SHIFT_MAX, RUN_SCORE_SHIFT = 14, 22, 16     # VS_SHIFT_MIN / VS_SHIFT_MAX, csrc/validation_scores_word.hpp


def check_score_shift(shift):
    """``shift`` as an int in 14 .. 22 (ValueError otherwise; no bool, no fraction).  At 14 and sixteen thresholds a score table is
    6.2 M cells already; below it would be gigabytes."""
    if isinstance(shift, (bool, np.bool_)) or not isinstance(shift, (int, np.integer)) or not SCORE_SHIFT_MIN <= shift <= SCORE_SHIFT_MAX:
        raise ValueError("score shift must be an int in %d .. %d, got %r" % (SCORE_SHIFT_MIN, SCORE_SHIFT_MAX, shift))
    return int(shift)


def score_cells(shift=RUN_SCORE_SHIFT):
    """Cells of one threshold's score table: ``2 * 3 * (curve_bins(shift) + 1)`` -- 97 548 at shift 16."""
    return 2 * len(RUN_STATES) * (curve_bins(check_score_shift(shift)) + 1)


def run_scores_host(probs, y, bounds, lengths, thresholds, shift=RUN_SCORE_SHIFT, min_run=15, max_gap=0):
    """What ``cf_validation_run_scores`` returns, in numpy: int64 [K, 2, 3, NB + 1], NB = ``curve_bins(shift)`` -- per threshold,
    kind and state of a run the histogram of the probabilities of the samples under those runs, and in the last cell their
    fixed-point sum (the reference's offline networks/process_output.py:15-137 ``check_for_false_neg`` collects
    ``predicted_scores[a:b + 1]`` of every missed homopolymer, and ``main`` :276-357 those of the "tp" and "fp" runs).

    Stretches, thresholds, the corrected prediction (``max_gap`` included), runs (``_runs_of``, the last-sample rule included),
    kinds and states are ``run_states_host``'s.  Every sample ``start .. end`` of a run of kind q and state s at threshold k adds one
    to ``out[k, q, s, curve_bin(bits of float32 p, shift)]`` and ``base_votes.q_of(p)`` -- ``floor(double(p) * 2^32)``, NaN and
    ``p < 0`` as 0, ``p > 1`` as 2^32 -- to ``out[k, q, s, NB]``.  The sample the last-sample rule adds to a run counts with its own
    probability (the reference's slice counts it too), and a sample that lies in a true run and in a called run counts once under
    each kind.  ``shift`` is an int in 14 .. 22 (``check_score_shift``)."""
    from .base_votes import q_of
    nb = curve_bins(check_score_shift(shift))
    stretches = _stretch_predictions(probs, y, bounds, lengths, thresholds, min_run, max_gap)
    p32 = np.ascontiguousarray(np.asarray(probs, dtype=np.float32).reshape(-1))
    out = np.zeros((len(thresholds), 2, 3, nb + 1), dtype=np.int64)
    for b0, n, truth, preds in stretches:
        bins = curve_bin(p32[b0:b0 + n].view(np.uint32), shift)
        q_to = np.concatenate(([0], np.cumsum(q_of(p32[b0:b0 + n]).astype(np.int64))))
        for k, pred in preds:
            for kind, mask, other in _kinds(truth, pred):
                starts, ends = _runs_of(mask)
                if not starts.size:
                    continue
                states = _states_of(starts, ends, other)
                edge = np.zeros(n + 1, dtype=np.int64)                     # the state of every sample's run, + 1; 0 outside the runs
                np.add.at(edge, starts, states + 1)
                np.add.at(edge, ends + 1, -(states + 1))
                painted = np.cumsum(edge[:n])
                inside = painted > 0
                out[k, kind, :, :nb] += np.bincount((painted[inside] - 1) * nb + bins[inside], minlength=3 * nb).reshape(3, nb)
                np.add.at(out[k, kind, :, nb], states, q_to[ends + 1] - q_to[starts])
    return out


def run_score_summary(table_k, shift=RUN_SCORE_SHIFT):
    """One threshold's ``[2, 3, NB + 1]`` score table -> ``[kind][state]`` dicts: ``n`` (samples), ``mean`` = sum / (n * 2^32), and
    ``q1`` / ``median`` / ``q3`` as ``(low, high)``: ``low`` is the lower edge of the bin that holds the lower-quantile sample (sample
    ``ceil(n * f)`` of the sorted ones, as ``_lower_median`` picks the middle one), ``high`` the lower edge of the next bin, 1.0 for
    the top bin -- the sample's probability lies in ``[low, high)``, or is clamped into the top bin.  An empty row gives None for
    all of them but ``n``."""
    nb = curve_bins(check_score_shift(shift))
    table = np.asarray(table_k)
    if table.shape != (2, 3, nb + 1):
        raise ValueError("one threshold's score table at shift %d is [2, 3, %d], got %s" % (shift, nb + 1, table.shape))
    edges = np.concatenate((curve_thresholds(shift).astype(np.float64), [1.0]))

    def summary(row):
        n = int(row[:nb].sum())
        if not n:
            return {"n": 0, "mean": None, "q1": None, "median": None, "q3": None}
        upto = np.cumsum(row[:nb])
        span = lambda rank: (lambda at: (float(edges[at]), float(edges[at + 1])))(int(np.searchsorted(upto, rank)))     # noqa: E731
        return {"n": n, "mean": int(row[nb]) / (n << 32),"q1": span((n + 3) // 4), "median": span((n + 1) // 2),
                "q3": span((3 * n + 3) // 4)}

    return [[summary(table[kind, state]) for state in range(3)] for kind in range(2)]


def finish(right, ce_sum, counts_k, bounds, tails):
    """The divisions of ``train_validate.score_validation_batch`` on the raw results: (acc float32 [n], loss float32 [n],
    (tp, fp, tn, fn)).  ``acc`` = count as float32 / size as float32; ``loss`` = ``ce_sum / size`` in double, then float32;
    every tail sample leaves the true negatives whether or not it was one (rnn_class.py:245-249)."""
    sizes = np.diff(np.asarray(bounds, dtype=np.int64))
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.asarray(right, dtype=np.int64).astype(np.float32) / sizes.astype(np.float32)
        loss = np.asarray(ce_sum, dtype=np.float64) / sizes
    tp, fp, tn, fn = (int(v) for v in counts_k)
    return acc, loss.astype(np.float32), (tp, fp, tn - int(np.sum(tails)), fn)


class DeviceValidationSet(object):
    """All validation reads of a run, concatenated: ``signal`` float32 [total] (cast once -- the values
    ``pack_validation_windows`` writes into its float32 batch), ``labels`` uint8 [total], ``offsets`` int64 [n_reads + 1],
    ``lengths`` int64 [n_reads]; ``basemap`` uint8 [total] or None -- the per-sample base map of reads that came with their
    event tables (``labelling.base_map_host``), what ``run_bases_host`` counts bases on; ``bases`` a ``base_votes.BaseTable`` over the
    same reads or None -- which samples belong to which base, what a round with ``vote_bases`` votes on (``from_tables``
    builds it)."""

    def __init__(self, signal, labels, offsets, device=None, basemap=None, bases=None):
        self.signal = signal
        self.labels = labels
        self.offsets = offsets
        self.lengths = np.diff(offsets)
        self.device = device
        if basemap is not None:
            basemap = np.asarray(basemap)
            if basemap.dtype != np.uint8 or basemap.shape != (int(offsets[-1]),):
                raise ValueError("basemap must be uint8 [%d], got %s %s" % (int(offsets[-1]), basemap.dtype, basemap.shape))
        self.basemap = basemap
        self.bases = None if bases is None else bases.check_set(offsets)
        self._dev = None                 # {"device", "signal", "labels"[, "basemap"][, "edges"]} on the card, uploaded once
        self.uploads = 0                 # how often the reads went to a card
        self._binary = None              # every label is 0 or 1 (looked at once)

    @classmethod
    def from_arrays(cls, signals, labels, device=None, basemaps=None):
        signals = [np.asarray(s).reshape(-1) for s in signals]
        labels = [_as_labels(l) for l in labels]
        if len(signals) != len(labels):
            raise ValueError("%d signals but %d label arrays" % (len(signals), len(labels)))
        for i, (s, l) in enumerate(zip(signals, labels)):
            if len(s) != len(l):
                raise ValueError("read %d: %d samples but %d labels" % (i, len(s), len(l)))
        if basemaps is not None:
            basemaps = [np.asarray(b).reshape(-1) for b in basemaps]
            if len(basemaps) != len(signals):
                raise ValueError("%d signals but %d base maps" % (len(signals), len(basemaps)))
            for i, (s, b) in enumerate(zip(signals, basemaps)):
                if b.dtype != np.uint8 or len(b) != len(s):
                    raise ValueError("read %d: the base map must be uint8 [%d], got %s [%d]" % (i, len(s), b.dtype, len(b)))
        offsets = np.zeros(len(signals) + 1, dtype=np.int64)
        np.cumsum(np.array([len(s) for s in signals], dtype=np.int64), out=offsets[1:])
        signal = np.zeros(int(offsets[-1]), dtype=np.float32)
        lab = np.zeros(int(offsets[-1]), dtype=np.uint8)
        for o, s, l in zip(offsets[:-1].tolist(), signals, labels):
            signal[o:o + len(s)] = s
            lab[o:o + len(l)] = l
        if basemaps is None:
            return cls(signal, lab, offsets, device)
        return cls(signal, lab, offsets, device, np.concatenate(basemaps) if basemaps else np.zeros(0, np.uint8))

    @classmethod
    def from_npz(cls, paths, loader=None, device=None):
        """The reads of ``paths`` (``raw`` + ``base_labels``, networks/reader.py:11-23), in that order."""
        if loader is None:
            from .train_validate import load_npz as loader
        signals, labels = [], []
        for path in paths:
            raw, lab = loader(path)
            signals.append(raw)
            labels.append(lab)
        return cls.from_arrays(signals, labels, device)

    @classmethod
    def from_tables(cls, signals, batch, device=None, kmer=5):
        """Reads that come with their tables instead of labels: ``signals[r]`` is read r's raw signal (its first ``final_signal``
        samples are kept, as the reference's collect_examples.py saves them) and ``batch`` a ``labelling.EventBatch`` (resquiggled
        reads, labelled with k-mer size ``kmer``) or ``labelling.MoveBatch`` (base-called reads; ``n_raw`` must not exceed the
        signals' lengths) over the same reads.  On a GPU (``labelling.label_device``: ``device`` a CUDA device, or None where one is
        there and the native library is built) the batch's entry point makes the labels and the base map: signal, labels and base
        map are the set's device arrays from then on (one upload) and labels and base map are copied back once for ``self.labels``
        / ``self.basemap``.  Otherwise (``device="cpu"``, or no GPU) ``batch.label_host`` makes them -- the same bytes."""
        from . import labelling
        from .base_votes import BaseTable
        kmer = batch.k_of(kmer)
        signals = [np.asarray(s).reshape(-1) for s in signals]
        if len(signals) != batch.n_reads:
            raise ValueError("%d signals but %d reads with tables" % (len(signals), batch.n_reads))
        offsets = np.asarray(batch.sample_offsets, dtype=np.int64).copy()
        signal = np.zeros(int(offsets[-1]), dtype=np.float32)
        for r, s in enumerate(signals):
            o, n = int(offsets[r]), int(offsets[r + 1] - offsets[r])
            if len(s) < n:
                raise ValueError("read %d: the labels cover %d samples, the raw signal has %d" % (r, n, len(s)))
            signal[o:o + n] = s[:n]
        bases = BaseTable.from_batch(batch)
        on_card = labelling.label_device(device)
        if on_card is None:
            labels, basemap = batch.label_host(kmer, base_map=True)
            return cls(signal, labels, offsets, device, basemap, bases)
        import torch
        labels_dev, basemap_dev, _tables = labelling.label_on_card(batch, kmer, on_card, base_map=True)
        back = lambda t: t.cpu().numpy() if t.numel() else np.zeros(0, np.uint8)     # noqa: E731
        vset = cls(signal, back(labels_dev), offsets, device, back(basemap_dev), bases)
        if signal.size:
            vset._dev = {"device": on_card, "signal": torch.from_numpy(signal).to(on_card), "labels": labels_dev, "basemap": basemap_dev,
                         "edges": torch.from_numpy(bases.edges).to(on_card)}
            vset.uploads = 1
        return vset

    @classmethod
    def from_source(cls, paths, source, device=None):
        """The reads of ``paths``, in that order, as ``source`` (a ``labelling.LabelSource``) says they are stored: labelled reads
        through ``from_npz``, event and move files (``source.load``) through ``from_tables``."""
        if not source.has_tables:
            return cls.from_npz(paths, device=device)
        reads = [source.load(path) for path in paths]
        return cls.from_tables([read["raw"] for read in reads], source.batch(reads), device, source.kmer)

    @classmethod
    def from_events(cls, signals, batch, kmer=5, device=None):
        return cls.from_tables(signals, batch, device, kmer)

    @classmethod
    def from_moves(cls, signals, batch, device=None):
        return cls.from_tables(signals, batch, device)

    @classmethod
    def from_event_npz(cls, paths, kmer=5, device=None):
        from .labelling import LabelSource
        return cls.from_source(paths, LabelSource("events", kmer), device)

    @classmethod
    def from_move_npz(cls, paths, device=None):
        from .labelling import LabelSource
        return cls.from_source(paths, LabelSource("moves"), device)

    @property
    def n_reads(self):
        return len(self.lengths)

    @property
    def labels_binary(self):
        """Whether every label of the set is 0 or 1 (what the border step needs); computed once and kept."""
        if self._binary is None:
            self._binary = not bool(np.any(np.asarray(self.labels) > 1))
        return self._binary

    # ------------------------------------------------------------------ one round on the host
    def select(self, window, max_seq_length, validation_start, max_number):
        """``train_validate.select_validation_stretches`` from the lengths alone: (read_index, first, length) int64 arrays.
        Same skip rule for reads shorter than the stretch, same stop at ``max_number``, same ValueError, and for "random"
        the same ``random.randint(0, room)`` calls on Python's global generator: one per long-enough read, in file order,
        none after the stop."""
        whole = validation_start == "complete"
        if not whole and validation_start != "random" and type(validation_start) != int:
            raise ValueError("validation_start must be an int, 'random' or 'complete'")
        n = max_seq_length // window * window
        picked = []
        for index, size in enumerate(self.lengths.tolist()):
            first, length = 0, size
            if not whole:
                room = size - n - (0 if validation_start == "random" else validation_start)
                if room < 0:
                    continue
                first = random.randint(0, room) if validation_start == "random" else validation_start
                first, stop, _ = slice(first, first + n).indices(size)          # raw[first:first + n] as Python slices it
                length = max(0, stop - first)
            picked.append((index, first, length))
            if len(picked) >= max_number:
                break
        table = np.array(picked, dtype=np.int64).reshape(-1, 3)
        return table[:, 0].copy(), table[:, 1].copy(), table[:, 2].copy()

    def pack(self, selection, window):
        """What the gather kernel writes, in numpy: (x float32 [sum N_i, window, 1], y uint8 [sum N_i * window], bounds,
        tails) -- ``train_validate.pack_validation_windows`` on the selected slices, with the labels kept as uint8."""
        read_index, first, length = selection
        bounds, tails = layout(length, window)
        x = np.zeros(int(bounds[-1]), dtype=np.float32)
        y = np.zeros(int(bounds[-1]), dtype=np.uint8)
        src = self.offsets[read_index] + first
        for b, s, n in zip(bounds[:-1].tolist(), src.tolist(), np.asarray(length).tolist()):
            x[b:b + n] = self.signal[s:s + n]
            y[b:b + n] = self.labels[s:s + n]
        return x.reshape(-1, window, 1), y, bounds, tails

    def pack_basemap(self, selection, window):
        """The base map of the selected stretches, packed like ``pack``'s ``y`` (uint8 [sum N_i * window], zero tails): what
        ``run_bases_host`` takes.  The card never makes this copy -- the kernel reads the set's base map in place.  ValueError for a
        set without one."""
        if self.basemap is None:
            raise ValueError("this set has no base map (only reads that come with event tables have one: from_events)")
        read_index, first, length = selection
        bounds, _tails = layout(length, window)
        out = np.zeros(int(bounds[-1]), dtype=np.uint8)
        src = self.offsets[read_index] + first
        for b, s, n in zip(bounds[:-1].tolist(), src.tolist(), np.asarray(length).tolist()):
            out[b:b + n] = self.basemap[s:s + n]
        return out

    def check_selection(self, selection):
        """Raise ValueError unless every stretch lies inside its read (the kernels index with these numbers)."""
        read_index, first, length = (np.asarray(a, dtype=np.int64) for a in selection)
        if not (read_index.shape == first.shape == length.shape and read_index.ndim == 1):
            raise ValueError("a selection is three int64 arrays of one length")
        if read_index.size and (read_index.min() < 0 or read_index.max() >= self.n_reads):
            raise ValueError("selection names a read that is not in the set")
        if np.any(first < 0) or np.any(length < 0) or np.any(first + length > self.lengths[read_index]):
            raise ValueError("selection reaches outside a read")
        return read_index, first, length

    score_host = staticmethod(score_host)
    run_states_host = staticmethod(run_states_host)
    run_borders_host = staticmethod(run_borders_host)
    run_bases_host = staticmethod(run_bases_host)
    curve_host = staticmethod(curve_host)
    run_scores_host = staticmethod(run_scores_host)
    finish = staticmethod(finish)
    layout = staticmethod(layout)

    # ------------------------------------------------------------------ the card's side
    def device_arrays(self, device=None):
        """(signal float32 [max(total, 1)], labels uint8 [max(total, 1)]) on ``device``; uploaded on the first call -- with the base
        map, when the set has one (``device_basemap``)."""
        import torch
        device = torch.device((self.device or "cuda") if device is None else device)
        if device.type != "cuda":
            raise ValueError("device_arrays: the reads go to a GPU")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev["device"] != device:
            up = lambda a, dt: torch.from_numpy(a if a.size else np.zeros(1, dt)).to(device)     # noqa: E731
            self._dev = {"device": device, "signal": up(self.signal, np.float32), "labels": up(self.labels, np.uint8)}
            if self.basemap is not None:
                self._dev["basemap"] = up(self.basemap, np.uint8)
            if self.bases is not None:
                self._dev["edges"] = torch.from_numpy(self.bases.edges).to(device)
            self.uploads += 1
        return self._dev["signal"], self._dev["labels"]

    def device_basemap(self, device=None):
        """The base map uint8 [max(total, 1)] on ``device`` (it goes up with ``device_arrays``' one upload); ValueError for a set
        without one."""
        if self.basemap is None:
            raise ValueError("this set has no base map (only reads that come with event tables have one: from_events)")
        self.device_arrays(device)
        return self._dev["basemap"]

    def base_table(self, who="vote_bases"):
        """The set's ``base_votes.BaseTable``; ValueError (naming the caller) for a set without one or without a base map."""
        if self.bases is None or self.basemap is None:
            raise ValueError("%s needs a set with a base table (only reads that come with their event or move tables have one: "
                             "DeviceValidationSet.from_events / from_moves)" % who)
        return self.bases

    def device_edges(self, device=None):
        """The base table's ``edges`` int64 [n_bases + 1] on ``device`` (they go up with ``device_arrays``' one upload); ValueError
        for a set without a table."""
        self.base_table("device_edges")
        self.device_arrays(device)
        return self._dev["edges"]
