"""Per-base calls on the host: ``base_votes`` (numpy, normative) -- the fixed point, a case worked by hand, the reference's own
``correct_events`` through tests/golden/base_votes_golden.npz, ``BaseTable`` and its refusals, the plan numbers of a round with
``vote_bases``, and the consistency of the two tables.  The batches the replay and the GPU tests share are built here."""
import os

import numpy as np
import pytest

from catfish_amd import base_votes as bv
from catfish_amd import device_validation as dv
from catfish_amd import labelling
from catfish_amd.device_validation import DeviceValidationSet
from catfish_amd.validation_round import EXTRA_RESULTS, RESULTS, VOTE_RESULTS, RoundPlan, RoundResult, RoundSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPE_THRESHOLDS = (0.5, 0.25, 0.75, 0.3, 0.9, 0.1, float(np.float32(0.1)), 0.0, 1.0, 0.5 + 1e-12, 0.5 - 1e-12,
                    float(np.nextafter(np.float32(0.5), np.float32(1.0))), float(np.nextafter(np.float32(0.5), np.float32(0.0))), 0.6, 0.7, 0.8,
                    0.125)                                 # 17: two launch groups


# ------------------------------------------------------------------------------------------------- batches shared with the other files
def set_of(reads):
    """``reads``: per read a list of events ``(letter, samples, truth)`` -> a host-only ``DeviceValidationSet`` with its base table.
    Only the FIRST sample of a base carries its truth; the others hold ``1 - truth`` (or 2), so a step that reads another sample
    shows."""
    labels, basemaps, edges, base_offsets, offsets = [], [], [0], [0], [0]
    for events in reads:
        for letter, n, truth in events:
            lab = np.full(n, 2 if n % 3 == 0 else 1 - truth, dtype=np.uint8)
            lab[0] = truth
            labels.append(lab)
            edges.append(edges[-1] + n)
        basemaps.append(labelling.base_map_host("".join(letter for letter, _n, _t in events), [n for _l, n, _t in events]))
        base_offsets.append(len(edges) - 1)
        offsets.append(edges[-1])
    labels, basemap = np.concatenate(labels), np.concatenate(basemaps)
    return DeviceValidationSet(np.zeros(labels.size, np.float32), labels, np.int64(offsets), "cpu", basemap,
                               bv.BaseTable(np.int64(edges), np.int64(base_offsets)))


def pack_probs(vset, selection, set_probs, window=35):
    """A round's packed probabilities from probabilities on the set's sample axis (the tails are zero) -> (packed float32, bounds)."""
    bounds, _tails = dv.layout(selection[2], window)
    packed = np.zeros(int(bounds[-1]), dtype=np.float32)
    for b0, s0, n in zip(bounds[:-1].tolist(), (vset.offsets[selection[0]] + selection[1]).tolist(), selection[2].tolist()):
        packed[b0:b0 + n] = set_probs[s0:s0 + n]
    return packed, bounds


def vote_of(vset, selection, packed, thresholds, max_bases, window=35, ranges=None):
    """``vote_host`` of a set's selection."""
    bounds, _tails = dv.layout(selection[2], window)
    return bv.vote_host(packed, vset.bases.edges, vset.labels, vset.basemap, vset.offsets[selection[0]] + selection[1], selection[2], bounds,
                        thresholds, max_bases, ranges)


def shape_batch():
    """Every launch shape and edge of the vote -> (vset, selection, packed probabilities).  Read 0: bases of 1, 2, 63, 64, 65 (the wave
    and its neighbours), ``LONG_BASE`` - 1 / + 0 / + 1 (where the whole wave takes a base over) and 4096 / 4097 / 4098 samples; read 1:
    one base; read 2: two neighbouring stretches that cut a called run of true bases; read 3: a stretch that starts and ends
    mid-event, with called bases at both ends of what it votes; read 4: a stretch that holds no whole event; read 5: a run of 33
    bases.  Letters ``A C G T N a``; probabilities with NaN, -1, 2 and means of exactly 0.5 / 0.25 / 0.75."""
    letters = "ACGTNa"
    sizes = (1, 2, 63, 64, 65, bv.LONG_BASE - 1, bv.LONG_BASE, bv.LONG_BASE + 1, 4096, 4097, 4098, 3, 1, 64)
    reads = [[(letters[i % 6], n, i % 2) for i, n in enumerate(sizes)],
             [("G", 7, 1)],
             [("C", 3 + i % 4, int(4 <= i < 16)) for i in range(24)],
             [(letters[i % 6], 5 + i % 3, int(i in (1, 2, 9, 10))) for i in range(12)],
             [("T", 50, 1), ("A", 4, 0)],
             [("T", 2, int(3 <= i < 36)) for i in range(40)]]
    vset = set_of(reads)
    edges, base_offsets = vset.bases.edges, vset.bases.base_offsets
    rng = np.random.default_rng(7)
    p = np.zeros(vset.bases.total, dtype=np.float32)
    for e, (a, b) in enumerate(zip(edges[:-1].tolist(), edges[1:].tolist())):
        mode = e % 5
        if mode == 0:
            p[a:b] = rng.uniform(0.55, 1.0, b - a)
        elif mode == 1:
            p[a:b] = rng.uniform(0.0, 0.45, b - a)
        elif mode == 2:
            p[a:b] = 0.5                                                           # a mean of exactly 0.5: called at 0.5
        elif mode == 3:
            p[a:b] = rng.integers(0, 257, b - a) / 256.0
        else:
            p[a:b] = np.where(np.arange(b - a) % 2 == 0, 0.25, 0.75)               # exactly 0.5 for an even count
    p[edges[3]:edges[4]] = 0.25                                                    # exactly 0.25, over one whole wave
    p[edges[9]:edges[10]] = 0.75                                                   # exactly 0.75, summed by the whole wave
    for r, (first, last, value) in {2: (2, 20, 0.9), 5: (3, 36, 0.95)}.items():    # called runs across the cut, and 33 bases long
        p[edges[base_offsets[r] + first]:edges[base_offsets[r] + last]] = value
    lo, hi = int(base_offsets[3]), int(base_offsets[4])
    p[edges[lo + 1]:edges[lo + 3]] = 0.99                                          # the first and last bases read 3's stretch votes
    p[edges[hi - 3]:edges[hi - 1]] = 0.99
    for at, value in ((0, np.nan), (4, -1.0), (5, 2.0), (int(edges[5]) + 9, np.nan), (int(edges[8]) + 70, 2.0), (int(edges[9]) + 4000, -1.0),
                      (int(edges[10]) + 1, np.inf), (int(edges[10]) + 2, -np.inf), (int(edges[10]) + 3, 1e-30)):
        p[at] = value
    size = np.diff(vset.offsets)
    cut = int(edges[base_offsets[2] + 10] - vset.offsets[2])                       # an event border inside the called run
    selection = (np.int64([0, 1, 2, 2, 3, 4, 5]), np.int64([0, 0, 0, cut, 3, 10, 0]),
                 np.int64([size[0], size[1], cut, size[2] - cut, size[3] - 3 - 4, 20, size[5]]))
    return vset, selection, pack_probs(vset, selection, p)[0]


def recipe_batch():
    """Three synthetic event reads labelled with k = 5, noisy probabilities around the labels -> (vset, selection, packed, reads)."""
    reads = [labelling.synthetic_event_read(n, seed) for n, seed in ((3000, 1), (2500, 2), (4000, 3))]
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in reads])
    vset = DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5, device="cpu")
    p = np.clip(0.7 * vset.labels + np.random.default_rng(0).normal(0.15, 0.25, vset.labels.size), 0, 1).astype(np.float32)
    selection = (np.int64([0, 1, 2]), np.int64([100, 0, 35]), np.int64([2800, 2500, 3500]))
    return vset, selection, pack_probs(vset, selection, p)[0], reads


RECIPE_THRESHOLDS = (0.3, 0.5, 0.9)


def assert_recipe_is_not_vacuous(confusion, runs):
    """Over the three thresholds every one of the four confusion cells is non-zero at least once, and so is every one of the three
    states of both kinds."""
    assert np.all(confusion.sum(axis=1).max(axis=0) > 0), confusion.sum(axis=1).tolist()
    assert np.all(runs.sum(axis=(3, 4)).max(axis=0) > 0), runs.sum(axis=(3, 4)).tolist()


# ---------------------------------------------------------------------------------------------------------------------------- the tests
def test_q_of_the_edge_values():
    got = bv.q_of(np.float32([np.nan, -1, .5, 1, 2, 1e-30, np.inf]))
    assert got.dtype == np.uint64 and got.tolist() == [0, 0, 2 ** 31, 2 ** 32, 2 ** 32, 0, 2 ** 32]
    assert bv.q_of(np.float32([-0.0, -np.inf, 0.25, np.nextafter(np.float32(1), np.float32(0))])).tolist() == [0, 0, 2 ** 30, 2 ** 32 - 2 ** 8]
    assert bv.q_of(np.float32(0.1)) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))


def test_a_case_worked_by_hand():
    """Three events of 2, 1 and 3 samples on the 1/4 grid: S = 2^32, 3 * 2^30, 3 * 2^30.  At 0.5 event 0's mean IS the threshold and is
    called (S = q(0.5) * 2), event 2 is not (3 * 2^30 < 3 * 2^31); at 0.75 only event 1 is called -- its mean is the threshold again."""
    vset = set_of([[("A", 2, 1), ("A", 1, 1), ("C", 3, 0)]])
    probs = np.float32([0.25, 0.75, 0.75, 0.0, 0.25, 0.5])
    selection = (np.int64([0]), np.int64([0]), np.int64([6]))
    sums, state, confusion, runs = vote_of(vset, selection, np.concatenate((probs, np.zeros(29, np.float32))), (0.5, 0.75), 4)
    assert sums.dtype == np.uint64 and sums.tolist() == [2 ** 32, 3 * 2 ** 30, 3 * 2 ** 30]
    assert state.dtype == np.uint8 and state.tolist() == [[0x83, 0x83, 0x84], [0x82, 0x83, 0x84]]
    want = np.zeros((2, 5, 2, 2), np.int64)
    want[0, 0, 1, 1], want[0, 1, 0, 0] = 2, 1
    want[1, 0, 1, 1], want[1, 0, 1, 0], want[1, 1, 0, 0] = 1, 1, 1
    assert np.array_equal(confusion, want)
    want = np.zeros((2, 2, 3, 5, 5), np.int64)
    want[0, 0, 0, 0, 2] = want[0, 1, 0, 0, 2] = 1            # one true run of two A found completely; one called run, wholly true
    want[1, 0, 1, 0, 2] = want[1, 1, 0, 0, 1] = 1            # at 0.75 the true run is found in part; the called run of one base is true
    assert np.array_equal(runs, want)
    assert bv.mean_p(sums, vset.bases.edges).tolist() == [0.5, 0.75, 0.25]
    assert bv.calls_of(sums, state[0], vset.bases) == [[(0, 2, "A", 0.625)]] and bv.calls_of(sums, state[1], vset.bases) == [[(1, 1, "A", 0.75)]]
    assert bv.call_bases_host([probs], [b"AAC"], [[2, 1, 3]], 0.5) == [[(0, 2, "A", 0.625)]]
    rates = bv.base_vote_rates(confusion[1])
    assert rates["voted_bases"] == 3 and rates["base_precision"] == 1 and rates["base_recall"] == 0.5 and rates["base_recall_by_base"] == [0.5, 0, 0, 0, 0]


def test_the_reference_loop_votes_the_same_bases_the_same_way():
    """tests/golden/base_votes_golden.npz: the classes ``correct_events`` printed (start 0; the whole read, and five samples less, where
    the last event is dropped) are the called bits at 0.5, and its count is the number of voted bases."""
    with np.load(os.path.join(GOLDEN, "base_votes_golden.npz")) as z:
        g = {key: z[key] for key in z.files}
    assert g["length"].size == 10
    dropped = 0
    for c in range(g["length"].size):
        lengths = g["event_lengths"][g["event_offsets"][c]:g["event_offsets"][c + 1]]
        bases = g["event_bases"][g["event_offsets"][c]:g["event_offsets"][c + 1]]
        scores = g["scores"][g["score_offsets"][c]:g["score_offsets"][c + 1]]
        classes = g["classes"][g["class_offsets"][c]:g["class_offsets"][c + 1]]
        edges = np.concatenate(([0], np.cumsum(lengths)))
        basemap = labelling.base_map_host(bases, lengths)
        sums, state, confusion, _runs = bv.vote_host(scores, edges, np.zeros(scores.size, np.uint8), basemap, [0], [g["length"][c]], [0], (0.5,), 16)
        voted = (state[0] & bv.VOTED) != 0
        assert int(voted.sum()) == int(g["count"][c]) == classes.size and voted[:classes.size].all()
        assert np.array_equal(state[0][voted] & bv.CALLED, classes)
        assert np.array_equal((state[0][voted] >> 2) & 7, bv.base_classes(bases[:classes.size])) and confusion.sum() == classes.size
        assert not np.any(sums[voted] * 2 == bv.ONE * lengths[voted].astype(np.uint64))      # no tie: there ``round`` and the vote differ
        dropped += int(classes.size < lengths.size)
    assert dropped == 5


def test_base_tables_from_events_and_moves():
    from test_label_moves_host import kmers_with_runs, table_of
    reads = [labelling.synthetic_event_read(700 + 40 * i, 30 + i, hp_fraction=0.3) for i in range(3)]
    batch = labelling.EventBatch.from_reads([(bases, lengths, (1, 2)) for _raw, bases, lengths in reads])
    table = bv.BaseTable.from_events(batch)
    assert table.edges.dtype == np.int64 and table.n_bases == batch.n_events and table.total == batch.total
    assert np.array_equal(np.diff(table.edges), batch.lengths) and np.array_equal(table.base_offsets, batch.event_offsets)
    labels, basemap = batch.label_host(5, base_map=True)
    want = np.concatenate([labelling.event_classes_host(*batch.read(r)[:1], *batch.read(r)[2], 5) for r in range(3)])
    assert np.array_equal(labels[table.edges[:-1]], want) and np.array_equal(basemap[table.edges[:-1]] & 0x7f, batch.bases)
    vset = DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5, device="cpu")
    assert np.array_equal(vset.bases.edges, table.edges) and vset.uploads == 0
    # move tables: merged events, one read cut by n_raw inside an event, one cut so that whole merged events are left without a sample
    moves = [table_of([7, 3, 9, 2, 5, 8, 4, 6, 3, 7], kmers_with_runs(10, ((2, 4),)), np.float32, [0, 1, 0, 2, 0, 0, 1, 0, 0, 3]),
             table_of([40] * 12, kmers_with_runs(12, ((4, 6),)), np.float32, n_raw=300),
             table_of([4] * 50, kmers_with_runs(50, ((0, 2), (47, 50))), np.float64, [1] * 50, clipped=(1, 1))]
    for group in (moves[:2], moves[2:]):
        mbatch = labelling.MoveBatch.from_reads(group)
        mtable = bv.BaseTable.from_moves(mbatch)
        mlabels, mmap = mbatch.label_host(base_map=True)
        assert mtable.total == mbatch.total and np.array_equal(mtable.edges[mtable.base_offsets], mbatch.sample_offsets)
        for r in range(mbatch.n_reads):
            states, lengths, mv, clipped, n_raw = mbatch.read(r)
            heads, n_signals = labelling.merge_moves_host(lengths, mv)
            kept = int(np.count_nonzero(np.cumsum(n_signals) - n_signals < mbatch.final[r]))      # merged events with a sample left
            a, b = int(mtable.base_offsets[r]), int(mtable.base_offsets[r + 1])
            assert b - a == kept
            first = mtable.edges[a:b]
            assert np.array_equal(mlabels[first], labelling.move_classes_host(states, heads, *clipped)[:kept])
            assert np.array_equal(mmap[first] & 0x7f, states[heads, states.shape[1] // 2][:kept])
            assert np.array_equal(first - mbatch.sample_offsets[r], (np.cumsum(n_signals) - n_signals)[:kept])
    cut = labelling.MoveBatch.from_reads(moves[:2])
    assert cut.final[1] == 300 and cut.merged[1] > bv.BaseTable.from_moves(cut).base_offsets[2] - bv.BaseTable.from_moves(cut).base_offsets[1]
    mset = DeviceValidationSet.from_moves([np.zeros(int(n)) for n in cut.n_raw], cut, device="cpu")
    assert mset.bases.n_bases == bv.BaseTable.from_moves(cut).n_bases


def test_every_refusal():
    good = bv.BaseTable([0, 2, 5, 9], [0, 1, 3])
    assert good.n_bases == 3 and good.n_reads == 2 and good.total == 9
    assert bv.BaseTable([0], [0]).n_bases == 0
    for edges, base_offsets in (([1, 2, 5], [0, 2]), ([0, 2, 2, 9], [0, 3]), ([0, 5, 2, 9], [0, 3]), ([0, 2, 5, 9], [0, 2]), ([0, 2, 5, 9], [1, 3]),
                                ([0, 2, 5, 9], [0, 2, 1, 3]), ([0.0, 2.0], [0, 1]), ([], [0]), ([0, 2], []), ([[0, 2]], [0, 1]),
                                ([0, 2 ** 31], [0, 1])):
        with pytest.raises(ValueError):
            bv.BaseTable(edges, base_offsets)
    good.check_set([0, 2, 9])
    for offsets in ([0, 3, 9], [0, 2, 10], [0, 9], [0, 2, 5, 9]):
        with pytest.raises(ValueError):
            good.check_set(offsets)
    signal, labels = np.zeros(9, np.float32), np.zeros(9, np.uint8)
    with pytest.raises(ValueError):                        # a table of another set
        DeviceValidationSet(signal, labels, np.int64([0, 3, 9]), "cpu", np.zeros(9, np.uint8), good)
    bare = DeviceValidationSet(signal, labels, np.int64([0, 2, 9]), "cpu")
    for who in (lambda: bare.base_table("vote"), lambda: bare.device_edges()):
        with pytest.raises(ValueError, match="from_events / from_moves"):
            who()
    for bad in (0, 33, -1, True, 16.0, "16"):
        with pytest.raises(ValueError, match="vote_bases"):
            RoundSpec.of(vote_bases=bad)
        with pytest.raises(ValueError):
            bv.vote_host(np.zeros(9, np.float32), good.edges, labels, labels, [0], [9], [0], (0.5,), bad)
    assert RoundSpec.of().vote_bases is None and RoundSpec.of(vote_bases=np.int64(7)).vote_bases == 7
    with pytest.raises(ValueError, match="share a voted base"):
        bv.event_ranges(good.edges, [0, 2], [9, 7])
    a, b = bv.event_ranges(good.edges, [0, 1, 5, 6, 9], [2, 4, 4, 2, 0])
    assert a.tolist() == [0, 1, 2, 3, 3] and b.tolist() == [1, 2, 3, 3, 3]          # whole events only; none is not an error
    with pytest.raises(ValueError):
        bv.calls_of(np.zeros(2, np.uint64), np.zeros(3, np.uint8), good)
    with pytest.raises(ValueError):
        bv.call_bases_host([np.zeros(3, np.float32)], [b"AC"], [[2, 2]])
    with pytest.raises(ValueError):
        bv.base_vote_rates(np.zeros((5, 2), np.int64))
    from catfish_amd import train_validate as tv
    with pytest.raises(ValueError, match="vote_bases needs a DeviceValidationSet"):      # paths are scored on the host: no table, no vote
        tv.validate(object(), [], 0, "some/round", vote_bases=16)


def test_plan_numbers_of_a_round_with_the_votes():
    """Worked by hand: 70 / 36 / 1 samples at window 35 are 175 packed samples; the confusion table is 5 * 2 * 2 = 20 cells and the run
    table 2 * 3 * 5 * 17 = 510 cells per threshold at 16 bins; a set of 100 bases needs (8 + K) * 100 bytes of work, rounded up to 16."""
    lengths = np.array((70, 36, 1), dtype=np.int64)
    assert RESULTS == ("right", "ce_sum", "counts", "run_states", "run_borders", "curve") and EXTRA_RESULTS == ("run_bases",)
    assert VOTE_RESULTS == ("base_confusion", "base_vote_runs")
    all_on = dict(thresholds=(0.3, 0.5), run_edges=(35,), border_reach=32, curve_shift=14, phases=(0, 17), max_bases=16)
    without = RoundPlan(RoundSpec.of(**all_on), lengths, 35)
    plan = RoundPlan(RoundSpec.of(vote_bases=16, **all_on), lengths, 35, n_bases=100)
    assert without.out_cells == 196785 and tuple(without.offset) == RESULTS + EXTRA_RESULTS
    assert without.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 2, "run_cells": 24, "border_cells": 652, "run_work": 384,
                            "curve_cells": 195075, "tiling_samples": 455, "base_cells": 1020}
    assert plan.cells["base_confusion"] == 40 and plan.cells["base_vote_runs"] == 1020
    assert plan.offset["base_confusion"] == 196785 and plan.offset["base_vote_runs"] == 196825 and plan.out_cells == 196785 + 2 * (20 + 510)
    assert tuple(plan.offset) == RESULTS + EXTRA_RESULTS + VOTE_RESULTS
    assert {k: v for k, v in plan.need.items() if k not in ("vote_cells", "vote_work")} == without.need
    assert plan.need["vote_cells"] == 1060 and plan.need["vote_work"] == 1008          # (8 + 2) * 100 = 1000 -> 1008
    for name in RESULTS + EXTRA_RESULTS:
        assert plan.offset[name] == without.offset[name] and plan.cells[name] == without.cells[name]
    assert not set(VOTE_RESULTS) & (set(without.cells) | set(without.offset)) and RoundSpec.of(**all_on).vote_bases is None
    alone = RoundPlan(RoundSpec.of(vote_bases=16), lengths, 35, n_bases=0)
    assert alone.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 1, "vote_cells": 530, "vote_work": 16}
    assert alone.offset["base_confusion"] == 10 and alone.offset["base_vote_runs"] == 30 and alone.out_cells == 540 and "run_bases" not in alone.offset
    assert RoundPlan(RoundSpec.of(vote_bases=1, thresholds=(0.5,) * 20), lengths, 35, n_bases=7).need == {
        "samples": 175, "reads": 3, "slots": 3, "thresholds": 20, "vote_cells": 20 * (20 + 60), "vote_work": 176}       # 16 per group: 24 * 7 = 168
    assert bv.work_bytes(0, 1) == 16 and bv.work_bytes(1, 1) == 16 and bv.work_bytes(2, 8) == 32 and bv.work_bytes(100, 16) == 2400
    with pytest.raises(ValueError, match="n_bases"):
        RoundPlan(RoundSpec.of(vote_bases=16), lengths, 35)
    # a plan without the votes is what it was, with or without the argument
    plain, old = RoundPlan(RoundSpec.of(), lengths, 35, n_bases=100), RoundPlan(RoundSpec.of(), lengths, 35)
    assert plain.offset == old.offset and plain.cells == old.cells and plain.need == old.need and plain.out_cells == old.out_cells == 10
    # the new results come last, by name and by position
    back = np.arange(alone.out_cells, dtype=np.int64)
    got = alone.results(back)
    assert isinstance(got, RoundResult) and len(got) == 5 and got.base_confusion is got[3] and got.base_vote_runs is got[4]
    assert got.run_bases is None and got.curve is None
    assert got.base_confusion.shape == (1, 5, 2, 2) and np.array_equal(got.base_confusion.reshape(-1), back[10:30])
    assert got.base_vote_runs.shape == (1, 2, 3, 5, 17) and np.array_equal(got.base_vote_runs.reshape(-1), back[30:])
    both = RoundPlan(RoundSpec.of(max_bases=4, vote_bases=2), lengths, 35, n_bases=5)
    got = both.results(np.arange(both.out_cells, dtype=np.int64))
    assert len(got) == 6 and got.run_bases is got[3] and got.base_confusion is got[4] and got.base_vote_runs is got[5]
    old = RoundPlan(RoundSpec.of(), lengths, 35).results(back[:10])
    assert len(old) == 3 and old.base_confusion is None and old.base_vote_runs is None


def _truth_runs(vset, selection, state_k):
    """A direct run-length encoding of ``truth`` over the voted bases of every stretch."""
    a, b = bv.event_ranges(vset.bases.edges, vset.offsets[selection[0]] + selection[1], selection[2])
    count = 0
    for lo, hi in zip(a.tolist(), b.tolist()):
        assert np.all(state_k[lo:hi] & bv.VOTED)
        truth = vset.labels[vset.bases.edges[lo:hi]] == 1
        count += int(np.count_nonzero(np.diff(np.concatenate(([0], truth.astype(np.int8)))) == 1))
    return count, int((b - a).sum())


@pytest.mark.parametrize("batch", ("shape", "recipe"))
def test_the_tables_are_consistent(batch):
    vset, selection, packed = shape_batch() if batch == "shape" else recipe_batch()[:3]
    thresholds = SHAPE_THRESHOLDS if batch == "shape" else RECIPE_THRESHOLDS
    sums, state, confusion, runs = vote_of(vset, selection, packed, thresholds, 16)
    if batch == "recipe":
        assert_recipe_is_not_vacuous(confusion, runs)
        assert int(np.count_nonzero(state[0] & bv.VOTED)) == 973
        assert confusion.sum(axis=1).tolist() == [[[823, 100], [0, 50]], [[918, 5], [0, 50]], [[923, 0], [46, 4]]]
        assert runs.sum(axis=(3, 4))[0].tolist() == [[7, 0, 0], [4, 3, 85]] and runs.sum(axis=(3, 4))[2].tolist() == [[0, 4, 3], [4, 0, 0]]
    for k in range(len(thresholds)):
        true_runs, voted = _truth_runs(vset, selection, state[k])
        assert runs[k, 0].sum() == true_runs and confusion[k].sum() == voted == np.count_nonzero(state[k] & bv.VOTED)
        assert np.array_equal(confusion[k].sum(axis=2)[:, 1], confusion[0].sum(axis=2)[:, 1])           # truth does not depend on the threshold
        assert np.array_equal(state[k] & ~np.uint8(bv.CALLED), state[0] & ~np.uint8(bv.CALLED))
    assert np.all(sums[(state[0] & bv.VOTED) == 0] == 0)
    if batch == "shape":
        a, b = bv.event_ranges(vset.bases.edges, vset.offsets[selection[0]] + selection[1], selection[2])
        assert (b - a).tolist() == [14, 1, 10, 14, 10, 0, 40]                          # mid-event ends drop a base each; one stretch votes nothing
        assert runs[0, 1, :, :, 10:].sum() >= 2                                         # the called run across the cut is two runs of ten ...
        assert not runs[0, :, :, :, 16][..., None].sum() == 0                           # ... and the 33 bases land in the last bin
        one = vote_of(vset, selection, packed, thresholds[:1], 1)[3]
        assert one.shape[-1] == 2 and one[0, :, :, :, 0].sum() == 0 and np.array_equal(one.sum(axis=-1), runs[:1].sum(axis=-1))
        wide = vote_of(vset, selection, packed, thresholds[:1], 32)[3]
        assert wide[0, 0, :, 3, 32].sum() == 1 and wide[0, 1, :, 3, 32].sum() == 1      # 33 T, true and called
        assert len({int(c) for c in (state[0] >> 2) & 7}) == 5 and sums.max() > 4097 * 2 ** 31
