"""``device_validation.run_bases_host`` -- which homopolymers a round found, by base and by length in bases -- against the
reference's own Counters (tests/golden/run_bases_golden.json, made by executing networks/process_output.py's functions), and the
host-only parts around it: the checks, the rates, the set's base map and the plan of a round that asks for the table.  No GPU."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import labelling
from catfish_amd.device_validation import DeviceValidationSet
from catfish_amd.validation_round import EXTRA_RESULTS, RESULTS, RoundPlan, RoundResult, RoundSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# group -> (kind, states) of the table: true / called = every run of the kind; tp = called runs that are not absent, fp = called
# runs that are, fn = true runs that are (create_confdict)
GROUPS = {"true": (0, (0, 1, 2)), "called": (1, (0, 1, 2)), "tp": (1, (0, 1)), "fp": (1, (2,)), "fn": (0, (2,))}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "run_bases_golden.npz")) as z:
        arrays = {key: z[key] for key in ("scores", "labels", "basemap", "offsets")}
    with open(os.path.join(GOLDEN, "run_bases_golden.json")) as fh:
        return arrays, json.load(fh)


def stretch_of(arrays, index):
    a, b = int(arrays["offsets"][index]), int(arrays["offsets"][index + 1])
    return arrays["scores"][a:b], arrays["labels"][a:b], arrays["basemap"][a:b], np.int64([0, b - a]), np.int64([b - a])


def cells_of(count_seq, max_bases):
    """The [5, max_bases + 1] cells a ``count_seq`` Counter stands for: a pure sequence "A" * n is cell [A, n], every other
    sequence of length n cell [other, n]; lengths from ``max_bases`` up are lumped."""
    out = np.zeros((5, max_bases + 1), dtype=np.int64)
    for seq, count in count_seq.items():
        pure = len(seq) >= 1 and seq[0] in "ACGT" and seq == seq[0] * len(seq)
        out["ACGT".index(seq[0]) if pure else 4, min(len(seq), max_bases)] += count
    return out


@pytest.mark.parametrize("max_bases", (1, 5, 16, 32))
def test_every_golden_counter_is_reproduced(golden, max_bases):
    arrays, book = golden
    assert book["groups"] == list(GROUPS) and tuple(book["classes"]) == dv.BASE_CLASSES
    seen = np.zeros((5, 5), dtype=np.int64)
    for case in book["cases"]:
        probs, y, basemap, bounds, lengths = stretch_of(arrays, case["stretch"])
        (table,) = dv.run_bases_host(probs, y, basemap, bounds, lengths, (case["threshold"],), max_bases, case["min_run"])
        for g, (group, (kind, states)) in enumerate(GROUPS.items()):
            got = table[kind][list(states)].sum(axis=0)
            want = cells_of(case["groups"][group]["seq"], max_bases)
            assert np.array_equal(got, want), (case["stretch"], case["threshold"], group)
            by_length = np.zeros(max_bases + 1, dtype=np.int64)
            for length, count in case["groups"][group]["bases"].items():
                by_length[min(int(length), max_bases)] += count
            assert np.array_equal(got.sum(axis=0), by_length)
            seen[g] += got.sum(axis=1)
    assert seen.min() >= 3                                 # every (group, class) pair


def test_the_table_sums_to_the_run_states(golden):
    from test_run_bases_replay import golden_base_batch, lumped, pack_base_stretches, planted_base_stretches
    for batch, options in ((golden_base_batch(), dict()), (golden_base_batch(), dict(min_run=1, max_gap=5)),
                           (pack_base_stretches(planted_base_stretches(4096)), dict())):
        probs, y, basemap, bounds, lengths = batch
        table = dv.run_bases_host(probs, y, basemap, bounds, lengths, (0.3, 0.5), 32, **options)
        states = dv.run_states_host(probs, y, bounds, lengths, (0.3, 0.5), (), **options)              # [K, 2, 1, 3]
        assert table.dtype == np.int64 and table.shape == (2, 2, 3, 5, 33) and table.sum() > 0
        assert np.array_equal(table.sum(axis=(3, 4)), states[:, :, 0, :])
        for max_bases in (1, 16):                          # fewer bins lump the upper ones
            assert np.array_equal(dv.run_bases_host(probs, y, basemap, bounds, lengths, (0.3, 0.5), max_bases, **options), lumped(table, max_bases))


def test_hand_cases_and_the_last_sample_rule():
    mark = lambda letter: 0x80 | ord(letter)               # noqa: E731
    n = 40
    y = np.zeros(n, np.uint8)
    y[10:n - 1] = 1                                        # the last one at n - 2: the run ends at n - 1
    basemap = np.full(n, ord("C"), np.uint8)
    basemap[[0, 9]] = mark("G")                            # outside
    basemap[[10, 20, n - 1]] = mark("C")                   # first sample, inside, and the sample the rule adds
    probs = np.where(y == 1, 0.9, 0.1).astype(np.float32)
    (table,) = dv.run_bases_host(probs, y, basemap, [0, n], [n], (0.5,), 16)
    assert table.sum() == 2 and table[0, 1, 1, 3] == 1 and table[1, 1, 1, 3] == 1          # C, three bases, either kind; incomplete: the other array is 0 at n - 1
    # the zero tail is ignored: a stretch packed at a larger size, with marks behind its end
    wide = np.concatenate((basemap, np.full(30, mark("T"), np.uint8)))
    (same,) = dv.run_bases_host(np.concatenate((probs, np.full(30, 0.9, np.float32))), np.concatenate((y, np.ones(30, np.uint8))), wide,
                                [0, 70], [n], (0.5,), 16)
    assert np.array_equal(same, table)
    for byte, cls in ((mark("A"), 0), (mark("T"), 3), (mark("N"), 4), (mark("a"), 4), (0x80, 4)):
        basemap[20] = byte
        basemap[[10, n - 1]] = byte if cls < 4 else mark("C")
        (table,) = dv.run_bases_host(probs, y, basemap, [0, n], [n], (0.5,), 2)
        assert table[0, 1, cls, 2] == 1 and table[0].sum() == 1
    none = np.full(n, ord("A"), np.uint8)                  # base bytes without a mark are no bases
    (table,) = dv.run_bases_host(probs, y, none, [0, n], [n], (0.5,), 16)
    assert table[0, 1, 4, 0] == 1 and table[1, 1, 4, 0] == 1 and table.sum() == 2
    empty = dv.run_bases_host(np.zeros(0, np.float32), np.zeros(0, np.uint8), np.zeros(0, np.uint8), [0, 0, 0], [0, 0], (0.5, 0.6), 7)
    assert empty.shape == (2, 2, 3, 5, 8) and not empty.any()


def test_max_bases_is_checked():
    assert dv.BASE_CLASSES == ("A", "C", "G", "T", "other")
    assert dv.check_max_bases(1) == 1 and dv.check_max_bases(np.int64(32)) == 32
    for bad in (0, 33, -1, True, False, 2.0, "16", None):
        with pytest.raises(ValueError, match="max_bases must be an int in 1 .. 32"):
            dv.check_max_bases(bad)
        if bad is not None:
            with pytest.raises(ValueError):
                RoundSpec.of(max_bases=bad)
    with pytest.raises(ValueError):
        dv.run_bases_host(np.zeros(1, np.float32), np.zeros(1, np.uint8), np.zeros(1, np.uint8), [0, 1], [1], (0.5,), 0)
    with pytest.raises(ValueError):
        dv.run_bases_host(np.zeros(1, np.float32), np.zeros(1, np.uint8), np.zeros(1, np.uint8), [0, 1], [1], (0.5,), 16, min_run=60, max_gap=5)


def test_rates_of_a_hand_table():
    table = np.zeros((2, 3, 5, 4), dtype=np.int64)
    table[0, 0, 0, 1] = 3                                  # true A runs of one base: 3 complete, 1 incomplete, 4 absent
    table[0, 1, 0, 1] = 1
    table[0, 2, 0, 1] = 4
    table[0, 0, 3, 3] = 2                                  # true T runs of three bases and more: 2 complete
    table[0, 2, 4, 0] = 5                                  # true runs without a base: all absent
    table[1, 0, 1, 2] = 6                                  # called: 6 pure, 2 other
    table[1, 2, 4, 2] = 2
    rates = dv.run_base_rates(table)
    assert rates["recall_by_base"] == [4 / 8, 0, 0, 1.0, 0] and rates["complete_by_base"] == [3 / 8, 0, 0, 1.0, 0]
    assert rates["recall_by_length"] == [0, 4 / 8, 0, 1.0] and rates["complete_by_length"] == [0, 3 / 8, 0, 1.0]
    assert rates["called_pure"] == 6 / 8
    nothing = dv.run_base_rates(np.zeros((2, 3, 5, 17), dtype=np.int64))
    assert nothing["called_pure"] == 0 and nothing["recall_by_base"] == [0] * 5 and nothing["recall_by_length"] == [0] * 17
    with pytest.raises(ValueError):
        dv.run_base_rates(np.zeros((2, 17, 3), dtype=np.int64))


def test_a_set_from_events_keeps_its_base_map():
    reads = [labelling.synthetic_event_read(700 + 36 * i, 40 + i) for i in range(3)]
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in reads])
    vset = DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5, device="cpu")
    labels, basemap = batch.label_host(5, base_map=True)
    assert vset.basemap.dtype == np.uint8 and np.array_equal(vset.basemap, basemap) and np.array_equal(vset.labels, labels)
    assert np.count_nonzero(vset.basemap & 0x80) == batch.n_events
    selection = (np.int64([2, 0]), np.int64([35, 0]), np.int64([501, 700]))
    x, y, bounds, tails = vset.pack(selection, 35)
    packed = vset.pack_basemap(selection, 35)
    assert packed.dtype == np.uint8 and packed.shape == y.shape
    for r, (read, first, n) in enumerate(zip(*selection)):
        b0, src = int(bounds[r]), int(vset.offsets[read] + first)
        assert np.array_equal(packed[b0:b0 + n], basemap[src:src + n]) and np.array_equal(y[b0:b0 + n], labels[src:src + n])
        assert not packed[b0 + n:int(bounds[r + 1])].any()
    # sets made from labelled reads have none, unless base maps come along
    plain = DeviceValidationSet.from_arrays([np.zeros(5), np.zeros(3)], [np.zeros(5, np.uint8), np.ones(3, np.uint8)])
    assert plain.basemap is None
    with pytest.raises(ValueError, match="no base map"):
        plain.pack_basemap((np.int64([0]), np.int64([0]), np.int64([5])), 35)
    with pytest.raises(ValueError, match="no base map"):
        plain.device_basemap()
    given = DeviceValidationSet.from_arrays([np.zeros(5), np.zeros(3)], [np.zeros(5, np.uint8), np.ones(3, np.uint8)],
                                            basemaps=[np.full(5, 65, np.uint8), np.full(3, 0x80 | 67, np.uint8)])
    assert given.basemap.tolist() == [65] * 5 + [0x80 | 67] * 3
    with pytest.raises(ValueError):
        DeviceValidationSet.from_arrays([np.zeros(5)], [np.zeros(5, np.uint8)], basemaps=[np.zeros(4, np.uint8)])
    with pytest.raises(ValueError):
        DeviceValidationSet(np.zeros(5, np.float32), np.zeros(5, np.uint8), np.int64([0, 5]), basemap=np.zeros(4, np.uint8))


def test_plan_numbers_of_a_round_with_the_table():
    """Worked by hand: 70 / 36 / 1 samples at window 35 are 2 / 2 / 1 windows, 175 packed samples; a table is 2 * 3 * 5 * 17 = 510
    cells per threshold at 16 bins."""
    lengths = np.array((70, 36, 1), dtype=np.int64)
    assert RESULTS == ("right", "ce_sum", "counts", "run_states", "run_borders", "curve") and EXTRA_RESULTS == ("run_bases",)
    all_on = dict(thresholds=(0.3, 0.5), run_edges=(35,), border_reach=32, curve_shift=14, phases=(0, 17))
    plan = RoundPlan(RoundSpec.of(max_bases=16, **all_on), lengths, 35)
    assert plan.cells["run_bases"] == 1020 and plan.offset["run_bases"] == 195765 and plan.out_cells == 196785
    assert tuple(plan.offset) == RESULTS + EXTRA_RESULTS
    assert plan.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 2, "run_cells": 24, "border_cells": 652, "run_work": 384,
                         "curve_cells": 195075, "tiling_samples": 455, "base_cells": 1020}
    alone = RoundPlan(RoundSpec.of(max_bases=16), lengths, 35)
    assert alone.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 1, "base_cells": 510, "run_work": 192}
    assert alone.offset["run_bases"] == 10 and alone.out_cells == 520 and alone.cells["curve"] == 0
    assert RoundPlan(RoundSpec.of(max_bases=1), lengths, 35).cells["run_bases"] == 60
    assert RoundPlan(RoundSpec.of(max_bases=32, thresholds=(0.5,) * 20), lengths, 35).cells["run_bases"] == 20 * 990
    # a plan without it is what it was
    without = RoundPlan(RoundSpec.of(**all_on), lengths, 35)
    assert RoundSpec.of(**all_on).max_bases is None
    assert without.offset == {"right": 0, "ce_sum": 3, "counts": 6, "run_states": 14, "run_borders": 38, "curve": 690}
    assert without.out_cells == 195765 and "base_cells" not in without.need and "run_bases" not in without.cells
    assert {k: v for k, v in plan.need.items() if k != "base_cells"} == without.need
    for name in RESULTS:
        assert plan.offset[name] == without.offset[name] and plan.cells[name] == without.cells[name]
    # the result comes last, by name and by position
    back = np.arange(alone.out_cells, dtype=np.int64)
    got = alone.results(back)
    assert isinstance(got, RoundResult) and len(got) == 4 and got.run_bases is got[3] and got.curve is None
    assert got.run_bases.shape == (1, 2, 3, 5, 17) and np.array_equal(got.run_bases.reshape(-1), back[10:])
    assert RoundPlan(RoundSpec.of(), lengths, 35).results(back[:10]).run_bases is None
