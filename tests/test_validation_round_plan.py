"""The host-only half of a validation round (catfish_amd/validation_round.py): the checked options, the sizes and the layout of the
result buffer, and the named results -- everything ``RNN.score_validation_device`` decides before its first launch.  No GPU."""
import ast
import itertools

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import infer, validation_round
from catfish_amd.validation_round import RESULTS, RoundPlan, RoundResult, RoundSpec

LENGTHS = (70, 36, 1)
WINDOW = 35
ALL_ON = dict(thresholds=(0.3, 0.5), run_edges=(35,), border_reach=32, curve_shift=14, phases=(0, 17))


def plan_of(lengths=LENGTHS, **options):
    return RoundPlan(RoundSpec.of(**options), np.array(lengths, dtype=np.int64), WINDOW)


def test_the_module_imports_no_torch_at_module_level():
    for module in (validation_round, dv):
        with open(module.__file__) as fh:
            tree = ast.parse(fh.read())
        names = [alias.name for node in tree.body if isinstance(node, ast.Import) for alias in node.names]
        names += [node.module or "" for node in tree.body if isinstance(node, ast.ImportFrom)]
        assert not any(name.split(".")[0] == "torch" for name in names)
        assert "torch" not in vars(module)


def test_plan_numbers_of_a_round_with_everything_asked_for():
    """The literals are worked out by hand from the old inline arithmetic: 70 / 36 / 1 samples at window 35 are 2 / 2 / 1 windows."""
    plan = plan_of(**ALL_ON)
    assert plan.n == 3
    assert plan.bounds.tolist() == [0, 70, 140, 175] and plan.bounds.dtype == np.int64
    assert plan.tails.tolist() == [0, 34, 34]
    assert plan.total == 175 and plan.longest == 70
    assert plan.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 2, "run_cells": 24, "border_cells": 652, "run_work": 384,
                         "curve_cells": 195075, "tiling_samples": 455}
    assert plan.run_work == 384
    assert plan.offset == {"right": 0, "ce_sum": 3, "counts": 6, "run_states": 14, "run_borders": 38, "curve": 690}
    assert plan.out_cells == 195765
    assert tuple(plan.offset) == RESULTS


def test_a_result_not_asked_for_has_no_key_and_no_cells():
    full = plan_of(**ALL_ON)
    for option, key, name in (("run_edges", "run_cells", "run_states"), ("border_reach", "border_cells", "run_borders"),
                              ("curve_shift", "curve_cells", "curve")):
        plan = plan_of(**{k: v for k, v in ALL_ON.items() if k != option})
        assert key not in plan.need and {k: v for k, v in full.need.items() if k != key} == plan.need
        assert plan.cells[name] == 0 and plan.out_cells == full.out_cells - full.cells[name]
        for later in RESULTS[RESULTS.index(name) + 1:]:
            assert plan.offset[later] == full.offset[later] - full.cells[name]
        for earlier in RESULTS[:RESULTS.index(name) + 1]:
            assert plan.offset[earlier] == full.offset[earlier]
    plain = plan_of()
    assert plain.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 1} and plain.out_cells == 3 + 3 + 4
    assert "run_work" in plan_of(run_edges=()).need and "run_work" in plan_of(border_reach=1).need
    assert "tiling_samples" not in plan_of(**dict(ALL_ON, phases=(0,))).need
    assert plan_of(**dict(ALL_ON, phases=(0,))).out_cells == full.out_cells


def test_threshold_groups_and_the_work_of_one_group():
    spec = RoundSpec.of(thresholds=tuple(np.linspace(0.05, 0.95, 20)), run_edges=())
    assert spec.k_all == 20 and spec.groups == [(0, 16), (16, 20)]
    plan = RoundPlan(spec, np.array(LENGTHS), WINDOW)
    assert plan.run_work == 16 * 192 == plan.need["run_work"]
    assert RoundSpec.of().groups == [(0, 1)] and RoundSpec.of(thresholds=(0.5,) * 16).groups == [(0, 16)]
    assert RoundSpec.of(thresholds=(0.5,) * 33).groups == [(0, 16), (16, 32), (32, 33)]


def test_an_empty_round_still_asks_for_one_element():
    plan = plan_of(lengths=(0, 0), run_edges=(35,), border_reach=4)
    assert plan.total == 0 and plan.longest == 0
    assert plan.need["samples"] == 1 and plan.need["run_work"] == 1 and plan.run_work == 1
    assert plan.need["reads"] == 2 and plan.need["slots"] == 2


def test_the_selection_table_is_what_a_round_uploads():
    plan = plan_of(**ALL_ON)
    set_offsets = np.array([0, 100, 1000, 1100, 5000], dtype=np.int64)
    table = plan.table(set_offsets, np.array([3, 0, 1]), np.array([7, 0, 900]))
    assert table.dtype == np.int64 and table.shape == (3, 4)
    assert table.tolist() == [[1107, 0, 1000, 0], [70, 36, 1, 0], [0, 70, 140, 175]]


@pytest.mark.parametrize("asked", list(itertools.product((False, True), repeat=3)))
def test_results_cut_the_buffer_into_named_items(asked):
    runs, borders, curve = asked
    options = dict(thresholds=(0.3, 0.5), run_edges=(35,) if runs else None, border_reach=32 if borders else None,
                   curve_shift=14 if curve else None)
    plan = plan_of(**options)
    back = np.arange(plan.out_cells, dtype=np.int64)
    got = plan.results(back)
    assert isinstance(got, RoundResult) and isinstance(got, tuple) and len(got) == 3 + sum(asked)
    assert got.right is got[0] and got.ce_sum is got[1] and got.counts is got[2]
    at = 3
    for wanted, name, shape in ((runs, "run_states", (2, 2, 2, 3)), (borders, "run_borders", (2, 2, 163)), (curve, "curve", (3, 65025))):
        item = getattr(got, name)
        if not wanted:
            assert item is None
            continue
        assert item is got[at] and item.shape == shape and item.dtype == np.int64
        assert np.array_equal(item.reshape(-1), back[plan.offset[name]:plan.offset[name] + plan.cells[name]])
        at += 1
    assert at == len(got)
    assert got.right.dtype == np.int64 and got.right.tolist() == [0, 1, 2]
    assert got.ce_sum.dtype == np.float64 and got.ce_sum.shape == (3,)
    assert got.ce_sum.tobytes() == back[3:6].tobytes() and np.array_equal(got.ce_sum, back[3:6].view(np.float64))
    assert got.counts.dtype == np.int64 and got.counts.tolist() == [[6, 7, 8, 9], [10, 11, 12, 13]]
    for item in got:                                       # copies: the buffer is written again by the next round
        assert not np.shares_memory(item, back)
    right, ce_sum, counts = got[:3]                        # a tuple as before
    assert right is got.right and counts is got.counts and list(got)[1] is ce_sum


@pytest.mark.parametrize("k", (1, 2, 16))
def test_run_work_is_the_librarys_work_bytes(k):
    """``RoundPlan.run_work`` replaces ``cf_validation_run_work_bytes`` / ``cf_validation_run_borders_work_bytes``: same bytes."""
    from catfish_amd import _native
    lib = _native.lib()
    spec = RoundSpec.of(thresholds=(0.5,) * k, run_edges=())
    for total in (0, 1, 63, 64, 65, 175, 2 ** 31 - 1):
        plan = RoundPlan(spec, np.array([total], dtype=np.int64), 1)          # window 1: no tail, total = the length
        assert plan.total == total
        assert plan.run_work == max(lib.cf_validation_run_work_bytes(total, k), 1)
        assert plan.run_work == max(lib.cf_validation_run_borders_work_bytes(total, k), 1)
        assert plan.run_work == max(min(k, 16) * ((total + 63) // 64 * 64), 1)


def test_refusals_keep_their_texts():
    with pytest.raises(ValueError, match="score_validation_device: no threshold given"):
        RoundSpec.of(thresholds=())
    for reach in (0, 129, True, 2.5):
        with pytest.raises(ValueError, match=r"border reach must be an int in 1 \.\. 128, got %s" % repr(reach)):
            RoundSpec.of(border_reach=reach)
    with pytest.raises(ValueError, match=r"curve shift must be an int in 10 \.\. 22, got 9"):
        RoundSpec.of(curve_shift=9)
    with pytest.raises(ValueError, match=r"run edges must be positive and ascending, got \(70, 35\)"):
        RoundSpec.of(run_edges=(70, 35))
    for bad, check in ((dict(bridge_gap=50), lambda: infer.check_bridge(50, 15)), (dict(phases=(0, 35)), lambda: infer.check_phases((0, 35)))):
        with pytest.raises(ValueError) as direct:
            check()
        with pytest.raises(ValueError) as through:
            RoundSpec.of(run_edges=(), **bad)
        assert str(through.value) == str(direct.value)
    spec = RoundSpec.of(**ALL_ON, bridge_gap=3, vote_weight="centre")
    assert spec.thresholds == (0.3, 0.5) and spec.run_edges == (35,) and spec.border_reach == 32 and spec.curve_shift == 14
    assert spec.rule.max_gap == 3 and spec.rule.phases == (0, 17) and spec.rule.vote_weight == "centre" and spec.rule.min_run == 15
    assert dv.MAX_THRESHOLDS == 16
