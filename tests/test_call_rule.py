"""``calling.CallRule``: the one place where the options of a call are checked.  Over a grid of good and bad values ``CallRule.of``
gives what the three checkers give -- the same fields, or the ValueError of the first one that refuses -- and the derived facts hold
at their edges."""
import itertools

import pytest

from catfish_amd import infer, tilings
from catfish_amd.calling import CallRule

MAX_GAPS = (None, 0, 3, 49, 50, -1, True, 2.5)
MIN_RUNS = (1, 15, 61, 64, 70)
PHASES = ((0,), (0, 17), (0, 12, 23), (0, 35), (1, 2), (0, 5, 5), ())
WEIGHTS = (None, "mean", "centre", "median")


def by_the_checkers(max_gap, min_run, phases, weight):
    """What the code before ``CallRule`` did, in its order -> (max_gap, phases, vote_weight), or the ValueError."""
    max_gap = infer.check_bridge(max_gap, min_run)
    phases = tilings.check_phases(phases)
    tilings.check_weight(weight)
    return max_gap, phases, "mean" if weight is None else weight


def test_the_grid_against_the_three_checkers():
    good = bad = 0
    for max_gap, min_run, phases, weight in itertools.product(MAX_GAPS, MIN_RUNS, PHASES, WEIGHTS):
        try:
            want = by_the_checkers(max_gap, min_run, phases, weight)
        except ValueError as exc:
            with pytest.raises(ValueError) as got:
                CallRule.of(0.5, min_run, max_gap, phases, weight)
            assert str(got.value) == str(exc), (max_gap, min_run, phases, weight)
            bad += 1
            continue
        rule = CallRule.of(0.5, min_run, max_gap, phases, weight)
        assert (rule.max_gap, rule.phases, rule.vote_weight) == want and type(rule.max_gap) is int
        assert (rule.threshold, rule.min_run, rule.scores) == (0.5, min_run, False)
        assert rule.n_tilings == len(want[1]) and rule.voted == (len(want[1]) > 1) and rule.bridged == (want[0] > 0)
        good += 1
    assert good >= 100 and bad >= 100
    # every kind of refusal is in the grid, each with its own text
    for args, text in (((50, 15), "min_run + max_gap <= 64"), ((3, 64), "min_run + max_gap <= 64"), ((-1, 15), "max_gap must be >= 0"),
                       ((True, 15), "max_gap must be an int"), ((2.5, 15), "max_gap must be an int")):
        with pytest.raises(ValueError, match=text.replace("+", r"\+")):
            CallRule.of(max_gap=args[0], min_run=args[1])
    for phases, text in (((0, 35), "every phase must be in"), ((1, 2), "first phase must be 0"), ((0, 5, 5), "strictly ascending"),
                         ((), "between 1 and 8")):
        with pytest.raises(ValueError, match=text):
            CallRule.of(phases=phases)
    with pytest.raises(ValueError, match="vote weight must be one of"):
        CallRule.of(vote_weight="median")
    with pytest.raises(ValueError, match="max_gap must be >= 0"):           # the first checker that refuses speaks
        CallRule.of(max_gap=-1, phases=(1, 2), vote_weight="median")
    with pytest.raises(ValueError, match="first phase must be 0"):
        CallRule.of(phases=(1, 2), vote_weight="median")


def test_defaults_and_immutability():
    rule = CallRule.of()
    assert rule == (0.5, 15, 0, (0,), "mean", False) and rule == CallRule.of(max_gap=None, phases=None, vote_weight=None)
    assert not rule.voted and not rule.bridged and not rule.scores_by_labels and rule.n_tilings == 1
    with pytest.raises(AttributeError):
        rule.max_gap = 3
    with pytest.raises(AttributeError):
        rule.extra = 1
    assert CallRule.of(phases=[0, 17]).phases == (0, 17)                       # a list comes back as the checked tuple


def test_derived_facts_at_their_edges():
    for scores, max_gap in itertools.product((False, True), (0, 1, 49)):
        rule = CallRule.of(max_gap=max_gap, scores=scores)
        assert rule.scores_by_labels is (scores and max_gap > 0)
    assert CallRule.of(max_gap=1, scores=1).scores_by_labels is True           # scores is a bool whatever was given
    for min_run in (1, 15, 64, 70):
        rule = CallRule.of(min_run=min_run)
        assert rule.max_runs(0) == 16
        for total in (1, min_run - 1, min_run, min_run + 1, 35, 4655, 2 ** 33 + 5):
            assert rule.max_runs(total) == total // min_run + 16
            # kept runs are at least min_run long with a gap between them: never more than the room
            assert (total + 1) // (min_run + 1) <= rule.max_runs(total)
    assert CallRule.of(min_run=1).max_runs(4655) == 4671 and CallRule.of(min_run=70).max_runs(4655) == 82
