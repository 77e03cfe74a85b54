"""``score_shift`` through the host-only half of a validation round (catfish_amd/validation_round.py): the checked option, its cells
behind the vote results, the doubled label work space, the named result -- and a round that does not ask, which plans what it planned
before.  Then the per-round JSON line of ``train_validate``'s checkpoint round, with the card's part stubbed.  No GPU."""
import json

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd import validation_round
from catfish_amd.validation_round import EXTRA_RESULTS, RESULTS, SCORE_RESULTS, VOTE_RESULTS, RoundPlan, RoundResult, RoundSpec
from test_run_states_host import packed, random_stretches

LENGTHS = (70, 36, 1)
WINDOW = 35
ALL_ON = dict(thresholds=(0.3, 0.5), run_edges=(35,), border_reach=32, curve_shift=14, phases=(0, 17))


def plan_of(lengths=LENGTHS, n_bases=None, **options):
    return RoundPlan(RoundSpec.of(**options), np.array(lengths, dtype=np.int64), WINDOW, n_bases)


def test_the_spec_checks_the_option_and_keeps_it_last():
    assert RoundSpec._fields[-1] == "score_shift" and RoundSpec.of().score_shift is None
    assert RoundSpec.of(score_shift=np.int64(14)).score_shift == 14 and type(RoundSpec.of(score_shift=np.int64(14)).score_shift) is int
    for bad in (13, 23, True, 16.0, "16"):
        with pytest.raises(ValueError, match=r"score shift must be an int in 14 \.\. 22"):
            RoundSpec.of(score_shift=bad)
    assert SCORE_RESULTS == ("run_scores",)
    assert RESULTS == ("right", "ce_sum", "counts", "run_states", "run_borders", "curve") and EXTRA_RESULTS == ("run_bases",)


def test_a_round_that_does_not_ask_plans_what_it_planned_before():
    """The literals are those of tests/test_validation_round_plan.py, from before the option existed."""
    plan = plan_of(**ALL_ON)
    assert plan.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 2, "run_cells": 24, "border_cells": 652, "run_work": 384,
                         "curve_cells": 195075, "tiling_samples": 455}
    assert plan.run_work == 384 and plan.out_cells == 195765
    assert plan.offset == {"right": 0, "ce_sum": 3, "counts": 6, "run_states": 14, "run_borders": 38, "curve": 690}
    assert plan.cells == {"right": 3, "ce_sum": 3, "counts": 8, "run_states": 24, "run_borders": 652, "curve": 195075}
    plain = plan_of()
    assert plain.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 1} and plain.out_cells == 10
    assert "run_scores" not in plain.cells and "run_scores" not in plain.offset
    assert sorted(vars(plan)) == ["bounds", "cells", "length", "longest", "n", "need", "offset", "out_cells", "run_work", "spec", "tails", "total"]


def test_the_cells_come_after_everything_else():
    per_k = 6 * (dv.curve_bins(16) + 1)
    assert dv.score_cells(16) == per_k == 97548
    base = plan_of(**ALL_ON)
    plan = plan_of(**ALL_ON, score_shift=16)
    assert plan.cells["run_scores"] == 2 * per_k and plan.offset["run_scores"] == base.out_cells
    assert plan.out_cells == base.out_cells + 2 * per_k
    assert {k: v for k, v in plan.offset.items() if k != "run_scores"} == base.offset
    assert plan.need == dict(base.need, score_cells=2 * per_k, run_work=2 * base.run_work) and plan.run_work == 768
    alone = plan_of(score_shift=14)                        # the labels and the paint: a round that asks for nothing else has them too
    assert alone.need == {"samples": 175, "reads": 3, "slots": 3, "thresholds": 1, "score_cells": 6 * 65026, "run_work": 384}
    assert alone.offset["run_scores"] == 10 and alone.out_cells == 10 + 6 * 65026
    voted = plan_of(n_bases=40, thresholds=(0.5,), max_bases=4, vote_bases=8, score_shift=22)
    assert list(voted.offset)[-4:] == list(EXTRA_RESULTS + VOTE_RESULTS + SCORE_RESULTS)
    assert voted.offset["run_scores"] == voted.offset["base_vote_runs"] + voted.cells["base_vote_runs"]
    assert voted.out_cells == voted.offset["run_scores"] + 6 * 256
    twenty = RoundPlan(RoundSpec.of(thresholds=(0.5,) * 20, score_shift=22), np.array(LENGTHS), WINDOW)
    assert twenty.run_work == 2 * 16 * 192 and twenty.cells["run_scores"] == 20 * 6 * 256


@pytest.mark.parametrize("k", (1, 2, 16))
def test_run_work_is_the_librarys_work_bytes(k):
    from catfish_amd import _native
    lib = _native.lib()
    spec = RoundSpec.of(thresholds=(0.5,) * k, score_shift=16)
    for total in (1, 63, 64, 65, 175, 2 ** 27):
        plan = RoundPlan(spec, np.array([total], dtype=np.int64), 1)          # window 1: no tail, total = the length
        assert plan.run_work == lib.cf_validation_run_scores_work_bytes(total, k) == 2 * lib.cf_validation_run_work_bytes(total, k)
    assert lib.cf_validation_run_scores_work_bytes(-1, 1) == -1 and lib.cf_validation_run_scores_work_bytes(0, 3) == 0


def test_results_cut_the_right_cells():
    plan = plan_of(thresholds=(0.3, 0.5), curve_shift=22, score_shift=22)
    back = np.arange(plan.out_cells, dtype=np.int64)
    got = plan.results(back)
    assert isinstance(got, RoundResult) and len(got) == 5 and got[-1] is got.run_scores and got[3] is got.curve
    assert got.run_scores.shape == (2, 2, 3, 256) and got.run_scores.dtype == np.int64 and not np.shares_memory(got.run_scores, back)
    assert np.array_equal(got.run_scores.reshape(-1), back[plan.offset["run_scores"]:]) and plan.offset["run_scores"] == 14 + 3 * 255
    assert np.array_equal(plan.cut(back, "run_scores"), back[-2 * 6 * 256:])
    without = plan_of(thresholds=(0.3, 0.5), curve_shift=22).results(back)
    assert len(without) == 4 and without.run_scores is None
    assert RoundResult(1, 2, 3).run_scores is None and RoundResult(1, 2, 3, run_scores=7)[-1] == 7


def test_the_grown_result_buffer_has_room_for_the_cells():
    torch = pytest.importorskip("torch")
    book = {"capacity": {}, "tensors": None, "allocations": 0}
    base, plan = plan_of(**ALL_ON), plan_of(**ALL_ON, score_shift=22)
    sized = validation_round.grow(book, base.need, "cpu")
    assert sized["out"].numel() == base.out_cells and sized["run_work"].numel() == 384
    sized = validation_round.grow(book, plan.need, "cpu")
    assert book["allocations"] == 2 and sized["out"].numel() == plan.out_cells and sized["run_work"].numel() == 768
    assert sized["out"].dtype == torch.int64
    validation_round.grow(book, base.need, "cpu")          # grow-only: the smaller round fits
    assert book["allocations"] == 2


class _Network(object):
    """What ``_checkpoint_round`` asks of a network, without a card."""
    validation_score_shift = 16

    def save_network_to_model_path(self, step):
        pass

    def evaluate(self, x, y):
        return 0.5, 0.25


def test_the_checkpoint_round_writes_one_json_line(tmp_path, monkeypatch):
    batch = packed(random_stretches(3, 6))
    table = dv.run_scores_host(*batch, (0.5,))[0]
    seen = {}

    def validate(network, *args, **options):
        seen.update(options)
        network.validation_run_scores = table
        return 0.9, 0.8, 0.7

    monkeypatch.setattr(tv, "validate", validate)
    report = str(tmp_path / "model.txt")
    assert tv._checkpoint_round(_Network(), 40, None, None, report, ("squiggles", 1050, "path", 0, 10)) == 0.5
    assert seen == {"score_shift": 16}
    with open(str(tmp_path / "model_hp_scores.jsonl")) as fh:
        (line,) = fh.read().splitlines()
    record = json.loads(line)
    assert record["step"] == 40 and record["threshold"] == 0.5 and record["shift"] == 16 and record["states"] == list(dv.RUN_STATES)
    want = json.loads(json.dumps(dv.run_score_summary(table, 16)))             # (tuples arrive as lists)
    assert [record["hp_scores"], record["called_scores"]] == want
    assert record["hp_scores"][0]["n"] > 0 and len(record["hp_scores"][0]["median"]) == 2
