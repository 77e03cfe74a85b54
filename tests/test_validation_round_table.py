"""The two tables a validation round is described by -- ``validation_round.OPTIONS`` (spec, plan, buffers, launches) and
``train_validate.REPORTS`` (network attributes, refusals, sweep fields, JSONL files) -- against what the hand-written ladders they
replace planned and reported: tests/golden/validation_round_plans.json and validation_round_reports.json were recorded with
``plans_now`` and ``reports_now`` below at the commit each file names, before the tables existed.  No GPU."""
import hashlib
import inspect
import itertools
import json
import os
import re

import numpy as np
import pytest

from catfish_amd import labelling
from catfish_amd import train_validate as tv
from catfish_amd import validation_round
from catfish_amd.device_validation import DeviceValidationSet
from catfish_amd.validation_round import EXTRA_RESULTS, RESULTS, SCORE_RESULTS, VOTE_RESULTS, RoundPlan, RoundSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPTION_VALUES = (("run_edges", (35, 70)), ("border_reach", 8), ("curve_shift", 10), ("max_bases", 4), ("vote_bases", 6), ("score_shift", 14))
OPTION_NAMES = tuple(name for name, _value in OPTION_VALUES)
LENGTHS, WINDOW, N_BASES = (70, 36, 1), 35, 40
THRESHOLDS = {1: (0.5,), 20: tuple(np.linspace(0.05, 0.95, 20).tolist())}


# --------------------------------------------------------------------------------------------------------------------------- plans
def plan_record(k, phases, options):
    """What ``RoundPlan`` decides, as JSON: ``need``; ``layout``, one ``[name, offset, cells, shape]`` per key of ``offset`` in its order
    (shape: that of the named result of ``results(arange(out_cells))``, null for a result that has its keys without being asked for);
    ``out_cells``; ``run_work``."""
    plan = RoundPlan(RoundSpec.of(THRESHOLDS[k], phases=phases, **options), np.array(LENGTHS, dtype=np.int64), WINDOW, N_BASES)
    assert list(plan.cells) == list(plan.offset)
    got = plan.results(np.arange(plan.out_cells, dtype=np.int64))
    named = {name: getattr(got, name) for name in RESULTS + EXTRA_RESULTS + VOTE_RESULTS + SCORE_RESULTS}
    assert [id(item) for item in named.values() if item is not None] == [id(item) for item in got]      # the tuple: those asked for, in order
    assert set(plan.offset) >= {name for name, item in named.items() if item is not None}
    for name, item in named.items():                       # every result starts at its offset and is int64 (ce_sum: the doubles' bits)
        if item is not None:
            assert item.dtype == (np.float64 if name == "ce_sum" else np.int64)
            assert int(item.reshape(-1)[:1].view(np.int64)[0]) == plan.offset[name] and item.size == plan.cells[name]
    layout = [[name, plan.offset[name], plan.cells[name], None if named[name] is None else list(named[name].shape)] for name in plan.offset]
    return {"need": plan.need, "layout": layout, "out_cells": plan.out_cells, "run_work": plan.run_work}


def plans_now():
    """{case: ``plan_record``} for all 64 subsets of the six options (a case is named by one digit per option, in the order of
    ``OPTION_VALUES``, and the number of thresholds) at 1 and at 20 thresholds.  The voted plan of the same case, ``phases=(0, 17)``,
    differs by one key of ``need`` alone: its value is the record's ``tiling_samples``."""
    plans = {}
    for asked in itertools.product((False, True), repeat=len(OPTION_VALUES)):
        options = {name: value for (name, value), on in zip(OPTION_VALUES, asked) if on}
        for k in sorted(THRESHOLDS):
            plain, voted = plan_record(k, (0,), options), plan_record(k, (0, 17), options)
            assert list(voted["need"])[:-1] == list(plain["need"]) and list(voted["need"])[-1] == "tiling_samples"
            plain["tiling_samples"] = voted["need"].pop("tiling_samples")
            assert voted == {key: value for key, value in plain.items() if key != "tiling_samples"}
            plans["%s/%d" % ("".join(str(int(on)) for on in asked), k)] = plain
    return json.loads(json.dumps(plans))


def test_every_plan_is_the_recorded_one():
    with open(os.path.join(GOLDEN, "validation_round_plans.json")) as fh:
        golden = json.load(fh)
    assert len(golden["recorded_at_commit"]) == 40 and len(golden["plans"]) == 64 * 2
    got = plans_now()
    assert list(got) == list(golden["plans"])
    for case, want in golden["plans"].items():
        assert got[case] == want and list(got[case]["need"]) == list(want["need"]), case


def test_the_two_tables_have_the_same_rows_and_name_every_result():
    assert tuple(row.option for row in validation_round.OPTIONS) == OPTION_NAMES == tuple(tv.REPORTS)
    assert set(OPTION_NAMES) == set(RoundSpec._fields) - {"thresholds", "rule"}
    names = tuple(name for row in validation_round.OPTIONS for name in row.names)
    assert RESULTS + EXTRA_RESULTS + VOTE_RESULTS + SCORE_RESULTS == ("right", "ce_sum", "counts") + names
    assert names == ("run_states", "run_borders", "curve", "run_bases", "base_confusion", "base_vote_runs", "run_scores")
    assert [row.option for row in validation_round.OPTIONS if row.listed] == ["run_edges", "border_reach", "curve_shift"]
    assert [row.option for row in validation_round.OPTIONS if row.bridged] == ["run_edges", "border_reach", "max_bases", "score_shift"]
    assert [row.option for row in validation_round.OPTIONS if not row.per_threshold] == ["curve_shift"]


def test_the_ladders_are_gone():
    """No option is tested against None where the tables are walked."""
    ladder = re.compile(r"\b(%s)\b\s+is\s+(not\s+)?None" % "|".join(OPTION_NAMES))
    for walked in (validation_round.walk, RoundPlan.__init__, RoundPlan.results, tv.validate, tv.threshold_sweep, tv._checkpoint_round):
        source = inspect.getsource(walked)
        assert not ladder.search(source), (walked.__qualname__, ladder.search(source).group(0))


# ------------------------------------------------------------------------------------------------------------------------- reports
EVERYTHING = dict(OPTION_VALUES)
REFUSED = [dict([pair]) for pair in OPTION_VALUES]


class StubNetwork(object):
    """What ``validate``, ``threshold_sweep`` and ``_checkpoint_round`` ask of a network, without a card: a round is
    ``plan.results`` of a seeded buffer."""
    window, model_type, tp, fp, tn, fn = WINDOW, "Stub", 0, 0, 0, 0

    def __init__(self):
        self.rounds = []

    def save_network_to_model_path(self, step):
        pass

    def evaluate(self, x, y):
        return 0.5, 0.25

    def score_validation_device(self, vset, selection, thresholds=(0.5,), **options):
        self.rounds.append(dict(options))
        spec = RoundSpec.of(thresholds, **options)
        plan = RoundPlan(spec, selection[2], self.window, vset.bases.n_bases)
        return plan.results(np.random.default_rng(len(thresholds)).integers(0, 50, plan.out_cells, dtype=np.int64))


def stub_set():
    reads = [labelling.synthetic_event_read(400 + 150 * i, 50 + i, hp_fraction=0.3) for i in range(3)]
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in reads])
    return DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5, device="cpu")


def refusal(call):
    with pytest.raises(ValueError) as refused:
        call()
    return str(refused.value)


def reports_now(directory):
    """What the reporting side makes of one stubbed round with everything asked for and ``bridge_gap`` 3; files go to ``directory``."""
    vset, here = stub_set(), os.getcwd()
    os.chdir(directory)
    try:
        net = StubNetwork()
        rows = tv.threshold_sweep(net, vset, [0.3, 0.5], 0, bridge_gap=3, **{k: v for k, v in EVERYTHING.items() if k != "curve_shift"})
        sweep_call = net.rounds.pop()
        validated = tv.validate(net, vset, 0, "some/dir/round", "complete", bridge_gap=3, **EVERYTHING)
        attributes = {name: [list(np.shape(value)), str(np.asarray(value).dtype), hashlib.sha256(np.asarray(value).tobytes()).hexdigest()]
                      for name, value in sorted(vars(net).items()) if name.startswith("validation_")}
        net = StubNetwork()
        for name, value in OPTION_VALUES:
            setattr(net, "validation_" + name, value)
        net.validation_bridge_gap = 3
        report = os.path.join(directory, "model.txt")
        batch_acc = tv._checkpoint_round(net, 40, None, None, report, (vset, 0, os.path.join(directory, "model"), "complete", 856))
        files = {}
        for name in sorted(os.listdir(directory)):
            if name.endswith(".jsonl"):
                with open(os.path.join(directory, name)) as fh:
                    files[name] = fh.read()
        plain = StubNetwork()
        tv.validate(plain, vset, 0, "some/dir/plain", "complete")
        tv.threshold_sweep(plain, vset, [0.5], 0)
    finally:
        os.chdir(here)
    refusals = {"paths " + ",".join(options): refusal(lambda: tv.validate(StubNetwork(), [], 0, "some/round", **options)) for options in REFUSED}
    refusals["validate bridge_gap"] = refusal(lambda: tv.validate(StubNetwork(), vset, 0, "some/round", bridge_gap=3, vote_bases=6, curve_shift=10))
    refusals["threshold_sweep bridge_gap"] = refusal(lambda: tv.threshold_sweep(StubNetwork(), vset, [0.5], 0, bridge_gap=3, vote_bases=6))
    calls = json.loads(json.dumps({"sweep": sweep_call, "checkpoint": net.rounds, "plain": plain.rounds}))
    return {"sweep_rows": json.dumps(rows), "validated": list(validated), "calls": calls, "attributes": attributes, "batch_acc": batch_acc,
            "files": files, "refusals": refusals}


def test_every_report_is_the_recorded_one(tmp_path):
    with open(os.path.join(GOLDEN, "validation_round_reports.json")) as fh:
        golden = json.load(fh)
    assert len(golden["recorded_at_commit"]) == 40
    got, want = reports_now(str(tmp_path)), golden["reports"]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the recording holds what it is there to guard: six files, bridge_gap in four of them, eight refusals, a sweep row of every kind
    assert sorted(want["files"]) == ["model_base_votes.jsonl", "model_curves.jsonl", "model_hp_bases.jsonl", "model_hp_borders.jsonl",
                                     "model_hp_scores.jsonl", "model_hp_states.jsonl"]
    assert sorted(name for name, text in want["files"].items() if '"bridge_gap": 3' in text) == [
        "model_hp_bases.jsonl", "model_hp_borders.jsonl", "model_hp_scores.jsonl", "model_hp_states.jsonl"]
    assert all(text.count("\n") == 1 and text.endswith("\n") for text in want["files"].values())
    assert len(want["refusals"]) == 8 and len(set(want["refusals"].values())) == 8
    assert {"hp_states", "hp_borders", "hp_bases", "base_confusion", "vote_runs", "hp_scores"} <= set(json.loads(want["sweep_rows"])[1])
    assert want["calls"]["plain"] == [{}, {}] and len(want["attributes"]) == 7
