"""``device_validation.run_scores_host`` -- the normative statement of the score step -- against the scores the reference's own
check_for_false_neg / main chains collect (tests/golden/make_run_scores_golden.py), against a plain per-sample loop, against the run
records of ``run_states_host`` and against ``curve_host``."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd.base_votes import q_of
from test_run_states_host import GOLDEN, golden, loop_records, packed, random_stretches

THRESHOLDS = (0.3, 0.5, 0.9)
ROWS = {"fn": ((0, 2),), "fp": ((1, 2),), "tp": ((1, 0), (1, 1))}      # create_confdict's names -> (kind, state) rows


@pytest.fixture(scope="module")
def golden_batch():
    scores, labels, offsets, _cases = golden()
    return [(scores[a:b], labels[a:b]) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]


@pytest.fixture(scope="module")
def golden_scores():
    with open(os.path.join(GOLDEN, "run_scores_golden.json")) as fh:
        return json.load(fh)


def histogram(values, shift):
    """float32 scores -> (counts int64 [NB], fixed-point sum)."""
    values = np.asarray(values, dtype=np.float32)
    nb = dv.curve_bins(shift)
    return np.bincount(dv.curve_bin(values.view(np.uint32), shift), minlength=nb).astype(np.int64), int(q_of(values).astype(np.int64).sum())


@pytest.mark.parametrize("shift", [14, 16, 22])
def test_the_reference_scores(golden_batch, golden_scores, shift):
    assert tuple(golden_scores["thresholds"]) == THRESHOLDS
    nb = dv.curve_bins(shift)
    edges = np.concatenate((dv.curve_thresholds(shift).astype(np.float64), [1.0]))
    checked = {name: 0 for name in ROWS}
    for case in golden_scores["cases"]:
        stretch = golden_batch[case["stretch"]]
        table = dv.run_scores_host(*packed([stretch]), (case["threshold"],), shift, min_run=1 if case["route"] == "A" else 15)[0]
        for name, values in case["scores"].items():
            got = sum(table[kind, state] for kind, state in ROWS[name])
            counts, total = histogram(values, shift)
            assert np.array_equal(got[:nb], counts), (case["stretch"], case["threshold"], case["route"], name)
            assert int(got[nb]) == total
            if not values:
                continue
            checked[name] += 1
            n = len(values)
            assert abs(int(got[nb]) / (n << 32) - case["mean"][name]) <= 2.0 ** -31
            if len(ROWS[name]) == 1:                       # one row: the summary is that row's
                summary = dv.run_score_summary(table, shift)[ROWS[name][0][0]][ROWS[name][0][1]]
                assert summary["n"] == n and summary["mean"] == int(got[nb]) / (n << 32)
                low = summary["median"][0]
            else:
                low = float(edges[int(np.searchsorted(np.cumsum(got[:nb]), (n + 1) // 2))])
            upper = int(np.searchsorted(np.cumsum(got[:nb]), n // 2 + 1))      # the bin of the upper middle sample
            assert low <= case["median"][name] <= float(edges[upper + 1]), (case["stretch"], case["threshold"], name)
    assert checked["fn"] >= 62 + 62 and checked["tp"] >= 50 and checked["fp"] >= 3      # (62 non-empty "fn" lists on route A alone)


@pytest.mark.parametrize("min_run, thresholds, rows", [(15, (0.3, 0.5), 12), (1, THRESHOLDS, 18)])
def test_no_row_of_the_golden_batch_is_empty(golden_batch, min_run, thresholds, rows):
    table = dv.run_scores_host(*packed(golden_batch), thresholds, dv.RUN_SCORE_SHIFT, min_run)
    filled = table[..., :-1].sum(axis=-1)
    assert filled.size == rows and filled.min() >= 20, filled.tolist()


def loop_table(stretches, thresholds, shift, min_run):
    """The definition as a plain loop over the samples of every run."""
    nb = dv.curve_bins(shift)
    out = np.zeros((len(thresholds), 2, 3, nb + 1), dtype=np.int64)
    for scores, truth in stretches:
        for k, t in enumerate(thresholds):
            for kind, start, end, state in loop_records(scores, truth, t, min_run):
                for i in range(start, end + 1):
                    out[k, kind, state, int(dv.curve_bin(np.float32(scores[i]).view(np.uint32), shift))] += 1
                    out[k, kind, state, nb] += int(q_of(np.float32(scores[i])))
    return out


@pytest.mark.parametrize("shift, min_run", [(16, 15), (14, 1), (22, 3)])
def test_against_a_plain_loop(shift, min_run):
    stretches = random_stretches(11 + shift, 12, longest=300)
    odd = np.float32([0.0, 0.5, 1.0, np.nextafter(np.float32(0.5), np.float32(0.0)), np.nan, 1.5, -0.25, 0.75] * 5)
    stretches.append((odd, np.repeat(np.uint8([1, 0, 1, 2, 1]), 8)))
    got = dv.run_scores_host(*packed(stretches), THRESHOLDS, shift, min_run)
    assert np.array_equal(got, loop_table(stretches, THRESHOLDS, shift, min_run))
    assert got[..., :-1].sum() > 1000


def test_row_totals_are_the_run_lengths_of_the_run_states():
    stretches = random_stretches(5, 10, longest=150)
    batch = packed(stretches)
    table = dv.run_scores_host(*batch, THRESHOLDS)
    want = np.zeros((3, 2, 3), dtype=np.int64)
    for first in range(1, 151, 6):                         # edges first .. first + 6: bins 1 .. 6 hold the runs of exactly first .. first + 5
        states = dv.run_states_host(*batch, THRESHOLDS, tuple(range(first, first + 7)))
        want += (states[:, :, 1:7, :] * np.arange(first, first + 6).reshape(1, 1, 6, 1)).sum(axis=2)
    assert np.array_equal(table[..., :-1].sum(axis=-1), want) and np.count_nonzero(want) >= 12
    by_loop = np.zeros((3, 2, 3), dtype=np.int64)
    for scores, truth in stretches:
        for k, t in enumerate(THRESHOLDS):
            for kind, start, end, state in loop_records(scores, truth, t):
                by_loop[k, kind, state] += end - start + 1
    assert np.array_equal(want, by_loop)


def test_true_runs_over_all_states_are_the_label_one_row_of_the_curve():
    # where the last-sample rule does not fire (the sample before the last is no 1) every label-1 sample lies in exactly one true run
    stretches = [(s, t) for s, t in random_stretches(8, 30) if len(t) < 2 or t[-2] != 1]
    assert len(stretches) >= 8
    batch = packed(stretches)
    for shift in (14, 16):
        table = dv.run_scores_host(*batch, (0.5, 0.9), shift)
        curve = dv.curve_host(*batch, shift)
        for k in range(2):
            assert np.array_equal(table[k, 0, :, :-1].sum(axis=0), curve[0])
        assert curve[0].sum() > 500


def test_the_summary_of_a_known_row():
    shift = 16
    nb = dv.curve_bins(shift)
    values = np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 1.0])
    table = np.zeros((2, 3, nb + 1), dtype=np.int64)
    table[0, 2, :nb], table[0, 2, nb] = histogram(values, shift)
    summary = dv.run_score_summary(table, shift)
    assert summary[1][0] == {"n": 0, "mean": None, "q1": None, "median": None, "q3": None}
    row = summary[0][2]
    assert row["n"] == 8 and abs(row["mean"] - float(values.astype(np.float64).mean())) <= 2.0 ** -32
    for name, sample in (("q1", 0.2), ("median", 0.4), ("q3", 0.6)):      # the lower quantile samples: 2nd, 4th and 6th of 8
        low, high = row[name]
        assert low <= np.float32(sample) < high and high - low <= 2.0 ** -7 * high
    table[0, 2, :nb], table[0, 2, nb] = histogram(np.float32([1.0, 1.0]), shift)
    assert dv.run_score_summary(table, shift)[0][2]["median"] == (1.0, 1.0)       # the top bin: exactly 1.0 and what is clamped into it
    with pytest.raises(ValueError):
        dv.run_score_summary(table[:, :, :-1], shift)


@pytest.mark.parametrize("shift", [13, 23, 0, -1, True, False, 16.0, "16", None, np.float32(16)])
def test_score_shifts_that_are_refused(shift):
    with pytest.raises(ValueError):
        dv.check_score_shift(shift)
    with pytest.raises(ValueError):
        dv.run_scores_host(np.zeros(35, np.float32), np.zeros(35, np.uint8), np.int64([0, 35]), np.int64([35]), (0.5,), shift)


def test_score_shifts_that_are_taken():
    assert [dv.check_score_shift(s) for s in (14, np.int64(16), 22)] == [14, 16, 22]
    assert dv.RUN_SCORE_SHIFT == 16 and dv.curve_bins(16) == 16257 and dv.score_cells(16) == 6 * 16258
    assert dv.run_scores_host(np.zeros(0, np.float32), np.zeros(0, np.uint8), np.int64([0, 0]), np.int64([0]), (0.5, 0.6)).shape == (2, 2, 3, 16258)
