"""``device_validation.run_borders_host`` -- the normative statement of the border step -- against the records written by the
reference's own hp_loc_dict / check_hp / correct_short (tests/golden/make_run_borders_golden.py) and against a plain per-run loop;
``split_run_borders`` and ``run_border_summary`` on hand-made tables; the refusals."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd.infer import correct_short

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "run_states_golden.npz")) as z:
        scores, labels, offsets = z["scores"], z["labels"], z["offsets"]
    with open(os.path.join(GOLDEN, "run_borders_golden.json")) as fh:
        cases = json.load(fh)["cases"]
    return scores, labels, offsets, cases


def table_of(runs, reach):
    """The [2, 5R+3] row of golden records [kind, start, end, l, r, gaps], by the cell rules of the issue."""
    row = np.zeros((2, 5 * reach + 3), dtype=np.int64)
    for kind, _s, _e, l, r, gaps in runs:
        row[kind, min(max(l, -reach), reach) + reach] += 1
        row[kind, 2 * reach + 1 + min(max(r, -reach), reach) + reach] += 1
        for g in gaps:
            row[kind, 4 * reach + 2 + min(g, reach) - 1] += 1
        row[kind, 5 * reach + 2] += 1 if gaps else 0
    return row


def plain_runs(mask, other):
    """Every non-absent run of ``mask`` as (s, e, l, r, gaps), sample by sample, from the definition."""
    n = len(mask)
    mask = list(mask)
    if n >= 2 and mask[-2] == 1:
        mask[-1] = 1
    out, i = [], 0
    while i < n:
        if mask[i] != 1:
            i += 1
            continue
        s = i
        while i + 1 < n and mask[i + 1] == 1:
            i += 1
        e = i
        i += 1
        if not any(other[s:e + 1]):
            continue
        if other[s]:
            l, j = 0, s - 1
            while j >= 1 and other[j]:
                l, j = l - 1, j - 1
        else:
            l = 0
            while not other[s + l]:
                l += 1
        if other[e]:
            r = 0
            while e + r + 1 < n and other[e + r + 1]:
                r += 1
        else:
            r = 0
            while not other[e + r]:
                r -= 1
        gaps, j = [], s
        while j <= e:
            if other[j]:
                j += 1
                continue
            a = j
            while j <= e and not other[j]:
                j += 1
            if a > s and j - 1 < e:
                gaps.append(j - a)
        out.append((s, e, l, r, gaps))
    return out


def test_the_golden_records_at_three_reaches(golden):
    scores, labels, offsets, cases = golden
    with open(os.path.join(GOLDEN, "run_states_golden.json")) as fh:                            # the same runs, less the absent ones
        states = json.load(fh)["cases"]
    assert [(c["stretch"], c["threshold"]) for c in cases] == [(c["stretch"], c["threshold"]) for c in states]
    assert [[run[:3] for run in c["runs"]] for c in cases] == [[run[:3] for run in c["runs"] if run[3] != 2] for c in states]
    assert sum(len(c["runs"]) for c in cases) == 264
    assert max(max(abs(run[3]), abs(run[4])) for c in cases for run in c["runs"]) > 64          # reach 64 clips
    for reach in (1, 64, 128):
        for case in cases:
            a, b = int(offsets[case["stretch"]]), int(offsets[case["stretch"] + 1])
            got = dv.run_borders_host(scores[a:b], labels[a:b], [0, b - a], [b - a], [case["threshold"]], reach, case["min_run"])
            assert got.shape == (1, 2, 5 * reach + 3) and got.dtype == np.int64
            assert np.array_equal(got[0], table_of(case["runs"], reach)), (reach, case["stretch"], case["threshold"])
    # ... and packed as a round packs them, two thresholds at once (the hand-made stretches have records at 0.5 only)
    for t in (0.3, 0.5, 0.9):
        mine = [c for c in cases if c["threshold"] == t]
        lengths = np.array([offsets[c["stretch"] + 1] - offsets[c["stretch"]] for c in mine], dtype=np.int64)
        bounds, _tails = dv.layout(lengths, 35)
        probs, y = np.full(int(bounds[-1]), 0.9, np.float32), np.zeros(int(bounds[-1]), np.uint8)
        for b0, c, n in zip(bounds[:-1].tolist(), mine, lengths.tolist()):
            a = int(offsets[c["stretch"]])
            probs[b0:b0 + n], y[b0:b0 + n] = scores[a:a + n], labels[a:a + n]
        want = sum(table_of(c["runs"], 64) for c in mine)
        assert np.array_equal(dv.run_borders_host(probs, y, bounds, lengths, (0.7, t), 64)[1], want)


def test_a_plain_loop_on_random_stretches_and_the_invariants():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(0, 201))
        truth = (np.cumsum(rng.random(n) < rng.choice([0.05, 0.2, 0.5])) & 1).astype(np.uint8)
        probs = np.where((np.cumsum(rng.random(n) < rng.choice([0.05, 0.2])) & 1) == 1, 0.9, 0.1).astype(np.float32)
        min_run = int(rng.choice([1, 3, 15]))
        reach = int(rng.choice([1, 5, 64, 128]))
        got = dv.run_borders_host(probs, truth, [0, n], [n], (0.5,), reach, min_run)
        want = np.zeros((2, 5 * reach + 3), dtype=np.int64)
        if n:
            pred = [int(v) for v in correct_short((probs.astype(np.float64) >= 0.5).astype(np.int64), min_run)]
            for kind, (mask, other) in enumerate(((truth.tolist(), pred), (pred, truth.tolist()))):
                want[kind] = table_of([[kind, s, e, l, r, gaps] for s, e, l, r, gaps in plain_runs(mask, other)], reach)[kind]
        assert np.array_equal(got[0], want), trial
        part = dv.split_run_borders(got, reach)
        assert np.array_equal(part["left"].sum(axis=-1), part["right"].sum(axis=-1))
        states = dv.run_states_host(probs, truth, [0, n], [n], (0.5,), (), min_run)
        assert np.array_equal(part["left"].sum(axis=-1), states[:, :, 0, 0] + states[:, :, 0, 1])
        assert np.all(part["interrupted"] <= part["gaps"].sum(axis=-1)) and np.all(part["interrupted"] <= part["left"].sum(axis=-1))


def test_split_and_summary_on_hand_made_tables():
    reach = 2                                              # cells: left 0..4 | right 5..9 | gaps 10..11 | interrupted 12
    table = np.arange(2 * 13, dtype=np.int64).reshape(1, 2, 13)
    part = dv.split_run_borders(table, reach)
    assert part["left"].tolist() == [[[0, 1, 2, 3, 4], [13, 14, 15, 16, 17]]] and part["right"][0, 0].tolist() == [5, 6, 7, 8, 9]
    assert part["gaps"][0, 1].tolist() == [23, 24] and part["interrupted"].tolist() == [[12, 25]]
    assert all(np.shares_memory(v, table) for v in part.values())
    row = np.zeros((2, 13), dtype=np.int64)
    row[0, :5] = (1, 0, 6, 2, 1)                           # left: offsets -2 (clip), 0 x 6, 1 x 2, 2 (clip): 10 runs
    row[0, 5:10] = (6, 0, 1, 3, 0)                         # right: six runs in the lower clip bin: the median falls into it
    row[0, 10:12] = (3, 1)
    row[0, 12] = 2
    hp, called = dv.run_border_summary(row, reach)
    assert hp == {"judged": 10, "exact_left": 0.6, "exact_right": 0.1, "median_left": 0, "median_right": None, "clipped": 0.8,
                  "interrupted": 0.2, "gaps": 4}
    assert called == {"judged": 0, "exact_left": 0, "exact_right": 0, "median_left": None, "median_right": None, "clipped": 0,
                      "interrupted": 0, "gaps": 0}
    row[1, :5] = (0, 1, 1, 1, 1)                           # lower median of four runs: the second
    row[1, 5:10] = (0, 0, 0, 1, 3)                         # the upper clip bin
    assert [dv.run_border_summary(row, reach)[1][key] for key in ("median_left", "median_right")] == [0, None]
    with pytest.raises(ValueError):
        dv.split_run_borders(table, 3)
    with pytest.raises(ValueError):
        dv.run_border_summary(row[:1], reach)


def test_refusals():
    probs, y = np.full(40, 0.9, np.float32), np.ones(40, np.uint8)
    for reach in (0, 129, True, 2.5, -1):
        with pytest.raises(ValueError):
            dv.run_borders_host(probs, y, [0, 40], [40], (0.5,), reach)
        with pytest.raises(ValueError):
            dv.check_border_reach(reach)
    assert dv.check_border_reach(np.int64(128)) == 128 and dv.border_cells(64) == 323
    with pytest.raises(ValueError):
        dv.run_borders_host(probs, y, [0, 40], [40], (0.5,), 64, min_run=0)
    bad = y.copy()
    bad[17] = 2
    with pytest.raises(ValueError):
        dv.run_borders_host(probs, bad, [0, 40], [40], (0.5,))
    assert dv.run_borders_host(probs, bad, [0, 18, 40], [17, 22], (0.5,)).sum() > 0          # the 2 sits in no stretch (a tail)
    assert dv.run_states_host(probs, bad, [0, 40], [40], (0.5,)).sum() > 0                   # the run states keep taking it
    flat = dv.DeviceValidationSet.from_arrays([probs, probs], [y, bad])
    assert flat.labels_binary is False and dv.DeviceValidationSet.from_arrays([probs], [y]).labels_binary is True
