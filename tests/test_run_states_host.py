"""``device_validation.run_states_host`` -- the normative statement of the run-state step -- against run records written by the
reference's own hp_loc_dict / check_hp / correct_short (tests/golden/make_run_states_golden.py) and against a plain double loop."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd.infer import correct_short

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    with np.load(os.path.join(GOLDEN, "run_states_golden.npz")) as z:
        scores, labels, offsets = z["scores"], z["labels"], z["offsets"]
    with open(os.path.join(GOLDEN, "run_states_golden.json")) as fh:
        cases = json.load(fh)["cases"]
    return scores, labels, offsets, cases


def table_of(records, edges=()):
    """Run records [kind, start, end, state] summed into the [2, B, 3] table."""
    out = np.zeros((2, len(edges) + 1, 3), dtype=np.int64)
    for kind, start, end, state in records:
        out[kind, int(np.searchsorted(np.asarray(edges, dtype=np.int64), end - start + 1, side="right")), state] += 1
    return out


def loop_records(scores, truth, threshold, min_run=15):
    """The definition as a plain loop over samples: [[kind, start, end, state], ...] of ONE stretch."""
    n = len(truth)
    if n == 0:
        return []
    pred = [int(v) for v in correct_short([1 if float(s) >= threshold else 0 for s in scores], min_run)]
    truth = [int(v) for v in truth]
    records = []
    for kind, (runs_in, other) in enumerate(((truth, pred), (pred, truth))):
        start = None
        for i in range(n):
            if start is None and runs_in[i] == 1:
                start = i
            if start is not None:
                if i + 1 == n:                             # an open run is closed AT the last sample, whatever it holds
                    end = i
                elif runs_in[i] != 1:
                    end = i - 1
                else:
                    continue
                inside = other[start:end + 1]
                state = 0 if all(v == 1 for v in inside) else 2 if all(v == 0 for v in inside) else 1
                records.append([kind, start, end, state])
                start = None
    return records


def random_stretches(seed, count, longest=400):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(0, longest + 1))
        walk = np.cumsum(rng.normal(0.0, 0.2, size=n)) + rng.normal(0.0, 0.4)
        z = 4.0 * walk + rng.normal(0.0, 0.8, size=n) + 2.5 * np.sin(np.arange(n) / 20.0 + rng.uniform(0.0, 6.28))
        out.append(((1.0 / (1.0 + np.exp(-z))).astype(np.float32), (walk > 0.0).astype(np.uint8)))
    return out


def packed(stretches, window=35):
    """Stretches laid out as a validation round packs them (zero tails up to the window multiple; the probabilities of a tail
    are set to 1 so that a tail taken for part of a stretch would show)."""
    lengths = np.array([len(s) for s, _ in stretches], dtype=np.int64)
    bounds, _tails = dv.layout(lengths, window)
    probs = np.ones(int(bounds[-1]), dtype=np.float32)
    y = np.zeros(int(bounds[-1]), dtype=np.uint8)
    for b, (s, t) in zip(bounds[:-1].tolist(), stretches):
        probs[b:b + len(s)] = s
        y[b:b + len(t)] = t
    return probs, y, bounds, lengths


def test_golden_records_of_the_reference():
    scores, labels, offsets, cases = golden()
    assert len(cases) > 100
    seen = np.zeros((2, 3), dtype=np.int64)
    for case in cases:
        a, b = int(offsets[case["stretch"]]), int(offsets[case["stretch"] + 1])
        want = table_of(case["runs"])
        got = dv.run_states_host(scores[a:b], labels[a:b], [0, b - a], [b - a], [case["threshold"]], (), case["min_run"])
        assert got.shape == (1, 2, 1, 3) and got.dtype == np.int64
        assert np.array_equal(got[0], want), case
        assert sorted(loop_records(scores[a:b], labels[a:b], case["threshold"], case["min_run"])) == sorted(case["runs"]), case
        edges = (2, 15, 16, 40)
        assert np.array_equal(dv.run_states_host(scores[a:b], labels[a:b], [0, b - a], [b - a], [case["threshold"]], edges)[0],
                              table_of(case["runs"], edges)), case
        seen += want[:, 0, :]
    assert seen.min() >= 3                                 # every (kind, state) pair is in the fixture
    # every threshold's cases as ONE packed batch (zero tails between the stretches)
    stretches = [(scores[a:b], labels[a:b]) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
    for t in (0.3, 0.5, 0.9):
        mine = [c for c in cases if c["threshold"] == t]
        assert len(mine) >= 40
        probs, y, bounds, lengths = packed([stretches[c["stretch"]] for c in mine])
        assert np.array_equal(dv.run_states_host(probs, y, bounds, lengths, (0.7, t))[1], sum(table_of(c["runs"]) for c in mine))


def test_the_hp_loc_dict_rule_and_the_hand_made_cases():
    one = lambda truth, called: dv.run_states_host(np.where(np.asarray(called) == 1, 0.9, 0.1).astype(np.float32),      # noqa: E731
                                                   np.asarray(truth, dtype=np.uint8), [0, len(truth)], [len(truth)], [0.5], (), 1)[0]
    # [0,1,1,0] gives the run (1, 3): judged over three samples, the last of which is not called
    assert one([0, 1, 1, 0], [0, 1, 1, 0]).tolist() == [[[0, 1, 0]], [[0, 1, 0]]]
    assert one([0, 1, 1, 1], [0, 1, 1, 1]).tolist() == [[[1, 0, 0]], [[1, 0, 0]]]
    # [0,1,0,1,0] gives (1, 1) and (3, 4)
    assert one([0, 1, 0, 1, 0], [0, 1, 0, 1, 1]).tolist() == [[[2, 0, 0]], [[1, 1, 0]]]
    assert sorted(loop_records(np.float32([.1, .9, .1, .9, .1]), [0, 1, 0, 1, 0], 0.5, 1)) == [[0, 1, 1, 0], [0, 3, 4, 1], [1, 1, 1, 0], [1, 3, 4, 1]]
    assert one([1], [0]).tolist() == [[[0, 0, 1]], [[0, 0, 0]]]
    assert one([0], [1]).tolist() == [[[0, 0, 0]], [[0, 0, 1]]]
    assert one([1, 0], [1, 0]).tolist() == [[[0, 1, 0]], [[0, 1, 0]]]                  # n - 2 = 0: the run is (0, 1)
    # a label other than 0 / 1 inside a called run: neither complete nor absent; and it is no true run
    assert one([0, 2, 0], [1, 1, 1]).tolist() == [[[0, 0, 0]], [[0, 1, 0]]]
    assert one([2, 2, 2], [1, 1, 1]).tolist() == [[[0, 0, 0]], [[0, 1, 0]]]
    # correct_short: a called run of 14 is erased, one of 15 is kept
    for size, want in ((14, [[[0, 0, 1]], [[0, 0, 0]]]), (15, [[[1, 0, 0]], [[1, 0, 0]]])):
        truth = [0] * 3 + [1] * size + [0] * 3
        got = dv.run_states_host(np.where(np.asarray(truth) == 1, 0.9, 0.1).astype(np.float32), np.uint8(truth), [0, len(truth)],
                                 [len(truth)], [0.5])
        assert got[0].tolist() == want
    # the comparison is score_host's: the float32 as a double against the double threshold
    p = np.full(20, np.float32(0.3), dtype=np.float32)     # float32(0.3) > 0.3
    assert dv.run_states_host(p, np.ones(20, np.uint8), [0, 20], [20], [0.3, float(np.float32(0.3)), 0.30000002])[:, 1, 0].tolist() == [
        [1, 0, 0], [1, 0, 0], [0, 0, 0]]


def test_equals_the_double_loop_on_random_stretches():
    stretches = random_stretches(11, 120)
    probs, y, bounds, lengths = packed(stretches)
    thresholds, edges = (0.3, 0.5, 0.9), (15, 35, 70)
    got = dv.run_states_host(probs, y, bounds, lengths, thresholds, edges)
    assert got.shape == (3, 2, 4, 3)
    for k, t in enumerate(thresholds):
        want = sum(table_of(loop_records(s, l, t), edges) for s, l in stretches)
        assert np.array_equal(got[k], want)
    assert got.sum(axis=(0, 2)).min() >= 1                 # every (kind, state) pair occurs


def test_bins_sum_to_the_unbinned_table():
    probs, y, bounds, lengths = packed(random_stretches(12, 60))
    whole = dv.run_states_host(probs, y, bounds, lengths, (0.5, 0.7), ())
    assert whole.shape == (2, 2, 1, 3)
    for edges in ((35,), (1, 2, 15, 16, 35, 70, 140)):
        binned = dv.run_states_host(probs, y, bounds, lengths, (0.5, 0.7), edges)
        assert binned.shape == (2, 2, len(edges) + 1, 3)
        assert np.array_equal(binned.sum(axis=2, keepdims=True), whole)
    seven = dv.run_states_host(probs, y, bounds, lengths, (0.5,), (1, 2, 15, 16, 35, 70, 140))[0]
    assert seven[:, 0].sum() == 0 and seven[1, :3].sum() == 0          # no run is shorter than 1, no called run shorter than 15


def test_a_stretch_adds_the_same_counts_wherever_it_stands():
    stretches = random_stretches(13, 30)
    thresholds, edges = (0.4, 0.6), (20, 50)
    alone = [dv.run_states_host(*packed([s]), thresholds, edges) for s in stretches]
    probs, y, bounds, lengths = packed(stretches)
    whole = dv.run_states_host(probs, y, bounds, lengths, thresholds, edges)
    assert np.array_equal(whole, sum(alone))
    order = np.random.default_rng(0).permutation(len(stretches))
    assert np.array_equal(dv.run_states_host(*packed([stretches[i] for i in order]), thresholds, edges), whole)
    ones = (np.ones(40, np.float32), np.ones(40, np.uint8))            # neighbours that would join a run across a boundary
    between = dv.run_states_host(*packed([ones, stretches[3], ones], window=1), thresholds, edges)
    assert np.array_equal(between, alone[3] + 2 * dv.run_states_host(*packed([ones]), thresholds, edges))


def test_zero_length_stretches():
    empty = (np.zeros(0, np.float32), np.zeros(0, np.uint8))
    some = random_stretches(14, 3)
    want = dv.run_states_host(*packed(some), (0.5,), (35,))
    assert np.array_equal(dv.run_states_host(*packed([empty, some[0], empty, empty, some[1], some[2], empty]), (0.5,), (35,)), want)
    none = dv.run_states_host(*packed([empty, empty]), (0.5, 0.6), (35,))
    assert none.shape == (2, 2, 2, 3) and not none.any()
    assert dv.run_states_host(np.zeros(0, np.float32), np.zeros(0, np.uint8), [0], [], (0.5,)).shape == (1, 2, 1, 3)


def test_bad_edges_are_refused():
    probs, y, bounds, lengths = packed(random_stretches(15, 2))
    for edges in ((0,), (-3, 5), (5, 5), (7, 3), (1, 2, 3, 4, 5, 6, 7, 8), (2.5,)):
        with pytest.raises(ValueError):
            dv.run_states_host(probs, y, bounds, lengths, (0.5,), edges)
        with pytest.raises(ValueError):
            dv.check_run_edges(edges)
    assert dv.check_run_edges([1, 2.0, np.int64(9)]) == (1, 2, 9)
    with pytest.raises(ValueError):
        dv.run_states_host(probs, y, bounds, lengths, (0.5,), (), min_run=0)


def test_rates():
    table = np.array([[[3, 1, 0], [1, 1, 2]], [[2, 2, 1], [0, 0, 0]]])
    assert dv.run_state_rates(table) == (4 / 8, 6 / 8, 1 / 5)
    assert dv.run_state_rates(np.zeros((2, 1, 3), dtype=np.int64)) == (0, 0, 0)
