"""Generate the run-state golden vectors by EXECUTING the reference's own pure-Python functions.

networks/process_output.py cannot be imported whole (matplotlib, the model classes), so the four function definitions the
offline evaluation is made of are extracted with ``ast`` and executed, as make_postproc_golden.py does:

  class_from_threshold (:572-582), hp_loc_dict (:614-643), check_hp (:814-895), correct_short (:1096-1123)

and chained the way its main loop chains them (:235-273): scores -> labels -> correct_short -> hp_loc_dict of prediction and
truth -> check_hp of every predicted run against the truth (:266) and of every true run against the prediction (:271).  The
reference reads its scores from a text dump, i.e. as Python floats; the float32 scores go in as the doubles they are.

Outputs (data only): tests/golden/run_states_golden.npz (float32 scores, uint8 labels, int64 offsets of the stretches) and
tests/golden/run_states_golden.json (per case: stretch, threshold, every run as [kind, start, end, state]; kind 0 = a true run
judged against the prediction, 1 = a predicted run judged against the truth; state 0 complete, 1 incomplete, 2 absent).
Run in the build container (needs /root/reference); the fixtures travel, the reference does not.
"""
import ast
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/networks/process_output.py"
STATES = {"complete": 0, "incomplete": 1, "absent": 2}
THRESHOLDS = (0.3, 0.5, 0.9)


def extract(path, names):
    with open(path) as fh:
        tree = ast.parse(fh.read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    ref = extract(REF, {"class_from_threshold", "hp_loc_dict", "check_hp", "correct_short"})
    rng = np.random.default_rng(20261018)

    def runs_of(scores, truth, threshold):
        """[[kind, start, end, state], ...] of one stretch, by the reference's functions."""
        if len(scores) == 0:
            return []                                      # (its correct_short indexes predictions[0])
        labels = ref["class_from_threshold"]([float(s) for s in scores], threshold)
        predicted = [int(v) for v in ref["correct_short"](labels)]
        truth = [int(v) for v in truth]
        predicted_hp, true_hp = ref["hp_loc_dict"](predicted), ref["hp_loc_dict"](truth)
        out = []
        for hp in true_hp.values():
            out.append([0, int(hp[0]), int(hp[1]), STATES[ref["check_hp"](hp, predicted, 0)[0]]])
        for hp in predicted_hp.values():
            out.append([1, int(hp[0]), int(hp[1]), STATES[ref["check_hp"](hp, truth, 0)[0]]])
        return out

    stretches = []                                         # (scores float32, truth uint8)
    for length in [0, 1, 2, 16, 35, 64, 65, 128, 300] + [int(v) for v in rng.integers(20, 301, size=31)]:
        # truth: a thresholded random walk; scores: the sigmoid of 4 x that walk + white noise + a slow drift
        walk = np.cumsum(rng.normal(0.0, 0.18, size=length)) + rng.normal(0.0, 0.4)
        truth = (walk > 0.0).astype(np.uint8)
        drift = 3.0 * np.sin(np.arange(length) / 25.0 + rng.uniform(0.0, 6.28))
        z = 4.0 * walk + rng.normal(0.0, 0.7, size=length) + drift
        stretches.append(((1.0 / (1.0 + np.exp(-z))).astype(np.float32), truth))

    def planted(truth, called=None):
        truth = np.asarray(truth, dtype=np.uint8)
        called = truth if called is None else np.asarray(called, dtype=np.uint8)
        return np.where(called == 1, np.float32(0.9), np.float32(0.1)).astype(np.float32), truth

    hand = [planted([0, 1, 1, 0]), planted([1, 0]), planted([0, 1, 0, 1, 0]), planted([1]), planted([0]),
            # a called run of 14 (erased by correct_short) and one of 15 (kept) over a true run of 31
            planted([0] * 3 + [1] * 31 + [0] * 3, [0] * 3 + [1] * 14 + [0] * 2 + [1] * 15 + [0] * 3),
            # the last-sample rule: the last one at n - 2, for the truth, for the prediction and for both
            planted([0] * 4 + [1] * 20 + [0], [0] * 25), planted([0] * 25, [0] * 4 + [1] * 20 + [0]),
            planted([0] * 4 + [1] * 20 + [0]), planted([1] * 20 + [0], [0] * 3 + [1] * 18)]
    exact = np.full(24, 0.1, dtype=np.float32)
    exact[4:20] = 0.5                                      # a score exactly AT the threshold 0.5 is a call
    exact[9] = np.nextafter(np.float32(0.5), np.float32(0.0))
    hand.append((exact, np.array([0] * 4 + [1] * 16 + [0] * 4, dtype=np.uint8)))
    n_random = len(stretches)
    stretches += hand

    cases, seen = [], np.zeros((2, 3), dtype=np.int64)
    for index, (scores, truth) in enumerate(stretches):
        for threshold in THRESHOLDS if index < n_random else (0.5,):
            runs = runs_of(scores, truth, threshold)
            for kind, _start, _end, state in runs:
                seen[kind, state] += 1
            cases.append({"stretch": index, "threshold": threshold, "min_run": 15, "runs": runs})
    assert seen.min() >= 3, seen                           # every (kind, state) pair occurs at least three times

    offsets = np.zeros(len(stretches) + 1, dtype=np.int64)
    np.cumsum([len(s) for s, _ in stretches], out=offsets[1:])
    np.savez_compressed(os.path.join(HERE, "run_states_golden.npz"), scores=np.concatenate([s for s, _ in stretches]).astype(np.float32),
                        labels=np.concatenate([t for _, t in stretches]).astype(np.uint8), offsets=offsets)
    with open(os.path.join(HERE, "run_states_golden.json"), "w") as fh:
        json.dump({"states": ["complete", "incomplete", "absent"], "cases": cases}, fh, separators=(",", ":"))
    print({"stretches": len(stretches), "cases": len(cases), "runs": int(seen.sum()), "kind x state": seen.tolist()})


if __name__ == "__main__":
    main()
