"""Generate the run-border golden records by EXECUTING the reference's own pure-Python functions.

As make_run_states_golden.py does, the four function definitions of networks/process_output.py the offline evaluation is made of
are extracted with ``ast`` and executed:

  class_from_threshold (:572-582), hp_loc_dict (:614-643), check_hp (:814-895), correct_short (:1096-1123)

and chained as its main loop chains them (:235-273), over the stretches already in run_states_golden.npz at the thresholds of
run_states_golden.json.  This file keeps the two thirds of ``check_hp``'s answer that make_run_states_golden.py drops: the offsets
``(l, r)`` and the interruptions.

Output (data only): tests/golden/run_borders_golden.json -- per case: stretch, threshold, min_run and every run that is not absent
as [kind, start, end, l, r, [gap lengths]]; kind 0 = a true run judged against the prediction, 1 = a predicted run judged against
the truth.  Run in the build container (needs /root/reference); the fixture travels, the reference does not.
"""
import ast
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/networks/process_output.py"


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
    with np.load(os.path.join(HERE, "run_states_golden.npz")) as z:
        scores, labels, offsets = z["scores"], z["labels"], z["offsets"]
    with open(os.path.join(HERE, "run_states_golden.json")) as fh:
        state_cases = json.load(fh)["cases"]

    def runs_of(stretch, threshold):
        a, b = int(offsets[stretch]), int(offsets[stretch + 1])
        if a == b:
            return [], [], []                              # (its correct_short indexes predictions[0])
        called = ref["class_from_threshold"]([float(s) for s in scores[a:b]], threshold)
        predicted = [int(v) for v in ref["correct_short"](called)]
        truth = [int(v) for v in labels[a:b]]
        out = []
        for kind, (runs, other) in enumerate(((ref["hp_loc_dict"](truth), predicted), (ref["hp_loc_dict"](predicted), truth))):
            for hp in runs.values():
                state, (l, r), gaps, _ids = ref["check_hp"](hp, other, 0)
                if state != "absent":
                    out.append([kind, int(hp[0]), int(hp[1]), int(l), int(r), [int(e - s + 1) for s, e in gaps]])
        return out, predicted, truth

    cases = []
    pairs = np.zeros((2, 3, 3), dtype=np.int64)            # [kind][sign of l][sign of r]
    interrupted = np.zeros(2, dtype=np.int64)
    at_zero = last_sample = total = largest = 0
    for case in state_cases:
        runs, predicted, truth = runs_of(case["stretch"], case["threshold"])
        for kind, s, e, l, r, gaps in runs:
            other, mask = (predicted, truth) if kind == 0 else (truth, predicted)
            pairs[kind, int(np.sign(l)) + 1, int(np.sign(r)) + 1] += 1
            interrupted[kind] += 1 if gaps else 0
            at_zero += 1 if s >= 1 and all(v == 1 for v in other[:s + 1]) else 0          # the position-0 rule bites
            last_sample += 1 if e == len(mask) - 1 and mask[e] != 1 else 0               # closed by the last-sample rule
            largest = max(largest, abs(l), abs(r))
            total += 1
        cases.append({"stretch": case["stretch"], "threshold": case["threshold"], "min_run": case["min_run"], "runs": runs})
    assert pairs.min() >= 5, pairs                         # each of the nine sign pairs, per kind
    assert at_zero >= 10 and last_sample >= 3 and interrupted.min() >= 5 and largest > 64, (at_zero, last_sample, interrupted, largest)
    with open(os.path.join(HERE, "run_borders_golden.json"), "w") as fh:
        json.dump({"record": ["kind", "start", "end", "l", "r", "gaps"], "cases": cases}, fh, separators=(",", ":"))
    print({"cases": len(cases), "runs": total, "sign pairs": pairs.tolist(), "position 0": at_zero, "last sample": last_sample,
           "interrupted": interrupted.tolist(), "largest offset": largest})


if __name__ == "__main__":
    main()
