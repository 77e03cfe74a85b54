"""Generate the run-score golden vectors by EXECUTING the reference's own pure-Python functions.

networks/process_output.py cannot be imported whole (matplotlib, the model classes), so the function definitions its offline
evaluation collects scores with are extracted with ``ast`` and executed, as make_run_states_golden.py does:

  class_from_threshold (:572-582), hp_loc_dict (:614-643), check_hp (:814-895), create_confdict (:1062-1092), correct_short (:1096-1123)

over the stretches of the existing run_states_golden.npz, at the thresholds 0.3, 0.5 and 0.9, chained two ways:

  route "A"  check_for_false_neg (:68-124): scores -> labels (NO correct_short) -> hp_loc_dict of prediction and truth -> check_hp of
             every true run against the prediction -> create_confdict(true_hp, fake_states, "fn") -> the scores
             predicted_scores[a:b + 1] of every missed homopolymer ("fn")
  route "B"  main (:221-287): the same with correct_short on the labels, and create_confdict's "tp" and "fp" runs of the prediction
             and "fn" runs of the truth; the scores under them are taken with the same slice

The reference reads its scores from a text dump, i.e. as Python floats; the float32 scores go in as the doubles they are.

Output (data only): tests/golden/run_scores_golden.json -- per case: stretch, threshold, route and per name ("fn"; "tp", "fp", "fn")
the sorted scores (written with float32's shortest digits: float32 of them is the score), and for a non-empty list ``sum / len`` and
``statistics.median`` of the doubles.  Run in the build container (needs /root/reference); the fixture travels, the reference does not.
"""
import ast
import json
import os
import statistics

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/networks/process_output.py"
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
    ref = extract(REF, {"class_from_threshold", "hp_loc_dict", "check_hp", "create_confdict", "correct_short"})
    with np.load(os.path.join(HERE, "run_states_golden.npz")) as z:
        scores, labels, offsets = z["scores"], z["labels"], z["offsets"]

    def under(runs, predicted_scores):
        out = []
        if runs != 0:                                      # (create_confdict returns 0 for an empty dict)
            for name in runs:
                out.extend(predicted_scores[runs[name][0]: runs[name][1] + 1])
        return out

    def collect(predicted_scores, true_labels, threshold, corrected):
        predicted_labels = ref["class_from_threshold"](predicted_scores, threshold)
        if corrected:
            predicted_labels = list(ref["correct_short"](predicted_labels))
        predicted_hp, true_hp = ref["hp_loc_dict"](predicted_labels), ref["hp_loc_dict"](true_labels)
        read_states = [ref["check_hp"](predicted_hp[hp], true_labels, hp) for hp in predicted_hp]
        fake_states = [ref["check_hp"](true_hp[hp], predicted_labels, hp) for hp in true_hp]
        got = {"fn": under(ref["create_confdict"](true_hp, fake_states, "fn"), predicted_scores)}
        if corrected:
            got["tp"] = under(ref["create_confdict"](predicted_hp, read_states, "tp"), predicted_scores)
            got["fp"] = under(ref["create_confdict"](predicted_hp, read_states, "fp"), predicted_scores)
        return got

    cases, seen = [], {}
    for index, (a, b) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist())):
        if a == b:
            continue                                       # (its correct_short indexes predictions[0])
        predicted_scores, true_labels = [float(s) for s in scores[a:b]], [int(v) for v in labels[a:b]]
        for threshold in THRESHOLDS:
            for route, corrected in (("A", False), ("B", True)):
                case = {"stretch": index, "threshold": threshold, "route": route, "scores": {}, "mean": {}, "median": {}}
                for name, values in collect(predicted_scores, true_labels, threshold, corrected).items():
                    values = sorted(values)
                    case["scores"][name] = [float(str(np.float32(v))) for v in values]
                    assert all(float(np.float32(w)) == v for w, v in zip(case["scores"][name], values))
                    if values:
                        case["mean"][name], case["median"][name] = sum(values) / len(values), statistics.median(values)
                        seen[(route, name)] = seen.get((route, name), 0) + 1
                cases.append(case)
    with open(os.path.join(HERE, "run_scores_golden.json"), "w") as fh:
        json.dump({"thresholds": list(THRESHOLDS), "cases": cases}, fh, separators=(",", ":"))
    print({"cases": len(cases), "non-empty": {"%s %s" % key: value for key, value in sorted(seen.items())}})


if __name__ == "__main__":
    main()
