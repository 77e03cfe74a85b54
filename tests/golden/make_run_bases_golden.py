"""Generate the run-bases golden vectors by EXECUTING the reference's own pure-Python functions.

networks/process_output.py cannot be imported whole (matplotlib, the model classes), so the function definitions its offline
evaluation by base is made of are extracted with ``ast`` and executed, as make_run_states_golden.py does:

  class_from_threshold, correct_short, hp_loc_dict, check_hp, create_confdict, prediction_information, base_count_dict, get_bases,
  get_prevalence

and chained the way its main loop chains them (:235-320, the ``on_hps`` branch): scores -> labels -> correct_short -> hp_loc_dict
of prediction and truth -> prediction_information of all true runs (:253) and all called runs (:259) -> check_hp of every run
-> create_confdict "tp" / "fn" / "fp" (:285-287) -> prediction_information of each (:292, :306, :319).  The ``bases`` / ``new``
strings the reference takes from base_to_signal.get_base_new_signal are built from ``labelling.base_map_host`` (the byte & 0x7f;
"n" where bit 7 is set, else "-"), which tests/golden/label_events_golden.npz pins to that function.

Outputs (data only): tests/golden/run_bases_golden.npz (float32 scores, uint8 labels, uint8 basemap, int64 offsets of the
stretches) and tests/golden/run_bases_golden.json (per case: stretch, threshold and, for the five groups true / called / tp / fp /
fn, the reference's ``count_bases`` {length in bases: runs} and ``count_seq`` {sequence: runs} Counters).
Run in the build container (needs /root/reference); the fixtures travel, the reference does not.
"""
import ast
import json
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/networks/process_output.py"
NAMES = {"class_from_threshold", "correct_short", "hp_loc_dict", "check_hp", "create_confdict", "prediction_information", "base_count_dict",
         "get_bases", "get_prevalence"}
THRESHOLDS = (0.3, 0.5, 0.9)
GROUPS = ("true", "called", "tp", "fp", "fn")


def extract(path, names):
    with open(path) as fh:
        tree = ast.parse(fh.read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    ns = {"np": np, "Counter": Counter}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def class_of(seq):
    return "ACGT".index(seq[0]) if seq and seq[0] in "ACGT" and seq == seq[0] * len(seq) else 4


def main():
    from catfish_amd import labelling
    ref = extract(REF, NAMES)
    rng = np.random.default_rng(20261020)

    def groups_of(scores, truth, basemap, threshold):
        """{group: {"bases": Counter, "seq": Counter}} of one stretch, by the reference's functions alone."""
        labels = ref["class_from_threshold"]([float(s) for s in scores], threshold)
        predicted = [int(v) for v in ref["correct_short"](labels)]
        truth = [int(v) for v in truth]
        bases = "".join(chr(int(b) & 0x7f) for b in basemap)
        new = "".join("n" if int(b) & 0x80 else "-" for b in basemap)
        predicted_hp, true_hp = ref["hp_loc_dict"](predicted), ref["hp_loc_dict"](truth)
        read_states = [ref["check_hp"](predicted_hp[hp], truth, hp) for hp in predicted_hp]
        fake_states = [ref["check_hp"](true_hp[hp], predicted, hp) for hp in true_hp]
        dicts = {"true": true_hp or 0, "called": predicted_hp or 0, "tp": ref["create_confdict"](predicted_hp, read_states, "tp"),
                 "fn": ref["create_confdict"](true_hp, fake_states, "fn"), "fp": ref["create_confdict"](predicted_hp, read_states, "fp")}
        out = {}
        for group in GROUPS:
            count_bases, count_seq = Counter(), Counter()
            if dicts[group] != 0:
                _measurements, count_bases, count_seq = ref["prediction_information"](dicts[group], bases, new)
            assert type(count_bases) is Counter and type(count_seq) is Counter       # nothing but the reference's functions made them
            out[group] = {"bases": {str(k): int(v) for k, v in sorted(count_bases.items())}, "seq": {k: int(v) for k, v in sorted(count_seq.items())}}
        return out

    stretches = []                                         # (scores float32, truth uint8, basemap uint8)
    for seed in range(6):                                  # event reads, labelled by the project's rule, with prediction noise
        _raw, bases, lengths = labelling.synthetic_event_read(1500, 900 + seed, hp_fraction=0.25)
        truth, basemap = labelling.label_read_host(bases, lengths, (0, 0), 5)
        n = truth.size
        drift = 3.0 * np.sin(np.arange(n) / 25.0 + rng.uniform(0.0, 6.28))
        z = 3.0 * (2.0 * np.roll(truth, int(rng.integers(-6, 7))).astype(np.float64) - 1.0) + rng.normal(0.0, 0.7, size=n) + drift
        stretches.append(((1.0 / (1.0 + np.exp(-z))).astype(np.float32), truth, basemap))
    n_random = len(stretches)

    def hand(events, truth_at, called_at):
        """``events``: [(base character, samples), ...]; ``truth_at`` / ``called_at``: (first, last + 1) in samples, or None."""
        basemap = labelling.base_map_host("".join(b for b, _ in events), [n for _, n in events])
        truth, called = np.zeros(basemap.size, np.uint8), np.zeros(basemap.size, np.uint8)
        if truth_at:
            truth[truth_at[0]:truth_at[1]] = 1
        if called_at:
            called[called_at[0]:called_at[1]] = 1
        stretches.append((np.where(called == 1, np.float32(0.9), np.float32(0.1)).astype(np.float32), truth, basemap))

    filler = [(b, 7) for b in "GTCAT"]
    before = 7 * len(filler)
    for block in ("A", "C", "G", "T", "N", "a", "AAC"):    # every class in every group, three times over
        for count, samples in ((5, 8), (6, 9), (9, 4)):
            events = filler + [(b, samples) for b in block[0] * (count - len(block) + 1) + block[1:]] + filler      # "AAC": AAAAC, mixed
            at = (before, before + count * samples)
            hand(events, at, at)                           # found completely: true, called, tp
            hand(events, at, (at[0] + 3, at[1] + 5))       # found partly, the call overshoots into the next base
            hand(events, at, None)                         # missed: fn
            hand(events, None, at)                         # called where nothing is: fp
    for shift in (0, 10, 25):                              # runs inside one long event that miss its centre: no base at all
        events = filler + [("A", 200)] + filler
        at = (before + 5 + shift, before + 45 + shift)
        hand(events, at, at)
        hand(events, at, None)
        hand(events, None, at)
    for tail in (1, 2):                                    # the last-sample rule adds the mark of a last event of one (or two) samples
        events = filler + [("C", 6)] * 5 + [("G", tail)]
        n = before + 30 + tail
        hand(events, (before, n - 1), (before, n - 1))
        hand(events, (before, n - 1), None)
    for count in (33, 40):                                 # more bases than any bin
        events = filler + [("T", 2)] * count + filler
        at = (before, before + 2 * count)
        hand(events, at, at)
        hand(events, at, None)
        hand(events, None, at)

    cases = []
    seen, empty = Counter(), 0
    for index, (scores, truth, basemap) in enumerate(stretches):
        for threshold in THRESHOLDS if index < n_random else (0.5,):
            groups = groups_of(scores, truth, basemap, threshold)
            for group in GROUPS:
                for seq, count in groups[group]["seq"].items():
                    seen[(group, class_of(seq))] += count
                empty += groups[group]["bases"].get("0", 0)
            cases.append({"stretch": index, "threshold": threshold, "min_run": 15, "groups": groups})
    for group in GROUPS:
        for cls in range(5):
            assert seen[(group, cls)] >= 3, (group, cls, seen[(group, cls)])
    assert empty >= 3, empty

    offsets = np.zeros(len(stretches) + 1, dtype=np.int64)
    np.cumsum([len(s) for s, _, _ in stretches], out=offsets[1:])
    np.savez_compressed(os.path.join(HERE, "run_bases_golden.npz"), scores=np.concatenate([s for s, _, _ in stretches]).astype(np.float32),
                        labels=np.concatenate([t for _, t, _ in stretches]).astype(np.uint8),
                        basemap=np.concatenate([b for _, _, b in stretches]).astype(np.uint8), offsets=offsets)
    with open(os.path.join(HERE, "run_bases_golden.json"), "w") as fh:
        json.dump({"groups": list(GROUPS), "classes": ["A", "C", "G", "T", "other"], "cases": cases}, fh, separators=(",", ":"))
    print({"stretches": len(stretches), "cases": len(cases), "no base": empty,
           "group x class": {group: [seen[(group, cls)] for cls in range(5)] for group in GROUPS}})


if __name__ == "__main__":
    main()
