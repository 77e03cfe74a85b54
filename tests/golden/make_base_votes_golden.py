"""Generate the per-base vote golden vectors by EXECUTING the reference's own unfinished function.

networks/correct_output.py (marked ``### NOT FINISHED ###``) cannot be imported (h5py, base_to_signal), so ``correct_events`` -- the
loop that averages the scores of the samples of every event and rounds the average to a class per base -- is extracted with ``ast``
and executed against a stand-in for ``h5py.File``: an object whose ``[...Events]`` is a structured array with ``length`` and ``base``.
The function returns nothing; its printed ``classes`` list and the count in its last printed line ("Classified N bases from event
A to B") are captured through the ``print`` it is given.

Only ``start = 0`` is used: the function's stop test compares the running sum against ``length``, not ``start + length``.  ``length``
is the whole read, and the whole read less five samples (the last event then lies partly outside and is dropped).  Scores lie on the
1/256 grid, so the reference's float mean is exact, and NO event mean equals 0.5 (asserted): Python's ``round`` sends that tie to 0,
``base_votes.vote_host`` calls it.

Output (data only): tests/golden/base_votes_golden.npz -- per case event lengths, bases, scores, the ``length`` argument, the classes
and the count.  Run in the build container (needs /root/reference); the fixture travels, the reference does not.
"""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/networks/correct_output.py"


class EventFile(object):
    """What ``correct_events`` needs of ``h5py.File``: a context manager whose items are the read's event table."""

    table = None

    def __init__(self, path, mode):
        assert mode == "r"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getitem__(self, key):
        assert key.endswith("BaseCalled_template/Events"), key
        return EventFile.table


def extract(path):
    with open(path) as fh:
        tree = ast.parse(fh.read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "correct_events"]
    assert len(body) == 1
    printed = []
    h5py = type("h5py", (), {"File": EventFile})
    ns = {"h5py": h5py, "print": lambda *args: printed.append(args)}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["correct_events"], printed


def main():
    correct_events, printed = extract(REF)
    rng = np.random.default_rng(20261020)
    cases = []
    for n_events in (40, 1, 2, 57, 120):
        lengths = rng.integers(1, 21, size=n_events).astype(np.int64)
        lengths[rng.integers(0, n_events)] = 300                                  # one long dwell
        bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, size=n_events)]
        level = rng.integers(0, 257, size=n_events)
        scores = np.clip(np.repeat(level, lengths) + rng.integers(-100, 101, size=int(lengths.sum())), 0, 256) / 256.0
        total = int(lengths.sum())
        for e, (a, b) in enumerate(zip(np.cumsum(lengths) - lengths, np.cumsum(lengths))):      # no mean of exactly 0.5
            if 2 * int(round(float(scores[a:b].sum()) * 256)) == 256 * int(b - a):
                scores[a] += (1 if scores[a] < 1 else -1) / 256.0
        for e, (a, b) in enumerate(zip(np.cumsum(lengths) - lengths, np.cumsum(lengths))):
            assert 2 * int(round(float(scores[a:b].sum()) * 256)) != 256 * int(b - a), e
        table = np.zeros(n_events, dtype=[("length", np.int64), ("base", "S1")])
        table["length"], table["base"] = lengths, bases.view("S1")
        for length in sorted({total, max(total - 5, 1)}):
            EventFile.table = table
            del printed[:]
            correct_events("read.fast5", [float(s) for s in scores], start=0, length=length)
            lists = [args[0] for args in printed if len(args) == 1 and isinstance(args[0], list)]
            assert len(lists) == 1
            classes = np.array(lists[0], dtype=np.int64)
            last = printed[-1][0]
            assert last.startswith("Classified ") and " bases from event 0 to " in last, last
            count = int(last.split()[1])
            assert count == classes.size and set(np.unique(classes)) <= {0, 1}
            cases.append((lengths, bases, scores.astype(np.float32), length, classes, count))
            assert np.array_equal(cases[-1][2].astype(np.float64), scores)         # the grid is exact in float32
    assert any(c[5] < c[0].size for c in cases) and any(c[5] == c[0].size for c in cases)       # a dropped last event, and none dropped
    assert sum(int(c[4].sum()) for c in cases) >= 10 and sum(int((1 - c[4]).sum()) for c in cases) >= 10

    def packed(index, dtype):
        offsets = np.zeros(len(cases) + 1, dtype=np.int64)
        np.cumsum([len(c[index]) for c in cases], out=offsets[1:])
        return np.concatenate([c[index] for c in cases]).astype(dtype), offsets

    lengths, event_offsets = packed(0, np.int64)
    bases, _ = packed(1, np.uint8)
    scores, score_offsets = packed(2, np.float32)
    classes, class_offsets = packed(4, np.uint8)
    np.savez_compressed(os.path.join(HERE, "base_votes_golden.npz"), event_lengths=lengths, event_bases=bases, event_offsets=event_offsets,
                        scores=scores, score_offsets=score_offsets, length=np.array([c[3] for c in cases], dtype=np.int64),
                        classes=classes, class_offsets=class_offsets, count=np.array([c[5] for c in cases], dtype=np.int64))
    print({"cases": len(cases), "events": [int(c[0].size) for c in cases], "classified": [c[5] for c in cases],
           "called": [int(c[4].sum()) for c in cases]})


if __name__ == "__main__":
    main()
