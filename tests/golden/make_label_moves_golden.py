"""Generate the move-table labelling golden cases by EXECUTING the reference's own code.

What is executed, and how it is reached (as tests/golden/make_label_events_golden.py does, whose ``lift`` and ``Group`` are used):

  networks/trainingDB/training_encodings.py   imported as it is (``hp_class_number``, ``extend_classification``)
  networks/trainingDB/TrainingRead.py         the class definition is lifted with ``ast`` and executed with ``Persistent`` bound to
                                              ``object`` and ``normalize_raw_signal`` bound to this project's; ``__init__`` then
                                              runs as written with ``use_tombo=False`` (the class's default): the ``raw`` setter
                                              (``first_sample_template``), the ``events`` setter's ``model_state`` / ``move`` /
                                              ``length`` branch, and ``classify_events`` through the ``classified`` setter

It reads a stand-in hdf object that answers exactly the look-ups those lines make.  In this branch the reference leaves
``final_signal`` None; ``classified`` is what is recorded.

Output (arrays only): tests/golden/label_moves_golden.npz -- the cases packed one behind the other:
  states uint8 (the k-mers' bytes, k per event), state_offsets int64 [n + 1] (into ``states``), k int32 [n];
  lengths float64 (per event; a case with length_f64 == 0 held them as float32, and every float32 is a float64), length_f64 int32 [n],
  moves int32 (per event), event_offsets int64 [n + 1]; clipped int32 [n, 2], n_raw int64 [n];
  labels uint8 (the reference's ``classified``), sample_offsets int64 [n + 1]
The generator asserts its teeth: among the float32 cases some read's labels differ from the same table taken as float64 (the
reference run again), some from the sums taken in reverse order, some from the product taken in float64.
Run where the reference is (/root/reference); the fixture travels, the reference does not.
"""
import ast
import os
import sys
from itertools import chain, repeat
from math import ceil
from random import sample

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_label_events_golden import REF, Group, lift, training_encodings  # noqa: E402
from catfish_amd import labelling  # noqa: E402
from catfish_amd.infer import normalize_raw_signal  # noqa: E402

HDF_PATH = "Analyses/Basecall_1D_000"
FIELDS = ("length", "model_state", "move")


class Table(object):
    """The Events dataset: a column per field name."""

    def __init__(self, columns):
        self.columns, self.attrs = columns, {}

    def __getitem__(self, key):
        assert key in FIELDS, key
        return self.columns[key].copy()


class Signal(object):
    def __init__(self, array):
        self.array, self.attrs = np.asarray(array), {}

    def __getitem__(self, key):
        assert isinstance(key, tuple) and key == (), key
        return self.array.copy()


def tree_of(states, lengths, moves, clipped, signal, first_sample):
    k = len(states[0])
    columns = {"length": np.asarray(lengths), "model_state": np.array(states, dtype="S%d" % k), "move": np.asarray(moves)}
    analyses = {"Basecall_1D_000": Group({"BaseCalled_template": Group({"Events": Table(columns)})}),
                "Segmentation_000": Group({"Summary": Group({"segmentation": Group(attrs={"first_sample_template": np.int64(first_sample)})})}),
                "RawGenomeCorrected_000": Group({"BaseCalled_template": Group({"Alignment": Group(attrs={
                    "clipped_bases_start": np.int64(clipped[0]), "clipped_bases_end": np.int64(clipped[1])})})})}
    return Group({"Analyses": Group(analyses), "Raw": Group({"Reads": Group({"Read_17": Group({"Signal": Signal(signal)})})})})


def merged_lengths(lengths, moves):
    """Per merged event, the lengths the reference adds up, in its order (the first one twice)."""
    out = [[lengths[0], lengths[0]]]
    for n in range(1, len(lengths)):
        if moves[n] != 0:
            out.append([lengths[n]])
        else:
            out[-1].append(lengths[n])
    return out


def counts_variant(lengths, moves, mode):
    """n_signals under another arithmetic: "reverse" sums right to left, "wide" takes the product in float64."""
    dt = lengths.dtype.type
    out = []
    for parts in merged_lengths(lengths, moves):
        total = dt(0)
        for value in (reversed(parts) if mode == "reverse" else parts):
            total = dt(total + value)
        out.append(ceil(np.float64(total) * 4000) if mode == "wide" else ceil(dt(total * dt(4000))))
    return np.array(out, dtype=np.int64)


def labels_variant(case, mode):
    states, lengths, moves, clipped, n_raw = case
    heads, _n = labelling.merge_moves_host(lengths, moves)
    counts = counts_variant(lengths, moves, mode)
    at = labelling.as_states(np.array(states, dtype="S%d" % len(states[0])))
    cls = labelling.move_classes_host(at, heads, clipped[0], clipped[1])
    return labelling.expand_events_host(cls, counts)[:min(int(counts.sum()), n_raw)]


def kmers_around(bases, k):
    pad = bytes(bases[:1]) * (k // 2) + bytes(bases) + bytes(bases[-1:]) * (k - 1 - k // 2)
    return [pad[i:i + k] for i in range(len(bases))]


def cases():
    """(states [list of k-byte strings], lengths float32 / float64 [E] in seconds, moves int [E], (cs, ce), n_raw or a word)."""
    rng = np.random.default_rng(20270)
    out = []

    def add(states, moves, lengths=None, clipped=(0, 0), n_raw="beyond", dtype=np.float32):
        if lengths is None:
            lengths = rng.integers(1, 60, size=len(states))
        out.append((list(states), (np.asarray(lengths, dtype=np.float64) / 4000.0).astype(dtype), np.asarray(moves, dtype=np.int64), tuple(clipped), n_raw))

    def random_read(n, k, dtype, clipped=(0, 0), n_raw="beyond", stay=0.45):
        """Merged events of which some are homopolymer k-mers; every one followed by stays with probability ``stay`` each."""
        states, moves = [], []
        bases = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())
        at = 3
        while at + k + 2 < n:
            bases[at:at + k + int(rng.integers(0, 3))] = bytes([bases[at]]) * (k + 2)
            at += int(rng.integers(9, 16))
        bases = bases[:n]
        for km in kmers_around(bytes(bases), k):
            states.append(km)
            moves.append(int(rng.choice([1, 1, 1, 2, -1])))
            while rng.random() < stay:
                states.append(km)
                moves.append(0)
        add(states, moves, clipped=clipped, n_raw=n_raw, dtype=dtype)

    for dtype in (np.float32, np.float64):
        for n in (1, 2, 3, 7, 40):
            random_read(n, 5, dtype)
        random_read(40, 5, dtype, n_raw="inside")
        random_read(40, 5, dtype, n_raw="border")
        random_read(30, 5, dtype, clipped=(2, 2))
        random_read(30, 1, dtype)
        random_read(30, 7, dtype, clipped=(0, 2))
        random_read(12, 5, dtype, stay=0.0)                                     # no stays
        add([b"AAAAA"] * 9, [0] * 9, dtype=dtype)                               # all stays: M = 1
        add([b"ACGTA"] * 6, [3] + [0] * 5, dtype=dtype)                         # a non-zero move[0], M = 1
        add([b"CCCCC"], [1], dtype=dtype)                                       # one event
        add([b"CCCCC"], [0], lengths=[1], dtype=dtype)
        filler = [b"ACGTA", b"CGTAC", b"GTACG", b"TACGT", b"ACGTC", b"CGTCA", b"GTCAG", b"TCAGT"]
        for hp_at in (0, 1, 6, 7):                                              # a homopolymer k-mer at merged positions 0, 1, M - 2, M - 1
            states = list(filler)
            states[hp_at] = b"TTTTT"
            add(states, [1, 2, 1, -1, 1, 1, 2, 1], dtype=dtype)
            doubled = [s for s in states for _ in (0, 1)]
            add(doubled, [5, 0, 1, 0, 2, 0, 1, 0, -3, 0, 1, 0, 1, 0, 1, 0], dtype=dtype)
        add(filler[:3] + [b"AANAA", b"NNNNN", b"aaaaa", b"AAaAA", b"ttttt", b"TTTTT"] + filler[3:], [1] * 14, dtype=dtype)
        add(filler[:2] + [b"GGGGG"] * 3 + filler[2:] + [b"AAAAA"], [1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1], clipped=(2, 2), dtype=dtype)
        add(filler[:2] + [b"GGGGG"] * 3 + filler[2:] + [b"AAAAA"], [1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1], clipped=(4, 6), dtype=dtype)   # cs + ce = M
        add([b"AAAAA"] * 4, [1, 1, 1, 1], clipped=(0, 4), dtype=dtype)
    for _ in range(12):                                                         # float32 tables whose answer depends on the arithmetic
        random_read(60, 5, np.float32, stay=0.6)
    return out


def main():
    namespace = {"Persistent": object, "normalize_raw_signal": normalize_raw_signal, "training_encodings": training_encodings, "np": np,
                 "chain": chain, "repeat": repeat, "ceil": ceil, "sample": sample}
    TrainingRead = lift(os.path.join(REF, "trainingDB", "TrainingRead.py"), "TrainingRead", ast.ClassDef, namespace)
    rng = np.random.default_rng(20271)

    def reference(states, lengths, moves, clipped, n_raw):
        first = int(rng.integers(0, 12))
        signal = rng.integers(200, 900, size=first + n_raw).astype(np.int16)
        read = TrainingRead(tree_of(states, lengths, moves, clipped, signal, first), "median", HDF_PATH, 99, len(states[0]), use_tombo=False)
        assert read.final_signal is None and len(read.raw) == n_raw
        labels = np.asarray(read.classified, dtype=np.int64)
        assert set(labels.tolist()) <= {0, 1}
        return labels.astype(np.uint8)

    packed = {k: [] for k in ("states", "lengths", "moves", "labels")}
    ks, f64, clipped_all, n_raws = [], [], [], []
    teeth = {"float64": 0, "reverse": 0, "wide": 0}
    seen = {"inside": 0, "border": 0, "beyond": 0}
    for states, lengths, moves, clipped, where in cases():
        _heads, counts = labelling.merge_moves_host(lengths, moves)
        covered = int(counts.sum())
        if where == "beyond":
            n_raw = covered + int(rng.integers(1, 40))
        elif where == "border":
            n_raw = int(np.cumsum(counts)[len(counts) // 2])
        else:
            mid = len(counts) // 2
            assert counts[mid] >= 2
            n_raw = int(np.cumsum(counts)[mid]) - int(counts[mid]) // 2
        seen[where] += 1
        labels = reference(states, lengths, moves, clipped, n_raw)
        assert labels.size == min(covered, n_raw)
        case = (states, lengths, moves, clipped, n_raw)
        host, _map = labelling.label_move_read_host(np.array(states, dtype="S%d" % len(states[0])), lengths, moves, clipped, n_raw)
        assert np.array_equal(host, labels)                                     # the module's definition, checked where the reference is
        if lengths.dtype == np.float32:
            wide = reference(states, lengths.astype(np.float64), moves, clipped, n_raw)
            teeth["float64"] += int(wide.size != labels.size or not np.array_equal(wide, labels))
            for mode in ("reverse", "wide"):
                other = labels_variant(case, mode)
                teeth[mode] += int(other.size != labels.size or not np.array_equal(other, labels))
        packed["states"].append(np.frombuffer(b"".join(states), dtype=np.uint8))
        packed["lengths"].append(lengths.astype(np.float64))
        packed["moves"].append(moves.astype(np.int32))
        packed["labels"].append(labels)
        ks.append(len(states[0]))
        f64.append(int(lengths.dtype == np.float64))
        clipped_all.append(clipped)
        n_raws.append(n_raw)
    assert all(teeth.values()), teeth                                           # a wrong dtype, order or product width shows
    assert all(seen.values()), seen

    def offsets(parts):
        return np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)

    positives = int(sum(int(l.sum()) for l in packed["labels"]))
    assert len(ks) >= 60 and positives > 500, (len(ks), positives)
    np.savez_compressed(os.path.join(HERE, "label_moves_golden.npz"),
                        states=np.concatenate(packed["states"]), state_offsets=offsets(packed["states"]), k=np.array(ks, dtype=np.int32),
                        lengths=np.concatenate(packed["lengths"]), length_f64=np.array(f64, dtype=np.int32),
                        moves=np.concatenate(packed["moves"]), event_offsets=offsets(packed["moves"]),
                        clipped=np.array(clipped_all, dtype=np.int32), n_raw=np.array(n_raws, dtype=np.int64),
                        labels=np.concatenate(packed["labels"]), sample_offsets=offsets(packed["labels"]))
    print({"cases": len(ks), "events": int(sum(len(m) for m in packed["moves"])), "samples": int(sum(len(l) for l in packed["labels"])),
           "positive samples": positives, "teeth": teeth})


if __name__ == "__main__":
    main()
