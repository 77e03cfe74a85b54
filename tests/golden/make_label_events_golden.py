"""Generate the event-labelling golden cases by EXECUTING the reference's own code.

What is executed, and how it is reached:

  networks/trainingDB/training_encodings.py   imported as it is (``hp_class_number``, ``extend_classification``)
  networks/trainingDB/TrainingRead.py         the class definition is lifted with ``ast`` and executed with ``Persistent`` bound to
                                              ``object`` and ``normalize_raw_signal`` (the one name it takes from helper_functions)
                                              bound to this project's ``infer.normalize_raw_signal``; ``__init__`` then runs as
                                              written: the ``raw`` setter, the ``events`` setter with ``use_tombo=True``, and
                                              ``classify_events`` (``label_raws``) through the ``classified`` setter
  networks/base_to_signal.py                  ``get_base_new_signal`` lifted the same way, ``h5py`` bound to a stand-in module

Both read a stand-in hdf object that answers exactly the look-ups those lines make: ``in``, ``[path]``, ``.attrs``,
``["length" | "base" | "start"]``, ``visit`` and ``[()]``.  Every part of the class could be executed; nothing falls back to
``hp_class_number`` + ``extend_classification`` + ``expand_sequence`` called directly (``main`` still checks that route gives the
same labels, which it must).

Output (arrays only): tests/golden/label_events_golden.npz -- the cases packed one behind the other:
  bases uint8, lengths int32 (per event), event_offsets int64 [n + 1]; clipped int32 [n, 2], kmer int32 [n];
  clip_source int32 [n] (0: the constructor's clipped_bases, 1: the Alignment's clipped_bases_*, 2: its trimmed_obs_*);
  labels uint8, basemap uint8 (per sample: the base byte, bit 7 where get_base_new_signal's second list says "n"), raw float64 (the
  reference's normalised signal cut to final_signal), sample_offsets int64 [n + 1];
  signal int16 (the DAC samples the stand-in file held), signal_offsets int64 [n + 1], read_start int32 [n]
Run where the reference is (/root/reference); the fixture travels, the reference does not.
"""
import ast
import os
import sys
import types
from itertools import chain, repeat
from math import ceil
from random import sample

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/networks"
EVENTS = "Analyses/RawGenomeCorrected_000/BaseCalled_template/Events"
ALIGNMENT = "Analyses/RawGenomeCorrected_000/BaseCalled_template/Alignment"

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "trainingDB"))

import training_encodings  # noqa: E402  (the reference's, as it is)
from catfish_amd.infer import normalize_raw_signal  # noqa: E402


def lift(path, name, kind, namespace):
    with open(path) as fh:
        tree = ast.parse(fh.read())
    body = [n for n in tree.body if isinstance(n, kind) and n.name == name]
    assert len(body) == 1, (path, name)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), namespace)
    return namespace[name]


class Dataset(object):
    """A dataset: ``[()]`` for the whole array, ``[field]`` for a column of a table, ``.attrs``."""

    def __init__(self, array, attrs=None):
        self.array, self.attrs = np.asarray(array), dict(attrs or {})

    def __getitem__(self, key):
        if isinstance(key, tuple) and key == ():
            return self.array.copy()
        assert key in ("length", "base", "start"), key
        return self.array[key].copy()


class Group(object):
    """A group: children by name, ``.attrs``, path look-ups with or without a trailing slash, ``in`` and ``visit``."""

    def __init__(self, children=None, attrs=None):
        self.children, self.attrs = dict(children or {}), dict(attrs or {})

    def find(self, path):
        node = self
        for part in [p for p in path.split("/") if p]:
            if not isinstance(node, Group) or part not in node.children:
                return None
            node = node.children[part]
        return node

    def __contains__(self, path):
        return self.find(path) is not None

    def __getitem__(self, path):
        node = self.find(path)
        if node is None:
            raise KeyError(path)
        return node

    def visit(self, func):
        for name in sorted(self.children):
            got = func(name)
            if got is not None:
                return got
        return None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def tree_of(bases, lengths, signal, read_start, clip_source, clipped):
    table = np.zeros(len(lengths), dtype=[("start", "<i8"), ("length", "<i8"), ("base", "S1")])
    table["length"] = lengths
    table["start"] = np.cumsum(lengths) - lengths
    table["base"] = np.frombuffer(bases, dtype="S1")
    template = {"Events": Dataset(table, {"read_start_rel_to_raw": np.int64(read_start)})}
    if clip_source:
        names = ("clipped_bases_start", "clipped_bases_end") if clip_source == 1 else ("trimmed_obs_start", "trimmed_obs_end")
        template["Alignment"] = Group(attrs={names[0]: np.int64(clipped[0]), names[1]: np.int64(clipped[1])})
    return Group({"Analyses": Group({"RawGenomeCorrected_000": Group({"BaseCalled_template": Group(template)})}),
                  "Raw": Group({"Reads": Group({"Read_17": Group({"Signal": Dataset(signal)})})})})


def filler(n, first=0):
    return bytes(b"CGT"[(first + i) % 3] for i in range(n))


def cases():
    rng = np.random.default_rng(20260)
    out = []

    def add(bases, lengths=None, clipped=(0, 0), kmer=5, source=0):
        if lengths is None:
            lengths = rng.integers(1, 13, size=len(bases))
        out.append((bytes(bases), np.asarray(lengths, dtype=np.int64), tuple(clipped), kmer, source))

    for n in (1, 2, 4, 5, 9, 60):                                   # plain reads of few events, with some runs by chance
        add(bytes(rng.choice(np.frombuffer(b"AACG", dtype=np.uint8), size=n)))
    add(b"A" * 5)
    add(b"A" * 4)
    add(b"A")
    add(b"A", kmer=1)
    for kmer in (1, 3, 5, 7):                                       # runs of exactly k - 1, k, k + 1 at the start, in the middle, at the end
        for run in (kmer - 1, kmer, kmer + 1):
            if run == 0:
                continue
            add(b"A" * run + filler(14), kmer=kmer)
            add(filler(7) + b"A" * run + filler(8, 1), kmer=kmer)
            add(filler(14) + b"A" * run, kmer=kmer)
    add(b"CGT" + b"AAANAAA" + b"CGTC")                              # an N inside a run
    add(b"CG" + b"AANAA" + b"TGC", kmer=3)
    add(b"CGT" + b"NNNNNNN" + b"CGT")                               # a run OF N
    add(b"AAAAAN")
    add(b"CGT" + b"aaaaaa" + b"CGT")                                # lower case: a base only equals itself
    add(b"CGT" + b"AAaAA" + b"CGTAAAAAc")
    add(b"ttttt" + b"TTTTT" + b"cg")
    long_read = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=60))
    long_read[8:15] = b"G" * 7
    long_read[30:36] = b"T" * 6
    long_read[52:60] = b"C" * 8
    for source in (0, 1, 2):                                        # clipping, from each of the three places the reference looks
        add(long_read, clipped=(10, 10), source=source)             # ... 10 / 10 cuts both outer runs
    add(long_read, clipped=(0, 0), source=1)
    add(long_read, clipped=(12, 3), source=2)
    add(long_read, clipped=(30, 30), source=1)                      # cs + ce == E
    add(b"CGAAAAAAT", clipped=(4, 5), source=1)
    add(b"CGAAAAAAT", clipped=(9, 0), source=2)
    add(b"CGAAAAAAT", clipped=(0, 9), source=1)
    add(b"A" * 20, clipped=(10, 10), source=0)
    add(b"A" * 20, clipped=(3, 4), source=1, kmer=7)
    add(b"CGAAAAATC", lengths=[1, 1, 300, 1, 1, 1, 1, 300, 1])      # events of one sample next to one of 300
    add(b"AAAAACGTC", lengths=[300, 1, 1, 1, 1, 1, 1, 1, 1])
    add(b"C", lengths=[300])
    for kmer in (1, 3, 5, 7):
        add(long_read, clipped=(3, 2), kmer=kmer, source=1)
    return out


def main():
    namespace = {"Persistent": object, "normalize_raw_signal": normalize_raw_signal, "training_encodings": training_encodings, "np": np,
                 "chain": chain, "repeat": repeat, "ceil": ceil, "sample": sample}
    TrainingRead = lift(os.path.join(REF, "trainingDB", "TrainingRead.py"), "TrainingRead", ast.ClassDef, namespace)
    opened = {}
    h5py = types.ModuleType("h5py")
    h5py.File = lambda path, mode: opened[path]
    base_new = lift(os.path.join(REF, "base_to_signal.py"), "get_base_new_signal", ast.FunctionDef, {"h5py": h5py})

    rng = np.random.default_rng(20261)
    packed = {k: [] for k in ("bases", "lengths", "labels", "basemap", "raw", "signal")}
    clipped_all, kmers, sources, read_starts = [], [], [], []
    for index, (bases, lengths, clipped, kmer, source) in enumerate(cases()):
        final, read_start = int(lengths.sum()), int(rng.integers(0, 12))
        signal = rng.integers(200, 900, size=read_start + final + int(rng.integers(0, 9))).astype(np.int16)
        hdf = tree_of(bases, lengths, signal, read_start, source, clipped)
        # source 0: no Alignment group, the constructor's clipped_bases counts (one number for both ends)
        assert source != 0 or clipped[0] == clipped[1]
        read = TrainingRead(hdf, "median", "Analyses/RawGenomeCorrected_000", clipped[0] if source == 0 else 99, kmer, use_tombo=True)
        labels = np.asarray(read.classified, dtype=np.int64)
        assert read.final_signal == final and labels.shape == (final,) and set(labels.tolist()) <= {0, 1}
        assert (read.clipped_bases_start, read.clipped_bases_end) == clipped
        # the same labels by the three functions alone (what a fall-back would have used)
        kmer_list = [km for km, _s, _r in read.condensed_events]
        direct = read.expand_sequence(training_encodings.extend_classification([training_encodings.hp_class_number(km) for km in kmer_list]))
        assert direct == labels.tolist()
        opened["case"] = hdf
        base_list, new_list = base_new("case")
        assert len(base_list) == len(new_list) == final and set(new_list) <= {"n", "-"}
        basemap = np.array([ord(b) for b in base_list], dtype=np.uint8) | np.array([0x80 if n == "n" else 0 for n in new_list], dtype=np.uint8)
        packed["bases"].append(np.frombuffer(bases, dtype=np.uint8))
        packed["lengths"].append(lengths.astype(np.int32))
        packed["labels"].append(labels.astype(np.uint8))
        packed["basemap"].append(basemap)
        packed["raw"].append(np.asarray(read.raw, dtype=np.float64)[:final])
        packed["signal"].append(signal)
        clipped_all.append(clipped)
        kmers.append(kmer)
        sources.append(source)
        read_starts.append(read_start)

    def offsets(parts):
        return np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)

    n = len(kmers)
    positives = int(sum(int(l.sum()) for l in packed["labels"]))
    assert n >= 40 and positives > 500, (n, positives)
    np.savez_compressed(os.path.join(HERE, "label_events_golden.npz"),
                        bases=np.concatenate(packed["bases"]), lengths=np.concatenate(packed["lengths"]), event_offsets=offsets(packed["bases"]),
                        clipped=np.array(clipped_all, dtype=np.int32), kmer=np.array(kmers, dtype=np.int32),
                        clip_source=np.array(sources, dtype=np.int32), labels=np.concatenate(packed["labels"]),
                        basemap=np.concatenate(packed["basemap"]), raw=np.concatenate(packed["raw"]), sample_offsets=offsets(packed["labels"]),
                        signal=np.concatenate(packed["signal"]), signal_offsets=offsets(packed["signal"]),
                        read_start=np.array(read_starts, dtype=np.int32))
    print({"cases": n, "events": int(sum(len(b) for b in packed["bases"])), "samples": int(sum(len(l) for l in packed["labels"])),
           "positive samples": positives, "cases with a positive": int(sum(1 for l in packed["labels"] if l.any()))})


if __name__ == "__main__":
    main()
