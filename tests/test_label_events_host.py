"""Labels from event tables, the host side: ``catfish_amd.labelling`` against the golden cases made by executing the reference
(tests/golden/make_label_events_golden.py), against a plain-loop restatement, its refusals, the ``.npz`` round trip, the validation
set built from events, and the converter through a stand-in ``h5py``.  The batches the replay and GPU tests share are built here."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import labelling  # noqa: E402
from catfish_amd.labelling import EventBatch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "label_events_golden.npz")
TILE = 4096
PIECE = 1024
_golden = []


def golden_cases():
    """[dict(bases, lengths, clipped, kmer, labels, basemap, raw, signal, read_start, clip_source)], loaded once."""
    if not _golden:
        with np.load(GOLDEN) as z:
            g = {k: z[k] for k in z.files}
        eo, so, go = g["event_offsets"], g["sample_offsets"], g["signal_offsets"]
        for i in range(len(g["kmer"])):
            _golden.append({"bases": g["bases"][eo[i]:eo[i + 1]], "lengths": g["lengths"][eo[i]:eo[i + 1]],
                            "clipped": (int(g["clipped"][i, 0]), int(g["clipped"][i, 1])), "kmer": int(g["kmer"][i]),
                            "labels": g["labels"][so[i]:so[i + 1]], "basemap": g["basemap"][so[i]:so[i + 1]], "raw": g["raw"][so[i]:so[i + 1]],
                            "signal": g["signal"][go[i]:go[i + 1]], "read_start": int(g["read_start"][i]),
                            "clip_source": int(g["clip_source"][i])})
    return _golden


def loop_labels(bases, lengths, cs, ce, kmer):
    """The issue's statement of the rule, one event and one sample at a time."""
    n, oh = len(bases), kmer // 2
    core = [0] * n
    for e in range(n):
        if not cs <= e < n - ce or e - oh < 0 or e + oh >= n or bases[e] == ord("N"):
            continue
        core[e] = int(all(bases[e + d] == bases[e] for d in range(-oh, oh + 1)))
    cls = [int(any(core[x] for x in range(max(0, e - 2), min(n, e + 3)))) for e in range(n)]
    labels, basemap = [], []
    for e in range(n):
        for j in range(int(lengths[e])):
            labels.append(cls[e])
            basemap.append(int(bases[e]) | (0x80 if j == int(lengths[e]) // 2 else 0))
    return np.array(labels, dtype=np.uint8), np.array(basemap, dtype=np.uint8)


def random_read(rng, n_events=None, longest=12):
    n = int(rng.integers(1, 61)) if n_events is None else n_events
    letters = np.frombuffer([b"AC", b"ACG", b"ACGTN", b"AaCGTN"][int(rng.integers(0, 4))], dtype=np.uint8)
    bases = rng.choice(letters, size=n)
    cs = int(rng.integers(0, n + 1))
    return bases, rng.integers(1, longest + 1, size=n).astype(np.int32), (cs, int(rng.integers(0, n - cs + 1)))


def run_read(n_events, lengths=None, run_at=(), letter=b"A", clipped=(0, 0)):
    """``n_events`` events of C, G, T in turn with runs of ``letter`` at [a, b) for (a, b) in ``run_at``; lengths default to 1."""
    bases = np.frombuffer(b"CGT" * (n_events // 3 + 1), dtype=np.uint8)[:n_events].copy()
    for a, b in run_at:
        bases[a:b] = ord(letter)
    return bases, (np.ones(n_events, np.int32) if lengths is None else np.asarray(lengths, np.int32)), clipped


def edge_batches():
    """name -> EventBatch: the sizes at which the kernels take another path (see tests/test_label_events_gpu.py)."""
    out = {}
    out["golden"] = EventBatch.from_reads([(c["bases"], c["lengths"], c["clipped"]) for c in golden_cases()])
    out["one event"] = EventBatch.from_reads([(b"A", [1])])
    out["one long event"] = EventBatch.from_reads([(b"A", [2 * TILE + 3])])
    out["a tile full of events"] = EventBatch.from_reads([run_read(TILE + 1, run_at=((TILE - 4, TILE + 1), (100, 106)))])

    def border_read(begin, run_at):                                  # 40 events of 200 samples, but event 21 begins at sample `begin`
        lengths = np.full(40, 200, np.int32)
        lengths[20] = begin - 20 * 200
        return run_read(40, lengths, run_at=(run_at,))

    out["event borders at a tile border"] = EventBatch.from_reads(
        [border_read(TILE - 1, (18, 24)), border_read(TILE, (18, 24)), border_read(TILE + 1, (18, 24)), border_read(TILE, (21, 27)),
         border_read(TILE - 1, (15, 21)), border_read(TILE + 1, (14, 19))])
    out["the piece border"] = EventBatch.from_reads(
        [run_read(n, np.arange(n) % 5 + 1, run_at=((PIECE - 3, min(n, PIECE + 3)), (5, 10), (n - 5, n))) for n in (PIECE - 1, PIECE, PIECE + 1)] +
        [run_read(2 * PIECE + 7, run_at=((PIECE - 9, PIECE - 2), (2 * PIECE - 2, 2 * PIECE + 7)), clipped=(3, 2))])
    out["neighbouring reads"] = EventBatch.from_reads([run_read(12, np.full(12, 3), run_at=((9, 12),)), run_read(12, np.full(12, 3), run_at=((0, 2),)),
                                                       run_read(7, run_at=((4, 7),)), run_read(7, run_at=((0, 3),))])
    reads = [labelling.synthetic_event_read(3000, seed) for seed in range(70)]
    out["synthetic reads"] = EventBatch.from_reads([(b, l, (10, 10) if len(b) > 20 else (0, 0)) for _raw, b, l in reads])
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the rule
def test_every_golden_case_byte_for_byte():
    cases = golden_cases()
    assert len(cases) >= 40 and {c["kmer"] for c in cases} == {1, 3, 5, 7} and {c["clip_source"] for c in cases} == {0, 1, 2}
    assert {len(c["bases"]) for c in cases} >= {1, 2, 4, 5, 9, 60}
    for i, c in enumerate(cases):
        labels, basemap = labelling.label_read_host(c["bases"], c["lengths"], c["clipped"], c["kmer"])
        assert labels.dtype == np.uint8 and np.array_equal(labels, c["labels"]), i
        assert basemap.dtype == np.uint8 and np.array_equal(basemap, c["basemap"]), i
        starts = np.cumsum(c["lengths"]) - c["lengths"]
        again, _ = labelling.label_read_host(c["bases"].tobytes(), c["lengths"].tolist(), c["clipped"], c["kmer"], starts=starts)
        assert np.array_equal(again, labels)
    assert sum(int(c["labels"].sum()) for c in cases) > 500


def test_two_hundred_random_reads_against_the_plain_loop():
    rng = np.random.default_rng(31)
    positives = 0
    for i in range(200):
        bases, lengths, (cs, ce) = random_read(rng)
        kmer = (1, 3, 5, 7, 9, 15)[i % 6]
        labels, basemap = labelling.label_read_host(bases, lengths, (cs, ce), kmer)
        want_labels, want_map = loop_labels(bases, lengths, cs, ce, kmer)
        assert np.array_equal(labels, want_labels) and np.array_equal(basemap, want_map), i
        assert np.array_equal(labelling.expand_events_host(labelling.event_classes_host(bases, cs, ce, kmer), lengths), labels)
        assert np.array_equal(labelling.base_map_host(bases, lengths), basemap)
        positives += int(labels.sum())
    assert positives > 1000


def test_batch_labels_are_the_reads_labels_and_the_edge_batches_hold_what_they_claim():
    batches = edge_batches()
    for kmer in (1, 5, 7):
        for name, batch in batches.items():
            labels, basemap = batch.label_host(kmer, base_map=True)
            assert labels.shape == basemap.shape == (batch.total,) and np.array_equal(batch.label_host(kmer), labels)
            r = batch.n_reads - 1
            bases, lengths, clipped = batch.read(r)
            one, one_map = labelling.label_read_host(bases, lengths, clipped, kmer)
            assert np.array_equal(labels[batch.sample_offsets[r]:], one) and np.array_equal(basemap[batch.sample_offsets[r]:], one_map), name
    assert batches["golden"].n_reads >= 40
    assert batches["one long event"].total == 2 * TILE + 3 and batches["a tile full of events"].n_events == TILE + 1
    borders = batches["event borders at a tile border"]
    firsts = [np.cumsum(borders.read(r)[1])[20] for r in range(borders.n_reads)]     # where event 21 begins
    assert {TILE - 1, TILE, TILE + 1} <= set(int(f) for f in firsts)
    assert [batches["the piece border"].read(r)[0].size for r in range(3)] == [PIECE - 1, PIECE, PIECE + 1]
    near = batches["neighbouring reads"]
    lab = near.label_host(5)
    assert not lab[:near.sample_offsets[2]].any()                    # AAA | AA across two reads is no 5-mer
    assert near.label_host(3)[:near.sample_offsets[2]].any()
    synthetic = batches["synthetic reads"]
    assert synthetic.n_reads == 70 and synthetic.total == 70 * 3000 and 0.01 < synthetic.label_host(5).mean() < 0.5


def test_synthetic_event_read():
    raw, bases, lengths = labelling.synthetic_event_read(20000, 3)
    assert raw.shape == (20000,) and raw.dtype == np.float64 and int(lengths.sum()) == 20000 and lengths.min() >= 1
    assert bases.dtype == np.uint8 and lengths.dtype == np.int32 and set(bases.tolist()) <= set(b"ACGT")
    again = labelling.synthetic_event_read(20000, 3)
    assert all(np.array_equal(a, b) for a, b in zip(again, (raw, bases, lengths)))
    labels, _ = labelling.label_read_host(bases, lengths)
    assert 0.01 < labels.mean() < 0.3 and np.median(raw) == 0


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_raises_value_error():
    ok = dict(bases=b"ACGTAAAAAC", lengths=[3] * 10)
    labelling.label_read_host(**ok)
    bad = [dict(bases=b"", lengths=[]),                                              # E == 0
           dict(lengths=[3] * 9 + [0]), dict(lengths=[3] * 9 + [-2]),                # a length < 1
           dict(lengths=[3] * 9), dict(lengths=[2.5] * 10),
           dict(clipped=(-1, 0)), dict(clipped=(0, -1)), dict(clipped=(6, 5)), dict(clipped=(11, 0)), dict(clipped=3),
           dict(kmer=4), dict(kmer=0), dict(kmer=17), dict(kmer=-3), dict(kmer=5.0), dict(kmer=True),
           dict(bases=np.array([65] * 9 + [128], np.uint8)), dict(bases="ACGTAAAAAé"), dict(bases=np.array(["AC"] * 10)),
           dict(bases=np.arange(10, dtype=np.int64)),
           dict(starts=np.arange(10) * 3 + 1), dict(starts=np.arange(9) * 3), dict(starts=[0, 3, 6, 9, 12, 15, 18, 21, 24, 28])]
    for change in bad:
        with pytest.raises(ValueError):
            labelling.label_read_host(**dict(ok, **change))
    labelling.label_read_host(starts=np.arange(10) * 3, **ok)
    for kmer in (4, 0, 17):
        with pytest.raises(ValueError):
            labelling.event_classes_host(b"AAAAA", 0, 0, kmer)
        with pytest.raises(ValueError):
            EventBatch.from_reads([(b"AAAAA", [1] * 5)]).label_host(kmer)
    # the batch makes the same refusals, and knows the raw samples it was given
    for change in bad:
        if "kmer" not in change:
            with pytest.raises(ValueError):
                EventBatch.from_reads([dict(ok), dict(ok, **change)])
    EventBatch.from_reads([dict(ok, raw=np.zeros(30))])
    EventBatch.from_reads([dict(ok, n_raw=31)])
    with pytest.raises(ValueError, match="raw signal has 29"):
        EventBatch.from_reads([dict(ok, raw=np.zeros(29))])                          # final_signal past the raw samples
    with pytest.raises(ValueError, match="raw signal has 29"):
        EventBatch.from_reads([(ok["bases"], ok["lengths"], (0, 0), None, 29)])
    with pytest.raises(ValueError):
        EventBatch.from_reads([(b"A",)])
    # 2^31 samples (no array of that size is made), and an event of 2^31
    half = (b"AC", [2 ** 30 - 1, 1])
    assert EventBatch.from_reads([half]).total == 2 ** 30
    with pytest.raises(ValueError, match="2\\^31"):
        EventBatch.from_reads([half, half])
    assert EventBatch.from_reads([half, (b"A", [2 ** 30 - 1])]).total == 2 ** 31 - 1
    with pytest.raises(ValueError, match="2\\^31"):
        EventBatch.from_reads([(b"A", [2 ** 31])])


# ---------------------------------------------------------------------------------------------------------------------------- files and loaders
def write_event_npz(path, raw, bases, lengths, clipped=None, starts=False, base_kind="S1"):
    bases = np.asarray(bases, np.uint8)
    keys = {"raw": raw, "event_length": lengths,
            "event_base": bases if base_kind == "u8" else bases.view("S1") if base_kind == "S1" else bases.view("S1").astype("U1")}
    if clipped is not None:
        keys["clipped_start"], keys["clipped_end"] = np.int64(clipped[0]), np.int64(clipped[1])
    if starts:
        keys["event_start"] = np.cumsum(lengths) - lengths
    np.savez(path, **keys)
    return str(path)


def test_event_batch_round_trips_load_event_npz(tmp_path):
    reads, paths = [], []
    for i, kind in enumerate(("S1", "U1", "u8", "S1")):
        raw, bases, lengths = labelling.synthetic_event_read(700 + 13 * i, 40 + i)
        raw = np.concatenate([raw, np.ones(5 * (i % 2))])                            # a raw tail behind final_signal is kept out
        clipped = None if i == 3 else (i, 2 * i)
        paths.append(write_event_npz(tmp_path / ("r%d.npz" % i), raw, bases, lengths, clipped, starts=bool(i % 2), base_kind=kind))
        reads.append((raw, bases, lengths, clipped or (0, 0)))
    loaded = [labelling.load_event_npz(p) for p in paths]
    batch = EventBatch.from_reads(loaded)
    want = EventBatch.from_reads([(b, l, c) for _raw, b, l, c in reads])
    for a, b in zip((batch.bases, batch.lengths, batch.event_offsets, batch.clipped, batch.sample_offsets),
                    (want.bases, want.lengths, want.event_offsets, want.clipped, want.sample_offsets)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert batch.bases.dtype == np.uint8 and batch.lengths.dtype == np.int32 and batch.event_offsets.dtype == np.int64
    assert batch.clipped.dtype == np.int32 and batch.clipped.shape == (4, 2) and batch.sample_offsets.dtype == np.int64
    for i, (rd, (raw, _b, _l, _c)) in enumerate(zip(loaded, reads)):
        assert np.array_equal(rd["raw"], raw) and (rd["starts"] is None) == (i % 2 == 0)
        sig, lab = labelling.load_labelled_event_npz(paths[i], 5)
        assert len(sig) == len(lab) == 700 + 13 * i and np.array_equal(sig, raw[:len(lab)])
        assert np.array_equal(lab, batch.label_host(5)[batch.sample_offsets[i]:batch.sample_offsets[i + 1]])
    np.savez(tmp_path / "bare.npz", raw=np.zeros(4), event_base=np.zeros(2, np.uint8))
    with pytest.raises(ValueError, match="event_length"):
        labelling.load_event_npz(str(tmp_path / "bare.npz"))
    short = write_event_npz(tmp_path / "short.npz", np.zeros(10), np.frombuffer(b"ACG", np.uint8), np.array([4, 4, 4]))
    with pytest.raises(ValueError, match="raw signal has 10"):
        EventBatch.from_reads([labelling.load_event_npz(short)])
    torn = write_event_npz(tmp_path / "torn.npz", np.zeros(12), np.frombuffer(b"ACG", np.uint8), np.array([4, 4, 4]))
    with np.load(torn) as z:
        np.savez(tmp_path / "torn2.npz", event_start=np.array([0, 4, 9]), **{k: z[k] for k in z.files})
    with pytest.raises(ValueError, match="contiguous"):
        EventBatch.from_reads([labelling.load_event_npz(str(tmp_path / "torn2.npz"))])
    assert labelling.kmer_from_env(None) is None and labelling.kmer_from_env(" ") is None and labelling.kmer_from_env("7") == 7
    for value in ("4", "x", "17"):
        with pytest.raises(ValueError, match="CATFISH_LABEL_KMER"):
            labelling.kmer_from_env(value)


def test_validation_set_from_events_on_the_cpu_equals_from_arrays(tmp_path):
    from catfish_amd.device_db import DeviceReadDb
    from catfish_amd.device_validation import DeviceValidationSet
    reads = [labelling.synthetic_event_read(900 + 35 * i, 60 + i) for i in range(5)]
    signals = [np.concatenate([raw, np.zeros(i)]) for i, (raw, _b, _l) in enumerate(reads)]      # tails behind final_signal
    batch = EventBatch.from_reads([(b, l, (2, 3)) for _raw, b, l in reads])
    for kmer in (3, 5):
        got = DeviceValidationSet.from_events(signals, batch, kmer=kmer, device="cpu")
        host = batch.label_host(kmer)
        want = DeviceValidationSet.from_arrays([raw for raw, _b, _l in reads],
                                               [host[batch.sample_offsets[r]:batch.sample_offsets[r + 1]] for r in range(5)])
        assert got.signal.dtype == np.float32 and np.array_equal(got.signal, want.signal)
        assert got.labels.dtype == np.uint8 and np.array_equal(got.labels, want.labels) and got.labels.any()
        assert np.array_equal(got.offsets, want.offsets) and got.uploads == 0
    with pytest.raises(ValueError):
        DeviceValidationSet.from_events(signals[:4], batch, device="cpu")
    with pytest.raises(ValueError):
        DeviceValidationSet.from_events([s[:100] for s in signals], batch, device="cpu")
    paths = [write_event_npz(tmp_path / ("v%d.npz" % i), signals[i], b, l, (2, 3), starts=True) for i, (_raw, b, l) in enumerate(reads)]
    from_files = DeviceValidationSet.from_event_npz(paths, kmer=5, device="cpu")
    assert np.array_equal(from_files.labels, want.labels) and np.array_equal(from_files.signal, want.signal)
    db = DeviceReadDb.from_event_npz(paths, kmer=5, seed=4, device="cpu")
    want_db = DeviceReadDb.from_arrays([raw for raw, _b, _l in reads],
                                       [host[batch.sample_offsets[r]:batch.sample_offsets[r + 1]] for r in range(5)], seed=4)
    assert np.array_equal(db.labels, want_db.labels) and np.array_equal(db.signal, want_db.signal) and np.array_equal(db.offsets, want_db.offsets)
    assert np.array_equal(db.pos_start, want_db.pos_start) and np.array_equal(db.neg_start, want_db.neg_start)


def test_train_validate_reads_event_directories_when_the_kmer_is_set(tmp_path, monkeypatch):
    """``CATFISH_LABEL_KMER``: the loaders ``main`` hands out read event files and give what ``load_npz`` gives for the labelled files
    made from them; unset, they are ``load_npz`` itself."""
    from catfish_amd import train_validate as tv
    raw, bases, lengths = labelling.synthetic_event_read(1500, 77)
    event_path = write_event_npz(tmp_path / "e.npz", raw, bases, lengths, (10, 10))
    labels, _ = labelling.label_read_host(bases, lengths, (10, 10), 5)
    np.savez(tmp_path / "l.npz", raw=raw, base_labels=labels)
    monkeypatch.delenv("CATFISH_LABEL_KMER", raising=False)
    assert tv.npz_loader_from_env() is tv.load_npz
    monkeypatch.setenv("CATFISH_LABEL_KMER", "5")
    loader = tv.npz_loader_from_env()
    got, want = loader(event_path), tv.load_npz(str(tmp_path / "l.npz"))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    a = tv.example_db_from_npz([event_path], loader=loader)
    b = tv.example_db_from_npz([str(tmp_path / "l.npz")])
    assert a.nb_pos == b.nb_pos > 0 and a.nb_neg == b.nb_neg and np.array_equal(np.asarray(a.pos), np.asarray(b.pos))
    sig_a = tv.select_validation_stretches([event_path], 35, 700, 100, 5, loader=loader)
    sig_b = tv.select_validation_stretches([str(tmp_path / "l.npz")], 35, 700, 100, 5)
    assert np.array_equal(sig_a[0][0], sig_b[0][0]) and np.array_equal(sig_a[1][0], sig_b[1][0])
    monkeypatch.setenv("CATFISH_LABEL_KMER", "6")
    with pytest.raises(ValueError, match="CATFISH_LABEL_KMER"):
        tv.npz_loader_from_env()


# ---------------------------------------------------------------------------------------------------------------------------- the converter
class _Dataset(object):
    def __init__(self, array, attrs=None):
        self.array, self.attrs = np.asarray(array), dict(attrs or {})

    def __getitem__(self, key):
        return self.array.copy() if isinstance(key, tuple) else self.array[key].copy()


class _Group(object):
    def __init__(self, children=None, attrs=None):
        self.children, self.attrs = dict(children or {}), dict(attrs or {})

    def _find(self, path):
        node = self
        for part in [p for p in path.split("/") if p]:
            if not isinstance(node, _Group) or part not in node.children:
                return None
            node = node.children[part]
        return node

    def __contains__(self, path):
        return self._find(path) is not None

    def __getitem__(self, path):
        node = self._find(path)
        if node is None:
            raise KeyError("Unable to open object (object %r doesn't exist)" % path)
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


def _tombo_tree(case, attr_names):
    table = np.zeros(len(case["lengths"]), dtype=[("start", "<i8"), ("length", "<i8"), ("base", "S1")])
    table["length"], table["base"] = case["lengths"], case["bases"].view("S1")
    table["start"] = np.cumsum(case["lengths"]) - case["lengths"]
    template = {"Events": _Dataset(table, {"read_start_rel_to_raw": np.int64(case["read_start"])})}
    if attr_names:
        template["Alignment"] = _Group(attrs={attr_names[0]: np.int64(case["clipped"][0]), attr_names[1]: np.int64(case["clipped"][1])})
    return _Group({"Analyses": _Group({"RawGenomeCorrected_000": _Group({"BaseCalled_template": _Group(template)})}),
                   "Raw": _Group({"Reads": _Group({"Read_9": _Group({"Signal": _Dataset(case["signal"])})})})})


def test_convert_events_through_a_stand_in_h5py(tmp_path, monkeypatch):
    from catfish_amd import convert
    registry = {}
    h5py = types.ModuleType("h5py")

    def open_file(path, mode="r"):
        if path not in registry:
            raise OSError("Unable to open file (file signature not found)")
        return registry[path]

    h5py.File = open_file
    monkeypatch.setitem(sys.modules, "h5py", h5py)
    names = {0: None, 1: ("clipped_bases_start", "clipped_bases_end"), 2: ("trimmed_obs_start", "trimmed_obs_end")}
    seen = set()
    for i, case in enumerate(golden_cases()):
        src, dst = str(tmp_path / ("read%d.fast5" % i)), str(tmp_path / ("read%d.npz" % i))
        open(src, "wb").write(b"stand-in, never parsed")
        registry[src] = _tombo_tree(case, names[case["clip_source"]])
        default = case["clipped"][0] if case["clip_source"] == 0 else 99            # without Alignment attributes the default counts
        assert convert.convert_events(src, dst, clipped_bases=default) == len(case["labels"])
        read = labelling.load_event_npz(dst)
        assert read["clipped"] == case["clipped"] and np.array_equal(read["starts"], np.cumsum(case["lengths"]) - case["lengths"])
        assert read["raw"].dtype == np.float64 and np.array_equal(read["raw"], case["raw"])          # the reference's normalised signal
        raw, labels = labelling.load_labelled_event_npz(dst, case["kmer"])
        assert np.array_equal(labels, case["labels"]) and len(raw) == len(labels)
        seen.add(case["clip_source"])
    assert seen == {0, 1, 2}
    case = golden_cases()[5]
    src = str(tmp_path / "default.fast5")
    open(src, "wb").write(b"x")
    registry[src] = _tombo_tree(case, None)
    convert.convert_events(src, str(tmp_path / "default.npz"))
    assert labelling.load_event_npz(str(tmp_path / "default.npz"))["clipped"] == (10, 10)       # the reference's --clipped-bases default
    # the directory walk and the flag
    out = tmp_path / "out"
    only = tmp_path / "only"
    only.mkdir()
    open(str(only / "a.fast5"), "wb").write(b"x")
    registry[str(only / "a.fast5")] = _tombo_tree(golden_cases()[20], names[1])
    assert convert.main(["-i", str(only), "-o", str(out), "--events"]) == 0
    assert sorted(os.listdir(str(out))) == ["a.npz"]
    with pytest.raises(ValueError, match="path to FAST5 is not correct"):
        convert.convert_events(str(tmp_path / "nope.fast5"), str(tmp_path / "nope.npz"))
    truncated = dict(case, signal=case["signal"][:case["read_start"] + len(case["labels"]) - 1])
    registry[src] = _tombo_tree(truncated, None)
    with pytest.raises(ValueError, match="raw signal has"):
        convert.convert_events(src, str(tmp_path / "t.npz"))
    monkeypatch.setitem(sys.modules, "h5py", None)
    with pytest.raises(ImportError, match="needs h5py"):
        convert.convert_events(src, str(tmp_path / "t.npz"))
