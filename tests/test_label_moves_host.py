"""Labels from a basecaller's move table, the host side: ``catfish_amd.labelling`` against the golden cases made by executing the
reference's ``TrainingRead(..., use_tombo=False)`` (tests/golden/make_label_moves_golden.py), against a plain-loop restatement, its
refusals, ``MoveBatch`` packing, the ``.npz`` round trip, and the converter through a stand-in ``h5py``.  The batches the replay and
GPU tests share are built here."""
import os
import sys
import types
from math import ceil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import labelling  # noqa: E402
from catfish_amd.labelling import MoveBatch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "label_moves_golden.npz")
TILE = 4096                   # samples per workgroup of the expand kernel
PIECE = 1024                  # P: events per piece of the merge and the classes kernel
_golden = []
FILLER = [b"ACGTA", b"CGTAC", b"GTACG", b"TACGT", b"ACGTC", b"CGTCA", b"GTCAG", b"TCAGT"]


def golden_cases():
    """[dict(states uint8 [E, k], lengths, moves, clipped, n_raw, labels)], loaded once; ``lengths`` in the dtype the case was made in."""
    if not _golden:
        with np.load(GOLDEN) as z:
            g = {k: z[k] for k in z.files}
        eo, so, to = g["event_offsets"], g["sample_offsets"], g["state_offsets"]
        for i in range(len(g["k"])):
            lengths = g["lengths"][eo[i]:eo[i + 1]]
            _golden.append({"states": g["states"][to[i]:to[i + 1]].reshape(-1, int(g["k"][i])),
                            "lengths": lengths.copy() if g["length_f64"][i] else lengths.astype(np.float32), "moves": g["moves"][eo[i]:eo[i + 1]],
                            "clipped": (int(g["clipped"][i, 0]), int(g["clipped"][i, 1])), "n_raw": int(g["n_raw"][i]),
                            "labels": g["labels"][so[i]:so[i + 1]]})
    return _golden


def golden_batches():
    """(k, dtype) -> (MoveBatch, labels): a batch has one k and one length dtype, so the golden cases make six."""
    groups = {}
    for c in golden_cases():
        groups.setdefault((c["states"].shape[1], c["lengths"].dtype.name), []).append(c)
    return {key: (MoveBatch.from_reads([(c["states"], c["lengths"], c["moves"], c["clipped"], c["n_raw"]) for c in some]),
                  np.concatenate([c["labels"] for c in some])) for key, some in groups.items()}


def loop_labels(states, lengths, moves, cs, ce, n_raw):
    """The issue's statement of the rule, one event and one sample at a time, scalars of the table's dtype."""
    dt = lengths.dtype.type
    merged = []                                                      # [head, running length]
    for n in range(len(lengths)):
        if n == 0:
            merged.append([0, dt(lengths[0] + lengths[0])])
        elif moves[n] != 0:
            merged.append([n, lengths[n]])
        else:
            merged[-1][1] = dt(merged[-1][1] + lengths[n])
    m, k = len(merged), states.shape[1]
    counts = [int(ceil(dt(total * dt(4000)))) for _h, total in merged]
    core = [int(cs <= j < m - ce and states[h][0] != ord("N") and all(b == states[h][0] for b in states[h])) for j, (h, _t) in enumerate(merged)]
    cls = [int(any(core[x] for x in range(max(0, j - 2), min(m, j + 3)))) for j in range(m)]
    labels, basemap = [], []
    for j, (h, _t) in enumerate(merged):
        for q in range(counts[j]):
            labels.append(cls[j])
            basemap.append(int(states[h][k // 2]) | (0x80 if q == counts[j] // 2 else 0))
    final = min(sum(counts), n_raw)
    return np.array(labels[:final], dtype=np.uint8), np.array(basemap[:final], dtype=np.uint8), final


def random_table(rng, dtype, n_events=None, k=5):
    n = int(rng.integers(1, 60)) if n_events is None else n_events
    letters = [b"A", b"AC", b"ACGTN", b"AaCGTN"][int(rng.integers(0, 4))]
    states = np.empty((n, k), dtype=np.uint8)
    for e in range(n):
        states[e] = np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), size=k)] if rng.random() < 0.6 else rng.choice(
            np.frombuffer(letters, dtype=np.uint8))
    lengths = (rng.integers(1, 60, size=n) / 4000.0).astype(dtype)
    moves = rng.choice(np.array([0, 0, 1, 1, 2, -1]), size=n)
    m = 1 + int(np.count_nonzero(moves[1:]))
    cs = int(rng.integers(0, min(m, 2) + 1))
    return states, lengths, moves, (cs, int(rng.integers(0, min(m - cs, 2) + 1)))


def secs(count, dtype, parts=1):
    """A length in seconds that, added up ``parts`` times, gives ``count`` samples whatever the rounding does: the sum aims at
    ``count - 0.5``."""
    return dtype((count - 0.5) / 4000.0 / parts)


def table_of(counts, kmers, dtype=np.float32, stays=None, clipped=(0, 0), n_raw=None):
    """A read whose merged event j has ``counts[j]`` samples and k-mer ``kmers[j]``, split into a head and ``stays[j]`` stays (the
    read's first length is halved: the rule counts it twice); checked against ``merge_moves_host``."""
    stays = [0] * len(counts) if stays is None else stays
    states, lengths, moves = [], [], []
    for j, (count, kmer, extra) in enumerate(zip(counts, kmers, stays)):
        parts = extra + 1 + (1 if j == 0 else 0)
        for q in range(extra + 1):
            states.append(np.frombuffer(kmer, dtype=np.uint8))
            lengths.append(secs(count, dtype, parts))
            moves.append(0 if q else 1 + j % 2)
    lengths = np.array(lengths, dtype=dtype)
    _heads, made = labelling.merge_moves_host(lengths, np.array(moves))
    assert made.tolist() == list(counts)
    return np.array(states), lengths, np.array(moves, dtype=np.int32), clipped, int(sum(counts)) if n_raw is None else n_raw


def kmers_with_runs(n, run_at=(), letter=b"AAAAA"):
    out = [FILLER[j % len(FILLER)] for j in range(n)]
    for a, b in run_at:
        out[a:b] = [letter] * (b - a)
    return out


def edge_batches(dtype=np.float32):
    """name -> MoveBatch: the sizes at which the kernels take another path (see tests/test_label_moves_gpu.py)."""
    out = {}
    rng = np.random.default_rng(5)

    def events_read(n, heads_at=(), stays_at=(), run_heads=(3,)):
        """``n`` events, a random half of them heads, those of ``heads_at`` too, none inside the ranges ``stays_at``; the merged
        events listed in ``run_heads`` (and the two behind each) carry AAAAA."""
        moves = (rng.random(n) < 0.5).astype(np.int32)
        moves[np.asarray(heads_at, dtype=np.int64)] = 1
        for a, b in stays_at:
            moves[a:b] = 0
        m_index = np.cumsum(np.concatenate(([1], (moves[1:] != 0).astype(np.int64)))) - 1
        kmers = kmers_with_runs(int(m_index[-1]) + 1, [(j, j + 3) for j in run_heads])
        states = np.array([np.frombuffer(kmers[j], dtype=np.uint8) for j in m_index])
        return states, (rng.integers(1, 30, size=n) / 4000.0).astype(dtype), moves, (0, 0)

    out["P - 1, P and P + 1 events"] = MoveBatch.from_reads([events_read(n, run_heads=(3, 200)) for n in (PIECE - 1, PIECE, PIECE + 1)])
    out["stays across a piece border"] = MoveBatch.from_reads(
        [events_read(2 * PIECE + 9, heads_at=[PIECE - 5], stays_at=[(PIECE - 4, PIECE + 6)]),
         events_read(3 * PIECE, heads_at=[500], stays_at=[(501, 2 * PIECE + 100)])])  # ... and one stay run over two borders
    out["heads at the ends of a piece"] = MoveBatch.from_reads(
        [events_read(2 * PIECE + 2, heads_at=[PIECE - 1, PIECE, 2 * PIECE - 1, 2 * PIECE]),
         events_read(PIECE + 1, heads_at=[PIECE], stays_at=[(PIECE - 6, PIECE)]), events_read(PIECE, heads_at=[PIECE - 1])])

    def border_read(begin, run_at, stays=None):                      # 40 merged events of 200 samples, but the 21st begins at `begin`
        counts = [200] * 40
        counts[20] = begin - 20 * 200
        return table_of(counts, kmers_with_runs(40, (run_at,)), dtype, stays)

    out["merged-event borders at a tile border"] = MoveBatch.from_reads(
        [border_read(TILE - 1, (18, 21)), border_read(TILE, (18, 21)), border_read(TILE + 1, (18, 21)), border_read(TILE, (21, 24), [1] * 40),
         border_read(TILE - 1, (23, 24)), border_read(TILE + 1, (14, 17), [0, 2] * 20)])
    out["one merged event of 8195 samples"] = MoveBatch.from_reads(
        [table_of([2 * TILE + 3], [b"AAAAA"], dtype, [6]), table_of([2 * TILE + 3], [b"ACGTA"], dtype)])
    out["4097 one-sample merged events"] = MoveBatch.from_reads(
        [table_of([1] * (TILE + 1), kmers_with_runs(TILE + 1, ((TILE - 2, TILE + 1), (100, 103))), dtype)])
    out["cut by the raw signal"] = MoveBatch.from_reads(
        [table_of([300] * 40, kmers_with_runs(40, ((2, 5), (11, 12))), dtype, n_raw=1000),            # inside the first tile, inside an event
         table_of([300] * 40, kmers_with_runs(40, ((2, 5), (11, 14))), dtype, n_raw=TILE),            # on a tile border
         table_of([300] * 40, kmers_with_runs(40, ((25, 28),)), dtype, n_raw=2 * TILE),
         table_of([300] * 40, kmers_with_runs(40, ((25, 28),)), dtype, n_raw=10 ** 12)])              # raw far beyond the events
    out["neighbouring reads"] = MoveBatch.from_reads(
        [table_of([3] * 12, kmers_with_runs(12, ((11, 12),)), dtype), table_of([3] * 12, kmers_with_runs(12, ((0, 1),)), dtype),
         table_of([1] * 7, kmers_with_runs(7, ((6, 7),)), dtype, [2] * 7), table_of([1] * 7, kmers_with_runs(7, ((0, 1),)), dtype)])
    reads = [labelling.synthetic_move_read(3000, seed, dtype=dtype) for seed in range(40)]
    out["synthetic reads"] = MoveBatch.from_reads([(s, l, m, (10, 10), len(raw)) for raw, s, l, m in reads])
    return out


def write_move_npz(path, raw, states, lengths, moves, clipped=None):
    arrays = {"raw": raw, "event_state": np.ascontiguousarray(states).view("S%d" % states.shape[1]).reshape(-1), "event_move": moves,
              "event_length": lengths}
    if clipped is not None:
        arrays["clipped_start"], arrays["clipped_end"] = np.int64(clipped[0]), np.int64(clipped[1])
    np.savez(str(path), **arrays)
    return str(path)


# ---------------------------------------------------------------------------------------------------------------------------- the rule
def test_every_golden_case_byte_for_byte():
    cases = golden_cases()
    assert len(cases) >= 60 and {c["states"].shape[1] for c in cases} == {1, 5, 7}
    assert {c["lengths"].dtype for c in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(c["moves"][0] != 0 for c in cases) and any((c["moves"] < 0).any() for c in cases) and any((c["moves"] == 2).any() for c in cases)
    for i, c in enumerate(cases):
        labels, basemap = labelling.label_move_read_host(c["states"], c["lengths"], c["moves"], c["clipped"], c["n_raw"])
        assert labels.dtype == np.uint8 and np.array_equal(labels, c["labels"]), i
        checked = labelling.check_move_read(c["states"], c["lengths"], c["moves"], c["clipped"], c["n_raw"])
        assert checked[7] == len(c["labels"]) == len(basemap), i                                       # final
        as_strings = np.ascontiguousarray(c["states"]).view("S%d" % c["states"].shape[1]).reshape(-1)
        again, _ = labelling.label_move_read_host(as_strings.astype(str), c["lengths"], c["moves"].tolist(), c["clipped"], c["n_raw"])
        assert np.array_equal(again, labels)
    assert sum(int(c["labels"].sum()) for c in cases) > 500
    # the teeth the generator asserted, seen from here: the float32 cases taken as float64 do not all give the same labels
    differ = 0
    for c in cases:
        if c["lengths"].dtype == np.float32:
            wide, _ = labelling.label_move_read_host(c["states"], c["lengths"].astype(np.float64), c["moves"], c["clipped"], c["n_raw"])
            differ += int(wide.size != c["labels"].size or not np.array_equal(wide, c["labels"]))
    assert differ >= 5


def test_the_first_length_counts_twice():
    """The reference starts its running length at length[0] and, having forced move[0] to 0, adds length[0] again."""
    states = np.array([np.frombuffer(b"AAAAA", np.uint8), np.frombuffer(b"ACGTA", np.uint8)])
    for dtype in (np.float32, np.float64):
        lengths = np.array([10, 10], dtype=np.float64).astype(dtype) / dtype(4000)
        heads, counts = labelling.merge_moves_host(lengths, [1, 1])
        assert heads.tolist() == [0, 1] and counts.tolist() == [20, 10]
        labels, basemap = labelling.label_move_read_host(states, lengths, [1, 1])
        assert labels.tolist() == [1] * 30 and basemap[10] == ord("A") | 0x80 and basemap[25] == ord("G") | 0x80
        assert np.count_nonzero(basemap & 0x80) == 2
        heads, counts = labelling.merge_moves_host(lengths, [7, 0])                                    # move[0] is ignored; one merged event
        assert heads.tolist() == [0] and counts.tolist() == [30]


def test_two_hundred_random_tables_against_the_plain_loop():
    rng = np.random.default_rng(41)
    positives = 0
    for i in range(200):
        dtype = (np.float32, np.float64)[i % 2]
        states, lengths, moves, (cs, ce) = random_table(rng, dtype, k=(1, 2, 5, 7, 15)[i % 5])
        _h, counts = labelling.merge_moves_host(lengths, moves)
        n_raw = int(rng.integers(1, int(counts.sum()) + 30))
        labels, basemap = labelling.label_move_read_host(states, lengths, moves, (cs, ce), n_raw)
        want_labels, want_map, final = loop_labels(states, lengths, moves, cs, ce, n_raw)
        assert labels.size == final and np.array_equal(labels, want_labels) and np.array_equal(basemap, want_map), i
        positives += int(labels.sum())
    assert positives > 1000


def test_every_refusal():
    states = np.array([np.frombuffer(b"AAAAA", np.uint8)] * 3)
    lengths = np.array([0.01, 0.02, 0.01], dtype=np.float32)
    ok = lambda **kw: labelling.check_move_read(**dict(dict(states=states, lengths=lengths, moves=[1, 0, 1], clipped=(0, 0), n_raw=50), **kw))  # noqa: E731
    assert ok()[7] == 50 and ok(n_raw=None)[7] == 160 + 40 and ok(clipped=(1, 1))[3] == (1, 1)
    for change, text in ((dict(states=states[:0], lengths=lengths[:0], moves=[]), "at least one event"),
                         (dict(lengths=np.array([0.01, np.nan, 0.01], np.float32)), "finite"), (dict(lengths=np.array([0.01, np.inf, 0.01])), "finite"),
                         (dict(lengths=np.array([0.01, 0.0, 0.01], np.float32)), "> 0"), (dict(lengths=np.array([0.01, -0.5, 0.01])), "> 0"),
                         (dict(lengths=np.array([0.01, 6.0e5, 0.01])), "2\\^31"), (dict(lengths=np.array([0.01, 3.0e38, 3.0e38], np.float32)), "2\\^31"),
                         (dict(lengths=np.array([1, 2, 1])), "float32 or float64"), (dict(lengths=lengths.astype(np.float16)), "float32 or float64"),
                         (dict(states=np.zeros((3, 0), np.uint8)), "1 .. 15"), (dict(states=np.full((3, 16), 65, np.uint8)), "1 .. 15"),
                         (dict(states=np.array([b"AAAAA", b"AAA", b"AAAAA"])), "k bytes"), (dict(states=np.full((3, 5), 200, np.uint8)), "k bytes"),
                         (dict(clipped=(-1, 0)), "clipped"), (dict(clipped=(0, -1)), "clipped"), (dict(clipped=(2, 1)), "clipped"),
                         (dict(clipped=(0, 3)), "clipped"), (dict(clipped=7), "clipped"), (dict(n_raw=0), "n_raw"), (dict(n_raw=-4), "n_raw"),
                         (dict(moves=[1, 0]), "moves"), (dict(moves=[1.5, 0, 1]), "integers"), (dict(lengths=lengths[:2]), "event lengths")):
        with pytest.raises(ValueError, match=text):
            ok(**change)
    assert ok(clipped=(1, 1))[5].tolist() == [0, 2]                                                     # cs + ce == M is taken
    with pytest.raises(ValueError, match="one k and one length dtype"):
        MoveBatch.from_reads([(states, lengths, [1, 0, 1]), (states, lengths.astype(np.float64), [1, 0, 1])])
    with pytest.raises(ValueError, match="one k and one length dtype"):
        MoveBatch.from_reads([(states, lengths, [1, 0, 1]), (states[:, :3], lengths, [1, 0, 1])])
    big = (np.array([np.frombuffer(b"ACGTA", np.uint8)] * 5), np.full(5, 5.0e4), [1] * 5, (0, 0))      # 5 x 2 * 10^8 samples + the doubled first
    with pytest.raises(ValueError, match="2\\^31 or more events or samples"):
        MoveBatch.from_reads([big, big])
    assert MoveBatch.from_reads([big + (1000,), big + (2000,)]).total == 3000                          # ... cut by the raw signal they fit


def test_move_batch_packing_and_the_edge_batches_hold_what_they_claim():
    rng = np.random.default_rng(43)
    for dtype in (np.float32, np.float64):
        reads = [random_table(rng, dtype) for _ in range(30)]
        batch = MoveBatch.from_reads([(s, l, m, c) for s, l, m, c in reads])
        assert batch.states.dtype == np.uint8 and batch.states.shape == (batch.n_events, 5) and batch.lengths.dtype == dtype
        assert batch.moves.dtype == np.int32 and batch.event_offsets.dtype == np.int64 and batch.clipped.shape == (30, 2)
        assert batch.n_raw.dtype == np.int64 and batch.final.dtype == np.int64 and np.array_equal(np.diff(batch.sample_offsets), batch.final)
        labels, basemap = batch.label_host(base_map=True)
        assert np.array_equal(batch.label_host(), labels)
        for r, (s, l, m, c) in enumerate(reads):
            got = batch.read(r)
            assert np.array_equal(got[0], s) and np.array_equal(got[1], l) and np.array_equal(got[2], m) and got[3] == c
            want_labels, want_map = labelling.label_move_read_host(s, l, m, c)
            a, b = batch.sample_offsets[r], batch.sample_offsets[r + 1]
            assert got[4] == batch.final[r] == b - a == want_labels.size and batch.merged[r] == 1 + np.count_nonzero(m[1:])
            assert np.array_equal(labels[a:b], want_labels) and np.array_equal(basemap[a:b], want_map)
    empty = MoveBatch.from_reads([])
    assert empty.n_reads == 0 and empty.n_events == 0 and empty.total == 0 and empty.label_host().size == 0
    for (k, name), (batch, want) in golden_batches().items():
        assert batch.kmer == k and batch.lengths.dtype.name == name and np.array_equal(batch.label_host(), want)
    assert len(golden_batches()) == 6
    batches = edge_batches()
    assert [int(n) for n in np.diff(batches["P - 1, P and P + 1 events"].event_offsets)] == [PIECE - 1, PIECE, PIECE + 1]
    b = batches["stays across a piece border"]
    second = 2 * PIECE + 9
    assert b.moves[PIECE - 5] and not b.moves[PIECE - 4:PIECE + 6].any() and b.moves[second + 500] and not b.moves[second + 501:second + 2 * PIECE + 100].any()
    b = batches["heads at the ends of a piece"]
    assert b.moves[PIECE - 1] and b.moves[PIECE] and b.moves[2 * PIECE - 1] and b.moves[2 * PIECE]
    assert b.moves[2 * PIECE + 2 + PIECE] and not b.moves[2 * PIECE + 2 + PIECE - 6:2 * PIECE + 2 + PIECE].any() and b.moves[-1]
    b = batches["merged-event borders at a tile border"]
    assert b.final.tolist() == [TILE - 1 + 19 * 200, TILE + 19 * 200, TILE + 1 + 19 * 200, TILE + 19 * 200, TILE - 1 + 19 * 200, TILE + 1 + 19 * 200]
    assert batches["one merged event of 8195 samples"].final.tolist() == [8195, 8195] and batches["one merged event of 8195 samples"].merged.tolist() == [1, 1]
    assert batches["4097 one-sample merged events"].final.tolist() == [4097] and batches["4097 one-sample merged events"].merged.tolist() == [4097]
    assert batches["cut by the raw signal"].final.tolist() == [1000, TILE, 2 * TILE, 12000]
    b = batches["neighbouring reads"]
    labels = b.label_host()
    so = b.sample_offsets
    assert labels[so[1] - 9:so[1]].all() and not labels[so[0]:so[1] - 9].any()                         # the last three merged events of read 0
    assert labels[so[1]:so[1] + 9].all() and not labels[so[1] + 9:so[2]].any()                         # ... and the first three of read 1: no crossing
    for name, batch in batches.items():
        assert 0 < int(batch.label_host().sum()) < batch.total, name
    wide = edge_batches(np.float64)
    assert any(not np.array_equal(wide[name].final, batches[name].final) or not np.array_equal(wide[name].label_host(), batches[name].label_host())
               for name in ("synthetic reads", "P - 1, P and P + 1 events"))                          # the dtype matters on these tables


# ---------------------------------------------------------------------------------------------------------------------------- files
def test_move_npz_round_trip(tmp_path):
    reads = [labelling.synthetic_move_read(4000 + 40 * i, 60 + i, dtype=(np.float32, np.float64)[i % 2]) for i in range(4)]
    positives = 0
    for i, (raw, states, lengths, moves) in enumerate(reads):
        path = write_move_npz(tmp_path / ("m%d.npz" % i), np.concatenate([raw, np.zeros(3 * i)]), states, lengths, moves, (10, 10) if i else None)
        read = labelling.load_move_npz(path)
        assert read["lengths"].dtype == lengths.dtype and np.array_equal(read["lengths"], lengths) and np.array_equal(read["states"], states)
        assert np.array_equal(read["moves"], moves) and read["clipped"] == ((10, 10) if i else (0, 0))
        batch = MoveBatch.from_reads([read])
        assert batch.n_raw.tolist() == [len(raw) + 3 * i]
        sig, lab = labelling.load_labelled_move_npz(path)
        want, _ = labelling.label_move_read_host(states, lengths, moves, read["clipped"], len(raw) + 3 * i)
        assert np.array_equal(lab, want) and np.array_equal(sig, np.concatenate([raw, np.zeros(3 * i)])[:want.size])
        positives += int(lab.sum())
    assert positives > 0
    np.savez(str(tmp_path / "bare.npz"), raw=np.zeros(4))
    with pytest.raises(ValueError, match="event_state"):
        labelling.load_move_npz(str(tmp_path / "bare.npz"))
    assert labelling.moves_from_env(None) is False and labelling.moves_from_env(" ") is False and labelling.moves_from_env("0") is False
    assert labelling.moves_from_env("1") is True
    with pytest.raises(ValueError, match="CATFISH_LABEL_MOVES"):
        labelling.moves_from_env("yes")


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


def _basecall_tree(case, signal, first_sample, alignment=True, group="Basecall_1D_000"):
    k = case["states"].shape[1]
    table = np.zeros(len(case["moves"]), dtype=[("mean", "<f4"), ("length", case["lengths"].dtype.str), ("model_state", "S%d" % k), ("move", "<i4")])
    table["length"], table["move"] = case["lengths"], case["moves"]
    table["model_state"] = np.ascontiguousarray(case["states"]).view("S%d" % k).reshape(-1)
    analyses = {group: _Group({"BaseCalled_template": _Group({"Events": _Dataset(table)})}),
                "Segmentation_000": _Group({"Summary": _Group({"segmentation": _Group(attrs={"first_sample_template": np.int64(first_sample)})})})}
    if alignment:
        analyses["RawGenomeCorrected_000"] = _Group({"BaseCalled_template": _Group({"Alignment": _Group(attrs={
            "clipped_bases_start": np.int64(case["clipped"][0]), "clipped_bases_end": np.int64(case["clipped"][1])})})})
    return _Group({"Analyses": _Group(analyses), "Raw": _Group({"Reads": _Group({"Read_9": _Group({"Signal": _Dataset(signal)})})})})


def test_convert_moves_through_a_stand_in_h5py(tmp_path, monkeypatch):
    from catfish_amd import convert, infer
    registry = {}
    h5py = types.ModuleType("h5py")

    def open_file(path, mode="r"):
        if path not in registry:
            raise OSError("Unable to open file (file signature not found)")
        return registry[path]

    h5py.File = open_file
    monkeypatch.setitem(sys.modules, "h5py", h5py)
    rng = np.random.default_rng(47)
    for i, case in enumerate(golden_cases()):
        src, dst = str(tmp_path / ("read%d.fast5" % i)), str(tmp_path / ("read%d.npz" % i))
        open(src, "wb").write(b"stand-in, never parsed")
        first = int(rng.integers(0, 12))
        signal = rng.integers(200, 900, size=first + case["n_raw"]).astype(np.int16)
        registry[src] = _basecall_tree(case, signal, first)
        assert convert.convert_moves(src, dst, clipped_bases=99) == len(case["labels"])
        read = labelling.load_move_npz(dst)
        assert read["clipped"] == case["clipped"] and read["lengths"].dtype == case["lengths"].dtype and np.array_equal(read["lengths"], case["lengths"])
        assert np.array_equal(read["states"], case["states"]) and np.array_equal(read["moves"], case["moves"])
        assert np.array_equal(read["raw"], infer.normalize_raw_signal(signal[first:], "median"))      # the whole trimmed signal: it is n_raw
        raw, labels = labelling.load_labelled_move_npz(dst)
        assert np.array_equal(labels, case["labels"]) and len(raw) == len(labels)
    case = golden_cases()[4]
    src = str(tmp_path / "default.fast5")
    open(src, "wb").write(b"x")
    signal = rng.integers(200, 900, size=case["n_raw"]).astype(np.int16)
    registry[src] = _basecall_tree(dict(case, clipped=(0, 0)), signal, 0, alignment=False)
    convert.convert_moves(src, str(tmp_path / "default.npz"))
    assert labelling.load_move_npz(str(tmp_path / "default.npz"))["clipped"] == (10, 10)             # the reference's --clipped-bases default
    short = golden_cases()[3]
    assert 1 + np.count_nonzero(short["moves"][1:]) == 7
    registry[src] = _basecall_tree(short, rng.integers(200, 900, size=short["n_raw"]).astype(np.int16), 0, alignment=False)
    with pytest.raises(ValueError, match="clipped"):                                                  # ... which a read of 7 merged events cannot give
        convert.convert_moves(src, str(tmp_path / "default.npz"))
    convert.convert_moves(src, str(tmp_path / "default.npz"), clipped_bases=1)
    assert labelling.load_move_npz(str(tmp_path / "default.npz"))["clipped"] == (1, 1)
    registry[src] = _basecall_tree(case, signal, 0, group="Basecall_1D_001")
    convert.convert_moves(src, str(tmp_path / "other.npz"), hdf_path="Analyses/Basecall_1D_001")
    with pytest.raises(ValueError, match="hdf path"):
        convert.convert_moves(src, str(tmp_path / "other.npz"))
    # the directory walk and the flag
    out, only = tmp_path / "out", tmp_path / "only"
    only.mkdir()
    open(str(only / "a.fast5"), "wb").write(b"x")
    registry[str(only / "a.fast5")] = _basecall_tree(golden_cases()[20], rng.integers(200, 900, size=golden_cases()[20]["n_raw"]).astype(np.int16), 0)
    assert convert.main(["-i", str(only), "-o", str(out), "--moves"]) == 0
    assert sorted(os.listdir(str(out))) == ["a.npz"]
    with pytest.raises(ValueError, match="path to FAST5 is not correct"):
        convert.convert_moves(str(tmp_path / "nope.fast5"), str(tmp_path / "nope.npz"))
    monkeypatch.setitem(sys.modules, "h5py", None)
    with pytest.raises(ImportError, match="needs h5py"):
        convert.convert_moves(src, str(tmp_path / "t.npz"))
