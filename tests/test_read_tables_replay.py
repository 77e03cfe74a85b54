"""A card side for device_db.DeviceReadDb, settled on the CPU under AddressSanitizer + UBSan before any kernel runs on a card:
tests/native/read_tables_replay.cpp states the three kernel bodies (count, fill, gather) serially, forms every index through
csrc/read_tables_plan.hpp -- the functions such kernels are to call -- and mallocs every buffer at exactly the size the Python layer
would allocate.  A stand-alone program run as its own process; nothing is preloaded.

* its tables equal device_db.centre_tables and its counts the brute-force loop's, on every edge of the rule and around every piece
  border, under every lessen and negative rule;
* its batches equal DeviceReadDb.gather bit for bit at the benchmark's shape (8 x 20 000 samples, "positives", batches of 4096 and
  256) for draws 0..63 and across the 32-bit wrap of the draw counter;
* a table entry of total - 34 and a row count one too large are REFUSED: the slot is zeroed, the status says so, the program exits 3
  and the sanitizers have nothing to report.  The guard is exercised here and never on a GPU.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import device_db as ddb
from test_read_db_host import LESSENS, NEG_RULES, brute_force, case_reads, chunk_edge_reads, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZER_WORDS = ("AddressSanitizer", "runtime error", "LeakSanitizer")


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("read_tables") / "read_tables_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "read_tables_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def _rule(neg_per_read):
    return (0, 0) if neg_per_read is None else (2, 0) if neg_per_read == "positives" else (1, int(neg_per_read))


def run_case(exe, tmp_path, signal, labels, offsets, lessen, neg_per_read, table_seed, seed, batches=(), forged=None, name="case"):
    """-> (exit status, output text, dict(n_pos, n_neg, counts, pos, neg, batches=[(x, is_pos, status), ...]))."""
    case, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".out"))
    mode, value = _rule(neg_per_read)
    with open(case, "wb") as fh:
        np.array([len(offsets) - 1, labels.size, lessen, mode, value, table_seed, seed, len(batches), int(forged is not None)], np.int64).tofile(fh)
        np.asarray(offsets, np.int64).tofile(fh)
        np.asarray(labels, np.uint8).tofile(fh)
        np.asarray(signal, np.float32).tofile(fh)
        np.asarray(list(batches), np.int64).reshape(-1, 3).tofile(fh)
        for claim, table in (forged or ()):
            np.array([claim, len(table)], np.int64).tofile(fh)
            np.asarray(table, np.int64).tofile(fh)
    run = subprocess.run([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    raw = np.fromfile(out, np.uint8) if os.path.exists(out) else np.zeros(0, np.uint8)
    got, at = {}, [0]

    def take(dtype, count):
        size = np.dtype(dtype).itemsize * count
        part = raw[at[0]:at[0] + size].view(dtype)
        assert part.size == count, "short output: " + run.stdout
        at[0] += size
        return part

    if run.returncode in (0, 3):
        got["n_pos"], got["n_neg"] = (int(v) for v in take(np.int64, 2))
        got["counts"] = take(np.uint32, 2 * (len(offsets) - 1)).reshape(-1, 2)
        got["pos"], got["neg"] = take(np.int64, got["n_pos"]), take(np.int64, got["n_neg"])
        got["batches"] = [(take(np.float32, size * 35).reshape(size, 35), take(np.uint8, size).astype(bool), take(np.int32, 2))
                          for _, size, _ in batches]
        assert at[0] == raw.size
    return run.returncode, run.stdout, got


def _counts_by_hand(labels, offsets, lessen):
    """Per read (positives, candidates) of the brute-force loop."""
    out = []
    for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        pos, _, per_read = brute_force(labels[a:b], np.array([0, b - a]), lessen, None, 0)
        out.append((len(pos), len(per_read[0][0])))
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


@pytest.mark.parametrize("reads", ["case_reads", "chunk_edge_reads"])
def test_replayed_tables_equal_centre_tables(replay, tmp_path, reads):
    assert ddb.TABLE_PIECE == 1024                                  # chunk_edge_reads places its edges on the piece borders
    signal, labels, offsets = pack({"case_reads": case_reads, "chunk_edge_reads": chunk_edge_reads}[reads](), seed=3)
    for lessen in LESSENS:
        by_hand = _counts_by_hand(labels, offsets, lessen)
        for rule in NEG_RULES:
            want_pos, want_neg = ddb.centre_tables(labels, offsets, lessen, rule, seed=9)
            batches = [(0, 7, 2), (1, 6, 3)] if rule is None else []
            rc, text, got = run_case(replay, tmp_path, signal, labels, offsets, lessen, rule, 9, 11, batches)
            assert rc == 0 and not any(w in text for w in SANITIZER_WORDS), (lessen, rule, text)
            assert np.array_equal(got["pos"], want_pos) and np.array_equal(got["neg"], want_neg), (lessen, rule)
            assert np.array_equal(got["counts"], by_hand), (lessen, rule)
            db = ddb.DeviceReadDb(signal, labels, offsets, seed=11, lessen=lessen)
            for (d, size, ratio), (x, is_pos, status) in zip(batches, got["batches"]):
                want_x, want_is_pos = db.gather(d, size, ratio)
                assert np.array_equal(x.view(np.uint32), want_x.view(np.uint32)) and np.array_equal(is_pos, want_is_pos)
                assert status.tolist() == [0, 0]


def test_replayed_empty_and_shortest_reads(replay, tmp_path):
    for lengths, want in (((), (0, 0)), ((34,), (0, 0)), ((35,), (1, 0))):
        signal, labels, offsets = pack([np.ones(n, np.uint8) for n in lengths])
        rc, text, got = run_case(replay, tmp_path, signal, labels, offsets, 1, None, 0, 0)
        assert rc == 0 and not any(w in text for w in SANITIZER_WORDS), text
        assert (got["n_pos"], got["n_neg"]) == want and got["pos"].tolist() == [0] * want[0]


def test_replayed_batches_at_the_benchmark_shape(replay, tmp_path):
    """8 reads of 20 000 samples, as many negatives as positives per read: batches of 4096 and of 256, draws 0 .. 63 and the four
    draws around 2^32 (the card's counter is 64 bits wide, the sampler uses its low 32)."""
    db = ddb.synthetic_device_read_db(8, 20000, seed=0, neg_per_read="positives")
    assert (db.nb_pos, db.nb_neg) == (7188, 7188)
    draws = list(range(64)) + [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    batches = [(d, size, 2) for size in (4096, 256) for d in draws]
    rc, text, got = run_case(replay, tmp_path, db.signal, db.labels, db.offsets, 1, "positives", db.seed, db.seed, batches)
    assert rc == 0 and not any(w in text for w in SANITIZER_WORDS), text
    assert np.array_equal(got["pos"], db.pos_start) and np.array_equal(got["neg"], db.neg_start)
    for (d, size, ratio), (x, is_pos, status) in zip(batches, got["batches"]):
        want_x, want_is_pos = db.gather(d, size, ratio)
        assert np.array_equal(x.view(np.uint32), want_x.view(np.uint32)) and np.array_equal(is_pos, want_is_pos), (d, size)
        assert status.tolist() == [0, 0]
    assert np.array_equal(got["batches"][66][0], got["batches"][0][0])          # draw 2^32 is draw 0


def test_forged_tables_are_refused_without_an_out_of_range_access(replay, tmp_path):
    """A start of total - 34 (its 35th sample would be signal[total]) and a row count one above the table's entries: every row is
    drawn (the positive share is the whole table), the bad one is skipped -- zeros in its slot, code and slot in status, exit 3 --
    and neither sanitizer reports anything."""
    db = ddb.synthetic_device_read_db(2, 6000, seed=3)
    assert (db.nb_pos, db.nb_neg) == (583, 10455)
    total = db.signal.size
    pos, neg = db.pos_start.copy(), db.neg_start
    # 1. a start one past the last window that fits
    bad = pos.copy()
    bad[100] = total - 34
    rc, text, got = run_case(replay, tmp_path, db.signal, db.labels, db.offsets, 1, None, db.seed, db.seed, [(0, 2 * 583, 2)],
                             forged=[(583, bad), (len(neg), neg)], name="start")
    assert rc == 3 and "skip: window start" in text and not any(w in text for w in SANITIZER_WORDS), text
    x, is_pos, status = got["batches"][0]
    want_x, want_is_pos = db.gather(0, 2 * 583, 2)
    slot = int(status[1])
    assert status[0] == 2 and want_is_pos[slot] and np.array_equal(want_x[slot], db.signal[pos[100]:pos[100] + 35])
    assert not x[slot].any() and not is_pos[slot]
    keep = np.arange(2 * 583) != slot
    assert np.array_equal(x[keep].view(np.uint32), want_x[keep].view(np.uint32)) and np.array_equal(is_pos[keep], want_is_pos[keep])
    # 2. a count that does not belong to the table: 584 rows claimed, 583 allocated
    rc, text, got = run_case(replay, tmp_path, db.signal, db.labels, db.offsets, 1, None, db.seed, db.seed, [(0, 2 * 584, 2)],
                             forged=[(584, pos), (len(neg), neg)], name="row")
    assert rc == 3 and "skip: table row" in text and not any(w in text for w in SANITIZER_WORDS), text
    x, is_pos, status = got["batches"][0]
    assert status[0] == 1 and not x[int(status[1])].any() and int(is_pos.sum()) == 583
    # and the same two tables unforged pass
    rc, text, got = run_case(replay, tmp_path, db.signal, db.labels, db.offsets, 1, None, db.seed, db.seed, [(0, 2 * 583, 2)],
                             forged=[(583, pos), (len(neg), neg)], name="fine")
    assert rc == 0 and np.array_equal(got["batches"][0][0].view(np.uint32), want_x.view(np.uint32)), text
