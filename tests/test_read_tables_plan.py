"""The index rules for read-table kernels (catfish_amd/csrc/read_tables_plan.hpp), on the CPU.

The header, compiled with g++ through tests/native/read_tables_plan_shim.cpp, is held to what device_db.py states and to what the
such kernels' buffers allow, for every read length from 0 to 3 pieces and 40 samples and for offsets near 2^31 and 2^33:

* a read's pieces tile its window starts [0, n - 34) exactly once, and a piece past the last is empty;
* the labels a piece sees stay inside the read and cover the 35 labels of each of its windows;
* the quota is device_db._neg_quota, the read key and the bijection are device_db's;
* output slots stay inside the read's share, gather addresses inside the signal.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import device_db as ddb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL, U = ctypes.c_longlong, ctypes.c_uint
OFFSETS = (0, 2 ** 31 - 5, 2 ** 31 + 3, 2 ** 33 + 1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("read_tables_plan") / "libread_tables_plan.so")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "read_tables_plan_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    dll = ctypes.CDLL(lib)
    for name, res, args in (("shim_skip", LL, []), ("shim_n_pieces", LL, [LL]), ("shim_piece_of", None, [LL, LL, LL, ctypes.POINTER(LL)]),
                            ("shim_label_src", LL, [LL, LL, LL, LL]), ("shim_quota", U, [ctypes.c_int, LL, U, U]),
                            ("shim_read_key", U, [U, LL]), ("shim_perm", U, [U, U, U]),
                            ("shim_perm_many", None, [ctypes.POINTER(U), ctypes.c_int, U, U, ctypes.POINTER(U)]),
                            ("shim_neg_selected", ctypes.c_int, [U, U, U, U]), ("shim_count_slot", LL, [LL, LL, ctypes.c_int]),
                            ("shim_out_slot", LL, [LL, LL, U]), ("shim_row_ok", ctypes.c_int, [U, U]), ("shim_table_row", LL, [U, LL]), ("shim_window_src", LL, [LL, LL]),
                            ("shim_batch_dst", LL, [U, U, U])):
        getattr(dll, name).restype, getattr(dll, name).argtypes = res, args
    return dll


def _piece(plan, o, n, p):
    out = (LL * 4)()
    plan.shim_piece_of(o, n, p, out)
    return list(out)


def test_constants(plan):
    assert plan.shim_piece() == ddb.TABLE_PIECE == 1024 and plan.shim_window() == ddb.WINDOW and plan.shim_skip() == -1


def test_pieces_tile_the_window_starts_and_labels_stay_inside_the_read(plan):
    piece = plan.shim_piece()
    for n in range(0, 3 * piece + 41):
        starts = max(0, n - 34)
        pieces = plan.shim_n_pieces(n)
        assert pieces == -(-starts // piece), n
        for o in OFFSETS:
            at = 0
            for p in range(pieces):
                lo, hi, lab_lo, lab_hi = _piece(plan, o, n, p)
                assert lo == at == p * piece and lo < hi <= min(lo + piece, starts), (n, o, p)            # in order, no gap, no overlap
                assert lab_lo == o + lo and lab_hi == o + hi + 34 <= o + n, (n, o, p)       # every window's 35 labels, none past the read
                assert lab_hi - lab_lo <= piece + 34
                at = hi
                assert plan.shim_label_src(o, n, p, 0) == lab_lo and plan.shim_label_src(o, n, p, lab_hi - lab_lo - 1) == lab_hi - 1
                assert plan.shim_label_src(o, n, p, lab_hi - lab_lo) == -1 and plan.shim_label_src(o, n, p, -1) == -1
            assert at == starts, (n, o)
            for p in (pieces, pieces + 1, -1, 2 ** 40):                                  # nothing past the last piece
                lo, hi, lab_lo, lab_hi = _piece(plan, o, n, p)
                assert lo == hi and lab_lo == lab_hi and plan.shim_label_src(o, n, p, 0) == -1, (n, o, p)


def test_quota_is_neg_quota(plan):
    for rule, mode, value in ((None, 0, 0), ("positives", 2, 0), (0, 1, 0), (5, 1, 5), (10 ** 9, 1, 10 ** 9), (2 ** 40, 1, 2 ** 40)):
        for m in (0, 1, 4, 5, 6, 1000, 2 ** 31 - 1, 2 ** 32 - 1):
            for n_pos in (0, 1, 5, 999, 1000, 1001, 2 ** 32 - 1):
                assert plan.shim_quota(mode, value, m, n_pos) == ddb._neg_quota(rule, m, n_pos), (rule, m, n_pos)


def test_read_key_and_bijection_are_device_dbs(plan):
    with np.errstate(over="ignore"):
        for seed in (0, 9, 0xFFFFFFFF):
            for rho in (0, 1, 7, 2 ** 31 - 1, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32 + 5):
                want = ddb.fmix32(np.uint32(seed) ^ ddb.fmix32(np.uint32(((rho + 1) * 0x9E3779B9) & 0xFFFFFFFF)))
                assert plan.shim_read_key(seed, rho) == int(want), (seed, rho)
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 4, 5, 16, 17, 1000, 2 ** 31 - 1):
        i = np.arange(n, dtype=np.uint32) if n <= 1000 else np.unique(np.concatenate(
            [rng.integers(0, n, 500), [0, 1, n - 2, n - 1]])).astype(np.uint32)
        for key in (0, 1, 0x9E3779B9, 0xFFFFFFFF):
            got = np.zeros(i.size, np.uint32)
            plan.shim_perm_many(i.ctypes.data_as(ctypes.POINTER(U)), i.size, n, key, got.ctypes.data_as(ctypes.POINTER(U)))
            want = ddb.keyed_permutation(i, n, np.uint32(key))
            assert np.array_equal(got, want), (n, key)
            if n <= 1000:
                assert sorted(got.tolist()) == list(range(n))
    # the subset rule: exactly q of m, everything when q == m, nothing for a number that is no candidate's
    for m, q in ((1, 0), (1, 1), (7, 3), (1000, 999), (1000, 1000), (1000, 2000)):
        chosen = [j for j in range(m) if plan.shim_neg_selected(j, m, q, 77)]
        want = np.flatnonzero(ddb.keyed_permutation(np.arange(m, dtype=np.uint32), m, np.uint32(77)) < q).tolist() if q < m else list(range(m))
        assert chosen == want
        assert not plan.shim_neg_selected(m, m, q, 77) and not plan.shim_neg_selected(2 ** 32 - 1, m, q, 77)
    assert not plan.shim_neg_selected(0, 0, 0, 1) and not plan.shim_neg_selected(0, 2 ** 31, 2 ** 31, 1)


def test_slots_and_gather_addresses_stay_inside(plan):
    big = 2 ** 33
    for lo, hi in ((0, 0), (0, 1), (5, 9), (big, big + 3), (2 ** 31 - 2, 2 ** 31 + 2)):
        for k in (0, 1, 2, 3, 4, 2 ** 32 - 1):
            want = 1 + lo + k if lo + k < hi else -1                    # behind the table's row count in entry 0
            assert plan.shim_out_slot(lo, hi, k) == want, (lo, hi, k)
    assert plan.shim_out_slot(-1, 5, 0) == -1 and plan.shim_out_slot(5, 4, 0) == -1
    for total in (0, 34, 35, 36, 12000, 2 ** 31 + 7, 2 ** 33):
        for start in (-(2 ** 63), -1, 0, 1, total - 36, total - 35, total - 34, total - 1, total, 2 ** 63 - 1):
            want = start if 0 <= start and start + 35 <= total else -1
            assert plan.shim_window_src(start, total) == want, (start, total)
    for n in (0, 1, 583, 2 ** 31 - 1):
        for row in (0, n - 1, n, n + 1, 2 ** 32 - 1):
            if row >= 0:
                assert plan.shim_row_ok(row, n) == int(row < n)
                assert plan.shim_table_row(row, n) == (1 + row if row < n else -1)
    assert plan.shim_table_row(0, -1) == -1 and plan.shim_table_row(0, 2 ** 31) == -1 and plan.shim_table_row(5, 2 ** 40) == -1
    for size in (1, 5, 4096, 2 ** 31 - 1):
        for slot in (0, size - 1, size, 2 ** 32 - 1):
            for t in (0, 34, 35, 63):
                want = slot * 35 + t if slot < size and t < 35 else -1
                assert plan.shim_batch_dst(slot, size, t) == want
    for n_reads in (0, 1, 40, 2 ** 31 - 1):
        for rho in (-1, 0, n_reads - 1, n_reads):
            for which in (0, 1, 2):
                want = rho * 2 + which if 0 <= rho < n_reads and which < 2 else -1
                assert plan.shim_count_slot(rho, n_reads, which) == want
