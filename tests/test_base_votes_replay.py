"""The bodies of base_votes_vote_kernel and base_votes_count_kernel on the CPU under AddressSanitizer + UBSan:
tests/native/base_votes_replay.cpp walks both grids serially through csrc/base_votes_rule.hpp -- the rules by which the kernels form
their addresses and the vote's fixed point -- with every buffer malloc'ed at exactly the size the Python layer allocates.  A
stand-alone program run as its own process; nothing is preloaded.  Its output must EQUAL ``base_votes.vote_host`` on the GPU test's
batches, whatever the grid and the long-base constant; forged device tables (edges that decrease, repeat, go negative or run past the
total, base ranges outside the table, stretches that leave the set) must be written inside the buffers only and give the "unvoted"
result of the definition; refused arguments give the refusal; and the sanitizers must have nothing to say."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import base_votes as bv
from catfish_amd import device_validation as dv
from test_base_votes_host import RECIPE_THRESHOLDS, SHAPE_THRESHOLDS, recipe_batch, shape_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("base_votes") / "base_votes_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "base_votes_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def tables_of(vset, selection, packed, window=35):
    """{name: array} of one call as the Python layer uploads it, copies: the set's arrays, the selection's tables, the host's ranges."""
    src = vset.offsets[selection[0]] + selection[1]
    bounds, _tails = dv.layout(selection[2], window)
    a, b = bv.event_ranges(vset.bases.edges, src, selection[2])
    return {"edges": vset.bases.edges.copy(), "labels": vset.labels.copy(), "basemap": vset.basemap.copy(), "src": src.astype(np.int64),
            "length": selection[2].astype(np.int64), "bounds": bounds.astype(np.int64), "ranges": np.concatenate((a, b)).astype(np.int64),
            "probs": np.ascontiguousarray(packed, dtype=np.float32)}


def replayed(exe, tmp_path, t, thresholds, max_bases, long_base=bv.LONG_BASE, grid=(0, 0), work_bytes=-1, **forged):
    """``t`` as ``tables_of`` gives them, unchecked -> None when the arguments are refused, else (sums, state, confusion, runs) as the
    program left them.  ``forged``: header sizes that differ from the arrays (n, total, n_bases, set_total, k, max_bases)."""
    n, k = int(t["src"].size), len(thresholds)
    head = {"n": n, "total": int(t["probs"].size), "n_bases": int(t["edges"].size) - 1, "set_total": int(t["labels"].size), "k": k,
            "max_bases": max_bases}
    head.update(forged)
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as fh:
        np.array([head["n"], head["total"], head["n_bases"], head["set_total"], head["k"], head["max_bases"], work_bytes,
                  int(np.diff(t["ranges"].reshape(2, -1), axis=0).max()) if n else 0, long_base, grid[0], grid[1], int(t["edges"].size)], np.int64).tofile(fh)
        for name, dtype in (("edges", np.int64), ("labels", np.uint8), ("basemap", np.uint8), ("src", np.int64), ("length", np.int64),
                            ("bounds", np.int64), ("ranges", np.int64)):
            np.asarray(t[name], dtype).tofile(fh)
        np.asarray(thresholds, np.float64).tofile(fh)
        np.asarray(t["probs"], np.float32).tofile(fh)
    run = subprocess.run([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    with open(out, "rb") as fh:
        refusal = int(np.fromfile(fh, np.int64, 1)[0])
        if refusal:
            assert fh.read() == b""
            return None
        n_bases = head["n_bases"]
        sums = np.fromfile(fh, np.uint64, n_bases)
        state = np.fromfile(fh, np.uint8, k * n_bases).reshape(k, n_bases)
        confusion = np.fromfile(fh, np.int64, k * 20).reshape(k, 5, 2, 2)
        runs = np.fromfile(fh, np.int64, k * 2 * 3 * 5 * (max_bases + 1)).reshape(k, 2, 3, 5, max_bases + 1)
        assert fh.read() == b""
    return sums, state, confusion, runs


def defined(t, thresholds, max_bases):
    """``vote_host`` on the same tables, trusted no more than the card trusts them."""
    return bv.vote_host(t["probs"], t["edges"], t["labels"], t["basemap"], t["src"], t["length"], t["bounds"], thresholds, max_bases,
                        t["ranges"].reshape(2, -1))


def same(got, want):
    return got is not None and all(a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a, b) for a, b in zip(got, want))


def test_the_constants_of_the_rule_header_are_the_modules():
    with open(os.path.join(ROOT, "catfish_amd", "csrc", "base_votes_rule.hpp")) as fh:
        text = fh.read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))           # noqa: E731
    assert value("BV_LONG_BASE") == bv.LONG_BASE and value("BV_MAX_K") == bv.MAX_THRESHOLDS == dv.MAX_THRESHOLDS
    assert value("BV_MAX_BASES") == dv.MAX_BASES_LIMIT and value("BV_CLASSES") == len(dv.BASE_CLASSES)


def test_the_library_asks_for_the_work_buffer_the_rule_header_sizes():
    from catfish_amd import _native
    lib = _native.lib()
    for n_bases, k in ((0, 1), (1, 1), (2, 8), (100, 16), (973, 3), (2 ** 31 - 1, 16)):
        assert lib.cf_base_votes_work_bytes(n_bases, k) == bv.work_bytes(n_bases, k)
    for n_bases, k in ((-1, 1), (2 ** 31, 1), (5, 0), (5, 17)):
        assert lib.cf_base_votes_work_bytes(n_bases, k) == -1


def test_the_gpu_batches_equal_the_host(replay, tmp_path):
    vset, selection, packed = shape_batch()
    t = tables_of(vset, selection, packed)
    for k0, k1 in ((0, 16), (16, 17), (0, 1)):
        for max_bases in (16, 32, 1):
            want = defined(t, SHAPE_THRESHOLDS[k0:k1], max_bases)
            assert same(replayed(replay, tmp_path, t, SHAPE_THRESHOLDS[k0:k1], max_bases), want), (k0, k1, max_bases)
    want = defined(t, SHAPE_THRESHOLDS[:3], 16)
    for long_base, grid in ((64, (0, 0)), (0, (0, 0)), (10 ** 6, (0, 0)), (bv.LONG_BASE, (3, 2)), (1, (1, 1)), (4096, (7, 7))):
        assert same(replayed(replay, tmp_path, t, SHAPE_THRESHOLDS[:3], 16, long_base=long_base, grid=grid), want), (long_base, grid)
    vset, selection, packed, _reads = recipe_batch()
    t = tables_of(vset, selection, packed)
    assert same(replayed(replay, tmp_path, t, RECIPE_THRESHOLDS, 16), defined(t, RECIPE_THRESHOLDS, 16))
    assert same(replayed(replay, tmp_path, t, RECIPE_THRESHOLDS, 16, work_bytes=(8 + 3) * vset.bases.n_bases), defined(t, RECIPE_THRESHOLDS, 16))


def test_forged_device_tables(replay, tmp_path):
    vset, selection, packed, _reads = recipe_batch()
    clean = tables_of(vset, selection, packed)
    n, n_bases, total, set_total = 3, vset.bases.n_bases, int(clean["probs"].size), int(clean["labels"].size)
    honest = defined(clean, RECIPE_THRESHOLDS, 16)
    a = clean["ranges"][:n]
    forgeries = []

    def forge(name, what, index, value):
        t = {key: array.copy() for key, array in clean.items()}
        t[what][index] = value
        forgeries.append((name, t))

    forge("edges that decrease", "edges", a[0] + 5, clean["edges"][a[0] + 3])
    forge("edges that repeat", "edges", a[1] + 7, clean["edges"][a[1] + 6])
    forge("a negative edge", "edges", a[2] + 4, -17)
    forge("a hugely negative edge", "edges", a[2] + 4, -2 ** 62)
    forge("an edge past the total", "edges", a[1] + 9, set_total + 1000)
    forge("a huge edge", "edges", a[1] + 9, 2 ** 62)
    forge("the last edge past the total", "edges", n_bases, set_total + 1)
    forge("a first edge below zero", "edges", 0, -5)
    forge("a range that begins below the table", "ranges", 0, -50)
    forge("a range that ends past the table", "ranges", n + 1, n_bases + 1000)
    forge("a range that is the whole table and more", "ranges", slice(0, 2 * n), [-2 ** 40, 0, 5, 2 ** 40, n_bases, 3])
    forge("a range turned round", "ranges", slice(0, 2 * n), np.concatenate((clean["ranges"][n:], clean["ranges"][:n])))
    forge("a start outside the set", "src", 1, set_total + 35)
    forge("a negative start", "src", 0, -100)
    forge("a huge start", "src", 2, 2 ** 62)
    forge("a length that leaves the set", "length", 2, set_total)
    forge("a negative length", "length", 1, -1)
    forge("a huge length", "length", 0, 2 ** 62)
    forge("a packed place past the probabilities", "bounds", 2, total - 100)
    forge("a negative packed place", "bounds", 1, -35)
    forge("a huge packed place", "bounds", 0, 2 ** 62)
    t = {key: array.copy() for key, array in clean.items()}
    t["edges"][:] = t["edges"][::-1].copy()
    forgeries.append(("all edges descending", t))
    t = {key: array.copy() for key, array in clean.items()}
    t["edges"][:] = 7
    forgeries.append(("all edges equal", t))
    changed = 0
    for name, t in forgeries:
        want = defined(t, RECIPE_THRESHOLDS, 16)
        for long_base, grid in ((bv.LONG_BASE, (0, 0)), (0, (2, 2))):
            got = replayed(replay, tmp_path, t, RECIPE_THRESHOLDS, 16, long_base=long_base, grid=grid)     # ... and a silent sanitizer
            assert same(got, want), name
        sums, state, confusion, runs = want
        voted = (state[0] & bv.VOTED) != 0
        assert np.all(sums[~voted] == 0) and np.all(state[:, ~voted] == 0), name
        assert confusion[0].sum() == voted.sum(), name                                  # a base counts for the stretch that votes it, only
        changed += int(not same(want, honest))
    assert changed >= len(forgeries) // 2                     # (a range forged wider changes nothing: no other stretch's base is taken)
    # what an unsound base does: it is unvoted, breaks the run it was in, and the bases around it stay as they were
    t = {key: array.copy() for key, array in clean.items()}
    truth = (honest[1][0] & (bv.VOTED | bv.TRUTH)) == (bv.VOTED | bv.TRUTH)
    inside = int(np.flatnonzero(truth[1:-1] & truth[:-2] & truth[2:])[0]) + 1          # a base in the middle of a true run
    t["edges"][inside + 1] = t["edges"][inside]                                         # it has no sample now; its neighbour is whole
    got = replayed(replay, tmp_path, t, RECIPE_THRESHOLDS, 16)
    assert same(got, defined(t, RECIPE_THRESHOLDS, 16))
    assert got[1][0][inside] == 0 and got[0][inside] == 0 and got[2][0].sum() == honest[2][0].sum() - 1
    assert np.array_equal(np.delete(got[1], inside, axis=1), np.delete(honest[1], inside, axis=1))
    assert got[3][0, 0].sum() == honest[3][0, 0].sum() + 1                               # one true run became two


def test_refused_arguments(replay, tmp_path):
    vset, selection, packed, _reads = recipe_batch()
    t = tables_of(vset, selection, packed)
    assert replayed(replay, tmp_path, t, (0.5,), 16) is not None
    floor = (8 + 1) * vset.bases.n_bases
    for change in (dict(n=-1), dict(total=-1), dict(n_bases=-1), dict(set_total=-1), dict(n=2 ** 31), dict(total=2 ** 31), dict(n_bases=2 ** 31),
                   dict(set_total=2 ** 31), dict(k=0), dict(k=17), dict(k=-1), dict(k=2 ** 32 + 1), dict(max_bases=0), dict(max_bases=33),
                   dict(max_bases=-1), dict(max_bases=2 ** 32 + 16), dict(work_bytes=floor - 1), dict(work_bytes=0)):
        assert replayed(replay, tmp_path, t, (0.5,), **dict({"max_bases": 16}, **change)) is None, change
    assert replayed(replay, tmp_path, t, (0.5,), 16, work_bytes=floor) is not None
    # zero voted work: the zeroed tables
    empty = {"edges": np.int64([0]), "labels": np.zeros(0, np.uint8), "basemap": np.zeros(0, np.uint8), "src": np.zeros(0, np.int64),
             "length": np.zeros(0, np.int64), "bounds": np.int64([0]), "ranges": np.zeros(0, np.int64), "probs": np.zeros(0, np.float32)}
    sums, state, confusion, runs = replayed(replay, tmp_path, empty, (0.5, 0.7), 16)
    assert sums.size == 0 and state.size == 0 and not confusion.any() and not runs.any() and runs.shape == (2, 2, 3, 5, 17)
    nothing = dict(t, ranges=np.zeros(6, np.int64))
    got = replayed(replay, tmp_path, nothing, (0.5,), 16)
    assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
