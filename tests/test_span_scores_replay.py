"""span_scores_kernel's body on the CPU under AddressSanitizer + UBSan: tests/native/span_scores_replay.cpp walks every run through
csrc/span_scores_rule.hpp -- the rules by which the kernel forms its addresses -- with every buffer malloc'ed at exactly the size the
Python layer allocates.  A stand-alone program run as its own process; nothing is preloaded.  Its rows must equal
``span_scores.span_scores_host`` on the planted batch (all thresholds and min_run of the GPU test), hostile start lists must give
empty rows or correct walks, and the sanitizers must have nothing to say."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd.span_scores import scores_from_device_rows, span_scores_host
from test_span_scores_host import MIN_RUNS, THRESHOLDS, brute_force, check_rows, planted_batch, random_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7777


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("span_scores") / "span_scores_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "span_scores_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def replayed(exe, tmp_path, batch, threshold, starts, count, with_signal=True):
    """-> (ends_paired [max_runs], sums [max_runs, 3], extremes [max_runs, 2]) as the program left them."""
    probs, signal, offsets, lengths = batch
    starts = np.asarray(starts, dtype=np.int64)
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "rows.bin")
    with open(case, "wb") as fh:
        np.array([len(lengths), len(probs), len(starts), count, int(with_signal)], np.int64).tofile(fh)
        np.array([np.float32(threshold)], np.float32).tofile(fh)
        np.zeros(1, np.uint32).tofile(fh)
        np.asarray(offsets, np.int64).tofile(fh)
        np.asarray(lengths, np.int64).tofile(fh)
        starts.tofile(fh)
        np.asarray(probs, np.float32).tofile(fh)
        if with_signal:
            np.asarray(signal, np.float32).tofile(fh)
    run = subprocess.run([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    m = len(starts)
    with open(out, "rb") as fh:
        ends = np.fromfile(fh, np.int64, m)
        sums = np.fromfile(fh, np.float64, 3 * m).reshape(m, 3)
        extremes = np.fromfile(fh, np.float32, 2 * m).reshape(m, 2)
    return ends, sums, extremes


def hostile_starts(batch, threshold=0.5):
    """(starts, what each row must be): -1, total, total + 5, a position in padding, a position in the middle of a run -- and
    one honest start.  ``None`` = an empty row; (start, end) = a walk."""
    probs, _signal, offsets, lengths = batch
    total = len(probs)
    want = span_scores_host(*batch, threshold, 15)
    k = int(np.argmax(want["end"] - want["start"]))          # the longest run
    mid = int(want["start"][k]) + 77
    padding = int(offsets[0] + lengths[0]) + 3                # 0.99 planted there
    assert probs[padding] == np.float32(0.99) and padding < offsets[1]
    starts = [-1, total, total + 5, padding, mid, int(want["start"][0]), np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    expect = [None, None, None, None, (mid, int(want["end"][k])), (int(want["start"][0]), int(want["end"][0])), None, None]
    return starts, expect


def check_hostile_rows(batch, starts, expect, ends, sums, extremes, with_signal=True):
    probs, signal, _offsets, _lengths = batch
    for k, (s, e) in enumerate(zip(starts, expect)):
        if e is None:
            assert ends[k] == s and sums[k, 0] == 0.0 and extremes[k, 0] == np.inf and extremes[k, 1] == -np.inf, (k, s)
            assert not with_signal or (sums[k, 1] == 0.0 and sums[k, 2] == 0.0)
            continue
        assert ends[k] == e[1]
        p, x = probs[e[0]:e[1]], signal[e[0]:e[1]].astype(np.float64)
        assert extremes[k, 0] == p.min() and extremes[k, 1] == p.max()
        for got, v in ((sums[k, 0], p.astype(np.float64)),) + (((sums[k, 1], x), (sums[k, 2], x * x)) if with_signal else ()):
            assert abs(got - math.fsum(v.tolist())) <= len(v) * 2.0 ** -53 * math.fsum(np.abs(v).tolist())


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_the_planted_batch(replay, tmp_path, threshold):
    batch = planted_batch()
    offsets, lengths = batch[2], batch[3]
    rng = np.random.default_rng(3)
    for min_run in MIN_RUNS:
        want = span_scores_host(*batch, threshold, min_run)
        n = len(want["start"])
        order = rng.permutation(n)                           # the device's lists come unsorted
        starts = np.concatenate((want["start"][order], [5, 6, 7]))       # three rows above the count
        ends, sums, extremes = replayed(replay, tmp_path, batch, threshold, starts, n)
        assert (ends[n:] == SENTINEL).all() and (sums[n:] == SENTINEL).all() and (extremes[n:] == SENTINEL).all()
        got, _order = scores_from_device_rows(starts[:n], ends[:n], sums[:n], extremes[:n], offsets, len(lengths))
        check_rows(got, brute_force(*batch, threshold, min_run))
        assert got["min_p"].tobytes() == want["min_p"].tobytes() and got["max_p"].tobytes() == want["max_p"].tobytes()
        assert np.array_equal(got["end"], want["end"]) and np.array_equal(got["read"], want["read"])
    # no signal: the two level columns are not written
    ends, sums, extremes = replayed(replay, tmp_path, batch, threshold, want["start"], n, with_signal=False)
    assert (sums[:, 1:] == SENTINEL).all() and np.array_equal(ends, want["end"])
    got, _order = scores_from_device_rows(want["start"], ends, sums, extremes, offsets, len(lengths), with_signal=False)
    check_rows(got, brute_force(*batch, threshold, min_run), signal=False)


def test_random_batches(replay, tmp_path):
    rng = np.random.default_rng(77)
    for _ in range(25):
        batch = random_batch(rng)
        threshold, min_run = float(rng.choice([0.5, 0.9])), int(rng.choice([1, 15, 64]))
        want = span_scores_host(*batch, threshold, min_run)
        n = len(want["start"])
        ends, sums, extremes = replayed(replay, tmp_path, batch, threshold, want["start"], n)
        got, _order = scores_from_device_rows(want["start"], ends, sums, extremes, batch[2], len(batch[3]))
        check_rows(got, brute_force(*batch, threshold, min_run))


def test_hostile_start_lists(replay, tmp_path):
    batch = planted_batch()
    starts, expect = hostile_starts(batch)
    ends, sums, extremes = replayed(replay, tmp_path, batch, 0.5, starts, len(starts))
    check_hostile_rows(batch, starts, expect, ends, sums, extremes)
    # a count larger than max_runs: max_runs rows, no more
    ends, sums, extremes = replayed(replay, tmp_path, batch, 0.5, starts[:5], 1 << 40)
    check_hostile_rows(batch, starts[:5], expect[:5], ends, sums, extremes)
    ends, sums, extremes = replayed(replay, tmp_path, batch, 0.5, starts, 2**64 - 1 - 2**63)
    check_hostile_rows(batch, starts, expect, ends, sums, extremes)
    # a count smaller than the list: the rest is untouched
    ends, sums, extremes = replayed(replay, tmp_path, batch, 0.5, starts, 2)
    assert (ends[2:] == SENTINEL).all() and (sums[2:] == SENTINEL).all() and (extremes[2:] == SENTINEL).all()
    # no reads at all, and no samples at all: every row empty, nothing loaded
    none = (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(1, np.int64), np.zeros(0, np.int64))
    ends, sums, extremes = replayed(replay, tmp_path, none, 0.5, [0, -1, 5], 3)
    assert ends.tolist() == [0, -1, 5] and (sums == 0).all() and (extremes[:, 0] == np.inf).all()
    # a read table that lies (lengths beyond the packed samples, a negative one): still inside the buffers
    probs, signal, offsets, lengths = batch
    lying = (probs, signal, offsets, np.where(np.arange(len(lengths)) % 2 == 0, np.iinfo(np.int64).max, -5).astype(np.int64))
    ends, _sums, _extremes = replayed(replay, tmp_path, lying, 0.5, [0, int(offsets[1]), int(offsets[-1]) - 1], 3)
    assert 0 < ends[0] <= offsets[1] and ends[1] == offsets[1] and ends[2] <= offsets[-1]
