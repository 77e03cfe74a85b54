"""postprocess_bridged_kernel's bit logic on the CPU under AddressSanitizer + UBSan: tests/native/post_bridge_replay.cpp replays every
wave serially over csrc/post_bridge_rule.hpp -- the 64 lanes' words with their valid / first masks, the fill, the opening, the
middle word out as labels and run boundaries.  A stand-alone program run as its own process; nothing is preloaded.  Labels and run
lists must EQUAL the host definition (``infer.bridge_gaps`` + ``correct_short`` per read) on the traps and on the random batch, for
every (max_gap, min_run) pair and both thresholds, and the sanitizers must have nothing to say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_bridge_host import PAIRS, REFUSED, THRESHOLDS, UNBRIDGED, host_bridged, random_batch, trap_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("post_bridge") / "post_bridge_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "post_bridge_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def replayed(exe, tmp_path, batch, threshold, max_gap, min_run, returncode=0):
    """-> (labels uint8 [total], starts, ends as the program listed them) or None when it refuses the pair."""
    probs, offsets, lengths = batch
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as fh:
        np.array([len(lengths), len(probs), max_gap, min_run], np.int64).tofile(fh)
        np.array([np.float32(threshold)], np.float32).tofile(fh)
        np.zeros(1, np.uint32).tofile(fh)
        np.asarray(offsets, np.int64).tofile(fh)
        np.asarray(lengths, np.int64).tofile(fh)
        np.asarray(probs, np.float32).tofile(fh)
    run = subprocess.run([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == returncode and run.stderr == "", run.stderr
    if returncode:
        return None
    with open(out, "rb") as fh:
        n_s, n_e = np.fromfile(fh, np.int64, 2).tolist()
        labels = np.fromfile(fh, np.uint8, len(probs))
        starts = np.fromfile(fh, np.int64, n_s)
        ends = np.fromfile(fh, np.int64, n_e)
    return labels, starts, ends


def check(got, want):
    labels, starts, ends = got
    assert np.array_equal(labels, want[0])
    assert np.array_equal(np.sort(starts), want[1]) and np.array_equal(np.sort(ends), want[2])


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("max_gap,min_run", PAIRS + UNBRIDGED)
def test_the_traps_and_the_random_batch(replay, tmp_path, threshold, max_gap, min_run):
    for batch in (trap_batch()[:3], random_batch()):
        check(replayed(replay, tmp_path, batch, threshold, max_gap, min_run), host_bridged(*batch, threshold, max_gap, min_run))


def test_every_gap_of_the_domain_at_min_run_15_and_1(replay, tmp_path):
    batch = trap_batch()[:3]
    for min_run in (15, 1):
        for max_gap in range(0, 65 - min_run):
            check(replayed(replay, tmp_path, batch, 0.5, max_gap, min_run), host_bridged(*batch, 0.5, max_gap, min_run))


def test_small_random_batches_packed_tightly(replay, tmp_path):
    """Short reads, most without padding, ones and gaps at every read boundary."""
    rng = np.random.default_rng(11)
    for _ in range(40):
        lengths = rng.integers(0, 90, size=int(rng.integers(1, 40)))
        pads = rng.integers(0, 3, size=len(lengths)) * (rng.random(len(lengths)) < 0.4)
        parts, offsets = [], [0]
        for n, pad in zip(lengths.tolist(), pads.tolist()):
            v = np.where(rng.random(n) < rng.choice([0.3, 0.6, 0.9]), 0.9, 0.1).astype(np.float32)
            parts += [v, np.full(pad, 0.99, np.float32)]
            offsets.append(offsets[-1] + n + pad)
        batch = (np.concatenate(parts), np.array(offsets, np.int64), lengths.astype(np.int64))
        if len(batch[0]) == 0:
            continue
        max_gap = int(rng.integers(0, 64))
        min_run = int(rng.integers(1, 65 - max_gap))
        check(replayed(replay, tmp_path, batch, 0.5, max_gap, min_run), host_bridged(*batch, 0.5, max_gap, min_run))


@pytest.mark.parametrize("max_gap,min_run", REFUSED)
def test_refused_pairs(replay, tmp_path, max_gap, min_run):
    assert replayed(replay, tmp_path, random_batch(), 0.5, max_gap, min_run, returncode=3) is None
