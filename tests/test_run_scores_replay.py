"""The two score kernels' bodies on the CPU under AddressSanitizer + UBSan: tests/native/validation_scores_replay.cpp paints every
stretch word by word through csrc/validation_scores_word.hpp -- mirrored, then forward, in pieces of a size given on the command
line, with masks and paint in exactly sized malloc'ed buffers -- and bins every sample with the key rule.  A stand-alone program run
as its own process; nothing is preloaded.  Its table must equal ``device_validation.run_scores_host`` on the golden stretches and on
the planted batch the GPU test uses (tests/test_run_scores_gpu.py imports it from here), and the sanitizers must have nothing to
say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd.infer import correct_short
from test_run_states_host import golden, packed
from test_run_states_replay import PIECE, PIECES, planted_stretches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted_batch(piece, window=35):
    """(probs, y, bounds, lengths): the structure of ``planted_stretches`` with seeded probabilities in place of its three levels --
    called samples (levels 1 and 2) uniform in [0.5, 1], the others uniform in [0, 0.5) -- so the corrected prediction at threshold
    0.5 and min_run 1 is the planted one.  Every fourth stretch holds ONE value per level (thousands of equal keys for the sort); the
    exact values 0.0, 0.5, 1.0 and nextafter(0.5, 0), one NaN and one value above 1 are planted where they keep the call."""
    stretches = planted_stretches(piece)
    rng = np.random.default_rng(20261020)
    lengths = np.array([len(c) for c, _ in stretches], dtype=np.int64)
    bounds, _tails = dv.layout(lengths, window)
    probs = np.full(int(bounds[-1]), 0.9, dtype=np.float32)                   # 0.9 in the zero tails: a tail taken for a sample shows
    y = np.zeros(int(bounds[-1]), dtype=np.uint8)
    below = np.nextafter(np.float32(0.5), np.float32(0.0))
    for index, (b, (called, truth)) in enumerate(zip(bounds[:-1].tolist(), stretches)):
        n = len(called)
        if index % 4 == 3:
            high, low = np.float32(rng.uniform(0.5, 1.0)), np.float32(rng.uniform(0.0, 0.5))
            p = np.where(called > 0, high, np.minimum(low, below)).astype(np.float32)
        else:
            p = np.where(called > 0, rng.uniform(0.5, 1.0, size=n), np.minimum(rng.uniform(0.0, 0.5, size=n).astype(np.float32), below))
            p = p.astype(np.float32)
        on, off = np.flatnonzero(called > 0), np.flatnonzero(called == 0)
        if on.size >= 4:
            p[on[:2]] = (0.5, 1.0)
        if off.size >= 4:
            p[off[:2]] = (0.0, below)
        probs[b:b + n] = p
        y[b:b + n] = truth
    big = int(np.argmax(lengths))                          # in the longest stretch: a NaN (not called) and 1.5 (called) where they keep the call
    called = stretches[big][0]
    probs[int(bounds[big]) + int(np.flatnonzero(called == 0)[5])] = np.nan
    probs[int(bounds[big]) + int(np.flatnonzero(called > 0)[5])] = 1.5
    for b, (called, _truth) in zip(bounds[:-1].tolist(), stretches):
        assert np.array_equal(probs[b:b + len(called)] >= 0.5, called > 0)
    return probs, y, bounds, lengths


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("validation_scores") / "validation_scores_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "validation_scores_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def case_file(tmp_path, batch, threshold, min_run):
    """The batch as the program reads it: per stretch its length, its labels, its corrected prediction at one threshold, its scores."""
    probs, y, bounds, lengths = batch
    case = str(tmp_path / ("case_%r_%d.bin" % (threshold, min_run)))
    with open(case, "wb") as fh:
        np.array([len(lengths)], np.int64).tofile(fh)
        for b0, n in zip(bounds[:-1].tolist(), lengths.tolist()):
            np.array([n], np.int64).tofile(fh)
            y[b0:b0 + n].tofile(fh)
            if n:
                np.asarray(correct_short((probs[b0:b0 + n].astype(np.float64) >= threshold).astype(np.int64), min_run)).astype(np.uint8).tofile(fh)
            probs[b0:b0 + n].astype(np.float32).tofile(fh)
    return case


def replayed(exe, case, piece, shift):
    run = subprocess.run([exe, case, str(piece), str(shift)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    table = np.zeros((6, dv.curve_bins(shift) + 1), dtype=np.int64)
    for line in run.stdout.splitlines():
        row, cell, count = (int(v) for v in line.split())
        table[row, cell] = count
    return table.reshape(2, 3, -1)


def test_the_golden_batch(replay, tmp_path):
    scores, labels, offsets, _cases = golden()
    batch = packed([(scores[a:b], labels[a:b]) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())])
    for min_run in (15, 1):
        want = {shift: dv.run_scores_host(*batch, (0.3, 0.5, 0.9), shift, min_run) for shift in (16, 22)}
        assert want[16][:2, :, :, :-1].sum(axis=-1).min() >= 20       # no empty row at 0.3 and 0.5
        for k, t in enumerate((0.3, 0.5, 0.9)):
            case = case_file(tmp_path, batch, t, min_run)
            for piece in PIECES:                           # 1 and 3 words: these short stretches cross piece borders too
                shift = 16 if piece == 3 else 22
                assert np.array_equal(replayed(replay, case, piece, shift), want[shift][k]), (min_run, t, piece)


def test_the_planted_batch(replay, tmp_path):
    batch = planted_batch(PIECE)
    for min_run in (15, 1):
        want = {shift: dv.run_scores_host(*batch, (0.5,), shift, min_run)[0] for shift in (14, 22)}
        assert want[14][:, :, :-1].sum(axis=-1).min() >= 20           # every (kind, state) row
        case = case_file(tmp_path, batch, 0.5, min_run)
        for piece in PIECES:
            shift = 14 if piece == 64 else 22
            assert np.array_equal(replayed(replay, case, piece, shift), want[shift]), (min_run, piece)
