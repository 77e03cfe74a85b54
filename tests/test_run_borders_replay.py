"""The border kernel's body on the CPU under AddressSanitizer + UBSan: tests/native/validation_borders_replay.cpp walks every
stretch word by word through csrc/validation_borders_word.hpp -- the rules the kernel runs one word per lane -- forward and
mirrored, in pieces of a size given on the command line, with the masks in exactly sized malloc'ed buffers.  A stand-alone program
run as its own process; nothing is preloaded.  Its table must equal ``device_validation.run_borders_host`` on the golden stretches
and on the planted batch the GPU test uses (tests/test_run_borders_gpu.py imports it from here), and the sanitizers must have
nothing to say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd.infer import correct_short

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIECE = 16384                                              # CF_RUN_PIECE (csrc/validation_runs.hpp); the GPU test asks the library
LEVELS = np.float32([0.1, 0.9])                            # planted probabilities: not called / called


def planted_border_stretches(piece):
    """[(called uint8 0 / 1, truth uint8 0 / 1), ...]: the smallest shapes at which the two walks can go wrong."""
    rng = np.random.default_rng(7)
    p = piece
    out = []

    def blank(n):
        return np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

    def both(runs, other):                                 # either array in either role
        out.append((runs.copy(), other.copy()))
        out.append((other.copy(), runs.copy()))

    for n in (1, 2, 63, 64, 65, 4095, 4096, 4097, p - 1, p, p + 1, 2 * p + 1):
        if n <= 65:
            for _ in range(3):
                out.append(((np.cumsum(rng.random(n) < 0.15) & 1).astype(np.uint8), (np.cumsum(rng.random(n) < 0.2) & 1).astype(np.uint8)))
            out.append((np.ones(n, np.uint8), np.ones(n, np.uint8)))
            continue
        # runs of 33 that END (boundary index + phase = 0 mod 4) or START (= 2 mod 4) exactly at, one sample before and one after
        # a multiple of 64 (tests/test_run_states_gpu.py's scheme); the other array's ends are shifted by -3 .. +3 on either side,
        # every eleventh run is absent, and one- to three-sample holes sit strictly inside or touch an end
        for variant in range(12 if n < p - 1 else 6):
            phase, turn = (variant // 3, variant % 3) if n < p - 1 else (2 * (variant // 3), variant % 3)
            runs, other = blank(n)
            count = variant
            for j in range(1, n // 64 + 1):
                kind = (j + phase) % 4
                d = ((j >> 1) + turn) % 3 - 1
                first = j * 64 - 33 + d if kind == 0 else j * 64 + d
                if kind not in (0, 2) or first < 4 or first + 33 + 4 > n:
                    continue
                runs[first:first + 33] = 1
                left, right = count % 7 - 3, (count // 7) % 7 - 3
                if count % 11 != 10:
                    other[first + left:first + 33 + right] = 1
                    hole = count % 5
                    if hole == 1:
                        other[first + 16] = 0              # strictly inside
                    elif hole == 2:
                        other[first + 4] = other[first + 20:first + 23] = 0      # two interruptions in one run
                    elif hole == 3:
                        other[first] = other[first + 1] = 0                      # touches the start: no interruption
                    elif hole == 4:
                        other[first + 32] = 0              # touches the end
                count += 1
            out.append((runs, other) if variant % 2 else (other, runs))
    # holes of 70 samples across a word, a wave and a piece border: strictly inside, touching the start, touching the end
    for base in (128, 4096, p, 2 * p):
        for where in range(3):
            runs, other = blank(base + 300)
            runs[base - 100:base + 120] = 1
            other[base - 103:base + 125] = 1
            other[(base - 35, base - 100, base + 50)[where]:(base + 35, base - 30, base + 120)[where]] = 0
            other[base - 90 + where] = 0 if where != 1 else 1
            both(runs, other)
    runs, other = blank(2 * p + 1)                         # an overshoot longer than a whole piece on either side
    other[:] = 1
    runs[p - 20:p + 20] = 1
    both(runs, other)
    other[0] = other[-1] = 0
    both(runs, other)
    for first in (0, 1, 5):                                # the position-0 rule: the other array's ones reach position 0
        runs, other = blank(200)
        runs[first:first + 40] = 1
        other[:60] = 1
        both(runs, other)
        other[0] = 0
        both(runs, other)
    for n in (129, 130, 193, p + 1, p + 2):                # the last-sample rule at n - 2, for either kind and for both
        for who in range(4):
            called, truth = blank(n)
            if who != 1:
                truth[n - 40:n - 1] = 1
            if who != 0:
                called[n - 30:n - (1 if who != 3 else 0)] = 1
            out.append((called, truth))
    alternating = (np.arange(4097) & 1).astype(np.uint8)   # 32 runs per word
    both(alternating, np.ones(4097, np.uint8))
    both(alternating, np.repeat(np.uint8([0, 1, 0, 1, 0]), [100, 1000, 1, 2000, 996]))
    out.append((alternating, 1 - alternating))
    called, truth = blank(400)                             # called runs of 14, 15 and 16 over one long true run
    truth[10:390] = 1
    called[20:34] = called[100:115] = called[200:216] = 1
    out.append((called, truth))
    return out


def pack_stretches(stretches, window=35):
    """(probs, y, bounds, lengths) as a round packs them; probability 0.9 in the zero tails, so a tail taken for a sample shows."""
    lengths = np.array([len(c) for c, _ in stretches], dtype=np.int64)
    bounds, _tails = dv.layout(lengths, window)
    probs = np.full(int(bounds[-1]), 0.9, dtype=np.float32)
    y = np.zeros(int(bounds[-1]), dtype=np.uint8)
    for b, (called, truth) in zip(bounds[:-1].tolist(), stretches):
        probs[b:b + len(called)] = LEVELS[called]
        y[b:b + len(truth)] = truth
    return probs, y, bounds, lengths


def golden_batch():
    """The 51 golden stretches, packed as a round packs them."""
    with np.load(os.path.join(GOLDEN, "run_states_golden.npz")) as z:
        scores, labels, offsets = z["scores"], z["labels"], z["offsets"]
    lengths = np.diff(offsets)
    bounds, _tails = dv.layout(lengths, 35)
    probs, y = np.full(int(bounds[-1]), 0.9, np.float32), np.zeros(int(bounds[-1]), np.uint8)
    for b0, a, n in zip(bounds[:-1].tolist(), offsets[:-1].tolist(), lengths.tolist()):
        probs[b0:b0 + n], y[b0:b0 + n] = scores[a:a + n], labels[a:a + n]
    return probs, y, bounds, lengths


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("validation_borders") / "validation_borders_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "validation_borders_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def replayed(exe, tmp_path, batch, threshold, reach, piece, min_run=15):
    probs, y, bounds, lengths = batch
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as fh:
        np.array([len(lengths)], np.int64).tofile(fh)
        for b0, n in zip(bounds[:-1].tolist(), lengths.tolist()):
            np.array([n], np.int64).tofile(fh)
            y[b0:b0 + n].tofile(fh)
            if n:
                np.asarray(correct_short((probs[b0:b0 + n].astype(np.float64) >= threshold).astype(np.int64), min_run)).astype(np.uint8).tofile(fh)
    run = subprocess.run([exe, case, str(reach), str(piece)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    return np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()], dtype=np.int64)


def test_the_golden_batch(replay, tmp_path):
    batch = golden_batch()
    for reach in (1, 64, 128):
        want = dv.run_borders_host(*batch, (0.3, 0.5, 0.9), reach)
        for k, t in enumerate((0.3, 0.5, 0.9)):
            for piece in (1, 2, 64, 128, 4096):            # 1 and 2 words: these short stretches cross piece borders too
                assert np.array_equal(replayed(replay, tmp_path, batch, t, reach, piece), want[k]), (reach, t, piece)


def test_the_planted_batch(replay, tmp_path):
    batch = pack_stretches(planted_border_stretches(PIECE))
    for min_run, reach in ((15, 64), (1, 128), (15, 1)):
        want = dv.run_borders_host(*batch, (0.5,), reach, min_run)[0]
        part = dv.split_run_borders(want, reach)
        assert part["interrupted"].min() >= 5 and part["left"][:, 0].min() >= 1 and part["right"][:, 2 * reach].min() >= 1
        for piece in (64, 128, 4096) + ((1, 3) if reach == 64 else ()):
            assert np.array_equal(replayed(replay, tmp_path, batch, 0.5, reach, piece, min_run), want), (min_run, reach, piece)
