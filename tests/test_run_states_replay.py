"""The run-state kernel's body on the CPU under AddressSanitizer + UBSan: tests/native/validation_runs_replay.cpp walks every stretch
word by word through csrc/validation_runs_word.hpp -- the rules the kernel runs one word per lane -- in pieces of a size given on
the command line, with the masks in exactly sized malloc'ed buffers.  A stand-alone program run as its own process; nothing is
preloaded.  Its table must equal ``device_validation.run_states_host`` on the golden stretches and on the planted batch the GPU test
uses (tests/test_run_states_gpu.py imports it from here), and the sanitizers must have nothing to say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd.infer import correct_short
from test_run_states_host import golden, packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 16384                                              # CF_RUN_PIECE (csrc/validation_walk.hpp); the GPU test asks the library
PIECES = (1, 3, 64, 256)                                   # words per piece of the replay
SEVEN = (1, 2, 15, 16, 64, 4096, 16385)
LEVELS = np.float32([0.1, 0.9, 0.5])                       # planted probabilities: not called / called / exactly 0.5


def planted_stretches(piece):
    """[(called uint8 with values 0 / 1 / 2 = an index into LEVELS, truth uint8), ...]"""
    rng = np.random.default_rng(3)
    out = []

    def blank(n):
        return np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

    for n in (0, 1, 2, 14, 15, 16, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, piece - 1, piece, piece + 1, 2 * piece + 1, 3 * piece + 17):
        if n <= 65:                                        # random runs, every level
            for _ in range(3):
                flips = rng.random(n) < 0.15
                called = (np.cumsum(flips) & 1).astype(np.uint8) * rng.choice(np.uint8([1, 1, 2]), size=n)
                out.append((called, (np.cumsum(rng.random(n) < 0.2) & 1).astype(np.uint8)))
            continue
        # runs of 33 that END (boundary index + phase = 0 mod 4) or START (= 2 mod 4) exactly at, one sample before and one
        # after a multiple of 64 -- word, wave (4096) and piece boundaries alike; phase and the rotation of the shift go through
        # every combination over the variants.  The other array holds, run by run, the same run (complete), the run with its
        # middle sample missing (incomplete), nothing (absent) or the run widened by three samples (complete one way, incomplete
        # the other); truth and prediction swap roles from variant to variant
        for variant in range(12 if n < piece - 1 else 6):
            phase, turn = (variant // 3, variant % 3) if n < piece - 1 else (2 * (variant // 3), variant % 3)
            runs, other = blank(n)
            count = 0
            for j in range(1, n // 64 + 1):
                kind = (j + phase) % 4
                d = ((j >> 1) + turn) % 3 - 1
                first = j * 64 - 33 + d if kind == 0 else j * 64 + d
                if kind not in (0, 2) or first < 4 or first + 33 + 4 > n:
                    continue
                runs[first:first + 33] = 1
                if count % 4 != 2:
                    other[first:first + 33] = 1
                if count % 4 == 1:
                    other[first + 16] = 0
                if count % 4 == 3:
                    other[first - 3:first + 36] = 1
                count += 1
            out.append((runs, other) if variant % 2 else (other, runs))
    p = piece
    called, truth = blank(3 * p)
    truth[p:2 * p] = 1                                     # a run of exactly one whole piece, found completely
    called[p:2 * p] = 1
    out.append((called.copy(), truth.copy()))
    called[p + p // 2] = 0                                 # ... and with one sample missing: incomplete, and two called runs
    out.append((called.copy(), truth.copy()))
    out.append((truth.copy(), called.copy()))
    called, truth = blank(3 * p + 2)
    truth[1:3 * p + 1] = 1                                 # three pieces long, across three piece boundaries; called nowhere: absent
    out.append((called.copy(), truth.copy()))
    out.append((truth.copy(), called.copy()))
    out.append((np.ones(2 * p + 1, np.uint8), np.ones(2 * p + 1, np.uint8)))             # one run of 2 P + 1 ones
    out.append((np.full(2 * p + 1, 2, np.uint8), np.ones(2 * p + 1, np.uint8)))          # ... called by probabilities of exactly 0.5
    out.append(blank(2 * p + 1))                                                           # zeros
    alternating = (np.arange(4097) & 1).astype(np.uint8)                                  # 32 true runs per word
    out.append((np.ones(4097, np.uint8), alternating))
    out.append((np.zeros(4097, np.uint8), 1 - alternating))
    out.append((np.repeat(np.uint8([0, 1, 0, 1, 0]), [100, 1000, 1, 2000, 996]), alternating))
    called, truth = blank(400)                             # called runs of 14, 15 and 16 over one long true run
    truth[10:390] = 1
    called[20:34] = 1
    called[100:115] = 1
    called[200:216] = 1
    out.append((called.copy(), truth.copy()))
    for n in (129, 130, 193, p + 1, p + 2):                # the last-sample rule at n - 2, for either kind and for both
        for who in range(3):
            called, truth = blank(n)
            if who != 1:
                truth[n - 40:n - 1] = 1
            if who != 0:
                called[n - 30:n - 1] = 1
            out.append((called, truth))
    called, truth = blank(300)                             # a label that is neither 0 nor 1 inside a called run
    called[50:250] = 1
    truth[60:240] = 1
    truth[100] = 2
    out.append((called, truth))
    return out


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("validation_runs") / "validation_runs_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "validation_runs_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def case_file(tmp_path, batch, threshold, min_run=15):
    """The batch as the program reads it: per stretch its length, its labels and its corrected prediction at one threshold."""
    probs, y, bounds, lengths = batch
    case = str(tmp_path / ("case_%r_%d.bin" % (threshold, min_run)))
    with open(case, "wb") as fh:
        np.array([len(lengths)], np.int64).tofile(fh)
        for b0, n in zip(bounds[:-1].tolist(), lengths.tolist()):
            np.array([n], np.int64).tofile(fh)
            y[b0:b0 + n].tofile(fh)
            if n:
                np.asarray(correct_short((probs[b0:b0 + n].astype(np.float64) >= threshold).astype(np.int64), min_run)).astype(np.uint8).tofile(fh)
    return case


def replayed(exe, case, edges, piece):
    run = subprocess.run([exe, case, str(piece)] + [str(e) for e in edges], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    return np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()], dtype=np.int64).reshape(2, len(edges) + 1, 3)


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


def test_the_golden_batch(replay, tmp_path):
    scores, labels, offsets, _cases = golden()
    batch = packed([(scores[a:b], labels[a:b]) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())])
    want = dv.run_states_host(*batch, (0.3, 0.5, 0.9), SEVEN)
    assert want.sum(axis=(0, 2)).min() >= 3                # every (kind, state) pair
    for k, t in enumerate((0.3, 0.5, 0.9)):
        case = case_file(tmp_path, batch, t)
        for piece in PIECES:                               # 1 and 3 words: these short stretches cross piece borders too
            assert np.array_equal(replayed(replay, case, (), piece), want[k].sum(axis=1, keepdims=True)), (t, piece)
            assert np.array_equal(replayed(replay, case, SEVEN, piece), want[k]), (t, piece)


def test_the_planted_batch(replay, tmp_path):
    batch = pack_stretches(planted_stretches(PIECE))
    for min_run in (15, 1):
        want = dv.run_states_host(*batch, (0.5,), SEVEN, min_run)[0]
        assert want.sum(axis=1).min() >= 3                 # every (kind, state) pair
        case = case_file(tmp_path, batch, 0.5, min_run)
        for piece in PIECES:
            assert np.array_equal(replayed(replay, case, (), piece), want.sum(axis=1, keepdims=True)), (min_run, piece)
            assert np.array_equal(replayed(replay, case, SEVEN, piece), want), (min_run, piece)
