"""The base kernel's body on the CPU under AddressSanitizer + UBSan: tests/native/validation_bases_replay.cpp walks every stretch
word by word through csrc/validation_bases_word.hpp -- the rules the kernel runs one word per lane -- in pieces of a size given on
the command line, with the masks in exactly sized malloc'ed buffers.  A stand-alone program run as its own process; nothing is
preloaded.  Its table must equal ``device_validation.run_bases_host`` on the golden stretches and on the planted batch the GPU test
uses (tests/test_run_bases_gpu.py imports it from here), and the sanitizers must have nothing to say."""
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
MARK = 0x80
LETTERS = b"ACGT"


def planted_base_stretches(piece):
    """[(called uint8 0 / 1, truth uint8 0 / 1, basemap uint8), ...]: the smallest shapes at which the walk can go wrong.  The base
    maps are written sample by sample (the kernel and the rule read nothing but the marked bytes): unmarked samples hold 'a', a
    byte no class takes, so a base taken from a sample without its mark would show."""
    rng = np.random.default_rng(11)
    p = piece
    out = []

    def blank(n):
        return np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.full(n, ord("a"), dtype=np.uint8)

    def both(runs, other, bmap):                           # either array in either role
        out.append((runs.copy(), other.copy(), bmap.copy()))
        out.append((other.copy(), runs.copy(), bmap.copy()))

    def mark(bmap, at, letter):
        bmap[at] = MARK | letter

    for n in (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, p - 1, p, p + 1, 2 * p + 1):
        if n <= 65:
            for _ in range(3):
                bmap = rng.choice(np.frombuffer(b"ACGTNa", np.uint8), size=n) | np.where(rng.random(n) < 0.3, MARK, 0).astype(np.uint8)
                out.append(((np.cumsum(rng.random(n) < 0.15) & 1).astype(np.uint8), (np.cumsum(rng.random(n) < 0.2) & 1).astype(np.uint8), bmap))
            out.append((np.ones(n, np.uint8), np.ones(n, np.uint8), np.full(n, MARK | ord("G"), np.uint8)))
            continue
        # runs of 33 that END (boundary index + phase = 0 mod 4) or START (= 2 mod 4) exactly at, one sample before and one after
        # a multiple of 64 (tests/test_run_states_gpu.py's scheme).  The other array holds, run by run, the same run (complete),
        # the run with its middle sample missing (incomplete), nothing (absent) or the run widened by three samples; the marks go
        # through eleven layouts, coprime to those four, and the letter changes every four runs, so every state meets every
        # layout and every letter
        for variant in range(12 if n < p - 1 else 6):
            phase, turn = (variant // 3, variant % 3) if n < p - 1 else (2 * (variant // 3), variant % 3)
            runs, other, bmap = blank(n)
            count = 37 * variant
            for j in range(1, n // 64 + 1):
                kind = (j + phase) % 4
                d = ((j >> 1) + turn) % 3 - 1
                first = j * 64 - 33 + d if kind == 0 else j * 64 + d
                if kind not in (0, 2) or first < 4 or first + 33 + 4 > n:
                    continue
                last = first + 32
                runs[first:last + 1] = 1
                if count % 4 != 2:
                    other[first:last + 1] = 1
                if count % 4 == 1:
                    other[first + 16] = 0
                if count % 4 == 3:
                    other[first - 3:last + 4] = 1
                letter = LETTERS[(count // 4) % 4]
                layout = count % 11
                if layout == 0:                            # the first and the last sample of the run
                    mark(bmap, [first, last], letter)
                elif layout == 1:                          # one sample outside either end: no base at all
                    mark(bmap, [first - 1, last + 1], letter)
                elif layout == 2:                          # bit 63 and bit 0 of the words the run touches, where they lie inside it
                    at = [i for i in (j * 64 - 1, j * 64) if first <= i <= last]
                    mark(bmap, at or [first + 5], letter)
                elif layout == 3:                          # mixed
                    mark(bmap, [first + 2, first + 20], letter)
                    mark(bmap, [first + 11], LETTERS[(count // 4 + 1) % 4])
                elif layout == 4:
                    mark(bmap, [first + 3, first + 9], ord("N"))
                elif layout == 5:                          # lower case is no class
                    mark(bmap, [first + 3, first + 9], letter | 0x20)
                elif layout == 6:                          # 15, 16, 17 bases: max_bases - 1, max_bases, max_bases + 1 at 16
                    mark(bmap, np.arange(first, first + 15 + (count // 44) % 3), letter)
                elif layout == 7:                          # 31, 32, 33 bases: the same at 32
                    mark(bmap, np.arange(first, first + 31 + (count // 44) % 3), letter)
                elif layout == 8:                          # one base; a second one right behind the run
                    mark(bmap, [first + 16, last + 1], letter)
                elif layout == 9:                          # 33 bases with one of another letter at the end
                    mark(bmap, np.arange(first, last + 1), letter)
                    mark(bmap, [last], ord("N"))
                # layout 10: no mark near the run
                count += 1
            out.append((runs, other, bmap) if variant % 2 else (other, runs, bmap))
    # runs whose bases span a word, a wave and a piece border: two bases on bit 63 / bit 0, then every sample marked (>= 64 bases:
    # the count saturates), then the same with one other letter just before the border
    for base in (128, 4096, p, 2 * p):
        for how in range(3):
            runs, other, bmap = blank(base + 300)
            runs[base - 100:base + 120] = 1
            other[base - 100 + 4 * how:base + 120] = 1
            if how == 0:
                mark(bmap, [base - 1, base], ord("C"))
            else:
                mark(bmap, np.arange(base - 100, base + 120), ord("T"))
            if how == 2:
                mark(bmap, [base - 1], ord("G"))
            mark(bmap, [base - 101, base + 120], ord("A"))                      # one sample outside either end
            both(runs, other, bmap)
    for at in (p, p + p // 2, 2 * p - 1):                  # a run of one whole piece with one base
        runs, other, bmap = blank(3 * p)
        runs[p:2 * p] = 1
        other[p:2 * p] = 1
        other[p + 7] = at & 1
        mark(bmap, [at], ord("G"))
        both(runs, other, bmap)
    for n in (129, 130, 193, p + 1, p + 2):                # the last-sample rule at n - 2 with a base on n - 1, for either kind and for both
        for who in range(3):
            called, truth, bmap = blank(n)
            if who != 1:
                truth[n - 40:n - 1] = 1
            if who != 0:
                called[n - 30:n - 1] = 1
            mark(bmap, [n - 20, n - 1], ord("C"))
            out.append((called, truth, bmap))
    runs, other, bmap = blank(41 * 71)                     # a ladder: run i holds i bases, i = 0 .. 40 -- every bin there is
    for i in range(41):
        runs[71 * i + 5:71 * i + 50] = 1
        other[71 * i + 5:71 * i + 50 + i % 3] = 1
        mark(bmap, np.arange(71 * i + 5, 71 * i + 5 + i), LETTERS[i % 4])
    both(runs, other, bmap)
    alternating = (np.arange(4097) & 1).astype(np.uint8)   # 32 runs per word, every sample a base
    everywhere = (MARK | np.frombuffer(LETTERS, np.uint8)[(np.arange(4097) // 2) % 4]).astype(np.uint8)
    both(alternating, np.ones(4097, np.uint8), everywhere)
    both(alternating, np.repeat(np.uint8([0, 1, 0, 1, 0]), [100, 1000, 1, 2000, 996]), everywhere)
    called, truth, bmap = blank(400)                       # called runs of 14, 15 and 16 over one long true run
    truth[10:390] = 1
    called[20:34] = called[100:115] = called[200:216] = 1
    mark(bmap, np.arange(12, 390, 9), ord("A"))
    out.append((called, truth, bmap))
    return out


def pack_base_stretches(stretches, window=35):
    """(probs, y, basemap, bounds, lengths) as a round packs them; probability 0.9 and a marked 'T' in the zero tails, so a tail taken
    for a sample shows."""
    lengths = np.array([len(c) for c, _, _ in stretches], dtype=np.int64)
    bounds, _tails = dv.layout(lengths, window)
    probs = np.full(int(bounds[-1]), 0.9, dtype=np.float32)
    y = np.zeros(int(bounds[-1]), dtype=np.uint8)
    basemap = np.full(int(bounds[-1]), MARK | ord("T"), dtype=np.uint8)
    for b, (called, truth, bmap) in zip(bounds[:-1].tolist(), stretches):
        probs[b:b + len(called)] = LEVELS[called]
        y[b:b + len(truth)] = truth
        basemap[b:b + len(bmap)] = bmap
    return probs, y, basemap, bounds, lengths


def set_base_map(stretches):
    """The base map as a SET keeps it -- every stretch starts mid-read, between marked bases that are not its own -- and where
    every stretch starts in it: (basemap uint8, src_first int64)."""
    parts, src_first, at = [], [], 0
    for r, (_called, _truth, bmap) in enumerate(stretches):
        before, after = 7 + r % 5, 3 + r % 4
        parts += [np.full(before, MARK | LETTERS[r % 4], np.uint8), bmap, np.full(after, MARK | LETTERS[(r + 1) % 4], np.uint8)]
        src_first.append(at + before)
        at += before + len(bmap) + after
    return np.concatenate(parts), np.array(src_first, dtype=np.int64)


def golden_base_batch():
    """The golden stretches, packed as a round packs them."""
    with np.load(os.path.join(GOLDEN, "run_bases_golden.npz")) as z:
        scores, labels, bmaps, offsets = z["scores"], z["labels"], z["basemap"], z["offsets"]
    lengths = np.diff(offsets)
    bounds, _tails = dv.layout(lengths, 35)
    probs, y = np.full(int(bounds[-1]), 0.9, np.float32), np.zeros(int(bounds[-1]), np.uint8)
    basemap = np.full(int(bounds[-1]), MARK | ord("T"), np.uint8)
    for b0, a, n in zip(bounds[:-1].tolist(), offsets[:-1].tolist(), lengths.tolist()):
        probs[b0:b0 + n], y[b0:b0 + n], basemap[b0:b0 + n] = scores[a:a + n], labels[a:a + n], bmaps[a:a + n]
    return probs, y, basemap, bounds, lengths


def lumped(table, max_bases):
    """A run-bases table at fewer bins: the bins from ``max_bases`` up added into one (``min(nb, max_bases)``)."""
    return np.concatenate((table[..., :max_bases], table[..., max_bases:].sum(axis=-1, keepdims=True)), axis=-1)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("validation_bases") / "validation_bases_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "validation_bases_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def replayed(exe, tmp_path, batch, threshold, max_bases, piece, min_run=15):
    probs, y, basemap, bounds, lengths = batch
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as fh:
        np.array([len(lengths)], np.int64).tofile(fh)
        for b0, n in zip(bounds[:-1].tolist(), lengths.tolist()):
            np.array([n], np.int64).tofile(fh)
            y[b0:b0 + n].tofile(fh)
            if n:
                np.asarray(correct_short((probs[b0:b0 + n].astype(np.float64) >= threshold).astype(np.int64), min_run)).astype(np.uint8).tofile(fh)
            basemap[b0:b0 + n].tofile(fh)
    run = subprocess.run([exe, case, str(max_bases), str(piece)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    return np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()], dtype=np.int64).reshape(2, 3, 5, max_bases + 1)


def test_the_golden_batch(replay, tmp_path):
    batch = golden_base_batch()
    for max_bases in (1, 16, 32):
        want = dv.run_bases_host(*batch, (0.3, 0.5, 0.9), max_bases)
        for k, t in enumerate((0.3, 0.5, 0.9)):
            for piece in (1, 2, 64, 128, 4096):            # 1 and 2 words: these short stretches cross piece borders too
                assert np.array_equal(replayed(replay, tmp_path, batch, t, max_bases, piece), want[k]), (max_bases, t, piece)


def test_the_planted_batch(replay, tmp_path):
    batch = pack_base_stretches(planted_base_stretches(PIECE))
    for min_run, max_bases in ((15, 16), (1, 32), (15, 1)):
        want = dv.run_bases_host(*batch, (0.5,), max_bases, min_run)[0]
        assert want.sum(axis=-1).min() >= 1                # every (kind, state, class)
        assert want.sum(axis=(0, 1, 2)).min() >= 1         # every bin
        for piece in (64, 128, 4096) + ((1, 2, 3) if max_bases == 16 else ()):
            assert np.array_equal(replayed(replay, tmp_path, batch, 0.5, max_bases, piece, min_run), want), (min_run, max_bases, piece)
