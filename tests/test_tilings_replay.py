"""The bodies of retile_windows_kernel and vote_tilings_kernel on the CPU under AddressSanitizer + UBSan: tests/native/tilings_replay.cpp
walks both grids serially through csrc/tilings_rule.hpp -- the rules by which the kernels form their addresses -- with every buffer
malloc'ed at exactly the size the Python layer allocates.  A stand-alone program run as its own process; nothing is preloaded.  Its
output must EQUAL ``tilings.retile_host`` / ``tilings.vote_host``, hostile tables must give zero regions and base values, refused
arguments the refusal, and the sanitizers must have nothing to say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import tilings
from test_tilings_host import LAYOUTS, PHASE_SETS, W, WEIGHTS, random_batch, same_bits, special_values, trap_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(-7777)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("tilings") / "tilings_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "tilings_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def replayed(exe, tmp_path, base, offsets, lengths, phases, weight=0, probs=None, logits=None, in_place=False, misalign=False,
             n_reads=None, total=None):
    """-> None when the arguments are refused, else (retiled [size], voted [total], voted logits or None) as the program left them.
    ``phases`` and ``weight`` go in unchecked."""
    n_reads = len(lengths) if n_reads is None else n_reads
    total = len(base) if total is None else total
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    ph = np.zeros(16, dtype=np.int32)
    ph[:len(phases)] = phases
    with open(case, "wb") as fh:
        np.array([n_reads, total, len(phases), weight, int(logits is not None), int(in_place), int(misalign)], np.int64).tofile(fh)
        ph.tofile(fh)
        np.asarray(offsets, np.int64).tofile(fh)
        np.asarray(lengths, np.int64).tofile(fh)
        np.asarray(base, np.float32).tofile(fh)
        if probs is not None:
            np.asarray(probs, np.float32).tofile(fh)
        if logits is not None:
            np.asarray(logits, np.float32).tofile(fh)
    run = subprocess.run([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    with open(out, "rb") as fh:
        refusal = int(np.fromfile(fh, np.int64, 1)[0])
        if refusal:
            assert fh.read() == b""
            return None
        size = tilings.tiling_size(total, n_reads, len(phases))
        retiled = np.fromfile(fh, np.float32, size)
        voted = np.fromfile(fh, np.float32, total)
        voted_logits = np.fromfile(fh, np.float32, total) if logits is not None else None
        assert fh.read() == b""
    return retiled, voted, voted_logits


def check_case(replay, tmp_path, batch, phases, rng, **how):
    base, offsets, lengths = batch
    size = tilings.tiling_size(len(base), len(lengths), len(phases))
    probs, logits = special_values(rng, size)
    for w, weight in enumerate(WEIGHTS):
        retiled, voted, voted_logits = replayed(replay, tmp_path, base, offsets, lengths, phases, w, probs, logits, **how)
        assert same_bits(retiled, tilings.retile_host(base, offsets, lengths, phases))
        assert same_bits(voted, tilings.vote_host(probs, offsets, lengths, phases, weight))
        assert same_bits(voted_logits, tilings.vote_host(logits, offsets, lengths, phases, weight))


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("phases", PHASE_SETS + ((0,),))
def test_the_trap_batch(replay, tmp_path, kind, phases):
    rng = np.random.default_rng(21)
    check_case(replay, tmp_path, trap_batch(kind), phases, rng)
    check_case(replay, tmp_path, trap_batch(kind, n_reads=1), phases, rng, in_place=True)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_random_batches_a_misaligned_buffer_and_no_logits(replay, tmp_path, kind):
    rng = np.random.default_rng(22)
    for k in range(8):
        batch = random_batch(rng, kind)
        phases = tuple([0] + sorted(rng.choice(np.arange(1, W), int(rng.integers(1, 8)), replace=False).tolist()))
        check_case(replay, tmp_path, batch, phases, rng, misalign=bool(k % 2), in_place=bool(k % 3 == 0))
    # a batch of more than one chunk per tiling, without logits
    base, offsets, lengths = trap_batch(kind, seed=4)
    base, offsets, lengths = np.tile(base, 8), np.concatenate([offsets[:-1] + k * offsets[-1] for k in range(8)] + [[8 * offsets[-1]]]), \
        np.tile(lengths, 8)
    assert len(base) > 2 * 4096
    probs, _ = special_values(rng, tilings.tiling_size(len(base), len(lengths), 3))
    retiled, voted, none = replayed(replay, tmp_path, base, offsets, lengths, (0, 12, 23), 1, probs)
    assert none is None and same_bits(retiled, tilings.retile_host(base, offsets, lengths, (0, 12, 23)))
    assert same_bits(voted, tilings.vote_host(probs, offsets, lengths, (0, 12, 23), "centre"))
    # no reads at all, and no samples at all
    retiled, voted, _ = replayed(replay, tmp_path, np.zeros(0, np.float32), [0], [], (0, 17), 0, np.zeros(0, np.float32))
    assert len(retiled) == 0 and len(voted) == 0
    retiled, voted, _ = replayed(replay, tmp_path, np.ones(70, np.float32), [70], [], (0, 17), 0, np.full(140, 0.25, np.float32), n_reads=0)
    assert retiled[:70].all() and not retiled[70:].any() and (voted == 0.25).all()


def hostile_tables(offsets, lengths, total):
    """(name, offsets, lengths, reads that are unsound, offsets ascend?)"""
    big, small = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    out = []
    for name, r, v in (("negative length", 8, -1), ("length past its region", 8, 736), ("length past its region", 5, 71),
                       ("huge length", 3, big), ("most negative length", 2, small)):
        lens = lengths.copy()
        lens[r] = v
        out.append((name, offsets, lens, [r], True))
    for name, k, v, bad, ascend in (("offset not a multiple of 35", 4, offsets[4] + 1, [3, 4], True),
                                    ("offset past total", 9, total + 35, [8], True),
                                    ("huge offset", 9, big, [8], True),
                                    ("negative first offset", 0, -35, [0], True),
                                    ("most negative first offset", 0, small, [0], True),
                                    ("descending last pair", 9, offsets[8] - 35, [8], False),
                                    ("descending pair in the middle", 5, offsets[3], [4], False),
                                    ("huge offset in the middle", 5, big, [4, 5], False)):
        offs = offsets.copy()
        offs[k] = v
        out.append((name, offs, lengths, bad, ascend))
    return out


def test_hostile_tables(replay, tmp_path):
    base, offsets, lengths = trap_batch("pipeline")
    total, n, phases = len(base), len(lengths), (0, 12, 23)
    rng = np.random.default_rng(23)
    probs, logits = special_values(rng, tilings.tiling_size(total, n, 3))
    for name, offs, lens, bad, ascend in hostile_tables(offsets, lengths, total):
        retiled, voted, voted_logits = replayed(replay, tmp_path, base, offs, lens, phases, 1, probs, logits)       # and a silent sanitizer
        assert not (retiled[total:] == SENTINEL).any(), name                     # every sample of the tiling regions was written
        assert same_bits(retiled[:total], base), name
        for r in bad:                                                            # an unsound read: base values, wherever its samples lie
            lo, hi = max(0, min(int(offs[r]), total)), max(0, min(int(offs[r + 1]), total))
            if ascend:
                assert same_bits(voted[lo:hi], probs[lo:hi]) and same_bits(voted_logits[lo:hi], logits[lo:hi]), name
        if ascend:                                                               # exactly the definition: that read zero, the others whole
            assert same_bits(retiled, tilings.retile_host(base, offs, lens, phases, total=total)), name
            assert same_bits(voted, tilings.vote_host(probs, offs, lens, phases, "centre", total=total)), name
            assert same_bits(voted_logits, tilings.vote_host(logits, offs, lens, phases, "centre", total=total)), name
            for r in bad:
                for j in (1, 2):
                    t_j = tilings.tiling_start(j, total, n)
                    lo, hi = max(0, min(int(offs[r]), total)), max(0, min(int(offs[r + 1]), total))
                    assert not retiled[t_j + lo + W * r:t_j + hi + W * (r + 1)].any(), name
        else:                                                                    # every value is a zero or a sample of the base region
            assert np.isin(retiled[total:], np.concatenate([base, [0]])).all(), name


def test_refused_arguments(replay, tmp_path):
    base, offsets, lengths = trap_batch("validation")
    ok = dict(base=base, offsets=offsets, lengths=lengths, phases=(0, 17), probs=np.zeros(tilings.tiling_size(len(base), 9, 2), np.float32))
    assert replayed(replay, tmp_path, **ok) is not None
    for change in (dict(phases=(1, 2)), dict(phases=(0, 35)), dict(phases=(0, 5, 5)), dict(phases=(0, 7, 3)), dict(phases=()),
                   dict(phases=tuple(range(9))), dict(phases=(0, -1)), dict(weight=2), dict(weight=-1), dict(total=len(base) + 1),
                   dict(total=-35), dict(n_reads=-1), dict(n_reads=2 ** 31), dict(total=35 * 2 ** 40)):
        assert replayed(replay, tmp_path, **dict(ok, **change)) is None, change
