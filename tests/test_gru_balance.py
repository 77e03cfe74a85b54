"""The balanced schedule of the fp32 biGRU throughput kernel (catfish_amd/csrc/gru_balance.hpp, gru_layer_kernel).

A workgroup's tiles x 35 steps are dealt to its waves as equal contiguous shares of STEPS instead of whole tiles; a tile cut
between two waves hands its state h over through memory.  The arithmetic of every step is untouched, so:

* on the GPU the outputs with the schedule forced off (CATFISH_GRU_BALANCE=0 behind the debug switch), forced on on the usual
  grid (=1), forced on on the one-workgroup-per-CU grid of the first layer (=2) and left to the launcher are the same bits, at the benchmark's launch size +- a ragged tile, at window counts that give a 128-workgroup
  launch 8, 9, 14, 15 and 17 tiles per workgroup, at small counts, and for a one-layer network whose last layer is also its first;
* on the CPU the schedule function itself (compiled with g++ through tests/native/gru_balance_shim.cpp) is checked for every
  (tiles, waves) in 1..64 x {1, 2, 4, 8}: the pieces cover every step exactly once, no piece is interior wherever the function
  says "balanced", a simulation of one step per time unit finishes without a tail ever lacking its head, and the worst SIMD
  load is 132 steps for 15 tiles on 8 waves, 124 for 14, and never above round-robin's.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import catfish_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 35


# ------------------------------------------------------------------------------------------ CPU: the schedule function
@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("gru_balance") / "libgru_balance.so")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "gru_balance_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    return ctypes.CDLL(lib)


def _pieces(sched, tiles, nwaves, wave):
    """The share of one wave in EXECUTION order: [(tile, s_begin, s_end)], head first, whole tiles, tail last -- the order of
    gru_layer_kernel's piece loop."""
    out = (ctypes.c_int * 8)()
    sched.shim_balanced_share(tiles, nwaves, wave, T, out)
    head_tile, head_end, whole_first, whole_count, tail_tile, tail_begin, interior, steps = list(out)
    if interior:
        return [(tail_tile, tail_begin, head_end)], steps
    pieces = []
    if head_end > 0:
        pieces.append((head_tile, 0, head_end))
    pieces += [(whole_first + i, 0, T) for i in range(whole_count)]
    if tail_begin < T:
        pieces.append((tail_tile, tail_begin, T))
    return pieces, steps


def _simulate(order, nwaves):
    """Every wave runs its pieces in order, one step per time unit; a piece with s_begin > 0 needs the piece that ends at its
    s_begin to be over.  -> (finish time per wave, total time spent waiting); raises on a deadlock."""
    done, t, idx, waits = {}, [0] * nwaves, [0] * nwaves, 0
    progressed = True
    while progressed:
        progressed = False
        for w in range(nwaves):
            while idx[w] < len(order[w]):
                tile, s0, s1 = order[w][idx[w]]
                if s0 > 0:
                    if (tile, s0) not in done:
                        break
                    if done[(tile, s0)] > t[w]:
                        waits += done[(tile, s0)] - t[w]
                        t[w] = done[(tile, s0)]
                t[w] += s1 - s0
                done[(tile, s1)] = t[w]
                idx[w] += 1
                progressed = True
    assert all(idx[w] == len(order[w]) for w in range(nwaves)), "deadlock"
    return t, waits


@pytest.mark.parametrize("nwaves", [1, 2, 4, 8])
def test_pieces_cover_every_step_once_and_balanced_means_no_interior_piece(sched, nwaves):
    for tiles in range(1, 65):
        covered = np.zeros(tiles * T, dtype=np.int32)
        interior = empty = False
        total = 0
        for w in range(nwaves):
            pieces, steps = _pieces(sched, tiles, nwaves, w)
            assert steps == sum(s1 - s0 for _, s0, s1 in pieces), (tiles, nwaves, w)
            total += steps
            empty |= steps == 0
            for tile, s0, s1 in pieces:
                assert 0 <= tile < tiles and 0 <= s0 < s1 <= T, (tiles, nwaves, w, pieces)
                covered[tile * T + s0:tile * T + s1] += 1
                interior |= s0 != 0 and s1 != T
        assert total == tiles * T and (covered == 1).all(), (tiles, nwaves)
        shares = [_pieces(sched, tiles, nwaves, w)[1] for w in range(nwaves)]
        assert max(shares) - min(shares) <= 1, (tiles, nwaves)
        assert bool(sched.shim_balance_ok(tiles, nwaves, T)) == (not interior and not empty), (tiles, nwaves)


@pytest.mark.parametrize("nwaves", [1, 2, 4, 8])
def test_simulation_never_lacks_a_head_and_waits_only_for_short_shares(sched, nwaves):
    for tiles in range(1, 65):
        if not sched.shim_balance_ok(tiles, nwaves, T):
            continue
        order = [_pieces(sched, tiles, nwaves, w)[0] for w in range(nwaves)]
        for w, pieces in enumerate(order):             # at most one head, first; at most one tail, last; its head is the previous wave's
            heads = [p for p in pieces if p[1] == 0 and p[2] < T]
            tails = [p for p in pieces if p[1] > 0]
            assert len(heads) <= 1 and len(tails) <= 1
            assert not heads or pieces[0] == heads[0]
            assert not tails or pieces[-1] == tails[0]
            if tails:
                assert w > 0 and order[w - 1][0] == (tails[0][0], 0, tails[0][1])
        t, waits = _simulate(order, nwaves)            # raises on a deadlock
        shares = [sum(s1 - s0 for _, s0, s1 in p) for p in order]
        if min(shares) >= T:                           # head over by b <= 35, tail no earlier than share - (35 - b): no wait
            assert waits == 0 and t == shares, (tiles, nwaves)
        assert max(t) <= max(sched.shim_round_robin_steps(tiles, nwaves, w, T) for w in range(nwaves)), (tiles, nwaves)


def test_worst_simd_load(sched):
    assert sched.shim_simd_load(15, 8, T, 1) == 132 and sched.shim_simd_load(15, 8, T, 0) == 140
    assert sched.shim_simd_load(14, 8, T, 1) == 124 and sched.shim_simd_load(14, 8, T, 0) == 140
    for nwaves in (1, 2, 4, 8):
        for tiles in range(1, 65):
            rr = [sched.shim_round_robin_steps(tiles, nwaves, w, T) for w in range(nwaves)]
            assert sum(rr) == tiles * T
            assert sched.shim_simd_load(tiles, nwaves, T, 0) == sum(sorted(rr)[-((nwaves + 3) // 4):])
            if sched.shim_balance_ok(tiles, nwaves, T):
                assert sched.shim_simd_load(tiles, nwaves, T, 1) <= sched.shim_simd_load(tiles, nwaves, T, 0), (tiles, nwaves)


def test_launch_choice_on_256_cus(sched):
    """What launch_gru derives from the same function: the benchmark's launch (1888 tiles +- 1 on 128 workgroups of 8 waves)
    goes from 140 to 132 steps on its worst SIMD; a launch that divides evenly and a small call gain nothing and so stay on
    round-robin; so does the first layer on its usual grid of two workgroups per CU (7 or 8 tiles each), which is why the launcher
    also weighs one workgroup per CU for it (the 128-workgroup figures above); a grid with too few tiles has no balanced schedule."""
    for n_tiles in (1887, 1888, 1889):
        assert sched.shim_grid_load(n_tiles, 128, 8, 1, T, 0) == 140
        assert sched.shim_grid_load(n_tiles, 128, 8, 1, T, 1) == 132
    assert sched.shim_grid_load(1024, 128, 8, 1, T, 1) == sched.shim_grid_load(1024, 128, 8, 1, T, 0) == 70
    assert sched.shim_grid_load(1888, 256, 8, 2, T, 1) == sched.shim_grid_load(1888, 256, 8, 2, T, 0) == 140
    assert sched.shim_grid_load(257, 65, 4, 1, T, 1) == sched.shim_grid_load(257, 65, 4, 1, T, 0) == 35      # 4097 windows
    assert sched.shim_grid_load(2 * 128, 128, 8, 1, T, 1) == -1          # 2 tiles on 8 waves: interior pieces
    assert sched.shim_grid_load(100, 128, 8, 1, T, 1) == -1


# ------------------------------------------------------------------------------------------ GPU: the same bits
def _every_way(eng, x, monkeypatch):
    """Outputs (probabilities and logits) with the schedule left to the launcher, forced off, forced on on the usual grid, and
    forced on with the first layer on one workgroup per CU."""
    outs = []
    for knob in (None, "0", "1", "2"):
        if knob is None:
            monkeypatch.delenv("CATFISH_GRU_BALANCE", raising=False)
        else:
            monkeypatch.setenv("CATFISH_GRU_BALANCE", knob)
        outs.append(eng.infer_host(x, return_logits=True))
        eng.check_error()
    monkeypatch.delenv("CATFISH_GRU_BALANCE", raising=False)
    return outs


def _assert_same_bits(outs, what):
    off, off_l = outs[1]
    assert np.isfinite(off).all() and np.isfinite(off_l).all(), what
    for i in (0, 2, 3):
        assert np.array_equal(outs[i][0], off) and np.array_equal(outs[i][1], off_l), (what, i)


@pytest.mark.gpu
@pytest.mark.parametrize("n_windows", [30208 - 7, 30208, 30208 + 7])
def test_balanced_schedule_is_bit_identical_at_benchmark_size(ckpt_weights, monkeypatch, n_windows):
    """Checkpoint weights at the shapes of test_throughput_kernel_at_benchmark_size: 1888 / 1889 tiles, 14 or 15 per workgroup
    on the two 128-input layers and, by default, on the first as well (one workgroup per CU); 7 or 8 on the first layer's usual
    two-per-CU grid, balanced only when forced."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    x = np.random.default_rng(n_windows).normal(0, 1.5, size=(n_windows, 35)).astype(np.float32)
    eng = HipEngine(ckpt_weights, device=0, max_windows_per_pass=32768)
    try:
        outs = _every_way(eng, x, monkeypatch)
        _assert_same_bits(outs, n_windows)
        m = 200
        want = oracle.forward(x[-m:], ckpt_weights, np.float64)
        assert np.abs(outs[2][0].reshape(n_windows, 35)[-m:].ravel() - want.ravel()).max() < 1e-4
    finally:
        eng.close()


@pytest.mark.gpu
def test_balanced_schedule_is_bit_identical_across_tiles_per_workgroup(monkeypatch):
    """Random weights.  On 256 CUs the 128-input layers run 128 workgroups per direction: 16 windows x 128 x k tiles give k tiles
    per workgroup, k = 8 (whole tiles only), 9, 14, 15 and 17, and counts in between mix k and k + 1 with a ragged last tile.  The
    first layer's 256 workgroups see half of that.  Small calls: 4097 windows = 257 tiles on 4-wave workgroups of 3 or 4 tiles,
    where the launcher stays on round-robin (test_launch_choice_on_256_cus) and the forced schedule still cuts tiles; 118
    windows run the cooperative kernels, which the knob does not reach."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    w = oracle.random_weights(seed=41)
    eng = HipEngine(w, device=0, max_windows_per_pass=40000)
    try:
        for k, extra in ((8, 0), (9, 0), (9, -37), (14, 0), (14, 16 * 50 + 3), (15, 0), (17, 0), (17, -5)):
            n = 16 * 128 * k + extra
            x = np.random.default_rng(n).normal(0, 1.4, size=(n, 35)).astype(np.float32)
            outs = _every_way(eng, x, monkeypatch)
            _assert_same_bits(outs, (k, extra))
            want = oracle.forward(x[-64:], w, np.float64)
            assert np.abs(outs[2][0].reshape(n, 35)[-64:].ravel() - want.ravel()).max() < 1e-4, (k, extra)
        for n in (4097, 4097 + 16 * 40, 118):
            x = np.random.default_rng(n).normal(0, 1.4, size=(n, 35)).astype(np.float32)
            _assert_same_bits(_every_way(eng, x, monkeypatch), n)
    finally:
        eng.close()


@pytest.mark.gpu
def test_balanced_schedule_is_bit_identical_for_a_single_layer(monkeypatch):
    """n_layers = 1: the kernel that fuses the dense partial sums (LAST) is also the first layer, 32 inputs wide and two
    workgroups per CU -- 256 per direction, so 16 x 256 x 9 windows are 9 tiles per workgroup, and the benchmark's count 7 or 8."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    w = oracle.random_weights(seed=43, n_layers=1)
    eng = HipEngine(w, n_layers=1, device=0, max_windows_per_pass=40000)
    try:
        for n in (16 * 256 * 9, 16 * 256 * 9 - 16 * 100 - 3, 30208):
            x = np.random.default_rng(n).normal(0, 1.4, size=(n, 35)).astype(np.float32)
            outs = _every_way(eng, x, monkeypatch)
            _assert_same_bits(outs, n)
            want = oracle.forward(x[-64:], w, np.float64, n_layers=1)
            assert np.abs(outs[2][0].reshape(n, 35)[-64:].ravel() - want.ravel()).max() < 1e-4, n
    finally:
        eng.close()
