"""The grid-wide schedule of the fp32 biGRU throughput kernel and its step 0 on the zero state
(catfish_amd/csrc/gru_balance.hpp, gru_layer_kernel, gru_tile).

Grid-wide: a direction's tiles x 35 steps are dealt as equal contiguous shares of STEPS to ALL waves of the launch, not workgroup
by workgroup, so a tile can be cut between the last wave of one workgroup and wave 0 of the next, which hands h over through an
agent-scope flag.  Zero state: step 0 of a tile skips the products with h = 0.  Neither touches the arithmetic that matters, so

* on the CPU the schedule functions (compiled with g++ through tests/native/gru_grid_balance_shim.cpp) are swept over
  gx in {1, 2, 3, 5, 128} workgroups x {4, 8} waves and gx * nwaves .. gx * nwaves + 40 tiles plus the benchmark's 1887..1889: the
  pieces cover every step once, shares differ by at most one step, nothing is interior where the schedule is feasible, every
  tail's producer is the wave with the next lower global index, a simulation over all workgroups ends without a deadlock and
  without a wait, and the load model and the launcher's choice give the figures of DESIGN.md section 4;
* on the GPU probabilities and logits are the bits of CATFISH_GRU_BALANCE=0 (round-robin), with the grid forced to 2, 3 and 5
  workgroups (CATFISH_GRU_GX) so that a boundary falls inside a tile and on a tile edge, on the production grid at 1025 tiles and
  at the benchmark's size +- 7 windows, and for a one-layer network; the zero-state skip is compared with
  CATFISH_GRU_ZERO_PRODUCTS=1, which runs the products.  The last 64 windows are held to the float64 oracle within 1e-4, the
  bound of tests/test_gru_balance.py.  No test provokes a timeout.
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
GRIDS = [(gx, nwaves) for gx in (1, 2, 3, 5, 128) for nwaves in (4, 8)]


# ------------------------------------------------------------------------------------------ CPU: the schedule functions
@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("gru_grid_balance") / "libgru_grid_balance.so")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "gru_grid_balance_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    return ctypes.CDLL(lib)


def _tile_counts(gx, nwaves):
    return sorted(set(range(gx * nwaves, gx * nwaves + 41)) | ({1887, 1888, 1889} if gx * nwaves <= 1887 else set()))


def _pieces(sched, n_tiles, gx, nwaves, g):
    """The share of global wave g in EXECUTION order: [(tile, s_begin, s_end)], head first, whole tiles, tail last."""
    out = (ctypes.c_int * 8)()
    sched.shim_gridwide_share(n_tiles, gx, nwaves, g, T, out)
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


def _simulate(order):
    """Every wave of the grid runs its pieces in order, one step per time unit (all workgroups resident, as on the production
    grid); a piece with s_begin > 0 needs the piece that ends at its s_begin to be over.  -> (finish times, total wait); raises on
    a deadlock."""
    n = len(order)
    done, t, idx, waits = {}, [0] * n, [0] * n, 0
    progressed = True
    while progressed:
        progressed = False
        for w in range(n):
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
    assert all(idx[w] == len(order[w]) for w in range(n)), "deadlock"
    return t, waits


@pytest.mark.parametrize("gx,nwaves", GRIDS)
def test_pieces_cover_every_step_once_and_feasible_means_no_interior_piece(sched, gx, nwaves):
    for n_tiles in _tile_counts(gx, nwaves):
        assert sched.shim_gridwide_ok(n_tiles, gx, nwaves) == 1, (n_tiles, gx, nwaves)
        covered = np.zeros(n_tiles * T, dtype=np.int32)
        shares = []
        for g in range(gx * nwaves):
            pieces, steps = _pieces(sched, n_tiles, gx, nwaves, g)
            assert steps == sum(s1 - s0 for _, s0, s1 in pieces), (n_tiles, gx, nwaves, g)
            shares.append(steps)
            for tile, s0, s1 in pieces:
                assert 0 <= tile < n_tiles and 0 <= s0 < s1 <= T, (n_tiles, gx, nwaves, g, pieces)
                assert s0 == 0 or s1 == T, ("interior piece", n_tiles, gx, nwaves, g, pieces)
                covered[tile * T + s0:tile * T + s1] += 1
        assert sum(shares) == n_tiles * T and (covered == 1).all(), (n_tiles, gx, nwaves)
        assert max(shares) - min(shares) <= 1 and min(shares) >= T, (n_tiles, gx, nwaves)
    for n_tiles in (0, 1, gx * nwaves - 1):
        assert sched.shim_gridwide_ok(n_tiles, gx, nwaves) == 0
        assert sched.shim_gridwide_load(n_tiles, gx, nwaves, 1, T) == -1


@pytest.mark.parametrize("gx,nwaves", GRIDS)
def test_simulation_over_all_workgroups_never_waits(sched, gx, nwaves):
    for n_tiles in _tile_counts(gx, nwaves):
        order = [_pieces(sched, n_tiles, gx, nwaves, g)[0] for g in range(gx * nwaves)]
        for g, pieces in enumerate(order):      # at most one head, first; at most one tail, last; its head is global wave g - 1's
            heads = [p for p in pieces if p[1] == 0 and p[2] < T]
            tails = [p for p in pieces if p[1] > 0]
            assert len(heads) <= 1 and len(tails) <= 1
            assert not heads or pieces[0] == heads[0]
            assert not tails or pieces[-1] == tails[0]
            if tails:
                assert g > 0 and order[g - 1][0] == (tails[0][0], 0, tails[0][1]), (n_tiles, gx, nwaves, g)
        t, waits = _simulate(order)             # raises on a deadlock
        assert waits == 0 and t == [sum(s1 - s0 for _, s0, s1 in p) for p in order], (n_tiles, gx, nwaves)


@pytest.mark.parametrize("gx,nwaves", GRIDS)
def test_load_model_is_the_worst_workgroups_largest_shares(sched, gx, nwaves):
    per_simd = (nwaves + 3) // 4
    for n_tiles in _tile_counts(gx, nwaves):
        worst = 0
        for b in range(gx):
            shares = sorted(_pieces(sched, n_tiles, gx, nwaves, b * nwaves + w)[1] for w in range(nwaves))
            worst = max(worst, sum(shares[-per_simd:]))
        assert sched.shim_gridwide_load(n_tiles, gx, nwaves, 1, T) == worst, (n_tiles, gx, nwaves)
        assert sched.shim_gridwide_load(n_tiles, gx, nwaves, 2, T) == 2 * worst


def test_loads_on_128_workgroups_of_8_waves(sched):
    for n_tiles in (1887, 1888, 1889):
        assert sched.shim_gridwide_load(n_tiles, 128, 8, 1, T) == 130
        assert sched.shim_grid_load(n_tiles, 128, 8, 1, T, 1) == 132
    assert sched.shim_gridwide_load(1024, 128, 8, 1, T) == 70
    assert sched.shim_gridwide_load(1025, 128, 8, 1, T) == 71
    assert sched.shim_gridwide_load(2048, 128, 8, 1, T) == 140
    assert sched.shim_gridwide_load(1023, 128, 8, 1, T) == -1
    assert sched.shim_gridwide_load(100, 128, 8, 1, T) == -1


def _choose(sched, n_tiles, gx, gx_one, nwaves, wg_per_cu, forced=-1):
    out = (ctypes.c_int * 3)()
    sched.shim_choose(n_tiles, gx, gx_one, nwaves, wg_per_cu, T, forced, out)
    return tuple(out)


def test_launch_choice_on_256_cus(sched):
    """launch_gru's decision (cf_gru_choose) on 256 CUs.  The 128-input layers run 128 workgroups per direction, the first layer
    256 (two per CU) with 128 as its second grid.  -> (schedule, workgroups per direction, worst SIMD load)."""
    for n_tiles in (1887, 1888, 1889):
        assert _choose(sched, n_tiles, 128, 128, 8, 1) == (2, 128, 130)
        assert _choose(sched, n_tiles, 256, 128, 8, 2) == (2, 128, 130)         # 1888 < 256 x 8: only the second grid is feasible
    for n_tiles, load in ((1024, 70), (2048, 140)):                             # divides evenly: what it ran
        assert _choose(sched, n_tiles, 128, 128, 8, 1) == (0, 128, load)
        assert sched.shim_gridwide_load(n_tiles, 128, 8, 1, T) == load          # feasible, but not strictly better
    assert _choose(sched, 1024, 256, 128, 8, 2) == (1, 128, 70)                 # first layer: 8 whole tiles per workgroup, as before
    assert _choose(sched, 2048, 256, 128, 8, 2) == (0, 256, 140)
    assert _choose(sched, 1025, 128, 128, 8, 1) == (2, 128, 71)
    assert _choose(sched, 257, 65, 128, 4, 1) == (0, 65, 35)                    # 4097 windows: 3 or 4 tiles on 4 waves
    assert _choose(sched, 4096 + 5, 256, 128, 8, 2)[0] == 2                     # two per CU, shares of 70 or 71 steps
    # forced: 0 round-robin, 1 / 2 the in-workgroup schedules as before, 3 grid-wide where feasible
    assert _choose(sched, 1888, 128, 128, 8, 1, forced=0) == (0, 128, 140)
    assert _choose(sched, 1888, 128, 128, 8, 1, forced=1) == (1, 128, 132)
    assert _choose(sched, 1888, 256, 128, 8, 2, forced=1) == (1, 256, 140)      # 7 or 8 tiles on 8 waves: balanced, no gain
    assert _choose(sched, 1888, 256, 128, 8, 2, forced=2) == (1, 128, 132)
    assert _choose(sched, 1888, 256, 128, 8, 2, forced=3) == (2, 128, 130)
    assert _choose(sched, 2048, 128, 128, 8, 1, forced=3) == (2, 128, 140)
    assert _choose(sched, 40, 2, 0, 8, 1, forced=3) == (2, 2, 176)              # 87 or 88 steps a wave: a forced two-workgroup grid (CATFISH_GRU_GX)
    assert _choose(sched, 15, 2, 0, 8, 1, forced=3)[0] != 2                     # fewer tiles than waves: not feasible


# ------------------------------------------------------------------------------------------ GPU: the same bits
_WAYS = (("0", "1"),        # round-robin, products run: the reference
         ("3", "1"),        # grid-wide, products run
         ("0", None),       # round-robin, step 0 skips the zero-state products
         ("3", None),       # both
         (None, None))      # what the launcher chooses


def _every_way(eng, x, monkeypatch):
    outs = []
    for balance, zero_products in _WAYS:
        for name, v in (("CATFISH_GRU_BALANCE", balance), ("CATFISH_GRU_ZERO_PRODUCTS", zero_products)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        outs.append(eng.infer_host(x, return_logits=True))
        eng.check_error()
    monkeypatch.delenv("CATFISH_GRU_BALANCE", raising=False)
    monkeypatch.delenv("CATFISH_GRU_ZERO_PRODUCTS", raising=False)
    return outs


def _assert_same_bits(outs, what):
    ref, ref_l = outs[0]
    assert np.isfinite(ref).all() and np.isfinite(ref_l).all(), what
    for i in range(1, len(outs)):
        assert np.array_equal(outs[i][0], ref) and np.array_equal(outs[i][1], ref_l), (what, _WAYS[i])


_TAIL = np.random.default_rng(64).normal(0, 1.4, size=(64, 35)).astype(np.float32)


def _oracle_tail(w, cache, **oracle_kw):
    """Windows are independent sequences, so every input of a test ends in the same 64 windows and the float64 oracle runs on
    them once per set of weights; where they fall in their tiles, and in which wave's share, changes with the window count."""
    if "want" not in cache:
        cache["want"] = oracle.forward(_TAIL, w, np.float64, **oracle_kw)
    return cache["want"]


def _check(eng, w, n, monkeypatch, what, cache, **oracle_kw):
    m = len(_TAIL)
    x = np.concatenate([np.random.default_rng(n).normal(0, 1.4, size=(n - m, 35)).astype(np.float32), _TAIL])
    outs = _every_way(eng, x, monkeypatch)
    _assert_same_bits(outs, what)
    want = _oracle_tail(w, cache, **oracle_kw)
    err = np.abs(outs[3][0].reshape(n, 35)[-m:].ravel() - want.ravel()).max()
    print("windows %d (%s): max |p - float64 oracle| over the last %d windows = %.3g" % (n, what, m, err))
    assert err < 1e-4, (what, err)


def _windows(tiles):
    """A window count of `tiles` tiles; every other count leaves the last tile ragged."""
    return 16 * tiles - ((tiles % 13) + 1 if tiles % 2 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("gx", [2, 3, 5])
def test_forced_grid_hands_h_across_workgroup_boundaries(monkeypatch, gx):
    """gx workgroups of 8 waves per direction on 16 gx .. 16 gx + 11 tiles: shares of 70 to 80 steps, so every wave but the first
    starts inside a tile or on its edge, the boundary between two workgroups included (inside a tile at 16 gx + 1, on an edge at
    16 gx and, for gx = 2, at every even count), in the first and in the last workgroup."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    monkeypatch.setenv("CATFISH_GRU_GX", str(gx))
    w = oracle.random_weights(seed=47)
    eng = HipEngine(w, device=0, max_windows_per_pass=4096)
    cache = {}
    try:
        for tiles in range(16 * gx, 16 * gx + 12):
            _check(eng, w, _windows(tiles), monkeypatch, (gx, tiles), cache)
    finally:
        eng.close()


@pytest.mark.gpu
def test_forced_grid_on_a_single_layer(monkeypatch):
    """n_layers = 1: LAST (the fused dense partial sums) runs on the 32-input kernel."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    monkeypatch.setenv("CATFISH_GRU_GX", "3")
    w = oracle.random_weights(seed=43, n_layers=1)
    eng = HipEngine(w, n_layers=1, device=0, max_windows_per_pass=32768)
    cache = {}
    try:
        for tiles in (48, 49, 53, 59):
            _check(eng, w, _windows(tiles), monkeypatch, ("one layer", tiles), cache, n_layers=1)
        monkeypatch.delenv("CATFISH_GRU_GX")
        _check(eng, w, 30208, monkeypatch, "one layer, production grid", cache, n_layers=1)
    finally:
        eng.close()


@pytest.mark.gpu
def test_production_grid_at_1025_tiles_and_smallest_throughput_call(monkeypatch):
    """16 400 windows = 1025 tiles: one tile more than the 1024 waves of a direction, shares of 35 or 36 steps (load 71), every
    wave but the first cut; the launcher takes the grid-wide schedule by itself.  4097 windows: the smallest call of the
    throughput kernel (257 tiles on 4-wave workgroups), where only the zero-state skip applies."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    w = oracle.random_weights(seed=41)
    eng = HipEngine(w, device=0, max_windows_per_pass=32768)
    cache = {}
    try:
        _check(eng, w, 16400, monkeypatch, "1025 tiles", cache)
        _check(eng, w, 4097, monkeypatch, "4097 windows", cache)
    finally:
        eng.close()


_CKPT_CACHE = {}


@pytest.mark.gpu
@pytest.mark.parametrize("n_windows", [30208 - 7, 30208, 30208 + 7])
def test_benchmark_size_with_checkpoint_weights(ckpt_weights, monkeypatch, n_windows):
    """1888 / 1889 tiles on 128 workgroups of 8 waves: shares of 64 or 65 steps, 130 on the worst SIMD."""
    from catfish_amd.engine import HipEngine
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    eng = HipEngine(ckpt_weights, device=0, max_windows_per_pass=32768)
    try:
        _check(eng, ckpt_weights, n_windows, monkeypatch, "benchmark size", _CKPT_CACHE)
    finally:
        eng.close()
