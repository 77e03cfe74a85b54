// Schedule of the fp32 biGRU throughput kernel (gru_layer_kernel): how a workgroup's tiles are dealt to its waves.
//
// A tile (16 windows) is CF_T = 35 serial steps.  Dealing whole tiles round-robin leaves some waves one tile (35 steps) ahead
// of the others whenever the tile count is not a multiple of the wave count.  The balanced schedule cuts in TIME instead:
// the workgroup's tiles x 35 steps are laid end to end and every wave takes an equal contiguous share (+-1 step), McNaughton's
// wrap-around rule for preemptive scheduling on identical machines.  A share is then
//     a tail  (steps a..34 of the tile the previous wave began),
//     zero or more whole tiles,
//     a head  (steps 0..b of the tile the next wave finishes),
// and the only state that crosses a cut is h.  A wave runs its head FIRST and its tail LAST: the head needs nothing, so the
// tail that waits for it (on the next wave) can never deadlock, and because a head is over by time b <= 35 while its tail
// starts no earlier than share - (35 - b), the tail does not wait at all when every share is at least 35 steps.
// The schedule is used only when no share needs an interior piece (one that neither starts at step 0 nor ends at step 35) and no
// share is empty; otherwise the launch deals round-robin.
//
// Plain C++, shared by the kernel, by launch_gru's choice between the two schedules and by tests/native/gru_balance_shim.cpp.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CF_BAL_HD __host__ __device__
#else
#define CF_BAL_HD
#endif

struct cf_gru_share {
    int head_tile, head_end;        // head piece: steps [0, head_end) of head_tile; head_end == 0: none
    int whole_first, whole_count;   // whole tiles [whole_first, whole_first + whole_count)
    int tail_tile, tail_begin;      // tail piece: steps [tail_begin, T) of tail_tile; tail_begin == T: none
    int interior;                   // != 0: the share lies strictly inside one tile (steps [tail_begin, head_end) of tail_tile)
    int steps;                      // steps of the whole share
};

// Share of `wave` out of `nwaves` for a workgroup of `tiles` tiles (tile indices relative to the workgroup's first tile).
CF_BAL_HD inline cf_gru_share cf_gru_balanced_share(int tiles, int nwaves, int wave, int T) {
    const int total = tiles * T;
    const int a = (int)((long long)wave * total / nwaves), b = (int)((long long)(wave + 1) * total / nwaves);
    cf_gru_share s;
    s.steps = b - a;
    s.tail_tile = a / T;
    s.tail_begin = a % T == 0 ? T : a % T;
    s.head_tile = b / T;
    s.head_end = b % T;
    s.interior = (a % T != 0 && b % T != 0 && a / T == b / T) ? 1 : 0;
    s.whole_first = (a + T - 1) / T;
    s.whole_count = b / T - s.whole_first;
    if (s.whole_count < 0) s.whole_count = 0;
    return s;
}

// Steps of `wave` under the round-robin dealing of whole tiles.
CF_BAL_HD inline int cf_gru_round_robin_steps(int tiles, int nwaves, int wave, int T) {
    return wave < tiles ? ((tiles - wave + nwaves - 1) / nwaves) * T : 0;
}

// Can a workgroup of `tiles` tiles run the balanced schedule (no interior piece, no empty share)?
CF_BAL_HD inline bool cf_gru_balance_ok(int tiles, int nwaves, int T) {
    if (tiles < 1 || nwaves < 1) return false;
    for (int w = 0; w < nwaves; ++w) {
        const cf_gru_share s = cf_gru_balanced_share(tiles, nwaves, w, T);
        if (s.interior || s.steps <= 0) return false;
    }
    return true;
}

// Worst SIMD load in steps: a CU has four SIMDs, so ceil(nwaves / 4) waves share one, and which ones is the hardware's choice:
// the bound is the sum of that many largest shares.  balanced != 0 asks for the balanced schedule (the caller checked
// cf_gru_balance_ok), 0 for round-robin.
CF_BAL_HD inline int cf_gru_simd_load(int tiles, int nwaves, int T, int balanced) {
    const int per_simd = (nwaves + 3) / 4;
    int top[2] = {0, 0};            // per_simd <= 2 for the at most 8 waves of a workgroup
    for (int w = 0; w < nwaves; ++w) {
        int v = balanced ? cf_gru_balanced_share(tiles, nwaves, w, T).steps : cf_gru_round_robin_steps(tiles, nwaves, w, T);
        if (v > top[0]) { const int t = top[0]; top[0] = v; v = t; }
        if (v > top[1]) top[1] = v;
    }
    return per_simd >= 2 ? top[0] + top[1] : top[0];
}

// The launch-level decision: workgroup b of gx takes tiles [b * n_tiles / gx, (b + 1) * n_tiles / gx), so the counts are
// floor(n_tiles / gx) and, unless it divides, one more.  -> worst SIMD load over the grid, or -1 when `balanced` is asked for and
// some workgroup cannot run it.
CF_BAL_HD inline int cf_gru_grid_load(int n_tiles, int gx, int nwaves, int wg_per_cu, int T, int balanced) {
    if (gx < 1 || n_tiles < gx) return balanced ? -1 : cf_gru_simd_load(1, nwaves, T, 0) * wg_per_cu;
    const int lo = n_tiles / gx, hi = (n_tiles % gx) ? lo + 1 : lo;
    int worst = 0;
    for (int t = lo; t <= hi; ++t) {
        if (balanced && !cf_gru_balance_ok(t, nwaves, T)) return -1;
        const int v = cf_gru_simd_load(t, nwaves, T, balanced);
        if (v > worst) worst = v;
    }
    return worst * wg_per_cu;
}

// ---- The grid-wide schedule: the same wrap-around rule with the whole grid as the "workgroup" ---------------------------------
// Workgroups of one launch get floor or ceil(n_tiles / gx) tiles, and the balanced schedule above cannot move work between them
// (1888 tiles on 128 workgroups: 14 or 15 tiles, 124 or 132 steps on the worst SIMD).  Here ALL of a direction's tiles x T steps
// are laid end to end and global wave g = workgroup * nwaves + wave takes cf_gru_balanced_share(n_tiles, gx * nwaves, g, T):
// shares differ by one step over the whole chip (64 or 65 at that size: 130).  Pieces, their order and the hand-off are the same;
// the one new thing is that the tail of a workgroup's wave 0 takes h from the LAST wave of the workgroup before it.
//
// Progress.  A tail waits only for the wave with the next lower global index.  That wave runs the wanted head before anything
// else and waits for nothing first, and it belongs to the same workgroup or to the one with the next lower index, which the
// dispatcher starts no later than this one (workgroups are dispatched in index order, x fastest, and a direction is a row of the
// grid): whenever a tail waits, its head is running or done -- no residency of the whole grid is assumed.  With every share at
// least T steps a head is over within T steps of its wave's start while the tail that needs it begins no earlier than
// share - T steps after ITS start (29 steps later at the benchmark's size), so in practice the wait does not spin; it is bounded
// all the same (gru_layer_kernel).
//
// Feasible: no empty share and no interior piece.  n_tiles >= gx * nwaves is sufficient (every share is then at least T steps,
// and a share of T steps or more that neither starts nor ends on a tile edge still crosses one), and it is also what the
// progress argument's "does not spin" needs, so it is the test.
CF_BAL_HD inline bool cf_gru_gridwide_ok(int n_tiles, int gx, int nwaves) {
    return gx >= 1 && nwaves >= 1 && (long long)n_tiles >= (long long)gx * nwaves;
}

// Worst SIMD load of the grid-wide schedule in steps: over the workgroups, the sum of the ceil(nwaves / 4) largest shares of that
// workgroup's waves, times the workgroups that share a CU; -1 when infeasible.
CF_BAL_HD inline int cf_gru_gridwide_load(int n_tiles, int gx, int nwaves, int wg_per_cu, int T) {
    if (!cf_gru_gridwide_ok(n_tiles, gx, nwaves)) return -1;
    const int per_simd = (nwaves + 3) / 4;
    const long long total = (long long)n_tiles * T, W = (long long)gx * nwaves;
    // shares are floor(total / W) or one more; walk the cut points without a division per wave
    const int q = (int)(total / W), r = (int)(total % W);
    int worst = 0;
    long long rem = 0;                  // (g * total) % W
    for (int b = 0; b < gx; ++b) {
        int big = 0;                    // waves of this workgroup with q + 1 steps
        for (int w = 0; w < nwaves; ++w) {
            rem += r;
            if (rem >= W) { rem -= W; ++big; }
        }
        const int v = per_simd * q + (big < per_simd ? big : per_simd);
        if (v > worst) worst = v;
    }
    return worst * wg_per_cu;
}

// launch_gru's choice.  gx: the usual grid (workgroups per direction), wg_per_cu of them on a CU; gx_one: the
// one-workgroup-per-CU grid of a layer whose weights leave room for two (0: the layer has no second grid).
// forced: CATFISH_GRU_BALANCE, -1 = unset: 0 round-robin, 1 balanced inside workgroups on the usual grid, 2 the same with the
// second grid where it exists, 3 grid-wide wherever feasible (second grid first).  Unforced, the in-workgroup schedules are weighed
// as they always were and the grid-wide one is taken only where its worst SIMD load is strictly below all of them, so a size
// that divides evenly runs what it ran.
struct cf_gru_choice {
    int balance;    // 0 round-robin, 1 balanced inside each workgroup, 2 grid-wide
    int gx;         // workgroups per direction
    int load;       // worst SIMD load of the chosen schedule, steps
};
CF_BAL_HD inline cf_gru_choice cf_gru_choose(int n_tiles, int gx, int gx_one, int nwaves, int wg_per_cu, int T, int forced) {
    const bool two = gx_one > 0 && gx > gx_one;
    const int load_rr = cf_gru_grid_load(n_tiles, gx, nwaves, wg_per_cu, T, 0);
    const int load_bal = cf_gru_grid_load(n_tiles, gx, nwaves, wg_per_cu, T, 1);
    const int load_one = two ? cf_gru_grid_load(n_tiles, gx_one, nwaves, 1, T, 1) : -1;
    const int load_grid = cf_gru_gridwide_load(n_tiles, gx, nwaves, wg_per_cu, T);
    const int load_grid_one = two ? cf_gru_gridwide_load(n_tiles, gx_one, nwaves, 1, T) : -1;
    cf_gru_choice c = {0, gx, load_rr};
    if (forced < 0 ? (load_bal >= 0 && load_bal < c.load) : (forced >= 1 && load_bal >= 0)) { c.balance = 1; c.load = load_bal; }
    if (forced < 0 ? (load_one >= 0 && load_one < c.load) : (forced >= 2 && load_one >= 0)) { c.balance = 1; c.gx = gx_one; c.load = load_one; }
    if (forced < 0 ? (load_grid >= 0 && load_grid < c.load) : (forced == 3 && load_grid >= 0)) { c.balance = 2; c.gx = gx; c.load = load_grid; }
    if (forced < 0 ? (load_grid_one >= 0 && load_grid_one < c.load) : (forced == 3 && load_grid_one >= 0)) { c.balance = 2; c.gx = gx_one; c.load = load_grid_one; }
    return c;
}
