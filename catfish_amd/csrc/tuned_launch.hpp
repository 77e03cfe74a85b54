// Launch plan of the tuned path (64 GRU units, 32 conv channels; the kernels of catfish_hip.hip and the headers it includes): every
// decision the host takes before a launch -- which kernel, waves per workgroup, grid, dynamic LDS bytes, chunk counts, what the
// launch leaves behind -- as pure functions of (tiles, CUs, the kernels' pack sizes, the debug knobs).  Plain C++17: no device
// types and no getenv, so tests/test_tuned_launch.py compiles it with g++ (tests/native/tuned_launch_shim.cpp) and sweeps it
// on the CPU.  catfish_hip.hip fills cf_knobs once per pass (cf_read_knobs) and executes the plans; it decides nothing itself.
//
// The regimes, by 16-window tiles n of a call on C CUs (DESIGN.md "Tuned path: launch regimes" has the table for 256 CUs):
//   n <= hoist limit (3 C / 16)  cooperative kernels, four waves per tile, x projection / dx on the idle CUs around them
//   n <= C                       cooperative kernels, up to two rounds of one (tile, direction) per CU
//   n >  C                       throughput kernels, one wave per tile, 1 / 2 / 4 / 8 waves per workgroup (cf_pick_waves)
//   n >= 48 (C / 2) - 7          fuse_layers = auto: all biGRU layers of an fp32 model in one launch
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#ifndef CF_T                // (catfish_hip.hip defines both before it includes this header)
#define CF_T 35             // window length
#define CF_TILE 16          // windows per tile
#endif
#define CF_GRU_MAX_WAVES 8                              // waves of a gru_layer_kernel workgroup: one hand-off flag (LDS) and one hand-off slot each
#define CF_COOP_XCH_FLOATS (2 * 4 * 64 * 4 + 4 * 64)    // LDS exchange area of the cooperative kernel: h, r*h, dense partials
#define CF_COOP_BWD_XCH_FLOATS (3 * 4 * 64 * 4)         // da_c, da_r, da_u exchange tiles
#include "gru_balance.hpp"

constexpr int CF_LDS_LIMIT = 160 * 1024;                // LDS of one CU (gfx950)
// `balance` of gru_layer_kernel: the schedule in the low bits, CF_GRU_RUN_ZERO_PRODUCTS on top of it
enum { CF_GRU_SCHED_MASK = 3, CF_GRU_RUN_ZERO_PRODUCTS = 4 };

// ---- debug knobs ------------------------------------------------------------------------------------------------------------------
// One int per CATFISH_* knob that changes a launch (tools/README.md lists their meanings); CF_KNOB_UNSET where the variable is not
// set or CATFISH_DEBUG_KNOBS is off.  ablate_four_waves is not a knob: it carries bit 2 of the CF_ABLATE build macro.
constexpr int CF_KNOB_UNSET = INT_MIN;
struct cf_knobs {
    int coop = CF_KNOB_UNSET, waves = CF_KNOB_UNSET, gru_balance = CF_KNOB_UNSET, gru_gx = CF_KNOB_UNSET, gru_zero_products = CF_KNOB_UNSET;
    int xproj_lds = CF_KNOB_UNSET, xproj_chunks = CF_KNOB_UNSET, hoist_tiles = CF_KNOB_UNSET, fuse = CF_KNOB_UNSET;
    int bf16_waves = CF_KNOB_UNSET, bf16_wgs = CF_KNOB_UNSET, bf16_pipe = CF_KNOB_UNSET;
    int res_fuse = CF_KNOB_UNSET, res_tpw = CF_KNOB_UNSET, res_chunks = CF_KNOB_UNSET, dx_chunks = CF_KNOB_UNSET;
    int ablate_four_waves = 0;
};
inline bool cf_knob_set(int v) { return v != CF_KNOB_UNSET; }
inline int cf_knob_or(int v, int unset) { return cf_knob_set(v) ? v : unset; }

// ---- the rules every plan shares --------------------------------------------------------------------------------------------------
constexpr int cf_ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int cf_half_cus(int n_cu) { return std::max(1, n_cu / 2); }      // a direction's share of the chip
// `len`-step chunks of a tile's CF_T steps for a wish of `want` chunks: the count that leaves no empty chunk
inline int cf_whole_chunks(int want) { return cf_ceil_div(CF_T, cf_ceil_div(CF_T, std::max(1, std::min(CF_T, want)))); }

// Waves per workgroup: 8 (two per SIMD) when the pass fills the chip; fewer for small calls (a single read is 8 tiles x 2
// directions) so that the tiles spread over more CUs instead of sharing SIMDs -- the 35-step chain is latency-bound there.
inline int cf_pick_waves(int n_tile_tasks, int n_cu) {
    const int w = cf_ceil_div(n_tile_tasks, n_cu);
    return w <= 1 ? 1 : (w <= 2 ? 2 : (w <= 4 ? 4 : 8));
}

// THE cooperative rule (latency mode): up to two rounds of one (tile, direction) per CU (0.35 units each) beat one wave per tile
// (1 unit).  The fp32 residual stack, the fp32 biGRU in inference and training and the raw dense-partial buffer all switch here.
inline bool cf_coop_rule(int n_tiles, int n_cu) { return n_tiles <= n_cu; }
inline int cf_coop_max_tiles(int n_cu) { return n_cu; }
inline int cf_coop_gx(int n_tiles, int n_cu) { return std::min(n_tiles, cf_half_cus(n_cu)); }

// Largest call (tiles) whose x projection (training: also dx) is hoisted onto the idle CUs: measured crossover
// (tools/bench_latency.py with CATFISH_HOIST_TILES), hoisting pays up to ~48 tiles = 768 windows on 256 CUs.  Sizes d_xp.
inline int cf_hoist_limit(int n_cu, int64_t cap_tiles, const cf_knobs& k) {
    int xpt = (int)std::min<int64_t>(cap_tiles, std::max(1, 3 * n_cu / 16));
    if (cf_knob_set(k.hoist_tiles)) xpt = std::max(1, std::min(k.hoist_tiles, (int)cap_tiles));
    return xpt;
}
inline size_t cf_xp_floats(int hoist_tiles) { return (size_t)hoist_tiles * CF_T * 2 * 12 * 64 * 4; }     // d_xp: [tiles][35][2][12][64] f32x4

// fuse_layers = auto: the dynamically scheduled single launch pays from ~6 full-chip rounds of 8-tile groups per pass
inline int cf_fuse_min_groups(int n_cu) { return 6 * cf_half_cus(n_cu); }
inline int64_t cf_fuse_auto_min_windows(int n_cu) { return ((int64_t)8 * cf_fuse_min_groups(n_cu) - 8) * CF_TILE + 1; }
// fuse: 0 never, 1 always, 2 auto (cf_model::fuse)
inline bool cf_fuse_now(int fuse, int n_tiles, int n_cu) { return fuse == 1 || (fuse == 2 && cf_ceil_div(n_tiles, 8) >= cf_fuse_min_groups(n_cu)); }
inline int cf_fuse_mode(bool eligible, int fuse_layers, const cf_knobs& k) {
    int fuse = (eligible && fuse_layers >= 0) ? (fuse_layers > 0 ? 1 : 2) : 0;
    if (cf_knob_set(k.fuse) && fuse) fuse = k.fuse != 0 ? 1 : 0;
    return fuse;
}
constexpr int cf_fused_lds(int pack_bytes) { return pack_bytes + 16; }
struct cf_fused_plan { int groups, grid, threads, lds_bytes; };
inline cf_fused_plan cf_fused_plan_for(int n_tiles, int n_cu, int n_layers, int pack_bytes) {
    cf_fused_plan p;
    p.groups = cf_ceil_div(n_tiles, 8);
    p.grid = n_layers * std::min(p.groups, cf_half_cus(n_cu)) * 2;      // per layer: a pool of workgroups for both directions
    p.threads = 512;
    p.lds_bytes = cf_fused_lds(pack_bytes);
    return p;
}

// ---- hoisted x projection (gru_coop.hpp) ------------------------------------------------------------------------------------------
// workgroups per tile in gru_xproj_kernel: one step each while the call is tiny (parallelism), five steps each otherwise (the
// weight fragments are fetched from L2 once per workgroup)
inline int cf_xproj_chunks(int n_tiles) { return n_tiles <= 8 ? CF_T : 7; }
// chunks of steps per (tile, direction) for gru_xproj_lds_kernel: the count that minimises rounds x (staging + steps per chunk),
// in 0.01 us (staging the x region ~2.5 us at Cin = 128, a step = 96 MFMAs of 32 cycles per wave)
inline int cf_xproj_plan(int n_tiles, int n_cu, int cin) {
    const int stage = cin >= 128 ? 250 : 80, step = cin >= 128 ? 128 : 32;
    const int slots = std::max(1, n_cu) * (cin >= 128 ? 1 : 4);            // resident workgroups: 96 KiB of LDS each at Cin = 128
    int best = 1, best_cost = 1 << 30;
    for (int c = 1; c <= CF_T; ++c) {
        const int tl = (CF_T + c - 1) / c;
        if ((CF_T + tl - 1) / tl != c) continue;                           // (only chunk counts that leave no empty chunk)
        const int rounds = (2 * n_tiles * c + slots - 1) / slots;
        const int cost = rounds * (stage + tl * step);
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}
// x projection of a small call on the CUs its recurrence leaves idle: weights through LDS, chunks sized to fill the chip once;
// CATFISH_XPROJ_LDS=0 selects round 2's kernel (fragments straight from L2), CATFISH_XPROJ_CHUNKS another valid chunk count
struct cf_xproj_launch { int lds_kernel, chunks, grid_x, lds_bytes; };     // grid (grid_x, 2), 256 threads
inline cf_xproj_launch cf_xproj_launch_for(int n_tiles, int n_cu, int cin, int x_bytes, const cf_knobs& k) {
    cf_xproj_launch p;
    p.lds_kernel = cf_knob_or(k.xproj_lds, 1) != 0;
    p.chunks = !p.lds_kernel ? cf_xproj_chunks(n_tiles) : (cf_knob_set(k.xproj_chunks) ? cf_whole_chunks(k.xproj_chunks) : cf_xproj_plan(n_tiles, n_cu, cin));
    p.grid_x = n_tiles * p.chunks;
    p.lds_bytes = p.lds_kernel ? x_bytes : 0;
    return p;
}

// ---- fp32 biGRU layer, inference (launch_gru) -------------------------------------------------------------------------------------
constexpr int cf_gru_coop_lds(int pack_bytes) { return pack_bytes + CF_COOP_XCH_FLOATS * 4; }
constexpr int cf_gru_layer_lds(int pack_bytes) { return pack_bytes + CF_GRU_MAX_WAVES * 4; }
// At most two workgroups per CU and direction share the chip, whatever the knobs: the bound d_hand and d_hand_flags are sized from
inline int cf_gru_max_gx(int n_cu) { return 2 * cf_half_cus(n_cu); }
inline size_t cf_hand_bytes(int n_cu) { return (size_t)2 * cf_gru_max_gx(n_cu) * CF_GRU_MAX_WAVES * 4 * 64 * 16; }     // [2 dirs][workgroups][8 waves][4][64] f32x4
inline size_t cf_hand_flag_bytes(int n_cu) { return ((size_t)2 * cf_gru_max_gx(n_cu) * sizeof(unsigned) + 15) / 16 * 16; }
// dense partials: [2][tiles][35][16] from the throughput kernels, [2][tiles <= CUs][35][4][64] raw per-lane partials from the
// cooperative kernels (cf_gru_plan::raw_partials)
inline size_t cf_dense_partial_floats(int64_t cap_tiles, int n_cu) {
    return std::max((size_t)2 * cap_tiles * CF_T * 16, (size_t)2 * std::min<int64_t>(cap_tiles, cf_coop_max_tiles(n_cu)) * CF_T * 256);
}
// CATFISH_GRU_GX: run the throughput kernel on that many 8-wave workgroups per direction whatever the size of the call, so that
// a test reaches a workgroup boundary of the grid-wide schedule with a few dozen tiles
inline int cf_forced_gx(int n_cu, const cf_knobs& k) { return cf_knob_set(k.gru_gx) ? std::max(0, std::min(k.gru_gx, cf_gru_max_gx(n_cu))) : 0; }
inline bool cf_use_coop(int n_tiles, int n_cu, const cf_knobs& k) {
    if (cf_forced_gx(n_cu, k) > 0) return false;
    const bool coop = k.coop >= 0 ? k.coop != 0 : cf_coop_rule(n_tiles, n_cu);
    return coop && !k.ablate_four_waves && cf_coop_rule(n_tiles, n_cu);      // (the raw dense-partial buffer is sized for n_cu tiles)
}

struct cf_gru_plan {
    int coop;               // 1: gru_layer_coop_kernel (256 threads), 0: gru_layer_kernel
    int hoist;              // coop: the x projection runs first (xproj), the kernel reads it from d_xp
    cf_xproj_launch xproj;
    int waves, gx;          // workgroup = waves x 64 threads, grid (gx, 2 directions)
    int per_dir, wg_per_cu, gx_one;     // throughput: the usual grid's cap, workgroups sharing a CU, the one-per-CU grid (0: none)
    int balance;            // throughput: the kernel's balance word (cf_gru_choice::balance | CF_GRU_RUN_ZERO_PRODUCTS)
    int load;               // throughput with hand-off: worst SIMD load of the schedule, steps; else -1
    int lds_bytes;
    int raw_partials;       // a LAST launch leaves raw per-lane partials [2][tiles][35][4][64] in d_p (head_kernel's last argument)
};
// Throughput schedule (gru_balance.hpp): equal shares of steps instead of whole tiles, only where the worst SIMD gets strictly less
// to do, so a call that divides evenly and a small call run what they always ran.  A layer whose weights leave room for two
// workgroups per CU has a second candidate: ONE balanced workgroup per CU (at the benchmark's 1888 tiles, 7 or 8 tiles on 8 waves
// cannot be balanced inside a workgroup, 14 or 15 can: 132 steps against 140; measured).  CATFISH_GRU_BALANCE
// forces a schedule wherever it exists, for tests and A/B: 0 round-robin, 1 balanced on the usual grid, 2 balanced on the
// one-workgroup-per-CU grid, 3 grid-wide.  The grid-wide schedule (shares dealt over all waves of a direction, h handed across
// workgroup boundaries through Slot::d_hand_flags) is one more candidate on either grid, taken only where it beats all of the
// above: 130 against 132 steps at the benchmark's size, nothing at 1024 or 2048 tiles.  CATFISH_GRU_ZERO_PRODUCTS=1 runs step 0's
// products with the zero state instead of skipping them (gru_tile), for the bit-identity test and A/B.
// has_hand: the call has a model workspace behind it (Slot::d_hand, d_hand_flags); without, the kernel runs as it always did.
// (12 waves = 3 per SIMD measured +0.3 % on the Cin = 128 layers and costs the Cin = 32 layer its second workgroup per CU)
inline cf_gru_plan cf_gru_plan_for(int n_tiles, int n_cu, int cin, int pack_bytes, int x_bytes, int hoist_tiles, bool has_hand, const cf_knobs& k) {
    cf_gru_plan p = {};
    p.load = -1;
    if (cf_use_coop(n_tiles, n_cu, k)) {
        p.coop = p.raw_partials = 1;
        p.waves = 4;
        p.gx = cf_coop_gx(n_tiles, n_cu);
        p.hoist = cin >= 32 && n_tiles <= hoist_tiles;       // few tiles: the x projection runs on the idle CUs first
        if (p.hoist) p.xproj = cf_xproj_launch_for(n_tiles, n_cu, cin, x_bytes, k);
        p.lds_bytes = cf_gru_coop_lds(pack_bytes);
        return p;
    }
    const int gx_env = cf_forced_gx(n_cu, k);
    p.waves = gx_env > 0 ? 8 : k.waves > 0 ? std::min(k.waves, 8) : (k.ablate_four_waves ? 4 : cf_pick_waves(2 * n_tiles, n_cu));
    const int groups = cf_ceil_div(n_tiles, p.waves);       // one workgroup pass = one tile per wave
    p.per_dir = cf_half_cus(n_cu);                          // persistent: half the CUs per direction
    if (pack_bytes <= CF_LDS_LIMIT / 2) p.per_dir *= 2;     // two workgroups fit per CU
    p.gx = std::min(groups, p.per_dir);
    if (gx_env > 0) p.gx = std::min(gx_env, groups);
    p.balance = CF_GRU_RUN_ZERO_PRODUCTS;
    if (has_hand) {
        p.wg_per_cu = std::max(1, cf_ceil_div(2 * p.gx, n_cu));
        p.gx_one = gx_env > 0 ? 0 : cf_half_cus(n_cu);
        const cf_gru_choice c = cf_gru_choose(n_tiles, p.gx, p.gx_one, p.waves, p.wg_per_cu, CF_T, cf_knob_or(k.gru_balance, -1));
        p.balance = c.balance | (cf_knob_or(k.gru_zero_products, 0) != 0 ? CF_GRU_RUN_ZERO_PRODUCTS : 0);
        p.gx = c.gx;
        p.load = c.load;
    }
    p.lds_bytes = cf_gru_layer_lds(pack_bytes);
    return p;
}

// ---- bf16 / bf16x3 biGRU layer (launch_gru_bf16), 32-window tiles ------------------------------------------------------------------
struct cf_gru_bf16_plan {
    int pipe;               // 1: the software-pipelined kernel (np = 1: gru_bf16_pipe_kernel, np = 2: gru_bf16x3_pipe_kernel), 0: round 1's
    int waves, gx, lds_bytes;
};
inline cf_gru_bf16_plan cf_gru_bf16_plan_for(int n_tiles32, int n_cu, int np, int pack_bytes, const cf_knobs& k) {
    cf_gru_bf16_plan p;
    p.pipe = cf_knob_or(k.bf16_pipe, 1) != 0;
    p.lds_bytes = pack_bytes;
    p.waves = k.bf16_waves > 0 ? std::min(k.bf16_waves, 8) : cf_pick_waves(2 * n_tiles32, n_cu);
    int per_dir = cf_half_cus(n_cu);
    if (np == 2 && p.pipe) {
        // bf16x3: one wave per SIMD (512 registers), four waves per workgroup, one workgroup per CU whatever its LDS
        p.waves = std::min(p.waves, 4);
    } else if (pack_bytes <= CF_LDS_LIMIT / 2) {
        per_dir *= 2;
    }
    if (k.bf16_wgs > 0) per_dir = k.bf16_wgs;
    p.gx = std::min(cf_ceil_div(n_tiles32, p.waves), per_dir);     // one workgroup pass = one 32-window tile per wave
    return p;
}

// ---- residual stack ---------------------------------------------------------------------------------------------------------------
constexpr int CF_XS_BYTES = CF_TILE * CF_T * 4;         // a wave's staged raw samples, fp32 kernels: [16][35]
// fp32.  Latency mode (cf_coop_rule): one workgroup per tile, four waves, each streaming a quarter of the 35 positions.
// Throughput mode: the first two blocks as ONE launch (res_stack2_kernel), block 0's output stays in registers.
struct cf_res_plan {
    int split;                                  // latency mode
    int chunks, waves, grid;                    // per-block launches (res_block_kernel), waves x 64 threads
    int lds_first, lds_other;                   // ... of block 0 and of the others
    int fused;                                  // blocks 0 and 1 in one launch
    int stack_chunks, stack_waves, stack_grid, stack_lds;       // ... res_stack2_kernel<split>
};
constexpr int cf_res_stack2_lds(int pack_first_bytes, int pack_other_bytes, int waves) { return pack_first_bytes + pack_other_bytes + waves * CF_XS_BYTES; }
inline cf_res_plan cf_res_plan_for(int n_tiles, int n_cu, int n_blocks, int pack_first_bytes, int pack_other_bytes, const cf_knobs& k) {
    cf_res_plan p = {};
    p.split = cf_coop_rule(n_tiles, n_cu);
    p.chunks = p.split ? 4 : 1;
    p.waves = p.split ? 4 : std::min(4, cf_pick_waves(n_tiles, n_cu * 2));
    p.grid = p.split ? n_tiles : std::min(cf_ceil_div(n_tiles, p.waves), n_cu * 4);
    p.lds_first = pack_first_bytes + p.waves * CF_XS_BYTES;
    p.lds_other = pack_other_bytes;
    p.fused = n_blocks >= 2 && cf_knob_or(k.res_fuse, 1) != 0;
    // latency mode: chunks of positions, one wave each, spread over the idle CUs (about four waves per CU in all)
    p.stack_chunks = p.split ? cf_whole_chunks(std::max(4, (4 * n_cu) / std::max(1, n_tiles))) : 1;
    p.stack_waves = p.waves;
    p.stack_lds = cf_res_stack2_lds(pack_first_bytes, pack_other_bytes, p.stack_waves);
    p.stack_grid = std::min(cf_ceil_div(n_tiles * p.stack_chunks, p.stack_waves), n_cu * 3);     // 51 KB of LDS: three workgroups per CU
    return p;
}
// bf16 / bf16x3, 32-window tiles, 256 threads.  Blocks 0 and 1 as one launch on the bf16 matrix pipe (res_stack2_bf16_kernel<np, tpw>),
// positions cut into chunks for about four waves per SIMD.  bf16: two tiles per wave on request (CATFISH_RES_TPW=2: every LDS read
// of a weight fragment or bias vector feeds two tiles), else one, `one_tile_waves` (CF_RES_BF16_WAVES) waves per SIMD; bf16x3: one
// tile per wave (twice the fragments), two waves per SIMD.
struct cf_res_bf16_plan {
    int fused;                                  // blocks 0 and 1 in one launch
    int np, tpw, chunks, per_cu, stack_grid, stack_lds;
    int grid, lds_first, lds_other;             // per-block launches (res_block_bf16_kernel)
};
inline cf_res_bf16_plan cf_res_bf16_plan_for(int n_tiles32, int n_cu, int n_blocks, int np, int pack_first_bytes, int pack_other_bytes,
                                             int one_tile_waves, const cf_knobs& k) {
    cf_res_bf16_plan p = {};
    p.fused = n_blocks >= 2 && cf_knob_or(k.res_fuse, 1) != 0;
    p.np = np > 1 ? 2 : 1;
    // two tiles per wave exist for one bf16 part only; any other value would launch a kernel that covers 1 / tpw of the tiles
    p.tpw = (p.np == 1 && cf_knob_or(k.res_tpw, 1) == 2) ? 2 : 1;
    const bool one_tile = p.np == 1 && p.tpw == 1;
    const int groups = cf_ceil_div(n_tiles32, p.tpw);
    const int slots = (one_tile ? 4 * one_tile_waves : 8) * n_cu;       // wave tasks resident at once on the whole chip
    // as many chunks as keep every task resident in ONE round (a second, mostly empty round costs a whole chunk's chain)
    p.chunks = cf_whole_chunks(cf_knob_set(k.res_chunks) ? k.res_chunks : slots / std::max(1, groups));
    p.stack_lds = pack_first_bytes + pack_other_bytes + 4 * p.tpw * 32 * CF_T * 4;
    p.per_cu = std::max(1, std::min(one_tile ? one_tile_waves : 2, CF_LDS_LIMIT / p.stack_lds));
    p.stack_grid = std::min(cf_ceil_div(groups * p.chunks, 4), n_cu * p.per_cu);
    p.grid = std::min(cf_ceil_div(n_tiles32, 4), n_cu * 4);
    p.lds_first = pack_first_bytes + 4 * 32 * CF_T * 4;
    p.lds_other = pack_other_bytes;
    return p;
}

// ---- training: biGRU forward / backward, weight gradient, head ----------------------------------------------------------------------
// Small batch (cf_coop_rule): four waves per tile, up to two rounds; at or below the hoist limit the x projection runs before the
// forward and dx is formed after the backward (defer), both on the idle CUs.  The knobs of the inference launch do not apply.
constexpr int cf_train_coop_lds(bool backward, int pack_bytes) { return pack_bytes + (backward ? CF_COOP_BWD_XCH_FLOATS : CF_COOP_XCH_FLOATS) * 4; }
struct cf_train_gru_plan {
    int coop;               // 1: gru_train_{fwd,bwd}_coop_kernel (256 threads), 0: gru_train_{fwd,bwd}_kernel
    int hoist;              // forward: x projection first; backward: dx deferred to gru_dx_kernel
    cf_xproj_launch xproj;  // forward with hoist
    int dx_chunks, dx_grid_x;       // backward with hoist: gru_dx_kernel, grid (dx_grid_x, 2), 256 threads, no LDS
    int waves, gx, lds_bytes;
};
// chunks of steps per (tile, direction) of the deferred input-gradient launch (launch shape only, results do not depend on it)
// -- about 2.25 workgroups per CU: at the reference's batch (256 windows = 16 tiles) 18 chunks instead of round 5's 7 took the
// training step from 0.756 to 0.738 ms (profiles/r06_train_dx_chunks.log); few tiles keep one step per workgroup, many keep 7 chunks.
// The wish is rounded to the count that leaves no empty chunk (14 chunks are 3 steps each, which 12 cover); CATFISH_DX_CHUNKS is
// taken as given.
inline int cf_dx_chunks(int n_tiles, int n_cu, const cf_knobs& k) {
    if (cf_knob_set(k.dx_chunks)) return std::max(1, std::min(k.dx_chunks, CF_T));
    const int want = (9 * std::max(1, n_cu) / 4 + 2 * n_tiles - 1) / (2 * std::max(1, n_tiles));
    return cf_whole_chunks(std::max(7, want));
}
inline cf_train_gru_plan cf_train_gru_plan_for(bool backward, int n_tiles, int n_cu, int cin, int pack_bytes, int x_bytes, int hoist_tiles,
                                               const cf_knobs& k) {
    cf_train_gru_plan p = {};
    p.coop = cf_coop_rule(n_tiles, n_cu);
    if (p.coop) {
        p.waves = 4;
        p.gx = cf_coop_gx(n_tiles, n_cu);
        p.hoist = n_tiles <= hoist_tiles;
        p.lds_bytes = cf_train_coop_lds(backward, pack_bytes);
        if (p.hoist && !backward) p.xproj = cf_xproj_launch_for(n_tiles, n_cu, cin, x_bytes, k);
        if (backward) p.dx_chunks = cf_dx_chunks(n_tiles, n_cu, k);
        if (p.hoist && backward) p.dx_grid_x = n_tiles * p.dx_chunks;
        return p;
    }
    p.waves = cf_pick_waves(2 * n_tiles, n_cu);
    p.gx = std::min(cf_ceil_div(n_tiles, p.waves), cf_half_cus(n_cu));
    p.lds_bytes = pack_bytes;
    return p;
}
// Weight gradient: two directions x n_chunks workgroups should cover the chip about once; at least 8 (tile, step) pairs each keeps
// the partial sums (148 KiB per workgroup) well below the traffic of the operands themselves
struct cf_wgrad_plan { int pairs_per_wg, n_chunks; int64_t workspace_floats; };
inline cf_wgrad_plan cf_wgrad_plan_for(int n_tiles, int n_cu, int partial_floats) {
    cf_wgrad_plan p;
    const int n_pairs = n_tiles * CF_T;
    p.pairs_per_wg = std::max(8, cf_ceil_div(2 * n_pairs, n_cu));
    p.n_chunks = cf_ceil_div(n_pairs, p.pairs_per_wg);
    p.workspace_floats = (int64_t)p.n_chunks * 2 * partial_floats;      // gru_wgrad_kernel writes one partial per (chunk, direction)
    return p;
}
// Head: a wave takes ~8 (tile, t) items: few enough partial sums that the fixed-order reduction stays a couple of microseconds
struct cf_train_head_plan { int waves, grid; int64_t workspace_floats; };      // 256 threads: four waves per workgroup
inline cf_train_head_plan cf_train_head_plan_for(int64_t n_tiles, int n_cu, int part_floats) {
    cf_train_head_plan p;
    const int64_t items = n_tiles * CF_T;
    p.grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + 31) / 32, (int64_t)n_cu * 2));
    p.waves = p.grid * 4;
    p.workspace_floats = (int64_t)p.waves * part_floats;                // train_head_kernel writes one partial per wave
    return p;
}
