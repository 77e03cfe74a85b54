// catfish_amd/csrc/tuned_launch.hpp (the launch plans of the tuned 64 / 32 path: plain C++, no device work) behind a C ABI, for
// tests/test_tuned_launch.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
// knobs: cf_knobs as its ints in declaration order (SHIM_KNOBS of them), or null for "every knob unset".
#include "../../catfish_amd/csrc/tuned_launch.hpp"

enum { SHIM_KNOBS = 17 };
static_assert(sizeof(cf_knobs) == SHIM_KNOBS * sizeof(int), "knobs_of names every member of cf_knobs");
static cf_knobs knobs_of(const int* v) {
    cf_knobs k;
    if (!v) return k;
    k.coop = v[0]; k.waves = v[1]; k.gru_balance = v[2]; k.gru_gx = v[3]; k.gru_zero_products = v[4];
    k.xproj_lds = v[5]; k.xproj_chunks = v[6]; k.hoist_tiles = v[7]; k.fuse = v[8];
    k.bf16_waves = v[9]; k.bf16_wgs = v[10]; k.bf16_pipe = v[11];
    k.res_fuse = v[12]; k.res_tpw = v[13]; k.res_chunks = v[14]; k.dx_chunks = v[15];
    k.ablate_four_waves = v[16];
    return k;
}

extern "C" {
int shim_n_knobs() { return SHIM_KNOBS; }
int shim_knob_unset() { return CF_KNOB_UNSET; }

// out[12]: hoist limit (tiles), cooperative maximum (tiles), fuse-auto minimum (windows), largest biGRU grid per direction,
// hand-off bytes, hand-off flag bytes, d_p floats, d_xp floats of the hoist limit, fuse mode of an eligible model with
// fuse_layers = 0 (auto), LDS limit, T, tile
void shim_bounds(int n_cu, long long cap_tiles, const int* knobs, long long* out) {
    const cf_knobs k = knobs_of(knobs);
    const int hoist = cf_hoist_limit(n_cu, cap_tiles, k);
    out[0] = hoist; out[1] = cf_coop_max_tiles(n_cu); out[2] = cf_fuse_auto_min_windows(n_cu); out[3] = cf_gru_max_gx(n_cu);
    out[4] = (long long)cf_hand_bytes(n_cu); out[5] = (long long)cf_hand_flag_bytes(n_cu);
    out[6] = (long long)cf_dense_partial_floats(cap_tiles, n_cu); out[7] = (long long)cf_xp_floats(hoist);
    out[8] = cf_fuse_mode(true, 0, k); out[9] = CF_LDS_LIMIT; out[10] = CF_T; out[11] = CF_TILE;
}
int shim_pick_waves(int n_tile_tasks, int n_cu) { return cf_pick_waves(n_tile_tasks, n_cu); }
int shim_fuse_now(int fuse, int n_tiles, int n_cu) { return cf_fuse_now(fuse, n_tiles, n_cu) ? 1 : 0; }
int shim_xproj_plan(int n_tiles, int n_cu, int cin) { return cf_xproj_plan(n_tiles, n_cu, cin); }
int shim_dx_chunks(int n_tiles, int n_cu, const int* knobs) { return cf_dx_chunks(n_tiles, n_cu, knobs_of(knobs)); }

static void put_xproj(const cf_xproj_launch& x, int* out) { out[0] = x.lds_kernel; out[1] = x.chunks; out[2] = x.grid_x; out[3] = x.lds_bytes; }

// out[16]: coop, hoist, waves, gx, per_dir, wg_per_cu, gx_one, balance word, load, lds_bytes, raw_partials, 0, xproj {lds_kernel,
// chunks, grid_x, lds_bytes}
void shim_gru_plan(int n_tiles, int n_cu, int cin, int pack_bytes, int x_bytes, int hoist_tiles, int has_hand, const int* knobs, int* out) {
    const cf_gru_plan p = cf_gru_plan_for(n_tiles, n_cu, cin, pack_bytes, x_bytes, hoist_tiles, has_hand != 0, knobs_of(knobs));
    out[0] = p.coop; out[1] = p.hoist; out[2] = p.waves; out[3] = p.gx; out[4] = p.per_dir; out[5] = p.wg_per_cu; out[6] = p.gx_one;
    out[7] = p.balance; out[8] = p.load; out[9] = p.lds_bytes; out[10] = p.raw_partials; out[11] = 0;
    put_xproj(p.xproj, out + 12);
}
// out[4]: groups, grid, threads, lds_bytes
void shim_fused_plan(int n_tiles, int n_cu, int n_layers, int pack_bytes, int* out) {
    const cf_fused_plan p = cf_fused_plan_for(n_tiles, n_cu, n_layers, pack_bytes);
    out[0] = p.groups; out[1] = p.grid; out[2] = p.threads; out[3] = p.lds_bytes;
}
// out[4]: pipe, waves, gx, lds_bytes
void shim_gru_bf16_plan(int n_tiles32, int n_cu, int np, int pack_bytes, const int* knobs, int* out) {
    const cf_gru_bf16_plan p = cf_gru_bf16_plan_for(n_tiles32, n_cu, np, pack_bytes, knobs_of(knobs));
    out[0] = p.pipe; out[1] = p.waves; out[2] = p.gx; out[3] = p.lds_bytes;
}
// out[11]: split, chunks, waves, grid, lds_first, lds_other, fused, stack_chunks, stack_waves, stack_grid, stack_lds
void shim_res_plan(int n_tiles, int n_cu, int n_blocks, int pack_first_bytes, int pack_other_bytes, const int* knobs, int* out) {
    const cf_res_plan p = cf_res_plan_for(n_tiles, n_cu, n_blocks, pack_first_bytes, pack_other_bytes, knobs_of(knobs));
    out[0] = p.split; out[1] = p.chunks; out[2] = p.waves; out[3] = p.grid; out[4] = p.lds_first; out[5] = p.lds_other; out[6] = p.fused;
    out[7] = p.stack_chunks; out[8] = p.stack_waves; out[9] = p.stack_grid; out[10] = p.stack_lds;
}
// out[10]: fused, np, tpw, chunks, per_cu, stack_grid, stack_lds, grid, lds_first, lds_other
void shim_res_bf16_plan(int n_tiles32, int n_cu, int n_blocks, int np, int pack_first_bytes, int pack_other_bytes, int one_tile_waves,
                        const int* knobs, int* out) {
    const cf_res_bf16_plan p = cf_res_bf16_plan_for(n_tiles32, n_cu, n_blocks, np, pack_first_bytes, pack_other_bytes, one_tile_waves, knobs_of(knobs));
    out[0] = p.fused; out[1] = p.np; out[2] = p.tpw; out[3] = p.chunks; out[4] = p.per_cu; out[5] = p.stack_grid; out[6] = p.stack_lds;
    out[7] = p.grid; out[8] = p.lds_first; out[9] = p.lds_other;
}
// out[11]: coop, hoist, dx_chunks, dx_grid_x, waves, gx, lds_bytes, xproj {lds_kernel, chunks, grid_x, lds_bytes}
void shim_train_gru_plan(int backward, int n_tiles, int n_cu, int cin, int pack_bytes, int x_bytes, int hoist_tiles, const int* knobs, int* out) {
    const cf_train_gru_plan p = cf_train_gru_plan_for(backward != 0, n_tiles, n_cu, cin, pack_bytes, x_bytes, hoist_tiles, knobs_of(knobs));
    out[0] = p.coop; out[1] = p.hoist; out[2] = p.dx_chunks; out[3] = p.dx_grid_x; out[4] = p.waves; out[5] = p.gx; out[6] = p.lds_bytes;
    put_xproj(p.xproj, out + 7);
}
// out[3]: pairs_per_wg, n_chunks, workspace_floats
void shim_wgrad_plan(int n_tiles, int n_cu, int partial_floats, long long* out) {
    const cf_wgrad_plan p = cf_wgrad_plan_for(n_tiles, n_cu, partial_floats);
    out[0] = p.pairs_per_wg; out[1] = p.n_chunks; out[2] = p.workspace_floats;
}
// out[3]: waves, grid, workspace_floats
void shim_train_head_plan(long long n_tiles, int n_cu, int part_floats, long long* out) {
    const cf_train_head_plan p = cf_train_head_plan_for(n_tiles, n_cu, part_floats);
    out[0] = p.waves; out[1] = p.grid; out[2] = p.workspace_floats;
}
}
