// The grid-wide part of catfish_amd/csrc/gru_balance.hpp (shares dealt over all waves of a direction, its feasibility test, its
// load model and launch_gru's choice between the schedules: plain C++, no device work) behind a C ABI, for
// tests/test_gru_grid_balance.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/gru_balance.hpp"

extern "C" {
// Share of global wave g = workgroup * nwaves + wave.  out[8]: head_tile, head_end, whole_first, whole_count, tail_tile,
// tail_begin, interior, steps (tile indices count from the direction's first tile)
void shim_gridwide_share(int n_tiles, int gx, int nwaves, int g, int T, int* out) {
    const cf_gru_share s = cf_gru_balanced_share(n_tiles, gx * nwaves, g, T);
    out[0] = s.head_tile; out[1] = s.head_end; out[2] = s.whole_first; out[3] = s.whole_count;
    out[4] = s.tail_tile; out[5] = s.tail_begin; out[6] = s.interior; out[7] = s.steps;
}
int shim_gridwide_ok(int n_tiles, int gx, int nwaves) { return cf_gru_gridwide_ok(n_tiles, gx, nwaves) ? 1 : 0; }
int shim_gridwide_load(int n_tiles, int gx, int nwaves, int wg_per_cu, int T) {
    return cf_gru_gridwide_load(n_tiles, gx, nwaves, wg_per_cu, T);
}
int shim_grid_load(int n_tiles, int gx, int nwaves, int wg_per_cu, int T, int balanced) {
    return cf_gru_grid_load(n_tiles, gx, nwaves, wg_per_cu, T, balanced);
}
// out[3]: balance (0 round-robin, 1 inside workgroups, 2 grid-wide), workgroups per direction, worst SIMD load
void shim_choose(int n_tiles, int gx, int gx_one, int nwaves, int wg_per_cu, int T, int forced, int* out) {
    const cf_gru_choice c = cf_gru_choose(n_tiles, gx, gx_one, nwaves, wg_per_cu, T, forced);
    out[0] = c.balance; out[1] = c.gx; out[2] = c.load;
}
}
