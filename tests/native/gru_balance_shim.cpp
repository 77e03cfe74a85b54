// catfish_amd/csrc/gru_balance.hpp (the biGRU throughput kernel's schedule: plain C++, no device work) behind a C ABI, for
// tests/test_gru_balance.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/gru_balance.hpp"

extern "C" {
// out[8]: head_tile, head_end, whole_first, whole_count, tail_tile, tail_begin, interior, steps
void shim_balanced_share(int tiles, int nwaves, int wave, int T, int* out) {
    const cf_gru_share s = cf_gru_balanced_share(tiles, nwaves, wave, T);
    out[0] = s.head_tile; out[1] = s.head_end; out[2] = s.whole_first; out[3] = s.whole_count;
    out[4] = s.tail_tile; out[5] = s.tail_begin; out[6] = s.interior; out[7] = s.steps;
}
int shim_round_robin_steps(int tiles, int nwaves, int wave, int T) { return cf_gru_round_robin_steps(tiles, nwaves, wave, T); }
int shim_balance_ok(int tiles, int nwaves, int T) { return cf_gru_balance_ok(tiles, nwaves, T) ? 1 : 0; }
int shim_simd_load(int tiles, int nwaves, int T, int balanced) { return cf_gru_simd_load(tiles, nwaves, T, balanced); }
int shim_grid_load(int n_tiles, int gx, int nwaves, int wg_per_cu, int T, int balanced) {
    return cf_gru_grid_load(n_tiles, gx, nwaves, wg_per_cu, T, balanced);
}
}
