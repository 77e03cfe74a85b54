// catfish_amd/csrc/anysize_launch.hpp (the launch shape of the any-size training recurrences: plain C++, no device work)
// behind a C ABI, for tests/test_anysize_launch.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/anysize_launch.hpp"
#include "../../catfish_amd/csrc/anysize_infer_launch.hpp"      // ... and of the any-size inference recurrences

extern "C" {
// out[10]: the class {h_via_y, gru_waves, gru_lds, gru2_waves, gru2_lds}, then the launch {kernel, waves, grid_x, lds_bytes, h_via_y}
void shim_anysize_infer_shape(int h16, int x3, int one_tile_only, int waves_cap, int tuned, int kbx, int n_tiles, int n_cu, long long* out) {
    const cf_anysize_infer_class c = cf_anysize_infer_class_for(h16, x3 != 0, one_tile_only != 0, waves_cap);
    const cf_anysize_infer_launch s = cf_anysize_infer_shape_for(c, tuned != 0, kbx, n_tiles, n_cu);
    out[0] = c.h_via_y; out[1] = c.gru_waves; out[2] = (long long)c.gru_lds; out[3] = c.gru2_waves; out[4] = (long long)c.gru2_lds;
    out[5] = s.kernel; out[6] = s.waves; out[7] = s.grid_x; out[8] = (long long)s.lds_bytes; out[9] = s.h_via_y;
}

// out[6]: waves, max_waves, grid_x, lds_bytes, arrays, h_via_y
void shim_anysize_shape(int backward, int h16, int n_tiles, int n_cu, long long* out) {
    const cf_anysize_shape s = backward ? cf_anysize_backward_shape(h16, n_tiles, n_cu) : cf_anysize_forward_shape(h16, n_tiles, n_cu);
    out[0] = s.waves; out[1] = s.max_waves; out[2] = s.grid_x; out[3] = (long long)s.lds_bytes; out[4] = s.arrays; out[5] = s.h_via_y;
}
}
