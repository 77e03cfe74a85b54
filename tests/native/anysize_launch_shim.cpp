// catfish_amd/csrc/anysize_launch.hpp (the launch shape of the any-size training recurrences: plain C++, no device work)
// behind a C ABI, for tests/test_anysize_launch.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/anysize_launch.hpp"

extern "C" {
// out[6]: waves, max_waves, grid_x, lds_bytes, arrays, h_via_y
void shim_anysize_shape(int backward, int h16, int n_tiles, int n_cu, long long* out) {
    const cf_anysize_shape s = backward ? cf_anysize_backward_shape(h16, n_tiles, n_cu) : cf_anysize_forward_shape(h16, n_tiles, n_cu);
    out[0] = s.waves; out[1] = s.max_waves; out[2] = s.grid_x; out[3] = (long long)s.lds_bytes; out[4] = s.arrays; out[5] = s.h_via_y;
}
}
