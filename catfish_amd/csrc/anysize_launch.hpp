// Launch shape of the any-size training recurrences (cf_gru_anysize_train_forward = gen_gru_kernel<true, false>,
// cf_gru_anysize_train_backward = gen_gru_bwd_kernel; csrc/generic.hpp): plain host C++, no device types, so that
// tests/test_anysize_launch.py can compile it with g++ (tests/native/anysize_launch_shim.cpp).
//
// One wave runs one 16-window tile of one direction and keeps its state in LDS: `arrays` arrays of h16 x 64 f32x4 (h16 KB
// each).  The forward wants three (h, r.h, h'); when eight waves of three do not fit the 160 KB of a CU it keeps two and reads
// h' back from the layer's output (h_via_y).  The backward keeps four (dh, da_c, da_r, da_u).  A workgroup holds as many waves
// as fit, a power of two up to 8 (max_waves), but no more than it takes to give every CU two tiles: ceil(2 tiles / n_cu).  The
// kernels address wave w's state at w * arrays * h16 * 64, so the dynamic LDS of a launch is waves * arrays * h16 KB.
//
//   layer size   forward                               backward
//   16 .. 80     three arrays, up to 8 waves           up to 8 waves   (80: 8 waves = 163 840 B, the whole LDS)
//   96           three arrays, up to 8 waves           up to 4 waves
//   112 .. 160   h_via_y, up to 8 waves                up to 4 waves   (160: forward 8 waves and backward 4 waves = 163 840 B)
//   176 .. 256   h_via_y, up to 4 waves                up to 2 waves
#pragma once

#include <cstddef>

constexpr size_t CF_ANYSIZE_LDS_LIMIT = 160 * 1024;      // LDS of one CU (gfx950), all of it available to one workgroup
constexpr size_t CF_ANYSIZE_ARRAY_BYTES = 64 * 16;       // one state array of one wave, per 16 units: 64 lanes x f32x4

struct cf_anysize_shape {
    int waves;          // waves per workgroup of this launch
    int max_waves;      // what fits the LDS at this layer size: 8, 4, 2 or 1
    int grid_x;         // workgroups per direction (grid y = 2 directions); waves past the last tile return at once
    size_t lds_bytes;   // dynamic LDS of the launch
    int arrays;         // state arrays per wave
    int h_via_y;        // forward only: h' is re-read from the layer's output instead of a third LDS array
};

// The largest power-of-two wave count up to 8 whose state fits the LDS.
inline int cf_anysize_max_waves(int h16, int arrays) {
    const size_t per_wave = (size_t)arrays * h16 * CF_ANYSIZE_ARRAY_BYTES;
    return per_wave * 8 <= CF_ANYSIZE_LDS_LIMIT ? 8 : (per_wave * 4 <= CF_ANYSIZE_LDS_LIMIT ? 4 : (per_wave * 2 <= CF_ANYSIZE_LDS_LIMIT ? 2 : 1));
}

inline cf_anysize_shape cf_anysize_shape_for(int h16, int arrays, int h_via_y, int n_tiles, int n_cu) {
    cf_anysize_shape s;
    s.arrays = arrays;
    s.h_via_y = h_via_y;
    s.max_waves = cf_anysize_max_waves(h16, arrays);
    const int want = (2 * n_tiles + n_cu - 1) / n_cu;
    s.waves = want < 1 ? 1 : (want > s.max_waves ? s.max_waves : want);
    s.grid_x = (n_tiles + s.waves - 1) / s.waves;
    s.lds_bytes = (size_t)s.waves * arrays * h16 * CF_ANYSIZE_ARRAY_BYTES;
    return s;
}

inline cf_anysize_shape cf_anysize_forward_shape(int h16, int n_tiles, int n_cu) {
    const int via_y = cf_anysize_max_waves(h16, 3) < 8 ? 1 : 0;      // as in the inference launch: h' through y above 96 units
    return cf_anysize_shape_for(h16, via_y ? 2 : 3, via_y, n_tiles, n_cu);
}

inline cf_anysize_shape cf_anysize_backward_shape(int h16, int n_tiles, int n_cu) {
    return cf_anysize_shape_for(h16, 4, 0, n_tiles, n_cu);
}
