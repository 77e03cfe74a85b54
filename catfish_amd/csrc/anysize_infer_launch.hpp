// Launch shape of the any-size inference recurrences (gen_build / gen_run_pass in csrc/generic_host.hpp; the kernels are
// gen_gru_kernel<false, X3> and gen_gru2_kernel of csrc/generic.hpp, and gru_layer_kernel of the tuned path for 64-unit layers
// with 16 / 32 / 128 inputs): plain host C++, no device types, so that tests/test_anysize_launch.py can compile it with g++
// (tests/native/anysize_launch_shim.cpp).  cf_anysize_infer_shape reports it per biGRU layer.
//
// What a model fixes when it is built (cf_anysize_infer_class_for), by layer size:
//
//   one-tile kernel (one wave = one 16-window tile of one direction, state in LDS, h16 KB per array):
//     16 .. 96     three arrays (h, r.h, h'), up to 8 waves          (96: 8 x 3 x 6 KB = 147 456 B)
//     112 .. 160   h_via_y (two arrays), up to 8 waves               (160: 8 x 2 x 10 KB = 163 840 B, the whole LDS)
//     176 .. 256   h_via_y, up to 4 waves                            (256: 4 x 2 x 16 KB = 131 072 B)
//   two-tile kernel (one wave = two tiles, two arrays per tile = 4 h16 KB per wave): fp32 only, layer sizes that are a multiple
//     of 64: 64 at 8 waves (131 072 B), 128 at 4 waves (131 072 B); 192 and 256 fit neither and never take it.
//
// What a pass of n_tiles tiles decides (cf_anysize_infer_shape_for), per layer: a layer with a tuned pack runs the LDS-resident
// kernel in the launch regimes of csrc/tuned_launch.hpp; otherwise the two-tile kernel when the model has one, the layer's input
// is a multiple of 64 features (kbx % 4 == 0) and there are at least 2 n_cu tiles, always at its full wave count; otherwise the
// one-tile kernel with ceil(2 tiles / n_cu) waves per workgroup, at least 1 and at most the class's count, and the dynamic LDS
// of that many waves.
#pragma once

#include "anysize_launch.hpp"

enum { CF_ANYSIZE_INFER_TUNED = 0, CF_ANYSIZE_INFER_ONE_TILE = 1, CF_ANYSIZE_INFER_TWO_TILE = 2 };

struct cf_anysize_infer_class {
    int h_via_y = 0;        // one-tile kernel: h' is re-read from the layer's output instead of a third LDS array
    int gru_waves = 8;      // one-tile kernel: most waves per workgroup
    size_t gru_lds = 0;     //   and their dynamic LDS (the kernel's opt-in limit)
    int gru2_waves = 0;     // two-tile kernel: waves per workgroup, 0 = the model does not use it
    size_t gru2_lds = 0;
};

struct cf_anysize_infer_launch {
    int kernel;             // CF_ANYSIZE_INFER_*
    int waves;              // waves per workgroup (0 for the tuned kernel: see csrc/tuned_launch.hpp)
    int grid_x;             // workgroups per direction (grid y = 2 directions)
    size_t lds_bytes;       // dynamic LDS of the launch
    int h_via_y;            // as passed to the one-tile kernel; 0 for the others
};

// x3: CF_PREC_BF16X3.  one_tile_only / waves_cap (0 = none): the A/B knobs CATFISH_GEN_ONE_TILE / CATFISH_GEN_WAVES.
inline cf_anysize_infer_class cf_anysize_infer_class_for(int h16, bool x3, bool one_tile_only, int waves_cap) {
    cf_anysize_infer_class c;
    size_t per_wave = (size_t)3 * h16 * CF_ANYSIZE_ARRAY_BYTES;
    c.h_via_y = per_wave * 8 > CF_ANYSIZE_LDS_LIMIT ? 1 : 0;
    if (c.h_via_y) per_wave = (size_t)2 * h16 * CF_ANYSIZE_ARRAY_BYTES;
    c.gru_waves = per_wave * 8 <= CF_ANYSIZE_LDS_LIMIT ? 8 : 4;
    if (waves_cap > 0 && waves_cap < c.gru_waves) c.gru_waves = waves_cap;
    c.gru_lds = per_wave * c.gru_waves;
    const size_t per_wave2 = (size_t)2 * 2 * h16 * CF_ANYSIZE_ARRAY_BYTES;
    c.gru2_waves = (h16 % 4) != 0 || x3 || one_tile_only ? 0
                   : (per_wave2 * 8 <= CF_ANYSIZE_LDS_LIMIT ? 8 : (per_wave2 * 4 <= CF_ANYSIZE_LDS_LIMIT ? 4 : 0));
    c.gru2_lds = per_wave2 * c.gru2_waves;
    return c;
}

// tuned: the layer has a pack of the LDS-resident kernel; kbx: 16-feature blocks of the layer's input.
inline cf_anysize_infer_launch cf_anysize_infer_shape_for(const cf_anysize_infer_class& c, bool tuned, int kbx, int n_tiles, int n_cu) {
    cf_anysize_infer_launch s;
    s.h_via_y = 0;
    if (tuned) {
        s.kernel = CF_ANYSIZE_INFER_TUNED;
        s.waves = 0;
        s.grid_x = 0;
        s.lds_bytes = 0;
        return s;
    }
    if (c.gru2_waves && (kbx % 4) == 0 && n_tiles >= 2 * n_cu) {      // enough tiles to fill the chip two per wave
        const int pairs = (n_tiles + 1) / 2;
        s.kernel = CF_ANYSIZE_INFER_TWO_TILE;
        s.waves = c.gru2_waves;
        s.grid_x = (pairs + c.gru2_waves - 1) / c.gru2_waves;
        s.lds_bytes = c.gru2_lds;
        return s;
    }
    // small calls (the reference's one-read-per-call pattern): fewer waves per workgroup, so that the tiles spread over the CUs
    const int want = (2 * n_tiles + n_cu - 1) / n_cu;
    s.kernel = CF_ANYSIZE_INFER_ONE_TILE;
    s.waves = want < 1 ? 1 : (want > c.gru_waves ? c.gru_waves : want);
    s.grid_x = (n_tiles + s.waves - 1) / s.waves;
    s.lds_bytes = c.gru_lds / c.gru_waves * s.waves;
    s.h_via_y = c.h_via_y;
    return s;
}
