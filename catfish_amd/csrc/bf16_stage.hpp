// bf16_stage.hpp -- the activation layout of the bf16 / bf16x3 kernels, decoded on the host (cf_debug_stage).  Plain C++: no HIP
// types and no device work, so tests/test_bf16_stage_decode.py compiles it with g++ (tests/native/bf16_stage_shim.cpp).
//
// Between the kernels of these precisions an activation of F features (32 behind the residual stack, 128 behind a biGRU layer) is
//   [tile32][t < T][kb < F / 16][part < NP][lane < 64][8 bf16]            (16 B per lane, 1 KiB per fragment)
// a tile is 32 windows, lane l holds window l & 31 of its tile, and element j of lane-half l >> 5 of k-block kb is feature
// cf_bf16_frag_feature(kb, l >> 5, j) (frag_feature32 of gru_bf16.hpp: catfish_hip.hip asserts that the two agree).  NP = 1: the
// value rounded to bf16.  NP = 2: part 0 = hi = bf16(v), part 1 = lo = bf16(v - hi); hi + lo is exact in a float.
#pragma once
#include <cstdint>
#include <cstring>

constexpr int cf_bf16_frag_feature(int kb, int hh, int j) { return 32 * (kb >> 1) + 16 * (kb & 1) + 8 * (j >> 2) + 4 * hh + (j & 3); }

// bf16 elements of the fragments that hold `n_windows` windows (whole 32-window tiles)
constexpr int64_t cf_bf16_stage_elems(int64_t n_windows, int t_len, int feats, int np) {
    return ((n_windows + 31) / 32) * t_len * (feats / 16) * np * 64 * 8;
}

static inline float cf_bf16_bits_to_float(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// frag: cf_bf16_stage_elems(...) bf16 bit patterns -> out [n_windows][t_len][feats]; windows past n_windows in the last tile are
// not read.  feats: a multiple of 16; np: 1 or 2.
static inline void cf_bf16_stage_decode(const uint16_t* frag, int64_t n_windows, int t_len, int feats, int np, float* out) {
    const int kbs = feats / 16;
    for (int64_t w = 0; w < n_windows; ++w)
        for (int t = 0; t < t_len; ++t)
            for (int kb = 0; kb < kbs; ++kb)
                for (int hh = 0; hh < 2; ++hh) {
                    const int lane = 32 * hh + (int)(w & 31);
                    const uint16_t* src = frag + (((((w >> 5) * t_len + t) * kbs + kb) * np) * 64 + lane) * 8;
                    for (int j = 0; j < 8; ++j) {
                        float v = cf_bf16_bits_to_float(src[j]);
                        if (np == 2) v += cf_bf16_bits_to_float(src[64 * 8 + j]);
                        out[(w * t_len + t) * feats + cf_bf16_frag_feature(kb, hh, j)] = v;
                    }
                }
}
