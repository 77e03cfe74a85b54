// Validation curves: the bin of a probability and the cell of a sample in the [3][bins] histogram (plain C++17, no device work;
// catfish_amd/device_validation.py states the same rules in numpy -- curve_bins, curve_bin and curve_host are normative).
//
// A probability is binned by the bit pattern of its float32: non-negative floats order as their bits do, so with t_b the float
// whose bits are b << shift,  p >= t_b  <=>  bin(p) >= b  for every p in [0, 1].  1.0 is 0x3F800000 = 127 << 23, a multiple of
// every 1 << shift with shift <= 23, so the top bin (0x3F800000 >> shift) starts exactly at 1.0; what lies above it (1 + ulp, +inf,
// positive NaN) is clamped into it, and every pattern with the sign bit (-0.0, negatives, negative NaN) goes to bin 0.  No bit
// pattern gives a bin outside [0, bins).
//
// csrc/validation_curve.hpp calls these for every cell it counts; tests/native/validation_curve_bin_shim.cpp puts them behind a C
// ABI for a sweep over all 2^32 patterns (tests/test_validation_curve_host.py).  Under hipcc the functions are __host__ __device__.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VC_HD __host__ __device__ __forceinline__
#else
#define VC_HD inline
#endif

#define VC_ONE_BITS 0x3F800000u  // float32 1.0
#define VC_SHIFT_MIN 10
#define VC_SHIFT_MAX 22
#define VC_ROWS 3                // label == 1, label == 0, any other label
#define VC_NO_KEY 0xffffffffu    // no sample here; above every cell (3 * bins <= 3 * 1040385 at shift 10)

VC_HD bool vc_shift_ok(int shift) { return shift >= VC_SHIFT_MIN && shift <= VC_SHIFT_MAX; }

// bins of the table, shift checked by the caller
VC_HD uint32_t vc_bins(int shift) { return (VC_ONE_BITS >> shift) + 1u; }

VC_HD uint32_t vc_bin(uint32_t bits, int shift) {
    const int32_t s = (int32_t)bits;
    const uint32_t v = (s < 0 ? 0u : (uint32_t)s) >> shift, top = VC_ONE_BITS >> shift;
    return v > top ? top : v;
}

VC_HD uint32_t vc_row(uint32_t label) { return label == 1u ? 0u : (label == 0u ? 1u : 2u); }

// the sample's cell in the flat [VC_ROWS][bins] table: always below VC_ROWS * vc_bins(shift)
VC_HD uint32_t vc_key(uint32_t bits, uint32_t label, int shift) { return vc_row(label) * vc_bins(shift) + vc_bin(bits, shift); }
