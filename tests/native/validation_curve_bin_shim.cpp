// catfish_amd/csrc/validation_curve_bin.hpp (the bin of a probability in the validation-curve histogram: plain C++, no device work)
// behind a C ABI, for tests/test_validation_curve_host.py:
//   g++ -std=c++17 -O3 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/validation_curve_bin.hpp"

extern "C" {
int shim_shift_ok(int shift) { return vc_shift_ok(shift) ? 1 : 0; }
unsigned shim_bins(int shift) { return vc_bins(shift); }
unsigned shim_bin(unsigned bits, int shift) { return vc_bin(bits, shift); }
unsigned shim_key(unsigned bits, unsigned label, int shift) { return vc_key(bits, label, shift); }
void shim_bin_many(const unsigned* bits, long long count, int shift, unsigned* out) {
    for (long long a = 0; a < count; ++a) out[a] = vc_bin(bits[a], shift);
}
// All 2^32 bit patterns, in three stretches.  out[0]: bins outside [0, NB); out[1]: places in [0.0, 1.0] where the bin falls from
// one pattern to the next; out[2]: patterns in [0.0, 1.0] whose bin is not bits >> shift; out[3]: patterns above 1.0 without the sign
// bit that miss the top bin; out[4]: patterns with the sign bit that miss bin 0.
void shim_sweep(int shift, long long* out) {
    const unsigned nb = vc_bins(shift);
    unsigned long long outside = 0, falls = 0, other = 0, not_top = 0, not_zero = 0;
    for (unsigned long long v = 0; v <= VC_ONE_BITS; ++v) {
        const unsigned bin = vc_bin((unsigned)v, shift);
        outside += bin >= nb;
        falls += v > 0 && bin < vc_bin((unsigned)v - 1u, shift);
        other += bin != ((unsigned)v >> shift);
    }
    for (unsigned long long v = VC_ONE_BITS + 1ull; v < 0x80000000ull; ++v) {
        const unsigned bin = vc_bin((unsigned)v, shift);
        outside += bin >= nb;
        not_top += bin != nb - 1u;
    }
    for (unsigned long long v = 0x80000000ull; v < 0x100000000ull; ++v) {
        const unsigned bin = vc_bin((unsigned)v, shift);
        outside += bin >= nb;
        not_zero += bin != 0u;
    }
    out[0] = (long long)outside; out[1] = (long long)falls; out[2] = (long long)other; out[3] = (long long)not_top; out[4] = (long long)not_zero;
}
}
