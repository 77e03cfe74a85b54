// Shifted-window voting: every rule by which retile_windows_kernel and vote_tilings_kernel (csrc/tilings.hpp) form a global-memory
// index (plain C++17: g++ and hipcc both compile it; under hipcc the functions are __host__ __device__).  catfish_amd/tilings.py
// states the result in numpy (retile_host and vote_host are the definitions); tests/native/tilings_replay.cpp runs the kernels' bodies
// serially over these functions under the sanitizers, with buffers of exactly the sizes the Python layer allocates.
//
// Base layout: read r owns packed samples offsets[r] .. offsets[r + 1] (multiples of 35), the first lengths[r] real; total =
// offsets[n].  Tiling j >= 1 shifts every read right by phi_j samples inside a region one window longer than the read's own:
//   T_j            = total + (j - 1) * (total + 35 n)                      first sample of tiling j in the one buffer (T_0 = 0)
//   read r there   = T_j + offsets[r] + 35 r,  offsets[r + 1] - offsets[r] + 35 samples
//   retiled[T_j + offsets[r] + 35 r + phi_j + i] = base[offsets[r] + i]    for 0 <= i < lengths[r]; every other sample is 0
// The tables live in device memory that a caller may have filled with anything: tl_sound vouches for a read's entries before an index
// is formed from them, and every index that passes lies in [0, total) (base) or [0, tiling size) (tilings) whatever the tables hold.
// A read whose entries are not sound is all zero in the tilings and keeps its base values in the vote.  Where `offsets` DESCENDS the
// search cannot tell which of two overlapping reads owns a sample: reads next to such a pair may come out zero / unvoted as well
// (still nothing outside the buffers is touched); with ascending offsets the result is exactly the definition.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TL_FN __host__ __device__ inline
#else
#define TL_FN inline
#endif

#define TL_WINDOW 35
#define TL_MAX_PHASES 8
#define TL_MAX_TOTAL (1LL << 40)         // samples of the base layout a call takes (the tiling size then stays far below 2^63)
#define TL_MAX_READS 0x7fffffffLL
#define TL_THREADS 256
#define TL_RETILE_CHUNK 4096             // destination samples per workgroup: four 16-byte stores per thread
#define TL_VOTE_CHUNK 2048               // base samples per workgroup: eight per thread

struct tl_phases { int32_t k; int32_t phi[TL_MAX_PHASES]; };      // travels by value in the kernel arguments

// ints, strictly ascending, phi_0 == 0, every phi_j in 0 .. 34, 1 <= K <= 8
TL_FN bool tl_phases_ok(const int32_t* phi, int32_t k) {
    if (!phi || k < 1 || k > TL_MAX_PHASES || phi[0] != 0) return false;
    for (int32_t j = 1; j < k; ++j)
        if (phi[j] <= phi[j - 1] || phi[j] >= TL_WINDOW) return false;
    return true;
}

// 0 when a call with these host arguments may launch; else which rule they break (the entry points answer CF_ERR_INVALID)
TL_FN int tl_refusal(int64_t n_reads, int64_t total, const int32_t* phi, int32_t k, int32_t weight) {
    if (n_reads < 0 || total < 0) return 1;
    if (n_reads > TL_MAX_READS || total > TL_MAX_TOTAL) return 2;
    if (total % TL_WINDOW != 0) return 3;
    if (!tl_phases_ok(phi, k)) return 4;
    if (weight != 0 && weight != 1) return 5;
    return 0;
}

TL_FN int64_t tl_region(int64_t total, int64_t n_reads) { return total + TL_WINDOW * n_reads; }          // one tiling, j >= 1
TL_FN int64_t tl_tiling_start(int32_t j, int64_t total, int64_t n_reads) {
    return j <= 0 ? 0 : total + (int64_t)(j - 1) * tl_region(total, n_reads);
}
TL_FN int64_t tl_tiling_size(int64_t total, int64_t n_reads, int32_t k) { return tl_tiling_start(k, total, n_reads); }

// weight 0 ("mean"): 1; weight 1 ("centre"): min(t + 1, 35 - t) for position t of the window -- 1 at both ends, 18 in the middle
TL_FN int32_t tl_weight(int32_t weight, int32_t t) {
    if (weight == 0) return 1;
    return t + 1 < TL_WINDOW - t ? t + 1 : TL_WINDOW - t;
}

// what the layout promises of read r's entries
TL_FN bool tl_sound(int64_t o0, int64_t o1, int64_t len, int64_t total) {
    return o0 >= 0 && o0 <= o1 && o1 <= total && o0 % TL_WINDOW == 0 && o1 % TL_WINDOW == 0 && len >= 0 && len <= o1 - o0;
}

// The largest r in [lo, hi) with offsets[r] + stride * r <= u, or -1 (an empty range, or the first entry lies beyond u).  Reads
// offsets[lo .. hi - 1] only; u >= 0 and stride * r is small, so nothing overflows whatever the table holds.  stride 0 searches the
// base layout, stride 35 a tiling region.
TL_FN int64_t tl_owner(const int64_t* offsets, int64_t lo, int64_t hi, int64_t u, int64_t stride) {
    if (hi <= lo || offsets[lo] > u - stride * lo) return -1;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= u - stride * mid) lo = mid; else hi = mid;
    }
    return lo;
}

// The reads [lo, hi) among which the owners of samples first .. last (first <= last) are searched: a workgroup finds them once for
// its chunk and every sample then searches only there.  With ascending offsets the result is that of a search over all n reads.
struct tl_range { int64_t lo, hi; };
TL_FN tl_range tl_chunk_reads(const int64_t* offsets, int64_t n_reads, int64_t first, int64_t last, int64_t stride) {
    const int64_t a = tl_owner(offsets, 0, n_reads, first, stride), b = tl_owner(offsets, 0, n_reads, last, stride);
    tl_range g = {a < 0 ? 0 : a, b + 1};
    return g;
}

// Destination samples [g0, g1) of a tiling region (indices relative to T_j) and where their values come from: a sound read's samples
// base[o0 .. o0 + len), or nothing (len == 0: all of [g0, g1) is zero).
struct tl_span { int64_t g0, g1, o0, len; };
TL_FN tl_span tl_locate(const int64_t* offsets, const int64_t* lengths, int64_t total, tl_range reads, int64_t u) {
    tl_span s = {u, u + 1, 0, 0};
    const int64_t r = tl_owner(offsets, reads.lo, reads.hi, u, TL_WINDOW);
    if (r < 0) return s;
    const int64_t o0 = offsets[r], o1 = offsets[r + 1], len = lengths[r];
    if (!tl_sound(o0, o1, len, total)) return s;
    const int64_t g0 = o0 + TL_WINDOW * r, g1 = o1 + TL_WINDOW * (r + 1);
    if (u >= g1) return s;                                                      // only when offsets descend somewhere
    s.g0 = g0; s.g1 = g1; s.o0 = o0; s.len = len;
    return s;
}
// the base index whose value destination sample u (inside s) of the tiling with phase phi holds, or -1 for a zero
TL_FN int64_t tl_source(const tl_span& s, int32_t phi, int64_t u) {
    const int64_t i = u - s.g0 - phi;
    return (i >= 0 && i < s.len) ? s.o0 + i : -1;                               // < o0 + len <= o1 <= total
}

// Base sample b: is it a real sample of a sound read?  Then `first` = offsets[r] + 35 r + i is where it sits in a tiling region at
// phase 0 (phase phi: first + phi < region, as i < len <= offsets[r + 1] - offsets[r]) and t0 = i % 35 its position in the base window.
struct tl_voter { bool votes; int64_t first; int32_t t0; };
TL_FN tl_voter tl_vote_where(const int64_t* offsets, const int64_t* lengths, int64_t total, tl_range reads, int64_t b) {
    tl_voter v = {false, 0, 0};
    const int64_t r = tl_owner(offsets, reads.lo, reads.hi, b, 0);
    if (r < 0) return v;
    const int64_t o0 = offsets[r], o1 = offsets[r + 1], len = lengths[r];
    if (!tl_sound(o0, o1, len, total)) return v;
    const int64_t i = b - o0;
    if (i >= len) return v;                                                     // the zero tail keeps the base value
    v.votes = true;
    v.first = o0 + TL_WINDOW * r + i;
    v.t0 = (int32_t)(i % TL_WINDOW);
    return v;
}

// The vote: float32((sum_j w(t_j) * double(p_j)) / (sum_j w(t_j))), both sums in double in the order j = 0 .. K - 1.  w * p is exact
// in double, so a fused multiply-add gives the same sum.  values: [tiling size] (base region first).
TL_FN float tl_vote_value(const float* values, const tl_phases& ph, int32_t weight, int64_t total, int64_t region, int64_t b,
                          const tl_voter& v) {
    double num = 0.0, den = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int32_t j = 0; j < TL_MAX_PHASES; ++j) {
        if (j < ph.k) {
            const int32_t s = v.t0 + ph.phi[j], t = s >= TL_WINDOW ? s - TL_WINDOW : s;
            const double w = (double)tl_weight(weight, t);
            const float p = j == 0 ? values[b] : values[total + (int64_t)(j - 1) * region + v.first + ph.phi[j]];
            num += w * (double)p;
            den += w;
        }
    }
    return (float)(num / den);
}
