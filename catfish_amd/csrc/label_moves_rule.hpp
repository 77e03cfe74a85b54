// Labels from a basecaller's move table: every rule by which label_moves_merge_kernel and label_moves_classes_kernel
// (csrc/label_moves.hpp) form a global-memory or LDS index, and the arithmetic that turns lengths in seconds into samples (plain
// C++17: g++ and hipcc both compile it; under hipcc the functions are __host__ __device__).  catfish_amd/labelling.py states the
// result in numpy (merge_moves_host, move_classes_host and MoveBatch.label_host are the definitions);
// tests/native/label_moves_replay.cpp runs the kernels' bodies serially over these functions under the sanitizers, with buffers of
// exactly the sizes the Python layer allocates.
//
// Layout: read r owns events event_offsets[r] .. event_offsets[r + 1] of `states` (uint8 [n_events, k]), `lengths` (float or double
// [n_events], seconds) and `moves` (int32); clipped[2 r], clipped[2 r + 1] are its clipped_start / clipped_end counted in MERGED
// events, n_raw[r] the samples of its raw signal, and it owns samples sample_offsets[r] .. sample_offsets[r + 1] of the outputs.
// An event with move != 0, and a read's first event whatever its move, is a head; a head and the events with move == 0 behind it
// are one merged event.  The work buffer (lm_work_bytes) holds the merged events of read r COMPACTED into the read's own slot
// [event_offsets[r], event_offsets[r + 1]) -- M <= E, so they fit; the entries behind the M-th are zero:
//     int32 mlen [n_events]    samples of the merged event
//     int32 start [n_events]   its first sample relative to the read (behind the M-th: where the last one ends)
//     int32 counts [2 n_reads] M and final = min(sum of mlen, n_raw) per read
//     uint8 cls, mbase, uniform [n_events] each: the class, the k-mer's middle byte, "the k-mer is one byte that is not 'N'"
// mbase / mlen / start / cls are exactly the tables label_expand_kernel (csrc/label_events.hpp) takes as bases / lengths / start /
// cls with the same event_offsets, so the expansion to per-sample bytes, and every rule of label_events_rule.hpp about tiles and
// samples, is shared: a sample is written only inside its tile inside its read, and a sample no merged event covers is 0.
//
// All tables live in device memory that a caller may have filled with anything, so nothing here trusts them:
//   - a read whose event range is not inside [0, n_events] has no events (le_events_sound): M = 0, final = 0;
//   - a length sum whose product with 4000 is not finite or not > 0 contributes no samples, one of 2^31 or more LE_SAT (lm_count_*);
//     the running sum of the counts saturates at LE_SAT (le_sat);
//   - a head walks its stays inside its read only (lm_stays_end takes the read's n);
//   - a function that cannot vouch for an index returns -1 ("skip").
// Sums go left to right from the head with one rounding per addition (lm_add_*), the product with one rounding (lm_mul_*), both in
// the table's own type: float32 sums differ from float64 ones, and from float32 sums in another order, often enough to matter.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "label_events_rule.hpp"

#define LM_THREADS LE_THREADS
#define LM_PIECE LE_PIECE                  // events per piece of both kernels: four per thread
#define LM_PER_THREAD LE_PER_THREAD
#define LM_MAX_KMER LE_MAX_KMER            // bytes of a model state: 1 .. 15, even ones too (the k-mer comes with the event)
#define LM_WIDEN LE_WIDEN
#define LM_CORE_SLOTS (LM_PIECE + 2 * LM_WIDEN)
#define LM_FREQUENCY 4000                  // samples per second: the reference's constant
#define LM_GRID LE_CLASS_GRID              // workgroups of the merge and the classes kernel; they stride over the reads

// 0 when a call with these host arguments may launch; else which rule they break (the entry point answers CF_ERR_INVALID)
LE_FN int lm_refusal(int64_t n_reads, int64_t n_events, int64_t total, int32_t k, int32_t lengths_f64, int64_t work_bytes) {
    if (n_reads < 0 || n_events < 0 || total < 0) return 1;
    if (n_events > LE_MAX_COUNT || total > LE_MAX_COUNT) return 2;
    if (k < 1 || k > LM_MAX_KMER) return 3;
    if (n_reads + total / LE_TILE > LE_MAX_BLOCKS) return 4;
    if (lengths_f64 != 0 && lengths_f64 != 1) return 6;
    if (work_bytes < 11 * n_events + 8 * n_reads) return 5;
    return 0;
}

// bytes of the work buffer, rounded up to 16 (never 0); -1 for sizes no call takes
LE_FN int64_t lm_work_bytes(int64_t n_reads, int64_t n_events) {
    if (n_reads < 0 || n_events < 0 || n_events > LE_MAX_COUNT || n_reads > LE_MAX_BLOCKS) return -1;
    const int64_t raw = 11 * n_events + 8 * n_reads;
    return raw < 16 ? 16 : (raw + 15) / 16 * 16;
}
// where the tables begin in it, in bytes (the int32 ones first: the buffer is 4-byte aligned)
LE_FN int64_t lm_work_mlen(int64_t, int64_t) { return 0; }
LE_FN int64_t lm_work_start(int64_t, int64_t n_events) { return 4 * n_events; }
LE_FN int64_t lm_work_counts(int64_t, int64_t n_events) { return 8 * n_events; }
LE_FN int64_t lm_work_cls(int64_t n_reads, int64_t n_events) { return 8 * n_events + 8 * n_reads; }
LE_FN int64_t lm_work_mbase(int64_t n_reads, int64_t n_events) { return 9 * n_events + 8 * n_reads; }
LE_FN int64_t lm_work_uniform(int64_t n_reads, int64_t n_events) { return 10 * n_events + 8 * n_reads; }

// ------------------------------------------------------------------------------------------------------------------ the arithmetic
// One IEEE addition / multiplication, rounded to nearest even, never contracted with its neighbour and never widened.
#if defined(__HIP_DEVICE_COMPILE__)
LE_FN float lm_add_f(float a, float b) { return __fadd_rn(a, b); }
LE_FN float lm_mul_f(float a, float b) { return __fmul_rn(a, b); }
LE_FN double lm_add_d(double a, double b) { return __dadd_rn(a, b); }
LE_FN double lm_mul_d(double a, double b) { return __dmul_rn(a, b); }
#else
LE_FN float lm_add_f(float a, float b) { volatile float s = a + b; return s; }
LE_FN float lm_mul_f(float a, float b) { volatile float p = a * b; return p; }
LE_FN double lm_add_d(double a, double b) { volatile double s = a + b; return s; }
LE_FN double lm_mul_d(double a, double b) { volatile double p = a * b; return p; }
#endif

// samples of a merged event whose lengths sum to `sum` seconds: ceil(sum * 4000), 0 where that is not a finite number > 0, LE_SAT
// from 2^31 on
LE_FN int64_t lm_count_f(float sum) {
    const float p = lm_mul_f(sum, (float)LM_FREQUENCY);
    if (!(p > 0.0f) || !(p <= FLT_MAX)) return 0;
    const float c = ceilf(p);
    return c >= 2147483648.0f ? LE_SAT : (int64_t)c;
}
LE_FN int64_t lm_count_d(double sum) {
    const double p = lm_mul_d(sum, (double)LM_FREQUENCY);
    if (!(p > 0.0) || !(p <= DBL_MAX)) return 0;
    const double c = ceil(p);
    return c >= 2147483648.0 ? LE_SAT : (int64_t)c;
}

// ---------------------------------------------------------------------------------------------------------------- the merge kernel
// event e of a read of n events (relative to the read) begins a merged event
LE_FN bool lm_is_head(const int32_t* moves_r, int64_t e, int64_t n) { return e >= 0 && e < n && (e == 0 || moves_r[e] != 0); }
// one past the last stay behind head h: the next head, or n.  Walks the read's own events only.
LE_FN int64_t lm_stays_end(const int32_t* moves_r, int64_t h, int64_t n) {
    if (h < 0 || h >= n) return h;
    int64_t e = h + 1;
    while (e < n && moves_r[e] == 0) ++e;
    return e;
}
// the samples of the merged event with head h and stays up to `end`: the sum goes left to right from the head, and the read's first
// merged event counts length[0] twice (the reference starts its running length at length[0] and adds length[0] again)
LE_FN int64_t lm_merged_count_f(const float* lengths_r, int64_t h, int64_t end) {
    float sum = lengths_r[h];
    if (h == 0) sum = lm_add_f(sum, lengths_r[0]);
    for (int64_t e = h + 1; e < end; ++e) sum = lm_add_f(sum, lengths_r[e]);
    return lm_count_f(sum);
}
LE_FN int64_t lm_merged_count_d(const double* lengths_r, int64_t h, int64_t end) {
    double sum = lengths_r[h];
    if (h == 0) sum = lm_add_d(sum, lengths_r[0]);
    for (int64_t e = h + 1; e < end; ++e) sum = lm_add_d(sum, lengths_r[e]);
    return lm_count_d(sum);
}
// the k bytes at `state` are one byte that is not 'N'
LE_FN uint8_t lm_uniform(const uint8_t* state, int32_t k) {
    const uint8_t b = state[0];
    if (b == (uint8_t)'N') return 0;
    for (int32_t q = 1; q < k; ++q)
        if (state[q] != b) return 0;
    return 1;
}
// slot of merged event j of a read of n events in the read's part of the compacted tables, or -1
LE_FN int64_t lm_merged_slot(int64_t j, int64_t n) { return (j < 0 || j >= n) ? -1 : j; }

// -------------------------------------------------------------------------------------------------------------- the classes kernel
// how many of the read's n slots hold a merged event: the count the merge kernel wrote, made to fit
LE_FN int64_t lm_merged_sound(int32_t m, int64_t n) { return m < 0 ? 0 : (m > n ? n : (int64_t)m); }
// LDS slot of merged event j among the core flags of the piece that begins at p0 (the piece and LM_WIDEN each side), or -1
LE_FN int32_t lm_core_slot(int64_t j, int64_t p0, int64_t m) {
    if (j < 0 || j >= m) return -1;
    const int64_t slot = j - p0 + LM_WIDEN;
    return (slot < 0 || slot >= LM_CORE_SLOTS) ? -1 : (int32_t)slot;
}
// core[j]: merged event j is outside the clipped ends and its k-mer is uniform
LE_FN uint8_t lm_core(const uint8_t* uniform_r, int64_t j, int64_t m, int64_t cs, int64_t ce) {
    if (j < 0 || j >= m || j < cs || j >= m - ce) return 0;
    return uniform_r[j] ? 1 : 0;
}
// cls[j]: some core within LM_WIDEN merged events of j, inside the read.  `cores` are the piece's LM_CORE_SLOTS flags.
LE_FN uint8_t lm_class(const uint8_t* cores, int64_t j, int64_t p0, int64_t m) {
    uint8_t any = 0;
    if (j < 0 || j >= m) return 0;
    for (int32_t d = -LM_WIDEN; d <= LM_WIDEN; ++d) {
        const int32_t slot = lm_core_slot(j + d, p0, m);
        if (slot >= 0) any |= cores[slot];
    }
    return any;
}
// the labels the read yields: the samples its merged events cover, cut at its raw signal
LE_FN int32_t lm_final(int64_t covered, int64_t n_raw) {
    const int64_t c = le_sat(covered < 0 ? 0 : covered);
    return (int32_t)(n_raw < 0 ? 0 : (n_raw < c ? n_raw : c));
}
