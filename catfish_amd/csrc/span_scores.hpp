// Per-call scores of homopolymer calls (cf_span_scores; catfish_amd/span_scores.py: span_scores_host is the definition).  For run k
// of the start list that cf_postprocess_spans wrote, row k receives the run's paired end, the sums of p, x and x * x over it
// (float64) and the smallest and largest p (float32): what says how sure a call was, at what current level the stretch sits and how
// flat it is -- from the probabilities and the normalised signal that are resident anyway.
//
// One wave per run, four waves per workgroup, grid-stride over min(counts[0], max_runs) -- the count is read on the card, the call
// stays asynchronous.  A step loads 64 consecutive probabilities (and signal samples), one per lane; a ballot of p >= threshold and
// the rule header (span_scores_rule.hpp) say how many leading lanes still belong to the run.  Those lanes accumulate in registers;
// at the run's end one butterfly of __shfl_xor in a fixed order reduces the wave, and lane 0 writes the row.  No LDS, no atomics; the
// order of every sum is a function of the run's position alone, so equal inputs give equal bits.
//
// The walk needs no min_run: the starts it is given are those of kept runs, and a kept run is the maximal streak from its start.
// Any other start (a caller's own list) is safe: one outside the real part of a read gets an empty row (end = start, zero sums,
// min = +inf, max = -inf) without a load; one inside a streak is walked from there to the streak's end.
#pragma once
#include "span_scores_rule.hpp"

#define CF_SCORE_WAVES 4           // waves (runs in flight) per workgroup
#define CF_SCORE_MAX_BLOCKS 2048   // grid-stride beyond: 8192 runs in flight fill the chip's wave slots

// LABELS (span_scores_labels_kernel, cf_span_scores_labels): "the run continues" is labels[i] != 0 instead of p >= threshold -- a run
// that cf_postprocess_spans_bridged reports holds samples below the threshold, and they count.  Everything else is the same code.
template <bool LABELS>
__device__ __forceinline__ void span_scores_body(
    const float* __restrict__ probs, const float* __restrict__ signal, const uint8_t* __restrict__ labels,
    const int64_t* __restrict__ read_offsets, const int64_t* __restrict__ read_lengths, int64_t n_reads, int64_t total, float threshold,
    const int64_t* __restrict__ starts, const unsigned long long* __restrict__ counts, int64_t max_runs, int64_t* __restrict__ ends_paired,
    double* __restrict__ sums, float* __restrict__ extremes) {
    const int lane = threadIdx.x & 63;
    const int64_t n_rows = ss_rows((uint64_t)counts[0], max_runs);
    const int64_t n_waves = (int64_t)gridDim.x * CF_SCORE_WAVES;
    for (int64_t k = (int64_t)blockIdx.x * CF_SCORE_WAVES + (threadIdx.x >> 6); k < n_rows; k += n_waves) {     // (whole wave: uniform)
        const int64_t start = starts[k];
        const ss_walk w = ss_open(read_offsets, read_lengths, n_reads, total, start);
        double sp = 0.0, sx = 0.0, sx2 = 0.0;
        float lo = __builtin_inff(), hi = -__builtin_inff();
        int64_t pos = start;
        bool go = w.open;
        while (go) {
            const int64_t left = w.end - pos;                               // > 0
            const bool in = lane < left;
            const int64_t i = pos + lane;                                   // in: start <= i < w.end <= total
            const float p = in ? probs[i] : 0.f;
            const float x = (in && signal != nullptr) ? signal[i] : 0.f;
            bool hit = in && p >= threshold;
            if constexpr (LABELS) hit = in && labels[i] != 0;
            const ss_taken t = ss_step(__ballot(hit), left);
            if (lane < t.take) {
                sp += (double)p;
                sx += (double)x;
                sx2 += (double)x * (double)x;
                lo = fminf(lo, p);
                hi = fmaxf(hi, p);
            }
            pos += t.take;
            go = t.go_on;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {                                 // the one order of every reduction
            sp += __shfl_xor(sp, d);
            sx += __shfl_xor(sx, d);
            sx2 += __shfl_xor(sx2, d);
            lo = fminf(lo, __shfl_xor(lo, d));
            hi = fmaxf(hi, __shfl_xor(hi, d));
        }
        if (lane == 0) {
            ends_paired[k] = pos;
            sums[ss_sum_index(k, 0)] = sp;
            if (signal != nullptr) {
                sums[ss_sum_index(k, 1)] = sx;
                sums[ss_sum_index(k, 2)] = sx2;
            }
            extremes[ss_extreme_index(k, 0)] = lo;
            extremes[ss_extreme_index(k, 1)] = hi;
        }
    }
}

__global__ __launch_bounds__(64 * CF_SCORE_WAVES) void span_scores_kernel(
    const float* __restrict__ probs, const float* __restrict__ signal, const int64_t* __restrict__ read_offsets,
    const int64_t* __restrict__ read_lengths, int64_t n_reads, int64_t total, float threshold, const int64_t* __restrict__ starts,
    const unsigned long long* __restrict__ counts, int64_t max_runs, int64_t* __restrict__ ends_paired, double* __restrict__ sums,
    float* __restrict__ extremes) {
    span_scores_body<false>(probs, signal, nullptr, read_offsets, read_lengths, n_reads, total, threshold, starts, counts, max_runs,
                            ends_paired, sums, extremes);
}

__global__ __launch_bounds__(64 * CF_SCORE_WAVES) void span_scores_labels_kernel(
    const float* __restrict__ probs, const float* __restrict__ signal, const uint8_t* __restrict__ labels,
    const int64_t* __restrict__ read_offsets, const int64_t* __restrict__ read_lengths, int64_t n_reads, int64_t total,
    const int64_t* __restrict__ starts, const unsigned long long* __restrict__ counts, int64_t max_runs, int64_t* __restrict__ ends_paired,
    double* __restrict__ sums, float* __restrict__ extremes) {
    span_scores_body<true>(probs, signal, labels, read_offsets, read_lengths, n_reads, total, 0.f, starts, counts, max_runs, ends_paired,
                           sums, extremes);
}
