// The rest of check_hp on the card (the reference's networks/process_output.py:814-895): by how many samples the other array
// reaches beyond a run's left and right border or falls short of it, and the interruptions inside the run -- histograms per
// threshold and kind.  catfish_amd/device_validation.py states the result in numpy -- run_borders_host is normative; integer
// counts only, so the kernel equals it bit for bit.  The per-word rules are plain C++ in validation_borders_word.hpp (read that
// first); tests/native/validation_borders_replay.cpp states this kernel's body serially over them under the sanitizers.
//
// Per threshold the post-processing kernel writes the corrected labels into its slice of `work` (validation_label_passes, the
// run-state step's own label passes); ONE launch of validation_run_borders_kernel then counts, blockIdx.x striding over the
// stretches and blockIdx.y over the thresholds.
//
// A workgroup walks its stretch twice in pieces of CF_RUN_PIECE samples, one 64-sample word per lane: forward (left offsets,
// interruptions, interrupted runs) and mirrored -- the last word first, every word bit-reversed, lanes and pieces in that order --
// for the right offsets; one routine serves both.  The masks are loaded as in validation_runs.hpp (64 coalesced byte loads +
// ballots per wave).  The vb_seg at the end of every word is an inclusive scan with vb_join: over the lanes of a wave by
// shuffles, over the four waves through LDS, from piece to piece in registers every thread keeps.  Inside a word a lane steps
// from edge to edge with bit operations (at most 32 of each kind); no lane walks the samples of a run.
//
// Counts collect in one LDS table per workgroup (2 * (5 reach + 3) cells) by integer LDS adds and go to the zeroed output with one
// 64-bit integer atomic per non-zero cell at the end of the stretch.  Equal inputs give equal bits whatever the grid.
#pragma once
#include "validation_borders_word.hpp"

#define CF_BORDER_MAX_CELLS (2 * (5 * VB_MAX_REACH + 3))

__device__ __forceinline__ vb_seg cf_border_shfl_up(const vb_seg v, int d) {
    return {(uint32_t)__shfl_up((int)v.run_len, d), (uint32_t)__shfl_up((int)v.o_cnt, d), (uint32_t)__shfl_up((int)v.flags, d)};
}

// One walk over the stretch [b0, b0 + n) of (threshold slice p, labels y): forward or mirrored.
template <bool MIRROR>
__device__ __forceinline__ void cf_border_walk(const uint8_t* __restrict__ p, const uint8_t* __restrict__ y, int64_t b0, int64_t n, int64_t total,
                                               int reach, vb_seg (&s_seg)[CF_RUN_WAVES][2], unsigned* s_tab) {
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t n_words = (n >> 6) + 1;                                          // the word that holds position n closes the last run
    const int cells = vb_cells(reach);
    vb_seg carry[2] = {vb_none(), vb_none()};
    for (int64_t w0 = 0; w0 < n_words; w0 += CF_RUN_THREADS) {
        // 1. masks: word j of this wave's 64 (in walking order) lands in lane j
        const int64_t wave_word = w0 + (int64_t)wave * 64;
        unsigned long long y1 = 0, p1 = 0;
        for (int j = 0; j < 64; ++j) {
            if (wave_word + j >= n_words) break;                                   // (uniform)
            const int64_t real = MIRROR ? n_words - 1 - (wave_word + j) : wave_word + j;
            const int64_t i = real * 64 + lane;
            unsigned yv = 0u, pv = 0u;
            if (i < n && (uint64_t)(b0 + i) < (uint64_t)total) {
                yv = y[b0 + i];
                pv = p[b0 + i];
            }
            const unsigned long long by1 = __ballot(yv == 1u), bp1 = __ballot(pv == 1u);
            if ((int)lane == j) { y1 = by1; p1 = bp1; }
        }
        unsigned long long run_y = y1, run_p = p1;
        const int64_t walked = wave_word + lane, word = MIRROR ? n_words - 1 - walked : walked;
        if (n >= 2 && word == ((n - 1) >> 6) && (uint64_t)(b0 + n - 2) < (uint64_t)total) {   // hp_loc_dict closes an open run AT the last sample
            const unsigned long long last = 1ull << ((n - 1) & 63);
            if (y[b0 + n - 2] == 1u) run_y |= last;
            if (p[b0 + n - 2] == 1u) run_p |= last;
        }
        if (MIRROR) {
            y1 = vb_reverse(y1); p1 = vb_reverse(p1); run_y = vb_reverse(run_y); run_p = vb_reverse(run_p);
        }
        // 2. the seg at the end of every word: inclusive scan over the wave, wave totals to LDS
        vb_seg inc[2] = {vb_word(run_y, p1), vb_word(run_p, y1)};
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const vb_seg o = cf_border_shfl_up(inc[q], d);
                if ((int)lane >= d) inc[q] = vb_join(o, inc[q]);
            }
        }
        if (lane == 63u) { s_seg[wave][0] = inc[0]; s_seg[wave][1] = inc[1]; }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            vb_seg in = carry[q];                                                  // at the end of the word before mine
#pragma unroll
            for (int v = 0; v < CF_RUN_WAVES; ++v) {
                const vb_seg t = s_seg[v][q];
                if (v < (int)wave) in = vb_join(in, t);
                carry[q] = vb_join(carry[q], t);                                   // (every thread: the piece's total)
            }
            const vb_seg left = cf_border_shfl_up(inc[q], 1);
            if (lane != 0u) in = vb_join(in, left);
            // 3. the events of my word (words past the stretch hold no bit: no event)
            unsigned* row = s_tab + q * cells;
            vb_events(q == 0 ? run_y : run_p, q == 0 ? p1 : y1, in, walked * 64, MIRROR, reach, [row](int cell) { atomicAdd(&row[cell], 1u); });
        }
        __syncthreads();                                                           // s_seg is written again by the next piece
    }
}

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_run_borders_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                                const uint8_t* __restrict__ y, const int64_t* __restrict__ bounds,
                                                                                const int64_t* __restrict__ length, int64_t n_reads, int64_t total,
                                                                                int K, int reach, unsigned long long* __restrict__ counts_out) {
    __shared__ vb_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned s_tab[CF_BORDER_MAX_CELLS];
    const int cells = 2 * vb_cells(reach);
    for (int c = threadIdx.x; c < cells; c += CF_RUN_THREADS) s_tab[c] = 0u;
    __syncthreads();
    for (int k = blockIdx.y; k < K; k += gridDim.y) {
        const uint8_t* __restrict__ p = pred + (int64_t)k * pred_stride;
        for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
            const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
            const int64_t n = length[r] < size ? length[r] : size;                 // the zero tail is not part of the stretch
            if (n <= 0) continue;                                                  // (uniform)
            cf_border_walk<false>(p, y, b0, n, total, reach, s_seg, s_tab);
            cf_border_walk<true>(p, y, b0, n, total, reach, s_seg, s_tab);
            // (the last barrier of the walk is behind every LDS add)
            for (int c = threadIdx.x; c < cells; c += CF_RUN_THREADS) {
                const unsigned v = s_tab[c];
                if (v != 0u) {
                    atomicAdd(&counts_out[(int64_t)k * cells + c], (unsigned long long)v);
                    s_tab[c] = 0u;
                }
            }
            __syncthreads();
        }
    }
}

// bytes of `work` for one call: cf_validation_run_work_bytes' rule (one label array per threshold, each on a 64-byte multiple)
extern "C" int64_t cf_validation_run_borders_work_bytes(int64_t total, int32_t n_thresholds) {
    return cf_validation_run_work_bytes(total, n_thresholds);
}

static int validation_run_borders_impl(const std::string& fn, cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds,
                                       const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                       int32_t n_thresholds, int32_t reach, int32_t max_gap, int32_t min_run, int64_t* counts_out, void* work,
                                       int64_t work_bytes, void* stream) {
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_borders_work_bytes", probs, y, bounds, length, n, total, longest,
                                              thresholds, n_thresholds, max_gap, min_run, counts_out, work, work_bytes)) return rc;
    if (reach < 1 || reach > VB_MAX_REACH)
        return fail(CF_ERR_INVALID, fn + ": reach must be in 1 .. " + std::to_string(VB_MAX_REACH));
    const int64_t stride = (total + 63) / 64 * 64;
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)n_thresholds * 2 * vb_cells(reach) * sizeof(int64_t), s));
    if (total == 0) return CF_OK;                              // stretches without a sample: the zeroed table
    uint8_t* lab = static_cast<uint8_t*>(work);
    if (const int rc = validation_label_passes(probs, bounds, length, n, total, thresholds, n_thresholds, max_gap, min_run, lab, stride, s)) return rc;
    hipLaunchKernelGGL(validation_run_borders_kernel, dim3((unsigned)std::min<int64_t>(n, 1 << 20), (unsigned)n_thresholds), dim3(CF_RUN_THREADS),
                       0, s, lab, stride, y, bounds, length, n, total, (int)n_thresholds, (int)reach,
                       reinterpret_cast<unsigned long long*>(counts_out));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_validation_run_borders(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                         int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                         int32_t reach, int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    return validation_run_borders_impl("cf_validation_run_borders", m, probs, y, bounds, length, n, total, longest, thresholds, n_thresholds,
                                       reach, 0, min_run, counts_out, work, work_bytes, stream);
}

// ... with gaps of at most max_gap samples bridged in every stretch before correct_short (device_validation.run_borders_host(max_gap=))
extern "C" int cf_validation_run_borders_bridged(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds,
                                                 const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                                 int32_t n_thresholds, int32_t reach, int32_t max_gap, int32_t min_run, int64_t* counts_out,
                                                 void* work, int64_t work_bytes, void* stream) {
    return validation_run_borders_impl("cf_validation_run_borders_bridged", m, probs, y, bounds, length, n, total, longest, thresholds,
                                       n_thresholds, reach, max_gap, min_run, counts_out, work, work_bytes, stream);
}
