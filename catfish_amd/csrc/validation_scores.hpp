// Scores under runs: per threshold, kind and state of a run (check_hp: complete / incomplete / absent) the histogram of the
// probabilities of the samples under those runs and their fixed-point sum -- how close the missed homopolymers were to the
// threshold, how confident the calls that hold none (the reference's offline networks/process_output.py:15-137 check_for_false_neg
// and :276-357 collect the same scores run by run).  catfish_amd/device_validation.py states the result in numpy -- run_scores_host
// is normative; integers only, so the table equals it bit for bit on every run and for every grid.  The per-word and per-sample rules
// are plain C++ in validation_scores_word.hpp, the walk is validation_walk.hpp (read those first); tests/native/
// validation_scores_replay.cpp states both kernels' bodies serially over them under the sanitizers.
//
// A sample's row depends on its whole run, so after the label passes (validation_label_passes) there are two launches:
//
//   paint  a workgroup walks its stretch twice.  Mirrored first: every word learns what its last run holds AFTER the word
//          (vs_after of the walk's `in`) and leaves those six bits in the byte of its first sample -- the per-word scratch, inside
//          the paint itself.  Forward second: with the `in` seg of what lies before and that byte a lane paints its word (vs_word),
//          the piece's masks go through LDS, and the workgroup writes one byte per sample (vs_byte's layout), 64 consecutive bytes per wave
//          and store.  Every sample of the stretch is written, so no scratch byte survives.
//   bin    one thread per sample over chunks of CF_SCORE_CHUNK, blockIdx.z over the thresholds: up to two keys per sample (vs_key),
//          combined by validation_curve.hpp's sort and count of equal runs -- the global atomics a workgroup issues number the
//          distinct cells of its chunk, whatever the data -- and the six fixed-point sums of the chunk, reduced over the wave by
//          shuffles and over the waves in LDS, with one atomic per non-zero row.
//
// `work` holds the labels [K][stride] and behind them the paint [K][stride], stride = total rounded up to 64.
#pragma once
#include "validation_scores_word.hpp"
#include "validation_walk.hpp"

struct cf_scores_step : vs_rule {
    uint8_t* paint;                                        // the stretch's first paint byte
    int64_t n, n_words;                                    // samples that may be written (inside the stretch and the buffer); words walked
    unsigned long long (*s_paint)[4];                      // per word of the piece: kind 0 low / high bit of the code, kind 1 low / high
    bool mirror;
    int64_t first;                                         // position of my word's bit 0, in walking order
    unsigned after;                                        // mirrored walk: vs_after of kind 0 | kind 1 << 3
    vs_paint mine[2];
    __device__ static vr_seg shfl_up(const vr_seg v, int d) { return {(uint32_t)__shfl_up((int)v.len, d), (uint32_t)__shfl_up((int)v.flags, d)}; }
    __device__ unsigned byte(int64_t) const { return 0u; }
    __device__ void count(int q, uint64_t run, uint64_t is1, uint64_t is0, const marks&, const vr_seg in, int64_t at, bool) {
        first = at;
        if (mirror) {
            after = (q == 0 ? 0u : after) | (vs_after(in) << (3 * q));
        } else {
            if (q == 0) after = at < n ? paint[at] : 0u;   // (the mirrored walk's last barrier is behind that store)
            mine[q] = vs_word(run, is1, is0, in, (after >> (3 * q)) & 7u);
        }
    }
    __device__ void piece_counts() {
        if (mirror) {
            const int64_t walked = first >> 6, at = (n_words - 1 - walked) * 64;
            if (walked < n_words && at < n) paint[at] = (uint8_t)after;
        } else {
            unsigned long long(&row)[4] = s_paint[threadIdx.x];
            row[0] = mine[0].c | mine[0].a;
            row[1] = mine[0].i | mine[0].a;
            row[2] = mine[1].c | mine[1].a;
            row[3] = mine[1].i | mine[1].a;
        }
    }
    __device__ void piece_totals() {                       // (behind barrier (B): the piece's masks are in LDS, its scratch bytes are read)
        if (mirror) return;
        const int64_t base = first - (int64_t)threadIdx.x * 64;                   // the piece's first sample
        const unsigned bit = threadIdx.x & 63u;
#pragma unroll 4
        for (int it = 0; it < 64; ++it) {
            const int64_t i = base + (int64_t)it * CF_RUN_THREADS + threadIdx.x;
            if (i - threadIdx.x >= n) break;                                       // (uniform)
            const unsigned long long(&row)[4] = s_paint[it * CF_RUN_WAVES + (threadIdx.x >> 6)];
            if (i < n)
                paint[i] = (uint8_t)(((row[0] >> bit) & 1ull) | (((row[1] >> bit) & 1ull) << 1) | (((row[2] >> bit) & 1ull) << 2) |
                                     (((row[3] >> bit) & 1ull) << 3));
        }
    }
};

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_scores_paint_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                                 const uint8_t* __restrict__ y, const int64_t* __restrict__ bounds,
                                                                                 const int64_t* __restrict__ length, int64_t n_reads, int64_t total,
                                                                                 int K, uint8_t* paint) {
    __shared__ vr_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned long long s_paint[CF_RUN_THREADS][4];
    cf_walk_stretches(pred, pred_stride, bounds, length, n_reads, K, [&](int k, int64_t, const uint8_t* __restrict__ p, int64_t b0, int64_t n) {
        const int64_t room = b0 < 0 || b0 >= total ? 0 : total - b0;              // a table that disagrees with the buffers writes nothing
        cf_scores_step step = {{}, paint + (int64_t)k * pred_stride + b0, n < room ? n : room, (n >> 6) + 1, s_paint, true, 0, 0u, {}};
        cf_walk<cf_scores_step, true>(step, p, y, b0, n, total, s_seg);
        step.mirror = false;
        cf_walk<cf_scores_step, false>(step, p, y, b0, n, total, s_seg);
    });
}

#define CF_SCORES_KEYS (2 * CF_SCORE_CHUNK)

__global__ __launch_bounds__(CF_CURVE_THREADS) void validation_scores_bin_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ paint,
                                                                                 int64_t paint_stride, const int64_t* __restrict__ bounds,
                                                                                 const int64_t* __restrict__ length, int64_t total, int K, int shift,
                                                                                 unsigned cells, unsigned long long* __restrict__ table) {
    __shared__ uint32_t s_key[CF_SCORES_KEYS];
    __shared__ unsigned long long s_sum[VS_ROWS];
    const int64_t r = blockIdx.x;
    const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
    const int64_t n = length[r] < size ? length[r] : size;                         // the zero tail is not part of the stretch
    const int64_t n_chunks = n > 0 ? (n + CF_SCORE_CHUNK - 1) / CF_SCORE_CHUNK : 0;
    const uint32_t bins = vc_bins(shift);
    for (int k = blockIdx.z; k < K; k += gridDim.z) {                              // (uniform)
        const uint8_t* __restrict__ paint_k = paint + (int64_t)k * paint_stride;
        for (int64_t c = blockIdx.y; c < n_chunks; c += gridDim.y) {               // (uniform)
            const int64_t first = c * CF_SCORE_CHUNK;
            const unsigned m = (unsigned)(n - first < CF_SCORE_CHUNK ? n - first : CF_SCORE_CHUNK);  // samples of this chunk, >= 1
            unsigned span = 2;                                                     // power of two in [2, CF_SCORES_KEYS] that holds 2 m keys
            while (span < 2u * m) span <<= 1;
            if (threadIdx.x < VS_ROWS) s_sum[threadIdx.x] = 0ull;
            unsigned long long sum[VS_ROWS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
            for (unsigned i = threadIdx.x; 2u * i < span; i += CF_CURVE_THREADS) {
                uint32_t key[2] = {VS_NO_KEY, VS_NO_KEY};
                const int64_t at = first + i;
                if (i < m && (uint64_t)(b0 + at) < (uint64_t)total) {
                    const float p = probs[b0 + at];
                    const unsigned byte = paint_k[b0 + at];
                    const uint32_t bin = vc_bin(__float_as_uint(p), shift);
                    const unsigned long long q = bv_q(p);
#pragma unroll
                    for (int kind = 0; kind < 2; ++kind) {
                        const int row = vs_row(byte, kind);
                        if (row >= 0) key[kind] = vs_key(k, row, bin, shift);
#pragma unroll
                        for (int st = 0; st < 3; ++st) sum[kind * 3 + st] += row == kind * 3 + st ? q : 0ull;      // (registers, no indexed array)
                    }
                }
                s_key[2u * i] = key[0];
                s_key[2u * i + 1u] = key[1];
            }
            __syncthreads();
#pragma unroll
            for (int row = 0; row < VS_ROWS; ++row) {
                const unsigned long long all = cf_run_wave_sum(sum[row]);
                if ((threadIdx.x & 63u) == 0u && all != 0ull) atomicAdd(&s_sum[row], all);
            }
            vc_sort_count(s_key, span, cells, table);
            __syncthreads();                                                       // behind every LDS add; s_key is written again by the next chunk
            if (threadIdx.x < VS_ROWS && s_sum[threadIdx.x] != 0ull) atomicAdd(&table[vs_key(k, (int)threadIdx.x, bins, shift)], s_sum[threadIdx.x]);
            __syncthreads();                                                       // s_sum is zeroed again by the next chunk
        }
    }
}

// bytes of `work` for one call: per threshold the corrected labels and the paint, each array starting on a 64-byte multiple
extern "C" int64_t cf_validation_run_scores_work_bytes(int64_t total, int32_t n_thresholds) {
    if (total < 0 || n_thresholds < 0) return -1;
    return 2 * cf_validation_run_work_bytes(total, n_thresholds);
}

extern "C" int cf_validation_run_scores(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                        int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                        int32_t shift, int32_t max_gap, int32_t min_run, int64_t* table_out, int64_t table_capacity, void* work,
                                        int64_t work_bytes, void* stream) {
    const std::string fn = "cf_validation_run_scores";
    const validation_run_args a = {m, probs, y, bounds, length, n, total, longest, thresholds, n_thresholds, max_gap, min_run, table_out, work,
                                   work_bytes, stream};
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_scores_work_bytes", a)) return rc;
    if (!vs_shift_ok(shift))
        return fail(CF_ERR_INVALID, fn + ": shift must be in " + std::to_string(VS_SHIFT_MIN) + " .. " + std::to_string(VS_SHIFT_MAX));
    const int64_t per_k = (int64_t)VS_ROWS * vs_row_cells(shift), cells = (int64_t)n_thresholds * per_k;
    if (table_capacity < cells)
        return fail(CF_ERR_INVALID, fn + ": table_out needs n_thresholds * 6 * ((0x3F800000 >> shift) + 2) = " + std::to_string(cells) + " entries");
    const int64_t need = cf_validation_run_scores_work_bytes(total, n_thresholds);
    if (work_bytes < need)
        return fail(CF_ERR_INVALID, fn + ": work needs cf_validation_run_scores_work_bytes(total, n_thresholds) = " + std::to_string(need) + " bytes");
    return validation_run_step(a, per_k, [&](dim3 grid, hipStream_t s, const uint8_t* lab, int64_t stride, unsigned long long* table) {
        uint8_t* paint = static_cast<uint8_t*>(work) + (int64_t)n_thresholds * stride;
        hipLaunchKernelGGL(validation_scores_paint_kernel, grid, dim3(CF_RUN_THREADS), 0, s, lab, stride, y, bounds, length, n, total,
                           (int)n_thresholds, paint);
        hipLaunchKernelGGL(validation_scores_bin_kernel, dim3((unsigned)n, validation_grid_height(longest, CF_SCORE_CHUNK), (unsigned)n_thresholds),
                           dim3(CF_CURVE_THREADS), 0, s, probs, paint, stride, bounds, length, total, (int)n_thresholds, (int)shift, (unsigned)cells,
                           table);
    });
}
