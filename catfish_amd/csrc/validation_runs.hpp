// Event-level validation: how many true homopolymers a round found completely, partly or not at all, and how many called
// stretches hold none (the reference's offline networks/process_output.py:235-273: hp_loc_dict cuts truth and corrected prediction
// into runs, check_hp gives every run a state against the other array).  catfish_amd/device_validation.py states the result in
// numpy -- run_states_host is normative; integer counts only, so the kernel equals it bit for bit.  The per-word rules are plain
// C++ in validation_runs_word.hpp, the walk that feeds them is validation_walk.hpp (read those first); tests/native/
// validation_runs_replay.cpp states this kernel's body serially over them under the sanitizers.
//
// Counts: a lane packs (bin, state) counts of a piece into 8-bit fields (<= 33 per word), widens them to 16 bits for the wave
// butterfly (<= 64 * 33), lane 0 spreads them into the wave's LDS row, the first CF_RUN_CELLS threads add the rows into a
// register that lives for the whole stretch and add it to the zeroed table with ONE integer atomic per non-zero cell.
//
// This file also holds what the three run steps share on the host: the label passes, the argument checks and the launch path.
// (CF_RUN_THREADS, CF_RUN_WAVES and CF_RUN_PIECE, once defined here, are the walk's and live in validation_walk.hpp; the edges and
// bins are the rule's, in validation_runs_word.hpp.)
#pragma once
#include "validation_runs_word.hpp"
#include "validation_walk.hpp"

#define CF_RUN_CELLS (2 * CF_RUN_BINS * 3)            // [kind][bin][state]

__device__ __forceinline__ unsigned long long cf_run_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}

struct cf_states_step : vr_rule {
    unsigned (*s_cnt)[CF_RUN_CELLS];                       // one LDS row per wave
    unsigned long long acc[2][3];                          // [kind][state]: 8 bins x 8 bits, the piece's counts of this lane
    unsigned mine;                                         // threads < CF_RUN_CELLS: the stretch's count of one cell
    __device__ static vr_seg shfl_up(const vr_seg v, int d) { return {(uint32_t)__shfl_up((int)v.len, d), (uint32_t)__shfl_up((int)v.flags, d)}; }
    __device__ unsigned byte(int64_t) const { return 0u; }
    __device__ void count(int q, uint64_t run, uint64_t is1, uint64_t is0, const marks&, const vr_seg in, int64_t, bool) {
        unsigned long long(&a)[3] = acc[q];                // (q is a constant once unrolled: registers, no indexed array)
        vr_count(run, is1, is0, in, edges, [&a](unsigned bin, bool all1, bool all0) {
            const unsigned long long one = 1ull << (8u * bin);
            a[0] += all1 ? one : 0ull;                     // complete
            a[1] += (!all1 && !all0) ? one : 0ull;         // incomplete
            a[2] += (!all1 && all0) ? one : 0ull;          // absent
        });
    }
    __device__ void piece_counts() {                       // 8-bit fields -> 16-bit fields -> wave sum -> the wave's LDS row
        const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                const unsigned long long even = cf_run_wave_sum(acc[q][st] & 0x00ff00ff00ff00ffull);
                const unsigned long long odd = cf_run_wave_sum((acc[q][st] >> 8) & 0x00ff00ff00ff00ffull);
                acc[q][st] = 0ull;
                if (lane == 0u) {
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        s_cnt[wave][(q * CF_RUN_BINS + 2 * f) * 3 + st] = (unsigned)(even >> (16 * f)) & 0xffffu;
                        s_cnt[wave][(q * CF_RUN_BINS + 2 * f + 1) * 3 + st] = (unsigned)(odd >> (16 * f)) & 0xffffu;
                    }
                }
            }
        }
    }
    __device__ void piece_totals() {
        if (threadIdx.x < CF_RUN_CELLS) {
#pragma unroll
            for (int v = 0; v < CF_RUN_WAVES; ++v) mine += s_cnt[v][threadIdx.x];
        }
    }
};

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_run_states_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                               const uint8_t* __restrict__ y, const int64_t* __restrict__ bounds,
                                                                               const int64_t* __restrict__ length, int64_t n_reads, int64_t total,
                                                                               int K, cf_run_edges edges, int n_bins,
                                                                               unsigned long long* __restrict__ counts_out) {
    __shared__ vr_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned s_cnt[CF_RUN_WAVES][CF_RUN_CELLS];
    cf_walk_stretches(pred, pred_stride, bounds, length, n_reads, K, [&](int k, int64_t, const uint8_t* __restrict__ p, int64_t b0, int64_t n) {
        cf_states_step step = {{edges}, s_cnt, {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}}, 0u};
        cf_walk<cf_states_step, false>(step, p, y, b0, n, total, s_seg);
        if (threadIdx.x < CF_RUN_CELLS && step.mine != 0u) {
            const int q = threadIdx.x / (CF_RUN_BINS * 3), bin = (threadIdx.x / 3) % CF_RUN_BINS, st = threadIdx.x % 3;
            if (bin < n_bins) atomicAdd(&counts_out[(((int64_t)k * 2 + q) * n_bins + bin) * 3 + st], (unsigned long long)step.mine);
        }
        __syncthreads();                                   // the next stretch's first piece writes s_seg and, later, s_cnt
    });
}

extern "C" int cf_validation_run_piece(void) { return CF_RUN_PIECE; }

// bytes of `work` for one call: one label array per threshold, each starting on a 64-byte multiple
extern "C" int64_t cf_validation_run_work_bytes(int64_t total, int32_t n_thresholds) {
    if (total < 0 || n_thresholds < 0) return -1;
    return (int64_t)n_thresholds * ((total + 63) / 64 * 64);
}

// what a bridged label pass needs: the bit-mask kernel's domain and a work buffer it can store 16 bytes at a time into
static bool validation_bridge_ok(int32_t min_run, int32_t max_gap, const void* work) {
    return max_gap == 0 || (pb_domain(min_run, max_gap) && (reinterpret_cast<uintptr_t>(work) & 15u) == 0);
}

// The corrected labels of the whole packed batch, one array per threshold at lab + k * stride (threshold + correct_short inside every
// stretch): what the run steps count on.
// max_gap > 0: gaps of at most max_gap samples inside a stretch are bridged first (postprocess_bridged_kernel; the callers have checked
// validation_bridge_ok).
static int validation_label_passes(const float* probs, const int64_t* bounds, const int64_t* length, int64_t n, int64_t total,
                                   const double* thresholds, int32_t n_thresholds, int32_t max_gap, int32_t min_run, uint8_t* lab,
                                   int64_t stride, hipStream_t s) {
    // the bit-mask kernel covers runs of up to 64 samples and stores labels 16 bytes at a time (cf_postprocess's rule)
    const bool bits = min_run <= 64 && (reinterpret_cast<uintptr_t>(lab) & 15u) == 0;
    for (int k = 0; k < n_thresholds; ++k) {
        // (double)p >= t  <=>  p >= tf with tf the smallest float not below t
        float tf = (float)thresholds[k];
        if ((double)tf < thresholds[k]) tf = std::nextafterf(tf, INFINITY);
        if (max_gap > 0) {
            hipLaunchKernelGGL(postprocess_bridged_kernel<false>, post_bits_grid(total), dim3(256), 0, s, probs, bounds, length,
                               n, total, tf, (int)max_gap, (int)min_run, lab + k * stride, (int64_t)0, (int64_t*)nullptr, (int64_t*)nullptr,
                               (unsigned long long*)nullptr);
        } else if (bits) {
            hipLaunchKernelGGL(postprocess_bits_kernel<false>, post_bits_grid(total), dim3(256), 0, s, probs, bounds, length, n,
                               total, tf, (int)min_run, lab + k * stride, (int64_t)0, (int64_t*)nullptr, (int64_t*)nullptr,
                               (unsigned long long*)nullptr);
        } else {
            hipLaunchKernelGGL(postprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, probs, bounds, length, n, total, tf,
                               (int)min_run, lab + k * stride);
        }
        HIP_TRY(hipGetLastError());
    }
    return CF_OK;
}

// What the entry points of the three run steps take in common.
struct validation_run_args {
    cf_model* m;
    const float* probs;
    const uint8_t* y;
    const int64_t *bounds, *length;
    int64_t n, total, longest;
    const double* thresholds;
    int32_t n_thresholds, max_gap, min_run;
    int64_t* counts_out;
    void* work;
    int64_t work_bytes;
    void* stream;
};

// The argument checks the run steps share (each keeps the ones of its own table); `work_fn` is the function the message about too
// small a work buffer names (the steps have one rule: cf_validation_run_work_bytes).
static int validation_run_args_ok(const std::string& fn, const char* work_fn, const validation_run_args& a) {
    if (!a.probs || !a.y || !a.bounds || !a.length || !a.thresholds || !a.counts_out || !a.work) return fail(CF_ERR_INVALID, fn + ": null argument");
    if (a.n <= 0 || a.n > 0x7fffffff) return fail(CF_ERR_INVALID, fn + ": n must be in [1, 2^31)");
    if (a.n_thresholds < 1 || a.n_thresholds > CF_SCORE_MAX_K)
        return fail(CF_ERR_INVALID, fn + ": between 1 and " + std::to_string(CF_SCORE_MAX_K) + " thresholds per call");
    if (a.total < 0 || a.total > 0x7fffffff || a.longest < 0 || a.longest > a.total) return fail(CF_ERR_INVALID, fn + ": bad size");
    if (a.min_run < 1) return fail(CF_ERR_INVALID, fn + ": min_run must be >= 1");
    if (!validation_bridge_ok(a.min_run, a.max_gap, a.work))
        return fail(CF_ERR_INVALID, fn + ": bridging needs max_gap >= 0, min_run + max_gap <= 64 and a 16-byte aligned work buffer");
    if (a.work_bytes < cf_validation_run_work_bytes(a.total, a.n_thresholds))
        return fail(CF_ERR_INVALID, fn + ": work needs " + work_fn + "(total, n_thresholds) bytes");
    return CF_OK;
}

// The launch path of a run step, behind its argument checks: the table of `cells` per threshold zeroed, the label passes, then
// launch(grid, stream, labels, stride between the thresholds' labels, table) starts the step's kernel.
template <class Launch>
static int validation_run_step(const validation_run_args& a, int64_t cells, Launch&& launch) {
    const int64_t stride = (a.total + 63) / 64 * 64;
    if (a.m) HIP_TRY(hipSetDevice(a.m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
    HIP_TRY(hipMemsetAsync(a.counts_out, 0, (size_t)a.n_thresholds * cells * sizeof(int64_t), s));
    if (a.total == 0) return CF_OK;                            // stretches without a sample: the zeroed table
    uint8_t* lab = static_cast<uint8_t*>(a.work);
    if (const int rc = validation_label_passes(a.probs, a.bounds, a.length, a.n, a.total, a.thresholds, a.n_thresholds, a.max_gap, a.min_run,
                                               lab, stride, s)) return rc;
    launch(dim3((unsigned)std::min<int64_t>(a.n, 1 << 20), (unsigned)a.n_thresholds), s, lab, stride, reinterpret_cast<unsigned long long*>(a.counts_out));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

static int validation_run_states_impl(const std::string& fn, const validation_run_args& a, const int64_t* edges, int32_t n_edges) {
    if (n_edges > 0 && !edges) return fail(CF_ERR_INVALID, fn + ": null argument");
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_work_bytes", a)) return rc;
    if (n_edges < 0 || n_edges > CF_RUN_MAX_EDGES)
        return fail(CF_ERR_INVALID, fn + ": at most " + std::to_string(CF_RUN_MAX_EDGES) + " edges");
    cf_run_edges e;
    for (int j = 0; j < CF_RUN_MAX_EDGES; ++j) e.e[j] = 0xffffffffu;
    for (int j = 0; j < n_edges; ++j) {
        if (edges[j] < 1 || (j > 0 && edges[j] <= edges[j - 1]))
            return fail(CF_ERR_INVALID, fn + ": edges must be positive and ascending");
        e.e[j] = (unsigned)std::min<int64_t>(edges[j], 0xffffffffll);
    }
    const int n_bins = n_edges + 1;
    return validation_run_step(a, 2 * n_bins * 3, [&](dim3 grid, hipStream_t s, const uint8_t* lab, int64_t stride, unsigned long long* table) {
        hipLaunchKernelGGL(validation_run_states_kernel, grid, dim3(CF_RUN_THREADS), 0, s, lab, stride, a.y, a.bounds, a.length, a.n, a.total,
                           (int)a.n_thresholds, e, n_bins, table);
    });
}

extern "C" int cf_validation_run_states(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                        int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                        const int64_t* edges, int32_t n_edges, int32_t min_run, int64_t* counts_out, void* work,
                                        int64_t work_bytes, void* stream) {
    return validation_run_states_impl("cf_validation_run_states", {m, probs, y, bounds, length, n, total, longest, thresholds, n_thresholds, 0,
                                                                   min_run, counts_out, work, work_bytes, stream}, edges, n_edges);
}

// ... with gaps of at most max_gap samples bridged in every stretch before correct_short (device_validation.run_states_host(max_gap=))
extern "C" int cf_validation_run_states_bridged(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds,
                                                const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                                int32_t n_thresholds, const int64_t* edges, int32_t n_edges, int32_t max_gap,
                                                int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    return validation_run_states_impl("cf_validation_run_states_bridged", {m, probs, y, bounds, length, n, total, longest, thresholds,
                                                                           n_thresholds, max_gap, min_run, counts_out, work, work_bytes, stream},
                                      edges, n_edges);
}
