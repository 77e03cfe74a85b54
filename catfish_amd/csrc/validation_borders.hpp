// The rest of check_hp on the card (the reference's networks/process_output.py:814-895): by how many samples the other array
// reaches beyond a run's left and right border or falls short of it, and the interruptions inside the run -- histograms per
// threshold and kind.  catfish_amd/device_validation.py states the result in numpy -- run_borders_host is normative; integer
// counts only, so the kernel equals it bit for bit.  The per-word rules are plain C++ in validation_borders_word.hpp, the walk that
// feeds them is validation_walk.hpp (read those first); tests/native/validation_borders_replay.cpp states this kernel's body
// serially over them under the sanitizers.
//
// A workgroup walks its stretch twice: forward (left offsets, interruptions, interrupted runs) and mirrored for the right offsets.
// Counts collect in the workgroup's LDS table (cf_walk_table: 2 * (5 reach + 3) cells).
#pragma once
#include "validation_walk.hpp"

#define CF_BORDER_MAX_CELLS (2 * (5 * VB_MAX_REACH + 3))

struct cf_borders_step : vb_rule, cf_walk_table {
    __device__ static vb_seg shfl_up(const vb_seg v, int d) {
        return {(uint32_t)__shfl_up((int)v.run_len, d), (uint32_t)__shfl_up((int)v.o_cnt, d), (uint32_t)__shfl_up((int)v.flags, d)};
    }
    __device__ unsigned byte(int64_t) const { return 0u; }
    __device__ void count(int q, uint64_t run, uint64_t is1, uint64_t is0, const marks& mk, const vb_seg in, int64_t first, bool mirror) const {
        events(run, is1, is0, mk, in, first, mirror, [this, q](int cell) { add(q, cell); });
    }
};

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_run_borders_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                                const uint8_t* __restrict__ y, const int64_t* __restrict__ bounds,
                                                                                const int64_t* __restrict__ length, int64_t n_reads, int64_t total,
                                                                                int K, int reach, unsigned long long* __restrict__ counts_out) {
    __shared__ vb_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned s_tab[CF_BORDER_MAX_CELLS];
    cf_borders_step step = {{reach}, {s_tab, vb_cells(reach)}};
    step.zero();
    cf_walk_stretches(pred, pred_stride, bounds, length, n_reads, K, [&](int k, int64_t, const uint8_t* __restrict__ p, int64_t b0, int64_t n) {
        cf_walk<cf_borders_step, false>(step, p, y, b0, n, total, s_seg);
        cf_walk<cf_borders_step, true>(step, p, y, b0, n, total, s_seg);
        step.flush(counts_out + (int64_t)k * 2 * step.cells);
    });
}

// bytes of `work` for one call: cf_validation_run_work_bytes' rule (one label array per threshold, each on a 64-byte multiple)
extern "C" int64_t cf_validation_run_borders_work_bytes(int64_t total, int32_t n_thresholds) {
    return cf_validation_run_work_bytes(total, n_thresholds);
}

static int validation_run_borders_impl(const std::string& fn, const validation_run_args& a, int32_t reach) {
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_borders_work_bytes", a)) return rc;
    if (reach < 1 || reach > VB_MAX_REACH)
        return fail(CF_ERR_INVALID, fn + ": reach must be in 1 .. " + std::to_string(VB_MAX_REACH));
    return validation_run_step(a, 2 * vb_cells(reach), [&](dim3 grid, hipStream_t s, const uint8_t* lab, int64_t stride, unsigned long long* table) {
        hipLaunchKernelGGL(validation_run_borders_kernel, grid, dim3(CF_RUN_THREADS), 0, s, lab, stride, a.y, a.bounds, a.length, a.n, a.total,
                           (int)a.n_thresholds, (int)reach, table);
    });
}

extern "C" int cf_validation_run_borders(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                         int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                         int32_t reach, int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    return validation_run_borders_impl("cf_validation_run_borders", {m, probs, y, bounds, length, n, total, longest, thresholds, n_thresholds, 0,
                                                                     min_run, counts_out, work, work_bytes, stream}, reach);
}

// ... with gaps of at most max_gap samples bridged in every stretch before correct_short (device_validation.run_borders_host(max_gap=))
extern "C" int cf_validation_run_borders_bridged(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds,
                                                 const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                                 int32_t n_thresholds, int32_t reach, int32_t max_gap, int32_t min_run, int64_t* counts_out,
                                                 void* work, int64_t work_bytes, void* stream) {
    return validation_run_borders_impl("cf_validation_run_borders_bridged", {m, probs, y, bounds, length, n, total, longest, thresholds,
                                                                             n_thresholds, max_gap, min_run, counts_out, work, work_bytes, stream},
                                       reach);
}
