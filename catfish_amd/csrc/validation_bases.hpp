// Which homopolymers a round found, by base and by length in BASES (the reference's offline networks/process_output.py:
// prediction_information -> base_count_dict / get_bases / get_prevalence over hp_loc_dict's runs and check_hp's states).  Per run
// the bases are the marked samples of the base map inside it -- cf_label_events marks the centre sample of every event, which is
// base_to_signal.get_base_new_signal's "n".  catfish_amd/device_validation.py states the result in numpy -- run_bases_host is
// normative; integer counts only, so the kernel equals it bit for bit.  The per-word rules are plain C++ in
// validation_bases_word.hpp, the walk that feeds them is validation_walk.hpp (read those first); tests/native/
// validation_bases_replay.cpp states this kernel's body serially over them under the sanitizers.
//
// The base map is read where the set keeps it, at basemap[src_first[r] + i]: no packed copy of it exists.  Its byte gives five more
// ballots per wave and word.  Counts collect in the workgroup's LDS table (cf_walk_table: 2 * 3 * 5 * (max_bases + 1) cells) at the
// falling edges.
#pragma once
#include "validation_bases_word.hpp"
#include "validation_walk.hpp"

#define CF_BASES_MAX_CELLS (2 * 3 * VBS_CLASSES * (VBS_MAX_BASES + 1))

struct cf_bases_step : vbs_rule, cf_walk_table {
    const uint8_t* __restrict__ basemap;
    int64_t basemap_total, src;                            // src: where the stretch starts in the base map
    __device__ static vbs_seg shfl_up(const vbs_seg v, int d) { return (vbs_seg)__shfl_up((int)v, d); }
    __device__ unsigned byte(int64_t i) const { return (uint64_t)(src + i) < (uint64_t)basemap_total ? basemap[src + i] : 0u; }
    __device__ void count(int q, uint64_t run, uint64_t is1, uint64_t is0, const marks& mk, const vbs_seg in, int64_t first, bool mirror) const {
        events(run, is1, is0, mk, in, first, mirror, [this, q](int cell) { add(q, cell); });
    }
};

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_run_bases_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                              const uint8_t* __restrict__ y, const uint8_t* __restrict__ basemap,
                                                                              int64_t basemap_total, const int64_t* __restrict__ src_first,
                                                                              const int64_t* __restrict__ bounds, const int64_t* __restrict__ length,
                                                                              int64_t n_reads, int64_t total, int K, int max_bases,
                                                                              unsigned long long* __restrict__ counts_out) {
    __shared__ vbs_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned s_tab[CF_BASES_MAX_CELLS];
    cf_bases_step step = {{max_bases}, {s_tab, vbs_cells(max_bases)}, basemap, basemap_total, 0};
    step.zero();
    cf_walk_stretches(pred, pred_stride, bounds, length, n_reads, K, [&](int k, int64_t r, const uint8_t* __restrict__ p, int64_t b0, int64_t n) {
        step.src = src_first[r];
        cf_walk<cf_bases_step, false>(step, p, y, b0, n, total, s_seg);
        step.flush(counts_out + (int64_t)k * 2 * step.cells);
    });
}

// Argument checks: validation_run_args_ok's, plus max_bases and the base map.  An exact check of the base map's size against the
// selection would need src_first on the host; the kernel checks every index against basemap_total instead (a sample past it has
// no mark), and DeviceValidationSet keeps the base map as long as its labels.
extern "C" int cf_validation_run_bases(cf_model* m, const float* probs, const uint8_t* y, const uint8_t* basemap, int64_t basemap_total,
                                       const int64_t* src_first, const int64_t* bounds, const int64_t* length, int64_t n, int64_t total,
                                       int64_t longest, const double* thresholds, int32_t n_thresholds, int32_t max_bases, int32_t max_gap,
                                       int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    const std::string fn = "cf_validation_run_bases";
    const validation_run_args a = {m, probs, y, bounds, length, n, total, longest, thresholds, n_thresholds, max_gap, min_run, counts_out, work,
                                   work_bytes, stream};
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_work_bytes", a)) return rc;
    if (!basemap || !src_first) return fail(CF_ERR_INVALID, fn + ": null argument");
    if (max_bases < 1 || max_bases > VBS_MAX_BASES)
        return fail(CF_ERR_INVALID, fn + ": max_bases must be in 1 .. " + std::to_string(VBS_MAX_BASES));
    if (basemap_total < 1 || basemap_total > 0x7fffffff) return fail(CF_ERR_INVALID, fn + ": basemap_total must be in [1, 2^31)");
    return validation_run_step(a, 2 * vbs_cells(max_bases), [&](dim3 grid, hipStream_t s, const uint8_t* lab, int64_t stride, unsigned long long* table) {
        hipLaunchKernelGGL(validation_run_bases_kernel, grid, dim3(CF_RUN_THREADS), 0, s, lab, stride, y, basemap, basemap_total, src_first, bounds,
                           length, n, total, (int)n_thresholds, (int)max_bases, table);
    });
}
