// Which homopolymers a round found, by base and by length in BASES (the reference's offline networks/process_output.py:
// prediction_information -> base_count_dict / get_bases / get_prevalence over hp_loc_dict's runs and check_hp's states).  Per run
// the bases are the marked samples of the base map inside it -- cf_label_events marks the centre sample of every event, which is
// base_to_signal.get_base_new_signal's "n".  catfish_amd/device_validation.py states the result in numpy -- run_bases_host is
// normative; integer counts only, so the kernel equals it bit for bit.  The per-word rules are plain C++ in
// validation_bases_word.hpp (read that first); tests/native/validation_bases_replay.cpp states this kernel's body serially over
// them under the sanitizers.
//
// Per threshold the post-processing kernel writes the corrected labels into its slice of `work` (validation_label_passes, the
// run-state step's own label passes); ONE launch of validation_run_bases_kernel then counts, blockIdx.x striding over the
// stretches and blockIdx.y over the thresholds.  The base map is read where the set keeps it, at basemap[src_first[r] + i]: no
// packed copy of it exists.
//
// A workgroup walks its stretch in pieces of CF_RUN_PIECE samples, one 64-sample word per lane (64 coalesced byte loads of the
// labels, the prediction and the base map + nine ballots per wave and word).  The vbs_seg at the end of every word is an inclusive
// scan with vbs_join: over the lanes of a wave by shuffles, over the four waves through LDS, from piece to piece in a register
// every thread keeps.  Inside a word a lane steps from falling edge to falling edge with bit operations; no lane walks samples.
//
// Counts collect in one LDS table per workgroup (2 * 3 * 5 * (max_bases + 1) cells) by integer LDS adds at the falling edges and go
// to the zeroed output with one 64-bit integer atomic per non-zero cell at the end of the stretch.  Equal inputs give equal bits
// whatever the grid.
#pragma once
#include "validation_bases_word.hpp"

#define CF_BASES_MAX_CELLS (2 * 3 * VBS_CLASSES * (VBS_MAX_BASES + 1))

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_run_bases_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                              const uint8_t* __restrict__ y, const uint8_t* __restrict__ basemap,
                                                                              int64_t basemap_total, const int64_t* __restrict__ src_first,
                                                                              const int64_t* __restrict__ bounds, const int64_t* __restrict__ length,
                                                                              int64_t n_reads, int64_t total, int K, int max_bases,
                                                                              unsigned long long* __restrict__ counts_out) {
    __shared__ vbs_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned s_tab[CF_BASES_MAX_CELLS];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int slab = vbs_cells(max_bases), cells = 2 * slab;
    for (int c = threadIdx.x; c < cells; c += CF_RUN_THREADS) s_tab[c] = 0u;
    __syncthreads();
    for (int k = blockIdx.y; k < K; k += gridDim.y) {
        const uint8_t* __restrict__ p = pred + (int64_t)k * pred_stride;
        for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
            const int64_t b0 = bounds[r], size = bounds[r + 1] - b0, src = src_first[r];
            const int64_t n = length[r] < size ? length[r] : size;                 // the zero tail is not part of the stretch
            if (n <= 0) continue;                                                  // (uniform)
            const int64_t n_words = (n >> 6) + 1;                                  // the word that holds position n closes the last run
            vbs_seg carry[2] = {vbs_none(), vbs_none()};
            for (int64_t w0 = 0; w0 < n_words; w0 += CF_RUN_THREADS) {
                // 1. masks: word j of this wave's 64 lands in lane j
                const int64_t wave_word = w0 + (int64_t)wave * 64;
                unsigned long long y1 = 0, y0 = 0, p1 = 0, p0 = 0, mk = 0, ma = 0, mc = 0, mg = 0, mt = 0;
                for (int j = 0; j < 64; ++j) {
                    const int64_t i0 = (wave_word + j) * 64;
                    if (i0 >= n) break;                                            // (uniform)
                    const int64_t i = i0 + lane;
                    unsigned yv = 0xffu, pv = 0xffu, bv = 0u;
                    if (i < n) {
                        if ((uint64_t)(b0 + i) < (uint64_t)total) {
                            yv = y[b0 + i];
                            pv = p[b0 + i];
                        }
                        if ((uint64_t)(src + i) < (uint64_t)basemap_total) bv = basemap[src + i];
                    }
                    const unsigned long long by1 = __ballot(yv == 1u), by0 = __ballot(yv == 0u);
                    const unsigned long long bp1 = __ballot(pv == 1u), bp0 = __ballot(pv == 0u);
                    const unsigned long long bmk = __ballot((bv & 0x80u) != 0u);
                    const unsigned long long ba = __ballot(bv == (0x80u | 'A')), bc = __ballot(bv == (0x80u | 'C'));
                    const unsigned long long bg = __ballot(bv == (0x80u | 'G')), bt = __ballot(bv == (0x80u | 'T'));
                    if ((int)lane == j) { y1 = by1; y0 = by0; p1 = bp1; p0 = bp0; mk = bmk; ma = ba; mc = bc; mg = bg; mt = bt; }
                }
                unsigned long long run_y = y1, run_p = p1;
                const int64_t word = wave_word + lane;
                if (n >= 2 && word == ((n - 1) >> 6) && (uint64_t)(b0 + n - 2) < (uint64_t)total) {   // hp_loc_dict closes an open run AT the last sample
                    const unsigned long long last = 1ull << ((n - 1) & 63);
                    if (y[b0 + n - 2] == 1u) run_y |= last;
                    if (p[b0 + n - 2] == 1u) run_p |= last;
                }
                const vbs_masks w[2] = {{run_y, p1, p0, mk, {ma, mc, mg, mt}}, {run_p, y1, y0, mk, {ma, mc, mg, mt}}};
                // 2. the seg at the end of every word: inclusive scan over the wave, wave totals to LDS
                vbs_seg inc[2] = {vbs_word(w[0]), vbs_word(w[1])};
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const vbs_seg o = (vbs_seg)__shfl_up((int)inc[q], d);
                        if ((int)lane >= d) inc[q] = vbs_join(o, inc[q]);
                    }
                }
                if (lane == 63u) { s_seg[wave][0] = inc[0]; s_seg[wave][1] = inc[1]; }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    vbs_seg in = carry[q];                                         // at the end of the word before mine
#pragma unroll
                    for (int v = 0; v < CF_RUN_WAVES; ++v) {
                        const vbs_seg t = s_seg[v][q];
                        if (v < (int)wave) in = vbs_join(in, t);
                        carry[q] = vbs_join(carry[q], t);                          // (every thread: the piece's total)
                    }
                    const vbs_seg left = (vbs_seg)__shfl_up((int)inc[q], 1);
                    if (lane != 0u) in = vbs_join(in, left);
                    // 3. the runs that end in my word (words past the stretch hold no bit and nothing open: no run)
                    unsigned* row = s_tab + q * slab;
                    vbs_count(w[q], in, max_bases, [row](int cell) { atomicAdd(&row[cell], 1u); });
                }
                __syncthreads();                                                   // s_seg is written again by the next piece
            }
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

// Argument checks: validation_run_args_ok's, plus max_bases and the base map.  An exact check of the base map's size against the
// selection would need src_first on the host; the kernel checks every index against basemap_total instead (a sample past it has
// no mark), and DeviceValidationSet keeps the base map as long as its labels.
extern "C" int cf_validation_run_bases(cf_model* m, const float* probs, const uint8_t* y, const uint8_t* basemap, int64_t basemap_total,
                                       const int64_t* src_first, const int64_t* bounds, const int64_t* length, int64_t n, int64_t total,
                                       int64_t longest, const double* thresholds, int32_t n_thresholds, int32_t max_bases, int32_t max_gap,
                                       int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    const std::string fn = "cf_validation_run_bases";
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_work_bytes", probs, y, bounds, length, n, total, longest, thresholds,
                                              n_thresholds, max_gap, min_run, counts_out, work, work_bytes)) return rc;
    if (!basemap || !src_first) return fail(CF_ERR_INVALID, fn + ": null argument");
    if (max_bases < 1 || max_bases > VBS_MAX_BASES)
        return fail(CF_ERR_INVALID, fn + ": max_bases must be in 1 .. " + std::to_string(VBS_MAX_BASES));
    if (basemap_total < 1 || basemap_total > 0x7fffffff) return fail(CF_ERR_INVALID, fn + ": basemap_total must be in [1, 2^31)");
    const int64_t stride = (total + 63) / 64 * 64;
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)n_thresholds * 2 * vbs_cells(max_bases) * sizeof(int64_t), s));
    if (total == 0) return CF_OK;                              // stretches without a sample: the zeroed table
    uint8_t* lab = static_cast<uint8_t*>(work);
    if (const int rc = validation_label_passes(probs, bounds, length, n, total, thresholds, n_thresholds, max_gap, min_run, lab, stride, s)) return rc;
    hipLaunchKernelGGL(validation_run_bases_kernel, dim3((unsigned)std::min<int64_t>(n, 1 << 20), (unsigned)n_thresholds), dim3(CF_RUN_THREADS),
                       0, s, lab, stride, y, basemap, basemap_total, src_first, bounds, length, n, total, (int)n_thresholds, (int)max_bases,
                       reinterpret_cast<unsigned long long*>(counts_out));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
