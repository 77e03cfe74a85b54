// Validation curves: a histogram of a round's probabilities at every representable threshold step, per label row (label == 1,
// label == 0, any other), from which the host draws the whole ROC and precision-recall curves and their areas
// (catfish_amd/device_validation.py states it in numpy -- curve_host is normative; the reference draws the same curves offline from
// text dumps of every score, networks/metrics.py:66-94 and networks/precision_recall_ROC.py:14-82).  Integer counts only, so the
// table equals curve_host bit for bit, every run.
//
// Stretch r is the first length[r] packed samples from bounds[r]; its zero tail is not counted.  A sample's cell is
// vc_key(bits of p, label, shift) (csrc/validation_curve_bin.hpp): row * bins + bin.
//
// Grid as in validation.hpp: blockIdx.x = stretch, blockIdx.y strides over its chunks of CF_SCORE_CHUNK samples, `longest` is only a
// hint.  The table (3 x 65 025 counters at shift 14, over three million at shift 10) does not fit the LDS, and real probabilities
// pile up near 0 and 1, so a workgroup combines its chunk on chip before it goes out:
//
//   1. every thread writes the keys of its samples into LDS (VC_NO_KEY where there is none);
//   2. a bitonic sort of the keys in LDS -- of the smallest power of two that holds the chunk's samples, so a stretch of one sample
//      costs one compare;
//   3. the thread that holds the FIRST key of a run of equal keys finds the run's end by bisection (the keys are sorted: at most 11
//      LDS reads) and adds the run's length to the zeroed table with ONE 64-bit integer atomic.
//
// So the global atomics a workgroup issues number the DISTINCT cells of its chunk, whatever the samples: 2048 equal probabilities
// cost one.  Their order cannot show (integers).  The sort was taken over an LDS hash table: its cost does not depend on the values
// (no probing, no LDS atomics on one hot slot, no loop whose length the data decides), and the sorted keys leave the workgroup as
// ascending, mostly adjacent addresses.
#pragma once
#include "validation_curve_bin.hpp"

#define CF_CURVE_THREADS 256

// Steps 2 and 3 over the `span` keys in s_key (a power of two in [2, 2 * CF_SCORE_CHUNK]; the caller's barrier is behind their
// writes): the bitonic sort, then one atomic per run of equal keys below `cells`.  validation_scores.hpp combines its keys the same way.
__device__ __forceinline__ void vc_sort_count(uint32_t* s_key, unsigned span, unsigned cells, unsigned long long* __restrict__ hist) {
    for (unsigned k = 2; k <= span; k <<= 1) {
        for (unsigned j = k >> 1; j >= 1; j >>= 1) {
            for (unsigned t = threadIdx.x; t < (span >> 1); t += CF_CURVE_THREADS) {
                const unsigned i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;              // i < l < span
                const uint32_t a = s_key[i], b = s_key[l];
                if ((a > b) == ((i & k) == 0u)) {                                  // ascending where bit k of i is clear
                    s_key[i] = b;
                    s_key[l] = a;
                }
            }
            __syncthreads();
        }
    }
    for (unsigned i = threadIdx.x; i < span; i += CF_CURVE_THREADS) {
        const uint32_t key = s_key[i];
        if (key >= cells || (i > 0u && s_key[i - 1u] == key)) continue;            // no sample here, or not the first of its run
        unsigned lo = i + 1u, hi = span;                                           // the run ends before the first other key in (i, span]
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if (s_key[mid] == key) lo = mid + 1u;
            else hi = mid;
        }
        atomicAdd(&hist[key], (unsigned long long)(lo - i));
    }
}

__global__ __launch_bounds__(CF_CURVE_THREADS) void validation_curve_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ y,
                                                                            const int64_t* __restrict__ bounds,
                                                                            const int64_t* __restrict__ length, int64_t total, int shift,
                                                                            unsigned cells, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_key[CF_SCORE_CHUNK];
    const int64_t r = blockIdx.x;
    const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
    const int64_t n = length[r] < size ? length[r] : size;                         // the zero tail is not part of the stretch
    const int64_t n_chunks = n > 0 ? (n + CF_SCORE_CHUNK - 1) / CF_SCORE_CHUNK : 0;
    for (int64_t c = blockIdx.y; c < n_chunks; c += gridDim.y) {                   // (uniform)
        const int64_t first = c * CF_SCORE_CHUNK;
        const unsigned m = (unsigned)(n - first < CF_SCORE_CHUNK ? n - first : CF_SCORE_CHUNK);      // samples of this chunk, >= 1
        unsigned span = 2;                                                         // power of two in [2, CF_SCORE_CHUNK] that holds them
        while (span < m) span <<= 1;
        for (unsigned i = threadIdx.x; i < span; i += CF_CURVE_THREADS) {
            uint32_t key = VC_NO_KEY;
            const int64_t at = first + i;
            if (i < m && at < length[r] && (uint64_t)(b0 + at) < (uint64_t)total)
                key = vc_key(__float_as_uint(probs[b0 + at]), y[b0 + at], shift);
            s_key[i] = key;
        }
        __syncthreads();
        vc_sort_count(s_key, span, cells, hist);
        __syncthreads();                                                           // s_key is written again by this workgroup's next chunk
    }
}

extern "C" int cf_validation_curve(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                   int64_t n, int64_t total, int64_t longest, int32_t shift, int64_t* hist_out, int64_t hist_capacity,
                                   void* stream) {
    if (!probs || !y || !bounds || !length || !hist_out) return fail(CF_ERR_INVALID, "cf_validation_curve: null argument");
    if (n <= 0 || n > 0x7fffffff) return fail(CF_ERR_INVALID, "cf_validation_curve: n must be in [1, 2^31)");
    if (!vc_shift_ok(shift))
        return fail(CF_ERR_INVALID, "cf_validation_curve: shift must be in " + std::to_string(VC_SHIFT_MIN) + " .. " + std::to_string(VC_SHIFT_MAX));
    if (total < 0 || longest < 0 || longest > total) return fail(CF_ERR_INVALID, "cf_validation_curve: bad size");
    const int64_t cells = (int64_t)VC_ROWS * vc_bins(shift);
    if (hist_capacity < cells)
        return fail(CF_ERR_INVALID, "cf_validation_curve: hist_out needs 3 * ((0x3F800000 >> shift) + 1) = " + std::to_string(cells) + " entries");
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(hist_out, 0, (size_t)cells * sizeof(int64_t), s));
    if (total == 0) return CF_OK;                              // stretches without a sample: the zeroed table
    hipLaunchKernelGGL(validation_curve_kernel, dim3((unsigned)n, validation_grid_height(longest, CF_SCORE_CHUNK)), dim3(CF_CURVE_THREADS), 0, s,
                       probs, y, bounds, length, total, (int)shift, (unsigned)cells, reinterpret_cast<unsigned long long*>(hist_out));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
