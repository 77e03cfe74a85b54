// Event-level validation: how many true homopolymers a round found completely, partly or not at all, and how many called
// stretches hold none (the reference's offline networks/process_output.py:235-273: hp_loc_dict cuts truth and corrected prediction
// into runs, check_hp gives every run a state against the other array).  catfish_amd/device_validation.py states the result in
// numpy -- run_states_host is normative; integer counts only, so the kernel equals it bit for bit.
//
// Per threshold the existing post-processing kernel writes the corrected labels of the whole packed batch (threshold +
// correct_short inside every stretch, read_offsets = bounds, read_lengths = length) into its slice of `work`; ONE launch of
// validation_run_states_kernel then counts, blockIdx.x striding over the stretches and blockIdx.y over the thresholds.
//
// A workgroup walks its stretch in pieces of CF_RUN_PIECE samples, one 64-sample word per lane.  Per kind (0: runs of y == 1 judged
// against the prediction, 1: runs of the prediction judged against y) a lane holds three masks of its word: run, other-is-1,
// other-is-0 (64 coalesced byte loads + ballots per wave, as in postprocess_bits_kernel).  hp_loc_dict's last-sample rule ORs bit
// n - 1 of the RUN mask with bit n - 2 (read straight from memory by the one lane that owns bit n - 1); the masks a run is judged
// against stay as they are.
//
// A run is counted once, at its falling edge (the first sample after it; a run is closed at sample n by the word that holds
// position n, which is why a stretch has n / 64 + 1 words).  The part of a run before the lane's word arrives as a carry
// (length, all-ones, all-zeros): the trailing run of every word is one element of a segmented scan whose "reset" flag is "this
// word is not all run" -- inclusive over the lanes of a wave by shuffles, over the four waves through LDS, and from piece to piece
// in a register every thread keeps.  Inside a word a lane steps from falling edge to falling edge (at most 32, alternating
// labels reach that) with bit operations; no lane walks the samples of a run, so a stretch of ones costs what a stretch of zeros costs.
//
// Counts: a lane packs (bin, state) counts of a piece into 8-bit fields (<= 33 per word), widens them to 16 bits for the wave
// butterfly (<= 64 * 33), lane 0 spreads them into the wave's LDS row, the first CF_RUN_CELLS threads add the rows into a
// register that lives for the whole stretch and add it to the zeroed table with ONE integer atomic per non-zero cell.  Equal
// inputs give equal bits whatever the grid.
#pragma once

#define CF_RUN_THREADS 256
#define CF_RUN_WAVES (CF_RUN_THREADS / 64)
#define CF_RUN_PIECE (CF_RUN_THREADS * 64)
#define CF_RUN_MAX_EDGES 7
#define CF_RUN_BINS (CF_RUN_MAX_EDGES + 1)
#define CF_RUN_CELLS (2 * CF_RUN_BINS * 3)            // [kind][bin][state]

struct cf_run_edges { unsigned e[CF_RUN_MAX_EDGES]; };     // ascending; unused ones 0xffffffff (no run is that long: total < 2^31)

// One element of the segmented scan: the run that is open at the end of a stretch of words.  flags: 1 = the stretch of words is
// not all run (what came before it cannot reach its end), 2 = the other array is 1 over the open run, 4 = it is 0 over it.
struct cf_run_seg { unsigned len, flags; };

__device__ __forceinline__ cf_run_seg cf_run_join(const cf_run_seg a, const cf_run_seg b) {      // a, then b
    const bool cut = (b.flags & 1u) != 0u;
    return {cut ? b.len : a.len + b.len, cut ? b.flags : ((a.flags & b.flags & 6u) | (a.flags & 1u))};
}

__device__ __forceinline__ cf_run_seg cf_run_shfl_up(const cf_run_seg v, int d) {
    return {(unsigned)__shfl_up((int)v.len, d), (unsigned)__shfl_up((int)v.flags, d)};
}

// the trailing run of one word (the ones that reach bit 63)
__device__ __forceinline__ cf_run_seg cf_run_word(unsigned long long run, unsigned long long is1, unsigned long long is0) {
    const unsigned long long gap = ~run;
    const int t = gap ? __builtin_clzll(gap) : 64;
    const unsigned long long m = t ? ~0ull << (64 - t) : 0ull;
    return {(unsigned)t, (t < 64 ? 1u : 0u) | ((is1 & m) == m ? 2u : 0u) | ((is0 & m) == m ? 4u : 0u)};
}

// the runs that END in this word (falling edges), `in` = the run open at the end of the word before.  acc[state]: 8 bins x 8 bits
__device__ __forceinline__ void cf_run_count(unsigned long long run, unsigned long long is1, unsigned long long is0, const cf_run_seg in,
                                             const cf_run_edges& edges, unsigned long long (&acc)[3]) {
    const unsigned long long before = (run << 1) | (in.len ? 1ull : 0ull);
    unsigned long long fall = ~run & before, rise = run & ~before;
    bool carried = in.len != 0u;
    while (fall) {
        const int e = __builtin_ctzll(fall);                   // the run covers [s, e) of this word (+ in.len samples before it)
        fall &= fall - 1ull;
        int s = 0;
        unsigned len = in.len, flags = in.flags;
        if (!carried) {
            s = __builtin_ctzll(rise);
            rise &= rise - 1ull;
            len = 0u;
            flags = 6u;
        }
        carried = false;
        const unsigned long long m = ((1ull << e) - 1ull) & ~((1ull << s) - 1ull);
        len += (unsigned)(e - s);
        const bool all1 = (flags & 2u) && (is1 & m) == m, all0 = (flags & 4u) && (is0 & m) == m;
        unsigned bin = 0;
#pragma unroll
        for (int j = 0; j < CF_RUN_MAX_EDGES; ++j) bin += len >= edges.e[j] ? 1u : 0u;
        const unsigned long long one = 1ull << (8u * bin);
        acc[0] += all1 ? one : 0ull;                           // complete
        acc[1] += (!all1 && !all0) ? one : 0ull;               // incomplete
        acc[2] += (!all1 && all0) ? one : 0ull;                // absent
    }
}

__device__ __forceinline__ unsigned long long cf_run_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}

__global__ __launch_bounds__(CF_RUN_THREADS) void validation_run_states_kernel(const uint8_t* __restrict__ pred, int64_t pred_stride,
                                                                               const uint8_t* __restrict__ y, const int64_t* __restrict__ bounds,
                                                                               const int64_t* __restrict__ length, int64_t n_reads, int64_t total,
                                                                               int K, cf_run_edges edges, int n_bins,
                                                                               unsigned long long* __restrict__ counts_out) {
    __shared__ cf_run_seg s_seg[CF_RUN_WAVES][2];
    __shared__ unsigned s_cnt[CF_RUN_WAVES][CF_RUN_CELLS];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const cf_run_seg none = {0u, 7u};                          // nothing open: what a stretch starts with
    for (int k = blockIdx.y; k < K; k += gridDim.y) {
        const uint8_t* __restrict__ p = pred + (int64_t)k * pred_stride;
        for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
            const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
            const int64_t n = length[r] < size ? length[r] : size;                 // the zero tail is not part of the stretch
            if (n <= 0) continue;                                                  // (uniform)
            const int64_t n_words = (n >> 6) + 1;                                  // the word that holds position n closes the last run
            cf_run_seg carry[2] = {none, none};
            unsigned mine = 0;                                                     // threads < CF_RUN_CELLS: the stretch's count of one cell
            for (int64_t w0 = 0; w0 < n_words; w0 += CF_RUN_THREADS) {
                // 1. masks: word j of this wave's 64 lands in lane j
                const int64_t wave_word = w0 + (int64_t)wave * 64;
                unsigned long long y1 = 0, y0 = 0, p1 = 0, p0 = 0;
                for (int j = 0; j < 64; ++j) {
                    const int64_t i0 = (wave_word + j) * 64;
                    if (i0 >= n) break;                                            // (uniform)
                    const int64_t i = i0 + lane;
                    unsigned yv = 0xffu, pv = 0xffu;
                    if (i < n && (uint64_t)(b0 + i) < (uint64_t)total) {
                        yv = y[b0 + i];
                        pv = p[b0 + i];
                    }
                    const unsigned long long by1 = __ballot(yv == 1u), by0 = __ballot(yv == 0u);
                    const unsigned long long bp1 = __ballot(pv == 1u), bp0 = __ballot(pv == 0u);
                    if ((int)lane == j) { y1 = by1; y0 = by0; p1 = bp1; p0 = bp0; }
                }
                unsigned long long run_y = y1, run_p = p1;
                const int64_t word = wave_word + lane;
                if (n >= 2 && word == ((n - 1) >> 6) && (uint64_t)(b0 + n - 2) < (uint64_t)total) {   // hp_loc_dict closes an open run AT the last sample
                    const unsigned long long last = 1ull << ((n - 1) & 63);
                    if (y[b0 + n - 2] == 1u) run_y |= last;
                    if (p[b0 + n - 2] == 1u) run_p |= last;
                }
                // 2. the run open at the end of every word: inclusive scan over the wave, wave totals to LDS
                cf_run_seg inc[2] = {cf_run_word(run_y, p1, p0), cf_run_word(run_p, y1, y0)};
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const cf_run_seg o = cf_run_shfl_up(inc[q], d);
                        if ((int)lane >= d) inc[q] = cf_run_join(o, inc[q]);
                    }
                }
                if (lane == 63u) { s_seg[wave][0] = inc[0]; s_seg[wave][1] = inc[1]; }
                __syncthreads();
                unsigned long long acc[2][3] = {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}};
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    cf_run_seg in = carry[q];                                      // open at the end of the word before mine
#pragma unroll
                    for (int v = 0; v < CF_RUN_WAVES; ++v) {
                        const cf_run_seg t = s_seg[v][q];
                        if (v < (int)wave) in = cf_run_join(in, t);
                        carry[q] = cf_run_join(carry[q], t);                       // (every thread: the piece's total)
                    }
                    const cf_run_seg left = cf_run_shfl_up(inc[q], 1);
                    if (lane != 0u) in = cf_run_join(in, left);
                    // 3. the runs that end in my word
                    if (q == 0) cf_run_count(run_y, p1, p0, in, edges, acc[0]);
                    else cf_run_count(run_p, y1, y0, in, edges, acc[1]);
                }
                // 4. counts: 8-bit fields -> 16-bit fields -> wave sum -> the wave's LDS row
#pragma unroll
                for (int q = 0; q < 2; ++q) {
#pragma unroll
                    for (int st = 0; st < 3; ++st) {
                        const unsigned long long even = cf_run_wave_sum(acc[q][st] & 0x00ff00ff00ff00ffull);
                        const unsigned long long odd = cf_run_wave_sum((acc[q][st] >> 8) & 0x00ff00ff00ff00ffull);
                        if (lane == 0u) {
#pragma unroll
                            for (int f = 0; f < 4; ++f) {
                                s_cnt[wave][(q * CF_RUN_BINS + 2 * f) * 3 + st] = (unsigned)(even >> (16 * f)) & 0xffffu;
                                s_cnt[wave][(q * CF_RUN_BINS + 2 * f + 1) * 3 + st] = (unsigned)(odd >> (16 * f)) & 0xffffu;
                            }
                        }
                    }
                }
                __syncthreads();
                if (threadIdx.x < CF_RUN_CELLS) {
#pragma unroll
                    for (int v = 0; v < CF_RUN_WAVES; ++v) mine += s_cnt[v][threadIdx.x];
                }
                // (s_seg is written again only after the barrier above, s_cnt only after the next piece's first barrier)
            }
            if (threadIdx.x < CF_RUN_CELLS && mine != 0u) {
                const int q = threadIdx.x / (CF_RUN_BINS * 3), bin = (threadIdx.x / 3) % CF_RUN_BINS, st = threadIdx.x % 3;
                if (bin < n_bins) atomicAdd(&counts_out[(((int64_t)k * 2 + q) * n_bins + bin) * 3 + st], (unsigned long long)mine);
            }
            __syncthreads();                                   // the next stretch's first piece writes s_seg and, later, s_cnt
        }
    }
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
// stretch): what cf_validation_run_states and cf_validation_run_borders count on.
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

// The argument checks cf_validation_run_states and cf_validation_run_borders share (each keeps the ones of its own table);
// `work_fn` is the function the message about too small a work buffer names (the two have one rule: cf_validation_run_work_bytes).
static int validation_run_args_ok(const std::string& fn, const char* work_fn, const float* probs, const uint8_t* y, const int64_t* bounds,
                                  const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                  int32_t n_thresholds, int32_t max_gap, int32_t min_run, const int64_t* counts_out, const void* work,
                                  int64_t work_bytes) {
    if (!probs || !y || !bounds || !length || !thresholds || !counts_out || !work) return fail(CF_ERR_INVALID, fn + ": null argument");
    if (n <= 0 || n > 0x7fffffff) return fail(CF_ERR_INVALID, fn + ": n must be in [1, 2^31)");
    if (n_thresholds < 1 || n_thresholds > CF_SCORE_MAX_K)
        return fail(CF_ERR_INVALID, fn + ": between 1 and " + std::to_string(CF_SCORE_MAX_K) + " thresholds per call");
    if (total < 0 || total > 0x7fffffff || longest < 0 || longest > total) return fail(CF_ERR_INVALID, fn + ": bad size");
    if (min_run < 1) return fail(CF_ERR_INVALID, fn + ": min_run must be >= 1");
    if (!validation_bridge_ok(min_run, max_gap, work))
        return fail(CF_ERR_INVALID, fn + ": bridging needs max_gap >= 0, min_run + max_gap <= 64 and a 16-byte aligned work buffer");
    if (work_bytes < cf_validation_run_work_bytes(total, n_thresholds))
        return fail(CF_ERR_INVALID, fn + ": work needs " + work_fn + "(total, n_thresholds) bytes");
    return CF_OK;
}

static int validation_run_states_impl(const std::string& fn, cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds,
                                      const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                      int32_t n_thresholds, const int64_t* edges, int32_t n_edges, int32_t max_gap, int32_t min_run,
                                      int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    if (n_edges > 0 && !edges) return fail(CF_ERR_INVALID, fn + ": null argument");
    if (const int rc = validation_run_args_ok(fn, "cf_validation_run_work_bytes", probs, y, bounds, length, n, total, longest, thresholds,
                                              n_thresholds, max_gap, min_run, counts_out, work, work_bytes)) return rc;
    if (n_edges < 0 || n_edges > CF_RUN_MAX_EDGES)
        return fail(CF_ERR_INVALID, fn + ": at most " + std::to_string(CF_RUN_MAX_EDGES) + " edges");
    cf_run_edges e;
    for (int j = 0; j < CF_RUN_MAX_EDGES; ++j) e.e[j] = 0xffffffffu;
    for (int j = 0; j < n_edges; ++j) {
        if (edges[j] < 1 || (j > 0 && edges[j] <= edges[j - 1]))
            return fail(CF_ERR_INVALID, fn + ": edges must be positive and ascending");
        e.e[j] = (unsigned)std::min<int64_t>(edges[j], 0xffffffffll);
    }
    const int64_t stride = (total + 63) / 64 * 64;
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_bins = n_edges + 1;
    HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)n_thresholds * 2 * n_bins * 3 * sizeof(int64_t), s));
    if (total == 0) return CF_OK;                              // stretches without a sample: the zeroed table
    uint8_t* lab = static_cast<uint8_t*>(work);
    if (const int rc = validation_label_passes(probs, bounds, length, n, total, thresholds, n_thresholds, max_gap, min_run, lab, stride, s)) return rc;
    hipLaunchKernelGGL(validation_run_states_kernel, dim3((unsigned)std::min<int64_t>(n, 1 << 20), (unsigned)n_thresholds), dim3(CF_RUN_THREADS),
                       0, s, lab, stride, y, bounds, length, n, total, (int)n_thresholds, e, n_bins,
                       reinterpret_cast<unsigned long long*>(counts_out));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_validation_run_states(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                        int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                        const int64_t* edges, int32_t n_edges, int32_t min_run, int64_t* counts_out, void* work,
                                        int64_t work_bytes, void* stream) {
    return validation_run_states_impl("cf_validation_run_states", m, probs, y, bounds, length, n, total, longest, thresholds, n_thresholds,
                                      edges, n_edges, 0, min_run, counts_out, work, work_bytes, stream);
}

// ... with gaps of at most max_gap samples bridged in every stretch before correct_short (device_validation.run_states_host(max_gap=))
extern "C" int cf_validation_run_states_bridged(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds,
                                                const int64_t* length, int64_t n, int64_t total, int64_t longest, const double* thresholds,
                                                int32_t n_thresholds, const int64_t* edges, int32_t n_edges, int32_t max_gap,
                                                int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream) {
    return validation_run_states_impl("cf_validation_run_states_bridged", m, probs, y, bounds, length, n, total, longest, thresholds,
                                      n_thresholds, edges, n_edges, max_gap, min_run, counts_out, work, work_bytes, stream);
}
