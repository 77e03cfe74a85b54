// Labels from a basecaller's move table (catfish_amd/labelling.py states the result in numpy -- merge_moves_host, move_classes_host
// and MoveBatch.label_host are the definitions; every index and arithmetic rule is in csrc/label_moves_rule.hpp and is replayed on
// the CPU under the sanitizers by tests/native/label_moves_replay.cpp).  An un-resquiggled read is a table of events (a k-mer, a
// move, a length in seconds); an event with move != 0 and the stays (move == 0) behind it are one merged event of
// ceil(sum of lengths * 4000) samples, and the labels are the homopolymer test on the merged event's own k-mer, widened by two
// merged events, repeated per sample and cut at the end of the raw signal.
//
//   merge    workgroups stride over the reads, a read goes through in pieces of LM_PIECE events, four consecutive ones per thread.
//            Head flags go through a block scan (le_block_scan of csrc/label_events.hpp over the 256 thread counts, a carry from
//            piece to piece): that is the merged index.  The thread that owns a head walks its stays in global memory -- across piece borders, never
//            across the read -- summing the lengths in the table's own type, left to right, one rounding per addition.  It writes
//            the sample count, the uniform-k-mer flag and the k-mer's middle byte to the read's slot of the compacted tables; the
//            slots behind the M-th are zeroed, and M goes to counts[2 r].
//   classes  the same walk over the compacted tables: core flags (uniform, outside the clips) for the piece and two merged events
//            each side go to LDS, then every thread takes four consecutive slots: their class, and their first sample from a block
//            scan of the counts.  final = min(sum, n_raw) goes to counts[2 r + 1].
//   expand   label_expand_kernel (csrc/label_events.hpp) as it is, over the compacted tables: every merged event of a sound read
//            has at least one sample, so its staging bound holds, and the zeroed slots cover nothing.
//
// No atomics: equal inputs give equal bytes.  No scratch.  The float path never widens to double and never reorders a sum.
#pragma once
#include "label_moves_rule.hpp"

__device__ inline int64_t lm_merged_count(const float* lengths_r, int64_t h, int64_t end) { return lm_merged_count_f(lengths_r, h, end); }
__device__ inline int64_t lm_merged_count(const double* lengths_r, int64_t h, int64_t end) { return lm_merged_count_d(lengths_r, h, end); }

template <typename T>
__global__ __launch_bounds__(LM_THREADS) void label_moves_merge_kernel(const uint8_t* __restrict__ states, const T* __restrict__ lengths,
                                                                       const int32_t* __restrict__ moves,
                                                                       const int64_t* __restrict__ event_offsets, int64_t n_reads,
                                                                       int64_t n_events, int32_t k, int32_t* __restrict__ mlen,
                                                                       uint8_t* __restrict__ mbase, uint8_t* __restrict__ uniform,
                                                                       int32_t* __restrict__ counts) {
    __shared__ int32_t s_scan[2][LM_THREADS];
    const int tid = (int)threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
        const int32_t* moves_r = moves + ev.first;
        const T* lengths_r = lengths + ev.first;
        int64_t carry = 0;                                                        // merged events before this piece
        for (int64_t p0 = 0; p0 < ev.n; p0 += LM_PIECE) {
            uint32_t heads = 0;                                                   // bit q: my q-th event is a head
#pragma unroll
            for (int q = 0; q < LM_PER_THREAD; ++q)
                heads |= (lm_is_head(moves_r, p0 + LM_PER_THREAD * tid + q, ev.n) ? 1u : 0u) << q;
            const int32_t mine = __popc(heads);
            const int cur = le_block_scan(s_scan, tid, mine);
            int64_t j = carry + s_scan[cur][tid] - mine;
#pragma unroll 1
            for (int q = 0; q < LM_PER_THREAD; ++q) {
                if (!((heads >> q) & 1u)) continue;
                const int64_t h = p0 + LM_PER_THREAD * tid + q;
                const int64_t slot = lm_merged_slot(j, ev.n);
                if (slot >= 0) {
                    const uint8_t* state = states + (ev.first + h) * k;
                    mlen[ev.first + slot] = (int32_t)lm_merged_count(lengths_r, h, lm_stays_end(moves_r, h, ev.n));
                    uniform[ev.first + slot] = lm_uniform(state, k);
                    mbase[ev.first + slot] = state[k / 2];
                }
                ++j;
            }
            carry += s_scan[cur][LM_THREADS - 1];
            __syncthreads();                                                      // the next piece (or read) scans again
        }
        for (int64_t slot = carry + tid; slot < ev.n; slot += LM_THREADS) {       // M <= E: the rest of the read's slot holds nothing
            mlen[ev.first + slot] = 0;
            uniform[ev.first + slot] = 0;
            mbase[ev.first + slot] = 0;
        }
        if (tid == 0) counts[2 * r] = (int32_t)carry;
    }
}

__global__ __launch_bounds__(LM_THREADS) void label_moves_classes_kernel(const int64_t* __restrict__ event_offsets,
                                                                         const int32_t* __restrict__ clipped,
                                                                         const int64_t* __restrict__ n_raw, int64_t n_reads,
                                                                         int64_t n_events, const int32_t* __restrict__ mlen,
                                                                         const uint8_t* __restrict__ uniform, int32_t* __restrict__ start,
                                                                         uint8_t* __restrict__ cls, int32_t* counts) {
    __shared__ uint8_t s_cores[LM_CORE_SLOTS];
    __shared__ int64_t s_scan[2][LM_THREADS];
    const int tid = (int)threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
        const int64_t m = lm_merged_sound(counts[2 * r], ev.n);
        const int64_t cs = clipped[2 * r], ce = clipped[2 * r + 1];
        const uint8_t* uniform_r = uniform + ev.first;
        int64_t carry = 0;
        for (int64_t p0 = 0; p0 < ev.n; p0 += LM_PIECE) {                         // all E slots: the expansion searches their starts
#pragma unroll 1
            for (int slot = tid; slot < LM_CORE_SLOTS; slot += LM_THREADS) {
                const int64_t j = p0 - LM_WIDEN + slot;
                s_cores[slot] = lm_core_slot(j, p0, m) >= 0 ? lm_core(uniform_r, j, m, cs, ce) : 0;
            }
            int64_t before[LM_PER_THREAD], sum = 0;
#pragma unroll
            for (int q = 0; q < LM_PER_THREAD; ++q) {
                const int64_t e = p0 + LM_PER_THREAD * tid + q;
                before[q] = sum;
                sum += e < ev.n ? le_len(mlen[ev.first + e]) : 0;
            }
            const int cur = le_block_scan(s_scan, tid, sum);
            const int64_t mine = carry + s_scan[cur][tid] - sum;                  // 1024 counts below 2^31 and a carry below 2^31
#pragma unroll
            for (int q = 0; q < LM_PER_THREAD; ++q) {
                const int64_t e = p0 + LM_PER_THREAD * tid + q;
                if (e < ev.n) {
                    start[ev.first + e] = (int32_t)le_sat(mine + before[q]);
                    cls[ev.first + e] = lm_class(s_cores, e, p0, m);
                }
            }
            carry = le_sat(carry + s_scan[cur][LM_THREADS - 1]);
            __syncthreads();                                                      // the next piece (or read) restages
        }
        if (tid == 0) counts[2 * r + 1] = lm_final(carry, n_raw[r]);
    }
}

extern "C" int64_t cf_label_moves_work_bytes(int64_t n_reads, int64_t n_events) { return lm_work_bytes(n_reads, n_events); }

extern "C" int cf_label_moves(cf_model* m, const uint8_t* states, const void* lengths, int32_t lengths_f64, const int32_t* moves,
                              const int64_t* event_offsets, const int32_t* clipped, const int64_t* n_raw, const int64_t* sample_offsets,
                              int64_t n_reads, int64_t n_events, int64_t total, int32_t k, uint8_t* labels_out, uint8_t* basemap_out,
                              void* work, int64_t work_bytes, void* stream) {
    switch (lm_refusal(n_reads, n_events, total, k, lengths_f64, work_bytes)) {
        case 0: break;
        case 1: return fail(CF_ERR_INVALID, "cf_label_moves: negative size");
        case 2: return fail(CF_ERR_INVALID, "cf_label_moves: at most 2^31 - 1 events and samples per call");
        case 3: return fail(CF_ERR_INVALID, "cf_label_moves: k must be in 1 .. 15");
        case 4: return fail(CF_ERR_INVALID, "cf_label_moves: too many reads for one call (reads + samples / 4096 above 2^23)");
        case 6: return fail(CF_ERR_INVALID, "cf_label_moves: lengths_f64 must be 0 (float) or 1 (double)");
        default: return fail(CF_ERR_INVALID, "cf_label_moves: the work buffer is smaller than cf_label_moves_work_bytes(n_reads, n_events)");
    }
    if (total == 0) return CF_OK;
    if (!states || !lengths || !moves || !event_offsets || !clipped || !n_raw || !sample_offsets || !labels_out || !work)
        return fail(CF_ERR_INVALID, "cf_label_moves: null argument");
    if (n_reads == 0) return fail(CF_ERR_INVALID, "cf_label_moves: samples but no reads");
    if (reinterpret_cast<uintptr_t>(work) % 4 != 0) return fail(CF_ERR_INVALID, "cf_label_moves: the work buffer must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(lengths) % (lengths_f64 ? 8 : 4) != 0)
        return fail(CF_ERR_INVALID, "cf_label_moves: the lengths must be aligned to their type");
    if (m) HIP_TRY(hipSetDevice(m->device));              // NULL: the calling thread's current device
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t* at = static_cast<uint8_t*>(work);
    int32_t* mlen = reinterpret_cast<int32_t*>(at + lm_work_mlen(n_reads, n_events));
    int32_t* start = reinterpret_cast<int32_t*>(at + lm_work_start(n_reads, n_events));
    int32_t* counts = reinterpret_cast<int32_t*>(at + lm_work_counts(n_reads, n_events));
    uint8_t* cls = at + lm_work_cls(n_reads, n_events);
    uint8_t* mbase = at + lm_work_mbase(n_reads, n_events);
    uint8_t* uniform = at + lm_work_uniform(n_reads, n_events);
    const int64_t grid = n_reads < LM_GRID ? n_reads : LM_GRID;
    if (lengths_f64)
        hipLaunchKernelGGL(label_moves_merge_kernel<double>, dim3((unsigned)grid), dim3(LM_THREADS), 0, s, states,
                           static_cast<const double*>(lengths), moves, event_offsets, n_reads, n_events, k, mlen, mbase, uniform, counts);
    else
        hipLaunchKernelGGL(label_moves_merge_kernel<float>, dim3((unsigned)grid), dim3(LM_THREADS), 0, s, states,
                           static_cast<const float*>(lengths), moves, event_offsets, n_reads, n_events, k, mlen, mbase, uniform, counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(label_moves_classes_kernel, dim3((unsigned)grid), dim3(LM_THREADS), 0, s, event_offsets, clipped, n_raw, n_reads,
                       n_events, mlen, uniform, start, cls, counts);
    HIP_TRY(hipGetLastError());
    const int64_t expand_grid = n_reads + total / LE_TILE;
    hipLaunchKernelGGL(label_expand_kernel, dim3((unsigned)expand_grid), dim3(LE_THREADS), 0, s, mbase, mlen, event_offsets, sample_offsets,
                       n_reads, n_events, total, start, cls, labels_out, basemap_out);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
