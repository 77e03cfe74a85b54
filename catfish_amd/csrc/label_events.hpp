// Labels from event tables (catfish_amd/labelling.py states the result in numpy -- event_classes_host, expand_events_host and
// base_map_host are the definitions; every index rule is in csrc/label_events_rule.hpp and is replayed on the CPU under the
// sanitizers by tests/native/label_events_replay.cpp).  A resquiggled read is a table of events (one base, a length in samples);
// its training labels are the 5-mer homopolymer test per event, widened by two events, repeated per event length.
//
//   classes  workgroups stride over the reads, a read goes through in pieces of LE_PIECE events.  A piece's bases go to LDS with a
//            halo of LE_HALO events, clipped to the read (never to the packed array: a run must not continue into the neighbour);
//            core flags for the piece and two events each side follow, then every thread takes four consecutive events: their
//            class, and their first sample from a block scan of the lengths (le_block_scan over the 256 thread sums, a carry
//            from piece to piece).  Both go to the work buffer.
//   expand   one workgroup per (read, tile of LE_TILE samples) -- le_block_read finds the pair from blockIdx alone.  One binary
//            search in the read's starts finds the tile's first event; the at most LE_TILE_EVENTS events the tile can meet are
//            staged in LDS (start, class, base: 24.6 KB).  A thread owns LE_RUN = 16 consecutive samples: one search in LDS for the
//            first, then it steps.  No thread walks the samples of an event and no sample searches global memory, so a 9 000-sample
//            event costs what 900 ten-sample events cost.  A whole run goes out as one 16-byte store where the address allows,
//            else as 8-, 4- or 1-byte stores.
//
// Integer only, no atomics: equal inputs give equal bytes.  HBM-bound streaming kernels; no scratch.
#pragma once
#include "label_events_rule.hpp"

// The inclusive block scan of one value per thread (Hillis-Steele over the LE_THREADS values in LDS, double-buffered): afterwards
// s_scan[cur][t] holds the sum of the values of threads 0 .. t, for the cur it returns.  Every thread of the block calls it; it
// ends in a barrier, and the caller places another before the buffers are written again.  The loop must stay rolled: unrolled,
// label_event_classes_kernel spills an SGPR.
template <typename T>
__device__ inline int le_block_scan(T (*s_scan)[LE_THREADS], int tid, T mine) {
    s_scan[0][tid] = mine;
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int step = 1; step < LE_THREADS; step <<= 1) {
        s_scan[cur ^ 1][tid] = s_scan[cur][tid] + (tid >= step ? s_scan[cur][tid - step] : 0);
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

__global__ __launch_bounds__(LE_THREADS) void label_event_classes_kernel(const uint8_t* __restrict__ bases, const int32_t* __restrict__ lengths,
                                                                         const int64_t* __restrict__ event_offsets,
                                                                         const int32_t* __restrict__ clipped, int64_t n_reads,
                                                                         int64_t n_events, int32_t kmer, int32_t* __restrict__ start,
                                                                         uint8_t* __restrict__ cls) {
    __shared__ uint8_t s_bases[LE_BASES_SLOTS];
    __shared__ uint8_t s_cores[LE_CORE_SLOTS];
    __shared__ int64_t s_scan[2][LE_THREADS];
    const int tid = (int)threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
        const int64_t cs = clipped[2 * r], ce = clipped[2 * r + 1];
        int64_t carry = 0;
        for (int64_t p0 = 0; p0 < ev.n; p0 += LE_PIECE) {
#pragma unroll 1
            for (int slot = tid; slot < LE_BASES_SLOTS; slot += LE_THREADS) {
                const int64_t e = p0 - LE_HALO + slot;
                if (le_base_slot(e, p0, ev.n) >= 0) s_bases[slot] = bases[ev.first + e];
            }
            __syncthreads();
#pragma unroll 1
            for (int slot = tid; slot < LE_CORE_SLOTS; slot += LE_THREADS) {
                const int64_t e = p0 - LE_WIDEN + slot;
                s_cores[slot] = le_core_slot(e, p0, ev.n) >= 0 ? le_core(s_bases, e, p0, ev.n, cs, ce, kmer) : 0;
            }
            int64_t before[LE_PER_THREAD], sum = 0;
#pragma unroll
            for (int q = 0; q < LE_PER_THREAD; ++q) {
                const int64_t e = p0 + LE_PER_THREAD * tid + q;
                before[q] = sum;
                sum += e < ev.n ? le_len(lengths[ev.first + e]) : 0;
            }
            const int cur = le_block_scan(s_scan, tid, sum);
            const int64_t mine = carry + s_scan[cur][tid] - sum;                  // 1024 lengths below 2^31 and a carry below 2^31
#pragma unroll
            for (int q = 0; q < LE_PER_THREAD; ++q) {
                const int64_t e = p0 + LE_PER_THREAD * tid + q;
                if (e < ev.n) {
                    start[ev.first + e] = (int32_t)le_sat(mine + before[q]);
                    cls[ev.first + e] = le_class(s_cores, e, p0, ev.n);
                }
            }
            carry = le_sat(carry + s_scan[cur][LE_THREADS - 1]);
            __syncthreads();                                                      // the next piece (or read) restages
        }
    }
}

// a thread's LE_RUN bytes, packed four to a word in sample order
struct le_run_words { uint32_t w[LE_RUN / 4]; };

__device__ inline void le_store_run(uint8_t* out, const le_run_words& v, int valid, int32_t width) {
    if (valid == LE_RUN && width == 16) {
        *reinterpret_cast<uint4*>(out) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    } else if (valid == LE_RUN && width == 8) {
        reinterpret_cast<uint2*>(out)[0] = make_uint2(v.w[0], v.w[1]);
        reinterpret_cast<uint2*>(out)[1] = make_uint2(v.w[2], v.w[3]);
    } else if (valid == LE_RUN && width == 4) {
#pragma unroll
        for (int q = 0; q < LE_RUN / 4; ++q) reinterpret_cast<uint32_t*>(out)[q] = v.w[q];
    } else {
#pragma unroll
        for (int q = 0; q < LE_RUN; ++q)
            if (q < valid) out[q] = (uint8_t)(v.w[q / 4] >> (8 * (q % 4)));
    }
}

__global__ __launch_bounds__(LE_THREADS) void label_expand_kernel(const uint8_t* __restrict__ bases, const int32_t* __restrict__ lengths,
                                                                  const int64_t* __restrict__ event_offsets,
                                                                  const int64_t* __restrict__ sample_offsets, int64_t n_reads,
                                                                  int64_t n_events, int64_t total, const int32_t* __restrict__ start,
                                                                  const uint8_t* __restrict__ cls, uint8_t* __restrict__ labels_out,
                                                                  uint8_t* __restrict__ basemap_out) {
    __shared__ int32_t s_start[LE_TILE_EVENTS + 1];
    __shared__ uint8_t s_cls[LE_TILE_EVENTS];
    __shared__ uint8_t s_base[LE_TILE_EVENTS];
    const int tid = (int)threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t r = le_block_read(sample_offsets, n_reads, b);
    if (r < 0) return;
    const le_tile tile = le_tile_of(b, r, sample_offsets[r], sample_offsets[r + 1], total);
    if (tile.t0 >= tile.t1) return;
    const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
    const int32_t* start_r = start + ev.first;
    const int64_t f = le_first_event(start_r, ev.n, tile.t0);
    const int32_t m = le_staged_events(f, ev.n);
    for (int32_t i = tid; i < m; i += LE_THREADS) {
        s_start[i] = start_r[f + i];
        s_cls[i] = cls[ev.first + f + i];
        s_base[i] = bases[ev.first + f + i];
    }
    if (tid == 0 && m > 0) s_start[m] = le_staged_end(start_r, lengths + ev.first, f, m, ev.n);
    __syncthreads();
    const int64_t j0 = tile.t0 + (int64_t)LE_RUN * tid;
    if (j0 >= tile.t1) return;
    const int valid = tile.t1 - j0 < LE_RUN ? (int)(tile.t1 - j0) : LE_RUN;
    int32_t i = le_staged_first(s_start, m, j0);
    le_run_words lab, map;
#pragma unroll
    for (int q = 0; q < LE_RUN / 4; ++q) lab.w[q] = map.w[q] = 0;
#pragma unroll
    for (int q = 0; q < LE_RUN; ++q) {
        if (q < valid) {
            const int32_t c = le_covering(s_start, m, &i, j0 + q);
            if (c >= 0) {
                lab.w[q / 4] |= (uint32_t)s_cls[c] << (8 * (q % 4));
                map.w[q / 4] |= (uint32_t)le_base_byte(s_start, s_base, c, j0 + q) << (8 * (q % 4));
            }
        }
    }
    uint8_t* lab_at = labels_out + tile.first;
    le_store_run(lab_at + j0, lab, valid, le_store_width(reinterpret_cast<uintptr_t>(lab_at)));
    if (basemap_out) {
        uint8_t* map_at = basemap_out + tile.first;
        le_store_run(map_at + j0, map, valid, le_store_width(reinterpret_cast<uintptr_t>(map_at)));
    }
}

extern "C" int64_t cf_label_events_work_bytes(int64_t n_events) { return le_work_bytes(n_events); }

extern "C" int cf_label_events(cf_model* m, const uint8_t* bases, const int32_t* lengths, const int64_t* event_offsets, const int32_t* clipped,
                               const int64_t* sample_offsets, int64_t n_reads, int64_t n_events, int64_t total, int32_t kmer,
                               uint8_t* labels_out, uint8_t* basemap_out, void* work, int64_t work_bytes, void* stream) {
    switch (le_refusal(n_reads, n_events, total, kmer, work_bytes)) {
        case 0: break;
        case 1: return fail(CF_ERR_INVALID, "cf_label_events: negative size");
        case 2: return fail(CF_ERR_INVALID, "cf_label_events: at most 2^31 - 1 events and samples per call");
        case 3: return fail(CF_ERR_INVALID, "cf_label_events: kmer must be odd and in 1 .. 15");
        case 4: return fail(CF_ERR_INVALID, "cf_label_events: too many reads for one call (reads + samples / 4096 above 2^23)");
        default: return fail(CF_ERR_INVALID, "cf_label_events: the work buffer is smaller than cf_label_events_work_bytes(n_events)");
    }
    if (total == 0) return CF_OK;
    if (!bases || !lengths || !event_offsets || !clipped || !sample_offsets || !labels_out || !work)
        return fail(CF_ERR_INVALID, "cf_label_events: null argument");
    if (n_reads == 0) return fail(CF_ERR_INVALID, "cf_label_events: samples but no reads");
    if (reinterpret_cast<uintptr_t>(work) % 4 != 0) return fail(CF_ERR_INVALID, "cf_label_events: the work buffer must be 4-byte aligned");
    if (m) HIP_TRY(hipSetDevice(m->device));              // NULL: the calling thread's current device
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int32_t* start = static_cast<int32_t*>(work);
    uint8_t* cls = static_cast<uint8_t*>(work) + 4 * n_events;
    const int64_t class_grid = n_reads < LE_CLASS_GRID ? n_reads : LE_CLASS_GRID;
    hipLaunchKernelGGL(label_event_classes_kernel, dim3((unsigned)class_grid), dim3(LE_THREADS), 0, s, bases, lengths, event_offsets, clipped,
                       n_reads, n_events, kmer, start, cls);
    HIP_TRY(hipGetLastError());
    const int64_t expand_grid = n_reads + total / LE_TILE;
    hipLaunchKernelGGL(label_expand_kernel, dim3((unsigned)expand_grid), dim3(LE_THREADS), 0, s, bases, lengths, event_offsets, sample_offsets,
                       n_reads, n_events, total, start, cls, labels_out, basemap_out);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
