// Per-base calls: the samples of every base of a round's stretches vote on it (the step the reference's networks/correct_output.py
// correct_events sketches: "majority voting by measurements belong to that event"), and the voted bases are scored by base.
// catfish_amd/base_votes.py states the result in numpy -- vote_host is normative; integer sums and counts only, so the kernels equal
// it bit for bit whatever the grid.  The index and arithmetic rules are plain C++ in base_votes_rule.hpp (read that first);
// tests/native/base_votes_replay.cpp states both kernels' bodies serially over them under the sanitizers.
//
// Launch A, base_votes_vote_kernel: blockIdx.y strides over the stretches, blockIdx.x over a stretch's bases, one lane per base.
// Neighbouring lanes own neighbouring segments of `probs`, so a wave reads one contiguous span.  A lane sums q(p) over its base's
// samples in uint64; a base of more than `long_base` samples is left to the whole wave (ballot, broadcast of its span, strided
// loads, a shuffle reduction).  All K thresholds are judged from the one sum: called_k = S >= q(t_k) * n.  The lane writes its sum
// and its K state bytes.
//
// Launch B, base_votes_count_kernel: the same grid with blockIdx.z over the thresholds.  A lane takes its base's state only when its
// own stretch votes the base (bv_state_of: the vote's test again).  Every voted base adds to the confusion
// table: the lanes of a wave that hold the same cell are counted with ballots and one lane adds their number to the workgroup's LDS
// table.  A lane whose base starts a run walks it (bv_run_cell: inside the stretch's range only) and adds one to the run's cell.
// The LDS table goes to the zeroed outputs with one 64-bit integer atomic per non-zero cell.  No float atomics anywhere.
#pragma once
#include "base_votes_rule.hpp"

struct bv_thresholds {
    unsigned long long q[BV_MAX_K];      // q(float32(t_k))
};

__global__ __launch_bounds__(BV_THREADS) void base_votes_vote_kernel(const float* __restrict__ probs, int64_t total,
                                                                     const uint8_t* __restrict__ labels, const uint8_t* __restrict__ basemap,
                                                                     int64_t set_total, const int64_t* __restrict__ edges, int64_t n_bases,
                                                                     const int64_t* __restrict__ src_first, const int64_t* __restrict__ length,
                                                                     const int64_t* __restrict__ bounds, const int64_t* __restrict__ ranges,
                                                                     int64_t n, int K, int64_t long_base, bv_thresholds qt,
                                                                     unsigned long long* __restrict__ sums, uint8_t* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = blockIdx.y; r < n; r += gridDim.y) {
        const int64_t a = bv_clamp(ranges[r], n_bases), b = bv_clamp(ranges[n + r], n_bases);
        if (b <= a) continue;                                                      // (uniform)
        const int64_t src = src_first[r], len = length[r], bound = bounds[r];
        for (int64_t e0 = a + (int64_t)blockIdx.x * BV_THREADS; e0 < b; e0 += (int64_t)gridDim.x * BV_THREADS) {      // (uniform)
            const int64_t e = e0 + threadIdx.x;
            int64_t s0 = 0, p0 = 0;
            const int64_t mine = e < b ? bv_span(edges, n_bases, e, src, len, bound, total, set_total, &s0, &p0) : 0;
            unsigned long long sum = 0;
            if (mine <= long_base)
                for (int64_t i = 0; i < mine; ++i) sum += bv_q(probs[p0 + i]);
            unsigned long long longs = __ballot(mine > long_base);
            while (longs) {                                                        // (uniform) the wave sums its long bases together
                const int owner = __ffsll((long long)longs) - 1;
                longs &= longs - 1;
                const int64_t at = (int64_t)__shfl((unsigned long long)p0, owner), count = (int64_t)__shfl((unsigned long long)mine, owner);
                unsigned long long part = 0;
                for (int64_t i = lane; i < count; i += 64) part += bv_q(probs[at + i]);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
                if (lane == owner) sum = part;
            }
            if (mine > 0) {
                sums[e] = sum;
                const bool truth = labels[s0] == 1u;
                const unsigned cls = bv_class(basemap[s0] & 0x7fu);
                for (int k = 0; k < K; ++k)
                    state[(int64_t)k * n_bases + e] = bv_state(sum >= qt.q[k] * (unsigned long long)mine, truth, cls);
            }
        }
    }
}

__global__ __launch_bounds__(BV_THREADS) void base_votes_count_kernel(const uint8_t* __restrict__ state, const int64_t* __restrict__ edges,
                                                                      int64_t n_bases, const int64_t* __restrict__ src_first,
                                                                      const int64_t* __restrict__ length, const int64_t* __restrict__ bounds,
                                                                      int64_t total, int64_t set_total, const int64_t* __restrict__ ranges,
                                                                      int64_t n, int K, int max_bases,
                                                                      unsigned long long* __restrict__ confusion_out,
                                                                      unsigned long long* __restrict__ runs_out) {
    __shared__ unsigned s_tab[BV_CONF_CELLS + 2 * 3 * BV_CLASSES * (BV_MAX_BASES + 1)];
    const int lane = threadIdx.x & 63;
    const int run_cells = bv_run_cells(max_bases), cells = BV_CONF_CELLS + run_cells;
    for (int k = blockIdx.z; k < K; k += gridDim.z) {
        const uint8_t* __restrict__ state_k = state + (int64_t)k * n_bases;
        for (int c = threadIdx.x; c < cells; c += BV_THREADS) s_tab[c] = 0u;
        __syncthreads();
        for (int64_t r = blockIdx.y; r < n; r += gridDim.y) {
            const int64_t a = bv_clamp(ranges[r], n_bases), b = bv_clamp(ranges[n + r], n_bases);
            if (b <= a) continue;                                                  // (uniform)
            const bv_stretch s = bv_window(src_first[r], length[r], bounds[r], total, set_total);
            for (int64_t e0 = a + (int64_t)blockIdx.x * BV_THREADS; e0 < b; e0 += (int64_t)gridDim.x * BV_THREADS) {  // (uniform)
                const int64_t e = e0 + threadIdx.x;
                const unsigned st = e < b ? bv_state_of(state_k, edges, n_bases, e, s) : 0u;
                const int cell = bv_conf_cell(st);
                unsigned long long open = __ballot(cell >= 0);
                while (open) {                                                     // (uniform) one LDS add per cell the wave holds
                    const int leader = __ffsll((long long)open) - 1;
                    const int theirs = __shfl(cell, leader);
                    const unsigned long long same = __ballot(cell == theirs);
                    if (lane == leader) atomicAdd(&s_tab[theirs], (unsigned)__popcll(same));
                    open &= ~same;
                }
                if (st & BV_VOTED) {
#pragma unroll 1
                    for (int kind = 0; kind < 2; ++kind) {
                        const int run = bv_run_cell(state_k, edges, n_bases, s, st, e, a, b, kind, max_bases);
                        if (run >= 0) atomicAdd(&s_tab[BV_CONF_CELLS + run], 1u);
                    }
                }
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += BV_THREADS) {
            const unsigned v = s_tab[c];
            if (v == 0u) continue;
            if (c < BV_CONF_CELLS) atomicAdd(&confusion_out[(int64_t)k * BV_CONF_CELLS + c], (unsigned long long)v);
            else atomicAdd(&runs_out[(int64_t)k * run_cells + (c - BV_CONF_CELLS)], (unsigned long long)v);
        }
        __syncthreads();
    }
}

extern "C" int64_t cf_base_votes_work_bytes(int64_t n_bases, int32_t n_thresholds) { return bv_work_bytes(n_bases, n_thresholds); }

extern "C" int cf_base_votes(cf_model* m, const float* probs, int64_t total, const uint8_t* labels, const uint8_t* basemap, int64_t set_total,
                             const int64_t* edges, int64_t n_bases, const int64_t* src_first, const int64_t* length, const int64_t* bounds,
                             const int64_t* ranges, int64_t n, int64_t longest_range, const double* thresholds, int32_t n_thresholds,
                             int32_t max_bases, int64_t* confusion_out, int64_t* runs_out, void* work, int64_t work_bytes, void* stream) {
    const std::string fn = "cf_base_votes";
    if (!probs || !labels || !basemap || !edges || !src_first || !length || !bounds || !ranges || !thresholds || !confusion_out || !runs_out || !work)
        return fail(CF_ERR_INVALID, fn + ": null argument");
    switch (bv_refusal(n, total, n_bases, set_total, n_thresholds, max_bases, work_bytes)) {
        case 0: break;
        case 1: return fail(CF_ERR_INVALID, fn + ": negative size");
        case 2: return fail(CF_ERR_INVALID, fn + ": 2^31 or more stretches, samples or bases");
        case 3: return fail(CF_ERR_INVALID, fn + ": n_thresholds must be in 1 .. " + std::to_string(BV_MAX_K));
        case 4: return fail(CF_ERR_INVALID, fn + ": max_bases must be in 1 .. " + std::to_string(BV_MAX_BASES));
        default: return fail(CF_ERR_INVALID, fn + ": work buffer too small (cf_base_votes_work_bytes)");
    }
    bv_thresholds qt = {};
    for (int k = 0; k < n_thresholds; ++k) qt.q[k] = bv_q((float)thresholds[k]);
    int64_t long_base = BV_LONG_BASE;
    if (const char* v = cf_knob("CATFISH_BASE_VOTES_LONG")) long_base = atoll(v);                // A/B only: the sums are integers
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int run_cells = bv_run_cells(max_bases);
    HIP_TRY(hipMemsetAsync(confusion_out, 0, (size_t)n_thresholds * BV_CONF_CELLS * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(runs_out, 0, (size_t)n_thresholds * run_cells * sizeof(int64_t), s));
    if (n_bases > 0) HIP_TRY(hipMemsetAsync(work, 0, (size_t)(8 + n_thresholds) * (size_t)n_bases, s));
    if (n == 0 || n_bases == 0 || total == 0 || set_total == 0) return CF_OK;                  // nothing can be voted: the zeroed tables
    unsigned long long* sums = static_cast<unsigned long long*>(work);
    uint8_t* state = static_cast<uint8_t*>(work) + bv_work_state(n_bases);
    const int64_t widest = longest_range < 1 ? 1 : (longest_range > n_bases ? n_bases : longest_range);     // (a hint: the workgroups stride)
    const unsigned gx = (unsigned)std::min<int64_t>((widest + BV_THREADS - 1) / BV_THREADS, BV_GRID_X);
    const unsigned gy = (unsigned)std::min<int64_t>(n, BV_GRID_Y);
    hipLaunchKernelGGL(base_votes_vote_kernel, dim3(gx, gy), dim3(BV_THREADS), 0, s, probs, total, labels, basemap, set_total, edges, n_bases,
                       src_first, length, bounds, ranges, n, (int)n_thresholds, long_base, qt, sums, state);
    HIP_TRY(hipGetLastError());
    // the count's workgroups stride over more stretches each: fewer tables to flush (measured: profiles/base_votes_bench.jsonl)
    int64_t count_blocks = BV_COUNT_BLOCKS;
    if (const char* v = cf_knob("CATFISH_BASE_VOTES_COUNT_BLOCKS")) count_blocks = atoll(v);  // A/B only: the counts are integers
    const unsigned gy_count = (unsigned)std::min<int64_t>(gy, std::max<int64_t>(1, count_blocks / ((int64_t)gx * n_thresholds)));
    hipLaunchKernelGGL(base_votes_count_kernel, dim3(gx, gy_count, (unsigned)n_thresholds), dim3(BV_THREADS), 0, s, state, edges, n_bases, src_first,
                       length, bounds, total, set_total, ranges, n, (int)n_thresholds, (int)max_bases, reinterpret_cast<unsigned long long*>(confusion_out),
                       reinterpret_cast<unsigned long long*>(runs_out));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
