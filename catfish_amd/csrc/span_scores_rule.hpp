// Per-call scores of homopolymer calls: every rule by which span_scores_kernel (csrc/span_scores.hpp) forms a global-memory index
// (plain C++17: g++ and hipcc both compile it; under hipcc the functions are __host__ __device__).  catfish_amd/span_scores.py
// states the result in numpy (span_scores_host is the definition); tests/native/span_scores_replay.cpp states the kernel's body
// serially over these functions and runs under the sanitizers with buffers of exactly the sizes the Python layer allocates.
//
// A run is walked from its start, 64 samples a step, for as long as p >= threshold holds and the real part of its read lasts.  The
// starts come from device memory that a caller may have filled with anything: ss_open vouches for a start before anything is loaded
// at it, and the walk never leaves [start, real end) -- a subset of [0, total) whatever the read table holds.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SS_FN __host__ __device__ inline
#else
#define SS_FN inline
#endif

#define SS_STEP 64                 // samples per step of the walk: one per lane

// The largest r in [0, n_reads) with read_offsets[r] <= start, or -1 (no read, or start lies before the first one).  Reads
// read_offsets[0 .. n_reads - 1] only, whatever the table holds.
SS_FN int64_t ss_owner(const int64_t* read_offsets, int64_t n_reads, int64_t start) {
    if (n_reads <= 0 || read_offsets[0] > start) return -1;
    int64_t lo = 0, hi = n_reads;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (read_offsets[mid] <= start) lo = mid; else hi = mid;
    }
    return lo;
}

// One past the last real sample of read r: min(read_offsets[r] + read_lengths[r], read_offsets[r + 1], total), formed without
// overflow for any table (a negative offset or length gives an empty read).  read_offsets has n_reads + 1 entries.
SS_FN int64_t ss_real_end(const int64_t* read_offsets, const int64_t* read_lengths, int64_t total, int64_t r) {
    const int64_t beg = read_offsets[r], len = read_lengths[r], next = read_offsets[r + 1];
    if (beg < 0 || beg >= total || len <= 0) return beg;
    int64_t end = len > total - beg ? total : beg + len;
    if (next < end) end = next;
    return end;
}

// Where the walk of the run at `start` may go: [start, end) with 0 <= start < end <= total, or nothing.
struct ss_walk { int64_t read, end; bool open; };

SS_FN ss_walk ss_open(const int64_t* read_offsets, const int64_t* read_lengths, int64_t n_reads, int64_t total, int64_t start) {
    ss_walk w = {-1, start, false};
    if (start < 0 || start >= total) return w;                                  // never dereferenced
    w.read = ss_owner(read_offsets, n_reads, start);
    if (w.read < 0) return w;
    const int64_t end = ss_real_end(read_offsets, read_lengths, total, w.read);
    if (end <= start) return w;                                                 // padding, or no real part at all
    w.end = end;
    w.open = true;
    return w;
}

// One step: bit b of `hit` says p[pos + b] >= threshold, `left` > 0 samples of the read's real part remain from pos on (lanes at or
// past `left` load nothing; their bits are ignored).  take = how many leading samples belong to the run; go_on = all 64 did and
// the read has more.
struct ss_taken { int take; bool go_on; };

SS_FN ss_taken ss_step(uint64_t hit, int64_t left) {
    const uint64_t real = left >= SS_STEP ? ~0ull : (1ull << left) - 1ull;     // 0 < left < 64: no shift by 64
    const uint64_t miss = ~(hit & real);
    const int take = miss ? __builtin_ctzll(miss) : SS_STEP;                    // no count of trailing zeros is taken of 0
    return {take, take == SS_STEP && left > SS_STEP};
}

// rows: sums [max_runs][3] = sum p, sum x, sum x * x; extremes [max_runs][2] = min p, max p
SS_FN int64_t ss_sum_index(int64_t k, int which) { return 3 * k + which; }
SS_FN int64_t ss_extreme_index(int64_t k, int which) { return 2 * k + which; }

// how many rows a call writes: min(counts[0], max_runs)
SS_FN int64_t ss_rows(uint64_t count, int64_t max_runs) {
    if (max_runs <= 0) return 0;
    return count < (uint64_t)max_runs ? (int64_t)count : max_runs;
}
