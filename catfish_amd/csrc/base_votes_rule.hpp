// Per-base calls: every rule by which base_votes_vote_kernel and base_votes_count_kernel (csrc/base_votes.hpp) form a global-memory
// or LDS index, and the fixed-point arithmetic of the vote (plain C++17: g++ and hipcc both compile it; under hipcc the functions are
// __host__ __device__).  catfish_amd/base_votes.py states the result in numpy (vote_host is the definition);
// tests/native/base_votes_replay.cpp runs both kernels' bodies serially over these functions under the sanitizers, with buffers of
// exactly the sizes the Python layer allocates.
//
// Layout: base e of the set owns samples edges[e] .. edges[e + 1] - 1 of the set's concatenated arrays (`labels`, `basemap`, uint8
// [set_total]).  Stretch r of a round is length[r] samples from sample src_first[r] of the set, packed at bounds[r] of `probs` (float
// [total]); ranges[r] .. ranges[n + r] - 1 are the bases that lie wholly inside it (the host's searchsorted).  The work buffer
// (bv_work_bytes) holds sums uint64 [n_bases] and behind them state uint8 [K][n_bases].
//
// All tables live in device memory that a caller may have filled with anything, so nothing here trusts them:
//   - a stretch's base range is clamped to [0, n_bases] (bv_clamp);
//   - a base is voted only when src <= edges[e] < edges[e + 1] <= src + length for its stretch, its samples lie inside the set and
//     their packed places inside [0, total) (bv_span); any other base is unvoted: nothing is read for it, its sum and states stay 0,
//     it breaks runs and is counted nowhere;
//   - the count asks the same of every base again, for ITS stretch (bv_state_of): a base another stretch voted is no base of this
//     one; a run is walked inside its stretch's clamped range only (bv_run_cell).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BV_FN __host__ __device__ inline
#else
#define BV_FN inline
#endif

#define BV_THREADS 256
#define BV_MAX_K 16                      // thresholds per call
#define BV_MAX_BASES 32                  // the most length bins in bases
#define BV_CLASSES 5                     // A C G T other
#define BV_CONF_CELLS (BV_CLASSES * 4)   // one threshold's confusion table: class, truth, called
#define BV_MAX_COUNT 0x7fffffffLL        // bases, samples per call (below 2^31)
#define BV_LONG_BASE 256                 // a base of more samples than this is summed by its whole wave (any value gives the same bits)
#define BV_GRID_X 1024                   // workgroups along a stretch's bases, at most; they stride
#define BV_GRID_Y 65535                  // ... and over the stretches
#define BV_WALK 4                        // bases a run walk loads at a time (at 6 and 8 the count kernel spills scalar registers)
#define BV_COUNT_BLOCKS 8192             // workgroups of the count launch, about: each ends in one atomic per non-zero cell of its table

#define BV_CALLED 0x01u
#define BV_TRUTH 0x02u
#define BV_VOTED 0x80u

// q(p): NaN or p < 0 -> 0, p > 1 -> 2^32, else floor(double(p) * 2^32) (the product is exact: a power of two)
BV_FN uint64_t bv_q(float p) {
    if (!(p >= 0.0f)) return 0;
    if (p > 1.0f) return 1ull << 32;
    return (uint64_t)((double)p * 4294967296.0);
}

// 0 when a call with these host arguments may launch; else which rule they break (the entry point answers CF_ERR_INVALID)
BV_FN int bv_refusal(int64_t n, int64_t total, int64_t n_bases, int64_t set_total, int32_t n_thresholds, int32_t max_bases, int64_t work_bytes) {
    if (n < 0 || total < 0 || n_bases < 0 || set_total < 0) return 1;
    if (n > BV_MAX_COUNT || total > BV_MAX_COUNT || n_bases > BV_MAX_COUNT || set_total > BV_MAX_COUNT) return 2;
    if (n_thresholds < 1 || n_thresholds > BV_MAX_K) return 3;
    if (max_bases < 1 || max_bases > BV_MAX_BASES) return 4;
    if (work_bytes < (8 + (int64_t)n_thresholds) * n_bases) return 5;
    return 0;
}

// bytes of the work buffer: uint64 sums [n_bases], uint8 state [K][n_bases], rounded up to 16 (never 0); -1 for sizes no call takes
BV_FN int64_t bv_work_bytes(int64_t n_bases, int32_t n_thresholds) {
    if (n_bases < 0 || n_bases > BV_MAX_COUNT || n_thresholds < 1 || n_thresholds > BV_MAX_K) return -1;
    const int64_t raw = (8 + (int64_t)n_thresholds) * n_bases;
    return raw < 16 ? 16 : (raw + 15) / 16 * 16;
}
BV_FN int64_t bv_work_state(int64_t n_bases) { return 8 * n_bases; }          // where the states begin in it, in bytes

BV_FN int64_t bv_clamp(int64_t e, int64_t n_bases) { return e < 0 ? 0 : (e > n_bases ? n_bases : e); }
// cells of one threshold's run table: [2][3][BV_CLASSES][max_bases + 1]
BV_FN int bv_run_cells(int max_bases) { return 2 * 3 * BV_CLASSES * (max_bases + 1); }

// The samples of base e when stretch (src, len, bound) votes it, else 0: *s0 its first sample in the set, *p0 that sample's packed place.
BV_FN int64_t bv_span(const int64_t* edges, int64_t n_bases, int64_t e, int64_t src, int64_t len, int64_t bound, int64_t total,
                      int64_t set_total, int64_t* s0, int64_t* p0) {
    if (e < 0 || e >= n_bases) return 0;
    if (src < 0 || len < 0 || bound < 0 || src > BV_MAX_COUNT || len > BV_MAX_COUNT || bound > BV_MAX_COUNT) return 0;
    const int64_t first = edges[e], end = edges[e + 1];
    if (first < src || end <= first || end > src + len || end > set_total) return 0;
    const int64_t at = bound + (first - src);                 // (no overflow: every term is below 2^32)
    if (at + (end - first) > total) return 0;
    *s0 = first;
    *p0 = at;
    return end - first;
}

// the class of a base byte (bit 7 already masked off): 0..3 for upper-case A C G T, 4 for anything else
BV_FN unsigned bv_class(unsigned byte) { return byte == 'A' ? 0u : byte == 'C' ? 1u : byte == 'G' ? 2u : byte == 'T' ? 3u : 4u; }
BV_FN uint8_t bv_state(bool called, bool truth, unsigned cls) {
    return (uint8_t)(BV_VOTED | (called ? BV_CALLED : 0u) | (truth ? BV_TRUTH : 0u) | (cls << 2));
}
BV_FN unsigned bv_state_class(unsigned st) { return (st >> 2) & 7u; }
// cell of a voted base in one threshold's [BV_CLASSES][2][2] confusion table (class, truth, called), or -1
BV_FN int bv_conf_cell(unsigned st) {
    if (!(st & BV_VOTED) || bv_state_class(st) >= BV_CLASSES) return -1;
    return (int)(bv_state_class(st) * 4u + ((st & BV_TRUTH) ? 2u : 0u) + ((st & BV_CALLED) ? 1u : 0u));
}

// bv_span's test folded into one window of the set's samples: the stretch votes base e when lo <= edges[e] < edges[e + 1] <= hi
// (hi = the least of the stretch's end, the set's end and the sample whose packed place is `total`; an unsound stretch has lo > hi)
struct bv_stretch {
    int64_t lo, hi;
};
BV_FN bv_stretch bv_window(int64_t src, int64_t len, int64_t bound, int64_t total, int64_t set_total) {
    if (src < 0 || len < 0 || bound < 0 || src > BV_MAX_COUNT || len > BV_MAX_COUNT || bound > BV_MAX_COUNT) return bv_stretch{1, 0};
    int64_t hi = src + len;
    if (set_total < hi) hi = set_total;
    if (total - bound + src < hi) hi = total - bound + src;
    return bv_stretch{src, hi};
}
// the state byte of base e as ITS stretch sees it: what the vote wrote when this stretch votes the base, else 0
BV_FN unsigned bv_state_of(const uint8_t* state_k, const int64_t* edges, int64_t n_bases, int64_t e, const bv_stretch& s) {
    if (e < 0 || e >= n_bases) return 0u;
    const int64_t first = edges[e], end = edges[e + 1];
    return first >= s.lo && end > first && end <= s.hi ? state_k[e] : 0u;
}

// The run of kind `kind` (0: truth judged against called, 1: called judged against truth) that STARTS at base e of a stretch whose
// clamped range is [a, b): its cell in one threshold's [2][3][BV_CLASSES][max_bases + 1] table, or -1 when no run starts at e.
// `state_k` is that threshold's uint8 [n_bases] row and `first` bv_state_of(e); a, b are clamped by the caller, so every index is in
// the row.
BV_FN int bv_run_cell(const uint8_t* state_k, const int64_t* edges, int64_t n_bases, const bv_stretch& s, unsigned first, int64_t e, int64_t a,
                      int64_t b, int kind, int max_bases) {
    const unsigned mine = kind == 0 ? BV_TRUTH : BV_CALLED, other = kind == 0 ? BV_CALLED : BV_TRUTH;
    if (e < a || e >= b) return -1;
    if ((first & (BV_VOTED | mine)) != (BV_VOTED | mine)) return -1;
    if (e > a && (bv_state_of(state_k, edges, n_bases, e - 1, s) & (BV_VOTED | mine)) == (BV_VOTED | mine)) return -1;   // the run began earlier
    int64_t count = 0, with_other = 0;
    unsigned cls = bv_state_class(first);
    bool open = true;
    for (int64_t i0 = e; open && i0 < b; i0 += BV_WALK) {      // BV_WALK bases at a time: their loads do not wait for one another
        unsigned st[BV_WALK];
        for (int j = 0; j < BV_WALK; ++j) st[j] = i0 + j < b ? bv_state_of(state_k, edges, n_bases, i0 + j, s) : 0u;
        for (int j = 0; j < BV_WALK; ++j) {                     // (no branch: what lies behind the run's end adds nothing)
            open = open && (st[j] & (BV_VOTED | mine)) == (BV_VOTED | mine);
            count += open ? 1 : 0;
            with_other += open && (st[j] & other) ? 1 : 0;
            cls = open && bv_state_class(st[j]) != cls ? BV_CLASSES - 1 : cls;
        }
    }
    if (cls >= BV_CLASSES) cls = BV_CLASSES - 1;
    const int state = with_other == count ? 0 : (with_other == 0 ? 2 : 1);      // RUN_STATES: complete, incomplete, absent
    const int bin = count < max_bases ? (int)count : max_bases;
    return ((kind * 3 + state) * BV_CLASSES + (int)cls) * (max_bases + 1) + bin;
}
