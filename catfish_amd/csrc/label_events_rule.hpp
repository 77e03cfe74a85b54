// Labels from event tables: every rule by which label_event_classes_kernel and label_expand_kernel (csrc/label_events.hpp) form a
// global-memory or LDS index (plain C++17: g++ and hipcc both compile it; under hipcc the functions are __host__ __device__).
// catfish_amd/labelling.py states the result in numpy (event_classes_host, expand_events_host and base_map_host are the definitions);
// tests/native/label_events_replay.cpp runs the kernels' bodies serially over these functions under the sanitizers, with buffers of
// exactly the sizes the Python layer allocates.
//
// Layout: read r owns events event_offsets[r] .. event_offsets[r + 1] of `bases` (uint8) and `lengths` (int32) and samples
// sample_offsets[r] .. sample_offsets[r + 1] of the outputs; clipped[2 r], clipped[2 r + 1] are its clipped_start / clipped_end.
// The work buffer holds, per event, its first sample relative to the read (int32 [n_events]) and behind those its class (uint8
// [n_events]).  All five tables live in device memory that a caller may have filled with anything, and `lengths` decide where labels
// go, so nothing here trusts them:
//   - a read whose event range is not inside [0, n_events] has no events (le_events_sound); a read whose sample range is not inside
//     [0, total] is not written at all (le_samples_sound);
//   - a length < 1 contributes nothing (le_len), and the running sum saturates at LE_SAT instead of wrapping (le_sat), so the starts
//     of a read ascend whatever the lengths hold;
//   - a sample is labelled by an event only when that event's [start, end) holds it AND the sample lies inside the tile, which lies
//     inside the read; samples no event covers get label 0 and base 0;
//   - a function that cannot vouch for an index returns -1 ("skip").
// Reads whose event ranges OVERLAP share entries of the work buffer: their labels are then some read's classes at some read's
// starts -- still zeros and ones inside the buffers, but not the definition.  A tile that meets more than LE_TILE_EVENTS events (only
// possible with lengths < 1) labels the samples behind the last staged event 0.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LE_FN __host__ __device__ inline
#else
#define LE_FN inline
#endif

#define LE_THREADS 256
#define LE_PIECE 1024                    // events per piece of the class kernel: four per thread
#define LE_PER_THREAD (LE_PIECE / LE_THREADS)
#define LE_MAX_KMER 15
#define LE_WIDEN 2                       // extend_classification: two events each way
#define LE_HALO (LE_MAX_KMER / 2 + LE_WIDEN)      // bases staged around a piece: 9 each side
#define LE_BASES_SLOTS (LE_PIECE + 2 * LE_HALO)
#define LE_CORE_SLOTS (LE_PIECE + 2 * LE_WIDEN)
#define LE_TILE 4096                     // CF_LABEL_TILE: samples per workgroup of the expand kernel, sixteen per thread
#define LE_RUN (LE_TILE / LE_THREADS)
#define LE_TILE_EVENTS (LE_TILE + 1)     // every event has at least one sample: a tile meets at most this many
#define LE_SAT 0x7fffffffLL              // where a running sum of lengths stops
#define LE_MAX_COUNT 0x7fffffffLL        // events, samples per call (below 2^31)
#define LE_MAX_BLOCKS (1LL << 23)        // workgroups of one launch
#define LE_CLASS_GRID 4096               // workgroups of the class kernel; they stride over the reads

// 0 when a call with these host arguments may launch; else which rule they break (the entry point answers CF_ERR_INVALID)
LE_FN int le_refusal(int64_t n_reads, int64_t n_events, int64_t total, int32_t kmer, int64_t work_bytes) {
    if (n_reads < 0 || n_events < 0 || total < 0) return 1;
    if (n_events > LE_MAX_COUNT || total > LE_MAX_COUNT) return 2;
    if (kmer < 1 || kmer > LE_MAX_KMER || kmer % 2 == 0) return 3;
    if (n_reads + total / LE_TILE > LE_MAX_BLOCKS) return 4;
    if (work_bytes < 5 * n_events) return 5;
    return 0;
}

// bytes of the work buffer: int32 start [n_events], uint8 class [n_events], rounded up to 16 (never 0)
LE_FN int64_t le_work_bytes(int64_t n_events) {
    if (n_events < 0 || n_events > LE_MAX_COUNT) return -1;
    const int64_t raw = 5 * n_events;
    return raw < 16 ? 16 : (raw + 15) / 16 * 16;
}

LE_FN int64_t le_len(int32_t length) { return length < 1 ? 0 : (int64_t)length; }
LE_FN int64_t le_sat(int64_t sum) { return sum > LE_SAT ? LE_SAT : sum; }      // sum >= 0 and far below 2^63

// read r's events: first = e0, count = n (0 when the table's entries are not what the layout promises)
struct le_events { int64_t first, n; };
LE_FN le_events le_events_sound(int64_t e0, int64_t e1, int64_t n_events) {
    le_events ev = {0, 0};
    if (e0 < 0 || e0 > e1 || e1 > n_events) return ev;
    ev.first = e0;
    ev.n = e1 - e0;
    return ev;
}

// read r's samples: first = s0, count = n, or n = -1: the read is not written
struct le_samples { int64_t first, n; };
LE_FN le_samples le_samples_sound(int64_t s0, int64_t s1, int64_t total) {
    le_samples sm = {0, -1};
    if (s0 < 0 || s0 > s1 || s1 > total) return sm;
    sm.first = s0;
    sm.n = s1 - s0;
    return sm;
}

// ---------------------------------------------------------------------------------------------------------------- the class kernel
// LDS slot of event e (relative to the read, any value) among the bases staged for the piece that begins at p0, or -1
LE_FN int32_t le_base_slot(int64_t e, int64_t p0, int64_t n) {
    if (e < 0 || e >= n) return -1;
    const int64_t slot = e - p0 + LE_HALO;
    return (slot < 0 || slot >= LE_BASES_SLOTS) ? -1 : (int32_t)slot;
}
// ... and among the piece's core flags (the piece and LE_WIDEN events each side)
LE_FN int32_t le_core_slot(int64_t e, int64_t p0, int64_t n) {
    if (e < 0 || e >= n) return -1;
    const int64_t slot = e - p0 + LE_WIDEN;
    return (slot < 0 || slot >= LE_CORE_SLOTS) ? -1 : (int32_t)slot;
}

// core[e]: the k-mer centred on event e lies inside the read and outside the clipped ends, and is k times one byte that is not 'N'.
// `staged` are the piece's LE_BASES_SLOTS bytes.  A k-mer that reaches outside what is staged cannot be vouched for: 0.
LE_FN uint8_t le_core(const uint8_t* staged, int64_t e, int64_t p0, int64_t n, int64_t cs, int64_t ce, int32_t kmer) {
    const int32_t oh = kmer / 2;
    if (e < cs || e >= n - ce || e - oh < 0 || e + oh >= n) return 0;
    const int32_t mid = le_base_slot(e, p0, n);
    if (mid < 0 || mid - oh < 0 || mid + oh >= LE_BASES_SLOTS) return 0;
    const uint8_t b = staged[mid];
    if (b == (uint8_t)'N') return 0;
    for (int32_t d = 1; d <= oh; ++d)
        if (staged[mid - d] != b || staged[mid + d] != b) return 0;
    return 1;
}

// cls[e]: some core within LE_WIDEN events of e, inside the read.  `cores` are the piece's LE_CORE_SLOTS flags.
LE_FN uint8_t le_class(const uint8_t* cores, int64_t e, int64_t p0, int64_t n) {
    uint8_t any = 0;
    for (int32_t d = -LE_WIDEN; d <= LE_WIDEN; ++d) {
        const int32_t slot = le_core_slot(e + d, p0, n);
        if (slot >= 0) any |= cores[slot];
    }
    return any;
}

// ---------------------------------------------------------------------------------------------------------------- the expand kernel
// Workgroup b of the expand grid (n_reads + total / LE_TILE workgroups) -> its read and tile.  Read r's tiles are the workgroups
// key(r) .. key(r) + tiles(r) - 1 with key(r) = sample_offsets[r] / LE_TILE + r: ascending offsets give strictly ascending keys
// that are at least tiles(r) apart, so every tile of every read has exactly one workgroup and the others idle.
LE_FN int64_t le_key(int64_t offset, int64_t r) { return (offset >= 0 ? offset / LE_TILE : -1) + r; }
// the largest r in [0, n_reads) with key(r) <= b, or -1; reads sample_offsets[0 .. n_reads - 1] only
LE_FN int64_t le_block_read(const int64_t* sample_offsets, int64_t n_reads, int64_t b) {
    int64_t lo = 0, hi = n_reads;
    if (hi <= lo || le_key(sample_offsets[lo], lo) > b) return -1;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (le_key(sample_offsets[mid], mid) <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// samples [t0, t1) of the read (relative to it) that workgroup b writes; t0 == t1: nothing
struct le_tile { int64_t first, t0, t1; };       // first: the read's first sample in the outputs
LE_FN le_tile le_tile_of(int64_t b, int64_t r, int64_t s0, int64_t s1, int64_t total) {
    le_tile t = {0, 0, 0};
    const le_samples sm = le_samples_sound(s0, s1, total);
    if (r < 0 || sm.n <= 0) return t;
    const int64_t j = b - le_key(s0, r);
    if (j < 0 || j > sm.n / LE_TILE) return t;                                  // (j * LE_TILE stays far below 2^63)
    const int64_t t0 = j * LE_TILE;
    if (t0 >= sm.n) return t;
    t.first = sm.first;
    t.t0 = t0;
    t.t1 = t0 + LE_TILE < sm.n ? t0 + LE_TILE : sm.n;
    return t;
}

// The largest e in [0, n) with start[e] <= t, or -1 (no events, or the first one starts beyond t).  `start` ascends (the class kernel
// wrote it from le_len and le_sat); where it does not, some event in range comes back all the same.
LE_FN int64_t le_first_event(const int32_t* start, int64_t n, int64_t t) {
    int64_t lo = 0, hi = n;
    if (hi <= lo || (int64_t)start[lo] > t) return -1;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)start[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// how many events the tile stages from event f on: at most LE_TILE_EVENTS, never past the read's last
LE_FN int32_t le_staged_events(int64_t f, int64_t n) {
    if (f < 0 || f >= n) return 0;
    return (int32_t)(n - f < LE_TILE_EVENTS ? n - f : LE_TILE_EVENTS);
}
// the end of the last staged event, f + m - 1: the next event's start, or start + length for the read's last event
LE_FN int32_t le_staged_end(const int32_t* start, const int32_t* lengths, int64_t f, int32_t m, int64_t n) {
    const int64_t last = f + m - 1;
    if (last + 1 < n) return start[last + 1];
    return (int32_t)le_sat((int64_t)start[last] + le_len(lengths[last]));
}

// Sample j of the read against the staged starts s[0 .. m] (s[m] = le_staged_end): the staged event that holds it, searching on from
// event i (the caller's last answer, or le_staged_first), or -1 when none does.  *i moves forward only.
LE_FN int32_t le_staged_first(const int32_t* s, int32_t m, int64_t j) {
    int32_t lo = 0, hi = m;
    if (hi <= lo || (int64_t)s[lo] > j) return -1;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)s[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}
LE_FN int32_t le_covering(const int32_t* s, int32_t m, int32_t* i, int64_t j) {
    if (*i < 0 || *i >= m) return -1;
    while (*i + 1 < m && (int64_t)s[*i + 1] <= j) ++*i;
    return ((int64_t)s[*i] <= j && j < (int64_t)s[*i + 1]) ? *i : -1;
}
// the base-map byte of sample j inside staged event i: the base, bit 7 set on the event's middle sample start + length / 2
LE_FN uint8_t le_base_byte(const int32_t* s, const uint8_t* bases, int32_t i, int64_t j) {
    const int64_t a = s[i], len = (int64_t)s[i + 1] - a;
    return (uint8_t)(bases[i] | (j == a + len / 2 ? 0x80 : 0));
}

// how many bytes one store of the outputs may carry: 16, 8, 4 or 1, by the address of the tile's first sample (a tile begins a whole
// number of LE_RUN = 16 samples into its read, so the read's first sample decides for all its tiles)
LE_FN int32_t le_store_width(uint64_t address) {
    return address % 16 == 0 ? 16 : address % 8 == 0 ? 8 : address % 4 == 0 ? 4 : 1;
}
