// Training set from labelled reads, on the card: every rule by which kernels that build the two tables of window starts and gather a
// batch through them form a global-memory index (plain C++17, no device work; catfish_amd/device_db.py states the same rules in
// numpy -- centre_tables and DeviceReadDb.gather are normative).  The kernels themselves are not in the tree (DESIGN section 4b says
// why); this header is what they are to call for every global load and store that a label, a table entry or a count governs.
//
// tests/native/read_tables_replay.cpp states the kernels' bodies serially over these functions and runs under AddressSanitizer with
// buffers of exactly the sizes the Python layer would allocate; tests/native/read_tables_plan_shim.cpp puts the functions behind a
// C ABI for a sweep (tests/test_read_tables_plan.py).  A function that cannot vouch for an index returns RT_SKIP and the caller
// neither loads nor stores.  Under hipcc the functions are __host__ __device__; nothing includes the header there yet.
//
// Sample offsets are int64_t throughout, per-read counts uint32_t (a read has fewer than 2^31 samples, a table fewer than 2^31
// rows: device_db._table_sizes_fit).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif
#if defined(__clang__)
#define RT_UNROLL _Pragma("unroll")
#else
#define RT_UNROLL
#endif

#define RT_WINDOW 35            // samples per window (CF_T)
#define RT_PIECE 1024           // window starts per piece of a read's walk (device_db.TABLE_PIECE)
#define RT_PIECE_LABELS (RT_PIECE + RT_WINDOW - 1)     // labels a whole piece sees
#define RT_SKIP ((int64_t)-1)
#define RT_PERM_ROUNDS 4

enum { RT_NEG_ALL = 0, RT_NEG_CAP = 1, RT_NEG_POSITIVES = 2 };      // neg_per_read: None | an int | "positives"

RT_HD uint32_t rt_fmix32(uint32_t v) {                 // murmur3's finaliser (cf_fmix32, device_db.fmix32)
    v ^= v >> 16; v *= 0x85ebca6bu; v ^= v >> 13; v *= 0xc2b2ae35u; v ^= v >> 16;
    return v;
}

RT_HD uint32_t rt_clz32(uint32_t v) {                  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clz(v);
#else
    return (uint32_t)__builtin_clz(v);
#endif
}

// P(i, n, key) of device_db.keyed_permutation: a keyed bijection of [0, n), 0 < n < 2^31, i < n (cf_perm of sample_batch.hpp, which
// keeps its own device-only copy).
RT_HD uint32_t rt_perm(uint32_t i, uint32_t n, uint32_t key) {
    uint32_t b = n > 1u ? 32u - rt_clz32(n - 1u) : 0u;
    b = b < 2u ? 2u : b;
    b += b & 1u;
    const uint32_t half = b >> 1, mask = (1u << half) - 1u;
    uint32_t k[RT_PERM_ROUNDS];
    RT_UNROLL
    for (int r = 0; r < RT_PERM_ROUNDS; ++r) k[r] = rt_fmix32(key + (uint32_t)(r + 1) * 0x9E3779B9u);
    uint32_t v = i;
    do {                                                  // cycle walk: v stays inside [0, 2^b), so the walk returns to [0, n)
        uint32_t L = v >> half, R = v & mask;
    RT_UNROLL
        for (int r = 0; r < RT_PERM_ROUNDS; ++r) {
            const uint32_t t = L ^ (rt_fmix32(R ^ k[r]) & mask);
            L = R;
            R = t;
        }
        v = (L << half) | R;
    } while (v >= n);
    return v;
}

// ---------------------------------------------------------------------------------------------------- pieces of a read
// Read of n samples at offset o.  Its windows start at s in [0, n - 34) (centre s + 17); piece p holds the starts
// [first_lo, first_hi) = [p RT_PIECE, (p + 1) RT_PIECE) clipped to n - 34, and must see the labels [lab_lo, lab_hi) =
// [o + first_lo, o + first_hi + 34) clipped to o + n -- absolute indices into the concatenated labels.
struct rt_piece {
    int64_t first_lo, first_hi;       // window starts, relative to the read
    int64_t lab_lo, lab_hi;           // labels, absolute
};

RT_HD int64_t rt_n_starts(int64_t n) { return n >= RT_WINDOW ? n - (RT_WINDOW - 1) : 0; }
RT_HD int64_t rt_n_pieces(int64_t n) { return (rt_n_starts(n) + (RT_PIECE - 1)) / RT_PIECE; }

RT_HD rt_piece rt_piece_of(int64_t o, int64_t n, int64_t p) {
    const int64_t w = rt_n_starts(n);
    rt_piece pc;
    pc.first_lo = p < 0 ? w : (p > w / RT_PIECE ? w : p * RT_PIECE);
    if (pc.first_lo > w) pc.first_lo = w;
    pc.first_hi = pc.first_lo + RT_PIECE < w ? pc.first_lo + RT_PIECE : w;
    pc.lab_lo = o + pc.first_lo;
    pc.lab_hi = pc.first_hi > pc.first_lo ? o + pc.first_hi + (RT_WINDOW - 1) : pc.lab_lo;
    if (pc.lab_hi > o + n) pc.lab_hi = o + n;
    return pc;
}

// label number i of the piece (i in [0, RT_PIECE_LABELS)) -> its index in the concatenated labels, or RT_SKIP past what the piece sees
RT_HD int64_t rt_label_src(const rt_piece& pc, int64_t i) {
    return (i >= 0 && pc.lab_lo >= 0 && i < pc.lab_hi - pc.lab_lo) ? pc.lab_lo + i : RT_SKIP;
}

// ---------------------------------------------------------------------------------------------------- quota, key, selection
// device_db._neg_quota: how many of a read's m candidates become negatives when it has n_pos positives
RT_HD uint32_t rt_quota(int mode, int64_t value, uint32_t m, uint32_t n_pos) {
    if (mode == RT_NEG_POSITIVES) return m < n_pos ? m : n_pos;
    if (mode == RT_NEG_CAP) return value < 0 ? 0u : ((int64_t)m < value ? m : (uint32_t)value);
    return m;
}

RT_HD uint32_t rt_read_key(uint32_t seed, int64_t rho) { return rt_fmix32(seed ^ rt_fmix32((uint32_t)(rho + 1) * 0x9E3779B9u)); }

// candidate j of a read's m is a negative iff q == m or P(j, m, key) < q
RT_HD bool rt_neg_selected(uint32_t j, uint32_t m, uint32_t q, uint32_t key) {
    if (j >= m || m >= 0x80000000u) return false;
    return q >= m || rt_perm(j, m, key) < q;
}

// ---------------------------------------------------------------------------------------------------- output slots
// counts [n_reads][2]: the two numbers of read rho
RT_HD int64_t rt_count_slot(int64_t rho, int64_t n_reads, int which) {
    return (rho >= 0 && rho < n_reads && (which == 0 || which == 1)) ? rho * 2 + which : RT_SKIP;
}

// A table is int64 [RT_TABLE_HEAD + rows]: entry 0 holds the number of rows, written by the kernel that fills the rows from the
// same offsets that sized the allocation, so that the gather checks a row against the count that belongs to the table it indexes
// and not against one it is told.
#define RT_TABLE_HEAD 1

// a read's selected window number k_local is row off[rho] + k_local, unless that is not below off[rho + 1] (lo, hi: those two)
// -> its index in the table's buffer
RT_HD int64_t rt_out_slot(int64_t lo, int64_t hi, uint32_t k_local) {
    if (lo < 0 || hi < lo) return RT_SKIP;
    const int64_t row = lo + (int64_t)k_local;
    return row < hi ? RT_TABLE_HEAD + row : RT_SKIP;
}

// ---------------------------------------------------------------------------------------------------- the gather
RT_HD bool rt_row_ok(uint32_t row, uint32_t n) { return row < n; }

// row of a table whose entry 0 reads n_in_table -> its index in the table's buffer
RT_HD int64_t rt_table_row(uint32_t row, int64_t n_in_table) {
    return (n_in_table >= 0 && n_in_table <= 0x7fffffff && rt_row_ok(row, (uint32_t)n_in_table)) ? RT_TABLE_HEAD + (int64_t)row : RT_SKIP;
}

// a table entry -> the index of the window's first sample in signal [total], or RT_SKIP unless all 35 samples lie inside
RT_HD int64_t rt_window_src(int64_t start, int64_t total) {
    return (start >= 0 && total >= RT_WINDOW && start <= total - RT_WINDOW) ? start : RT_SKIP;
}

// slot of a batch of `size` windows, sample t -> index into x / y [size][35]
RT_HD int64_t rt_batch_dst(uint32_t slot, uint32_t size, uint32_t t) {
    return (slot < size && t < RT_WINDOW) ? (int64_t)slot * RT_WINDOW + t : RT_SKIP;
}
