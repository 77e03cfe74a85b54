// The three kernels of a card side for device_db.DeviceReadDb (count a read's windows, fill the two tables, gather a batch through
// them) stated serially on the CPU, for tests/test_read_tables_replay.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o read_tables_replay read_tables_replay.cpp
//   read_tables_replay CASE OUT
// Every index into labels, counts, the offset arrays, the tables, the signal and the batch is formed by the functions of
// read_tables_plan.hpp -- the functions such kernels are to call -- and every buffer is malloc'ed at exactly the size the Python
// layer would allocate on the card, so an index the plan lets through although it lies outside is an AddressSanitizer report.  A serial scan stands in for the workgroup's scans: the numbers k, j and the two ranks simply run on.
//
// CASE (little endian): int64 n_reads, total, lessen, neg_mode, neg_value, table_seed, seed, n_batches, forged;
//   int64 offsets[n_reads + 1]; uint8 labels[total]; float signal[total]; int64 (draw, size, ratio)[n_batches];
//   forged != 0: int64 claim_pos, have_pos, pos[have_pos], claim_neg, have_neg, neg[have_neg] -- tables to gather through INSTEAD of
//   the built ones, allocated at have_* rows (and saying so in their entry 0) while the gather is told claim_*.
// OUT: int64 n_pos, n_neg; uint32 counts[n_reads][2]; int64 pos_start[n_pos], neg_start[n_neg];
//   per batch float x[size][35], uint8 is_pos[size], int32 status[2].
// Exit status: 0 fine; 3 some index was skipped (reported on stderr, OUT still complete); 2 bad case file; 4 a batch's labels differ
// inside a window or a built table's entry 0 is not its row count.
#include "../../catfish_amd/csrc/read_tables_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_skips = 0;
static void skipped(const char* what, long long a, long long b) {
    if (g_skips++ < 8) std::fprintf(stderr, "skip: %s (%lld, %lld)\n", what, a, b);
}

template <typename T>
static T* exact(int64_t n) {                                   // n elements and not one more; "at least one element" is the caller's
    T* p = static_cast<T*>(std::malloc((size_t)n * sizeof(T)));
    if (!p) std::exit(2);
    return p;
}

struct Tables {
    const uint8_t* labels; const int64_t* offsets; int64_t n_reads; uint32_t lessen;
};

// the table walk for one read (FILL: the second pass): the pieces in order, the carries running
template <bool FILL>
static void walk_read(const Tables& t, int64_t rho, uint32_t seed, const int64_t* pos_off, const int64_t* neg_off, const uint32_t* cand,
                      const uint32_t* quota, int64_t* pos_start, int64_t* neg_start, uint32_t* counts) {
    const int64_t o = t.offsets[rho], n = t.offsets[rho + 1] - o;
    const int64_t n_pieces = (o >= 0 && n >= 0 && n <= 0x7fffffff) ? rt_n_pieces(n) : 0;
    uint32_t m = 0, q = 0, key = 0;
    int64_t pos_lo = 0, pos_hi = 0, neg_lo = 0, neg_hi = 0;
    if (FILL) {
        m = cand[rho]; q = quota[rho]; key = rt_read_key(seed, rho);
        pos_lo = pos_off[rho]; pos_hi = pos_off[rho + 1];
        neg_lo = neg_off[rho]; neg_hi = neg_off[rho + 1];
        if (rho == t.n_reads - 1) { pos_start[0] = pos_hi; neg_start[0] = neg_hi; }
    }
    uint32_t k = 0, j = 0, pos_run = 0, neg_run = 0;
    uint8_t lab[RT_PIECE_LABELS];
    int ones[RT_PIECE_LABELS + 1], zeros[RT_PIECE_LABELS + 1];
    for (int64_t p = 0; p < n_pieces; ++p) {
        const rt_piece pc = rt_piece_of(o, n, p);
        ones[0] = zeros[0] = 0;
        for (int i = 0; i < RT_PIECE_LABELS; ++i) {
            const int64_t g = rt_label_src(pc, i);
            lab[i] = g != RT_SKIP ? t.labels[g] : 0xff;
            ones[i + 1] = ones[i] + (lab[i] == 1);
            zeros[i + 1] = zeros[i] + (lab[i] == 0);
        }
        const int64_t n_first = pc.first_hi - pc.first_lo;
        for (int64_t s = 0; s < n_first; ++s) {
            const bool all1 = ones[s + RT_WINDOW] - ones[s] == RT_WINDOW, all0 = zeros[s + RT_WINDOW] - zeros[s] == RT_WINDOW;
            const int64_t first = o + pc.first_lo + s;
            if (lab[s + RT_WINDOW / 2] == 1) {
                if (k % t.lessen == 0u && all1) {
                    if (FILL) {
                        const int64_t slot = rt_out_slot(pos_lo, pos_hi, pos_run);
                        if (slot != RT_SKIP) pos_start[slot] = first; else skipped("positive slot", rho, pos_run);
                    }
                    ++pos_run;
                }
                ++k;
            }
            if (all0) {
                if (FILL && rt_neg_selected(j, m, q, key)) {
                    const int64_t slot = rt_out_slot(neg_lo, neg_hi, neg_run);
                    if (slot != RT_SKIP) neg_start[slot] = first; else skipped("negative slot", rho, neg_run);
                    ++neg_run;
                }
                ++j;
            }
        }
    }
    if (!FILL) {
        const int64_t c0 = rt_count_slot(rho, t.n_reads, 0), c1 = rt_count_slot(rho, t.n_reads, 1);
        if (c0 != RT_SKIP) counts[c0] = pos_run; else skipped("count slot", rho, 0);
        if (c1 != RT_SKIP) counts[c1] = j; else skipped("count slot", rho, 1);
    }
}

// the gather for one slot: sample_batch_kernel with one indirection (lanes 0 .. 63 in turn, 35 of them move a sample)
static void gather_slot(const float* signal, int64_t total, const int64_t* pos_start, uint32_t n_pos, const int64_t* neg_start, uint32_t n_neg,
                        uint32_t size, uint32_t n_draw_pos, uint32_t seed, const int64_t* draw_counter, float* x, float* y, int32_t* status,
                        uint32_t slot) {
    if (slot >= size) return;
    const uint32_t draw = (uint32_t)draw_counter[0];
    const uint32_t base = rt_fmix32(seed ^ rt_fmix32(draw * 0x85ebca6bu));
    const uint32_t rank = rt_perm(slot, size, base ^ 1u);
    const bool is_pos = rank < n_draw_pos;
    const uint32_t row = is_pos ? rt_perm(rank, n_pos, base ^ 2u) : rt_perm(rank - n_draw_pos, n_neg, base ^ 3u);
    const int64_t* table = is_pos ? pos_start : neg_start;
    const int64_t at = rt_table_row(row, table[0]);
    const bool row_ok = at != RT_SKIP;
    const int64_t start = row_ok ? table[at] : RT_SKIP;
    const int64_t src = rt_window_src(start, total);
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        const int64_t dst = rt_batch_dst(slot, size, lane);
        if (dst != RT_SKIP) {
            x[dst] = src != RT_SKIP ? signal[src + lane] : 0.0f;
            y[dst] = (src != RT_SKIP && is_pos) ? 1.0f : 0.0f;
        }
    }
    if (src == RT_SKIP) {
        status[0] = row_ok ? 2 : 1;
        status[1] = (int32_t)slot;
        skipped(row_ok ? "window start" : "table row", row_ok ? (long long)start : (long long)row, slot);
    }
}

static bool get(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static void put(std::FILE* f, const void* p, size_t bytes) {
    if (bytes && std::fwrite(p, 1, bytes, f) != bytes) std::exit(2);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int64_t h[9];
    if (!get(in, h, sizeof h)) return 2;
    const int64_t n_reads = h[0], total = h[1], lessen = h[2], neg_value = h[4], n_batches = h[7], forged = h[8];
    const int neg_mode = (int)h[3];
    const uint32_t table_seed = (uint32_t)h[5], seed = (uint32_t)h[6];
    if (n_reads < 0 || total < 0 || lessen < 1 || n_batches < 0) return 2;
    // what goes up: offsets [R + 1], labels and signal at `total` entries (at least one)
    int64_t* offsets = exact<int64_t>(n_reads + 1);
    uint8_t* labels = exact<uint8_t>(total > 0 ? total : 1);
    float* signal = exact<float>(total > 0 ? total : 1);
    if (!get(in, offsets, (size_t)(n_reads + 1) * 8) || !get(in, labels, (size_t)total) || !get(in, signal, (size_t)total * 4)) return 2;
    std::vector<int64_t> batches((size_t)n_batches * 3);
    if (!get(in, batches.data(), batches.size() * 8)) return 2;

    // pass 1, then the host step of the Python layer, then pass 2
    const Tables t = {labels, offsets, n_reads, (uint32_t)lessen};
    uint32_t* counts = exact<uint32_t>(n_reads > 0 ? n_reads * 2 : 1);
    for (int64_t rho = 0; rho < n_reads; ++rho) walk_read<false>(t, rho, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, counts);
    int64_t* pos_off = exact<int64_t>(n_reads + 1);
    int64_t* neg_off = exact<int64_t>(n_reads + 1);
    uint32_t* cand = exact<uint32_t>(n_reads > 0 ? n_reads : 1);
    uint32_t* quota = exact<uint32_t>(n_reads > 0 ? n_reads : 1);
    pos_off[0] = neg_off[0] = 0;
    for (int64_t rho = 0; rho < n_reads; ++rho) {
        cand[rho] = counts[rho * 2 + 1];
        quota[rho] = rt_quota(neg_mode, neg_value, cand[rho], counts[rho * 2]);
        pos_off[rho + 1] = pos_off[rho] + counts[rho * 2];
        neg_off[rho + 1] = neg_off[rho] + quota[rho];
    }
    int64_t n_pos = pos_off[n_reads], n_neg = neg_off[n_reads];
    int64_t* pos_start = exact<int64_t>(RT_TABLE_HEAD + n_pos);          // zeroed on the card: a table of no reads keeps its 0 rows
    int64_t* neg_start = exact<int64_t>(RT_TABLE_HEAD + n_neg);
    pos_start[0] = neg_start[0] = 0;
    for (int64_t rho = 0; rho < n_reads; ++rho)
        walk_read<true>(t, rho, table_seed, pos_off, neg_off, cand, quota, pos_start, neg_start, nullptr);
    put(out, &n_pos, 8);
    put(out, &n_neg, 8);
    put(out, counts, (size_t)n_reads * 2 * 4);
    if (pos_start[0] != n_pos || neg_start[0] != n_neg) return 4;
    put(out, pos_start + RT_TABLE_HEAD, (size_t)n_pos * 8);
    put(out, neg_start + RT_TABLE_HEAD, (size_t)n_neg * 8);

    const int64_t* gather_pos = pos_start;
    const int64_t* gather_neg = neg_start;
    if (forged) {
        int64_t c[2];
        for (int which = 0; which < 2; ++which) {
            if (!get(in, c, sizeof c) || c[0] < 0 || c[1] < 0) return 2;
            int64_t* tab = exact<int64_t>(RT_TABLE_HEAD + c[1]);
            tab[0] = c[1];
            if (!get(in, tab + RT_TABLE_HEAD, (size_t)c[1] * 8)) return 2;
            (which ? gather_neg : gather_pos) = tab;
            (which ? n_neg : n_pos) = c[0];
        }
    }
    int64_t* counter = exact<int64_t>(1);
    int32_t* status = exact<int32_t>(2);
    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t draw = batches[b * 3], size = batches[b * 3 + 1], ratio = batches[b * 3 + 2];
        // the launch's refusals (sample_batch_launch's, and a signal that holds a window)
        if (size <= 0 || size > 0x7fffffff || ratio <= 0 || n_pos > 0x7fffffff || n_neg > 0x7fffffff || total < RT_WINDOW) return 2;
        const int64_t k_pos = size / ratio;
        if (k_pos > n_pos || size - k_pos > n_neg) return 2;
        float* x = exact<float>(size * RT_WINDOW);
        float* y = exact<float>(size * RT_WINDOW);
        counter[0] = draw;
        status[0] = status[1] = 0;
        const uint32_t n_slots = (uint32_t)((size + 3) / 4 * 4);           // the grid's waves: four slots per workgroup
        for (uint32_t slot = 0; slot < n_slots; ++slot)
            gather_slot(signal, total, gather_pos, (uint32_t)n_pos, gather_neg, (uint32_t)n_neg, (uint32_t)size, (uint32_t)k_pos, seed, counter, x,
                        y, status, slot);
        std::vector<uint8_t> is_pos((size_t)size);
        for (int64_t s = 0; s < size; ++s) {
            for (int l = 1; l < RT_WINDOW; ++l)
                if (y[s * RT_WINDOW + l] != y[s * RT_WINDOW]) return 4;
            is_pos[(size_t)s] = y[s * RT_WINDOW] == 1.0f;
        }
        put(out, x, (size_t)size * RT_WINDOW * 4);
        put(out, is_pos.data(), (size_t)size);
        put(out, status, 8);
        std::free(x);
        std::free(y);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::free(offsets); std::free(labels); std::free(signal); std::free(counts); std::free(pos_off); std::free(neg_off); std::free(cand);
    std::free(quota); std::free(counter); std::free(status);
    if (gather_pos != pos_start) std::free(const_cast<int64_t*>(gather_pos));
    if (gather_neg != neg_start) std::free(const_cast<int64_t*>(gather_neg));
    std::free(pos_start); std::free(neg_start);
    return g_skips ? 3 : 0;
}
