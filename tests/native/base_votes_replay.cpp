// The bodies of base_votes_vote_kernel and base_votes_count_kernel (csrc/base_votes.hpp), walked serially on the CPU through
// csrc/base_votes_rule.hpp -- the rules by which the kernels form their addresses and the vote's fixed-point arithmetic -- with every
// buffer malloc'ed at exactly the size the Python layer allocates.  Built with -fsanitize=address,undefined by
// tests/test_base_votes_replay.py and run as its own process: an index outside a buffer, whatever the tables hold, ends the run.
//
// usage: base_votes_replay <case file> <output file>
// case:  int64 header [n, total, n_bases, set_total, K, max_bases, work_bytes (-1: what cf_base_votes_work_bytes says), longest_range,
//        long_base, grid_x (0: the entry point's), grid_y (0: the entry point's), edges_len], then edges int64 [edges_len], labels uint8
//        [set_total], basemap uint8 [set_total], src_first int64 [n], length int64 [n], bounds int64 [n + 1], ranges int64 [2 n],
//        thresholds double [K], probs float [total] -- the buffer sizes are taken from the arrays as the test wrote them (sizes that
//        the header forges negative or huge are refused before anything is allocated).
// out:   int64 refusal; when 0: sums uint64 [n_bases], state uint8 [K][n_bases], confusion int64 [K][20], runs int64 [K][run cells]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../catfish_amd/csrc/base_votes_rule.hpp"

template <class T>
static T* read_array(FILE* fh, int64_t count) {
    T* p = static_cast<T*>(malloc((size_t)count * sizeof(T)));
    if (count > 0 && fread(p, sizeof(T), (size_t)count, fh) != (size_t)count) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return p;
}

static int popcount64(unsigned long long v) { return __builtin_popcountll(v); }

// launch A, one workgroup
static void vote_block(int64_t bx, int64_t by, int64_t gx, int64_t gy, const float* probs, int64_t total, const uint8_t* labels,
                       const uint8_t* basemap, int64_t set_total, const int64_t* edges, int64_t n_bases, const int64_t* src_first,
                       const int64_t* length, const int64_t* bounds, const int64_t* ranges, int64_t n, int K, int64_t long_base,
                       const unsigned long long* qt, unsigned long long* sums, uint8_t* state) {
    for (int64_t r = by; r < n; r += gy) {
        const int64_t a = bv_clamp(ranges[r], n_bases), b = bv_clamp(ranges[n + r], n_bases);
        if (b <= a) continue;
        const int64_t src = src_first[r], len = length[r], bound = bounds[r];
        for (int64_t e0 = a + bx * BV_THREADS; e0 < b; e0 += gx * BV_THREADS) {
            for (int wave = 0; wave < BV_THREADS / 64; ++wave) {
                int64_t mine[64], s0[64], p0[64];
                unsigned long long sum[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const int64_t e = e0 + wave * 64 + lane;
                    s0[lane] = p0[lane] = 0;
                    mine[lane] = e < b ? bv_span(edges, n_bases, e, src, len, bound, total, set_total, &s0[lane], &p0[lane]) : 0;
                    sum[lane] = 0;
                    if (mine[lane] <= long_base)
                        for (int64_t i = 0; i < mine[lane]; ++i) sum[lane] += bv_q(probs[p0[lane] + i]);
                }
                for (int owner = 0; owner < 64; ++owner) {             // the ballot's set bits, in order
                    if (!(mine[owner] > long_base)) continue;
                    unsigned long long whole = 0;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int64_t i = lane; i < mine[owner]; i += 64) whole += bv_q(probs[p0[owner] + i]);
                    sum[owner] = whole;
                }
                for (int lane = 0; lane < 64; ++lane) {
                    const int64_t e = e0 + wave * 64 + lane;
                    if (mine[lane] <= 0) continue;
                    sums[e] = sum[lane];
                    const bool truth = labels[s0[lane]] == 1u;
                    const unsigned cls = bv_class(basemap[s0[lane]] & 0x7fu);
                    for (int k = 0; k < K; ++k)
                        state[(int64_t)k * n_bases + e] = bv_state(sum[lane] >= qt[k] * (unsigned long long)mine[lane], truth, cls);
                }
            }
        }
    }
}

// launch B, one workgroup
static void count_block(int64_t bx, int64_t by, int64_t bz, int64_t gx, int64_t gy, int64_t gz, const uint8_t* state, const int64_t* edges,
                        int64_t n_bases, const int64_t* src_first, const int64_t* length, const int64_t* bounds, int64_t total,
                        int64_t set_total, const int64_t* ranges, int64_t n, int K, int max_bases, unsigned long long* confusion_out, unsigned long long* runs_out) {
    unsigned* s_tab = static_cast<unsigned*>(malloc(sizeof(unsigned) * (BV_CONF_CELLS + 2 * 3 * BV_CLASSES * (BV_MAX_BASES + 1))));
    const int run_cells = bv_run_cells(max_bases), cells = BV_CONF_CELLS + run_cells;
    for (int64_t k = bz; k < K; k += gz) {
        const uint8_t* state_k = state + k * n_bases;
        for (int c = 0; c < cells; ++c) s_tab[c] = 0u;
        for (int64_t r = by; r < n; r += gy) {
            const int64_t a = bv_clamp(ranges[r], n_bases), b = bv_clamp(ranges[n + r], n_bases);
            if (b <= a) continue;
            const bv_stretch s = bv_window(src_first[r], length[r], bounds[r], total, set_total);
            for (int64_t e0 = a + bx * BV_THREADS; e0 < b; e0 += gx * BV_THREADS) {
                for (int wave = 0; wave < BV_THREADS / 64; ++wave) {
                    int cell[64];
                    unsigned st[64];
                    unsigned long long open = 0;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int64_t e = e0 + wave * 64 + lane;
                        st[lane] = e < b ? bv_state_of(state_k, edges, n_bases, e, s) : 0u;
                        cell[lane] = bv_conf_cell(st[lane]);
                        if (cell[lane] >= 0) open |= 1ull << lane;
                    }
                    while (open) {
                        const int leader = __builtin_ctzll(open);
                        unsigned long long same = 0;
                        for (int lane = 0; lane < 64; ++lane)
                            if (cell[lane] == cell[leader]) same |= 1ull << lane;
                        s_tab[cell[leader]] += (unsigned)popcount64(same);
                        open &= ~same;
                    }
                    for (int lane = 0; lane < 64; ++lane) {
                        const int64_t e = e0 + wave * 64 + lane;
                        if (!(st[lane] & BV_VOTED)) continue;
                        for (int kind = 0; kind < 2; ++kind) {
                            const int run = bv_run_cell(state_k, edges, n_bases, s, st[lane], e, a, b, kind, max_bases);
                            if (run >= 0) s_tab[BV_CONF_CELLS + run] += 1u;
                        }
                    }
                }
            }
        }
        for (int c = 0; c < cells; ++c) {
            if (s_tab[c] == 0u) continue;
            if (c < BV_CONF_CELLS) confusion_out[k * BV_CONF_CELLS + c] += s_tab[c];
            else runs_out[k * run_cells + (c - BV_CONF_CELLS)] += s_tab[c];
        }
    }
    free(s_tab);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t head[12];
    if (fread(head, sizeof(int64_t), 12, fh) != 12) return 2;
    const int64_t n = head[0], total = head[1], n_bases = head[2], set_total = head[3], longest_range = head[7], long_base = head[8];
    const int32_t K = (int32_t)head[4], max_bases = (int32_t)head[5];
    int64_t work_bytes = head[6];
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (work_bytes < 0) work_bytes = bv_work_bytes(n_bases, K);
    int64_t refusal = head[4] != K || head[5] != max_bases ? 3 : bv_refusal(n, total, n_bases, set_total, K, max_bases, work_bytes);
    fwrite(&refusal, sizeof(int64_t), 1, out);
    if (refusal) {
        fclose(out);
        fclose(fh);
        return 0;
    }
    int64_t* edges = read_array<int64_t>(fh, head[11]);
    uint8_t* labels = read_array<uint8_t>(fh, set_total);
    uint8_t* basemap = read_array<uint8_t>(fh, set_total);
    int64_t* src_first = read_array<int64_t>(fh, n);
    int64_t* length = read_array<int64_t>(fh, n);
    int64_t* bounds = read_array<int64_t>(fh, n + 1);
    int64_t* ranges = read_array<int64_t>(fh, 2 * n);
    double* thresholds = read_array<double>(fh, K);
    float* probs = read_array<float>(fh, total);
    fclose(fh);
    if (head[11] != n_bases + 1) return 2;

    unsigned long long qt[BV_MAX_K] = {};
    for (int k = 0; k < K; ++k) qt[k] = bv_q((float)thresholds[k]);
    const int run_cells = bv_run_cells(max_bases);
    uint8_t* work = static_cast<uint8_t*>(malloc((size_t)work_bytes));                       // what the Python layer allocates
    unsigned long long* confusion = static_cast<unsigned long long*>(calloc((size_t)K * BV_CONF_CELLS, sizeof(unsigned long long)));
    unsigned long long* runs = static_cast<unsigned long long*>(calloc((size_t)K * run_cells, sizeof(unsigned long long)));
    memset(work, 0xEE, (size_t)work_bytes);
    memset(work, 0, (size_t)(8 + K) * (size_t)n_bases);                                      // the entry point's memset
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(work);
    uint8_t* state = work + bv_work_state(n_bases);
    if (!(n == 0 || n_bases == 0 || total == 0 || set_total == 0)) {
        const int64_t widest = longest_range < 1 ? 1 : (longest_range > n_bases ? n_bases : longest_range);
        const int64_t gx = head[9] > 0 ? head[9] : std::min<int64_t>((widest + BV_THREADS - 1) / BV_THREADS, BV_GRID_X);
        const int64_t gy = head[10] > 0 ? head[10] : std::min<int64_t>(n, BV_GRID_Y);
        for (int64_t by = 0; by < gy; ++by)
            for (int64_t bx = 0; bx < gx; ++bx)
                vote_block(bx, by, gx, gy, probs, total, labels, basemap, set_total, edges, n_bases, src_first, length, bounds, ranges, n, K,
                           long_base, qt, sums, state);
        for (int64_t bz = 0; bz < K; ++bz)
            for (int64_t by = 0; by < gy; ++by)
                for (int64_t bx = 0; bx < gx; ++bx)
                    count_block(bx, by, bz, gx, gy, K, state, edges, n_bases, src_first, length, bounds, total, set_total, ranges, n, K, max_bases, confusion, runs);
    }
    fwrite(sums, sizeof(unsigned long long), (size_t)n_bases, out);
    fwrite(state, 1, (size_t)K * (size_t)n_bases, out);
    fwrite(confusion, sizeof(unsigned long long), (size_t)K * BV_CONF_CELLS, out);
    fwrite(runs, sizeof(unsigned long long), (size_t)K * run_cells, out);
    fclose(out);
    free(edges); free(labels); free(basemap); free(src_first); free(length); free(bounds); free(ranges); free(thresholds); free(probs);
    free(work); free(confusion); free(runs);
    return 0;
}
