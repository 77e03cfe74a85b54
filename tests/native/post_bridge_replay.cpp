// postprocess_bridged_kernel's body (catfish_amd/csrc/ingest_post.hpp), serially, over the same rule header: one "wave" of 64 lanes per
// 62 payload words, every lane's valid / first masks from the read table as the kernel forms them, the ballots as loops over the
// samples, the neighbours' words as array reads, then pb_fill and pb_open on the lane's 192-bit window and the middle word out as
// labels and run boundaries.  A stand-alone program for AddressSanitizer + UBSan; every buffer is malloc'ed at exactly its size.
//
//   post_bridge_replay CASE OUT
// CASE: int64 n_reads, total, max_gap, min_run; uint32 threshold bits, uint32 0; int64 read_offsets[n_reads + 1],
//       read_lengths[n_reads]; float probs[total]
// OUT:  int64 n_starts, n_ends; uint8 labels[total] (filled with 7 before the walk); int64 starts[n_starts]; int64 ends[n_ends]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../catfish_amd/csrc/post_bridge_rule.hpp"

#define POST_WORDS 62              // CF_POST_WORDS: payload words per wave

template <class T>
static T* exactly(FILE* fh, int64_t n) {                   // n values in a block of exactly n * sizeof(T) bytes
    T* p = static_cast<T*>(malloc((size_t)n * sizeof(T)));
    if (n > 0 && (!p || fread(p, sizeof(T), (size_t)n, fh) != (size_t)n)) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t head[4];
    uint32_t tbits[2];
    if (fread(head, sizeof(int64_t), 4, fh) != 4 || fread(tbits, sizeof(uint32_t), 2, fh) != 2) return 2;
    const int64_t n_reads = head[0], total = head[1];
    const int max_gap = (int)head[2], min_run = (int)head[3];
    if (!pb_domain(min_run, max_gap)) return 3;            // what the host refuses before any launch
    float threshold;
    memcpy(&threshold, &tbits[0], sizeof(float));
    int64_t* read_offsets = exactly<int64_t>(fh, n_reads + 1);
    int64_t* read_lengths = exactly<int64_t>(fh, n_reads);
    float* probs = exactly<float>(fh, total);
    fclose(fh);
    uint8_t* labels = static_cast<uint8_t*>(malloc((size_t)total));
    for (int64_t i = 0; i < total; ++i) labels[i] = 7;
    std::vector<int64_t> starts, ends;

    const int64_t n_words = (total + 63) >> 6;
    for (int64_t chunk = 0; chunk * POST_WORDS < n_words && n_reads > 0; ++chunk) {          // one wave
        const int64_t w0 = chunk * POST_WORDS;
        uint64_t mine[64], valid[64], first[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t w = w0 - 1 + lane, base = w * 64;
            uint64_t v = 0, f = 0;
            if (w >= 0 && base < total) {                  // 1. which samples of the lane's word are real samples of a read
                int64_t lo = 0, hi = n_reads;
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (read_offsets[mid] <= base) lo = mid; else hi = mid;
                }
                for (int64_t r = lo; r < n_reads; ++r) {
                    const int64_t beg = read_offsets[r];
                    if (beg >= base + 64) break;
                    const int64_t end = beg + read_lengths[r];
                    const int64_t a = beg > base ? beg - base : 0, b = (end < base + 64 ? end : base + 64) - base;
                    if (b > a) v |= (b - a >= 64 ? ~0ull : ((1ull << (b - a)) - 1ull)) << a;
                    if (beg >= base) f |= 1ull << (beg - base);
                }
            }
            uint64_t bal = 0;                              // 2. threshold bits: the ballot of the lane's word
            for (int b = 0; b < 64; ++b) {
                const int64_t i = base + b;
                const float p = (i >= 0 && i < total) ? probs[i] : -1.f;
                if (p >= threshold) bal |= 1ull << b;
            }
            mine[lane] = bal & v;
            valid[lane] = v;
            first[lane] = f;
        }
        for (int lane = 1; lane < 63; ++lane) {            // (lanes 0 and 63 are halo lanes)
            const int64_t base = (w0 - 1 + lane) * 64;
            if (base >= total) break;
            const pb_w192 bits = {mine[lane - 1], mine[lane], mine[lane + 1]};
            const pb_w192 v = {valid[lane - 1], valid[lane], valid[lane + 1]};
            const pb_w192 f = {first[lane - 1], first[lane], first[lane + 1]};
            const pb_w192 cut = pb_not(f);
            const pb_w192 x = pb_open(max_gap > 0 ? pb_fill(bits, v, f, max_gap) : bits, cut, min_run);      // 2 1/2 and 3
            const uint64_t sm = x.m & (~((x.m << 1) | (x.p >> 63)) | ~cut.m);
            const uint64_t em = x.m & (~((x.m >> 1) | (x.n << 63)) | ((~cut.m >> 1) | (~cut.n << 63)));
            for (int b = 0; b < 64; ++b) {
                if ((sm >> b) & 1ull) starts.push_back(base + b);
                if ((em >> b) & 1ull) ends.push_back(base + b + 1);
                if (base + b < total) labels[base + b] = (uint8_t)((x.m >> b) & 1ull);          // 4.
            }
        }
    }

    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    const int64_t counts[2] = {(int64_t)starts.size(), (int64_t)ends.size()};
    fwrite(counts, sizeof(int64_t), 2, fh);
    fwrite(labels, 1, (size_t)total, fh);
    if (!starts.empty()) fwrite(starts.data(), sizeof(int64_t), starts.size(), fh);
    if (!ends.empty()) fwrite(ends.data(), sizeof(int64_t), ends.size(), fh);
    fclose(fh);
    free(read_offsets);
    free(read_lengths);
    free(probs);
    free(labels);
    return 0;
}
