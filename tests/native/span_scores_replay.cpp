// span_scores_kernel's body (catfish_amd/csrc/span_scores.hpp), serially, over the same rule header: one "wave" of 64 lanes per run,
// the ballot as a loop over the lanes, the __shfl_xor butterfly as 64 additions per stage in the kernel's order.  A stand-alone
// program for AddressSanitizer + UBSan; every buffer is malloc'ed at exactly the size the Python layer allocates, so an index formed
// wrongly is a report, not a wrong number.
//
//   span_scores_replay CASE OUT
// CASE: int64 n_reads, total, max_runs, count, has_signal; uint32 threshold bits, uint32 0; int64 read_offsets[n_reads + 1],
//       read_lengths[n_reads], starts[max_runs]; float probs[total]; float signal[total] when has_signal
// OUT:  int64 ends_paired[max_runs]; double sums[max_runs][3]; float extremes[max_runs][2] -- filled with -7777 before the walk
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../catfish_amd/csrc/span_scores_rule.hpp"

template <class T>
static T* exactly(FILE* fh, int64_t n) {                   // n values in a block of exactly n * sizeof(T) bytes
    T* p = static_cast<T*>(malloc((size_t)n * sizeof(T)));
    if (n > 0 && (!p || fread(p, sizeof(T), (size_t)n, fh) != (size_t)n)) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return p;
}

template <class T>
static T* filled(int64_t n, T v) {
    T* p = static_cast<T*>(malloc((size_t)n * sizeof(T)));
    for (int64_t i = 0; i < n; ++i) p[i] = v;
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t head[5];
    uint32_t tbits[2];
    if (fread(head, sizeof(int64_t), 5, fh) != 5 || fread(tbits, sizeof(uint32_t), 2, fh) != 2) return 2;
    const int64_t n_reads = head[0], total = head[1], max_runs = head[2];
    const uint64_t count = (uint64_t)head[3];
    float threshold;
    memcpy(&threshold, &tbits[0], sizeof(float));
    int64_t* read_offsets = exactly<int64_t>(fh, n_reads + 1);
    int64_t* read_lengths = exactly<int64_t>(fh, n_reads);
    int64_t* starts = exactly<int64_t>(fh, max_runs);
    float* probs = exactly<float>(fh, total);
    float* signal = head[4] ? exactly<float>(fh, total) : nullptr;
    fclose(fh);
    int64_t* ends_paired = filled<int64_t>(max_runs, -7777);
    double* sums = filled<double>(3 * max_runs, -7777.0);
    float* extremes = filled<float>(2 * max_runs, -7777.f);

    const int64_t n_rows = ss_rows(count, max_runs);
    for (int64_t k = 0; k < n_rows; ++k) {                                  // one wave per run
        const int64_t start = starts[k];
        const ss_walk w = ss_open(read_offsets, read_lengths, n_reads, total, start);
        double sp[64], sx[64], sx2[64];
        float lo[64], hi[64];
        for (int lane = 0; lane < 64; ++lane) {
            sp[lane] = sx[lane] = sx2[lane] = 0.0;
            lo[lane] = std::numeric_limits<float>::infinity();
            hi[lane] = -std::numeric_limits<float>::infinity();
        }
        int64_t pos = start;
        bool go = w.open;
        while (go) {
            const int64_t left = w.end - pos;
            float p[64], x[64];
            uint64_t hit = 0;
            for (int lane = 0; lane < 64; ++lane) {                         // the loads and the ballot
                const bool in = lane < left;
                p[lane] = in ? probs[pos + lane] : 0.f;
                x[lane] = (in && signal) ? signal[pos + lane] : 0.f;
                if (in && p[lane] >= threshold) hit |= 1ull << lane;
            }
            const ss_taken t = ss_step(hit, left);
            for (int lane = 0; lane < t.take; ++lane) {
                sp[lane] += (double)p[lane];
                sx[lane] += (double)x[lane];
                sx2[lane] += (double)x[lane] * (double)x[lane];
                lo[lane] = fminf(lo[lane], p[lane]);
                hi[lane] = fmaxf(hi[lane], p[lane]);
            }
            pos += t.take;
            go = t.go_on;
        }
        for (int d = 32; d >= 1; d >>= 1) {                                 // the butterfly: lane l adds lane l ^ d
            double np_[64], nx[64], nx2[64];
            float nlo[64], nhi[64];
            for (int lane = 0; lane < 64; ++lane) {
                np_[lane] = sp[lane] + sp[lane ^ d];
                nx[lane] = sx[lane] + sx[lane ^ d];
                nx2[lane] = sx2[lane] + sx2[lane ^ d];
                nlo[lane] = fminf(lo[lane], lo[lane ^ d]);
                nhi[lane] = fmaxf(hi[lane], hi[lane ^ d]);
            }
            memcpy(sp, np_, sizeof sp);
            memcpy(sx, nx, sizeof sx);
            memcpy(sx2, nx2, sizeof sx2);
            memcpy(lo, nlo, sizeof lo);
            memcpy(hi, nhi, sizeof hi);
        }
        ends_paired[k] = pos;
        sums[ss_sum_index(k, 0)] = sp[0];
        if (signal) {
            sums[ss_sum_index(k, 1)] = sx[0];
            sums[ss_sum_index(k, 2)] = sx2[0];
        }
        extremes[ss_extreme_index(k, 0)] = lo[0];
        extremes[ss_extreme_index(k, 1)] = hi[0];
    }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(ends_paired, sizeof(int64_t), (size_t)max_runs, out);
    fwrite(sums, sizeof(double), (size_t)(3 * max_runs), out);
    fwrite(extremes, sizeof(float), (size_t)(2 * max_runs), out);
    fclose(out);
    free(read_offsets); free(read_lengths); free(starts); free(probs); free(signal);
    free(ends_paired); free(sums); free(extremes);
    return 0;
}
