// The base kernel's body (catfish_amd/csrc/validation_bases.hpp), stated serially over catfish_amd/csrc/
// validation_bases_word.hpp: a stand-alone program that tests/test_run_bases_replay.py builds with g++ -fsanitize=address,
// undefined and holds to device_validation.run_bases_host.
//
//   validation_bases_replay <batch file> <max_bases> <piece in words>
//
// Batch file: int64 count, then per stretch int64 n, n label bytes, n bytes of corrected prediction, n bytes of base map.
// Output: two lines (kind 0, kind 1) of 3 * 5 * (max_bases + 1) counts, summed over the stretches.
//
// Per stretch the masks sit in exactly sized malloc'ed buffers of n / 64 + 1 words, so a word index that is off by one is a heap
// overflow the sanitizer reports.  As in the kernel a stretch is walked in pieces: inside a piece the seg at the end of every word
// is an inclusive scan with vbs_join that starts from nothing, and what is open from the pieces before comes in as a carry.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../catfish_amd/csrc/validation_bases_word.hpp"

template <class Pred>
static uint64_t* words_of(const unsigned char* v, int64_t n, int64_t n_words, Pred&& pred) {
    uint64_t* w = static_cast<uint64_t*>(malloc((size_t)n_words * sizeof(uint64_t)));
    if (!w) exit(3);
    for (int64_t j = 0; j < n_words; ++j) w[j] = 0ull;
    for (int64_t i = 0; i < n; ++i)
        if (pred(v[i])) w[i >> 6] |= 1ull << (i & 63);
    return w;
}

struct side { uint64_t *run, *is1, *is0; };

static side side_of(const unsigned char* mine, const unsigned char* other, int64_t n, int64_t n_words) {
    side s = {words_of(mine, n, n_words, [](unsigned char b) { return b == 1u; }), words_of(other, n, n_words, [](unsigned char b) { return b == 1u; }),
              words_of(other, n, n_words, [](unsigned char b) { return b == 0u; })};
    if (n >= 2 && mine[n - 2] == 1u) s.run[(n - 1) >> 6] |= 1ull << ((n - 1) & 63);          // hp_loc_dict closes an open run AT the last sample
    return s;
}

static void walk(const side& s, const uint64_t* mark, uint64_t* const (&is)[4], int64_t n_words, int64_t piece, int max_bases, long long* row) {
    std::vector<vbs_seg> inc((size_t)piece);
    vbs_seg carry = vbs_none();
    auto word = [&](int64_t w) { return vbs_masks{s.run[w], s.is1[w], s.is0[w], mark[w], {is[0][w], is[1][w], is[2][w], is[3][w]}}; };
    for (int64_t w0 = 0; w0 < n_words; w0 += piece) {
        const int64_t count = n_words - w0 < piece ? n_words - w0 : piece;
        for (int64_t i = 0; i < count; ++i) {
            const vbs_seg mine = vbs_word(word(w0 + i));
            inc[(size_t)i] = i ? vbs_join(inc[(size_t)i - 1], mine) : mine;
        }
        for (int64_t i = 0; i < count; ++i) {
            const vbs_seg in = i ? vbs_join(carry, inc[(size_t)i - 1]) : carry;
            vbs_count(word(w0 + i), in, max_bases, [&](int cell) { ++row[cell]; });
        }
        carry = vbs_join(carry, inc[(size_t)count - 1]);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int max_bases = atoi(argv[2]);
    const int64_t piece = atoll(argv[3]);
    if (max_bases < 1 || max_bases > VBS_MAX_BASES || piece < 1) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t count = 0;
    if (fread(&count, sizeof count, 1, fh) != 1) return 2;
    const int slab = vbs_cells(max_bases);
    std::vector<long long> table((size_t)(2 * slab), 0);
    for (int64_t r = 0; r < count; ++r) {
        int64_t n = 0;
        if (fread(&n, sizeof n, 1, fh) != 1 || n < 0) return 2;
        if (n == 0) continue;
        unsigned char* y = static_cast<unsigned char*>(malloc((size_t)n));
        unsigned char* p = static_cast<unsigned char*>(malloc((size_t)n));
        unsigned char* b = static_cast<unsigned char*>(malloc((size_t)n));
        if (!y || !p || !b || fread(y, 1, (size_t)n, fh) != (size_t)n || fread(p, 1, (size_t)n, fh) != (size_t)n ||
            fread(b, 1, (size_t)n, fh) != (size_t)n) return 2;
        const int64_t n_words = (n >> 6) + 1;              // the word that holds position n closes the last run
        side truth = side_of(y, p, n, n_words), called = side_of(p, y, n, n_words);
        uint64_t* mark = words_of(b, n, n_words, [](unsigned char v) { return (v & 0x80u) != 0u; });
        uint64_t* const is[4] = {words_of(b, n, n_words, [](unsigned char v) { return v == (0x80u | 'A'); }),
                                 words_of(b, n, n_words, [](unsigned char v) { return v == (0x80u | 'C'); }),
                                 words_of(b, n, n_words, [](unsigned char v) { return v == (0x80u | 'G'); }),
                                 words_of(b, n, n_words, [](unsigned char v) { return v == (0x80u | 'T'); })};
        walk(truth, mark, is, n_words, piece, max_bases, table.data());
        walk(called, mark, is, n_words, piece, max_bases, table.data() + slab);
        free(y); free(p); free(b); free(mark);
        for (int c = 0; c < 4; ++c) free(is[c]);
        free(truth.run); free(truth.is1); free(truth.is0); free(called.run); free(called.is1); free(called.is0);
    }
    fclose(fh);
    for (int kind = 0; kind < 2; ++kind) {
        for (int c = 0; c < slab; ++c) printf(c ? " %lld" : "%lld", table[(size_t)(kind * slab + c)]);
        printf("\n");
    }
    return 0;
}
