// The border kernel's body (catfish_amd/csrc/validation_borders.hpp), stated serially over catfish_amd/csrc/
// validation_borders_word.hpp: a stand-alone program that tests/test_run_borders_replay.py builds with g++ -fsanitize=address,
// undefined and holds to device_validation.run_borders_host.
//
//   validation_borders_replay <batch file> <reach> <piece in words>
//
// Batch file: int64 count, then per stretch int64 n, n label bytes, n bytes of corrected prediction (both 0 / 1; anything else
// counts as 0, as in the kernel).  Output: two lines (kind 0, kind 1) of 5 * reach + 3 counts, summed over the stretches.
//
// Per stretch the four masks sit in exactly sized malloc'ed buffers of n / 64 + 1 words, so a word index that is off by one is a
// heap overflow the sanitizer reports.  As in the kernel a stretch is walked twice in pieces: forward (left offsets, interruptions)
// and mirrored -- last word first, every word bit-reversed -- for the right offsets; inside a piece the seg at the end of every
// word is an inclusive scan with vb_join that starts from nothing, and what is open from the pieces before comes in as a carry.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../catfish_amd/csrc/validation_borders_word.hpp"

static uint64_t* words_of(const unsigned char* v, int64_t n, int64_t n_words, bool last_rule) {
    uint64_t* w = static_cast<uint64_t*>(malloc((size_t)n_words * sizeof(uint64_t)));
    if (!w) exit(3);
    for (int64_t j = 0; j < n_words; ++j) w[j] = 0ull;
    for (int64_t i = 0; i < n; ++i)
        if (v[i] == 1u) w[i >> 6] |= 1ull << (i & 63);
    if (last_rule && n >= 2 && v[n - 2] == 1u) w[(n - 1) >> 6] |= 1ull << ((n - 1) & 63);     // hp_loc_dict closes an open run AT the last sample
    return w;
}

static void walk(const uint64_t* run, const uint64_t* o, int64_t n_words, int64_t piece, bool mirror, int reach, long long* row) {
    std::vector<vb_seg> inc((size_t)piece);
    vb_seg carry = vb_none();
    auto word = [&](const uint64_t* m, int64_t w) { return mirror ? vb_reverse(m[n_words - 1 - w]) : m[w]; };
    for (int64_t w0 = 0; w0 < n_words; w0 += piece) {
        const int64_t count = n_words - w0 < piece ? n_words - w0 : piece;
        for (int64_t i = 0; i < count; ++i) {
            const vb_seg mine = vb_word(word(run, w0 + i), word(o, w0 + i));
            inc[(size_t)i] = i ? vb_join(inc[(size_t)i - 1], mine) : mine;
        }
        for (int64_t i = 0; i < count; ++i) {
            const vb_seg in = i ? vb_join(carry, inc[(size_t)i - 1]) : carry;
            vb_events(word(run, w0 + i), word(o, w0 + i), in, (w0 + i) * 64, mirror, reach, [&](int cell) { ++row[cell]; });
        }
        carry = vb_join(carry, inc[(size_t)count - 1]);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int reach = atoi(argv[2]);
    const int64_t piece = atoll(argv[3]);
    if (reach < 1 || reach > VB_MAX_REACH || piece < 1) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t count = 0;
    if (fread(&count, sizeof count, 1, fh) != 1) return 2;
    std::vector<long long> table((size_t)(2 * vb_cells(reach)), 0);
    for (int64_t r = 0; r < count; ++r) {
        int64_t n = 0;
        if (fread(&n, sizeof n, 1, fh) != 1 || n < 0) return 2;
        if (n == 0) continue;
        unsigned char* y = static_cast<unsigned char*>(malloc((size_t)n));
        unsigned char* p = static_cast<unsigned char*>(malloc((size_t)n));
        if (!y || !p || fread(y, 1, (size_t)n, fh) != (size_t)n || fread(p, 1, (size_t)n, fh) != (size_t)n) return 2;
        const int64_t n_words = (n >> 6) + 1;              // the word that holds position n closes the last run
        uint64_t* y1 = words_of(y, n, n_words, false);
        uint64_t* p1 = words_of(p, n, n_words, false);
        uint64_t* run_y = words_of(y, n, n_words, true);
        uint64_t* run_p = words_of(p, n, n_words, true);
        for (int mirror = 0; mirror < 2; ++mirror) {
            walk(run_y, p1, n_words, piece, mirror != 0, reach, table.data());
            walk(run_p, y1, n_words, piece, mirror != 0, reach, table.data() + vb_cells(reach));
        }
        free(y); free(p); free(y1); free(p1); free(run_y); free(run_p);
    }
    fclose(fh);
    for (int kind = 0; kind < 2; ++kind) {
        for (int c = 0; c < vb_cells(reach); ++c) printf(c ? " %lld" : "%lld", table[(size_t)(kind * vb_cells(reach) + c)]);
        printf("\n");
    }
    return 0;
}
