// The two score kernels' bodies (catfish_amd/csrc/validation_scores.hpp), stated serially over catfish_amd/csrc/
// validation_scores_word.hpp: a stand-alone program that tests/test_run_scores_replay.py builds with g++ -fsanitize=address,
// undefined and holds to device_validation.run_scores_host.  Masks and their exactly sized buffers: validation_replay_common.hpp.
//
//   validation_scores_replay <batch file> <piece in words> <shift>      -> one line "row cell count" per non-zero cell, row = kind * 3 +
//                                                                          state, cell = bin or, for the fixed-point sum, the bins
//
// Batch file: int64 count, then per stretch int64 n, n label bytes, n bytes of corrected prediction and n float32 probabilities.
//
// Paint, as the kernel does it: the stretch is walked MIRRORED first, in pieces, and every word leaves what follows it (vs_after of
// the seg before it in walking order) in the paint byte of its first sample; then forward, where a word is painted from the seg
// before it and that byte, and every sample's byte is written.  The paint is a malloc'ed block of exactly n bytes.  Bin: every
// sample's keys (vs_row, vs_key) are counted and its bv_q summed.
#include "validation_replay_common.hpp"

#include <cstring>

#include "../../catfish_amd/csrc/validation_scores_word.hpp"

struct word_masks { uint64_t run, is1, is0; };

static word_masks word_of(const side& s, int64_t n_words, int64_t walked, bool mirror) {
    if (!mirror) return {s.run[walked], s.is1[walked], s.is0[walked]};
    const int64_t w = n_words - 1 - walked;
    return {vb_reverse(s.run[w]), vb_reverse(s.is1[w]), vb_reverse(s.is0[w])};
}

// One walk over both kinds in pieces of `piece` words; word(walked, in[2], masks[2]) sees the seg at the end of the word before.
template <class Word>
static void walk_both(const side (&kinds)[2], int64_t n_words, int64_t piece, bool mirror, Word&& word) {
    std::vector<vr_seg> inc[2] = {std::vector<vr_seg>((size_t)piece), std::vector<vr_seg>((size_t)piece)};
    vr_seg carry[2] = {vs_rule::none(), vs_rule::none()};
    for (int64_t w0 = 0; w0 < n_words; w0 += piece) {
        const int64_t count = n_words - w0 < piece ? n_words - w0 : piece;
        for (int q = 0; q < 2; ++q)
            for (int64_t i = 0; i < count; ++i) {
                const word_masks m = word_of(kinds[q], n_words, w0 + i, mirror);
                const vr_seg mine = vs_rule::word(m.run, m.is1, m.is0, {});
                inc[q][(size_t)i] = i ? vs_rule::join(inc[q][(size_t)i - 1], mine) : mine;
            }
        for (int64_t i = 0; i < count; ++i) {
            vr_seg in[2];
            word_masks m[2];
            for (int q = 0; q < 2; ++q) {
                in[q] = i ? vs_rule::join(carry[q], inc[q][(size_t)i - 1]) : carry[q];
                m[q] = word_of(kinds[q], n_words, w0 + i, mirror);
            }
            word(w0 + i, in, m);
        }
        for (int q = 0; q < 2; ++q) carry[q] = vs_rule::join(carry[q], inc[q][(size_t)count - 1]);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int64_t piece = atoll(argv[2]);
    const int shift = atoi(argv[3]);
    FILE* fh = fopen(argv[1], "rb");
    if (!fh || piece < 1 || !vs_shift_ok(shift)) return 2;
    const uint32_t bins = vc_bins(shift);
    std::vector<long long> table((size_t)VS_ROWS * vs_row_cells(shift), 0);
    int64_t* count = exactly<int64_t>(fh, 1);
    for (int64_t r = 0; r < *count; ++r) {
        int64_t* np = exactly<int64_t>(fh, 1);
        const int64_t n = *np;
        if (n < 0) return 2;
        if (n > 0) {
            unsigned char *y = exactly<unsigned char>(fh, n), *p = exactly<unsigned char>(fh, n);
            float* probs = exactly<float>(fh, n);
            unsigned char* paint = static_cast<unsigned char*>(malloc((size_t)n));
            if (!paint) return 3;
            memset(paint, 0xee, (size_t)n);                                    // a byte the walks leave behind shows as a wild row
            const side kinds[2] = {side_of(y, p, n), side_of(p, y, n)};
            const int64_t n_words = words_in(n);
            walk_both(kinds, n_words, piece, true, [&](int64_t walked, const vr_seg (&in)[2], const word_masks (&)[2]) {
                const int64_t at = (n_words - 1 - walked) * 64;
                if (at < n) paint[at] = (unsigned char)(vs_after(in[0]) | (vs_after(in[1]) << 3));
            });
            walk_both(kinds, n_words, piece, false, [&](int64_t walked, const vr_seg (&in)[2], const word_masks (&m)[2]) {
                const int64_t at = walked * 64;
                const unsigned after = at < n ? paint[at] : 0u;
                const vs_paint truth = vs_word(m[0].run, m[0].is1, m[0].is0, in[0], after & 7u);
                const vs_paint called = vs_word(m[1].run, m[1].is1, m[1].is0, in[1], (after >> 3) & 7u);
                for (int bit = 0; bit < 64 && at + bit < n; ++bit) paint[at + bit] = (unsigned char)vs_byte(truth, called, bit);
            });
            for (int64_t i = 0; i < n; ++i) {
                uint32_t bits;
                memcpy(&bits, &probs[i], sizeof bits);
                for (int kind = 0; kind < 2; ++kind) {
                    const int row = vs_row(paint[i], kind);
                    if (row < 0) continue;
                    ++table.at(vs_key(0, row, vc_bin(bits, shift), shift));
                    table.at(vs_key(0, row, bins, shift)) += (long long)bv_q(probs[i]);
                }
            }
            for (void* q : {(void*)y, (void*)p, (void*)probs, (void*)paint, (void*)kinds[0].run, (void*)kinds[0].is1, (void*)kinds[0].is0,
                            (void*)kinds[1].run, (void*)kinds[1].is1, (void*)kinds[1].is0}) free(q);
        }
        free(np);
    }
    free(count);
    fclose(fh);
    for (int row = 0; row < VS_ROWS; ++row)
        for (uint32_t c = 0; c <= bins; ++c)
            if (table[(size_t)row * vs_row_cells(shift) + c]) printf("%d %u %lld\n", row, c, table[(size_t)row * vs_row_cells(shift) + c]);
    return 0;
}
