// What validation_runs_replay.cpp, validation_borders_replay.cpp and validation_bases_replay.cpp share: the walk of catfish_amd/
// csrc/validation_walk.hpp, stated serially over the rule type of the step (vr_rule, vb_rule, vbs_rule: the word headers the
// kernels run one word per lane).
//
// Batch file: int64 count, then per stretch int64 n, n label bytes, n bytes of corrected prediction (both 0 / 1; anything else is
// neither, as in the kernels) and, for a rule with marks, n bytes of base map.  Output: two lines (kind 0, kind 1) of `cells`
// counts, summed over the stretches.
//
// Per stretch every mask sits in an exactly sized malloc'ed buffer of n / 64 + 1 words, so a word index that is off by one is a
// heap overflow the sanitizer reports.  As in the kernels a stretch is walked in pieces, forward and -- for the border step --
// mirrored (last word first, every word bit-reversed): inside a piece the seg at the end of every word is an inclusive scan with
// the rule's join that starts from nothing, and what is open from the pieces before comes in as a carry.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../catfish_amd/csrc/validation_borders_word.hpp"

static int64_t words_in(int64_t n) { return (n >> 6) + 1; }                     // the word that holds position n closes the last run

template <class Pred>
static uint64_t* words_of(const unsigned char* v, int64_t n, Pred&& pred) {
    const int64_t n_words = words_in(n);
    uint64_t* w = static_cast<uint64_t*>(malloc((size_t)n_words * sizeof(uint64_t)));
    if (!w) exit(3);
    for (int64_t j = 0; j < n_words; ++j) w[j] = 0ull;
    for (int64_t i = 0; i < n; ++i)
        if (pred(v[i])) w[i >> 6] |= 1ull << (i & 63);
    return w;
}

struct side { uint64_t *run, *is1, *is0; };                // one kind: the runs of `mine` judged against `other`

static side side_of(const unsigned char* mine, const unsigned char* other, int64_t n) {
    side s = {words_of(mine, n, [](unsigned b) { return b == 1u; }), words_of(other, n, [](unsigned b) { return b == 1u; }),
              words_of(other, n, [](unsigned b) { return b == 0u; })};
    if (n >= 2 && mine[n - 2] == 1u) s.run[(n - 1) >> 6] |= 1ull << ((n - 1) & 63);          // hp_loc_dict closes an open run AT the last sample
    return s;
}

template <class Rule>
static void walk(const Rule& rule, const side& s, uint64_t* const* mk, int64_t n_words, int64_t piece, bool mirror, long long* row) {
    typedef typename Rule::seg seg;
    std::vector<seg> inc((size_t)piece);
    seg carry = Rule::none();
    auto word = [&](const uint64_t* m, int64_t w) { return mirror ? vb_reverse(m[n_words - 1 - w]) : m[w]; };
    auto marks = [&](int64_t w) {
        typename Rule::marks m{};
        for (int c = 0; c < Rule::marks::N; ++c) m.set(c, word(mk[c], w));
        return m;
    };
    for (int64_t w0 = 0; w0 < n_words; w0 += piece) {
        const int64_t count = n_words - w0 < piece ? n_words - w0 : piece;
        for (int64_t i = 0; i < count; ++i) {
            const seg mine = Rule::word(word(s.run, w0 + i), word(s.is1, w0 + i), word(s.is0, w0 + i), marks(w0 + i));
            inc[(size_t)i] = i ? Rule::join(inc[(size_t)i - 1], mine) : mine;
        }
        for (int64_t i = 0; i < count; ++i) {
            const seg in = i ? Rule::join(carry, inc[(size_t)i - 1]) : carry;
            rule.events(word(s.run, w0 + i), word(s.is1, w0 + i), word(s.is0, w0 + i), marks(w0 + i), in, (w0 + i) * 64, mirror,
                        [&](int cell) { ++row[cell]; });
        }
        carry = Rule::join(carry, inc[(size_t)count - 1]);
    }
}

template <class T>
static T* exactly(FILE* fh, int64_t n) {                    // n values in a block of exactly n * sizeof(T) bytes
    T* p = static_cast<T*>(malloc((size_t)n * sizeof(T)));
    if (!p || fread(p, sizeof(T), (size_t)n, fh) != (size_t)n) exit(2);
    return p;
}

// The whole program behind the arguments: `cells` per kind, `mirrored` = walk every stretch a second time, mirrored.
template <class Rule>
static int replay(const char* path, const Rule& rule, int64_t piece, int cells, bool mirrored) {
    FILE* fh = fopen(path, "rb");
    if (!fh || piece < 1) return 2;
    int64_t* count = exactly<int64_t>(fh, 1);
    std::vector<long long> table((size_t)(2 * cells), 0);
    for (int64_t r = 0; r < *count; ++r) {
        int64_t* n = exactly<int64_t>(fh, 1);
        if (*n < 0) return 2;
        if (*n > 0) {
            unsigned char *y = exactly<unsigned char>(fh, *n), *p = exactly<unsigned char>(fh, *n);
            unsigned char* b = Rule::marks::N > 0 ? exactly<unsigned char>(fh, *n) : nullptr;
            const side truth = side_of(y, p, *n), called = side_of(p, y, *n);
            uint64_t* mk[Rule::marks::N + 1];
            for (int c = 0; c < Rule::marks::N; ++c) mk[c] = words_of(b, *n, [c](unsigned v) { return Rule::marks::is(c, v); });
            for (int mirror = 0; mirror <= (mirrored ? 1 : 0); ++mirror) {
                walk(rule, truth, mk, words_in(*n), piece, mirror != 0, table.data());
                walk(rule, called, mk, words_in(*n), piece, mirror != 0, table.data() + cells);
            }
            for (int c = 0; c < Rule::marks::N; ++c) free(mk[c]);
            for (void* q : {(void*)y, (void*)p, (void*)b, (void*)truth.run, (void*)truth.is1, (void*)truth.is0, (void*)called.run,
                            (void*)called.is1, (void*)called.is0}) free(q);
        }
        free(n);
    }
    free(count);
    fclose(fh);
    for (int kind = 0; kind < 2; ++kind) {
        for (int c = 0; c < cells; ++c) printf(c ? " %lld" : "%lld", table[(size_t)(kind * cells + c)]);
        printf("\n");
    }
    return 0;
}
