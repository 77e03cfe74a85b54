// The score step of a validation round, word by word (plain C++17: g++ and hipcc both compile it; under hipcc the functions are
// __host__ __device__).  csrc/validation_scores.hpp runs these rules -- the paint one 64-sample word per lane through
// csrc/validation_walk.hpp, the key one thread per sample; tests/native/validation_scores_replay.cpp runs them serially under the
// sanitizers.  device_validation.run_scores_host is the definition.
//
// Paint: every sample of a run gets the run's state (check_hp: complete / incomplete / absent), so a word needs what a run holds
// BEFORE the word and AFTER it.  A word is three masks as in validation_runs_word.hpp: `run` (the array whose runs are painted,
// hp_loc_dict's last-sample rule already applied) and `is1` / `is0` (the other array is 1 / is 0).  The part before arrives as the
// forward walk's vr_seg (`in`: length, VR_ALL1, VR_ALL0); the part after is the same seg of the MIRRORED walk, cut down to three
// bits (vs_after: VS_OPEN when the run goes on behind bit 63, VR_ALL1 / VR_ALL0 over that part).  Inside a word the rule steps from
// run to run (at most 32, alternating labels reach that) with bit operations.  No shift here is by 64 and no count of zeros is
// taken of 0: vb_low guards the masks and every ctz is of a non-zero word.
//
// Key: a sample's cell in the flat [K][2][3][bins + 1] table -- the bin is csrc/validation_curve_bin.hpp's, cell `bins` of a row
// holds the fixed-point sum of bv_q (csrc/base_votes_rule.hpp, = base_votes.q_of).
#pragma once
#include "base_votes_rule.hpp"
#include "validation_curve_bin.hpp"
#include "validation_runs_word.hpp"

#define VS_SHIFT_MIN 14    // at 14 and sixteen thresholds the table is 6.2 M cells already
#define VS_SHIFT_MAX 22
#define VS_OPEN 1u         // vs_after: the run goes on behind the word (the bit VR_CUT takes in a seg)
#define VS_ROWS 6          // [kind][state] of one threshold
#define VS_NO_KEY 0xffffffffu      // no sample here; above every cell (16 * 6 * 65 026 at shift 14)

VB_FN bool vs_shift_ok(int shift) { return shift >= VS_SHIFT_MIN && shift <= VS_SHIFT_MAX; }

// cells of one (threshold, kind, state) row: the bins and the sum
VB_FN uint32_t vs_row_cells(int shift) { return vc_bins(shift) + 1u; }

// what a word keeps of the seg of the words AFTER it (the mirrored walk's `in`)
VB_FN uint32_t vs_after(const vr_seg in) { return (in.len != 0u ? VS_OPEN : 0u) | (in.flags & (VR_ALL1 | VR_ALL0)); }

// The samples of one word that lie in a complete / incomplete / absent run; c | i | a == run.
struct vs_paint { uint64_t c, i, a; };

VB_FN vs_paint vs_word(uint64_t run, uint64_t is1, uint64_t is0, const vr_seg in, uint32_t after) {
    vs_paint out = {0ull, 0ull, 0ull};
    for (uint64_t left = run; left;) {
        const int s = __builtin_ctzll(left);                                    // the run covers [s, e) of this word
        const uint64_t gaps = ~(left >> s);                                     // (s <= 63; above bit 63 - s only ones: the shift fills zeros)
        const int e = gaps ? s + __builtin_ctzll(gaps) : 64;                    // (gaps == 0: s == 0 and the word is all run)
        const uint64_t m = vb_low(e) & ~vb_low(s);
        bool all1 = (is1 & m) == m, all0 = (is0 & m) == m;
        if (s == 0 && in.len != 0u) {                                           // it began before the word
            all1 = all1 && (in.flags & VR_ALL1);
            all0 = all0 && (in.flags & VR_ALL0);
        }
        if (e == 64 && (after & VS_OPEN)) {                                     // it goes on behind it
            all1 = all1 && (after & VR_ALL1);
            all0 = all0 && (after & VR_ALL0);
        }
        if (all1) out.c |= m;                                                   // check_hp: complete, else absent, else incomplete
        else if (all0) out.a |= m;
        else out.i |= m;
        left &= ~m;
    }
    return out;
}

struct vs_rule {                                           // (what a walk asks of a step: vb_rule, validation_borders_word.hpp)
    typedef vr_seg seg;
    typedef vb_no_marks marks;
    VB_FN static seg none() { return vr_none(); }
    VB_FN static seg join(const seg a, const seg b) { return vr_join(a, b); }
    VB_FN static seg word(uint64_t run, uint64_t is1, uint64_t is0, const marks&) { return vr_word(run, is1, is0); }
};

// The paint of one sample, both kinds in a byte: bits 0-1 kind 0, bits 2-3 kind 1; 0 = in no run, else state + 1.
VB_FN unsigned vs_code(const vs_paint& p, int bit) {
    return (unsigned)((p.c >> bit) & 1ull) | ((unsigned)((p.i >> bit) & 1ull) << 1) | ((unsigned)((p.a >> bit) & 1ull) * 3u);
}
VB_FN unsigned vs_byte(const vs_paint& truth, const vs_paint& called, int bit) { return vs_code(truth, bit) | (vs_code(called, bit) << 2); }

// row of a painted sample within its threshold, kind * 3 + state, or -1 when the sample lies in no run of that kind
VB_FN int vs_row(unsigned byte, int kind) {
    const unsigned code = (byte >> (2 * kind)) & 3u;
    return code ? kind * 3 + (int)code - 1 : -1;
}

// the cell of (threshold k, row, bin) in the flat table; `bin` == vc_bins(shift) is the row's sum
VB_FN uint32_t vs_key(int k, int row, uint32_t bin, int shift) { return (uint32_t)(k * VS_ROWS + row) * vs_row_cells(shift) + bin; }
