// The run-state step of a validation round, word by word (plain C++17: g++ and hipcc both compile it; under hipcc the functions are
// __host__ __device__).  csrc/validation_runs.hpp runs these rules one 64-sample word per lane through csrc/validation_walk.hpp;
// tests/native/validation_runs_replay.cpp runs them serially under the sanitizers.  device_validation.run_states_host is the
// definition.
//
// A word is three masks: `run` (the array whose runs are counted, hp_loc_dict's last-sample rule already applied) and `is1` / `is0`
// (the other array is 1 / is 0).  Bit i is sample 64 * word + i; bits past the stretch are 0 in all.  A run is counted once, at its
// falling edge (the first sample after it; a run is closed at sample n by the word that holds position n).  The part of a run
// before the word arrives as a vr_seg -- length, all-ones, all-zeros -- and vr_join puts two stretches of words together, so the
// segs of all words come from a scan.  Inside a word the count steps from falling edge to falling edge (at most 32, alternating
// labels reach that) with bit operations.  No shift here is by 64 and no count of zeros is taken of 0: vb_low and vb_trailing
// guard vr_word's, and vr_count shifts by the ctz of a non-zero word.
#pragma once
#include "validation_borders_word.hpp"

#define CF_RUN_MAX_EDGES 7
#define CF_RUN_BINS (CF_RUN_MAX_EDGES + 1)
#define VR_CUT 1u          // the words of the seg are not all run (what came before cannot reach their end)
#define VR_ALL1 2u         // the other array is 1 over the whole open run
#define VR_ALL0 4u         // ... is 0 over it

struct cf_run_edges { unsigned e[CF_RUN_MAX_EDGES]; };     // ascending; unused ones 0xffffffff (no run is that long: total < 2^31)

// The run that is open at the end of a stretch of words.
struct vr_seg { uint32_t len, flags; };

VB_FN vr_seg vr_none() { return {0u, VR_CUT | VR_ALL1 | VR_ALL0}; }           // nothing open: what a stretch starts with

VB_FN vr_seg vr_join(const vr_seg a, const vr_seg b) {                         // the words of a, then those of b
    const bool cut = (b.flags & VR_CUT) != 0u;
    return {cut ? b.len : a.len + b.len, cut ? b.flags : ((a.flags & b.flags & (VR_ALL1 | VR_ALL0)) | (a.flags & VR_CUT))};
}

// the trailing run of one word (the ones that reach bit 63)
VB_FN vr_seg vr_word(uint64_t run, uint64_t is1, uint64_t is0) {
    const int t = vb_trailing(run);
    const uint64_t m = ~vb_low(64 - t);
    return {(uint32_t)t, (t < 64 ? VR_CUT : 0u) | ((is1 & m) == m ? VR_ALL1 : 0u) | ((is0 & m) == m ? VR_ALL0 : 0u)};
}

VB_FN unsigned vr_bin(uint32_t len, const cf_run_edges& edges) {               // searchsorted(edges, len, side="right")
    unsigned bin = 0;
    for (int j = 0; j < CF_RUN_MAX_EDGES; ++j) bin += len >= edges.e[j] ? 1u : 0u;
    return bin;
}

// The runs that END in this word (falling edges), `in` = the seg at the end of the word before.  `add(bin, all1, all0)` counts one
// run: complete when all1, else absent when all0, else incomplete (check_hp).
template <class Add>
VB_FN void vr_count(uint64_t run, uint64_t is1, uint64_t is0, const vr_seg in, const cf_run_edges& edges, Add&& add) {
    bool carried = in.len != 0u;
    const uint64_t before = (run << 1) | (carried ? 1ull : 0ull);
    uint64_t rise = run & ~before;
    for (uint64_t fall = ~run & before; fall; fall &= fall - 1ull) {
        const int e = __builtin_ctzll(fall);                                    // the run covers [s, e) of this word (+ in.len samples before it)
        int s = 0;
        uint32_t len = in.len, flags = in.flags;
        if (!carried) {
            s = __builtin_ctzll(rise);
            rise &= rise - 1ull;
            len = 0u;
            flags = VR_ALL1 | VR_ALL0;
        }
        carried = false;
        const uint64_t m = ((1ull << e) - 1ull) & ~((1ull << s) - 1ull);        // (e, s <= 63: each is the ctz of a non-zero word)
        add(vr_bin(len + (uint32_t)(e - s), edges), (flags & VR_ALL1) && (is1 & m) == m, (flags & VR_ALL0) && (is0 & m) == m);
    }
}

struct vr_rule {                                           // (what a walk asks of a step: vb_rule, validation_borders_word.hpp)
    typedef vr_seg seg;
    typedef vb_no_marks marks;
    cf_run_edges edges;
    VB_FN static seg none() { return vr_none(); }
    VB_FN static seg join(const seg a, const seg b) { return vr_join(a, b); }
    VB_FN static seg word(uint64_t run, uint64_t is1, uint64_t is0, const marks&) { return vr_word(run, is1, is0); }
    template <class Add>                                   // add(cell) of the [bin][state] table (the kernel packs its counts itself)
    VB_FN void events(uint64_t run, uint64_t is1, uint64_t is0, const marks&, const seg in, int64_t, bool, Add&& add) const {
        vr_count(run, is1, is0, in, edges, [&add](unsigned bin, bool all1, bool all0) { add((int)bin * 3 + (all1 ? 0 : all0 ? 2 : 1)); });
    }
};
