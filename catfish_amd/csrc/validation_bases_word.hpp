// The base step of a validation round, word by word (plain C++17: g++ and hipcc both compile it; under hipcc the functions are
// __host__ __device__).  csrc/validation_bases.hpp runs these rules one 64-sample word per lane; tests/native/
// validation_bases_replay.cpp runs them serially under the sanitizers.  device_validation.run_bases_host is the definition.
//
// A word of one kind is a vbs_masks: `run` (the array whose runs are counted, hp_loc_dict's last-sample rule already applied),
// `is1` / `is0` (the other array is 1 / is 0), `mark` (bit 7 of the base map: the centre sample of an event, one per base) and
// is[c] = "mark, and the base byte is 'A' / 'C' / 'G' / 'T'".  Bit i is sample 64 * word + i; bits past the stretch are 0 in all.
//
// What a run needs from BEFORE the word arrives as a vbs_seg, vr_seg (validation_runs_word.hpp) without the length and widened
// by the marks and the base of the open run, in one 32-bit word:
//   bit 0     VBS_CUT   the words of the seg are not all run (what came before cannot reach their end)
//   bit 1, 2  VBS_ALL1 / VBS_ALL0   the other array is 1 / is 0 over the whole open run
//   bit 3     VBS_OPEN  a run is open at the end
//   bits 4-6  base of the open run: 0 no mark yet, 1 .. 4 every mark so far is A / C / G / T, 5 anything else
//   bits 8-15 marks in the open run, saturating at VBS_MARK_CAP (no bin lies above 32; a saturating add is associative)
// vbs_join puts two such stretches of words together, so the segs of all words come from a scan.  A run is counted once, at its
// falling edge, from bit operations only.  No shift here is by 64 and no count of zeros is taken of 0: vb_low and vb_trailing guard both.
#pragma once
#include "validation_borders_word.hpp"

#define VBS_MAX_BASES 32
#define VBS_MARK_CAP 63u
#define VBS_CUT 1u
#define VBS_ALL1 2u
#define VBS_ALL0 4u
#define VBS_OPEN 8u
#define VBS_OTHER 5u           // base: mixed, 'N', lower case, ...
#define VBS_CLASSES 5          // A C G T other -- device_validation.BASE_CLASSES

typedef uint32_t vbs_seg;

struct vbs_masks { uint64_t run, is1, is0, mark, is[4]; };

struct vbs_base_marks {                                    // the masks of the base-map byte as a walk loads them (vb_no_marks'
    enum { N = 5 };                                        // interface): m[0] = mark, m[1 + c] = is[c]
    uint64_t m[N];
    VB_FN static bool is(int c, unsigned b) { return c == 0 ? (b & 0x80u) != 0u : b == (0x80u | (unsigned)"ACGT"[c - 1]); }
    VB_FN void set(int c, uint64_t v) { m[c] = v; }
    VB_FN vbs_masks word(uint64_t run, uint64_t is1, uint64_t is0) const { return {run, is1, is0, m[0], {m[1], m[2], m[3], m[4]}}; }
};

VB_FN vbs_seg vbs_none() { return VBS_CUT | VBS_ALL1 | VBS_ALL0; }               // nothing open: what a stretch starts with
VB_FN uint32_t vbs_base(vbs_seg v) { return (v >> 4) & 7u; }
VB_FN uint32_t vbs_marks(vbs_seg v) { return (v >> 8) & 0xffu; }
VB_FN vbs_seg vbs_pack(uint32_t flags, uint32_t base, uint32_t marks) { return flags | (base << 4) | (marks << 8); }

VB_FN uint32_t vbs_add_marks(uint32_t a, uint32_t b) { return a + b < VBS_MARK_CAP ? a + b : VBS_MARK_CAP; }
VB_FN uint32_t vbs_join_base(uint32_t a, uint32_t b) { return a == 0u ? b : (b == 0u || a == b) ? a : VBS_OTHER; }

// base of the marks `mk` (already cut to a run's samples): 0 without one, 1 .. 4 when every one is that letter, else 5
VB_FN uint32_t vbs_base_of(uint64_t mk, const vbs_masks& w) {
    if (mk == 0ull) return 0u;
    for (uint32_t c = 0; c < 4u; ++c)
        if ((mk & ~w.is[c]) == 0ull) return c + 1u;
    return VBS_OTHER;
}

// the trailing run of one word (the ones that reach bit 63)
VB_FN vbs_seg vbs_word(const vbs_masks& w) {
    const int t = vb_trailing(w.run);
    const uint64_t m = ~vb_low(64 - t);
    const uint64_t mk = w.mark & m;
    const uint32_t flags = (t < 64 ? VBS_CUT : 0u) | ((w.is1 & m) == m ? VBS_ALL1 : 0u) | ((w.is0 & m) == m ? VBS_ALL0 : 0u) | (t > 0 ? VBS_OPEN : 0u);
    return vbs_pack(flags, vbs_base_of(mk, w), vbs_add_marks((uint32_t)__builtin_popcountll(mk), 0u));
}

VB_FN vbs_seg vbs_join(const vbs_seg a, const vbs_seg b) {                       // the words of a, then those of b
    if (b & VBS_CUT) return b;
    // b is all run; a seg without an open run holds no mark and no base
    return vbs_pack((a & b & (VBS_ALL1 | VBS_ALL0)) | (a & VBS_CUT) | VBS_OPEN, vbs_join_base(vbs_base(a), vbs_base(b)),
                    vbs_add_marks(vbs_marks(a), vbs_marks(b)));
}

// cells of one (threshold, kind) slab: [state][class][bin], bin = min(marks, max_bases)
VB_FN int vbs_cells(int max_bases) { return 3 * VBS_CLASSES * (max_bases + 1); }
VB_FN int vbs_cell(int state, uint32_t base, uint32_t marks, int max_bases) {
    const int cls = base >= 1u && base <= 4u ? (int)base - 1 : 4;
    const int bin = marks < (uint32_t)max_bases ? (int)marks : max_bases;
    return (state * VBS_CLASSES + cls) * (max_bases + 1) + bin;
}

// The runs that END in this word (falling edges), `in` = the seg at the end of the word before.  `add(cell)` counts one run.
template <class Add>
VB_FN void vbs_count(const vbs_masks& w, const vbs_seg in, int max_bases, Add&& add) {
    bool carried = (in & VBS_OPEN) != 0u;
    const uint64_t before = (w.run << 1) | (carried ? 1ull : 0ull);
    uint64_t rise = w.run & ~before;
    for (uint64_t fall = ~w.run & before; fall; fall &= fall - 1ull) {
        const int e = __builtin_ctzll(fall);                                    // the run covers [s, e) of this word
        int s = 0;
        uint32_t flags = VBS_ALL1 | VBS_ALL0, base = 0u, marks = 0u;
        if (carried) {
            flags = in;
            base = vbs_base(in);
            marks = vbs_marks(in);
        } else {
            s = __builtin_ctzll(rise);
            rise &= rise - 1ull;
        }
        carried = false;
        const uint64_t m = vb_low(e) & ~vb_low(s);
        const uint64_t mk = w.mark & m;
        const bool all1 = (flags & VBS_ALL1) && (w.is1 & m) == m, all0 = (flags & VBS_ALL0) && (w.is0 & m) == m;
        base = vbs_join_base(base, vbs_base_of(mk, w));
        marks = vbs_add_marks(marks, (uint32_t)__builtin_popcountll(mk));
        add(vbs_cell(all1 ? 0 : all0 ? 2 : 1, base, marks, max_bases));         // complete / absent / incomplete (check_hp)
    }
}

struct vbs_rule {                                          // (what a walk asks of a step: vb_rule, validation_borders_word.hpp)
    typedef vbs_seg seg;
    typedef vbs_base_marks marks;
    int max_bases;
    VB_FN static seg none() { return vbs_none(); }
    VB_FN static seg join(const seg a, const seg b) { return vbs_join(a, b); }
    VB_FN static seg word(uint64_t run, uint64_t is1, uint64_t is0, const marks& mk) { return vbs_word(mk.word(run, is1, is0)); }
    template <class Add>
    VB_FN void events(uint64_t run, uint64_t is1, uint64_t is0, const marks& mk, const seg in, int64_t, bool, Add&& add) const {
        vbs_count(mk.word(run, is1, is0), in, max_bases, add);
    }
};
