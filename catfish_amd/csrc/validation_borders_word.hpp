// The border step of a validation round, word by word (plain C++17: g++ and hipcc both compile it; under hipcc the functions are
// __host__ __device__).  csrc/validation_borders.hpp runs these rules one 64-sample word per lane; tests/native/
// validation_borders_replay.cpp runs them serially under the sanitizers.  device_validation.run_borders_host is the definition.
//
// A word is two masks: `run` (the array whose runs are judged, hp_loc_dict's last-sample rule already applied) and `o` (the other
// array is 1).  Bit i is sample 64 * word + i; bits past the stretch are 0 in both.  Everything a run needs from BEFORE the word
// arrives as a vb_seg -- how long the run open at the end of the words so far is, how long the stretch of equal values of `o`
// there is, and a few facts about the open run -- and vb_join puts two such stretches of words together, so the segs of all words
// come from a scan.  What a run needs from AFTER it is what the same rules give on the mirrored stretch (bit-reversed words, last
// word first): the right offset of a run is minus the left offset of its mirror image.
//
//   left offset l of a run [s, e] that is not absent, counted where it is known from the past alone:
//     o[s] == 1: at s, l = -(ones of o ending at s - 1), position 0 not counted (check_hp's `not position <= 0`; forward only)
//     o[s] == 0: at f, the first one of o in the run -- o rises at f, run[f] == 1 and the M >= 1 run samples ending at f - 1 all
//                lie in the Z zeros of o ending there (M <= Z): l = M
//   interruption: o rises at f, run[f] == 1 and M > Z >= 1: the Z zeros lie strictly inside the run, g = Z
//   interrupted run: at its falling edge, when the open run held two ones of o with a zero between them
//
// No shift here is by 64 and no count of leading zeros is taken of 0: vb_low and vb_top guard both.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VB_FN __host__ __device__ inline
#else
#define VB_FN inline
#endif

#define VB_MAX_REACH 128
#define VB_CUT 1u          // the words of the seg are not all run (what came before cannot reach their end)
#define VB_ANY 2u          // o is 1 somewhere in the open run
#define VB_INT 4u          // ... twice, with a zero between
#define VB_F1 8u           // o is 1 at the first sample of the open run (as far as these words hold it)
#define VB_OVAL 16u        // o at the last sample
#define VB_OMIX 32u        // o is not one value over all the words (o_cnt does not reach their start)

// The end of a stretch of words: run_len run samples and o_cnt equal values of o end there.
struct vb_seg { uint32_t run_len, o_cnt, flags; };

VB_FN vb_seg vb_none() { return {0u, 0u, VB_CUT | VB_OMIX}; }                  // what a stretch starts with

VB_FN uint64_t vb_low(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1ull; }  // bits below k, k in 0 .. 64
VB_FN int vb_top(uint64_t x) { return 63 - __builtin_clzll(x); }               // highest set bit, x != 0
VB_FN int vb_trailing(uint64_t x) { return ~x ? __builtin_clzll(~x) : 64; }    // how many ones reach bit 63
VB_FN uint64_t vb_reverse(uint64_t x) {                                        // bit i <-> bit 63 - i: a word of the mirrored stretch
#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse64)
#define VB_HAS_BITREVERSE 1
#endif
#endif
#ifdef VB_HAS_BITREVERSE
    return __builtin_bitreverse64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(x);
#endif
}
VB_FN bool vb_two_blocks(uint64_t x) {                                         // two ones of x with a zero between them
    const uint64_t starts = x & ~(x << 1);
    return (starts & (starts - 1ull)) != 0ull;
}
// how many ones of x end just below bit f (f in 1 .. 63); `reached` when they go down to bit 0
VB_FN uint32_t vb_ones_below(uint64_t x, int f, bool& reached) {
    const uint64_t gaps = ~x & vb_low(f);
    reached = gaps == 0ull;
    return (uint32_t)(reached ? f : f - 1 - vb_top(gaps));
}

VB_FN vb_seg vb_word(uint64_t run, uint64_t o) {
    const int t = vb_trailing(run);
    const uint64_t x = o & ~vb_low(64 - t);
    uint32_t flags = (t < 64 ? VB_CUT : 0u) | (x ? VB_ANY : 0u) | (vb_two_blocks(x) ? VB_INT : 0u);
    if (t > 0 && ((o >> (64 - t)) & 1ull)) flags |= VB_F1;
    const bool last = (o >> 63) != 0ull;
    const int c = vb_trailing(last ? o : ~o);
    flags |= (last ? VB_OVAL : 0u) | (c < 64 ? VB_OMIX : 0u);
    return {(uint32_t)t, (uint32_t)c, flags};
}

VB_FN vb_seg vb_join(const vb_seg a, const vb_seg b) {                          // the words of a, then those of b
    vb_seg r = b;
    if (!(b.flags & VB_OMIX)) {
        const bool same = ((a.flags ^ b.flags) & VB_OVAL) == 0u;
        r.o_cnt = same ? a.o_cnt + b.o_cnt : b.o_cnt;
        r.flags = (r.flags & ~VB_OMIX) | (same ? (a.flags & VB_OMIX) : VB_OMIX);
    }
    if (!(b.flags & VB_CUT)) {                                                  // b is all run
        if (a.run_len == 0u) {
            r.flags |= VB_CUT;
        } else {
            const bool both = (a.flags & VB_ANY) && (b.flags & VB_ANY);
            const bool touch = (a.flags & VB_OVAL) && (b.flags & VB_F1);
            r.run_len = a.run_len + b.run_len;
            r.flags = (r.flags & ~(VB_CUT | VB_ANY | VB_INT | VB_F1)) | (a.flags & (VB_CUT | VB_F1)) | ((a.flags | b.flags) & (VB_ANY | VB_INT)) |
                      (both && !touch ? VB_INT : 0u);
        }
    }
    return r;
}

// cells of one (threshold, kind) row -- device_validation.split_run_borders
VB_FN int vb_cells(int reach) { return 5 * reach + 3; }
VB_FN uint32_t vb_clip(uint32_t v, int reach) { return v < (uint32_t)reach ? v : (uint32_t)reach; }
VB_FN int vb_cell_offset(bool right, bool beyond, uint32_t by, int reach) {     // beyond: the other array's ones reach past the run
    const int at = (int)vb_clip(by, reach);
    return (right ? 2 * reach + 1 : 0) + reach + ((right ? beyond : !beyond) ? at : -at);
}
VB_FN int vb_cell_gap(uint32_t g, int reach) { return 4 * reach + 2 + (int)vb_clip(g, reach) - 1; }
VB_FN int vb_cell_interrupted(int reach) { return 5 * reach + 2; }

// The events of one word: `in` = the seg at the end of the word before, `first` = the stretch's position of bit 0.  Forward walk
// (mirror == false): left offsets, interruptions and interrupted runs; mirrored walk: the right offsets only (no position-0 rule).
// `add(cell)` counts one event.
template <class Add>
VB_FN void vb_events(uint64_t run, uint64_t o, const vb_seg in, int64_t first, bool mirror, int reach, Add&& add) {
    const bool in_one = (in.flags & VB_OVAL) != 0u;
    const uint32_t ones_in = in_one ? in.o_cnt : 0u, zeros_in = in_one ? 0u : in.o_cnt;
    const uint64_t before = (run << 1) | (in.run_len ? 1ull : 0ull);
    bool reached;
    // runs that start on a one of o: the other array's ones reach `a` samples past the border
    for (uint64_t rise = run & ~before & o; rise; rise &= rise - 1ull) {
        const int s = __builtin_ctzll(rise);
        uint32_t a = ones_in;
        if (s > 0) {
            a = vb_ones_below(o, s, reached);
            if (reached) a += ones_in;
        }
        if (!mirror && a > 0u && (int64_t)a == first + s) --a;                 // ... but never as far as position 0
        add(vb_cell_offset(mirror, true, a, reach));
    }
    // o rises inside a run: the first one of o in it (the border is called M late), or the end of an interruption
    for (uint64_t up = o & ~((o << 1) | (in_one ? 1ull : 0ull)) & run; up; up &= up - 1ull) {
        const int f = __builtin_ctzll(up);
        uint32_t z = zeros_in, m = in.run_len;
        if (f > 0) {
            z = vb_ones_below(~o, f, reached);
            if (reached) z += zeros_in;
            m = vb_ones_below(run, f, reached);
            if (reached) m += in.run_len;
        }
        if (m == 0u) continue;                                                 // the run starts here (counted above)
        if (m <= z) add(vb_cell_offset(mirror, false, m, reach));
        else if (!mirror) add(vb_cell_gap(z, reach));
    }
    if (mirror) return;
    // runs that end here: interrupted or not
    bool carried = in.run_len != 0u;
    uint64_t starts = run & ~before;
    for (uint64_t fall = ~run & before; fall; fall &= fall - 1ull) {
        const int e = __builtin_ctzll(fall);                                   // the run covers [s, e) of this word
        int s = 0;
        if (!carried) {
            s = __builtin_ctzll(starts);
            starts &= starts - 1ull;
        }
        const uint64_t x = o & vb_low(e) & ~vb_low(s);
        bool cut = vb_two_blocks(x);
        if (carried)
            cut = cut || (in.flags & VB_INT) || ((in.flags & VB_ANY) && x && !(in_one && (o & 1ull)));
        carried = false;
        if (cut) add(vb_cell_interrupted(reach));
    }
}

// What a walk (csrc/validation_walk.hpp on the card, tests/native/validation_replay_common.hpp serially) asks of a step: its seg
// with none / word / join, the masks it takes from a third byte per sample (`marks`: N masks, mask c holds the samples whose byte
// `is(c, byte)`; here none), and the events of one word of one kind -- run / is1 / is0 as above, `first` = the stretch's position of
// bit 0 in walking order.  validation_runs_word.hpp and validation_bases_word.hpp state theirs the same way.
struct vb_no_marks {
    enum { N = 0 };
    VB_FN static bool is(int, unsigned) { return false; }
    VB_FN void set(int, uint64_t) {}
    VB_FN vb_no_marks mirrored() const { return {}; }
};

struct vb_rule {
    typedef vb_seg seg;
    typedef vb_no_marks marks;
    int reach;
    VB_FN static seg none() { return vb_none(); }
    VB_FN static seg join(const seg a, const seg b) { return vb_join(a, b); }
    VB_FN static seg word(uint64_t run, uint64_t is1, uint64_t, const marks&) { return vb_word(run, is1); }
    template <class Add>
    VB_FN void events(uint64_t run, uint64_t is1, uint64_t, const marks&, const seg in, int64_t first, bool mirror, Add&& add) const {
        vb_events(run, is1, in, first, mirror, reach, add);
    }
};
