// Bridging short gaps between called stretches: the bit logic of postprocess_bridged_kernel (csrc/ingest_post.hpp) on its 192-bit
// window (plain C++17: g++ and hipcc both compile it; under hipcc the functions are __host__ __device__).  catfish_amd/infer.py
// states the result in numpy (bridge_gaps is the definition); tests/native/post_bridge_replay.cpp replays a wave serially over
// these functions under the sanitizers.
//
// A window is three 64-sample words, bit b of a word = sample (word index * 64 + b): p the word before mine, m mine, n the next.
// `bits` holds the threshold bits of real samples only (padding is 0), `valid` the real samples, `first` the samples at which a
// read begins.  A maximal run of zeros INSIDE the real part of one read, at most max_gap long, with a one of the same read directly
// before and directly after it, becomes ones.  Zeros that touch a read's first or last real sample stay; nothing joins two reads,
// also where they are packed without padding.
//
// How: z = the zeros of real samples.  pb_open (the opening the kernel applies to the ones, cut where reads begin) gives the zero
// runs of more than max_gap samples; what is left of z are the short runs.  A short run is bounded by a one of its own read below
// iff any of its zeros has a one of the same read within max_gap samples below it (the run is maximal, so the nearest such one is
// its neighbour), and likewise above: two dilations of the ones that stop where a read begins, in doubling steps.
//
// What is exact: shifts move zeros in at the window's two ends, so long zero runs are known, and ones are found, only from samples
// inside the window.  The filled bits are exact from max_gap samples above the window's first sample to max_gap below its last;
// the opening by min_run - 1 that follows needs them exact min_run - 1 samples either side of the middle word and of its two
// neighbour bits: min_run + max_gap <= 64 (pb_domain).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PB_FN __host__ __device__ inline
#else
#define PB_FN inline
#endif

struct pb_w192 { uint64_t p, m, n; };

PB_FN pb_w192 pb_shr(const pb_w192& x, int s) {       // towards lower sample indices, 0 < s < 64
    return {(x.p >> s) | (x.m << (64 - s)), (x.m >> s) | (x.n << (64 - s)), x.n >> s};
}
PB_FN pb_w192 pb_shl(const pb_w192& x, int s) {       // towards higher sample indices, 0 < s < 64
    return {x.p << s, (x.m << s) | (x.p >> (64 - s)), (x.n << s) | (x.m >> (64 - s))};
}
PB_FN pb_w192 pb_and(const pb_w192& a, const pb_w192& b) { return {a.p & b.p, a.m & b.m, a.n & b.n}; }
PB_FN pb_w192 pb_or(const pb_w192& a, const pb_w192& b) { return {a.p | b.p, a.m | b.m, a.n | b.n}; }
PB_FN pb_w192 pb_not(const pb_w192& a) { return {~a.p, ~a.m, ~a.n}; }

// the pairs the bit-mask path takes (max_gap == 0 is the unbridged kernel's domain: min_run 1 .. 64)
PB_FN bool pb_domain(int min_run, int max_gap) { return min_run >= 1 && max_gap >= 0 && min_run + max_gap <= 64; }

// Every sample of a run of >= min_run ones that lies inside one read (1 <= min_run <= 64): erode by min_run - 1, dilate back.
// cut = ~first.  Stretches of `have` ones beginning at i and at i + have join only when no read begins at i + have; the last,
// overlapping step needs no such mask (its two stretches share samples).
PB_FN pb_w192 pb_open(pb_w192 x, const pb_w192& cut, int min_run) {
    int have = 1;
    while (2 * have <= min_run) {
        x = pb_and(x, pb_shr(pb_and(x, cut), have));
        have *= 2;
    }
    if (have < min_run) x = pb_and(x, pb_shr(x, min_run - have));
    have = 1;
    while (2 * have <= min_run) {
        x = pb_or(x, pb_shl(x, have));
        have *= 2;
    }
    if (have < min_run) x = pb_or(x, pb_shl(x, min_run - have));
    return x;
}

// The window with its short gaps filled (1 <= max_gap <= 63).
PB_FN pb_w192 pb_fill(const pb_w192& bits, const pb_w192& valid, const pb_w192& first, int max_gap) {
    const pb_w192 cut = pb_not(first);
    const pb_w192 z = pb_and(pb_not(bits), valid);
    const pb_w192 is_short = pb_and(z, pb_not(pb_open(z, cut, max_gap + 1)));
    // up: a one of the same read at most `reach` samples below; dn: above.  free_up: no read begins in the s samples up to and
    // including mine (what a shift by s up must not cross); free_dn: none in the s samples after mine.  (Zeros move in at the
    // window's ends: nothing is found from beyond them.)  The steps double, so the reach ends at the first 2^k - 1 >= max_gap, which
    // may be MORE than max_gap (3 for max_gap 2).  That is safe: up and dn only decide for zeros of a SHORT run, whose length is_short
    // already bounds.  Such a run is maximal inside its read, so whatever one of the same read is found below it, at any distance,
    // has the run's lower neighbour between itself and the run -- a real sample of that read that is no zero of the run: a one.
    // Reaching too far can therefore not fill a run that has no one next to it; it only must not reach too SHORT (>= max_gap).
    pb_w192 up = bits, dn = bits, free_up = cut, free_dn = pb_shr(cut, 1);
    for (int s = 1, reach = 0; reach < max_gap; reach += s, s *= 2) {      // s = 1, 2, 4, .. 32: reach 2 s - 1 <= 63 afterwards
        up = pb_or(up, pb_and(pb_shl(up, s), free_up));
        dn = pb_or(dn, pb_and(pb_shr(dn, s), free_dn));
        if (reach + s < max_gap) {
            free_up = pb_and(free_up, pb_shl(free_up, s));
            free_dn = pb_and(free_dn, pb_shr(free_dn, s));
        }
    }
    return pb_or(bits, pb_and(is_short, pb_and(up, dn)));
}
