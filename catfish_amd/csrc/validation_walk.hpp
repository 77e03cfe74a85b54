// The walk the three run steps of a validation round share (validation_runs.hpp, validation_borders.hpp, validation_bases.hpp):
// a workgroup walks one stretch of corrected labels and truth in pieces of CF_RUN_PIECE samples, one 64-sample word per lane, and
// hands every lane the masks of its word together with the seg at the end of the word before -- what the step's word rule
// (validation_runs_word.hpp, validation_borders_word.hpp, validation_bases_word.hpp: plain C++, read those first) needs to count the
// events of the word from bit operations alone.  No lane walks the samples of a run, so a stretch of ones costs what a stretch of
// zeros costs.  tests/native/validation_replay_common.hpp states the same walk serially under the sanitizers.
//
// Per threshold the post-processing kernel writes the corrected labels of the whole packed batch into its slice of `work`
// (validation_label_passes, validation_runs.hpp); ONE launch of the step's kernel then counts, blockIdx.x striding over the stretches and
// blockIdx.y over the thresholds (cf_walk_stretches).  Counts are integers and reach the zeroed table by integer atomics: equal
// inputs give equal bits whatever the grid.
//
// A step on the card is its word rule (vr_rule, vb_rule, vbs_rule) and
//   shfl_up(seg, d)                                   the seg of the lane d below
//   byte(i)                                           the byte of sample i that the rule's marks are taken from (0 without marks)
//   count(q, run, is1, is0, marks, in, first, mirror) the events of one word of kind q, into the step's own counters
//   piece_counts() / piece_totals()                   what it does with a piece's counts before / after the piece's second barrier
#pragma once
#include "validation_borders_word.hpp"

#define CF_RUN_THREADS 256
#define CF_RUN_WAVES (CF_RUN_THREADS / 64)
#define CF_RUN_PIECE (CF_RUN_THREADS * 64)

// One walk over the stretch [b0, b0 + n) of (threshold slice p, labels y): forward, or MIRRORed -- the last word first, every word
// bit-reversed, lanes and pieces in that order (what lies AFTER a run is what lies before its mirror image).  Kind 0: the runs of
// y == 1 judged against p; kind 1: the runs of p == 1 judged against y.
//
// Barriers, two per piece: (A) is behind the piece's write of s_seg and behind the step's piece_totals() of the piece before, so
// piece_counts() may write the step's LDS rows again; (B) is behind every read of s_seg, so the next piece -- or the next walk --
// may write it again, behind piece_counts(), so piece_totals() may read its rows, and behind every LDS add of count(), so a table
// may be flushed after the last piece.
template <class Step, bool MIRROR>
__device__ __forceinline__ void cf_walk(Step& step, const uint8_t* __restrict__ p, const uint8_t* __restrict__ y, int64_t b0, int64_t n,
                                        int64_t total, typename Step::seg (&s_seg)[CF_RUN_WAVES][2]) {
    typedef typename Step::seg seg;
    typedef typename Step::marks marks;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t n_words = (n >> 6) + 1;                                          // the word that holds position n closes the last run
    seg carry[2] = {Step::none(), Step::none()};
    for (int64_t w0 = 0; w0 < n_words; w0 += CF_RUN_THREADS) {
        // 1. masks: 64 coalesced byte loads + ballots per wave; word j of this wave's 64 (in walking order) lands in lane j.  A
        //    sample past the stretch is neither 0 nor 1 and has no mark.
        const int64_t wave_word = w0 + (int64_t)wave * 64;
        unsigned long long y1 = 0, y0 = 0, p1 = 0, p0 = 0;
        marks mk = {};
#pragma unroll 1                                                                   // (every pass waits for its own loads: two per trip only add branches)
        for (int j = 0; j < 64; ++j) {
            if (wave_word + j >= n_words) break;                                   // (uniform)
            const int64_t i = (MIRROR ? n_words - 1 - (wave_word + j) : wave_word + j) * 64 + lane;
            unsigned yv = 0xffu, pv = 0xffu, bv = 0u;
            if (i < n) {
                if ((uint64_t)(b0 + i) < (uint64_t)total) {
                    yv = y[b0 + i];
                    pv = p[b0 + i];
                }
                bv = step.byte(i);
            }
            const unsigned long long by1 = __ballot(yv == 1u), by0 = __ballot(yv == 0u);
            const unsigned long long bp1 = __ballot(pv == 1u), bp0 = __ballot(pv == 0u);
            marks bm = {};
#pragma unroll
            for (int c = 0; c < marks::N; ++c) bm.set(c, __ballot(marks::is(c, bv)));
            if ((int)lane == j) { y1 = by1; y0 = by0; p1 = bp1; p0 = bp0; mk = bm; }      // (one branch for all the masks of the word)
        }
        unsigned long long run_y = y1, run_p = p1;
        const int64_t walked = wave_word + lane, word = MIRROR ? n_words - 1 - walked : walked;
        if (n >= 2 && word == ((n - 1) >> 6) && (uint64_t)(b0 + n - 2) < (uint64_t)total) {   // hp_loc_dict closes an open run AT the last sample
            const unsigned long long last = 1ull << ((n - 1) & 63);                // (only the RUN mask changes, never what a run is judged against)
            if (y[b0 + n - 2] == 1u) run_y |= last;
            if (p[b0 + n - 2] == 1u) run_p |= last;
        }
        if constexpr (MIRROR) {
            y1 = vb_reverse(y1); y0 = vb_reverse(y0); p1 = vb_reverse(p1); p0 = vb_reverse(p0);
            run_y = vb_reverse(run_y); run_p = vb_reverse(run_p); mk = mk.mirrored();
        }
        // 2. the seg at the end of every word: an inclusive segmented scan with the rule's join over the lanes of a wave by
        //    shuffles, over the four waves through LDS, and from piece to piece in a carry every thread keeps
        seg inc[2] = {Step::word(run_y, p1, p0, mk), Step::word(run_p, y1, y0, mk)};
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const seg o = Step::shfl_up(inc[q], d);
                if ((int)lane >= d) inc[q] = Step::join(o, inc[q]);
            }
        }
        if (lane == 63u) { s_seg[wave][0] = inc[0]; s_seg[wave][1] = inc[1]; }
        __syncthreads();                                                           // (A)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            seg in = carry[q];                                                     // at the end of the word before mine
#pragma unroll
            for (int v = 0; v < CF_RUN_WAVES; ++v) {
                const seg t = s_seg[v][q];
                if (v < (int)wave) in = Step::join(in, t);
                carry[q] = Step::join(carry[q], t);                                // (every thread: the piece's total)
            }
            const seg left = Step::shfl_up(inc[q], 1);
            if (lane != 0u) in = Step::join(in, left);
            // 3. the events of my word (a word past the stretch holds no bit: no event)
            step.count(q, q == 0 ? run_y : run_p, q == 0 ? p1 : y1, q == 0 ? p0 : y0, mk, in, walked * 64, MIRROR);
        }
        step.piece_counts();
        __syncthreads();                                                           // (B)
        step.piece_totals();
    }
}

// The stretches and thresholds of one workgroup: stretch(k, r, p, b0, n) for every non-empty stretch r of every threshold k of its,
// p = the threshold's label slice.  Uniform over the workgroup, so `stretch` may hold barriers.
template <class Stretch>
__device__ __forceinline__ void cf_walk_stretches(const uint8_t* __restrict__ pred, int64_t pred_stride, const int64_t* __restrict__ bounds,
                                                  const int64_t* __restrict__ length, int64_t n_reads, int K, Stretch&& stretch) {
    for (int k = blockIdx.y; k < K; k += gridDim.y) {
        for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
            const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
            const int64_t n = length[r] < size ? length[r] : size;                 // the zero tail is not part of the stretch
            if (n > 0) stretch(k, r, pred + (int64_t)k * pred_stride, b0, n);
        }
    }
}

// The counters of a step that counts by integer LDS adds (borders, bases): one table per workgroup, `cells` per kind, which goes
// to the zeroed output with one 64-bit integer atomic per non-zero cell at the end of a stretch.
struct cf_walk_table {
    unsigned* tab;
    int cells;
    __device__ void zero() const {
        for (int c = threadIdx.x; c < 2 * cells; c += CF_RUN_THREADS) tab[c] = 0u;
        __syncthreads();
    }
    __device__ void add(int q, int cell) const { atomicAdd(&tab[q * cells + cell], 1u); }
    __device__ void piece_counts() const {}
    __device__ void piece_totals() const {}
    __device__ void flush(unsigned long long* __restrict__ out) const {           // (barrier (B) of the last piece is behind every add)
        for (int c = threadIdx.x; c < 2 * cells; c += CF_RUN_THREADS) {
            const unsigned v = tab[c];
            if (v != 0u) {
                atomicAdd(&out[c], (unsigned long long)v);
                tab[c] = 0u;
            }
        }
        __syncthreads();                                                           // the next stretch adds to the table again
    }
};
