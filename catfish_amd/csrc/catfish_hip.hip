// catfish_hip.hip -- hand-written CDNA4 (gfx950) kernels + C ABI for the
// homopolymer-calling forward pass (see include/catfish_hip.h for the
// reference call this replaces: catfish/models/rnn_class.py:214-216).
//
// Design (DESIGN.md has the long version):
//   * The unit of work is a TILE of 16 windows (35 samples each).  Windows are
//     independent (zero GRU state, window-local SAME padding:
//     rnn_class.py:159,170-171; infer.py:43), so a wave owns a tile for a whole
//     layer and never synchronises with another wave.
//   * Every matmul is D[feature][window] = W^T * X on v_mfma_f32_16x16x4_f32
//     (exact fp32, k-ordered fma chain).  Weights are the A operand, read from
//     LDS in pre-packed fragment order; activations are the B operand.
//   * The D register layout (col = lane&15 = window, row = 4*(lane>>4)+reg =
//     feature) is ALSO a valid B-operand layout when the k index is permuted:
//     register r of M-tile m is k-step 4m+r carrying features {16m+4q+r}.
//     The weight packer applies the same permutation, so the recurrent state,
//     r*h and the conv intermediates feed the next MFMA straight from
//     registers: no LDS round trip, no cross-lane traffic on the serial chain.
//   * Inter-layer activations live in HBM in that same "fragment" order
//     [tile][t][mtile][lane][4], so every load/store is a coalesced 16 B/lane
//     (1 KiB per wave-instruction) access.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <vector>
#include <string>
#include <cmath>
#include <mutex>
#include <set>
#include <functional>

#include "../../include/catfish_hip.h"
#include "../../include/catfish_hip_ext.h"      // cf_clip_norm / cf_opt_step_guarded: declared there, defined below

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define CF_T 35          // window length (rnn_class.py:27)
#define CF_H 64          // GRU units per direction of the shipped model
#define CF_C 32          // conv channels of the shipped model
#define CF_TILE 16       // windows per tile = MFMA N

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// Timing-only ablations (tools/ablate.sh builds variants; results are WRONG when set):
//   bit 0: skip the sigmoid/tanh VALU phases   bit 1: no per-step global loads/stores
//   bit 2: 4 waves per workgroup (one per SIMD) instead of 8
#ifndef CF_ABLATE
#define CF_ABLATE 0
#endif
#ifndef CF_PREFETCH
#define CF_PREFETCH 1        // k-steps of A-fragment prefetch in the fp32 GRU step (1 or 2)
#endif

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float cf_sigmoid(float x) {
    // tf.nn.sigmoid; v_exp_f32 + v_rcp_f32 (1 ulp each), saturates correctly at +-inf
    return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float cf_tanh(float x) {
    // tanh(x) = 1 - 2 / (1 + exp(2x)); absolute error ~1e-7
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)), 1.0f);
}
// The GRU packers pre-scale the gate weights/biases by -log2(e) and the candidate's by 2*log2(e), so
// the MFMA accumulators already hold the exp2 arguments (saves one v_mul per gate element):
//   sigmoid(x) = 1 / (1 + 2^(-x log2 e)),   tanh(x) = 1 - 2 / (1 + 2^(2 x log2 e)).
#define CF_GATE_SCALE (-1.4426950408889634)
#define CF_CAND_SCALE (2.8853900817779268)
__device__ __forceinline__ float cf_sigmoid_pre(float a) {   // a = -x * log2(e)
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(a));
}
__device__ __forceinline__ float cf_tanh_pre(float a) {      // a = 2 * x * log2(e)
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(a)), 1.0f);
}
// two elements at a time: the "+ 1" and the tanh fma become packed-fp32 instructions (v_pk_add_f32 / v_pk_fma_f32)
__device__ __forceinline__ f32x2 cf_sigmoid_pre2(f32x2 a) {
    f32x2 e = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
    e = e + (f32x2){1.0f, 1.0f};
    return (f32x2){__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
}
__device__ __forceinline__ f32x2 cf_tanh_pre2(f32x2 a) {
    return __builtin_elementwise_fma((f32x2){-2.0f, -2.0f}, cf_sigmoid_pre2(a), (f32x2){1.0f, 1.0f});
}
// LDS arrays larger than a ds_read immediate offset reaches (64 KiB): three base pointers kept live in registers.
// The opaque offsets stop the compiler from folding them back into base + constant, which it would re-add in
// front of every far read.  Index with compile-time constants (unrolled loops) so the selection folds away.
template <typename T>
struct far_lds {
    static constexpr int N64K = 65536 / sizeof(T);
    const T *b0, *b1, *b2;
    __device__ __forceinline__ explicit far_lds(const T* base) {
        int o1 = N64K, o2 = 2 * N64K;
        asm volatile("" : "+v"(o1), "+v"(o2));
        b0 = base; b1 = base + o1; b2 = base + o2;
    }
    __device__ __forceinline__ const T& operator[](int e) const { return e < N64K ? b0[e] : (e < 2 * N64K ? b1[e - N64K] : b2[e - 2 * N64K]); }
};
__device__ __forceinline__ f32x4 cf_sigmoid_pre4(f32x4 a) {
    f32x4 e = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y), __builtin_amdgcn_exp2f(a.z), __builtin_amdgcn_exp2f(a.w)};
    e = e + (f32x4){1.0f, 1.0f, 1.0f, 1.0f};
    return (f32x4){__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y), __builtin_amdgcn_rcpf(e.z), __builtin_amdgcn_rcpf(e.w)};
}
__device__ __forceinline__ f32x4 cf_tanh_pre4(f32x4 a) {
    return __builtin_elementwise_fma((f32x4){-2.0f, -2.0f, -2.0f, -2.0f}, cf_sigmoid_pre4(a), (f32x4){1.0f, 1.0f, 1.0f, 1.0f});
}
// Output dropout of the training kernels (DropoutWrapper(output_keep_prob), rnn_class.py:151-154) without a stored mask: whether
// element e of a layer's output survives is a hash of (seed, layer, optimizer step, e), evaluated where the value is produced
// (forward: the dropped copy the next layer reads) and again where its gradient arrives (backward).  keep_prob >= 1: off.
struct cf_dropout {
    float keep_prob = 1.f;
    uint32_t seed = 0;
    int32_t layer = 0;
    const double* step = nullptr;      // device: optimizer steps taken so far (a new mask every step, also under graph replay)
};
__device__ __forceinline__ uint32_t cf_fmix32(uint32_t v) {      // murmur3 finalizer: full avalanche on 32 bits
    v ^= v >> 16; v *= 0x85ebca6bu; v ^= v >> 13; v *= 0xc2b2ae35u; v ^= v >> 16;
    return v;
}
__device__ __forceinline__ uint32_t cf_drop_key(const cf_dropout& d) {
    const uint32_t st = d.step ? (uint32_t)(long long)d.step[0] : 0u;
    return cf_fmix32(d.seed ^ cf_fmix32(0x9E3779B9u * (uint32_t)(d.layer + 1) + st * 0x85ebca6bu));
}
// mask / keep_prob of the four elements of f32x4 number idx4 of a layer output [tile][t][8][lane]
__device__ __forceinline__ f32x4 cf_drop_scale4(uint32_t key, float keep_prob, int64_t idx4) {
    const uint32_t thresh = (uint32_t)fminf(keep_prob * 4294967296.0f, 4294967040.0f);
    const float inv = 1.0f / keep_prob;
    const uint64_t e = (uint64_t)idx4 * 4u;
    const uint32_t base = (uint32_t)e ^ ((uint32_t)(e >> 32) * 0x9E3779B9u);
    f32x4 o;
    o.x = cf_fmix32((base + 0u) ^ key) < thresh ? inv : 0.f;
    o.y = cf_fmix32((base + 1u) ^ key) < thresh ? inv : 0.f;
    o.z = cf_fmix32((base + 2u) ^ key) < thresh ? inv : 0.f;
    o.w = cf_fmix32((base + 3u) ^ key) < thresh ? inv : 0.f;
    return o;
}

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    f32x4 o;
    o.x = fmaxf(v.x, 0.f); o.y = fmaxf(v.y, 0.f); o.z = fmaxf(v.z, 0.f); o.w = fmaxf(v.w, 0.f);
    return o;
}

// ------------------------------------------------------------------------------------------
// Packed-weight geometry shared by host packer and kernels
// ------------------------------------------------------------------------------------------
// GRU direction-layer blob (floats):
//   X  region: [ks < CIN/4][g < 3][lane][j < 4]   A fragments of output M-tile 4g+j, k-step ks (x rows)
//   HG region: [ks < 16][g < 2][lane][j]          gates (r,u) M-tiles 0..7, h rows
//   HC region: [ks < 16][lane][j]                 candidate M-tiles 8..11, h rows (multiply r*h)
//   BIAS     : [mo < 12][q < 4][r < 4]            bias of feature 16mo+4q+r   (gates | candidate)
//   DENSE    : [m < 4][q][r]                      final_fully_connected weight of this direction
// Output M-tiles: 0..3 = r gate, 4..7 = u gate, 8..11 = candidate.
__host__ __device__ constexpr int gru_x_floats(int cin) { return (cin / 4) * 3 * 256; }
__host__ __device__ constexpr int gru_hg_floats() { return 16 * 2 * 256; }
__host__ __device__ constexpr int gru_hc_floats() { return 16 * 256; }
__host__ __device__ constexpr int gru_bias_off(int cin) { return gru_x_floats(cin) + gru_hg_floats() + gru_hc_floats(); }
__host__ __device__ constexpr int gru_dense_off(int cin) { return gru_bias_off(cin) + 192; }
__host__ __device__ constexpr int gru_pack_floats(int cin) { return gru_dense_off(cin) + 64; }
#include "tuned_launch.hpp"      // every launch decision of the kernels below (host-only, tested on the CPU); includes gru_balance.hpp

// Residual-block blob (floats): NU 32x32 units of 1024 floats [ks < 8][lane][mo < 2], then
// bias vectors of 32 floats each in [mo][q][r] order.
//   first block (Cin = 1): units {c3 tap0, tap1, tap2, last}; vectors {b_c3, b_last, w_sc, b_sc, w_first, b_first}
//   other blocks          : units {sc, first, c3 tap0, tap1, tap2, last}; vectors {b_sc, b_first, b_c3, b_last}
__host__ __device__ constexpr int res_units(bool first) { return first ? 4 : 6; }
__host__ __device__ constexpr int res_vecs(bool first) { return first ? 6 : 4; }
__host__ __device__ constexpr int res_pack_floats(bool first) { return res_units(first) * 1024 + res_vecs(first) * 32; }

// feature carried by lane-quarter q in k-step ks (== register ks&3 of M-tile ks>>2 of a D tile)
__host__ __device__ constexpr int frag_feature(int ks, int q) { return 16 * (ks >> 2) + 4 * q + (ks & 3); }

// ------------------------------------------------------------------------------------------
// Kernel 1: residual block (resnet_class.py:44-82), BN folded into the convs.
// One wave = one tile of 16 windows, streamed over t with a one-step lookahead
// for the k=3 conv (zero padding at both window edges).  Small calls (latency mode) split a tile's 35
// positions into `t_chunks` chunks, one wave each: a chunk starts one position early to rebuild the k=3
// conv's left neighbour, otherwise the stream is the same.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void unit_mma(const float* __restrict__ unit, int lane, const f32x4 (&in)[2], f32x4 (&acc)[2]) {
    const f32x2* u2 = reinterpret_cast<const f32x2*>(unit) + lane;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const f32x2 a = u2[ks * 64];
        const float b = in[ks >> 2][ks & 3];
        acc[0] = MFMA16(a.x, b, acc[0]);
        acc[1] = MFMA16(a.y, b, acc[1]);
    }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void res_block_kernel(const float* __restrict__ wpack,
                                                        const float* __restrict__ x_nat,   // FIRST: [n_windows, 35]
                                                        const f32x4* __restrict__ x_frag,  // !FIRST: [tile][t][2][lane]
                                                        f32x4* __restrict__ y_frag,        // [tile][t][2][lane]
                                                        int64_t n_windows, int n_tiles, int t_chunks) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PACK = res_pack_floats(FIRST);
    constexpr int VEC0 = res_units(FIRST) * 1024;
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(wpack);
        f32x4* dst = reinterpret_cast<f32x4*>(lds);
        for (int i = threadIdx.x; i < PACK / 4; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane >> 4;
    const int waves_per_block = blockDim.x >> 6;
    float* xs = lds + PACK + wave * (CF_TILE * CF_T);  // FIRST only: this wave's x tile [16][35]

    auto vec = [&](int v, int mo) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(lds + VEC0 + v * 32 + mo * 16 + q * 4);
    };

    const int chunk_len = (CF_T + t_chunks - 1) / t_chunks;
    for (int task = blockIdx.x * waves_per_block + wave; task < n_tiles * t_chunks; task += gridDim.x * waves_per_block) {
        const int tile = task / t_chunks;
        const int p0 = (task - tile * t_chunks) * chunk_len;          // this wave writes positions [p0, p1)
        const int p1 = min(p0 + chunk_len, CF_T);
        f32x4 w_sc[2], b_sc[2], w_f[2], b_f[2];
        if constexpr (FIRST) {
            // stage the tile's raw samples: 16 windows x 35 = 560 contiguous floats
            const int64_t base = (int64_t)tile * CF_TILE * CF_T;
            const int64_t limit = n_windows * CF_T;
            for (int i = lane; i < CF_TILE * CF_T; i += 64) xs[i] = (base + i < limit) ? x_nat[base + i] : 0.f;
#pragma unroll
            for (int mo = 0; mo < 2; ++mo) { w_sc[mo] = vec(2, mo); b_sc[mo] = vec(3, mo); w_f[mo] = vec(4, mo); b_f[mo] = vec(5, mo); }
            // xs is private to this wave: a wave-level fence orders its ds_writes before the reads
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        f32x4 o1_pp[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        f32x4 o1_p[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        f32x4 sc_p[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        for (int i = p0 > 0 ? p0 - 1 : 0; i <= p1; ++i) {
            f32x4 o1_c[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            f32x4 sc_c[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            if (i < CF_T) {
                if constexpr (FIRST) {
                    // Cin = 1: conv1d is a rank-1 update (resnet_class.py:60,64)
                    const float xv = xs[(lane & 15) * CF_T + i];
#pragma unroll
                    for (int mo = 0; mo < 2; ++mo) {
                        sc_c[mo] = w_sc[mo] * xv + b_sc[mo];
                        o1_c[mo] = relu4(w_f[mo] * xv + b_f[mo]);
                    }
                } else {
                    f32x4 in[2];
                    const f32x4* src = x_frag + ((int64_t)tile * CF_T + i) * 2 * 64 + lane;
                    in[0] = src[0];
                    in[1] = src[64];
                    sc_c[0] = vec(0, 0); sc_c[1] = vec(0, 1);
                    unit_mma(lds + 0 * 1024, lane, in, sc_c);                 // shortcut, no relu (:60-61)
                    f32x4 acc[2] = {vec(1, 0), vec(1, 1)};
                    unit_mma(lds + 1 * 1024, lane, in, acc);                  // first conv (:64-66)
                    o1_c[0] = relu4(acc[0]); o1_c[1] = relu4(acc[1]);
                }
            }
            if (i >= p0 + 1) {
                constexpr int U3 = FIRST ? 0 : 2;      // first k=3 tap unit
                constexpr int VB3 = FIRST ? 0 : 2;     // bias vector of the k=3 conv
                f32x4 acc[2] = {vec(VB3, 0), vec(VB3, 1)};
                unit_mma(lds + (U3 + 0) * 1024, lane, o1_pp, acc);            // tap 0 * o1[t-1]
                unit_mma(lds + (U3 + 1) * 1024, lane, o1_p, acc);             // tap 1 * o1[t]
                unit_mma(lds + (U3 + 2) * 1024, lane, o1_c, acc);             // tap 2 * o1[t+1]
                f32x4 o2[2] = {relu4(acc[0]), relu4(acc[1])};                 // (:69-71)
                f32x4 acc3[2] = {vec(VB3 + 1, 0), vec(VB3 + 1, 1)};
                unit_mma(lds + (U3 + 3) * 1024, lane, o2, acc3);              // last conv (:74-76)
                f32x4* dst = y_frag + ((int64_t)tile * CF_T + (i - 1)) * 2 * 64 + lane;
                dst[0] = relu4(relu4(acc3[0]) + sc_p[0]);                     // add + relu (:79-80)
                dst[64] = relu4(relu4(acc3[1]) + sc_p[1]);
            }
#pragma unroll
            for (int mo = 0; mo < 2; ++mo) { o1_pp[mo] = o1_p[mo]; o1_p[mo] = o1_c[mo]; sc_p[mo] = sc_c[mo]; }
        }
        if constexpr (FIRST) __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------
// Kernel 1c: the first TWO residual blocks in one launch (throughput mode).  Block 1 runs one position behind
// block 0 in the same stream, so block 0's 32-channel output goes from its accumulators straight into block 1's
// first MFMAs (the accumulator layout is a B-operand layout, see the header) and never exists in HBM: 256 B per
// sample of traffic and one launch less.  Same operations in the same order as two res_block_kernel launches:
// bit-identical output.  Small calls (latency mode) split a tile's 35 positions into `t_chunks` chunks, one wave each, on
// as many CUs as the call leaves idle: a chunk starts two positions early (block 0's k=3 neighbourhood, then block 1's),
// so a single read's conv stack is ~7 positions deep instead of 2 x 35; there block 0's output is also stored (y0_frag)
// for the debug / test hook.
// ------------------------------------------------------------------------------------------
template <bool CHUNKED>
__global__ __launch_bounds__(256) void res_stack2_kernel(const float* __restrict__ wpack0, const float* __restrict__ wpack1,
                                                         const float* __restrict__ x_nat,   // [n_windows, 35]
                                                         f32x4* __restrict__ y_frag,        // [tile][t][2][lane], block 1's output
                                                         f32x4* __restrict__ y0_frag,       // block 0's output, or null
                                                         int64_t n_windows, int n_tiles, int t_chunks) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PACK0 = res_pack_floats(true), PACK1 = res_pack_floats(false);
    constexpr int VEC0 = res_units(true) * 1024, VEC1 = res_units(false) * 1024;
    {
        const f32x4* src0 = reinterpret_cast<const f32x4*>(wpack0);
        const f32x4* src1 = reinterpret_cast<const f32x4*>(wpack1);
        f32x4* dst = reinterpret_cast<f32x4*>(lds);
        for (int i = threadIdx.x; i < PACK0 / 4; i += blockDim.x) dst[i] = src0[i];
        for (int i = threadIdx.x; i < PACK1 / 4; i += blockDim.x) dst[PACK0 / 4 + i] = src1[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane >> 4;
    const int waves_per_block = blockDim.x >> 6;
    const float* w0 = lds;                 // block 0: units {c3 tap0, tap1, tap2, last}; vectors {b_c3, b_last, w_sc, b_sc, w_first, b_first}
    const float* w1 = lds + PACK0;         // block 1: units {sc, first, c3 tap0, tap1, tap2, last}; vectors {b_sc, b_first, b_c3, b_last}
    float* xs = lds + PACK0 + PACK1 + wave * (CF_TILE * CF_T);      // this wave's x tile [16][35]
    auto vec0 = [&](int v, int mo) -> f32x4 { return *reinterpret_cast<const f32x4*>(w0 + VEC0 + v * 32 + mo * 16 + q * 4); };
    auto vec1 = [&](int v, int mo) -> f32x4 { return *reinterpret_cast<const f32x4*>(w1 + VEC1 + v * 32 + mo * 16 + q * 4); };
    const f32x4 zero = {0, 0, 0, 0};

    if (!CHUNKED) t_chunks = 1;                                       // throughput mode: the chunk arithmetic folds away
    const int chunk_len = CHUNKED ? (CF_T + t_chunks - 1) / t_chunks : CF_T;
    for (int task = blockIdx.x * waves_per_block + wave; task < n_tiles * t_chunks; task += gridDim.x * waves_per_block) {
        const int tile = CHUNKED ? task / t_chunks : task;
        const int p0 = CHUNKED ? (task - tile * t_chunks) * chunk_len : 0;      // this wave writes positions [p0, p1)
        const int p1 = CHUNKED ? min(p0 + chunk_len, CF_T) : CF_T;
        if (CHUNKED && p0 >= p1) continue;
        {
            const int64_t base = (int64_t)tile * CF_TILE * CF_T;
            const int64_t limit = n_windows * CF_T;
            for (int i = lane; i < CF_TILE * CF_T; i += 64) xs[i] = (base + i < limit) ? x_nat[base + i] : 0.f;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        f32x4 w_sc[2], b_sc[2], w_f[2], b_f[2];
#pragma unroll
        for (int mo = 0; mo < 2; ++mo) { w_sc[mo] = vec0(2, mo); b_sc[mo] = vec0(3, mo); w_f[mo] = vec0(4, mo); b_f[mo] = vec0(5, mo); }
        f32x4 a_pp[2] = {zero, zero}, a_p[2] = {zero, zero}, a_sp[2] = {zero, zero};     // block 0: o1[t-1], o1[t], shortcut[t]
        f32x4 b_pp[2] = {zero, zero}, b_p[2] = {zero, zero}, b_sp[2] = {zero, zero};     // block 1, one position behind
        for (int i = p0 > 2 ? p0 - 2 : 0; i <= p1 + 1; ++i) {
            // ---- block 0, front at position i: Cin = 1, conv1d is a rank-1 update (resnet_class.py:60,64)
            f32x4 a_c[2] = {zero, zero}, a_sc[2] = {zero, zero};
            if (i < CF_T) {
                const float xv = xs[(lane & 15) * CF_T + i];
#pragma unroll
                for (int mo = 0; mo < 2; ++mo) {
                    a_sc[mo] = w_sc[mo] * xv + b_sc[mo];
                    a_c[mo] = relu4(w_f[mo] * xv + b_f[mo]);
                }
            }
            // ---- block 0, back: its output at position i - 1 stays in registers as block 1's input
            f32x4 y0[2] = {zero, zero};
            const bool have_y0 = i >= 1 && i <= CF_T && i >= p0;       // block 0's output at i - 1 >= p0 - 1
            if (have_y0) {
                f32x4 acc[2] = {vec0(0, 0), vec0(0, 1)};
                unit_mma(w0 + 0 * 1024, lane, a_pp, acc);                 // tap 0 * o1[t-1]
                unit_mma(w0 + 1 * 1024, lane, a_p, acc);                  // tap 1 * o1[t]
                unit_mma(w0 + 2 * 1024, lane, a_c, acc);                  // tap 2 * o1[t+1]
                f32x4 o2[2] = {relu4(acc[0]), relu4(acc[1])};             // (:69-71)
                f32x4 acc3[2] = {vec0(1, 0), vec0(1, 1)};
                unit_mma(w0 + 3 * 1024, lane, o2, acc3);                  // last conv (:74-76)
                y0[0] = relu4(relu4(acc3[0]) + a_sp[0]);                  // add + relu (:79-80)
                y0[1] = relu4(relu4(acc3[1]) + a_sp[1]);
                if (CHUNKED && y0_frag && i - 1 >= p0 && i - 1 < p1) {
                    f32x4* d0 = y0_frag + ((int64_t)tile * CF_T + (i - 1)) * 2 * 64 + lane;
                    d0[0] = y0[0];
                    d0[64] = y0[1];
                }
            }
            // ---- block 1, front at position p = i - 1 (zero padding past the window end, p = T)
            f32x4 b_c[2] = {zero, zero}, b_sc[2] = {zero, zero};
            if (have_y0) {
                b_sc[0] = vec1(0, 0); b_sc[1] = vec1(0, 1);
                unit_mma(w1 + 0 * 1024, lane, y0, b_sc);                  // shortcut, no relu (:60-61)
                f32x4 acc[2] = {vec1(1, 0), vec1(1, 1)};
                unit_mma(w1 + 1 * 1024, lane, y0, acc);                   // first conv (:64-66)
                b_c[0] = relu4(acc[0]); b_c[1] = relu4(acc[1]);
            }
            // ---- block 1, back: output position p - 1 = i - 2
            if (i >= 2 && i - 2 >= p0 && i - 2 < p1) {
                f32x4 acc[2] = {vec1(2, 0), vec1(2, 1)};
                unit_mma(w1 + 2 * 1024, lane, b_pp, acc);
                unit_mma(w1 + 3 * 1024, lane, b_p, acc);
                unit_mma(w1 + 4 * 1024, lane, b_c, acc);
                f32x4 o2[2] = {relu4(acc[0]), relu4(acc[1])};
                f32x4 acc3[2] = {vec1(3, 0), vec1(3, 1)};
                unit_mma(w1 + 5 * 1024, lane, o2, acc3);
                f32x4* dst = y_frag + ((int64_t)tile * CF_T + (i - 2)) * 2 * 64 + lane;
                dst[0] = relu4(relu4(acc3[0]) + b_sp[0]);
                dst[64] = relu4(relu4(acc3[1]) + b_sp[1]);
            }
#pragma unroll
            for (int mo = 0; mo < 2; ++mo) {
                a_pp[mo] = a_p[mo]; a_p[mo] = a_c[mo]; a_sp[mo] = a_sc[mo];
                if (i >= 1) { b_pp[mo] = b_p[mo]; b_p[mo] = b_c[mo]; b_sp[mo] = b_sc[mo]; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------
// Kernel 2: one bidirectional GRU layer (rnn_class.py:142-148,165-171), both
// directions in one grid (blockIdx.y).  A workgroup stages its direction's
// packed weights in LDS once; each wave then owns tiles of 16 windows and runs
// the 35-step recurrence with h, r*h and all pre-activations in registers.
// LAST = true fuses the dense(128->1) partial dot (rnn_class.py:179) instead
// of writing h.
// ------------------------------------------------------------------------------------------
template <int CIN>
__device__ __forceinline__ void gru_stage_weights(float* lds, const float* __restrict__ wpack, int dir) {
    constexpr int PACK = gru_pack_floats(CIN);
    const f32x4* src = reinterpret_cast<const f32x4*>(wpack + (size_t)dir * PACK);
    f32x4* dst = reinterpret_cast<f32x4*>(lds);
    for (int i = threadIdx.x; i < PACK / 4; i += blockDim.x) dst[i] = src[i];
}

// One tile (16 windows) of one direction of one layer: the whole 35-step recurrence.
// STASH (training forward): also write the activated gates r, u and the candidate c of every step to
// S[tile][t][dir][12][lane] (r = 0..3, u = 4..7, c = 8..11) for the backward pass.
// [s_begin, s_end) is the range of steps to run (gru_balance.hpp: a tile may be cut in time between two waves).  A piece that
// starts late takes h from the hand-off slot HO ([4][64] f32x4, register layout) instead of the zero state, one that ends early
// leaves h there; the steps themselves do not know.  Every other caller runs the whole tile and compiles to what it was.
// SKIP0 (gru_layer_kernel only; switched by the run-time flag skip0, so that the step body exists once): step 0 of a tile runs
// on the zero state, where the 128 gate MFMAs Wh_g h and the 64 candidate MFMAs Wh_c (r*h) add exact zeros and r is never used:
// a wave-uniform branch goes round them.  Same bits: fma(w, 0, acc) == acc for every finite w except that an acc of -0 would
// have become +0, and the sigmoid or tanh that follows maps both zeros to one value, so h and every output are unchanged.
// NOT covered: non-finite weights (w * 0 = NaN would have reached h).  The training forward (STASH) stores r and never skips.
// One k-step region: the A-fragment reads of the NEXT k-step go out before this k-step's MFMAs (left alone the
// scheduler sinks them behind most of the MFMAs, which leaves ~100 cycles between a read and its first use).
#ifndef CF_SCHED_DS_FIRST
#define CF_SCHED_DS_FIRST 1
#endif
#if CF_SCHED_DS_FIRST
#define CF_KSTEP_SCHED(nds, nmfma)                               \
    __builtin_amdgcn_sched_group_barrier(0x100, nds, 0);         \
    __builtin_amdgcn_sched_group_barrier(0x008, nmfma, 0);       \
    __builtin_amdgcn_sched_barrier(0)
#else
#define CF_KSTEP_SCHED(nds, nmfma) __builtin_amdgcn_sched_barrier(0)
#endif
template <int CIN, bool LAST, bool STASH = false, bool SKIP0 = false>
__device__ __forceinline__ void gru_tile(const float* lds, int lane, int dir, int tile, const f32x4* __restrict__ X,
                                         f32x4* __restrict__ Y, float* __restrict__ P, int n_tiles,
                                         f32x4* __restrict__ S = nullptr, f32x4* __restrict__ YD = nullptr, cf_dropout drop = cf_dropout(),
                                         int s_begin = 0, int s_end = CF_T, f32x4* HO = nullptr, bool skip0 = false) {
    const uint32_t drop_key = (STASH && YD) ? cf_drop_key(drop) : 0u;
    constexpr int KGX = CIN / 16;   // f32x4 registers of x per lane and step
    constexpr int KSX = CIN / 4;    // k-steps of the x part
    constexpr int XN4 = gru_x_floats(CIN) / 4;        // region sizes in f32x4 units
    constexpr int HG4 = gru_hg_floats() / 4;
    constexpr int BIAS = gru_bias_off(CIN);
    constexpr int DENSE = gru_dense_off(CIN);
    const int q = lane >> 4;
    const f32x4* WX = reinterpret_cast<const f32x4*>(lds) + lane;     // + (ks*3+g)*64
    const far_lds<f32x4> WL(WX);      // the packed weights span up to 144 KiB (far_lds: 32 v_add per step less, 168 -> 122 VGPRs)
    const f32x4* B4 = reinterpret_cast<const f32x4*>(lds + BIAS) + q;  // + mo*4
    const f32x4* D4 = reinterpret_cast<const f32x4*>(lds + DENSE) + q; // + m*4
    {
        f32x4 h[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // GRUCellZeroState
        if (s_begin > 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) h[m] = HO[m * 64 + lane];
        }
        f32x4 xc[KGX];
        {
            const int t0 = dir ? (CF_T - 1 - s_begin) : s_begin;
            const f32x4* src = X + ((int64_t)tile * CF_T + t0) * KGX * 64 + lane;
#pragma unroll
            for (int g = 0; g < KGX; ++g) xc[g] = src[g * 64];
        }
        for (int s = s_begin; s < s_end; ++s) {
            const int t = dir ? (CF_T - 1 - s) : s;    // bw = time-reversed sequence (ReverseV2)
            f32x4 acc[12];
#pragma unroll
            for (int mo = 0; mo < 12; ++mo) acc[mo] = B4[mo * 4];     // (bias held in registers as the first C operand: measured neutral)
            // The A fragments are software-pipelined one k-step ahead by hand; the
            // sched_barriers keep hipcc from hoisting hundreds of ds_reads (it spills otherwise).
            // k-steps of the whole step form one sequence p: x part [0, KSX), gate h part [KSX, KSX+16), candidate
            // h part [KSX+16, KSX+32); fragments are fetched PF k-steps ahead.
            constexpr int PF = CF_PREFETCH;
            auto loadA = [&](int p, f32x4 (&d)[3]) {
                if (p < KSX) { d[0] = WL[(p * 3 + 0) * 64]; d[1] = WL[(p * 3 + 1) * 64]; d[2] = WL[(p * 3 + 2) * 64]; }
                else if (p < KSX + 16) { d[0] = WL[XN4 + ((p - KSX) * 2 + 0) * 64]; d[1] = WL[XN4 + ((p - KSX) * 2 + 1) * 64]; }
                else if (p < KSX + 32) { d[0] = WL[XN4 + HG4 + (p - KSX - 16) * 64]; }
            };
            f32x4 ac[3], an[3], a2[3];
            loadA(0, ac);
            if (PF == 2) loadA(1, an);
            // x part: [r | u | c] += Wx^T x_t
#pragma unroll
            for (int ks = 0; ks < KSX; ++ks) {
                if (PF == 2) loadA(ks + 2, a2); else loadA(ks + 1, an);
                const float b = xc[ks >> 2][ks & 3];
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    acc[4 * g + 0] = MFMA16(ac[g].x, b, acc[4 * g + 0]);
                    acc[4 * g + 1] = MFMA16(ac[g].y, b, acc[4 * g + 1]);
                    acc[4 * g + 2] = MFMA16(ac[g].z, b, acc[4 * g + 2]);
                    acc[4 * g + 3] = MFMA16(ac[g].w, b, acc[4 * g + 3]);
                }
                CF_KSTEP_SCHED(3, 12);
#pragma unroll
                for (int g = 0; g < 3; ++g) { ac[g] = an[g]; if (PF == 2) an[g] = a2[g]; }
            }
            // x_t is dead: fetch the next step's x into the same registers (clamped on the last
            // step: a harmless re-read); the h part below hides the latency.
            {
                int tn = dir ? (t - 1) : (t + 1);
                tn = tn < 0 ? 0 : (tn > CF_T - 1 ? CF_T - 1 : tn);
                const f32x4* src = X + ((int64_t)tile * CF_T + tn) * KGX * 64 + lane;
#pragma unroll
                for (int g = 0; g < KGX; ++g) if (!(CF_ABLATE & 2)) xc[g] = src[g * 64];
            }
            // step 0 on the zero state (SKIP0 above): nothing below changes acc[4..11] or needs r.  The fragments already fetched
            // for the gate part are dropped; the next step starts its prefetch ring from k-step 0 like every step.
            // (the empty asm pins the accumulators where the x part left them: without it the register allocator renames them
            // ahead of the branch and the Cin = 32 LAST instance goes from 122 to 132 VGPRs, past four waves per SIMD)
            const bool run_h = !SKIP0 || !(skip0 && s == 0);
            if constexpr (SKIP0) {
#pragma unroll
                for (int mo = 0; mo < 12; ++mo) asm volatile("" : "+v"(acc[mo]));
            }
            if (run_h) {
            // h part of the gates: [r | u] += Wh_g^T h          (gru_cell/MatMul)
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (PF == 2) loadA(KSX + ks + 2, a2); else loadA(KSX + ks + 1, an);
                const float b = h[ks >> 2][ks & 3];
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    acc[4 * g + 0] = MFMA16(ac[g].x, b, acc[4 * g + 0]);
                    acc[4 * g + 1] = MFMA16(ac[g].y, b, acc[4 * g + 1]);
                    acc[4 * g + 2] = MFMA16(ac[g].z, b, acc[4 * g + 2]);
                    acc[4 * g + 3] = MFMA16(ac[g].w, b, acc[4 * g + 3]);
                }
                CF_KSTEP_SCHED(2, 8);
                ac[0] = an[0]; ac[1] = an[1];
                if (PF == 2) { an[0] = a2[0]; an[1] = a2[1]; }
            }
            // r = sigmoid(.), r*h feeds the candidate matmul (reset applied BEFORE the matmul:
            // gru_cell/mul -> concat_1 -> MatMul_1)
            f32x4 rh[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (CF_ABLATE & 1) { rh[m] = acc[m] * 0.001f; continue; }
                const f32x4 rv = cf_sigmoid_pre4(acc[m]);            // packed-fp32 "+ 1" and products, same rounding as scalar
                rh[m] = rv * h[m];
                if constexpr (STASH) acc[m] = rv;
            }
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                if (PF == 2) loadA(KSX + 16 + ks + 2, a2); else loadA(KSX + 16 + ks + 1, an);
                const float b = rh[ks >> 2][ks & 3];
                acc[8] = MFMA16(ac[0].x, b, acc[8]);
                acc[9] = MFMA16(ac[0].y, b, acc[9]);
                acc[10] = MFMA16(ac[0].z, b, acc[10]);
                acc[11] = MFMA16(ac[0].w, b, acc[11]);
                CF_KSTEP_SCHED(1, 4);
                ac[0] = an[0];
                if (PF == 2) an[0] = a2[0];
            }
            }
            // h' = u*h + (1-u)*c                                  (gru_cell/mul_1, sub, mul_2, add)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (CF_ABLATE & 1) { h[m] = acc[4 + m] * 0.001f + acc[8 + m] * 0.001f; continue; }
                const f32x4 u = cf_sigmoid_pre4(acc[4 + m]);
                const f32x4 c = cf_tanh_pre4(acc[8 + m]);
                h[m] = __builtin_elementwise_fma(u, h[m] - c, c);
                if constexpr (STASH) { acc[4 + m] = u; acc[8 + m] = c; }
            }
            if constexpr (STASH) {
                f32x4* sdst = S + (((int64_t)tile * CF_T + t) * 2 + dir) * 12 * 64 + lane;
#pragma unroll
                for (int j = 0; j < 12; ++j) sdst[j * 64] = acc[j];
            }
            if constexpr (!LAST) {
                f32x4* dst = Y + (((int64_t)tile * CF_T + t) * 8 + dir * 4) * 64 + lane;
#pragma unroll
                for (int m = 0; m < 4; ++m) if (!(CF_ABLATE & 2) || s == CF_T - 1) dst[m * 64] = h[m];
                if constexpr (STASH) {
                    if (YD) {       // training with dropout: the copy the next layer (or the dense head) reads
                        const int64_t i0 = (((int64_t)tile * CF_T + t) * 8 + dir * 4) * 64 + lane;
#pragma unroll
                        for (int m = 0; m < 4; ++m) YD[i0 + m * 64] = h[m] * cf_drop_scale4(drop_key, drop.keep_prob, i0 + m * 64);
                    }
                }
            } else {
                // partial logit of this direction: sum_f w[f] * h[f]   (final_fully_connected/MatMul)
                // summation order shared with the cooperative kernel (bit-identical results): one fma chain per
                // M-tile, the four M-tile sums added in order, then the lane quarters
                float pm[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const f32x4 wd = D4[m * 4];
                    pm[m] = wd.x * h[m].x;
                    pm[m] = fmaf(wd.y, h[m].y, pm[m]); pm[m] = fmaf(wd.z, h[m].z, pm[m]); pm[m] = fmaf(wd.w, h[m].w, pm[m]);
                }
                float p = ((pm[0] + pm[1]) + pm[2]) + pm[3];
                p += __shfl_xor(p, 16);
                p += __shfl_xor(p, 32);
                if (lane < 16) P[(((int64_t)dir * n_tiles + tile) * CF_T + t) * 16 + lane] = p;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (s_end < CF_T) {
#pragma unroll
            for (int m = 0; m < 4; ++m) HO[m * 64 + lane] = h[m];
        }
    }
}

// Hand-off of h between two waves of ONE workgroup (gru_balance.hpp): the flag is an LDS word, the data goes through global
// memory.  Order as in cdna_hip_programming.md Guideline 16: drain the stores, release, drain again (ROCm 7.2 can drop the
// fence's own wait), then the flag; the consumer polls relaxed from one lane, then acquires once.  Workgroup scope reaches every
// wave of a workgroup: they share the CU's vector cache.  The wait is bounded like cf_wait_flag.
__device__ __forceinline__ void cf_handoff_publish(unsigned* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void cf_handoff_wait(unsigned* flag, int lane, unsigned* err) {
    if (lane == 0) {
        bool ok = false;
        for (int it = 0; it < 1000000 && !ok; ++it) {
            ok = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u;
            if (!ok) __builtin_amdgcn_s_sleep(16);
        }
        if (!ok && err) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// The same hand-off across a workgroup boundary (grid-wide schedule, gru_balance.hpp): producer and consumer sit on different CUs
// and maybe different XCDs, so the flag is a word in global memory and both sides work at agent scope, as gru_fused_worker does.
// Each flag has ONE consumer, which reads it once, as the last thing its wave does before its last piece, and stores 0 back after
// the acquire: the buffer is zeroed at allocation and by cf_clear_error and needs neither a memset nor an epoch per launch (a
// captured graph would replay a stale epoch).  A timeout sets the sticky error word and the wave carries on, so the grid drains;
// the flag it may leave set is what cf_clear_error zeroes.
__device__ __forceinline__ void cf_handoff_publish_agent(unsigned* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cf_handoff_wait_agent(unsigned* flag, int lane, unsigned* err) {
    if (lane == 0) {
        bool ok = false;
        for (int it = 0; it < 1000000 && !ok; ++it) {
            ok = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            if (!ok) __builtin_amdgcn_s_sleep(16);
        }
        if (!ok && err) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


template <int CIN, bool LAST>
__global__ __launch_bounds__(512, 2) void gru_layer_kernel(const float* __restrict__ wpack,  // [2][gru_pack_floats(CIN)]
                                                           const f32x4* __restrict__ X,      // [tile][t][CIN/16][lane]
                                                           f32x4* __restrict__ Y,            // [tile][t][8][lane]
                                                           float* __restrict__ P,            // [2][tile][t][16]
                                                           int n_tiles,
                                                           int balance_arg,                  // schedule, chosen by launch_gru
                                                           f32x4* hand,                      // [2][gridDim.x][8][4][64] hand-off slots
                                                           unsigned* gflags,                 // [2][gridDim.x] boundary flags (grid-wide)
                                                           unsigned* err) {                  // sticky: a hand-off wait timed out
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int dir = blockIdx.y;
    gru_stage_weights<CIN>(lds, wpack, dir);
    unsigned* flags = reinterpret_cast<unsigned*>(lds + gru_pack_floats(CIN));     // one word per wave behind the weights
    if (threadIdx.x < CF_GRU_MAX_WAVES) flags[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    // Every workgroup takes an equal contiguous share of the tiles (+-1).  Round-robin deals whole tiles to the waves; the
    // balanced schedule deals equal shares of tiles x 35 steps (gru_balance.hpp).  Either way a wave runs a list of pieces
    // (tile, [s_begin, s_end)) through ONE call site: the step body is 576 MFMAs unrolled.  balance == 2 is the grid-wide
    // schedule: the same shares with the direction's tiles as the "workgroup" and the global wave index as the "wave".
    const int balance = balance_arg & CF_GRU_SCHED_MASK;
    const bool skip0 = !(balance_arg & CF_GRU_RUN_ZERO_PRODUCTS);
    int t0 = (int)((int64_t)blockIdx.x * n_tiles / gridDim.x);
    const int t1 = (int)((int64_t)(blockIdx.x + 1) * n_tiles / gridDim.x);
    cf_gru_share sh;
    int n_pieces;
    if (balance == 2) {
        sh = cf_gru_balanced_share(n_tiles, (int)gridDim.x * nwaves, (int)blockIdx.x * nwaves + wave, CF_T);
        n_pieces = (sh.head_end > 0) + sh.whole_count + (sh.tail_begin < CF_T);
        t0 = 0;
    } else if (balance) {
        sh = cf_gru_balanced_share(t1 - t0, nwaves, wave, CF_T);
        n_pieces = (sh.head_end > 0) + sh.whole_count + (sh.tail_begin < CF_T);
    } else {
        sh.head_tile = sh.head_end = 0; sh.whole_first = sh.whole_count = 0; sh.tail_tile = 0; sh.tail_begin = CF_T;
        n_pieces = t1 - t0 > wave ? (t1 - t0 - wave + nwaves - 1) / nwaves : 0;
    }
    // slot w of workgroup b holds the h that wave w of b hands on; the wave before wave 0 is the last wave of workgroup b - 1
    f32x4* slots = hand + ((size_t)(dir * gridDim.x + blockIdx.x) * CF_GRU_MAX_WAVES) * 4 * 64;
    unsigned* gflag = gflags + dir * gridDim.x + blockIdx.x;                       // set by this workgroup's last wave
    const int has_head = balance && sh.head_end > 0;
    for (int i = 0; i < n_pieces; ++i) {
        int tile, s_begin = 0, s_end = CF_T;
        f32x4* ho = nullptr;
        if (!balance) {
            tile = t0 + wave + i * nwaves;
        } else if (i < has_head) {                          // the head first: the next wave's tail waits for it
            tile = t0 + sh.head_tile; s_end = sh.head_end; ho = slots + wave * 4 * 64;
        } else if (i < has_head + sh.whole_count) {
            tile = t0 + sh.whole_first + (i - has_head);
        } else {                                            // the tail last: the previous wave's head is long over
            tile = t0 + sh.tail_tile; s_begin = sh.tail_begin;
            if (wave > 0) {
                ho = slots + (wave - 1) * 4 * 64;
                cf_handoff_wait(flags + (wave - 1), lane, err);
            } else {                                        // grid-wide only: wave 0 of a workgroup has no tail otherwise
                ho = slots - (CF_GRU_MAX_WAVES - (nwaves - 1)) * 4 * 64;
                cf_handoff_wait_agent(gflag - 1, lane, err);
            }
        }
        gru_tile<CIN, LAST, false, true>(lds, lane, dir, tile, X, Y, P, n_tiles, nullptr, nullptr, cf_dropout(), s_begin, s_end, ho, skip0);
        if (s_end < CF_T) {                                 // (a workgroup's last wave has a head only in the grid-wide schedule)
            if (wave < nwaves - 1) cf_handoff_publish(flags + wave);
            else cf_handoff_publish_agent(gflag);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Kernel 2b: all biGRU layers in ONE launch.  A separate launch per layer leaves CUs idle in every
// layer's last round (1888 tiles per direction on 1024 SIMDs = 3.69 rounds: dealt as whole tiles, 7.8 % lost per launch; the
// per-layer kernel's balanced schedule, gru_balance.hpp, brings its own loss down to 2.2 %).
// Here workgroups are ordered layer-major (a pool per layer and direction that pulls 8-tile groups from a
// queue), so the first groups of layer l+1 start on the CUs that layer l's tail frees.  A group of layer
// l > 0 waits for both directions of the same group of layer l-1 through agent-scope flags
// (release/acquire exactly as cdna_hip_programming.md Guideline 16).  Every wait is bounded: on a
// timeout the workgroup records an error code and carries on, so the grid always drains.
// Progress argument: workgroups are dispatched in index order per XCD, so when a waiting workgroup holds
// a CU every workgroup of the previous layer has already been dispatched and none of those ever waits on
// a later one.
// ------------------------------------------------------------------------------------------
struct cf_fused_args {
    const float* w[3];       // packed weights of layer 0..2, [2 dirs]
    const f32x4* x0;         // layer-0 input (conv output / embedding), fragment layout
    f32x4* y[2];             // layer outputs (layer l writes y[l & 1])
    float* p;                // dense partials
    unsigned* flags;         // [n_layers][groups][2] completion flags, then [n_layers][2] queue heads; zeroed before the launch
    int lds_floats;          // floats of dynamic LDS holding weights (one broadcast word follows)
    unsigned* err;           // [1], zeroed before the launch; != 0 after a wait timed out
    int n_tiles;
    int groups;              // ceil(n_tiles / 8)
    int n_layers;            // 1..3
    int cin0;                // 32 (ResNetRNN) or 16 (plain RNN)
};

__device__ __forceinline__ bool cf_wait_flag(unsigned* flag) {
    for (int it = 0; it < 1000000; ++it) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return true;
        __builtin_amdgcn_s_sleep(16);
    }
    return false;
}

// A workgroup serves ONE (layer, direction): it stages those weights once, then pulls 8-tile groups from
// that (layer, direction)'s queue until it is empty.
template <int CIN, bool LAST>
__device__ __forceinline__ void gru_fused_worker(float* lds, const cf_fused_args& a, int layer, int dir) {
    const f32x4* X = layer == 0 ? a.x0 : a.y[(layer - 1) & 1];
    f32x4* Y = a.y[layer & 1];
    gru_stage_weights<CIN>(lds, a.w[layer], dir);
    volatile int* slot = reinterpret_cast<volatile int*>(lds + a.lds_floats);   // broadcast word behind the weights
    unsigned* queue = a.flags + (size_t)a.n_layers * a.groups * 2 + layer * 2 + dir;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // A pool member serves at most `groups` groups before it sees the queue empty: the loop is bounded by
    // construction (a plain `for (;;)` with a break in the middle hung on gfx950 / ROCm 7.2).
    int group = 0;
    for (int iter = 0; iter <= a.groups && group < a.groups; ++iter) {
        if (threadIdx.x == 0) {
            const int g = (int)__hip_atomic_fetch_add(queue, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (layer > 0 && g < a.groups) {
                // consumer side: ONE lane polls relaxed, then ONE agent-scope acquire
                unsigned* f = a.flags + ((size_t)(layer - 1) * a.groups + g) * 2;
                if (!cf_wait_flag(f) || !cf_wait_flag(f + 1)) __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            *slot = g;
        }
        __syncthreads();
        group = *slot;                                   // the same value in every thread
        if (group < a.groups) {
            const int tile = group * 8 + wave;
            if (tile < a.n_tiles) gru_tile<CIN, LAST>(lds, lane, dir, tile, X, Y, a.p, a.n_tiles);
            // producer side: every storing wave drains, barrier, ONE lane releases at agent scope, then the flag
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (!LAST && threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(a.flags + ((size_t)layer * a.groups + group) * 2 + dir, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__global__ __launch_bounds__(512, 2) void gru_fused_kernel(cf_fused_args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int per_layer = gridDim.x / a.n_layers;          // workgroups per layer, directions interleaved
    const int layer = blockIdx.x / per_layer;
    const int dir = (blockIdx.x - layer * per_layer) & 1;
    const bool last = layer == a.n_layers - 1;
    if (layer == 0) {
        if (a.cin0 == 16) { if (last) gru_fused_worker<16, true>(lds, a, layer, dir); else gru_fused_worker<16, false>(lds, a, layer, dir); }
        else { if (last) gru_fused_worker<32, true>(lds, a, layer, dir); else gru_fused_worker<32, false>(lds, a, layer, dir); }
    } else {
        if (last) gru_fused_worker<128, true>(lds, a, layer, dir); else gru_fused_worker<128, false>(lds, a, layer, dir);
    }
}

#include "gru_coop.hpp"
#include "gru_train.hpp"
static_assert(gtb_pack_floats(32) == ((32 + CF_H) / 16 / 2) * 128 * 48 && gtb_pack_floats(128) == ((128 + CF_H) / 16 / 2) * 128 * 48,
              "gru_train_bwd_coop_kernel's PACK must equal gtb_pack_floats");
#include "gru_wgrad.hpp"
#include "res_train.hpp"
#include "train_step.hpp"

// ------------------------------------------------------------------------------------------
// Kernel 1b: plain RNN type (no residual blocks, rnn_class.py:165-175 applied to the raw signal).
// The GRU kernels want >= 4 input features per k-step, so the single input feature is embedded
// in a 16-feature fragment tile (feature 0 = x, the rest 0; the packed weight rows are 0 too).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ x_nat, f32x4* __restrict__ y_frag,
                                                    int64_t n_windows, int n_tiles) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (tile, t, lane)
    if (idx >= (int64_t)n_tiles * CF_T * 64) return;
    const int lane = (int)(idx & 63);
    const int64_t tt = idx >> 6;
    const int t = (int)(tt % CF_T);
    const int64_t w = (tt / CF_T) * CF_TILE + (lane & 15);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((lane >> 4) == 0 && w < n_windows) v.x = x_nat[w * CF_T + t];
    y_frag[idx] = v;
}

#include "gru_bf16.hpp"
#include "gru_bf16_pipe.hpp"
#include "gru_bf16x3_pipe.hpp"

// ------------------------------------------------------------------------------------------
// Kernel 3: head -- logits = p_fw + p_bw + b, probs = sigmoid (rnn_class.py:84,179-181),
// transposing the [tile][t][16] partials back to the reference's window-major order.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ P, const float* __restrict__ dense_bias, float* __restrict__ probs,
                                                   float* __restrict__ logits, int64_t n_windows, int n_tiles, int tile_shift, int raw) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_windows * CF_T) return;
    const float bias = dense_bias[0];
    const int64_t w = idx / CF_T;
    const int t = (int)(idx - w * CF_T);
    const int64_t tile = w >> tile_shift;            // 16-window tiles (fp32 path) or 32-window tiles (bf16 path)
    const int tw = 1 << tile_shift;
    const int wl = (int)(w & (tw - 1));
    float z;
    if (raw) {
        // latency-mode kernels leave per-lane partials [dir][tile][t][4 M-tiles][64 lanes]: M-tile sums added in order, then
        // the lane quarters as the one-wave kernel's two xor-shuffles do: (q0 + q1) + (q2 + q3)
        float pd[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const float* src = P + ((((int64_t)d * n_tiles + tile) * CF_T + t) * 4) * 64 + wl;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = ((src[q * 16] + src[64 + q * 16]) + src[128 + q * 16]) + src[192 + q * 16];
            pd[d] = (v[0] + v[1]) + (v[2] + v[3]);
        }
        z = pd[0] + pd[1] + bias;
    } else {
        z = P[((tile)*CF_T + t) * tw + wl] + P[(((int64_t)n_tiles + tile) * CF_T + t) * tw + wl] + bias;
    }
    if (logits) logits[idx] = z;
    if (probs) probs[idx] = 1.0f / (1.0f + expf(-z));
}

// ------------------------------------------------------------------------------------------
// Kernel 4: class_from_threshold + correct_short (infer.py:128-138,174-198) per read.
// Reads are packed back to back WITH their zero padding: read r owns samples
// [read_offsets[r], read_offsets[r+1]) of which the first read_lengths[r] are real
// (infer.py:47 trims the padding before thresholding).  A positive sample survives iff its
// positive run inside the real part of its own read has length >= min_run.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ probs,
                                                          const int64_t* __restrict__ read_offsets,
                                                          const int64_t* __restrict__ read_lengths, int64_t n_reads,
                                                          int64_t total, float threshold, int min_run,
                                                          uint8_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    uint8_t out = 0;
    if (probs[i] >= threshold) {
        // read containing i: largest r with read_offsets[r] <= i
        int64_t lo = 0, hi = n_reads;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (read_offsets[mid] <= i) lo = mid; else hi = mid;
        }
        const int64_t beg = read_offsets[lo], end = beg + read_lengths[lo];
        if (i < end) {
            int run = 1;
            for (int64_t j = i - 1; j >= beg && run < min_run && probs[j] >= threshold; --j) ++run;
            for (int64_t j = i + 1; j < end && run < min_run && probs[j] >= threshold; ++j) ++run;
            out = run >= min_run ? 1 : 0;
        }
    }
    labels[i] = out;
}

// ------------------------------------------------------------------------------------------
// Kernel 4b: run boundaries of the corrected labels (first half of hp_in_pred, infer.py:141-162).
// Every sample that opens (closes) a positive run appends its packed position to `starts`
// (`ends`, exclusive) through an atomic counter.  Padding labels are 0, so runs never cross reads;
// after sorting both lists ascending on the host the k-th start pairs with the k-th end.
// ------------------------------------------------------------------------------------------
#define CF_SPANS_PER_THREAD 16
__global__ __launch_bounds__(256) void spans_kernel(const uint8_t* __restrict__ labels, int64_t total, int64_t max_runs,
                                                    int64_t* __restrict__ starts, int64_t* __restrict__ ends,
                                                    unsigned long long* __restrict__ counts) {
    // A workgroup scans 256 * CF_SPANS_PER_THREAD samples, reserves room for all its boundaries with ONE global atomic per
    // list (slots inside the reservation come from LDS counters), then writes them.
    __shared__ unsigned n_loc[2];
    __shared__ unsigned long long base[2];
    if (threadIdx.x < 2) n_loc[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * 256 * CF_SPANS_PER_THREAD + threadIdx.x;
    unsigned ms = 0, me = 0;                               // bit j: sample i0 + 256 j starts / ends a run
#pragma unroll
    for (int j = 0; j < CF_SPANS_PER_THREAD; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (i < total && labels[i]) {
            if (i == 0 || !labels[i - 1]) ms |= 1u << j;
            if (i == total - 1 || !labels[i + 1]) me |= 1u << j;
        }
    }
    unsigned os = 0, oe = 0;
    if (ms) os = atomicAdd(&n_loc[0], (unsigned)__popc(ms));
    if (me) oe = atomicAdd(&n_loc[1], (unsigned)__popc(me));
    __syncthreads();
    if (threadIdx.x < 2 && n_loc[threadIdx.x]) base[threadIdx.x] = atomicAdd(&counts[threadIdx.x], (unsigned long long)n_loc[threadIdx.x]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CF_SPANS_PER_THREAD; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (ms & (1u << j)) {
            const unsigned long long k = base[0] + os++;
            if ((int64_t)k < max_runs) starts[k] = i;
        }
        if (me & (1u << j)) {
            const unsigned long long k = base[1] + oe++;
            if ((int64_t)k < max_runs) ends[k] = i + 1;
        }
    }
}

// Kernel 4c: a read packed without padding (read_lengths[r] == read_offsets[r + 1] - read_offsets[r]) touches the next one, and
// spans_kernel, which sees labels only, reports a positive run across the boundary as one.  One thread per read boundary splits it.
__global__ __launch_bounds__(256) void spans_cut_kernel(const uint8_t* __restrict__ labels, const int64_t* __restrict__ read_offsets,
                                                        const int64_t* __restrict__ read_lengths, int64_t n_reads, int64_t total, int64_t max_runs,
                                                        int64_t* __restrict__ starts, int64_t* __restrict__ ends,
                                                        unsigned long long* __restrict__ counts) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;         // boundary between read r - 1 and read r
    if (r >= n_reads) return;
    const int64_t at = read_offsets[r];
    if (at <= 0 || at >= total || read_offsets[r - 1] + read_lengths[r - 1] != at || read_lengths[r] <= 0) return;
    if (!labels[at - 1] || !labels[at]) return;
    const unsigned long long ks = atomicAdd(&counts[0], 1ull), ke = atomicAdd(&counts[1], 1ull);
    if ((int64_t)ks < max_runs) starts[ks] = at;
    if ((int64_t)ke < max_runs) ends[ke] = at;
}

// ------------------------------------------------------------------------------------------
// Kernel 5: signal ingest -- per-read median / MAD normalisation of raw int16 DAC samples
// (normalize_raw_signal, infer.py:96-105) fused with the zero padding + window packing of
// infer.py:31-43.  One workgroup per read.  Medians are found exactly by radix selection over
// LDS histograms (int16 keys: 8 + 8 bits; doubled absolute deviations, 17 bits: 9 + 8 bits); for
// even lengths the two middle order statistics are averaged like numpy.median.  The division is
// done in double and rounded once to fp32, i.e. bit-identical to numpy's float64 result cast to
// float32 (what TF's feed does, rnn_class.py:214).
// ------------------------------------------------------------------------------------------
template <typename KeyFn>
__device__ int radix_select(const int16_t* __restrict__ v, int64_t n, int64_t rank, int hi_bits, KeyFn key, unsigned* hist,
                            unsigned* sh) {
    // level 1: histogram of the high bits
    const int nb1 = 1 << hi_bits;
    for (int i = threadIdx.x; i < nb1; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[key(v[i]) >> 8], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        int b = 0;
        for (; b < nb1; ++b) {
            if (acc + hist[b] > rank) break;
            acc += hist[b];
        }
        sh[0] = (unsigned)b;
        sh[1] = (unsigned)(rank - acc);     // rank inside the bin
    }
    __syncthreads();
    const unsigned bin = sh[0];
    const unsigned r2 = sh[1];
    __syncthreads();
    // level 2: histogram of the low 8 bits inside that bin
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned k = key(v[i]);
        if ((k >> 8) == bin) atomicAdd(&hist[k & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned acc = 0;
        int b = 0;
        for (; b < 256; ++b) {
            if (acc + hist[b] > r2) break;
            acc += hist[b];
        }
        sh[2] = (bin << 8) | (unsigned)b;
    }
    __syncthreads();
    const int out = (int)sh[2];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(256) void normalize_kernel(const int16_t* __restrict__ dac, const int64_t* __restrict__ dac_offsets,
                                                        const int64_t* __restrict__ win_offsets, float* __restrict__ x_out) {
    __shared__ unsigned hist[512];
    __shared__ unsigned sh[4];
    const int64_t r = blockIdx.x;
    const int16_t* v = dac + dac_offsets[r];
    const int64_t n = dac_offsets[r + 1] - dac_offsets[r];
    float* out = x_out + win_offsets[r] * CF_T;
    const int64_t n_pad = (win_offsets[r + 1] - win_offsets[r]) * CF_T;
    if (n <= 0) {
        for (int64_t i = threadIdx.x; i < n_pad; i += blockDim.x) out[i] = 0.f;
        return;
    }
    auto key16 = [](int16_t x) -> unsigned { return (unsigned)((int)x + 32768); };
    const int lo = radix_select(v, n, (n - 1) / 2, 8, key16, hist, sh);
    const int hi = (n & 1) ? lo : radix_select(v, n, n / 2, 8, key16, hist, sh);
    const int med2 = (lo - 32768) + (hi - 32768);            // 2 * median, exact
    auto keydev = [med2](int16_t x) -> unsigned { const int d = 2 * (int)x - med2; return (unsigned)(d < 0 ? -d : d); };
    const int dlo = radix_select(v, n, (n - 1) / 2, 9, keydev, hist, sh);
    const int dhi = (n & 1) ? dlo : radix_select(v, n, n / 2, 9, keydev, hist, sh);
    const double shift = 0.5 * (double)med2;
    const double scale = 0.25 * (double)(dlo + dhi);          // median(|raw - shift|)
    for (int64_t i = threadIdx.x; i < n_pad; i += blockDim.x)
        out[i] = i < n ? (float)(((double)v[i] - shift) / scale) : 0.f;
}

#include "ingest_post.hpp"      // round 5: normalize_regs_kernel, postprocess_bits_kernel (same results, see there)
#include "span_scores.hpp"      // span_scores_kernel: per-call scores of the runs postprocess_bits_kernel<true> reports

// ==========================================================================================
// Host side
// ==========================================================================================
#include "anysize_infer_launch.hpp"      // kernel, waves, grid and LDS bytes of the any-size inference recurrences: host-only, tested on the CPU
#include "generic.hpp"

// A/B and test knobs: environment variables (CATFISH_GENERIC, CATFISH_WAVES, CATFISH_BF16_PIPE, ... -- tools/README.md lists
// them) that change WHICH kernels a call uses.  They are for tools/ and tests and are honoured only while
// CATFISH_DEBUG_KNOBS=1 is set as well; every knob that takes effect is named once on stderr, so a stray variable can
// neither change results nor do so silently.
static bool cf_knobs_on() {
    const char* on = getenv("CATFISH_DEBUG_KNOBS");
    return on && atoi(on) != 0;
}
static const char* cf_knob(const char* name) {
    if (!cf_knobs_on()) return nullptr;
    const char* v = getenv(name);
    if (v) {
        static std::mutex mu;
        static std::set<std::string> seen;
        std::lock_guard<std::mutex> lock(mu);
        if (seen.insert(std::string(name) + "=" + v).second) fprintf(stderr, "catfish_hip: debug knob %s=%s is active\n", name, v);
    }
    return v;
}
// The knobs of the tuned path's launch plans (tuned_launch.hpp), read ONCE per run_pass, per training entry and per cf_model_create:
// with the debug switch off that is one getenv.
static cf_knobs cf_read_knobs() {
    cf_knobs k;
    k.ablate_four_waves = (CF_ABLATE & 4) ? 1 : 0;
    if (!cf_knobs_on()) return k;
    auto num = [](const char* name) { const char* v = cf_knob(name); return v ? atoi(v) : CF_KNOB_UNSET; };
    k.coop = num("CATFISH_COOP");
    k.waves = num("CATFISH_WAVES");
    k.gru_balance = num("CATFISH_GRU_BALANCE");
    k.gru_gx = num("CATFISH_GRU_GX");
    k.gru_zero_products = num("CATFISH_GRU_ZERO_PRODUCTS");
    k.xproj_lds = num("CATFISH_XPROJ_LDS");
    k.xproj_chunks = num("CATFISH_XPROJ_CHUNKS");
    k.hoist_tiles = num("CATFISH_HOIST_TILES");
    k.fuse = num("CATFISH_FUSE");
    k.bf16_waves = num("CATFISH_BF16_WAVES");
    k.bf16_wgs = num("CATFISH_BF16_WGS");
    k.bf16_pipe = num("CATFISH_BF16_PIPE");
    k.res_fuse = num("CATFISH_RES_FUSE");
    k.res_tpw = num("CATFISH_RES_TPW");
    k.res_chunks = num("CATFISH_RES_CHUNKS");
    k.dx_chunks = num("CATFISH_DX_CHUNKS");
    return k;
}

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(CF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

enum { SLOT_RES_FIRST = 0, SLOT_RES, SLOT_GRU0, SLOT_GRU, SLOT_GRU_LAST, SLOT_HEAD, SLOT_POST, SLOT_NORM, SLOT_GRU_FUSED, SLOT_RES_STACK2 };
static const char* k_slot_names[CF_PROF_SLOTS] = {"res_block_first", "res_block",      "gru_layer_first", "gru_layer_mid",
                                                  "gru_layer_last",  "head",           "postprocess",     "normalize",       "gru_fused",
                                                  "res_stack2",      "unused",         "unused"};

struct cf_param_map;
static void pm_destroy(cf_param_map* pm);

struct cf_model {
    cf_hparams hp;
    int device = 0;
    int n_cu = 256;
    std::vector<float*> d_res;   // per residual block packed weights
    std::vector<float*> d_gru;   // per layer packed weights [2 dirs]
    std::vector<int> gru_cin;
    std::vector<char*> d_res_b;  // per residual block packed bf16 weights (precision != fp32)
    std::vector<char*> d_gru_b;  // per layer packed bf16 weights [2 dirs] (precision != fp32)
    int np = 0;                  // bf16 parts per operand: 0 = fp32 path, 1 = bf16, 2 = bf16x3
    float* d_dense_bias = nullptr;   // [1]: read by both head kernels, so that cf_model_load_params can replace it on the device
    cf_param_map* pmap = nullptr;    // gather map of cf_model_load_params (params_dev.hpp), built by its first call
    // workspace
    int64_t cap_windows = 0;              // per workspace slot
    int64_t cap_tiles = 0;
    // A pass needs ~2.6 KB of scratch per sample; every slot owns one scratch set and one
    // internal stream, so consecutive sub-batches overlap (the tail of one layer's grid leaves
    // CUs idle that the other slot's kernels fill).
    struct Slot {
        float* d_a[2] = {nullptr, nullptr};   // conv ping-pong, F = 32
        float* d_y[2] = {nullptr, nullptr};   // GRU layer outputs ping-pong, F = 128
        float* d_p = nullptr;                 // dense partials [2][tiles][35][16]
        unsigned* d_flags = nullptr;          // fused launch: [n_layers][groups][2] completion flags
        float* d_hand = nullptr;              // balanced biGRU schedule: h hand-off slots [2 dirs][workgroups][8 waves][4][64] f32x4
        unsigned* d_hand_flags = nullptr;     // grid-wide schedule: boundary flags [2 dirs][workgroups]; zero between launches
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        int64_t last_windows = 0;             // windows of the last pass (debug hook)
        bool last_res_fused = false;          // the last pass ran blocks 0 and 1 as one launch: block 0's output was never stored
    };
    std::vector<Slot> slots;
    cf_generic* gen = nullptr;                // any-size path (generic.hpp): set when the geometry is not the shipped 64 / 32
    int fuse = 0;                             // all GRU layers in one launch (fp32 path, n_layers <= 3): 0 never, 1 always,
                                              // 2 auto = only for passes of >= 6 rounds, where the dynamic queues pay
    float* d_xp = nullptr;                    // hoisted x projection of small calls: [xp_tiles][35][2][12][64] f32x4
    int xp_tiles = 0;
    float* d_host_x = nullptr;                // cf_infer_host staging (grown on demand)
    float* d_host_p = nullptr;
    size_t host_stage_bytes = 0;
    unsigned* h_err = nullptr;                // host-mapped: set by a fused launch whose bounded wait timed out (sticky)
    unsigned* d_err = nullptr;                // device view of h_err
    hipEvent_t fork = nullptr;
    int64_t ws_bytes = 0;
    // profiling
    bool prof = false;                    // events around the kernels of THIS call (set per cf_infer from prof_every)
    int prof_every = 0;                   // 0 = off, N = time every N-th cf_infer call
    int64_t prof_calls = 0;
    struct Ev { hipEvent_t a, b; int slot; };
    std::vector<Ev> ev_pending;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[CF_PROF_SLOTS] = {0};
    int64_t prof_n[CF_PROF_SLOTS] = {0};
};

// ---- weight packing ----------------------------------------------------------------------
// Every packed fp32 element is a TERM over the checkpoint's inference tensors:
//   zero  |  raw parameter x c  |  BN-folded kernel element (parameter x s of its channel) x c  |  BN-folded bias (b s + beta - mean s) x c
// with s = gamma / sqrt(var + eps) and c from cf_term_const.  The packers below only EMIT terms (sink(index, term)):
// cf_model_create evaluates them on the host (cf_host_params), cf_model_load_params records them once as a gather map and
// evaluates them on the device (params_dev.hpp).  Both sides go through cf_bn_scale / cf_bn_bias / cf_term_value: double math
// in the same order, contraction off, rounded to fp32 at the end -- so a load gives the bits a create of the same values gives.
enum { CF_TERM_ZERO = 0, CF_TERM_RAW = 1, CF_TERM_KERN = 2, CF_TERM_BIAS = 3 };
enum { CF_K_ONE = 0, CF_K_GATE = 1, CF_K_CAND = 2 };
__host__ __device__ inline double cf_term_const(int c) { return c == CF_K_GATE ? CF_GATE_SCALE : (c == CF_K_CAND ? CF_CAND_SCALE : 1.0); }

__host__ __device__ inline double cf_bn_scale(float gamma, float var, float eps) {
#pragma clang fp contract(off)
    return (double)gamma / sqrt((double)var + (double)eps);
}
__host__ __device__ inline double cf_bn_bias(float bias, float beta, float mean, double s) {
#pragma clang fp contract(off)
    return (double)bias * s + (double)beta - (double)mean * s;
}
// p: the term's parameter (RAW, KERN), s / b: its channel's BN scale (KERN) / folded bias (BIAS)
__host__ __device__ inline float cf_term_value(int kind, float p, double s, double b, int c) {
#pragma clang fp contract(off)
    const double base = kind == CF_TERM_RAW ? (double)p : (kind == CF_TERM_KERN ? (double)p * s : (kind == CF_TERM_BIAS ? b : 0.0));
    return (float)(base * cf_term_const(c));
}

struct cf_term {
    int32_t kind = CF_TERM_ZERO;
    int32_t tensor = 0, elem = 0;      // RAW, KERN: element `elem` of tensor `tensor` (cf_tid_*)
    int32_t ch = 0;                    // KERN, BIAS: BN channel = conv unit * cout + output channel
    int32_t c = CF_K_ONE;              // constant factor (cf_term_const)
};
static inline cf_term cf_zero(int c = CF_K_ONE) { cf_term t; t.c = c; return t; }
static inline cf_term cf_raw(int tensor, int elem) { cf_term t; t.kind = CF_TERM_RAW; t.tensor = tensor; t.elem = elem; return t; }
static inline cf_term cf_scaled(cf_term t, int c) { t.c = c; return t; }

// tensor ids = positions in the operator's order (torch_ops.tensor_names): per conv unit kernel, bias, gamma, beta, moving_mean,
// moving_variance; per GRU layer and direction gates kernel, gates bias, candidate kernel, candidate bias; dense kernel, bias
static inline int cf_tid_conv(int unit, int which) { return 6 * unit + which; }
static inline int cf_tid_gru(int n_res, int layer, int dir, int which) { return 24 * n_res + 4 * (2 * layer + dir) + which; }
static inline int cf_tid_dense(int n_res, int n_layers, int which) { return 24 * n_res + 8 * n_layers + which; }
static inline int cf_n_tensors(int n_res, int n_layers) { return 24 * n_res + 8 * n_layers + 2; }

// y = BN(conv(x)) = conv'(x): W' = W s, b' = b s + beta - mean s
struct ConvTerms {
    int k = 0, cin = 0, cout = 0, unit = 0;
    cf_term w(int tap, int in, int o) const {
        cf_term t = cf_raw(cf_tid_conv(unit, 0), (tap * cin + in) * cout + o);
        t.kind = CF_TERM_KERN; t.ch = unit * cout + o;
        return t;
    }
    cf_term b(int o) const { cf_term t; t.kind = CF_TERM_BIAS; t.ch = unit * cout + o; return t; }
};
static ConvTerms conv_terms(int k, int cin, int cout, int unit) { ConvTerms f; f.k = k; f.cin = cin; f.cout = cout; f.unit = unit; return f; }
// conv unit u of the geometry hp (resnet_class.py:44-82: per block shortcut, first, middle (k = 3), last; block 0's first two see the signal)
static ConvTerms unit_terms(const cf_hparams& hp, int u) {
    const int C = hp.layer_size_res;
    return conv_terms(u % 4 == 2 ? 3 : 1, (u < 2) ? 1 : C, C, u);
}

// one direction of a GRU layer of h units over cin_real inputs (kernel rows [0, cin_real) x, [cin_real, cin_real + h) state)
struct GruTerms {
    int t0 = 0, h = 0;                 // tensor id of the gates kernel
    cf_term gk(int in, int o) const { return cf_raw(t0, in * 2 * h + o); }
    cf_term gb(int o) const { return cf_raw(t0 + 1, o); }
    cf_term ck(int in, int o) const { return cf_raw(t0 + 2, in * h + o); }
    cf_term cb(int o) const { return cf_raw(t0 + 3, o); }
};
static GruTerms gru_terms(int t0, int h) { GruTerms g; g.t0 = t0; g.h = h; return g; }

// host evaluation of terms (cf_model_create): tensor pointers of cf_weights, per-channel s and b'
struct cf_host_params {
    std::vector<const float*> t;
    std::vector<double> s, b;
    float param(const cf_term& x) const { return x.kind == CF_TERM_RAW || x.kind == CF_TERM_KERN ? t[x.tensor][x.elem] : 0.f; }
    float value(const cf_term& x) const {
        return cf_term_value(x.kind, param(x), x.kind == CF_TERM_KERN ? s[x.ch] : 0.0, x.kind == CF_TERM_BIAS ? b[x.ch] : 0.0, x.c);
    }
    double base(const cf_term& x) const {          // the term without its constant (the bf16x3 packers scale and split it themselves)
        return x.kind == CF_TERM_RAW ? (double)param(x) : (x.kind == CF_TERM_KERN ? (double)param(x) * s[x.ch] : (x.kind == CF_TERM_BIAS ? b[x.ch] : 0.0));
    }
};
static cf_host_params host_params(const cf_weights* w, const cf_hparams& hp, int cout) {
    cf_host_params P;
    P.t.assign((size_t)cf_n_tensors(hp.n_layers_res, hp.n_layers), nullptr);
    for (int u = 0; u < 4 * hp.n_layers_res; ++u) {
        const cf_conv_bn& c = w->conv[u];
        const float* src[6] = {c.kernel, c.bias, c.gamma, c.beta, c.moving_mean, c.moving_variance};
        for (int i = 0; i < 6; ++i) P.t[cf_tid_conv(u, i)] = src[i];
        for (int o = 0; o < cout; ++o) {
            const double s = cf_bn_scale(c.gamma[o], c.moving_variance[o], hp.bn_epsilon);
            P.s.push_back(s);
            P.b.push_back(cf_bn_bias(c.bias[o], c.beta[o], c.moving_mean[o], s));
        }
    }
    for (int l = 0; l < hp.n_layers; ++l)
        for (int d = 0; d < 2; ++d) {
            const cf_gru_dir& g = w->gru[2 * l + d];
            const float* src[4] = {g.gates_kernel, g.gates_bias, g.candidate_kernel, g.candidate_bias};
            for (int i = 0; i < 4; ++i) P.t[cf_tid_gru(hp.n_layers_res, l, d, i)] = src[i];
        }
    P.t[cf_tid_dense(hp.n_layers_res, hp.n_layers, 0)] = w->dense_kernel;
    P.t[cf_tid_dense(hp.n_layers_res, hp.n_layers, 1)] = w->dense_bias;
    return P;
}
struct HostSink {                      // sink that evaluates every term into a host blob
    const cf_host_params& p;
    float* out;
    void operator()(size_t i, const cf_term& t) const { out[i] = p.value(t); }
};

// [mo][q][r] order == natural order of 16mo+4q+r
template <class E, class V>
static void pack_vec(E& e, size_t off, V v) {
    for (int i = 0; i < CF_C; ++i) e(off + i, v(i));
}

// 32x32 unit: dst[(ks*64 + lane)*2 + mo] = W[in = frag_feature(ks, lane>>4)][out = 16mo + (lane&15)]
template <class E, class W>
static void pack_unit(E& e, size_t off, W w /*(in < 32, out < 32) -> term*/) {
    for (int ks = 0; ks < 8; ++ks)
        for (int lane = 0; lane < 64; ++lane)
            for (int mo = 0; mo < 2; ++mo) e(off + (ks * 64 + lane) * 2 + mo, w(frag_feature(ks, lane >> 4), 16 * mo + (lane & 15)));
}

// the bf16 packers take folded values (double) instead of terms
struct FoldedConv {
    int k = 0, cin = 0;
    std::vector<double> w;  // [k][cin][32] scaled by BN
    std::vector<double> b;  // [32]
};

static FoldedConv fold(const cf_conv_bn& c, float eps) {
    FoldedConv f;
    f.k = c.ksize; f.cin = c.cin;
    f.w.resize((size_t)c.ksize * c.cin * CF_C);
    f.b.resize(CF_C);
    for (int o = 0; o < CF_C; ++o) {
        const double s = cf_bn_scale(c.gamma[o], c.moving_variance[o], eps);
        f.b[o] = cf_bn_bias(c.bias[o], c.beta[o], c.moving_mean[o], s);
        for (int k = 0; k < c.ksize; ++k)
            for (int i = 0; i < c.cin; ++i)
                f.w[((size_t)k * c.cin + i) * CF_C + o] = (double)c.kernel[((size_t)k * c.cin + i) * CF_C + o] * s;
    }
    return f;
}

static std::vector<double> tap(const FoldedConv& f, int k) {
    return std::vector<double>(f.w.begin() + (size_t)k * f.cin * CF_C, f.w.begin() + (size_t)(k + 1) * f.cin * CF_C);
}

// c4: the block's four units (shortcut, first, middle, last); res_pack_floats(first) elements
template <class E>
static int pack_res_block(E& e, const ConvTerms* c4, bool first) {
    const ConvTerms &sc = c4[0], &f1 = c4[1], &f3 = c4[2], &fl = c4[3];
    const int cin = first ? 1 : CF_C;
    if (sc.k != 1 || f1.k != 1 || f3.k != 3 || fl.k != 1 || sc.cin != cin || f1.cin != cin || f3.cin != CF_C || fl.cin != CF_C)
        return fail(CF_ERR_INVALID, "residual block geometry not supported (need k = 1,1,3,1 and 32 channels)");
    const size_t vecs = (size_t)res_units(first) * 1024;
    auto tap_of = [](const ConvTerms& f, int k) { return [&f, k](int in, int o) { return f.w(k, in, o); }; };
    auto b_of = [](const ConvTerms& f) { return [&f](int o) { return f.b(o); }; };
    auto w0_of = [](const ConvTerms& f) { return [&f](int o) { return f.w(0, 0, o); }; };
    if (first) {
        for (int k = 0; k < 3; ++k) pack_unit(e, (size_t)k * 1024, tap_of(f3, k));
        pack_unit(e, 3 * 1024, tap_of(fl, 0));
        pack_vec(e, vecs + 0 * 32, b_of(f3)); pack_vec(e, vecs + 1 * 32, b_of(fl));
        pack_vec(e, vecs + 2 * 32, w0_of(sc)); pack_vec(e, vecs + 3 * 32, b_of(sc));
        pack_vec(e, vecs + 4 * 32, w0_of(f1)); pack_vec(e, vecs + 5 * 32, b_of(f1));
    } else {
        pack_unit(e, 0 * 1024, tap_of(sc, 0));
        pack_unit(e, 1 * 1024, tap_of(f1, 0));
        for (int k = 0; k < 3; ++k) pack_unit(e, (size_t)(2 + k) * 1024, tap_of(f3, k));
        pack_unit(e, 5 * 1024, tap_of(fl, 0));
        pack_vec(e, vecs + 0 * 32, b_of(sc)); pack_vec(e, vecs + 1 * 32, b_of(f1));
        pack_vec(e, vecs + 2 * 32, b_of(f3)); pack_vec(e, vecs + 3 * 32, b_of(fl));
    }
    return CF_OK;
}

static int pack_res_block_bf16(const cf_conv_bn* c4, bool first, float eps, int np, std::vector<char>& out) {
    out.assign(rb_pack_bytes(first, np), 0);
    const FoldedConv sc = fold(c4[0], eps), f1 = fold(c4[1], eps), f3 = fold(c4[2], eps), fl = fold(c4[3], eps);
    const int cin = first ? 1 : CF_C;
    if (sc.k != 1 || f1.k != 1 || f3.k != 3 || fl.k != 1 || sc.cin != cin || f1.cin != cin || f3.cin != CF_C || fl.cin != CF_C)
        return fail(CF_ERR_INVALID, "residual block geometry not supported (need k = 1,1,3,1 and 32 channels)");
    const size_t ub = (size_t)2 * np * 1024;     // bytes per unit
    char* vecs = out.data() + rb_vec_off(first, np);
    if (first) {
        for (int k = 0; k < 3; ++k) pack_unit_bf16(out.data() + k * ub, tap(f3, k), np);
        pack_unit_bf16(out.data() + 3 * ub, tap(fl, 0), np);
        pack_vec32(vecs + 0 * 128, f3.b); pack_vec32(vecs + 1 * 128, fl.b);
        pack_vec32(vecs + 2 * 128, sc.w); pack_vec32(vecs + 3 * 128, sc.b);
        pack_vec32(vecs + 4 * 128, f1.w); pack_vec32(vecs + 5 * 128, f1.b);
    } else {
        pack_unit_bf16(out.data() + 0 * ub, tap(sc, 0), np);
        pack_unit_bf16(out.data() + 1 * ub, tap(f1, 0), np);
        for (int k = 0; k < 3; ++k) pack_unit_bf16(out.data() + (2 + k) * ub, tap(f3, k), np);
        pack_unit_bf16(out.data() + 5 * ub, tap(fl, 0), np);
        pack_vec32(vecs + 0 * 128, sc.b); pack_vec32(vecs + 1 * 128, f1.b);
        pack_vec32(vecs + 2 * 128, f3.b); pack_vec32(vecs + 3 * 128, fl.b);
    }
    return CF_OK;
}

// one direction, gru_pack_floats(cin) elements from `off`; dense_t: tensor id of the dense kernel (-1: zeros), dense_e its first element
template <class E>
static void pack_gru_dir(E& e, size_t off, const GruTerms& g, int cin, int cin_real, int dense_t, int dense_e) {
    // cin = padded input width of the kernel instantiation, cin_real = rows of the x part in the checkpoint
    auto wfull = [&](int in, int o) -> cf_term {   // pre-scaled: the accumulators are exp2 arguments
        if (in < 0) return cf_zero();
        return o < 2 * CF_H ? cf_scaled(g.gk(in, o), CF_K_GATE) : cf_scaled(g.ck(in, o - 2 * CF_H), CF_K_CAND);
    };
    const size_t px = off;
    for (int ks = 0; ks < cin / 4; ++ks)
        for (int gq = 0; gq < 3; ++gq)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    e(px + ((ks * 3 + gq) * 64 + lane) * 4 + j,
                      wfull(frag_feature(ks, lane >> 4) < cin_real ? frag_feature(ks, lane >> 4) : -1, 16 * (4 * gq + j) + (lane & 15)));
    const size_t pg = off + gru_x_floats(cin);
    for (int ks = 0; ks < 16; ++ks)
        for (int gq = 0; gq < 2; ++gq)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    e(pg + ((ks * 2 + gq) * 64 + lane) * 4 + j, wfull(cin_real + frag_feature(ks, lane >> 4), 16 * (4 * gq + j) + (lane & 15)));
    const size_t pc = pg + gru_hg_floats();
    for (int ks = 0; ks < 16; ++ks)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j)
                e(pc + (ks * 64 + lane) * 4 + j, wfull(cin_real + frag_feature(ks, lane >> 4), 2 * CF_H + 16 * j + (lane & 15)));
    const size_t pb = off + gru_bias_off(cin);
    for (int i = 0; i < 2 * CF_H; ++i) e(pb + i, cf_scaled(g.gb(i), CF_K_GATE));
    for (int i = 0; i < CF_H; ++i) e(pb + 2 * CF_H + i, cf_scaled(g.cb(i), CF_K_CAND));
    const size_t pd = off + gru_dense_off(cin);
    for (int i = 0; i < CF_H; ++i) e(pd + i, dense_t >= 0 ? cf_raw(dense_t, dense_e + i) : cf_zero());
}

// the same from host arrays (cf_gru_pack_map's index-encoded weights)
static void pack_gru_dir(const cf_gru_dir& g, int cin, int cin_real, const float* dense_w /*64 floats of this direction or null*/,
                         float* out) {
    cf_host_params P;
    P.t = {g.gates_kernel, g.gates_bias, g.candidate_kernel, g.candidate_bias, dense_w};
    HostSink e{P, out};
    pack_gru_dir(e, 0, gru_terms(0, CF_H), cin, cin_real, dense_w ? 4 : -1, 0);
}

// ---- model lifetime ----------------------------------------------------------------------
static int upload(const std::vector<float>& host, float** dev) {
    HIP_TRY(hipMalloc((void**)dev, host.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(*dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return CF_OK;
}

static bool gen_wanted(const cf_hparams* hp);
static int gen_build(cf_model* m, const cf_weights* w);
static void gen_destroy(cf_generic* g);
static hipError_t cf_optin_all();      // every kernel family's dynamic-LDS opt-in (defined after the last launch helper)

extern "C" void cf_model_destroy(cf_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    for (float* p : m->d_res) if (p) (void)hipFree(p);
    for (float* p : m->d_gru) if (p) (void)hipFree(p);
    for (char* p : m->d_gru_b) if (p) (void)hipFree(p);
    for (char* p : m->d_res_b) if (p) (void)hipFree(p);
    for (auto& sl : m->slots) {
        for (int i = 0; i < 2; ++i) { if (sl.d_a[i]) (void)hipFree(sl.d_a[i]); if (sl.d_y[i]) (void)hipFree(sl.d_y[i]); }
        if (sl.d_p) (void)hipFree(sl.d_p);
        if (sl.d_flags) (void)hipFree(sl.d_flags);
        if (sl.d_hand) (void)hipFree(sl.d_hand);
        if (sl.d_hand_flags) (void)hipFree(sl.d_hand_flags);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    gen_destroy(m->gen);
    pm_destroy(m->pmap);
    if (m->d_dense_bias) (void)hipFree(m->d_dense_bias);
    if (m->d_xp) (void)hipFree(m->d_xp);
    if (m->d_host_x) (void)hipFree(m->d_host_x);
    if (m->h_err) (void)hipHostFree(m->h_err);
    if (m->fork) (void)hipEventDestroy(m->fork);
    for (auto& e : m->ev_pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto& e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;
}

extern "C" int cf_model_create(const cf_weights* w, const cf_hparams* hp, int device, cf_model** out) {
    if (!w || !hp || !out) return fail(CF_ERR_INVALID, "cf_model_create: null argument");
    *out = nullptr;
    if (hp->window != CF_T) return fail(CF_ERR_INVALID, "window must be 35 (rnn_class.py:27)");
    if (hp->n_layers < 1 || hp->n_layers_res < 0) return fail(CF_ERR_INVALID, "n_layers must be >= 1 and n_layers_res >= 0");
    // the shipped geometry (64 GRU units, 32 conv channels) runs on the tuned kernels, every other one on generic.hpp (and so
    // does the plain RNN type in bf16x3; in bf16 it is refused here or by gen_build)
    const bool generic = gen_wanted(hp);
    if (!generic && hp->n_layers_res == 0 && hp->precision != CF_PREC_FP32)
        return fail(CF_ERR_INVALID, "the plain RNN type (n_layers_res = 0) is only built for CF_PREC_FP32");
    if ((hp->n_layers_res > 0 && !w->conv) || !w->gru || !w->dense_kernel || !w->dense_bias)
        return fail(CF_ERR_INVALID, "cf_weights has null members");
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(CF_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    if (hp->precision < CF_PREC_FP32 || hp->precision > CF_PREC_BF16)
        return fail(CF_ERR_INVALID, "precision must be CF_PREC_FP32, CF_PREC_BF16X3 or CF_PREC_BF16");
    cf_model* m = new cf_model();
    m->hp = *hp;
    m->device = device;
    m->np = hp->precision == CF_PREC_FP32 ? 0 : (hp->precision == CF_PREC_BF16X3 ? 2 : 1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->n_cu = prop.multiProcessorCount;
    {
        hipError_t e = hipMalloc((void**)&m->d_dense_bias, sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(m->d_dense_bias, w->dense_bias, sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { cf_model_destroy(m); return fail(CF_ERR_HIP, std::string("dense bias upload: ") + hipGetErrorString(e)); }
    }
    if (generic) {
        const int grc = gen_build(m, w);
        if (grc != CF_OK) { cf_model_destroy(m); return grc; }
        *out = m;
        return CF_OK;
    }
    int rc = CF_OK;
    const cf_host_params P = host_params(w, *hp, CF_C);
    // residual blocks
    for (int b = 0; b < hp->n_layers_res && rc == CF_OK; ++b) {
        std::vector<float> blob(res_pack_floats(b == 0), 0.f);
        ConvTerms c4[4];
        for (int u = 0; u < 4; ++u) c4[u] = conv_terms(w->conv[4 * b + u].ksize, w->conv[4 * b + u].cin, CF_C, 4 * b + u);
        HostSink e{P, blob.data()};
        rc = pack_res_block(e, c4, b == 0);
        if (rc == CF_OK) { float* d = nullptr; rc = upload(blob, &d); m->d_res.push_back(d); }
        if (rc == CF_OK && m->np > 0) {
            std::vector<char> bblob;
            rc = pack_res_block_bf16(w->conv + 4 * b, b == 0, hp->bn_epsilon, m->np, bblob);
            if (rc == CF_OK) {
                char* bptr = nullptr;
                hipError_t e = hipMalloc((void**)&bptr, bblob.size());
                if (e == hipSuccess) e = hipMemcpy(bptr, bblob.data(), bblob.size(), hipMemcpyHostToDevice);
                if (e != hipSuccess) rc = fail(CF_ERR_HIP, std::string("bf16 conv weight upload: ") + hipGetErrorString(e));
                m->d_res_b.push_back(bptr);
            }
        }
    }
    // GRU layers
    for (int l = 0; l < hp->n_layers && rc == CF_OK; ++l) {
        const int cin_real = l == 0 ? (hp->n_layers_res > 0 ? CF_C : 1) : 2 * CF_H;
        const int cin = cin_real == 1 ? 16 : cin_real;     // RNN type: the raw sample embedded in 16 features
        if (w->gru[2 * l].cin != cin_real || w->gru[2 * l + 1].cin != cin_real) { rc = fail(CF_ERR_INVALID, "GRU layer input width mismatch"); break; }
        const bool last = l == hp->n_layers - 1;
        std::vector<float> blob((size_t)2 * gru_pack_floats(cin));
        HostSink e{P, blob.data()};
        for (int d = 0; d < 2; ++d)
            pack_gru_dir(e, (size_t)d * gru_pack_floats(cin), gru_terms(cf_tid_gru(hp->n_layers_res, l, d, 0), CF_H), cin, cin_real,
                         last ? cf_tid_dense(hp->n_layers_res, hp->n_layers, 0) : -1, d * CF_H);
        float* dptr = nullptr;
        rc = upload(blob, &dptr);
        m->d_gru.push_back(dptr);
        m->gru_cin.push_back(cin);
        if (rc == CF_OK && m->np > 0) {
            const size_t bytes = (size_t)gb_pack_bytes(cin, m->np);
            std::vector<char> bblob(2 * bytes, 0);
            for (int d = 0; d < 2; ++d)
                pack_gru_dir_bf16(w->gru[2 * l + d], cin, m->np, last ? w->dense_kernel + d * CF_H : nullptr, bblob.data() + d * bytes);
            char* bptr = nullptr;
            hipError_t e = hipMalloc((void**)&bptr, bblob.size());
            if (e == hipSuccess) e = hipMemcpy(bptr, bblob.data(), bblob.size(), hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = fail(CF_ERR_HIP, std::string("bf16 weight upload: ") + hipGetErrorString(e));
            m->d_gru_b.push_back(bptr);
        }
    }
    // workspace
    if (rc == CF_OK) {
        int64_t cap = hp->max_windows_per_pass > 0 ? hp->max_windows_per_pass : 32768;
        cap = (cap + 2 * CF_TILE - 1) / (2 * CF_TILE) * (2 * CF_TILE);   // whole 32-window tiles (bf16 path)
        m->cap_windows = cap;
        m->cap_tiles = cap / CF_TILE;
        const size_t a_bytes = (size_t)m->cap_tiles * CF_T * 2 * 64 * sizeof(f32x4);
        const size_t y_bytes = (size_t)m->cap_tiles * CF_T * 8 * 64 * sizeof(f32x4);
        // bounds of the launch plans (tuned_launch.hpp): dense partials in either layout, hand-off slots and boundary flags of the
        // largest grid any fp32 biGRU plan returns
        const cf_knobs knobs = cf_read_knobs();
        const size_t p_bytes = cf_dense_partial_floats(m->cap_tiles, m->n_cu) * sizeof(float);
        const size_t hand_bytes = cf_hand_bytes(m->n_cu);
        hipError_t e = hipSuccess;
        int n_slots = hp->n_streams > 0 ? hp->n_streams : 1;   // measured: splitting one call over 2 internal streams is slower
        if (n_slots > 8) n_slots = 8;
        m->slots.resize(n_slots);
        for (auto& sl : m->slots) {
            for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc((void**)&sl.d_a[i], a_bytes);
            for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc((void**)&sl.d_y[i], y_bytes);
            if (e == hipSuccess) e = hipMalloc((void**)&sl.d_p, p_bytes);
            if (e == hipSuccess) e = hipMalloc((void**)&sl.d_flags, (size_t)3 * ((m->cap_tiles + 7) / 8) * 2 * sizeof(unsigned) + 64);
            // (never memset: a slot is written by a head piece before the tail piece of the same launch reads it)
            if (e == hipSuccess && m->np == 0) e = hipMalloc((void**)&sl.d_hand, hand_bytes);
            // zeroed HERE and by cf_clear_error only: every flag's one consumer stores 0 back (cf_handoff_wait_agent)
            if (e == hipSuccess && m->np == 0) e = hipMalloc((void**)&sl.d_hand_flags, cf_hand_flag_bytes(m->n_cu));
            if (e == hipSuccess && m->np == 0) e = hipMemset(sl.d_hand_flags, 0, cf_hand_flag_bytes(m->n_cu));
            if (e == hipSuccess && n_slots > 1) e = hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking);
            if (e == hipSuccess && n_slots > 1) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
        }
        if (e == hipSuccess && n_slots > 1) e = hipEventCreateWithFlags(&m->fork, hipEventDisableTiming);
        if (e == hipSuccess && n_slots == 1 && m->np == 0) {
            // small calls: room for one layer's hoisted x projection
            const int xpt = cf_hoist_limit(m->n_cu, m->cap_tiles, knobs);
            e = hipMalloc((void**)&m->d_xp, cf_xp_floats(xpt) * sizeof(float));
            if (e == hipSuccess) m->xp_tiles = xpt;
        }
        if (e == hipSuccess) e = hipHostMalloc((void**)&m->h_err, sizeof(unsigned), hipHostMallocMapped);
        if (e == hipSuccess) { *m->h_err = 0u; e = hipHostGetDevicePointer((void**)&m->d_err, m->h_err, 0); }
        m->fuse = cf_fuse_mode(m->np == 0 && hp->n_layers <= 3, hp->fuse_layers, knobs);
        if (e != hipSuccess) rc = fail(CF_ERR_NOMEM, std::string("workspace allocation: ") + hipGetErrorString(e));
        m->ws_bytes = (int64_t)n_slots * (int64_t)(2 * a_bytes + 2 * y_bytes + p_bytes + (m->np == 0 ? hand_bytes : 0));
    }
    if (rc == CF_OK) {
        hipError_t e = cf_optin_all();
        if (e != hipSuccess) rc = fail(CF_ERR_HIP, std::string("hipFuncSetAttribute(max dynamic LDS): ") + hipGetErrorString(e));
    }
    if (rc != CF_OK) { std::string keep = g_err; cf_model_destroy(m); g_err = keep; return rc; }
    *out = m;
    return CF_OK;
}

// ---- launch helpers ----------------------------------------------------------------------
static int prof_begin(cf_model* m, int slot, hipStream_t s, size_t* idx) {
    if (!m->prof) return CF_OK;
    cf_model::Ev ev;
    ev.slot = slot;
    for (hipEvent_t* p : {&ev.a, &ev.b}) {
        if (!m->ev_pool.empty()) { *p = m->ev_pool.back(); m->ev_pool.pop_back(); }
        else HIP_TRY(hipEventCreate(p));
    }
    HIP_TRY(hipEventRecord(ev.a, s));
    m->ev_pending.push_back(ev);
    *idx = m->ev_pending.size() - 1;
    return CF_OK;
}
static int prof_end(cf_model* m, hipStream_t s, size_t idx) {
    if (!m->prof) return CF_OK;
    HIP_TRY(hipEventRecord(m->ev_pending[idx].b, s));
    return CF_OK;
}

// f(std::integral_constant<int, V>{}) for the V among Vs that equals the run-time v (the idiom of gru_bf16x3_pipe.hpp): cin
// (16 / 32 / 128), LAST, NP, ... become template arguments inside a generic lambda, so every launch is written once.
template <int... Vs, class F>
static int cf_with(int v, F&& f) {
    int rc = CF_OK;
    const bool hit = ((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return hit ? rc : fail(CF_ERR_INVALID, "no kernel is built for template argument " + std::to_string(v));
}

// Kernels launched with more than 64 KiB of dynamic LDS have to opt in.  Every family states the most it is ever launched with ONCE,
// next to its launch helper, as the plan's own LDS function of its largest pack; cf_model_create opts in all of them (cf_optin_all),
// gen_build the fp32 biGRU family its tuned layers run on.
struct cf_optin {
    hipError_t e = hipSuccess;
    void operator()(const void* f, int bytes) { if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }
};

// ---- fp32 biGRU layer: gru_layer_coop_kernel (+ hoisted x projection) or gru_layer_kernel, as cf_gru_plan_for says ----------------
template <int CIN> constexpr int k_gru_pack_bytes = gru_pack_floats(CIN) * 4;
template <int CIN> constexpr int k_gru_x_bytes = gru_x_floats(CIN) * 4;
static void optin_gru_layer(cf_optin& o) {
    for (int cin : {16, 32, 128})
        for (int last : {0, 1})
            cf_with<16, 32, 128>(cin, [&](auto C) { return cf_with<0, 1>(last, [&](auto L) {
                constexpr int CIN = decltype(C)::value;
                constexpr bool LAST = decltype(L)::value != 0;
                o((const void*)gru_layer_kernel<CIN, LAST>, cf_gru_layer_lds(k_gru_pack_bytes<CIN>));
                o((const void*)gru_layer_coop_kernel<CIN, LAST>, cf_gru_coop_lds(k_gru_pack_bytes<CIN>));
                return CF_OK;
            }); });
    o((const void*)gru_fused_kernel, cf_fused_lds(k_gru_pack_bytes<128>));
    o((const void*)gru_xproj_lds_kernel<32>, k_gru_x_bytes<32>);
    o((const void*)gru_xproj_lds_kernel<128>, k_gru_x_bytes<128>);
}

template <int CIN>
static void launch_xproj(cf_model* m, const cf_xproj_launch& xp, const float* wpack, const float* X, int n_tiles, hipStream_t s) {
    if (xp.lds_kernel)
        hipLaunchKernelGGL((gru_xproj_lds_kernel<CIN>), dim3(xp.grid_x, 2), dim3(256), xp.lds_bytes, s, wpack,
                           reinterpret_cast<const f32x4*>(X), reinterpret_cast<f32x4*>(m->d_xp), n_tiles, xp.chunks);
    else
        hipLaunchKernelGGL((gru_xproj_kernel<CIN>), dim3(xp.grid_x, 2), dim3(256), 0, s, wpack,
                           reinterpret_cast<const f32x4*>(X), reinterpret_cast<f32x4*>(m->d_xp), n_tiles, xp.chunks);
}

// -> the plan it ran (cf_gru_plan::raw_partials tells the head what a LAST launch left in P)
static int launch_gru(cf_model* m, const cf_knobs& k, int cin, bool last, const float* wpack, const float* X, float* Y, float* P, int n_tiles,
                      hipStream_t s, int slot, cf_gru_plan* ran = nullptr,
                      float* hand = nullptr,        // hand-off slots of the balanced schedule (Slot::d_hand); none: round-robin
                      unsigned* hand_flags = nullptr) {     // boundary flags of the grid-wide schedule (Slot::d_hand_flags)
    return cf_with<16, 32, 128>(cin, [&](auto C) { return cf_with<0, 1>(last, [&](auto L) {
        constexpr int CIN = decltype(C)::value;
        constexpr bool LAST = decltype(L)::value != 0;
        const cf_gru_plan p = cf_gru_plan_for(n_tiles, m->n_cu, CIN, k_gru_pack_bytes<CIN>, k_gru_x_bytes<CIN>, m->xp_tiles, hand && hand_flags, k);
        if (ran) *ran = p;
        size_t pi = 0;
        int rc = prof_begin(m, slot, s, &pi);
        if (rc != CF_OK) return rc;
        if (p.coop) {
            if (p.hoist) launch_xproj<CIN>(m, p.xproj, wpack, X, n_tiles, s);
            hipLaunchKernelGGL((gru_layer_coop_kernel<CIN, LAST>), dim3(p.gx, 2), dim3(p.waves * 64), p.lds_bytes, s, wpack,
                               reinterpret_cast<const f32x4*>(X), reinterpret_cast<f32x4*>(Y), P, n_tiles,
                               p.hoist ? reinterpret_cast<const f32x4*>(m->d_xp) : nullptr);
        } else {
            hipLaunchKernelGGL((gru_layer_kernel<CIN, LAST>), dim3(p.gx, 2), dim3(p.waves * 64), p.lds_bytes, s, wpack,
                               reinterpret_cast<const f32x4*>(X), reinterpret_cast<f32x4*>(Y), P, n_tiles, p.balance,
                               reinterpret_cast<f32x4*>(hand), hand_flags, m->d_err);
        }
        HIP_TRY(hipGetLastError());
        return prof_end(m, s, pi);
    }); });
}

// ---- bf16 / bf16x3 biGRU layer: the pipelined kernel of its precision, or round 1's, as cf_gru_bf16_plan_for says ------------------
static void optin_gru_bf16(cf_optin& o) {
    for (int cin : {32, 128})
        for (int last : {0, 1})
            cf_with<32, 128>(cin, [&](auto C) { return cf_with<0, 1>(last, [&](auto L) {
                constexpr int CIN = decltype(C)::value;
                constexpr bool LAST = decltype(L)::value != 0;
                o((const void*)gru_layer_bf16_kernel<CIN, LAST, 1>, gb_pack_bytes(CIN, 1));
                o((const void*)gru_bf16_pipe_kernel<CIN, LAST>, gb_pack_bytes(CIN, 1));
                o((const void*)gru_layer_bf16_kernel<CIN, LAST, 2>, gb_pack_bytes(CIN, 2));
                o((const void*)gru_bf16x3_pipe_kernel<CIN, LAST>, gb_pack_bytes(CIN, 2));
                return CF_OK;
            }); });
}

static int launch_gru_bf16(cf_model* m, const cf_knobs& k, int cin, bool last, const char* wpack, const float* X, float* Y, float* P,
                           int n_tiles32, hipStream_t s, int slot) {
    return cf_with<32, 128>(cin, [&](auto C) { return cf_with<0, 1>(last, [&](auto L) { return cf_with<1, 2>(m->np, [&](auto N) {
        constexpr int CIN = decltype(C)::value, NP = decltype(N)::value;
        constexpr bool LAST = decltype(L)::value != 0;
        const cf_gru_bf16_plan p = cf_gru_bf16_plan_for(n_tiles32, m->n_cu, NP, gb_pack_bytes(CIN, NP), k);
        size_t pi = 0;
        int rc = prof_begin(m, slot, s, &pi);
        if (rc != CF_OK) return rc;
        const dim3 grid(p.gx, 2), block(p.waves * 64);
        const bf16x8* x8 = reinterpret_cast<const bf16x8*>(X);
        bf16x8* y8 = reinterpret_cast<bf16x8*>(Y);
        if (!p.pipe)
            hipLaunchKernelGGL((gru_layer_bf16_kernel<CIN, LAST, NP>), grid, block, p.lds_bytes, s, wpack, x8, y8, P, n_tiles32);
        else if constexpr (NP == 1)      // plain bf16: the software-pipelined kernel (vector work issued behind every MFMA)
            hipLaunchKernelGGL((gru_bf16_pipe_kernel<CIN, LAST>), grid, block, p.lds_bytes, s, wpack, x8, y8, P, n_tiles32);
        else                             // bf16x3: the one-wave-per-SIMD pipelined kernel (512 registers, four waves per workgroup)
            hipLaunchKernelGGL((gru_bf16x3_pipe_kernel<CIN, LAST>), grid, block, p.lds_bytes, s, wpack, x8, y8, P, n_tiles32);
        HIP_TRY(hipGetLastError());
        return prof_end(m, s, pi);
    }); }); });
}

#include "generic_host.hpp"
#include "params_dev.hpp"   // cf_model_param_floats / cf_model_load_params: the packers' terms as a device gather map

// ---- residual stack: fp32 (res_block_kernel, res_stack2_kernel) and bf16 / bf16x3 (res_block_bf16_kernel, res_stack2_bf16_kernel) ----
constexpr int k_res_first_bytes = res_pack_floats(true) * 4, k_res_other_bytes = res_pack_floats(false) * 4;
static void optin_res(cf_optin& o) {
    o((const void*)res_stack2_kernel<true>, cf_res_stack2_lds(k_res_first_bytes, k_res_other_bytes, 4));
    o((const void*)res_stack2_kernel<false>, cf_res_stack2_lds(k_res_first_bytes, k_res_other_bytes, 4));
}

static int run_res_fp32(cf_model* m, cf_model::Slot& sl, const cf_knobs& k, const float* x, int64_t n_windows, int n_tiles, hipStream_t s) {
    const cf_res_plan p = cf_res_plan_for(n_tiles, m->n_cu, m->hp.n_layers_res, k_res_first_bytes, k_res_other_bytes, k);
    sl.last_res_fused = p.fused && !p.split;       // (latency mode also stores block 0's output, for the debug hook)
    int rc;
    size_t pi = 0;
    if (p.fused) {
        if ((rc = prof_begin(m, SLOT_RES_STACK2, s, &pi)) != CF_OK) return rc;
        f32x4* y1 = reinterpret_cast<f32x4*>(sl.d_a[1]);
        if (p.split)
            hipLaunchKernelGGL(res_stack2_kernel<true>, dim3(p.stack_grid), dim3(p.stack_waves * 64), p.stack_lds, s, m->d_res[0], m->d_res[1], x,
                               y1, reinterpret_cast<f32x4*>(sl.d_a[0]), n_windows, n_tiles, p.stack_chunks);
        else
            hipLaunchKernelGGL(res_stack2_kernel<false>, dim3(p.stack_grid), dim3(p.stack_waves * 64), p.stack_lds, s, m->d_res[0], m->d_res[1], x,
                               y1, (f32x4*)nullptr, n_windows, n_tiles, 1);
        HIP_TRY(hipGetLastError());
        if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
    }
    for (int b = p.fused ? 2 : 0; b < m->hp.n_layers_res; ++b) {
        if ((rc = prof_begin(m, b == 0 ? SLOT_RES_FIRST : SLOT_RES, s, &pi)) != CF_OK) return rc;
        f32x4* dst = reinterpret_cast<f32x4*>(sl.d_a[b & 1]);
        if (b == 0)
            hipLaunchKernelGGL((res_block_kernel<true>), dim3(p.grid), dim3(p.waves * 64), p.lds_first, s, m->d_res[0], x,
                               (const f32x4*)nullptr, dst, n_windows, n_tiles, p.chunks);
        else
            hipLaunchKernelGGL((res_block_kernel<false>), dim3(p.grid), dim3(p.waves * 64), p.lds_other, s, m->d_res[b], (const float*)nullptr,
                               reinterpret_cast<const f32x4*>(sl.d_a[(b - 1) & 1]), dst, n_windows, n_tiles, p.chunks);
        HIP_TRY(hipGetLastError());
        if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
    }
    return CF_OK;
}

static int run_res_bf16(cf_model* m, cf_model::Slot& sl, const cf_knobs& k, const float* x, int64_t n_windows, int n_tiles32, hipStream_t s) {
    return cf_with<1, 2>(m->np, [&](auto N) {
        constexpr int NP = decltype(N)::value;
        const cf_res_bf16_plan p = cf_res_bf16_plan_for(n_tiles32, m->n_cu, m->hp.n_layers_res, NP, rb_pack_bytes(true, NP), rb_pack_bytes(false, NP),
                                                        CF_RES_BF16_WAVES, k);
        sl.last_res_fused = p.fused;
        int rc;
        size_t pi = 0;
        if (p.fused) {
            if ((rc = prof_begin(m, SLOT_RES_STACK2, s, &pi)) != CF_OK) return rc;
            rc = cf_with<1, NP == 1 ? 2 : 1>(p.tpw, [&](auto W) {      // (two tiles per wave are built for one bf16 part only)
                hipLaunchKernelGGL((res_stack2_bf16_kernel<NP, decltype(W)::value>), dim3(p.stack_grid), dim3(256), p.stack_lds, s, m->d_res_b[0],
                                   m->d_res_b[1], x, reinterpret_cast<bf16x8*>(sl.d_a[1]), n_windows, n_tiles32, p.chunks);
                return CF_OK;
            });
            if (rc != CF_OK) return rc;
            HIP_TRY(hipGetLastError());
            if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
        }
        for (int b = p.fused ? 2 : 0; b < m->hp.n_layers_res; ++b) {
            if ((rc = prof_begin(m, b == 0 ? SLOT_RES_FIRST : SLOT_RES, s, &pi)) != CF_OK) return rc;
            bf16x8* dst = reinterpret_cast<bf16x8*>(sl.d_a[b & 1]);
            if (b == 0)
                hipLaunchKernelGGL((res_block_bf16_kernel<true, NP>), dim3(p.grid), dim3(256), p.lds_first, s, m->d_res_b[0], x, (const bf16x8*)nullptr,
                                   dst, n_windows, n_tiles32);
            else
                hipLaunchKernelGGL((res_block_bf16_kernel<false, NP>), dim3(p.grid), dim3(256), p.lds_other, s, m->d_res_b[b], (const float*)nullptr,
                                   reinterpret_cast<const bf16x8*>(sl.d_a[(b - 1) & 1]), dst, n_windows, n_tiles32);
            HIP_TRY(hipGetLastError());
            if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
        }
        return CF_OK;
    });
}

static int run_pass(cf_model* m, cf_model::Slot& sl, const float* x, int64_t n_windows, float* probs, float* logits, hipStream_t s) {
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    const int n_tiles32 = (int)((n_windows + 2 * CF_TILE - 1) / (2 * CF_TILE));
    const cf_knobs k = cf_read_knobs();
    int rc;
    size_t pi = 0;
    if ((rc = m->np > 0 ? run_res_bf16(m, sl, k, x, n_windows, n_tiles32, s) : run_res_fp32(m, sl, k, x, n_windows, n_tiles, s)) != CF_OK) return rc;
    if (m->hp.n_layers_res == 0) {
        if ((rc = prof_begin(m, SLOT_RES_FIRST, s, &pi)) != CF_OK) return rc;
        const int64_t n_el = (int64_t)n_tiles * CF_T * 64;
        hipLaunchKernelGGL(embed_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s, x,
                           reinterpret_cast<f32x4*>(sl.d_a[0]), n_windows, n_tiles);
        HIP_TRY(hipGetLastError());
        if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
    }
    const float* cur = m->hp.n_layers_res == 0 ? sl.d_a[0] : sl.d_a[(m->hp.n_layers_res - 1) & 1];
    // GRU layers
    cf_gru_plan last_gru = {};      // what the last biGRU launch left in d_p: only the fp32 per-layer launch can leave raw partials
    const int cin0 = m->hp.n_layers_res == 0 ? 16 : CF_C;     // RNN type: the raw sample embedded in 16 features
    if (cf_fuse_now(m->fuse, n_tiles, m->n_cu)) {
        cf_fused_args a;
        a.lds_floats = m->hp.n_layers > 1 ? gru_pack_floats(128) : gru_pack_floats(cin0);
        const cf_fused_plan p = cf_fused_plan_for(n_tiles, m->n_cu, m->hp.n_layers, a.lds_floats * 4);
        for (int l = 0; l < 3; ++l) a.w[l] = l < m->hp.n_layers ? m->d_gru[l] : nullptr;
        a.x0 = reinterpret_cast<const f32x4*>(cur);
        a.y[0] = reinterpret_cast<f32x4*>(sl.d_y[0]);
        a.y[1] = reinterpret_cast<f32x4*>(sl.d_y[1]);
        a.p = sl.d_p;
        a.flags = sl.d_flags;
        a.err = m->d_err;
        a.n_tiles = n_tiles;
        a.groups = p.groups;
        a.n_layers = m->hp.n_layers;
        a.cin0 = cin0;
        HIP_TRY(hipMemsetAsync(sl.d_flags, 0, ((size_t)a.n_layers * a.groups * 2 + (size_t)a.n_layers * 2) * sizeof(unsigned), s));
        if ((rc = prof_begin(m, SLOT_GRU_FUSED, s, &pi)) != CF_OK) return rc;
        hipLaunchKernelGGL(gru_fused_kernel, dim3((unsigned)p.grid), dim3(p.threads), p.lds_bytes, s, a);
        HIP_TRY(hipGetLastError());
        if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
    } else {
        for (int l = 0; l < m->hp.n_layers; ++l) {
            const bool last = l == m->hp.n_layers - 1;
            const int slot = last ? SLOT_GRU_LAST : (l == 0 ? SLOT_GRU0 : SLOT_GRU);
            float* y = sl.d_y[l & 1];
            rc = m->np > 0 ? launch_gru_bf16(m, k, m->gru_cin[l], last, m->d_gru_b[l], cur, y, sl.d_p, n_tiles32, s, slot)
                           : launch_gru(m, k, m->gru_cin[l], last, m->d_gru[l], cur, y, sl.d_p, n_tiles, s, slot, &last_gru, sl.d_hand, sl.d_hand_flags);
            if (rc != CF_OK) return rc;
            cur = y;
        }
    }
    // head
    if ((rc = prof_begin(m, SLOT_HEAD, s, &pi)) != CF_OK) return rc;
    const int64_t total = n_windows * CF_T;
    hipLaunchKernelGGL(head_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sl.d_p, m->d_dense_bias, probs, logits, n_windows,
                       m->np > 0 ? n_tiles32 : n_tiles, m->np > 0 ? 5 : 4, last_gru.raw_partials);
    HIP_TRY(hipGetLastError());
    if ((rc = prof_end(m, s, pi)) != CF_OK) return rc;
    sl.last_windows = n_windows;
    return CF_OK;
}

static const char* k_fused_timeout_msg = "a fused biGRU launch timed out waiting for a producer workgroup; its results are invalid "
                                         "(create the model with fuse_layers = -1)";

extern "C" int cf_check_error(cf_model* m) {
    if (!m) return fail(CF_ERR_INVALID, "cf_check_error: null model");
    if (m->h_err && *m->h_err) return fail(CF_ERR_HIP, k_fused_timeout_msg);
    return CF_OK;
}

extern "C" int cf_clear_error(cf_model* m) {
    if (!m) return fail(CF_ERR_INVALID, "cf_clear_error: null model");
    if (m->h_err) *m->h_err = 0u;       // every fused launch re-initialises its own queues and flags
    // the grid-wide biGRU schedule's boundary flags are zero between launches unless a wait timed out: a flag published after its
    // consumer gave up stays set
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    for (auto& sl : m->slots)
        if (sl.d_hand_flags) HIP_TRY(hipMemset(sl.d_hand_flags, 0, cf_hand_flag_bytes(m->n_cu)));
    return CF_OK;
}

extern "C" int cf_launch_regimes(const cf_model* m, int64_t out[4]) {
    if (!m || !out) return fail(CF_ERR_INVALID, "cf_launch_regimes: null argument");
    out[0] = m->n_cu;
    if (m->gen) { out[1] = out[2] = out[3] = 0; return CF_OK; }       // one launch shape at every size
    out[1] = (int64_t)m->xp_tiles * CF_TILE;
    out[2] = m->np == 0 ? (int64_t)cf_coop_max_tiles(m->n_cu) * CF_TILE : 0;
    out[3] = m->fuse == 1 ? 1 : (m->fuse == 2 ? cf_fuse_auto_min_windows(m->n_cu) : 0);
    return CF_OK;
}

extern "C" int cf_infer_logits(cf_model* m, const float* x, int64_t n_windows, float* probs, float* logits, void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_infer: null model");
    if (n_windows < 0) return fail(CF_ERR_INVALID, "cf_infer: negative n_windows");
    if (n_windows == 0) return CF_OK;
    if (!x || (!probs && !logits)) return fail(CF_ERR_INVALID, "cf_infer: null buffer");
    if (m->h_err && *m->h_err) return fail(CF_ERR_HIP, k_fused_timeout_msg);
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    m->prof = m->prof_every > 0 && (m->prof_calls++ % m->prof_every) == 0;
    if (m->gen) {
        for (int64_t off = 0; off < n_windows; off += m->cap_windows) {
            const int64_t n = std::min(m->cap_windows, n_windows - off);
            const int rc = gen_run_pass(m, x + off * CF_T, n, probs ? probs + off * CF_T : nullptr, logits ? logits + off * CF_T : nullptr, s);
            if (rc != CF_OK) return rc;
        }
        return CF_OK;
    }
    const int n_slots = (int)m->slots.size();
    // sub-batch size: split the call evenly over the slots, in whole 8-tile groups (128 windows)
    int64_t chunk = m->cap_windows;
    if (n_slots > 1) {
        const int64_t per = ((n_windows + n_slots - 1) / n_slots + 127) / 128 * 128;
        chunk = std::min(m->cap_windows, std::max<int64_t>(per, 128));
    }
    if (n_slots == 1 || n_windows <= 2048) {
        // small calls (a single read) are launch-bound: no fork/join
        for (int64_t off = 0; off < n_windows; off += m->cap_windows) {
            const int64_t n = std::min(m->cap_windows, n_windows - off);
            const int rc = run_pass(m, m->slots[0], x + off * CF_T, n, probs ? probs + off * CF_T : nullptr,
                                    logits ? logits + off * CF_T : nullptr, s);
            if (rc != CF_OK) return rc;
        }
        if (n_slots > 1) {
            // keep slot 0's scratch ordered against a later forked call on its internal stream
            HIP_TRY(hipEventRecord(m->slots[0].done, s));
            HIP_TRY(hipStreamWaitEvent(m->slots[0].stream, m->slots[0].done, 0));
        }
        return CF_OK;
    }
    // fork: every slot stream waits for the caller's stream, runs its sub-batches, joins back
    HIP_TRY(hipEventRecord(m->fork, s));
    for (auto& sl : m->slots) HIP_TRY(hipStreamWaitEvent(sl.stream, m->fork, 0));
    int k = 0;
    for (int64_t off = 0; off < n_windows; off += chunk, ++k) {
        const int64_t n = std::min(chunk, n_windows - off);
        cf_model::Slot& sl = m->slots[k % n_slots];
        const int rc = run_pass(m, sl, x + off * CF_T, n, probs ? probs + off * CF_T : nullptr, logits ? logits + off * CF_T : nullptr, sl.stream);
        if (rc != CF_OK) return rc;
    }
    for (auto& sl : m->slots) {
        HIP_TRY(hipEventRecord(sl.done, sl.stream));
        HIP_TRY(hipStreamWaitEvent(s, sl.done, 0));
    }
    return CF_OK;
}

extern "C" int cf_infer(cf_model* m, const float* x, int64_t n_windows, float* probs, void* stream) {
    if (n_windows > 0 && !probs) return fail(CF_ERR_INVALID, "cf_infer: null buffer");
    return cf_infer_logits(m, x, n_windows, probs, nullptr, stream);
}

extern "C" int cf_infer_host_logits(cf_model* m, const float* x, int64_t n_windows, float* probs, float* logits) {
    if (!m) return fail(CF_ERR_INVALID, "cf_infer_host: null model");
    if (n_windows < 0) return fail(CF_ERR_INVALID, "cf_infer_host: negative n_windows");
    if (n_windows == 0) return CF_OK;
    if (!x || (!probs && !logits)) return fail(CF_ERR_INVALID, "cf_infer_host: null buffer");
    HIP_TRY(hipSetDevice(m->device));
    const size_t bytes = (size_t)n_windows * CF_T * sizeof(float);
    // device staging buffers are kept across calls (the reference calls infer once per read): x, probs, logits
    if (m->host_stage_bytes < bytes) {
        if (m->d_host_x) (void)hipFree(m->d_host_x);
        m->d_host_x = m->d_host_p = nullptr;
        m->host_stage_bytes = 0;
        const size_t cap = (bytes + bytes / 4 + 255) / 256 * 256;
        hipError_t e2 = hipMalloc((void**)&m->d_host_x, 3 * cap);
        if (e2 != hipSuccess) { m->d_host_x = nullptr; return fail(CF_ERR_NOMEM, "cf_infer_host: hipMalloc failed"); }
        m->d_host_p = m->d_host_x + cap / sizeof(float);
        m->host_stage_bytes = cap;
    }
    float *dx = m->d_host_x, *dp = m->d_host_p, *dl = m->d_host_p + m->host_stage_bytes / sizeof(float);
    hipError_t e = hipSuccess;
    int rc = CF_OK;
    if ((e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice)) != hipSuccess) rc = fail(CF_ERR_HIP, hipGetErrorString(e));
    if (rc == CF_OK) rc = cf_infer_logits(m, dx, n_windows, probs ? dp : nullptr, logits ? dl : nullptr, nullptr);
    if (rc == CF_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = fail(CF_ERR_HIP, hipGetErrorString(e));
    if (rc == CF_OK) rc = cf_check_error(m);
    if (rc == CF_OK && probs && (e = hipMemcpy(probs, dp, bytes, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail(CF_ERR_HIP, hipGetErrorString(e));
    if (rc == CF_OK && logits && (e = hipMemcpy(logits, dl, bytes, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail(CF_ERR_HIP, hipGetErrorString(e));
    return rc;
}

extern "C" int cf_infer_host(cf_model* m, const float* x, int64_t n_windows, float* probs) {
    if (n_windows > 0 && !probs) return fail(CF_ERR_INVALID, "cf_infer_host: null buffer");
    return cf_infer_host_logits(m, x, n_windows, probs, nullptr);
}

// grid of the bit-mask post-processing kernels over `total` packed samples: 64 samples a word, CF_POST_WORDS payload words a wave,
// four waves a workgroup
static dim3 post_bits_grid(int64_t total) {
    const int64_t n_words = (total + 63) / 64, n_chunks = (n_words + CF_POST_WORDS - 1) / CF_POST_WORDS;
    return dim3((unsigned)((n_chunks + 3) / 4));
}

extern "C" int cf_postprocess(cf_model* m, const float* probs, const int64_t* read_offsets, const int64_t* read_lengths,
                              int64_t n_reads, int64_t total_samples, float threshold, int32_t min_run, uint8_t* labels,
                              void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_postprocess: null model");
    if (n_reads < 0 || total_samples < 0) return fail(CF_ERR_INVALID, "cf_postprocess: negative size");
    if (n_reads == 0 || total_samples == 0) return CF_OK;
    if (min_run < 1) return fail(CF_ERR_INVALID, "cf_postprocess: min_run must be >= 1");
    if (!probs || !read_offsets || !read_lengths || !labels) return fail(CF_ERR_INVALID, "cf_postprocess: null buffer");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    size_t pi = 0;
    int rc = prof_begin(m, SLOT_POST, s, &pi);
    if (rc != CF_OK) return rc;
    const bool v1 = cf_knob("CATFISH_INGEST_V1") && atoi(cf_knob("CATFISH_INGEST_V1")) != 0;
    // the bit-mask kernel's window covers runs of up to 64 samples (the reference uses 15) and it stores labels 16 bytes at a time
    if (v1 || min_run > 64 || (reinterpret_cast<uintptr_t>(labels) & 15u) != 0) {
        hipLaunchKernelGGL(postprocess_kernel, dim3((unsigned)((total_samples + 255) / 256)), dim3(256), 0, s, probs, read_offsets,
                           read_lengths, n_reads, total_samples, threshold, (int)min_run, labels);
    } else {
        hipLaunchKernelGGL(postprocess_bits_kernel<false>, post_bits_grid(total_samples), dim3(256), 0, s, probs, read_offsets,
                           read_lengths, n_reads, total_samples, threshold, (int)min_run, labels, (int64_t)0, (int64_t*)nullptr,
                           (int64_t*)nullptr, (unsigned long long*)nullptr);
    }
    HIP_TRY(hipGetLastError());
    return prof_end(m, s, pi);
}

// cf_postprocess + cf_spans as ONE launch ("one segmented-scan kernel returning spans"): the corrected labels' run
// boundaries come straight from the bit masks; labels may be NULL when only the spans are wanted (the streaming pipeline).
extern "C" int cf_postprocess_spans(cf_model* m, const float* probs, const int64_t* read_offsets, const int64_t* read_lengths,
                                    int64_t n_reads, int64_t total_samples, float threshold, int32_t min_run, uint8_t* labels,
                                    int64_t max_runs, int64_t* starts, int64_t* ends, uint64_t* counts, void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_postprocess_spans: null model");
    if (n_reads < 0 || total_samples < 0 || max_runs < 0) return fail(CF_ERR_INVALID, "cf_postprocess_spans: negative size");
    if (!counts) return fail(CF_ERR_INVALID, "cf_postprocess_spans: null counts");
    if (min_run < 1) return fail(CF_ERR_INVALID, "cf_postprocess_spans: min_run must be >= 1");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s));
    if (n_reads == 0 || total_samples == 0) return CF_OK;
    if (!probs || !read_offsets || !read_lengths || (max_runs > 0 && (!starts || !ends)))
        return fail(CF_ERR_INVALID, "cf_postprocess_spans: null buffer");
    const bool v1 = cf_knob("CATFISH_INGEST_V1") && atoi(cf_knob("CATFISH_INGEST_V1")) != 0;
    if (v1 || min_run > 64 || (reinterpret_cast<uintptr_t>(labels) & 15u) != 0) {
        // what the bit-mask kernel does not cover (min_run > 64, an unaligned labels pointer) or is told not to take (the
        // CATFISH_INGEST_V1 A/B knob) goes through the two calls it replaces.  They need a labels buffer: a caller that asked for the
        // spans only (labels NULL -- the streaming pipeline) gets a stream-ordered temporary one.
        uint8_t* lab = labels;
        if (!lab) {
            hipError_t e = hipMallocAsync((void**)&lab, (size_t)total_samples, s);
            if (e != hipSuccess) return fail(CF_ERR_NOMEM, std::string("cf_postprocess_spans: no device memory for the temporary labels: ") + hipGetErrorString(e));
        }
        int rc = cf_postprocess(m, probs, read_offsets, read_lengths, n_reads, total_samples, threshold, min_run, lab, stream);
        if (rc == CF_OK) rc = cf_spans(m, lab, total_samples, max_runs, starts, ends, counts, stream);
        if (rc == CF_OK && n_reads > 1) {
            // cf_spans sees labels only: where an UNPADDED read's last sample and the next read's first are both positive it found one
            // run; cut it at the read boundary (one end + one start more; the lists are sorted before pairing, so order is free)
            hipLaunchKernelGGL(spans_cut_kernel, dim3((unsigned)((n_reads - 1 + 255) / 256)), dim3(256), 0, s, lab, read_offsets, read_lengths,
                               n_reads, total_samples, max_runs, starts, ends, reinterpret_cast<unsigned long long*>(counts));
            if (hipGetLastError() != hipSuccess) rc = fail(CF_ERR_HIP, "cf_postprocess_spans: launch failed");
        }
        if (!labels) (void)hipFreeAsync(lab, s);
        return rc;
    }
    size_t pi = 0;
    int rc = prof_begin(m, SLOT_POST, s, &pi);
    if (rc != CF_OK) return rc;
    hipLaunchKernelGGL(postprocess_bits_kernel<true>, post_bits_grid(total_samples), dim3(256), 0, s, probs, read_offsets, read_lengths,
                       n_reads, total_samples, threshold, (int)min_run, labels, max_runs, starts, ends,
                       reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return prof_end(m, s, pi);
}

// cf_postprocess_spans with gaps of at most max_gap samples between two stretches of one read bridged before correct_short
// (csrc/post_bridge_rule.hpp; infer.bridge_gaps is the definition).  max_gap == 0 IS cf_postprocess_spans; any other pair must lie in
// the bit-mask kernel's domain -- there is no slower route to fall back to.
extern "C" int cf_postprocess_spans_bridged(cf_model* m, const float* probs, const int64_t* read_offsets, const int64_t* read_lengths,
                                            int64_t n_reads, int64_t total_samples, float threshold, int32_t max_gap, int32_t min_run,
                                            uint8_t* labels, int64_t max_runs, int64_t* starts, int64_t* ends, uint64_t* counts,
                                            void* stream) {
    if (max_gap == 0)
        return cf_postprocess_spans(m, probs, read_offsets, read_lengths, n_reads, total_samples, threshold, min_run, labels, max_runs, starts,
                                    ends, counts, stream);
    if (!m) return fail(CF_ERR_INVALID, "cf_postprocess_spans_bridged: null model");
    if (n_reads < 0 || total_samples < 0 || max_runs < 0) return fail(CF_ERR_INVALID, "cf_postprocess_spans_bridged: negative size");
    if (!counts) return fail(CF_ERR_INVALID, "cf_postprocess_spans_bridged: null counts");
    if (!pb_domain(min_run, max_gap))
        return fail(CF_ERR_INVALID, "cf_postprocess_spans_bridged: needs min_run >= 1, max_gap >= 0 and min_run + max_gap <= 64");
    if ((reinterpret_cast<uintptr_t>(labels) & 15u) != 0) return fail(CF_ERR_INVALID, "cf_postprocess_spans_bridged: labels must be 16-byte aligned");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s));
    if (n_reads == 0 || total_samples == 0) return CF_OK;
    if (!probs || !read_offsets || !read_lengths || (max_runs > 0 && (!starts || !ends)))
        return fail(CF_ERR_INVALID, "cf_postprocess_spans_bridged: null buffer");
    size_t pi = 0;
    int rc = prof_begin(m, SLOT_POST, s, &pi);
    if (rc != CF_OK) return rc;
    hipLaunchKernelGGL(postprocess_bridged_kernel<true>, post_bits_grid(total_samples), dim3(256), 0, s, probs, read_offsets,
                       read_lengths, n_reads, total_samples, threshold, (int)max_gap, (int)min_run, labels, max_runs, starts, ends,
                       reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return prof_end(m, s, pi);
}

// Per-call scores (csrc/span_scores.hpp): row k belongs to starts[k]; rows at and above min(counts[0], max_runs) are left untouched.
extern "C" int cf_span_scores(cf_model* m, const float* probs, const float* signal, const int64_t* read_offsets,
                              const int64_t* read_lengths, int64_t n_reads, int64_t total_samples, float threshold, const int64_t* starts,
                              const uint64_t* counts, int64_t max_runs, int64_t* ends_paired, double* sums, float* extremes, void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_span_scores: null model");
    if (n_reads < 0 || total_samples < 0 || max_runs < 0) return fail(CF_ERR_INVALID, "cf_span_scores: negative size");
    if (!counts) return fail(CF_ERR_INVALID, "cf_span_scores: null counts");
    if (max_runs == 0) return CF_OK;
    if (!starts || !ends_paired || !sums || !extremes) return fail(CF_ERR_INVALID, "cf_span_scores: null buffer");
    if (n_reads > 0 && total_samples > 0 && (!probs || !read_offsets || !read_lengths)) return fail(CF_ERR_INVALID, "cf_span_scores: null buffer");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (with no read or no sample every start is outside every read: the kernel writes empty rows without a load)
    const int64_t blocks = (max_runs + CF_SCORE_WAVES - 1) / CF_SCORE_WAVES;
    hipLaunchKernelGGL(span_scores_kernel, dim3((unsigned)(blocks < CF_SCORE_MAX_BLOCKS ? blocks : CF_SCORE_MAX_BLOCKS)), dim3(64 * CF_SCORE_WAVES),
                       0, s, probs, signal, read_offsets, read_lengths, n_reads, total_samples, threshold, starts,
                       reinterpret_cast<const unsigned long long*>(counts), max_runs, ends_paired, sums, extremes);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

// cf_span_scores over runs that are given by LABELS (what cf_postprocess_spans_bridged wrote): a bridged run holds samples below the
// threshold, and they belong to its sums and extremes.
extern "C" int cf_span_scores_labels(cf_model* m, const float* probs, const float* signal, const uint8_t* labels, const int64_t* read_offsets,
                                     const int64_t* read_lengths, int64_t n_reads, int64_t total_samples, const int64_t* starts,
                                     const uint64_t* counts, int64_t max_runs, int64_t* ends_paired, double* sums, float* extremes,
                                     void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_span_scores_labels: null model");
    if (n_reads < 0 || total_samples < 0 || max_runs < 0) return fail(CF_ERR_INVALID, "cf_span_scores_labels: negative size");
    if (!counts) return fail(CF_ERR_INVALID, "cf_span_scores_labels: null counts");
    if (max_runs == 0) return CF_OK;
    if (!starts || !ends_paired || !sums || !extremes) return fail(CF_ERR_INVALID, "cf_span_scores_labels: null buffer");
    if (n_reads > 0 && total_samples > 0 && (!probs || !labels || !read_offsets || !read_lengths))
        return fail(CF_ERR_INVALID, "cf_span_scores_labels: null buffer");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t blocks = (max_runs + CF_SCORE_WAVES - 1) / CF_SCORE_WAVES;
    hipLaunchKernelGGL(span_scores_labels_kernel, dim3((unsigned)(blocks < CF_SCORE_MAX_BLOCKS ? blocks : CF_SCORE_MAX_BLOCKS)),
                       dim3(64 * CF_SCORE_WAVES), 0, s, probs, signal, labels, read_offsets, read_lengths, n_reads, total_samples, starts,
                       reinterpret_cast<const unsigned long long*>(counts), max_runs, ends_paired, sums, extremes);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_spans(cf_model* m, const uint8_t* labels, int64_t total_samples, int64_t max_runs, int64_t* starts,
                        int64_t* ends, uint64_t* counts, void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_spans: null model");
    if (total_samples < 0 || max_runs < 0) return fail(CF_ERR_INVALID, "cf_spans: negative size");
    if (!counts) return fail(CF_ERR_INVALID, "cf_spans: null counts");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s));
    if (total_samples == 0) return CF_OK;
    if (!labels || (max_runs > 0 && (!starts || !ends))) return fail(CF_ERR_INVALID, "cf_spans: null buffer");
    const int64_t per_wg = 256 * CF_SPANS_PER_THREAD;
    hipLaunchKernelGGL(spans_kernel, dim3((unsigned)((total_samples + per_wg - 1) / per_wg)), dim3(256), 0, s, labels, total_samples, max_runs,
                       starts, ends, reinterpret_cast<unsigned long long*>(counts));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_normalize(cf_model* m, const int16_t* dac, const int64_t* dac_offsets, const int64_t* win_offsets,
                            int64_t n_reads, float* x_out, void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_normalize: null model");
    if (n_reads < 0) return fail(CF_ERR_INVALID, "cf_normalize: negative n_reads");
    if (n_reads == 0) return CF_OK;
    if (!dac || !dac_offsets || !win_offsets || !x_out) return fail(CF_ERR_INVALID, "cf_normalize: null buffer");
    if (n_reads > 0x7FFFFFFF) return fail(CF_ERR_INVALID, "cf_normalize: too many reads in one call");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    size_t pi = 0;
    int rc = prof_begin(m, SLOT_NORM, s, &pi);
    if (rc != CF_OK) return rc;
    if (cf_knob("CATFISH_INGEST_V1") && atoi(cf_knob("CATFISH_INGEST_V1")) != 0)      // A/B and bit-identity tests: round 1's kernel
        hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)n_reads), dim3(256), 0, s, dac, dac_offsets, win_offsets, x_out);
    else {                                                                              // reads <= 4096 samples, then the longer ones
        hipLaunchKernelGGL(normalize_regs_kernel<CF_NORM_REGS_SMALL>, dim3((unsigned)n_reads), dim3(256), 0, s, dac, dac_offsets, win_offsets, x_out);
        hipLaunchKernelGGL(normalize_regs_kernel<CF_NORM_REGS_LARGE>, dim3((unsigned)n_reads), dim3(256), 0, s, dac, dac_offsets, win_offsets, x_out);
    }
    HIP_TRY(hipGetLastError());
    return prof_end(m, s, pi);
}

// ---- training support (BASELINE config 5) ------------------------------------------------
// Gather map of the weight re-tiling, so that a trainer can re-tile updated weights ON DEVICE
// (packed = src[idx] * scale) instead of round-tripping through the host packers every step.
// src (one direction) = [gates_kernel ((cin+64)*128) | candidate_kernel ((cin+64)*64) | gates_bias (128) |
// candidate_bias (64) | 0.0]; the map is derived from the host packers themselves (index-encoded weights).
extern "C" int cf_gru_pack_map(int32_t cin, int32_t backward, int32_t* idx, float* scale, int64_t capacity, int64_t* n_floats) {
    if (cin != CF_C && cin != 2 * CF_H) return fail(CF_ERR_INVALID, "cf_gru_pack_map: cin must be 32 or 128");
    const int64_t n = backward ? gtb_pack_floats(cin) : gru_pack_floats(cin);
    if (n_floats) *n_floats = n;
    if (!idx || !scale) return CF_OK;                       // size query
    if (capacity < n) return fail(CF_ERR_INVALID, "cf_gru_pack_map: buffers too small");
    const int rows = cin + CF_H;
    const size_t n_gk = (size_t)rows * 2 * CF_H, n_ck = (size_t)rows * CF_H;
    const size_t n_src = n_gk + n_ck + 2 * CF_H + CF_H;     // + the trailing zero slot = index n_src
    std::vector<float> gk(n_gk), ck(n_ck), gb(2 * CF_H), cb(CF_H);
    cf_gru_dir g;
    g.gates_kernel = gk.data(); g.gates_bias = gb.data(); g.candidate_kernel = ck.data(); g.candidate_bias = cb.data(); g.cin = cin;
    std::vector<float> ones((size_t)n), enc((size_t)n);
    auto run = [&](std::vector<float>& out) {
        if (backward) pack_gru_dir_bwd(g, cin, out.data());
        else pack_gru_dir(g, cin, cin, nullptr, out.data());
    };
    for (auto* v : {&gk, &ck, &gb, &cb}) std::fill(v->begin(), v->end(), 1.0f);
    run(ones);                                              // = the scale applied to every packed element (0 = constant zero)
    size_t base = 0;
    for (auto* v : {&gk, &ck, &gb, &cb}) { for (size_t i = 0; i < v->size(); ++i) (*v)[i] = (float)(base + i + 1); base += v->size(); }
    run(enc);
    for (int64_t i = 0; i < n; ++i) {
        scale[i] = ones[i];
        idx[i] = ones[i] == 0.f ? (int32_t)n_src : (int32_t)(std::llround((double)enc[i] / (double)ones[i]) - 1);
        if (idx[i] < 0 || idx[i] > (int32_t)n_src) return fail(CF_ERR_INVALID, "cf_gru_pack_map: internal index error");
    }
    return CF_OK;
}

static int train_cin_ok(const cf_model* m, int cin) {
    if (m->np != 0) return fail(CF_ERR_INVALID, "training kernels need a CF_PREC_FP32 model");
    if (m->hp.layer_size != CF_H) return fail(CF_ERR_INVALID, "training kernels: layer_size 64 only (other sizes: cf_gru_anysize_train_*)");
    if (m->gen) return fail(CF_ERR_INVALID, "training kernels need a model on the tuned path (unset CATFISH_GENERIC)");
    if (cin != CF_C && cin != 2 * CF_H) return fail(CF_ERR_INVALID, "training kernels: cin must be 32 or 128");
    return CF_OK;
}

static cf_dropout make_dropout(float keep_prob, uint32_t seed, int32_t layer, const double* step_count) {
    cf_dropout d;
    d.keep_prob = keep_prob;
    d.seed = seed;
    d.layer = layer;
    d.step = step_count;
    return d;
}

extern "C" int cf_gru_train_forward_dropout(cf_model* m, int32_t cin, const float* wpack, const float* x_frag, float* y_frag, float* stash,
                                            int64_t n_windows, float* y_drop_frag, float keep_prob, uint32_t seed, int32_t layer,
                                            const double* step_count, void* stream) {
    if (!m || !wpack || !x_frag || !y_frag || !stash) return fail(CF_ERR_INVALID, "cf_gru_train_forward: null argument");
    if (y_drop_frag && !(keep_prob > 0.f && keep_prob < 1.f)) return fail(CF_ERR_INVALID, "cf_gru_train_forward_dropout: keep_prob must be in (0, 1)");
    f32x4* yd = reinterpret_cast<f32x4*>(y_drop_frag);
    const cf_dropout drop = make_dropout(y_drop_frag ? keep_prob : 1.f, seed, layer, step_count);
    if (n_windows <= 0) return fail(CF_ERR_INVALID, "cf_gru_train_forward: n_windows must be positive");
    int rc = train_cin_ok(m, cin);
    if (rc != CF_OK) return rc;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    const cf_knobs k = cf_read_knobs();
    return cf_with<32, 128>(cin, [&](auto C) {
        constexpr int CIN = decltype(C)::value;
        const cf_train_gru_plan p = cf_train_gru_plan_for(false, n_tiles, m->n_cu, CIN, k_gru_pack_bytes<CIN>, k_gru_x_bytes<CIN>, m->xp_tiles, k);
        const f32x4 *x4 = reinterpret_cast<const f32x4*>(x_frag);
        f32x4 *y4 = reinterpret_cast<f32x4*>(y_frag), *st4 = reinterpret_cast<f32x4*>(stash);
        if (p.coop) {
            if (p.hoist) launch_xproj<CIN>(m, p.xproj, wpack, x_frag, n_tiles, s);
            hipLaunchKernelGGL((gru_train_fwd_coop_kernel<CIN>), dim3(p.gx, 2), dim3(p.waves * 64), p.lds_bytes, s, wpack, x4, y4, st4, n_tiles,
                               p.hoist ? reinterpret_cast<const f32x4*>(m->d_xp) : nullptr, yd, drop);
        } else {
            hipLaunchKernelGGL((gru_train_fwd_kernel<CIN>), dim3(p.gx, 2), dim3(p.waves * 64), p.lds_bytes, s, wpack, x4, y4, st4, n_tiles, yd, drop);
        }
        HIP_TRY(hipGetLastError());
        return CF_OK;
    });
}

extern "C" int cf_gru_train_forward(cf_model* m, int32_t cin, const float* wpack, const float* x_frag, float* y_frag, float* stash,
                                    int64_t n_windows, void* stream) {
    return cf_gru_train_forward_dropout(m, cin, wpack, x_frag, y_frag, stash, n_windows, nullptr, 1.f, 0u, 0, nullptr, stream);
}

// ---- training: biGRU forward / backward (cf_train_gru_plan_for) -------------------------------------------------------------------
static void optin_gru_train(cf_optin& o) {
    for (int cin : {32, 128})
        cf_with<32, 128>(cin, [&](auto C) {
            constexpr int CIN = decltype(C)::value, BWD = gtb_pack_floats(CIN) * 4;
            o((const void*)gru_train_fwd_coop_kernel<CIN>, cf_train_coop_lds(false, k_gru_pack_bytes<CIN>));
            o((const void*)gru_train_bwd_coop_kernel<CIN>, cf_train_coop_lds(true, BWD));
            o((const void*)gru_train_fwd_kernel<CIN>, k_gru_pack_bytes<CIN>);
            o((const void*)gru_train_bwd_kernel<CIN>, BWD);
            return CF_OK;
        });
}

extern "C" int cf_gru_train_backward_dropout(cf_model* m, int32_t cin, const float* wpack_bwd, const float* y_frag, const float* stash,
                                             const float* dy_frag, const float* dy2_frag, const float* dy_scale, float* dx_frag, float* da,
                                             int64_t n_windows, float keep_prob, uint32_t seed, int32_t layer, const double* step_count,
                                             void* stream) {
    const cf_dropout drop = make_dropout((keep_prob > 0.f && keep_prob < 1.f) ? keep_prob : 1.f, seed, layer, step_count);
    if (!m || !wpack_bwd || !y_frag || !stash || !dy_frag || !dx_frag || !da)
        return fail(CF_ERR_INVALID, "cf_gru_train_backward: null argument");
    if (n_windows <= 0) return fail(CF_ERR_INVALID, "cf_gru_train_backward: n_windows must be positive");
    int rc = train_cin_ok(m, cin);
    if (rc != CF_OK) return rc;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    const cf_knobs k = cf_read_knobs();
    return cf_with<32, 128>(cin, [&](auto C) {
        constexpr int CIN = decltype(C)::value;
        const cf_train_gru_plan p = cf_train_gru_plan_for(true, n_tiles, m->n_cu, CIN, gtb_pack_floats(CIN) * 4, 0, m->xp_tiles, k);
        const f32x4 *y4 = reinterpret_cast<const f32x4*>(y_frag), *st4 = reinterpret_cast<const f32x4*>(stash), *dy4 = reinterpret_cast<const f32x4*>(dy_frag),
                    *dy24 = reinterpret_cast<const f32x4*>(dy2_frag), *sc4 = reinterpret_cast<const f32x4*>(dy_scale);
        f32x4 *dx4 = reinterpret_cast<f32x4*>(dx_frag), *da4 = reinterpret_cast<f32x4*>(da);
        if (p.coop) {
            hipLaunchKernelGGL((gru_train_bwd_coop_kernel<CIN>), dim3(p.gx, 2), dim3(p.waves * 64), p.lds_bytes, s, wpack_bwd, y4, st4, dy4, dy24, sc4,
                               dx4, da4, n_tiles, p.hoist, drop);
            if (p.hoist)         // few tiles: dx is formed afterwards on the idle CUs
                hipLaunchKernelGGL((gru_dx_kernel<CIN>), dim3(p.dx_grid_x, 2), dim3(256), 0, s, wpack_bwd, da4, dx4, n_tiles, p.dx_chunks);
        } else {
            hipLaunchKernelGGL((gru_train_bwd_kernel<CIN>), dim3(p.gx, 2), dim3(p.waves * 64), p.lds_bytes, s, wpack_bwd, y4, st4, dy4, dy24, sc4, dx4,
                               da4, n_tiles, drop);
        }
        HIP_TRY(hipGetLastError());
        return CF_OK;
    });
}

extern "C" int cf_gru_train_backward(cf_model* m, int32_t cin, const float* wpack_bwd, const float* y_frag, const float* stash,
                                     const float* dy_frag, const float* dy2_frag, const float* dy_scale, float* dx_frag, float* da,
                                     int64_t n_windows, void* stream) {
    return cf_gru_train_backward_dropout(m, cin, wpack_bwd, y_frag, stash, dy_frag, dy2_frag, dy_scale, dx_frag, da, n_windows, 1.f, 0u, 0,
                                         nullptr, stream);
}

// ---- any-size biGRU layer for training (generic.hpp): forward with gate stash, backward chain -----------------------------------
#include "anysize_launch.hpp"      // waves, grid, LDS bytes and h_via_y of the two launches below: host-only, tested on the CPU

static int anysize_args_ok(const cf_model* m, int32_t layer_size, int64_t n_windows, const char* who) {
    if (!m) return fail(CF_ERR_INVALID, std::string(who) + ": null model");
    if (layer_size < 16 || layer_size > 256 || (layer_size % 16) != 0)
        return fail(CF_ERR_INVALID, std::string(who) + ": layer_size must be a multiple of 16 between 16 and 256");
    if (n_windows <= 0 || (n_windows % CF_TILE) != 0) return fail(CF_ERR_INVALID, std::string(who) + ": n_windows must be a positive multiple of 16");
    return CF_OK;
}

template <bool X3>
static int anysize_train_forward(cf_model* m, int32_t layer_size, int32_t cin_blocks, const float* wpack, const float* bpack, const float* x_frag,
                                 float* y_frag, float* stash, int64_t n_windows, void* stream, const char* who) {
    int rc = anysize_args_ok(m, layer_size, n_windows, who);
    if (rc != CF_OK) return rc;
    if (!wpack || !bpack || !x_frag || !y_frag || !stash) return fail(CF_ERR_INVALID, std::string(who) + ": null buffer");
    if (cin_blocks < 1 || cin_blocks > 32) return fail(CF_ERR_INVALID, std::string(who) + ": cin_blocks must be 1..32 (input features / 16)");
    HIP_TRY(hipSetDevice(m->device));
    const int h16 = layer_size / 16, n_tiles = (int)(n_windows / CF_TILE);
    const cf_anysize_shape sh = cf_anysize_forward_shape(h16, n_tiles, m->n_cu);        // the state in LDS is fp32 in both precisions
    HIP_TRY(hipFuncSetAttribute((const void*)gen_gru_kernel<true, X3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((gen_gru_kernel<true, X3>), dim3((unsigned)sh.grid_x, 2), dim3(sh.waves * 64), sh.lds_bytes,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f32x4*>(wpack), reinterpret_cast<const f32x4*>(bpack),
                       reinterpret_cast<const f32x4*>(x_frag), reinterpret_cast<f32x4*>(y_frag), h16, (int)cin_blocks, sh.h_via_y,
                       reinterpret_cast<f32x4*>(stash), n_tiles);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

template <bool X3>
static int anysize_train_backward(cf_model* m, int32_t layer_size, const float* wtpack, const float* y_frag, const float* stash,
                                  const float* dy_frag, float* da, int64_t n_windows, void* stream, const char* who) {
    int rc = anysize_args_ok(m, layer_size, n_windows, who);
    if (rc != CF_OK) return rc;
    if (!wtpack || !y_frag || !stash || !dy_frag || !da) return fail(CF_ERR_INVALID, std::string(who) + ": null buffer");
    HIP_TRY(hipSetDevice(m->device));
    const int h16 = layer_size / 16, n_tiles = (int)(n_windows / CF_TILE);
    const cf_anysize_shape sh = cf_anysize_backward_shape(h16, n_tiles, m->n_cu);
    HIP_TRY(hipFuncSetAttribute((const void*)gen_gru_bwd_kernel<X3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(gen_gru_bwd_kernel<X3>, dim3((unsigned)sh.grid_x, 2), dim3(sh.waves * 64), sh.lds_bytes,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f32x4*>(wtpack), reinterpret_cast<const f32x4*>(y_frag),
                       reinterpret_cast<const f32x4*>(stash), reinterpret_cast<const f32x4*>(dy_frag), reinterpret_cast<f32x4*>(da), n_tiles, h16);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gru_anysize_train_forward(cf_model* m, int32_t layer_size, int32_t cin_blocks, const float* wpack, const float* bpack,
                                            const float* x_frag, float* y_frag, float* stash, int64_t n_windows, void* stream) {
    return anysize_train_forward<false>(m, layer_size, cin_blocks, wpack, bpack, x_frag, y_frag, stash, n_windows, stream,
                                        "cf_gru_anysize_train_forward");
}

extern "C" int cf_gru_anysize_train_backward(cf_model* m, int32_t layer_size, const float* wtpack, const float* y_frag, const float* stash,
                                             const float* dy_frag, float* da, int64_t n_windows, void* stream) {
    return anysize_train_backward<false>(m, layer_size, wtpack, y_frag, stash, dy_frag, da, n_windows, stream, "cf_gru_anysize_train_backward");
}

// ---- training precision "bf16x3": the same two launches on bf16x3 packs (gen_gru_kernel<true, true>, gen_gru_bwd_kernel<true>) ----
extern "C" int cf_gru_anysize_train_forward_x3(cf_model* m, int32_t layer_size, int32_t cin_blocks, const float* wpack_x3, const float* bpack,
                                               const float* x_frag, float* y_frag, float* stash, int64_t n_windows, void* stream) {
    return anysize_train_forward<true>(m, layer_size, cin_blocks, wpack_x3, bpack, x_frag, y_frag, stash, n_windows, stream,
                                       "cf_gru_anysize_train_forward_x3");
}

extern "C" int cf_gru_anysize_train_backward_x3(cf_model* m, int32_t layer_size, const float* wtpack_x3, const float* y_frag, const float* stash,
                                                const float* dy_frag, float* da, int64_t n_windows, void* stream) {
    return anysize_train_backward<true>(m, layer_size, wtpack_x3, y_frag, stash, dy_frag, da, n_windows, stream,
                                        "cf_gru_anysize_train_backward_x3");
}

static bool anysize_x3_sizes_ok(int32_t layer_size, int32_t cin_blocks) {
    return layer_size >= 16 && layer_size <= 256 && (layer_size % 16) == 0 && cin_blocks >= 1 && cin_blocks <= 32;
}

extern "C" int cf_gru_anysize_x3_pack_floats(int32_t layer_size, int32_t cin_blocks, int64_t out[2]) {
    if (!out) return fail(CF_ERR_INVALID, "cf_gru_anysize_x3_pack_floats: null output");
    if (!anysize_x3_sizes_ok(layer_size, cin_blocks))
        return fail(CF_ERR_INVALID, "cf_gru_anysize_x3_pack_floats: layer_size must be a multiple of 16 between 16 and 256, cin_blocks 1..32");
    const int64_t h16 = layer_size / 16;
    out[0] = 2 * 3 * h16 * (gen_x3_pad(cin_blocks) + gen_x3_pad((int)h16)) * 256;
    out[1] = 2 * h16 * (gen_x3_pad((int)h16) + gen_x3_pad(2 * (int)h16)) * 256;
    return CF_OK;
}

extern "C" int cf_gen_repack_x3(cf_model* m, int32_t layer_size, int32_t cin_blocks, int32_t transposed, const float* pack, float* pack_x3,
                                void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_gen_repack_x3: null model");
    if (!pack || !pack_x3) return fail(CF_ERR_INVALID, "cf_gen_repack_x3: null buffer");
    if (!anysize_x3_sizes_ok(layer_size, transposed ? 1 : cin_blocks))
        return fail(CF_ERR_INVALID, "cf_gen_repack_x3: layer_size must be a multiple of 16 between 16 and 256, cin_blocks 1..32");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int h16 = layer_size / 16;
    auto launch = [&](const float* src, float* dst, int dirs, int rows, int k0, int k1, int64_t src_stride, int64_t dst_stride) {
        const int64_t threads = (int64_t)rows * ((gen_x3_pad(k0) + gen_x3_pad(k1)) / 2) * 64;
        hipLaunchKernelGGL(gen_repack_x3_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)dirs), dim3(256), 0, s,
                           reinterpret_cast<const f32x4*>(src), reinterpret_cast<f32x4*>(dst), rows, k0, k1, src_stride, dst_stride);
    };
    if (!transposed) {                                       // [2][3][H16] rows of [x: cin_blocks | h: H16]
        launch(pack, pack_x3, 1, 6 * h16, cin_blocks, h16, 0, 0);
    } else {                                                 // per direction Wc_h^T: H16 rows of [H16], then Wg_h^T: H16 rows of [2 H16]
        const int kc = gen_x3_pad(h16), kg = gen_x3_pad(2 * h16);
        const int64_t ss = (int64_t)3 * h16 * h16 * 64, ds = (int64_t)h16 * (kc + kg) * 64;      // f32x4 per direction
        launch(pack, pack_x3, 2, h16, h16, 0, ss, ds);
        HIP_TRY(hipGetLastError());
        launch(pack + (int64_t)h16 * h16 * 256, pack_x3 + (int64_t)h16 * kc * 256, 2, h16, 2 * h16, 0, ss, ds);
    }
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

// The launch shape of the two calls above for `n_windows` windows on this model's device, for tests and tools: out = forward
// {waves, grid_x, lds_bytes, h_via_y}, backward {waves, grid_x, lds_bytes, max_waves}.  Nothing is launched.
extern "C" int cf_gru_anysize_train_shape(const cf_model* m, int32_t layer_size, int64_t n_windows, int64_t out[8]) {
    int rc = anysize_args_ok(m, layer_size, n_windows, "cf_gru_anysize_train_shape");
    if (rc != CF_OK) return rc;
    if (!out) return fail(CF_ERR_INVALID, "cf_gru_anysize_train_shape: null output");
    const int h16 = layer_size / 16, n_tiles = (int)(n_windows / CF_TILE);
    const cf_anysize_shape f = cf_anysize_forward_shape(h16, n_tiles, m->n_cu), b = cf_anysize_backward_shape(h16, n_tiles, m->n_cu);
    out[0] = f.waves; out[1] = f.grid_x; out[2] = (int64_t)f.lds_bytes; out[3] = f.h_via_y;
    out[4] = b.waves; out[5] = b.grid_x; out[6] = (int64_t)b.lds_bytes; out[7] = b.max_waves;
    return CF_OK;
}

// The launch shape of every biGRU layer of an any-size model in one pass of `n_windows` windows (what gen_run_pass takes from
// csrc/anysize_infer_launch.hpp), for tests and tools: out = one row per layer of {kernel (0 tuned LDS-resident, 1 one tile per
// wave, 2 two tiles per wave), waves per workgroup, grid x, dynamic LDS bytes, h_via_y}.  Nothing is launched.
extern "C" int cf_anysize_infer_shape(const cf_model* m, int64_t n_windows, int64_t* out, int64_t capacity) {
    if (!m || !out) return fail(CF_ERR_INVALID, "cf_anysize_infer_shape: null argument");
    if (!m->gen) return fail(CF_ERR_INVALID, "cf_anysize_infer_shape: the model is not on the any-size path");
    if (n_windows <= 0 || n_windows > m->cap_windows)
        return fail(CF_ERR_INVALID, "cf_anysize_infer_shape: n_windows must be between 1 and the model's windows per pass");
    const cf_generic* g = m->gen;
    if (capacity < (int64_t)g->layers.size()) return fail(CF_ERR_INVALID, "cf_anysize_infer_shape: out needs one row of 5 values per biGRU layer");
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    for (size_t l = 0; l < g->layers.size(); ++l) {
        const cf_generic::Layer& L = g->layers[l];
        const cf_anysize_infer_launch sh = cf_anysize_infer_shape_for(g->cls, L.tuned != nullptr, L.kbx, n_tiles, m->n_cu);
        int64_t* row = out + 5 * l;
        row[0] = sh.kernel; row[1] = sh.waves; row[2] = sh.grid_x; row[3] = (int64_t)sh.lds_bytes; row[4] = sh.h_via_y;
    }
    return CF_OK;
}

__global__ __launch_bounds__(256) void dropout_scale_kernel(f32x4* __restrict__ out, int64_t n4, cf_dropout drop) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) out[i] = cf_drop_scale4(cf_drop_key(drop), drop.keep_prob, i);
}

// The mask / keep_prob tensor the training kernels apply to the output of `layer` (fragment layout [tiles][35][8][64][4]), written out
// for tests and tools: the kernels themselves never store it.
extern "C" int cf_dropout_scale(cf_model* m, float keep_prob, uint32_t seed, int32_t layer, const double* step_count, int64_t n_windows,
                                float* scale_frag, void* stream) {
    if (!m || !scale_frag) return fail(CF_ERR_INVALID, "cf_dropout_scale: null argument");
    if (!(keep_prob > 0.f && keep_prob < 1.f) || n_windows <= 0) return fail(CF_ERR_INVALID, "cf_dropout_scale: keep_prob must be in (0, 1), n_windows > 0");
    HIP_TRY(hipSetDevice(m->device));
    const int64_t n4 = ((n_windows + CF_TILE - 1) / CF_TILE) * CF_T * 8 * 64;
    hipLaunchKernelGGL(dropout_scale_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<f32x4*>(scale_frag), n4, make_dropout(keep_prob, seed, layer, step_count));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int64_t cf_gru_wgrad_workspace_floats(cf_model* m, int32_t cin, int64_t n_windows) {
    if (!m || (cin != CF_C && cin != 2 * CF_H) || n_windows <= 0) return 0;
    return cf_wgrad_plan_for((int)((n_windows + CF_TILE - 1) / CF_TILE), m->n_cu, gwg_partial_floats(cin)).workspace_floats;
}

extern "C" int cf_gru_train_wgrad(cf_model* m, int32_t cin, const float* x_frag, const float* y_frag, const float* stash,
                                  const float* da, int64_t n_windows, float* workspace, int64_t workspace_floats, float* grads,
                                  void* stream) {
    if (!m || !x_frag || !y_frag || !stash || !da || !workspace || !grads)
        return fail(CF_ERR_INVALID, "cf_gru_train_wgrad: null argument");
    if (n_windows <= 0) return fail(CF_ERR_INVALID, "cf_gru_train_wgrad: n_windows must be positive");
    int rc = train_cin_ok(m, cin);
    if (rc != CF_OK) return rc;
    if (workspace_floats < cf_gru_wgrad_workspace_floats(m, cin, n_windows))
        return fail(CF_ERR_INVALID, "cf_gru_train_wgrad: workspace too small (see cf_gru_wgrad_workspace_floats)");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    const cf_wgrad_plan p = cf_wgrad_plan_for(n_tiles, m->n_cu, gwg_partial_floats(cin));
    rc = cf_with<32, 128>(cin, [&](auto C) {
        hipLaunchKernelGGL((gru_wgrad_kernel<decltype(C)::value>), dim3(p.n_chunks, 2), dim3(CF_WGRAD_WAVES * 64), 0, s,
                           reinterpret_cast<const f32x4*>(x_frag), reinterpret_cast<const f32x4*>(y_frag), reinterpret_cast<const f32x4*>(stash),
                           reinterpret_cast<const f32x4*>(da), workspace, n_tiles, p.pairs_per_wg);
        return CF_OK;
    });
    if (rc != CF_OK) return rc;
    HIP_TRY(hipGetLastError());
    const int per = gwg_partial_floats(cin);
    hipLaunchKernelGGL(gru_wgrad_reduce_kernel, dim3((per + 63) / 64, 2), dim3(256), 0, s, workspace, grads, gwg_rows(cin), p.n_chunks);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

// ---- residual conv stack, training ---------------------------------------------------------
static int res_train_ok(const cf_model* m, int n_blocks) {
    if (n_blocks < 1 || 4 * n_blocks > RT_MAX_UNITS) return fail(CF_ERR_INVALID, "residual training kernels: 1..4 blocks");
    if (m->hp.layer_size_res != CF_C) return fail(CF_ERR_INVALID, "residual training kernels: 32 conv channels only");
    if (m->gen) return fail(CF_ERR_INVALID, "residual training kernels need a model on the tuned path (unset CATFISH_GENERIC)");
    return CF_OK;
}

extern "C" int64_t cf_res_train_param_floats(int32_t n_blocks) {
    if (n_blocks < 1 || 4 * n_blocks > RT_MAX_UNITS) return 0;
    return rt_make_layout(n_blocks).off[4 * n_blocks];
}

extern "C" int64_t cf_res_train_workspace_floats(int32_t n_blocks, int64_t n_windows) {
    if (n_blocks < 1 || 4 * n_blocks > RT_MAX_UNITS || n_windows <= 0) return 0;
    const int win = rt_win_for(n_windows);
    return ((n_windows + win - 1) / win) * (int64_t)rt_make_layout(n_blocks).off[4 * n_blocks];
}

extern "C" int cf_res_train_forward(cf_model* m, int32_t n_blocks, const float* params, const float* x, float* z_stash, float* out,
                                    int64_t n_windows, void* stream) {
    if (!m || !params || !x || !z_stash || !out) return fail(CF_ERR_INVALID, "cf_res_train_forward: null argument");
    if (n_windows <= 0) return fail(CF_ERR_INVALID, "cf_res_train_forward: n_windows must be positive");
    int rc = res_train_ok(m, n_blocks);
    if (rc != CF_OK) return rc;
    HIP_TRY(hipSetDevice(m->device));
    const int win = rt_win_for(n_windows);
    const int n_wg = (int)((n_windows + win - 1) / win);
    hipLaunchKernelGGL(res_train_fwd_kernel, dim3(n_wg), dim3(RT_THREADS), RT_FWD_LDS_BYTES, reinterpret_cast<hipStream_t>(stream), x, params,
                       z_stash, out, rt_make_layout(n_blocks), (int)n_windows, n_blocks, m->hp.bn_epsilon, win);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_res_train_backward(cf_model* m, int32_t n_blocks, const float* params, const float* x, const float* z_stash,
                                     const float* d_out, float* workspace, int64_t workspace_floats, float* grads, int64_t n_windows,
                                     void* stream) {
    if (!m || !params || !x || !z_stash || !d_out || !workspace || !grads) return fail(CF_ERR_INVALID, "cf_res_train_backward: null argument");
    if (n_windows <= 0) return fail(CF_ERR_INVALID, "cf_res_train_backward: n_windows must be positive");
    int rc = res_train_ok(m, n_blocks);
    if (rc != CF_OK) return rc;
    if (workspace_floats < cf_res_train_workspace_floats(n_blocks, n_windows))
        return fail(CF_ERR_INVALID, "cf_res_train_backward: workspace too small (see cf_res_train_workspace_floats)");
    HIP_TRY(hipSetDevice(m->device));
    const int lds_bytes = RT_BWD_LDS_BYTES;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const rt_layout L = rt_make_layout(n_blocks);
    const int win = rt_win_for(n_windows);
    const int n_wg = (int)((n_windows + win - 1) / win);
    hipLaunchKernelGGL(res_train_bwd_kernel, dim3(n_wg), dim3(RT_THREADS), lds_bytes, s, x, params, z_stash, d_out, workspace, L,
                       (int)n_windows, n_blocks, m->hp.bn_epsilon, win);
    HIP_TRY(hipGetLastError());
    const int nf = L.off[4 * n_blocks];
    hipLaunchKernelGGL(res_train_reduce_kernel, dim3((nf + 63) / 64), dim3(256), 0, s, workspace, grads, nf, n_wg);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

static hipError_t cf_optin_all() {
    cf_optin o;
    optin_gru_layer(o);
    optin_gru_bf16(o);
    optin_res(o);
    optin_gru_train(o);
    o((const void*)res_train_fwd_kernel, RT_FWD_LDS_BYTES);
    o((const void*)res_train_bwd_kernel, RT_BWD_LDS_BYTES);
    return o.e;
}

// ---- dense head + loss, optimizer (training) ------------------------------------------------
extern "C" int64_t cf_train_head_workspace_floats(cf_model* m, int64_t n_windows) {
    if (!m || n_windows <= 0) return 0;
    return cf_train_head_plan_for((n_windows + CF_TILE - 1) / CF_TILE, m->n_cu, CF_HEAD_PART).workspace_floats;
}

extern "C" int cf_train_head(cf_model* m, const float* y_frag, const float* dense_kernel, const float* dense_bias, const float* labels,
                             int64_t n_windows, float* dy_frag, float* logits, float* workspace, int64_t workspace_floats, float* grads,
                             float* loss, void* stream) {
    if (!m || !y_frag || !dense_kernel || !dense_bias || !labels || !dy_frag || !workspace || !grads || !loss)
        return fail(CF_ERR_INVALID, "cf_train_head: null argument");
    if (n_windows <= 0) return fail(CF_ERR_INVALID, "cf_train_head: n_windows must be positive");
    if (m->hp.layer_size != CF_H) return fail(CF_ERR_INVALID, "cf_train_head: layer_size 64 only");
    if (workspace_floats < cf_train_head_workspace_floats(m, n_windows))
        return fail(CF_ERR_INVALID, "cf_train_head: workspace too small (see cf_train_head_workspace_floats)");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_tiles = (int)((n_windows + CF_TILE - 1) / CF_TILE);
    const cf_train_head_plan p = cf_train_head_plan_for(n_tiles, m->n_cu, CF_HEAD_PART);
    const float inv_count = (float)(1.0 / ((double)n_windows * CF_T));
    hipLaunchKernelGGL(train_head_kernel, dim3(p.grid), dim3(256), 0, s, reinterpret_cast<const f32x4*>(y_frag), dense_kernel, dense_bias,
                       labels, reinterpret_cast<f32x4*>(dy_frag), logits, workspace, n_windows, n_tiles, inv_count);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(train_head_reduce_kernel, dim3(3), dim3(256), 0, s, workspace, p.waves, grads, loss, inv_count);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_opt_step(cf_model* m, int32_t kind, float* params, const float* grads, float* slot1, float* slot2, int64_t n, float lr,
                           double* step_count, const int32_t* pack_idx, const float* pack_scale, float* packed, int64_t n_packed,
                           void* stream) {
    if (!m || !params || !grads || !slot1 || !slot2 || !step_count) return fail(CF_ERR_INVALID, "cf_opt_step: null argument");
    if (kind != 0 && kind != 1) return fail(CF_ERR_INVALID, "cf_opt_step: kind must be 0 (RMSProp) or 1 (Adam)");
    if (n <= 0 || n_packed < 0) return fail(CF_ERR_INVALID, "cf_opt_step: bad size");
    if (n_packed > 0 && (!pack_idx || !pack_scale || !packed)) return fail(CF_ERR_INVALID, "cf_opt_step: null packing argument");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(opt_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (int)kind, params, grads, slot1, slot2, n, lr,
                       step_count);
    HIP_TRY(hipGetLastError());
    // the re-tiling launch also advances the step counter (it runs after every block of the update has read it)
    const int64_t ng = std::max<int64_t>(n_packed, 1);
    hipLaunchKernelGGL(gather_scale_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, params, pack_idx, pack_scale, packed, n_packed,
                       step_count);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

// ---- global-norm clipping + non-finite-step guard (include/catfish_hip_ext.h; kernels in train_step.hpp) ----
extern "C" int cf_ext_abi_version(void) { return CF_EXT_ABI_VERSION; }

extern "C" int64_t cf_clip_workspace_doubles(int64_t n) { return n <= 0 ? 0 : (n + CF_CLIP_CHUNK - 1) / CF_CLIP_CHUNK; }

extern "C" int cf_clip_norm(cf_model* m, const float* grads, int64_t n, double clip_norm, int32_t flags, const float* loss,
                            double* workspace, int64_t workspace_doubles, double* record, void* stream) {
    if (!m || !grads || !workspace || !record) return fail(CF_ERR_INVALID, "cf_clip_norm: null argument");
    if (n <= 0) return fail(CF_ERR_INVALID, "cf_clip_norm: bad size");
    if (reinterpret_cast<uintptr_t>(grads) % 16) return fail(CF_ERR_INVALID, "cf_clip_norm: grads must be 16-byte aligned");
    if (flags <= 0 || (flags & ~(CF_CLIP_SCALE | CF_CLIP_SKIP_NONFINITE)))
        return fail(CF_ERR_INVALID, "cf_clip_norm: flags must be CF_CLIP_SCALE and / or CF_CLIP_SKIP_NONFINITE");
    if ((flags & CF_CLIP_SCALE) && !(std::isfinite(clip_norm) && clip_norm > 0.0))
        return fail(CF_ERR_INVALID, "cf_clip_norm: clip_norm must be a finite positive number");
    const int64_t n_parts = cf_clip_workspace_doubles(n);
    if (workspace_doubles < n_parts) return fail(CF_ERR_INVALID, "cf_clip_norm: workspace too small (see cf_clip_workspace_doubles)");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_sq_partial_kernel, dim3((unsigned)n_parts), dim3(256), 0, s, grads, n, workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, workspace, n_parts, clip_norm, (int)flags, loss, record);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_opt_step_guarded(cf_model* m, int32_t kind, float* params, const float* grads, float* slot1, float* slot2, int64_t n,
                                   float lr, double* step_count, const int32_t* pack_idx, const float* pack_scale, float* packed,
                                   int64_t n_packed, const double* record, void* stream) {
    if (!m || !params || !grads || !slot1 || !slot2 || !step_count || !record)
        return fail(CF_ERR_INVALID, "cf_opt_step_guarded: null argument");
    if (kind != 0 && kind != 1) return fail(CF_ERR_INVALID, "cf_opt_step_guarded: kind must be 0 (RMSProp) or 1 (Adam)");
    if (n <= 0 || n_packed < 0) return fail(CF_ERR_INVALID, "cf_opt_step_guarded: bad size");
    if (n_packed > 0 && (!pack_idx || !pack_scale || !packed)) return fail(CF_ERR_INVALID, "cf_opt_step_guarded: null packing argument");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(opt_step_guarded_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (int)kind, params, grads, slot1, slot2, n,
                       lr, step_count, record);
    HIP_TRY(hipGetLastError());
    const int64_t ng = std::max<int64_t>(n_packed, 1);
    hipLaunchKernelGGL(gather_scale_guarded_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, params, pack_idx, pack_scale, packed,
                       n_packed, step_count, record);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

#include "gen_train.hpp"      // whole-step training of any geometry (conv stack, GRU dx / dW, dropout, head)
#include "sample_batch.hpp"   // device-resident training set: cf_sample_batch draws and gathers a training step's next batch on the card
#include "validation.hpp"     // device-resident validation set: cf_validation_gather packs a round's stretches, cf_validation_score scores them
#include "validation_runs.hpp" // ... and cf_validation_run_states counts the homopolymers found: run states per threshold and length bin
#include "validation_borders.hpp" // ... cf_validation_run_borders the rest of check_hp: how far called borders miss, and the interruptions
#include "validation_bases.hpp" // ... cf_validation_run_bases the same runs by base and by length in bases, read from the set's base map
#include "validation_curve.hpp" // ... and cf_validation_curve bins the probabilities at every threshold step: whole ROC / PR curves and AUC
#include "validation_scores.hpp" // ... and cf_validation_run_scores the probabilities under the runs of every state: what the misses scored
#include "tilings.hpp"          // shifted-window voting: cf_retile_windows lays out K tilings of a batch, cf_vote_tilings merges their results
#include "label_events.hpp"     // labels from event tables: cf_label_events classifies a batch's events and expands them to per-sample labels
#include "label_moves.hpp"      // labels from a basecaller's move table: cf_label_moves merges stays into their heads, then classifies and expands
#include "base_votes.hpp"       // per-base calls: cf_base_votes lets every base's samples vote on it and scores the voted bases by base

// ---- profiling ---------------------------------------------------------------------------
static int prof_collect(cf_model* m) {
    for (auto& ev : m->ev_pending) {
        HIP_TRY(hipEventSynchronize(ev.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        m->prof_ms[ev.slot] += ms;
        m->prof_n[ev.slot] += 1;
        m->ev_pool.push_back(ev.a);
        m->ev_pool.push_back(ev.b);
    }
    m->ev_pending.clear();
    return CF_OK;
}
extern "C" int cf_profile_enable(cf_model* m, int on) {
    if (!m) return fail(CF_ERR_INVALID, "null model");
    if (!on && m->prof_every) { int rc = prof_collect(m); if (rc != CF_OK) return rc; }
    m->prof_every = on < 0 ? 0 : on;
    m->prof = on != 0;
    m->prof_calls = 0;
    return CF_OK;
}
extern "C" int cf_profile_reset(cf_model* m) {
    if (!m) return fail(CF_ERR_INVALID, "null model");
    int rc = prof_collect(m);
    if (rc != CF_OK) return rc;
    for (int i = 0; i < CF_PROF_SLOTS; ++i) { m->prof_ms[i] = 0; m->prof_n[i] = 0; }
    return CF_OK;
}
extern "C" int cf_profile_read(cf_model* m, double ms[CF_PROF_SLOTS], int64_t launches[CF_PROF_SLOTS]) {
    if (!m || !ms || !launches) return fail(CF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    int rc = prof_collect(m);
    if (rc != CF_OK) return rc;
    for (int i = 0; i < CF_PROF_SLOTS; ++i) { ms[i] = m->prof_ms[i]; launches[i] = m->prof_n[i]; }
    return CF_OK;
}
extern "C" const char* cf_profile_slot_name(int slot) {
    return (slot >= 0 && slot < CF_PROF_SLOTS) ? k_slot_names[slot] : "";
}

// ---- debug hook --------------------------------------------------------------------------
#include "bf16_stage.hpp"   // the bf16 / bf16x3 activation layout, decoded on the host
constexpr bool cf_bf16_stage_layout_agrees() {
    for (int kb = 0; kb < 8; ++kb)
        for (int hh = 0; hh < 2; ++hh)
            for (int j = 0; j < 8; ++j)
                if (cf_bf16_frag_feature(kb, hh, j) != frag_feature32(kb, hh, j)) return false;
    return true;
}
static_assert(cf_bf16_stage_layout_agrees(), "bf16_stage.hpp decodes the layout the bf16 kernels write");

extern "C" int cf_debug_stage(cf_model* m, int stage, int64_t n_windows, float* out_host) {
    if (!m || !out_host) return fail(CF_ERR_INVALID, "cf_debug_stage: null argument");
    if (m->gen) return fail(CF_ERR_INVALID, "cf_debug_stage: not available on the any-size path");
    const cf_model::Slot& sl = m->slots[0];
    if (n_windows <= 0 || (stage != 100 && n_windows > sl.last_windows)) return fail(CF_ERR_INVALID, "cf_debug_stage: n_windows exceeds slot 0's last pass");
    HIP_TRY(hipSetDevice(m->device));
    if (stage == 100) {      // raw dense-partial buffer of slot 0 (diagnostic builds park their in-kernel stamps there)
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out_host, sl.d_p, (size_t)n_windows * sizeof(float), hipMemcpyDeviceToHost));
        return CF_OK;
    }
    int feats, mt;
    const float* src;
    if (stage >= 0 && stage < m->hp.n_layers_res) {
        // ping-pong: only the last two blocks survive a pass
        if (stage < m->hp.n_layers_res - 2) return fail(CF_ERR_INVALID, "cf_debug_stage: stage overwritten");
        if (stage == 0 && sl.last_res_fused)
            return fail(CF_ERR_INVALID, "cf_debug_stage: block 0's output is not materialised by the fused two-block launch (throughput mode)");
        feats = CF_C; mt = 2; src = sl.d_a[stage & 1];
    } else if (stage >= m->hp.n_layers_res && stage < m->hp.n_layers_res + m->hp.n_layers - 1) {
        const int l = stage - m->hp.n_layers_res;
        if (l < m->hp.n_layers - 3) return fail(CF_ERR_INVALID, "cf_debug_stage: stage overwritten");
        feats = 2 * CF_H; mt = 8; src = sl.d_y[l & 1];
    } else {
        return fail(CF_ERR_INVALID, "cf_debug_stage: no such stage");
    }
    if (m->np > 0) {         // bf16 / bf16x3: the same buffers in the layout of bf16_stage.hpp (np = 2: hi + lo)
        std::vector<uint16_t> frag16((size_t)cf_bf16_stage_elems(n_windows, CF_T, feats, m->np));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(frag16.data(), src, frag16.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
        cf_bf16_stage_decode(frag16.data(), n_windows, CF_T, feats, m->np, out_host);
        return CF_OK;
    }
    const int64_t n_tiles = (n_windows + CF_TILE - 1) / CF_TILE;
    std::vector<float> frag((size_t)n_tiles * CF_T * mt * 256);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(frag.data(), src, frag.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t w = 0; w < n_windows; ++w)
        for (int t = 0; t < CF_T; ++t)
            for (int f = 0; f < feats; ++f) {
                const int mo = f >> 4, qq = (f >> 2) & 3, r = f & 3;
                const int lane = qq * 16 + (int)(w & 15);
                out_host[(w * CF_T + t) * feats + f] = frag[((((w >> 4) * CF_T + t) * mt + mo) * 64 + lane) * 4 + r];
            }
    return CF_OK;
}

extern "C" int64_t cf_workspace_bytes(const cf_model* m) { return m ? m->ws_bytes : 0; }
extern "C" const char* cf_last_error(void) { return g_err.c_str(); }
#include "chunks_host.hpp"
#include "loader_host.hpp"
#include "split_host.hpp"

// Which card is HIP device `device` of this process (rank placement and the N > 1 bench line: catfish_amd/placement.py)
extern "C" int cf_device_identity(int device, char* pci_bus_id, int64_t bus_cap, char* uuid_hex, int64_t uuid_cap) {
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(CF_ERR_INVALID, "cf_device_identity: no such device");
    if (pci_bus_id) {
        if (bus_cap < 13) return fail(CF_ERR_INVALID, "cf_device_identity: pci_bus_id needs 13 bytes");
        HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, (int)std::min<int64_t>(bus_cap, 64), device));
    }
    if (uuid_hex) {
        if (uuid_cap < 33) return fail(CF_ERR_INVALID, "cf_device_identity: uuid_hex needs 33 bytes");
        hipUUID id;
        HIP_TRY(hipDeviceGetUuid(&id, device));
        static const char* hex = "0123456789abcdef";
        for (int i = 0; i < 16; ++i) {
            uuid_hex[2 * i] = hex[((unsigned char)id.bytes[i]) >> 4];
            uuid_hex[2 * i + 1] = hex[((unsigned char)id.bytes[i]) & 15];
        }
        uuid_hex[32] = 0;
    }
    return CF_OK;
}

extern "C" int cf_abi_version(void) { return CF_ABI_VERSION; }
extern "C" const char* cf_version(void) { return "catfish_hip 0.3 (gfx950; fp32 MFMA 16x16x4, bf16 / bf16x3 MFMA 32x32x16)"; }
