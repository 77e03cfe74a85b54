// Whole-step training of ANY geometry (layer_size 16..256, layer_size_res 16..256, any depth; the draws of
// networks/train_validate.py:66-111): the pieces around the any-size recurrences (cf_gru_anysize_train_forward / _backward) that
// the torch-autograd path (catfish_amd/anysize_train.py) left to torch.  Run-time sizes everywhere; every activation is a
// fragment-layout plane [tile][35][F/16][64][4] (element (window n, step t, feature f) at gt_fi), so the recurrences read and
// write them without a re-layout.
//
//   gt_conv_fwd      conv (k = 1 or 3, window-local SAME padding) + bias, stash z, BN(inference: moving stats constant) as an
//                    epilogue affine z s + t (s, t from gamma / beta / mean / var of the step), ReLU, shortcut + ReLU
//   gt_conv_dx       adjoint of that conv: flipped taps, transposed channel matrices (read from the TF kernel in place)
//   gt_gru_dx        biGRU input gradient  dx = sum_dir sum_gate da_gate W_{gate,x}^T  (a k = 1 "conv" from 6H features)
//   gt_wgrad         sum over positions of L(p, m) R(p, n) (conv dW + bias with a tap shift, GRU dW + bias with the +-1 step
//                    shift of h_prev, dense-head dW + bias): per-workgroup partials over fixed position chunks ...
//   gt_reduce        ... summed in chunk order into the flat gradient buffer (no atomics: a step is bit-reproducible)
//   gt_bn_bwd        ReLU / BN adjoints: dz = g [a > 0] [z s + t > 0] s, per-tile partials of d gamma, d beta
//   gt_dropout       y * mask / keep_prob with the tuned kernels' hash (cf_drop_scale4 of the f32x4 index of the output plane),
//                    or with an explicit factor tensor; the same launch scales the incoming gradient in the backward
//   gt_head          dense head + sigmoid cross-entropy per position (logit, d logit, d input, loss term), padding windows 0
//   gt_loss_reduce   mean loss, one workgroup, fixed order
//   gt_x_frag        the plain RNN's one input feature into a 16-feature fragment plane
//   gt_head_bwd      head backward from an upstream d probability (the operator's autograd: no labels, no loss)
//   gt_signal_grad   d loss / d signal from block 0's two cin-1 units (ResNetRNN) or layer 0's gate gradients (plain RNN)
//   gt_bn_stat_grads d moving_mean, d moving_variance from the unit's d gamma, d beta
//
// The GEMM-shaped kernels share one LDS-tiled core (64 x 64 outputs per workgroup, 4 x 4 per thread, k in steps of 16, fmaf in
// a fixed k order: exact fp32 products, the same sum on every run).  Included by catfish_hip.hip after cf_opt_step.
#pragma once

#define GT_BN_EPS 1e-3f             // tf.layers.batch_normalization default
#define GT_CHUNK_WINDOWS 32         // positions per weight-gradient partial: 32 windows x 35 steps

__device__ __forceinline__ int64_t gt_fi(int n, int t, int f, int F16) {
    return ((((int64_t)(n >> 4) * CF_T + t) * F16 + (f >> 4)) * 64 + (((f >> 2) & 3) * 16 + (n & 15))) * 4 + (f & 3);
}

// C[m][n] (+)= sum_{k in [k0, k1)} A(m, k) B(k, n) for the workgroup's 64 x 64 block; op.a / op.b return 0 outside the operands
template <class Op>
__device__ __forceinline__ void gt_tile(const Op& op, int M, int N, int k0, int k1, float (&acc)[4][4], int mb, int nb) {
    __shared__ float As[16][65], Bs[16][65];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kb = k0; kb < k1; kb += 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + 256 * e, kk = idx >> 6, mm = idx & 63;
            const int k = kb + kk, m = mb + mm, n = nb + mm;
            As[kk][mm] = (k < k1 && m < M) ? op.a(m, k) : 0.f;
            Bs[kk][mm] = (k < k1 && n < N) ? op.b(k, n) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = As[kk][ty + 16 * i]; bv[i] = Bs[kk][tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
}

// out = op.store(m, n, C[m][n]) over the whole K: grid (ceil(M / 64), ceil(N / 64))
template <class Op>
__global__ __launch_bounds__(256) void gt_gemm_kernel(Op op, int M, int N, int K) {
    float acc[4][4];
    const int mb = blockIdx.x * 64, nb = blockIdx.y * 64;
    gt_tile(op, M, N, 0, K, acc, mb, nb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = mb + ty + 16 * i, n = nb + tx + 16 * j;
            if (m < M && n < N) op.store(m, n, acc[i][j]);
        }
}

// partial[chunk][m * N + n] = sum over the chunk's positions: grid (ceil(M / 64), ceil(N / 64), chunks)
template <class Op>
__global__ __launch_bounds__(256) void gt_wgrad_kernel(Op op, int M, int N, int P, int chunk, float* __restrict__ part) {
    float acc[4][4];
    const int mb = blockIdx.x * 64, nb = blockIdx.y * 64;
    const int k0 = blockIdx.z * chunk, k1 = min(P, k0 + chunk);
    gt_tile(op, M, N, k0, k1, acc, mb, nb);
    float* dst = part + (int64_t)blockIdx.z * M * N;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = mb + ty + 16 * i, n = nb + tx + 16 * j;
            if (m < M && n < N) dst[(int64_t)m * N + n] = acc[i][j];
        }
}

__global__ __launch_bounds__(256) void gt_reduce_kernel(const float* __restrict__ part, int64_t len, int chunks, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * len + i];
    dst[i] = s;
}

// ---- operand maps (position p = 35 n + t; L / A read an activation plane, B / R the TF-layout parameters) -----------------------
struct GtIn {            // input of a conv: one feature as [n][35] (cin = 1) or a fragment plane
    const float* x;
    int cin, cin16;
    __device__ __forceinline__ float at(int n, int t, int c) const {
        return cin == 1 ? x[(int64_t)n * CF_T + t] : x[gt_fi(n, t, c, cin16)];
    }
};

struct GtConvFwd {
    GtIn in;
    const float* w;      // unit: kernel [kw][cin][cout] | bias | gamma | beta | moving_mean | moving_variance
    int kw, cout;
    const float* res;    // shortcut to add before the last ReLU (fragment, cout features) or null
    int relu;
    float* z;            // pre-BN stash
    float* y;
    __device__ __forceinline__ float a(int p, int k) const {
        const int n = p / CF_T, t = p - n * CF_T, tap = k / in.cin, c = k - tap * in.cin, tt = t + tap - (kw - 1) / 2;
        return (tt >= 0 && tt < CF_T) ? in.at(n, tt, c) : 0.f;
    }
    __device__ __forceinline__ float b(int k, int co) const { return w[(int64_t)k * cout + co]; }
    __device__ __forceinline__ void store(int p, int co, float acc) const {
        const float* prm = w + (int64_t)kw * in.cin * cout;
        const float zz = acc + prm[co];
        const float s = prm[cout + co] * rsqrtf(prm[4 * cout + co] + GT_BN_EPS);      // bias | gamma | beta | mean | var
        float v = fmaf(zz, s, prm[2 * cout + co] - prm[3 * cout + co] * s);
        if (relu) v = fmaxf(v, 0.f);
        const int n = p / CF_T, t = p - n * CF_T;
        const int64_t o = gt_fi(n, t, co, cout >> 4);
        if (res) v = fmaxf(v + res[o], 0.f);
        z[o] = zz;
        y[o] = v;
    }
};

struct GtConvDx {
    const float* dz;     // [.., cout]
    const float* w;
    int kw, cin, cout;
    const float* add;    // added to the result (the other branch's gradient) or null
    float* dx;           // [.., cin]
    __device__ __forceinline__ float a(int p, int k) const {
        const int n = p / CF_T, t = p - n * CF_T, tap = k / cout, co = k - tap * cout, tt = t - tap + (kw - 1) / 2;
        return (tt >= 0 && tt < CF_T) ? dz[gt_fi(n, tt, co, cout >> 4)] : 0.f;
    }
    __device__ __forceinline__ float b(int k, int ci) const {
        const int tap = k / cout, co = k - tap * cout;
        return w[((int64_t)tap * cin + ci) * cout + co];
    }
    __device__ __forceinline__ void store(int p, int ci, float acc) const {
        const int n = p / CF_T, t = p - n * CF_T;
        const int64_t o = gt_fi(n, t, ci, cin >> 4);
        dx[o] = add ? acc + add[o] : acc;
    }
};

struct GtGruDx {
    const float* da;     // [.., 6 H]: (dir, gate r / u / c, unit)
    const float* prm;    // layer: per direction gates kernel [cin + H][2H] | gates bias | candidate kernel [cin + H][H] | candidate bias
    int h, cin;
    float* dx;
    __device__ __forceinline__ float a(int p, int k) const {
        const int n = p / CF_T, t = p - n * CF_T;
        return da[gt_fi(n, t, k, 3 * (h >> 3))];
    }
    __device__ __forceinline__ float b(int k, int ci) const {
        const int64_t dir_floats = (int64_t)(cin + h) * 3 * h + 3 * h;
        const int d = k / (3 * h), r = k - d * 3 * h;
        const float* pd = prm + d * dir_floats;
        return r < 2 * h ? pd[(int64_t)ci * 2 * h + r] : pd[(int64_t)(cin + h) * 2 * h + 2 * h + (int64_t)ci * h + (r - 2 * h)];
    }
    __device__ __forceinline__ void store(int p, int ci, float acc) const {
        const int n = p / CF_T, t = p - n * CF_T;
        dx[gt_fi(n, t, ci, cin >> 4)] = acc;
    }
};

// weight-gradient operands: a(m, p) = L(p, m), b(p, n) = R(p, n)
struct GtConvDw {
    GtIn in;
    const float* dz;
    int kw, cout;
    __device__ __forceinline__ float a(int m, int p) const {
        const int n = p / CF_T, t = p - n * CF_T;
        if (m == kw * in.cin) return 1.f;                       // bias row
        const int tap = m / in.cin, c = m - tap * in.cin, tt = t + tap - (kw - 1) / 2;
        return (tt >= 0 && tt < CF_T) ? in.at(n, tt, c) : 0.f;
    }
    __device__ __forceinline__ float b(int p, int co) const {
        const int n = p / CF_T, t = p - n * CF_T;
        return dz[gt_fi(n, t, co, cout >> 4)];
    }
};

struct GtGruDw {
    const float* x;      // [.., cin] fragment plane with kbx feature tiles
    const float* y;      // the layer's output [.., 2H] (before dropout): h_prev
    const float* stash;  // [.., 6H] activated gates (r for the candidate's r . h_prev)
    const float* da;     // [.., 6H]
    int cin, kbx, h, dir, cand;
    __device__ __forceinline__ float a(int m, int p) const {
        const int n = p / CF_T, t = p - n * CF_T;
        if (m < cin) return x[gt_fi(n, t, m, kbx)];
        const int j = m - cin;
        if (j == h) return 1.f;                                  // bias row
        const int tp = dir == 0 ? t - 1 : t + 1;
        float hp = (tp >= 0 && tp < CF_T) ? y[gt_fi(n, tp, dir * h + j, h >> 3)] : 0.f;
        if (cand) hp *= stash[gt_fi(n, t, dir * 3 * h + j, 3 * (h >> 3))];
        return hp;
    }
    __device__ __forceinline__ float b(int p, int o) const {
        const int n = p / CF_T, t = p - n * CF_T;
        return da[gt_fi(n, t, dir * 3 * h + (cand ? 2 * h : 0) + o, 3 * (h >> 3))];
    }
};

struct GtHeadDw {
    const float* in;     // [.., F]
    const float* dl;     // [npad * 35] d loss / d logit
    int f16;
    __device__ __forceinline__ float a(int m, int p) const {
        if (m == 16 * f16) return 1.f;
        const int n = p / CF_T, t = p - n * CF_T;
        return in[gt_fi(n, t, m, f16)];
    }
    __device__ __forceinline__ float b(int p, int) const { return dl[p]; }
};

// ---- element-wise and small reductions -------------------------------------------------------------------------------------------
// one thread per (tile, channel): dz of the tile's 560 positions and (kPart) its partial sums of d gamma, d beta (part[tile][gamma C | beta C])
template <bool kPart>
__global__ __launch_bounds__(256) void gt_bn_bwd_kernel(const float* __restrict__ g, const float* __restrict__ mask, int relu,
                                                        const float* __restrict__ z, const float* __restrict__ prm, int cout,
                                                        float* __restrict__ dz, float* __restrict__ part, int n_tiles) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n_tiles * cout) return;
    const int tile = (int)(i / cout), c = (int)(i - (int64_t)tile * cout), c16 = cout >> 4;
    const float gam = prm[c], inv = rsqrtf(prm[3 * cout + c] + GT_BN_EPS);      // prm = gamma | beta | mean | var
    const float mean = prm[2 * cout + c], s = gam * inv;
    float sg = 0.f, sb = 0.f;
    for (int t = 0; t < CF_T; ++t)
        for (int w = 0; w < CF_TILE; ++w) {
            const int64_t o = gt_fi(tile * CF_TILE + w, t, c, c16);
            const float zz = z[o];
            float v = g[o];
            if (mask && !(mask[o] > 0.f)) v = 0.f;
            if (relu && !(fmaf(zz, s, prm[cout + c] - mean * s) > 0.f)) v = 0.f;      // the unit's own ReLU, from z as in gt_conv_fwd
            sb += v;
            sg = fmaf(v, (zz - mean) * inv, sg);
            dz[o] = v * s;
        }
    if (kPart) {
        part[(int64_t)tile * 2 * cout + c] = sg;
        part[(int64_t)tile * 2 * cout + cout + c] = sb;
    }
}

__global__ __launch_bounds__(256) void gt_dropout_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, const f32x4* __restrict__ scale,
                                                         int64_t n4, cf_dropout drop) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    out[i] = in[i] * (scale ? scale[i] : cf_drop_scale4(cf_drop_key(drop), drop.keep_prob, i));
}

__global__ __launch_bounds__(256) void gt_head_kernel(const float* __restrict__ in, int f16, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ labels, int64_t n_real, float inv_count, float* __restrict__ din,
                                                      float* __restrict__ dl, float* __restrict__ lossp, float* __restrict__ logits, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int n = (int)(p / CF_T), t = (int)(p - (int64_t)n * CF_T);
    float s = 0.f;
    for (int f = 0; f < 16 * f16; ++f) s = fmaf(in[gt_fi(n, t, f, f16)], w[f], s);
    s += bias[0];
    const bool real = n < n_real;
    const float lab = labels[p];
    const float d = real ? (1.f / (1.f + expf(-s)) - lab) * inv_count : 0.f;
    dl[p] = d;
    lossp[p] = real ? fmaxf(s, 0.f) - s * lab + log1pf(expf(-fabsf(s))) : 0.f;
    if (logits && real) logits[p] = s;
    for (int f = 0; f < 16 * f16; ++f) din[gt_fi(n, t, f, f16)] = d * w[f];
}

__global__ __launch_bounds__(256) void gt_loss_reduce_kernel(const float* __restrict__ lossp, int64_t P, float inv_count, float* __restrict__ loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int64_t p = threadIdx.x; p < P; p += 256) s += lossp[p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] * inv_count;
}

__global__ __launch_bounds__(256) void gt_x_frag_kernel(const float* __restrict__ x, float* __restrict__ xf, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int n = (int)(p / CF_T), t = (int)(p - (int64_t)n * CF_T);
    for (int f = 0; f < 16; ++f) xf[gt_fi(n, t, f, 1)] = f == 0 ? x[p] : 0.f;
}

// ---- backward of the inference function (torch.ops.catfish.resnetrnn_forward's autograd, catfish_amd/op_grad.py) ---------------
// head from an upstream gradient of the probabilities: p = sigmoid(z), dz = g p (1 - p) = g e / (1 + e)^2 with e = exp(-|z|) (no
// overflow for any z); d input = dz w.  Padding windows carry g = 0, so every gradient they feed is an exact zero.
__global__ __launch_bounds__(256) void gt_head_bwd_kernel(const float* __restrict__ in, int f16, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ dprobs, float* __restrict__ din, float* __restrict__ dl, int64_t P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int n = (int)(p / CF_T), t = (int)(p - (int64_t)n * CF_T);
    float s = 0.f;
    for (int f = 0; f < 16 * f16; ++f) s = fmaf(in[gt_fi(n, t, f, f16)], w[f], s);
    s += bias[0];
    const float e = expf(-fabsf(s)), q = 1.f + e;
    const float d = dprobs[p] * (e / (q * q));
    dl[p] = d;
    for (int f = 0; f < 16 * f16; ++f) din[gt_fi(n, t, f, f16)] = d * w[f];
}

// d loss / d signal [n_windows][35], one thread per position (threads of a wave walk the 16 windows of a tile, then the steps), one
// fixed summation order.  ResNetRNN (c > 0): the signal feeds only block 0's shortcut and first conv (kw 1, cin 1, kernel = c
// weights): dx = sum_o dz_sc[o] w_sc[o] + dz_1[o] w_1[o].  Plain RNN (h > 0): the signal is row 0 of layer 0's input; da holds
// (dir, gate r / u / c, unit) at the step each direction consumed x_t (both directions in natural time order, as in GtGruDx) and
// the candidate's x part is not gated by r: dx = sum_dir (sum_j<2H da_ru[j] Wg[0][j] + sum_j<H da_c[j] Wc[0][j]).
__global__ __launch_bounds__(256) void gt_signal_grad_kernel(int h, int c, const float* __restrict__ p0, const float* __restrict__ g0,
                                                             const float* __restrict__ p1, const float* __restrict__ g1, float* __restrict__ dx,
                                                             int64_t P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int64_t tile = i / (CF_TILE * CF_T);
    const int r = (int)(i - tile * CF_TILE * CF_T), t = r / CF_TILE, n = (int)tile * CF_TILE + (r - t * CF_TILE);
    float s = 0.f;
    if (c > 0) {
        const int c16 = c >> 4;
        for (int o = 0; o < c; ++o) {
            s = fmaf(g0[gt_fi(n, t, o, c16)], p0[o], s);
            s = fmaf(g1[gt_fi(n, t, o, c16)], p1[o], s);
        }
    } else {
        const int f16 = 3 * (h >> 3);
        const int64_t dir_floats = (int64_t)(1 + h) * 3 * h + 3 * h;
        for (int d = 0; d < 2; ++d) {
            const float* pd = p0 + d * dir_floats;
            const float* wc = pd + (int64_t)(1 + h) * 2 * h + 2 * h;
            for (int j = 0; j < 2 * h; ++j) s = fmaf(g0[gt_fi(n, t, d * 3 * h + j, f16)], pd[j], s);
            for (int j = 0; j < h; ++j) s = fmaf(g0[gt_fi(n, t, d * 3 * h + 2 * h + j, f16)], wc[j], s);
        }
    }
    dx[(int64_t)n * CF_T + t] = s;
}

// BN moving statistics: y = (z - mean) gamma / sqrt(var + eps) + beta, so from the BN-output sums d gamma, d beta of the unit
// d mean = -gamma d beta / sqrt(var + eps) and d var = -gamma d gamma / (2 (var + eps)); one thread per channel
__global__ __launch_bounds__(256) void gt_bn_stat_grads_kernel(const float* __restrict__ prm, float* __restrict__ grads, int cout) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c >= cout) return;
    const float gam = prm[c], ve = prm[3 * cout + c] + GT_BN_EPS;                 // prm, grads = gamma | beta | mean | var
    grads[2 * cout + c] = -gam * grads[cout + c] * rsqrtf(ve);
    grads[3 * cout + c] = -gam * grads[c] / (2.f * ve);
}

// ---- C ABI (include/catfish_hip.h, "whole-step training of any geometry") --------------------------------------------------------
static int gt_args(const cf_model* m, int64_t n_windows, const char* who) {
    if (!m) return fail(CF_ERR_INVALID, std::string(who) + ": null model");
    if (n_windows <= 0 || (n_windows % CF_TILE) != 0 || n_windows > (int64_t)1 << 24)
        return fail(CF_ERR_INVALID, std::string(who) + ": n_windows must be a positive multiple of 16");
    return CF_OK;
}
static bool gt_ch_ok(int c) { return c >= 16 && c <= 512 && (c % 16) == 0; }
static int gt_chunks(int64_t n_windows) { return (int)((n_windows + GT_CHUNK_WINDOWS - 1) / GT_CHUNK_WINDOWS); }

template <class Op>
static int gt_wgrad(const Op& op, int M, int N, int64_t n_windows, float* ws, int64_t ws_floats, float* dst, hipStream_t s, const char* who) {
    const int chunks = gt_chunks(n_windows);
    const int64_t len = (int64_t)M * N;
    if (!ws || ws_floats < len * chunks) return fail(CF_ERR_INVALID, std::string(who) + ": workspace too small");
    hipLaunchKernelGGL(gt_wgrad_kernel<Op>, dim3((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64), (unsigned)chunks), dim3(256), 0, s, op, M, N,
                       (int)(n_windows * CF_T), GT_CHUNK_WINDOWS * CF_T, ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gt_reduce_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, ws, len, chunks, dst);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int64_t cf_gen_train_workspace_floats(int32_t rows, int32_t cols, int64_t n_windows) {
    if (rows <= 0 || cols <= 0 || n_windows <= 0) return 0;
    return (int64_t)rows * cols * gt_chunks(n_windows);
}

extern "C" int cf_gen_conv_forward(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* x, const float* shortcut,
                                   int32_t relu, float* z_stash, float* out, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_conv_forward");
    if (rc != CF_OK) return rc;
    if (!unit || !x || !z_stash || !out) return fail(CF_ERR_INVALID, "cf_gen_conv_forward: null buffer");
    if ((kw != 1 && kw != 3) || !(cin == 1 || gt_ch_ok(cin)) || !gt_ch_ok(cout))
        return fail(CF_ERR_INVALID, "cf_gen_conv_forward: kw must be 1 or 3, cin 1 or a multiple of 16 up to 512, cout a multiple of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    const int P = (int)(n_windows * CF_T);
    GtConvFwd op{GtIn{x, cin, cin / 16}, unit, kw, cout, shortcut, relu ? 1 : 0, z_stash, out};
    hipLaunchKernelGGL(gt_gemm_kernel<GtConvFwd>, dim3((unsigned)((P + 63) / 64), (unsigned)((cout + 63) / 64)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), op, P, (int)cout, (int)(kw * cin));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_conv_backward_data(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* dz,
                                         const float* add, float* dx, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_conv_backward_data");
    if (rc != CF_OK) return rc;
    if (!unit || !dz || !dx) return fail(CF_ERR_INVALID, "cf_gen_conv_backward_data: null buffer");
    if ((kw != 1 && kw != 3) || !gt_ch_ok(cin) || !gt_ch_ok(cout))
        return fail(CF_ERR_INVALID, "cf_gen_conv_backward_data: kw must be 1 or 3, cin and cout multiples of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    const int P = (int)(n_windows * CF_T);
    GtConvDx op{dz, unit, kw, cin, cout, add, dx};
    hipLaunchKernelGGL(gt_gemm_kernel<GtConvDx>, dim3((unsigned)((P + 63) / 64), (unsigned)((cin + 63) / 64)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), op, P, (int)cin, (int)(kw * cout));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_bn_backward(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* g, const float* mask,
                                  int32_t relu, const float* z_stash, float* dz, float* workspace, int64_t workspace_floats,
                                  float* unit_grads, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_bn_backward");
    if (rc != CF_OK) return rc;
    if (!unit || !g || !z_stash || !dz || !workspace || !unit_grads) return fail(CF_ERR_INVALID, "cf_gen_bn_backward: null buffer");
    if ((kw != 1 && kw != 3) || !(cin == 1 || gt_ch_ok(cin)) || !gt_ch_ok(cout))
        return fail(CF_ERR_INVALID, "cf_gen_bn_backward: kw must be 1 or 3, cin 1 or a multiple of 16 up to 512, cout a multiple of 16 up to 512");
    const int n_tiles = (int)(n_windows / CF_TILE);
    if (workspace_floats < (int64_t)n_tiles * 2 * cout) return fail(CF_ERR_INVALID, "cf_gen_bn_backward: workspace too small");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t kf = (int64_t)kw * cin * cout + cout;            // gamma follows kernel | bias
    const int64_t items = (int64_t)n_tiles * cout;
    hipLaunchKernelGGL(gt_bn_bwd_kernel<true>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, g, mask, relu ? 1 : 0, z_stash, unit + kf, (int)cout,
                       dz, workspace, n_tiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gt_reduce_kernel, dim3((unsigned)((2 * cout + 255) / 256)), dim3(256), 0, s, workspace, (int64_t)2 * cout, n_tiles,
                       unit_grads + kf);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_conv_wgrad(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* x, const float* dz, float* workspace,
                                 int64_t workspace_floats, float* unit_grads, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_conv_wgrad");
    if (rc != CF_OK) return rc;
    if (!x || !dz || !unit_grads) return fail(CF_ERR_INVALID, "cf_gen_conv_wgrad: null buffer");
    if ((kw != 1 && kw != 3) || !(cin == 1 || gt_ch_ok(cin)) || !gt_ch_ok(cout))
        return fail(CF_ERR_INVALID, "cf_gen_conv_wgrad: kw must be 1 or 3, cin 1 or a multiple of 16 up to 512, cout a multiple of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    GtConvDw op{GtIn{x, cin, cin / 16}, dz, kw, cout};
    return gt_wgrad(op, kw * cin + 1, cout, n_windows, workspace, workspace_floats, unit_grads, reinterpret_cast<hipStream_t>(stream),
                    "cf_gen_conv_wgrad");
}

extern "C" int cf_gen_gru_dx(cf_model* m, int32_t layer_size, int32_t cin, const float* layer_params, const float* da, float* dx,
                             int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_gru_dx");
    if (rc != CF_OK) return rc;
    if (!layer_params || !da || !dx) return fail(CF_ERR_INVALID, "cf_gen_gru_dx: null buffer");
    if (layer_size < 16 || layer_size > 256 || (layer_size % 16) != 0 || !gt_ch_ok(cin))
        return fail(CF_ERR_INVALID, "cf_gen_gru_dx: layer_size must be a multiple of 16 up to 256, cin a multiple of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    const int P = (int)(n_windows * CF_T);
    GtGruDx op{da, layer_params, layer_size, cin, dx};
    hipLaunchKernelGGL(gt_gemm_kernel<GtGruDx>, dim3((unsigned)((P + 63) / 64), (unsigned)((cin + 63) / 64)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), op, P, (int)cin, 6 * layer_size);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_gru_wgrad(cf_model* m, int32_t layer_size, int32_t cin, const float* x_frag, const float* y_frag, const float* stash,
                                const float* da, float* workspace, int64_t workspace_floats, float* layer_grads, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_gru_wgrad");
    if (rc != CF_OK) return rc;
    if (!x_frag || !y_frag || !stash || !da || !layer_grads) return fail(CF_ERR_INVALID, "cf_gen_gru_wgrad: null buffer");
    if (layer_size < 16 || layer_size > 256 || (layer_size % 16) != 0 || !(cin == 1 || gt_ch_ok(cin)))
        return fail(CF_ERR_INVALID, "cf_gen_gru_wgrad: layer_size must be a multiple of 16 up to 256, cin 1 or a multiple of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int h = layer_size, rows = cin + h + 1, kbx = (cin + 15) / 16;
    const int64_t dir_floats = (int64_t)(cin + h) * 3 * h + 3 * h;
    for (int d = 0; d < 2; ++d)
        for (int cand = 0; cand < 2; ++cand) {
            GtGruDw op{x_frag, y_frag, stash, da, cin, kbx, h, d, cand};
            float* dst = layer_grads + d * dir_floats + (cand ? (int64_t)rows * 2 * h : 0);     // gates kernel | bias, candidate kernel | bias
            rc = gt_wgrad(op, rows, cand ? h : 2 * h, n_windows, workspace, workspace_floats, dst, s, "cf_gen_gru_wgrad");
            if (rc != CF_OK) return rc;
        }
    return CF_OK;
}

extern "C" int cf_gen_dropout(cf_model* m, int32_t layer_size, float keep_prob, uint32_t seed, int32_t layer, const double* step_count,
                              const float* scale_frag, const float* in_frag, float* out_frag, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_dropout");
    if (rc != CF_OK) return rc;
    if (!in_frag || !out_frag) return fail(CF_ERR_INVALID, "cf_gen_dropout: null buffer");
    if (layer_size < 16 || layer_size > 256 || (layer_size % 16) != 0) return fail(CF_ERR_INVALID, "cf_gen_dropout: layer_size must be a multiple of 16 up to 256");
    if (!scale_frag && !(keep_prob > 0.f && keep_prob < 1.f)) return fail(CF_ERR_INVALID, "cf_gen_dropout: keep_prob must be in (0, 1)");
    HIP_TRY(hipSetDevice(m->device));
    const int64_t n4 = n_windows / CF_TILE * CF_T * (layer_size / 8) * 64;
    hipLaunchKernelGGL(gt_dropout_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const f32x4*>(in_frag), reinterpret_cast<f32x4*>(out_frag), reinterpret_cast<const f32x4*>(scale_frag), n4,
                       make_dropout(keep_prob, seed, layer, step_count));
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_head(cf_model* m, int32_t features, const float* in_frag, const float* dense, const float* labels, int64_t n_real,
                           float* din_frag, float* logits, float* workspace, int64_t workspace_floats, float* dense_grads, float* loss,
                           int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_head");
    if (rc != CF_OK) return rc;
    if (!in_frag || !dense || !labels || !din_frag || !workspace || !dense_grads || !loss) return fail(CF_ERR_INVALID, "cf_gen_head: null buffer");
    if (!gt_ch_ok(features)) return fail(CF_ERR_INVALID, "cf_gen_head: features must be a multiple of 16 up to 512");
    if (n_real <= 0 || n_real > n_windows || n_windows - n_real >= CF_TILE) return fail(CF_ERR_INVALID, "cf_gen_head: n_real must be in (n_windows - 16, n_windows]");
    const int64_t P = n_windows * CF_T;
    const int64_t need = 2 * P + cf_gen_train_workspace_floats(features + 1, 1, n_windows);
    if (workspace_floats < need) return fail(CF_ERR_INVALID, "cf_gen_head: workspace too small (cf_gen_head_workspace_floats)");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float inv_count = (float)(1.0 / ((double)n_real * CF_T));
    float* dl = workspace;
    float* lossp = workspace + P;
    hipLaunchKernelGGL(gt_head_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, in_frag, (int)features / 16, dense, dense + features, labels,
                       n_real, inv_count, din_frag, dl, lossp, logits, P);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gt_loss_reduce_kernel, dim3(1), dim3(256), 0, s, lossp, P, inv_count, loss);
    HIP_TRY(hipGetLastError());
    GtHeadDw op{in_frag, dl, (int)features / 16};
    return gt_wgrad(op, features + 1, 1, n_windows, workspace + 2 * P, workspace_floats - 2 * P, dense_grads, s, "cf_gen_head");
}

extern "C" int64_t cf_gen_head_workspace_floats(int32_t features, int64_t n_windows) {
    if (features <= 0 || n_windows <= 0) return 0;
    return 2 * n_windows * CF_T + cf_gen_train_workspace_floats(features + 1, 1, n_windows);
}

extern "C" int cf_gen_x_frag(cf_model* m, const float* x, float* x_frag, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_x_frag");
    if (rc != CF_OK) return rc;
    if (!x || !x_frag) return fail(CF_ERR_INVALID, "cf_gen_x_frag: null buffer");
    HIP_TRY(hipSetDevice(m->device));
    const int64_t P = n_windows * CF_T;
    hipLaunchKernelGGL(gt_x_frag_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, x_frag, P);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}


// ---- C ABI (include/catfish_hip.h, "backward of the inference function") ---------------------------------------------------------
extern "C" int64_t cf_gen_head_backward_workspace_floats(int32_t features, int64_t n_windows) {
    if (features <= 0 || n_windows <= 0) return 0;
    return n_windows * CF_T + cf_gen_train_workspace_floats(features + 1, 1, n_windows);
}

extern "C" int cf_gen_head_backward(cf_model* m, int32_t features, const float* in_frag, const float* dense, const float* dprobs, float* din_frag,
                                    float* workspace, int64_t workspace_floats, float* dense_grads, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_head_backward");
    if (rc != CF_OK) return rc;
    if (!in_frag || !dense || !dprobs || !din_frag || !workspace) return fail(CF_ERR_INVALID, "cf_gen_head_backward: null buffer");
    if (!gt_ch_ok(features)) return fail(CF_ERR_INVALID, "cf_gen_head_backward: features must be a multiple of 16 up to 512");
    const int64_t P = n_windows * CF_T;
    if (workspace_floats < cf_gen_head_backward_workspace_floats(features, n_windows))
        return fail(CF_ERR_INVALID, "cf_gen_head_backward: workspace too small (cf_gen_head_backward_workspace_floats)");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* dl = workspace;
    hipLaunchKernelGGL(gt_head_bwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, in_frag, (int)features / 16, dense, dense + features,
                       dprobs, din_frag, dl, P);
    HIP_TRY(hipGetLastError());
    if (!dense_grads) return CF_OK;
    GtHeadDw op{in_frag, dl, (int)features / 16};
    return gt_wgrad(op, features + 1, 1, n_windows, workspace + P, workspace_floats - P, dense_grads, s, "cf_gen_head_backward");
}

extern "C" int cf_gen_signal_grad(cf_model* m, int32_t layer_size, int32_t channels, const float* params0, const float* grad0, const float* params1,
                                  const float* grad1, float* dx, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_signal_grad");
    if (rc != CF_OK) return rc;
    if (!params0 || !grad0 || !dx || (channels != 0 && (!params1 || !grad1))) return fail(CF_ERR_INVALID, "cf_gen_signal_grad: null buffer");
    const bool res = layer_size == 0 && gt_ch_ok(channels);
    const bool rnn = channels == 0 && layer_size >= 16 && layer_size <= 256 && (layer_size % 16) == 0;
    if (!res && !rnn)
        return fail(CF_ERR_INVALID, "cf_gen_signal_grad: give either channels (a multiple of 16 up to 512, layer_size 0) or layer_size "
                                    "(a multiple of 16 up to 256, channels 0)");
    HIP_TRY(hipSetDevice(m->device));
    const int64_t P = n_windows * CF_T;
    hipLaunchKernelGGL(gt_signal_grad_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (int)layer_size,
                       (int)channels, params0, grad0, params1, grad1, dx, P);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_bn_backward_data(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* g, const float* mask,
                                       int32_t relu, const float* z_stash, float* dz, int64_t n_windows, void* stream) {
    int rc = gt_args(m, n_windows, "cf_gen_bn_backward_data");
    if (rc != CF_OK) return rc;
    if (!unit || !g || !z_stash || !dz) return fail(CF_ERR_INVALID, "cf_gen_bn_backward_data: null buffer");
    if ((kw != 1 && kw != 3) || !(cin == 1 || gt_ch_ok(cin)) || !gt_ch_ok(cout))
        return fail(CF_ERR_INVALID, "cf_gen_bn_backward_data: kw must be 1 or 3, cin 1 or a multiple of 16 up to 512, cout a multiple of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    const int n_tiles = (int)(n_windows / CF_TILE);
    const int64_t kf = (int64_t)kw * cin * cout + cout;
    const int64_t items = (int64_t)n_tiles * cout;
    hipLaunchKernelGGL(gt_bn_bwd_kernel<false>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, mask,
                       relu ? 1 : 0, z_stash, unit + kf, (int)cout, dz, nullptr, n_tiles);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_gen_bn_stat_grads(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, float* unit_grads, void* stream) {
    if (!m) return fail(CF_ERR_INVALID, "cf_gen_bn_stat_grads: null model");
    if (!unit || !unit_grads) return fail(CF_ERR_INVALID, "cf_gen_bn_stat_grads: null buffer");
    if ((kw != 1 && kw != 3) || !(cin == 1 || gt_ch_ok(cin)) || !gt_ch_ok(cout))
        return fail(CF_ERR_INVALID, "cf_gen_bn_stat_grads: kw must be 1 or 3, cin 1 or a multiple of 16 up to 512, cout a multiple of 16 up to 512");
    HIP_TRY(hipSetDevice(m->device));
    const int64_t kf = (int64_t)kw * cin * cout + cout;
    hipLaunchKernelGGL(gt_bn_stat_grads_kernel, dim3((unsigned)((cout + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), unit + kf,
                       unit_grads + kf, (int)cout);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
