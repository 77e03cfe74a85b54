// train_step.hpp -- the parts of the training step around the conv stack and the biGRU layers (BASELINE config 5),
// included by catfish_hip.hip:
//
//   train_head_kernel     final_fully_connected + tf.losses.sigmoid_cross_entropy (rnn_class.py:74-79,178-183), forward AND
//                         backward in one pass over the last biGRU layer's output in the kernels' fragment layout:
//                           z = w . h + b,  loss = mean(max(z,0) - z y + log1p(exp(-|z|))),
//                           dz = (sigmoid(z) - y) / count,  dh = dz w,  dw = sum dz h,  db = sum dz
//   train_head_reduce     partial sums added in a fixed order (bit-reproducible, no atomics)
//   opt_step_kernel       tf.train.RMSPropOptimizer / AdamOptimizer update (TF-1 defaults, rnn_class.py:62-71) of ALL variables
//                         at once: parameters, gradients and both slot variables live in flat buffers of one layout
//   gather_scale_kernel   re-tiling of the updated biGRU weights into MFMA fragment order: packed[i] = flat[idx[i]] * scale[i]
#pragma once

#define CF_HEAD_PART 132            // floats per partial: dw[128] | db | loss | 2 pad

// One wave per (tile, t) item: 16 windows x 128 features as 8 f32x4 per lane (feature 16m + 4q + r of window lane & 15).
__global__ __launch_bounds__(256) void train_head_kernel(const f32x4* __restrict__ Y,      // [tile][t][8][lane]: the dense layer's input
                                                         const float* __restrict__ w,      // final_fully_connected/kernel [128]
                                                         const float* __restrict__ bias,   // [1]
                                                         const float* __restrict__ labels, // [n_windows][35]
                                                         f32x4* __restrict__ DY,           // [tile][t][8][lane]: d loss / d input
                                                         float* __restrict__ logits,       // [n_windows][35] or null
                                                         float* __restrict__ part,         // [n_waves][CF_HEAD_PART]
                                                         int64_t n_windows, int n_tiles, float inv_count) {
    const int lane = threadIdx.x & 63;
    const int q = lane >> 4, wl = lane & 15;
    const int wave_g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * (blockDim.x >> 6);
    f32x4 wv[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) wv[m] = *reinterpret_cast<const f32x4*>(w + 16 * m + 4 * q);
    const float b = bias[0];
    f32x4 dw[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) dw[m] = (f32x4){0, 0, 0, 0};
    float db = 0.f, loss = 0.f;
    const int n_items = n_tiles * CF_T;
    for (int item = wave_g; item < n_items; item += n_waves) {
        const int tile = item / CF_T, t = item - tile * CF_T;
        const f32x4* src = Y + (int64_t)item * 8 * 64 + lane;
        f32x4 h[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) h[m] = src[m * 64];
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            s = fmaf(wv[m].x, h[m].x, s); s = fmaf(wv[m].y, h[m].y, s); s = fmaf(wv[m].z, h[m].z, s); s = fmaf(wv[m].w, h[m].w, s);
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float z = s + b;
        const int64_t win = (int64_t)tile * CF_TILE + wl;
        float dz = 0.f;
        if (win < n_windows) {
            const float yv = labels[win * CF_T + t];
            if (q == 0) {
                loss += fmaxf(z, 0.f) - z * yv + log1pf(expf(-fabsf(z)));
                if (logits) logits[win * CF_T + t] = z;
            }
            dz = (1.0f / (1.0f + expf(-z)) - yv) * inv_count;
        }
        if (q == 0) db += dz;
        f32x4* dst = DY + (int64_t)item * 8 * 64 + lane;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            dst[m * 64] = wv[m] * dz;
            dw[m] += h[m] * dz;
        }
    }
    // reduce over the 16 windows of a lane quarter; lane 16 q then holds features 16 m + 4 q + r
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = dw[m][r];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
            dw[m][r] = v;
        }
    db += __shfl_xor(db, 1); db += __shfl_xor(db, 2); db += __shfl_xor(db, 4); db += __shfl_xor(db, 8);
    loss += __shfl_xor(loss, 1); loss += __shfl_xor(loss, 2); loss += __shfl_xor(loss, 4); loss += __shfl_xor(loss, 8);
    float* out = part + (size_t)wave_g * CF_HEAD_PART;
    if (wl == 0) {
#pragma unroll
        for (int m = 0; m < 8; ++m) *reinterpret_cast<f32x4*>(out + 16 * m + 4 * q) = dw[m];
        if (q == 0) { out[128] = db; out[129] = loss; out[130] = 0.f; out[131] = 0.f; }
    }
}

// grads = dw[128] | db[1]; loss_out[0] = mean loss.  One 256-thread block per 64 elements (cf_reduce_parts' contract).
__global__ __launch_bounds__(256) void train_head_reduce_kernel(const float* __restrict__ part, int n_parts, float* __restrict__ grads,
                                                                float* __restrict__ loss_out, float inv_count) {
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const float sum = cf_reduce_parts(part, CF_HEAD_PART, n_parts, e, e < 130);
    if (threadIdx.x >= 64 || e >= 130) return;
    if (e < 129) grads[e] = sum;
    else loss_out[0] = sum * inv_count;
}

// kind 0 = RMSProp (decay 0.9, momentum 0, epsilon 1e-10; slot1 = rms (initialised to 1), slot2 = momentum)
// kind 1 = Adam (beta 0.9 / 0.999, epsilon 1e-8; slot1 = m, slot2 = v); t_dev holds the number of steps taken BEFORE this one
__device__ __forceinline__ float opt_adam_lr_t(float lr, const double* __restrict__ t_dev) {
    const double t = t_dev[0] + 1.0;
    return (float)((double)lr * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
}

// the update of element i with gradient gi: the one statement of the formulas, for opt_step_kernel and opt_step_guarded_kernel
__device__ __forceinline__ void opt_update(int kind, float* __restrict__ p, float gi, float* __restrict__ s1, float* __restrict__ s2,
                                           int64_t i, float lr, float lr_t) {
    if (kind == 0) {
        float ms = s1[i] * 0.9f;
        ms = fmaf(0.1f * gi, gi, ms);                    // addcmul(rms, g, g, value = 1 - decay)
        const float upd = gi / sqrtf(ms + 1e-10f) * lr;
        s1[i] = ms;
        s2[i] = upd;
        p[i] -= upd;
    } else {
        float m = s1[i] * 0.9f;
        m = fmaf(0.1f, gi, m);
        float v = s2[i] * 0.999f;
        v = fmaf(0.001f * gi, gi, v);
        s1[i] = m;
        s2[i] = v;
        p[i] -= m / (sqrtf(v) + 1e-8f) * lr_t;
    }
}

__global__ __launch_bounds__(256) void opt_step_kernel(int kind, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                       float* __restrict__ s2, int64_t n, float lr, const double* __restrict__ t_dev) {
    __shared__ float lr_t_s;
    if (kind == 1 && threadIdx.x == 0) lr_t_s = opt_adam_lr_t(lr, t_dev);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    opt_update(kind, p, g[i], s1, s2, i, lr, lr_t_s);
}

__global__ __launch_bounds__(256) void gather_scale_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ scale, float* __restrict__ dst, int64_t n,
                                                           double* __restrict__ t_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && t_dev) t_dev[0] += 1.0;                // the optimizer step that precedes this launch has read it
    if (i < n) dst[i] = src[idx[i]] * scale[i];
}

// ---- global-norm gradient clipping and the non-finite-step guard (include/catfish_hip_ext.h) ----------------------------------
// record (device double[4]): [0] g = sqrt(sum g_i^2) of the last step, [1] the scale applied (CF_CLIP_SKIPPED on a skipped step),
// [2] steps clipped, [3] steps skipped.
//   grad_sq_partial_kernel    one workgroup per chunk of CF_CLIP_CHUNK floats: part[chunk] = sum of double(g_i)^2
//   grad_norm_finish_kernel   one workgroup: folds the partials, decides scale / skip, updates the record
//   opt_step_guarded_kernel   opt_step_kernel on float32(g_i * scale); nothing on a skipped step
//   gather_scale_guarded_kernel   gather_scale_kernel; neither the gather nor the step count on a skipped step
// Every sum has a fixed shape that depends on n alone (a thread's terms in ascending order, then clip_block_sum's tree), and there
// are no atomics: equal inputs give equal bits.

// sum of v over the 256 threads of a workgroup, in one fixed order: xor butterfly within a wave, then waves 0..3 in order; the
// result is valid in thread 0
__device__ __forceinline__ double clip_block_sum(double v, double* __restrict__ wave_sums) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

__global__ __launch_bounds__(256) void grad_sq_partial_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    __shared__ double wave_sums[4];
    const int64_t base = (int64_t)blockIdx.x * CF_CLIP_CHUNK;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < CF_CLIP_CHUNK / 1024; ++k) {
        const int64_t i = base + (int64_t)(k * 256 + (int)threadIdx.x) * 4;
        if (i + 3 < n) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
            acc += (double)v.x * (double)v.x;                // the square of a float32 is exact in float64
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        } else {
            for (int64_t j = i; j < n; ++j) acc += (double)g[j] * (double)g[j];
        }
    }
    const double sum = clip_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ part, int64_t n_parts, double clip_norm, int flags,
                                                               const float* __restrict__ loss, double* __restrict__ rec) {
    __shared__ double wave_sums[4];
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < n_parts; c += 256) acc += part[c];
    const double S = clip_block_sum(acc, wave_sums);
    if (threadIdx.x != 0) return;
    const double gn = sqrt(S);
    const bool skip = (flags & CF_CLIP_SKIP_NONFINITE) && (!isfinite(S) || (loss && !isfinite(loss[0])));
    const float s32 = (flags & CF_CLIP_SCALE) ? (float)(clip_norm / fmax(gn, clip_norm)) : 1.0f;
    rec[0] = gn;
    rec[1] = skip ? (double)CF_CLIP_SKIPPED : (double)s32;
    if (skip) rec[3] += 1.0;
    else if (s32 < 1.0f) rec[2] += 1.0;
}

__global__ __launch_bounds__(256) void opt_step_guarded_kernel(int kind, float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ s1, float* __restrict__ s2, int64_t n, float lr,
                                                               const double* __restrict__ t_dev, const double* __restrict__ rec) {
    __shared__ float lr_t_s;
    const double scale = rec[1];
    if (scale == (double)CF_CLIP_SKIPPED) return;            // uniform over the grid: a skipped step writes nothing
    if (kind == 1 && threadIdx.x == 0) lr_t_s = opt_adam_lr_t(lr, t_dev);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    opt_update(kind, p, __fmul_rn(g[i], (float)scale), s1, s2, i, lr, lr_t_s);      // one rounding; g_i * 1.0f is g_i
}

__global__ __launch_bounds__(256) void gather_scale_guarded_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                                   const float* __restrict__ scale, float* __restrict__ dst, int64_t n,
                                                                   double* __restrict__ t_dev, const double* __restrict__ rec) {
    if (rec[1] == (double)CF_CLIP_SKIPPED) return;           // a skipped step is not counted and re-tiles nothing
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) t_dev[0] += 1.0;                            // the optimizer step that precedes this launch has read it
    if (i < n) dst[i] = src[idx[i]] * scale[i];
}
