// Device-resident validation set: one checkpoint round's stretches are packed and scored on the card
// (catfish_amd/device_validation.py states both steps in numpy -- DeviceValidationSet.pack and score_host are normative; the
// reference's round is networks/train_validate.py:188-295 with rnn_class.py:222-261 per read).
//
//   gather   packed sample bounds[r] + i  <-  signal[src_first[r] + i], labels[src_first[r] + i]   for i < length[r], else 0 and 0
//            (the zero tail up to the window multiple).  Every sample depends on its own index only.
//   score    per read: how many samples have rint(p) == y, and the sum of the fp64 sigmoid cross-entropy of the logits;
//            per threshold t over the whole batch: tp / fp / tn / fn of (p >= t) against y.
//
// Grid: blockIdx.x = read, blockIdx.y strides over the read's pieces, so any grid height is correct and the host's longest-read
// figure is only a hint for it.
//
// score cuts a read into chunks of CF_SCORE_CHUNK samples; one workgroup reduces one chunk.  The cross-entropy goes thread ->
// wave butterfly -> LDS, waves added in wave order -> the chunk's slot of `partials`; a second launch adds a read's slots in chunk
// order.  No floating-point atomics: two runs give the same bits.  The integer counts are summed per thread, over the wave by the same
// butterfly, over the waves in LDS, and added to the (zeroed) outputs with integer atomics, whose order cannot show.
//
// Chunk c of read r owns slot bounds[r] / CF_SCORE_CHUNK + r + c: consecutive reads' first slots differ by at least
// floor(size / CHUNK) + 1 >= ceil(size / CHUNK), so slots never collide and total / CF_SCORE_CHUNK + n of them suffice.
#pragma once

#define CF_SCORE_CHUNK 2048
#define CF_SCORE_MAX_K 16
#define CF_SCORE_THREADS 256
#define CF_SCORE_PER_THREAD (CF_SCORE_CHUNK / CF_SCORE_THREADS)
#define CF_SCORE_WAVES (CF_SCORE_THREADS / 64)
#define CF_SCORE_COUNTS (3 * CF_SCORE_MAX_K + 3)

__global__ __launch_bounds__(256) void validation_gather_kernel(const float* __restrict__ signal, const uint8_t* __restrict__ labels,
                                                                int64_t signal_total, const int64_t* __restrict__ src_first,
                                                                const int64_t* __restrict__ length, const int64_t* __restrict__ bounds,
                                                                int64_t total, float* __restrict__ x, uint8_t* __restrict__ y) {
    const int64_t r = blockIdx.x;
    const int64_t b0 = bounds[r], size = bounds[r + 1] - b0, len = length[r], src = src_first[r];
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < size; i += (int64_t)gridDim.y * 256) {
        if ((uint64_t)(b0 + i) >= (uint64_t)total) continue;                     // a table that disagrees with the buffers writes nothing
        const bool real = i < len && (uint64_t)(src + i) < (uint64_t)signal_total;
        x[b0 + i] = real ? signal[src + i] : 0.0f;
        y[b0 + i] = real ? labels[src + i] : (uint8_t)0;
    }
}

// three counts of at most 512 per wave (64 lanes x CF_SCORE_PER_THREAD samples) ride in one word, 10 bits each
#define CF_SCORE_FIELD 10
#define CF_SCORE_FIELD_MASK ((1u << CF_SCORE_FIELD) - 1u)
static_assert(64 * CF_SCORE_PER_THREAD <= (int)CF_SCORE_FIELD_MASK, "a wave's count must fit its field");

__device__ __forceinline__ unsigned cf_wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(CF_SCORE_THREADS) void validation_score_kernel(const float* __restrict__ probs, const float* __restrict__ logits,
                                                                            const uint8_t* __restrict__ y, const int64_t* __restrict__ bounds,
                                                                            int64_t total, const double* __restrict__ thresholds, int K,
                                                                            unsigned long long* __restrict__ right_out,
                                                                            unsigned long long* __restrict__ counts_out,
                                                                            double* __restrict__ partials, int64_t partial_slots) {
    __shared__ double s_ce[CF_SCORE_WAVES];
    __shared__ unsigned s_cnt[CF_SCORE_WAVES][CF_SCORE_COUNTS];
    __shared__ unsigned s_tot[CF_SCORE_COUNTS];
    const int64_t r = blockIdx.x;
    const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
    const int64_t n_chunks = (size + CF_SCORE_CHUNK - 1) / CF_SCORE_CHUNK;
    const int64_t slot0 = b0 / CF_SCORE_CHUNK + r;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (int64_t c = blockIdx.y; c < n_chunks; c += gridDim.y) {
        float p[CF_SCORE_PER_THREAD];
        unsigned kind[CF_SCORE_PER_THREAD];                // what a CALLED sample adds: 1 | (y == 1) << 10 | (y == 0) << 20; 0 = no sample here
        double ce = 0.0;
        unsigned own = 0;                                  // samples | zero labels << 10 | right << 20
#pragma unroll
        for (int j = 0; j < CF_SCORE_PER_THREAD; ++j) {
            const int64_t i = c * CF_SCORE_CHUNK + j * CF_SCORE_THREADS + threadIdx.x;
            p[j] = 0.0f;
            kind[j] = 0u;
            if (i < size && (uint64_t)(b0 + i) < (uint64_t)total) {
                p[j] = probs[b0 + i];
                const unsigned label = y[b0 + i];
                const double zd = (double)logits[b0 + i], yd = (double)label;
                ce += fmax(zd, 0.0) - zd * yd + log1p(exp(-fabs(zd)));
                kind[j] = 1u | (label == 1u ? 1u << CF_SCORE_FIELD : 0u) | (label == 0u ? 1u << (2 * CF_SCORE_FIELD) : 0u);
                own += 1u + (label == 0u ? 1u << CF_SCORE_FIELD : 0u)
                       + (rint((double)p[j]) == yd ? 1u << (2 * CF_SCORE_FIELD) : 0u);          // half to even: p = 0.5 -> 0
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ce += __shfl_xor(ce, off);
        own = cf_wave_sum(own);
        if (lane == 0) {
            s_ce[wave] = ce;
            s_cnt[wave][3 * CF_SCORE_MAX_K + 0] = own & CF_SCORE_FIELD_MASK;
            s_cnt[wave][3 * CF_SCORE_MAX_K + 1] = (own >> CF_SCORE_FIELD) & CF_SCORE_FIELD_MASK;
            s_cnt[wave][3 * CF_SCORE_MAX_K + 2] = own >> (2 * CF_SCORE_FIELD);
        }
        for (int k = 0; k < K; ++k) {
            const double t = thresholds[k];
            unsigned called = 0;
#pragma unroll
            for (int j = 0; j < CF_SCORE_PER_THREAD; ++j) called += (double)p[j] >= t ? kind[j] : 0u;
            called = cf_wave_sum(called);
            if (lane == 0) {
                s_cnt[wave][3 * k + 0] = called & CF_SCORE_FIELD_MASK;                          // called
                s_cnt[wave][3 * k + 1] = (called >> CF_SCORE_FIELD) & CF_SCORE_FIELD_MASK;      // called, y == 1
                s_cnt[wave][3 * k + 2] = called >> (2 * CF_SCORE_FIELD);                        // called, y == 0
            }
        }
        __syncthreads();
        if (threadIdx.x < CF_SCORE_COUNTS) {
            unsigned v = 0;
#pragma unroll
            for (int w = 0; w < CF_SCORE_WAVES; ++w) v += s_cnt[w][threadIdx.x];
            s_tot[threadIdx.x] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double sum = s_ce[0];
#pragma unroll
            for (int w = 1; w < CF_SCORE_WAVES; ++w) sum += s_ce[w];
            if (slot0 + c < partial_slots) partials[slot0 + c] = sum;
            atomicAdd(&right_out[r], (unsigned long long)s_tot[3 * CF_SCORE_MAX_K + 2]);
        }
        if ((int)threadIdx.x < K) {
            const unsigned n_all = s_tot[3 * CF_SCORE_MAX_K + 0], n_y0 = s_tot[3 * CF_SCORE_MAX_K + 1];
            const unsigned called = s_tot[3 * threadIdx.x + 0], tp = s_tot[3 * threadIdx.x + 1], called_zero = s_tot[3 * threadIdx.x + 2];
            unsigned long long* out = counts_out + 4 * threadIdx.x;
            atomicAdd(out + 0, (unsigned long long)tp);                                        // called, y == 1
            atomicAdd(out + 1, (unsigned long long)(called - tp));                             // called, y != 1
            atomicAdd(out + 2, (unsigned long long)(n_y0 - called_zero));                      // not called, y == 0 (tails still in)
            atomicAdd(out + 3, (unsigned long long)((n_all - n_y0) - (called - called_zero))); // not called, y != 0
        }
        __syncthreads();                                   // the LDS tables are reused by this workgroup's next chunk
    }
}

// one thread per read: its chunks' partial sums, in chunk order
__global__ __launch_bounds__(256) void validation_score_finish_kernel(const int64_t* __restrict__ bounds, int64_t n,
                                                                      const double* __restrict__ partials, int64_t partial_slots,
                                                                      double* __restrict__ ce_sum_out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t b0 = bounds[r], size = bounds[r + 1] - b0;
    const int64_t n_chunks = (size + CF_SCORE_CHUNK - 1) / CF_SCORE_CHUNK;
    const int64_t slot0 = b0 / CF_SCORE_CHUNK + r;
    double sum = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c)
        if (slot0 + c < partial_slots) sum += partials[slot0 + c];
    ce_sum_out[r] = sum;
}

static unsigned validation_grid_height(int64_t longest, int64_t per_block) {
    const int64_t pieces = (longest + per_block - 1) / per_block;
    return (unsigned)std::min<int64_t>(std::max<int64_t>(pieces, 1), 65535);
}

extern "C" int cf_validation_score_chunk(void) { return CF_SCORE_CHUNK; }

extern "C" int cf_validation_gather(cf_model* m, const float* signal, const uint8_t* labels, int64_t signal_total, const int64_t* src_first,
                                    const int64_t* length, const int64_t* bounds, int64_t n, int64_t total, int64_t longest, float* x_out,
                                    uint8_t* y_out, void* stream) {
    if (!signal || !labels || !src_first || !length || !bounds || !x_out || !y_out) return fail(CF_ERR_INVALID, "cf_validation_gather: null argument");
    if (n <= 0 || n > 0x7fffffff) return fail(CF_ERR_INVALID, "cf_validation_gather: n must be in [1, 2^31)");
    if (signal_total < 0 || total < 0 || longest < 0 || longest > total) return fail(CF_ERR_INVALID, "cf_validation_gather: bad size");
    if (m) HIP_TRY(hipSetDevice(m->device));              // NULL: the calling thread's current device
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(validation_gather_kernel, dim3((unsigned)n, validation_grid_height(longest, 256 * 8)), dim3(256), 0, s, signal, labels,
                       signal_total, src_first, length, bounds, total, x_out, y_out);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_validation_score(cf_model* m, const float* probs, const float* logits, const uint8_t* y, const int64_t* bounds, int64_t n,
                                   int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds, int64_t* right_out,
                                   double* ce_sum_out, int64_t* counts_out, double* partials, int64_t partial_slots, void* stream) {
    if (!probs || !logits || !y || !bounds || !thresholds || !right_out || !ce_sum_out || !counts_out || !partials)
        return fail(CF_ERR_INVALID, "cf_validation_score: null argument");
    if (n <= 0 || n > 0x7fffffff) return fail(CF_ERR_INVALID, "cf_validation_score: n must be in [1, 2^31)");
    if (n_thresholds < 1 || n_thresholds > CF_SCORE_MAX_K)
        return fail(CF_ERR_INVALID, "cf_validation_score: between 1 and " + std::to_string(CF_SCORE_MAX_K) + " thresholds per call");
    if (total < 0 || longest < 0 || longest > total) return fail(CF_ERR_INVALID, "cf_validation_score: bad size");
    if (partial_slots < total / CF_SCORE_CHUNK + n)
        return fail(CF_ERR_INVALID, "cf_validation_score: partials needs total / " + std::to_string(CF_SCORE_CHUNK) + " + n slots");
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(right_out, 0, (size_t)n * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)n_thresholds * 4 * sizeof(int64_t), s));
    hipLaunchKernelGGL(validation_score_kernel, dim3((unsigned)n, validation_grid_height(longest, CF_SCORE_CHUNK)), dim3(CF_SCORE_THREADS), 0, s,
                       probs, logits, y, bounds, total, thresholds, (int)n_thresholds, reinterpret_cast<unsigned long long*>(right_out),
                       reinterpret_cast<unsigned long long*>(counts_out), partials, partial_slots);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(validation_score_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bounds, n, partials, partial_slots,
                       ce_sum_out);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
