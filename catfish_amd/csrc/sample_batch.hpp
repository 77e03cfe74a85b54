// Device-resident training set: the next balanced batch is drawn and gathered on the card, inside the captured step
// (catfish_amd/device_db.py states the sampler on the host -- DeviceExampleDb.batch_indices is normative, this file reproduces it
// exactly; the reference's sampler is ExampleDb.get_training_set, networks/trainingDB/ExampleDb.py:57-83).
//
//   base = fmix(seed ^ fmix(draw * 0x85ebca6b))
//   rank = P(slot, size, base ^ 1)                              the shuffle over the batch's slots
//   row  = rank < size / ratio ? P(rank, n_pos, base ^ 2)       distinct positives
//                              : P(rank - size / ratio, n_neg, base ^ 3)      distinct negatives
//
// P(i, n, key) is a keyed bijection of [0, n): a balanced four-round Feistel network over 2^b >= n (b even, at least 2) with the
// murmur3 finaliser as round function, walked until the value is below n.  Every slot is evaluated on its own: no state, no
// atomics, no communication; distinct rows follow from bijectivity.
//
// One wave per slot (the permutation is wave-uniform: scalar registers and a uniform walk), lanes 0..34 move the window's 35
// samples and write its 35 labels with dword accesses (rows are 140 bytes: not 16-byte aligned).
#pragma once

#define CF_SAMPLE_ROUNDS 4

__device__ __forceinline__ uint32_t cf_perm(uint32_t i, uint32_t n, uint32_t key) {
    uint32_t b = n > 1u ? 32u - (uint32_t)__clz(n - 1u) : 0u;
    b = b < 2u ? 2u : b;
    b += b & 1u;
    const uint32_t half = b >> 1, mask = (1u << half) - 1u;
    uint32_t k[CF_SAMPLE_ROUNDS];
#pragma unroll
    for (int r = 0; r < CF_SAMPLE_ROUNDS; ++r) k[r] = cf_fmix32(key + (uint32_t)(r + 1) * 0x9E3779B9u);
    uint32_t v = i;
    do {                                                  // cycle walk: v stays inside [0, 2^b), so the walk returns to [0, n)
        uint32_t L = v >> half, R = v & mask;
#pragma unroll
        for (int r = 0; r < CF_SAMPLE_ROUNDS; ++r) {
            const uint32_t t = L ^ (cf_fmix32(R ^ k[r]) & mask);
            L = R;
            R = t;
        }
        v = (L << half) | R;
    } while (v >= n);
    return v;
}

__global__ __launch_bounds__(256) void sample_batch_kernel(const float* __restrict__ pos, uint32_t n_pos, const float* __restrict__ neg,
                                                           uint32_t n_neg, uint32_t size, uint32_t n_draw_pos, uint32_t seed,
                                                           const int64_t* __restrict__ draw_counter, float* __restrict__ x,
                                                           float* __restrict__ y) {
    const uint32_t slot = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (slot >= size) return;
    const uint32_t draw = (uint32_t)draw_counter[0];
    const uint32_t base = cf_fmix32(seed ^ cf_fmix32(draw * 0x85ebca6bu));
    const uint32_t rank = cf_perm(slot, size, base ^ 1u);
    const bool is_pos = rank < n_draw_pos;
    const uint32_t row = is_pos ? cf_perm(rank, n_pos, base ^ 2u) : cf_perm(rank - n_draw_pos, n_neg, base ^ 3u);
    if (lane < CF_T) {
        const float* src = (is_pos ? pos : neg) + (size_t)row * CF_T;
        x[(size_t)slot * CF_T + lane] = src[lane];
        y[(size_t)slot * CF_T + lane] = is_pos ? 1.0f : 0.0f;
    }
}

// after every sampling workgroup has read the counter (stream order): one thread moves it on.  With a loss log it also files the
// loss of the step BEFORE this draw (prev_loss[0] still holds it) under log[*log_pos - 1] and moves log_pos on: a chain of replayed
// steps keeps its losses on the card without a launch of its own; the last step's loss is read from prev_loss itself.
__global__ void sample_advance_kernel(int64_t* draw_counter, const float* __restrict__ prev_loss, float* __restrict__ log, int64_t capacity,
                                      int64_t* log_pos) {
    draw_counter[0] += 1;
    if (log) {
        const int64_t p = log_pos[0];
        if (p >= 1 && p <= capacity) log[p - 1] = prev_loss[0];
        log_pos[0] = p + 1;
    }
}

static int sample_batch_launch(const char* who, cf_model* m, const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int64_t size,
                               int32_t ratio, uint32_t seed, int64_t* draw_counter, float* x, float* y, const float* prev_loss, float* log,
                               int64_t capacity, int64_t* log_pos, void* stream) {
    const std::string w(who);
    if (!draw_counter || !x || !y) return fail(CF_ERR_INVALID, w + ": null argument");
    if (size <= 0 || size > 0x7fffffff || ratio <= 0) return fail(CF_ERR_INVALID, w + ": size and ratio must be positive");
    if (n_pos < 0 || n_neg < 0 || n_pos > 0x7fffffff || n_neg > 0x7fffffff) return fail(CF_ERR_INVALID, w + ": bad pool size");
    const int64_t k_pos = size / ratio, k_neg = size - k_pos;
    if (k_pos > n_pos || k_neg > n_neg) return fail(CF_ERR_INVALID, w + ": a pool is smaller than its share of the batch");
    if ((k_pos > 0 && !pos) || (k_neg > 0 && !neg)) return fail(CF_ERR_INVALID, w + ": null pool");
    if (log && (!prev_loss || !log_pos || capacity <= 0)) return fail(CF_ERR_INVALID, w + ": a loss log needs prev_loss, log_pos and a capacity");
    if (m) HIP_TRY(hipSetDevice(m->device));              // NULL: the calling thread's current device
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sample_batch_kernel, dim3((unsigned)((size + 3) / 4)), dim3(256), 0, s, pos, (uint32_t)n_pos, neg, (uint32_t)n_neg,
                       (uint32_t)size, (uint32_t)k_pos, seed, draw_counter, x, y);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, s, draw_counter, prev_loss, log, capacity, log_pos);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_sample_batch(cf_model* m, const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int64_t size, int32_t ratio,
                               uint32_t seed, int64_t* draw_counter, float* x, float* y, void* stream) {
    return sample_batch_launch("cf_sample_batch", m, pos, n_pos, neg, n_neg, size, ratio, seed, draw_counter, x, y, nullptr, nullptr, 0, nullptr,
                               stream);
}

extern "C" int cf_sample_batch_logged(cf_model* m, const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int64_t size, int32_t ratio,
                                      uint32_t seed, int64_t* draw_counter, float* x, float* y, const float* prev_loss, float* log,
                                      int64_t capacity, int64_t* log_pos, void* stream) {
    if (!log) return fail(CF_ERR_INVALID, "cf_sample_batch_logged: null log");
    return sample_batch_launch("cf_sample_batch_logged", m, pos, n_pos, neg, n_neg, size, ratio, seed, draw_counter, x, y, prev_loss, log, capacity,
                               log_pos, stream);
}
