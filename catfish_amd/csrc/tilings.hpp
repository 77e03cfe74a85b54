// Shifted-window voting (catfish_amd/tilings.py states both steps in numpy -- retile_host and vote_host are the definitions; every
// index rule is in csrc/tilings_rule.hpp and is replayed on the CPU under the sanitizers by tests/native/tilings_replay.cpp).
//
//   retile   one launch fills tilings 1 .. K - 1 of the one buffer completely, zeros included: blockIdx.y = tiling - 1, blockIdx.x =
//            a chunk of TL_RETILE_CHUNK destination samples.  The workgroup finds the reads its chunk touches once (two binary
//            searches on values that depend on blockIdx only: scalar loads), a thread then owns 16-byte groups at ABSOLUTE multiples
//            of four floats, so the stores are full dwordx4 wherever a group lies inside one tiling; the up to three samples at a
//            tiling's edges go out as dwords.  The loads are the base region shifted by phi_j: consecutive lanes, consecutive dwords.
//   vote     grid over base samples in chunks of TL_VOTE_CHUNK; a thread loads a sample's K values, sums in double in the order
//            j = 0 .. K - 1 and stores once.  It reads values[b] before it writes out[b] and touches no other base sample, so
//            out == values is safe.
//
// Streaming kernels: HBM-bound (MI355X_MICROARCH: 8 TB/s peak, ~5 measured for plain copies), no LDS, no atomics, no scratch.
#pragma once
#include "tilings_rule.hpp"

__global__ __launch_bounds__(TL_THREADS) void retile_windows_kernel(float* x, const int64_t* __restrict__ offsets,
                                                                    const int64_t* __restrict__ lengths, int64_t n_reads, int64_t total,
                                                                    tl_phases ph, int aligned) {
    const int32_t j = (int32_t)blockIdx.y + 1;
    int32_t phi = 0;
#pragma unroll
    for (int32_t q = 1; q < TL_MAX_PHASES; ++q) phi = q == j ? ph.phi[q] : phi;
    const int64_t region = tl_region(total, n_reads), T = tl_tiling_start(j, total, n_reads);
    const int64_t a0 = aligned ? (T & ~(int64_t)3) : T;                       // absolute index of this tiling's first group
    const int64_t A = a0 + (int64_t)blockIdx.x * TL_RETILE_CHUNK;
    const int64_t first = A > T ? A - T : 0;
    const int64_t last = A + TL_RETILE_CHUNK - 1 - T < region - 1 ? A + TL_RETILE_CHUNK - 1 - T : region - 1;
    if (first > last) return;
    const tl_range reads = tl_chunk_reads(offsets, n_reads, first, last, TL_WINDOW);
    tl_span span = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < TL_RETILE_CHUNK / (4 * TL_THREADS); ++s) {
        const int64_t a = A + 4 * ((int64_t)s * TL_THREADS + threadIdx.x);
        float v[4];
        bool in[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t u = a + e - T;
            in[e] = u >= 0 && u < region;
            v[e] = 0.0f;
            if (in[e]) {
                if (u < span.g0 || u >= span.g1) span = tl_locate(offsets, lengths, total, reads, u);
                const int64_t src = tl_source(span, phi, u);
                if (src >= 0) v[e] = x[src];
            }
        }
        if (aligned && in[0] && in[3]) {
            *reinterpret_cast<float4*>(x + a) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (in[e]) x[a + e] = v[e];
        }
    }
}

__global__ __launch_bounds__(TL_THREADS) void vote_tilings_kernel(const float* probs, const float* logits, const int64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ lengths, int64_t n_reads, int64_t total,
                                                                  tl_phases ph, int32_t weight, float* probs_out, float* logits_out) {
    const int64_t region = tl_region(total, n_reads);
    const int64_t first = (int64_t)blockIdx.x * TL_VOTE_CHUNK;
    const int64_t last = first + TL_VOTE_CHUNK - 1 < total - 1 ? first + TL_VOTE_CHUNK - 1 : total - 1;
    if (first > last) return;
    const tl_range reads = tl_chunk_reads(offsets, n_reads, first, last, 0);
#pragma unroll
    for (int s = 0; s < TL_VOTE_CHUNK / TL_THREADS; ++s) {
        const int64_t b = first + (int64_t)s * TL_THREADS + threadIdx.x;
        if (b > last) continue;
        const tl_voter v = tl_vote_where(offsets, lengths, total, reads, b);
        const float p = v.votes ? tl_vote_value(probs, ph, weight, total, region, b, v) : probs[b];
        probs_out[b] = p;
        if (logits) {
            const float z = v.votes ? tl_vote_value(logits, ph, weight, total, region, b, v) : logits[b];
            logits_out[b] = z;
        }
    }
}

static int tilings_check(const char* who, int64_t n_reads, int64_t total, const int32_t* phases, int32_t n_phases, int32_t weight) {
    switch (tl_refusal(n_reads, total, phases, n_phases, weight)) {
        case 0: return CF_OK;
        case 1: return fail(CF_ERR_INVALID, std::string(who) + ": negative size");
        case 2: return fail(CF_ERR_INVALID, std::string(who) + ": at most 2^31 - 1 reads and 2^40 samples per call");
        case 3: return fail(CF_ERR_INVALID, std::string(who) + ": total must be a multiple of 35");
        case 4: return fail(CF_ERR_INVALID, std::string(who) + ": phases must be 1..8 strictly ascending ints in 0..34, the first one 0");
        default: return fail(CF_ERR_INVALID, std::string(who) + ": weight must be 0 (mean) or 1 (centre)");
    }
}

static tl_phases tilings_pack(const int32_t* phases, int32_t n_phases) {
    tl_phases ph;
    ph.k = n_phases;
    for (int32_t j = 0; j < TL_MAX_PHASES; ++j) ph.phi[j] = j < n_phases ? phases[j] : 0;
    return ph;
}

extern "C" int cf_retile_windows(cf_model* m, float* x, const int64_t* offsets, const int64_t* lengths, int64_t n_reads, int64_t total,
                                 const int32_t* phases, int32_t n_phases, void* stream) {
    if (!x || !offsets || !phases || (!lengths && n_reads > 0)) return fail(CF_ERR_INVALID, "cf_retile_windows: null argument");
    const int rc = tilings_check("cf_retile_windows", n_reads, total, phases, n_phases, 0);
    if (rc != CF_OK) return rc;
    const int64_t region = tl_region(total, n_reads);
    if (n_phases == 1 || region == 0) return CF_OK;
    if (m) HIP_TRY(hipSetDevice(m->device));              // NULL: the calling thread's current device
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int aligned = (reinterpret_cast<uintptr_t>(x) & 15u) == 0 ? 1 : 0;
    const int64_t chunks = (region + 3 + TL_RETILE_CHUNK - 1) / TL_RETILE_CHUNK;      // a tiling may begin up to 3 floats into its first group
    hipLaunchKernelGGL(retile_windows_kernel, dim3((unsigned)chunks, (unsigned)(n_phases - 1)), dim3(TL_THREADS), 0, s, x, offsets, lengths,
                       n_reads, total, tilings_pack(phases, n_phases), aligned);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}

extern "C" int cf_vote_tilings(cf_model* m, const float* probs, const float* logits, const int64_t* offsets, const int64_t* lengths,
                               int64_t n_reads, int64_t total, const int32_t* phases, int32_t n_phases, int32_t weight, float* probs_out,
                               float* logits_out, void* stream) {
    if (!probs || !probs_out || !offsets || !phases || (!lengths && n_reads > 0)) return fail(CF_ERR_INVALID, "cf_vote_tilings: null argument");
    if ((logits == nullptr) != (logits_out == nullptr)) return fail(CF_ERR_INVALID, "cf_vote_tilings: logits_out must be NULL exactly when logits is");
    const int rc = tilings_check("cf_vote_tilings", n_reads, total, phases, n_phases, weight);
    if (rc != CF_OK) return rc;
    if (total == 0) return CF_OK;
    if (m) HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n_phases == 1) {                                  // the output is the input, bit for bit
        if (probs_out != probs) HIP_TRY(hipMemcpyAsync(probs_out, probs, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (logits && logits_out != logits) HIP_TRY(hipMemcpyAsync(logits_out, logits, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, s));
        return CF_OK;
    }
    const int64_t chunks = (total + TL_VOTE_CHUNK - 1) / TL_VOTE_CHUNK;
    hipLaunchKernelGGL(vote_tilings_kernel, dim3((unsigned)chunks), dim3(TL_THREADS), 0, s, probs, logits, offsets, lengths, n_reads, total,
                       tilings_pack(phases, n_phases), weight, probs_out, logits_out);
    HIP_TRY(hipGetLastError());
    return CF_OK;
}
