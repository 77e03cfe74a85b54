// The bodies of retile_windows_kernel and vote_tilings_kernel (catfish_amd/csrc/tilings.hpp), serially, over the same rule header:
// the grid as loops over blockIdx.y, blockIdx.x and threadIdx.x, a 16-byte store as four assignments.  A stand-alone program for
// AddressSanitizer + UBSan; every buffer is malloc'ed at exactly the size the Python layer allocates, so an index formed wrongly is a
// report, not a wrong number.
//
//   tilings_replay CASE OUT
// CASE: int64 n_reads, total, n_phases, weight, has_logits, in_place, misalign; int32 phases[16];
//       then, unless the arguments are refused: int64 offsets[n_reads + 1], lengths[n_reads]; float base[total];
//       float probs_all[size]; float logits_all[size] when has_logits                      (size = tl_tiling_size)
// OUT:  int64 refusal (tl_refusal: 0 = the call would launch); unless refused: float retiled[size] -- the tiling regions filled with
//       -7777 before the walk --, float voted[total], float voted_logits[total] when has_logits
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../catfish_amd/csrc/tilings_rule.hpp"

template <class T>
static T* exactly(FILE* fh, int64_t n, int64_t lead = 0) {  // n values in a block of exactly (lead + n) * sizeof(T) bytes, behind `lead`
    T* p = static_cast<T*>(malloc((size_t)(lead + n) * sizeof(T)));
    if (n > 0 && (!p || fread(p + lead, sizeof(T), (size_t)n, fh) != (size_t)n)) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return p;
}

static void retile(float* x, const int64_t* offsets, const int64_t* lengths, int64_t n_reads, int64_t total, const tl_phases& ph, int aligned) {
    const int64_t region = tl_region(total, n_reads);
    if (ph.k == 1 || region == 0) return;
    const int64_t chunks = (region + 3 + TL_RETILE_CHUNK - 1) / TL_RETILE_CHUNK;
    for (int32_t by = 0; by < ph.k - 1; ++by)
        for (int64_t bx = 0; bx < chunks; ++bx)
            for (int tid = 0; tid < TL_THREADS; ++tid) {
                const int32_t j = by + 1;
                int32_t phi = 0;
                for (int32_t q = 1; q < TL_MAX_PHASES; ++q) phi = q == j ? ph.phi[q] : phi;
                const int64_t T = tl_tiling_start(j, total, n_reads);
                const int64_t a0 = aligned ? (T & ~(int64_t)3) : T;
                const int64_t A = a0 + bx * TL_RETILE_CHUNK;
                const int64_t first = A > T ? A - T : 0;
                const int64_t last = A + TL_RETILE_CHUNK - 1 - T < region - 1 ? A + TL_RETILE_CHUNK - 1 - T : region - 1;
                if (first > last) continue;
                const tl_range reads = tl_chunk_reads(offsets, n_reads, first, last, TL_WINDOW);
                tl_span span = {0, 0, 0, 0};
                for (int s = 0; s < TL_RETILE_CHUNK / (4 * TL_THREADS); ++s) {
                    const int64_t a = A + 4 * ((int64_t)s * TL_THREADS + tid);
                    float v[4];
                    bool in[4];
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
                        if (a % 4 != 0) { fprintf(stderr, "a 16-byte store at float %lld\n", (long long)a); exit(3); }
                        for (int e = 0; e < 4; ++e) x[a + e] = v[e];
                    } else {
                        for (int e = 0; e < 4; ++e)
                            if (in[e]) x[a + e] = v[e];
                    }
                }
            }
}

static void vote(const float* probs, const float* logits, const int64_t* offsets, const int64_t* lengths, int64_t n_reads, int64_t total,
                 const tl_phases& ph, int32_t weight, float* probs_out, float* logits_out) {
    if (total == 0) return;
    if (ph.k == 1) {
        if (probs_out != probs) memcpy(probs_out, probs, (size_t)total * sizeof(float));
        if (logits && logits_out != logits) memcpy(logits_out, logits, (size_t)total * sizeof(float));
        return;
    }
    const int64_t region = tl_region(total, n_reads), chunks = (total + TL_VOTE_CHUNK - 1) / TL_VOTE_CHUNK;
    for (int64_t bx = 0; bx < chunks; ++bx)
        for (int tid = 0; tid < TL_THREADS; ++tid) {
            const int64_t first = bx * TL_VOTE_CHUNK;
            const int64_t last = first + TL_VOTE_CHUNK - 1 < total - 1 ? first + TL_VOTE_CHUNK - 1 : total - 1;
            if (first > last) continue;
            const tl_range reads = tl_chunk_reads(offsets, n_reads, first, last, 0);
            for (int s = 0; s < TL_VOTE_CHUNK / TL_THREADS; ++s) {
                const int64_t b = first + (int64_t)s * TL_THREADS + tid;
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
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t head[7];
    int32_t phases[16];
    if (fread(head, sizeof(int64_t), 7, fh) != 7 || fread(phases, sizeof(int32_t), 16, fh) != 16) return 2;
    const int64_t n_reads = head[0], total = head[1];
    const int32_t n_phases = (int32_t)head[2], weight = (int32_t)head[3];
    const bool has_logits = head[4] != 0, in_place = head[5] != 0;
    const int64_t lead = head[6] ? 1 : 0;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int64_t refusal = tl_refusal(n_reads, total, phases, n_phases, weight);
    fwrite(&refusal, sizeof(int64_t), 1, out);
    if (refusal != 0) {
        fclose(out);
        fclose(fh);
        return 0;
    }
    tl_phases ph;
    ph.k = n_phases;
    for (int32_t j = 0; j < TL_MAX_PHASES; ++j) ph.phi[j] = j < n_phases ? phases[j] : 0;
    const int64_t size = tl_tiling_size(total, n_reads, n_phases);
    int64_t* offsets = exactly<int64_t>(fh, n_reads + 1);
    int64_t* lengths = exactly<int64_t>(fh, n_reads);
    float* x_block = static_cast<float*>(malloc((size_t)(lead + size) * sizeof(float)));       // malloc aligns to 16 bytes: lead 1 = a misaligned x
    float* x = x_block + lead;
    if (total > 0 && fread(x, sizeof(float), (size_t)total, fh) != (size_t)total) return 2;
    for (int64_t i = total; i < size; ++i) x[i] = -7777.f;
    float* probs = exactly<float>(fh, size);
    float* logits = has_logits ? exactly<float>(fh, size) : nullptr;
    fclose(fh);

    retile(x, offsets, lengths, n_reads, total, ph, lead == 0 ? 1 : 0);
    float* voted = in_place ? probs : static_cast<float*>(malloc((size_t)total * sizeof(float)));
    float* voted_logits = !has_logits ? nullptr : (in_place ? logits : static_cast<float*>(malloc((size_t)total * sizeof(float))));
    vote(probs, logits, offsets, lengths, n_reads, total, ph, weight, voted, voted_logits);

    fwrite(x, sizeof(float), (size_t)size, out);
    fwrite(voted, sizeof(float), (size_t)total, out);
    if (has_logits) fwrite(voted_logits, sizeof(float), (size_t)total, out);
    fclose(out);
    if (!in_place) { free(voted); free(voted_logits); }
    free(offsets); free(lengths); free(x_block); free(probs); free(logits);
    return 0;
}
