// The bodies of label_moves_merge_kernel and label_moves_classes_kernel (catfish_amd/csrc/label_moves.hpp) and of the
// label_expand_kernel they hand their tables to (csrc/label_events.hpp), serially, over the same rule headers: the grids as loops
// over blockIdx.x and threadIdx.x, each stretch between two barriers as one loop over the threads, a block scan as a running sum, a
// 16-byte store as sixteen assignments behind a check of its address.  A stand-alone program for AddressSanitizer + UBSan; every
// buffer is malloc'ed at exactly the size the Python layer allocates, so an index formed wrongly is a report, not a wrong number.
// The expansion (over the compacted tables: bases = mbase, lengths = mlen) and the case-file reading are label_replay_common.hpp's.
//
//   label_moves_replay CASE OUT
// CASE: int64 n_reads, n_events, total, k, has_basemap, lead (bytes the outputs sit behind a 16-byte boundary), work_bytes (-1: what
//       the library's query answers), lengths_f64; then, unless the arguments are refused: int64 event_offsets[n_reads + 1],
//       sample_offsets[n_reads + 1], n_raw[n_reads]; int32 clipped[2 n_reads], moves[n_events]; float or double lengths[n_events];
//       uint8 states[n_events * k]
// OUT:  int64 refusal (lm_refusal: 0 = the call would launch); unless refused: uint8 labels[total], basemap[total] when has_basemap
//       -- both filled with 0xEE before the walk -- and int32 counts[2 n_reads] (M and final per read; 0xEE bytes when total == 0)
#include "../../catfish_amd/csrc/label_moves_rule.hpp"
#include "label_replay_common.hpp"

static int64_t merged_count(const float* lengths_r, int64_t h, int64_t end) { return lm_merged_count_f(lengths_r, h, end); }
static int64_t merged_count(const double* lengths_r, int64_t h, int64_t end) { return lm_merged_count_d(lengths_r, h, end); }

template <class T>
static void merge(const uint8_t* states, const T* lengths, const int32_t* moves, const int64_t* event_offsets, int64_t n_reads, int64_t n_events,
                  int32_t k, int32_t* mlen, uint8_t* mbase, uint8_t* uniform, int32_t* counts) {
    const int64_t grid = n_reads < LM_GRID ? n_reads : LM_GRID;
    for (int64_t bx = 0; bx < grid; ++bx)
        for (int64_t r = bx; r < n_reads; r += grid) {
            const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
            const int32_t* moves_r = moves + ev.first;
            const T* lengths_r = lengths + ev.first;
            int64_t carry = 0;
            for (int64_t p0 = 0; p0 < ev.n; p0 += LM_PIECE) {
                int64_t scanned = 0;                            // the exclusive block scan at this thread
                for (int tid = 0; tid < LM_THREADS; ++tid) {
                    uint32_t heads = 0;
                    for (int q = 0; q < LM_PER_THREAD; ++q)
                        heads |= (lm_is_head(moves_r, p0 + LM_PER_THREAD * tid + q, ev.n) ? 1u : 0u) << q;
                    int64_t j = carry + scanned;
                    for (int q = 0; q < LM_PER_THREAD; ++q) {
                        if (!((heads >> q) & 1u)) continue;
                        const int64_t h = p0 + LM_PER_THREAD * tid + q;
                        const int64_t slot = lm_merged_slot(j, ev.n);
                        if (slot >= 0) {
                            const uint8_t* state = states + (ev.first + h) * k;
                            mlen[ev.first + slot] = (int32_t)merged_count(lengths_r, h, lm_stays_end(moves_r, h, ev.n));
                            uniform[ev.first + slot] = lm_uniform(state, k);
                            mbase[ev.first + slot] = state[k / 2];
                        }
                        ++j;
                    }
                    scanned += __builtin_popcount(heads);
                }
                carry += scanned;
            }
            for (int tid = 0; tid < LM_THREADS; ++tid)
                for (int64_t slot = carry + tid; slot < ev.n; slot += LM_THREADS) {
                    mlen[ev.first + slot] = 0;
                    uniform[ev.first + slot] = 0;
                    mbase[ev.first + slot] = 0;
                }
            counts[2 * r] = (int32_t)carry;
        }
}

static void classes(const int64_t* event_offsets, const int32_t* clipped, const int64_t* n_raw, int64_t n_reads, int64_t n_events,
                    const int32_t* mlen, const uint8_t* uniform, int32_t* start, uint8_t* cls, int32_t* counts) {
    const int64_t grid = n_reads < LM_GRID ? n_reads : LM_GRID;
    uint8_t* s_cores = static_cast<uint8_t*>(malloc(LM_CORE_SLOTS));
    for (int64_t bx = 0; bx < grid; ++bx)
        for (int64_t r = bx; r < n_reads; r += grid) {
            const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
            const int64_t m = lm_merged_sound(counts[2 * r], ev.n);
            const int64_t cs = clipped[2 * r], ce = clipped[2 * r + 1];
            const uint8_t* uniform_r = uniform + ev.first;
            int64_t carry = 0;
            for (int64_t p0 = 0; p0 < ev.n; p0 += LM_PIECE) {
                for (int tid = 0; tid < LM_THREADS; ++tid)
                    for (int slot = tid; slot < LM_CORE_SLOTS; slot += LM_THREADS) {
                        const int64_t j = p0 - LM_WIDEN + slot;
                        s_cores[slot] = lm_core_slot(j, p0, m) >= 0 ? lm_core(uniform_r, j, m, cs, ce) : 0;
                    }
                int64_t scanned = 0;
                for (int tid = 0; tid < LM_THREADS; ++tid) {
                    int64_t before[LM_PER_THREAD], sum = 0;
                    for (int q = 0; q < LM_PER_THREAD; ++q) {
                        const int64_t e = p0 + LM_PER_THREAD * tid + q;
                        before[q] = sum;
                        sum += e < ev.n ? le_len(mlen[ev.first + e]) : 0;
                    }
                    const int64_t mine = carry + scanned;
                    for (int q = 0; q < LM_PER_THREAD; ++q) {
                        const int64_t e = p0 + LM_PER_THREAD * tid + q;
                        if (e < ev.n) {
                            start[ev.first + e] = (int32_t)le_sat(mine + before[q]);
                            cls[ev.first + e] = lm_class(s_cores, e, p0, m);
                        }
                    }
                    scanned += sum;
                }
                carry = le_sat(carry + scanned);
            }
            counts[2 * r + 1] = lm_final(carry, n_raw[r]);
        }
    free(s_cores);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t head[8];
    if (fread(head, sizeof(int64_t), 8, fh) != 8) return 2;
    const int64_t n_reads = head[0], n_events = head[1], total = head[2];
    const int32_t k = (int32_t)head[3];
    const bool has_basemap = head[4] != 0;
    const int64_t lead = head[5] & 15;
    const int64_t work_bytes = head[6] < 0 ? lm_work_bytes(n_reads, n_events) : head[6];
    const int32_t lengths_f64 = (int32_t)head[7];
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int64_t refusal = head[3] != k ? 3 : head[7] != lengths_f64 ? 6 : lm_refusal(n_reads, n_events, total, k, lengths_f64, work_bytes);
    fwrite(&refusal, sizeof(int64_t), 1, out);
    if (refusal != 0) {
        fclose(out);
        fclose(fh);
        return 0;
    }
    int64_t* event_offsets = exactly<int64_t>(fh, n_reads + 1);
    int64_t* sample_offsets = exactly<int64_t>(fh, n_reads + 1);
    int64_t* n_raw = exactly<int64_t>(fh, n_reads);
    int32_t* clipped = exactly<int32_t>(fh, 2 * n_reads);
    int32_t* moves = exactly<int32_t>(fh, n_events);
    float* lengths_f = lengths_f64 ? nullptr : exactly<float>(fh, n_events);
    double* lengths_d = lengths_f64 ? exactly<double>(fh, n_events) : nullptr;
    uint8_t* states = exactly<uint8_t>(fh, n_events * k);
    fclose(fh);
    // malloc aligns to 16 bytes: `lead` bytes in, the outputs are misaligned by that much
    uint8_t* labels_block = static_cast<uint8_t*>(malloc((size_t)(lead + total)));
    uint8_t* basemap_block = has_basemap ? static_cast<uint8_t*>(malloc((size_t)(lead + total))) : nullptr;
    uint8_t* labels = labels_block + lead;
    uint8_t* basemap = has_basemap ? basemap_block + lead : nullptr;
    memset(labels_block, 0xEE, (size_t)(lead + total));
    if (has_basemap) memset(basemap_block, 0xEE, (size_t)(lead + total));
    uint8_t* work = static_cast<uint8_t*>(malloc((size_t)work_bytes));
    memset(work, 0xEE, (size_t)work_bytes);
    int32_t* counts = reinterpret_cast<int32_t*>(work + lm_work_counts(n_reads, n_events));
    if (total > 0 && n_reads > 0) {
        int32_t* mlen = reinterpret_cast<int32_t*>(work + lm_work_mlen(n_reads, n_events));
        int32_t* start = reinterpret_cast<int32_t*>(work + lm_work_start(n_reads, n_events));
        uint8_t* cls = work + lm_work_cls(n_reads, n_events);
        uint8_t* mbase = work + lm_work_mbase(n_reads, n_events);
        uint8_t* uniform = work + lm_work_uniform(n_reads, n_events);
        if (lengths_f64) merge(states, lengths_d, moves, event_offsets, n_reads, n_events, k, mlen, mbase, uniform, counts);
        else merge(states, lengths_f, moves, event_offsets, n_reads, n_events, k, mlen, mbase, uniform, counts);
        classes(event_offsets, clipped, n_raw, n_reads, n_events, mlen, uniform, start, cls, counts);
        expand(mbase, mlen, event_offsets, sample_offsets, n_reads, n_events, total, start, cls, labels, basemap);
    }
    fwrite(labels, 1, (size_t)total, out);
    if (has_basemap) fwrite(basemap, 1, (size_t)total, out);
    fwrite(counts, sizeof(int32_t), (size_t)(2 * n_reads), out);
    fclose(out);
    free(event_offsets); free(sample_offsets); free(n_raw); free(clipped); free(moves); free(lengths_f); free(lengths_d); free(states);
    free(labels_block); free(basemap_block); free(work);
    return 0;
}
