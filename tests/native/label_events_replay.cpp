// The bodies of label_event_classes_kernel and label_expand_kernel (catfish_amd/csrc/label_events.hpp), serially, over the same rule
// header: the grids as loops over blockIdx.x and threadIdx.x, each stretch between two barriers as one loop over the threads, the
// block scan as a running sum, a 16-byte store as sixteen assignments behind a check of its address.  A stand-alone program for
// AddressSanitizer + UBSan; every buffer is malloc'ed at exactly the size the Python layer allocates, so an index formed wrongly is a
// report, not a wrong number.  The expansion and the case-file reading are label_replay_common.hpp's, shared with the moves program.
//
//   label_events_replay CASE OUT
// CASE: int64 n_reads, n_events, total, kmer, has_basemap, lead (bytes the outputs sit behind a 16-byte boundary), work_bytes (-1: what
//       the library's query answers), 0; then, unless the arguments are refused: int64 event_offsets[n_reads + 1],
//       sample_offsets[n_reads + 1]; int32 clipped[2 n_reads], lengths[n_events]; uint8 bases[n_events]
// OUT:  int64 refusal (le_refusal: 0 = the call would launch); unless refused: uint8 labels[total], and basemap[total] when has_basemap
//       -- both filled with 0xEE before the walk
#include "label_replay_common.hpp"

static void classes(const uint8_t* bases, const int32_t* lengths, const int64_t* event_offsets, const int32_t* clipped, int64_t n_reads,
                    int64_t n_events, int32_t kmer, int32_t* start, uint8_t* cls) {
    const int64_t grid = n_reads < LE_CLASS_GRID ? n_reads : LE_CLASS_GRID;
    uint8_t* s_bases = static_cast<uint8_t*>(malloc(LE_BASES_SLOTS));
    uint8_t* s_cores = static_cast<uint8_t*>(malloc(LE_CORE_SLOTS));
    for (int64_t bx = 0; bx < grid; ++bx)
        for (int64_t r = bx; r < n_reads; r += grid) {
            const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
            const int64_t cs = clipped[2 * r], ce = clipped[2 * r + 1];
            int64_t carry = 0;
            for (int64_t p0 = 0; p0 < ev.n; p0 += LE_PIECE) {
                for (int tid = 0; tid < LE_THREADS; ++tid)
                    for (int slot = tid; slot < LE_BASES_SLOTS; slot += LE_THREADS) {
                        const int64_t e = p0 - LE_HALO + slot;
                        if (le_base_slot(e, p0, ev.n) >= 0) s_bases[slot] = bases[ev.first + e];
                    }
                for (int tid = 0; tid < LE_THREADS; ++tid)
                    for (int slot = tid; slot < LE_CORE_SLOTS; slot += LE_THREADS) {
                        const int64_t e = p0 - LE_WIDEN + slot;
                        s_cores[slot] = le_core_slot(e, p0, ev.n) >= 0 ? le_core(s_bases, e, p0, ev.n, cs, ce, kmer) : 0;
                    }
                int64_t scanned = 0;                            // the exclusive block scan at this thread
                for (int tid = 0; tid < LE_THREADS; ++tid) {
                    int64_t before[LE_PER_THREAD], sum = 0;
                    for (int q = 0; q < LE_PER_THREAD; ++q) {
                        const int64_t e = p0 + LE_PER_THREAD * tid + q;
                        before[q] = sum;
                        sum += e < ev.n ? le_len(lengths[ev.first + e]) : 0;
                    }
                    const int64_t mine = carry + scanned;
                    for (int q = 0; q < LE_PER_THREAD; ++q) {
                        const int64_t e = p0 + LE_PER_THREAD * tid + q;
                        if (e < ev.n) {
                            start[ev.first + e] = (int32_t)le_sat(mine + before[q]);
                            cls[ev.first + e] = le_class(s_cores, e, p0, ev.n);
                        }
                    }
                    scanned += sum;
                }
                carry = le_sat(carry + scanned);
            }
        }
    free(s_bases);
    free(s_cores);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int64_t head[8];
    if (fread(head, sizeof(int64_t), 8, fh) != 8) return 2;
    const int64_t n_reads = head[0], n_events = head[1], total = head[2];
    const int32_t kmer = (int32_t)head[3];
    const bool has_basemap = head[4] != 0;
    const int64_t lead = head[5] & 15;
    const int64_t work_bytes = head[6] < 0 ? le_work_bytes(n_events) : head[6];
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int64_t refusal = head[3] != kmer ? 3 : le_refusal(n_reads, n_events, total, kmer, work_bytes);
    fwrite(&refusal, sizeof(int64_t), 1, out);
    if (refusal != 0) {
        fclose(out);
        fclose(fh);
        return 0;
    }
    int64_t* event_offsets = exactly<int64_t>(fh, n_reads + 1);
    int64_t* sample_offsets = exactly<int64_t>(fh, n_reads + 1);
    int32_t* clipped = exactly<int32_t>(fh, 2 * n_reads);
    int32_t* lengths = exactly<int32_t>(fh, n_events);
    uint8_t* bases = exactly<uint8_t>(fh, n_events);
    fclose(fh);
    // malloc aligns to 16 bytes: `lead` bytes in, the outputs are misaligned by that much
    uint8_t* labels_block = static_cast<uint8_t*>(malloc((size_t)(lead + total)));
    uint8_t* basemap_block = has_basemap ? static_cast<uint8_t*>(malloc((size_t)(lead + total))) : nullptr;
    uint8_t* labels = labels_block + lead;
    uint8_t* basemap = has_basemap ? basemap_block + lead : nullptr;
    memset(labels_block, 0xEE, (size_t)(lead + total));
    if (has_basemap) memset(basemap_block, 0xEE, (size_t)(lead + total));
    uint8_t* work = static_cast<uint8_t*>(malloc((size_t)work_bytes));
    if (total > 0 && n_reads > 0) {
        int32_t* start = reinterpret_cast<int32_t*>(work);
        uint8_t* cls = work + 4 * n_events;
        classes(bases, lengths, event_offsets, clipped, n_reads, n_events, kmer, start, cls);
        expand(bases, lengths, event_offsets, sample_offsets, n_reads, n_events, total, start, cls, labels, basemap);
    }
    fwrite(labels, 1, (size_t)total, out);
    if (has_basemap) fwrite(basemap, 1, (size_t)total, out);
    fclose(out);
    free(event_offsets); free(sample_offsets); free(clipped); free(lengths); free(bases);
    free(labels_block); free(basemap_block); free(work);
    return 0;
}
