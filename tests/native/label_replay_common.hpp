// What label_events_replay.cpp and label_moves_replay.cpp share: reading a case file into blocks of exactly the size the Python layer
// allocates, and label_expand_kernel's body (catfish_amd/csrc/label_events.hpp), serially -- the grid as a loop over blockIdx.x, each
// stretch between two barriers as one loop over the threads, a 16-byte store as sixteen assignments behind a check of its address.
// The moves program hands it its compacted tables (bases = mbase, lengths = mlen), as the library does.
//
// The kernels' block scan (le_block_scan) is not replayed as such: it forms no address from its input, and its result is the sum of
// the threads before -- which the programs' `classes` / `merge` loops carry as a running sum.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../catfish_amd/csrc/label_events_rule.hpp"

template <class T>
static T* exactly(FILE* fh, int64_t n) {                    // n values in a block of exactly n * sizeof(T) bytes
    T* p = static_cast<T*>(malloc((size_t)n * sizeof(T)));
    if (n > 0 && (!p || fread(p, sizeof(T), (size_t)n, fh) != (size_t)n)) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return p;
}

struct run_words { uint32_t w[LE_RUN / 4]; };

static void store_run(uint8_t* out, const run_words& v, int valid, int32_t width) {
    if (valid == LE_RUN && width > 1) {
        if (reinterpret_cast<uintptr_t>(out) % (uintptr_t)width != 0) {
            fprintf(stderr, "a %d-byte store at an address that is not a multiple of it\n", width);
            exit(3);
        }
        for (int q = 0; q < LE_RUN; ++q) out[q] = (uint8_t)(v.w[q / 4] >> (8 * (q % 4)));
    } else {
        for (int q = 0; q < LE_RUN; ++q)
            if (q < valid) out[q] = (uint8_t)(v.w[q / 4] >> (8 * (q % 4)));
    }
}

static void expand(const uint8_t* bases, const int32_t* lengths, const int64_t* event_offsets, const int64_t* sample_offsets, int64_t n_reads,
                   int64_t n_events, int64_t total, const int32_t* start, const uint8_t* cls, uint8_t* labels_out, uint8_t* basemap_out) {
    const int64_t grid = n_reads + total / LE_TILE;
    int32_t* s_start = static_cast<int32_t*>(malloc((LE_TILE_EVENTS + 1) * sizeof(int32_t)));
    uint8_t* s_cls = static_cast<uint8_t*>(malloc(LE_TILE_EVENTS));
    uint8_t* s_base = static_cast<uint8_t*>(malloc(LE_TILE_EVENTS));
    for (int64_t b = 0; b < grid; ++b) {
        const int64_t r = le_block_read(sample_offsets, n_reads, b);
        if (r < 0) continue;
        const le_tile tile = le_tile_of(b, r, sample_offsets[r], sample_offsets[r + 1], total);
        if (tile.t0 >= tile.t1) continue;
        const le_events ev = le_events_sound(event_offsets[r], event_offsets[r + 1], n_events);
        const int32_t* start_r = start + ev.first;
        const int64_t f = le_first_event(start_r, ev.n, tile.t0);
        const int32_t m = le_staged_events(f, ev.n);
        for (int tid = 0; tid < LE_THREADS; ++tid) {
            for (int32_t i = tid; i < m; i += LE_THREADS) {
                s_start[i] = start_r[f + i];
                s_cls[i] = cls[ev.first + f + i];
                s_base[i] = bases[ev.first + f + i];
            }
            if (tid == 0 && m > 0) s_start[m] = le_staged_end(start_r, lengths + ev.first, f, m, ev.n);
        }
        for (int tid = 0; tid < LE_THREADS; ++tid) {
            const int64_t j0 = tile.t0 + (int64_t)LE_RUN * tid;
            if (j0 >= tile.t1) continue;
            const int valid = tile.t1 - j0 < LE_RUN ? (int)(tile.t1 - j0) : LE_RUN;
            int32_t i = le_staged_first(s_start, m, j0);
            run_words lab, map;
            for (int q = 0; q < LE_RUN / 4; ++q) lab.w[q] = map.w[q] = 0;
            for (int q = 0; q < LE_RUN; ++q) {
                if (q < valid) {
                    const int32_t c = le_covering(s_start, m, &i, j0 + q);
                    if (c >= 0) {
                        lab.w[q / 4] |= (uint32_t)s_cls[c] << (8 * (q % 4));
                        map.w[q / 4] |= (uint32_t)le_base_byte(s_start, s_base, c, j0 + q) << (8 * (q % 4));
                    }
                }
            }
            uint8_t* lab_at = labels_out + tile.first;
            store_run(lab_at + j0, lab, valid, le_store_width(reinterpret_cast<uintptr_t>(lab_at)));
            if (basemap_out) {
                uint8_t* map_at = basemap_out + tile.first;
                store_run(map_at + j0, map, valid, le_store_width(reinterpret_cast<uintptr_t>(map_at)));
            }
        }
    }
    free(s_start);
    free(s_cls);
    free(s_base);
}
