#!/usr/bin/env python3
"""Labels from a basecaller's move table: the card route (``labelling.label_moves`` -> ``cf_label_moves``) against the host route
(``MoveBatch.label_host``) on the same tables, with ``cf_label_events`` on the merged events as the yardstick.

    python tools/bench_label_moves.py [--reads 856] [--length 20000] [--rounds 7] [--f64]

The batch is ``--reads`` reads of ``labelling.synthetic_event_read(--length, seed)`` (856 x 20 000: the label bench's size) whose
events are split into a head and a geometric number of stays, one on average, with lengths in seconds as float32 (``--f64``:
float64).  After one warm-up of each route they alternate for ``--rounds`` rounds; a row per timing and a summary row (median, min,
max) are appended to profiles/label_moves_bench.jsonl:

    card_kernels    the three launches alone (HIP events), tables already on the card
    card_resident   tables to the card and the three launches, the labels left on the card; ends in a device synchronise
    host            ``label_host`` on the CPU
    events_kernels  ``cf_label_events``' two launches (HIP events) on the event table that holds the same merged events: what the
                    Tombo route pays for the same labels

Needs a GPU: without one it stops, it does not fall back.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import _native as N  # noqa: E402
from catfish_amd import labelling  # noqa: E402


def move_table(length, seed, dtype):
    """``synthetic_event_read``'s events, each split into a head and ``geometric(1/2) - 1`` stays (never more parts than samples).
    -> (states uint8 [E, 5], lengths dtype [E] in seconds, moves int32 [E])."""
    _raw, bases, samples = labelling.synthetic_event_read(length, seed)
    rng = np.random.default_rng(seed + 104729)
    samples = samples.astype(np.int64)
    parts = np.minimum(rng.geometric(0.5, size=bases.size), samples)
    owner = np.repeat(np.arange(bases.size), parts)
    within = np.arange(owner.size) - np.repeat(np.cumsum(parts) - parts, parts)
    size = (samples // parts)[owner] + (within < (samples % parts)[owner])
    padded = np.concatenate((bases[:1], bases[:1], bases, bases[-1:], bases[-1:]))
    kmers = np.lib.stride_tricks.sliding_window_view(padded, 5)
    return np.ascontiguousarray(kmers[owner]), (size / float(labelling.FREQUENCY)).astype(dtype), (within == 0).astype(np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=856)
    ap.add_argument("--length", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_moves_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_moves: no GPU; the card route is not measured anywhere else")
    if args.rounds < 5:
        raise SystemExit("bench_label_moves: at least five rounds")
    dtype = np.float64 if args.f64 else np.float32
    tables = [move_table(args.length, seed, dtype) for seed in range(args.reads)]
    batch = labelling.MoveBatch.from_reads([(s, l, m, (10, 10) if 1 + np.count_nonzero(m[1:]) >= 20 else (0, 0)) for s, l, m in tables])
    # the yardstick: one event per merged event, its middle base and its samples (the k-mer test there slides over the bases, so its
    # labels are its own; the work per event and per sample is what is compared)
    merged = [labelling.merge_moves_host(l, m) for _s, l, m in tables]
    events = labelling.EventBatch.from_reads([(s[heads, 2], n, (10, 10) if heads.size >= 20 else (0, 0)) for (s, _l, _m), (heads, n) in zip(tables, merged)])
    assert events.total == batch.total and events.n_events == int(batch.merged.sum())
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = N.lib()

    def card_resident():
        got = labelling.label_moves(batch, dev)
        torch.cuda.synchronize(dev)
        return got[0]

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    on_card = [up(batch.states.reshape(-1)), up(batch.lengths), up(batch.moves), up(batch.event_offsets), up(batch.clipped.reshape(-1)),
               up(batch.n_raw), up(batch.sample_offsets)]
    out = torch.empty(batch.total, dtype=torch.uint8, device=dev)
    work_bytes = int(lib.cf_label_moves_work_bytes(batch.n_reads, batch.n_events))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    ev_card = [up(events.bases), up(events.lengths), up(events.event_offsets), up(events.clipped.reshape(-1)), up(events.sample_offsets)]
    ev_out = torch.empty(events.total, dtype=torch.uint8, device=dev)
    ev_work_bytes = int(lib.cf_label_events_work_bytes(events.n_events))
    ev_work = torch.empty(ev_work_bytes, dtype=torch.uint8, device=dev)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = N.current_stream_ptr(torch, dev)

    def card_kernels():
        begin.record()
        N.check(lib.cf_label_moves(None, N._p(on_card[0]), N._p(on_card[1]), int(args.f64), *[N._p(t) for t in on_card[2:]], batch.n_reads,
                                   batch.n_events, batch.total, batch.kmer, N._p(out), None, N._p(work), work_bytes, stream))
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / 1e3

    def events_kernels():
        begin.record()
        N.check(lib.cf_label_events(None, *[N._p(t) for t in ev_card], events.n_reads, events.n_events, events.total, 5, N._p(ev_out), None,
                                    N._p(ev_work), ev_work_bytes, stream))
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / 1e3

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, got

    want = batch.label_host()                                        # warm-up of the host route, and the answer
    assert np.array_equal(card_resident().cpu().numpy(), want)      # warm-up of the card route
    card_kernels()
    assert np.array_equal(out.cpu().numpy(), want)
    events_kernels()
    assert np.array_equal(ev_out.cpu().numpy(), events.label_host(5))
    rows, times = [], {"card_kernels": [], "card_resident": [], "host": [], "events_kernels": []}
    for rnd in range(args.rounds):
        for variant, fn in (("card_resident", card_resident), ("host", batch.label_host)):
            seconds, _ = timed(fn)
            times[variant].append(seconds)
            rows.append({"row": "round", "round": rnd, "variant": variant, "seconds": seconds})
        for variant, fn in (("card_kernels", card_kernels), ("events_kernels", events_kernels)):
            seconds = fn()
            times[variant].append(seconds)
            rows.append({"row": "round", "round": rnd, "variant": variant, "seconds": seconds})
    summary = {"row": "summary", "workload": "%d synthetic reads x %d samples, %s lengths: %d events, %d merged, %d samples" %
               (args.reads, args.length, np.dtype(dtype).name, batch.n_events, int(batch.merged.sum()), batch.total), "rounds": args.rounds,
               "device": torch.cuda.get_device_name(dev), "label_share": float(want.mean())}
    for variant, ts in times.items():
        summary[variant] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
                            "median_samples_per_s": batch.total / float(np.median(ts))}
    # bytes the three launches must move at the least: states, lengths and moves read; four compacted tables and the starts written
    # and read back; the labels written
    least = batch.n_events * (batch.kmer + batch.lengths.dtype.itemsize + 4 + 2 * 11) + batch.total
    summary["card_kernels"]["least_bytes"] = int(least)
    summary["card_kernels"]["bytes_per_s_at_median"] = least / summary["card_kernels"]["median_s"]
    summary["moves_over_events_kernels"] = summary["card_kernels"]["median_s"] / summary["events_kernels"]["median_s"]
    summary["host_over_card_resident"] = summary["host"]["median_s"] / summary["card_resident"]["median_s"]
    with open(args.out, "a") as fh:
        for row in rows + [summary]:
            fh.write(json.dumps(row) + "\n")
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
