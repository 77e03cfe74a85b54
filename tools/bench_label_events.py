#!/usr/bin/env python3
"""Labels from event tables: the card route (``labelling.label_reads`` -> ``cf_label_events``) against the host route
(``EventBatch.label_host``) on the same tables.

    python tools/bench_label_events.py [--reads 856] [--length 20000] [--rounds 7] [--kmer 5]

The batch is ``--reads`` reads of ``labelling.synthetic_event_read(--length, seed)`` (856 x 20 000: a validation set of the size
``train_validate`` takes).  After one warm-up of each route the two alternate for ``--rounds`` rounds; a row per timing and a summary
row (median, min, max) are appended to profiles/label_events_bench.jsonl.  Three card timings per round, each ending in a device
synchronise:

    card_call     tables to the card, both launches, labels back on the host: what ``DeviceValidationSet.from_events`` pays
    card_resident the same without the copy back: the labels stay on the card, where the validation set keeps them
    card_kernels  the two launches alone (HIP events), tables already on the card

and ``host``: ``label_host`` on the CPU.  Needs a GPU: without one it stops, it does not fall back.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=856)
    ap.add_argument("--length", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kmer", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_events_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_events: no GPU; the card route is not measured anywhere else")
    if args.rounds < 5:
        raise SystemExit("bench_label_events: at least five rounds")
    reads = [labelling.synthetic_event_read(args.length, seed) for seed in range(args.reads)]
    batch = labelling.EventBatch.from_reads([(b, l, (10, 10) if len(b) >= 20 else (0, 0)) for _raw, b, l in reads])
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = N.lib()

    def card_call():
        return labelling.label_reads(batch, args.kmer, dev).cpu().numpy()

    def card_resident():
        labels = labelling.label_reads(batch, args.kmer, dev)
        torch.cuda.synchronize(dev)
        return labels

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    tables = [up(batch.bases), up(batch.lengths), up(batch.event_offsets), up(batch.clipped.reshape(-1)), up(batch.sample_offsets)]
    out = torch.empty(batch.total, dtype=torch.uint8, device=dev)
    work_bytes = int(lib.cf_label_events_work_bytes(batch.n_events))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def card_kernels():
        begin.record()
        N.check(lib.cf_label_events(None, *[N._p(t) for t in tables], batch.n_reads, batch.n_events, batch.total, args.kmer, N._p(out), None,
                                    N._p(work), work_bytes, N.current_stream_ptr(torch, dev)))
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / 1e3

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, got

    want = batch.label_host(args.kmer)                               # warm-up of the host route, and the answer
    assert np.array_equal(card_call(), want) and np.array_equal(card_resident().cpu().numpy(), want)     # warm-up of the card route
    card_kernels()
    assert np.array_equal(out.cpu().numpy(), want)
    rows, times = [], {"card_call": [], "card_resident": [], "card_kernels": [], "host": []}
    for rnd in range(args.rounds):
        for variant, fn in (("card_call", card_call), ("host", lambda: batch.label_host(args.kmer)), ("card_resident", card_resident)):
            seconds, _ = timed(fn)
            times[variant].append(seconds)
            rows.append({"row": "round", "round": rnd, "variant": variant, "seconds": seconds})
        seconds = card_kernels()
        times["card_kernels"].append(seconds)
        rows.append({"row": "round", "round": rnd, "variant": "card_kernels", "seconds": seconds})
    summary = {"row": "summary", "workload": "%d synthetic reads x %d samples, kmer %d: %d events, %d samples" %
               (args.reads, args.length, args.kmer, batch.n_events, batch.total), "rounds": args.rounds,
               "device": torch.cuda.get_device_name(dev), "label_share": float(want.mean())}
    for variant, ts in times.items():
        summary[variant] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
                            "median_samples_per_s": batch.total / float(np.median(ts))}
    # bytes the two launches must move at the least: bases + lengths + start and class written and read back + labels
    least = batch.n_events * (1 + 4 + 2 * 5) + batch.total
    summary["card_kernels"]["least_bytes"] = int(least)
    summary["card_kernels"]["bytes_per_s_at_median"] = least / summary["card_kernels"]["median_s"]
    summary["host_over_card_call"] = summary["host"]["median_s"] / summary["card_call"]["median_s"]
    with open(args.out, "a") as fh:
        for row in rows + [summary]:
            fh.write(json.dumps(row) + "\n")
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
