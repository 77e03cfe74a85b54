"""What shifted-window voting costs (tilings.py, ``ReadPipeline(phases=)``): per-batch time of the streaming pipeline at the command
line's batch size -- 1110 reads x 4096 samples, 131 072 windows per pass, fp32, host to host -- for K = 1, 2 and 3 tilings, K = 1
against another tree (the parent commit, built), each figure from a FRESH process and the variants alternating, so that what shares
the host hits all alike; and the HIP-event times of the two new kernels with their bytes moved, beside ``cf_validation_gather`` --
the project's own comparable streaming kernel -- measured in the same process.

    python tools/bench_tilings.py [--repeats 5] [--batches 12] [--parent PATH] [--out profiles/tilings_bench.jsonl]
    python tools/bench_tilings.py --worker --phases 0,12,23      # one figure, one JSON line (what the driver starts)
    python tools/bench_tilings.py --kernels                      # the kernel rows alone

The driver appends one row per process, the kernel rows and one summary row: medians, and the spread (max - min over median) of
every variant's own repeats -- a difference below the spread of the parent's repeats is no difference.  The default path (K = 1)
is the only performance claim; for K > 1 the measured ratio is written down, not promised."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
READS, SAMPLES, WINDOWS_PER_PASS = 1110, 4096, 131072
PHASES = {"k1": (0,), "k2": (0, 17), "k3": (0, 12, 23)}


def worker(args):
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    import torch
    import bench
    from catfish_amd.engine import HipEngine
    from catfish_amd.pipeline import ReadPipeline
    from oracle import catfish_oracle as oracle
    phases = tuple(int(v) for v in args.phases.split(","))
    w = bench.load_weights()
    dac = oracle.synthetic_dac(256, SAMPLES, seed=11)
    batches = [[dac[(b * 7 + i) % len(dac)] for i in range(READS)] for b in range(args.batches)]
    eng = HipEngine(w, device=0, max_windows_per_pass=WINDOWS_PER_PASS, precision="fp32")
    kw = {"phases": phases, "vote_weight": args.weight} if len(phases) > 1 else {}       # (the other tree's pipeline does not know the option)
    pipe = ReadPipeline(eng, max_samples_per_batch=READS * SAMPLES, **kw)
    list(pipe.run(batches[:2], as_lists=False))                  # warm-up: code objects, pinned slots
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_spans = 0
    for res in pipe.run(batches, as_lists=False):
        n_spans += len(res[0])
    dt = time.perf_counter() - t0
    eng.close()
    print(json.dumps({"row": "process", "variant": args.name, "phases": list(phases), "samples_per_s": args.batches * READS * SAMPLES / dt,
                      "ms_per_batch": dt / args.batches * 1e3, "batches": args.batches, "spans": n_spans}))


def kernels(args):
    """HIP-event times of cf_retile_windows, cf_vote_tilings and cf_validation_gather over one batch of the size above."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from catfish_amd import tilings
    from catfish_amd.engine import HipEngine
    eng = HipEngine(bench.load_weights(), device=0, max_windows_per_pass=1024, precision="fp32")
    dev = torch.device("cuda", 0)
    lengths = np.full(READS, SAMPLES, dtype=np.int64)
    offsets = np.zeros(READS + 1, dtype=np.int64)
    np.cumsum((lengths // 35 + 1) * 35, out=offsets[1:])
    total = int(offsets[-1])
    d_off, d_len = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
    rows = []

    def timed(call, reps=20):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for name, phases in sorted(PHASES.items()):
        if len(phases) == 1:
            continue
        k = len(phases)
        size, region = tilings.tiling_size(total, READS, k), tilings.region_size(total, READS)
        x_all = torch.randn(size, dtype=torch.float32, device=dev)
        probs_all, logits_all = torch.rand(size, dtype=torch.float32, device=dev), torch.randn(size, dtype=torch.float32, device=dev)
        out, lout = torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.float32, device=dev)
        for kernel, call, moved in (
                ("cf_retile_windows", lambda: eng.retile_device(x_all, d_off, d_len, total, phases), 4 * (k - 1) * (READS * SAMPLES + region)),
                ("cf_vote_tilings", lambda: eng.vote_device(probs_all, d_off, d_len, total, phases, args.weight, out=out),
                 4 * (total + (k - 1) * READS * SAMPLES + total)),
                ("cf_vote_tilings+logits", lambda: eng.vote_device(probs_all, d_off, d_len, total, phases, args.weight, logits_all=logits_all,
                                                                    out=out, logits_out=lout), 8 * (total + (k - 1) * READS * SAMPLES + total))):
            med, lo, hi = timed(call)
            rows.append({"row": "kernel", "kernel": kernel, "phases": list(phases), "weight": args.weight, "ms": med, "ms_min": lo, "ms_max": hi,
                         "bytes": moved, "gb_per_s": moved / med / 1e6})
        del x_all, probs_all, logits_all
    signal = torch.randn(READS * SAMPLES, dtype=torch.float32, device=dev)
    labels = torch.zeros(READS * SAMPLES, dtype=torch.uint8, device=dev)
    src = torch.arange(READS, dtype=torch.int64, device=dev) * SAMPLES
    x, y = torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    med, lo, hi = timed(lambda: eng.gather_validation(signal, labels, src, d_len, d_off, total, int(np.diff(offsets).max()), x, y))
    moved = 5 * (READS * SAMPLES + total)
    rows.append({"row": "kernel", "kernel": "cf_validation_gather", "ms": med, "ms_min": lo, "ms_max": hi, "bytes": moved,
                 "gb_per_s": moved / med / 1e6})
    torch.cuda.synchronize()
    eng.check_error()
    eng.close()
    for row in rows:
        print(json.dumps(row))


def one(argv, timeout=900):
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=timeout)
    if res.returncode != 0:                                     # a failed process ends the whole measurement: nothing is started after it
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(argv), res.returncode, res.stderr[-2000:]))
    return [json.loads(line) for line in res.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--name", default="k3")
    ap.add_argument("--phases", default="0,12,23")
    ap.add_argument("--weight", default="mean")
    ap.add_argument("--tree", default=None, help="import the package from this tree instead of this one")
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: K = 1 is measured against it too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tilings_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.kernels:
        return kernels(args)
    variants = [(name, phases, None) for name, phases in sorted(PHASES.items())]
    if args.parent:
        variants.insert(0, ("parent", (0,), os.path.abspath(args.parent)))
    rows = []
    with open(args.out, "a") as fh:
        def keep(row):
            fh.write(json.dumps(row) + "\n")
            fh.flush()
            print(json.dumps(row), flush=True)
        for _ in range(args.repeats):
            for name, phases, tree in variants:                # alternating: parent, k1, k2, k3, parent, ...
                argv = ["--worker", "--name", name, "--phases", ",".join(str(p) for p in phases), "--weight", args.weight,
                        "--batches", str(args.batches)] + (["--tree", tree] if tree else [])
                (row,) = one(argv)
                rows.append(row)
                keep(row)
        for row in one(["--kernels", "--weight", args.weight]):
            keep(row)
        summary = {"row": "summary", "repeats": args.repeats,
                   "workload": "%d reads x %d samples per batch, %d windows per pass, fp32, %d batches, host to host" % (READS, SAMPLES, WINDOWS_PER_PASS,
                                                                                                                       args.batches)}
        for name, _phases, _tree in variants:
            v = [r["ms_per_batch"] for r in rows if r["variant"] == name]
            summary[name] = {"median_ms_per_batch": statistics.median(v), "min": min(v), "max": max(v),
                             "spread_over_median": (max(v) - min(v)) / statistics.median(v)}
        for name in ("k2", "k3"):
            summary[name + "_over_k1"] = summary[name]["median_ms_per_batch"] / summary["k1"]["median_ms_per_batch"]
        if args.parent:
            summary["k1_over_parent"] = summary["k1"]["median_ms_per_batch"] / summary["parent"]["median_ms_per_batch"]
        keep(summary)


if __name__ == "__main__":
    main()
