"""What bridging costs (infer.bridge_gaps, ``ReadPipeline(max_gap=)``): host-to-host rate of the streaming pipeline on the README's shape
-- 256 reads x 4096 samples per batch, fp32 -- with ``max_gap=8`` against ``max_gap=0``, and ``max_gap=0`` against another tree (the
parent commit, built), each figure from a FRESH process and the variants alternating, so that what shares the host hits all alike.

    python tools/bench_bridge.py [--repeats 5] [--batches 48] [--parent PATH] [--out profiles/bridge_gap_bench.jsonl]
    python tools/bench_bridge.py --worker --gap 8              # one figure, one JSON line (what the driver starts)
    python tools/bench_bridge.py --worker --gap 8 --batches 8 --both   # under rocprofv3 --kernel-trace --stats: the same batches with
                                                                       # max_gap=0 first, so that both kernels are in one table

The driver appends one row per process and one summary row: medians, and the spread (max - min over median) of every variant's
own repeats -- a difference below the spread of the parent's repeats is no difference."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
READS, SAMPLES = 256, 4096


def worker(args):
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    import torch
    import bench
    from catfish_amd.engine import HipEngine
    from catfish_amd.pipeline import ReadPipeline
    from oracle import catfish_oracle as oracle
    w = bench.load_weights()
    dac = oracle.synthetic_dac(512, SAMPLES, seed=11)
    batches = [[dac[(b * READS + i) % len(dac)] for i in range(READS)] for b in range(args.batches)]
    eng = HipEngine(w, device=0, max_windows_per_pass=READS * 118, precision="fp32")
    if args.both:                                                # the unbridged kernel over the same batches, for the trace
        plain = ReadPipeline(eng, max_samples_per_batch=READS * SAMPLES)
        for _res in plain.run(batches[:3] + batches, as_lists=False):
            pass
        torch.cuda.synchronize()
    kw = {"max_gap": args.gap} if args.gap else {}               # (the other tree's pipeline may not know the option)
    pipe = ReadPipeline(eng, max_samples_per_batch=READS * SAMPLES, **kw)
    list(pipe.run(batches[:3], as_lists=False))                  # warm-up: code objects, pinned slots
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_spans = 0
    for res in pipe.run(batches, as_lists=False):
        n_spans += len(res[0])
    dt = time.perf_counter() - t0
    eng.close()
    print(json.dumps({"row": "process", "variant": args.name, "max_gap": args.gap, "samples_per_s": args.batches * READS * SAMPLES / dt,
                      "ms_per_batch": dt / args.batches * 1e3, "batches": args.batches, "spans": n_spans}))


def one(name, gap, batches, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--name", name, "--gap", str(int(gap)), "--batches", str(batches)]
    if tree:
        cmd += ["--tree", tree]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    if res.returncode != 0:                                     # a failed process ends the whole measurement: nothing is started after it
        raise SystemExit("%s failed (%d):\n%s" % (name, res.returncode, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--name", default="gap_8")
    ap.add_argument("--gap", type=int, default=8)
    ap.add_argument("--both", action="store_true", help="worker: run the batches with max_gap=0 first (one kernel trace with both kernels)")
    ap.add_argument("--tree", default=None, help="import the package from this tree instead of this one")
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: max_gap=0 is measured against it too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridge_gap_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    variants = [("gap_0", 0, None), ("gap_8", 8, None)]
    if args.parent:
        variants.insert(0, ("parent", 0, os.path.abspath(args.parent)))
    rows = []
    with open(args.out, "a") as fh:
        for _ in range(args.repeats):
            for name, gap, tree in variants:                   # alternating: parent, 0, 8, parent, 0, 8, ...
                row = one(name, gap, args.batches, tree)
                rows.append(row)
                fh.write(json.dumps(row) + "\n")
                fh.flush()
                print(json.dumps(row), flush=True)
        summary = {"row": "summary", "workload": "%d reads x %d samples per batch, fp32, %d batches, host to host" % (READS, SAMPLES, args.batches),
                   "repeats": args.repeats}
        for name, _gap, _tree in variants:
            v = [r["samples_per_s"] for r in rows if r["variant"] == name]
            summary[name] = {"median_samples_per_s": statistics.median(v), "min": min(v), "max": max(v),
                             "spread_over_median": (max(v) - min(v)) / statistics.median(v)}
        summary["gap_8_over_gap_0"] = summary["gap_8"]["median_samples_per_s"] / summary["gap_0"]["median_samples_per_s"]
        if args.parent:
            summary["gap_0_over_parent"] = summary["gap_0"]["median_samples_per_s"] / summary["parent"]["median_samples_per_s"]
        fh.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
