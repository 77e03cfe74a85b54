"""What the per-call scores cost (catfish_amd/span_scores.py): host-to-host rate of the streaming pipeline on the README's shape -- 256
reads x 4096 samples per batch, fp32 -- with ``scores=True`` against ``scores=False``, and ``scores=False`` against another tree (the
parent commit, built), each figure from a FRESH process and the variants alternating, so that what shares the host hits all alike.

    python tools/bench_span_scores.py [--repeats 5] [--batches 48] [--parent PATH] [--out profiles/span_scores_bench.jsonl]
    python tools/bench_span_scores.py --worker --scores 1      # one figure, one JSON line (what the driver starts)
    python tools/bench_span_scores.py --worker --scores 1 --batches 8     # under rocprofv3 --kernel-trace --stats, for the kernel's time

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
    kw = {"scores": True} if args.scores else {}                 # (the other tree's pipeline may not know the option)
    pipe = ReadPipeline(eng, max_samples_per_batch=READS * SAMPLES, **kw)
    list(pipe.run(batches[:3], as_lists=False))                  # warm-up: code objects, pinned slots
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_spans = 0
    for res in pipe.run(batches, as_lists=False):
        n_spans += len(res[0])
    dt = time.perf_counter() - t0
    eng.close()
    print(json.dumps({"row": "process", "variant": args.name, "scores": bool(args.scores), "samples_per_s": args.batches * READS * SAMPLES / dt,
                      "ms_per_batch": dt / args.batches * 1e3, "batches": args.batches, "spans": n_spans}))


def one(name, scores, batches, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--name", name, "--scores", str(int(scores)), "--batches", str(batches)]
    if tree:
        cmd += ["--tree", tree]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    if res.returncode != 0:                                     # a failed process ends the whole measurement: nothing is started after it
        raise SystemExit("%s failed (%d):\n%s" % (name, res.returncode, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--name", default="scores_on")
    ap.add_argument("--scores", type=int, default=1)
    ap.add_argument("--tree", default=None, help="import the package from this tree instead of this one")
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: scores off is measured against it too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "span_scores_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    variants = [("scores_off", False, None), ("scores_on", True, None)]
    if args.parent:
        variants.insert(0, ("parent", False, os.path.abspath(args.parent)))
    rows = []
    with open(args.out, "a") as fh:
        for _ in range(args.repeats):
            for name, scores, tree in variants:                # alternating: parent, off, on, parent, off, on, ...
                row = one(name, scores, args.batches, tree)
                rows.append(row)
                fh.write(json.dumps(row) + "\n")
                fh.flush()
                print(json.dumps(row), flush=True)
        summary = {"row": "summary", "workload": "%d reads x %d samples per batch, fp32, %d batches, host to host" % (READS, SAMPLES, args.batches),
                   "repeats": args.repeats}
        for name, _scores, _tree in variants:
            v = [r["samples_per_s"] for r in rows if r["variant"] == name]
            summary[name] = {"median_samples_per_s": statistics.median(v), "min": min(v), "max": max(v),
                             "spread_over_median": (max(v) - min(v)) / statistics.median(v)}
        summary["scores_on_over_off"] = summary["scores_on"]["median_samples_per_s"] / summary["scores_off"]["median_samples_per_s"]
        if args.parent:
            summary["scores_off_over_parent"] = summary["scores_off"]["median_samples_per_s"] / summary["parent"]["median_samples_per_s"]
        fh.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
