"""Training step in fp32 and with ``precision="bf16x3"`` (split bf16 products on the serial chain of the any-size recurrences), at
geometries other than the shipped 64 / 32: the native whole step (``native=True``) and torch autograd around the recurrence kernels
(the default), graph-replayed, batch 256 and 512.  The two precisions of a path alternate in one process, so that clock and
neighbour drift hit both alike; one JSON line per (batch, geometry, path) with the medians, every round's time and the loss
trajectories' largest difference.

    --fp32-only          fp32 alone (no ``precision`` argument is passed: also runs on a tree without the mode, for A/B of libraries)
    --only H/C/L/R       one geometry, e.g. 128/64/3/2
    --batch N            one batch size
    --path native|autograd   one path
    --steps N --rounds N timed steps per round (10) and alternating rounds (3)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from catfish_amd.training import Trainer  # noqa: E402
from oracle import catfish_oracle as oracle  # noqa: E402
import bench  # noqa: E402

GEOMETRIES = ((32, 16, 3, 2), (128, 64, 3, 2), (256, 128, 3, 2), (128, 0, 2, 0), (128, 64, 5, 5))


def timed(tr, x, y, n):
    for _ in range(3):
        tr.train_step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.train_step(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    fp32_only = "--fp32-only" in sys.argv
    steps, rounds = int(arg("--steps", 10)), int(arg("--rounds", 3))
    geos = GEOMETRIES if "--only" not in sys.argv else (tuple(int(v) for v in arg("--only", "").split("/")),)
    batches = (256, 512) if "--batch" not in sys.argv else (int(arg("--batch", 256)),)
    reads = bench.make_reads(8, seed=5).reshape(-1, 35)
    rng = np.random.default_rng(0)
    for B in batches:
        x = reads[rng.permutation(len(reads))[:B]]
        y = np.repeat((np.arange(B) % 2)[:, None], 35, axis=1).astype(np.float32)
        for h, c, nl, nr in geos:
            w = oracle.random_weights(seed=3, layer_size=h, n_layers=nl, layer_size_res=max(c, 16), n_layers_res=nr)
            for path, native in (("native", True), ("autograd", None)):
                if arg("--path", path) != path:
                    continue
                kinds = {"fp32": {}} if fp32_only else {"fp32": {}, "bf16x3": {"precision": "bf16x3"}}
                res = dict(layer_size=h, layer_size_res=c, n_layers=nl, n_layers_res=nr, batch=B, path=path, steps=steps)
                # the same eight updates without dropout in both precisions: how far the losses part
                losses = {}
                for name, kw in kinds.items():
                    tr = Trainer(w, nl, nr, "Adam", 1e-3, keep_prob=1.0, seed=0, native=native, **kw)
                    losses[name] = [tr.train_step(x, y) for _ in range(8)]
                    tr.engine.close()
                if not fp32_only:
                    res["max_loss_diff_bf16x3_vs_fp32"] = float(np.max(np.abs(np.array(losses["fp32"]) - np.array(losses["bf16x3"]))))
                res["last_loss_fp32"] = float(losses["fp32"][-1])
                trs = {name: Trainer(w, nl, nr, "Adam", 1e-3, keep_prob=0.8, seed=0, native=native, **kw) for name, kw in kinds.items()}
                times = {name: [] for name in kinds}
                for _ in range(rounds):                    # alternate the precisions
                    for name, tr in trs.items():
                        times[name].append(timed(tr, x, y, steps))
                for name, ts in times.items():
                    res[name + "_ms"] = float(np.median(ts))
                    res[name + "_ms_rounds"] = [round(float(t), 4) for t in ts]
                if not fp32_only:
                    res["bf16x3_speedup"] = res["fp32_ms"] / res["bf16x3_ms"]
                for tr in trs.values():
                    tr.engine.close()
                print(json.dumps(res), flush=True)


main()
