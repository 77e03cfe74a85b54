"""What gradient clipping adds to a training step, and what it does to one lr = 0.1 draw.

Device-fed steps (``network.train_network_steps`` on a ``DeviceExampleDb``: the captured step replayed back to back) of the tuned
64 / 32 model and of one any-size geometry (128 / 64, ``native_training=True``), 256 windows, as alternating rounds of

    parent   another checkout (``--parent DIR``, built), options off
    off      this tree, options off: the launches of the parent
    clip     this tree, ``clip_norm=1.0``: cf_clip_norm + cf_opt_step_guarded in place of cf_opt_step (two launches more)

Every measurement is a process of its own (one at a time), warmed by time, at least 0.5 s of steps, ended by a synchronise.  One JSON
line per (variant, round, geometry), a summary line per geometry, then two 200-step loss curves of one draw of the random search at
learning rate 0.1 (Adam, three 128-unit layers, two 64-channel blocks), with and without ``clip_norm=1.0``, with the record.

    python tools/bench_train_clip.py [--parent DIR] [--rounds 3] [--out profiles/train_clip_bench.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = dict(optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64, n_layers=3, keep_prob=0.8, layer_size_res=32,
               n_layers_res=2)
WIDE = dict(optimizer_choice="Adam", learning_rate=0.001, layer_size=128, n_layers=3, keep_prob=0.8, layer_size_res=64, n_layers_res=2,
            native_training=True)
CONFIGS = [("64/32 tuned", SHIPPED), ("128/64 any-size", WIDE)]
BATCH, WARM_S, TIMED_S, CHUNK = 256, 0.3, 0.5, 200


def worker(args):
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    from catfish_amd import train_validate as tv
    from catfish_amd.device_db import DeviceExampleDb
    host_db = tv.synthetic_example_db(8, 20000)

    def network(hp):
        net = tv.build_model("ResNetRNN", **dict(hp, batch_size=BATCH, train_seed=0))
        net.initialize_network(seed=4)
        return net, DeviceExampleDb.from_window_db(host_db, seed=0)

    def close(net):
        net.engine.close()
        if net._trainer is not None and net._trainer.engine is not None:
            net._trainer.engine.close()

    if args.worker == "curves":
        for clip in (None, 1.0):
            net, db = network(dict(WIDE, learning_rate=0.1, **({} if clip is None else {"clip_norm": clip})))
            losses = net.train_network_steps(db, 200)
            rec = dict(curve=True, draw=dict(WIDE, learning_rate=0.1), clip_norm=clip, steps=200, losses=[float(v) for v in losses],
                       finite_steps=int(np.isfinite(losses).sum()), step_stats=net.step_stats() if clip is not None else None)
            print("ROW " + json.dumps(rec), flush=True)
            close(net)
        return
    extra = {"clip_norm": 1.0} if args.worker == "clip" else {}
    for geometry, hp in CONFIGS:
        net, db = network(dict(hp, **extra))

        def run_for(seconds):
            torch.cuda.synchronize()
            steps, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                net.train_network_steps(db, CHUNK)
                steps += CHUNK
            torch.cuda.synchronize()
            return steps, time.perf_counter() - t0

        run_for(WARM_S)
        steps, seconds = run_for(TIMED_S)
        rec = dict(geometry=geometry, batch=BATCH, variant=args.worker, round=args.round, steps=steps, ms_per_step=seconds / steps * 1e3,
                   last_loss=float(net.train_loss), device=torch.cuda.get_device_name(0))
        if extra:
            rec["step_stats"] = net.step_stats()
        print("ROW " + json.dumps(rec), flush=True)
        close(net)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; left out: no parent rows")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_clip_bench.jsonl"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import numpy as np
    rows = []

    def child(variant, root, rnd):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", variant, "--root", root, "--round", str(rnd)],
                             stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
        if res.returncode != 0:                             # nothing more is started after a failed measurement
            raise SystemExit("worker %s (round %d) ended with status %d" % (variant, rnd, res.returncode))
        for line in res.stdout.splitlines():
            if line.startswith("ROW "):
                print(line[4:], flush=True)
                rows.append(json.loads(line[4:]))

    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("off", ROOT), ("clip", ROOT)]
    for rnd in range(max(3, args.rounds)):                  # alternate, so that clock and neighbour drift hit every variant alike
        for variant, root in trees:
            child(variant, root, rnd)
    for geometry, _ in CONFIGS:
        ms = {v: [r["ms_per_step"] for r in rows if r.get("geometry") == geometry and r["variant"] == v] for v, _ in trees}
        med = {v: float(np.median(t)) for v, t in ms.items()}
        base = "parent" if args.parent else "off"
        rows.append(dict(geometry=geometry, batch=BATCH, summary=True, median_ms=med, spread_ms={v: max(t) - min(t) for v, t in ms.items()},
                         off_minus_parent_ms=med["off"] - med[base], clip_minus_off_ms=med["clip"] - med["off"]))
        print(json.dumps(rows[-1]), flush=True)
    child("curves", ROOT, 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for r in rows:
            out.write(json.dumps(r) + "\n")


main()
