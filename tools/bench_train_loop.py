"""The training LOOP, not only the step: per (geometry, batch), alternating in one process, at least three rounds each,

    (a) today's loop      db.get_training_set + reshape_input x2 + network.train_network   (host sampler, host-fed step)
    (b) the bare step     Trainer.train_step on a cycle of ready-made host batches
    (c) device-fed        network.train_network_steps on a DeviceExampleDb holding the same windows (the batch is drawn by a
                          HIP kernel inside the captured step; no copy, read-back or synchronise between steps)

Every timed window is preceded by a warm-up by time, runs at least 0.5 s of steps and ends in a synchronise.  One JSON line per
(geometry, batch, variant, round), then one summary line per (geometry, batch) with the medians, (b)'s spread (max - min over its
rounds) and the two conditions: (c) not slower than (b) beyond that spread, (c) faster than (a).

    python tools/bench_train_loop.py [--rounds 3] [--out profiles/train_loop_bench.jsonl] [--quick]
    python tools/bench_train_loop.py --trace-steps 300       # variant (c) alone at 256 windows, for rocprofv3 --kernel-trace --stats
    python tools/bench_train_loop.py --trace-steps 100 --trace-variant b --trace-batch 4096      # the bare step, to compare kernel times
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from catfish_amd import train_validate as tv  # noqa: E402
from catfish_amd.device_db import DeviceExampleDb  # noqa: E402

SHIPPED = dict(optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64, n_layers=3, keep_prob=0.8, layer_size_res=32,
               n_layers_res=2)
WIDE = dict(optimizer_choice="Adam", learning_rate=0.001, layer_size=128, n_layers=3, keep_prob=0.8, layer_size_res=64, n_layers_res=2)
CONFIGS = [("64/32 native", SHIPPED, 256), ("64/32 native", SHIPPED, 4096), ("128/64 autograd", WIDE, 256),
           ("128/64 native", dict(WIDE, native_training=True), 256)]
WARM_S, TIMED_S = 0.3, 0.5


def network(hp, batch):
    net = tv.build_model("ResNetRNN", **dict(hp, batch_size=batch, train_seed=0))
    net.initialize_network(seed=4)
    return net


def run_for(seconds, body):
    """Call ``body()`` (which returns the number of steps it ran) until ``seconds`` have passed; synchronise; (steps, seconds)."""
    torch.cuda.synchronize()
    steps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        steps += body()
    torch.cuda.synchronize()
    return steps, time.perf_counter() - t0


def variants(hp, batch, host_db):
    net_a, net_b, net_c = network(hp, batch), network(hp, batch), network(hp, batch)
    dev_db = DeviceExampleDb.from_window_db(host_db, seed=0)

    def loop_a():
        windows, labels, _ = host_db.get_training_set(batch, ratio=2)
        net_a.train_network(tv.reshape_input(windows, net_a.window, net_a.n_inputs),
                            tv.reshape_input(labels, net_a.window, net_a.n_outputs), 0)
        return 1

    ready = []
    for _ in range(8):
        windows, labels, _ = host_db.get_training_set(batch, ratio=2)
        ready.append((np.asarray(windows, np.float32).reshape(batch, 35), np.asarray(labels, np.float32).reshape(batch, 35)))
    trainer_b = net_b._require_trainer()
    turn = [0]

    def loop_b():
        x, y = ready[turn[0] % len(ready)]
        turn[0] += 1
        trainer_b.train_step(x, y)
        return 1

    chunk = [32]

    def loop_c():
        net_c.train_network_steps(dev_db, chunk[0])
        return chunk[0]

    def size_chunk():                                      # about a fifth of a timed window per call, from a first estimate
        n, s = run_for(0.1, loop_c)
        chunk[0] = int(max(32, min(4096, TIMED_S / 5 / (s / n))))

    return [("a_host_loop", loop_a, None), ("b_bare_step", loop_b, None), ("c_device_fed", loop_c, size_chunk)], (net_a, net_b, net_c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loop_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="shipped geometry at 256 windows only")
    ap.add_argument("--trace-steps", type=int, default=0, help="one variant alone for this many steps, then exit")
    ap.add_argument("--trace-variant", choices=("b", "c"), default="c")
    ap.add_argument("--trace-batch", type=int, default=256)
    args = ap.parse_args()
    host_db = tv.synthetic_example_db(8, 20000)
    if args.trace_steps:
        todo, nets = variants(SHIPPED, args.trace_batch, host_db)
        name, body, _ = todo[1 if args.trace_variant == "b" else 2]
        steps = 0
        while steps < args.trace_steps:
            steps += body()
        torch.cuda.synchronize()
        print(json.dumps(dict(traced=name, batch=args.trace_batch, steps=steps)))
        return
    rounds = max(3, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for geometry, hp, batch in (CONFIGS[:1] if args.quick else CONFIGS):
            todo, nets = variants(hp, batch, host_db)
            ms = {name: [] for name, _, _ in todo}
            for name, body, prepare in todo:               # captures, allocator, lazy initialisation
                run_for(WARM_S, body)
                if prepare:
                    prepare()
            for rnd in range(rounds):                      # alternate, so that clock and neighbour drift hit all three alike
                for name, body, _ in todo:
                    run_for(WARM_S, body)
                    steps, seconds = run_for(TIMED_S, body)
                    ms[name].append(seconds / steps * 1e3)
                    emit(dict(geometry=geometry, batch=batch, variant=name, round=rnd, steps=steps, seconds=round(seconds, 4),
                              ms_per_step=seconds / steps * 1e3))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            spread_b = float(max(ms["b_bare_step"]) - min(ms["b_bare_step"]))
            emit(dict(geometry=geometry, batch=batch, summary=True, median_ms=med, spread_b_ms=spread_b,
                      c_not_slower_than_b=bool(med["c_device_fed"] <= med["b_bare_step"] + spread_b),
                      c_faster_than_a=bool(med["c_device_fed"] < med["a_host_loop"]),
                      a_over_c=med["a_host_loop"] / med["c_device_fed"], final_losses=[float(n._trainer.last_loss) for n in nets]))
            for n in nets:
                n.engine.close()
                if n._trainer is not None and n._trainer.engine is not None:
                    n._trainer.engine.close()


main()
