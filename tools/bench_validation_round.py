"""One checkpoint round of validation (``train_validate.validate``), three routes in one process on the shipped checkpoint,
alternating, at least five timed rounds each after a warm-up round:

    (a) paths      today's ``validate`` on the list of NPZ files (re-opened every round)
    (b) memory     today's ``validate`` with a loader that serves the same reads from memory: (a) without the file I/O
    (c) resident   ``validate`` on a ``device_validation.DeviceValidationSet`` (reads on the card; gather, forward pass and scoring
                   there, raw counts and sums back)

The set is 856 synthetic labelled reads of 20 000 samples (``synthetic_labelled_read``), written as NPZ to a temporary directory;
a round scores a stretch of 4 900 samples per read from a random start (seeded per round, the same for the three routes, whose
reports are compared).  Every timed round ends in a synchronise.  One JSON line per (route, round) and one summary line (median
and range of seconds per round, and whether (c)'s range lies below (a)'s and below (b)'s) are APPENDED to the output file.

    python tools/bench_validation_round.py [--rounds 5] [--commit <id>] [--out profiles/validation_round_bench.jsonl]
    python tools/bench_validation_round.py --trace-rounds 3      # route (c) alone, for rocprofv3 --kernel-trace --stats
    python tools/bench_validation_round.py --resident-rounds 15  # route (c) alone, timed: one summary line (to compare two builds,
                                                                 # run them alternately and compare against the spread of each)
    python tools/bench_validation_round.py --run-states          # the run-state leg, see below
    python tools/bench_validation_round.py --curve               # the curve leg, see below
    python tools/bench_validation_round.py --trace-curve 3       # rounds with the curve at shift 14 and shift 10, for rocprofv3
    python tools/bench_validation_round.py --borders --rounds 7  # the border leg, see below
    python tools/bench_validation_round.py --trace-borders 3     # rounds with border_reach=64, for rocprofv3 --kernel-trace --stats
    python tools/bench_validation_round.py --bases --rounds 7    # the base leg, see below
    python tools/bench_validation_round.py --trace-bases 3       # rounds with max_bases=16, for rocprofv3 --kernel-trace --stats
    python tools/bench_validation_round.py --scores --rounds 7   # the score leg, see below

The run-state leg (``--run-states``) times the device-resident round itself (``RNN.score_validation_device`` on a seeded selection,
ending in its copy back), alternating per round: without run states, with ``run_edges=(35, 70, 140)``, and the forward pass of
that round alone -- at 1 and at 16 thresholds.  Its summary line gives the medians, the time the run-state step adds to the round
and the forward pass's share of the round.

The curve leg (``--curve``) times the same round, alternating per round: without the curve, with ``curve_shift=14``, with
``curve_shift=10``, and ``HipEngine.curve_validation`` alone (launch to synchronise, no copy back) at both shifts on the round's
own probabilities and on an all-equal input (every probability 0.5, every label 1: all samples on one cell).  Its summary line
gives the medians and the milliseconds the curve adds to the round.

The border leg (``--borders``) times the same round, alternating per round: without borders, with ``run_edges=(35, 70, 140)`` (the
yardstick, in the same process), with ``border_reach=64`` -- at 1 and at 16 thresholds -- and ``HipEngine.run_borders_validation``
and ``run_states_validation`` alone (launch to synchronise, no copy back) on the round's own probabilities.  Its summary line gives
the medians, what either step adds to the round and the microseconds per threshold of either call alone.

The base leg (``--bases``) needs reads with event tables, so it makes its own set of the same shape: ``--reads`` reads of
``--read-len`` samples dealt from 64 distinct ``labelling.synthetic_event_read`` reads, labelled on the card
(``DeviceValidationSet.from_events``, k = 5).  It times the same round, alternating per round: without run tables, with
``run_edges=()`` (the yardstick, in the same process), with ``max_bases=16`` -- at 1 and at 16 thresholds -- and
``HipEngine.run_bases_validation`` and ``run_states_validation`` alone (launch to synchronise, no copy back; both include their
label passes) on the round's own probabilities.  Its summary line gives the medians, what either step adds to the round, the
microseconds per threshold of either call alone and their ratio.

The score leg (``--scores``) times the same round, alternating per round: with ``run_edges=(35, 70, 140)`` alone (the base line), the
same with ``score_shift=16`` and with ``score_shift=14``, and with ``curve_shift=14`` instead (the curve step, in the same process)
-- at 1 and at 16 thresholds -- and ``HipEngine.run_scores_validation`` at both shifts, ``run_states_validation`` and
``curve_validation`` alone (launch to synchronise, no copy back; the run steps include their label passes) on the round's own
probabilities.  Its summary line gives the medians, the milliseconds either shift and the curve add to the round with run states,
and the milliseconds of every call alone.
"""
import argparse
import contextlib
import functools
import io
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from catfish_amd import train_validate as tv  # noqa: E402
from catfish_amd.device_validation import DeviceValidationSet  # noqa: E402
from catfish_amd.resnet_class import ResNetRNN  # noqa: E402

SHIPPED = dict(batch_size=256, optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64, n_layers=3, keep_prob=0.8,
               layer_size_res=32, n_layers_res=2)
STRETCH, START, MOST = 4900, "random", 856


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def one_round(net, source, seed, name):
    """A seeded round -> (seconds, report text, returned tuple)."""
    random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        got = tv.validate(net, source, STRETCH, name, START, MOST)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    with open(name + ".txt") as fh:
        text = fh.read()
    os.remove(name + ".txt")
    return seconds, text, got


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values):
    return dict(median_s=float(np.median(values)), min_s=float(min(values)), max_s=float(max(values)))


def run_states_leg(net, resident, rounds, emit, edges=(35, 70, 140)):
    for thresholds in ((0.5,), tuple(float(t) for t in np.linspace(0.2, 0.95, 16))):
        seconds = {"plain": [], "run_states": [], "forward": []}
        for rnd in range(-1, rounds):                      # round -1 warms up (buffers grow once)
            random.seed(rnd)
            selection = resident.select(net.window, STRETCH, START, MOST)
            plain = timed(lambda: net.score_validation_device(resident, selection, thresholds))
            with_runs = timed(lambda: net.score_validation_device(resident, selection, thresholds, run_edges=edges))
            t = net.validation_buffers["tensors"]
            total = int(np.sum(-(-selection[2] // net.window) * net.window))
            forward = timed(lambda: net.engine.infer_device(t["x"][:total].view(-1, net.window), out=t["probs"][:total],
                                                            logits=t["logits"][:total]))
            if rnd >= 0:
                for key, value in (("plain", plain), ("run_states", with_runs), ("forward", forward)):
                    seconds[key].append(value)
                emit(dict(leg="run_states", thresholds=len(thresholds), round=rnd, plain_s=plain, run_states_s=with_runs, forward_s=forward))
        stats = {key: spread(v) for key, v in seconds.items()}
        added = stats["run_states"]["median_s"] - stats["plain"]["median_s"]
        emit(dict(summary=True, leg="run_states", thresholds=len(thresholds), edges=list(edges), reads=resident.n_reads, stretch=STRETCH,
                  rounds=rounds, samples_per_round=resident.n_reads * (STRETCH // 35 * 35), legs=stats, added_s=added,
                  forward_share_of_round=stats["forward"]["median_s"] / stats["plain"]["median_s"],
                  added_over_forward=added / stats["forward"]["median_s"]))


def borders_leg(net, resident, rounds, emit, reach=64, edges=(35, 70, 140)):
    from catfish_amd import device_validation as dv
    device = "cuda:%d" % net.device
    for thresholds in ((0.5,), tuple(float(t) for t in np.linspace(0.2, 0.95, 16))):
        k = len(thresholds)
        names = ("plain", "run_states", "borders", "states_call", "borders_call")
        seconds = {name: [] for name in names}
        counts = torch.empty(k * 2 * max(dv.border_cells(reach), (len(edges) + 1) * 3), dtype=torch.int64, device=device)
        for rnd in range(-1, rounds):                      # round -1 warms up (buffers grow once)
            random.seed(rnd)
            selection = resident.select(net.window, STRETCH, START, MOST)
            took = {"plain": timed(lambda: net.score_validation_device(resident, selection, thresholds)),
                    "run_states": timed(lambda: net.score_validation_device(resident, selection, thresholds, run_edges=edges)),
                    "borders": timed(lambda: net.score_validation_device(resident, selection, thresholds, border_reach=reach))}
            t = net.validation_buffers["tensors"]
            bounds, _tails = dv.layout(selection[2], net.window)
            n, total, longest = len(selection[2]), int(bounds[-1]), int(np.diff(bounds).max())
            len_d, bounds_d = t["table"][n + 1:2 * n + 1], t["table"][2 * (n + 1):3 * (n + 1)]
            took["states_call"] = timed(lambda: net.engine.run_states_validation(t["probs"][:total], t["y"][:total], bounds_d, len_d, total,
                                                                                 longest, thresholds, edges, counts, t["run_work"]))
            took["borders_call"] = timed(lambda: net.engine.run_borders_validation(t["probs"][:total], t["y"][:total], bounds_d, len_d, total,
                                                                                   longest, thresholds, reach, counts, t["run_work"]))
            if rnd >= 0:
                for name in names:
                    seconds[name].append(took[name])
                emit(dict(leg="borders", thresholds=k, round=rnd, **{name + "_s": took[name] for name in names}))
        stats = {name: spread(v) for name, v in seconds.items()}
        emit(dict(summary=True, leg="borders", thresholds=k, reach=reach, edges=list(edges), reads=resident.n_reads, stretch=STRETCH,
                  rounds=rounds, samples_per_round=resident.n_reads * (STRETCH // 35 * 35), legs=stats,
                  added_ms={name: 1e3 * (stats[name]["median_s"] - stats["plain"]["median_s"]) for name in ("run_states", "borders")},
                  call_us_per_threshold={name: 1e6 * stats[name]["median_s"] / k for name in ("states_call", "borders_call")},
                  borders_over_states_call=stats["borders_call"]["median_s"] / stats["states_call"]["median_s"]))


def event_set(reads, read_len, distinct=64):
    """A resident set of ``reads`` event reads (dealt from ``distinct`` synthetic ones), labelled on the card, with its base map."""
    from catfish_amd import labelling
    made = [labelling.synthetic_event_read(read_len, seed=7000 + i) for i in range(min(reads, distinct))]
    dealt = [made[i % len(made)] for i in range(reads)]
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in dealt])
    return DeviceValidationSet.from_events([raw for raw, _b, _l in dealt], batch, 5)


def bases_leg(net, resident, rounds, emit, max_bases=16, edges=()):
    from catfish_amd import device_validation as dv
    device = "cuda:%d" % net.device
    for thresholds in ((0.5,), tuple(float(t) for t in np.linspace(0.2, 0.95, 16))):
        k = len(thresholds)
        names = ("plain", "run_states", "bases", "states_call", "bases_call")
        seconds = {name: [] for name in names}
        counts = torch.empty(k * 2 * 3 * len(dv.BASE_CLASSES) * (max_bases + 1), dtype=torch.int64, device=device)
        for rnd in range(-1, rounds):                      # round -1 warms up (buffers grow once)
            random.seed(rnd)
            selection = resident.select(net.window, STRETCH, START, MOST)
            took = {"plain": timed(lambda: net.score_validation_device(resident, selection, thresholds)),
                    "run_states": timed(lambda: net.score_validation_device(resident, selection, thresholds, run_edges=edges)),
                    "bases": timed(lambda: net.score_validation_device(resident, selection, thresholds, max_bases=max_bases))}
            t = net.validation_buffers["tensors"]
            bounds, _tails = dv.layout(selection[2], net.window)
            n, total, longest = len(selection[2]), int(bounds[-1]), int(np.diff(bounds).max())
            src_d, len_d, bounds_d = t["table"][:n], t["table"][n + 1:2 * n + 1], t["table"][2 * (n + 1):3 * (n + 1)]
            basemap = resident.device_basemap(device)
            took["states_call"] = timed(lambda: net.engine.run_states_validation(t["probs"][:total], t["y"][:total], bounds_d, len_d, total,
                                                                                 longest, thresholds, edges, counts, t["run_work"]))
            took["bases_call"] = timed(lambda: net.engine.run_bases_validation(t["probs"][:total], t["y"][:total], basemap, src_d, bounds_d,
                                                                               len_d, total, longest, thresholds, max_bases, counts,
                                                                               t["run_work"]))
            if rnd >= 0:
                for name in names:
                    seconds[name].append(took[name])
                emit(dict(leg="bases", thresholds=k, round=rnd, **{name + "_s": took[name] for name in names}))
        stats = {name: spread(v) for name, v in seconds.items()}
        emit(dict(summary=True, leg="bases", thresholds=k, max_bases=max_bases, edges=list(edges), reads=resident.n_reads, stretch=STRETCH,
                  rounds=rounds, samples_per_round=resident.n_reads * (STRETCH // 35 * 35), legs=stats,
                  added_ms={name: 1e3 * (stats[name]["median_s"] - stats["plain"]["median_s"]) for name in ("run_states", "bases")},
                  call_us_per_threshold={name: 1e6 * stats[name]["median_s"] / k for name in ("states_call", "bases_call")},
                  bases_over_states_call=stats["bases_call"]["median_s"] / stats["states_call"]["median_s"]))


def scores_leg(net, resident, rounds, emit, shifts=(16, 14), edges=(35, 70, 140)):
    from catfish_amd import device_validation as dv
    device = "cuda:%d" % net.device
    for thresholds in ((0.5,), tuple(float(t) for t in np.linspace(0.2, 0.95, 16))):
        k = len(thresholds)
        rounds_of = ["run_states"] + ["scores_%d" % s for s in shifts] + ["curve_14"]
        calls = ["scores_call_%d" % s for s in shifts] + ["states_call", "curve_call"]
        seconds = {name: [] for name in rounds_of + calls}
        table = torch.empty(k * max(dv.score_cells(s) for s in shifts), dtype=torch.int64, device=device)
        hist = torch.empty(3 * dv.curve_bins(14), dtype=torch.int64, device=device)
        for rnd in range(-1, rounds):                      # round -1 warms up (buffers grow once)
            random.seed(rnd)
            selection = resident.select(net.window, STRETCH, START, MOST)
            took = {"run_states": timed(lambda: net.score_validation_device(resident, selection, thresholds, run_edges=edges))}
            for s in shifts:
                took["scores_%d" % s] = timed(lambda: net.score_validation_device(resident, selection, thresholds, run_edges=edges, score_shift=s))
            took["curve_14"] = timed(lambda: net.score_validation_device(resident, selection, thresholds, run_edges=edges, curve_shift=14))
            t = net.validation_buffers["tensors"]
            bounds, _tails = dv.layout(selection[2], net.window)
            n, total, longest = len(selection[2]), int(bounds[-1]), int(np.diff(bounds).max())
            len_d, bounds_d = t["table"][n + 1:2 * n + 1], t["table"][2 * (n + 1):3 * (n + 1)]
            probs, y = t["probs"][:total], t["y"][:total]
            for s in shifts:
                took["scores_call_%d" % s] = timed(lambda: net.engine.run_scores_validation(probs, y, bounds_d, len_d, total, longest, thresholds,
                                                                                            s, table, t["run_work"]))
            took["states_call"] = timed(lambda: net.engine.run_states_validation(probs, y, bounds_d, len_d, total, longest, thresholds, edges,
                                                                                 table, t["run_work"]))
            took["curve_call"] = timed(lambda: net.engine.curve_validation(probs, y, bounds_d, len_d, total, longest, 14, hist))
            if rnd >= 0:
                for name in seconds:
                    seconds[name].append(took[name])
                emit(dict(leg="scores", thresholds=k, round=rnd, **{name + "_s": took[name] for name in seconds}))
        stats = {name: spread(v) for name, v in seconds.items()}
        emit(dict(summary=True, leg="scores", thresholds=k, shifts=list(shifts), edges=list(edges), reads=resident.n_reads, stretch=STRETCH,
                  rounds=rounds, samples_per_round=resident.n_reads * (STRETCH // 35 * 35), legs=stats,
                  added_ms={name: 1e3 * (stats[name]["median_s"] - stats["run_states"]["median_s"]) for name in rounds_of[1:]},
                  call_ms={name: 1e3 * stats[name]["median_s"] for name in calls},
                  table_bytes={str(s): 8 * k * dv.score_cells(s) for s in shifts}))


def curve_leg(net, resident, rounds, emit, shifts=(14, 10)):
    from catfish_amd import device_validation as dv
    thresholds = (0.5,)
    names = ["plain"] + ["curve_%d" % s for s in shifts] + ["kernel_%d" % s for s in shifts] + ["kernel_equal_%d" % s for s in shifts]
    seconds = {name: [] for name in names}
    hist = {s: torch.empty(3 * dv.curve_bins(s), dtype=torch.int64, device="cuda:%d" % net.device) for s in shifts}
    equal = None
    for rnd in range(-1, rounds):                          # round -1 warms up (buffers grow once per shift)
        random.seed(rnd)
        selection = resident.select(net.window, STRETCH, START, MOST)
        took = {"plain": timed(lambda: net.score_validation_device(resident, selection, thresholds))}
        for s in shifts:
            took["curve_%d" % s] = timed(lambda: net.score_validation_device(resident, selection, thresholds, curve_shift=s))
        t = net.validation_buffers["tensors"]
        bounds, _tails = dv.layout(selection[2], net.window)
        n, total, longest = len(selection[2]), int(bounds[-1]), int(np.diff(bounds).max())
        len_d, bounds_d = t["table"][n + 1:2 * n + 1], t["table"][2 * (n + 1):3 * (n + 1)]
        if equal is None or equal[0].numel() < total:
            equal = (torch.full((total,), 0.5, dtype=torch.float32, device=hist[shifts[0]].device),
                     torch.ones(total, dtype=torch.uint8, device=hist[shifts[0]].device))
        for s in shifts:
            took["kernel_%d" % s] = timed(lambda: net.engine.curve_validation(t["probs"][:total], t["y"][:total], bounds_d, len_d, total,
                                                                              longest, s, hist[s]))
            took["kernel_equal_%d" % s] = timed(lambda: net.engine.curve_validation(equal[0][:total], equal[1][:total], bounds_d, len_d,
                                                                                    total, longest, s, hist[s]))
        if rnd >= 0:
            for name in names:
                seconds[name].append(took[name])
            emit(dict(leg="curve", round=rnd, **{name + "_s": took[name] for name in names}))
    stats = {name: spread(v) for name, v in seconds.items()}
    emit(dict(summary=True, leg="curve", shifts=list(shifts), reads=resident.n_reads, stretch=STRETCH, rounds=rounds,
              samples_per_round=resident.n_reads * (STRETCH // 35 * 35), legs=stats,
              added_ms={str(s): 1e3 * (stats["curve_%d" % s]["median_s"] - stats["plain"]["median_s"]) for s in shifts},
              kernel_ms={str(s): 1e3 * stats["kernel_%d" % s]["median_s"] for s in shifts},
              kernel_equal_ms={str(s): 1e3 * stats["kernel_equal_%d" % s]["median_s"] for s in shifts},
              histogram_bytes={str(s): 24 * dv.curve_bins(s) for s in shifts}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reads", type=int, default=856)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--commit", default=None, help="stamp of the lines (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_round_bench.jsonl"))
    ap.add_argument("--trace-rounds", type=int, default=0, help="route (c) alone for this many rounds, then exit")
    ap.add_argument("--resident-rounds", type=int, default=0, help="route (c) alone, timed for this many rounds, then exit")
    ap.add_argument("--run-states", action="store_true", help="the run-state leg alone, then exit")
    ap.add_argument("--curve", action="store_true", help="the curve leg alone, then exit")
    ap.add_argument("--trace-curve", type=int, default=0, help="this many rounds with the curve at shift 14 and at shift 10, then exit")
    ap.add_argument("--borders", action="store_true", help="the border leg alone, then exit")
    ap.add_argument("--trace-borders", type=int, default=0, help="this many rounds with border_reach=64 at 16 thresholds, then exit")
    ap.add_argument("--bases", action="store_true", help="the base leg alone (on a set of event reads of its own), then exit")
    ap.add_argument("--scores", action="store_true", help="the score leg alone, then exit")
    ap.add_argument("--trace-bases", type=int, default=0, help="this many rounds with max_bases=16 at 16 thresholds, then exit")
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    commit = args.commit or commit_id()
    with np.load(os.path.join(ROOT, "tests", "golden", "ckpnt-30000-inference.npz")) as z:
        weights = {k: z[k] for k in z.files}
    net = ResNetRNN(**SHIPPED)
    with contextlib.redirect_stdout(io.StringIO()):
        net.set_weights(weights)
    out_path = os.path.abspath(args.out)
    if args.bases or args.trace_bases:
        resident = event_set(args.reads, args.read_len)
        if args.trace_bases:
            for rnd in range(args.trace_bases):
                random.seed(rnd)
                selection = resident.select(net.window, STRETCH, START, MOST)
                net.score_validation_device(resident, selection, tuple(float(t) for t in np.linspace(0.2, 0.95, 16)), run_edges=(), max_bases=16)
            print(json.dumps(dict(traced="bases", rounds=args.trace_bases, max_bases=16, thresholds=16)))
        else:
            os.makedirs(os.path.dirname(out_path), exist_ok=True)
            with open(out_path, "a") as out:
                def emit_line(rec):
                    line = json.dumps(dict(rec, commit=commit))
                    print(line, flush=True)
                    out.write(line + "\n")
                    out.flush()

                bases_leg(net, resident, rounds, emit_line)
        net.engine.close()
        return
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        paths, memory = [], {}
        for i in range(args.reads):
            raw, lab = tv.synthetic_labelled_read(args.read_len, seed=7000 + i)
            paths.append(os.path.join(tmp, "read_%04d.npz" % i))
            np.savez(paths[-1], raw=raw, base_labels=lab)
            memory[paths[-1]] = (raw, lab)
        t0 = time.perf_counter()
        resident = DeviceValidationSet.from_npz(paths)
        load_s = time.perf_counter() - t0
        from_paths = tv.select_validation_stretches
        from_memory = functools.partial(from_paths, loader=memory.__getitem__)

        def route(name, source, select):
            def run(seed):
                tv.select_validation_stretches = select
                try:
                    return one_round(net, source, seed, name)
                finally:
                    tv.select_validation_stretches = from_paths
            return name, run

        routes = [route("a_paths", paths, from_paths), route("b_memory", paths, from_memory), route("c_resident", resident, from_paths)]
        if args.trace_rounds:
            for rnd in range(args.trace_rounds):
                routes[2][1](rnd)
            print(json.dumps(dict(traced="c_resident", rounds=args.trace_rounds)))
            os.chdir(ROOT)
            return
        if args.trace_curve:
            for rnd in range(args.trace_curve):
                random.seed(rnd)
                selection = resident.select(net.window, STRETCH, START, MOST)
                for shift in (14, 10):
                    net.score_validation_device(resident, selection, (0.5,), curve_shift=shift)
            print(json.dumps(dict(traced="curve", rounds=args.trace_curve, shifts=[14, 10])))
            os.chdir(ROOT)
            return
        if args.trace_borders:
            for rnd in range(args.trace_borders):
                random.seed(rnd)
                selection = resident.select(net.window, STRETCH, START, MOST)
                net.score_validation_device(resident, selection, tuple(float(t) for t in np.linspace(0.2, 0.95, 16)), run_edges=(35, 70, 140),
                                            border_reach=64)
            print(json.dumps(dict(traced="borders", rounds=args.trace_borders, reach=64, thresholds=16)))
            os.chdir(ROOT)
            return
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as out:
            def emit(rec):
                line = json.dumps(dict(rec, commit=commit))
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()

            if args.resident_rounds or args.run_states or args.curve or args.borders or args.scores:
                if args.resident_rounds:
                    routes[2][1](-1)
                    took = [routes[2][1](rnd)[0] for rnd in range(args.resident_rounds)]
                    emit(dict(summary=True, leg="resident_only", reads=args.reads, read_len=args.read_len, stretch=STRETCH,
                              rounds=args.resident_rounds, seconds=took, **spread(took)))
                if args.run_states:
                    run_states_leg(net, resident, rounds, emit)
                if args.curve:
                    curve_leg(net, resident, rounds, emit)
                if args.borders:
                    borders_leg(net, resident, rounds, emit)
                if args.scores:
                    scores_leg(net, resident, rounds, emit)
                os.chdir(ROOT)
                net.engine.close()
                return
            for name, run in routes:                       # warm-up: allocator, page cache, the set's upload, lazy initialisation
                run(-1)
            seconds = {name: [] for name, _ in routes}
            same = True
            for rnd in range(rounds):                      # alternate, so that clock and neighbour drift hit all three alike
                seen = []
                for name, run in routes:
                    s, text, got = run(rnd)
                    seconds[name].append(s)
                    seen.append((text.replace(name, "route"), got))
                    emit(dict(route=name, round=rnd, seconds=s))
                same = same and seen[0] == seen[1] == seen[2]
            stats = {name: dict(median_s=float(np.median(v)), min_s=float(min(v)), max_s=float(max(v))) for name, v in seconds.items()}
            emit(dict(summary=True, reads=args.reads, read_len=args.read_len, stretch=STRETCH, start=START, rounds=rounds,
                      samples_per_round=args.reads * (STRETCH // 35 * 35), load_resident_set_s=load_s, routes=stats,
                      reports_equal=bool(same),
                      c_range_below_a=bool(stats["c_resident"]["max_s"] < stats["a_paths"]["min_s"]),
                      c_range_below_b=bool(stats["c_resident"]["max_s"] < stats["b_memory"]["min_s"]),
                      a_over_c=stats["a_paths"]["median_s"] / stats["c_resident"]["median_s"],
                      b_over_c=stats["b_memory"]["median_s"] / stats["c_resident"]["median_s"]))
        os.chdir(ROOT)
    net.engine.close()


main()
