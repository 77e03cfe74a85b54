#!/usr/bin/env python3
"""Per-base calls: what the vote step (``HipEngine.base_votes_validation`` -> ``cf_base_votes``, two launches) costs per threshold
group, next to the run-bases step of the same round and to the numpy definition on the host.

    python tools/bench_base_votes.py [--reads 856] [--read-len 20000] [--rounds 7] [--commit <id>]
    python tools/bench_base_votes.py --trace 3        # calls only, for rocprofv3 --kernel-trace --stats: the two launches apart

The set is the validation-round bench's base leg: ``--reads`` event reads of ``--read-len`` samples dealt from 64 distinct
``labelling.synthetic_event_read`` reads, labelled on the card; a round is 856 stretches of 4 900 samples at a random start (4.19 M
samples, about 0.46 M voted bases).  One forward pass fills the round's probabilities; then, at 1 and at 16 thresholds, the legs
alternate for ``--rounds`` rounds after one warm-up and a row per timing and a summary row (median, min, max) are appended to
profiles/base_votes_bench.jsonl:

    votes_call     the vote step alone, launch to synchronise (three memsets and two launches)
    votes_events   the same between two HIP events
    bases_call     ``run_bases_validation`` alone on the same round, launch to synchronise: the sibling step
    host           ``base_votes.vote_host`` in numpy, once (it is a definition, not a route)

and, with the library's debug knob ``CATFISH_BASE_VOTES_LONG`` (the sums are integers: no value changes a result), ``votes_call`` at
several values of the long-base constant -- 0: every base by its whole wave; 2^31 - 1: one lane per base throughout -- on that set,
whose bases are short, and on a copy of it in which one base in 400 swallows the 120 behind it (stalls of about a thousand samples);
and, with ``CATFISH_BASE_VOTES_COUNT_BLOCKS``, at several sizes of the count launch's grid.

Synthetic reads only.  Needs a GPU: without one it stops, it does not fall back.
"""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from catfish_amd import base_votes as bv  # noqa: E402
from catfish_amd import device_validation as dv  # noqa: E402

# the validation-round bench's model and round (tools/bench_validation_round.py)
SHIPPED = dict(batch_size=256, optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64, n_layers=3, keep_prob=0.8,
               layer_size_res=32, n_layers_res=2)
STRETCH, START, MOST = 4900, "random", 856
LONG_VALUES = (0, 64, 256, 1024, 2 ** 31 - 1)
COUNT_BLOCKS = (512, 2048, 8192, 2 ** 30)             # 2^30: a workgroup per stretch, piece and threshold


def commit_id():
    import subprocess
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values):
    return dict(median_s=float(np.median(values)), min_s=float(min(values)), max_s=float(max(values)))


def event_set(reads, read_len, distinct=64):
    """A resident set of ``reads`` event reads (dealt from ``distinct`` synthetic ones), labelled on the card, with its base table."""
    from catfish_amd import labelling
    made = [labelling.synthetic_event_read(read_len, seed=7000 + i) for i in range(min(reads, distinct))]
    dealt = [made[i % len(made)] for i in range(reads)]
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in dealt])
    return dv.DeviceValidationSet.from_events([raw for raw, _b, _l in dealt], batch, 5)


def stalled(resident, every=400, swallow=120):
    """A copy of ``resident`` whose table has one base in ``every`` swallow the ``swallow`` bases behind it, inside its read."""
    table = resident.bases
    keep = np.ones(table.n_bases + 1, dtype=bool)
    for lo, hi in zip(table.base_offsets[:-1].tolist(), table.base_offsets[1:].tolist()):
        for e in range(lo + every // 2, hi - swallow - 1, every):
            keep[e + 1:e + 1 + swallow] = False
    base_offsets = np.concatenate(([0], np.cumsum(keep[:-1])))[table.base_offsets]
    return dv.DeviceValidationSet(resident.signal, resident.labels, resident.offsets, resident.device, resident.basemap,
                                  bv.BaseTable(table.edges[keep], base_offsets))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=856)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--commit", default=None, help="stamp of the lines (default: git rev-parse HEAD)")
    ap.add_argument("--trace", type=int, default=0, help="this many vote calls at 16 thresholds and nothing else, then exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "base_votes_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    from catfish_amd.resnet_class import ResNetRNN
    if not torch.cuda.is_available():
        raise SystemExit("bench_base_votes: no GPU; the card route is not measured anywhere else")
    if args.rounds < 5 and not args.trace:
        raise SystemExit("bench_base_votes: at least five rounds")
    commit = args.commit or commit_id()
    with np.load(os.path.join(ROOT, "tests", "golden", "ckpnt-30000-inference.npz")) as z:
        weights = {k: z[k] for k in z.files}
    net = ResNetRNN(**SHIPPED)
    with contextlib.redirect_stdout(io.StringIO()):
        net.set_weights(weights)                          # the shipped checkpoint, as the validation-round bench has it
    device = torch.device("cuda", net.device)
    sixteen = tuple(float(t) for t in np.linspace(0.2, 0.95, 16))
    rows = []

    def emit(rec):
        rows.append(dict(rec, commit=commit))

    def a_round(resident, thresholds, seed):
        """One round with the votes on -> everything a stand-alone call of the step needs, the round's buffers included."""
        random.seed(seed)
        selection = resident.select(net.window, STRETCH, START, MOST)
        got = net.score_validation_device(resident, selection, thresholds, max_bases=16, vote_bases=16)
        t = net.validation_buffers["tensors"]
        bounds, _tails = dv.layout(selection[2], net.window)
        n, total = len(selection[2]), int(bounds[-1])
        a, b = bv.event_ranges(resident.bases.edges, resident.offsets[selection[0]] + selection[1], selection[2])
        return dict(selection=selection, got=got, t=t, n=n, total=total, longest=int(np.diff(bounds).max()), widest=int((b - a).max()),
                    voted=int((b - a).sum()), src_d=t["table"][:n], len_d=t["table"][n + 1:2 * n + 1], bounds_d=t["table"][2 * (n + 1):3 * (n + 1)],
                    labels=resident.device_arrays(device)[1], basemap=resident.device_basemap(device), edges=resident.device_edges(device))

    def votes_call(r, thresholds, out):
        t = r["t"]
        net.engine.base_votes_validation(t["probs"][:r["total"]], r["labels"], r["basemap"], r["edges"], r["src_d"], r["bounds_d"], r["len_d"],
                                         t["vote_ranges"][:2 * r["n"]], r["total"], r["widest"], thresholds, 16, out[:20 * len(thresholds)],
                                         out[20 * len(thresholds):], t["vote_work"])

    resident = event_set(args.reads, args.read_len)
    out = torch.empty(16 * (20 + 510), dtype=torch.int64, device=device)
    if args.trace:
        r = a_round(resident, sixteen, 0)
        for _ in range(args.trace):
            votes_call(r, sixteen, out)
        torch.cuda.synchronize()
        print(json.dumps(dict(traced="base_votes", calls=args.trace, thresholds=16, voted_bases=r["voted"])))
        return 0
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def votes_events(r, thresholds):
        begin.record()
        votes_call(r, thresholds, out)
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / 1e3

    for thresholds in ((0.5,), sixteen):
        k = len(thresholds)
        names = ("votes_call", "votes_events", "bases_call")
        seconds = {name: [] for name in names}
        for rnd in range(-1, args.rounds):                 # round -1 warms up (buffers grow once)
            r = a_round(resident, thresholds, rnd)
            t = r["t"]
            took = {"votes_call": timed(lambda: votes_call(r, thresholds, out)), "votes_events": votes_events(r, thresholds),
                    "bases_call": timed(lambda: net.engine.run_bases_validation(t["probs"][:r["total"]], t["y"][:r["total"]], r["basemap"], r["src_d"],
                                                                                r["bounds_d"], r["len_d"], r["total"], r["longest"], thresholds, 16,
                                                                                out[:k * 510], t["run_work"]))}
            if rnd >= 0:
                for name in names:
                    seconds[name].append(took[name])
                emit(dict(row="round", thresholds=k, round=rnd, **{name + "_s": took[name] for name in names}))
        stats = {name: spread(v) for name, v in seconds.items()}
        summary = dict(row="summary", thresholds=k, reads=resident.n_reads, stretch=STRETCH, rounds=args.rounds, samples_per_round=r["total"],
                       voted_bases=r["voted"], n_bases=resident.bases.n_bases,
                       called_runs=int(r["got"].base_vote_runs[0, 1].sum()), called_runs_of_16_or_more=int(r["got"].base_vote_runs[0, 1, :, :, 16].sum()), device=torch.cuda.get_device_name(device), legs=stats,
                       call_us_per_threshold={name: 1e6 * stats[name]["median_s"] / k for name in names},
                       votes_over_bases_call=stats["votes_call"]["median_s"] / stats["bases_call"]["median_s"])
        if k == 1:                                         # the definition, once, and the card's bits against it
            probs = r["t"]["probs"][:r["total"]].cpu().numpy()
            sel = r["selection"]
            t0 = time.perf_counter()
            want = bv.vote_host(probs, resident.bases.edges, resident.labels, resident.basemap, resident.offsets[sel[0]] + sel[1], sel[2],
                                dv.layout(sel[2], net.window)[0], thresholds, 16)
            summary["host_s"] = time.perf_counter() - t0
            assert np.array_equal(r["got"].base_confusion, want[2]) and np.array_equal(r["got"].base_vote_runs, want[3])
            summary["equal_to_host"] = True
        emit(summary)
        print(json.dumps(rows[-1]))

    os.environ["CATFISH_DEBUG_KNOBS"] = "1"
    for name, vset in (("short bases", resident), ("one base in 400 stalls", stalled(resident))):
        seconds = {value: [] for value in LONG_VALUES}
        longest_base, want = int(np.diff(vset.bases.edges).max()), None
        for rnd in range(-1, args.rounds):
            r = a_round(vset, sixteen, rnd)
            for value in LONG_VALUES:                      # alternating
                os.environ["CATFISH_BASE_VOTES_LONG"] = str(value)
                took = timed(lambda: votes_call(r, sixteen, out))
                tables = out.cpu().numpy().copy()
                want = tables if value == LONG_VALUES[0] else want
                assert np.array_equal(tables, want)                                   # no value changes a result
                if rnd >= 0:
                    seconds[value].append(took)
                    emit(dict(row="long_base_round", set=name, long_base=value, round=rnd, votes_call_s=took))
        del os.environ["CATFISH_BASE_VOTES_LONG"]
        emit(dict(row="long_base_summary", set=name, thresholds=16, rounds=args.rounds, n_bases=vset.bases.n_bases, voted_bases=r["voted"],
                  longest_base=longest_base, shipped_long_base=bv.LONG_BASE,
                  votes_call={str(value): spread(v) for value, v in seconds.items()}))
        print(json.dumps(rows[-1]))
    seconds = {value: [] for value in COUNT_BLOCKS}
    for rnd in range(-1, args.rounds):
        r = a_round(resident, sixteen, rnd)
        for value in COUNT_BLOCKS:                         # alternating
            os.environ["CATFISH_BASE_VOTES_COUNT_BLOCKS"] = str(value)
            took = timed(lambda: votes_call(r, sixteen, out))
            assert np.array_equal(out.cpu().numpy()[:16 * 20], r["got"].base_confusion.reshape(-1))
            if rnd >= 0:
                seconds[value].append(took)
                emit(dict(row="count_blocks_round", count_blocks=value, round=rnd, votes_call_s=took))
    del os.environ["CATFISH_BASE_VOTES_COUNT_BLOCKS"]
    emit(dict(row="count_blocks_summary", thresholds=16, rounds=args.rounds, voted_bases=r["voted"],
              votes_call={str(value): spread(v) for value, v in seconds.items()}))
    print(json.dumps(rows[-1]))
    with open(args.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
