"""Shifted-window voting on the card against the host definitions of ``catfish_amd/tilings.py``: ``cf_retile_windows`` and
``cf_vote_tilings`` through the C ABI on the trap batch (every phase set, both layouts, both weights; outputs must be EQUAL), their
refusals and hostile tables, the golden read through ``ReadPipeline`` and against the float64 oracle, every route above the engine,
and a validation round."""
import ctypes as C
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import infer, tilings
from test_tilings_host import LAYOUTS, PHASE_SETS, W, WEIGHTS, same_bits, special_values, trap_batch
from test_tilings_replay import hostile_tables

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = np.float32(-7777)
GUARD = 64


@pytest.fixture(scope="module")
def model(hp):
    from catfish_amd.resnet_class import ResNetRNN
    m = ResNetRNN(**hp)
    with np.load(os.path.join(GOLDEN, "ckpnt-30000-inference.npz")) as z:
        m.set_weights({k: z[k] for k in z.files})
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def engine(model):
    return model.engine


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def retile_abi(engine, base, offsets, lengths, phases, total=None, n_reads=None, x=None):
    """``cf_retile_windows`` straight through the C ABI on a buffer whose tiling regions and guard band hold a sentinel ->
    (the buffer [tiling size], the guard band) as the card left them.  ``phases`` go in unchecked."""
    import torch
    from catfish_amd import _native as N
    total = len(base) if total is None else total
    n_reads = len(lengths) if n_reads is None else n_reads
    size = tilings.tiling_size(max(total, 0), max(n_reads, 0), max(len(phases), 1))
    if x is None:
        x = torch.full((size + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
        x[:len(base)] = _dev(np.asarray(base, np.float32))
    d_off, d_len = _dev(np.asarray(offsets, np.int64)), _dev(np.asarray(lengths, np.int64))       # alive until the synchronise below
    N.check(engine._lib.cf_retile_windows(engine._handle, _ptr(x), _ptr(d_off), _ptr(d_len), n_reads, total, (C.c_int32 * max(len(phases), 1))(*phases), len(phases),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    engine.check_error()
    got = x.cpu().numpy()
    return got[:size], got[size:]


def vote_abi(engine, probs, logits, offsets, lengths, phases, weight, in_place=False, total=None):
    """``cf_vote_tilings`` straight through the C ABI -> (voted, voted logits or None, the inputs as the card left them)."""
    import torch
    from catfish_amd import _native as N
    total = int(offsets[-1]) if total is None else total
    d_probs, d_logits = _dev(np.asarray(probs, np.float32)), None if logits is None else _dev(np.asarray(logits, np.float32))
    out = d_probs if in_place else torch.full((total + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    lout = None if logits is None else (d_logits if in_place else torch.full((total + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda:0"))
    d_off, d_len = _dev(np.asarray(offsets, np.int64)), _dev(np.asarray(lengths, np.int64))       # alive until the synchronise below
    N.check(engine._lib.cf_vote_tilings(engine._handle, _ptr(d_probs), _ptr(d_logits), _ptr(d_off), _ptr(d_len), len(lengths), total, (C.c_int32 * max(len(phases), 1))(*phases),
                                        len(phases), weight, _ptr(out), _ptr(lout), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    engine.check_error()
    if not in_place:
        assert (out[total:] == float(SENTINEL)).all() and (lout is None or (lout[total:] == float(SENTINEL)).all())
    return out[:total].cpu().numpy(), None if lout is None else lout[:total].cpu().numpy(), d_probs.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. cf_retile_windows
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("n_reads", (1, 9))
def test_retile_equals_the_host_definition(engine, kind, n_reads):
    base, offsets, lengths = trap_batch(kind, n_reads)
    for phases in PHASE_SETS:
        got, guard = retile_abi(engine, base, offsets, lengths, phases)
        assert not (got[len(base):] == SENTINEL).any()                       # every sample of the tiling regions was written
        assert same_bits(got, tilings.retile_host(base, offsets, lengths, phases)), phases
        assert (guard == SENTINEL).all()
    got, guard = retile_abi(engine, base, offsets, lengths, (0,))             # one phase: nothing is launched
    assert same_bits(got, base) and (guard == SENTINEL).all()


def test_retile_a_misaligned_buffer_and_the_engine_wrapper(engine):
    import torch
    base, offsets, lengths = trap_batch("pipeline")
    phases = (0, 12, 23)
    size = tilings.tiling_size(len(base), 9, 3)
    want = tilings.retile_host(base, offsets, lengths, phases)
    block = torch.full((size + GUARD + 1,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    x = block[1:]                                                             # 4 bytes off a 16-byte boundary: dword stores throughout
    x[:len(base)] = _dev(base)
    got, guard = retile_abi(engine, base, offsets, lengths, phases, x=x)
    assert same_bits(got, want) and (guard == SENTINEL).all() and float(block[0]) == float(SENTINEL)
    x_all = torch.empty(size, dtype=torch.float32, device="cuda:0")
    x_all[:len(base)] = _dev(base)
    assert engine.retile_device(x_all, _dev(offsets), _dev(lengths), len(base), phases) is x_all
    torch.cuda.synchronize()
    assert same_bits(x_all.cpu().numpy(), want)
    with pytest.raises(ValueError, match="x_all needs"):
        engine.retile_device(x_all[:size - 1], _dev(offsets), _dev(lengths), len(base), phases)
    with pytest.raises(ValueError, match="first phase"):
        engine.retile_device(x_all, _dev(offsets), _dev(lengths), len(base), (1, 2))


# ------------------------------------------------------------------------------------------------ 2. cf_vote_tilings
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("phases", PHASE_SETS)
def test_vote_equals_the_host_definition(engine, kind, phases):
    _base, offsets, lengths = trap_batch(kind)
    rng = np.random.default_rng(31)
    probs, logits = special_values(rng, tilings.tiling_size(int(offsets[-1]), 9, len(phases)))
    assert (probs == 0).any() and (probs == 1).any() and (np.abs(logits) == 30).any() and ((probs > 0) & (probs < 1e-38)).any()
    for w, weight in enumerate(WEIGHTS):
        want_p, want_z = tilings.vote_host(probs, offsets, lengths, phases, weight), tilings.vote_host(logits, offsets, lengths, phases, weight)
        for in_place in (False, True):
            got_p, got_z, left = vote_abi(engine, probs, logits, offsets, lengths, phases, w, in_place)
            assert same_bits(got_p, want_p) and same_bits(got_z, want_z), (weight, in_place)
            assert same_bits(left[int(offsets[-1]):], probs[int(offsets[-1]):])          # the tilings themselves are only read
            got_p, none, _left = vote_abi(engine, probs, None, offsets, lengths, phases, w, in_place)
            assert none is None and same_bits(got_p, want_p)
    assert not same_bits(want_p, probs[:int(offsets[-1])])


def test_vote_with_one_phase_copies_and_the_engine_wrapper(engine):
    import torch
    _base, offsets, lengths = trap_batch("validation")
    total = int(offsets[-1])
    rng = np.random.default_rng(32)
    probs, logits = special_values(rng, total)
    for in_place in (False, True):
        got_p, got_z, left = vote_abi(engine, probs, logits, offsets, lengths, (0,), 1, in_place)
        assert same_bits(got_p, probs) and same_bits(got_z, logits) and same_bits(left, probs)
    phases = (0, 17)
    probs, logits = special_values(rng, tilings.tiling_size(total, 9, 2))
    d_off, d_len, d_p, d_z = _dev(offsets), _dev(lengths), _dev(probs), _dev(logits)
    voted = engine.vote_device(d_p, d_off, d_len, total, phases, "centre")
    both = engine.vote_device(d_p, d_off, d_len, total, phases, "centre", logits_all=d_z)
    torch.cuda.synchronize()
    assert same_bits(voted.cpu().numpy(), tilings.vote_host(probs, offsets, lengths, phases, "centre"))
    assert same_bits(both[0].cpu().numpy(), voted.cpu().numpy())
    assert same_bits(both[1].cpu().numpy(), tilings.vote_host(logits, offsets, lengths, phases, "centre"))
    assert engine.vote_device(d_p, d_off, d_len, total, phases, "mean", out=d_p) is d_p                  # in place
    torch.cuda.synchronize()
    assert same_bits(d_p[:total].cpu().numpy(), tilings.vote_host(probs, offsets, lengths, phases, "mean"))
    with pytest.raises(ValueError, match="vote weight"):
        engine.vote_device(d_p, d_off, d_len, total, phases, "median")
    with pytest.raises(ValueError, match="probs_all needs"):
        engine.vote_device(d_p[:total], d_off, d_len, total, phases)
    engine.check_error()


# ------------------------------------------------------------------------------------------------ 3. refusals and hostile tables
def test_refused_arguments(engine):
    import torch
    from catfish_amd import _native as N
    base, offsets, lengths = trap_batch("pipeline")
    total, n = len(base), 9
    size = tilings.tiling_size(total, n, 2)
    x, d_off, d_len = torch.zeros(size, dtype=torch.float32, device="cuda:0"), _dev(offsets), _dev(lengths)
    out = torch.zeros(total, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, h = engine._lib, engine._handle

    def ph(*p):
        return (C.c_int32 * max(len(p), 1))(*p), len(p)
    good = ph(0, 17)
    assert lib.cf_retile_windows(h, _ptr(x), _ptr(d_off), _ptr(d_len), n, total, *good, stream) == N.CF_OK
    assert lib.cf_retile_windows(None, _ptr(x), _ptr(d_off), _ptr(d_len), n, total, *good, stream) == N.CF_OK       # m may be NULL
    assert lib.cf_vote_tilings(None, _ptr(x), None, _ptr(d_off), _ptr(d_len), n, total, *good, 0, _ptr(out), None, stream) == N.CF_OK
    retile_bad = [(None, _ptr(d_off), _ptr(d_len), n, total, *good), (_ptr(x), None, _ptr(d_len), n, total, *good),
                  (_ptr(x), _ptr(d_off), None, n, total, *good), (_ptr(x), _ptr(d_off), _ptr(d_len), n, total, None, 2),
                  (_ptr(x), _ptr(d_off), _ptr(d_len), -1, total, *good), (_ptr(x), _ptr(d_off), _ptr(d_len), n, -35, *good),
                  (_ptr(x), _ptr(d_off), _ptr(d_len), n, total + 1, *good)]
    bad_phases = [ph(1, 2), ph(0, 35), ph(0, 5, 5), ph(0, 7, 3), ph(), ph(*range(9)), ph(0, -1)]
    retile_bad += [(_ptr(x), _ptr(d_off), _ptr(d_len), n, total, *p) for p in bad_phases]
    for args in retile_bad:
        with pytest.raises(ValueError):
            N.check(lib.cf_retile_windows(h, *args, stream))
    head = (_ptr(x), None, _ptr(d_off), _ptr(d_len), n, total)
    vote_bad = [(None,) + head[1:] + good + (0, _ptr(out), None), head + good + (0, None, None), head + good + (2, _ptr(out), None),
                head + good + (-1, _ptr(out), None), head + good + (0, _ptr(out), _ptr(out)),                  # logits_out without logits
                (_ptr(x), _ptr(x)) + head[2:] + good + (0, _ptr(out), None),                                # logits without logits_out
                head[:4] + (-1, total) + good + (0, _ptr(out), None), head[:4] + (n, total + 1) + good + (0, _ptr(out), None),
                (_ptr(x), None, None, _ptr(d_len), n, total) + good + (0, _ptr(out), None)]
    vote_bad += [head + p + (0, _ptr(out), None) for p in bad_phases]
    for args in vote_bad:
        with pytest.raises(ValueError):
            N.check(lib.cf_vote_tilings(h, *args, stream))
    torch.cuda.synchronize()
    engine.check_error()
    assert not x.any() and not out.any()                                       # nothing was launched by a refused call


def test_hostile_tables_give_the_defined_result(engine):
    base, offsets, lengths = trap_batch("pipeline")
    total, n, phases = len(base), len(lengths), (0, 12, 23)
    rng = np.random.default_rng(33)
    probs, logits = special_values(rng, tilings.tiling_size(total, n, 3))
    for name, offs, lens, bad, ascend in hostile_tables(offsets, lengths, total):
        got, guard = retile_abi(engine, base, offs, lens, phases, total=total)
        voted, voted_z, _left = vote_abi(engine, probs, logits, offs, lens, phases, 1, total=total)
        assert (guard == SENTINEL).all() and not (got[total:] == SENTINEL).any() and same_bits(got[:total], base), name
        if ascend:              # exactly the definition: the unsound reads zero and unvoted, the others whole
            assert same_bits(got, tilings.retile_host(base, offs, lens, phases, total=total)), name
            assert same_bits(voted, tilings.vote_host(probs, offs, lens, phases, "centre", total=total)), name
            assert same_bits(voted_z, tilings.vote_host(logits, offs, lens, phases, "centre", total=total)), name
            for r in bad:
                lo, hi = max(0, min(int(offs[r]), total)), max(0, min(int(offs[r + 1]), total))
                assert same_bits(voted[lo:hi], probs[lo:hi]), name
                for j in (1, 2):
                    t_j = tilings.tiling_start(j, total, n)
                    assert not got[t_j + lo + W * r:t_j + hi + W * (r + 1)].any(), name
        else:                   # descending offsets: every value is a zero or a sample of the base region, nothing beyond the buffers
            assert np.isin(got[total:], np.concatenate([base, [0]])).all(), name
    engine.check_error()


# ------------------------------------------------------------------------------------------------ 4. the golden read end to end
def spans_of(p, gap=0):
    bits = (np.asarray(p, np.float32) >= np.float32(0.5)).astype(np.int64)
    return [list(s) for s in infer.hp_in_pred(infer.correct_short(infer.bridge_gaps(bits, gap)))]


def voted_batch(pipe, dac):
    """Submit one read -> (ticket, x of all tilings, probabilities of all tilings, base x, voted probabilities) downloaded before
    the batch is collected."""
    t = pipe.submit([dac])
    t.done.synchronize()
    x_all = None if t.tilings is None else t.tilings[0].cpu().numpy().reshape(-1)
    probs_all = None if t.tilings is None else t.tilings[1].cpu().numpy().reshape(-1)
    return t, x_all, probs_all, t.keep[2].cpu().numpy().reshape(-1), t.keep[3].cpu().numpy().reshape(-1)


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("phases", ((0,), (0, 17), (0, 12, 23)))
def test_the_golden_read_through_the_pipeline(model, golden_read, phases, weight):
    import torch
    from catfish_amd.pipeline import ReadPipeline
    from catfish_amd.span_scores import scores_of_runs
    from test_span_scores_gpu import check_summary_rows
    dac = np.ascontiguousarray(golden_read["dac"], dtype=np.int16)
    plain = ReadPipeline(model.engine, 12000)
    today = plain.collect(plain.submit([dac]))
    for scores, gap in ((False, 0), (True, 0), (False, 3), (True, 3)):
        pipe = ReadPipeline(model.engine, 12000, phases=phases, vote_weight=weight, scores=scores, max_gap=gap)
        t, x_all, probs_all, x, voted = voted_batch(pipe, dac)
        offsets, lengths = t.s_off, t.lengths
        assert len(x) == len(voted) == 4130
        if len(phases) == 1:
            assert t.tilings is None
        else:
            assert len(x_all) == len(probs_all) == tilings.tiling_size(4130, 1, len(phases))
            assert same_bits(x_all, tilings.retile_host(x, offsets, lengths, phases))
            assert same_bits(voted, tilings.vote_host(probs_all, offsets, lengths, phases, weight))
        got = pipe.collect(t)
        assert t.tilings is None and t.keep is None
        want = spans_of(voted[:4096], gap)
        assert got[0][0] == want and got[0][1] == 4096 and len(want) >= 1
        if len(phases) == 1 and gap == 0:
            assert [r[:2] for r in got] == today
        if scores:
            runs = np.array([[s + 11, e - 16] for s, e in want], dtype=np.int64).reshape(-1, 2)
            check_summary_rows(got[0][2], scores_of_runs(voted, x, runs[:, 0], runs[:, 1], offsets, 1), voted, x)
    torch.cuda.synchronize()
    model.engine.check_error()


# ------------------------------------------------------------------------------------------------ 5. against the oracle
def test_voted_probabilities_against_the_float64_oracle(model, golden_read, ckpt_weights):
    import torch
    from oracle import catfish_oracle as oracle
    from oracle import tolerances
    bound = tolerances.GATE_MAX_ABS_DP + 2.0 ** -24            # the fp32 gate of infer_device, plus the vote's one float32 rounding
    phases = (0, 12, 23)
    reads = [infer.normalize_raw_signal(np.asarray(golden_read["dac"]), "median"),
             infer.normalize_raw_signal(oracle.synthetic_dac(1, 700, seed=41)[0], "median")]
    for sig in reads:
        n = len(sig)
        total = (n // W + 1) * W
        base = np.zeros(total, dtype=np.float32)
        base[:n] = sig
        offsets, lengths = np.array([0, total], np.int64), np.array([n], np.int64)
        x_all = tilings.retile_host(base, offsets, lengths, phases)
        want_all = oracle.forward(x_all.reshape(-1, W), ckpt_weights, np.float64).reshape(-1)      # every tiling, in float64
        d_x = _dev(x_all)
        d_off, d_len = _dev(offsets), _dev(lengths)
        probs_all = model.engine.infer_device(d_x.view(-1, W))
        for weight in WEIGHTS:
            got = model.engine.vote_device(probs_all, d_off, d_len, total, phases, weight).cpu().numpy()
            # the same vote over the oracle's float64 values, without the float32 rounding of its inputs or its result
            num, den = np.zeros(n), np.zeros(n)
            i = np.arange(n)
            for j, phi in enumerate(phases):
                w = tilings.window_weight(weight, (i + phi) % W)
                first = tilings.tiling_start(j, total, 1) + (phi if j else 0)
                num, den = num + w * want_all[first:first + n], den + w
            err = np.abs(got[:n].astype(np.float64) - num / den).max()
            print("voted against the float64 oracle:", n, weight, "max |dp| %.3g (bound %.3g)" % (err, bound))
            assert err < bound
            # and against vote_host of the float32-rounded oracle values: the route the issue names
            host = tilings.vote_host(want_all.astype(np.float32), offsets, lengths, phases, weight)
            assert np.abs(got[:n].astype(np.float64) - host[:n]).max() < bound
    torch.cuda.synchronize()
    model.engine.check_error()


def test_bf16_votes_exactly(ckpt_weights, golden_read):
    from catfish_amd.engine import HipEngine
    from catfish_amd.pipeline import ReadPipeline
    eng = HipEngine(ckpt_weights, device=0, max_windows_per_pass=4096, precision="bf16")
    try:
        dac = np.ascontiguousarray(golden_read["dac"], dtype=np.int16)
        pipe = ReadPipeline(eng, 12000, phases=(0, 12, 23), vote_weight="centre")
        t, x_all, probs_all, x, voted = voted_batch(pipe, dac)
        assert same_bits(x_all, tilings.retile_host(x, t.s_off, t.lengths, (0, 12, 23)))
        assert same_bits(voted, tilings.vote_host(probs_all, t.s_off, t.lengths, (0, 12, 23), "centre"))
        assert pipe.collect(t)[0][0] == spans_of(voted[:4096])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. the routes above the engine
@pytest.fixture(scope="module")
def route_reads(golden_read):
    from oracle import catfish_oracle as oracle
    return [np.ascontiguousarray(golden_read["dac"], dtype=np.int16)] + [oracle.synthetic_dac(1, n, seed=500 + i)[0]
                                                                         for i, n in enumerate((4096, 2500, 700, 35, 34))]


def test_the_batch_routes_and_the_runner(model, route_reads):
    from catfish_amd import batching, sharding
    dacs = route_reads
    sigs = [infer.normalize_raw_signal(d, "median") for d in dacs]
    changed = {}
    for phases, weight in (((0,), "mean"), ((0, 17), "mean"), ((0, 12, 23), "centre")):
        kw = dict(phases=phases, vote_weight=weight)
        got, probs = batching.infer_reads_dac(model, dacs, return_probs=True, **kw)
        assert [(s, n) for s, n in got] == [(spans_of(p), len(d)) for p, d in zip(probs, dacs)]
        assert batching.infer_reads_dac(model, dacs, **kw) == got
        packed = batching.pack_reads(sigs)
        res, probs = batching.infer_packed(model.engine, packed, return_probs=True, **kw)
        assert res == [(spans_of(p), len(d)) for p, d in zip(probs, dacs)]
        assert batching.infer_reads(model, sigs, **kw) == res
        assert batching.infer_reads(model, sigs, max_windows=150, **kw) == res                     # several buckets
        res3 = batching.infer_packed(model.engine, packed, max_gap=3, **kw)
        assert res3 == [(spans_of(p, 3), len(d)) for p, d in zip(probs, dacs)]
        runner = sharding.EngineBatchRunner(model, 12000, **kw)
        assert runner.phases == phases and runner.pipe.phases == phases and runner.vote_weight == weight
        # the runner cuts other batches than infer_reads_dac's one bucket: windows are independent, so the spans are the same
        assert [r for b in runner.run([dacs[:2], dacs[2:]]) for r in b] == got
        floats = [infer.normalize_raw_signal(s, "median") for s in sigs[:3]]
        assert [r for b in runner.run([sigs[:3]]) for r in b] == batching.infer_reads(model, floats, max_windows=12000 // 35, **kw)
        # one read at a time: the same batch composition as a packed launch of that read alone
        for sig in sigs:
            (alone,), (p,) = batching.infer_packed(model.engine, batching.pack_reads([sig]), return_probs=True, **kw)
            assert alone == (spans_of(p), len(sig)) and infer.infer_class_from_raw(sig, model, **kw) == alone
            assert infer.infer_class_from_raw(sig, model, max_gap=3, **kw) == (spans_of(p, 3), len(sig))
        spans, n, rows = infer.infer_class_from_raw(sigs[0], model, scores=True, **kw)
        assert (spans, n) == batching.infer_packed(model.engine, batching.pack_reads(sigs[:1]), **kw)[0] and rows.shape == (len(spans), 6)
        if len(phases) == 1:
            assert batching.infer_reads_dac(model, dacs) == got and batching.infer_reads(model, sigs) == res
            plain = got
        else:
            changed[phases] = sum(a != b for a, b in zip(got, plain))
    assert changed[(0, 17)] >= 1 and changed[(0, 12, 23)] >= 1      # voting did something on these reads
    for call in (lambda: batching.infer_reads_dac(model, dacs, phases=(0, 35)), lambda: batching.infer_reads(model, sigs, phases=(1, 2)),
                 lambda: sharding.EngineBatchRunner(model, 12000, phases=(0, 5, 5)),
                 lambda: batching.infer_packed(model.engine, batching.pack_reads(sigs), phases=(0, 5), vote_weight="median")):
        with pytest.raises(ValueError):
            call()
    model.engine.check_error()


def test_run_pipeline_and_the_command_line(tmp_path, ckpt_weights, route_reads, monkeypatch):
    import contextlib
    import io
    import json
    from click.testing import CliRunner
    from catfish_amd import batching, cli, neural_network
    from test_gpu_pipeline import _write_model_dir
    net = _write_model_dir(tmp_path, ckpt_weights)
    reads = tmp_path / "reads"
    reads.mkdir()
    for i, d in enumerate(route_reads[:4]):
        np.save(reads / ("read_%d.npy" % i), d)
    names = ["read_%d.npy" % i for i in range(4)]
    model = neural_network.load_network("ResNetRNN", str(net), checkpoint=30000, device=0, max_windows_per_pass=32768)
    docs = {}
    for phases in ((0,), (0, 17)):
        spans = batching.infer_reads_dac(model, route_reads[:4], phases=phases, vote_weight="centre")
        want_hp, want_non = {}, {}
        for name, (sp, length) in zip(names, spans):
            merged, non = cli.chunks_of_read([list(v) for v in sp], length, 300)
            if merged is not None:
                want_hp[name] = merged
            want_non[name] = json.loads(json.dumps(non))
        out = tmp_path / ("out%d" % len(phases))
        with contextlib.redirect_stdout(io.StringIO()):
            res = cli.run_pipeline(str(reads), str(out), chunk_size=300, network_path=str(net), device=0, phases=phases, vote_weight="centre")
        assert res["reads"] == 4
        docs[phases] = (json.load(open(out / "TEMP" / "hp_positions.json")), json.load(open(out / "TEMP" / "nonhp_positions.json")))
        assert docs[phases] == (want_hp, want_non)
    model.engine.close()
    monkeypatch.chdir(tmp_path)                                # the command line resolves "ResNetRNN" relative to the CWD
    monkeypatch.setenv("CATFISH_TILINGS", "0,17")
    monkeypatch.setenv("CATFISH_TILING_WEIGHT", "centre")
    done = CliRunner().invoke(cli._build_click_main(), ["-i", str(reads), "-s", str(tmp_path / "cli"), "-c", "300"])
    assert done.exit_code == 0, done.output
    assert json.load(open(tmp_path / "cli" / "TEMP" / "hp_positions.json")) == docs[(0, 17)][0]
    assert json.load(open(tmp_path / "cli" / "TEMP" / "nonhp_positions.json")) == docs[(0, 17)][1]
    monkeypatch.setenv("CATFISH_TILINGS", "0,40")
    bad = CliRunner().invoke(cli._build_click_main(), ["-i", str(reads), "-s", str(tmp_path / "bad"), "-c", "300", "-g", "2"])
    assert bad.exit_code != 0 and "CATFISH_TILINGS" in str(bad.exception) and not (tmp_path / "bad").exists()


# ------------------------------------------------------------------------------------------------ 7. validation
def test_a_validation_round_and_the_sweep(hp):
    from catfish_amd import train_validate as tv
    from catfish_amd.device_validation import DeviceValidationSet
    from catfish_amd.resnet_class import ResNetRNN
    signals, labels = [], []
    for i, n in enumerate((35, 70, 71, 0, 1500, 333)):
        raw, lab = tv.synthetic_labelled_read(max(n, 40), seed=80 + i)
        signals.append(np.asarray(raw, dtype=np.float64)[:n])
        labels.append(np.asarray(lab)[:n])
    resident = DeviceValidationSet.from_arrays(signals, labels)
    selection = resident.select(35, 0, "complete", 856)
    assert selection[2].tolist() == [35, 70, 71, 0, 1500, 333]
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    try:
        ths, edges, reach, phases = (0.5, 0.45), (35,), 8, (0, 17)
        plain = net.score_validation_device(resident, selection, ths, run_edges=edges, border_reach=reach, curve_shift=14)
        assert net.validation_buffers["allocations"] == 1 and "tiling_samples" not in net.validation_buffers["capacity"]
        same = net.score_validation_device(resident, selection, ths, run_edges=edges, border_reach=reach, curve_shift=14, phases=(0,))
        assert all(np.array_equal(a, b) for a, b in zip(plain, same)) and net.validation_buffers["allocations"] == 1
        bounds, _tails = dv.layout(selection[2], 35)
        total, n = int(bounds[-1]), len(selection[2])
        for weight in WEIGHTS:
            got = net.score_validation_device(resident, selection, ths, run_edges=edges, border_reach=reach, curve_shift=14, phases=phases,
                                              vote_weight=weight)
            assert net.validation_buffers["allocations"] == 2                  # grown once for the tilings, not again
            assert net.validation_buffers["capacity"]["tiling_samples"] == tilings.tiling_size(total, n, 2)
            t = net.validation_buffers["tensors"]
            size = tilings.tiling_size(total, n, 2)
            x_all, probs_all, logits_all = (t[k][:size].cpu().numpy() for k in ("tilings_x", "tilings_probs", "tilings_logits"))
            y = t["y"][:total].cpu().numpy()
            assert same_bits(x_all, tilings.retile_host(resident.pack(selection, 35)[0].reshape(-1), bounds, selection[2], phases))
            probs = tilings.vote_host(probs_all, bounds, selection[2], phases, weight)
            logits = tilings.vote_host(logits_all, bounds, selection[2], phases, weight)
            assert same_bits(t["probs"][:total].cpu().numpy(), probs) and same_bits(t["logits"][:total].cpu().numpy(), logits)
            right, ce_sum, counts = dv.score_host(probs, logits, y, bounds, ths)
            assert np.array_equal(got[0], right) and np.array_equal(got[2], counts)
            np.testing.assert_allclose(got[1], ce_sum, rtol=1e-11, atol=0)
            assert np.array_equal(got[3], dv.run_states_host(probs, y, bounds, selection[2], ths, edges, 15))
            assert np.array_equal(got[4], dv.run_borders_host(probs, y, bounds, selection[2], ths, reach, 15))
            assert np.array_equal(got[5], dv.curve_host(probs, y, bounds, selection[2], 14))
            assert not same_bits(probs, probs_all[:total])
        net.score_validation_device(resident, selection, ths, run_edges=edges, border_reach=reach, curve_shift=14, phases=phases)
        assert net.validation_buffers["allocations"] == 2
        # the sweeps
        rows = tv.threshold_sweep(net, resident, ths, 0, run_edges=edges, border_reach=reach, phases=phases, vote_weight="centre")
        assert [(r["tp"], r["fp"], r["fn"]) for r in rows] == [tuple(int(v) for v in (c[0], c[1], c[3])) for c in got[2]]
        assert tv.threshold_sweep(net, resident, ths, 0, phases=(0,)) == tv.threshold_sweep(net, resident, ths, 0)
        sets = ((0,), (0, 17), (0, 12, 23))
        sweep = tv.tiling_sweep(net, resident, sets, 0, weight="centre", run_edges=edges, border_reach=reach)
        assert [r["phases"] for r in sweep] == [list(s) for s in sets] and all(r["weight"] == "centre" for r in sweep)
        for key in ("tp", "fp", "tn", "fn", "precision", "recall", "f1", "hp_complete", "hp_found", "called_absent", "hp_interrupted",
                    "called_interrupted"):
            assert all(key in r for r in sweep)
        first = tv.threshold_sweep(net, resident, [0.5], 0, run_edges=edges, border_reach=reach)[0]
        assert all(sweep[0][k] == first[k] for k in ("tp", "fp", "tn", "fn", "f1", "hp_found"))
        assert (sweep[1]["tp"], sweep[1]["fp"], sweep[1]["fn"]) == (rows[0]["tp"], rows[0]["fp"], rows[0]["fn"])
        with pytest.raises(ValueError):
            net.score_validation_device(resident, selection, ths, phases=(0, 35))
        net.engine.check_error()
    finally:
        net.engine.close()
