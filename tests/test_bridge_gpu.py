"""Bridging on the card against the host definition (``infer.bridge_gaps`` + ``correct_short`` per read): ``cf_postprocess_spans_bridged``
on the traps and the random batch of tests/test_bridge_host.py for every (max_gap, min_run) pair and both thresholds -- labels, run
lists and counts must be EQUAL --, ``cf_span_scores_labels`` over the bridged runs, the two bridged validation calls, and the golden
read through the pipeline and ``infer_class_from_raw`` with the bundled checkpoint."""
import ctypes as C
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import infer
from catfish_amd.span_scores import scores_of_runs
from test_bridge_host import PAIRS, REFUSED, THRESHOLDS, UNBRIDGED, host_bridged, random_batch, trap_batch
from test_span_scores_host import check_rows, planted_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = -7777


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


def on_device(batch):
    probs, offsets, lengths = batch[:3]
    rng = np.random.default_rng(len(probs))
    signal = (rng.standard_normal(len(probs)) * 1.5 + 0.25).astype(np.float32)
    return {"host": (probs, offsets, lengths), "signal_host": signal, "probs": _dev(np.array(probs)), "signal": _dev(signal),
            "offsets": _dev(offsets), "lengths": _dev(lengths)}


@pytest.fixture(scope="module")
def batches():
    return {"traps": on_device(trap_batch()), "random": on_device(random_batch())}


def bridged_on_device(engine, case, threshold, max_gap, min_run, labels=True, max_runs=None, plain=False):
    """One call of cf_postprocess_spans_bridged (``plain``: of cf_postprocess_spans) straight through the C ABI -> (labels or None,
    starts, ends as the card listed them up to max_runs, counts)."""
    import torch
    from catfish_amd import _native as N
    total, n_reads = len(case["host"][0]), len(case["host"][2])
    if max_runs is None:
        max_runs = total // min_run + 16
    lab = torch.full((total,), 7, dtype=torch.uint8, device="cuda:0") if labels else None
    starts = torch.full((max(max_runs, 1),), SENTINEL, dtype=torch.int64, device="cuda:0")
    ends = torch.full((max(max_runs, 1),), SENTINEL, dtype=torch.int64, device="cuda:0")
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (engine._handle, C.c_void_p(case["probs"].data_ptr()), C.c_void_p(case["offsets"].data_ptr()),
            C.c_void_p(case["lengths"].data_ptr()), n_reads, total, float(threshold))
    tail = (C.c_void_p(lab.data_ptr()) if labels else None, max_runs, C.c_void_p(starts.data_ptr()) if max_runs else None,
            C.c_void_p(ends.data_ptr()) if max_runs else None, C.c_void_p(counts.data_ptr()), stream)
    if plain:
        N.check(engine._lib.cf_postprocess_spans(*head, min_run, *tail))
    else:
        N.check(engine._lib.cf_postprocess_spans_bridged(*head, max_gap, min_run, *tail))
    torch.cuda.synchronize()
    engine.check_error()
    return (lab.cpu().numpy() if labels else None, starts.cpu().numpy(), ends.cpu().numpy(), counts.cpu().numpy())


def check_against_host(got, want):
    labels, starts, ends, counts = got
    n = len(want[1])
    assert counts.tolist() == [n, n]
    if labels is not None:
        assert np.array_equal(labels, want[0])
    assert np.array_equal(np.sort(starts[:n]), want[1]) and np.array_equal(np.sort(ends[:n]), want[2])
    assert (starts[n:] == SENTINEL).all() and (ends[n:] == SENTINEL).all()


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("max_gap,min_run", PAIRS + UNBRIDGED)
def test_labels_and_runs_equal_the_host_definition(engine, batches, threshold, max_gap, min_run):
    for name in ("traps", "random"):
        case = batches[name]
        want = host_bridged(*case["host"], threshold, max_gap, min_run)
        if name == "random" and max_gap:
            assert want[3] >= 50 and want[4] >= 50             # gaps filled, interior gaps kept: the case shows something
        check_against_host(bridged_on_device(engine, case, threshold, max_gap, min_run), want)
        # labels NULL: the same lists
        check_against_host(bridged_on_device(engine, case, threshold, max_gap, min_run, labels=False), want)


def test_max_runs_0_and_a_truncated_list_report_the_true_counts(engine, batches):
    case = batches["random"]
    want = host_bridged(*case["host"], 0.5, 5, 15)
    n = len(want[1])
    assert n > 40
    labels, starts, ends, counts = bridged_on_device(engine, case, 0.5, 5, 15, max_runs=0)
    assert np.array_equal(labels, want[0]) and counts.tolist() == [n, n] and starts[0] == SENTINEL and ends[0] == SENTINEL
    labels, starts, ends, counts = bridged_on_device(engine, case, 0.5, 5, 15, labels=False, max_runs=0)
    assert counts.tolist() == [n, n]
    labels, starts, ends, counts = bridged_on_device(engine, case, 0.5, 5, 15, max_runs=7)
    assert np.array_equal(labels, want[0]) and counts.tolist() == [n, n]
    assert set(starts.tolist()) <= set(want[1].tolist()) and set(ends.tolist()) <= set(want[2].tolist()) and len(set(starts.tolist())) == 7
    # the wrapper asks again with room for all of them
    got = engine.postprocess_spans_device(case["probs"], case["offsets"], case["lengths"], 0.5, 15, max_runs=7, max_gap=5)
    assert np.array_equal(got[0], want[1]) and np.array_equal(got[1], want[2])


@pytest.mark.parametrize("min_run", (1, 15, 64))
def test_max_gap_0_is_the_unbridged_call_bit_for_bit(engine, batches, min_run):
    for case in batches.values():
        for threshold in THRESHOLDS:
            a = bridged_on_device(engine, case, threshold, 0, min_run)
            b = bridged_on_device(engine, case, threshold, 0, min_run, plain=True)
            assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
            n = int(a[3][0])
            assert np.sort(a[1][:n]).tobytes() == np.sort(b[1][:n]).tobytes() and np.sort(a[2][:n]).tobytes() == np.sort(b[2][:n]).tobytes()


@pytest.mark.parametrize("max_gap,min_run", REFUSED + ((-1, 15),))
def test_refused_pairs(engine, batches, max_gap, min_run):
    import torch
    from catfish_amd.pipeline import ReadPipeline
    case = batches["random"]
    with pytest.raises(ValueError):                            # the library, before any launch
        bridged_on_device(engine, case, 0.5, max_gap, min_run)
    with pytest.raises(ValueError):
        engine.postprocess_spans_device(case["probs"], case["offsets"], case["lengths"], 0.5, min_run, max_gap=max_gap)
    with pytest.raises(ValueError):
        ReadPipeline(engine, 12000, min_run=min_run, max_gap=max_gap)
    torch.cuda.synchronize()
    engine.check_error()


def test_an_unaligned_labels_pointer_is_refused(engine, batches):
    import torch
    from catfish_amd import _native as N
    case = batches["random"]
    total = len(case["host"][0])
    lab = torch.zeros(total + 16, dtype=torch.uint8, device="cuda:0")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):
        N.check(engine._lib.cf_postprocess_spans_bridged(
            engine._handle, C.c_void_p(case["probs"].data_ptr()), C.c_void_p(case["offsets"].data_ptr()),
            C.c_void_p(case["lengths"].data_ptr()), len(case["host"][2]), total, 0.5, 3, 15, C.c_void_p(lab.data_ptr() + 1), 0, None, None,
            C.c_void_p(counts.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    engine.check_error()


# ------------------------------------------------------------------------------------------------ scores over bridged runs
def rows_of_runs(probs, signal, offsets, starts, ends):
    """``test_span_scores_host.brute_force``'s rows for given runs."""
    rows = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        ps, xs = [float(v) for v in probs[s:e]], [float(v) for v in signal[s:e]]
        rows.append({"read": int(np.searchsorted(offsets[:-1], s, side="right") - 1), "start": s, "end": e, "p": ps, "x": xs,
                     "x2": [v * v for v in xs], "min_p": probs[s:e].min(), "max_p": probs[s:e].max()})
    return rows


@pytest.mark.parametrize("max_gap,min_run", ((5, 15), (49, 15), (8, 1)))
def test_scores_of_the_bridged_runs(engine, batches, max_gap, min_run):
    case = batches["random"]
    probs, offsets, lengths = case["host"]
    want = host_bridged(probs, offsets, lengths, 0.5, max_gap, min_run)
    starts, ends, lab, got = engine.postprocess_spans_device(case["probs"], case["offsets"], case["lengths"], 0.5, min_run, labels=True,
                                                             scores=True, signal=case["signal"], max_gap=max_gap)
    assert np.array_equal(starts, want[1]) and np.array_equal(ends, want[2]) and np.array_equal(lab.cpu().numpy(), want[0])
    host = scores_of_runs(np.asarray(probs), case["signal_host"], want[1], want[2], offsets, len(lengths))
    for key in ("start", "end", "read", "min_p", "max_p"):
        assert got[key].dtype == host[key].dtype and got[key].tobytes() == host[key].tobytes(), key
    assert (got["min_p"] < 0.5).sum() >= 20                    # runs that hold samples below the threshold: the bridged gaps count
    check_rows(got, rows_of_runs(probs, case["signal_host"], offsets, want[1], want[2]))
    # without the signal the level columns are NaN, the rest the same
    _s, _e, bare = engine.postprocess_spans_device(case["probs"], case["offsets"], case["lengths"], 0.5, min_run, scores=True, max_gap=max_gap)
    assert bare["sum_p"].tobytes() == got["sum_p"].tobytes() and np.isnan(bare["sum_x"]).all()


def test_hostile_start_lists_by_labels(engine):
    """The start list of tests/test_span_scores_gpu.py (-1, total, beyond, padding, mid-run, honest, int64 extremes) walked by labels."""
    import torch
    from test_span_scores_replay import check_hostile_rows, hostile_starts
    host = planted_batch()
    probs, signal, offsets, lengths = host
    case = {"host": (probs, offsets, lengths), "probs": _dev(probs), "offsets": _dev(offsets), "lengths": _dev(lengths)}
    labels = bridged_on_device(engine, case, 0.5, 0, 15)[0]
    starts, expect = hostile_starts(host)
    m = len(starts)
    for with_signal in (True, False):
        out = (torch.full((m,), SENTINEL, dtype=torch.int64, device="cuda:0"), torch.full((m, 3), float(SENTINEL), dtype=torch.float64, device="cuda:0"),
               torch.full((m, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0"))
        engine.span_scores_device(case["probs"], _dev(signal) if with_signal else None, case["offsets"], case["lengths"],
                                  _dev(np.asarray(starts, dtype=np.int64)), _dev(np.array([m, m], np.int64)), out=out, labels=_dev(labels))
        torch.cuda.synchronize()
        engine.check_error()
        ends, sums, extremes = (t.cpu().numpy() for t in out)
        check_hostile_rows(host, starts, expect, ends, sums, extremes, with_signal=with_signal)


def test_a_start_inside_a_bridged_gap_is_walked_by_the_labels(engine, batches):
    """Where the walk by labels differs from the walk by threshold: a start on a sample BELOW the threshold inside a bridged run goes
    on to the run's end (by threshold it would be an empty walk); the same start with unbridged labels gets a row of no samples."""
    import torch
    from test_span_scores_replay import check_hostile_rows
    case = batches["traps"]
    probs, offsets, lengths = case["host"]
    signal = case["signal_host"]
    host = (np.asarray(probs), signal, offsets, lengths)
    bridged = bridged_on_device(engine, case, 0.5, 5, 15)[0]
    plain = bridged_on_device(engine, case, 0.5, 0, 15)[0]
    # the gap of four at the workgroup edge, its run [12713, 16679) -- and the chain 5 3 5 3 5, a call only when bridged
    a, b = 15870, 15874
    assert not (probs[a:b] >= 0.5).any() and bridged[a:b].all() and not plain[a:b].any()
    want = host_bridged(probs, offsets, lengths, 0.5, 5, 15)
    end = int(want[2][np.searchsorted(want[2], a, side="right")])
    assert bridged[a:end].all() and not bridged[end] and end - a > 700
    starts = [a, a + 3, 205, 208, -1, len(probs)]             # 205: the chain's first gap (below the threshold), 208: a one behind it
    expect = [(a, end), (a + 3, end), (205, 221), (208, 221), None, None]
    for labels, rows in ((bridged, expect), (plain, [(a, a), (a + 3, a + 3), (205, 205), (208, 208), None, None])):
        m = len(starts)
        out = (torch.full((m,), SENTINEL, dtype=torch.int64, device="cuda:0"), torch.full((m, 3), float(SENTINEL), dtype=torch.float64, device="cuda:0"),
               torch.full((m, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0"))
        engine.span_scores_device(case["probs"], case["signal"], case["offsets"], case["lengths"], _dev(np.asarray(starts, dtype=np.int64)),
                                  _dev(np.array([m, m], np.int64)), out=out, labels=_dev(labels))
        torch.cuda.synchronize()
        engine.check_error()
        ends, sums, extremes = (t.cpu().numpy() for t in out)
        if labels is bridged:
            check_hostile_rows(host, starts, rows, ends, sums, extremes)
            assert extremes[0, 0] == np.float32(0.1) and extremes[2, 0] == np.float32(0.1)      # the gap's samples are in the row
        else:                                                  # no label at the start: the walk takes nothing
            assert ends.tolist() == [s for s in starts] and (sums == 0).all() and (extremes[:, 0] == np.inf).all()


# ------------------------------------------------------------------------------------------------ validation
@pytest.fixture(scope="module")
def validation_case():
    """The random batch as a validation round packs it, with a seeded truth of 6 % ones in runs; references computed once."""
    probs, offsets, lengths = random_batch()
    rng = np.random.default_rng(6)
    y = np.zeros(len(probs), np.uint8)
    for beg, n in zip(offsets[:-1].tolist(), lengths.tolist()):
        i = 0
        while i < n:
            if rng.random() < 0.06 / 20:
                d = int(rng.integers(8, 40))
                y[beg + i:beg + min(n, i + d)] = 1
                i += d
            i += 1
    assert 0.03 < y.mean() < 0.12
    case = {"host": (np.asarray(probs), y, offsets, lengths), "probs": _dev(np.array(probs)), "y": _dev(y), "bounds": _dev(offsets),
            "length": _dev(lengths), "total": int(offsets[-1]), "longest": int(np.diff(offsets).max()), "states": {}, "borders": {}}
    for gap in (0, 3, 15):
        case["states"][gap] = dv.run_states_host(*case["host"], THRESHOLDS, (15, 40), 15, max_gap=gap)
        case["borders"][gap] = dv.run_borders_host(*case["host"], THRESHOLDS, 16, 15, max_gap=gap)
    return case


@pytest.mark.parametrize("gap", (0, 3, 15))
def test_the_bridged_validation_calls(engine, validation_case, gap):
    import torch
    case = validation_case
    k, edges, reach = len(THRESHOLDS), (15, 40), 16
    work = torch.full((max(engine.run_states_work_bytes(case["total"], k), 1),), 7, dtype=torch.uint8, device="cuda:0")
    states = torch.full((k * 2 * 3 * 3,), -1, dtype=torch.int64, device="cuda:0")
    borders = torch.full((k * 2 * (5 * reach + 3),), -1, dtype=torch.int64, device="cuda:0")
    args = (case["probs"], case["y"], case["bounds"], case["length"], case["total"], case["longest"], THRESHOLDS)
    engine.run_states_validation(*args, edges, states, work, max_gap=gap)
    engine.run_borders_validation(*args, reach, borders, work, max_gap=gap)
    torch.cuda.synchronize()
    engine.check_error()
    got_states, got_borders = states.cpu().numpy().reshape(k, 2, 3, 3), borders.cpu().numpy().reshape(k, 2, -1)
    print("gap", gap, "true runs complete / incomplete / absent at 0.5:", got_states[0, 0].sum(axis=0).tolist(),
          "interrupted:", got_borders[0, :, -1].tolist())
    assert np.array_equal(got_states, case["states"][gap]) and np.array_equal(got_borders, case["borders"][gap])
    if gap == 0:                                               # the existing calls, untouched
        engine.run_states_validation(*args, edges, states, work)
        engine.run_borders_validation(*args, reach, borders, work)
        torch.cuda.synchronize()
        assert np.array_equal(states.cpu().numpy().reshape(k, 2, 3, 3), got_states)
        assert np.array_equal(borders.cpu().numpy().reshape(k, 2, -1), got_borders)
    else:
        assert not np.array_equal(got_states, case["states"][0]) and not np.array_equal(got_borders, case["borders"][0])
        # bridging only adds ones to the prediction: no true run can become absent, and here some are found that were not
        assert got_states[0, 0, :, 2].sum() < case["states"][0][0, 0, :, 2].sum()


def validation_direct(engine, case, what, max_gap, edges=(15, 40), reach=16, min_run=15):
    """``cf_validation_run_states`` / ``_borders`` (``max_gap`` None) or their ``_bridged`` forms straight through the C ABI ->
    the table as the card wrote it (filled with -1 before)."""
    import torch
    from catfish_amd import _native as N
    k = len(THRESHOLDS)
    cells = 2 * (len(edges) + 1) * 3 if what == "states" else 2 * (5 * reach + 3)
    out = torch.full((k * cells,), -1, dtype=torch.int64, device="cuda:0")
    work = torch.full((max(engine.run_states_work_bytes(case["total"], k), 1),), 7, dtype=torch.uint8, device="cuda:0")
    head = [engine._handle, C.c_void_p(case["probs"].data_ptr()), C.c_void_p(case["y"].data_ptr()), C.c_void_p(case["bounds"].data_ptr()),
            C.c_void_p(case["length"].data_ptr()), len(case["host"][3]), case["total"], case["longest"], (C.c_double * k)(*THRESHOLDS), k]
    head += [(C.c_int64 * len(edges))(*edges), len(edges)] if what == "states" else [reach]
    tail = [min_run, C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), int(work.numel()),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    name = "cf_validation_run_%s" % what + ("" if max_gap is None else "_bridged")
    N.check(getattr(engine._lib, name)(*(head + ([] if max_gap is None else [max_gap]) + tail)))
    torch.cuda.synchronize()
    engine.check_error()
    return out.cpu().numpy()


def test_the_bridged_symbols_at_gap_0_equal_the_existing_calls(engine, validation_case):
    for what in ("states", "borders"):
        old = validation_direct(engine, validation_case, what, None)
        new = validation_direct(engine, validation_case, what, 0)
        assert (old >= 0).all() and old.sum() > 0 and new.tobytes() == old.tobytes()
        assert np.array_equal(new.reshape(validation_case[what][0].shape), validation_case[what][0])
        for min_run in (1, 64):                                # the corners of the unbridged domain
            assert validation_direct(engine, validation_case, what, 0, min_run=min_run).tobytes() == \
                validation_direct(engine, validation_case, what, None, min_run=min_run).tobytes()
        # ... and with a gap the symbol itself (not the engine's wrapper) gives the host definition
        got = validation_direct(engine, validation_case, what, 3)
        assert np.array_equal(got.reshape(validation_case[what][3].shape), validation_case[what][3])


def test_the_validation_calls_refuse_what_the_kernel_does_not_cover(engine, validation_case):
    import torch
    case = validation_case
    work = torch.zeros(max(engine.run_states_work_bytes(case["total"], 1), 1) + 16, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(2 * (5 * 16 + 3), dtype=torch.int64, device="cuda:0")
    args = (case["probs"], case["y"], case["bounds"], case["length"], case["total"], case["longest"], (0.5,))
    for max_gap, min_run in REFUSED:
        with pytest.raises(ValueError):
            engine.run_states_validation(*args, (), out, work, min_run=min_run, max_gap=max_gap)
        with pytest.raises(ValueError):
            engine.run_borders_validation(*args, 16, out, work, min_run=min_run, max_gap=max_gap)
    with pytest.raises(ValueError):                            # a work buffer the bit-mask kernel cannot store into
        engine.run_states_validation(*args, (), out, work[1:], max_gap=3)
    torch.cuda.synchronize()
    engine.check_error()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("gap", (0, 3, 15))
def test_the_golden_read_end_to_end(model, golden_read, gap):
    import torch
    from catfish_amd.pipeline import ReadPipeline
    from test_span_scores_gpu import check_summary_rows
    dac = np.ascontiguousarray(golden_read["dac"], dtype=np.int16)
    plain = ReadPipeline(model.engine, 12000)
    today = plain.collect(plain.submit([dac]))
    for scores in (False, True):
        pipe = ReadPipeline(model.engine, 12000, max_gap=gap, scores=scores)
        t = pipe.submit([dac])
        t.done.synchronize()
        assert (t.labels is not None) == (scores and gap > 0)      # labels are written only for the scores of bridged runs
        x, probs = t.keep[2].cpu().numpy().reshape(-1), t.keep[3].cpu().numpy()      # what the batch's kernels saw
        _lab, starts, ends, _f, _k = host_bridged(probs, t.s_off, t.lengths, 0.5, gap, 15)
        got = pipe.collect(t)
        assert got[0][0] == [[int(s) - 11, int(e) + 16] for s, e in zip(starts, ends)] and got[0][1] == 4096 and len(starts) >= 1
        if gap == 0:
            assert [r[:2] for r in got] == today
        if scores:
            check_summary_rows(got[0][2], scores_of_runs(probs, x, starts, ends, t.s_off, 1), probs, x)
    # one read through infer_class_from_raw
    sig = infer.normalize_raw_signal(dac, "median")
    raw_in = infer.reshape_input(np.hstack((sig, np.zeros(infer.padding_size_for(4096)))), 35, 1)
    x = np.ascontiguousarray(raw_in, dtype=np.float32).reshape(-1)
    probs = model.engine.infer_device(_dev(x).view(-1, 35)).cpu().numpy().reshape(-1)      # what the card produced, downloaded
    _lab, starts, ends, _f, _k = host_bridged(probs, np.array([0, len(x)]), np.array([4096]), 0.5, gap, 15)
    spans_want = [[int(s) - 11, int(e) + 16] for s, e in zip(starts, ends)]
    assert infer.infer_class_from_raw(sig, model, max_gap=gap) == (spans_want, 4096)
    spans, length, rows = infer.infer_class_from_raw(sig, model, max_gap=gap, scores=True)
    assert (spans, length) == (spans_want, 4096)
    check_summary_rows(rows, scores_of_runs(probs, x, starts, ends, [0, len(x)], 1), probs, x)
    if gap == 0:
        assert infer.infer_class_from_raw(sig, model) == (spans_want, 4096)
    torch.cuda.synchronize()
    model.engine.check_error()


# ------------------------------------------------------------------------------------------------ the routes above the engine
def host_spans(p, gap, min_run=15, threshold=0.5):
    """One read's spans by the definition, from its real samples' probabilities."""
    from test_bridge_host import bits_of
    return [list(s) for s in infer.hp_in_pred(infer.correct_short(infer.bridge_gaps(bits_of(p, threshold), gap), min_run))]


@pytest.fixture(scope="module")
def route_reads(golden_read):
    from oracle import catfish_oracle as oracle
    return [np.ascontiguousarray(golden_read["dac"], dtype=np.int16)] + [oracle.synthetic_dac(1, n, seed=500 + i)[0]
                                                                         for i, n in enumerate((4096, 2500, 700, 35, 34))]


def test_the_batch_routes_and_the_runner(model, route_reads):
    """``infer_reads_dac``, ``infer_packed`` / ``infer_reads`` and ``EngineBatchRunner`` (pipeline route for DAC reads, host route for
    float traces) with a gap: the spans are the definition applied to the probabilities the card produced for the same batch."""
    from catfish_amd import batching, sharding
    dacs = route_reads
    sigs = [infer.normalize_raw_signal(d, "median") for d in dacs]
    changed = 0
    for gap in (0, 3, 15):
        got, probs = batching.infer_reads_dac(model, dacs, max_gap=gap, return_probs=True)
        want = [(host_spans(p, gap), len(d)) for p, d in zip(probs, dacs)]
        assert [(s, n) for s, n in got] == want and batching.infer_reads_dac(model, dacs, max_gap=gap) == got
        packed = batching.pack_reads(sigs)
        res, probs = batching.infer_packed(model.engine, packed, return_probs=True, max_gap=gap)
        assert res == [(host_spans(p, gap), len(d)) for p, d in zip(probs, dacs)]
        assert batching.infer_reads(model, sigs, max_gap=gap) == res
        assert batching.infer_reads(model, sigs, max_windows=150, max_gap=gap) == res           # several buckets
        runner = sharding.EngineBatchRunner(model, 12000, max_gap=gap)
        assert runner.max_gap == gap and runner.pipe.max_gap == gap
        batches = [dacs[:2], dacs[2:]]
        assert [r for b in runner.run(batches) for r in b] == got
        # float traces take the host normalisation and ``batching.infer_reads``
        floats = [infer.normalize_raw_signal(s, "median") for s in sigs[:3]]
        assert [r for b in runner.run([sigs[:3]]) for r in b] == batching.infer_reads(model, floats, max_windows=12000 // 35, max_gap=gap)
        if gap == 0:
            assert batching.infer_reads_dac(model, dacs) == got and batching.infer_reads(model, sigs) == res
            plain = got
        else:
            changed += sum(a != b for a, b in zip(got, plain))
            with pytest.raises(ValueError):
                batching.infer_reads_dac(model, dacs, min_run=64, max_gap=gap)
    assert changed >= 2                                        # the gap did something on these reads
    with pytest.raises(ValueError):
        sharding.EngineBatchRunner(model, 12000, max_gap=50)
    model.engine.check_error()


def test_run_pipeline_and_the_command_line_with_a_gap(tmp_path, ckpt_weights, route_reads, monkeypatch):
    """``cli.run_pipeline(bridge_gap=g)`` over a small directory (int16 reads and one float trace) and the command line with
    ``CATFISH_BRIDGE_GAP=g``: the documents are ``chunks_of_read`` of the bridged spans; a bad value ends the command."""
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
    trace = infer.normalize_raw_signal(route_reads[1], "median")
    np.save(reads / "read_9.npy", trace)                       # a float trace: the runner's host route
    names = ["read_%d.npy" % i for i in range(4)] + ["read_9.npy"]
    model = neural_network.load_network("ResNetRNN", str(net), checkpoint=30000, device=0, max_windows_per_pass=32768)
    docs = {}
    for gap in (0, 4):
        spans = batching.infer_reads_dac(model, route_reads[:4], max_gap=gap)
        spans += batching.infer_reads(model, [infer.normalize_raw_signal(trace, "median")], max_gap=gap)
        want_hp, want_non = {}, {}
        for name, (sp, length) in zip(names, spans):
            merged, non = cli.chunks_of_read([list(v) for v in sp], length, 300)
            if merged is not None:
                want_hp[name] = merged
            want_non[name] = json.loads(json.dumps(non))
        with contextlib.redirect_stdout(io.StringIO()):
            res = cli.run_pipeline(str(reads), str(tmp_path / ("out%d" % gap)), chunk_size=300, network_path=str(net), device=0,
                                   bridge_gap=gap)
        assert res["reads"] == 5
        docs[gap] = (json.load(open(tmp_path / ("out%d" % gap) / "TEMP" / "hp_positions.json")),
                     json.load(open(tmp_path / ("out%d" % gap) / "TEMP" / "nonhp_positions.json")))
        assert docs[gap] == (want_hp, want_non)
    model.engine.close()
    assert docs[4] != docs[0]
    with contextlib.redirect_stdout(io.StringIO()):            # the default is gap 0
        cli.run_pipeline(str(reads), str(tmp_path / "plain"), chunk_size=300, network_path=str(net), device=0)
    assert json.load(open(tmp_path / "plain" / "TEMP" / "hp_positions.json")) == docs[0][0]
    monkeypatch.chdir(tmp_path)                                # the command line resolves "ResNetRNN" relative to the CWD
    monkeypatch.setenv("CATFISH_BRIDGE_GAP", "4")
    done = CliRunner().invoke(cli._build_click_main(), ["-i", str(reads), "-s", str(tmp_path / "cli"), "-c", "300"])
    assert done.exit_code == 0, done.output
    assert json.load(open(tmp_path / "cli" / "TEMP" / "hp_positions.json")) == docs[4][0]
    assert json.load(open(tmp_path / "cli" / "TEMP" / "nonhp_positions.json")) == docs[4][1]
    monkeypatch.setenv("CATFISH_BRIDGE_GAP", "four")
    bad = CliRunner().invoke(cli._build_click_main(), ["-i", str(reads), "-s", str(tmp_path / "bad"), "-c", "300"])
    assert bad.exit_code != 0 and "CATFISH_BRIDGE_GAP" in str(bad.exception) and not (tmp_path / "bad").exists()


def test_rounds_and_sweeps_on_a_validation_set(hp, tmp_path, monkeypatch):
    """``score_validation_device(bridge_gap=)``, ``validate``, ``threshold_sweep``, ``bridge_sweep`` and
    ``CATFISH_VALIDATION_BRIDGE`` over a small ``DeviceValidationSet``: the tables are the host definitions with ``max_gap`` on the
    round's own probabilities; without the option nothing changes."""
    import json
    from catfish_amd import train_validate as tv
    from catfish_amd.device_validation import DeviceValidationSet
    from catfish_amd.resnet_class import ResNetRNN
    (tmp_path / "val").mkdir()
    paths = []
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(3000 + 36 * i, seed=50 + i)
        paths.append(str(tmp_path / "val" / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    resident = DeviceValidationSet.from_npz(paths)
    selection = resident.select(35, 0, "complete", 856)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    plain = net.score_validation_device(resident, selection, (0.5,), run_edges=(35,), border_reach=16)
    bounds, _tails = dv.layout(selection[2], 35)
    total = int(bounds[-1])
    t = net.validation_buffers["tensors"]
    probs, y = t["probs"][:total].cpu().numpy(), t["y"][:total].cpu().numpy()
    middle = np.sort(probs)
    ths = tuple(float(middle[int(q * (total - 1))]) for q in (0.5, 0.8))      # scores this network really gives: gaps to bridge
    host = {g: (dv.run_states_host(probs, y, bounds, selection[2], ths, (35,), 15, max_gap=g),
                dv.run_borders_host(probs, y, bounds, selection[2], ths, 16, 15, max_gap=g)) for g in (0, 2, 8)}
    assert not np.array_equal(host[8][0], host[0][0]) and not np.array_equal(host[8][1], host[0][1])      # the gap shows in both tables
    for g in (0, 2, 8):
        got = net.score_validation_device(resident, selection, ths, run_edges=(35,), border_reach=16, bridge_gap=g)
        assert len(got) == 5 and np.array_equal(got[3], host[g][0]) and np.array_equal(got[4], host[g][1])
        assert np.array_equal(net.score_validation_device(resident, selection, ths, run_edges=(35,), bridge_gap=g)[3], host[g][0])
        assert np.array_equal(net.score_validation_device(resident, selection, ths, border_reach=16, bridge_gap=g)[3], host[g][1])
        rows = tv.threshold_sweep(net, resident, ths, 0, run_edges=(35,), border_reach=16, bridge_gap=g)
        for k, row in enumerate(rows):
            assert row["hp_states"] == host[g][0][k, 0].tolist() and row["called_states"] == host[g][0][k, 1].tolist()
            assert (row["hp_complete"], row["hp_found"], row["called_absent"]) == dv.run_state_rates(host[g][0][k])
            assert (row["hp_borders"], row["called_borders"]) == tv.border_report(host[g][1][k], 16)
    unbridged = tv.threshold_sweep(net, resident, ths, 0, run_edges=(35,), border_reach=16)
    assert unbridged == tv.threshold_sweep(net, resident, ths, 0, run_edges=(35,), border_reach=16, bridge_gap=0)
    assert [{k: r[k] for k in ("tp", "fp", "tn", "fn")} for r in rows] == [{k: r[k] for k in ("tp", "fp", "tn", "fn")} for r in unbridged]
    # bridge_sweep: per gap the rates of the run states and the share of judged runs with an interruption
    sweep = tv.bridge_sweep(net, resident, (0, 2, 8), 0, threshold=ths[0], run_edges=(35,), border_reach=16)
    assert [r["bridge_gap"] for r in sweep] == [0, 2, 8]
    for row in sweep:
        states, borders = host[row["bridge_gap"]][0][0], host[row["bridge_gap"]][1][0]
        assert sorted(row) == sorted(["bridge_gap", "hp_complete", "hp_found", "called_absent", "hp_states", "called_states",
                                      "hp_interrupted", "called_interrupted"])
        assert (row["hp_complete"], row["hp_found"], row["called_absent"]) == dv.run_state_rates(states)
        assert row["hp_states"] == states[0].tolist() and row["called_states"] == states[1].tolist()
        for kind, key in enumerate(("hp_interrupted", "called_interrupted")):
            judged = int(borders[kind, :33].sum())
            assert judged == int(states[kind, :, :2].sum()) and row[key] == (int(borders[kind, -1]) / judged if judged else 0)
    assert sweep[2]["hp_found"] >= sweep[0]["hp_found"]        # bridging only adds ones to the prediction
    # validate: the two tables of the round at 0.5, bridged; report and return value as without
    monkeypatch.chdir(tmp_path)
    base = tv.validate(net, resident, 0, str(tmp_path / "m0"), "complete", run_edges=(35,), border_reach=16)
    states0, borders0 = np.array(net.validation_run_states), np.array(net.validation_run_borders)
    assert tv.validate(net, resident, 0, str(tmp_path / "m4"), "complete", run_edges=(35,), border_reach=16, bridge_gap=4) == base
    assert (tmp_path / "m0.txt").read_text() == (tmp_path / "m4.txt").read_text()
    assert np.array_equal(net.validation_run_states, dv.run_states_host(probs, y, bounds, selection[2], (0.5,), (35,), 15, max_gap=4)[0])
    assert np.array_equal(net.validation_run_borders, dv.run_borders_host(probs, y, bounds, selection[2], (0.5,), 16, 15, max_gap=4)[0])
    assert np.array_equal(states0, plain[3][0]) and np.array_equal(borders0, plain[4][0])
    with pytest.raises(ValueError):
        tv.validate(net, resident, 0, str(tmp_path / "m"), "complete", bridge_gap=4)           # nothing it could change
    with pytest.raises(ValueError):
        net.score_validation_device(resident, selection, ths, run_edges=(35,), bridge_gap=50)
    net.engine.close()

    # CATFISH_VALIDATION_BRIDGE: every checkpoint round is validated with the gap, and its JSON lines say so
    (tmp_path / "train").mkdir()
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(12000, seed=70 + i)
        np.savez(tmp_path / "train" / ("t%d.npz" % i), raw=raw, base_labels=lab)
    real_build, real_validate, seen = tv.build_model, tv.validate, []

    def seeded(kind, **kw):                                    # main() draws its weights and its dropout from the clock: pin both
        network = real_build(kind, **dict(kw, train_seed=0))
        init = network.initialize_network
        network.initialize_network = lambda seed=None: init(seed=4)
        return network

    def watched(network, *args, **kw):
        seen.append(dict(kw))
        return real_validate(network, *args, **kw)

    monkeypatch.setattr(tv, "build_model", seeded)
    monkeypatch.setattr(tv, "validate", watched)
    monkeypatch.setenv("CATFISH_SHIPPED_HPARAMS", "1")
    monkeypatch.setenv("CATFISH_DEVICE_VALIDATION", "1")
    for name in ("CATFISH_DEVICE_DB", "CATFISH_NATIVE_TRAINING", "CATFISH_TRAINING_PRECISION", "CATFISH_VALIDATION_CURVE",
                 "CATFISH_VALIDATION_RUNS", "CATFISH_VALIDATION_BORDERS"):
        monkeypatch.delenv(name, raising=False)
    argv = ["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"]
    monkeypatch.setenv("CATFISH_VALIDATION_BRIDGE", "4")
    (tmp_path / "alone").mkdir()
    monkeypatch.chdir(tmp_path / "alone")
    with pytest.raises(ValueError, match="CATFISH_VALIDATION_BRIDGE"):        # neither run states nor borders asked for
        tv.main(argv)
    assert seen == []
    monkeypatch.setenv("CATFISH_VALIDATION_RUNS", "1")
    monkeypatch.setenv("CATFISH_VALIDATION_BORDERS", "8")
    (tmp_path / "both").mkdir()
    monkeypatch.chdir(tmp_path / "both")
    tv.main(argv)
    assert len(seen) == 1 and seen[0]["bridge_gap"] == 4 and seen[0]["border_reach"] == 8
    (model_dir,) = [d for d in (tmp_path / "both").iterdir() if d.is_dir()]
    for suffix in ("_hp_states.jsonl", "_hp_borders.jsonl"):
        with open(str(model_dir) + suffix) as fh:
            (line,) = fh.read().splitlines()
        assert json.loads(line)["bridge_gap"] == 4 and json.loads(line)["step"] == 20
