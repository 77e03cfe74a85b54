"""What every route "raw read in, homopolymer spans out" asks of the C ABI, as data: a recording proxy around ``engine._lib`` and a
driver that takes each public route through each option set once.  Shared by tests/test_call_chain_trace_gpu.py (compares) and
tools/record_call_chain_trace.py (records tests/golden/call_chain_trace.json); only public functions are used, so the same file
drives any revision of the package."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRACE_FILE = os.path.join(GOLDEN, "call_chain_trace.json")

# (max_gap, phases, vote_weight, scores, min_run)
OPTION_SETS = ((0, (0,), "mean", False, 15), (0, (0,), "mean", True, 15), (3, (0,), "mean", False, 15), (3, (0, 17), "centre", True, 15),
               (0, (0, 12, 23), "mean", False, 15), (0, (0,), "mean", False, 70))
ROUTES = ("pipeline", "infer_reads_dac", "infer_reads", "infer_packed", "infer_class_from_raw", "runner")
MIN_RUN_ROUTES = ("pipeline", "infer_packed")            # the routes that run the min_run 70 set
# below one window, an exact multiple (a full extra window), one over, two windows, several windows
SYNTHETIC_LENGTHS = (34, 35, 36, 70, 211)
# the launch functions: their last argument is the stream
STREAMED = ("cf_infer", "cf_infer_logits", "cf_postprocess", "cf_spans", "cf_normalize", "cf_postprocess_spans", "cf_span_scores",
            "cf_postprocess_spans_bridged", "cf_span_scores_labels", "cf_retile_windows", "cf_vote_tilings", "cf_model_load_params")


def _is_pointer(argtype):
    return argtype in (C.c_void_p, C.c_char_p) or hasattr(argtype, "contents")


class RecordingLib(object):
    """Stands in for ``engine._lib``: forwards everything, and appends one entry per ``cf_*`` call to ``trace`` -- the name, every
    integer or float argument as it is, "null" or "set" for a pointer (the values of a small ctypes int array, such as the phases),
    and ``{"stream": k}`` for the stream, k counting the streams in the order in which the trace first meets them."""

    def __init__(self, lib, trace):
        from catfish_amd import _native as N
        self._lib, self._symbols, self.trace, self._streams = lib, N.SYMBOLS, trace, {}

    def _pointer(self, a):
        if isinstance(a, C.Array) and isinstance(a[0] if len(a) else 0, int):
            return [int(v) for v in a]
        if a is None or (isinstance(a, C.c_void_p) and not a.value) or (isinstance(a, int) and a == 0):
            return "null"
        return "set"

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cf_"):
            return fn
        argtypes = self._symbols[name][1]

        def call(*args):
            entry = [name]
            for i, (a, kind) in enumerate(zip(args, argtypes)):
                if name in STREAMED and i == len(argtypes) - 1:
                    value = (a.value if isinstance(a, C.c_void_p) else a) or 0
                    entry.append({"stream": self._streams.setdefault(value, len(self._streams))})
                elif _is_pointer(kind):
                    entry.append(self._pointer(a))
                else:
                    entry.append(float(a) if isinstance(a, float) else int(a))
            self.trace.append(entry)
            return fn(*args)
        return call


def reads_of(golden_dac):
    """The int16 reads every route gets: five synthetic ones with fixed seeds and the golden read (so that some runs exist)."""
    from oracle import catfish_oracle as oracle
    return [oracle.synthetic_dac(1, n, seed=900 + i)[0] for i, n in enumerate(SYNTHETIC_LENGTHS)] + [
        np.ascontiguousarray(golden_dac, dtype=np.int16)]


def drive(route, model, dacs, option_set):
    """One route, once, with one option set; options the route does not take are left out."""
    from catfish_amd import batching, infer, sharding
    from catfish_amd.pipeline import ReadPipeline
    max_gap, phases, weight, scores, min_run = option_set
    kw = dict(max_gap=max_gap, phases=phases, vote_weight=weight)
    sigs = [infer.normalize_raw_signal(d, "median") for d in dacs]
    if route == "pipeline":
        pipe = ReadPipeline(model.engine, 12000, min_run=min_run, scores=scores, **kw)
        return pipe.collect(pipe.submit(dacs))
    if route == "infer_reads_dac":
        return batching.infer_reads_dac(model, dacs, min_run=min_run, **kw)
    if route == "infer_reads":
        return batching.infer_reads(model, sigs, min_run=min_run, **kw)
    if route == "infer_packed":
        return batching.infer_packed(model.engine, batching.pack_reads(sigs), min_run=min_run, return_probs=True, **kw)
    if route == "infer_class_from_raw":
        return [infer.infer_class_from_raw(s, model, scores=scores, **kw) for s in sigs]
    if route == "runner":
        runner = sharding.EngineBatchRunner(model, 12000, min_run=min_run, **kw)
        return list(runner.run([dacs, [np.asarray(d, dtype=np.float64) for d in dacs]]))       # one int16 batch, one float batch
    raise ValueError(route)


def key_of(route, option_set):
    max_gap, phases, weight, scores, min_run = option_set
    return "%s gap=%d phases=%s weight=%s scores=%d min_run=%d" % (route, max_gap, ",".join(str(p) for p in phases), weight, scores, min_run)


def record(model, golden_dac):
    """{key: trace} for every route and option set, in a fixed order; ``engine._lib`` is the library again afterwards."""
    import torch
    dacs = reads_of(golden_dac)
    engine = model.engine
    lib, traces = engine._lib, {}
    try:
        for route in ROUTES:
            for option_set in OPTION_SETS:
                if option_set[4] != 15 and route not in MIN_RUN_ROUTES:
                    continue
                trace = []
                engine._lib = RecordingLib(lib, trace)
                drive(route, model, dacs, option_set)
                torch.cuda.synchronize()
                traces[key_of(route, option_set)] = trace
    finally:
        engine._lib = lib
    engine.check_error()
    return traces
