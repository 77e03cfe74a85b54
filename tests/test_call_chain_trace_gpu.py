"""What is launched: every route from raw reads to homopolymer spans (tests/call_chain_routes.py), for every option set, must ask the C
ABI for exactly the calls recorded in tests/golden/call_chain_trace.json -- the same functions in the same order, the same scalar
arguments, the same pointers null or set (the labels buffer among them), the same assignment to streams.  The file was recorded
with tools/record_call_chain_trace.py at the commit it names, before the chain was gathered into ``catfish_amd/calling.py``."""
import json
import os

import numpy as np
import pytest

import call_chain_routes as routes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hp):
    from catfish_amd.resnet_class import ResNetRNN
    m = ResNetRNN(**hp)
    with np.load(os.path.join(routes.GOLDEN, "ckpnt-30000-inference.npz")) as z:
        m.set_weights({k: z[k] for k in z.files})
    yield m
    m.engine.close()


def test_every_route_launches_what_was_recorded(model, golden_read):
    with open(routes.TRACE_FILE) as fh:
        golden = json.load(fh)
    assert len(golden["recorded_at_commit"]) == 40
    lib = model.engine._lib
    got = json.loads(json.dumps(routes.record(model, golden_read["dac"])))
    assert model.engine._lib is lib                                          # the proxy is gone again
    want = golden["traces"]
    assert list(got) == list(want) and len(want) == 5 * len(routes.ROUTES) + len(routes.MIN_RUN_ROUTES)
    for key in want:
        assert len(got[key]) == len(want[key]), (key, [e[0] for e in got[key]], [e[0] for e in want[key]])
        for k, (a, b) in enumerate(zip(got[key], want[key])):
            assert a == b, (key, k)
    # the recording holds what it is there to guard: all five post-processing launches, both kinds of labels pointer, three streams
    calls = [e for t in want.values() for e in t]
    assert {"cf_postprocess", "cf_spans", "cf_postprocess_spans", "cf_postprocess_spans_bridged", "cf_span_scores", "cf_span_scores_labels",
            "cf_retile_windows", "cf_vote_tilings", "cf_normalize", "cf_infer", "cf_infer_host"} <= {e[0] for e in calls}
    assert {e[9] for e in calls if e[0] == "cf_postprocess_spans"} == {"null", "set"}
    assert {e[10] for e in calls if e[0] == "cf_postprocess_spans_bridged"} == {"null", "set"}
    assert max(e[-1]["stream"] for e in calls if isinstance(e[-1], dict)) >= 2
