"""What a validation round launches: with everything asked for, and with nothing, ``RNN.score_validation_device`` must ask the C ABI
for exactly the calls recorded in tests/golden/validation_round_trace.json -- the same functions in the same order, the same scalar
arguments, the same pointers null or set.  The file was recorded with ``traces_now`` below at the commit it names, when ``walk`` was a
ladder of ``if``s; it now walks ``validation_round.OPTIONS``.  And every result of the all-on round is, bit for bit, that of a round
that asks for it alone."""
import json
import os

import numpy as np
import pytest

import call_chain_routes as routes
from catfish_amd import labelling
from catfish_amd.device_validation import DeviceValidationSet

pytestmark = pytest.mark.gpu

TRACE_FILE = os.path.join(routes.GOLDEN, "validation_round_trace.json")
OPTIONS = dict(run_edges=(35, 70), border_reach=8, curve_shift=10, max_bases=4, vote_bases=6, score_shift=14)
RESULTS_OF = dict(run_edges=("run_states",), border_reach=("run_borders",), curve_shift=("curve",), max_bases=("run_bases",),
                  vote_bases=("base_confusion", "base_vote_runs"), score_shift=("run_scores",))
RULE = dict(bridge_gap=3, phases=(0, 17), vote_weight="centre")
THRESHOLDS = tuple(np.linspace(0.05, 0.95, 20).tolist())           # two launch groups: 16 + 4


@pytest.fixture(scope="module")
def net(hp, ckpt_weights):
    from catfish_amd.resnet_class import ResNetRNN
    m = ResNetRNN(**hp)
    m.set_weights(ckpt_weights)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def resident():
    reads = [labelling.synthetic_event_read(n, seed, hp_fraction=0.3) for n, seed in ((300, 61), (520, 62), (700, 63))]
    batch = labelling.EventBatch.from_reads([(bases, lengths) for _raw, bases, lengths in reads])
    return DeviceValidationSet.from_events([raw for raw, _b, _l in reads], batch, 5)


def traces_now(net, resident):
    """({round: trace}, the all-on round's results): one round with everything asked for and one with nothing, in that order;
    ``engine._lib`` is the library again afterwards."""
    import torch
    selection = resident.select(net.window, 0, "complete", 856)
    engine = net.engine
    lib, traces, results = engine._lib, {}, {}
    try:
        for key, options in (("everything", dict(thresholds=THRESHOLDS, **OPTIONS, **RULE)), ("nothing", {})):
            trace = []
            engine._lib = routes.RecordingLib(lib, trace)
            results[key] = net.score_validation_device(resident, selection, **options)
            torch.cuda.synchronize()
            traces[key] = trace
    finally:
        engine._lib = lib
    engine.check_error()
    return json.loads(json.dumps(traces)), results["everything"]


def test_a_round_launches_what_was_recorded_and_every_result_is_its_own(net, resident):
    with open(TRACE_FILE) as fh:
        golden = json.load(fh)
    assert len(golden["recorded_at_commit"]) == 40
    lib = net.engine._lib
    got, everything = traces_now(net, resident)
    assert net.engine._lib is lib                                            # the proxy is gone again
    want = golden["traces"]
    assert list(got) == list(want) == ["everything", "nothing"]
    for key in want:
        assert [e[0] for e in got[key]] == [e[0] for e in want[key]], key
        for k, (a, b) in enumerate(zip(got[key], want[key])):
            assert a == b, (key, k)
    # the recording holds what it is there to guard: every step of a round, the per-threshold ones once per group, the curve last
    names = [e[0] for e in want["everything"]]
    per_group = ["cf_validation_score", "cf_validation_run_states_bridged", "cf_validation_run_borders_bridged", "cf_validation_run_bases",
                 "cf_base_votes", "cf_validation_run_scores"]
    at = names.index("cf_validation_score")
    assert names[at:] == per_group * 2 + ["cf_validation_curve", "cf_check_error"], names
    assert {"cf_validation_gather", "cf_retile_windows", "cf_vote_tilings"} <= set(names[:at])
    assert [e[0] for e in want["nothing"]] == ["cf_validation_gather", "cf_infer_logits", "cf_validation_score", "cf_check_error"]
    # every result alone: the same bits
    selection = resident.select(net.window, 0, "complete", 856)
    assert len(everything) == 10 and all(np.asarray(item).size for item in everything)
    for option, value in OPTIONS.items():
        alone = net.score_validation_device(resident, selection, THRESHOLDS, **{option: value}, **RULE)
        assert len(alone) == 3 + len(RESULTS_OF[option])
        for name in ("right", "ce_sum", "counts") + RESULTS_OF[option]:
            a, b = getattr(alone, name), getattr(everything, name)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (option, name)
    assert sum(int(getattr(everything, name).sum()) > 0 for names in RESULTS_OF.values() for name in names) == 7
    net.engine.check_error()
