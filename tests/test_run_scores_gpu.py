"""The score step on the card (csrc/validation_scores.hpp through the C ABI) against ``device_validation.run_scores_host``, bit for
bit: the golden stretches, the planted batch with seeded probabilities, sixteen thresholds in one call, a bridged prediction, a whole
round through a real model with every other result on, and the refusals (argument errors only, refused before any launch)."""
import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from test_run_scores_replay import planted_batch
from test_run_states_host import golden, packed

pytestmark = pytest.mark.gpu

SIXTEEN = (0.5, 0.3, 0.7, 0.1, float(np.float32(0.1)), 0.9, float(np.float32(0.9)), 0.0, 1.0, 0.5 + 1e-12, 0.5 - 1e-12,
           float(np.nextafter(np.float32(0.5), np.float32(1.0))), float(np.nextafter(np.float32(0.5), np.float32(0.0))), 0.25, 0.75, 0.6)


@pytest.fixture(scope="module")
def engine(ckpt_weights):
    from catfish_amd.engine import HipEngine
    eng = HipEngine(ckpt_weights)
    yield eng
    eng.close()


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


def on_card(batch):
    probs, y, bounds, lengths = batch
    return {"probs": _dev(probs), "y": _dev(y), "bounds": _dev(bounds), "length": _dev(lengths), "total": int(bounds[-1]),
            "longest": int(np.diff(bounds).max()), "host": batch}


@pytest.fixture(scope="module")
def planted(engine):
    piece = int(engine._lib.cf_validation_run_piece())
    assert piece >= 4096 and piece % 64 == 0
    batch = planted_batch(piece)
    _values, counts = np.unique(batch[0], return_counts=True)
    assert counts.max() >= 4096 and np.isnan(batch[0]).sum() == 1 and (batch[0] > 1).sum() == 1       # equal keys by the thousand
    return on_card(batch)


@pytest.fixture(scope="module")
def golden_case():
    scores, labels, offsets, _cases = golden()
    return on_card(packed([(scores[a:b], labels[a:b]) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]))


def scores_on_device(engine, case, thresholds, shift, min_run=15, max_gap=0, longest=None, buffers=None):
    import torch
    k = len(thresholds)
    if buffers is None:
        buffers = (torch.full((k * dv.score_cells(shift),), -1, dtype=torch.int64, device="cuda:0"),
                   torch.full((max(engine.run_scores_work_bytes(case["total"], k), 1),), 7, dtype=torch.uint8, device="cuda:0"))
    table, work = buffers
    engine.run_scores_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"],
                                 case["longest"] if longest is None else longest, thresholds, shift, table, work, min_run=min_run, max_gap=max_gap)
    torch.cuda.synchronize()
    engine.check_error()
    return table.cpu().numpy().reshape(k, 2, 3, -1)


@pytest.mark.parametrize("min_run", (15, 1))
@pytest.mark.parametrize("shift", (14, 16, 22))
def test_the_golden_batch(engine, golden_case, shift, min_run):
    want = dv.run_scores_host(*golden_case["host"], (0.3, 0.5, 0.9), shift, min_run)
    assert want[:2, :, :, :-1].sum(axis=-1).min() >= 20
    assert np.array_equal(scores_on_device(engine, golden_case, (0.3, 0.5, 0.9), shift, min_run), want)


@pytest.mark.parametrize("min_run", (15, 1))
def test_the_planted_batch_twice_into_one_buffer(engine, planted, min_run):
    import torch
    want = dv.run_scores_host(*planted["host"], (0.5,), 16, min_run)
    print("samples per (kind, state):", want[0, :, :, :-1].sum(axis=-1).tolist())
    assert want[0, :, :, :-1].sum(axis=-1).min() >= 20
    buffers = (torch.full((dv.score_cells(16),), -1, dtype=torch.int64, device="cuda:0"),
               torch.full((engine.run_scores_work_bytes(planted["total"], 1),), 7, dtype=torch.uint8, device="cuda:0"))
    first = scores_on_device(engine, planted, (0.5,), 16, min_run, buffers=buffers)
    assert np.array_equal(first, want)
    assert np.array_equal(scores_on_device(engine, planted, (0.5,), 16, min_run, longest=0, buffers=buffers), first)


def test_sixteen_thresholds_in_one_call(engine, planted):
    want = dv.run_scores_host(*planted["host"], SIXTEEN, 16)
    assert np.array_equal(scores_on_device(engine, planted, SIXTEEN, 16), want)


def test_a_bridged_prediction(engine, planted, golden_case):
    for case, thresholds in ((planted, (0.5,)), (golden_case, (0.3, 0.5, 0.9))):
        want = dv.run_scores_host(*case["host"], thresholds, 16, 15, 3)
        assert not np.array_equal(want, dv.run_scores_host(*case["host"], thresholds, 16, 15))             # bridging changes these runs
        assert np.array_equal(scores_on_device(engine, case, thresholds, 16, max_gap=3), want)


def test_single_and_empty_stretches(engine, planted):
    probs, y, bounds, lengths = planted["host"]
    r = int(np.argmax(lengths))
    a, n = int(bounds[r]), int(lengths[r])
    one = on_card((probs[a:a + n], y[a:a + n], np.int64([0, n]), np.int64([n])))
    assert np.array_equal(scores_on_device(engine, one, (0.5, 0.95), 22), dv.run_scores_host(*one["host"], (0.5, 0.95), 22))
    empty = {"probs": _dev(np.zeros(1, np.float32)), "y": _dev(np.zeros(1, np.uint8)), "bounds": _dev(np.int64([0, 0, 0])),
             "length": _dev(np.int64([0, 0])), "total": 0, "longest": 0}
    assert not scores_on_device(engine, empty, (0.5,), 16).any()


def test_a_whole_round_with_every_result_on(hp, tmp_path):
    """20 thresholds go in two groups; the other results are the bits of the same round without ``score_shift``; the sweep's rows
    carry the summary of their threshold."""
    from catfish_amd.resnet_class import ResNetRNN
    paths = []
    for i in range(3):
        raw, lab = tv.synthetic_labelled_read(3000 + 36 * i, seed=50 + i)
        paths.append(str(tmp_path / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    resident = DeviceValidationSet.from_npz(paths)
    selection = resident.select(35, 0, "complete", 856)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    net.score_validation_device(resident, selection, (0.5,))
    bounds, _tails = dv.layout(selection[2], 35)
    total = int(bounds[-1])
    middle = np.sort(net.validation_buffers["tensors"]["probs"][:total].cpu().numpy())
    thresholds = tuple(float(middle[int(q * (total - 1))]) for q in np.linspace(0.05, 0.95, 20))              # scores the model really gives
    options = dict(run_edges=(35, 70), border_reach=16, curve_shift=14)
    plain = net.score_validation_device(resident, selection, thresholds, **options)
    got = net.score_validation_device(resident, selection, thresholds, score_shift=16, **options)
    assert len(plain) == 6 and len(got) == 7 and got[6] is got.run_scores and plain.run_scores is None
    for a, b in zip(plain, got[:6]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    t = net.validation_buffers["tensors"]
    host = (t["probs"][:total].cpu().numpy(), t["y"][:total].cpu().numpy(), bounds, selection[2])
    want = dv.run_scores_host(*host, thresholds, 16)
    print("samples under true / called runs per threshold:", want[:, 0, :, :-1].sum(axis=(1, 2)).tolist(), want[:, 1, :, :-1].sum(axis=(1, 2)).tolist())
    assert got.run_scores.dtype == np.int64 and np.array_equal(got.run_scores, want)
    assert want[:, 1, :, :-1].sum() > 0                    # the thresholds are the model's own scores: something is called
    again = net.score_validation_device(resident, selection, thresholds, **options)
    assert len(again) == 6 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
    before = tv.threshold_sweep(net, resident, thresholds[8:10], 0)
    rows = tv.threshold_sweep(net, resident, thresholds[8:10], 0, score_shift=16)
    for k, (row, old) in enumerate(zip(rows, before)):
        assert {key: row[key] for key in old} == old and sorted(set(row) - set(old)) == ["called_scores", "hp_scores"]
        assert [row["hp_scores"], row["called_scores"]] == dv.run_score_summary(want[8 + k], 16)
    net.engine.close()


def test_refusals_arrive_as_value_errors(engine, planted):
    """Argument errors only, refused on the host before any launch; the messages name the size needed; the engine stays usable."""
    import torch
    total = planted["total"]

    def call(thresholds=(0.5,), shift=16, table=None, work=None, case=planted, **kw):
        k = max(len(thresholds), 1)
        table = torch.zeros(k * dv.score_cells(16), dtype=torch.int64, device="cuda:0") if table is None else table
        work = torch.zeros(engine.run_scores_work_bytes(case["total"], k), dtype=torch.uint8, device="cuda:0") if work is None else work
        engine.run_scores_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"], case["longest"], thresholds,
                                     shift, table, work, **kw)

    assert engine.run_scores_work_bytes(total, 3) == 2 * engine.run_states_work_bytes(total, 3) == 6 * ((total + 63) // 64 * 64)
    for bad in (dict(thresholds=()), dict(thresholds=SIXTEEN + (0.125,)), dict(shift=13), dict(shift=23), dict(shift=True), dict(shift=16.5),
                dict(min_run=0), dict(max_gap=-1), dict(max_gap=50, min_run=15)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError, match=str(dv.score_cells(16))):         # a table one cell short
        call(table=torch.zeros(dv.score_cells(16) - 1, dtype=torch.int64, device="cuda:0"))
    need = engine.run_scores_work_bytes(total, 1)
    with pytest.raises(ValueError, match=str(need)):                       # a work buffer one byte short
        call(work=torch.zeros(need - 1, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):                                        # n = 0
        call(case=dict(planted, bounds=planted["bounds"][:1], length=planted["length"][:0]))
    with pytest.raises(ValueError):                                        # probabilities of another type
        call(case=dict(planted, probs=planted["probs"].double()))
    with pytest.raises(ValueError):                                        # longest > total
        call(case=dict(planted, longest=total + 1))
    assert np.array_equal(scores_on_device(engine, planted, (0.9,), 22), dv.run_scores_host(*planted["host"], (0.9,), 22))
