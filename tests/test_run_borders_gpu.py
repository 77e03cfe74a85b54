"""The border step on the card (csrc/validation_borders.hpp through the C ABI) against ``device_validation.run_borders_host``: the
golden stretches and a planted batch straight into the kernel, a whole round through real models, the sweep and the per-round JSON
line, and the host-side refusals."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from test_run_borders_host import table_of
from test_run_borders_replay import GOLDEN, PIECE, golden_batch, pack_stretches, planted_border_stretches
from test_run_states_gpu import THRESHOLDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(ckpt_weights):
    from catfish_amd.engine import HipEngine
    eng = HipEngine(ckpt_weights)
    yield eng
    eng.close()


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


def on_device(host):
    probs, y, bounds, lengths = host
    return {"probs": _dev(probs if probs.size else np.zeros(1, np.float32)), "y": _dev(y if y.size else np.zeros(1, np.uint8)),
            "bounds": _dev(bounds), "length": _dev(lengths), "total": int(bounds[-1]),
            "longest": int(np.diff(bounds).max()) if len(lengths) else 0, "host": host}


def run_borders_on_device(engine, case, thresholds, reach, min_run=15, longest=None):
    import torch
    k, cells = len(thresholds), 5 * reach + 3
    counts = torch.full((k * 2 * cells,), -1, dtype=torch.int64, device="cuda:0")
    work = torch.full((max(engine.run_borders_work_bytes(case["total"], k), 1),), 7, dtype=torch.uint8, device="cuda:0")
    engine.run_borders_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"],
                                  case["longest"] if longest is None else longest, thresholds, reach, counts, work, min_run=min_run)
    torch.cuda.synchronize()
    engine.check_error()
    return counts.cpu().numpy().reshape(k, 2, cells)


@pytest.fixture(scope="module")
def planted(engine):
    """The planted batch, packed as a round packs it, and its reference (computed once: 16 thresholds, reach 64)."""
    piece = int(engine._lib.cf_validation_run_piece())
    assert piece == PIECE                                  # (the replay test plants around the same piece borders)
    case = on_device(pack_stretches(planted_border_stretches(piece)))
    case["want"] = dv.run_borders_host(*case["host"], THRESHOLDS, 64)
    return case


def test_the_golden_batch(engine):
    """All 51 golden stretches as a round packs them, three thresholds in one call: the table the reference's own check_hp gives."""
    case = on_device(golden_batch())
    with np.load(os.path.join(GOLDEN, "run_states_golden.npz")) as z:
        scores, labels, offsets = z["scores"], z["labels"], z["offsets"]
    with open(os.path.join(GOLDEN, "run_borders_golden.json")) as fh:
        records = json.load(fh)["cases"]
    for reach in (1, 64, 128):
        want = np.zeros((3, 2, 5 * reach + 3), dtype=np.int64)
        for k, t in enumerate((0.3, 0.5, 0.9)):
            have = {c["stretch"]: c["runs"] for c in records if c["threshold"] == t}
            for stretch in range(len(offsets) - 1):
                a, b = int(offsets[stretch]), int(offsets[stretch + 1])
                if stretch in have:
                    want[k] += table_of(have[stretch], reach)
                else:                                      # the hand-made stretches have records at 0.5 only
                    want[k] += dv.run_borders_host(scores[a:b], labels[a:b], [0, b - a], [b - a], (t,), reach)[0]
        assert len([c for c in records if c["threshold"] == 0.5]) == len(offsets) - 1 == 51
        assert np.array_equal(want, dv.run_borders_host(*case["host"], (0.3, 0.5, 0.9), reach))
        first = run_borders_on_device(engine, case, (0.3, 0.5, 0.9), reach)
        print("reach", reach, "judged per (threshold, kind):", first[:, :, :2 * reach + 1].sum(axis=-1).tolist())
        assert np.array_equal(first, want)
        assert np.array_equal(run_borders_on_device(engine, case, (0.3, 0.5, 0.9), reach), first)
        assert np.array_equal(run_borders_on_device(engine, case, (0.3, 0.5, 0.9), reach, longest=0), first)


@pytest.mark.parametrize("k", (1, 16))
def test_planted_borders_equal_the_host_statement(engine, planted, k):
    want = planted["want"][:k]
    part = dv.split_run_borders(want[0], 64)
    assert part["interrupted"].min() >= 5 and part["left"][:, 0].min() >= 1 and part["right"][:, 128].min() >= 1
    first = run_borders_on_device(engine, planted, THRESHOLDS[:k], 64)
    print("judged / interrupted per kind at 0.5:", first[0, :, :129].sum(axis=-1).tolist(), first[0, :, -1].tolist())
    assert np.array_equal(first, want)
    assert np.array_equal(run_borders_on_device(engine, planted, THRESHOLDS[:k], 64, longest=0), first)
    if k == 16:                                            # one call of sixteen = sixteen calls of one
        alone = [run_borders_on_device(engine, planted, (t,), 64)[0] for t in THRESHOLDS]
        assert np.array_equal(np.stack(alone), first)


def test_other_reaches_and_min_run(engine, planted):
    """Reach 1 and 128 on the planted batch; min_run 1 and 64 on the bit-mask kernel, 65 on the per-sample one."""
    for reach in (1, 128):
        assert np.array_equal(run_borders_on_device(engine, planted, (0.5,), reach), dv.run_borders_host(*planted["host"], (0.5,), reach))
    for min_run in (1, 64, 65):
        want = dv.run_borders_host(*planted["host"], (0.5,), 64, min_run)
        assert np.array_equal(run_borders_on_device(engine, planted, (0.5,), 64, min_run=min_run), want), min_run


def test_no_leak_between_stretches(engine):
    """Two stretches of 70 and 105 samples (multiples of the window: no tail between them); the first ends and the second begins
    with ones in both arrays: the offsets at the shared border are 0, not the neighbour's run length."""
    called, truth = np.zeros(175, np.uint8), np.zeros(175, np.uint8)
    called[40:70] = truth[50:70] = 1
    called[70:100] = truth[70:95] = 1
    two = pack_stretches([(called[:70], truth[:70]), (called[70:], truth[70:])])
    assert two[2].tolist() == [0, 70, 175]
    got = run_borders_on_device(engine, on_device(two), (0.5,), 64)
    assert np.array_equal(got, dv.run_borders_host(*two, (0.5,), 64))
    part = dv.split_run_borders(got[0], 64)
    # kind 0: true [50, 69] against called [40, 69] -> (l, r) = (-10, 0); true [0, 24] against called [0, 29] -> (0, 5)
    assert np.flatnonzero(part["left"][0]).tolist() == [54, 64] and np.flatnonzero(part["right"][0]).tolist() == [64, 69]
    # kind 1: called [40, 69] against the truth -> (10, 0); called [0, 29] -> (0, -5)
    assert np.flatnonzero(part["left"][1]).tolist() == [64, 74] and np.flatnonzero(part["right"][1]).tolist() == [59, 64]
    for stretch in ((called[:70], truth[:70]), (called[70:], truth[70:])):               # ... and as batches of one stretch
        one = pack_stretches([stretch])
        assert np.array_equal(run_borders_on_device(engine, on_device(one), (0.5,), 64), dv.run_borders_host(*one, (0.5,), 64))
    probs, y, bounds, lengths = two                        # a label other than 1 counts as 0 in the kernel (the Python layers refuse it)
    odd, zeroed = y.copy(), y.copy()
    odd[60], zeroed[60] = 2, 0
    assert np.array_equal(run_borders_on_device(engine, on_device((probs, odd, bounds, lengths)), (0.5,), 64),
                          dv.run_borders_host(probs, zeroed, bounds, lengths, (0.5,), 64))
    empty = (np.zeros(0, np.float32), np.zeros(0, np.uint8), np.int64([0, 0, 0]), np.int64([0, 0]))
    assert not run_borders_on_device(engine, on_device(empty), (0.5,), 64).any()


def _validation_reads(tmp_path, count=3):
    val_dir = tmp_path / "val"
    val_dir.mkdir()
    paths = []
    for i in range(count):
        raw, lab = tv.synthetic_labelled_read(3000 + 36 * i, seed=50 + i)
        paths.append(str(val_dir / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    return paths


def test_a_whole_round_through_a_real_model(hp, tmp_path):
    """The borders are run_borders_host of the round's own probabilities, between the run states and the histogram, which stay what
    the call without border_reach returns; 20 thresholds go in two groups; without border_reach nothing changes."""
    from catfish_amd.resnet_class import ResNetRNN
    paths = _validation_reads(tmp_path)
    resident = DeviceValidationSet.from_npz(paths)
    selection = resident.select(35, 0, "complete", 856)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    plain = net.score_validation_device(resident, selection, (0.3, 0.5))
    assert len(plain) == 3 and "border_cells" not in net.validation_buffers["capacity"]
    old = net.score_validation_device(resident, selection, (0.3, 0.5), run_edges=(35,), curve_shift=14)
    assert len(old) == 5 and "border_cells" not in net.validation_buffers["capacity"]
    got = net.score_validation_device(resident, selection, (0.3, 0.5), run_edges=(35,), border_reach=32, curve_shift=14)
    assert len(got) == 6 and net.validation_buffers["capacity"]["border_cells"] == 2 * 2 * 163
    for a, b in zip(old, got[:4] + got[5:]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    bounds, _tails = dv.layout(selection[2], 35)
    total = int(bounds[-1])
    t = net.validation_buffers["tensors"]
    probs, y = t["probs"][:total].cpu().numpy(), t["y"][:total].cpu().numpy()
    want = dv.run_borders_host(probs, y, bounds, selection[2], (0.3, 0.5), 32)
    print("judged per (threshold, kind):", want[:, :, :65].sum(axis=-1).tolist())
    assert got[4].dtype == np.int64 and got[4].shape == (2, 2, 163) and np.array_equal(got[4], want)
    alone = net.score_validation_device(resident, selection, (0.3, 0.5), border_reach=32)
    assert len(alone) == 4 and np.array_equal(alone[3], want)
    middle = np.sort(probs)
    twenty = tuple(float(middle[int(q * (total - 1))]) for q in np.linspace(0.05, 0.95, 20))            # scores the model really gives
    many = net.score_validation_device(resident, selection, twenty, border_reach=32)[3]
    assert many.shape == (20, 2, 163) and many[:, 1, :65].sum() > 0
    groups = [net.score_validation_device(resident, selection, twenty[a:b], border_reach=32)[3] for a, b in ((0, 16), (16, 20))]
    assert np.array_equal(many, np.concatenate(groups)) and np.array_equal(many, dv.run_borders_host(probs, y, bounds, selection[2], twenty, 32))
    again = net.score_validation_device(resident, selection, (0.3, 0.5))
    assert len(again) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
    two = DeviceValidationSet.from_arrays([resident.signal[:3000]], [np.where(np.arange(3000) == 7, 2, resident.labels[:3000])])
    with pytest.raises(ValueError):                        # a set that holds a label 2
        net.score_validation_device(two, two.select(35, 0, "complete", 856), (0.5,), border_reach=32)
    assert len(net.score_validation_device(two, two.select(35, 0, "complete", 856), (0.5,), run_edges=())) == 4
    for reach in (0, 129, True, 2.5):
        with pytest.raises(ValueError):
            net.score_validation_device(resident, selection, (0.5,), border_reach=reach)
    with pytest.raises(ValueError):                        # no DeviceValidationSet: nothing to compare on the card
        tv.validate(net, paths, 0, str(tmp_path / "m"), "complete", border_reach=32)
    net.engine.close()


SUMMARY_KEYS = ["clipped", "exact_left", "exact_right", "gaps", "interrupted", "judged", "median_left", "median_right"]
REPORT_KEYS = sorted(SUMMARY_KEYS + ["left", "right", "gaps_by_length", "interrupted_runs"])


def test_sweep_rows_and_the_report_line(hp, tmp_path, monkeypatch):
    """threshold_sweep rows carry the two border reports; CATFISH_VALIDATION_BORDERS appends one JSON line per checkpoint round and
    leaves both .txt reports as they are without it."""
    from catfish_amd.resnet_class import ResNetRNN
    paths = _validation_reads(tmp_path, 2)
    resident = DeviceValidationSet.from_npz(paths)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    before = tv.threshold_sweep(net, resident, [0.4, 0.5], 0, run_edges=(35,))
    rows = tv.threshold_sweep(net, resident, [0.4, 0.5], 0, run_edges=(35,), border_reach=16)
    selection = resident.select(35, 0, "complete", 856)
    table = net.score_validation_device(resident, selection, (0.4, 0.5), border_reach=16)[3]
    for k, (row, old) in enumerate(zip(rows, before)):
        assert {key: row[key] for key in old} == old and sorted(set(row) - set(old)) == ["called_borders", "hp_borders"]
        for kind, key in enumerate(("hp_borders", "called_borders")):
            report, part = row[key], dv.split_run_borders(table[k, kind], 16)
            assert sorted(report) == REPORT_KEYS
            assert {name: report[name] for name in SUMMARY_KEYS} == dv.run_border_summary(table[k], 16)[kind]
            assert report["left"] == part["left"].tolist() and report["right"] == part["right"].tolist()
            assert report["gaps_by_length"] == part["gaps"].tolist() and report["interrupted_runs"] == int(part["interrupted"])
        assert row["hp_borders"]["judged"] == sum(row["hp_states"][b][s] for b in range(2) for s in range(2)) > 0
    assert sorted(tv.threshold_sweep(net, resident, [0.5], 0, border_reach=16)[0]) == sorted(
        ["threshold", "tp", "fp", "tn", "fn", "precision", "recall", "f1", "hp_borders", "called_borders"])
    net.engine.close()

    (tmp_path / "train").mkdir()
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(12000, seed=70 + i)
        np.savez(tmp_path / "train" / ("t%d.npz" % i), raw=raw, base_labels=lab)
    real_build = tv.build_model

    def seeded(kind, **kw):                                # main() draws its weights and its dropout from the clock: pin both
        network = real_build(kind, **dict(kw, train_seed=0))
        init = network.initialize_network
        network.initialize_network = lambda seed=None: init(seed=4)
        return network

    monkeypatch.setattr(tv, "build_model", seeded)
    monkeypatch.setenv("CATFISH_SHIPPED_HPARAMS", "1")
    monkeypatch.setenv("CATFISH_DEVICE_VALIDATION", "1")
    for name in ("CATFISH_DEVICE_DB", "CATFISH_NATIVE_TRAINING", "CATFISH_TRAINING_PRECISION", "CATFISH_VALIDATION_RUNS", "CATFISH_VALIDATION_CURVE"):
        monkeypatch.delenv(name, raising=False)
    reports = {}
    for switch, reach in (("0", None), ("1", 64), ("3", 3)):
        (tmp_path / switch).mkdir()
        monkeypatch.chdir(tmp_path / switch)
        monkeypatch.setenv("CATFISH_VALIDATION_BORDERS", switch)
        tv.main(["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"])
        (model_dir,) = [d for d in (tmp_path / switch).iterdir() if d.is_dir()]
        with open(str(model_dir) + ".txt") as fh:
            model_report = fh.read()
        with open(model_dir.name + ".txt") as fh:
            reports[switch] = (model_report, fh.read())
        lines_at = str(model_dir) + "_hp_borders.jsonl"
        assert not os.path.exists(str(model_dir) + "_hp_states.jsonl") and not os.path.exists(str(model_dir) + "_curves.jsonl")
        if reach is None:
            assert not os.path.exists(lines_at)
            continue
        with open(lines_at) as fh:
            (line,) = fh.read().splitlines()
        assert "None" not in line and "NaN" not in line
        record = json.loads(line)
        assert sorted(record) == ["called_borders", "hp_borders", "reach", "step", "threshold"]
        assert record["step"] == 20 and record["threshold"] == 0.5 and record["reach"] == reach
        for key in ("hp_borders", "called_borders"):
            report = record[key]
            assert sorted(report) == REPORT_KEYS and len(report["left"]) == len(report["right"]) == 2 * reach + 1
            assert len(report["gaps_by_length"]) == reach and sum(report["left"]) == sum(report["right"]) == report["judged"]
            assert report["median_left"] is None or isinstance(report["median_left"], int)
        assert record["hp_borders"]["judged"] > 0
    assert "Saved checkpoint at step 20" in reports["0"][0] and "---NEXT ROUND OF VALIDATION---" in reports["0"][1]
    assert reports["0"] == reports["1"] == reports["3"]


def test_refusals_arrive_as_value_errors(engine, planted):
    """Argument errors only, refused on the host before any launch; the engine stays usable."""
    import torch
    ok = dict(thresholds=(0.5,), reach=64, min_run=15)

    def call(case=planted, work=None, counts=None, **kw):
        args = dict(ok, **kw)
        k = max(len(args["thresholds"]), 1)
        reach = args["reach"] if type(args["reach"]) is int and 1 <= args["reach"] <= 128 else 128
        counts = torch.zeros(k * 2 * (5 * reach + 3), dtype=torch.int64, device="cuda:0") if counts is None else counts
        work = torch.zeros(max(engine.run_borders_work_bytes(case["total"], k), 1), dtype=torch.uint8, device="cuda:0") if work is None else work
        engine.run_borders_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"], case["longest"],
                                      args["thresholds"], args["reach"], counts, work, min_run=args["min_run"])

    for bad in (dict(thresholds=()), dict(thresholds=THRESHOLDS + (0.125,)), dict(reach=0), dict(reach=129), dict(reach=True), dict(reach=2.5),
                dict(min_run=0), dict(min_run=-1)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):                        # a work buffer one byte short
        call(work=torch.zeros(engine.run_borders_work_bytes(planted["total"], 1) - 1, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):                        # n = 0
        call(case=dict(planted, bounds=planted["bounds"][:1], length=planted["length"][:0]))
    with pytest.raises(ValueError):                        # too small a table
        call(counts=torch.zeros(2 * 323 - 1, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError):                        # probabilities of another type
        call(case=dict(planted, probs=planted["probs"].double()))
    with pytest.raises(ValueError):                        # fewer labels than samples
        call(case=dict(planted, y=planted["y"][:-1]))
    with pytest.raises(ValueError):                        # longest > total
        call(case=dict(planted, longest=planted["total"] + 1))
    import ctypes as C
    from catfish_amd import _native as N
    lib = engine._lib                                       # null pointers and a bad reach, straight at the C entry
    one = (C.c_double * 1)(0.5)
    buf = torch.zeros(2048, dtype=torch.int64, device="cuda:0")
    good = [None, C.c_void_p(planted["probs"].data_ptr()), C.c_void_p(planted["y"].data_ptr()), C.c_void_p(planted["bounds"].data_ptr()),
            C.c_void_p(planted["length"].data_ptr()), 1, 64, 64, one, 1, 64, 15, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), 2048, None]
    for position in (1, 2, 3, 4, 8, 12, 13):
        args = list(good)
        args[position] = None
        with pytest.raises(ValueError):
            N.check(lib.cf_validation_run_borders(*args))
    for position, value in ((10, 0), (10, 129), (11, 0), (9, 17), (14, 63)):
        args = list(good)
        args[position] = value
        with pytest.raises(ValueError):
            N.check(lib.cf_validation_run_borders(*args))
    assert lib.cf_validation_run_borders_work_bytes(100, 3) == lib.cf_validation_run_work_bytes(100, 3) == 3 * 128
    assert np.array_equal(run_borders_on_device(engine, planted, (0.5,), 64), planted["want"][:1])
