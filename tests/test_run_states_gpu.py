"""The run-state step on the card (csrc/validation_runs.hpp through the C ABI) against ``device_validation.run_states_host``:
planted probabilities straight into the kernel, a whole round through real models, the sweep and the per-round JSON line, and the
host-side refusals."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet
from test_run_states_replay import planted_stretches

pytestmark = pytest.mark.gpu

SEVEN = (1, 2, 15, 16, 64, 4096, 16385)
LEVELS = np.float32([0.1, 0.9, 0.5])                       # planted probabilities: not called / called / exactly 0.5
THRESHOLDS = (0.5, 0.3, 0.7, 0.1, float(np.float32(0.1)), 0.9, float(np.float32(0.9)), 0.0, 1.0, 0.5 + 1e-12, 0.5 - 1e-12,
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


@pytest.fixture(scope="module")
def planted(engine):
    """The planted batch, packed as a round packs it, and its reference (computed once: 16 thresholds, seven edges)."""
    piece = int(engine._lib.cf_validation_run_piece())
    assert piece >= 4096 and piece % 64 == 0
    stretches = planted_stretches(piece)
    lengths = np.array([len(c) for c, _ in stretches], dtype=np.int64)
    bounds, _tails = dv.layout(lengths, 35)
    probs = np.full(int(bounds[-1]), 0.9, dtype=np.float32)                                # a tail taken for a sample would show
    y = np.zeros(int(bounds[-1]), dtype=np.uint8)
    for b, (called, truth) in zip(bounds[:-1].tolist(), stretches):
        probs[b:b + len(called)] = LEVELS[called]
        y[b:b + len(truth)] = truth
    want = dv.run_states_host(probs, y, bounds, lengths, THRESHOLDS, SEVEN)
    assert want[0].sum(axis=1).min() >= 3                  # every (kind, state) pair at threshold 0.5
    return {"probs": _dev(probs), "y": _dev(y), "bounds": _dev(bounds), "length": _dev(lengths), "total": int(bounds[-1]),
            "longest": int(np.diff(bounds).max()), "want": want, "host": (probs, y, bounds, lengths)}


def run_states_on_device(engine, case, thresholds, edges, min_run=15, longest=None):
    import torch
    k = len(thresholds)
    counts = torch.full((k * 2 * (len(edges) + 1) * 3,), -1, dtype=torch.int64, device="cuda:0")
    work = torch.full((max(engine.run_states_work_bytes(case["total"], k), 1),), 7, dtype=torch.uint8, device="cuda:0")
    engine.run_states_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"],
                                 case["longest"] if longest is None else longest, thresholds, edges, counts, work, min_run=min_run)
    torch.cuda.synchronize()
    engine.check_error()
    return counts.cpu().numpy().reshape(k, 2, len(edges) + 1, 3)


@pytest.mark.parametrize("k", (1, 16))
@pytest.mark.parametrize("edges", ((), SEVEN), ids=("unbinned", "seven-edges"))
def test_planted_runs_equal_the_host_statement(engine, planted, k, edges):
    """(a) bit-equal to run_states_host, twice, whatever the grid hint."""
    want = planted["want"][:k]
    if not edges:
        want = want.sum(axis=2, keepdims=True)             # (tests/test_run_states_host.py: the bins sum to the unbinned table)
    first = run_states_on_device(engine, planted, THRESHOLDS[:k], edges)
    print("runs per (kind, state) at 0.5:", first[0].sum(axis=1).tolist())
    assert np.array_equal(first, want)
    assert np.array_equal(run_states_on_device(engine, planted, THRESHOLDS[:k], edges, longest=0), first)


def test_min_run_and_single_stretches(engine, planted):
    """Other min_run values (1, 16, 64 on the bit-mask kernel, 65 on the per-sample one) and a batch of ONE stretch."""
    probs, y, bounds, lengths = planted["host"]
    for min_run in (1, 16, 64, 65):
        want = dv.run_states_host(probs, y, bounds, lengths, (0.5,), (15, 64), min_run)
        assert np.array_equal(run_states_on_device(engine, planted, (0.5,), (15, 64), min_run=min_run), want)
    r = int(np.argmax(lengths))
    a, n = int(bounds[r]), int(lengths[r])
    one = {"probs": _dev(probs[a:a + n]), "y": _dev(y[a:a + n]), "bounds": _dev(np.int64([0, n])), "length": _dev(np.int64([n])),
           "total": n, "longest": n}
    want = dv.run_states_host(probs[a:a + n], y[a:a + n], [0, n], [n], (0.5, 0.95), (35,))
    assert np.array_equal(run_states_on_device(engine, one, (0.5, 0.95), (35,)), want)
    empty = {"probs": _dev(np.zeros(1, np.float32)), "y": _dev(np.zeros(1, np.uint8)), "bounds": _dev(np.int64([0, 0, 0])),
             "length": _dev(np.int64([0, 0])), "total": 0, "longest": 0}
    assert not run_states_on_device(engine, empty, (0.5,), (35,)).any()


def _validation_reads(tmp_path, count=3):
    val_dir = tmp_path / "val"
    val_dir.mkdir()
    paths = []
    for i in range(count):
        raw, lab = tv.synthetic_labelled_read(3000 + 36 * i, seed=50 + i)
        paths.append(str(val_dir / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    return paths


def test_a_whole_round_through_real_models(hp, tmp_path):
    """(b) the fourth result of score_validation_device is run_states_host of the round's own probabilities; the first three are
    the bits of the call without run_edges; 18 thresholds go in two groups."""
    from catfish_amd.resnet_class import ResNetRNN
    resident = DeviceValidationSet.from_npz(_validation_reads(tmp_path))
    selection = resident.select(35, 0, "complete", 856)
    for sizes in (dict(), dict(layer_size=128, layer_size_res=64)):
        net = ResNetRNN(**dict(hp, **sizes))
        net.initialize_network(seed=5)
        plain = net.score_validation_device(resident, selection, (0.5,))
        bounds, _tails = dv.layout(selection[2], 35)
        total = int(bounds[-1])
        middle = np.sort(net.validation_buffers["tensors"]["probs"][:total].cpu().numpy())
        thresholds = tuple(float(middle[int(q * (total - 1))]) for q in np.linspace(0.05, 0.95, 18))          # scores the model really gives
        plain = net.score_validation_device(resident, selection, thresholds)
        assert len(plain) == 3
        for edges in ((), (35, 70, 140)):
            got = net.score_validation_device(resident, selection, thresholds, run_edges=edges)
            assert len(got) == 4
            for a, b in zip(plain, got[:3]):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
            t = net.validation_buffers["tensors"]
            want = dv.run_states_host(t["probs"][:total].cpu().numpy(), t["y"][:total].cpu().numpy(), bounds, selection[2], thresholds, edges)
            print("true / called runs per threshold:", want[:, 0].sum(axis=(1, 2)).tolist(), want[:, 1].sum(axis=(1, 2)).tolist())
            assert got[3].dtype == np.int64 and np.array_equal(got[3], want)
            assert want[:, 1].sum() > 0                    # the thresholds are the model's own scores: something is called
        again = net.score_validation_device(resident, selection, thresholds)                    # and back: three results, the same bits
        assert len(again) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
        net.engine.close()


def test_sweep_rows_and_the_report_line(hp, tmp_path, monkeypatch):
    """(c) threshold_sweep rows carry the tables and the rates; CATFISH_VALIDATION_RUNS=1 appends one JSON line per checkpoint round
    and leaves both .txt reports as they are without it."""
    from catfish_amd.resnet_class import ResNetRNN
    paths = _validation_reads(tmp_path, 2)
    resident = DeviceValidationSet.from_npz(paths)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    before = tv.threshold_sweep(net, resident, [0.4, 0.5], 0)
    rows = tv.threshold_sweep(net, resident, [0.4, 0.5], 0, run_edges=(35, 70, 140))
    selection = resident.select(35, 0, "complete", 856)
    table = net.score_validation_device(resident, selection, (0.4, 0.5), run_edges=(35, 70, 140))[3]
    for k, (row, old) in enumerate(zip(rows, before)):
        assert {key: row[key] for key in old} == old
        assert sorted(set(row) - set(old)) == ["called_absent", "called_states", "hp_complete", "hp_found", "hp_states"]
        assert row["hp_states"] == table[k, 0].tolist() and row["called_states"] == table[k, 1].tolist()
        true_runs, called = table[k, 0].sum(axis=0), table[k, 1].sum(axis=0)
        assert true_runs.sum() > 0
        assert row["hp_complete"] == true_runs[0] / true_runs.sum() and row["hp_found"] == (true_runs[0] + true_runs[1]) / true_runs.sum()
        assert row["called_absent"] == (called[2] / called.sum() if called.sum() else 0)
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
    for name in ("CATFISH_DEVICE_DB", "CATFISH_NATIVE_TRAINING", "CATFISH_TRAINING_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    reports = {}
    for switch in ("0", "1"):
        (tmp_path / switch).mkdir()
        monkeypatch.chdir(tmp_path / switch)
        monkeypatch.setenv("CATFISH_VALIDATION_RUNS", switch)
        tv.main(["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"])
        (model_dir,) = [d for d in (tmp_path / switch).iterdir() if d.is_dir()]
        with open(str(model_dir) + ".txt") as fh:
            model_report = fh.read()
        with open(model_dir.name + ".txt") as fh:
            reports[switch] = (model_report, fh.read())
        lines_at = str(model_dir) + "_hp_states.jsonl"
        if switch == "0":
            assert not os.path.exists(lines_at)
            continue
        with open(lines_at) as fh:
            (line,) = fh.read().splitlines()
        record = json.loads(line)
        assert record["step"] == 20 and record["threshold"] == 0.5 and record["edges"] == [35, 70, 140]
        assert record["states"] == ["complete", "incomplete", "absent"]
        hp_states, called_states = np.array(record["hp_states"]), np.array(record["called_states"])
        assert hp_states.shape == called_states.shape == (4, 3) and hp_states.sum() > 0
        assert record["hp_found"] == hp_states[:, :2].sum() / hp_states.sum() and 0 <= record["called_absent"] <= 1
    assert "Saved checkpoint at step 20" in reports["0"][0] and "---NEXT ROUND OF VALIDATION---" in reports["0"][1]
    assert reports["0"] == reports["1"]


def test_refusals_arrive_as_value_errors(engine, planted):
    """(d) argument errors only, refused on the host before any launch; the engine stays usable."""
    import torch
    ok = dict(thresholds=(0.5,), edges=(35,), min_run=15)

    def call(case=planted, work=None, counts=None, **kw):
        args = dict(ok, **kw)
        k = max(len(args["thresholds"]), 1)
        counts = torch.zeros(k * 2 * (len(args["edges"]) + 1) * 3, dtype=torch.int64, device="cuda:0") if counts is None else counts
        work = torch.zeros(max(engine.run_states_work_bytes(case["total"], k), 1), dtype=torch.uint8, device="cuda:0") if work is None else work
        engine.run_states_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"], case["longest"],
                                     args["thresholds"], args["edges"], counts, work, min_run=args["min_run"])

    for bad in (dict(thresholds=()), dict(thresholds=THRESHOLDS + (0.125,)), dict(edges=(1, 2, 3, 4, 5, 6, 7, 8)), dict(edges=(0,)),
                dict(edges=(-5, 3)), dict(edges=(35, 35)), dict(edges=(70, 35)), dict(min_run=0), dict(min_run=-1)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):                        # a work buffer one byte short
        call(work=torch.zeros(engine.run_states_work_bytes(planted["total"], 1) - 1, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):                        # n = 0
        call(case=dict(planted, bounds=planted["bounds"][:1], length=planted["length"][:0]))
    with pytest.raises(ValueError):                        # too small a table
        call(counts=torch.zeros(11, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError):                        # probabilities of another type
        call(case=dict(planted, probs=planted["probs"].double()))
    with pytest.raises(ValueError):                        # longest > total
        call(case=dict(planted, longest=planted["total"] + 1))
    lib = engine._lib                                       # null pointers, straight at the C entry
    import ctypes as C
    from catfish_amd import _native as N
    one = (C.c_double * 1)(0.5)
    buf = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    good = [None, C.c_void_p(planted["probs"].data_ptr()), C.c_void_p(planted["y"].data_ptr()), C.c_void_p(planted["bounds"].data_ptr()),
            C.c_void_p(planted["length"].data_ptr()), 1, 64, 64, one, 1, None, 0, 15, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), 2048, None]
    for position in (1, 2, 3, 4, 8, 13, 14):
        args = list(good)
        args[position] = None
        with pytest.raises(ValueError):
            N.check(lib.cf_validation_run_states(*args))
    args = list(good)
    args[11] = 1                                           # one edge announced, none given
    with pytest.raises(ValueError):
        N.check(lib.cf_validation_run_states(*args))
    assert np.array_equal(run_states_on_device(engine, planted, (0.5,), (35,)),
                          dv.run_states_host(*planted["host"], (0.5,), (35,)))
