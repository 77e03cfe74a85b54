"""The curve step on the card (csrc/validation_curve.hpp through the C ABI) against ``device_validation.curve_host``: tensors the
test writes itself straight into the kernel (every length around the chunk, every special bit pattern, inputs that pile up on one
cell), the refusals, then a whole round through a 64 / 32 model with random weights, ``validation_curves`` and the per-round JSON
line of ``train_validate.main``."""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_validation as dv
from catfish_amd import train_validate as tv
from catfish_amd.device_validation import DeviceValidationSet

pytestmark = pytest.mark.gpu

SHIFTS = (10, 14, 22)
ONE = 0x3F800000
LENGTHS = (0, 1, 34, 35, 36, 2047, 2048, 2049, 4097, 70000)
TAIL_BITS = 0x3F666666                                     # 0.9 in the zero tails: a tail taken for a sample would show


@pytest.fixture(scope="module")
def engine(hp):
    from catfish_amd.resnet_class import ResNetRNN
    net = ResNetRNN(**hp)
    net.initialize_network(seed=11)
    yield net.engine
    net.engine.close()


def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


def _case(bits, y, lengths, window=35):
    """Packed as a round packs it: stretch r holds its ``lengths[r]`` patterns, its tail TAIL_BITS and label 0."""
    lengths = np.asarray(lengths, dtype=np.int64)
    bounds, _tails = dv.layout(lengths, window)
    total = int(bounds[-1])
    packed = np.full(max(total, 1), TAIL_BITS, dtype=np.uint32)
    labels = np.zeros(max(total, 1), dtype=np.uint8)
    at = 0
    for b0, n in zip(bounds[:-1].tolist(), lengths.tolist()):
        packed[b0:b0 + n] = bits[at:at + n]
        labels[b0:b0 + n] = y[at:at + n]
        at += n
    probs = packed.view(np.float32)
    return {"probs": _dev(probs), "y": _dev(labels), "bounds": _dev(bounds), "length": _dev(lengths), "total": total,
            "longest": int(np.diff(bounds).max()), "host": (probs, labels, bounds, lengths)}


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(14)
    n = int(np.sum(LENGTHS))
    bits = rng.integers(0, ONE + 1, size=n, dtype=np.int64).astype(np.uint32)               # uniform over the patterns of [0, 1]
    special = [0x00000000, ONE, 0x00000001, 0x007FFFFF, 0x80000000, 0xBF000000, ONE + 1, 0x7F800000, 0x7FC00000, 0xFFC00000]
    for shift in SHIFTS:                                   # bin edges and one ulp either side, low, middle and top
        for b in (1, 2, (ONE >> shift) // 2, (ONE >> shift) - 1, ONE >> shift):
            special += [(b << shift) - 1, b << shift, (b << shift) + 1]
    where = rng.choice(np.arange(72, n), size=4 * len(special), replace=False)              # (the first stretches keep their own)
    bits[where] = np.tile(np.array(special, dtype=np.uint32), 4)
    bits[:len(special)] = np.array(special, dtype=np.uint32)                                 # ... and the short stretches get some too
    y = rng.choice(np.uint8([0, 0, 0, 1, 1, 1, 2, 255]), size=n)
    case = _case(bits, y, LENGTHS)
    case["want"] = {shift: dv.curve_host(*case["host"], shift) for shift in SHIFTS}          # computed once
    return case


def curve_on_device(engine, case, shift, longest=None, out=None):
    import torch
    cells = 3 * dv.curve_bins(shift)
    hist = torch.full((cells,), -1, dtype=torch.int64, device="cuda:0") if out is None else out
    engine.curve_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"],
                            case["longest"] if longest is None else longest, shift, hist)
    torch.cuda.synchronize()
    engine.check_error()
    return hist.cpu().numpy().reshape(3, -1)


@pytest.mark.parametrize("shift", SHIFTS)
def test_planted_patterns_equal_the_host_statement(engine, planted, shift):
    """Bit-equal to curve_host; a second call into the same buffer gives the same bits (the zeroing, the repeatability); the grid
    hint does not show."""
    import torch
    want = planted["want"][shift]
    assert want.sum() == np.sum(LENGTHS) and (want.sum(axis=1) > 0).all() and want[0, -1] > 0 and want[1, 0] > 0
    hist = torch.full((3 * dv.curve_bins(shift),), -1, dtype=torch.int64, device="cuda:0")
    first = curve_on_device(engine, planted, shift, out=hist)
    assert first.dtype == np.int64 and np.array_equal(first, want)
    assert np.array_equal(curve_on_device(engine, planted, shift, out=hist), first)
    assert np.array_equal(curve_on_device(engine, planted, shift, longest=1), first)         # real longest: 70 000


def test_inputs_that_pile_up_on_one_cell(engine):
    n = 300000
    half = np.float32(0.5).view(np.uint32)
    cases = [_case(np.full(n, half, dtype=np.uint32), np.ones(n, dtype=np.uint8), [n])]
    y = (np.arange(n) % 3 == 0).astype(np.uint8)
    cases.append(_case(np.where(y == 1, ONE, 0).astype(np.uint32), y, [n]))                  # p = 1.0 for label 1, 0.0 for label 0
    few = np.random.default_rng(2).integers(0, ONE + 1, size=2000, dtype=np.int64).astype(np.uint32)
    cases.append(_case(few, (few & 1).astype(np.uint8), [1] * 2000))                         # 2 000 stretches of one sample
    for case in cases:
        for shift in (14, 22):
            want = dv.curve_host(*case["host"], shift)
            assert want.sum() == case["host"][3].sum()
            assert np.array_equal(curve_on_device(engine, case, shift), want)
    assert dv.curve_host(*cases[0]["host"], 14)[0, int(half) >> 14] == n


def test_refusals_write_nothing(engine, planted):
    import torch
    nb = dv.curve_bins(14)
    hist = torch.full((3 * nb,), -1, dtype=torch.int64, device="cuda:0")

    def call(case=planted, shift=14, out=hist):
        engine.curve_validation(case["probs"], case["y"], case["bounds"], case["length"], case["total"], case["longest"], shift, out)

    for bad in (dict(shift=9), dict(shift=23), dict(out=hist[:3 * nb - 1]),
                dict(case=dict(planted, bounds=planted["bounds"][:1], length=planted["length"][:0])),        # n = 0
                dict(case=dict(planted, probs=planted["probs"].double())), dict(case=dict(planted, longest=planted["total"] + 1)),
                dict(shift=14.5), dict(out=hist.int())):
        with pytest.raises(ValueError):
            call(**bad)
    import ctypes as C
    from catfish_amd import _native as N
    good = [None, C.c_void_p(planted["probs"].data_ptr()), C.c_void_p(planted["y"].data_ptr()), C.c_void_p(planted["bounds"].data_ptr()),
            C.c_void_p(planted["length"].data_ptr()), len(LENGTHS), planted["total"], planted["longest"], 14, C.c_void_p(hist.data_ptr()),
            3 * nb, None]
    for position in (1, 2, 3, 4, 9):                        # null pointers, straight at the C entry
        args = list(good)
        args[position] = None
        with pytest.raises(ValueError):
            N.check(engine._lib.cf_validation_curve(*args))
    torch.cuda.synchronize()
    assert bool((hist == -1).all())
    assert np.array_equal(curve_on_device(engine, planted, 14, out=hist), planted["want"][14])          # the engine stays usable


# ---------------------------------------------------------------------------------------------------------------- whole rounds
READS = (300, 701, 1500, 2048, 3333, 5000)


def _validation_reads(tmp_path):
    val_dir = tmp_path / "val"
    val_dir.mkdir()
    paths = []
    for i, n in enumerate(READS):
        raw, lab = tv.synthetic_labelled_read(n, seed=90 + i)
        paths.append(str(val_dir / ("sq%d.npz" % i)))
        np.savez(paths[-1], raw=raw, base_labels=lab)
    return paths


def _read_back(net, selection):
    """(probs, y, bounds, real) of the round just scored: ``real`` marks the samples that are not tail."""
    bounds, _tails = dv.layout(selection[2], 35)
    total = int(bounds[-1])
    t = net.validation_buffers["tensors"]
    real = np.zeros(total, dtype=bool)
    for b0, n in zip(bounds[:-1].tolist(), selection[2].tolist()):
        real[b0:b0 + n] = True
    return t["probs"][:total].cpu().numpy(), t["y"][:total].cpu().numpy(), bounds, real


def pairwise_auc(scores, y):
    pos, neg = scores[y == 1].astype(np.float64), scores[y == 0].astype(np.float64)
    wins = 0.0
    for a in range(0, pos.size, 1024):
        block = pos[a:a + 1024, None]
        wins += np.count_nonzero(block > neg[None, :]) + 0.5 * np.count_nonzero(block == neg[None, :])
    return wins / (pos.size * neg.size)


def test_a_whole_round_and_validation_curves(hp, tmp_path):
    from catfish_amd.resnet_class import ResNetRNN
    resident = DeviceValidationSet.from_npz(_validation_reads(tmp_path))
    selection = resident.select(35, 0, "complete", 856)
    assert selection[2].tolist() == list(READS)
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    net.score_validation_device(resident, selection, (0.5,))
    probs, y, bounds, real = _read_back(net, selection)
    edges = dv.curve_thresholds(14)
    at = sorted(set(int(b) for b in dv.curve_bin(np.quantile(probs[real], [0.1, 0.3, 0.5, 0.7, 0.9]).astype(np.float32).view(np.uint32), 14)))
    at = (at + [b for b in (1, 2, 3, 4, 5) if b not in at])[:5]                               # five bin edges the model's scores reach
    thresholds = tuple(float(edges[b]) for b in at)
    plain = net.score_validation_device(resident, selection, thresholds)
    before = dict(net.validation_buffers["capacity"])
    assert len(plain) == 3 and "curve_cells" not in before
    got = net.score_validation_device(resident, selection, thresholds, curve_shift=14)
    assert len(got) == 4 and net.validation_buffers["capacity"]["curve_cells"] == 3 * 65025
    for a, b in zip(plain, got[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    probs, y, bounds, real = _read_back(net, selection)
    hist = got[3]
    assert hist.dtype == np.int64 and hist.shape == (3, 65025) and hist.sum() == sum(READS)
    assert np.array_equal(hist, dv.curve_host(probs, y, bounds, selection[2], 14))
    # the cumulative sums are that call's counts, which also hold the tail samples (label 0: false positive when called, else
    # in the raw true negatives)
    curves = dv.curves_from_histogram(hist, 14)
    assert not np.isnan(probs).any()
    for k, b in enumerate(at):
        tail_called = int(np.count_nonzero(probs[~real] >= edges[b]))
        want = (curves["tp"][b], curves["fp"][b] + tail_called, curves["tn"][b] + int((~real).sum()) - tail_called, curves["fn"][b])
        assert got[2][k].tolist() == [int(v) for v in want], (k, b)
    five = net.score_validation_device(resident, selection, thresholds, run_edges=(35, 70), curve_shift=14)
    assert len(five) == 5 and five[3].shape == (5, 2, 3, 3) and np.array_equal(five[4], hist)
    assert np.array_equal(five[3], net.score_validation_device(resident, selection, thresholds, run_edges=(35, 70))[3])
    for a, b in zip(plain, five[:3]):
        assert a.tobytes() == b.tobytes()
    small = net.score_validation_device(resident, selection, thresholds, curve_shift=22)      # another shift: the room stays (grow-only)
    assert small[3].shape == (3, 255) and np.array_equal(small[3], dv.curve_host(probs, y, bounds, selection[2], 22))
    assert net.validation_buffers["capacity"]["curve_cells"] == 3 * 65025
    again = net.score_validation_device(resident, selection, thresholds)                       # and back: three results, the same bits
    assert len(again) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))
    with pytest.raises(ValueError):
        net.score_validation_device(resident, selection, thresholds, curve_shift=9)

    curves = tv.validation_curves(net, resident, 0)
    assert curves["shift"] == 14 and np.array_equal(curves["thresholds"], edges)
    assert sorted(curves) == sorted(["tp", "fp", "tn", "fn", "n_pos", "n_neg", "n_other", "tpr", "fpr", "precision", "recall", "roc_auc",
                                     "roc_auc_slack", "pr_auc", "best_f1", "shift", "thresholds"])
    assert np.array_equal(curves["tp"], dv.curves_from_histogram(hist, 14)["tp"])
    assert curves["n_pos"] == int(np.count_nonzero(y[real] == 1)) > 0 and curves["n_neg"] == int(np.count_nonzero(y[real] == 0)) > 0
    exact = pairwise_auc(probs[real], y[real])
    print("roc_auc %.9f +- %.3g, pairwise on the probabilities %.9f, pr_auc %.6f, best f1 %r" % (
        curves["roc_auc"], curves["roc_auc_slack"], exact, curves["pr_auc"], curves["best_f1"]))
    assert abs(exact - curves["roc_auc"]) <= curves["roc_auc_slack"] + 1e-12                   # (1e-12: float64 rounding of the quotients)
    assert 0.0 <= curves["pr_auc"] <= 1.0 and 0.0 <= curves["best_f1"]["f1"] <= 1.0
    coarse = tv.validation_curves(net, resident, 0, shift=22)
    assert coarse["thresholds"].shape == (255,) and abs(exact - coarse["roc_auc"]) <= coarse["roc_auc_slack"] + 1e-12
    net.engine.close()


def test_the_report_line(tmp_path, monkeypatch):
    """CATFISH_VALIDATION_CURVE=1 appends one JSON line per checkpoint round and leaves both .txt reports as they are without it."""
    _validation_reads(tmp_path)
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
    for name in ("CATFISH_DEVICE_DB", "CATFISH_NATIVE_TRAINING", "CATFISH_TRAINING_PRECISION", "CATFISH_VALIDATION_RUNS"):
        monkeypatch.delenv(name, raising=False)
    reports = {}
    for switch in ("0", "1"):
        (tmp_path / switch).mkdir()
        monkeypatch.chdir(tmp_path / switch)
        monkeypatch.setenv("CATFISH_VALIDATION_CURVE", switch)
        tv.main(["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"])
        (model_dir,) = [d for d in (tmp_path / switch).iterdir() if d.is_dir()]
        with open(str(model_dir) + ".txt") as fh:
            model_report = fh.read()
        with open(model_dir.name + ".txt") as fh:
            reports[switch] = (model_report, fh.read())
        lines_at = str(model_dir) + "_curves.jsonl"
        assert not os.path.exists(str(model_dir) + "_hp_states.jsonl")
        if switch == "0":
            assert not os.path.exists(lines_at)
            continue
        with open(lines_at) as fh:
            (line,) = fh.read().splitlines()
        assert "NaN" not in line
        record = json.loads(line)
        assert sorted(record) == ["best_f1", "n_neg", "n_other", "n_pos", "pr_auc", "roc_auc", "roc_auc_slack", "shift", "step"]
        assert record["step"] == 20 and record["shift"] == 14 and record["n_other"] == 0
        assert record["n_pos"] + record["n_neg"] == 1050 * sum(1 for n in READS if n >= 1050) and record["n_pos"] > 0
        assert 0.0 <= record["roc_auc"] <= 1.0 and 0.0 <= record["roc_auc_slack"] <= 0.5 and 0.0 <= record["pr_auc"] <= 1.0
        assert sorted(record["best_f1"]) == ["f1", "precision", "recall", "threshold"]
    assert "Saved checkpoint at step 20" in reports["0"][0] and "---NEXT ROUND OF VALIDATION---" in reports["0"][1]
    assert reports["0"] == reports["1"]
    assert tv._json_line({"a": float("nan"), "b": {"c": float("nan"), "d": 1.5}}) == '{"a": null, "b": {"c": null, "d": 1.5}}\n'
