"""``training.Trainer`` in every mode of ``catfish_amd/train_mode.py``'s table, run captured, eagerly and fed by the card, against
what commit e39d6a2 (the last one with the per-mode branches in ``Trainer``) computed on an MI355X with the same library:
``tests/golden/trainer_modes_e39d6a2.json`` holds that commit's losses (float32 bit patterns) and SHA-256 digests of its variables
and optimizer slots, written by ``PYTHONPATH=<that checkout> python tests/test_trainer_modes_gpu.py OUT.json``."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from catfish_amd.device_db import DeviceExampleDb
from oracle import catfish_oracle as oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_modes_e39d6a2.json")
STEPS = 6
# the whole step on the HIP kernels: dropout hashed from (seed, layer, opt.t, element), fixed-order reductions -> bit-equal trajectories
NATIVE = {"tuned_step": ("shipped", None, "fp32"), "anysize_step-128-64": ((128, 64, 2, 1), True, "fp32"),
          "anysize_step-128-64-bf16x3": ((128, 64, 2, 1), True, "bf16x3"), "anysize_step-rnn32": ((32, 32, 2, 0), True, "fp32")}
NATIVE_WAYS = ("captured", "eager", "fed", "eager50")       # 50 windows: not a multiple of the 16-window tile, the padded tail
# autograd around the any-size recurrences: dropout comes from torch generators that every replay advances -> compared without it
AUTOGRAD = {"anysize_autograd-rnn32": (32, 32, 2, 0), "anysize_autograd-128-64": (128, 64, 2, 1)}
AUTOGRAD_WAYS = ("captured", "eager", "fed")


def _pools():
    rng = np.random.default_rng(12)
    return rng.normal(size=(500, 35)).astype(np.float32), rng.normal(size=(900, 35)).astype(np.float32)


def _db():
    return DeviceExampleDb(*_pools(), seed=7)


def _weights(geo, ckpt_weights):
    if geo == "shipped":
        return ckpt_weights, 3, 2
    h, c, n_layers, n_blocks = geo
    return oracle.random_weights(seed=21, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks), n_layers, n_blocks


def _trainer(geo, ckpt_weights, native, kp, **kw):
    from catfish_amd.training import Trainer
    w, n_layers, n_blocks = _weights(geo, ckpt_weights)
    return Trainer(w, n_layers, n_blocks, "RMSProp" if geo == "shipped" else "Adam", 1e-3, kp, seed=5, native=native, **kw)


def _digest(named):
    h = hashlib.sha256()
    for k in sorted(named):
        a = np.ascontiguousarray(named[k])
        h.update(("%s %s %s" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _bits(losses):
    return [int(v) for v in np.asarray(losses, dtype=np.float32).view(np.uint32)]


def run_way(geo, ckpt_weights, native, kp, precision, way):
    """Six steps one way -> {"losses": float32 bit patterns, "variables": digest, "slots": digest of both optimizer slots}."""
    n = 50 if way == "eager50" else 64
    tr = _trainer(geo, ckpt_weights, native, kp, precision=precision, use_graph=way in ("captured", "fed"))
    try:
        if way == "fed":
            db = _db()
            losses = tr.train_steps(db, STEPS, n)
            assert db.draw == STEPS and tr._fed is not None and tr._graph is None
        else:
            twin = _db()
            losses = [tr.train_step(x, y) for x, y, _ in (twin.get_training_set(n) for _ in range(STEPS))]
            assert tr._fed is None and (tr._graph is not None) == (way == "captured")
        assert float(tr.opt.t) == STEPS and tr.last_loss == float(np.float32(losses[-1]))
        return {"losses": _bits(losses), "variables": _digest(tr.net.numpy_weights()), "slots": _digest(tr.opt.state_tf())}
    finally:
        if tr.engine is not None:
            tr.engine.close()


def _masks(n, h, n_layers, kp, seed=3):
    rng = np.random.default_rng(seed)
    return {(layer, d): (rng.random((n, 35, h)) < kp).astype(np.float32) for layer in range(n_layers) for d in ("fw", "bw")}


def run_masks(ckpt_weights):
    """Two eager steps of the 32-unit ``anysize_autograd`` trainer with explicit masks at keep_prob 0.8."""
    geo = (32, 32, 2, 0)
    tr = _trainer(geo, ckpt_weights, None, 1.0)
    try:
        twin = _db()
        losses = []
        for i in range(2):
            x, y, _ = twin.get_training_set(64)
            losses.append(tr.train_step(x, y, keep_prob=0.8, masks=_masks(64, 32, 2, 0.8, seed=3 + i)))
        assert tr._graph is None and float(tr.opt.t) == 2.0
        return {"losses": _bits(losses), "variables": _digest(tr.net.numpy_weights()), "slots": _digest(tr.opt.state_tf())}
    finally:
        tr.engine.close()


def record(ckpt_weights):
    out = {}
    for name, (geo, native, precision) in NATIVE.items():
        out[name] = {way: run_way(geo, ckpt_weights, native, 0.8, precision, way) for way in NATIVE_WAYS}
    for name, geo in AUTOGRAD.items():
        out[name] = {way: run_way(geo, ckpt_weights, None, 1.0, "fp32", way) for way in AUTOGRAD_WAYS}
    out["anysize_autograd-rnn32-masks"] = {"eager": run_masks(ckpt_weights)}
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _floats(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("way", NATIVE_WAYS)
@pytest.mark.parametrize("name", sorted(NATIVE))
def test_native_step_trajectories_are_what_they_were(name, way, golden, ckpt_weights):
    """Losses, variables and both optimizer slots after six steps at keep_prob 0.8, bit for bit.  The recording's two runs on
    e39d6a2 agreed with each other in every case, and its captured, eager and device-fed runs of one mode with one another."""
    geo, native, precision = NATIVE[name]
    want = golden[name]
    assert want["captured"] == want["eager"] == want["fed"] and want["eager50"] != want["eager"]
    got = run_way(geo, ckpt_weights, native, 0.8, precision, way)
    print(name, way, "losses", _floats(got["losses"]), "recorded", _floats(want[way]["losses"]))
    assert got == want[way]


# what the recording saw: do two runs of e39d6a2 give the same bits?  (tests/test_device_db_gpu.py::test_device_fed_equals_host_fed's
# rule: bit-equal where they do, else the 1e-6 that DESIGN section 4 documents for these trajectories).  The 32-unit RNN repeated
# itself bit for bit in all three ways.  128 / 64 did not: two runs of e39d6a2 differed by one float32 ulp of the loss (6e-8) in
# every way, as that test's docstring already reports for its host-fed runs.
AUTOGRAD_TOL = {"anysize_autograd-rnn32": 0.0, "anysize_autograd-128-64": 1e-6}


@pytest.mark.parametrize("way", AUTOGRAD_WAYS)
@pytest.mark.parametrize("name", sorted(AUTOGRAD))
def test_autograd_trajectories_are_what_they_were(name, way, golden, ckpt_weights):
    got = run_way(AUTOGRAD[name], ckpt_weights, None, 1.0, "fp32", way)
    have, want = _floats(got["losses"]), _floats(golden[name][way]["losses"])
    tol = AUTOGRAD_TOL[name]
    print(name, way, "losses", have, "recorded", want, "largest difference", np.abs(have.astype(np.float64) - want).max(), "tolerance", tol)
    assert np.isfinite(have).all()
    if tol:
        assert np.abs(have.astype(np.float64) - want).max() <= tol
    else:
        assert got["losses"] == golden[name][way]["losses"]


def test_explicit_masks_go_through_the_autograd_step(golden, ckpt_weights):
    got = run_masks(ckpt_weights)
    print("losses", _floats(got["losses"]), "recorded", _floats(golden["anysize_autograd-rnn32-masks"]["eager"]["losses"]))
    assert got["losses"] == golden["anysize_autograd-rnn32-masks"]["eager"]["losses"]


# ---------------------------------------------------------------------------------------------------- attributes per kind
# name -> (kind, geometry, native, the CPU table's row (tests/test_train_mode.py::GRID), step class or None); every one is stepped
KINDS = {"tuned_step": ("tuned_step", "shipped", None, (True, "cuda", True, None, 1, "fp32"), "NativeTrainStep"),
         "anysize_step": ("anysize_step", (32, 32, 2, 0), True, (False, "cuda", True, True, 0, "fp32"), "AnySizeTrainStep"),
         "anysize_autograd": ("anysize_autograd", (32, 32, 2, 0), None, (False, "cuda", True, None, 0, "fp32"), None),
         # 64 units where the tuned kernels do not go: without a conv stack (a one-feature input) when native=True asks, and with
         # five blocks, one more than the tuned conv-stack kernels have
         "anysize_step-rnn64": ("anysize_step", (64, 32, 2, 0), True, (True, "cuda", True, True, 0, "fp32"), "AnySizeTrainStep"),
         "anysize_autograd-64-32-x5": ("anysize_autograd", (64, 32, 2, 5), None, (True, "cuda", True, None, 5, "fp32"), None),
         "anysize_step-64-32-x5": ("anysize_step", (64, 32, 2, 5), True, (True, "cuda", True, True, 5, "fp32"), "AnySizeTrainStep"),
         "torch": ("torch", (32, 32, 2, 0), False, (False, "cuda", True, False, 0, "fp32"), None)}


@pytest.mark.parametrize("name", sorted(KINDS))
def test_attributes_follow_the_table(name, ckpt_weights):
    from test_train_mode import GRID
    from catfish_amd.training import AutogradStep
    kind, geo, native, row, step_class = KINDS[name]
    want_kind, engine_kwargs, want_native, want_anysize = GRID[row]
    assert want_kind == kind
    tr = _trainer(geo, ckpt_weights, native, 1.0)
    try:
        assert tr.mode == kind and tr.native is want_native and tr.anysize is want_anysize
        assert (tr.engine is None) == (engine_kwargs is None)
        if step_class is None:
            assert tr.step_impl is None and type(tr.step) is AutogradStep
        else:
            assert type(tr.step_impl).__name__ == step_class and tr.step is tr.step_impl
        assert tr.use_graph and tr._graph is None and tr._fed is None and tr.last_loss is None
        twin = _db()
        x, y, _ = twin.get_training_set(64)
        loss = tr.train_step(x, y)
        assert tr._graph is not None and tr._fed is None and tr.last_loss == loss
        db = _db()
        losses = tr.train_steps(db, 2, 64)
        assert tr._graph is not None and tr._fed is not None and tr._fed["key"] == (64, 2) and tr.last_loss == float(losses[-1])
        assert float(tr.opt.t) == 3.0 and np.isfinite(losses).all() and np.isfinite(loss)
    finally:
        if tr.engine is not None:
            tr.engine.close()


if __name__ == "__main__":                                 # the recording: PYTHONPATH=<checkout> python tests/test_trainer_modes_gpu.py OUT.json
    with np.load(os.path.join(os.path.dirname(GOLDEN), "ckpnt-30000-inference.npz")) as z:
        ckpt = {k: z[k] for k in z.files}
    with open(sys.argv[1], "w") as fh:
        json.dump(record(ckpt), fh, indent=1, sort_keys=True)
