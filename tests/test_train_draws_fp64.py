"""Every cell of the random search's space takes a step, and its loss and gradients are float64's (GPU).

tests/test_train_draws_host.py maps every network that ``generate_random_hyperparameters`` can draw, with ``native_training`` and
``training_precision``, to a cell (kind, type, 64 units?, depth class, precision) and lists one or two cases per cell in
``STEPPED_CELLS``.  This module builds each case through the public surface -- ``train_validate.build_model(type, **hp)``,
``initialize_network(seed=...)``, ``train_network`` -- and checks, per case:

  1  ``net._trainer.mode``, ``.native``, ``.anysize`` and the step's class are the cell's;
  2  ``Trainer.gradients(x, y, keep_prob=1.0)`` at 50 windows (a ragged fourth tile) against ``TorchResNetRNN(dtype=float64)`` on
     the same batch: the loss (absolute error) and every trainable tensor by TF name (``max|d| / max|ref|``);
  3  two ``train_network`` steps at the case's own ``keep_prob`` at 64 windows (the captured step): finite losses, ``opt.t == 2``,
     another loss the second time, another ``infer`` afterwards.

Beside them: the 64-unit RNN's device-fed steps against host-fed ones on the twin database, bit for bit; save / load / resume of the
three cells that came to the any-size kernels with this module (before, their first step was refused); 64 / 32 in float64 on the card against the CPU; the
library's deepest tuned conv stack against ``train_mode.TUNED_MAX_BLOCKS``.

Bounds of item 2.  The rule of tests/test_train_kernels_fp64.py and tests/test_anysize_train_x3.py.  A measuring run
(CATFISH_PARITY_LOG names a file) records for every case and quantity the kernels' error and the error of the float32 pure-torch
``Trainer(native=False)`` on the same batch; a bf16x3 case adds the error of the scheme's float64 emulation
(``test_anysize_train_x3._emulated_loss``), and its yardstick is the sum of the two.  The asserted bound of a quantity is 4 x the
largest yardstick over its section (S: fp32, X: bf16x3), rounded down to three digits, and never looser than the older bounds
(loss 5e-6 absolute, gradients 2e-3).  The rows are in profiles/train_draws_fp64_parity.jsonl; ``BOUNDS`` holds the constants and
tests/test_train_draws_host.py checks them against that file.

As measured, every case meets the rule and none falls back to the older bound.  Both gradient yardsticks come from the smallest
network, the 16-unit one-layer RNN, whose ``final_fully_connected/bias`` gradient is a near-cancelling sum over 1750 positions
(float32 torch 9.05e-6, the emulation 8.36e-5 of its tiny maximum).  The fp32 kernels' largest gradient error is 2.74e-5, on the
first layer's candidate bias of the five-layer 64-unit RNN: 6.0 x that case's own yardstick (7.8 x at one layer), yet 0.76 x the
bound.  It is a cancelling sum, not a matter of 64 units or of the one-feature input: on this batch that gradient, 1750 terms of
both signs, has a largest element of 1.2e-3.  A per-tensor look (one run, not in the profile) found the kernels' absolute error on
it to be 1.5e-8 here and 1.9e-8 on a batch of 64 windows where the gradient is four times as large (3.9e-6 relative), and the same
factor on the same tensor at 16 units (8.1e-6 against float32 torch's 1.4e-6): what one expects of a running fp32 sum over all
positions beside torch's pairwise reduction.  The loss moves in
float32 ulps of a value near 0.69 (6e-8): one ulp is already 8.6 x the float32 trainer's error where that happens to round to the
float64 loss (16 / 16, 1.1e-9), which is why the bound is a section's, not a case's.  bf16x3 sits on the emulation: 0.85 .. 1.02 x
its case's yardstick on the gradients.  The runs are deterministic up to one ulp of the autograd paths' losses; if a reordering of
sums trips a bound, re-measure, do not widen by hand.  The longest case (64 / 32 with five blocks through autograd, which builds
the convolution library's kernels) takes 4 s, most take under 0.5 s.
"""
import json
import os

import numpy as np
import pytest

import test_train_draws_host as draws
from test_train_draws_host import STEPPED_CELLS, hyperparameters
from test_train_kernels_fp64 import T, _measuring, _rel, _stamp
from test_trainer_modes_gpu import AUTOGRAD_TOL, _db

pytestmark = pytest.mark.gpu

# quantity -> asserted bound = min(4 x largest yardstick over the section, older bound).  The largest yardsticks in
# profiles/train_draws_fp64_parity.jsonl (MI355X, 256 CUs), float32 torch (+ emulation), and the kernels' largest error next to them:
#   S.loss 6.457e-08 (kernels 6.75e-08)      S.grads 9.052e-06 (2.74e-05)
#   X.loss 5.66e-08 + 5.91e-08 (1.11e-07)    X.grads 9.05e-06 + 8.358e-05 (8.56e-05)
# 4 x each, rounded down, is below the older bound of its quantity (loss 5e-6 absolute, gradients 2e-3), so it is the bound.
BOUNDS = {"S.loss": 2.58e-7, "S.grads": 3.62e-5, "X.loss": 4.62e-7, "X.grads": 3.70e-4}
OLDER_BOUNDS = {"S.loss": 5e-6, "S.grads": 2e-3, "X.loss": 5e-6, "X.grads": 2e-3}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "train_draws_fp64_parity.jsonl")
INIT_SEED = 7

# kind -> (Trainer.native, Trainer.anysize, class of Trainer.step, is it Trainer.step_impl, has the trainer an engine)
EXPECT = {"tuned_step": (True, False, "NativeTrainStep", True, True), "anysize_step": (True, False, "AnySizeTrainStep", True, True),
          "anysize_autograd": (False, True, "AutogradStep", False, True), "torch": (False, False, "AutogradStep", False, False)}


def bounds_from_profile(path=PROFILE):
    """{quantity: min(4 x largest (float32-torch + emulation) error in the profile, older bound)}: what ``BOUNDS`` may not exceed."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            key = "%s.%s" % (row["section"], row["quantity"])
            worst[key] = max(worst.get(key, 0.0), row["torch_fp32"] + (row["emulation"] or 0.0))
    return {k: min(4.0 * v, OLDER_BOUNDS[k]) for k, v in worst.items()}


def _record(section, case, quantity, kernel, torch_fp32, emulation, worst):
    row = {"section": section, "case": case, "quantity": quantity, "kernel": float(kernel),
           "torch_fp32": None if torch_fp32 is None else float(torch_fp32), "emulation": None if emulation is None else float(emulation),
           "worst": worst}
    print("parity %s" % json.dumps(row))
    path = os.environ.get("CATFISH_PARITY_LOG")
    if path and torch_fp32 is not None:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(_stamp(), **row)) + "\n")


def _batch(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1.2, size=(n, T)).astype(np.float32)
    y = np.repeat((rng.random(n) < 0.4)[:, None], T, axis=1).astype(np.float32)
    return x, y


def _build(case, batch_size=64, **override):
    from catfish_amd import train_validate as tv
    net = tv.build_model(case.network_type, train_seed=5, **dict(hyperparameters(case, batch_size), **override))
    net.initialize_network(seed=INIT_SEED)
    return net


def _close(*nets):
    for net in nets:
        if net._trainer is not None and net._trainer.engine is not None:
            net._trainer.engine.close()
        if net.engine is not None:
            net.engine.close()


# ------------------------------------------------------------------------------------------------ the float64 side, once per geometry
_REFERENCE = {}


def _grad_errors(grads, ref_grads):
    """(largest per-tensor error of {TF name: ndarray} against the float64 gradients, the tensor that has it)."""
    import torch
    assert sorted(grads) == sorted(ref_grads)
    errs = {k: _rel(torch.as_tensor(np.asarray(grads[k])), g) for k, g in ref_grads.items()}
    worst = max(errs, key=errs.get)
    return errs[worst], worst


def _reference(case, weights, n_blocks, x, y):
    """Loss and gradients of the case's network on (x, y) in float64, shared by every case of the same geometry; in a measuring
    run also the errors of the float32 torch trainer and of the bf16x3 scheme's float64 emulation against them."""
    import torch
    from catfish_amd.training import TorchResNetRNN, Trainer
    key = (case.network_type, case.layer_size, case.n_layers, case.layer_size_res)
    ref = _REFERENCE.get(key)
    if ref is None:
        net64 = TorchResNetRNN(weights, case.n_layers, n_blocks, device="cuda", dtype=torch.float64)
        loss64 = net64.loss(x, y)
        loss64.backward()
        ref = _REFERENCE[key] = {"loss": float(loss64.detach()), "grads": {k: p.grad.detach().cpu() for k, p in net64.trainable().items()}}
        assert all(float(g.abs().max()) > 0.0 for g in ref["grads"].values())
    if _measuring() and "torch_fp32" not in ref:
        yard = Trainer(weights, case.n_layers, n_blocks, "Adam", 1e-3, 1.0, device="cuda", native=False, use_graph=False)
        loss_t, grads_t = yard.gradients(x, y, keep_prob=1.0)
        assert yard.mode == "torch"
        ref["torch_fp32"] = (abs(loss_t - ref["loss"]),) + _grad_errors(grads_t, ref["grads"])
    if _measuring() and case.precision == "bf16x3" and "emulation" not in ref:
        import test_anysize_train_x3 as x3
        emu = TorchResNetRNN(weights, case.n_layers, n_blocks, device="cuda", dtype=torch.float64)
        ones = {(layer, d): np.ones((x.shape[0], T, case.layer_size), np.float32) for layer in range(case.n_layers) for d in ("fw", "bw")}
        loss_e = x3._emulated_loss(emu, x, y, 1.0, ones)
        loss_e.backward()
        ref["emulation"] = (abs(float(loss_e.detach()) - ref["loss"]),) + _grad_errors({k: p.grad.cpu().numpy() for k, p in emu.trainable().items()}, ref["grads"])
    return ref


# ------------------------------------------------------------------------------------------------ every cell
@pytest.mark.parametrize("case", STEPPED_CELLS, ids=[case.name for case in STEPPED_CELLS])
def test_draw_takes_its_path_matches_float64_and_steps(case):
    from catfish_amd.training import AutogradStep
    net = _build(case)
    try:
        tr = net._require_trainer()
        kind = case.cell[0]
        native, anysize, step_class, is_impl, has_engine = EXPECT[kind]
        # 1. the path is the cell's
        assert tr.mode == kind and tr.native is native and tr.anysize is anysize and tr.precision == case.precision
        assert type(tr.step).__name__ == step_class and (tr.step_impl is tr.step if is_impl else tr.step_impl is None)
        assert (tr.engine is not None) == has_engine and (step_class != "AutogradStep" or type(tr.step) is AutogradStep)
        assert draws.resolve(case.network_type, case.layer_size, case.n_layers, case.layer_size_res or 32, case.native, case.precision) == case.cell
        # 2. loss and gradients against float64, without dropout
        x, y = _batch(50, 50)
        loss_k, grads_k = tr.gradients(x, y, keep_prob=1.0)
        ref = _reference(case, net.weights, net.n_layers_res_, x, y)
        e_loss = abs(loss_k - ref["loss"])
        e_grads, worst = _grad_errors(grads_k, ref["grads"])
        t_loss, t_grads, t_worst = ref.get("torch_fp32", (None, None, None))
        m_loss, m_grads, m_worst = ref["emulation"] if case.precision == "bf16x3" and "emulation" in ref else (None, None, None)
        section = "X" if case.precision == "bf16x3" else "S"
        print("worst gradient of %s: %s (float32 torch: %s, emulation: %s)" % (case.name, worst, t_worst, m_worst))
        _record(section, case.name, "loss", e_loss, t_loss, m_loss, None)
        _record(section, case.name, "grads", e_grads, t_grads, m_grads, worst)
        # 3. two steps at the draw's own keep_prob, captured
        xs, ys = _batch(64, 64)
        probe = xs[:16].reshape(16, T, 1)
        before = net.infer(probe)
        losses = []
        for step in range(2):
            net.train_network(xs, ys, step)
            losses.append(net.train_loss)
        after = net.infer(probe)
        print("losses of %s: %r" % (case.name, losses))
        assert net._trainer is tr and tr._graph is not None and float(tr.opt.t) == 2.0
        assert np.isfinite(losses).all() and losses[1] != losses[0]
        assert np.isfinite(before).all() and np.isfinite(after).all() and not np.array_equal(before, after)
        bad = {q: (e, BOUNDS["%s.%s" % (section, q)]) for q, e in (("loss", e_loss), ("grads", e_grads)) if not e <= BOUNDS["%s.%s" % (section, q)]}
        assert not bad, (case.name, bad, worst)
    finally:
        _close(net)


# ------------------------------------------------------------------------------------------------ the 64-unit RNN fed by the card
def test_rnn64_native_device_fed_equals_host_fed():
    """``train_network_steps`` on a ``DeviceExampleDb`` (the sampler inside the captured step) against ``train_network`` on the twin
    database's batches: the same three losses, bit for bit (the rule of test_device_db_gpu.py::test_device_fed_equals_host_fed)."""
    case = {c.name: c for c in STEPPED_CELLS}["rnn64-x1-step"]
    fed, host = _build(case), _build(case)
    try:
        db, twin = _db(), _db()
        got = fed.train_network_steps(db, 3)
        assert fed._trainer.mode == "anysize_step" and fed._trainer._fed is not None and db.draw == 3
        want = []
        for step in range(3):
            x, y, _ = twin.get_training_set(64)
            host.train_network(x, y, step)
            want.append(host.train_loss)
        print("fed", got, "host", want)
        assert np.isfinite(got).all() and len(set(want)) == 3
        assert np.asarray(got, np.float32).view(np.uint32).tolist() == np.asarray(want, np.float32).view(np.uint32).tolist()
    finally:
        _close(fed, host)


# ------------------------------------------------------------------------------------------------ save, load, resume
@pytest.mark.parametrize("name", ["rnn64-x1-step", "res64-32-x5-step", "res64-32-x5-autograd"])
def test_resume_from_a_checkpoint_continues_the_run(name, tmp_path):
    """Three steps, ``save_network``, ``restore_network`` into a fresh model, three more steps on both, at keep_prob 1.0.  Weights and
    slots are float32 in the bundle and Adam's ``t`` comes back from ``beta2_power``, so a native step, which repeats itself bit for
    bit, continues bit for bit; the autograd cell gets what tests/test_trainer_modes_gpu.py documents for two runs of an
    ``anysize_autograd`` trainer with a conv stack (one float32 ulp of the loss: 1e-6)."""
    from catfish_amd import train_validate as tv
    case = {c.name: c for c in STEPPED_CELLS}[name]
    net = _build(case, keep_prob=1.0)
    fresh = None
    try:
        batches = [_batch(64, 100 + i) for i in range(6)]
        for step in range(3):
            net.train_network(*batches[step], step)
        net.save_network(str(tmp_path), 3)
        fresh = tv.build_model(case.network_type, train_seed=5, **dict(hyperparameters(case, 64), keep_prob=1.0))
        fresh.restore_network(str(tmp_path), "ckpnt-3")
        on, back = [], []
        for step in range(3, 6):
            net.train_network(*batches[step], step)
            fresh.train_network(*batches[step], step)
            on.append(net.train_loss)
            back.append(fresh.train_loss)
        print("uninterrupted", on, "restored", back)
        assert fresh._trainer.mode == net._trainer.mode == case.cell[0]
        assert float(fresh._trainer.opt.t) == float(net._trainer.opt.t) == 6.0 and np.isfinite(on).all() and len(set(on)) == 3
        if case.cell[0] == "anysize_autograd":
            assert np.abs(np.asarray(on) - np.asarray(back)).max() <= AUTOGRAD_TOL["anysize_autograd-128-64"]
        else:
            assert np.asarray(on, np.float32).view(np.uint32).tolist() == np.asarray(back, np.float32).view(np.uint32).tolist()
    finally:
        _close(*([net] if fresh is None else [net, fresh]))


# ------------------------------------------------------------------------------------------------ float64 on the card
def test_float64_on_the_card_trains_on_torch_and_matches_the_cpu():
    """64 / 32 (3, 2) with ``dtype=float64`` and ``native=None`` on the card: the ``torch`` row.  Loss, gradients and two steps
    against the CPU float64 trainer at 1e-9 relative -- derived, not measured: float64 summation noise over at most ~1e5 terms is
    ~1e-11, and nothing computed in float32 comes within five orders of that."""
    import torch
    from catfish_amd.training import AutogradStep, Trainer
    from oracle import catfish_oracle as oracle
    w = oracle.random_weights(seed=3)
    mk = lambda device: Trainer(w, 3, 2, "Adam", 1e-3, 1.0, device=device, dtype=torch.float64, seed=1)      # noqa: E731
    card, cpu = mk("cuda"), mk("cpu")
    assert card.mode == cpu.mode == "torch" and not card.native and not card.anysize and card.engine is None
    assert card.step_impl is None and type(card.step) is AutogradStep and card.net.dtype == torch.float64
    x, y = _batch(50, 50)
    (loss_a, grads_a), (loss_b, grads_b) = card.gradients(x, y, keep_prob=1.0), cpu.gradients(x, y, keep_prob=1.0)
    errs = {k: float(np.abs(grads_a[k] - grads_b[k]).max() / np.abs(grads_b[k]).max()) for k in grads_b}
    worst = max(errs, key=errs.get)
    print("float64 card against cpu: loss %.3g relative, worst gradient %s %.3g" % (abs(loss_a - loss_b) / abs(loss_b), worst, errs[worst]))
    assert sorted(grads_a) == sorted(grads_b) and len(grads_b) == 58 and all(g.dtype == np.float64 for g in grads_a.values())
    assert abs(loss_a - loss_b) <= 1e-9 * abs(loss_b) and errs[worst] <= 1e-9
    xs, ys = _batch(64, 64)
    a, b = [card.train_step(xs, ys) for _ in range(2)], [cpu.train_step(xs, ys) for _ in range(2)]
    print("losses on the card", a, "on the cpu", b)
    assert float(card.opt.t) == 2.0 and card._graph is not None and np.isfinite(a).all() and a[1] != a[0]
    assert np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-9 * max(b)


# ------------------------------------------------------------------------------------------------ the limit and the library
def test_tuned_max_blocks_is_the_librarys():
    from catfish_amd import _native as N
    from catfish_amd.train_mode import TUNED_MAX_BLOCKS
    lib = N.lib()
    assert TUNED_MAX_BLOCKS == 4
    assert int(lib.cf_res_train_param_floats(TUNED_MAX_BLOCKS)) > 0 and int(lib.cf_res_train_param_floats(TUNED_MAX_BLOCKS + 1)) == 0


def test_native_step_refuses_a_stack_deeper_than_the_tuned_kernels():
    """``NativeTrainStep`` at five blocks: a ValueError at construction that names the limit (the trainer never asks for one)."""
    from catfish_amd.engine import HipEngine
    from catfish_amd.native_step import NativeTrainStep
    from catfish_amd.training import TFOptimizer, TorchResNetRNN
    from oracle import catfish_oracle as oracle
    w = oracle.random_weights(seed=2, n_layers=1, n_layers_res=5)
    net = TorchResNetRNN(w, 1, 5, device="cuda")
    eng = HipEngine(w, n_layers=1, n_layers_res=5, device=0, max_windows_per_pass=256, fuse_layers=False)
    try:
        with pytest.raises(ValueError, match=r"1\.\.4 blocks, not 5"):
            NativeTrainStep(net, TFOptimizer(net.trainable(), "Adam", 1e-3), eng, 1.0, seed=1)
    finally:
        eng.close()
