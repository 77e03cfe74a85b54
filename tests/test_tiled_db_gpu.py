"""The tiled training set on a GPU: the training kernels on a batch whose windows hold borders against float64, and the host-fed
loops (``Trainer.train_steps``, ``train_and_validate``) on a ``DeviceTiledDb``.

Bounds of the float64 comparison.  The rule of tests/test_train_draws_fp64.py: ``Trainer.gradients(x, y, keep_prob=1.0)`` at 50
windows (a ragged fourth tile) against ``TorchResNetRNN(dtype=float64)`` on the same batch -- the loss by absolute error, every
trainable tensor by ``max|d| / max|ref|``.  A measuring run (CATFISH_PARITY_LOG names a file) records for both trainers and both
quantities the kernels' error and the error of the float32 pure-torch ``Trainer(native=False)`` on the same batch; the asserted
bound of a quantity is 4 x the largest such yardstick, rounded down to three digits, and never looser than the older bounds (loss
5e-6 absolute, gradients 2e-3).  4 x is the project's margin for two implementations with different summation orders.  The rows are
in profiles/tiled_db_parity.jsonl; ``BOUNDS`` holds the constants and tests/test_tiled_db_host.py checks them against that file.
The labels of this batch are what is new: windows with a border after sample 0 and after sample 33, an isolated 1, an isolated 0,
all ones and all zeros, where every earlier battery repeats one label over a window.
"""
import json
import os

import numpy as np
import pytest

from catfish_amd import device_db as ddb, train_validate as tv
from catfish_amd.device_db import WINDOW

pytestmark = pytest.mark.gpu

# quantity -> asserted bound = min(4 x largest float32-torch error in profiles/tiled_db_parity.jsonl, older bound).  The largest
# yardsticks there (MI355X, 256 CUs) and the kernels' largest error next to them:
#   loss 5.653e-08 (kernels 5.56e-08, the tuned step; 3.1e-09 any-size)      grads 2.787e-06 (kernels 2.14e-06 tuned, 1.10e-06 any-size)
# 4 x each, rounded down, is below the older bound of its quantity, so it is the bound.  Both head kernels meet the rule on windows
# that hold a border; the any-size step's worst gradient (the first layer's backward gates bias) is 3.5 x its own case's yardstick
# and 0.10 x the bound.
BOUNDS = {"loss": 2.26e-7, "grads": 1.11e-5}
OLDER_BOUNDS = {"loss": 5e-6, "grads": 2e-3}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tiled_db_parity.jsonl")
TRAINERS = [("shipped", None), ((32, 16, 1, 1), True)]
TRAINER_IDS = ["tuned-64-32", "anysize-32-16"]


def bounds_from_profile(path=PROFILE):
    """{quantity: min(4 x largest float32-torch error in the profile, older bound)}: what ``BOUNDS`` may not exceed."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            worst[row["quantity"]] = max(worst.get(row["quantity"], 0.0), row["torch_fp32"])
    return {k: min(4.0 * v, OLDER_BOUNDS[k]) for k, v in worst.items()}


# ---------------------------------------------------------------------------------------------------- the trainer
def _weights(geo, ckpt_weights):
    from oracle import catfish_oracle as oracle
    if geo == "shipped":
        return ckpt_weights, 3, 2
    h, c, n_layers, n_blocks = geo
    return oracle.random_weights(seed=21, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks), n_layers, n_blocks


def _trainer(geo, ckpt_weights, native, kp, **kw):
    from catfish_amd.training import Trainer
    w, n_layers, n_blocks = _weights(geo, ckpt_weights)
    return Trainer(w, n_layers, n_blocks, "RMSProp" if geo == "shipped" else "Adam", 1e-3, kp, seed=5, native=native, **kw)


def _close(*trainers):
    for tr in trainers:
        if tr.engine is not None:
            tr.engine.close()


def _db():
    return ddb.synthetic_device_tiled_db(n_reads=2, read_len=12000, seed=2, miss_per_read="hits")


# ---------------------------------------------------------------------------------------------------- mixed labels against float64
def _mixed_batch(n=50, seed=50):
    """``n`` windows of noise whose labels cycle through: a border after sample 0 (both ways round), a border after sample 33 (both
    ways round), one isolated 1, one isolated 0, all ones, all zeros."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1.2, size=(n, WINDOW)).astype(np.float32)
    y = np.zeros((n, WINDOW), np.float32)
    for i in range(n):
        kind = i % 8
        if kind == 0:
            y[i, 1:] = 1.0
        elif kind == 1:
            y[i, 0] = 1.0
        elif kind == 2:
            y[i, :34] = 1.0
        elif kind == 3:
            y[i, 34] = 1.0
        elif kind == 4:
            y[i, int(rng.integers(1, 34))] = 1.0
        elif kind == 5:
            y[i] = 1.0
            y[i, int(rng.integers(1, 34))] = 0.0
        elif kind == 6:
            y[i] = 1.0
    return x, y


def _grad_errors(grads, ref_grads):
    import torch
    assert sorted(grads) == sorted(ref_grads)
    errs = {}
    for k, g in ref_grads.items():
        ref = g.double()
        errs[k] = float((torch.as_tensor(np.asarray(grads[k])).double() - ref).abs().max() / ref.abs().max())
    worst = max(errs, key=errs.get)
    return errs[worst], worst


def _stamp():
    import subprocess
    import torch
    commit = os.environ.get("CATFISH_PARITY_COMMIT")
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", os.path.dirname(PROFILE), "rev-parse", "--short=12", "HEAD"],
                                             stderr=subprocess.DEVNULL).decode().strip()
        except (OSError, subprocess.CalledProcessError):
            commit = None
    prop = torch.cuda.get_device_properties(0)
    return {"commit": commit, "device": "%s, %d CUs" % (prop.name, prop.multi_processor_count)}


@pytest.mark.parametrize("geo,native", TRAINERS, ids=TRAINER_IDS)
def test_mixed_labels_match_float64(geo, native, ckpt_weights):
    import torch
    from catfish_amd.training import TorchResNetRNN, Trainer
    case = TRAINER_IDS[TRAINERS.index((geo, native))]
    w, n_layers, n_blocks = _weights(geo, ckpt_weights)
    x, y = _mixed_batch()
    assert {int(v) for v in y.sum(1)} == {0, 1, 34, 35} and y[0, 0] == 0 and y[0, 1] == 1 and y[2, 33] == 1 and y[2, 34] == 0
    tr = _trainer(geo, ckpt_weights, native, 1.0)
    try:
        assert tr.mode == ("tuned_step" if geo == "shipped" else "anysize_step")
        loss_k, grads_k = tr.gradients(x, y, keep_prob=1.0)
        net64 = TorchResNetRNN(w, n_layers, n_blocks, device="cuda", dtype=torch.float64)
        loss64 = net64.loss(x, y)
        loss64.backward()
        ref_loss, ref_grads = float(loss64.detach()), {k: p.grad.detach().cpu() for k, p in net64.trainable().items()}
        assert all(float(g.abs().max()) > 0.0 for g in ref_grads.values())
        e_loss = abs(loss_k - ref_loss)
        e_grads, worst = _grad_errors(grads_k, ref_grads)
        t_loss = t_grads = t_worst = None
        log = os.environ.get("CATFISH_PARITY_LOG")
        if log:                                            # the yardstick: the float32 pure-torch trainer on the same batch
            yard = Trainer(w, n_layers, n_blocks, "Adam", 1e-3, 1.0, device="cuda", native=False, use_graph=False)
            loss_t, grads_t = yard.gradients(x, y, keep_prob=1.0)
            assert yard.mode == "torch"
            t_loss = abs(loss_t - ref_loss)
            t_grads, t_worst = _grad_errors(grads_t, ref_grads)
        for quantity, kernel, yardstick, where in (("loss", e_loss, t_loss, None), ("grads", e_grads, t_grads, worst)):
            row = {"case": case, "quantity": quantity, "kernel": float(kernel), "torch_fp32": yardstick, "worst": where,
                   "torch_fp32_worst": t_worst if quantity == "grads" else None}
            print("parity %s" % json.dumps(row))
            if log:
                with open(log, "a") as fh:
                    fh.write(json.dumps(dict(_stamp(), **row)) + "\n")
        bad = {q: (e, BOUNDS[q]) for q, e in (("loss", e_loss), ("grads", e_grads)) if not e <= BOUNDS[q]}
        assert not bad, (case, bad, worst)
    finally:
        _close(tr)


# ---------------------------------------------------------------------------------------------------- the host-fed loops
@pytest.mark.parametrize("geo,native", TRAINERS, ids=TRAINER_IDS)
def test_train_steps_feeds_the_true_labels_from_the_host(geo, native, ckpt_weights):
    """A ``DeviceTiledDb`` has no card side: ``train_steps(db, 6, 32)`` at keep_prob 0.8 takes ``get_training_set`` + ``train_step``
    per step, and its losses are bit-equal to ``train_step`` on the twin's six gathered batches, per-sample labels included."""
    pytest.importorskip("torch")
    twin = _db()
    batches = [twin.gather(d, 32) for d in range(6)]
    assert any(0 < row.sum() < WINDOW for _, y in batches for row in y)            # windows with a border inside are among them
    host = _trainer(geo, ckpt_weights, native, 0.8)
    want = np.array([host.train_step(x, y.astype(np.float32)) for x, y in batches], dtype=np.float32)
    fed = _trainer(geo, ckpt_weights, native, 0.8)
    db = _db()
    got = fed.train_steps(db, 6, 32)
    print("losses train_step", want, "train_steps", got)
    assert fed.mode == host.mode == ("tuned_step" if geo == "shipped" else "anysize_step") and fed._fed is None and db._dev is None
    assert got.dtype == np.float32 and np.isfinite(got).all() and len(set(got.tolist())) == 6 and db.draw == 6
    assert np.array_equal(got, want)
    lx, ly = db.last_batch()
    assert np.array_equal(lx, batches[-1][0]) and np.array_equal(ly, batches[-1][1])
    _close(fed, host)


def test_train_save_load_infer_loop_tiled(hp, tmp_path, monkeypatch):
    """tests/test_gpu_pipeline.py::test_train_save_load_infer_loop's scenario (20 steps of 64, checkpoint, validation, load_network)
    on a DeviceTiledDb: the report's share of positive labels is the batches' own, no longer one half."""
    pytest.importorskip("torch")
    from catfish_amd import neural_network
    val_dir = tmp_path / "val"
    val_dir.mkdir()
    squiggles = []
    for i in range(3):
        raw, lab = tv.synthetic_labelled_read(3000 + 35 * i, seed=50 + i)
        np.savez(val_dir / ("sq%d.npz" % i), raw=raw, base_labels=lab)
        squiggles.append(str(val_dir / ("sq%d.npz" % i)))
    monkeypatch.chdir(tmp_path)
    net = tv.build_model("ResNetRNN", save=True, **dict(hp, batch_size=64, train_seed=0))
    net.initialize_network(seed=4)
    db, twin = _db(), _db()
    acc = tv.train_and_validate(net, db, 20 * 64, squiggles, 2000, net.model_path, 0, 856)
    assert 0.0 <= acc <= 1.0 and np.isfinite(net.train_loss) and db.draw == 20
    report = open(net.model_path + ".txt").read()
    assert "Training on 1280 examples in 20 batches" in report and "Saved checkpoint at step 20" in report
    share = sum(int(twin.gather(d, 64)[1].sum()) for d in range(20)) / (WINDOW * 1280)
    assert 0.0 < share < 0.5 and "Training set had {:.2%} HPs".format(share) in report
    assert "---NEXT ROUND OF VALIDATION---" in open(os.path.basename(net.model_path) + ".txt").read()
    loaded = neural_network.load_network("ResNetRNN", net.model_path, checkpoint=20)
    x = np.random.default_rng(0).normal(0, 1.2, size=(40, 35, 1))
    assert np.array_equal(loaded.infer(x), net.infer(x))
    loaded.engine.close(); net.engine.close()
