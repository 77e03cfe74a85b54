"""``catfish_amd.train_mode``: the trainer's mode over the whole grid of its inputs, and the torch reference trainer on the CPU,
against what the commit before the module existed (e39d6a2) decided and computed.  No GPU, no native library."""
import hashlib
import itertools

import numpy as np
import pytest

from catfish_amd.train_mode import KINDS, STEP_KINDS, TrainMode, geometry
from oracle import catfish_oracle as oracle

X3 = "precision='bf16x3' is a mode of the any-size training recurrences; "
X3_SHIPPED = X3 + "the tuned training kernels of the shipped 64 / 32 geometry are fp32"
X3_CPU = X3 + "it runs on the HIP kernels: device='cpu' has none"
X3_REFERENCE = X3 + "native=False is the pure-torch reference"
X3_DTYPE = X3 + "the training kernels are float32 (dtype torch.float64)"
NATIVE_NEEDS = "native=True runs the fp32 HIP training kernels: it needs device='cuda' and dtype float32"
PER_LAYER = {"fuse_layers": False}
WIDE = {"layer_size": 128, "layer_size_res": 64}
WIDE_RNN = {"layer_size": 128, "layer_size_res": 32}           # no conv stack: c counts as 32

# (shipped, device type, float32, native, conv stack, precision) -> (kind, engine keywords, Trainer.native, Trainer.anysize) or the
# ValueError's text.  Produced by evaluating the mode expressions of Trainer.__init__ at commit e39d6a2 (training.py:317-348 there),
# transcribed into a script, over the grid -- not by the function under test.  Shipped rows are 64 / 32, the others 128 / 64.
GRID = {
    (True, 'cpu', True, None, True, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', True, None, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', True, None, False, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', True, None, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', True, True, True, 'fp32'): NATIVE_NEEDS,
    (True, 'cpu', True, True, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', True, True, False, 'fp32'): NATIVE_NEEDS,
    (True, 'cpu', True, True, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', True, False, True, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', True, False, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', True, False, False, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', True, False, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', False, None, True, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', False, None, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', False, None, False, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', False, None, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', False, True, True, 'fp32'): NATIVE_NEEDS,
    (True, 'cpu', False, True, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', False, True, False, 'fp32'): NATIVE_NEEDS,
    (True, 'cpu', False, True, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', False, False, True, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', False, False, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cpu', False, False, False, 'fp32'): ('torch', None, False, False),
    (True, 'cpu', False, False, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', True, None, True, 'fp32'): ('tuned_step', PER_LAYER, True, False),
    (True, 'cuda', True, None, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', True, None, False, 'fp32'): ('torch', None, False, False),
    (True, 'cuda', True, None, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', True, True, True, 'fp32'): ('tuned_step', PER_LAYER, True, False),
    (True, 'cuda', True, True, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', True, True, False, 'fp32'): ('tuned_autograd', PER_LAYER, True, False),
    (True, 'cuda', True, True, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', True, False, True, 'fp32'): ('torch', None, False, False),
    (True, 'cuda', True, False, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', True, False, False, 'fp32'): ('torch', None, False, False),
    (True, 'cuda', True, False, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', False, None, True, 'fp32'): ('tuned_autograd', PER_LAYER, True, False),
    (True, 'cuda', False, None, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', False, None, False, 'fp32'): ('torch', None, False, False),
    (True, 'cuda', False, None, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', False, True, True, 'fp32'): NATIVE_NEEDS,
    (True, 'cuda', False, True, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', False, True, False, 'fp32'): NATIVE_NEEDS,
    (True, 'cuda', False, True, False, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', False, False, True, 'fp32'): ('torch', None, False, False),
    (True, 'cuda', False, False, True, 'bf16x3'): X3_SHIPPED,
    (True, 'cuda', False, False, False, 'fp32'): ('torch', None, False, False),
    (True, 'cuda', False, False, False, 'bf16x3'): X3_SHIPPED,
    (False, 'cpu', True, None, True, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', True, None, True, 'bf16x3'): X3_CPU,
    (False, 'cpu', True, None, False, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', True, None, False, 'bf16x3'): X3_CPU,
    (False, 'cpu', True, True, True, 'fp32'): NATIVE_NEEDS,
    (False, 'cpu', True, True, True, 'bf16x3'): X3_CPU,
    (False, 'cpu', True, True, False, 'fp32'): NATIVE_NEEDS,
    (False, 'cpu', True, True, False, 'bf16x3'): X3_CPU,
    (False, 'cpu', True, False, True, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', True, False, True, 'bf16x3'): X3_CPU,
    (False, 'cpu', True, False, False, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', True, False, False, 'bf16x3'): X3_CPU,
    (False, 'cpu', False, None, True, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', False, None, True, 'bf16x3'): X3_CPU,
    (False, 'cpu', False, None, False, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', False, None, False, 'bf16x3'): X3_CPU,
    (False, 'cpu', False, True, True, 'fp32'): NATIVE_NEEDS,
    (False, 'cpu', False, True, True, 'bf16x3'): X3_CPU,
    (False, 'cpu', False, True, False, 'fp32'): NATIVE_NEEDS,
    (False, 'cpu', False, True, False, 'bf16x3'): X3_CPU,
    (False, 'cpu', False, False, True, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', False, False, True, 'bf16x3'): X3_CPU,
    (False, 'cpu', False, False, False, 'fp32'): ('torch', None, False, False),
    (False, 'cpu', False, False, False, 'bf16x3'): X3_CPU,
    (False, 'cuda', True, None, True, 'fp32'): ('anysize_autograd', WIDE, False, True),
    (False, 'cuda', True, None, True, 'bf16x3'): ('anysize_autograd', WIDE, False, True),
    (False, 'cuda', True, None, False, 'fp32'): ('anysize_autograd', WIDE_RNN, False, True),
    (False, 'cuda', True, None, False, 'bf16x3'): ('anysize_autograd', WIDE_RNN, False, True),
    (False, 'cuda', True, True, True, 'fp32'): ('anysize_step', WIDE, True, False),
    (False, 'cuda', True, True, True, 'bf16x3'): ('anysize_step', WIDE, True, False),
    (False, 'cuda', True, True, False, 'fp32'): ('anysize_step', WIDE_RNN, True, False),
    (False, 'cuda', True, True, False, 'bf16x3'): ('anysize_step', WIDE_RNN, True, False),
    (False, 'cuda', True, False, True, 'fp32'): ('torch', None, False, False),
    (False, 'cuda', True, False, True, 'bf16x3'): X3_REFERENCE,
    (False, 'cuda', True, False, False, 'fp32'): ('torch', None, False, False),
    (False, 'cuda', True, False, False, 'bf16x3'): X3_REFERENCE,
    (False, 'cuda', False, None, True, 'fp32'): ('torch', None, False, False),
    (False, 'cuda', False, None, True, 'bf16x3'): X3_DTYPE,
    (False, 'cuda', False, None, False, 'fp32'): ('torch', None, False, False),
    (False, 'cuda', False, None, False, 'bf16x3'): X3_DTYPE,
    (False, 'cuda', False, True, True, 'fp32'): NATIVE_NEEDS,
    (False, 'cuda', False, True, True, 'bf16x3'): X3_DTYPE,
    (False, 'cuda', False, True, False, 'fp32'): NATIVE_NEEDS,
    (False, 'cuda', False, True, False, 'bf16x3'): X3_DTYPE,
    (False, 'cuda', False, False, True, 'fp32'): ('torch', None, False, False),
    (False, 'cuda', False, False, True, 'bf16x3'): X3_REFERENCE,
    (False, 'cuda', False, False, False, 'fp32'): ('torch', None, False, False),
    (False, 'cuda', False, False, False, 'bf16x3'): X3_REFERENCE,
}


def _mode(row):
    shipped, dev, f32, native, conv, precision = row
    h, c = (64, 32) if shipped else (128, 64 if conv else 32)
    return TrainMode.of(h, c, 1 if conv else 0, dev, f32, native, precision, dtype_name="torch.float32" if f32 else "torch.float64")


def test_the_whole_grid_is_what_the_constructor_decided():
    grid = list(itertools.product((True, False), ("cpu", "cuda"), (True, False), (None, True, False), (True, False), ("fp32", "bf16x3")))
    assert len(grid) == 96 and sorted(map(repr, grid)) == sorted(map(repr, GRID))
    for row in grid:
        want = GRID[row]
        if isinstance(want, str):
            with pytest.raises(ValueError) as e:
                _mode(row)
            assert str(e.value) == want, row
        else:
            m = _mode(row)
            assert tuple(m) == want and (m.kind, m.engine_kwargs, m.native, m.anysize) == want, row
            assert type(m.native) is bool and type(m.anysize) is bool
            with pytest.raises(AttributeError):
                m.kind = "torch"


def test_the_five_kinds_partition_the_rows_that_do_not_raise():
    rows = {row: _mode(row) for row, want in GRID.items() if not isinstance(want, str)}
    assert len(rows) == 40
    by_kind = {k: [r for r, m in rows.items() if m.kind == k] for k in KINDS}
    assert sum(len(v) for v in by_kind.values()) == len(rows) and all(by_kind[k] for k in KINDS)
    assert STEP_KINDS == ("tuned_step", "anysize_step")
    for row, m in rows.items():
        assert (m.engine_kwargs is None) == (m.kind == "torch")
        assert m.anysize == (m.kind == "anysize_autograd")
        if m.kind != "torch":
            assert m.engine_kwargs == (PER_LAYER if m.kind.startswith("tuned") else WIDE if row[4] else WIDE_RNN)
    # the two combinations no test trains through land where they always did: an engine with per-layer launches and no step
    odd = [(True, "cuda", True, True, False, "fp32"), (True, "cuda", False, None, True, "fp32")]
    assert sorted(by_kind["tuned_autograd"]) == sorted(odd)
    for row in odd:
        assert tuple(rows[row]) == ("tuned_autograd", PER_LAYER, True, False)


def test_geometry_with_and_without_a_conv_stack():
    assert geometry(oracle.random_weights(seed=1), 2) == (64, 32, True)
    assert geometry(oracle.random_weights(seed=1, layer_size=128, layer_size_res=64, n_layers=2, n_layers_res=1), 1) == (128, 64, False)
    assert geometry(oracle.random_weights(seed=1, layer_size=64, layer_size_res=16, n_layers=1, n_layers_res=1), 1) == (64, 16, False)
    # no conv stack: c counts as 32, so a 64-unit RNN is at the shipped geometry and a 32-unit one is not
    assert geometry(oracle.random_weights(seed=1, layer_size=64, n_layers=2, n_layers_res=0), 0) == (64, 32, True)
    assert geometry(oracle.random_weights(seed=1, layer_size=32, n_layers=2, n_layers_res=0), 0) == (32, 32, False)
    assert geometry({k: v.tolist() for k, v in oracle.random_weights(seed=1, layer_size=16, layer_size_res=48, n_layers_res=1).items()}, 1) == (16, 48, False)
    torch = pytest.importorskip("torch")
    w = {k: torch.as_tensor(v) for k, v in oracle.random_weights(seed=1, layer_size=48, layer_size_res=32, n_layers_res=1).items()}
    assert geometry(w, 1) == (48, 32, False)


# ---------------------------------------------------------------------------------------------------- the CPU reference trainer
def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def cpu_run(dtype_name):
    """Six seeded steps with dropout on a 16 / 16 one-layer model at batch 8, then ``gradients`` of a seventh batch:
    (digest of the losses, of the final variables and optimizer slots, of the gradients call)."""
    import torch
    from catfish_amd.training import Trainer
    w = oracle.random_weights(seed=3, layer_size=16, n_layers=1, layer_size_res=16, n_layers_res=1)
    tr = Trainer(w, 1, 1, "Adam", 1e-3, 0.8, device="cpu", seed=11, dtype=getattr(torch, dtype_name))
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1.2, size=(7, 8, 35)).astype(np.float32)
    y = (rng.random((7, 8, 35)) < 0.3).astype(np.float32)
    losses = np.array([tr.train_step(x[i], y[i]) for i in range(6)], dtype=np.float64)
    assert tr.last_loss == losses[-1] and tr.step_impl is None and tr.engine is None and not tr.native and not tr.anysize
    state = [d[k].detach().numpy().copy() for d in (tr.net.params, tr.opt.m, tr.opt.v) for k in sorted(d)]      # in the run's own dtype
    assert float(tr.opt.t) == 6.0
    loss, grads = tr.gradients(x[6], y[6])
    return (_digest(losses), _digest(*state),
            _digest(np.float64(loss), *(grads[k] for k in sorted(grads))))


# taken on commit e39d6a2 with this file's cpu_run
CPU_DIGESTS = {
    "float32": ("e60af3716b06f7e4e80bc0469c4aa05e41b03b8869aa724596fdbc3936aaab0f",
                "da20358b1b7db9ffe5a75f42b4053cf3babbc9af91ac3c42064fe938c0b56fb0",
                "b00a28b4d851abea4b5768fc1409c8e0f523d5fd34bc72ad0aa22822816bb842"),
    "float64": ("a5395465fcbedfffeded8445b3c7ec30c4e9d1e65f597526ae6c57195233cd6c",
                "7aaee2012763f68a5f46fc96420fb2c909a44e1b624ba86806e9757ba462e129",
                "78eb3e2340604be88ed0f7aa41307c29c97c05224c9ca2a2d6baa3f2d84a9051"),
}


@pytest.mark.parametrize("dtype_name", sorted(CPU_DIGESTS))
def test_cpu_trainer_computes_what_it_computed(dtype_name):
    pytest.importorskip("torch")
    got = cpu_run(dtype_name)
    print(dtype_name, got)
    assert got == CPU_DIGESTS[dtype_name]
