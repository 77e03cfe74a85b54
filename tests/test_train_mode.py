"""``catfish_amd.train_mode``: the trainer's mode over the whole grid of its inputs, and the torch reference trainer on the CPU,
against what the commit before the module existed (e39d6a2) decided and computed.  No GPU, no native library."""
import hashlib
import itertools

import numpy as np
import pytest

from catfish_amd.train_mode import KINDS, STEP_KINDS, TUNED_MAX_BLOCKS, TrainMode, geometry, tuned_geometry
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
SHIPPED_SIZES = {"layer_size": 64, "layer_size_res": 32}       # 64 / 32 where the any-size kernels train it

# (shipped, device type, float32, native, conv stack, precision) -> (kind, engine keywords, Trainer.native, Trainer.anysize) or the
# ValueError's text.  Produced by evaluating the mode expressions of Trainer.__init__ at commit e39d6a2 (training.py:317-348 there),
# transcribed into a script, over the grid -- not by the function under test.  Shipped rows are 64 / 32, the others 128 / 64.
# That constructor knew a conv stack only as present or absent, and its two ``tuned_autograd`` rows could not take a step
# (tests/test_train_draws_fp64.py); ``GRID`` below adds the depth class and says where they went.
RECORDED = {
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


DEPTHS = {0: (0,), 1: (1, TUNED_MAX_BLOCKS), 5: (TUNED_MAX_BLOCKS + 1, 12)}      # depth class -> the depths a row is evaluated at

# The three recorded decisions that changed, by their row with the depth class.  The 64-unit RNN with native=True and 64 / 32 in
# float64 were ``tuned_autograd``; the first is now the any-size step (and takes bf16x3, as every row of that kind), the second
# trains on torch as every other float64 model on the card.
MOVED = {
    (True, "cuda", True, True, 0, "fp32"): ("anysize_step", SHIPPED_SIZES, True, False),
    (True, "cuda", True, True, 0, "bf16x3"): ("anysize_step", SHIPPED_SIZES, True, False),
    (True, "cuda", False, None, 1, "fp32"): ("torch", None, False, False),
}


def _with_depth_class():
    """(shipped, device type, float32, native, depth class 0 | 1 | 5, precision) -> decision.  Class 0 (no conv stack) and class 1
    (1 .. 4 blocks) are the recorded rows without and with a conv stack.  Class 5 (deeper than the tuned kernels go) is at every
    size what the recorded constructor decided for a conv stack at 128 / 64, with the row's own sizes as engine keywords."""
    grid = {}
    for (shipped, dev, f32, native, conv, precision), want in RECORDED.items():
        grid[(shipped, dev, f32, native, 1 if conv else 0, precision)] = want
        if conv and not shipped:
            grid[(False, dev, f32, native, 5, precision)] = want
            deep = want if isinstance(want, str) or want[1] is None else (want[0], SHIPPED_SIZES) + want[2:]
            grid[(True, dev, f32, native, 5, precision)] = deep
    assert set(MOVED) <= set(grid) and all("tuned_autograd" in grid[row] or grid[row] == X3_SHIPPED for row in MOVED)
    grid.update(MOVED)
    return grid


GRID = _with_depth_class()


def _modes(row):
    """The row's decision at every depth of its class (one TrainMode, or one ValueError's text, per depth)."""
    shipped, dev, f32, native, depth_class, precision = row
    h, c = (64, 32) if shipped else (128, 64 if depth_class else 32)
    out = []
    for depth in DEPTHS[depth_class]:
        try:
            out.append(TrainMode.of(h, c, depth, dev, f32, native, precision, dtype_name="torch.float32" if f32 else "torch.float64"))
        except ValueError as e:
            out.append(str(e))
    return out


def _mode(row):
    """The one decision of the row's depth class, or None if its depths disagree."""
    modes = _modes(row)
    return modes[0] if all(m == modes[0] for m in modes) else None


def test_the_whole_grid_is_what_the_constructor_decided():
    grid = list(itertools.product((True, False), ("cpu", "cuda"), (True, False), (None, True, False), (0, 1, 5), ("fp32", "bf16x3")))
    assert len(grid) == 144 and sorted(map(repr, grid)) == sorted(map(repr, GRID))
    assert len(RECORDED) == 96 and sum("tuned_autograd" in v for v in RECORDED.values()) == 2
    for row in grid:
        want = GRID[row]
        for m in _modes(row):                                  # both ends of the depth class decide alike
            if isinstance(want, str):
                assert m == want, row
            else:
                assert not isinstance(m, str), (row, m)
                assert tuple(m) == want and (m.kind, m.engine_kwargs, m.native, m.anysize) == want, row
                assert type(m.native) is bool and type(m.anysize) is bool
                with pytest.raises(AttributeError):
                    m.kind = "torch"
    # every recorded decision stands, apart from the three that moved
    for (shipped, dev, f32, native, conv, precision), want in RECORDED.items():
        row = (shipped, dev, f32, native, 1 if conv else 0, precision)
        assert GRID[row] == want or row in MOVED, row


def test_the_four_kinds_partition_the_rows_that_do_not_raise():
    rows = {row: _mode(row) for row, want in GRID.items() if not isinstance(want, str)}
    assert len(rows) == 63 and None not in rows.values()          # 40 recorded, 11 more in each deep class, one refusal lifted
    by_kind = {k: [r for r, m in rows.items() if m.kind == k] for k in KINDS}
    assert sum(len(v) for v in by_kind.values()) == len(rows) and all(by_kind[k] for k in KINDS)
    assert KINDS == ("tuned_step", "anysize_step", "anysize_autograd", "torch") and STEP_KINDS == ("tuned_step", "anysize_step")
    for row, m in rows.items():
        assert (m.engine_kwargs is None) == (m.kind == "torch")
        assert m.anysize == (m.kind == "anysize_autograd")
        assert m.native == (m.kind in STEP_KINDS)
        if m.kind != "torch":
            assert m.engine_kwargs == (PER_LAYER if m.kind == "tuned_step" else SHIPPED_SIZES if row[0] else WIDE if row[4] else WIDE_RNN)
    # the tuned step is 64 / 32 on the card in float32 with 1 .. 4 blocks and nothing else; no input reaches ``tuned_autograd``
    assert set(by_kind["tuned_step"]) == {(True, "cuda", True, None, 1, "fp32"), (True, "cuda", True, True, 1, "fp32")}
    assert not any("tuned_autograd" in repr(v) for v in GRID.values())
    # 64 / 32 where the tuned kernels do not go: five blocks as any other size, the RNN type only when native=True asks
    assert rows[(True, "cuda", True, None, 5, "fp32")].kind == "anysize_autograd" and rows[(True, "cuda", True, True, 5, "fp32")].kind == "anysize_step"
    assert rows[(True, "cuda", True, None, 0, "fp32")].kind == "torch" and rows[(True, "cuda", True, True, 0, "fp32")].kind == "anysize_step"
    assert GRID[(True, "cuda", True, None, 1, "bf16x3")] == GRID[(True, "cuda", True, True, 1, "bf16x3")] == X3_SHIPPED


def test_tuned_geometry_is_64_32_with_one_to_four_blocks():
    assert TUNED_MAX_BLOCKS == 4
    assert [d for d in range(0, 14) if tuned_geometry(64, 32, d)] == [1, 2, 3, 4]
    assert not any(tuned_geometry(h, c, d) for h, c in ((64, 16), (32, 32), (128, 32), (64, 64)) for d in range(0, 6))


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
