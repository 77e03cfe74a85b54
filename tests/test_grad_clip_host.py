"""Global-norm gradient clipping and the non-finite-step guard, on the host: the second header's table, and
``Trainer(device="cpu", dtype=float64, clip_norm=c)`` against a numpy float64 restatement of the definition

    S = sum double(g_i)^2,  g = sqrt(S),  s32 = float32(c / max(g, c)),  the optimizer consumes g_i * s32,
    a step whose S or loss is not finite changes nothing (``skip_nonfinite``), the step counter included.
"""
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from catfish_amd import _native as N
from catfish_amd.training import Trainer
from oracle import catfish_oracle as oracle

EXT = ("cf_ext_abi_version", "cf_clip_workspace_doubles", "cf_clip_norm", "cf_opt_step_guarded")
U64 = 2.0 ** -53          # one float64 rounding, relative


def test_second_header_is_read_by_the_same_parser_and_the_core_table_stays():
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "catfish_hip_ext.h")) as fh:
        symbols, constants, structs = N.parse_header(fh.read())
    assert sorted(symbols) == sorted(EXT) and symbols == N.EXT_SYMBOLS and structs == {}
    assert constants["CF_EXT_ABI_VERSION"] == 1 == N.CF_EXT_ABI_VERSION
    assert symbols["cf_ext_abi_version"] == (C.c_int, [])
    assert symbols["cf_clip_workspace_doubles"] == (C.c_int64, [C.c_int64])
    assert symbols["cf_clip_norm"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.c_void_p, C.c_void_p])
    # cf_opt_step's arguments plus the record pointer, in front of the stream
    core = N.SYMBOLS["cf_opt_step"]
    assert symbols["cf_opt_step_guarded"] == (core[0], core[1][:-1] + [C.c_void_p] + core[1][-1:])
    assert len(N.SYMBOLS) == 103 and not set(N.SYMBOLS) & set(N.EXT_SYMBOLS) and N.CF_ABI_VERSION == 9


def test_the_library_source_includes_the_second_header_and_the_build_depends_on_it(monkeypatch):
    from catfish_amd import build
    with open(build.SRC) as fh:
        assert '#include "../../include/catfish_hip_ext.h"' in fh.read()
    assert os.path.samefile(N.EXT_HEADER, os.path.join(os.path.dirname(N.HEADER), "catfish_hip_ext.h"))
    real = os.path.getmtime                                # a second header newer than the library asks for a rebuild
    monkeypatch.setattr(os.path, "exists", lambda path: True)
    monkeypatch.setattr(os.path, "getmtime", lambda path: 2.0 if path == N.EXT_HEADER else 1.0)
    assert build.needs_build()
    monkeypatch.setattr(os.path, "getmtime", lambda path: 1.0)
    assert not build.needs_build()
    monkeypatch.setattr(os.path, "getmtime", real)


# ------------------------------------------------------------------------------------------------ the definition, in numpy
def _model():
    w = oracle.random_weights(seed=5, n_layers=1, n_layers_res=1)
    rng = np.random.default_rng(3)
    return w, rng.normal(size=(4, 35)), (rng.random((4, 35)) < 0.3).astype(np.float64)


def _trainer(w, choice, **kw):
    return Trainer(w, 1, 1, choice, 1e-2, keep_prob=1.0, device="cpu", dtype=torch.float64, seed=0, **kw)


def _state(tr):
    first, second = (tr.opt.m, tr.opt.v) if tr.opt.choice == "Adam" else (tr.opt.ms, tr.opt.mom)
    return ({k: v.detach().numpy().copy() for k, v in tr.opt.params.items()}, {k: v.numpy().copy() for k, v in first.items()},
            {k: v.numpy().copy() for k, v in second.items()})


def _norm(grads):
    return math.sqrt(math.fsum(float(v) ** 2 for a in grads.values() for v in a.ravel()))


def _restated_step(choice, p, g, s1, s2, lr, t, c):
    """One clipped step of one variable in numpy float64 -> (p, slot1, slot2); ``t`` steps were taken before; ``g``: the norm."""
    from test_train_kernels_fp64 import opt_step_float64
    s32 = float(np.float32(c / max(g[1], c)))
    new_p, a, b, _ = opt_step_float64(0 if choice == "RMSProp" else 1, p, g[0] * s32, s1, s2, lr, t)
    return new_p, a, b


def _close(got, want, scale):
    """|got - want| <= 16 roundings of float64 relative to ``scale`` (the update for a variable, the slot for a slot: each passes
    fewer than 16 float64 operations in either evaluation) plus one spacing of the result."""
    return np.all(np.abs(got - want) <= 32 * U64 * np.abs(scale) + np.spacing(np.abs(want)))


@pytest.mark.parametrize("choice", ["Adam", "RMSProp"])
def test_clipped_steps_follow_the_definition(choice):
    w, x, y = _model()
    probe = _trainer(w, choice)
    _, grads = probe.gradients(x, y)
    norm = _norm(grads)
    n = sum(a.size for a in grads.values())
    plain = _trainer(w, choice)
    plain.train_step(x, y)
    for factor, clipped in ((0.5, 1), (2.0, 0)):
        c = factor * norm
        tr = _trainer(w, choice, clip_norm=c)
        assert tr.clip_norm == c and tr.skip_nonfinite is True
        p0, a0, b0 = _state(tr)
        tr.train_step(x, y)
        stats = tr.step_stats()
        s32 = float(np.float32(c / max(norm, c)))
        assert abs(stats["grad_norm"] - norm) <= n * U64 * norm
        assert stats["scale"] == s32 and (s32 < 1.0) == bool(clipped) and (factor < 1 or s32 == 1.0)
        assert stats["clipped"] == clipped and stats["skipped"] == 0 and float(tr.opt.t) == 1.0
        p1, a1, b1 = _state(tr)
        for k in grads:
            want_p, want_a, want_b = _restated_step(choice, p0[k], (grads[k], norm), a0[k], b0[k], 1e-2, 0, c)
            assert _close(p1[k], want_p, want_p - p0[k]) and _close(a1[k], want_a, want_a) and _close(b1[k], want_b, want_b), k
        same = all(np.array_equal(u[k], v[k]) for u, v in zip(_state(plain), (p1, a1, b1)) for k in grads)
        assert same == (factor == 2.0)                     # s32 == 1: bit for bit the step without the option


@pytest.mark.parametrize("choice", ["Adam", "RMSProp"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_gradient_skips_the_step_and_the_next_clean_one_proceeds(choice, bad):
    w, x, y = _model()
    tr = _trainer(w, choice, clip_norm=1.0)
    tr.train_step(x, y)                                    # slots and counter away from their initial values
    loss, grads = tr.gradients(x, y)
    before = _state(tr)

    def plant(poison):
        for k, p in tr.opt.params.items():
            p.grad = torch.from_numpy(grads[k].copy())
        if poison:
            next(iter(tr.opt.params.values())).grad.view(-1)[1] = bad
        tr.opt.step(torch.tensor(loss, dtype=torch.float64))

    plant(True)
    stats = tr.step_stats()
    assert stats["skipped"] == 1 and stats["scale"] == N.CF_CLIP_SKIPPED and not math.isfinite(stats["grad_norm"])
    assert float(tr.opt.t) == 1.0
    assert all(np.array_equal(u[k], v[k]) for u, v in zip(before, _state(tr)) for k in grads)
    plant(False)
    stats = tr.step_stats()
    assert stats["skipped"] == 1 and 0.0 < stats["scale"] <= 1.0 and float(tr.opt.t) == 2.0
    after = _state(tr)
    assert all(np.isfinite(after[0][k]).all() and not np.array_equal(after[0][k], before[0][k]) for k in grads)


def test_a_non_finite_loss_skips_too_and_the_guard_works_without_clipping():
    w, x, y = _model()
    tr = _trainer(w, "Adam", skip_nonfinite=True)
    assert tr.clip_norm is None and tr.skip_nonfinite is True
    _, grads = tr.gradients(x, y)
    before = _state(tr)
    for k, p in tr.opt.params.items():
        p.grad = torch.from_numpy(grads[k].copy())
    tr.opt.step(torch.tensor(float("nan"), dtype=torch.float64))
    assert tr.step_stats()["skipped"] == 1 and float(tr.opt.t) == 0.0
    assert all(np.array_equal(u[k], v[k]) for u, v in zip(before, _state(tr)) for k in grads)
    plain = _trainer(w, "Adam")
    plain.train_step(x, y)
    tr.train_step(x, y)                                    # skip_nonfinite alone: s32 = 1, the step of a trainer without options
    assert tr.step_stats() == {"grad_norm": pytest.approx(_norm(grads), rel=1e-12), "scale": 1.0, "clipped": 0, "skipped": 1}
    assert all(np.array_equal(u[k], v[k]) for u, v in zip(_state(plain), _state(tr)) for k in grads)


def test_options_off_by_default_and_bad_clip_norms_are_refused():
    w, _, _ = _model()
    tr = _trainer(w, "Adam")
    assert tr.clip_norm is None and tr.skip_nonfinite is False and not tr.opt.guarded
    assert tr.step_stats() == {"grad_norm": 0.0, "scale": 0.0, "clipped": 0, "skipped": 0}
    assert _trainer(w, "Adam", clip_norm=2, skip_nonfinite=False).skip_nonfinite is False
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), float("-inf"), "1.0", True):
        with pytest.raises(ValueError):
            _trainer(w, "Adam", clip_norm=bad)


def test_model_classes_and_the_environment_pass_the_option_on(monkeypatch):
    from catfish_amd import train_validate
    from catfish_amd.rnn_class import RNN
    net = RNN(batch_size=8, optimizer_choice="Adam", learning_rate=1e-3, layer_size=16, n_layers=1, keep_prob=1.0, clip_norm=0.5)
    assert net.clip_norm == 0.5 and net.skip_nonfinite is None and net.step_stats() is None
    seen = {}

    class Stop(Exception):
        pass

    def build_model(kind, **kwargs):
        seen.update(kwargs)
        raise Stop()

    monkeypatch.setattr(train_validate, "build_model", build_model)
    monkeypatch.setenv("CATFISH_CLIP_NORM", "0.25")
    with pytest.raises(Stop):
        train_validate.main(["prog", "ResNetRNN", "train", "100", "val", "1000"])
    assert seen["clip_norm"] == 0.25


def test_a_device_fed_draw_ends_after_a_chunk_of_skipped_steps(tmp_path):
    """``train_validate._train_device_fed``: steps go out one read-back chunk at a time; a chunk in which every step was skipped
    ends the draw with a line in the report, a chunk with one step taken does not; without the options it is one call."""
    from catfish_amd import train_validate

    class Net(object):
        clip_norm, skip_nonfinite = 1.0, None

        def __init__(self, skipped_per_chunk):
            self.plan, self.calls, self.skipped = list(skipped_per_chunk), [], 0

        def _require_trainer(self):
            return type("T", (), {"loss_log_capacity": 4})()

        def step_stats(self):
            return {"grad_norm": 1.0, "scale": 1.0, "clipped": 0, "skipped": self.skipped}

        def train_network_steps(self, db, k):
            self.calls.append(k)
            self.skipped += self.plan.pop(0)

    report = str(tmp_path / "report.txt")
    net = Net([0, 3, 4, 0])
    assert train_validate._train_device_fed(net, None, 14, 100, report) == (12, False) and net.calls == [4, 4, 4]
    with open(report) as fh:
        assert "Draw ended at step 112: all 4 steps of the last chunk were skipped" in fh.read()
    net = Net([0, 3, 3, 1])                                 # the last chunk has two steps, one of them taken
    assert train_validate._train_device_fed(net, None, 14, 0, report) == (14, True) and net.calls == [4, 4, 4, 2]
    net = Net([0])
    net.clip_norm = None
    assert train_validate._train_device_fed(net, None, 14, 0, report) == (14, True) and net.calls == [14]
