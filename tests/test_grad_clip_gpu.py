"""Global-norm gradient clipping and the non-finite-step guard on the card (include/catfish_hip_ext.h): the norm call alone, the
guarded optimizer call alone, the whole step of every native path, and the captured device-fed loop.

The definition (``training.TFOptimizer``): S = sum double(g_i)^2 in float64, g = sqrt(S), s32 = float32(c / max(g, c)), the
optimizer consumes g_i' = float32(g_i * s32); a step whose S or loss is not finite changes nothing, the step counter included.

Bounds.  The norm: positive terms added in any order carry at most (n - 1) u relative error on the sum (u = 2^-53; the squares
themselves are exact), the root halves it and adds one rounding: |g^ - g| <= n 2^-53 g against ``math.fsum`` of the exact squares.
The update: the derived bounds of ``tests/test_train_kernels_fp64.py::test_opt_step_matches_float64``, applied to g' built in
numpy float32 from the norm the card reported; no number is added here."""
import ctypes as C
import math

import numpy as np
import pytest

from catfish_amd.device_db import DeviceExampleDb
from oracle import catfish_oracle as oracle
from test_train_kernels_fp64 import _opt_inputs, opt_step_bounds_hold

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53


@pytest.fixture(scope="module")
def engine():
    """A model handle for the calls made directly: they use its device and nothing else of it."""
    from catfish_amd.engine import HipEngine
    eng = HipEngine(oracle.random_weights(seed=31), device=0, max_windows_per_pass=256)
    yield eng
    eng.close()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _exact_norm(g):
    return math.sqrt(math.fsum((np.asarray(g, dtype=np.float64) ** 2).tolist()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


class Norm(object):
    """cf_clip_norm on a device buffer, with its workspace and a zeroed record."""

    def __init__(self, engine, g):
        import torch
        from catfish_amd import _native as N
        self.N, self.lib, self.handle = N, engine._lib, engine._handle
        self.g = g
        self.n = int(g.numel())
        self.ws = torch.full((int(self.lib.cf_clip_workspace_doubles(self.n)),), float("nan"), dtype=torch.float64, device="cuda")
        self.rec = torch.zeros(4, dtype=torch.float64, device="cuda")

    def __call__(self, clip_norm, flags, loss=None):
        self.N.check(self.lib.cf_clip_norm(self.handle, _ptr(self.g), self.n, clip_norm, flags, _ptr(loss), _ptr(self.ws),
                                           int(self.ws.numel()), _ptr(self.rec), _stream()))
        return self.rec.cpu().numpy().copy()


def _sizes():
    from catfish_amd import _native as N
    chunk = N.CF_CLIP_CHUNK
    return [1, 255, 256, 257, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]


# ------------------------------------------------------------------------------------------------ the norm call alone
@pytest.mark.parametrize("which", range(8))
def test_norm_matches_the_exact_sum_and_repeats_itself(engine, which):
    import torch
    from catfish_amd import _native as N
    n = _sizes()[which]
    assert int(engine._lib.cf_clip_workspace_doubles(n)) == (n + N.CF_CLIP_CHUNK - 1) // N.CF_CLIP_CHUNK
    rng = np.random.default_rng(100 + n)
    g = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 4, n)).astype(np.float32)
    want = _exact_norm(g)
    norm = Norm(engine, torch.from_numpy(g).cuda())
    both = N.CF_CLIP_SCALE | N.CF_CLIP_SKIP_NONFINITE
    first = norm(0.5 * want, both)
    print("n %d: norm %.17g, exact %.17g, error %.3g of the allowed %.3g" % (n, first[0], want, abs(first[0] - want), n * U64 * want))
    assert abs(first[0] - want) <= n * U64 * want
    assert first[1] == float(np.float32(0.5 * want / max(first[0], 0.5 * want))) and first[1] < 1.0
    assert list(first[2:]) == [1.0, 0.0]
    norm.ws.fill_(float("nan"))                              # nothing is left over from the first run
    second = norm(0.5 * want, both)
    assert _same_bits(first[:2], second[:2]) and list(second[2:]) == [2.0, 0.0]
    loose = norm(2.0 * want, both)                           # g <= c: exactly 1, not counted as clipped
    assert loose[1] == 1.0 and _same_bits(loose[:1], first[:1]) and list(loose[2:]) == [2.0, 0.0]
    alone = norm(0.0, N.CF_CLIP_SKIP_NONFINITE)              # the guard alone: no scale, clip_norm not looked at
    assert alone[1] == 1.0 and list(alone[2:]) == [2.0, 0.0]
    bad_loss = norm(0.5 * want, both, loss=torch.full((1,), float("inf"), device="cuda"))
    assert bad_loss[1] == N.CF_CLIP_SKIPPED and _same_bits(bad_loss[:1], first[:1]) and list(bad_loss[2:]) == [2.0, 1.0]
    fine_loss = norm(0.5 * want, both, loss=torch.full((1,), 0.7, device="cuda"))
    assert _same_bits(fine_loss[:2], first[:2]) and list(fine_loss[2:]) == [3.0, 1.0]


@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("bad,where", [(float("nan"), "middle"), (float("-inf"), "last")])
def test_a_non_finite_gradient_makes_the_guarded_step_skip(engine, which, bad, where):
    """One NaN anywhere, or one -Inf in the last element of the last chunk: the record says skipped, and cf_opt_step_guarded
    leaves parameters, both slots, the packed buffer and the counter as they were, bit for bit.  With the guard off the same
    buffer goes through (and poisons the update, as without the option)."""
    import torch
    from catfish_amd import _native as N
    lib, handle = engine._lib, engine._handle
    n = _sizes()[which]
    p, g, s1, s2 = _opt_inputs(n, 1, seed=n)
    g[n // 2 if where == "middle" else n - 1] = bad
    rng = np.random.default_rng(n)
    n_packed = n + 3
    idx, scale = rng.integers(0, n, n_packed).astype(np.int32), rng.choice([1.0, -2.0], n_packed).astype(np.float32)
    dp, dg, d1, d2 = (torch.from_numpy(a.copy()).cuda() for a in (p, g, s1, s2))
    didx, dscale = torch.from_numpy(idx).cuda(), torch.from_numpy(scale).cuda()
    packed0 = rng.normal(size=n_packed).astype(np.float32)
    packed = torch.from_numpy(packed0.copy()).cuda()
    t_dev = torch.full((), 7.0, dtype=torch.float64, device="cuda")
    norm = Norm(engine, dg)
    rec = norm(1.0, N.CF_CLIP_SCALE | N.CF_CLIP_SKIP_NONFINITE)
    assert not math.isfinite(rec[0]) and rec[1] == N.CF_CLIP_SKIPPED and list(rec[2:]) == [0.0, 1.0]
    N.check(lib.cf_opt_step_guarded(handle, 1, _ptr(dp), _ptr(dg), _ptr(d1), _ptr(d2), n, 1e-3, _ptr(t_dev), _ptr(didx), _ptr(dscale),
                                    _ptr(packed), n_packed, _ptr(norm.rec), _stream()))
    assert float(t_dev) == 7.0
    for got, want in ((dp, p), (d1, s1), (d2, s2), (packed, packed0), (dg, g)):
        assert _same_bits(got.cpu().numpy(), want)
    rec = norm(1.0, N.CF_CLIP_SCALE)                         # the guard switched off: not a skip
    assert rec[1] != N.CF_CLIP_SKIPPED and list(rec[2:]) in ([0.0, 1.0], [1.0, 1.0])


def test_bad_arguments_are_refused_before_any_launch(engine):
    import torch
    from catfish_amd import _native as N
    lib, handle = engine._lib, engine._handle
    n = N.CF_CLIP_CHUNK + 1
    g = torch.ones(n, device="cuda")
    ws = torch.zeros(2, dtype=torch.float64, device="cuda")
    rec = torch.zeros(4, dtype=torch.float64, device="cuda")
    both = N.CF_CLIP_SCALE | N.CF_CLIP_SKIP_NONFINITE
    assert int(lib.cf_ext_abi_version()) == N.CF_EXT_ABI_VERSION
    assert int(lib.cf_clip_workspace_doubles(0)) == 0 and int(lib.cf_clip_workspace_doubles(-5)) == 0
    calls = [(handle, _ptr(g), n, c, both, None, _ptr(ws), 2, _ptr(rec)) for c in (0.0, -1.0, float("nan"), float("inf"))]
    calls += [(handle, _ptr(g), n, 1.0, both, None, _ptr(ws), 1, _ptr(rec)),          # a short workspace
              (handle, _ptr(g), 0, 1.0, both, None, _ptr(ws), 2, _ptr(rec)), (handle, _ptr(g), -1, 1.0, both, None, _ptr(ws), 2, _ptr(rec)),
              (handle, None, n, 1.0, both, None, _ptr(ws), 2, _ptr(rec)), (handle, _ptr(g), n, 1.0, both, None, None, 2, _ptr(rec)),
              (handle, _ptr(g), n, 1.0, both, None, _ptr(ws), 2, None), (None, _ptr(g), n, 1.0, both, None, _ptr(ws), 2, _ptr(rec)),
              (handle, _ptr(g), n, 1.0, 0, None, _ptr(ws), 2, _ptr(rec)), (handle, _ptr(g), n, 1.0, 4, None, _ptr(ws), 2, _ptr(rec)),
              (handle, C.c_void_p(g.data_ptr() + 4), n - 1, 1.0, both, None, _ptr(ws), 2, _ptr(rec))]      # not 16-byte aligned
    for args in calls:
        assert lib.cf_clip_norm(*args, _stream()) == N.CF_ERR_INVALID, args
    with pytest.raises(ValueError, match="clip_norm"):
        N.check(lib.cf_clip_norm(*calls[0], _stream()))
    p = torch.ones(4, device="cuda")
    t_dev = torch.zeros((), dtype=torch.float64, device="cuda")
    ok = [handle, 1, _ptr(p), _ptr(p), _ptr(p), _ptr(p), 4, 1e-3, _ptr(t_dev), None, None, None, 0, _ptr(rec)]
    for at, value in ((0, None), (1, 2), (2, None), (3, None), (4, None), (5, None), (6, 0), (8, None), (12, -1), (12, 3), (13, None)):
        args = list(ok)
        args[at] = value
        assert lib.cf_opt_step_guarded(*args, _stream()) == N.CF_ERR_INVALID, (at, value)
    torch.cuda.synchronize()
    assert float(t_dev) == 0.0 and rec.cpu().tolist() == [0.0] * 4 and p.cpu().tolist() == [1.0] * 4 and ws.cpu().tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the guarded optimizer call alone
@pytest.mark.parametrize("kind,steps_before", [(0, 0), (1, 0), (1, 1), (1, 999), (1, 50000)])
def test_guarded_opt_step_matches_float64_on_the_scaled_gradients(engine, kind, steps_before):
    """At the sizes of ``test_opt_step_matches_float64``.  c = half the norm the card reports: its derived bounds hold for
    g' = float32(g * s32).  c = twice it: the result is cf_opt_step's, bit for bit, the packed buffer and the counter included."""
    import torch
    from catfish_amd import _native as N
    lib, handle = engine._lib, engine._handle
    lr = float(np.float32(1e-3))
    for n in (1, 255, 256, 257, 70003):
        p, g, s1, s2 = _opt_inputs(n, kind, seed=n + steps_before)
        rng = np.random.default_rng(n)
        n_packed = 3 * n + 5
        idx = rng.integers(0, n, n_packed).astype(np.int32)
        scale = rng.choice([1.0, -2.0, 0.72134752], n_packed).astype(np.float32)
        didx, dscale = torch.from_numpy(idx).cuda(), torch.from_numpy(scale).cuda()
        exact = _exact_norm(g)
        results = {}
        for factor in (0.5, 2.0, None):                      # None: cf_opt_step itself
            dp, dg, d1, d2 = (torch.from_numpy(a.copy()).cuda() for a in (p, g, s1, s2))
            packed = torch.full((n_packed,), float("nan"), device="cuda")
            t_dev = torch.full((), float(steps_before), dtype=torch.float64, device="cuda")
            args = (handle, kind, _ptr(dp), _ptr(dg), _ptr(d1), _ptr(d2), n, lr, _ptr(t_dev), _ptr(didx), _ptr(dscale), _ptr(packed), n_packed)
            if factor is None:
                N.check(lib.cf_opt_step(*args, _stream()))
            else:
                c = factor * exact
                norm = Norm(engine, dg)
                rec = norm(c, N.CF_CLIP_SCALE | N.CF_CLIP_SKIP_NONFINITE)
                s32 = np.float32(c / max(rec[0], c))         # from the norm the card reported
                assert rec[1] == float(s32) and (s32 == 1.0) == (factor == 2.0) and abs(rec[0] - exact) <= n * U64 * exact
                N.check(lib.cf_opt_step_guarded(*args, _ptr(norm.rec), _stream()))
                assert np.array_equal(dg.cpu().numpy(), g)
                scaled = (g * s32).astype(np.float32)
                got = dp.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()
                assert opt_step_bounds_hold(kind, got[0], got[1], got[2], p, scaled, s1, s2, lr, steps_before) == [], (kind, n, factor)
                assert _same_bits(packed.cpu().numpy(), got[0][idx] * scale)
            assert float(t_dev) == steps_before + 1.0
            results[factor] = [a.cpu().numpy() for a in (dp, d1, d2, packed)]
        assert all(_same_bits(a, b) for a, b in zip(results[2.0], results[None])), (kind, n)
        if n == 70003:                                       # (a single zero or 1e-20 gradient moves nothing either way)
            assert not _same_bits(results[0.5][0], results[None][0]), (kind, n)


# ------------------------------------------------------------------------------------------------ the whole step
# name -> (units, channels, layers, blocks, native, optimizer, windows): the smallest model each native path takes
MODELS = {"tuned-16": (64, 32, 1, 1, None, "RMSProp", 16), "tuned-17": (64, 32, 1, 1, None, "Adam", 17),      # 17: one real window in tile 2
          "anysize-16": (16, 16, 1, 1, True, "Adam", 16), "rnn32-16": (32, 32, 1, 0, True, "RMSProp", 16)}
KINDS = {"tuned-16": "tuned_step", "tuned-17": "tuned_step", "anysize-16": "anysize_step", "rnn32-16": "anysize_step"}
LR = 1e-3


def _trainer(name, kp, **kw):
    from catfish_amd.training import Trainer
    h, c, n_layers, n_blocks, native, choice, _ = MODELS[name]
    w = oracle.random_weights(seed=21, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks)
    tr = Trainer(w, n_layers, n_blocks, choice, LR, kp, seed=5, native=native, **kw)
    assert tr.mode == KINDS[name]
    return tr


def _batch(name, seed=4):
    n = MODELS[name][6]
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 35)).astype(np.float32), (rng.random((n, 35)) < 0.3).astype(np.float32)


def _flat(tr):
    """(params, slot1, slot2, packed) of the native step's flat buffers, on the host."""
    s = tr.step_impl
    n = s.n_total - 1
    return [a.detach().cpu().numpy().copy() for a in (s.pflat[:n], s.s1[:n], s.s2[:n], s.packed)]


def _close(tr):
    if tr.engine is not None:
        tr.engine.close()


_FIRST = {}


def _first_gradients(name, kp):
    """(exact norm, trainable gradient floats) of the first step's gradients, from ``Trainer.gradients``: computed once per case."""
    if (name, kp) not in _FIRST:
        probe = _trainer(name, kp)
        x, y = _batch(name)
        _, grads = probe.gradients(x, y)
        _close(probe)
        _FIRST[name, kp] = (_exact_norm(np.concatenate([a.ravel() for a in grads.values()])), sum(a.size for a in grads.values()))
    return _FIRST[name, kp]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_clipped_step_follows_the_definition(name):
    """c = half the norm of the first step's gradients (numpy, over the dict of trainable gradients): the record's norm is that
    norm to the bound of the norm test -- the never-written slots of the moving statistics add nothing --, and after one step every
    variable and slot meets the optimizer's derived bounds for g' = float32(g * s32)."""
    kp = 0.8
    norm, n_trainable = _first_gradients(name, kp)
    assert norm > 0
    c = 0.5 * norm
    tr = _trainer(name, kp, clip_norm=c, use_graph=False)
    x, y = _batch(name)
    p0, a0, b0, _ = _flat(tr)
    loss = tr.train_step(x, y)
    stats = tr.step_stats()
    n = tr.step_impl.n_total - 1
    print(name, "loss", loss, "norm", stats["grad_norm"], "numpy", norm, "error", abs(stats["grad_norm"] - norm), "allowed", n_trainable * U64 * norm)
    assert abs(stats["grad_norm"] - norm) <= n_trainable * U64 * norm
    s32 = np.float32(c / max(stats["grad_norm"], c))
    assert stats == {"grad_norm": stats["grad_norm"], "scale": float(s32), "clipped": 1, "skipped": 0} and s32 < 1 and float(tr.opt.t) == 1.0
    g = tr.step_impl.gflat[:n].cpu().numpy()
    assert abs(_exact_norm(g) - norm) <= n * U64 * norm
    p1, a1, b1, packed1 = _flat(tr)
    kind = tr.step_impl.kind
    assert opt_step_bounds_hold(kind, p1, a1, b1, p0, (g * s32).astype(np.float32), a0, b0, float(np.float32(LR)), 0) == []
    assert not _same_bits(p1, p0)
    idx, scale = tr.step_impl.pack_idx.cpu().numpy(), tr.step_impl.pack_scale.cpu().numpy()
    full = tr.step_impl.pflat.cpu().numpy()
    assert _same_bits(packed1, full[idx] * scale)
    _close(tr)


@pytest.mark.parametrize("kp", [1.0, 0.8])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_a_clip_that_never_bites_changes_no_bit(name, kp):
    """c = twice the first norm: three (captured) steps give the losses, variables, slots and packs of ``clip_norm=None``."""
    norm, _ = _first_gradients(name, kp)
    out = {}
    for c in (None, 2.0 * norm):
        tr = _trainer(name, kp, clip_norm=c)
        losses = [tr.train_step(*_batch(name, seed=4)) for _ in range(3)]       # one batch: the norm only falls
        out[c] = (np.asarray(losses, dtype=np.float32), _flat(tr), tr.step_stats())
        assert float(tr.opt.t) == 3.0 and tr._graph is not None
        _close(tr)
    plain, clipped = out[None], out[2.0 * norm]
    print(name, kp, "losses", plain[0], clipped[0], "stats", clipped[2])
    assert clipped[2]["scale"] == 1.0 and clipped[2]["clipped"] == 0 and clipped[2]["skipped"] == 0 and clipped[2]["grad_norm"] > 0
    assert plain[2] == {"grad_norm": 0.0, "scale": 0.0, "clipped": 0, "skipped": 0}
    assert _same_bits(plain[0], clipped[0]) and np.isfinite(plain[0]).all()
    assert all(_same_bits(a, b) for a, b in zip(plain[1], clipped[1]))


# ------------------------------------------------------------------------------------------------ capture
def _db():
    rng = np.random.default_rng(12)
    return DeviceExampleDb(rng.normal(size=(500, 35)).astype(np.float32), rng.normal(size=(900, 35)).astype(np.float32), seed=7)


@pytest.mark.parametrize("name", ["tuned-16", "anysize-16"])
def test_captured_device_fed_steps_equal_eager_ones(name):
    """Five replays of the device-fed graph against five eager ``train_step`` calls on the twin database, clipping live in every
    step: losses, variables, slots and packs bit for bit, the record too, five steps clipped."""
    kp = 0.8
    norm, _ = _first_gradients(name, kp)
    c = 0.01 * norm                                          # far below any batch's norm: live in every step
    eager = _trainer(name, kp, clip_norm=c, use_graph=False)
    twin = _db()
    want = np.asarray([eager.train_step(x, y) for x, y, _ in (twin.get_training_set(16) for _ in range(5))], dtype=np.float32)
    fed = _trainer(name, kp, clip_norm=c)
    got = fed.train_steps(_db(), 5, 16)
    assert fed._fed is not None and _same_bits(got, want) and np.isfinite(got).all()
    assert all(_same_bits(a, b) for a, b in zip(_flat(fed), _flat(eager)))
    assert fed.step_stats() == eager.step_stats() and fed.step_stats()["clipped"] == 5 and fed.step_stats()["skipped"] == 0
    _close(fed), _close(eager)


def test_a_nan_planted_between_replays_is_skipped():
    """A NaN in the static gradient buffer, not a diverging model: an update-free run fills the buffer, then the NaN goes into a
    float that no kernel of the any-size step writes, a moving statistic's slot (``include/catfish_hip.h``: "the moving statistics
    are not written"; every other float is rewritten by the replay, and the tuned conv-stack reduction rewrites these too, with
    zeros).  The next replay is skipped: variables, slots, packs and ``opt.t`` stay bit for bit.  With the NaN taken out again the
    replay after it proceeds."""
    name, kp = "anysize-16", 0.8
    norm, _ = _first_gradients(name, kp)
    fed = _trainer(name, kp, clip_norm=0.01 * norm)
    db = _db()
    fed.train_steps(db, 2, 16)
    step = fed.step_impl
    off = next(o for k, o, _ in step.entries if k.endswith("/moving_mean"))
    fed.gradients(*_batch(name))                             # update-free: gradients into the static buffer, nothing else moves
    assert float(step.gflat[off]) == 0.0 and float(fed.opt.t) == 2.0 and fed.step_stats()["clipped"] == 2
    before = _flat(fed)
    step.gflat[off] = float("nan")
    fed.train_steps(db, 1, 16)
    stats = fed.step_stats()
    print("after the planted NaN:", stats, "opt.t", float(fed.opt.t))
    assert stats["skipped"] == 1 and stats["clipped"] == 2 and stats["scale"] == -1.0 and float(fed.opt.t) == 2.0
    assert all(_same_bits(a, b) for a, b in zip(_flat(fed), before))
    step.gflat[off] = 0.0
    last = fed.train_steps(db, 1, 16)
    stats = fed.step_stats()
    assert stats["skipped"] == 1 and stats["clipped"] == 3 and float(fed.opt.t) == 3.0 and np.isfinite(last).all()
    assert not _same_bits(_flat(fed)[0], before[0])
    _close(fed)
