"""The any-size training kernels against float64, per LDS size class and wave count (GPU).

The second kernel family trains every geometry but the shipped 64 / 32 one and carries the operator's backward:
``gen_gru_kernel<true, false>`` / ``gen_gru_bwd_kernel`` (csrc/generic.hpp) and the ``cf_gen_*`` GEMM-shaped kernels
(csrc/gen_train.hpp).  Their launch shape (csrc/anysize_launch.hpp, tests/test_anysize_launch.py on the CPU) gives a workgroup
1..8 waves by tiles per CU and by how many waves' state fits the LDS at the layer size; every case here asserts the regime it
is there for through ``cf_gru_anysize_train_shape`` and then compares with float64:

  F  one layer through ``anysize_train.anysize_bigru`` against ``bigru_layer`` (tests/test_train_kernels_fp64.py, tied to the
     golden graph there): y, dx and the eight weight gradients per tensor, y and dx also per window.  Layer sizes 16, 48, 80,
     96, 112, 160, 176, 256 cover the four LDS classes, the three launches that ask for exactly 163 840 bytes (80 backward and
     160 forward at 8 waves, 160 backward at 4) and the output-tile groups of four with a remainder; window counts are
     ``16 tiles - 5`` with tiles = C/2 + 1, C + 1, 3C/2 + 1, 2C + 1, 7C/2 + 1 on C CUs: 2, 3, 4, 5 and 8 waves, the last
     workgroup partly empty, the last tile padded.  Above 2048 windows the references run in slabs of 2048 and their weight
     gradients are summed in float64 (the sum is linear in windows).
  G  ``cf_gen_gru_wgrad`` and ``cf_gen_gru_dx`` directly on random fragment planes against float64 ``A^T dA`` (A = [x | h_prev | 1]
     for the gates, [x | r h_prev | 1] for the candidate) and ``da_g Wg[:cin]^T + da_c Wc[:cin]^T``: row counts one past a
     multiple of 64 (the bias row alone in its row block), N of 16 / 48 / 96 / 192, a last position chunk of 16 windows.
  H  the whole ``AnySizeTrainStep`` with dropout (masks drawn in the kernels, and the same masks passed in) against
     ``TorchResNetRNN(dtype=float64)`` under those masks: (96, 48, 2, 1) at 3 waves and the plain RNN (112, 0, 2, 0) at 2.

Bounds.  As in tests/test_train_kernels_fp64.py every case records two errors against float64, ``max|d| / max|ref|`` per tensor
(the loss: absolute): the kernels' and the float32 eager torch restatement's of the same computation (``bigru_layer`` in
float32 for F, the same products in float32 for G, the float32 ``TorchResNetRNN`` for H, there only in the measuring run).  The
asserted bound of a quantity is 4 x the largest yardstick error over its section and never looser than what the older any-size
tests allow (2e-4 relative, loss 1e-5 absolute).  The pairs are in profiles/anysize_train_fp64_parity.jsonl (appended, with
commit and device, when CATFISH_PARITY_LOG names a file); ``BOUNDS`` holds the constants and tests/test_training.py checks
them against that file.
Every quantity met the rule as measured, none fell back to the older bound: F y 6.62e-6 (per window 6.75e-6), dx 2.80e-6 (per
window 4.37e-6), weight gradients 2.57e-5; G weight gradients 7.97e-6, dx 2.28e-6; H loss 1.31e-7 absolute, gradients 2.81e-6.
Case by case the kernels' y is up to 4 x the yardstick's error of that case (96 units, 43 windows: 7.1e-7 against 1.8e-7), which
is where the approximate ``v_rcp`` / ``v_exp`` of the gate activations show; over the section their largest error is 1.05 x the
yardstick's largest (1.74e-6 against 1.66e-6, both at 256 units and 512 inputs), so the rule holds without a fallback.

H's loss bound is about two float32 ulps of a loss near 0.7 (the kernels: 3.9e-8), as the rule makes it; the runs are
deterministic, but a harmless reordering of the head's sums can trip it: re-measure then, do not widen by hand.  The largest
case (160 units, 14 347 windows, 8 waves forward and 4 backward, both at the whole 160 KB) takes 0.8 s on an MI355X, the
whole step at (96, 48, 2, 1) and 4107 windows is the longest: 1.0 s in an ordinary run, 10 s in the measuring run, where the
float32 yardstick's convolution library builds its kernels for the size.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from test_train_kernels_fp64 import GRU_KEYS, GRU_PRE, T, _measuring, _record, _rel, _rel_window, bigru_layer

pytestmark = pytest.mark.gpu

# quantity -> asserted bound = min(4 x largest float32-torch error, older tests' bound).  The largest float32-torch errors in
# profiles/anysize_train_fp64_parity.jsonl (MI355X, 256 CUs), and the largest errors of the kernels next to them:
#   F.y 1.656e-06 (kernels 1.74e-06)   F.y_window 1.688e-06 (1.82e-06)   F.dx 7.006e-07 (7.23e-07)   F.dx_window 1.095e-06 (1.18e-06)
#   F.wgrad 6.446e-06 (1.38e-05)   G.wgrad 1.994e-06 (1.26e-06)   G.dx 5.723e-07 (1.77e-06)   H.loss 3.286e-08 (3.87e-08)
#   H.grads 7.047e-07 (5.61e-07)
# 4 x each of them, rounded down, is far below the older bound of its quantity (2e-4; loss 1e-5 absolute), so it is the bound.
# G.dx is the tightest (0.77 of its bound, h 256 / cin 512: gt_tile sums the 1536 products of an element in one chain of fmaf),
# F.wgrad next (0.54, h 16 at 14 347 windows: a library GEMM over 502 145 positions in both the kernels' path and the yardstick).
BOUNDS = {
    "F.y": 6.62e-6, "F.y_window": 6.75e-6, "F.dx": 2.80e-6, "F.dx_window": 4.37e-6, "F.wgrad": 2.57e-5,
    "G.wgrad": 7.97e-6, "G.dx": 2.28e-6,
    "H.loss": 1.31e-7, "H.grads": 2.81e-6,
}
# what tests/test_anysize_native_step.py and tests/test_gpu_pipeline.py allow for the quantity (the loss: absolute)
OLDER_BOUNDS = {"F.y": 2e-4, "F.y_window": 2e-4, "F.dx": 2e-4, "F.dx_window": 2e-4, "F.wgrad": 2e-4, "G.wgrad": 2e-4, "G.dx": 2e-4,
                "H.loss": 1e-5, "H.grads": 2e-4}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "anysize_train_fp64_parity.jsonl")
SLAB = 2048              # windows per evaluation of a reference
LDS_LIMIT = 163840


def bounds_from_profile(path=PROFILE):
    """{quantity: min(4 x largest float32-torch error in the profile, older bound)}: what ``BOUNDS`` may not exceed
    (tests/test_training.py checks that on the CPU)."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            key = "%s.%s" % (row["section"], row["quantity"])
            worst[key] = max(worst.get(key, 0.0), row["torch_fp32"])
    return {k: min(4.0 * v, OLDER_BOUNDS[k]) for k, v in worst.items()}


def _check(section, case, pairs):
    """pairs: {quantity: (kernel error, yardstick error)}.  All are recorded (printed as ``parity`` rows), then all are asserted."""
    for q, (k, y) in pairs.items():
        _record(section, case, q, k, y)
    bad = {q: (k, BOUNDS["%s.%s" % (section, q)]) for q, (k, _) in pairs.items() if not k <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ launch regimes
# tiles by label on C CUs, and the waves per workgroup ceil(2 tiles / C) the label stands for (before the size's own maximum)
TILES = {"1": lambda c: 1, "43": lambda c: 3, "W2": lambda c: c // 2 + 1, "W3": lambda c: c + 1, "W4": lambda c: 3 * c // 2 + 1,
         "W5": lambda c: 2 * c + 1, "W8": lambda c: 7 * c // 2 + 1}
WAVES = {"1": 1, "43": 1, "W2": 2, "W3": 3, "W4": 4, "W5": 5, "W8": 8}
# layer size -> (state arrays of the forward, most waves of the forward, of the backward): DESIGN.md "Any-size path"
CLASSES = {16: (3, 8, 8), 48: (3, 8, 8), 80: (3, 8, 8), 96: (3, 8, 4), 112: (2, 8, 4), 160: (2, 8, 4), 176: (2, 4, 2), 256: (2, 4, 2)}
SIZES = sorted(CLASSES)


def _windows(label, n_cu):
    return 1 if label == "1" else 16 * TILES[label](n_cu) - 5


def _shape(engine, h, npad):
    """cf_gru_anysize_train_shape: the launch shape of both recurrences at ``npad`` windows."""
    from catfish_amd import _native as N
    out = (C.c_int64 * 8)()
    N.check(engine._lib.cf_gru_anysize_train_shape(engine._handle, h, npad, out))
    keys = ("waves", "grid_x", "lds_bytes")
    return dict(zip(keys, out[0:3]), h_via_y=int(out[3])), dict(zip(keys, out[4:7]), max_waves=int(out[7]))


def _assert_regime(engine, h, label):
    """The case (h, label) runs what its label says: the wave count of the label, clamped by the size's class; with more than
    one wave a partly empty last workgroup; LDS = waves x arrays x h / 16 KB.  -> (forward, backward) shapes."""
    tiles = TILES[label](engine.launch_regimes()["n_cu"])
    arrays, fwd_max, bwd_max = CLASSES[h]
    fwd, bwd = _shape(engine, h, 16 * tiles)
    print("regime h %d, %s: %d tiles, forward %s, backward %s" % (h, label, tiles, fwd, bwd))
    assert fwd["waves"] == min(WAVES[label], fwd_max) and bwd["waves"] == min(WAVES[label], bwd_max), (h, label, fwd, bwd)
    assert fwd["h_via_y"] == int(arrays == 2) and bwd["max_waves"] == bwd_max
    assert fwd["lds_bytes"] == fwd["waves"] * arrays * (h // 16) * 1024 <= LDS_LIMIT
    assert bwd["lds_bytes"] == bwd["waves"] * 4 * (h // 16) * 1024 <= LDS_LIMIT
    for s in (fwd, bwd):
        assert s["grid_x"] * s["waves"] >= tiles > (s["grid_x"] - 1) * s["waves"]
        assert s["waves"] == 1 or s["grid_x"] * s["waves"] > tiles, (h, label, s)          # waves past the last tile return early
    return fwd, bwd


@pytest.fixture(scope="module")
def engine():
    """The C-ABI handle the launches go through: the entry points under test take the layer size as an argument."""
    from catfish_amd.engine import HipEngine
    geo = dict(layer_size=16, n_layers=1, layer_size_res=16, n_layers_res=1)
    eng = HipEngine(oracle.random_weights(seed=41, **geo), device=0, max_windows_per_pass=256, **geo)
    yield eng
    eng.close()


def test_the_exact_limit_launches_are_among_the_cases(engine):
    """Three launches ask for the whole 160 KB: 80 units backward and 160 units forward at 8 waves, 160 units backward at 4."""
    assert ("W8", 80) in F_CASES_SET and ("W8", 160) in F_CASES_SET and ("W5", 160) in F_CASES_SET
    fwd, bwd = _assert_regime(engine, 80, "W8")
    assert (fwd["waves"], bwd["waves"], bwd["lds_bytes"]) == (8, 8, LDS_LIMIT)
    fwd, bwd = _assert_regime(engine, 160, "W8")
    assert (fwd["waves"], fwd["lds_bytes"], bwd["waves"], bwd["lds_bytes"]) == (8, LDS_LIMIT, 4, LDS_LIMIT)
    fwd, bwd = _assert_regime(engine, 160, "W5")
    assert (fwd["waves"], bwd["waves"], bwd["lds_bytes"]) == (5, 4, LDS_LIMIT)


def test_shape_call_checks_its_arguments_like_the_launches(engine):
    """cf_gru_anysize_train_shape refuses what cf_gru_anysize_train_forward / _backward refuse: a layer size that is no multiple
    of 16 or above 256, a window count that is no positive multiple of 16, a null output."""
    from catfish_amd import _native as N
    out = (C.c_int64 * 8)()
    for h, n, o in ((24, 16, out), (272, 16, out), (0, 16, out), (16, 17, out), (16, 0, out), (16, 16, None)):
        with pytest.raises(ValueError):
            N.check(engine._lib.cf_gru_anysize_train_shape(engine._handle, h, n, o))
    N.check(engine._lib.cf_gru_anysize_train_shape(engine._handle, 256, 16, out))
    assert list(out) == [1, 1, 2 * 16 * 1024, 1, 1, 1, 4 * 16 * 1024, 2]


# ------------------------------------------------------------------------------------------------ F. one layer
def _layer_params(h, cin, seed):
    """Glorot weights of one biGRU layer with ``cin`` inputs, from oracle.random_weights: the 8 arrays (gates kernel, gates bias,
    candidate kernel, candidate bias) of the forward, then of the backward direction."""
    if cin == 1:                     # layer 0 of the plain RNN type
        w, layer = oracle.random_weights(seed=seed, layer_size=h, n_layers=1, n_layers_res=0), 0
    elif cin == 2 * h:               # a layer above the first
        w, layer = oracle.random_weights(seed=seed, layer_size=h, n_layers=2, layer_size_res=16, n_layers_res=1), 1
    else:                            # layer 0 behind a conv stack of cin channels
        w, layer = oracle.random_weights(seed=seed, layer_size=h, n_layers=1, layer_size_res=cin, n_layers_res=1), 0
    p = [w[(GRU_PRE % (layer, d)) + k] for d in ("fw", "bw") for k in GRU_KEYS]
    assert p[0].shape == (cin + h, 2 * h) and p[2].shape == (cin + h, h)
    return p


F_CASES = ([(label, h, cin) for label in ("1", "43") for h in SIZES for cin in (16, 2 * h)] +
           [(label, h, cin) for label in ("1", "43") for h, cin in ((112, 1), (48, 80))] +
           [("W2", h, 16) for h in SIZES] +
           [(label, h, 16) for label in ("W3", "W4") for h in (16, 96, 112, 176, 256)] +
           [(label, h, 16) for label in ("W5", "W8") for h in (16, 80, 96, 160)])
F_CASES_SET = {(label, h) for label, h, _ in F_CASES}


@pytest.mark.parametrize("label,h,cin", F_CASES)
def test_anysize_bigru_layer_matches_float64(engine, label, h, cin):
    """y, dx and the eight weight gradients of one layer on gen_gru_kernel<true, false> / gen_gru_bwd_kernel (the weight and
    input gradients are anysize_bigru's library GEMMs over the kernels' da) against ``bigru_layer`` in float64."""
    import torch
    from catfish_amd.anysize_train import anysize_bigru
    _assert_regime(engine, h, label)
    n = _windows(label, engine.launch_regimes()["n_cu"])
    p_np = _layer_params(h, cin, seed=1000 * h + cin)
    gen = torch.Generator(device="cuda").manual_seed(100000 * h + 100 * cin + WAVES[label] + n)
    x32 = torch.randn(n, T, cin, generator=gen, device="cuda", dtype=torch.float32) * 1.2
    g32 = torch.randn(n, T, 2 * h, generator=gen, device="cuda", dtype=torch.float32)

    def reference(dtype):
        """(y, dx, weight gradients in float64) of ``bigru_layer`` in ``dtype``, in slabs of at most SLAB windows."""
        ps = [torch.tensor(p, dtype=dtype, device="cuda", requires_grad=True) for p in p_np]
        ys, dxs, gw = [], [], [torch.zeros(p.shape, dtype=torch.float64, device="cuda") for p in p_np]
        for a in range(0, n, SLAB):
            x = x32[a:a + SLAB].to(dtype).requires_grad_(True)
            y = bigru_layer(x, ps)
            grads = torch.autograd.grad(y, [x] + ps, g32[a:a + SLAB].to(dtype))
            ys.append(y.detach())
            dxs.append(grads[0])
            for acc, g in zip(gw, grads[1:]):
                acc += g.double()
        return torch.cat(ys), torch.cat(dxs), gw

    y64, dx64, gw64 = reference(torch.float64)
    y_t, dx_t, gw_t = reference(torch.float32)
    x = x32.clone().requires_grad_(True)
    ps = [torch.tensor(p, dtype=torch.float32, device="cuda", requires_grad=True) for p in p_np]
    y_k = anysize_bigru(x, ps, engine)
    grads = torch.autograd.grad(y_k, [x] + ps, g32)
    y_k, dx_k, gw_k = y_k.detach(), grads[0], grads[1:]
    assert y_k.shape == (n, T, 2 * h) and dx_k.shape == (n, T, cin)
    _check("F", "h %d, cin %d, %d windows (%s)" % (h, cin, n, label), {
        "y": (_rel(y_k, y64), _rel(y_t, y64)),
        "y_window": (_rel_window(y_k, y64), _rel_window(y_t, y64)),
        "dx": (_rel(dx_k, dx64), _rel(dx_t, dx64)),
        "dx_window": (_rel_window(dx_k, dx64), _rel_window(dx_t, dx64)),
        "wgrad": (max(_rel(a, b) for a, b in zip(gw_k, gw64)), max(_rel(a, b) for a, b in zip(gw_t, gw64))),
    })


# ------------------------------------------------------------------------------------------------ G. cf_gen_gru_wgrad, cf_gen_gru_dx
# (h, cin, windows): windows 16 = one half chunk of positions, 64 = two chunks, 48 = a full chunk then a half one
G_CASES = ([(h, cin, n) for h, cin in ((16, 16),        # smallest shape
                                       (16, 48),        # 65 rows: the bias row alone in its row block
                                       (48, 96),        # N of 96 and 48
                                       (112, 1),        # layer 0 of the plain RNN: weight gradients only
                                       (96, 192))       # 289 rows, N of 192 and 96
            for n in (16, 64)] +
           [(256, 512, 48)])                            # 13 row blocks, 8 column blocks


@pytest.mark.parametrize("h,cin,npad", G_CASES)
def test_gen_gru_wgrad_and_dx_match_float64(engine, h, cin, npad):
    """cf_gen_gru_wgrad and cf_gen_gru_dx on random fragments: y from tanh, the stash from a sigmoid, da zero in the 5 padding
    windows of the last tile (the kernels' contract) and random everywhere else, workspace and outputs pre-filled with NaN.
    h_prev = y shifted by one step in the direction's order, zero at its first step."""
    import torch
    from catfish_amd import _native as N
    from catfish_amd.native_train import frag_to_nat
    lib, hd = engine._lib, engine._handle
    tiles, h16, kbx, rows = npad // 16, h // 16, (cin + 15) // 16, cin + h + 1
    gen = torch.Generator(device="cuda").manual_seed(10000 * h + 10 * cin + npad)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, device="cuda", dtype=torch.float32)      # noqa: E731
    x_frag, y_frag = rnd(tiles, T, kbx, 64, 4), torch.tanh(rnd(tiles, T, 2 * h16, 64, 4))
    stash = torch.sigmoid(rnd(tiles, T, 2, 3, h16, 64, 4))
    da = rnd(tiles, T, 2, 3, h16, 64, 4)
    da.view(tiles, T, 2, 3, h16, 4, 16, 4)[tiles - 1, :, :, :, :, :, 11:, :] = 0.0       # lane = 16 q + window
    p_np = _layer_params(h, cin, seed=7 * h + cin)
    params = torch.cat([torch.from_numpy(np.ascontiguousarray(p)).reshape(-1) for p in p_np]).cuda()
    dir_floats = (cin + h) * 3 * h + 3 * h
    assert params.numel() == 2 * dir_floats
    ws_floats = int(lib.cf_gen_train_workspace_floats(rows, 2 * h, npad))
    ws = torch.full((ws_floats,), float("nan"), device="cuda")
    grads = torch.full((2 * dir_floats,), float("nan"), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(lib.cf_gen_gru_wgrad(hd, h, cin, N._p(x_frag), N._p(y_frag), N._p(stash), N._p(da), N._p(ws), ws_floats, N._p(grads), npad, stream))
    dx_frag = torch.full((tiles, T, kbx, 64, 4), float("nan"), device="cuda")
    if cin == 1:
        with pytest.raises(ValueError):                  # the one signal feature has no fragment plane of gradients
            N.check(lib.cf_gen_gru_dx(hd, h, cin, N._p(params), N._p(da), N._p(dx_frag), npad, stream))
    else:
        N.check(lib.cf_gen_gru_dx(hd, h, cin, N._p(params), N._p(da), N._p(dx_frag), npad, stream))

    def reference(dtype):
        """([per direction: gates kernel | bias row, candidate kernel | bias row], dx [npad, 35, cin])"""
        x2 = frag_to_nat(x_frag).to(dtype)[:, :, :cin].reshape(-1, cin)
        y = frag_to_nat(y_frag).to(dtype)
        one = x2.new_ones(x2.shape[0], 1)
        res, dx = [], 0
        for d in range(2):
            da_d = frag_to_nat(da[:, :, d].reshape(tiles, T, 3 * h16, 64, 4)).to(dtype)          # r | u | c
            assert float(da_d[npad - 5:].abs().max()) == 0.0 and float(da_d[npad - 6].abs().max()) > 0.0
            r = frag_to_nat(stash[:, :, d, 0]).to(dtype)
            hd_ = y[:, :, h * d:h * d + h]
            hprev = torch.zeros_like(hd_)
            if d == 0:
                hprev[:, 1:] = hd_[:, :-1]
            else:
                hprev[:, :-1] = hd_[:, 1:]
            da_g, da_c = da_d[:, :, :2 * h].reshape(-1, 2 * h), da_d[:, :, 2 * h:].reshape(-1, h)
            a_g = torch.cat([x2, hprev.reshape(-1, h), one], 1)
            a_c = torch.cat([x2, (r * hprev).reshape(-1, h), one], 1)
            res += [a_g.t() @ da_g, a_c.t() @ da_c]
            wg, wc = (torch.as_tensor(p_np[4 * d + k], dtype=dtype, device="cuda") for k in (0, 2))
            dx = dx + da_g @ wg[:cin].t() + da_c @ wc[:cin].t()
        return res, dx.reshape(npad, T, cin)

    (w64, dx64), (w32, dx32) = reference(torch.float64), reference(torch.float32)
    e_k = e_t = 0.0
    for d in range(2):
        o = grads[d * dir_floats:(d + 1) * dir_floats]
        got = [o[:rows * 2 * h].view(rows, 2 * h), o[rows * 2 * h:].view(rows, h)]
        for a, b, c in zip(got, w32[2 * d:2 * d + 2], w64[2 * d:2 * d + 2]):
            # kernel and bias row are separate tensors of the model: each over its own maximum
            e_k = max(e_k, _rel(a[:-1], c[:-1]), _rel(a[-1], c[-1]))
            e_t = max(e_t, _rel(b[:-1], c[:-1]), _rel(b[-1], c[-1]))
    pairs = {"wgrad": (e_k, e_t)}
    if cin > 1:
        pairs["dx"] = (_rel(frag_to_nat(dx_frag), dx64), _rel(dx32, dx64))
    _check("G", "h %d, cin %d, %d windows" % (h, cin, npad), pairs)


# ------------------------------------------------------------------------------------------------ H. the whole step
@pytest.mark.parametrize("geo,label", [((96, 48, 2, 1), "W3"), ((112, 0, 2, 0), "W2")])
def test_anysize_step_with_dropout_matches_float64(geo, label):
    """Loss and every gradient of AnySizeTrainStep at keep_prob 0.8, masks drawn in the kernels and the same masks given as
    tensors, against the float64 graph under those masks.  (96, 48, 2, 1) at C + 1 tiles: 3 waves in both recurrences, conv
    units of 145 rows and 48 columns, BN backward over C + 1 tiles, the head with 5 windows of padding; the plain RNN
    (112, 0, 2, 0) at C / 2 + 1 tiles: 2 waves, h' through y, layer 0 on the one signal feature."""
    import torch
    from catfish_amd.training import Trainer, TorchResNetRNN
    h, c, n_layers, n_blocks = geo
    sizes = dict(layer_size=h, n_layers=n_layers, n_layers_res=n_blocks)
    if n_blocks:
        sizes["layer_size_res"] = c
    w = oracle.random_weights(seed=13, **sizes)
    tr = Trainer(w, n_layers, n_blocks, "RMSProp", 1e-3, keep_prob=0.8, device="cuda", native=True, seed=11, use_graph=False)
    try:
        assert type(tr.step_impl).__name__ == "AnySizeTrainStep"
        _assert_regime(tr.engine, h, label)
        n = _windows(label, tr.engine.launch_regimes()["n_cu"])
        rng = np.random.default_rng(n)
        x = rng.normal(0, 1.2, size=(n, T)).astype(np.float32)
        y = np.repeat((rng.random(n) < 0.4)[:, None], T, axis=1).astype(np.float32)
        masks = tr.step_impl.dropout_scales(n)
        assert abs(np.mean([m.mean() for m in masks.values()]) - 0.8) < 0.01
        loss_k, grads_k = tr.gradients(x, y)                       # masks drawn inside the kernels
        loss_m, grads_m = tr.gradients(x, y, masks=masks)          # the same masks as the scale operand
        ref = TorchResNetRNN(w, n_layers, n_blocks, device="cuda", dtype=torch.float64)
        loss64 = ref.loss(x, y, keep_prob=0.8, masks=masks)
        loss64.backward()
        l64 = float(loss64.detach())

        def grad_errors(grads):
            errs = {k: _rel(torch.as_tensor(grads[k], device=p.device), p.grad) for k, p in ref.trainable().items()}
            assert sorted(errs) == sorted(grads)
            worst = max(errs, key=errs.get)
            return errs[worst], worst

        e_loss_t = e_grads_t = None
        if _measuring():
            yard = TorchResNetRNN(w, n_layers, n_blocks, device="cuda")
            loss_t = yard.loss(x, y, keep_prob=0.8, masks=masks)
            loss_t.backward()
            e_loss_t = abs(float(loss_t.detach()) - l64)
            e_grads_t, worst_t = grad_errors({k: p.grad for k, p in yard.trainable().items()})
            print("worst gradient of float32 torch: %s" % worst_t)
        for path, loss, grads in (("in-kernel masks", loss_k, grads_k), ("mask tensors", loss_m, grads_m)):
            e_grads_k, worst_k = grad_errors(grads)
            print("worst gradient of the kernels: %s" % worst_k)
            _check("H", "%s, %d windows (%s), %s" % (geo, n, label, path), {"loss": (abs(loss - l64), e_loss_t), "grads": (e_grads_k, e_grads_t)})
    finally:
        tr.engine.close()
