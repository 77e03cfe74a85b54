"""Training precision "bf16x3" of the any-size recurrences against float64 (GPU).

``gen_gru_kernel<true, true>`` / ``gen_gru_bwd_kernel<true>`` (csrc/generic.hpp) evaluate the matrix products on the serial chain
of a biGRU layer -- forward ``[x | h] W_g`` and ``[x | r.h] W_c``, backward ``Wc_h^T da_c`` and ``Wg_h^T [da_r; da_u]`` -- as
``a_hi w_hi + a_lo w_hi + a_hi w_lo`` on the bf16 MFMA, from packs that ``gen_repack_x3_kernel`` splits on the device.  State,
gate activations, stash, accumulation and every GEMM over all (window, step) pairs stay fp32.

  R  ``cf_gen_repack_x3`` bit for bit against ``repack_x3_numpy`` below (the layout of include/catfish_hip.h restated on the
     fp32 bit patterns; tests/test_anysize_train_x3_host.py works one example by hand), forward and transposed packs, the
     destination pre-filled with 0xFF bytes: every slot written, padding tiles exactly zero.
  F  one layer through ``anysize_bigru(..., precision="bf16x3")`` against ``bigru_layer`` in float64: y, dx and the eight
     weight gradients per tensor, y and dx also per window.  Layer sizes 16 .. 256 cover the two-chain dot, the remainders of
     the groups of four, every padding of the h and transposed segments, ``h_via_y`` and the four-wave class; inputs of 16
     (three padding tiles), 2h, 1 and 80 features; window counts of one window, three tiles, two waves and the two launches at
     exactly 160 KB.  Each case asserts its launch regime and that y is NOT bit-equal to the fp32 call's: the mode ran.
  H  loss and every gradient of ``Trainer.gradients`` at keep_prob 0.8 with the masks passed in, against the float64 network
     under those masks: (96, 48, 2, 1) on the native and the autograd path, the plain RNN (112, 0, 2, 0) on the native one.
  S  ten Adam steps under graph replay at 128 / 64 (2 + 1), both paths, against the pure-torch fp32 trainer; the split packs
     after step 10 against a fresh repack of ``packed``; ``use_graph=False`` bit for bit.

Bounds of F and H.  The rule of tests/test_anysize_train_fp64.py with one more term.  A measuring run (CATFISH_PARITY_LOG names a
file) records three errors against exact float64 for every quantity, ``max|d| / max|ref|`` per tensor (the loss: absolute): the
kernels', the float32 torch restatement's, and that of a float64 EMULATION OF THE SCHEME -- ``emulated_bigru_layer``: ``bigru_layer``
with every product of the recurrence replaced by ``x3_product``, whose forward is ``a_hi w_hi + a_lo w_hi + a_hi w_lo`` in float64
(hi = bf16(float32(v)), lo = bf16(float32(v) - hi), the weights split after the exp2 pre-scaling, as the kernels see them) and
whose backward applies the same split product to the state columns only (g against W_h^T, unscaled, as the transposed pack) and
is exact for the input columns and the weight gradient.  The kernels carry both the scheme and fp32 accumulation, so the
yardstick of a quantity is the emulation's error PLUS the float32 restatement's; the asserted bound is 4 x the largest yardstick
over the section, never looser than the older bounds (2e-4 relative, loss 1e-5 absolute).  The triples are in
profiles/anysize_train_x3_parity.jsonl; ``BOUNDS`` holds the constants and tests/test_anysize_train_x3_host.py checks them against
that file.  An ordinary run computes the kernels' errors only and prints the other two as null.

As measured (MI355X, 256 CUs) every quantity meets the rule, none falls back to the older bound: F y 9.89e-5 (per window 1.02e-4),
dx 4.03e-5 (per window 4.96e-5), weight gradients 6.58e-5; H loss 1.95e-7 absolute, gradients 5.44e-5.  The kernels sit on the
emulation: for y and the step's gradients their error is 0.96 .. 1.04 x the emulation's of the same case, for dx 0.91 .. 1.11 x
(y 2.365e-5 against 2.354e-5 at 112 units and 224 inputs), and never above 1.01 x the case's yardstick: what separates them from
float64 is the scheme, not its implementation.  The two
thinner margins: the weight gradients of one layer reach 1.56 x their case's yardstick (80 units, 14 347 windows: library GEMMs
over 502 145 positions) and the step's loss 2.1 x (1.03e-7 against 3.2e-8 + 1.6e-8 at (96, 48, 2, 1), about two float32 ulps of a
loss near 0.7), both inside the factor of 4.  The runs are deterministic; if a reordering of sums trips one, re-measure, do not
widen by hand.  The longest case is the native step at (96, 48, 2, 1), 4 s in the measuring run that builds the float32
yardstick's convolution kernels, under 1 s otherwise; the layer cases take 0.1 .. 1.5 s.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
import test_anysize_train_fp64 as fp64_cases
from test_anysize_train_fp64 import _assert_regime, _layer_params, _windows
from test_train_kernels_fp64 import GRU_KEYS, GRU_PRE, T, _measuring, _rel, _rel_window, _stamp, bigru_layer, stacked_loss  # noqa: F401

pytestmark = pytest.mark.gpu

# 32 units is not among the float64 cases of the fp32 kernels: three state arrays, 8 waves forward and backward (8 x 4 x 2 KB)
fp64_cases.CLASSES.setdefault(32, (3, 8, 8))

# quantity -> asserted bound = min(4 x largest (emulation + float32-torch) error over the section, older bound)
# The largest yardsticks in profiles/anysize_train_x3_parity.jsonl (MI355X, 256 CUs) as emulation + float32-torch, and the kernels'
# largest error next to them:
#   F.y 2.354e-05 + 1.19e-06 (kernels 2.365e-05)   F.y_window 2.434e-05 + 1.23e-06 (2.446e-05)   F.dx 9.90e-06 + 2.0e-07 (9.77e-06)
#   F.dx_window 1.202e-05 + 4.0e-07 (1.199e-05)   F.wgrad 1.07e-05 + 5.7e-06 (1.240e-05)   H.loss 3.24e-08 + 1.65e-08 (1.03e-07)
#   H.grads 1.287e-05 + 7.5e-07 (1.287e-05)
# 4 x each sum, rounded down, is below the older bound of its quantity (2e-4; loss 1e-5 absolute), so it is the bound.
BOUNDS = {
    "F.y": 9.89e-5, "F.y_window": 1.02e-4, "F.dx": 4.03e-5, "F.dx_window": 4.96e-5, "F.wgrad": 6.58e-5,
    "H.loss": 1.95e-7, "H.grads": 5.44e-5,
}
OLDER_BOUNDS = {"F.y": 2e-4, "F.y_window": 2e-4, "F.dx": 2e-4, "F.dx_window": 2e-4, "F.wgrad": 2e-4, "H.loss": 1e-5, "H.grads": 2e-4}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "anysize_train_x3_parity.jsonl")
SLAB = 2048
LOG2E = 1.4426950408889634


def bounds_from_profile(path=PROFILE):
    """{quantity: min(4 x largest (emulation + float32-torch) error in the profile, older bound)}: what ``BOUNDS`` may not exceed."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            key = "%s.%s" % (row["section"], row["quantity"])
            worst[key] = max(worst.get(key, 0.0), row["emulation"] + row["torch_fp32"])
    return {k: min(4.0 * v, OLDER_BOUNDS[k]) for k, v in worst.items()}


def _record(section, case, quantity, kernel, torch_fp32, emulation):
    row = {"section": section, "case": case, "quantity": quantity, "kernel": float(kernel),
           "torch_fp32": None if torch_fp32 is None else float(torch_fp32), "emulation": None if emulation is None else float(emulation)}
    print("parity %s" % json.dumps(row))
    path = os.environ.get("CATFISH_PARITY_LOG")
    if path and torch_fp32 is not None and emulation is not None:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(_stamp(), **row)) + "\n")


def _check(section, case, triples):
    """triples: {quantity: (kernel error, float32-torch error, emulation error)}.  All are recorded, then all are asserted."""
    for q, (k, t, e) in triples.items():
        _record(section, case, q, k, t, e)
    bad = {q: (k, BOUNDS["%s.%s" % (section, q)]) for q, (k, _, _) in triples.items() if not k <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ the repack layout, in numpy
def bf16_bits(v):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even on the fp32 bit pattern (finite values)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def x3_pad(k):
    return (k + 3) & ~3


def repack_x3_numpy(src, segments):
    """src float32 [rows][sum(segments)][64][4], an A-fragment pack whose K axis is the concatenation of ``segments`` (tile
    counts) -> uint16 [rows][sum(x3_pad(k))][64][8]: per segment, pair p takes source tiles a = 2p, b = 2p + 1 (zeros past k);
    per lane hi = bf16(a[0..3] | b[0..3]) goes to slot 2p and lo = bf16(v - hi) to slot 2p + 1 of the padded segment."""
    rows = src.shape[0]
    assert src.shape[1:] == (sum(segments), 64, 4)
    out, k_off = [], 0
    for k in segments:
        kp = x3_pad(k)
        seg = np.zeros((rows, kp, 64, 4), np.float32)
        seg[:, :k] = src[:, k_off:k_off + k]
        k_off += k
        dst = np.zeros((rows, kp, 64, 8), np.uint16)
        for p in range(kp // 2):
            v = np.concatenate([seg[:, 2 * p], seg[:, 2 * p + 1]], axis=-1)
            hi = bf16_bits(v)
            dst[:, 2 * p] = hi
            dst[:, 2 * p + 1] = bf16_bits(v - bf16_value(hi))
        out.append(dst)
    return np.concatenate(out, axis=1)


@pytest.fixture(scope="module")
def engine():
    from catfish_amd.engine import HipEngine
    geo = dict(layer_size=16, n_layers=1, layer_size_res=16, n_layers_res=1)
    eng = HipEngine(oracle.random_weights(seed=41, **geo), device=0, max_windows_per_pass=256, **geo)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------ R. the repack kernel
@pytest.mark.parametrize("h,cin", [(16, 1), (16, 16), (48, 80), (80, 160), (112, 1), (256, 512)])
def test_repack_kernel_matches_the_layout_bit_for_bit(engine, h, cin):
    """cf_gen_repack_x3 on the packs ``pack_maps`` gathers from Glorot weights (both signs, normal range; the zero rows of an
    input padded to 16 features, -0.0 where the gate scale is negative), destination pre-filled with 0xFF bytes."""
    import torch
    from catfish_amd import _native as N
    from catfish_amd.anysize_train import pack_maps, x3_pack_floats
    lib, hd = engine._lib, engine._handle
    h16, kbx = h // 16, (cin + 15) // 16
    w_idx, w_scale, _, _, wt_idx = pack_maps(h, cin, "cuda")
    p_np = _layer_params(h, cin, seed=3 * h + cin)
    srcs = [torch.cat([torch.from_numpy(np.ascontiguousarray(a)).reshape(-1) for a in (p_np[4 * d], p_np[4 * d + 2], p_np[4 * d + 1], p_np[4 * d + 3])] +
                      [torch.zeros(1)]).cuda() for d in range(2)]
    wpack = torch.stack([s[w_idx] * w_scale for s in srcs]).contiguous()
    wtpack = torch.stack([s[wt_idx] for s in srcs]).contiguous()
    nw, nt = x3_pack_floats(lib, h, kbx)
    assert nw == 6 * h16 * (x3_pad(kbx) + x3_pad(h16)) * 256 and nt == 2 * h16 * (x3_pad(h16) + x3_pad(2 * h16)) * 256
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_w = torch.full((nw,), -1, dtype=torch.int32, device="cuda").view(torch.float32)          # 0xFF bytes
    out_t = torch.full((nt,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    N.check(lib.cf_gen_repack_x3(hd, h, kbx, 0, N._p(wpack), N._p(out_w), stream))
    N.check(lib.cf_gen_repack_x3(hd, h, kbx, 1, N._p(wtpack), N._p(out_t), stream))
    torch.cuda.synchronize()
    src_w = wpack.cpu().numpy().reshape(6 * h16, kbx + h16, 64, 4)
    assert np.isfinite(src_w).all() and (src_w < 0).any() and (src_w > 0).any()
    tiny = np.abs(src_w[src_w != 0]).min()
    assert tiny > 1e-30                                           # no subnormals, in the source or in its lo parts
    if cin == 1:                                                  # the zero rows of the input padded to 16 features
        assert (src_w[:, 0, 16:] == 0).all() and (src_w[:, 0, :16, 1:] == 0).all() and (src_w[:, 0, :16, 0] != 0).all()
    want_w = repack_x3_numpy(src_w, (kbx, h16))
    got_w = out_w.cpu().numpy().view(np.uint16).reshape(want_w.shape)
    assert np.array_equal(got_w, want_w)
    for k, off in ((kbx, 0), (h16, x3_pad(kbx))):                 # padding tiles: exactly zero
        if x3_pad(k) > k + (k & 1):
            assert not got_w[:, off + k + (k & 1):off + x3_pad(k)].any()
    src_t = wtpack.cpu().numpy().reshape(2, 3 * h16 * h16, 64, 4)
    want_t = np.concatenate([np.concatenate([repack_x3_numpy(src_t[d, :h16 * h16].reshape(h16, h16, 64, 4), (h16,)).reshape(-1),
                                             repack_x3_numpy(src_t[d, h16 * h16:].reshape(h16, 2 * h16, 64, 4), (2 * h16,)).reshape(-1)])
                             for d in range(2)])
    got_t = out_t.cpu().numpy().view(np.uint16)
    assert got_t.shape == want_t.shape and np.array_equal(got_t, want_t)
    with pytest.raises(ValueError):
        N.check(lib.cf_gen_repack_x3(hd, 24, kbx, 0, N._p(wpack), N._p(out_w), stream))
    with pytest.raises(ValueError):
        N.check(lib.cf_gen_repack_x3(hd, h, 33, 0, N._p(wpack), N._p(out_w), stream))
    with pytest.raises(ValueError):
        N.check(lib.cf_gen_repack_x3(hd, h, kbx, 0, None, N._p(out_w), stream))


# ------------------------------------------------------------------------------------------------ the emulation of the scheme
def _split(v):
    """float64 -> (hi, lo) as float64: hi = bf16(float32(v)), lo = bf16(float32(v) - hi)."""
    import torch
    f = v.to(torch.float32)
    hi = f.to(torch.bfloat16).to(torch.float32)
    lo = (f - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double(), lo.double()


def _x3_matmul(a, w):
    ah, al = _split(a)
    wh, wl = _split(w)
    return ah @ wh + al @ wh + ah @ wl


_X3 = None


def x3_product(a, w, n_x, scale):
    """out = a @ w as the kernels evaluate it, in float64: a [N, n_x + H] = [input | state columns], w [n_x + H, M]."""
    global _X3
    import torch
    if _X3 is None:
        class X3Product(torch.autograd.Function):
            @staticmethod
            def forward(ctx, a, w, n_x, scale):
                sc = float(np.float32(scale))                       # the packs are scaled in float32, then split
                ws = (w.to(torch.float32) * torch.tensor(sc, dtype=torch.float32, device=w.device)).double()
                ctx.save_for_backward(a, w)
                ctx.n_x = n_x
                return _x3_matmul(a, ws) / sc

            @staticmethod
            def backward(ctx, g):
                a, w = ctx.saved_tensors
                n_x = ctx.n_x
                da = torch.cat([g @ w[:n_x].t(), _x3_matmul(g, w[n_x:].t().contiguous())], 1)     # exact for x, split for the state
                return da, a.t() @ g, None, None
        _X3 = X3Product
    return _X3.apply(a, w, n_x, scale)


def emulated_bigru_layer(x, params8):
    """``bigru_layer`` (tests/test_train_kernels_fp64.py) in float64 with the kernels' split products on the serial chain."""
    import torch
    n, t_len, cin = x.shape
    outs = []
    for d, steps in ((0, range(t_len)), (1, range(t_len - 1, -1, -1))):
        wg, bg, wc, bc = params8[4 * d:4 * d + 4]
        hsz = wc.shape[1]
        h = x.new_zeros(n, hsz)
        seq = [None] * t_len
        for s in steps:
            g = torch.sigmoid(x3_product(torch.cat([x[:, s], h], 1), wg, cin, -LOG2E) + bg)
            r, u = g[:, :hsz], g[:, hsz:]
            c = torch.tanh(x3_product(torch.cat([x[:, s], r * h], 1), wc, cin, 2.0 * LOG2E) + bc)
            h = u * h + (1 - u) * c
            seq[s] = h
        outs.append(torch.stack(seq, 1))
    return torch.cat(outs, 2)


def test_emulation_is_the_exact_layer_up_to_the_scheme():
    """With operands that bf16 holds exactly in hi + lo the emulation IS ``bigru_layer``; with Glorot weights it differs from it
    by the scheme's error and no more (a few 1e-6 at most: three bf16 products keep 16 bits of each operand)."""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(5)
    p_np = _layer_params(48, 16, seed=9)
    ps = [torch.tensor(p, dtype=torch.float64, device="cuda", requires_grad=True) for p in p_np]
    x = (torch.randn(7, T, 16, generator=gen, device="cuda", dtype=torch.float32) * 1.2).double().requires_grad_(True)
    g = torch.randn(7, T, 96, generator=gen, device="cuda", dtype=torch.float64)
    y0, y1 = bigru_layer(x, ps), emulated_bigru_layer(x, ps)
    g0, g1 = torch.autograd.grad(y0, [x] + ps, g), torch.autograd.grad(y1, [x] + ps, g)
    errs = [_rel(y1, y0)] + [_rel(a, b) for a, b in zip(g1, g0)]
    assert 1e-9 < max(errs) < 5e-5, errs
    hi, lo = _split(torch.tensor([1.00390625, -3.0, 0.0], dtype=torch.float64))
    assert hi.tolist() == [1.0, -3.0, 0.0] and lo.tolist() == [0.00390625, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ F. one layer
SIZES = (16, 32, 48, 80, 96, 112, 176, 256)
F_CASES = ([(label, h, cin) for label in ("1", "43") for h in SIZES for cin in (16, 2 * h)] +
           [(label, h, cin) for label in ("1", "43") for h, cin in ((112, 1), (48, 80))] +
           [("W2", h, 16) for h in (16, 112, 256)] +
           [("W8", h, 16) for h in (80, 160)])


@pytest.mark.parametrize("label,h,cin", F_CASES)
def test_anysize_bigru_layer_bf16x3_matches_float64(engine, label, h, cin):
    """y, dx and the eight weight gradients of one layer on gen_gru_kernel<true, true> / gen_gru_bwd_kernel<true> against
    ``bigru_layer`` in float64; the float32 restatement and the emulation of the scheme next to them in a measuring run."""
    import torch
    from catfish_amd.anysize_train import anysize_bigru
    _assert_regime(engine, h, label)
    n = _windows(label, engine.launch_regimes()["n_cu"])
    p_np = _layer_params(h, cin, seed=1000 * h + cin)
    gen = torch.Generator(device="cuda").manual_seed(100000 * h + 100 * cin + n)
    x32 = torch.randn(n, T, cin, generator=gen, device="cuda", dtype=torch.float32) * 1.2
    g32 = torch.randn(n, T, 2 * h, generator=gen, device="cuda", dtype=torch.float32)

    def reference(dtype, layer=bigru_layer):
        ps = [torch.tensor(p, dtype=dtype, device="cuda", requires_grad=True) for p in p_np]
        ys, dxs, gw = [], [], [torch.zeros(p.shape, dtype=torch.float64, device="cuda") for p in p_np]
        for a in range(0, n, SLAB):
            x = x32[a:a + SLAB].to(dtype).requires_grad_(True)
            y = layer(x, ps)
            grads = torch.autograd.grad(y, [x] + ps, g32[a:a + SLAB].to(dtype))
            ys.append(y.detach())
            dxs.append(grads[0])
            for acc, g in zip(gw, grads[1:]):
                acc += g.double()
        return torch.cat(ys), torch.cat(dxs), gw

    def kernels(precision):
        x = x32.clone().requires_grad_(True)
        ps = [torch.tensor(p, dtype=torch.float32, device="cuda", requires_grad=True) for p in p_np]
        y = anysize_bigru(x, ps, engine, precision=precision)
        grads = torch.autograd.grad(y, [x] + ps, g32)
        return y.detach(), grads[0], grads[1:]

    y64, dx64, gw64 = reference(torch.float64)
    y_k, dx_k, gw_k = kernels("bf16x3")
    y_f = kernels("fp32")[0]
    assert y_k.shape == (n, T, 2 * h) and dx_k.shape == (n, T, cin)
    assert not torch.equal(y_k, y_f)                                  # the split products ran
    errors = lambda y, dx, gw: (_rel(y, y64), _rel_window(y, y64), _rel(dx, dx64), _rel_window(dx, dx64),          # noqa: E731
                                max(_rel(a, b) for a, b in zip(gw, gw64)))
    e_k = errors(y_k, dx_k, gw_k)
    e_t = e_e = (None,) * 5
    if _measuring():
        e_t = errors(*reference(torch.float32))
        e_e = errors(*reference(torch.float64, emulated_bigru_layer))
    _check("F", "h %d, cin %d, %d windows (%s)" % (h, cin, n, label),
           dict(zip(("y", "y_window", "dx", "dx_window", "wgrad"), zip(e_k, e_t, e_e))))


# ------------------------------------------------------------------------------------------------ H. the whole step
def _emulated_loss(net, x, y, keep_prob, masks):
    """``stacked_loss`` with the emulated layers and the output dropout of TorchResNetRNN under ``masks`` (float64)."""
    import torch
    p = net.params
    a = torch.as_tensor(x, dtype=net.dtype, device=net.device)[:, None, :]
    for d in range(net.n_layers_res):
        sc = net._conv_bn(a, 4 * d)
        o = torch.relu(net._conv_bn(a, 4 * d + 1))
        o = torch.relu(net._conv_bn(o, 4 * d + 2))
        o = torch.relu(net._conv_bn(o, 4 * d + 3))
        a = torch.relu(o + sc)
    a = a.permute(0, 2, 1)
    for layer in range(net.n_layers):
        a = emulated_bigru_layer(a, [p[(GRU_PRE % (layer, d)) + k] for d in ("fw", "bw") for k in GRU_KEYS])
        m = torch.cat([torch.as_tensor(masks[(layer, d)], dtype=net.dtype, device=net.device) for d in ("fw", "bw")], 2)
        a = a / keep_prob * m
    z = a.reshape(-1, a.shape[2]) @ p["final_fully_connected/kernel"] + p["final_fully_connected/bias"]
    yt = torch.as_tensor(y, dtype=net.dtype, device=net.device).reshape(-1, 1)
    return torch.nn.functional.binary_cross_entropy_with_logits(z, yt, reduction="mean")


@pytest.mark.parametrize("geo,label,native", [((96, 48, 2, 1), "43", True), ((96, 48, 2, 1), "43", None), ((112, 0, 2, 0), "W2", True)])
def test_step_bf16x3_with_dropout_matches_float64(geo, label, native):
    """Loss and every gradient of ``Trainer(..., precision="bf16x3").gradients`` at keep_prob 0.8 under given masks against the
    float64 network under those masks: the whole native step (AnySizeTrainStep) and the autograd path around the recurrences."""
    import torch
    from catfish_amd.training import Trainer, TorchResNetRNN
    h, c, n_layers, n_blocks = geo
    sizes = dict(layer_size=h, n_layers=n_layers, n_layers_res=n_blocks)
    if n_blocks:
        sizes["layer_size_res"] = c
    w = oracle.random_weights(seed=13, **sizes)
    tr = Trainer(w, n_layers, n_blocks, "RMSProp", 1e-3, keep_prob=0.8, device="cuda", native=native, seed=11, use_graph=False,
                 precision="bf16x3")
    try:
        assert (type(tr.step_impl).__name__ == "AnySizeTrainStep") if native else (tr.anysize and tr.step_impl is None)
        assert tr.precision == "bf16x3" and tr.net.precision == "bf16x3"
        _assert_regime(tr.engine, h, label)
        n = _windows(label, tr.engine.launch_regimes()["n_cu"])
        rng = np.random.default_rng(n)
        x = rng.normal(0, 1.2, size=(n, T)).astype(np.float32)
        y = np.repeat((rng.random(n) < 0.4)[:, None], T, axis=1).astype(np.float32)
        masks = {(layer, d): (rng.random((n, T, h)) < 0.8).astype(np.float32) for layer in range(n_layers) for d in ("fw", "bw")}
        loss_k, grads_k = tr.gradients(x, y, masks=masks)
        ref = TorchResNetRNN(w, n_layers, n_blocks, device="cuda", dtype=torch.float64)
        loss64 = ref.loss(x, y, keep_prob=0.8, masks=masks)
        loss64.backward()
        l64 = float(loss64.detach())

        def grad_errors(grads):
            errs = {k: _rel(torch.as_tensor(grads[k], device=p.device), p.grad) for k, p in ref.trainable().items()}
            assert sorted(errs) == sorted(grads)
            return max(errs.values())

        e_t = e_e = (None, None)
        if _measuring():
            yard = TorchResNetRNN(w, n_layers, n_blocks, device="cuda")
            loss_t = yard.loss(x, y, keep_prob=0.8, masks=masks)
            loss_t.backward()
            e_t = (abs(float(loss_t.detach()) - l64), grad_errors({k: p.grad for k, p in yard.trainable().items()}))
            emu = TorchResNetRNN(w, n_layers, n_blocks, device="cuda", dtype=torch.float64)
            loss_e = _emulated_loss(emu, x, y, 0.8, masks)
            loss_e.backward()
            e_e = (abs(float(loss_e.detach()) - l64), grad_errors({k: p.grad for k, p in emu.trainable().items()}))
        _check("H", "%s, %d windows (%s), native=%s" % (geo, n, label, native),
               {"loss": (abs(loss_k - l64), e_t[0], e_e[0]), "grads": (grad_errors(grads_k), e_t[1], e_e[1])})
    finally:
        tr.engine.close()


# ------------------------------------------------------------------------------------------------ S. steps under graph replay
def test_ten_adam_steps_bf16x3_under_graph_replay():
    """128 / 64 (2 + 1) at 64 windows: the autograd path and the native step with ``precision="bf16x3"`` follow the pure-torch
    fp32 trainer's losses (the tolerance of test_trainer_uses_the_any_size_kernels_for_other_geometries); the native step's
    split packs after step 10 are a fresh repack of its fp32 packs, bit for bit; without the graph, the same ten losses."""
    import torch
    from catfish_amd.training import Trainer
    w = oracle.random_weights(seed=5, layer_size=128, n_layers=2, layer_size_res=64, n_layers_res=1)
    rng = np.random.default_rng(0)
    batches = [(rng.normal(0, 1.0, size=(64, 35)).astype(np.float32), np.repeat((rng.random(64) < 0.5)[:, None], 35, axis=1).astype(np.float32))
               for _ in range(10)]
    mk = lambda **kw: Trainer(w, 2, 1, "Adam", 1e-3, 1.0, seed=1, **kw)      # noqa: E731
    auto, nat, eager, ref = mk(precision="bf16x3"), mk(native=True, precision="bf16x3"), mk(native=True, precision="bf16x3", use_graph=False), mk(native=False)
    try:
        assert auto.anysize and auto.use_graph and nat.use_graph and type(nat.step_impl).__name__ == "AnySizeTrainStep"
        losses = {name: [t.train_step(x, y) for x, y in batches] for name, t in (("auto", auto), ("nat", nat), ("eager", eager), ("ref", ref))}
        print("losses %s" % json.dumps(losses))
        assert nat._graph is not None and auto._graph is not None and eager._graph is None
        for name in ("auto", "nat"):
            got = losses[name]
            assert np.isfinite(got).all() and got[-1] < got[0]
            assert np.allclose(got, losses["ref"], rtol=0, atol=2e-3), (name, got, losses["ref"])
        assert losses["eager"] == losses["nat"]
        step = nat.step_impl
        torch.cuda.synchronize()
        stale = step.packed_x3.clone()
        fresh = torch.full((stale.numel(),), -1, dtype=torch.int32, device=stale.device).view(torch.float32)
        step.walk.repack_x3(step.packed, fresh, step._stream())
        torch.cuda.synchronize()
        assert torch.equal(stale.view(torch.int32), fresh.view(torch.int32))
    finally:
        for t in (auto, nat, eager):
            t.engine.close()
