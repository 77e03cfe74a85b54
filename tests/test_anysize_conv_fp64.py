"""The any-size conv, head and operator-backward kernels against float64, kernel by kernel (GPU).

csrc/gen_train.hpp holds the GEMM-shaped and element-wise kernels around the any-size recurrences; tests/test_anysize_train_fp64.py
(section G) calls two of its entry points directly, the others were reached only through whole networks at 2e-4 of a tensor's
maximum.  Here every other one runs alone, on planes this module builds, at the smallest shapes at which each guard of the 64 x 64
tiles (``m < M``, ``n < N``, ``k < k1``), each chunk of the weight gradients and each gate is live:

  I  conv units as (kw, cin, cout, windows), ``I_CASES``: ``cf_gen_conv_forward`` (ReLU off / on, without and with a shortcut
     plane: z, y per tensor and per window, y also on steps 0 and 34 alone, where a tap that leaks across a window edge shows:
     the neighbouring windows hold data), ``cf_gen_conv_backward_data`` (``add`` null, a plane of its own, ``add == dx`` in
     place; cin 1 is refused), ``cf_gen_bn_backward`` / ``cf_gen_bn_backward_data`` (ReLU off / on, mask null / given, channels
     with gamma 0 and beta > 0, negative gamma, moving variance 0: dz per tensor and per window, d gamma, d beta, every other slot
     of the gradient buffer bit-identical, both entry points the same dz bit for bit), ``cf_gen_conv_wgrad`` (kernel rows and
     bias row each over its own maximum).
  J  ``cf_gen_head``: 16 / 96 / 224 / 512 features, 16 / 48 windows of which 0, 5 or 15 are padding: logits, d input, d logit,
     loss, dense gradients; exact zeros and the pre-fill in the padding windows; one case with logits past +-80.
  K  ``cf_gen_head_backward``, ``cf_gen_signal_grad`` (both network types), ``cf_gen_bn_stat_grads``.
  exact sections (no bound, bit equality): ``cf_gen_x_frag``, ``cf_gen_dropout`` with a scale plane, and with its own hash
     against ``drop_scale_plane``, a numpy restatement of ``cf_drop_key`` / ``cf_drop_scale4`` from their comments.

References.  Every operation is written out below in torch on natural-layout tensors [windows, 35, features]: the taps as shifted
matrix products (pad, slice, ``@``), no library convolution.  The same function runs in float64 (the reference) and in float32 (the
yardstick); each takes ``departure=``, a named way of being subtly wrong, which tests/test_anysize_conv_host.py uses on the CPU to
show that the measures and bounds of this module see it.  Inputs come from seeded CPU generators, so that file sees the very
planes of the GPU run.  The discontinuous gates are inputs of the kernels under test: ``settle`` moves every z whose float64
``|z s + t|`` is below 1e-3 to 2e-3 with its sign (fewer than 1 % of the elements, asserted), mask planes hold positive values,
+0.0, -0.0 and negative values.  Outputs and workspaces are NaN before every launch.

Bounds.  As in tests/test_anysize_train_fp64.py: every case records the kernels' error and the float32 yardstick's against
float64 (``max|d| / max|ref|`` per tensor; the loss: ``|d| / max(1, |ref|)``; ``K.dstat``: per element, an exact zero where the
reference is one), the asserted bound of a quantity is 4 x the largest yardstick over its section, rounded down to three digits,
never looser than ``OLDER_BOUNDS`` (2e-4, loss 1e-5).  ``I.y`` is the larger of y over the tensor and y on steps 0 and 34,
``I.y_window`` the larger of z and y per window.  profiles/anysize_conv_fp64_parity.jsonl holds one measuring run, ``BOUNDS`` the
constants, tests/test_training.py checks the one against the other.

The summation-order term.  Five quantities missed the rule with float32 torch alone, by 1.2 to 3.6 x their would-be bounds: the
head's logit (11 x its case's yardstick at 512 features), the dense gradients of both heads (21 x and 7 x), d gamma / d beta (18 x)
and the signal gradient (14 x at 256 units).  In each the kernel sums in ONE float32 chain -- ``gt_head_kernel`` over the features,
``gt_tile`` with a single output column over the 1120 positions of a chunk, ``gt_bn_bwd_kernel`` over the 560 positions of a
tile, ``gt_signal_grad_kernel`` over up to 1536 products -- where float32 torch sums in a tree or across many lanes: a property of
the arithmetic, not a defect (the GEMMs with many columns, whose yardstick is a library GEMM with chains of its own, meet the rule
as they are).  So those quantities, ``CHAIN_TERM``, carry a second yardstick term: the error against float64 of that one step
evaluated in float32 in the kernel's order (``chain_dot``, ``chain_wgrad``, ``_chain_sums``, ``chain_pairs``: fmaf as an exact
float64 product and sum rounded once, from the float64 reference's operands rounded to float32), recorded as ``chain`` in every
row (null for the quantities without such a sum).  The emulation lands on the kernels: at every logit and signal gradient
case and in 25 of the 40 BN rows the two errors agree to 1 %; the dense gradients' differ more (the kernels sum over their own
d logit), the kernels' at most 1.75 x the emulation's.  The largest is d gamma at (1, 64, 80, 16), 6.6e-6: the
zero-variance channel's terms reach 312 and its partial sums thousands while its sum is -30 and the tensor's maximum 88.
No case forced a change to csrc/gen_train.hpp.

As measured (MI355X, 256 CUs) no quantity fell back to the older bound: I z 2.66e-6, y 2.52e-6 (per window 3.39e-6), dx 2.58e-6,
dz 6.69e-7 (per window 6.69e-7), d gamma / d beta 2.99e-5, weight gradients 7.83e-6; J logits 5.00e-6, d input 3.81e-6, d logit
3.78e-6, loss 3.45e-7, dense gradients 1.77e-5; K d input 6.86e-7, d logit 6.65e-7, dense gradients 6.76e-6, signal gradient
6.83e-6, statistics gradients 8.96e-7: 6.7 to 300 x tighter than 2e-4, the loss 29 x tighter than 1e-5.  The two thinnest margins: K's d logit at 0.62 of its bound
and d input at 0.59 (4.11e-7 and 4.06e-7, both the head backward at 512 features, 48 windows, 33 real: the logit's chain of 512
products, which these two quantities inherit without the term); next I's dx at 0.45 ((3, 256, 256, 16): gt_tile's chain of 768).
Case by case the kernels reach 4.6 x their case's yardstick in the loss (512 features, 33 of 48 windows: 7.6e-8 against 1.7e-8, about
one ulp of a loss near 0.8), 4.0 x in J's d logit and 3.3 x in its d input, 3.5 x and 3.1 x in K's, 2.4 to 2.6 x in the GEMMs of I (z, y, dx,
weight gradients), 1.3 x at most where the chain term is part of the yardstick, 1.0 x in dz and 0.63 x in the statistics gradients.
The runs are deterministic; if a reordering of sums trips a bound, re-measure, do not widen by hand.  A case takes 0.01 to 0.2 s,
the module 7 s.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from test_train_kernels_fp64 import T, _measuring, _rel, _rel_window, _stamp      # noqa: F401

pytestmark = pytest.mark.gpu

# quantity -> asserted bound = min(4 x largest yardstick over the section, older bound).  The largest yardsticks in
# profiles/anysize_conv_fp64_parity.jsonl (MI355X, 256 CUs; float32 torch, + the chain term where ``CHAIN_TERM`` names the quantity),
# and the kernels' largest error next to them:
#   I.z 6.663e-07 (kernels 9.72e-07)   I.y 6.313e-07 (9.52e-07)   I.y_window 8.500e-07 (1.31e-06)   I.dx 6.463e-07 (1.16e-06)
#   I.dz 1.674e-07 (1.09e-07)   I.dz_window 1.674e-07 (1.16e-07)   I.bn 7.492e-06 (6.59e-06)   I.wgrad 1.960e-06 (1.27e-06)
#   J.logits 1.250e-06 (1.15e-06)   J.din 9.546e-07 (1.68e-06)   J.dl 9.456e-07 (1.68e-06)   J.loss 8.636e-08 (9.20e-08)
#   J.wgrad 4.437e-06 (2.74e-06)   K.din 1.716e-07 (4.06e-07)   K.dl 1.664e-07 (4.11e-07)   K.wgrad 1.690e-06 (1.48e-06)
#   K.dsignal 1.709e-06 (1.60e-06)   K.dstat 2.241e-07 (1.40e-07)
# 4 x each of them, rounded down, is far below the older bound of its quantity (2e-4; loss 1e-5), so it is the bound.
BOUNDS = {
    "I.z": 2.66e-6, "I.y": 2.52e-6, "I.y_window": 3.39e-6, "I.dx": 2.58e-6, "I.dz": 6.69e-7, "I.dz_window": 6.69e-7, "I.bn": 2.99e-5,
    "I.wgrad": 7.83e-6,
    "J.logits": 5.00e-6, "J.din": 3.81e-6, "J.dl": 3.78e-6, "J.loss": 3.45e-7, "J.wgrad": 1.77e-5,
    "K.din": 6.86e-7, "K.dl": 6.65e-7, "K.wgrad": 6.76e-6, "K.dsignal": 6.83e-6, "K.dstat": 8.96e-7,
}
# what tests/test_anysize_native_step.py, tests/test_op_autograd.py and tests/test_gpu_pipeline.py allow for the quantity
OLDER_BOUNDS = dict({k: 2e-4 for k in BOUNDS}, **{"J.loss": 1e-5})
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "anysize_conv_fp64_parity.jsonl")
BN_EPS = 1e-3            # GT_BN_EPS
GATE_MARGIN = 1e-3       # no |BN(z)| of a case is below it: float32 and the kernels take the gates float64 takes
CHUNK_WINDOWS = 32       # GT_CHUNK_WINDOWS


# quantities whose yardstick carries the summation-order term: the kernels sum them in one float32 chain (gt_head_kernel's logit
# over the features, gt_tile's weight gradients over the 1120 positions of a chunk at one column, gt_bn_bwd_kernel's sums over the
# 560 positions of a tile, gt_signal_grad_kernel's over up to 1536 products), which float32 torch, summing in a tree or across
# many lanes, does not
CHAIN_TERM = ("I.bn", "J.logits", "J.wgrad", "K.wgrad", "K.dsignal")


def yardstick(row):
    """The yardstick of one profile row: float32 torch (+ the summation-order term where named)."""
    key = "%s.%s" % (row["section"], row["quantity"])
    return row["torch_fp32"] + (row["chain"] if key in CHAIN_TERM else 0.0)


def bounds_from_profile(path=PROFILE):
    """{quantity: min(4 x largest yardstick in the profile, older bound)}: what ``BOUNDS`` may not exceed
    (tests/test_training.py checks that on the CPU)."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            key = "%s.%s" % (row["section"], row["quantity"])
            worst[key] = max(worst.get(key, 0.0), yardstick(row))
    return {k: min(4.0 * v, OLDER_BOUNDS[k]) for k, v in worst.items()}


def _record(section, case, quantity, kernel, torch_fp32, chain):
    """Print the row (always, before any assertion) and append it to the file CATFISH_PARITY_LOG names."""
    row = {"section": section, "case": case, "quantity": quantity, "kernel": float(kernel), "torch_fp32": float(torch_fp32),
           "chain": None if chain is None else float(chain)}
    print("parity %s" % json.dumps(row))
    path = os.environ.get("CATFISH_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(_stamp(), **row)) + "\n")


def _check(section, case, kernel, yard, chain=None):
    """kernel, yard: {quantity: error} of the kernels and of the float32 yardstick; chain: {quantity: error of the float32
    emulation of the kernels' summation order} for the quantities that have one (every row carries the field, null elsewhere).
    All are recorded (printed as ``parity`` rows), then all are asserted."""
    chain = chain or {}
    assert sorted(kernel) == sorted(yard) and set(chain) <= set(kernel)
    assert all(("%s.%s" % (section, q) in CHAIN_TERM) == (q in chain) for q in kernel), (section, sorted(chain))
    for q, k in kernel.items():
        _record(section, case, q, k, yard[q], chain.get(q))
    bad = {q: (k, BOUNDS["%s.%s" % (section, q)]) for q, k in kernel.items() if not k <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ inputs (CPU generators)
def _gen(*key):
    import torch
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator().manual_seed(seed)


def _randn(gen, *shape):
    import torch
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def _rand(gen, *shape):
    import torch
    return torch.rand(*shape, generator=gen, dtype=torch.float32)


UNIT_KEYS = ("kernel", "bias", "gamma", "beta", "mean", "var")


def unit_params(gen, kw, cin, cout, special=False):
    """One conv unit as a dict of float32 tensors: kernel [kw, cin, cout], bias, gamma, beta, moving mean, moving variance.
    ``special``: channel 1 has gamma 0.0 and beta 0.25, channel 2 gamma -0.75, channel 3 moving variance 0.0."""
    u = {"kernel": _randn(gen, kw, cin, cout) / float(np.sqrt(kw * cin)), "bias": 0.1 * _randn(gen, cout),
         "gamma": 0.5 + _rand(gen, cout), "beta": 0.3 * _randn(gen, cout), "mean": 0.2 * _randn(gen, cout), "var": 0.5 + _rand(gen, cout)}
    if special:
        u["gamma"][1], u["beta"][1], u["gamma"][2], u["var"][3] = 0.0, 0.25, -0.75, 0.0
    return u


def unit_flat(u):
    """kernel | bias | gamma | beta | moving_mean | moving_variance, as the entry points take a unit."""
    import torch
    return torch.cat([u[k].reshape(-1) for k in UNIT_KEYS])


def mask_plane(gen, *shape):
    """A block output as the mask operand: 55 % positive, 15 % +0.0, 15 % -0.0, 15 % negative (the last three mean off)."""
    import torch
    r, v = _rand(gen, *shape), 0.1 + _rand(gen, *shape)
    zero = torch.zeros(shape)
    return torch.where(r < 0.55, v, torch.where(r < 0.70, zero, torch.where(r < 0.85, -zero, -v)))


def bn_affine(u, dtype, departure=None):
    """(s, t) of BN(z) = z s + t with the moving statistics constant: s = gamma / sqrt(var + eps), t = beta - mean s."""
    import torch
    gam, beta, mean, var = (u[k].to(dtype) for k in ("gamma", "beta", "mean", "var"))
    inv = 1.0 / (torch.sqrt(var) + BN_EPS) if departure == "eps_outside_root" else 1.0 / torch.sqrt(var + BN_EPS)
    s = gam * inv
    return s, beta - mean * s


def settle(z, u):
    """z (float32, [.., cout]) with every element whose float64 |z s + t| is below GATE_MARGIN moved to where it is 2 GATE_MARGIN,
    keeping its sign -> (z', fraction of elements moved).  Channels with s = 0 are left alone (their BN(z) is beta)."""
    import torch
    s, t = bn_affine(u, torch.float64)
    v = z.double() * s + t
    near = (v.abs() < GATE_MARGIN) & (s != 0)
    target = torch.where(v < 0, -2 * GATE_MARGIN, 2 * GATE_MARGIN)
    safe = torch.where(s != 0, s, torch.ones_like(s))
    z2 = torch.where(near, ((target - t) / safe).float(), z)
    assert float((z2.double() * s + t).abs().min()) >= GATE_MARGIN
    return z2, float(near.double().mean())


# (kw, cin, cout, windows)
I_CASES = [(1, 1, 16, 16),        # smallest: K = 1, M = 2 rows of the weight gradient
           (3, 1, 16, 16),        # K = 3: the ABI admits it, no model uses it
           (1, 16, 48, 16),       # cout 48
           (3, 16, 16, 48),       # 49 rows; a full chunk of positions, then a half one
           (1, 64, 80, 16),       # 65 rows: the bias row alone in its row block; two column blocks, the second partial
           (3, 64, 64, 64),       # 193 rows; two full chunks
           (3, 80, 80, 16),       # K = 240
           (1, 256, 256, 48),     # large
           (3, 256, 256, 16),     # large, K = 768
           (1, 512, 16, 16)]      # the ABI's largest cin


def conv_forward_inputs(kw, cin, cout, npad):
    """(x [npad, 35, cin], the unit, a shortcut plane [npad, 35, cout])"""
    gen = _gen(1, kw, cin, cout, npad)
    return 1.2 * _randn(gen, npad, T, cin), unit_params(gen, kw, cin, cout), _randn(gen, npad, T, cout)


def conv_dx_inputs(kw, cin, cout, npad):
    """(dz [npad, 35, cout], the unit, a plane to add [npad, 35, cin])"""
    gen = _gen(2, kw, cin, cout, npad)
    return _randn(gen, npad, T, cout), unit_params(gen, kw, cin, cout), _randn(gen, npad, T, cin)


def bn_backward_inputs(kw, cin, cout, npad):
    """(g, mask, z settled, the unit with its special channels, fraction of z moved)"""
    gen = _gen(3, kw, cin, cout, npad)
    u = unit_params(gen, kw, cin, cout, special=True)
    g, mask = _randn(gen, npad, T, cout), mask_plane(gen, npad, T, cout)
    z, moved = settle(1.5 * _randn(gen, npad, T, cout), u)
    return g, mask, z, u, moved


def conv_wgrad_inputs(kw, cin, cout, npad):
    """(x [npad, 35, cin], dz [npad, 35, cout])"""
    gen = _gen(4, kw, cin, cout, npad)
    return 1.2 * _randn(gen, npad, T, cin), _randn(gen, npad, T, cout)


def head_inputs(features, npad, n_real, reach=None):
    """(in [npad, 35, features], dense weights [features], bias [1], labels [npad, 35]: 0 / 1 per window).  ``reach``: the inputs
    are scaled so that the float64 logits of the real windows pass +-reach."""
    gen = _gen(5, features, npad, n_real)
    x, w, b = _randn(gen, npad, T, features), _randn(gen, features) / float(np.sqrt(features)), 0.1 * _randn(gen, 1)
    labels = (_rand(gen, npad) < 0.4).float()[:, None].repeat(1, T)
    if reach is not None:
        s = (x[:n_real].double().reshape(-1, features) @ w.double()) + b.double()
        x = x * float(1.02 * reach / min(float(s.max()), -float(s.min())))
    return x, w, b, labels.contiguous()


def head_backward_inputs(features, npad, n_real):
    """head_inputs without labels, and d loss / d probability [npad, 35]: of both signs, zero in the padding windows"""
    gen = _gen(6, features, npad, n_real)
    x, w, b, _ = head_inputs(features, npad, n_real)
    dprobs = 0.5 + _randn(gen, npad, T)
    dprobs[n_real:] = 0.0
    return x, w, b, dprobs


def gru_layer0_flat(gen, h):
    """Layer 0 of the plain RNN type (one input feature), flat: per direction gates kernel [1 + h, 2h] | gates bias | candidate
    kernel [1 + h, h] | candidate bias."""
    import torch
    parts = []
    for _ in range(2):
        parts += [_randn(gen, 1 + h, 2 * h) / float(np.sqrt(1 + h)), 0.1 * _randn(gen, 2 * h),
                  _randn(gen, 1 + h, h) / float(np.sqrt(1 + h)), 0.1 * _randn(gen, h)]
    return torch.cat([p.reshape(-1) for p in parts])


# ------------------------------------------------------------------------------------------------ references (any device, any dtype)
def shifted(x, d, departure=None):
    """x [N, 35, C] -> x'[n, t] = x[n, t + d], zero where t + d leaves the window (SAME padding, window by window)."""
    import torch.nn.functional as F
    n, t, c = x.shape
    if departure == "neighbour_padding":                 # the windows run on: t = -1 of window n is t = 34 of window n - 1
        flat = F.pad(x.reshape(n * t, c), (0, 0, 2, 2))
        return flat[2 + d:2 + d + n * t].reshape(n, t, c)
    return F.pad(x, (0, 0, 2, 2))[:, 2 + d:2 + d + t]


def tap_offsets(kw, departure=None):
    """The step offset of each tap: tap - (kw - 1) / 2."""
    return [tap - (kw - 1) // 2 + (1 if departure == "taps_shifted" else 0) for tap in range(kw)]


def conv_forward_ref(x, u, kw, relu, shortcut, dtype, departure=None):
    """(z, y): z = conv(x) + bias, y = BN(z), ReLU if ``relu``, then ReLU(y + shortcut) if there is one."""
    import torch
    n, t, cin = x.shape
    xd, k = x.to(dtype), u["kernel"].to(dtype)
    z = u["bias"].to(dtype)
    for tap, d in enumerate(tap_offsets(kw, departure)):
        z = z + shifted(xd, d, departure).reshape(n * t, cin) @ k[tap]
    z = z.reshape(n, t, -1)
    s, tt = bn_affine(u, dtype, departure)
    y = z * s + tt
    if relu:
        y = torch.relu(y)
    if shortcut is not None:
        y = torch.relu(y + shortcut.to(dtype))
    return z, y


def conv_dx_ref(dz, u, kw, add, dtype, departure=None):
    """dx[n, t] = sum_tap dz[n, t - offset(tap)] kernel[tap]^T (+ add)."""
    n, t, cout = dz.shape
    dzd, k = dz.to(dtype), u["kernel"].to(dtype)
    dx = 0
    for tap, d in enumerate(tap_offsets(kw)):
        dx = dx + shifted(dzd, -d).reshape(n * t, cout) @ k[tap].t()
    dx = dx.reshape(n, t, -1)
    if add is not None:
        dx = dx + add.to(dtype) * (2 if departure == "add_twice" else 1)
    return dx


def bn_gated(g, mask, relu, z, u, dtype, departure=None):
    """v = g where the mask is on (> 0; +0.0, -0.0 and negative values are off) and, with ``relu``, where BN(z) > 0; else 0."""
    import torch
    s, t = bn_affine(u, dtype)
    v = g.to(dtype)
    if mask is not None:
        on = mask > 0
        if departure == "negative_zero_on":
            on = on | ((mask == 0) & torch.signbit(mask))
        v = torch.where(on, v, torch.zeros_like(v))
    if relu:
        on = (mask > 0) if departure == "gate_from_a" else (z.to(dtype) * s + t > 0)
        v = torch.where(on, v, torch.zeros_like(v))
    return v


def bn_backward_ref(g, mask, relu, z, u, dtype, departure=None):
    """(dz, d gamma, d beta) = (v s, sum v (z - mean) / sqrt(var + eps), sum v) with v of ``bn_gated``."""
    import torch
    s, _ = bn_affine(u, dtype)
    v = bn_gated(g, mask, relu, z, u, dtype, departure)
    zhat = (z.to(dtype) - u["mean"].to(dtype)) / torch.sqrt(u["var"].to(dtype) + BN_EPS)
    cout = z.shape[-1]
    return v * s, (v * zhat).reshape(-1, cout).sum(0), v.reshape(-1, cout).sum(0)


def conv_wgrad_ref(x, dz, kw, dtype, departure=None):
    """(kernel rows [kw cin, cout], bias row [cout]) = [x at each tap | 1]^T dz over all positions."""
    import torch
    n, t, cin = x.shape
    if departure == "last_chunk_dropped":                # the positions past the last full chunk of 32 windows
        n = n // CHUNK_WINDOWS * CHUNK_WINDOWS
        x, dz = x[:n], dz[:n]
    xd, dzd = x.to(dtype), dz.to(dtype).reshape(n * t, -1)
    cols = [shifted(xd, d, departure).reshape(n * t, cin) for d in tap_offsets(kw, departure)]
    a = torch.cat(cols + [xd.new_ones(n * t, 1)], 1)
    w = a.t() @ dzd
    return w[:-1], (torch.zeros_like(w[-1]) if departure == "bias_dropped" else w[-1])


def head_ref(x, w, b, labels, n_real, dtype, departure=None):
    """Dense head with sigmoid cross-entropy over the ``n_real`` real windows: logits, d input, d logit, mean loss, dense gradients."""
    import torch
    n, t, f = x.shape
    nr = n_real - 1 if departure == "n_real_off_by_one" else n_real
    xd, wd, lab = x.to(dtype).reshape(n * t, f), w.to(dtype), labels.to(dtype).reshape(-1)
    s = xd @ wd + b.to(dtype)
    real = (torch.arange(n, device=x.device) < nr).repeat_interleave(t)
    zero = torch.zeros_like(s)
    dl = torch.where(real, (torch.sigmoid(s) - lab) / (nr * t), zero)
    lossp = torch.clamp(s, min=0) - s * lab + torch.log1p(torch.exp(-s.abs()))
    loss = torch.where(real, lossp, zero).sum() / (nr * t)
    return {"logits": s.reshape(n, t), "din": (dl[:, None] * wd).reshape(n, t, f), "dl": dl, "loss": loss, "gw": xd.t() @ dl,
            "gb": dl.sum().reshape(1)}


def head_backward_ref(x, w, b, dprobs, dtype):
    """Head backward from d loss / d probability: d logit = g p (1 - p), d input = d logit w, dense gradients."""
    import torch
    n, t, f = x.shape
    xd, wd = x.to(dtype).reshape(n * t, f), w.to(dtype)
    p = torch.sigmoid(xd @ wd + b.to(dtype))
    dl = dprobs.to(dtype).reshape(-1) * (p * (1 - p))
    return {"din": (dl[:, None] * wd).reshape(n, t, f), "dl": dl, "gw": xd.t() @ dl, "gb": dl.sum().reshape(1)}


def signal_grad_res_ref(w_sc, dz_sc, w_1, dz_1, dtype):
    """ResNetRNN: the signal feeds block 0's shortcut and first conv (kw 1, cin 1): dx = sum_o dz_sc[o] w_sc[o] + dz_1[o] w_1[o]."""
    return dz_sc.to(dtype) @ w_sc.to(dtype) + dz_1.to(dtype) @ w_1.to(dtype)


def signal_grad_rnn_ref(params, da, h, dtype, departure=None):
    """Plain RNN: the signal is row 0 of layer 0's input; da [N, 35, 6h] holds (dir, gate r / u / c, unit):
    dx = sum_dir (sum_j<2h da_ru[j] Wg[0][j] + sum_j<h da_c[j] Wc[0][j])."""
    dir_floats = (1 + h) * 3 * h + 3 * h
    dad, dx = da.to(dtype), 0
    for d in range(2):
        p = params[(1 - d if departure == "directions_swapped" else d) * dir_floats:].to(dtype)
        wg0, wc0 = p[:2 * h], p[(1 + h) * 2 * h + 2 * h:][:h]
        dx = dx + dad[:, :, d * 3 * h:d * 3 * h + 2 * h] @ wg0 + dad[:, :, d * 3 * h + 2 * h:(d + 1) * 3 * h] @ wc0
    return dx


def bn_stat_ref(u, dgamma, dbeta, dtype, departure=None):
    """(d moving_mean, d moving_variance) = (-gamma d beta / sqrt(var + eps), -gamma d gamma / (2 (var + eps)))."""
    import torch
    gam, var = u["gamma"].to(dtype), u["var"].to(dtype)
    root = torch.sqrt(var) + BN_EPS if departure == "eps_outside_root" else torch.sqrt(var + BN_EPS)
    return -gam * dbeta.to(dtype) / root, -gam * dgamma.to(dtype) / (2 * root * root)


def drop_scale_plane(n4, keep_prob, seed, layer, step):
    """The factors of ``cf_gen_dropout``'s own hash for the first ``n4`` f32x4 of an output plane, as float32 [n4, 4], from the
    comments of cf_drop_key / cf_drop_scale4 (csrc/catfish_hip.hip): the key is fmix32(seed ^ fmix32(0x9E3779B9 (layer + 1) +
    step 0x85ebca6b)) with the step count taken from its double as a 32-bit unsigned number; element 4 idx4 + j survives when
    fmix32(element ^ key) < thresh, thresh = min(keep_prob 2^32, 4294967040) evaluated in float32; survivors carry 1 / keep_prob."""
    from catfish_amd.device_db import fmix32
    m32 = 0xFFFFFFFF
    st = int(step) & m32
    inner = int(fmix32(np.array([(0x9E3779B9 * (layer + 1) + st * 0x85EBCA6B) & m32], dtype=np.uint32))[0])
    key = fmix32(np.array([(int(seed) & m32) ^ inner], dtype=np.uint32))[0]
    kp = np.float32(keep_prob)
    thresh = np.uint32(min(np.float32(kp * np.float32(4294967296.0)), np.float32(4294967040.0)))
    e = np.arange(n4, dtype=np.uint64) * np.uint64(4)
    base = (e & np.uint64(m32)).astype(np.uint32) ^ ((e >> np.uint64(32)) * np.uint64(0x9E3779B9) & np.uint64(m32)).astype(np.uint32)
    elem = base[:, None] + np.arange(4, dtype=np.uint32)[None, :]
    keep = fmix32(elem ^ key) < thresh
    return np.where(keep, np.float32(1.0) / kp, np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ error measures
EDGE = [0, T - 1]


def forward_errors(got, ref):
    """got, ref: (z, y).  y also on steps 0 and 34 alone; per window both z and y."""
    (z, y), (z64, y64) = got, ref
    return {"z": _rel(z, z64), "y": max(_rel(y, y64), _rel(y[:, EDGE], y64[:, EDGE])), "y_window": max(_rel_window(y, y64), _rel_window(z, z64))}


def bn_errors(got, ref):
    """got, ref: (dz, d gamma, d beta)"""
    return {"dz": _rel(got[0], ref[0]), "dz_window": _rel_window(got[0], ref[0]), "bn": max(_rel(got[1], ref[1]), _rel(got[2], ref[2]))}


def wgrad_errors(got, ref):
    """got, ref: (kernel rows, bias row): separate tensors of the model, each over its own maximum"""
    return {"wgrad": max(_rel(got[0], ref[0]), _rel(got[1], ref[1]))}


def loss_error(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def head_errors(got, ref, n_real):
    out = {"din": _rel(got["din"], ref["din"]), "dl": _rel(got["dl"], ref["dl"]),
           "wgrad": max(_rel(got["gw"], ref["gw"]), _rel(got["gb"], ref["gb"]))}
    if "loss" in ref:
        out.update(logits=_rel(got["logits"][:n_real], ref["logits"][:n_real]), loss=loss_error(got["loss"], ref["loss"]))
    return out


def elementwise_error(got, ref):
    """max over elements of |d| / |ref|; where the reference is an exact zero, so must ``got`` be."""
    ref = ref.double()
    nz = ref != 0
    assert bool((got.double()[~nz] == 0).all())
    return float(((got.double() - ref).abs()[nz] / ref.abs()[nz]).max())


# ------------------------------------------------------------------------------------------------ launches
@pytest.fixture(scope="module")
def engine():
    """The C-ABI handle the launches go through: the entry points under test take the sizes as arguments."""
    from catfish_amd.engine import HipEngine
    geo = dict(layer_size=16, n_layers=1, layer_size_res=16, n_layers_res=1)
    eng = HipEngine(oracle.random_weights(seed=41, **geo), device=0, max_windows_per_pass=256, **geo)
    yield eng
    eng.close()


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _plane(npad, f):
    """A fragment plane of f features, NaN."""
    return _nan(npad // 16, T, f // 16, 64, 4)


def _frag(x):
    """natural [N, 35, F] on the CPU -> fragment plane on the device; the one signal feature -> [N, 35]"""
    from catfish_amd.native_train import nat_to_frag
    return x[:, :, 0].contiguous().cuda() if x.shape[2] == 1 else nat_to_frag(x.cuda())


def _nat(frag):
    from catfish_amd.native_train import frag_to_nat
    return frag_to_nat(frag)


def _cuda(u):
    return {k: v.cuda() for k, v in u.items()}


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ I. conv units
@pytest.mark.parametrize("kw,cin,cout,npad", I_CASES)
def test_conv_forward_matches_float64(engine, kw, cin, cout, npad):
    """cf_gen_conv_forward with ReLU off / on, without and with a shortcut plane."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    x, u, sc = conv_forward_inputs(kw, cin, cout, npad)
    x_dev, flat, sc_frag = _frag(x), unit_flat(u).cuda(), _frag(sc)
    x, u, sc = x.cuda(), _cuda(u), sc.cuda()
    for relu in (0, 1):
        for short in (None, sc):
            z, y = _plane(npad, cout), _plane(npad, cout)
            N.check(lib.cf_gen_conv_forward(hd, kw, cin, cout, N._p(flat), N._p(x_dev), None if short is None else N._p(sc_frag), relu,
                                            N._p(z), N._p(y), npad, _stream()))
            ref = conv_forward_ref(x, u, kw, relu, short, torch.float64)
            yard = conv_forward_ref(x, u, kw, relu, short, torch.float32)
            _check("I", "forward (%d, %d, %d, %d), relu %d, shortcut %d" % (kw, cin, cout, npad, relu, short is not None),
                   forward_errors((_nat(z), _nat(y)), ref), forward_errors(yard, ref))


@pytest.mark.parametrize("kw,cin,cout,npad", I_CASES)
def test_conv_backward_data_matches_float64(engine, kw, cin, cout, npad):
    """cf_gen_conv_backward_data with ``add`` null, a plane of its own and ``add == dx`` in place; cin 1 is refused."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    dz, u, add = conv_dx_inputs(kw, cin, cout, npad)
    dz_frag, flat = _frag(dz), unit_flat(u).cuda()
    if cin == 1:
        with pytest.raises(ValueError):                  # the one signal feature has no fragment plane of gradients
            dx = _nan(npad, T)
            N.check(lib.cf_gen_conv_backward_data(hd, kw, cin, cout, N._p(flat), N._p(dz_frag), None, N._p(dx), npad, _stream()))
        return
    add_frag = _frag(add)
    dz, u, add = dz.cuda(), _cuda(u), add.cuda()
    for how in ("null", "plane", "in place"):
        dx = add_frag.clone() if how == "in place" else _plane(npad, cin)
        src = {"null": None, "plane": N._p(add_frag), "in place": N._p(dx)}[how]
        N.check(lib.cf_gen_conv_backward_data(hd, kw, cin, cout, N._p(flat), N._p(dz_frag), src, N._p(dx), npad, _stream()))
        a = None if how == "null" else add
        ref, yard = conv_dx_ref(dz, u, kw, a, torch.float64), conv_dx_ref(dz, u, kw, a, torch.float32)
        _check("I", "backward data (%d, %d, %d, %d), add %s" % (kw, cin, cout, npad, how), {"dx": _rel(_nat(dx), ref)}, {"dx": _rel(yard, ref)})
    assert _same_bits(add_frag, _frag(add.cpu()))        # the operand of the out-of-place call is not written


def _fma(a, b, acc):
    """fmaf(a, b, acc) on float32 tensors: the product is exact in float64, the sum is rounded there and once more to float32."""
    return (a.double() * b.double() + acc.double()).float()


def chain_dot(x, w, bias):
    """gt_head_kernel's logit in float32: one fmaf chain over the features in order, then the bias.  x [P, F], w [F]."""
    import torch
    s = torch.zeros(x.shape[0], device=x.device)
    for f in range(x.shape[1]):
        s = _fma(x[:, f], w[f], s)
    return s + bias


def chain_wgrad(a, r):
    """gt_wgrad_kernel and gt_reduce_kernel in float32 at one column: a [P, M], r [P] -> [M], per chunk of 32 windows one fmaf
    chain over its positions in order (the chunks side by side here, a short last one padded with zeros: fmaf(0, 0, acc) is
    acc), then the chunks summed in order."""
    import torch
    import torch.nn.functional as F
    p, m = a.shape
    chunk = CHUNK_WINDOWS * T
    chunks = (p + chunk - 1) // chunk
    a = F.pad(a.float(), (0, 0, 0, chunks * chunk - p)).reshape(chunks, chunk, m)
    r = F.pad(r.float(), (0, chunks * chunk - p)).reshape(chunks, chunk, 1)
    acc = torch.zeros(chunks, m, device=a.device)
    for i in range(chunk):
        acc = _fma(a[:, i], r[:, i], acc)
    tot = torch.zeros(m, device=a.device)
    for c in range(chunks):
        tot = tot + acc[c]
    return tot


def chain_pairs(pairs):
    """gt_signal_grad_kernel's sum in float32: one fmaf chain over ``pairs`` [(plane [P], weight)] in order."""
    import torch
    s = torch.zeros(pairs[0][0].shape[0], device=pairs[0][0].device)
    for g, w in pairs:
        s = _fma(g, w, s)
    return s


def head_chain_errors(x, ref, n_real=None):
    """The summation-order term of the head's quantities: chain_dot for the logits (with ``n_real``), chain_wgrad of [x | 1] over
    the float64 reference's d logit rounded to float32, each against the float64 reference."""
    import torch
    n, t, f = x.shape
    x2 = x.float().reshape(n * t, f)
    gw = chain_wgrad(torch.cat([x2, x2.new_ones(n * t, 1)], 1), ref["dl"].float())
    out = {"wgrad": max(_rel(gw[:-1], ref["gw"]), _rel(gw[-1:], ref["gb"]))}
    if n_real is not None:
        out["logits"] = _rel(chain_dot(x2, ref["w32"], ref["b32"]).reshape(n, t)[:n_real], ref["logits"][:n_real])
    return out


def _chain_sums(v, zhat):
    """d gamma, d beta summed as gt_bn_bwd_kernel sums them, emulated in float32: per tile one chain over (step, window) (the fma
    of d gamma through float64, rounded once), then the tiles in order."""
    import torch
    tiles, c = v.shape[0] // 16, v.shape[2]
    v, zhat = v.float().reshape(tiles, 16, T, c), zhat.float().reshape(tiles, 16, T, c)
    sg, sb = torch.zeros(tiles, c, device=v.device), torch.zeros(tiles, c, device=v.device)
    for t in range(T):
        for w in range(16):
            sb = sb + v[:, w, t]
            sg = (v[:, w, t].double() * zhat[:, w, t].double() + sg.double()).float()
    g, b = torch.zeros(c, device=v.device), torch.zeros(c, device=v.device)
    for tile in range(tiles):
        g, b = g + sg[tile], b + sb[tile]
    return g, b


@pytest.mark.parametrize("kw,cin,cout,npad", I_CASES)
def test_bn_backward_matches_float64(engine, kw, cin, cout, npad):
    """cf_gen_bn_backward and cf_gen_bn_backward_data with ReLU off / on and the mask null / given, on a unit with a zero gamma
    (beta > 0: the gate is on, dz is zero, d gamma is not), a negative gamma and a zero moving variance."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    g, mask, z, u, moved = bn_backward_inputs(kw, cin, cout, npad)
    assert moved < 0.01
    assert float(u["gamma"][1]) == 0.0 and float(u["beta"][1]) > 0 and float(u["gamma"][2]) < 0 and float(u["var"][3]) == 0.0
    zeros = mask[mask == 0]
    assert bool(torch.signbit(zeros).any() and (~torch.signbit(zeros)).any() and (mask > 0).any() and (mask < 0).any())
    g_frag, mask_frag, z_frag, flat = _frag(g), _frag(mask), _frag(z), unit_flat(u).cuda()
    g, mask, z, u = g.cuda(), mask.cuda(), z.cuda(), _cuda(u)
    kf, ws_floats = kw * cin * cout + cout, npad // 16 * 2 * cout
    for relu in (0, 1):
        for m, m_frag in ((None, None), (mask, mask_frag)):
            dz, dz2, ws, grads = _plane(npad, cout), _plane(npad, cout), _nan(ws_floats), _nan(flat.numel())
            mp = None if m is None else N._p(m_frag)
            N.check(lib.cf_gen_bn_backward(hd, kw, cin, cout, N._p(flat), N._p(g_frag), mp, relu, N._p(z_frag), N._p(dz), N._p(ws), ws_floats,
                                           N._p(grads), npad, _stream()))
            N.check(lib.cf_gen_bn_backward_data(hd, kw, cin, cout, N._p(flat), N._p(g_frag), mp, relu, N._p(z_frag), N._p(dz2), npad, _stream()))
            assert _same_bits(dz, dz2)
            pre = _nan(flat.numel())
            assert _same_bits(grads[:kf], pre[:kf]) and _same_bits(grads[kf + 2 * cout:], pre[kf + 2 * cout:])     # kernel, bias; mean, variance
            got = (_nat(dz), grads[kf:kf + cout], grads[kf + cout:kf + 2 * cout])
            ref, yard = bn_backward_ref(g, m, relu, z, u, torch.float64), bn_backward_ref(g, m, relu, z, u, torch.float32)
            v64 = bn_gated(g, m, relu, z, u, torch.float64)
            assert torch.equal(bn_gated(g, m, relu, z, u, torch.float32) != 0, v64 != 0)      # float32 takes the gates float64 takes
            zhat = (z.double() - u["mean"].double()) / torch.sqrt(u["var"].double() + BN_EPS)
            chain = _chain_sums(v64, zhat)
            _check("I", "bn backward (%d, %d, %d, %d), relu %d, mask %d" % (kw, cin, cout, npad, relu, m is not None), bn_errors(got, ref),
                   bn_errors(yard, ref), {"bn": max(_rel(chain[0], ref[1]), _rel(chain[1], ref[2]))})


@pytest.mark.parametrize("kw,cin,cout,npad", I_CASES)
def test_conv_wgrad_matches_float64(engine, kw, cin, cout, npad):
    """cf_gen_conv_wgrad: the kernel rows and the bias row; gamma through variance are not its to write."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    x, dz = conv_wgrad_inputs(kw, cin, cout, npad)
    x_dev, dz_frag = _frag(x), _frag(dz)
    rows = kw * cin + 1
    ws_floats = int(lib.cf_gen_train_workspace_floats(rows, cout, npad))
    assert ws_floats == rows * cout * ((npad + CHUNK_WINDOWS - 1) // CHUNK_WINDOWS)
    ws, grads = _nan(ws_floats), _nan(rows * cout + 4 * cout)
    N.check(lib.cf_gen_conv_wgrad(hd, kw, cin, cout, N._p(x_dev), N._p(dz_frag), N._p(ws), ws_floats, N._p(grads), npad, _stream()))
    assert _same_bits(grads[rows * cout:], _nan(4 * cout))
    w = grads[:rows * cout].view(rows, cout)
    x, dz = x.cuda(), dz.cuda()
    ref, yard = conv_wgrad_ref(x, dz, kw, torch.float64), conv_wgrad_ref(x, dz, kw, torch.float32)
    _check("I", "wgrad (%d, %d, %d, %d)" % (kw, cin, cout, npad), wgrad_errors((w[:-1], w[-1]), ref), wgrad_errors(yard, ref))


# ------------------------------------------------------------------------------------------------ J. the head with its loss
J_CASES = [(f, npad, pad) for f in (16, 96, 224, 512) for npad in (16, 48) for pad in (0, 5, 15)]


def _run_head(engine, x, w, b, labels, n_real):
    """cf_gen_head on NaN outputs -> what head_ref returns, from the kernels."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    npad, _, f = x.shape
    p = npad * T
    ws_floats = int(lib.cf_gen_head_workspace_floats(f, npad))
    din, logits, ws, grads, loss = _plane(npad, f), _nan(npad, T), _nan(ws_floats), _nan(f + 1), _nan(1)
    dense, x_frag, lab = torch.cat([w, b]).cuda(), _frag(x), labels.cuda()          # held until the launch has run
    N.check(lib.cf_gen_head(hd, f, N._p(x_frag), N._p(dense), N._p(lab), n_real, N._p(din), N._p(logits), N._p(ws), ws_floats,
                            N._p(grads), N._p(loss), npad, _stream()))
    return {"logits": logits, "din": _nat(din), "dl": ws[:p].clone(), "loss": loss[0], "gw": grads[:f], "gb": grads[f:]}


def _assert_padding(got, n_real, logits=True):
    """d input and d logit of the padding windows are exact zeros; their logits keep the pre-fill."""
    import torch
    assert float(got["din"][n_real:].abs().sum()) == 0.0 and float(got["dl"][n_real * T:].abs().sum()) == 0.0
    if logits:
        assert bool(torch.isnan(got["logits"][n_real:]).all()) and bool(torch.isfinite(got["logits"][:n_real]).all())


@pytest.mark.parametrize("features,npad,pad", J_CASES)
def test_head_matches_float64(engine, features, npad, pad):
    """cf_gen_head: logits, d input, d logit, the loss, the dense gradients (weights and bias separately)."""
    import torch
    n_real = npad - pad
    x, w, b, labels = head_inputs(features, npad, n_real)
    assert n_real < 8 or 0 < float(labels[:n_real, 0].sum()) < n_real      # both labels among the real windows
    got = _run_head(engine, x, w, b, labels, n_real)
    _assert_padding(got, n_real)
    args = (x.cuda(), w.cuda(), b.cuda(), labels.cuda(), n_real)
    ref, yard = head_ref(*args, torch.float64), head_ref(*args, torch.float32)
    ref.update(w32=args[1], b32=args[2])
    _check("J", "%d features, %d windows, %d real" % (features, npad, n_real), head_errors(got, ref, n_real), head_errors(yard, ref, n_real),
           head_chain_errors(args[0], ref, n_real))


def test_head_stays_finite_with_saturated_logits(engine):
    """Inputs scaled so that the float64 logits pass +-80 (scaled for 92: exp(-s) overflows float32 past 88.7): the loss and every
    gradient are finite and meet the bounds, the loss relative to max(1, |ref|)."""
    import torch
    features, npad, n_real = 96, 16, 11
    x, w, b, labels = head_inputs(features, npad, n_real, reach=90.0)
    args = (x.cuda(), w.cuda(), b.cuda(), labels.cuda(), n_real)
    ref, yard = head_ref(*args, torch.float64), head_ref(*args, torch.float32)
    s = ref["logits"][:n_real]
    assert float(s.max()) >= 80.0 and float(s.min()) <= -80.0, (float(s.min()), float(s.max()))
    got = _run_head(engine, x, w, b, labels, n_real)
    _assert_padding(got, n_real)
    for k in ("din", "dl", "loss", "gw", "gb"):
        assert bool(torch.isfinite(got[k]).all()), k
    ref.update(w32=args[1], b32=args[2])
    _check("J", "saturated: %d features, %d windows, %d real" % (features, npad, n_real), head_errors(got, ref, n_real),
           head_errors(yard, ref, n_real), head_chain_errors(args[0], ref, n_real))


# ------------------------------------------------------------------------------------------------ K. the operator's own kernels
@pytest.mark.parametrize("features,npad,pad", J_CASES)
def test_head_backward_matches_float64(engine, features, npad, pad):
    """cf_gen_head_backward from a random d probability that is zero in the padding windows; without a gradient buffer it writes none."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    n_real, p = npad - pad, npad * T
    x, w, b, dprobs = head_backward_inputs(features, npad, n_real)
    ws_floats = int(lib.cf_gen_head_backward_workspace_floats(features, npad))
    dense, x_frag, g = torch.cat([w, b]).cuda(), _frag(x), dprobs.cuda()
    got = None
    for with_grads in (True, False):
        din, ws, grads = _plane(npad, features), _nan(ws_floats), _nan(features + 1)
        N.check(lib.cf_gen_head_backward(hd, features, N._p(x_frag), N._p(dense), N._p(g), N._p(din), N._p(ws), ws_floats,
                                         N._p(grads) if with_grads else None, npad, _stream()))
        if with_grads:
            got = {"din": _nat(din), "dl": ws[:p].clone(), "gw": grads[:features], "gb": grads[features:]}
        else:
            assert _same_bits(grads, _nan(features + 1)) and _same_bits(_nat(din), got["din"]) and _same_bits(ws[:p], got["dl"])
    _assert_padding(got, n_real, logits=False)
    args = (x.cuda(), w.cuda(), b.cuda(), g)
    ref, yard = head_backward_ref(*args, torch.float64), head_backward_ref(*args, torch.float32)
    _check("K", "head backward: %d features, %d windows, %d real" % (features, npad, n_real), head_errors(got, ref, n_real),
           head_errors(yard, ref, n_real), head_chain_errors(args[0], ref))


@pytest.mark.parametrize("npad", [16, 48])
@pytest.mark.parametrize("channels", [16, 48, 512])
def test_signal_grad_of_the_conv_stack_matches_float64(engine, channels, npad):
    """cf_gen_signal_grad, ResNetRNN: 560 positions at 16 windows leave the last block of 256 threads partly empty."""
    import torch
    from catfish_amd import _native as N
    gen = _gen(7, channels, npad)
    w_sc, w_1 = _randn(gen, channels), _randn(gen, channels)
    dz_sc, dz_1 = _randn(gen, npad, T, channels), _randn(gen, npad, T, channels)
    dx, g_sc, g_1 = _nan(npad, T), _frag(dz_sc), _frag(dz_1)
    args = (w_sc.cuda(), dz_sc.cuda(), w_1.cuda(), dz_1.cuda())
    N.check(engine._lib.cf_gen_signal_grad(engine._handle, 0, channels, N._p(args[0]), N._p(g_sc), N._p(args[2]), N._p(g_1), N._p(dx), npad,
                                           _stream()))
    ref, yard = signal_grad_res_ref(*args, torch.float64), signal_grad_res_ref(*args, torch.float32)
    g0, g1 = args[1].reshape(-1, channels), args[3].reshape(-1, channels)
    chain = chain_pairs([pair for o in range(channels) for pair in ((g0[:, o], args[0][o]), (g1[:, o], args[2][o]))]).reshape(npad, T)
    _check("K", "signal gradient: %d channels, %d windows" % (channels, npad), {"dsignal": _rel(dx, ref)}, {"dsignal": _rel(yard, ref)},
           {"dsignal": _rel(chain, ref)})


@pytest.mark.parametrize("npad", [16, 48])
@pytest.mark.parametrize("h", [16, 112, 256])
def test_signal_grad_of_the_plain_rnn_matches_float64(engine, h, npad):
    """cf_gen_signal_grad, plain RNN: row 0 of both directions' gates and candidate kernels over layer 0's gate gradients."""
    import torch
    from catfish_amd import _native as N
    gen = _gen(8, h, npad)
    params, da = gru_layer0_flat(gen, h), _randn(gen, npad, T, 6 * h)
    dx, p_dev, da_frag = _nan(npad, T), params.cuda(), _frag(da)
    N.check(engine._lib.cf_gen_signal_grad(engine._handle, h, 0, N._p(p_dev), N._p(da_frag), None, None, N._p(dx), npad, _stream()))
    ref, yard = (signal_grad_rnn_ref(p_dev, da.cuda(), h, dt) for dt in (torch.float64, torch.float32))
    g0, dir_floats, pairs = da.cuda().reshape(-1, 6 * h), (1 + h) * 3 * h + 3 * h, []
    for d in range(2):                                   # per direction: row 0 of the gates kernel over r | u, then of the candidate kernel
        wg0, wc0 = p_dev[d * dir_floats:][:2 * h], p_dev[d * dir_floats + (1 + h) * 2 * h + 2 * h:][:h]
        pairs += [(g0[:, d * 3 * h + j], wg0[j]) for j in range(2 * h)] + [(g0[:, d * 3 * h + 2 * h + j], wc0[j]) for j in range(h)]
    _check("K", "signal gradient: %d units, %d windows" % (h, npad), {"dsignal": _rel(dx, ref)}, {"dsignal": _rel(yard, ref)},
           {"dsignal": _rel(chain_pairs(pairs).reshape(npad, T), ref)})


def bn_stat_inputs(cout):
    """(the unit with its special channels, d gamma, d beta)"""
    gen = _gen(9, cout)
    return unit_params(gen, 1, 16, cout, special=True), _randn(gen, cout), _randn(gen, cout)


@pytest.mark.parametrize("cout", [16, 80, 512])
def test_bn_stat_grads_match_float64(engine, cout):
    """cf_gen_bn_stat_grads: d moving_mean and d moving_variance from d gamma and d beta, element by element (a zero gamma gives
    exact zeros); every other slot of the gradient buffer keeps its bits."""
    import torch
    from catfish_amd import _native as N
    kw, cin = 1, 16
    u, dgamma, dbeta = bn_stat_inputs(cout)
    flat = unit_flat(u).cuda()
    kf = kw * cin * cout + cout
    grads = _nan(flat.numel())
    grads[kf:kf + cout], grads[kf + cout:kf + 2 * cout] = dgamma.cuda(), dbeta.cuda()
    before = grads.clone()
    N.check(engine._lib.cf_gen_bn_stat_grads(engine._handle, kw, cin, cout, N._p(flat), N._p(grads), _stream()))
    assert _same_bits(grads[:kf + 2 * cout], before[:kf + 2 * cout])
    got = (grads[kf + 2 * cout:kf + 3 * cout], grads[kf + 3 * cout:])
    args = (_cuda(u), dgamma.cuda(), dbeta.cuda())
    ref, yard = bn_stat_ref(*args, torch.float64), bn_stat_ref(*args, torch.float32)
    assert float(ref[0][1]) == 0.0 and float(ref[1][1]) == 0.0
    err = lambda o: max(elementwise_error(o[0], ref[0]), elementwise_error(o[1], ref[1]))      # noqa: E731
    _check("K", "BN statistics: %d channels" % cout, {"dstat": err(got)}, {"dstat": err(yard)})


# ------------------------------------------------------------------------------------------------ exact sections
@pytest.mark.parametrize("npad", [16, 48])
def test_x_frag_is_the_signal_in_feature_zero(engine, npad):
    """cf_gen_x_frag is nat_to_frag of [signal | 15 zero features], bit for bit."""
    import torch
    from catfish_amd import _native as N
    x = _randn(_gen(10, npad), npad, T)
    out, x_dev = _plane(npad, 16), x.cuda()
    N.check(engine._lib.cf_gen_x_frag(engine._handle, N._p(x_dev), N._p(out), npad, _stream()))
    want = torch.zeros(npad, T, 16)
    want[:, :, 0] = x
    assert _same_bits(out, _frag(want))


@pytest.mark.parametrize("h", [16, 48, 256])
def test_dropout_with_a_scale_plane_is_the_product(engine, h):
    """cf_gen_dropout with an explicit scale plane: out = in * scale as float32 bits (keep_prob is not looked at then)."""
    from catfish_amd import _native as N
    npad = 48
    gen = _gen(11, h)
    x, scale = _frag(_randn(gen, npad, T, 2 * h)), _frag(mask_plane(gen, npad, T, 2 * h) * 1.25)
    out = _plane(npad, 2 * h)
    N.check(engine._lib.cf_gen_dropout(engine._handle, h, 0.0, 5, 0, None, N._p(scale), N._p(x), N._p(out), npad, _stream()))
    assert _same_bits(out, x * scale)


@pytest.mark.parametrize("h", [16, 48, 256])
def test_dropout_hash_is_the_stated_hash(engine, h):
    """cf_gen_dropout with its own hash against ``drop_scale_plane``: keep_prob 0.8 / 0.5 / 0.999999, layers 0 and 2, steps 0, 7
    and 2^32 + 3 (read from a device double, taken modulo 2^32).  In place as well: the backward scales a gradient where it lies."""
    import torch
    from catfish_amd import _native as N
    npad, seed = 32, 0xC0FFEE11
    x = _frag(1.0 + _rand(_gen(12, h), npad, T, 2 * h))
    n4 = x.numel() // 4
    seen = set()
    for keep_prob in (0.8, 0.5, 0.999999):
        for layer in (0, 2):
            for step in (0, 7, 2 ** 32 + 3):
                count = torch.tensor([float(step)], dtype=torch.float64, device="cuda")
                out = _plane(npad, 2 * h)
                N.check(engine._lib.cf_gen_dropout(engine._handle, h, keep_prob, seed, layer, N._p(count), None, N._p(x), N._p(out), npad,
                                                   _stream()))
                scale = drop_scale_plane(n4, keep_prob, seed, layer, step)
                want = x.cpu().numpy().reshape(n4, 4) * scale
                assert np.array_equal(out.cpu().numpy().reshape(n4, 4).view(np.uint32), want.view(np.uint32)), (keep_prob, layer, step)
                kept = float((scale != 0).mean())
                assert abs(kept - float(np.float32(keep_prob))) < 4.0 / np.sqrt(4 * n4), (keep_prob, kept)
                if keep_prob < 0.9:
                    seen.add((keep_prob, scale.tobytes()))
                if step == 7:
                    inplace = x.clone()
                    N.check(engine._lib.cf_gen_dropout(engine._handle, h, keep_prob, seed, layer, N._p(count), None, N._p(inplace), N._p(inplace),
                                                       npad, _stream()))
                    assert _same_bits(inplace, out)
    assert len(seen) == 2 * 2 * 3                          # every (keep_prob, layer, step) draws a mask of its own
    a, b = (drop_scale_plane(64, 0.8, seed, 1, s) for s in (3, 2 ** 32 + 3))
    assert np.array_equal(a, b)


def test_dropout_hash_at_64_units_is_the_tuned_kernels_mask(engine):
    """At layer size 64 the factors are cf_dropout_scale's: the plane the tuned training kernels apply."""
    import torch
    from catfish_amd import _native as N
    npad, seed, layer, keep_prob = 32, 1234567, 1, 0.8
    count = torch.tensor([5.0], dtype=torch.float64, device="cuda")
    ones = torch.ones(npad // 16, T, 8, 64, 4, device="cuda")
    out, scale = _plane(npad, 128), _plane(npad, 128)
    N.check(engine._lib.cf_gen_dropout(engine._handle, 64, keep_prob, seed, layer, N._p(count), None, N._p(ones), N._p(out), npad, _stream()))
    N.check(engine._lib.cf_dropout_scale(engine._handle, keep_prob, seed, layer, N._p(count), npad, N._p(scale), _stream()))
    assert _same_bits(out, scale)
    assert np.array_equal(out.cpu().numpy().reshape(-1, 4), drop_scale_plane(out.numel() // 4, keep_prob, seed, layer, 5))
