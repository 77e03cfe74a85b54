"""The tuned conv stack and head training kernels against float64, kernel by kernel (GPU).

The shipped geometry (64 GRU units, 32 conv channels) trains on csrc/res_train.hpp (``res_train_fwd_kernel``,
``res_train_bwd_kernel``, ``res_train_reduce_kernel`` behind ``cf_res_train_forward`` / ``cf_res_train_backward``) and on
csrc/train_step.hpp's ``train_head_kernel`` / ``train_head_reduce_kernel`` behind ``cf_train_head``.  Their float64 coverage was
one case (1027 windows, 2 blocks, gamma and variance in [0.5, 1.5], one maximum over all gradients) and none.  Here both run
alone, through ``engine._lib``, on operands this module builds:

  S  the conv stack as (windows, blocks), ``S_CASES``: 1, 2, 3 x 1 (one window per workgroup, the reduction's tail loop), 17 x 2,
     130 x 3, 1024 x 4 (the last count with one window per workgroup: 1024 partials, whole rounds of 16), 1025 x 4 (the first
     with two: the last workgroup holds one window; 513 partials, a tail of one), 1026 x 2 (every workgroup full); the regime is
     asserted from the workspace size.  Forward: every unit's ``Z`` per tensor, ``out`` per tensor and per window, ``out`` and
     the width-3 units' ``Z`` on steps 0 and 34 alone, where a tap that reads the neighbouring window (two-window layout) or
     stale LDS (one-window layout) shows: the neighbouring windows hold data.  Backward FROM A GIVEN STASH: the backward's
     operands are x, Z, d_out and the parameters, it recomputes every activation and gate from Z.  Z is the float64 forward's z
     of each unit rounded to float32 and settled (``settle_stash``: every z of units 1 to 3 whose float64 ``|BN(z)|`` is below
     1e-3 moves to 2e-3 with its sign, every z of unit 0 whose ``|relu(BN(z3)) + BN(z0)|`` is below it likewise; fewer than 1 %
     of the elements, asserted per case), so that float32 and the kernels take the gates float64 takes.  The reference is the
     float64 gradient of the stack given that stash (``stack_backward``, written out unit by unit; tests/test_tuned_train_host.py
     ties it to plain autograd through ``TorchResNetRNN(dtype=float64)`` to 1e-12 when the stash is the forward's own).  Kernel
     and bias gradients, and gamma and beta gradients, each tensor over its own maximum, the largest per unit kind (``first``: cin
     1, ``point``: width 1 on 32 channels, ``wide``: width 3), so a defect in unit 0 of block 0 is not averaged away by the
     others.  Exact: no slot of ``grads`` is NaN (``NativeResStack.backward`` allocates it uninitialised), the moving_mean and
     moving_variance slots are exact zeros, two calls give the same bits.  Refused before any launch: 0 and 5 blocks, a workspace
     one float short.  (The backward from the kernels' own stash stays where it is: tests/test_train_kernels_fp64.py, 1027
     windows.)
  T  the head, inputs laid out by ``nat_to_frag``: 1, 11, 16, 17 and 48 windows (15, 5, 0, 15 and 0 padding windows in the last
     tile), one count above the grid cap computed from the device's CU count (the smallest tile count with ceil(35 tiles / 32) >
     2 n_cu, minus 5 windows: 7499 windows on 256 CUs; below it a wave takes at most 8 items, the regime is asserted from the
     workspace size), labels 0 / 1 per element, once all ones, once with the dense kernel scaled until the logits pass +-100 on
     both labels.  The padding windows of the input hold 1e30 and must contribute nothing.  Logits over the largest, d input per
     tensor over the real windows, d kernel and d bias, the loss as ``|d| / max(1, |ref|)``.  Exact: d input is zero in every
     padding window, ``logits`` rows past n keep their NaN, the call with ``logits == NULL`` (the one ``NativeTrainStep.run``
     makes) gives bit-identical dy, grads and loss, two calls give the same bits.

Parameters of S.  Units come from ``unit_params(..., special=True)`` of tests/test_anysize_conv_fp64.py: in EVERY unit channel 1
has gamma 0 and beta 0.25, channel 2 gamma -0.75, channel 3 moving variance 0.  The one change: the variance-0 channel's gamma is
0.03, so its scale gamma / sqrt(1e-3) is 0.95 and not 32, which over four blocks would grow the activations to 2e5 and let that
one channel decide every maximum-relative measure.  No block output exceeds 100 in float64 (asserted).

References.  Every one is a function of a dtype, float64 the reference and float32 the yardstick, built on the per-unit
references of tests/test_anysize_conv_fp64.py and their ``departure=`` argument, which tests/test_tuned_train_host.py uses on the
CPU to show that the measures and bounds of this module see a subtly wrong kernel.  Inputs come from seeded CPU generators (the
stash is computed and settled on the CPU), so that file sees the very tensors of the GPU run.  Outputs and workspaces are NaN
before every launch.

Bounds.  As in the sibling modules: every case records the kernels' error and the float32 yardstick's against float64, the
asserted bound of a quantity is 4 x the largest yardstick over its section, rounded down to three digits, never looser than
``OLDER_BOUNDS`` (what tests/test_gpu_pipeline.py allows: 1e-5 on the stack's output and Z, 2e-5 on its gradients, 2e-6 on the
loss, 2e-5 on the logits, 1e-4 on the head's gradients).  profiles/tuned_train_fp64_parity.jsonl holds one measuring run,
``BOUNDS`` the constants, tests/test_training.py checks the one against the other.  Every row also carries ``chain`` where the
quantity has a sum the kernels take in an order of their own: the error against float64 of that one step evaluated in float32 in
the kernels' order from the float64 reference's operands (``stack_chain_grads``: a thread's positions, the 8 position groups,
``cf_reduce_parts`` over the workgroups; ``head_chain``: the 32-product logit chain per lane quarter, a wave's items, the 16
windows of a lane quarter, ``cf_reduce_parts`` over the waves).  ``CHAIN_TERM`` names the quantities whose yardstick includes it.

As measured (MI355X, 256 CUs; yardstick = float32 torch, largest over the section -> bound; the kernels' largest error; its share
of the bound):
  S  z 4.88e-7 -> 1.95e-6, kernels 4.96e-7 (0.25); out 4.30e-7 -> 1.71e-6, 3.05e-7 (0.18); out per window 7.28e-7 -> 2.91e-6,
     4.37e-7 (0.15); edge steps 4.20e-7 -> 1.67e-6, 3.08e-7 (0.18); kernel and bias gradients: first 2.06e-6 -> 8.25e-6, 5.57e-7
     (0.07), point 5.89e-6 -> the older 2e-5, 6.36e-7 (0.03), wide 7.73e-6 -> the older 2e-5, 4.20e-7 (0.02); gamma and beta
     gradients: first 7.01e-7 -> 2.80e-6, 1.18e-6 (0.42), point 5.97e-7 -> 2.38e-6, 8.28e-7 (0.35), wide 5.53e-7 -> 2.21e-6,
     4.83e-7 (0.22).
  T  logits 1.52e-7 -> 6.07e-7, kernels 1.91e-7 (0.32); d input 1.18e-6 -> 4.72e-6, 1.61e-6 (0.34, both in the saturated case);
     dense gradients 9.27e-7 -> 3.70e-6, 1.83e-7 (0.05); loss 1.04e-7 -> 4.13e-7, 4.17e-8 (0.10).
The two thinnest margins: the gamma and beta gradients of the first units at 0.42 of their bound (1.18e-6 at 1026 windows x 2
blocks; 1.03e-6 at 130 x 3, there 3.2 x that case's float32 torch) and of the point units at 0.35 (8.28e-7 at 1024 x 4).  The
first is d gamma of the variance-0 channel of block 0's unit 1, the tensor's largest element: its zhat is 31.6 x the others', its
terms cancel (at 130 x 3 to 1 / 87 of their absolute sum), and its upstream gradient has passed every later unit in float32, which
the emulation, fed from float64, leaves out (at 1026 x 2, with fewer units behind it, the emulation gives 9.6e-7 of the 1.18e-6).  Two
quantities fell back to the older bound, ``S.wgrad_point`` and ``S.wgrad_wide``: float32 torch, one GEMM over all positions, is 9
to 18 x less accurate there than the kernels, whose partial sums per workgroup and fixed-order reduction behave like a tree.  No
quantity needed the summation-order term: the emulation is recorded in every row that has one and lands on the kernels (it gives
the kernels' logits error digit for digit in every T case, the loss in 4 of 8 and the dense gradients in 2 of 8; the
stack's gradients are 0.24 to 5.2 x their emulation's: those also carry the float32 error of the upstream gradient, which the
emulation, fed from float64, does not).  Every bound is 2.4 to 33 x tighter than the gate it replaces, the two fallen back excepted.  No kernel had
to change: csrc/res_train.hpp and csrc/train_step.hpp are as they were.  The runs are deterministic; if a reordering of sums trips
a bound, re-measure, do not widen by hand.  A case takes 0.01 to 0.2 s (the 4-block cases at 1024 and 1025 windows 0.17 s, the
capped head case 0.13 s), the module 4.2 s, 2.7 s of them the engine and the first launch.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from test_train_kernels_fp64 import T, _rel, _rel_window, _stamp
from test_anysize_conv_fp64 import (BN_EPS, GATE_MARGIN, UNIT_KEYS, _fma, _gen, _rand, _randn, bn_affine, conv_dx_ref,      # noqa: F401
                                    conv_forward_ref, conv_wgrad_ref, loss_error, settle, shifted, tap_offsets, unit_flat, unit_params)

pytestmark = pytest.mark.gpu

# quantity -> asserted bound = min(4 x largest yardstick over the section, older bound).  The largest yardsticks in
# profiles/tuned_train_fp64_parity.jsonl (MI355X, 256 CUs; float32 torch: no quantity needed the summation-order term), and the
# kernels' largest error next to them:
#   S.z 4.877e-07 (kernels 4.96e-07)   S.out 4.295e-07 (3.05e-07)   S.out_window 7.278e-07 (4.37e-07)   S.edge 4.195e-07 (3.08e-07)
#   S.wgrad_first 2.063e-06 (5.57e-07)   S.wgrad_point 5.894e-06 (6.36e-07)   S.wgrad_wide 7.731e-06 (4.20e-07)
#   S.bn_first 7.010e-07 (1.18e-06)   S.bn_point 5.972e-07 (8.28e-07)   S.bn_wide 5.527e-07 (4.83e-07)
#   T.logits 1.519e-07 (1.91e-07)   T.din 1.182e-06 (1.61e-06)   T.wgrad 9.271e-07 (1.83e-07)   T.loss 1.035e-07 (4.17e-08)
# 4 x each of them, rounded down, is the bound, except for S.wgrad_point and S.wgrad_wide: 4 x their yardstick (2.36e-5, 3.09e-5) is
# above the older 2e-5, which therefore stays (float32 torch takes those gradients as one GEMM over up to 35 875 positions).
BOUNDS = {
    "S.z": 1.95e-6, "S.out": 1.71e-6, "S.out_window": 2.91e-6, "S.edge": 1.67e-6,
    "S.wgrad_first": 8.25e-6, "S.wgrad_point": 2e-5, "S.wgrad_wide": 2e-5, "S.bn_first": 2.80e-6, "S.bn_point": 2.38e-6, "S.bn_wide": 2.21e-6,
    "T.logits": 6.07e-7, "T.din": 4.72e-6, "T.wgrad": 3.70e-6, "T.loss": 4.13e-7,
}
# what tests/test_gpu_pipeline.py allows for the quantity (test_native_res_stack_training_kernels_match_torch_autograd,
# test_train_head_kernel_matches_torch)
OLDER_BOUNDS = {
    "S.z": 1e-5, "S.out": 1e-5, "S.out_window": 1e-5, "S.edge": 1e-5,
    "S.wgrad_first": 2e-5, "S.wgrad_point": 2e-5, "S.wgrad_wide": 2e-5, "S.bn_first": 2e-5, "S.bn_point": 2e-5, "S.bn_wide": 2e-5,
    "T.logits": 2e-5, "T.din": 1e-4, "T.wgrad": 1e-4, "T.loss": 2e-6,
}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tuned_train_fp64_parity.jsonl")
RT_SMALL_BATCH = 1024    # csrc/res_train.hpp: up to this many windows a workgroup takes one window, above it two
RT_PG = 8                # position groups of a workgroup: thread (channel, group) walks positions group, group + 8, ...
HEAD_PART = 132          # CF_HEAD_PART: floats per wave of the head's workspace
CHANNELS = 32

# quantities whose yardstick carries the summation-order term: none.  The candidates were each unit's parameter gradients (a
# thread's positions in one chain) and the head's partial sums (a wave's items in one chain); with at most 9 positions and 9 items
# per chain the kernels stay inside 4 x float32 torch as they are, so ``chain`` is recorded and not used.
CHAIN_TERM = ()


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


def _check(section, case, kernel, yard, chain):
    """kernel, yard: {quantity: error} of the kernels and of float32 torch; chain: {quantity: error of the float32 emulation of
    the kernels' summation order} for the quantities that have such a sum (null in the rows of the others).  All are recorded
    (printed as ``parity`` rows), then all are asserted."""
    assert sorted(kernel) == sorted(yard) and set(chain) <= set(kernel)
    assert all(q in chain for q in kernel if "%s.%s" % (section, q) in CHAIN_TERM)
    for q, k in kernel.items():
        _record(section, case, q, k, yard[q], chain.get(q))
    bad = {q: (k, BOUNDS["%s.%s" % (section, q)]) for q, k in kernel.items() if not k <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ S. inputs (CPU generators)
# (windows, blocks)
S_CASES = [(1, 1), (2, 1), (3, 1), (17, 2), (130, 3), (1024, 4), (1025, 4), (1026, 2)]
GRAD_KEYS = ("kernel", "bias", "gamma", "beta")


def unit_shape(u):
    """(kernel width, input channels) of unit u of the stack: widths 1, 1, 3, 1 per block; the signal has one channel."""
    return (3 if u % 4 == 2 else 1), (1 if u < 2 else CHANNELS)


def unit_kind(u):
    return "first" if u < 2 else ("wide" if u % 4 == 2 else "point")


def workgroups(n):
    """Workgroups of the stack's launches at n windows, and the windows of each."""
    win = 1 if n <= RT_SMALL_BATCH else 2
    return (n + win - 1) // win, win


def stack_inputs(n, n_blocks):
    """(x [n, 35], the units, d_out [n, 35, 32]).  Every unit has the special channels of ``unit_params``; the variance-0
    channel's gamma is 0.03."""
    gen = _gen(20, n, n_blocks)
    units = []
    for u in range(4 * n_blocks):
        kw, cin = unit_shape(u)
        p = unit_params(gen, kw, cin, CHANNELS, special=True)
        p["gamma"][3] = 0.03
        units.append(p)
    return 1.2 * _randn(gen, n, T), units, _randn(gen, n, T, CHANNELS)


def stack_flat(units):
    import torch
    return torch.cat([unit_flat(u) for u in units])


def split_grads(flat, n_blocks):
    """The gradient buffer -> per unit {kernel [kw cin, 32], bias, gamma, beta, mean, var}."""
    out, o = [], 0
    for u in range(4 * n_blocks):
        kw, cin = unit_shape(u)
        rows = kw * cin
        d = {"kernel": flat[o:o + rows * CHANNELS].view(rows, CHANNELS)}
        o += rows * CHANNELS
        for k in ("bias", "gamma", "beta", "mean", "var"):
            d[k] = flat[o:o + CHANNELS]
            o += CHANNELS
        out.append(d)
    assert o == flat.numel()
    return out


# ------------------------------------------------------------------------------------------------ S. references (any device, any dtype)
def stack_forward(x, units, dtype, departure=None):
    """The blocks of csrc/res_train.hpp's header -> (z of every unit [n, 35, 32], the output of every block)."""
    a = x.to(dtype)[:, :, None]
    zs, outs = [], []
    for d in range(len(units) // 4):
        u0, u1, u2, u3 = units[4 * d:4 * d + 4]
        z0, sc = conv_forward_ref(a, u0, 1, 0, None, dtype, departure)
        z1, o1 = conv_forward_ref(a, u1, 1, 1, None, dtype, departure)
        z2, o2 = conv_forward_ref(o1, u2, 3, 1, None, dtype, departure)
        z3, a = conv_forward_ref(o2, u3, 1, 1, sc, dtype, departure)
        zs += [z0, z1, z2, z3]
        outs.append(a)
    return zs, outs


def block_from_stash(z4, units4, dtype, departure=None):
    """(BN(z) of the four units, relu(BN(z3)) + BN(z0)) of one block from its stashed z."""
    import torch
    y = []
    for z, u in zip(z4, units4):
        s, t = bn_affine(u, dtype, departure)
        y.append(z.to(dtype) * s + t)
    return y, torch.relu(y[3]) + y[0]


def settle_stash(zs, units):
    """zs: the float64 forward's z per unit -> (float32 stash, share of elements moved).  Units 1 to 3 of a block through
    ``settle``; then every z0 whose float64 |relu(BN(z3)) + BN(z0)| is below GATE_MARGIN moves to where it is 2 GATE_MARGIN with
    its sign (channels with a zero scale are left alone: their shortcut is beta)."""
    import torch
    out, moved = [None] * len(zs), 0.0
    for d in range(len(zs) // 4):
        for i in (1, 2, 3):
            out[4 * d + i], share = settle(zs[4 * d + i].float(), units[4 * d + i])
            moved += share * zs[4 * d + i].numel()
        (s0, t0), (s3, t3) = bn_affine(units[4 * d], torch.float64), bn_affine(units[4 * d + 3], torch.float64)
        o3 = torch.relu(out[4 * d + 3].double() * s3 + t3)
        z0 = zs[4 * d].float()
        pre = o3 + z0.double() * s0 + t0
        near = (pre.abs() < GATE_MARGIN) & (s0 != 0)
        target = torch.where(pre < 0, -2 * GATE_MARGIN, 2 * GATE_MARGIN)
        safe = torch.where(s0 != 0, s0, torch.ones_like(s0))
        out[4 * d] = torch.where(near, ((target - o3 - t0) / safe).float(), z0)
        assert float((o3 + out[4 * d].double() * s0 + t0).abs().min()) >= GATE_MARGIN
        moved += float(near.double().sum())
    return out, moved / sum(z.numel() for z in zs)


def bn_backward(g, mask, relu, z, u, dtype, departure=None):
    """(v, dz, d gamma, d beta, zhat): v = g where ``mask`` > 0 (if given) and, with ``relu``, where BN(z) > 0, else 0; dz = v s,
    d gamma = sum v zhat, zhat = (z - mean) / sqrt(var + eps), d beta = sum v."""
    import torch
    s, t = bn_affine(u, dtype, departure)
    zd, v = z.to(dtype), g
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    if relu:
        v = torch.where(zd * s + t > 0, v, torch.zeros_like(v))
    var = u["var"].to(dtype)
    inv = 1.0 / (torch.sqrt(var) + BN_EPS) if departure == "eps_outside_root" else 1.0 / torch.sqrt(var + BN_EPS)
    zhat = (zd - u["mean"].to(dtype)) * inv
    dgamma = (v * zhat).reshape(-1, CHANNELS).sum(0)
    if departure == "abs_gamma":                         # d gamma taken through |gamma|: the sign of a negative gamma is lost
        dgamma = dgamma * torch.where(u["gamma"].to(dtype) < 0, -1.0, 1.0)
    return v, v * s, dgamma, v.reshape(-1, CHANNELS).sum(0), zhat


def stack_backward(x, units, stash, d_out, dtype, departure=None, operands=None):
    """The gradient of sum(out d_out) with respect to every unit's kernel, bias, gamma and beta GIVEN THE STASH: every activation
    and every gate is recomputed from ``stash`` (z per unit), as res_train_bwd_kernel does -> per unit {kernel [kw cin, 32], bias,
    gamma, beta}.  ``operands``: a list that receives per unit (input activation, v, dz, zhat) for the summation-order emulation."""
    import torch
    n_blocks = len(units) // 4
    g = d_out.to(dtype)
    if departure == "last_partial_dropped":              # the reduction leaves out the last workgroup's partial sums
        n_wg, win = workgroups(x.shape[0])
        g = g.clone()
        g[(n_wg - 1) * win:] = 0
    grads, ops = [None] * len(units), [None] * len(units)

    def unit(j, a_in, upstream, mask, relu):
        kw = unit_shape(j)[0]
        v, dz, dgamma, dbeta, zhat = bn_backward(upstream, mask, relu, stash[j], units[j], dtype, departure)
        kernel, bias = conv_wgrad_ref(a_in, dz, kw, dtype, departure)
        grads[j], ops[j] = {"kernel": kernel, "bias": bias, "gamma": dgamma, "beta": dbeta}, (a_in, v, dz, zhat)
        return dz

    for d in reversed(range(n_blocks)):
        j = 4 * d
        if d == 0:
            a = x.to(dtype)[:, :, None]
        else:
            a = torch.relu(block_from_stash(stash[j - 4:j], units[j - 4:j], dtype, departure)[1])
        y, pre = block_from_stash(stash[j:j + 4], units[j:j + 4], dtype, departure)
        o1, o2 = torch.relu(y[1]), torch.relu(y[2])
        dz3 = unit(j + 3, o2, g, pre, 1)
        dz2 = unit(j + 2, o1, conv_dx_ref(dz3, units[j + 3], 1, None, dtype), None, 1)
        dz1 = unit(j + 1, a, conv_dx_ref(dz2, units[j + 2], 3, None, dtype), None, 1)
        dz0 = unit(j, a, g, pre, 0)
        if d > 0:
            g = conv_dx_ref(dz1, units[j + 1], 1, None, dtype) + conv_dx_ref(dz0, units[j], 1, None, dtype)
    if operands is not None:
        operands[:] = ops
    return grads


def reduce_parts(parts):
    """cf_reduce_parts (csrc/gru_wgrad.hpp) in float32: parts [n_parts, F] -> [F].  Thread group g = 0 .. 3 adds parts g, g + 4,
    ... : four accumulators per trip while part c + 12 exists, the rest one by one into the first; (a0 + a1) + (a2 + a3) per
    group, (g0 + g1) + (g2 + g3) over the groups."""
    import torch
    n = parts.shape[0]
    red = []
    for g in range(4):
        a = [torch.zeros_like(parts[0]) for _ in range(4)]
        c = g
        while c + 12 < n:
            for i in range(4):
                a[i] = a[i] + parts[c + 4 * i]
            c += 16
        while c < n:
            a[0] = a[0] + parts[c]
            c += 4
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    return (red[0] + red[1]) + (red[2] + red[3])


def _wg_positions(t, n_wg, win):
    """[n, 35, C] -> [n_wg, trips, 8 groups, C]: position p = 8 trip + group of a workgroup's windows, zeros past the end."""
    import torch.nn.functional as F
    n, _, c = t.shape
    t = F.pad(t.float(), (0, 0, 0, 0, 0, n_wg * win - n)).reshape(n_wg, win * T, c)
    trips = (win * T + RT_PG - 1) // RT_PG
    return F.pad(t, (0, 0, 0, trips * RT_PG - win * T)).reshape(n_wg, trips, RT_PG, c)


def stack_chain_grads(units, operands, n):
    """The parameter gradients summed as the kernels sum them, in float32, from the float64 reference's operands rounded to
    float32: per workgroup and position group one chain over the thread's positions (fmaf for the weights and d gamma), the 8
    groups added in order, the workgroups through ``reduce_parts``."""
    import torch
    n_wg, win = workgroups(n)
    parts, sizes = [], []
    for j, (a_in, v, dz, zhat) in enumerate(operands):
        kw = unit_shape(j)[0]
        cols = torch.cat([shifted(a_in, d) for d in tap_offsets(kw)], 2)
        rows = cols.shape[2]
        a4, dz4, v4, zh4 = (_wg_positions(t, n_wg, win) for t in (cols, dz, v, zhat))
        s32 = bn_affine(units[j], torch.float64)[0].float().to(a4.device)
        accw = torch.zeros(n_wg, RT_PG, rows, CHANNELS, device=a4.device)
        sb, sg = torch.zeros(n_wg, RT_PG, CHANNELS, device=a4.device), torch.zeros(n_wg, RT_PG, CHANNELS, device=a4.device)
        for trip in range(a4.shape[1]):
            accw = _fma(a4[:, trip, :, :, None], dz4[:, trip, :, None, :], accw)
            sb = sb + v4[:, trip]
            sg = _fma(v4[:, trip], zh4[:, trip], sg)
        part = torch.cat([accw.reshape(n_wg, RT_PG, rows * CHANNELS), sb * s32, sg, sb], 2)
        tot = part[:, 0]
        for grp in range(1, RT_PG):
            tot = tot + part[:, grp]
        parts.append(tot)
        sizes.append(rows)
    flat = reduce_parts(torch.cat(parts, 1))
    out, o = [], 0
    for rows in sizes:
        d = {"kernel": flat[o:o + rows * CHANNELS].view(rows, CHANNELS)}
        o += rows * CHANNELS
        for k in ("bias", "gamma", "beta"):
            d[k] = flat[o:o + CHANNELS]
            o += CHANNELS
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ S. error measures
EDGE = [0, T - 1]


def forward_errors(got, ref):
    """got, ref: (z per unit, out).  ``edge``: out and the width-3 units' z on steps 0 and 34 alone."""
    (z, out), (z64, out64) = got, ref
    wide = [j for j in range(len(z)) if j % 4 == 2]
    return {"z": max(_rel(a, b) for a, b in zip(z, z64)), "out": _rel(out, out64), "out_window": _rel_window(out, out64),
            "edge": max([_rel(out[:, EDGE], out64[:, EDGE])] + [_rel(z[j][:, EDGE], z64[j][:, EDGE]) for j in wide])}


def grad_errors(got, ref):
    """got, ref: per unit {kernel, bias, gamma, beta} -> per unit kind the largest of the kernel's and the bias's error
    (``wgrad_*``) and of gamma's and beta's (``bn_*``), each tensor over its own maximum."""
    out = {}
    for j, (a, b) in enumerate(zip(got, ref)):
        kind = unit_kind(j)
        for q, keys in (("wgrad_", ("kernel", "bias")), ("bn_", ("gamma", "beta"))):
            out[q + kind] = max(out.get(q + kind, 0.0), max(_rel(a[k].reshape(b[k].shape), b[k]) for k in keys))
    return out


# ------------------------------------------------------------------------------------------------ T. inputs and references
# (windows or "capped", labels)
T_CASES = [(1, "mixed"), (11, "mixed"), (11, "ones"), (16, "mixed"), (17, "mixed"), (48, "mixed"), ("capped", "mixed")]
FEATURES = 128
PADDING_VALUE = 1e30


def capped_windows(n_cu):
    """The smallest tile count whose ceil(35 tiles / 32) workgroups exceed the cap of 2 per CU, minus 5 windows."""
    tiles = 1
    while (T * tiles + 31) // 32 <= 2 * n_cu:
        tiles += 1
    return 16 * tiles - 5


def head_waves(n, n_cu):
    """Waves of train_head_kernel at n windows: four per workgroup, ceil(35 tiles / 32) workgroups, at most 2 per CU."""
    tiles = (n + 15) // 16
    return 4 * max(1, min((T * tiles + 31) // 32, 2 * n_cu))


def head_inputs(n, labels="mixed", reach=None):
    """(input [npad, 35, 128] with 1e30 in the padding windows, dense kernel [128], bias [1], labels [n, 35]).  ``reach``: the
    dense kernel is scaled so that the float64 logits pass +-reach under label 0 and under label 1."""
    import torch
    gen = _gen(30, n, labels == "ones", reach or 0)
    npad = (n + 15) // 16 * 16
    x, w, b = _randn(gen, npad, T, FEATURES), _randn(gen, FEATURES) / float(np.sqrt(FEATURES)), 0.1 * _randn(gen, 1)
    lab = torch.ones(n, T) if labels == "ones" else (_rand(gen, n, T) < 0.4).float()
    x[n:] = PADDING_VALUE
    if reach is not None:
        s = x[:n].double().reshape(-1, FEATURES) @ w.double()
        l1 = lab.reshape(-1) > 0
        low = min(float(s[l1].max()), -float(s[l1].min()), float(s[~l1].max()), -float(s[~l1].min()))
        w = w * float(1.02 * reach / low)
    return x, w, b, lab


def head_ref(x, w, b, labels, dtype, departure=None):
    """Dense head with sigmoid cross-entropy over the n = len(labels) real windows of x [npad, 35, 128]: logits [n, 35], d input
    [n, 35, 128], d logit, per-position loss, mean loss, dense gradients."""
    import torch
    n, npad = labels.shape[0], x.shape[0]
    count = (npad if departure == "padded_count" else n) * T
    lab = labels.to(dtype)
    if departure == "label_one_window_off":
        lab = lab.roll(-1, 0)
    xd, wd, lab = x[:n].to(dtype).reshape(n * T, FEATURES), w.to(dtype), lab.reshape(-1)
    s = xd @ wd + b.to(dtype)
    dl = (torch.sigmoid(s) - lab) / count
    lossp = torch.clamp(s, min=0) - s * lab + torch.log1p(torch.exp(-s.abs()))
    return {"logits": s.reshape(n, T), "din": (dl[:, None] * wd).reshape(n, T, FEATURES), "dl": dl, "lossp": lossp, "lab": lab,
            "loss": lossp.sum() / count, "gw": xd.t() @ dl, "gb": dl.sum().reshape(1)}


def head_errors(got, ref):
    return {"logits": _rel(got["logits"], ref["logits"]), "din": _rel(got["din"], ref["din"]),
            "wgrad": max(_rel(got["gw"], ref["gw"]), _rel(got["gb"], ref["gb"])), "loss": loss_error(got["loss"], ref["loss"])}


def _pair_tree(v):
    """v [waves, 16, ...] -> [waves, ...]: the butterfly over the 16 windows of a lane quarter (lane ^ 1, 2, 4, 8)."""
    for _ in range(4):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def head_chain(x, w, b, ref, n_waves):
    """train_head_kernel and train_head_reduce_kernel in float32, from the float64 reference's d logit and per-position loss
    rounded to float32: the logit as one fmaf chain over the 32 features of a lane quarter (16 m + 4 q + r, m outer), the
    quarters added (q0 + q1) + (q2 + q3), then the bias; a wave's partial sums as one chain over its items (tile, step), item =
    wave + trip n_waves; the butterfly over the 16 windows; ``reduce_parts`` over the waves."""
    import torch
    npad, n = x.shape[0], ref["logits"].shape[0]
    tiles = npad // 16
    items = tiles * T
    x4 = x[:n].float().reshape(n * T, 8, 4, 4)                                       # [position, m, q, r]
    w4 = w.float().reshape(8, 4, 4)
    s = torch.zeros(n * T, 4, device=x.device)
    for m in range(8):
        for r in range(4):
            s = _fma(x4[:, m, :, r], w4[m, :, r], s)
    logits = (((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) + b.float()).reshape(n, T)

    def by_item(t):                                      # [n, 35, ...] of the real windows -> [trips, waves, 16, ...], zeros elsewhere
        t = t.float()
        t = torch.cat([t, t.new_zeros((npad - n,) + tuple(t.shape[1:]))], 0)
        t = t.reshape((tiles, 16, T) + tuple(t.shape[2:])).transpose(1, 2).reshape((items, 16) + tuple(t.shape[2:]))
        trips = (items + n_waves - 1) // n_waves
        t = torch.cat([t, t.new_zeros((trips * n_waves - items,) + tuple(t.shape[1:]))], 0)
        return t.reshape((trips, n_waves) + tuple(t.shape[1:]))

    h, dl, lp = by_item(x[:n]), by_item(ref["dl"].reshape(n, T)), by_item(ref["lossp"].reshape(n, T))
    dw = torch.zeros(n_waves, 16, FEATURES, device=x.device)
    db, loss = torch.zeros(n_waves, 16, device=x.device), torch.zeros(n_waves, 16, device=x.device)
    for trip in range(h.shape[0]):
        dw = _fma(h[trip], dl[trip][:, :, None], dw)
        db, loss = db + dl[trip], loss + lp[trip]
    tot = reduce_parts(torch.cat([_pair_tree(dw), _pair_tree(db)[:, None], _pair_tree(loss)[:, None]], 1))
    inv_count = torch.tensor(1.0 / (n * T), dtype=torch.float64).float().to(x.device)
    return {"logits": logits, "gw": tot[:FEATURES], "gb": tot[FEATURES:FEATURES + 1], "loss": tot[FEATURES + 1] * inv_count}


def head_chain_errors(chain, ref):
    return {"logits": _rel(chain["logits"], ref["logits"]), "wgrad": max(_rel(chain["gw"], ref["gw"]), _rel(chain["gb"], ref["gb"])),
            "loss": loss_error(chain["loss"], ref["loss"])}


# ------------------------------------------------------------------------------------------------ launches
@pytest.fixture(scope="module")
def engine():
    """One engine of the shipped geometry serves all cases: the stack's entry points take the block count per call."""
    from catfish_amd.engine import HipEngine
    eng = HipEngine(oracle.random_weights(seed=31), device=0, max_windows_per_pass=256)
    yield eng
    eng.close()


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _cuda(u):
    return {k: v.cuda() for k, v in u.items()}


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    import torch
    return bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------ S. the conv stack
@pytest.mark.parametrize("n,n_blocks", S_CASES)
def test_res_stack_matches_float64(engine, n, n_blocks):
    """cf_res_train_forward (Z, out) and cf_res_train_backward from the settled float64 stash, in the case's launch regime."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    x, units, d_out = stack_inputs(n, n_blocks)
    for u in units:
        assert float(u["gamma"][1]) == 0.0 and float(u["beta"][1]) > 0 and float(u["gamma"][2]) < 0 and float(u["var"][3]) == 0.0
    n_wg, win = workgroups(n)
    nf = int(lib.cf_res_train_param_floats(n_blocks))
    ws_floats = int(lib.cf_res_train_workspace_floats(n_blocks, n))
    flat = stack_flat(units).cuda()
    assert flat.numel() == nf and ws_floats == n_wg * nf and n_wg == (n if n <= RT_SMALL_BATCH else (n + 1) // 2)
    stash, moved = settle_stash(stack_forward(x, units, torch.float64)[0], units)            # on the CPU: the host file's tensors
    assert moved < 0.01
    x, units, d_out, stash = x.cuda(), [_cuda(u) for u in units], d_out.cuda(), [z.cuda() for z in stash]

    # ---- forward
    z_k, out_k = _nan(4 * n_blocks, n, T, CHANNELS), _nan(n, T, CHANNELS)
    N.check(lib.cf_res_train_forward(hd, n_blocks, N._p(flat), N._p(x), N._p(z_k), N._p(out_k), n, _stream()))
    z64, outs64 = stack_forward(x, units, torch.float64)
    assert all(float(o.abs().max()) < 100.0 for o in outs64)
    z32, outs32 = stack_forward(x, units, torch.float32)
    fwd_k = forward_errors((list(z_k), out_k), (z64, outs64[-1]))
    fwd_t = forward_errors((z32, outs32[-1]), (z64, outs64[-1]))

    # ---- backward from the given stash
    z_in = torch.stack(stash).contiguous()
    ws, grads = _nan(ws_floats), _nan(nf)
    N.check(lib.cf_res_train_backward(hd, n_blocks, N._p(flat), N._p(x), N._p(z_in), N._p(d_out), N._p(ws), ws_floats, N._p(grads), n, _stream()))
    ws2, grads2 = _nan(ws_floats), _nan(nf)
    N.check(lib.cf_res_train_backward(hd, n_blocks, N._p(flat), N._p(x), N._p(z_in), N._p(d_out), N._p(ws2), ws_floats, N._p(grads2), n, _stream()))
    assert not bool(torch.isnan(grads).any()) and not bool(torch.isnan(ws).any())            # every slot written
    assert _same_bits(grads, grads2) and _same_bits(ws, ws2)
    g_k = split_grads(grads, n_blocks)
    for u in g_k:
        assert float(u["mean"].abs().max()) == 0.0 and float(u["var"].abs().max()) == 0.0    # moving statistics do not train
    operands = []
    g64 = stack_backward(x, units, stash, d_out, torch.float64, operands=operands)
    g32 = stack_backward(x, units, stash, d_out, torch.float32)
    g_c = stack_chain_grads(units, operands, n)
    case = "%d windows, %d blocks, %d workgroups of %d" % (n, n_blocks, n_wg, win)
    _check("S", case, dict(fwd_k, **grad_errors(g_k, g64)), dict(fwd_t, **grad_errors(g32, g64)), grad_errors(g_c, g64))


def test_res_stack_refuses_bad_block_counts_and_a_short_workspace(engine):
    """0 and 5 blocks, and a workspace one float short: an error before any launch, nothing written."""
    import torch
    from catfish_amd import _native as N
    lib, hd = engine._lib, engine._handle
    n = 3
    x, units, d_out = stack_inputs(n, 1)
    flat5 = torch.cat([stack_flat(units)] * 20).cuda()                                        # room for any admitted layout
    x, d_out = x.cuda(), d_out.cuda()
    assert int(lib.cf_res_train_param_floats(0)) == 0 and int(lib.cf_res_train_param_floats(5)) == 0
    assert int(lib.cf_res_train_workspace_floats(0, n)) == 0 and int(lib.cf_res_train_workspace_floats(5, n)) == 0
    z, out, ws, grads = _nan(20, n, T, CHANNELS), _nan(n, T, CHANNELS), _nan(8 * flat5.numel()), _nan(flat5.numel())
    for n_blocks in (0, 5):
        with pytest.raises(ValueError):
            N.check(lib.cf_res_train_forward(hd, n_blocks, N._p(flat5), N._p(x), N._p(z), N._p(out), n, _stream()))
        with pytest.raises(ValueError):
            N.check(lib.cf_res_train_backward(hd, n_blocks, N._p(flat5), N._p(x), N._p(z), N._p(d_out), N._p(ws), ws.numel(), N._p(grads), n,
                                              _stream()))
    need = int(lib.cf_res_train_workspace_floats(1, n))
    with pytest.raises(ValueError):
        N.check(lib.cf_res_train_backward(hd, 1, N._p(flat5), N._p(x), N._p(z), N._p(d_out), N._p(ws), need - 1, N._p(grads), n, _stream()))
    torch.cuda.synchronize()
    assert _all_nan(z) and _all_nan(out) and _all_nan(ws) and _all_nan(grads)


# ------------------------------------------------------------------------------------------------ T. the head
def _run_head(engine, x_frag, w, b, labels, n, npad, with_logits=True):
    """cf_train_head on NaN outputs -> (d input [npad, 35, 128], logits [npad, 35] or None, grads [129], loss [1], workspace)."""
    from catfish_amd import _native as N
    from catfish_amd.native_train import frag_to_nat
    lib, hd = engine._lib, engine._handle
    ws_floats = int(lib.cf_train_head_workspace_floats(hd, npad))
    dy, logits, ws, grads, loss = _nan(*x_frag.shape), _nan(npad, T), _nan(ws_floats), _nan(FEATURES + 1), _nan(1)
    N.check(lib.cf_train_head(hd, N._p(x_frag), N._p(w), N._p(b), N._p(labels), n, N._p(dy), N._p(logits) if with_logits else None, N._p(ws),
                              ws_floats, N._p(grads), N._p(loss), _stream()))
    return {"din": frag_to_nat(dy), "logits": logits if with_logits else None, "grads": grads, "loss": loss, "dy": dy}


def _head_case(engine, n, labels, reach=None):
    import torch
    from catfish_amd.native_train import nat_to_frag
    n_cu = engine.launch_regimes()["n_cu"]
    capped = n == "capped"
    if capped:
        n = capped_windows(n_cu)
    x, w, b, lab = head_inputs(n, labels, reach)
    npad = x.shape[0]
    assert npad - n == {1: 15, 11: 5, 16: 0, 17: 15, 48: 0}.get(n, 5)
    assert npad == n or float(x[n:].min()) > 0.99 * PADDING_VALUE
    waves = int(engine._lib.cf_train_head_workspace_floats(engine._handle, npad)) // HEAD_PART
    uncapped = 4 * ((T * (npad // 16) + 31) // 32)
    assert waves == head_waves(n, n_cu) and (waves == 8 * n_cu and uncapped > waves if capped else waves == uncapped < 8 * n_cu)
    x, w, b, lab = x.cuda(), w.cuda(), b.cuda(), lab.cuda().contiguous()
    x_frag = nat_to_frag(x)
    got = _run_head(engine, x_frag, w, b, lab, n, npad)
    again = _run_head(engine, x_frag, w, b, lab, n, npad)
    bare = _run_head(engine, x_frag, w, b, lab, n, npad, with_logits=False)                  # the call NativeTrainStep.run makes
    for other in (again, bare):
        assert _same_bits(got["dy"], other["dy"]) and _same_bits(got["grads"], other["grads"]) and _same_bits(got["loss"], other["loss"])
    assert _same_bits(got["logits"], again["logits"])
    assert npad == n or float(got["din"][n:].abs().max()) == 0.0                             # exact zeros in the padding windows
    assert _all_nan(got["logits"][n:]) and bool(torch.isfinite(got["logits"][:n]).all())
    for k in ("din", "grads", "loss"):
        assert bool(torch.isfinite(got[k]).all()), k
    ref, yard = head_ref(x, w, b, lab, torch.float64), head_ref(x, w, b, lab, torch.float32)
    chain = head_chain(x, w, b, ref, waves)
    res = {"logits": got["logits"][:n], "din": got["din"][:n], "gw": got["grads"][:FEATURES], "gb": got["grads"][FEATURES:], "loss": got["loss"][0]}
    return n, npad, waves, ref, head_errors(res, ref), head_errors(yard, ref), head_chain_errors(chain, ref)


@pytest.mark.parametrize("n,labels", T_CASES)
def test_train_head_matches_float64(engine, n, labels):
    """cf_train_head: logits, d input, dense gradients and the loss; padding windows of 1e30 contribute nothing."""
    n, npad, waves, ref, e_k, e_t, e_c = _head_case(engine, n, labels)
    assert labels == "ones" or n < 8 or 0.2 < float(ref["lab"].mean()) < 0.6  # both labels among the positions
    _check("T", "%d windows of %d, %d waves, labels %s" % (n, npad, waves, labels), e_k, e_t, e_c)


def test_train_head_stays_finite_with_saturated_logits(engine):
    """The dense kernel scaled so that the float64 logits pass +-100 under both labels (expf(100) overflows float32): the loss
    and every gradient stay finite and meet the same bounds."""
    n, npad, waves, ref, e_k, e_t, e_c = _head_case(engine, 48, "mixed", reach=100.0)
    s, one = ref["logits"].reshape(-1), ref["lab"] > 0
    for sel in (one, ~one):
        assert float(s[sel].max()) > 100.0 and float(s[sel].min()) < -100.0
    _check("T", "saturated: %d windows of %d, %d waves" % (n, npad, waves), e_k, e_t, e_c)
