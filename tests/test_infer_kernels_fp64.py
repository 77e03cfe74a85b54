"""The inference kernels against float64 on LOGITS, per launch shape (GPU).

The other inference parity tests compare sigmoid outputs with the float64 oracle at 1e-4, the largest element of a whole call.
The sigmoid divides a logit error by at least 4 and with random weights no probability leaves 0.51 .. 0.76, so that gate is 250 x
(fp32) and 20 x (bf16x3) looser than the kernels: tests/test_infer_parity_host.py plants seven defects that pass it.  Here the
quantities are, each ``max|d| / max|ref|`` against ``oracle.forward(..., np.float64, return_stages=True)`` (in slabs of 2048):

  logits          ``infer_host(x, return_logits=True)``
  logits_window   each window's error over that window's own largest |logit| (``_rel_window``, which has no floor: a window of 35
                  logits that are all tiny would need one; the smallest window maximum met here is printed with every case)
  stages          tuned fp32 path only (``debug_stage``): res1 and gru0 / gru1, every window of the pass
  probs           absolute error: the weakest of the four, kept

  P  the tuned fp32 path (64 / 32), window counts from ``engine.launch_regimes()``: hoisted / cooperative / throughput kernels either
     side of both switches, the throughput kernel with a ragged last tile, 1 and 17 windows; the fused launch (``fuse_layers=True``)
     one count below and one above the auto threshold ``fuse_auto_min`` (98 177 windows on 256 CUs: the logits of a 1024-window
     sample with both ends and the ragged tile, the stages on the first 256 windows; a float64 reference of the whole call would
     take a minute).  Random weights (seed 5) at every count, the bundled checkpoint, whose logits saturate, at two.
  Q  the any-size fp32 path per LDS class and wave count: 16 / 48 / 96 (three state arrays, 8 waves), 112 / 160 (``h_via_y``, 8
     waves; 160 at 8 waves is the launch at exactly 163 840 B), 176 / 256 (``h_via_y``, 4 waves), each at 1 and 17 windows and at
     2, 3, 4 and 8 waves (4 in the last class) with a ragged last tile and a partly empty last workgroup; the two-tile kernel
     at (64, 64) and (128, 64) and 2 n_cu + 1 tiles; (48, 80, 3, 2), whose second block takes gen_conv_kernel's shortcut path, and
     the plain RNN (112, 0, 2, 0).  Every case asserts kernel, waves, LDS bytes and ``h_via_y`` through ``cf_anysize_infer_shape``.
  R  bf16x3: the tuned pipelined kernel and its unpipelined form (CATFISH_BF16_PIPE=0) at 33, 257 and coop_max + 3 windows, and
     gen_gru_kernel<false, true> / gen_conv_kernel<true> at 16, 48, 112, 176 and 256 units at one window, three tiles and two
     waves.  Each case asserts that its logits are not bit-equal to the fp32 engine's: the mode ran.

Yardsticks and bounds.  A measuring run (CATFISH_PARITY_LOG names a file) records for every case and quantity the kernels' error
and, against the same float64 reference, the error of ``oracle.forward(x, w, np.float32)`` (an independent fp32 implementation with
another summation order), of ``model_forward(..., act="kernel")`` (the float64 network with sigmoid and tanh evaluated as the
kernels evaluate them: exp2 of the pre-scaled argument, 1 + e, reciprocal, one fma, each in float32) and, for R, of
``model_forward(..., x3=True)``: the float64 network with every matrix product the kernels split -- the convolutions with more
than one input channel on their batch-norm-folded weights, ``[x | h] W_g`` and ``[x | r.h] W_c`` on weights scaled by -log2(e) and
2 log2(e) in double and rounded to float before the split, the activations split from their fp32 values where they enter a
product (the tuned kernels store them split, the any-size kernels split them on the fly: the same numbers) -- replaced by
``a_hi w_hi + a_lo w_hi + a_hi w_lo``; block 0's one-channel convolutions and the dense head stay exact, as in the kernels.  The
yardstick of a quantity is the float32 oracle's error, plus the emulation's in R, plus the activation term for the quantities named in
``ACTIVATION_TERM``; the asserted bound is 4 x the largest yardstick over the section, rounded down to three digits, and never
looser than the older tests (``OLDER_BOUNDS``: probabilities 1e-4, stages 2e-5, logits 4e-4).  ``BOUNDS`` holds the constants,
profiles/infer_kernels_fp64_parity.jsonl the rows, tests/test_infer_parity_host.py checks the one against the other.

As measured (MI355X, 256 CUs) every quantity meets the rule with the float32 oracle (and the emulation) alone: no quantity needed
the activation term (``ACTIVATION_TERM`` is empty; the term is recorded in every row all the same), and one fell back to the older
bound, P's stages (4 x 7.13e-6 > 2e-5).  P logits 2.54e-6 (per window 8.18e-6), stages 2e-5, probabilities 1.61e-6; Q logits 4.87e-6
(per window 9.26e-6), probabilities 5.15e-7; R logits 4.93e-5 (per window 1.44e-4), probabilities 3.19e-5: 40 to 160 x tighter than the
gate in fp32, 3 to 8 x in bf16x3.  Case by case the kernels reach 1.44 x their case's yardstick in P (the stages at one window), 2.85 x
in Q (112 units at one window, 5.7e-7 against 2.0e-7: where the approximate ``v_rcp`` / ``v_exp`` of the gate activations show, as in
the training modules) and 1.16 x in R (the checkpoint per window, 4.18e-5 against 3.60e-5: the kernels sit on the emulation).  The
two thinnest margins: P's stages at 0.44 of their bound (8.82e-6, the checkpoint's gru1 at 4099 windows) and Q's per-window logits at
0.45 (4.18e-6, the plain RNN (112, 0, 2, 0) at 2059 windows).  The runs are deterministic; if a reordering of sums trips one,
re-measure, do not widen by hand.  The longest case is 256 units at 14 347 windows: 1.6 s in an ordinary run, 4.5 s in the
measuring run (4.9 s there for the tuned bf16x3 case at 4099 windows, which also computes the emulation).

Compared with float64 here and nowhere before: every any-size launch of more than one wave except 64 / 128 units (16, 48, 96, 112,
160, 176 and 256 units at 2, 3, 4 and 8 waves, the 160-unit launch at exactly 163 840 B among them), the two-tile kernel itself (so
far only held to the one-tile kernel plus 83 sampled windows), the fused launch and the cooperative / throughput switches on logits,
stages and per window, the unpipelined bf16x3 kernel, and bf16x3 at 16, 48, 112 and 176 units.

``model_forward(..., bf16=True)`` and its float32 implementation (``arith="float32"``) are the rounding scheme of plain bf16; the
module that holds those kernels to it is tests/test_infer_bf16_parity.py.
"""
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from test_train_kernels_fp64 import T, _measuring, _rel, _rel_window, _stamp

pytestmark = pytest.mark.gpu

# quantity -> asserted bound = min(4 x largest yardstick over the section, older bound).  The largest yardsticks in
# profiles/infer_kernels_fp64_parity.jsonl (MI355X, 256 CUs; R: emulation + float32 oracle), and the kernels' largest error next to them:
#   P.logits 6.374e-07 (kernels 6.13e-07)   P.logits_window 2.047e-06 (2.28e-06)   P.stages 7.130e-06 (8.82e-06)   P.probs 4.036e-07 (3.65e-07)
#   Q.logits 1.219e-06 (1.58e-06)   Q.logits_window 2.317e-06 (4.18e-06)   Q.probs 1.288e-07 (1.44e-07)
#   R.logits 1.141e-05 + 9.28e-07 (1.12e-05)   R.logits_window 3.478e-05 + 1.23e-06 (4.18e-05)   R.probs 7.60e-06 + 3.9e-07 (6.15e-06)
# 4 x each, rounded down, is below the older bound of its quantity and so is the bound, except for P.stages: 4 x 7.13e-6 is above
# the 2e-5 of the older tests, which stays (the checkpoint's gru1 at 4099 windows; random weights give 3.8e-7).
BOUNDS = {
    "P.logits": 2.54e-6, "P.logits_window": 8.18e-6, "P.stages": 2e-5, "P.probs": 1.61e-6,
    "Q.logits": 4.87e-6, "Q.logits_window": 9.26e-6, "Q.probs": 5.15e-7,
    "R.logits": 4.93e-5, "R.logits_window": 1.44e-4, "R.probs": 3.19e-5,
}
# what the older tests allow: the 1e-4 gate on probabilities (a logit error is divided by at least 4 on its way there, so the gate
# implies no more than 4e-4 on a logit; taken relative to max|logit|, which is about 1 with random weights), 2e-5 on the stages
OLDER_BOUNDS = {"P.logits": 4e-4, "P.logits_window": 4e-4, "P.stages": 2e-5, "P.probs": 1e-4,
                "Q.logits": 4e-4, "Q.logits_window": 4e-4, "Q.probs": 1e-4,
                "R.logits": 4e-4, "R.logits_window": 4e-4, "R.probs": 1e-4}
# quantities whose yardstick carries the activation term (the approximate reciprocal / exponential of the gate activations)
ACTIVATION_TERM = ()
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "infer_kernels_fp64_parity.jsonl")
SLAB = 2048              # windows per evaluation of a reference
LDS_LIMIT = 163840
LOG2E = 1.4426950408889634
GATE_SCALE, CAND_SCALE = -LOG2E, 2.0 * LOG2E       # CF_GATE_SCALE / CF_CAND_SCALE of csrc/catfish_hip.hip


def yardstick(row):
    """The yardstick of one profile row: float32 oracle (+ emulation of the scheme in R) (+ activation term where named)."""
    key = "%s.%s" % (row["section"], row["quantity"])
    y = row["oracle_fp32"]
    if row["section"] == "R":
        y += row["emulation"]
    if key in ACTIVATION_TERM:
        y += row["activation"]
    return y


def bounds_from_profile(path=PROFILE):
    """{quantity: min(4 x largest yardstick in the profile, older bound)}: what ``BOUNDS`` may not exceed."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            key = "%s.%s" % (row["section"], row["quantity"])
            worst[key] = max(worst.get(key, 0.0), yardstick(row))
    return {k: min(4.0 * v, OLDER_BOUNDS[k]) for k, v in worst.items()}


def _record(section, case, quantity, kernel, yards):
    """Print the row (always, before any assertion) and append it to the file CATFISH_PARITY_LOG names.  ``yards``: None or
    dict(oracle_fp32, activation, emulation)."""
    row = {"section": section, "case": case, "quantity": quantity, "kernel": float(kernel)}
    for k in ("oracle_fp32", "activation", "emulation"):
        row[k] = None if yards is None or yards.get(k) is None else float(yards[k])
    print("parity %s" % json.dumps(row))
    path = os.environ.get("CATFISH_PARITY_LOG")
    if path and yards is not None:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(_stamp(), **row)) + "\n")


def _check(section, case, kernel, yards):
    """kernel: {quantity: error}; yards: None or {name: {quantity: error}}.  All are recorded, then all are asserted."""
    for q, k in kernel.items():
        _record(section, case, q, k, None if yards is None else {name: e.get(q) for name, e in yards.items()})
    bad = {q: (k, BOUNDS["%s.%s" % (section, q)]) for q, k in kernel.items() if not k <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ the network in numpy, float64
def bf16_round(v):
    """float32 array -> the nearest bf16 (ties to even) as float32, on the bit pattern (finite values)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def split(v, keep_lo=True):
    """float64 -> (hi, lo) as float64: hi = bf16(float32(v)), lo = bf16(float32(v) - hi) (gen_split / split8 of the kernels)."""
    f = np.asarray(v).astype(np.float32)
    hi = bf16_round(f)
    lo = bf16_round(f - hi) if keep_lo else np.zeros_like(hi)
    return hi.astype(np.float64), lo.astype(np.float64)


class _Product(object):
    """``a @ w`` exactly, or as the bf16x3 kernels evaluate it: w scaled in double, rounded to float, split; a split from its
    float32 value; a_hi w_hi + a_lo w_hi + a_hi w_lo, un-scaled again (the kernels feed the scaled sum to exp2).
    With ``bf16`` as the plain bf16 kernels evaluate it: ``a_hi @ w_hi`` with w_hi = bf16(float(scale w)) and a_hi = bf16(float(a)),
    accumulated in float64.  Departures from that scheme, for tests/test_infer_bf16_parity_host.py: ``late_scale`` (the weights are
    rounded before they are scaled), ``keep`` (an index of the weights left in float), ``rounded=False`` (a enters as it is)."""

    def __init__(self, x3, bf16=False):
        assert not (x3 and bf16)
        self.x3, self.bf16 = x3, bf16

    def weights(self, w, scale=1.0, late_scale=False, keep=None):
        w = np.asarray(w, dtype=np.float64)
        if self.bf16:
            f = (w if late_scale else w * scale).astype(np.float32)
            hi = bf16_round(f).astype(np.float64)
            if keep is not None:
                hi[keep] = f[keep]
            return (hi * scale if late_scale else hi, None, scale)
        if not self.x3:
            return (w,)
        hi, lo = split((w * scale).astype(np.float32))
        return (hi + lo, hi, scale)

    def __call__(self, a, wp, keep_lo=True, rounded=True):
        if self.bf16:
            return ((split(a, False)[0] if rounded else np.asarray(a, dtype=np.float64)) @ wp[0]) / wp[2]
        if not self.x3:
            return a @ wp[0]
        ah, al = split(a, keep_lo)
        return (ah @ wp[0] + al @ wp[1]) / wp[2]


def _sigmoid_kernel(pre):
    """cf_sigmoid_pre on the pre-scaled argument, every operation in float32 (correctly rounded here; v_exp_f32 and v_rcp_f32 are
    good to 1 ulp)."""
    with np.errstate(over="ignore"):
        e = np.exp2((pre * GATE_SCALE).astype(np.float32))
    return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float64)


def _tanh_kernel(pre):
    """cf_tanh_pre: fma(-2, rcp(1 + exp2(a)), 1), one rounding for the fma."""
    with np.errstate(over="ignore"):
        e = np.exp2((pre * CAND_SCALE).astype(np.float32))
    r = (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float64)
    return (1.0 - 2.0 * r).astype(np.float32).astype(np.float64)


def _gru_direction(x, wg, bg, wc, bc, reverse, mm, act, defect):
    """oracle.gru_direction in float64 with the products through ``mm``; ``defect``: set of names planted in this direction."""
    n, t, cin = x.shape
    hsz = wc.shape[1]
    late = "scale_after_rounding" in defect
    block = (slice(16, 32), slice(0, 16)) if "block_unrounded" in defect else None
    wgx, wgh, wcx, wch = (mm.weights(wg[:cin], GATE_SCALE, late), mm.weights(wg[cin:], GATE_SCALE, late),
                          mm.weights(wc[:cin], CAND_SCALE, late), mm.weights(wc[cin:], CAND_SCALE, late, keep=block))
    x2 = x.reshape(n * t, cin)
    xg = (mm(x2, wgx) + bg).reshape(n, t, 2 * hsz)             # the input's share of both pre-activations, all steps at once
    xc = (mm(x2, wcx) + bc).reshape(n, t, hsz)
    sigmoid, tanh = (_sigmoid_kernel, _tanh_kernel) if act == "kernel" else (oracle._sigmoid, np.tanh)
    h = np.zeros((n, hsz))
    out = np.empty((n, t, hsz))
    for s in (range(t - 1, -1, -1) if reverse else range(t)):
        pre = xg[:, s] + mm(h, wgh, keep_lo="state_hi_only" not in defect)
        gates = sigmoid(pre)
        if "sigmoid_off" in defect:
            gates = gates + 1e-5 * np.sin(1e3 * pre)
        r, u = gates[:, :hsz], gates[:, hsz:]
        c = tanh(xc[:, s] + mm(r * h, wch, keep_lo="rh_hi_only" not in defect, rounded="rh_unrounded" not in defect))
        if "tanh_off" in defect:
            c = c + 1e-5 * np.sin(1e3 * c)
        h = u * h + (1 - u) * c
        out[:, s] = h
    return out


def _folded(w, j):
    """Conv unit j with its batch norm folded in, in double -> (kernel [taps, cin, cout], the 1 / sqrt scale [cout], bias [cout])."""
    k = np.asarray(w[oracle.conv_names(j) + "/kernel"], dtype=np.float64)
    g = lambda name: np.asarray(w[oracle.bn_names(j) + "/" + name], dtype=np.float64)      # noqa: E731
    inv = g("gamma") / np.sqrt(g("moving_variance") + oracle.BN_EPS)
    bias = (np.asarray(w[oracle.conv_names(j) + "/bias"], dtype=np.float64) - g("moving_mean")) * inv + g("beta")
    return k, inv, bias


def _conv_bn(x, w, j, mm, rounded=True):
    """conv1d SAME + inference batch norm, folded as the packers fold it: W' = W gamma / sqrt(var + eps), b' = (b - mean) gamma /
    sqrt(var + eps) + beta.  One input channel: plain fp32 arithmetic in every kernel, exact here."""
    k, inv, bias = _folded(w, j)
    n, t, cin = x.shape
    taps, left = k.shape[0], (k.shape[0] - 1) // 2
    xp = np.zeros((n, t + taps - 1, cin))
    xp[:, left:left + t] = x
    mm = mm if cin > 1 else _Product(False)
    out = bias
    for i in range(taps):
        out = out + mm(np.ascontiguousarray(xp[:, i:i + t]).reshape(n * t, cin), mm.weights(k[i] * inv), rounded=rounded).reshape(n, t, -1)
    return out


def _fma32(a, b, c):
    """a b + c on float32 arrays with the product exact (in double): rounded to double, then to float.  A true fma rounds once;
    the two agree except where the double lands on a tie of the float grid."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _conv_bn_f32(x, w, j):
    """``_conv_bn`` as the plain bf16 kernels compute it, float32 throughout: folded weights and bias rounded to float; one input
    channel as one fma; otherwise bias + sum over taps of bf16(x) @ bf16(W'), products and sums in float32."""
    k, inv, bias = _folded(w, j)
    n, t, cin = x.shape
    taps, left = k.shape[0], (k.shape[0] - 1) // 2
    b32 = bias.astype(np.float32)
    if cin == 1:
        assert taps == 1
        return _fma32((k[0, 0] * inv).astype(np.float32), x, b32)
    xp = np.zeros((n, t + taps - 1, cin), dtype=np.float32)
    xp[:, left:left + t] = bf16_round(x)
    out = np.broadcast_to(b32, (n * t, b32.shape[0]))
    for i in range(taps):
        out = out + np.ascontiguousarray(xp[:, i:i + t]).reshape(n * t, cin) @ bf16_round((k[i] * inv).astype(np.float32))
    return out.reshape(n, t, -1)


def _gru_direction_f32(x, wg, bg, wc, bc, reverse):
    """One direction as gru_bf16_pipe_kernel / gru_layer_bf16_kernel<., ., 1> compute it, float32 throughout and in the pre-scaled
    domain: weights bf16(float(scale W)), biases float(scale b), bf16(x), bf16(h) and bf16(r h) into the products, sigmoid =
    rcp(1 + exp2(.)), tanh = fma(-2, rcp(1 + exp2(.)), 1), h = fma(u, h - c, c); h itself stays float32."""
    f32 = np.float32
    n, t, cin = x.shape
    hsz = wc.shape[1]
    wgs, wcs = bf16_round((wg * GATE_SCALE).astype(f32)), bf16_round((wc * CAND_SCALE).astype(f32))
    x2 = bf16_round(x).reshape(n * t, cin)
    xg = ((bg * GATE_SCALE).astype(f32) + x2 @ wgs[:cin]).reshape(n, t, 2 * hsz)
    xc = ((bc * CAND_SCALE).astype(f32) + x2 @ wcs[:cin]).reshape(n, t, hsz)
    one = f32(1.0)
    h = np.zeros((n, hsz), dtype=f32)
    out = np.empty((n, t, hsz), dtype=f32)
    with np.errstate(over="ignore"):
        for s in (range(t - 1, -1, -1) if reverse else range(t)):
            gates = one / (one + np.exp2(xg[:, s] + bf16_round(h) @ wgs[cin:]))
            r, u = gates[:, :hsz], gates[:, hsz:]
            c = _fma32(f32(-2.0), one / (one + np.exp2(xc[:, s] + bf16_round(r * h) @ wcs[cin:])), one)
            h = _fma32(u, h - c, c)
            out[:, s] = h
    return out


def _model_forward_bf16_f32(x, w, n_layers, n_layers_res):
    """The second implementation of the plain bf16 scheme (``model_forward(..., bf16=True, arith="float32")``): what the kernels do
    in fp32 is done in float32 here, with numpy's summation order and correctly rounded exp2 and reciprocal."""
    f32 = np.float32
    a = np.asarray(x, dtype=f32)
    a = a[:, :, None] if a.ndim == 2 else a
    stages = {}
    zero = f32(0.0)
    for d in range(n_layers_res):
        sc = _conv_bn_f32(a, w, 4 * d)
        o = np.maximum(_conv_bn_f32(a, w, 4 * d + 1), zero)
        o = np.maximum(_conv_bn_f32(o, w, 4 * d + 2), zero)
        o = np.maximum(_conv_bn_f32(o, w, 4 * d + 3), zero)
        a = np.maximum(o + sc, zero)
        stages["res%d" % d] = a
    for layer in range(n_layers):
        outs = []
        for dname, rev in (("fw", False), ("bw", True)):
            p = oracle.gru_prefix(layer, dname)
            outs.append(_gru_direction_f32(a, *(np.asarray(w[p + k], dtype=np.float64) for k in
                                                ("/gates/kernel", "/gates/bias", "/candidate/kernel", "/candidate/bias")), reverse=rev))
        a = np.concatenate(outs, axis=2)
        stages["gru%d" % layer] = a
    dw = np.asarray(w["final_fully_connected/kernel"], dtype=f32)
    hsz = a.shape[2] // 2
    a2 = a.reshape(-1, a.shape[2])
    logits = a2[:, :hsz] @ dw[:hsz] + a2[:, hsz:] @ dw[hsz:] + np.asarray(w["final_fully_connected/bias"], dtype=f32)
    stages["logits"] = logits.reshape(-1)
    return (f32(1.0) / (f32(1.0) + np.exp(-logits))).reshape(-1), stages


BF16_DEFECTS = {"rh_unrounded", "block_unrounded", "scale_after_rounding", "conv_in_unrounded", "dense_on_bf16_h"}


def model_forward(x, w, n_layers=3, n_layers_res=2, x3=False, act="exact", defects=(), bf16=False, arith="float64"):
    """The network of ``oracle.forward`` in float64 -> (probs [N * 35], stages), with options: ``x3`` the split products of the
    bf16x3 kernels, ``act="kernel"`` the kernels' sigmoid / tanh, ``defects`` (name, layer or None for all, direction or None)
    triples planted in the recurrences: "state_hi_only" (the state enters the gates' product without its lo part), "rh_hi_only"
    (r.h enters the candidate's product without its lo part), "sigmoid_off" / "tanh_off" (1e-5 sin(1e3 .) added).

    ``bf16``: the rounding scheme of the plain bf16 kernels (``_Product``): a_hi @ w_hi, accumulated in float64, for every product
    x3 splits; the layer input, h, r.h and the conv intermediates are rounded where they enter a product and nowhere else (block
    0's one-channel convolutions, the shortcut sum, biases, the state between steps and the dense head, which runs on the fp32 h,
    stay exact).  With ``arith="float32"`` the same scheme in the kernels' own arithmetic (``_model_forward_bf16_f32``).  Defects
    of the bf16 scheme: "rh_unrounded" (r.h enters the candidate's product as it is), "block_unrounded" (rows 16 .. 31, columns
    0 .. 15 of the candidate's recurrent kernel stay in float), "scale_after_rounding" (weights rounded, then scaled),
    "conv_in_unrounded" (the 32-channel convolutions take their inputs as they are), "dense_on_bf16_h" (the head reads bf16(h))."""
    if arith == "float32":
        assert bf16 and not x3 and act == "exact" and not defects, "the float32 implementation is that of the plain bf16 scheme"
        return _model_forward_bf16_f32(x, w, n_layers, n_layers_res)
    assert arith == "float64", arith
    mm = _Product(x3, bf16)
    everywhere = {name for name, l, d in defects if l is None and d is None}
    assert bf16 or not {name for name, _, _ in defects} & BF16_DEFECTS, "these defects are departures from the bf16 scheme"
    rounded = "conv_in_unrounded" not in everywhere
    a = np.asarray(x, dtype=np.float64)
    a = a[:, :, None] if a.ndim == 2 else a
    stages = {}
    for d in range(n_layers_res):
        sc = _conv_bn(a, w, 4 * d, mm, rounded)
        o = np.maximum(_conv_bn(a, w, 4 * d + 1, mm, rounded), 0)
        o = np.maximum(_conv_bn(o, w, 4 * d + 2, mm, rounded), 0)
        o = np.maximum(_conv_bn(o, w, 4 * d + 3, mm, rounded), 0)
        a = np.maximum(o + sc, 0)
        stages["res%d" % d] = a
    for layer in range(n_layers):
        outs = []
        for dname, rev in (("fw", False), ("bw", True)):
            p = oracle.gru_prefix(layer, dname)
            planted = {name for name, l, d in defects if l in (None, layer) and d in (None, dname)}
            outs.append(_gru_direction(a, *(np.asarray(w[p + k], dtype=np.float64) for k in
                                            ("/gates/kernel", "/gates/bias", "/candidate/kernel", "/candidate/bias")),
                                       reverse=rev, mm=mm, act=act, defect=planted))
        a = np.concatenate(outs, axis=2)
        stages["gru%d" % layer] = a
    if "dense_on_bf16_h" in everywhere:
        a = split(a, False)[0]
    logits = (a.reshape(-1, a.shape[2]) @ np.asarray(w["final_fully_connected/kernel"], dtype=np.float64)
              + np.asarray(w["final_fully_connected/bias"], dtype=np.float64))
    stages["logits"] = logits.reshape(-1)
    return oracle._sigmoid(logits).reshape(-1), stages


def in_slabs(fn, x, keep=("logits",)):
    """``fn(x) -> (probs, stages)`` over slabs of SLAB windows, several slabs at a time -> {"probs": [N, 35], "logits": [N, 35],
    kept stages}."""
    from concurrent.futures import ThreadPoolExecutor
    parts = {k: [] for k in ("probs",) + tuple(keep)}
    starts = list(range(0, len(x), SLAB))
    with ThreadPoolExecutor(max_workers=min(8, len(starts))) as pool:      # numpy's element-wise exp and tanh run on one core each
        results = list(pool.map(lambda a: fn(x[a:a + SLAB]), starts))
    for a, (probs, stages) in zip(starts, results):
        m = len(x[a:a + SLAB])
        parts["probs"].append(np.asarray(probs, dtype=np.float64).reshape(m, T))
        for k in keep:
            v = np.asarray(stages[k], dtype=np.float64)
            parts[k].append(v.reshape(m, T) if k == "logits" else v)
    return {k: np.concatenate(v) for k, v in parts.items()}


def errors(got, ref):
    """{quantity: error} of ``got`` against ``ref`` (dicts of ``in_slabs`` form; the stages ``got`` has are compared)."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    out = {"logits": _rel(t(got["logits"]), t(ref["logits"])), "logits_window": _rel_window(t(got["logits"]), t(ref["logits"])),
           "probs": float(np.abs(got["probs"] - ref["probs"]).max())}
    stage_keys = [k for k in got if k not in ("probs", "logits")]
    if stage_keys:
        out["stages"] = max(_rel(t(got[k]), t(ref[k][:len(got[k])])) for k in stage_keys)
    return out


# ------------------------------------------------------------------------------------------------ references, shared
_CASES = {}


def _case(wkey, w, geo, n, keep=("logits",), sample=None):
    """x (normal(0, 1.5), seeded by the count) and the float64 reference of one (weights, count), computed once; ``sample``: the
    windows the reference is computed for (None: all).  -> dict(x, idx, ref, yards): ``yards`` is filled by ``_yards``."""
    key = (wkey, n)
    if key not in _CASES:
        while len(_CASES) >= 3:
            _CASES.pop(next(iter(_CASES)))
        x = np.random.default_rng(n).normal(0, 1.5, size=(n, T)).astype(np.float32)
        idx = np.arange(n) if sample is None else sample
        kw = dict(n_layers=geo[2], n_layers_res=geo[3])
        ref = in_slabs(lambda xs: oracle.forward(xs, w, np.float64, return_stages=True, **kw), x[idx], keep)
        _CASES[key] = dict(x=x, idx=idx, ref=ref, w=w, kw=kw, keep=keep, yards={})
    return _CASES[key]


def _yards(case, x3=False):
    """The yardsticks of a case in a measuring run, else None: {name: {quantity: error}} for the float32 oracle, the float64
    network with the kernels' activations and (``x3``) the emulation of the scheme."""
    if not _measuring():
        return None
    x, w, kw, keep, ref, y = case["x"][case["idx"]], case["w"], case["kw"], case["keep"], case["ref"], case["yards"]
    if "oracle_fp32" not in y:
        y["oracle_fp32"] = errors(in_slabs(lambda xs: oracle.forward(xs, w, np.float32, return_stages=True, **kw), x, keep), ref)
        y["activation"] = errors(in_slabs(lambda xs: model_forward(xs, w, act="kernel", **kw), x, keep), ref)
    if x3 and "emulation" not in y:
        y["emulation"] = errors(in_slabs(lambda xs: model_forward(xs, w, x3=True, **kw), x, keep), ref)
    return {k: v for k, v in y.items() if x3 or k != "emulation"}


def _kernels(eng, case, stages=()):
    """One ``infer_host`` of the case's windows -> dict of ``in_slabs`` form at the reference's windows; ``stages``: (name,
    debug_stage index) pairs fetched for the first windows of the pass (as many as the reference has, all by default)."""
    n, idx = len(case["x"]), case["idx"]
    probs, logits = eng.infer_host(case["x"], return_logits=True)
    eng.check_error()
    assert np.isfinite(logits).all() and probs.shape == logits.shape == (n * T,)
    got = {"probs": probs.astype(np.float64).reshape(n, T)[idx], "logits": logits.astype(np.float64).reshape(n, T)[idx]}
    for name, stage in stages:
        m = n if len(idx) == n else 256
        assert np.array_equal(idx[:m], np.arange(m))
        got[name] = eng.debug_stage(stage, m).astype(np.float64)
    print("smallest window maximum of |logit|: %.3g" % np.abs(case["ref"]["logits"]).max(axis=1).min())
    return got


GEO_TUNED = (64, 32, 3, 2)


def _new_engine(w, geo, precision="fp32", cap=16384, fuse_layers=False):
    from catfish_amd.engine import HipEngine
    h, c, n_layers, n_blocks = geo
    return HipEngine(w, layer_size=h, n_layers=n_layers, layer_size_res=max(c, 16), n_layers_res=n_blocks, device=0,
                     max_windows_per_pass=cap, precision=precision, fuse_layers=fuse_layers)


def _weights(geo, seed):
    h, c, n_layers, n_blocks = geo
    return oracle.random_weights(seed=seed, layer_size=h, n_layers=n_layers, layer_size_res=max(c, 16), n_layers_res=n_blocks)


@pytest.fixture(scope="module")
def engine():
    """The tuned fp32 engine on random weights (seed 5: the weights of test_launch_regime_boundaries), one launch per layer."""
    eng = _new_engine(oracle.random_weights(seed=5), GEO_TUNED, cap=8192)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------ P. the tuned fp32 path
# window counts by label: H = hoist_max, K = coop_max of the engine under test -> (count, the kernels the count runs on)
P_WINDOWS = {
    "1": lambda H, K: 1, "17": lambda H, K: 17,
    "H": lambda H, K: H, "H+16": lambda H, K: H + 16,            # the last hoisted tile count, the first without the hoist
    "K": lambda H, K: K, "K+16": lambda H, K: K + 16,            # the last cooperative launch, the first throughput launch
    "K+3": lambda H, K: K + 3,                                   # throughput kernel, last tile with 3 valid windows
}
P_REGIME = {"1": "hoisted", "17": "hoisted", "H": "hoisted", "H+16": "cooperative", "K": "cooperative", "K+16": "throughput",
            "K+3": "throughput"}
P_STAGES = (("res1", 1), ("gru0", 2), ("gru1", 3))


def _regime(n, reg):
    return "hoisted" if n <= reg["hoist_max"] else ("cooperative" if n <= reg["coop_max"] else "throughput")


def _p_windows(label, reg):
    """The count of a label on this engine; the label means what it says (the switch points are where the module expects them)."""
    assert reg["hoist_max"] == 16 * (3 * reg["n_cu"] // 16) and reg["coop_max"] == 16 * reg["n_cu"] and reg["hoist_max"] + 16 < reg["coop_max"]
    n = P_WINDOWS[label](reg["hoist_max"], reg["coop_max"])
    assert _regime(n, reg) == P_REGIME[label], (label, n, reg)
    return n


def _slots(eng, fn):
    """``fn()`` with the per-kernel profile on -> (its result, the names of the launch slots that ran)."""
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        out = fn()
        return out, set(eng.profile_read())
    finally:
        eng.profile_enable(False)


@pytest.mark.parametrize("label", list(P_WINDOWS))
def test_tuned_fp32_path_matches_float64(engine, label):
    """Logits (whole call and per window), res1 / gru0 / gru1 on every window and probabilities, random weights."""
    reg = engine.launch_regimes()
    assert reg["fuse_auto_min"] == 0
    n = _p_windows(label, reg)
    case = _case("P-random5", oracle.random_weights(seed=5), GEO_TUNED, n, keep=("logits", "res1", "gru0", "gru1"))
    got, slots = _slots(engine, lambda: _kernels(engine, case, P_STAGES))
    assert "gru_fused" not in slots and {"gru_layer_first", "gru_layer_mid", "gru_layer_last"} <= slots, slots
    _check("P", "random weights, %d windows (%s, %s)" % (n, label, P_REGIME[label]), errors(got, case["ref"]), _yards(case))


@pytest.mark.parametrize("label", ["H+16", "K+3"])
def test_tuned_fp32_path_matches_float64_on_the_checkpoint(ckpt_weights, label):
    """The bundled checkpoint, whose logits saturate (tens in magnitude), at a cooperative and a ragged throughput count."""
    eng = _new_engine(ckpt_weights, GEO_TUNED, cap=8192)
    try:
        n = _p_windows(label, eng.launch_regimes())
        case = _case("P-checkpoint", ckpt_weights, GEO_TUNED, n, keep=("logits", "res1", "gru0", "gru1"))
        got = _kernels(eng, case, P_STAGES)
    finally:
        eng.close()
    print("largest |logit|: %.3g" % np.abs(case["ref"]["logits"]).max())
    _check("P", "checkpoint, %d windows (%s, %s)" % (n, label, P_REGIME[label]), errors(got, case["ref"]), _yards(case))


@pytest.mark.parametrize("side", ["below", "above"])
def test_fused_launch_matches_float64(side):
    """``fuse_layers=True``: all three biGRU layers in one launch, at ``fuse_auto_min - 1`` windows (whole tiles) and at
    ``fuse_auto_min + 10`` (ragged), the threshold read from an engine in auto mode.  The float64 reference covers the first and
    the last 256 windows and 512 random ones; the stages the first 256 windows."""
    w = oracle.random_weights(seed=5)
    auto = _new_engine(w, GEO_TUNED, cap=256, fuse_layers=None)
    try:
        fmin = auto.launch_regimes()["fuse_auto_min"]
    finally:
        auto.close()
    assert fmin > 16 * 256
    n = fmin - 1 if side == "below" else fmin + 10
    rng = np.random.default_rng(n + 1)
    sample = np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), rng.integers(256, n - 256, size=512)]))
    eng = _new_engine(w, GEO_TUNED, cap=(n + 15) // 16 * 16, fuse_layers=True)
    try:
        assert eng.launch_regimes()["fuse_auto_min"] == 1
        case = _case("P-random5-fused", w, GEO_TUNED, n, keep=("logits", "res1", "gru0", "gru1"), sample=sample)
        got, slots = _slots(eng, lambda: _kernels(eng, case, P_STAGES))
        assert "gru_fused" in slots and not slots & {"gru_layer_first", "gru_layer_mid", "gru_layer_last"}, slots
    finally:
        eng.close()
    _check("P", "random weights, fused launch, %d windows (%s fuse_auto_min), %d compared" % (n, side, len(sample)),
           errors(got, case["ref"]), _yards(case))


# ------------------------------------------------------------------------------------------------ Q. the any-size fp32 path
# tiles by label on C CUs, and the waves per workgroup ceil(2 tiles / C) the label stands for (before the size's own maximum)
TILES = {"1": lambda c: 1, "17": lambda c: 2, "43": lambda c: 3, "W2": lambda c: c // 2 + 1, "W3": lambda c: c + 1,
         "W4": lambda c: 3 * c // 2 + 1, "T2": lambda c: 2 * c + 1, "W8": lambda c: 7 * c // 2 + 1}
WAVES = {"1": 1, "17": 1, "43": 1, "W2": 2, "W3": 3, "W4": 4, "T2": 5, "W8": 8}
# layer size -> (state arrays, most waves per workgroup): csrc/anysize_infer_launch.hpp
CLASSES = {16: (3, 8), 48: (3, 8), 64: (3, 8), 96: (3, 8), 112: (2, 8), 128: (2, 8), 160: (2, 8), 176: (2, 4), 256: (2, 4)}
Q_SIZES = (16, 48, 96, 112, 160, 176, 256)
Q_LABELS = ("1", "17", "W2", "W3", "W4", "W8")


def _windows(label, n_cu):
    return {"1": 1, "17": 17}.get(label) or 16 * TILES[label](n_cu) - 5


def _assert_shape(eng, h, label, kernel="one_tile"):
    """Every biGRU layer of the engine runs what the label says at the label's count: kernel, waves (the label's, clamped by the
    size's class), LDS = waves x arrays x h / 16 KB, ``h_via_y``, and with more than one wave a partly empty last workgroup."""
    n_cu = eng.launch_regimes()["n_cu"]
    tiles, n = TILES[label](n_cu), _windows(label, n_cu)
    assert (n + 15) // 16 == tiles
    arrays, most = CLASSES[h]
    shapes = eng.anysize_infer_shape(n)
    print("shape h %d, %s: %d windows, %d tiles, %s" % (h, label, n, tiles, shapes))
    for s in shapes:
        assert s["kernel"] == kernel, (h, label, s)
        if kernel == "two_tile":
            assert s["waves"] == {64: 8, 128: 4}[h] and s["lds_bytes"] == s["waves"] * 4 * (h // 16) * 1024 == 131072 and s["h_via_y"] == 0
            assert s["grid_x"] * s["waves"] >= (tiles + 1) // 2 > (s["grid_x"] - 1) * s["waves"]
            continue
        assert s["waves"] == min(WAVES[label], most) and s["h_via_y"] == int(arrays == 2), (h, label, s)
        assert s["lds_bytes"] == s["waves"] * arrays * (h // 16) * 1024 <= LDS_LIMIT, (h, label, s)
        assert s["grid_x"] * s["waves"] >= tiles > (s["grid_x"] - 1) * s["waves"]
        assert s["waves"] == 1 or s["grid_x"] * s["waves"] > tiles, (h, label, s)           # waves past the last tile return early
    return n, shapes


_ENGINE = {}


def _engine_for(geo, seed, precision="fp32"):
    """The engine of (geometry, seed, precision), kept until another one is asked for."""
    key = (geo, seed, precision)
    if _ENGINE.get("key") != key:
        _close_engine()
        _ENGINE.update(key=key, eng=_new_engine(_weights(geo, seed), geo, precision))
    return _ENGINE["eng"]


def _close_engine():
    if _ENGINE.get("eng") is not None:
        _ENGINE["eng"].close()
    _ENGINE.clear()


@pytest.fixture(scope="module", autouse=True)
def _engines_closed():
    yield
    _close_engine()
    _CASES.clear()


def _anysize_case(section, geo, label, kernel="one_tile", x3=False):
    seed = 1000 + geo[0] + geo[1]
    eng = _engine_for(geo, seed, "bf16x3" if x3 else "fp32")
    n, shapes = _assert_shape(eng, geo[0], label, kernel)
    assert len(shapes) == geo[2]
    w = _weights(geo, seed)
    case = _case("%s-%s" % (section, geo), w, geo, n)
    got = _kernels(eng, case)
    if x3:
        f32 = _new_engine(w, geo, "fp32")
        try:
            plain = f32.infer_host(case["x"], return_logits=True)[1]
        finally:
            f32.close()
        assert not np.array_equal(plain.astype(np.float64).reshape(n, T)[case["idx"]], got["logits"])      # the split products ran
    s = shapes[0]
    _check(section, "%s, %d windows (%s): %s, %d waves, %d B%s" % (geo, n, label, s["kernel"], s["waves"], s["lds_bytes"],
                                                                   ", h_via_y" if s["h_via_y"] else ""),
           errors(got, case["ref"]), _yards(case, x3))
    return s


@pytest.mark.parametrize("label", Q_LABELS)
@pytest.mark.parametrize("h", Q_SIZES)
def test_anysize_fp32_layer_matches_float64(h, label):
    """One biGRU layer of ``h`` units behind one residual block of 16 channels, per LDS class and wave count."""
    s = _anysize_case("Q", (h, 16, 1, 1), label)
    if (h, label) == (160, "W8"):
        assert s["waves"] == 8 and s["lds_bytes"] == LDS_LIMIT          # the launch that takes the whole LDS


@pytest.mark.parametrize("h", [64, 128])
def test_anysize_two_tile_kernel_matches_float64(h):
    """gen_gru2_kernel at the two sizes gen_build gives it to, behind 64 channels (it needs an input that is a multiple of 64
    features), at 2 n_cu + 1 tiles with a ragged last tile and an odd tile without a partner."""
    _anysize_case("Q", (h, 64, 1, 1), "T2", kernel="two_tile")


@pytest.mark.parametrize("geo,label", [((48, 80, 3, 2), "43"), ((48, 80, 3, 2), "W2"), ((112, 0, 2, 0), "43"), ((112, 0, 2, 0), "W2")])
def test_anysize_fp32_deeper_models_match_float64(geo, label):
    """(48, 80, 3, 2): the second block takes gen_conv_kernel's shortcut path, the upper layers 96 inputs; the plain RNN type."""
    _anysize_case("Q", geo, label)


# ------------------------------------------------------------------------------------------------ R. bf16x3
@pytest.mark.parametrize("pipelined", [True, False])
@pytest.mark.parametrize("label", ["33", "257", "K+3"])
def test_tuned_bf16x3_matches_float64(engine, monkeypatch, label, pipelined):
    """gru_bf16x3_pipe_kernel and, behind CATFISH_BF16_PIPE=0, gru_layer_bf16_kernel<., ., 2>, with the bf16x3 residual stack."""
    reg = engine.launch_regimes()
    n = _p_windows("K+3", reg) if label == "K+3" else int(label)
    w = oracle.random_weights(seed=5)
    case = _case("P-random5", w, GEO_TUNED, n, keep=("logits", "res1", "gru0", "gru1"))
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    monkeypatch.delenv("CATFISH_BF16_PIPE", raising=False)
    eng = _new_engine(w, GEO_TUNED, "bf16x3", cap=8192)
    try:
        assert eng.launch_regimes()["coop_max"] == 0                 # no cooperative regime in this precision
        piped = _kernels(eng, case)
        monkeypatch.setenv("CATFISH_BF16_PIPE", "0")
        plain = _kernels(eng, case)
    finally:
        eng.close()
    # the knob switched kernels: the two differ in single lo parts of r.h (tests/test_gpu_parity.py), in a few windows already
    print("pipelined and unpipelined logits differ in %d of %d" % (int((piped["logits"] != plain["logits"]).sum()), n * T))
    assert n < 257 or not np.array_equal(piped["logits"], plain["logits"])
    got = piped if pipelined else plain
    fp32 = engine.infer_host(case["x"], return_logits=True)[1].astype(np.float64).reshape(n, T)
    assert not np.array_equal(fp32, got["logits"])                   # the split products ran
    _check("R", "tuned %s, %d windows (%s)" % ("pipelined" if pipelined else "unpipelined", n, label), errors(got, case["ref"]),
           _yards(case, x3=True))


def test_tuned_bf16x3_matches_float64_on_the_checkpoint(ckpt_weights):
    eng, f32 = _new_engine(ckpt_weights, GEO_TUNED, "bf16x3", cap=8192), _new_engine(ckpt_weights, GEO_TUNED, cap=8192)
    try:
        case = _case("R-checkpoint", ckpt_weights, GEO_TUNED, 257)
        got = _kernels(eng, case)
        assert not np.array_equal(f32.infer_host(case["x"], return_logits=True)[1].astype(np.float64).reshape(257, T), got["logits"])
    finally:
        eng.close(); f32.close()
    _check("R", "tuned pipelined, checkpoint, 257 windows", errors(got, case["ref"]), _yards(case, x3=True))


@pytest.mark.parametrize("label", ["1", "43", "W2"])
@pytest.mark.parametrize("h", [16, 48, 112, 176, 256])
def test_anysize_bf16x3_layer_matches_float64(h, label):
    """gen_gru_kernel<false, true> behind gen_conv_kernel<true>: one layer of ``h`` units behind one block of 16 channels."""
    _anysize_case("R", (h, 16, 1, 1), label, x3=True)


def test_shape_query_refuses_what_it_cannot_answer(engine):
    """cf_anysize_infer_shape: not on the tuned 64 / 32 path, not outside one pass of the model, not into too little room."""
    import ctypes as C
    from catfish_amd import _native as N
    with pytest.raises(ValueError, match="any-size"):
        engine.anysize_infer_shape(16)
    geo = (48, 80, 3, 2)
    eng = _engine_for(geo, 1000 + geo[0] + geo[1])
    for n in (0, -1, 16384 + 1):
        with pytest.raises(ValueError, match="n_windows"):
            eng.anysize_infer_shape(n)
    out = (C.c_int64 * 15)()
    with pytest.raises(ValueError, match="one row"):
        N.check(eng._lib.cf_anysize_infer_shape(eng._handle, 16, out, 2))
    with pytest.raises(ValueError, match="null"):
        N.check(eng._lib.cf_anysize_infer_shape(eng._handle, 16, None, 3))
    assert [s["kernel"] for s in eng.anysize_infer_shape(16384)] == ["one_tile"] * 3
