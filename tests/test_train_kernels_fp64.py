"""The training kernels against float64 in every launch regime (GPU).

What is compared, and with what:

  B  one biGRU layer through ``native_bigru`` (cf_gru_train_forward / _backward) at every switch point of the launcher,
     read from ``engine.launch_regimes()``: hoisted / not hoisted, one / two cooperative rounds, ``coop_max`` itself, and the
     throughput kernels ``gru_train_fwd_kernel`` / ``gru_train_bwd_kernel`` at 4 waves, at 8 waves, and on the second trip
     of their grid-stride loop, each with a zero-padded last tile (``native_bigru`` pads to whole tiles).  y, dx and the
     eight weight gradients per tensor, y and dx also per window (each window's error over that window's own maximum).
  C  the whole native step with dropout (in-kernel masks, and the same masks as the DSC operand) above ``coop_max`` and in the
     cooperative regime without the hoist, against ``TorchResNetRNN(dtype=float64)`` under those masks: here the kernels
     themselves see a partial last tile (the dropout hash over padding lanes, the head's window count).  The conv stack
     alone at an odd window count above its two-windows-per-workgroup threshold.
  D  ``cf_gru_train_wgrad`` directly against float64 ``A^T dA``.
  E  ``cf_opt_step`` directly against the float64 formulas of csrc/train_step.hpp.

The reference of B is ``bigru_layer`` below, a float64 restatement of one layer that tests/test_training.py ties to
``TorchResNetRNN(dtype=float64)`` (to 1e-12) and so to tests/golden/graph_train_golden.npz.

Bounds of B, C and D.  Every case computes two errors against float64, ``max|d| / max|ref|`` per tensor: the kernels' and the
float32 eager torch restatement's of the same computation (an independent fp32 implementation with another summation
order: the yardstick; ``bigru_layer`` in float32 for B, the same products in float32 for D, the float32 ``TorchResNetRNN``
for C, there only in the measuring run: see ``_measuring``).  The asserted bound of a quantity is 4 x the largest yardstick error seen for it over all cases of its section, and
never looser than what the older tests allow for the quantity (``OLDER_BOUNDS``).  The measured pairs are in
profiles/train_kernels_fp64_parity.jsonl (appended by this module, with commit and device, when CATFISH_PARITY_LOG names a
file); ``BOUNDS`` holds the constants and tests/test_training.py checks them against that file: B y 5.75e-6 (per window
6.00e-6), dx 2.12e-6 (per window 2.94e-6), weight gradients 6.16e-5; C loss 2.65e-7, the step's gradients 8.25e-4, conv stack
output 9.98e-7 and gradients 3.19e-6; D weight gradients 3.34e-5.

Two of C's margins are thin, as the rule makes them.  The step's gradients pass at 7.7e-4 against 8.25e-4, on one tensor,
``conv1d_6/kernel`` at 4117 windows; the loss bound is about four float32 ulps.  The runs are deterministic, but a harmless
reordering of the conv stack's partial sums can trip either: re-measure then, do not widen by hand.

Bounds of E are derived, not measured: see ``test_opt_step_matches_float64``.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle

pytestmark = pytest.mark.gpu

T = 35
GRU_PRE = "stack_bidirectional_rnn/cell_%d/bidirectional_rnn/%s/gru_cell"
GRU_KEYS = ("/gates/kernel", "/gates/bias", "/candidate/kernel", "/candidate/bias")

# quantity -> asserted bound = min(4 x largest float32-torch error, older tests' bound).  The largest float32-torch errors in
# profiles/train_kernels_fp64_parity.jsonl (MI355X, 256 CUs), and the largest errors of the kernels next to them:
#   B.y 1.438e-06 (kernels 1.32e-06)   B.y_window 1.501e-06 (1.40e-06)   B.dx 5.307e-07 (9.67e-07)   B.dx_window 7.362e-07 (1.46e-06)
#   B.wgrad 1.542e-05 (1.00e-05)   C.loss 6.631e-08 (6.63e-08)   C.grads 2.064e-04 (7.74e-04)   C.res_out 2.496e-07 (2.07e-07)
#   C.res_grads 7.980e-07 (2.65e-07)   D.wgrad 8.371e-06 (1.10e-06)
# 4 x each of them, rounded down, is below the older bound of its quantity (2e-3; loss 5e-6 absolute; conv stack 1e-5 and 2e-5), so
# it is the bound.  C.grads is the tightest: conv1d_6/kernel, a sum over 144 095 positions, 3.75 x the yardstick's error.
BOUNDS = {
    "B.y": 5.75e-6, "B.y_window": 6.00e-6, "B.dx": 2.12e-6, "B.dx_window": 2.94e-6, "B.wgrad": 6.16e-5,
    "C.loss": 2.65e-7, "C.grads": 8.25e-4,
    "C.res_out": 9.98e-7, "C.res_grads": 3.19e-6,
    "D.wgrad": 3.34e-5,
}


OLDER_BOUNDS = {"B.y": 2e-3, "B.y_window": 2e-3, "B.dx": 2e-3, "B.dx_window": 2e-3, "B.wgrad": 2e-3, "C.loss": 5e-6, "C.grads": 2e-3,
                "C.res_out": 1e-5, "C.res_grads": 2e-5, "D.wgrad": 2e-3}      # what tests/test_gpu_pipeline.py allows for the quantity
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "train_kernels_fp64_parity.jsonl")


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


def _measuring():
    """True when CATFISH_PARITY_LOG names a file: the run that writes profiles/train_kernels_fp64_parity.jsonl.  Section C
    computes its yardstick, the stock float32 ``TorchResNetRNN``, only then: the convolution library builds its kernels for a
    batch size on first use, which took 10 s of the 4117-window case in the first process that met the size on a machine and
    0.3 s in the next.  An ordinary run prints C's kernel errors with ``torch_fp32: null``; sections B and D always compute
    theirs.  The asserted bounds are constants either way."""
    return bool(os.environ.get("CATFISH_PARITY_LOG"))


_STAMP = {}


def _stamp():
    """commit and device of a measuring run: CATFISH_PARITY_COMMIT or ``git rev-parse`` (None in a tree without history)."""
    if not _STAMP:
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
        _STAMP.update(commit=commit, device="%s, %d CUs" % (prop.name, prop.multi_processor_count))
    return _STAMP


def _record(section, case, quantity, kernel, yardstick):
    """Print the pair (always, before any assertion) and append it to the file CATFISH_PARITY_LOG names."""
    row = {"section": section, "case": case, "quantity": quantity, "kernel": float(kernel),
           "torch_fp32": None if yardstick is None else float(yardstick)}
    print("parity %s" % json.dumps(row))
    path = os.environ.get("CATFISH_PARITY_LOG")
    if path and yardstick is not None:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(_stamp(), **row)) + "\n")


def _check(section, case, pairs):
    """pairs: {quantity: (kernel error, yardstick error)}.  All are recorded, then all are asserted."""
    for q, (k, y) in pairs.items():
        _record(section, case, q, k, y)
    bad = {q: (k, BOUNDS["%s.%s" % (section, q)]) for q, (k, _) in pairs.items() if not k <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------ A. the reference
def bigru_layer(x, params8):
    """One bidirectional GRU layer in plain torch, in the dtype of its arguments: x [N,35,Cin], params8 = (gates kernel
    [Cin+H,2H], gates bias, candidate kernel [Cin+H,H], candidate bias) of the forward, then of the backward direction
    -> y [N,35,2H], forward direction first.  Zero initial state; gates in tf.contrib.rnn.GRUCell's order (r | u), reset
    gate applied to the state before the candidate's matrix product, h' = u h + (1 - u) c."""
    import torch
    n, t_len, cin = x.shape
    outs = []
    for d, steps in ((0, range(t_len)), (1, range(t_len - 1, -1, -1))):
        wg, bg, wc, bc = params8[4 * d:4 * d + 4]
        hsz = wc.shape[1]
        xg = x.reshape(n * t_len, cin) @ wg[:cin] + bg           # the input's share of both pre-activations, all steps at once
        xc = x.reshape(n * t_len, cin) @ wc[:cin] + bc
        xg, xc = xg.reshape(n, t_len, 2 * hsz), xc.reshape(n, t_len, hsz)
        h = x.new_zeros(n, hsz)
        seq = [None] * t_len
        for s in steps:
            g = torch.sigmoid(xg[:, s] + h @ wg[cin:])
            r, u = g[:, :hsz], g[:, hsz:]
            c = torch.tanh(xc[:, s] + (r * h) @ wc[cin:])
            h = u * h + (1 - u) * c
            seq[s] = h
        outs.append(torch.stack(seq, 1))
    return torch.cat(outs, 2)


def stacked_loss(net, x, y, params=None):
    """``net``'s loss (a TorchResNetRNN) with its recurrent part replaced by ``bigru_layer`` per layer: conv stack and dense
    head are ``net``'s own.  ``params``: {TF name: tensor} that replaces ``net.params`` for the biGRU layers."""
    import torch
    p = net.params if params is None else params
    a = torch.as_tensor(x, dtype=net.dtype, device=net.device)[:, None, :]
    for d in range(net.n_layers_res):
        sc = net._conv_bn(a, 4 * d)
        o = torch.relu(net._conv_bn(a, 4 * d + 1))
        o = torch.relu(net._conv_bn(o, 4 * d + 2))
        o = torch.relu(net._conv_bn(o, 4 * d + 3))
        a = torch.relu(o + sc)
    a = a.permute(0, 2, 1)
    for layer in range(net.n_layers):
        a = bigru_layer(a, [p[(GRU_PRE % (layer, d)) + k] for d in ("fw", "bw") for k in GRU_KEYS])
    z = (a.reshape(-1, a.shape[2]) @ net.params["final_fully_connected/kernel"] + net.params["final_fully_connected/bias"])
    yt = torch.as_tensor(y, dtype=net.dtype, device=net.device).reshape(-1, 1)
    return torch.nn.functional.binary_cross_entropy_with_logits(z, yt, reduction="mean")


# ------------------------------------------------------------------------------------------------ helpers
def _rel(got, ref):
    """max|got - ref| / max|ref| of one tensor, in float64."""
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _rel_window(got, ref):
    """The largest per-window error: each window's max|d| over that window's own max|ref|."""
    ref = ref.double()
    err = (got.double() - ref).abs().flatten(1).amax(1)
    return float((err / ref.abs().flatten(1).amax(1)).max())


@pytest.fixture(scope="module")
def engine():
    from catfish_amd.engine import HipEngine
    eng = HipEngine(oracle.random_weights(seed=31), device=0, max_windows_per_pass=8192, fuse_layers=False)
    yield eng
    eng.close()


# window counts by label: H = hoist_max, K = coop_max of the engine under test (launch_regimes())
WINDOWS = {
    "1": lambda H, K: 1, "15": lambda H, K: 15, "16": lambda H, K: 16, "17": lambda H, K: 17,     # one tile: a single window, padded, full; two tiles
    "144": lambda H, K: 144, "384": lambda H, K: 384,          # dx_chunks() between its two clamps (9 and 24 tiles on 256 CUs)
    "H-3": lambda H, K: H - 3, "H": lambda H, K: H,            # the last hoisted tile count, padded and full
    "H+1": lambda H, K: H + 1, "H+16": lambda H, K: H + 16,    # the first one without the hoist, padded and full
    "K/2": lambda H, K: K // 2, "K/2+11": lambda H, K: K // 2 + 16 - 5,      # one cooperative round; two rounds, padded
    "K-7": lambda H, K: K - 7, "K": lambda H, K: K,            # the last cooperative launch
    "K+5": lambda H, K: K + 5,                                 # first throughput launch: 4 waves, last tile with 5 valid windows
    "2K": lambda H, K: 2 * K,                                  # 512 tiles on 256 CUs: the last 4-wave size
    "2K+19": lambda H, K: 2 * K + 16 + 3,                      # 8 waves
    "4K+39": lambda H, K: 4 * K + 48 - 9,                      # 8 waves, 3 tiles on the second trip of the grid-stride loop, padded
    "K+21": lambda H, K: K + 16 + 5, "H+19": lambda H, K: H + 16 + 3,       # section C
}


def _windows(label, reg):
    return WINDOWS[label](reg["hoist_max"], reg["coop_max"])


def test_regimes_of_the_engine_under_test(engine):
    """The labels of section B mean what they say only if the engine hoists up to the full 3 n_cu / 16 tiles and the
    cooperative kernels run up to one tile per CU; with 8 tiles per workgroup the largest count takes a second trip."""
    reg = engine.launch_regimes()
    assert reg["hoist_max"] == 16 * (3 * reg["n_cu"] // 16) and reg["coop_max"] == 16 * reg["n_cu"]
    assert reg["hoist_max"] + 16 < reg["coop_max"] // 2
    assert (_windows("4K+39", reg) + 15) // 16 == 8 * (reg["n_cu"] // 2) + 3


# ------------------------------------------------------------------------------------------------ B. one layer, every regime
B_COUNTS = [k for k in WINDOWS if k not in ("K+21", "H+19")]


@pytest.mark.parametrize("cin", [32, 128])
@pytest.mark.parametrize("label", B_COUNTS)
def test_bigru_layer_matches_float64(engine, label, cin):
    """y, dx and the eight weight gradients of one layer on the HIP kernels against ``bigru_layer`` in float64.  ``native_bigru``
    pads x and dy with zero windows to whole tiles, so the kernels see full tiles here; what a count that is no multiple of
    16 checks is that the padding windows of the last tile leave the valid ones and the weight gradients alone (per window)."""
    import torch
    from catfish_amd.native_train import native_bigru
    n = _windows(label, engine.launch_regimes())
    w = oracle.random_weights(seed=31)
    layer = 0 if cin == 32 else 1
    p_np = [w[(GRU_PRE % (layer, d)) + k] for d in ("fw", "bw") for k in GRU_KEYS]
    gen = torch.Generator(device="cuda").manual_seed(1000 * cin + n)
    x32 = (torch.randn(n, T, cin, generator=gen, device="cuda", dtype=torch.float32) * 1.2)
    g32 = torch.randn(n, T, 128, generator=gen, device="cuda", dtype=torch.float32)

    def run(fn, dtype):
        x = x32.to(dtype).requires_grad_(True)
        ps = [torch.tensor(p, dtype=dtype, device="cuda", requires_grad=True) for p in p_np]
        y = fn(x, ps)
        grads = torch.autograd.grad(y, [x] + ps, g32.to(dtype))
        return y.detach(), grads[0], grads[1:]

    y64, dx64, gw64 = run(bigru_layer, torch.float64)
    y_t, dx_t, gw_t = run(bigru_layer, torch.float32)
    y_k, dx_k, gw_k = run(lambda x, ps: native_bigru(x, ps, engine), torch.float32)
    assert y_k.shape == (n, T, 128) and dx_k.shape == (n, T, cin)
    _check("B", "%s windows (%s), cin %d" % (n, label, cin), {
        "y": (_rel(y_k, y64), _rel(y_t, y64)),
        "y_window": (_rel_window(y_k, y64), _rel_window(y_t, y64)),
        "dx": (_rel(dx_k, dx64), _rel(dx_t, dx64)),
        "dx_window": (_rel_window(dx_k, dx64), _rel_window(dx_t, dx64)),
        "wgrad": (max(_rel(a, b) for a, b in zip(gw_k, gw64)), max(_rel(a, b) for a, b in zip(gw_t, gw64))),
    })


# ------------------------------------------------------------------------------------------------ C. the whole step
def _grad_errors(grads, net64):
    """Largest per-tensor error of {name: ndarray or tensor} against the .grad of ``net64``'s trainable parameters, and the
    name of the tensor that has it."""
    import torch
    errs = {k: _rel(torch.as_tensor(grads[k], device=p.device), p.grad) for k, p in net64.trainable().items()}
    assert len(errs) == 58
    worst = max(errs, key=errs.get)
    return errs[worst], worst


@pytest.mark.parametrize("label", ["K+21", "H+19"])
def test_native_step_with_dropout_matches_float64(ckpt_weights, label):
    """Loss and all 58 gradients of the native step at keep_prob 0.8, masks drawn in the kernels and the same masks given as
    tensors, against the float64 graph under those masks: K' + 21 windows run the throughput kernels (in-kernel dropout, DY2,
    DSC, 4 waves, ragged) and the conv stack with two windows per workgroup and an odd count; H' + 19 windows the cooperative
    kernels without the hoist.  K' and H' are the Trainer's own engine's."""
    import torch
    from catfish_amd.training import Trainer, TorchResNetRNN
    tr = Trainer(ckpt_weights, 3, 2, "RMSProp", 1e-3, keep_prob=0.8, device="cuda", native=True, seed=11, use_graph=False)
    try:
        n = _windows(label, tr.engine.launch_regimes())
        rng = np.random.default_rng(n)
        x = rng.normal(0, 1.2, size=(n, T)).astype(np.float32)
        y = np.repeat((rng.random(n) < 0.4)[:, None], T, axis=1).astype(np.float32)
        masks = tr.step_impl.dropout_scales(n)
        assert abs(np.mean([m.mean() for m in masks.values()]) - 0.8) < 0.01
        loss_k, grads_k = tr.gradients(x, y)                       # masks drawn inside the kernels
        loss_m, grads_m = tr.gradients(x, y, masks=masks)          # the same masks as the DSC operand
        ref = TorchResNetRNN(ckpt_weights, 3, 2, device="cuda", dtype=torch.float64)
        loss64 = ref.loss(x, y, keep_prob=0.8, masks=masks)
        loss64.backward()
        l64 = float(loss64.detach())
        e_loss_t = e_grads_t = None
        if _measuring():
            yard = TorchResNetRNN(ckpt_weights, 3, 2, device="cuda")
            loss_t = yard.loss(x, y, keep_prob=0.8, masks=masks)
            loss_t.backward()
            e_loss_t = abs(float(loss_t.detach()) - l64) / abs(l64)
            e_grads_t, worst_t = _grad_errors({k: p.grad for k, p in yard.trainable().items()}, ref)
            print("worst gradient of float32 torch: %s" % worst_t)
        for path, loss, grads in (("in-kernel masks", loss_k, grads_k), ("mask tensors", loss_m, grads_m)):
            e_grads_k, worst_k = _grad_errors(grads, ref)
            print("worst gradient of the kernels: %s" % worst_k)
            _check("C", "%d windows (%s), %s" % (n, label, path),
                   {"loss": (abs(loss - l64) / abs(l64), e_loss_t), "grads": (e_grads_k, e_grads_t)})
    finally:
        tr.engine.close()


def test_res_stack_two_windows_per_workgroup_odd_count_matches_float64(engine):
    """cf_res_train_forward / _backward at 1027 windows: above 1024 a workgroup takes two windows and the last one is left with
    one.  Output and every kernel / bias / gamma / beta gradient against the float64 blocks."""
    import torch
    from catfish_amd.training import TorchResNetRNN
    from catfish_amd.native_train import native_res_stack, res_unit_names
    n, n_blocks = 1027, 2
    w = oracle.random_weights(seed=31)
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, T, generator=gen, device="cuda") * 1.2
    g = torch.randn(n, T, 32, generator=gen, device="cuda")
    names = [k for unit in res_unit_names(n_blocks) for k in unit]

    def blocks(net):
        a = x.to(net.dtype)[:, None, :]
        for d in range(n_blocks):
            sc = net._conv_bn(a, 4 * d)
            o = torch.relu(net._conv_bn(a, 4 * d + 1))
            o = torch.relu(net._conv_bn(o, 4 * d + 2))
            o = torch.relu(net._conv_bn(o, 4 * d + 3))
            a = torch.relu(o + sc)
        return a.permute(0, 2, 1)

    def run(net, fn):
        out = fn(net)
        train = [net.params[k] for k in names if net.params[k].requires_grad]
        return out.detach(), torch.autograd.grad(out, train, g.to(net.dtype))

    o64, g64 = run(TorchResNetRNN(w, 3, n_blocks, device="cuda", dtype=torch.float64), blocks)
    e_out_t = e_grads_t = None
    if _measuring():
        o_t, g_t = run(TorchResNetRNN(w, 3, n_blocks, device="cuda"), blocks)
        e_out_t, e_grads_t = _rel(o_t, o64), max(_rel(a, b) for a, b in zip(g_t, g64))
    o_k, g_k = run(TorchResNetRNN(w, 3, n_blocks, device="cuda"),
                   lambda net: native_res_stack(x, [net.params[k] for k in names], engine))
    _check("C", "conv stack, %d windows" % n, {
        "res_out": (_rel(o_k, o64), e_out_t),
        "res_grads": (max(_rel(a, b) for a, b in zip(g_k, g64)), e_grads_t),
    })


# ------------------------------------------------------------------------------------------------ D. cf_gru_train_wgrad
def _wgrad_chunks(engine, cin, tiles):
    """Workgroups per direction of the weight-gradient launch at ``tiles`` tiles, from the size of its workspace (one
    partial of (cin + 65) x 192 floats per chunk and direction)."""
    return int(engine._lib.cf_gru_wgrad_workspace_floats(engine._handle, cin, 16 * tiles)) // (2 * (cin + 65) * 192)


def _wgrad_tiles(engine, cin):
    """Tile counts of section D, each with the path through the launch and through cf_reduce_parts it is there for, asserted on
    the engine under test.  A reducing thread of group g = 0..3 adds parts g, g + 4, ...: four per trip of its first loop
    while part c + 12 exists, the rest one by one in its second.

    The launcher gives a workgroup max(8, ceil(2 pairs / n_cu)) pairs and a tile has 35, so on 256 CUs the chunk counts go
    5, 9, 14, 18, 22, ...: the 1, 13, 16 and 17 chunks the test was first asked for cannot be reached through the entry
    point.  5 and 9 run the second loop only, 14 the first loop in two groups and the second in the other two, 18 both
    loops one after the other in one thread, which is what those counts stand for."""
    chunks = lambda t: _wgrad_chunks(engine, cin, t)      # noqa: E731
    eight = lambda t: chunks(t) == (T * t + 7) // 8       # noqa: E731    (8 pairs per chunk, the last one partial)
    assert eight(1) and chunks(1) <= 12 and T % 8                           # second loop only, one or two parts per thread
    assert eight(2) and chunks(2) <= 12 and chunks(2) > 8                   # second loop only, three parts in group 0
    assert eight(3) and 12 < chunks(3) < 16                                 # first loop in groups 0 .. chunks - 13, second in the others
    assert eight(4) and 16 < chunks(4) <= 28                                # first loop, then second loop, in the same thread
    big = (2 * engine.launch_regimes()["coop_max"] + 19 + 15) // 16
    assert chunks(big) < (T * big + 7) // 8 and chunks(big) > 44 and (T * big) % ((T * big + chunks(big) - 1) // chunks(big))
    return [1, 2, 3, 4, big]                                                # big: more than 8 pairs per chunk, partial last chunk, several trips


@pytest.mark.parametrize("cin", [32, 128])
def test_wgrad_kernel_matches_float64(engine, cin):
    """cf_gru_train_wgrad on random fragments against float64 A^T dA, A = [x | h_prev] for the gates and [x | r h_prev] for the
    candidate, h_prev = y shifted by one step in the direction's order and zero at its first step (as NativeBiGRU.backward
    builds it).  The last tile is partly padding: its padding windows hold zero in da (the kernel's contract) and random values
    everywhere else."""
    import torch
    from catfish_amd import _native as N
    from catfish_amd.native_train import frag_to_nat
    rows = cin + 64
    for tiles in _wgrad_tiles(engine, cin):
        n = 16 * tiles - 5
        gen = torch.Generator(device="cuda").manual_seed(100 * tiles + cin)
        rnd = lambda *shape: torch.randn(*shape, generator=gen, device="cuda", dtype=torch.float32)      # noqa: E731
        x_frag, y_frag = rnd(tiles, T, cin // 16, 64, 4), torch.tanh(rnd(tiles, T, 8, 64, 4))
        stash = torch.sigmoid(rnd(tiles, T, 2, 12, 64, 4))
        da = rnd(tiles, T, 2, 12, 64, 4)
        da.view(tiles, T, 2, 12, 4, 16, 4)[tiles - 1, :, :, :, :, 11:, :] = 0.0       # lane = 16 q + window
        ws_floats = int(engine._lib.cf_gru_wgrad_workspace_floats(engine._handle, cin, n))
        ws = torch.full((ws_floats,), float("nan"), device="cuda")
        out = torch.full((2, rows * 192 + 192), float("nan"), device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        N.check(engine._lib.cf_gru_train_wgrad(engine._handle, cin, p(x_frag), p(y_frag), p(stash), p(da), n, p(ws), ws_floats, p(out),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))

        def reference(dtype):
            x2 = frag_to_nat(x_frag).to(dtype).reshape(-1, cin)
            y = frag_to_nat(y_frag).to(dtype)
            res = []
            for d in range(2):
                da_d = frag_to_nat(da[:, :, d]).to(dtype)
                assert float(da_d[n:].abs().max()) == 0.0 and float(da_d[n - 1].abs().max()) > 0.0
                r = frag_to_nat(stash[:, :, d, 0:4]).to(dtype)
                h = y[:, :, 64 * d:64 * d + 64]
                hprev = torch.zeros_like(h)
                if d == 0:
                    hprev[:, 1:] = h[:, :-1]
                else:
                    hprev[:, :-1] = h[:, 1:]
                da_g, da_c = da_d[:, :, :128].reshape(-1, 128), da_d[:, :, 128:].reshape(-1, 64)
                a_g = torch.cat([x2, hprev.reshape(-1, 64)], 1)
                a_c = torch.cat([x2, (r * hprev).reshape(-1, 64)], 1)
                res.append([a_g.t() @ da_g, da_g.sum(0), a_c.t() @ da_c, da_c.sum(0)])
            return res

        ref64, ref32 = reference(torch.float64), reference(torch.float32)
        e_k = e_t = 0.0
        for d in range(2):
            o = out[d]
            got = [o[:rows * 128].view(rows, 128), o[rows * 128:rows * 128 + 128],
                   o[rows * 128 + 128:rows * 128 + 128 + rows * 64].view(rows, 64), o[rows * 128 + 128 + rows * 64:]]
            for a, b, c in zip(got, ref32[d], ref64[d]):
                e_k, e_t = max(e_k, _rel(a, c)), max(e_t, _rel(b, c))
        chunks = _wgrad_chunks(engine, cin, tiles)
        _check("D", "%d tiles = %d chunks, cin %d" % (tiles, chunks, cin), {"wgrad": (e_k, e_t)})


# ------------------------------------------------------------------------------------------------ E. cf_opt_step
U = 2.0 ** -23        # float32 machine epsilon: one rounding is at most U / 2 relative


def _opt_inputs(n, kind, seed):
    """p, g, slot1, slot2 (float32).  g: normal values, exact zeros, +-1e-20 and +-1e4; p of both signs; the slots hold their
    initial values (rms 1, everything else 0) in a part and accumulated values elsewhere; the rms slot is also 0 and 1e-30 under
    normal gradients, where the place of the epsilon decides the update.  Adam's first moment has the
    sign of g wherever both are non-zero: with opposite signs 0.9 m + 0.1 g cancels and no bound relative to the result holds
    for any fp32 evaluation."""
    rng = np.random.default_rng(seed)
    p = (rng.normal(0, 0.3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g = rng.normal(0, 1e-2, n)
    sel = rng.integers(0, 6, n)
    g[sel == 0] = 0.0
    g[sel == 1] = 1e-20 * rng.choice([-1.0, 1.0], n)[sel == 1]
    g[sel == 2] = 1e4 * rng.choice([-1.0, 1.0], n)[sel == 2]
    g = g.astype(np.float32)
    fresh = rng.random(n) < 0.3
    if kind == 0:
        s1 = np.where(fresh, 1.0, rng.uniform(1e-6, 2.0, n))                                 # rms
        s1[sel == 3] = rng.choice([0.0, 1e-30], n)[sel == 3]                                 # decayed away: the epsilon decides
        s1 = s1.astype(np.float32)
        s2 = np.where(fresh, 0.0, rng.normal(0, 1e-3, n)).astype(np.float32)                 # momentum: overwritten
    else:
        mag = np.abs(rng.normal(0, 1e-2, n))
        s1 = np.where(fresh, 0.0, mag * np.where(g != 0, np.sign(g), rng.choice([-1.0, 1.0], n))).astype(np.float32)
        s2 = np.where(fresh, 0.0, rng.uniform(1e-8, 1e-2, n)).astype(np.float32)
    return p, g, s1, s2


def opt_step_float64(kind, p, g, s1, s2, lr, t):
    """The update of csrc/train_step.hpp's header in float64: (p, slot1, slot2, update) after one step; ``t`` steps were taken
    before it.  RMSProp: decay 0.9, momentum 0, epsilon 1e-10 inside the root.  Adam: beta 0.9 / 0.999, epsilon 1e-8
    outside the root, lr_t = lr sqrt(1 - 0.999^(t+1)) / (1 - 0.9^(t+1))."""
    p, g, s1, s2 = (np.asarray(a, dtype=np.float64) for a in (p, g, s1, s2))
    if kind == 0:
        ms = 0.9 * s1 + 0.1 * g * g
        upd = lr * g / np.sqrt(ms + 1e-10)
        return p - upd, ms, upd, upd
    m = 0.9 * s1 + 0.1 * g
    v = 0.999 * s2 + 0.001 * g * g
    lr_t = lr * np.sqrt(1.0 - 0.999 ** (t + 1.0)) / (1.0 - 0.9 ** (t + 1.0))
    upd = lr_t * m / (np.sqrt(v) + 1e-8)
    return p - upd, m, v, upd


def opt_step_bounds_hold(kind, got_p, got_s1, got_s2, p, g, s1, s2, lr, t):
    """The derived bounds of ``test_opt_step_matches_float64`` for one result; returns the list of violated ones."""
    p64, a64, b64, upd64 = opt_step_float64(kind, p, g, s1, s2, lr, t)
    tiny = 2.0 ** -149                                              # spacing of the float32 subnormals (g = 1e-20: g^2 is one)
    bad = []
    if not np.all(np.abs(got_p - p64) <= 8 * U * np.abs(upd64) + np.spacing(np.abs(p64).astype(np.float32)).astype(np.float64) + tiny):
        bad.append("p")
    if not np.all(np.abs(got_s1 - a64) <= 4 * U * np.abs(a64) + tiny):
        bad.append("slot1")
    if not np.all(np.abs(got_s2 - b64) <= 4 * U * np.abs(b64) + tiny):
        bad.append("slot2")
    return bad


@pytest.mark.parametrize("kind,steps_before", [(0, 0), (1, 0), (1, 1), (1, 999), (1, 50000)])
def test_opt_step_matches_float64(engine, kind, steps_before):
    """cf_opt_step (opt_step_kernel + gather_scale_kernel) against the float64 formulas, for n in {1, 255, 256, 257, 70 003}.

    Derived bounds (u = 2^-24 per rounding, constants such as 0.9f count as one): a slot is a sum of two products of the same
    sign, each with at most two roundings, and one rounding of the fused sum: below 3 u, asserted 4 * 2^-23 relative.  The
    update passes at most eight roundings (slot 3 u, + epsilon, root, quotient, learning rate (and its float cast for Adam)),
    and the final subtraction adds one of the result: |p - p64| <= 8 * 2^-23 |upd64| + ulp(|p64|).  RMSProp's second slot is
    the update itself; the root halves the error of its argument, so it carries about 5.5 u and meets the slots' 4 * 2^-23 as
    well.  Every bound carries the spacing of the float32 subnormals, 2^-149, as an absolute term: the square of g = 1e-20
    is one, and no relative bound can hold for it.  sqrtf and the quotient are correctly rounded in this build (no fast-math
    flag), and the MI355X meets the bounds as they stand: nothing was widened.
    The step counter rises by exactly 1.0 per call; packed == p_new[idx] * scale bit for bit; a call with n_packed = 0 and null
    packing pointers succeeds, updates p and advances the counter."""
    import torch
    from catfish_amd import _native as N
    lib, handle = engine._lib, engine._handle
    lr = float(np.float32(1e-3))                         # the entry point takes a float
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())             # noqa: E731
    for n in (1, 255, 256, 257, 70003):
        p, g, s1, s2 = _opt_inputs(n, kind, seed=n + steps_before)
        rng = np.random.default_rng(n)
        n_packed = 3 * n + 5
        idx = rng.integers(0, n, n_packed).astype(np.int32)
        scale = rng.choice([1.0, -2.0, 0.72134752], n_packed).astype(np.float32)
        dp, dg, d1, d2 = (torch.from_numpy(a.copy()).cuda() for a in (p, g, s1, s2))
        didx, dscale = torch.from_numpy(idx).cuda(), torch.from_numpy(scale).cuda()
        packed = torch.full((n_packed,), float("nan"), device="cuda")
        t_dev = torch.full((), float(steps_before), dtype=torch.float64, device="cuda")
        N.check(lib.cf_opt_step(handle, kind, ptr(dp), ptr(dg), ptr(d1), ptr(d2), n, lr, ptr(t_dev), ptr(didx), ptr(dscale), ptr(packed),
                                n_packed, stream()))
        assert float(t_dev) == steps_before + 1.0
        got_p, got_1, got_2 = dp.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()
        assert np.array_equal(dg.cpu().numpy(), g)
        assert opt_step_bounds_hold(kind, got_p, got_1, got_2, p, g, s1, s2, lr, steps_before) == [], (kind, n)
        assert np.array_equal(packed.cpu().numpy().view(np.uint32), (got_p[idx] * scale).view(np.uint32))
        # second call, without re-tiling: null packing pointers, the next step on the state the first one left
        N.check(lib.cf_opt_step(handle, kind, ptr(dp), ptr(dg), ptr(d1), ptr(d2), n, lr, ptr(t_dev), None, None, None, 0, stream()))
        assert float(t_dev) == steps_before + 2.0
        assert opt_step_bounds_hold(kind, dp.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy(), got_p, g, got_1, got_2, lr,
                                    steps_before + 1) == [], (kind, n, "second call")
