"""The bounds of tests/test_infer_kernels_fp64.py, on the CPU: they follow from the module's profile, they admit the yardsticks they
were made from, and they reject a subtly wrong network that the 1e-4 gate on probabilities lets through.

The defects are those of the experiment that motivated the module, restated here: ``oracle.random_weights(seed=5)`` (the weights of
test_launch_regime_boundaries), 512 windows drawn from normal(0, 1.5), a defect planted in a float64 forward pass and compared with
the clean float64 pass.  With these weights all 17 920 probabilities lie in 0.51 .. 0.76 and the logits in 0.04 .. 1.16: no label
is near a flip and the sigmoid divides a logit error by at least 4, which is why every row passes the gate."""
import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from oracle.tolerances import GATE_MAX_ABS_DP
import test_infer_kernels_fp64 as m

KEEP = ("logits", "res1", "gru0", "gru1")


def test_bounds_of_the_inference_parity_module_follow_from_its_profile():
    """Each bound is at most 4 x the largest yardstick that profiles/infer_kernels_fp64_parity.jsonl records for the quantity, at
    most the older tests' bound, and not so far below (rounded down to three digits) that it is a different number."""
    want = m.bounds_from_profile()
    assert sorted(want) == sorted(m.BOUNDS) == sorted(m.OLDER_BOUNDS)
    for k, b in m.BOUNDS.items():
        assert 0.99 * want[k] <= b <= want[k], (k, b, want[k])
    assert set(m.ACTIVATION_TERM) <= set(m.BOUNDS)


@pytest.fixture(scope="module")
def setup():
    w = oracle.random_weights(seed=5)
    x = np.random.default_rng(1).normal(0, 1.5, size=(512, 35)).astype(np.float32)
    ref = m.in_slabs(lambda xs: oracle.forward(xs, w, np.float64, return_stages=True), x, KEEP)
    assert 0.5 < ref["probs"].min() and ref["probs"].max() < 0.77 and 0.03 < ref["logits"].min() and ref["logits"].max() < 1.2
    return w, x, ref


def _errors(setup, fn):
    _, x, ref = setup
    return m.errors(m.in_slabs(fn, x, KEEP), ref)


@pytest.mark.parametrize("geo", [(64, 32, 3, 2), (48, 80, 2, 2), (112, 0, 2, 0)])
def test_the_restated_network_is_the_oracle(geo):
    """``model_forward`` without options is ``oracle.forward`` in float64, stage by stage (it folds the batch norm as the packers
    do and takes the input's share of the recurrent products for all steps at once: other roundings, the same numbers)."""
    h, c, n_layers, n_blocks = geo
    w = oracle.random_weights(seed=3, layer_size=h, n_layers=n_layers, layer_size_res=max(c, 16), n_layers_res=n_blocks)
    x = np.random.default_rng(2).normal(0, 1.5, size=(40, 35)).astype(np.float32)
    kw = dict(n_layers=n_layers, n_layers_res=n_blocks)
    p0, s0 = oracle.forward(x, w, np.float64, return_stages=True, **kw)
    p1, s1 = m.model_forward(x, w, **kw)
    assert sorted(s0) == sorted(s1) and np.abs(p0 - p1).max() < 1e-14
    for k in s0:
        assert s0[k].shape == s1[k].shape and np.abs(s0[k] - s1[k]).max() < 1e-12 * max(1.0, np.abs(s0[k]).max()), k


def test_split_keeps_sixteen_bits_and_the_split_product_is_exact_on_them():
    hi, lo = m.split(np.array([1.00390625, -3.0, 0.0, 1.0 + 2.0 ** -9 + 2.0 ** -20]))
    assert hi.tolist() == [1.0, -3.0, 0.0, 1.0] and lo.tolist()[:3] == [0.00390625, 0.0, 0.0] and lo[3] == 2.0 ** -9
    assert m.split(np.array([1.00390625]), keep_lo=False)[1].tolist() == [0.0]
    rng = np.random.default_rng(0)
    a = m.bf16_round(rng.normal(size=(5, 32)).astype(np.float32)).astype(np.float64)      # operands bf16 holds exactly
    wm = m.bf16_round(rng.normal(size=(32, 7)).astype(np.float32)).astype(np.float64)
    x3 = m._Product(True)
    assert np.array_equal(x3(a, x3.weights(wm)), a @ wm)
    b, wb = rng.normal(size=(5, 32)), rng.normal(size=(32, 7))
    err = np.abs(x3(b, x3.weights(wb, m.GATE_SCALE)) - b @ wb).max()
    assert 1e-9 < err < 1e-4                                  # a_lo w_lo is dropped and hi + lo keeps 16 .. 17 bits of each operand


def test_the_yardsticks_pass_their_own_bounds(setup):
    """The float32 oracle meets the bounds of the fp32 sections, the emulation of the scheme those of R (the pattern of
    test_opt_step_bounds_admit_a_plain_float32_evaluation): a correct implementation of either kind is not refused."""
    w = setup[0]
    e32 = _errors(setup, lambda xs: oracle.forward(xs, w, np.float32, return_stages=True))
    emu = _errors(setup, lambda xs: m.model_forward(xs, w, x3=True))
    print("float32 oracle %s, emulation %s" % (e32, emu))
    for q, e in e32.items():
        assert e <= m.BOUNDS["P." + q], (q, e)
        assert q == "stages" or e <= m.BOUNDS["Q." + q], (q, e)
    for q in ("logits", "logits_window", "probs"):
        assert emu[q] <= m.BOUNDS["R." + q], (q, emu[q])
    assert emu["logits"] > 4 * e32["logits"]                  # the scheme's own error is what R's yardstick is made of


def _with(w, **changed):
    out = dict(w)
    out.update(changed)
    return out


def _block_hi_only(w):
    """One 16 x 16 block of one candidate kernel (layer 1, backward) without its lo part."""
    name = oracle.gru_prefix(1, "bw") + "/candidate/kernel"
    k = np.array(w[name], dtype=np.float64)
    k[16:32, 0:16] = m.bf16_round(k[16:32, 0:16].astype(np.float32))
    return _with(w, **{name: k})


def _bn_epsilon(fn):
    def run(xs):
        eps = oracle.BN_EPS
        oracle.BN_EPS = 1.1e-3
        try:
            return fn(xs)
        finally:
            oracle.BN_EPS = eps
    return run


# name -> (sections whose bounds must reject it, what computes it from (weights, windows))
DEFECTS = {
    "state hi-only, layer 0 forward": ("R", lambda w, xs: m.model_forward(xs, w, x3=True, defects=[("state_hi_only", 0, "fw")])),
    "state hi-only, every layer and direction": ("R", lambda w, xs: m.model_forward(xs, w, x3=True, defects=[("state_hi_only", None, None)])),
    "r.h rounded to bf16, layer 0 forward": ("R", lambda w, xs: m.model_forward(xs, w, x3=True, defects=[("rh_hi_only", 0, "fw")])),
    "one 16 x 16 weight block hi-only, bf16x3": ("R", lambda w, xs: m.model_forward(xs, _block_hi_only(w), x3=True)),
    "one 16 x 16 weight block hi-only, float64": ("PQ", lambda w, xs: oracle.forward(xs, _block_hi_only(w), np.float64, return_stages=True)),
    "BN epsilon 1.1e-3": ("PQ", lambda w, xs: _bn_epsilon(lambda v: oracle.forward(v, w, np.float64, return_stages=True))(xs)),
    "dense bias rounded to bf16": ("PQ", lambda w, xs: oracle.forward(
        xs, _with(w, **{"final_fully_connected/bias": m.bf16_round(w["final_fully_connected/bias"])}), np.float64, return_stages=True)),
    "sigmoid off by 1e-5": ("PQ", lambda w, xs: m.model_forward(xs, w, defects=[("sigmoid_off", None, None)])),
    "tanh off by 1e-5": ("PQ", lambda w, xs: m.model_forward(xs, w, defects=[("tanh_off", None, None)])),
}


UNDER_THE_WINDOW_BOUND = ("state hi-only, layer 0 forward", "state hi-only, every layer and direction", "one 16 x 16 weight block hi-only, bf16x3")


@pytest.mark.parametrize("name", list(DEFECTS))
def test_the_bounds_reject_what_the_gate_accepts(setup, name):
    """Every planted defect stays inside the 1e-4 gate on probabilities and is refused by the logits bound of its section: R for
    what is planted in the emulation of the bf16x3 scheme, P and Q for what is planted in the float64 network.  As measured every
    row clears that bound: in R by 1.26 x (the state without its lo part in one direction of one layer), 2.2 x (in all of them),
    4.7 x (r.h) and 2.2 x (the weight block); in P / Q by 3.9 / 2.0 x (sigmoid), 8 / 4.2 x (tanh), 17 / 8.8 x (BN epsilon), 41 /
    21 x (the weight block) and 113 / 59 x (dense bias).  The per-window bounds refuse every row as well except three in R, the two
    state rows and the weight block (6.8e-5, 1.30e-4 and 1.40e-4 against 1.44e-4, a bound that the checkpoint's saturating logits
    set): ``UNDER_THE_WINDOW_BOUND``.  Every ratio is printed."""
    w = setup[0]
    sections, fn = DEFECTS[name]
    e = _errors(setup, lambda xs: fn(w, xs))
    print("%s: %s" % (name, {q: "%.3g" % v for q, v in e.items()}))
    assert e["probs"] < GATE_MAX_ABS_DP, (name, e)
    for section in sections:
        bound = m.BOUNDS[section + ".logits"]
        print("  %s: logits %.2f x the bound, per window %.2f x%s" % (
            section, e["logits"] / bound, e["logits_window"] / m.BOUNDS[section + ".logits_window"],
            ", stages %.2f x" % (e["stages"] / m.BOUNDS["P.stages"]) if section == "P" else ""))
        assert e["logits"] > bound, (name, section, e["logits"], bound)
        if name not in UNDER_THE_WINDOW_BOUND:
            assert e["logits_window"] > m.BOUNDS[section + ".logits_window"], (name, section, e["logits_window"])
