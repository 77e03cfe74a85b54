"""Plain bf16 inference (``precision="bf16"``, BASELINE config 4) against an emulation of its rounding scheme, stage by stage (GPU).

The older gates on this path -- max|dp| < 3e-2 / 5e-2 (tests/test_gpu_parity.py), 1e-2 on reads (tests/test_gpu_pipeline.py), a label
match rate, bit-identity between the kernels' own variants -- are 6 to 60 x looser than the scheme's own error and cannot see a
kernel that departs from the scheme in a direction that is closer to float64 (tests/test_infer_bf16_parity_host.py plants six
such departures; every older gate accepts all six).  Here the kernels are compared with the scheme itself.

The emulation is ``model_forward(..., bf16=True)`` of tests/test_infer_kernels_fp64.py: every product the bf16x3 emulation splits is
``a_hi @ w_hi`` accumulated in float64, with w_hi = bf16(float(scale w)) (the -log2 e / 2 log2 e pre-scaling applied in double before
the rounding, as pack_gru_dir_bf16 does; conv weights batch-norm-folded in double, as pack_unit_bf16 gets them) and a_hi =
bf16(float(a)) where a enters a product (layer input, h, r.h, the conv intermediates o1, o2 and the block output); block 0's
one-channel convolutions and shortcut, block 1's shortcut sum, biases, the state between steps and the dense head (on the fp32 h)
stay exact.  It is a reference here, computed in ordinary runs too.  ``arith="float32"`` is a second implementation of the same
scheme in the kernels' arithmetic (float32 sums in numpy's order, folded weights and pre-scaled biases rounded to float, the
one-channel convolutions as one fma, exp2 / reciprocal activations, h = fma(u, h - c, c)): two correct implementations differ by
rounding flips near ties of the bf16 grid, and the second against the first measures how many.

Quantities, each recorded for every case, then asserted:
  against float64    logits, logits_window, probs as in tests/test_infer_kernels_fp64.py; yardstick: float32 oracle + emulation
  against emulation  emu_logits (max|d| / max|ref|), emu_logits_rms (rms(d) / rms(ref) over the case: the stable one, the maximum is
                     flip-tailed), emu_stage_rms (the worst of res1, gru0, gru1 as ``debug_stage`` reads them in this precision) and
                     emu_share.res1 / gru0 / gru1 (the share of stage elements that are not equal to the emulation's stage rounded
                     to bf16); yardstick: the second implementation against the first.  The shares are asserted where the stages
                     cover at least 256 windows (below that they count a handful of events) and recorded everywhere.

Cases (C = n_cu; every case asserts the launch slots that ran, the knob cases that the knob took effect):
  S  random weights, seed 5.  gru_bf16_pipe_kernel behind res_stack2_bf16_kernel<1, 1> at 1, 33 (a second tile with one valid
     window) and 257 windows (one-wave workgroups), 32 (C / 2 + 1) - 5 (two waves) and 32 (2 C + 1) - 5 (eight waves; these two with
     the references on the first and last 256 windows and 512 random ones, the stages on the first 256); 133 windows behind
     CATFISH_BF16_WGS=1 CATFISH_BF16_WAVES=2 (wave 0 walks tiles 0, 2, 4: the pipelined kernel's prologue for a wave's second and
     third tile, bit-equal to the natural launch); gru_layer_bf16_kernel<., ., 1> behind CATFISH_BF16_PIPE=0 at 33 and 257; and the
     bf16 logits against the fp32 engine's (not bit-equal: the mode ran).
  T  the bundled checkpoint, whose logits saturate, at 257 windows on both biGRU kernels.
  U  random weights with ``n_layers_res=3`` at 33 windows: the third block runs on res_block_bf16_kernel<false, 1>.  Another
     network than S's with yardsticks up to 2.7 x S's on the logits, hence its own section.

Bounds.  A measuring run (CATFISH_PARITY_LOG names a file) appends kernel and yardstick rows to profiles/infer_bf16_parity.jsonl;
``BOUNDS`` is 4 x the largest yardstick of the quantity over its section, rounded down to three digits, and never looser than the
tightest older bound on plain bf16 (``OLDER_BOUNDS``: CONFIG4_MAX_ABS_DP_TEST on probabilities, four times that on logits);
tests/test_infer_bf16_parity_host.py checks the constants against the profile.  4 x is the project's margin for two
implementations with different summation orders.

As measured (MI355X, 256 CUs) the kernels sit on the scheme: no kernel or packer departs from it, and no quantity needed a term
beyond its yardstick.  Largest kernel error, largest yardstick of the section, their ratio (shares: asserted cases):
  S  logits 3.10e-3 / 3.10e-3 (1.00)   logits_window 4.04e-3 / 4.04e-3 (1.00)   probs 7.70e-4 / 7.63e-4 (1.01)
     emu_logits 7.87e-4 / 7.54e-4 (1.04)   emu_logits_rms 1.14e-4 / 1.12e-4 (1.01)   emu_stage_rms 3.96e-4 / 3.66e-4 (1.08)
     emu_share res1 3.73e-4 / 1.24e-3 (0.30)   gru0 5.54e-3 / 5.16e-3 (1.07)   gru1 2.36e-2 / 2.13e-2 (1.10)
  T  logits 5.58e-3 / 5.39e-3 (1.04)   logits_window 2.73e-2 / 2.73e-2 (1.00)   probs 4.52e-3 / 4.36e-3 (1.04)
     emu_logits 1.30e-3 / 1.30e-3 (1.00)   emu_logits_rms 3.34e-4 / 3.36e-4 (1.00)   emu_stage_rms 4.35e-4 / 4.19e-4 (1.04)
     emu_share res1 9.73e-5 / 9.03e-5 (1.08)   gru0 4.89e-3 / 4.56e-3 (1.07)   gru1 2.32e-2 / 2.12e-2 (1.09)
  U  logits 4.59e-3 / 4.60e-3 (1.00)   logits_window 6.43e-3 / 6.44e-3 (1.00)   probs 5.85e-4 / 5.86e-4 (1.00)
     emu_logits 1.45e-3 / 1.45e-3 (1.00)   emu_logits_rms 2.57e-4 / 3.03e-4 (0.85)   emu_stage_rms 3.72e-4 / 4.45e-4 (0.84)
     (shares recorded only: res1 1.00, gru0 0.68, gru1 0.74 of the case's yardstick)
Case by case the kernels reach at most 1.15 x their case's yardstick on the continuous quantities (emu_stage_rms at 33 windows)
and 2.76 x on a share (res1 at 32 (C / 2 + 1) - 5 windows: 58 flipped elements of 286 720 against 21).  Two bounds fall back to the
older ones, T's logits_window (4 x 2.73e-2 > 4e-2) and T's probs (4 x 4.36e-3 > 1e-2), and they are the two thinnest margins: the
checkpoint at 257 windows at 0.68 (logits_window) and 0.45 (probs) of the bound; everything else sits at 0.08 to 0.28.  The runs
are deterministic; if a reordering of sums trips a bound, re-measure, do not widen by hand.  The longest case takes 1.8 s in the
measuring run (eight waves, 16 411 windows), 1.4 s in an ordinary one.
"""
import json
import os
import sys

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from oracle.tolerances import CONFIG4_MAX_ABS_DP_TEST
from test_train_kernels_fp64 import T, _measuring, _stamp
import test_infer_kernels_fp64 as m

pytestmark = pytest.mark.gpu

STAGES = ("res1", "gru0", "gru1")
FP64_QUANTITIES = ("logits", "logits_window", "probs")
EMU_QUANTITIES = ("emu_logits", "emu_logits_rms", "emu_stage_rms") + tuple("emu_share." + s for s in STAGES)
SHARE_MIN_WINDOWS = 256      # below this many stage windows a share counts a handful of discrete events: recorded, not asserted

BOUNDS = {
    "S.logits": 1.23e-2, "S.logits_window": 1.61e-2, "S.probs": 3.05e-3,
    "S.emu_logits": 3.01e-3, "S.emu_logits_rms": 4.48e-4, "S.emu_stage_rms": 1.46e-3,
    "S.emu_share.res1": 4.97e-3, "S.emu_share.gru0": 2.06e-2, "S.emu_share.gru1": 8.53e-2,
    "T.logits": 2.15e-2, "T.logits_window": 4e-2, "T.probs": 1e-2,
    "T.emu_logits": 5.20e-3, "T.emu_logits_rms": 1.34e-3, "T.emu_stage_rms": 1.67e-3,
    "T.emu_share.res1": 3.61e-4, "T.emu_share.gru0": 1.82e-2, "T.emu_share.gru1": 8.49e-2,
    "U.logits": 1.83e-2, "U.logits_window": 2.57e-2, "U.probs": 2.34e-3,
    "U.emu_logits": 5.80e-3, "U.emu_logits_rms": 1.21e-3, "U.emu_stage_rms": 1.78e-3,
    "U.emu_share.res1": 4.97e-3, "U.emu_share.gru0": 2.70e-2, "U.emu_share.gru1": 9.41e-2,
}
# the tightest bound the older tests put on plain bf16: CONFIG4_MAX_ABS_DP_TEST on probabilities (tests/test_gpu_pipeline.py), and
# four times that on logits (the sigmoid divides a logit error by at least 4).  Nothing older bounds the emu_* quantities.
OLDER_BOUNDS = {"logits": 4.0 * CONFIG4_MAX_ABS_DP_TEST, "logits_window": 4.0 * CONFIG4_MAX_ABS_DP_TEST, "probs": CONFIG4_MAX_ABS_DP_TEST}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "infer_bf16_parity.jsonl")
KEEP = ("logits",) + STAGES


def yardstick(row):
    """The yardstick of one profile row.  Against float64: the float32 oracle's error plus the emulation's.  Against the emulation:
    the second implementation of the scheme (``model_forward(..., bf16=True, arith="float32")``) against the first."""
    return row["oracle_fp32"] + row["emulation"] if row["quantity"] in FP64_QUANTITIES else row["second"]


def bounds_from_profile(path=PROFILE):
    """{section.quantity: min(4 x largest yardstick in the profile, older bound)}: what ``BOUNDS`` may not exceed."""
    worst = {}
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            key = "%s.%s" % (row["section"], row["quantity"])
            worst[key] = max(worst.get(key, 0.0), yardstick(row))
    return {k: min(4.0 * v, OLDER_BOUNDS.get(k.split(".", 1)[1], np.inf)) for k, v in worst.items()}


def _rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64)))))


def _as_bf16(v):
    return m.bf16_round(np.asarray(v).astype(np.float32)).astype(np.float64)


def emu_errors(got, emu, extra=()):
    """{quantity: error} of ``got`` against the emulation ``emu`` (dicts of ``in_slabs`` form).  Logits: max|d| / max|ref| and
    rms(d) / rms(ref).  Stages (those ``got`` has, over the windows it has of them; both sides rounded to bf16, which is what the
    kernels store): the worst rms(d) / rms(ref), and per stage the share of elements that differ (as numbers: the two zeros are
    one).  ``extra``: stages beyond ``STAGES`` that enter the worst rms and whose share is printed only."""
    d = got["logits"] - emu["logits"]
    out = {"emu_logits": float(np.abs(d).max() / np.abs(emu["logits"]).max()), "emu_logits_rms": _rms(d) / _rms(emu["logits"])}
    worst = 0.0
    for k in STAGES + tuple(extra):
        if k not in got:
            continue
        g, ref = _as_bf16(got[k]), _as_bf16(emu[k][:len(got[k])])
        worst = max(worst, _rms(g - ref) / _rms(ref))
        share = float((g != ref).mean())
        if k in STAGES:
            out["emu_share." + k] = share
        else:
            print("share of %s elements that differ: %.3g" % (k, share))
    if any(k in got for k in STAGES):
        out["emu_stage_rms"] = worst
    return out


def _record(section, case, quantity, kernel, yards):
    """Print the row (always, before any assertion) and, in a measuring run, append it to the file CATFISH_PARITY_LOG names."""
    row = {"section": section, "case": case, "quantity": quantity, "kernel": float(kernel)}
    for k in ("oracle_fp32", "emulation", "second"):
        v = None if yards is None else yards[k].get(quantity)
        row[k] = None if v is None else float(v)
    print("parity %s" % json.dumps(row))
    path = os.environ.get("CATFISH_PARITY_LOG")
    if path and yards is not None:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(_stamp(), **row)) + "\n")


def _check(section, case, kernel, yards, stage_windows):
    """kernel: {quantity: error}.  All are recorded, then all are asserted (the shares only over at least SHARE_MIN_WINDOWS)."""
    for q, k in kernel.items():
        _record(section, case, q, k, yards)
    asserted = [q for q in kernel if not q.startswith("emu_share.") or stage_windows >= SHARE_MIN_WINDOWS]
    bad = {q: (kernel[q], BOUNDS["%s.%s" % (section, q)]) for q in asserted if not kernel[q] <= BOUNDS["%s.%s" % (section, q)]}
    assert not bad, (case, bad)


def _bf16_case(wkey, w, geo, n, keep=KEEP, sample=None):
    """``m._case`` (x, the float64 reference) with the emulation of the bf16 scheme at the same windows, computed once."""
    case = m._case(wkey, w, geo, n, keep=keep, sample=sample)
    if "emu" not in case:
        case["emu"] = m.in_slabs(lambda xs: m.model_forward(xs, w, bf16=True, **case["kw"]), case["x"][case["idx"]], keep)
    return case


def _yards(case, stage_windows):
    """The yardsticks of a case in a measuring run, else None: {name: {quantity: error}}."""
    if not _measuring():
        return None
    y = case["yards"]
    if "second" not in y:
        x, w, kw, keep = case["x"][case["idx"]], case["w"], case["kw"], case["keep"]
        y["oracle_fp32"] = m.errors(m.in_slabs(lambda xs: oracle.forward(xs, w, np.float32, return_stages=True, **kw), x, keep), case["ref"])
        y["emulation"] = m.errors(case["emu"], case["ref"])
        second = m.in_slabs(lambda xs: m.model_forward(xs, w, bf16=True, arith="float32", **kw), x, keep)
        second = {k: (v if k in ("probs", "logits") else v[:stage_windows]) for k, v in second.items()}
        y["second"] = emu_errors(second, case["emu"], extra=[k for k in keep if k not in KEEP])
    return y


def _run(section, label, eng, case, stages, want_slots):
    """One pass of the case's windows with the per-kernel profile on -> (errors against float64 and against the emulation, the
    windows the stages cover, the kernels' results).  ``want_slots``: exactly the launch slots that must have run."""
    got, slots = m._slots(eng, lambda: m._kernels(eng, case, stages))
    assert slots == set(want_slots), (label, slots)
    stage_windows = len(got[stages[0][0]])
    e = {q: v for q, v in m.errors(got, case["ref"]).items() if q in FP64_QUANTITIES}
    e.update(emu_errors(got, case["emu"], extra=[name for name, _ in stages if name not in STAGES]))
    print("%s: %d windows, stages over %d; largest |logit| %.3g" % (label, len(case["x"]), stage_windows, np.abs(case["ref"]["logits"]).max()))
    _check(section, label, e, _yards(case, stage_windows), stage_windows)
    return got


GEO = m.GEO_TUNED
SLOTS = ("res_stack2", "gru_layer_first", "gru_layer_mid", "gru_layer_last", "head")
STAGE_INDEX = (("res1", 1), ("gru0", 2), ("gru1", 3))
# window counts by label on C CUs -> (count, waves per workgroup of the biGRU launches: cf_pick_waves(2 tiles, C))
WINDOWS = {"1": lambda c: 1, "33": lambda c: 33, "257": lambda c: 257, "W2": lambda c: 32 * (c // 2 + 1) - 5, "W8": lambda c: 32 * (2 * c + 1) - 5}
WAVES = {"1": 1, "33": 1, "257": 1, "W2": 2, "W8": 8}


def _pick_waves(tiles32, n_cu):
    w = -(-2 * tiles32 // n_cu)
    return 1 if w <= 1 else (2 if w <= 2 else (4 if w <= 4 else 8))


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def weights():
    return oracle.random_weights(seed=5)


@pytest.fixture(scope="module")
def engine(weights):
    """The plain bf16 engine on random weights (seed 5), with room for the largest count in one pass."""
    eng = m._new_engine(weights, GEO, "bf16", cap=WINDOWS["W8"](_n_cu()) + 5)
    assert eng.launch_regimes()["n_cu"] == _n_cu()
    yield eng
    eng.close()


@pytest.fixture(scope="module", autouse=True)
def _cases_dropped():
    yield
    m._CASES.clear()


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("CATFISH_DEBUG_KNOBS", "CATFISH_BF16_PIPE", "CATFISH_BF16_WGS", "CATFISH_BF16_WAVES", "CATFISH_RES_FUSE", "CATFISH_RES_TPW",
              "CATFISH_RES_CHUNKS"):
        monkeypatch.delenv(k, raising=False)


def _sample(n):
    """The windows the references cover: all, or (sampled cases) the first and the last 256 and 512 random ones."""
    if n <= 2048:
        return None
    rng = np.random.default_rng(n + 1)
    return np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), rng.integers(256, n - 256, size=512)]))


# ------------------------------------------------------------------------------------------------ S. random weights (seed 5)
@pytest.mark.parametrize("label", list(WINDOWS))
def test_pipelined_kernels_match_the_rounding_model(engine, weights, label):
    """gru_bf16_pipe_kernel behind res_stack2_bf16_kernel<1, 1>: one window, a second tile with one valid window, nine tiles on
    one-wave workgroups, and two- and eight-wave workgroups with a ragged last tile (references sampled)."""
    n_cu = engine.launch_regimes()["n_cu"]
    n = WINDOWS[label](n_cu)
    assert _pick_waves((n + 31) // 32, n_cu) == WAVES[label], (label, n, n_cu)
    case = _bf16_case("S-random5", weights, GEO, n, sample=_sample(n))
    _run("S", "pipelined, random weights, %d windows (%s)" % (n, label), engine, case, STAGE_INDEX, SLOTS)


def test_bf16_logits_are_not_the_fp32_engines(engine, weights):
    """The mode ran: the bf16 engine's logits are not those of the fp32 engine on the same weights and windows."""
    case = _bf16_case("S-random5", weights, GEO, 33)
    f32 = m._new_engine(weights, GEO, "fp32", cap=64)
    try:
        plain = f32.infer_host(case["x"], return_logits=True)[1]
    finally:
        f32.close()
    got = engine.infer_host(case["x"], return_logits=True)[1]
    engine.check_error()
    assert plain.shape == got.shape and not np.array_equal(plain, got)
    assert np.abs(plain.astype(np.float64) - got).max() > 1e-5 * np.abs(plain).max()       # by far more than an fp32 reordering


def test_a_wave_that_walks_several_tiles_matches_the_rounding_model(engine, weights, monkeypatch, capfd):
    """CATFISH_BF16_WGS=1 CATFISH_BF16_WAVES=2 at 133 windows (five tiles): one workgroup per direction, wave 0 walks tiles 0, 2
    and 4, wave 1 tiles 1 and 3, so the pipelined kernel's prologue runs for a wave's second and third tile.  The library names
    every knob it honours on stderr, once per process and value: that is how the knobs are seen to have taken effect (no other
    test sets these two).  A tile's arithmetic does not depend on the wave that runs it: the logits are those of the natural launch."""
    case = _bf16_case("S-random5", weights, GEO, 133)
    natural = engine.infer_host(case["x"], return_logits=True)[1]
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    monkeypatch.setenv("CATFISH_BF16_WGS", "1")
    monkeypatch.setenv("CATFISH_BF16_WAVES", "2")
    capfd.readouterr()
    try:
        got = _run("S", "pipelined, random weights, 133 windows, one workgroup of two waves", engine, case, STAGE_INDEX, SLOTS)
    finally:
        out, err = capfd.readouterr()
        sys.stdout.write(out)
        sys.stderr.write(err)
    assert "debug knob CATFISH_BF16_WGS=1 is active" in err and "debug knob CATFISH_BF16_WAVES=2 is active" in err, err
    assert np.array_equal(got["logits"].reshape(-1), natural.astype(np.float64))


@pytest.mark.parametrize("n", [33, 257])
def test_unpipelined_kernel_matches_the_rounding_model(engine, weights, monkeypatch, n):
    """gru_layer_bf16_kernel<., ., 1> behind CATFISH_BF16_PIPE=0.  The knob switched kernels: the two accumulate in another order,
    so some fp32 logits differ (asserted from 257 windows on, the count printed)."""
    case = _bf16_case("S-random5", weights, GEO, n)
    piped = engine.infer_host(case["x"], return_logits=True)[1]
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
    monkeypatch.setenv("CATFISH_BF16_PIPE", "0")
    got = _run("S", "unpipelined, random weights, %d windows" % n, engine, case, STAGE_INDEX, SLOTS)
    differ = int((got["logits"].reshape(-1) != piped).sum())
    print("pipelined and unpipelined logits differ in %d of %d" % (differ, n * T))
    assert n < 257 or differ > 0


# ------------------------------------------------------------------------------------------------ U. random weights, three blocks
def test_three_block_stack_matches_the_rounding_model():
    """``n_layers_res=3``: the third block runs on res_block_bf16_kernel<false, 1> behind the fused launch of the first two.
    Another network than S's (its yardsticks on the logits are up to 2.7 x those of S), hence a section of its own."""
    geo = (64, 32, 3, 3)
    w = m._weights(geo, 5)
    keep = ("logits", "res1", "res2", "gru0", "gru1")
    case = _bf16_case("S-random5-three-blocks", w, geo, 33, keep=keep)
    eng = m._new_engine(w, geo, "bf16", cap=64)
    try:
        _run("U", "pipelined, random weights, three blocks, 33 windows", eng, case, (("res1", 1), ("res2", 2), ("gru0", 3), ("gru1", 4)),
             SLOTS + ("res_block",))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ T. the bundled checkpoint
@pytest.mark.parametrize("pipelined", [True, False])
def test_checkpoint_matches_the_rounding_model(ckpt_weights, monkeypatch, pipelined):
    """The bundled checkpoint, whose logits saturate, at 257 windows on both biGRU kernels."""
    case = _bf16_case("T-checkpoint", ckpt_weights, GEO, 257)
    eng = m._new_engine(ckpt_weights, GEO, "bf16", cap=512)
    try:
        piped = eng.infer_host(case["x"], return_logits=True)[1]
        if not pipelined:
            monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")
            monkeypatch.setenv("CATFISH_BF16_PIPE", "0")
        got = _run("T", "%s, checkpoint, 257 windows" % ("pipelined" if pipelined else "unpipelined"), eng, case, STAGE_INDEX, SLOTS)
    finally:
        eng.close()
    assert np.array_equal(got["logits"].reshape(-1), piped) == pipelined            # the knob switched kernels
