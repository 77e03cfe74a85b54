"""Shifted-window voting on the host: ``infer.check_phases``, the numpy definitions of ``catfish_amd/tilings.py`` against deliberately
naive per-sample loops, the one-read convenience, the route of a model without an engine, and the environment parsers.  The batches
and the naive loops here are shared with the replay and the GPU tests."""
import os

import numpy as np
import pytest

from catfish_amd import cli, infer, tilings
from test_bridge_host import _HostModel

W = 35
TRAP_LENGTHS = (0, 1, 34, 35, 36, 69, 70, 71, 700)
PHASE_SETS = ((0, 1), (0, 17), (0, 34), (0, 12, 23), (0, 5, 10, 15, 20, 25, 30, 34))
WEIGHTS = ("mean", "centre")
LAYOUTS = ("pipeline", "validation")


def layout_of(lengths, kind):
    """(offsets, lengths): the pipeline's layout (always at least one pad sample: n // 35 + 1 windows) or the validation's (an exact
    multiple of 35 has no tail, an empty read no window)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_win = lengths // W + 1 if kind == "pipeline" else (lengths + W - 1) // W
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(n_win * W, out=offsets[1:])
    return offsets, lengths


def trap_batch(kind, n_reads=9, seed=0):
    """(base [total], offsets, lengths): the trap lengths (or the last one alone), real samples random and never 0, tails 0."""
    rng = np.random.default_rng(seed)
    offsets, lengths = layout_of(TRAP_LENGTHS if n_reads == 9 else TRAP_LENGTHS[-n_reads:], kind)
    base = np.zeros(int(offsets[-1]), dtype=np.float32)
    for r, n in enumerate(lengths):
        base[offsets[r]:offsets[r] + n] = rng.uniform(0.5, 2.0, int(n)).astype(np.float32) * rng.choice([-1.0, 1.0], int(n)).astype(np.float32)
    return base, offsets, lengths


def random_batch(rng, kind):
    lengths = rng.integers(0, 300, int(rng.integers(1, 12)))
    offsets, lengths = layout_of(lengths, kind)
    base = np.zeros(int(offsets[-1]), dtype=np.float32)
    for r, n in enumerate(lengths):
        base[offsets[r]:offsets[r] + n] = rng.standard_normal(int(n)).astype(np.float32) + np.float32(3.0)
    return base, offsets, lengths


def special_values(rng, size):
    """float32 probabilities and logits with exact 0.0 and 1.0, denormals and +-30 logits among them."""
    probs = rng.random(size, dtype=np.float32)
    logits = (rng.standard_normal(size) * 6).astype(np.float32)
    pick = rng.integers(0, 12, size)
    probs[pick == 0], probs[pick == 1] = 0.0, 1.0
    probs[pick == 2], probs[pick == 3] = np.float32(1e-45), np.float32(3e-39)
    logits[pick == 4], logits[pick == 5], logits[pick == 6] = 30.0, -30.0, np.float32(-2e-40)
    return probs, logits


def naive_retile(base, offsets, lengths, phases):
    total, n = int(offsets[-1]), len(lengths)
    out = [0.0] * (total + (len(phases) - 1) * (total + W * n))
    for b in range(total):
        out[b] = base[b]
    for j in range(1, len(phases)):
        t_j = total + (j - 1) * (total + W * n)
        for r in range(n):
            for i in range(int(lengths[r])):
                out[t_j + int(offsets[r]) + W * r + phases[j] + i] = base[int(offsets[r]) + i]
    return np.array(out, dtype=np.float32)


def naive_vote(values, offsets, lengths, phases, weight):
    total, n = int(offsets[-1]), len(lengths)
    out = [values[b] for b in range(total)]
    if len(phases) > 1:
        for r in range(n):
            for i in range(int(lengths[r])):
                num = den = 0.0                                   # Python floats: doubles, summed in the order j = 0 .. K - 1
                for j, phi in enumerate(phases):
                    t = (i + phi) % W
                    w = 1 if weight == "mean" else min(t + 1, W - t)
                    where = int(offsets[r]) + i if j == 0 else total + (j - 1) * (total + W * n) + int(offsets[r]) + W * r + phi + i
                    num += w * float(values[where])
                    den += w
                out[int(offsets[r]) + i] = np.float32(num / den)
    return np.array(out, dtype=np.float32)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------- the rule
def test_check_phases():
    assert infer.check_phases is tilings.check_phases
    assert infer.check_phases((0,)) == (0,) and infer.check_phases([0]) == (0,) and infer.check_phases(None) == (0,)
    assert infer.check_phases(np.array([0, 12, 23])) == (0, 12, 23)
    eight = (0, 5, 10, 15, 20, 25, 30, 34)
    assert infer.check_phases(eight) == eight and all(type(p) is int for p in infer.check_phases(np.array(eight)))
    with pytest.raises(ValueError, match="between 1 and 8"):
        infer.check_phases(tuple(range(9)))
    with pytest.raises(ValueError, match="between 1 and 8"):
        infer.check_phases(())
    with pytest.raises(ValueError, match="first phase must be 0"):
        infer.check_phases((1, 2))
    with pytest.raises(ValueError, match="0 .. 34"):
        infer.check_phases((0, 35))
    with pytest.raises(ValueError, match="strictly ascending"):
        infer.check_phases((0, 5, 5))
    with pytest.raises(ValueError, match="strictly ascending"):
        infer.check_phases((0, 7, 3))
    with pytest.raises(ValueError, match="first phase must be 0"):
        infer.check_phases((-1, 3))
    for bad in ((0, 17.0), (0, "17"), (0, True), (0, None), "0,17", 17):
        with pytest.raises(ValueError, match="ints"):
            infer.check_phases(bad)
    assert tilings.check_weight("mean") == 0 and tilings.check_weight("centre") == 1 and tilings.check_weight(None) == 0
    for bad in ("center", 1, "", "MEAN"):
        with pytest.raises(ValueError, match="vote weight"):
            tilings.check_weight(bad)
    assert tilings.window_weight("centre", np.arange(W)).tolist() == [min(t + 1, W - t) for t in range(W)]
    assert tilings.window_weight("centre", [0, 17, 34]).tolist() == [1, 18, 1] and (tilings.window_weight("mean", np.arange(W)) == 1).all()
    assert tilings.tiling_size(700, 3, 1) == 700 and tilings.tiling_size(700, 3, 3) == 700 + 2 * (700 + 105)
    assert tilings.tiling_start(0, 700, 3) == 0 and tilings.tiling_start(2, 700, 3) == 700 + 805


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("phases", PHASE_SETS)
def test_trap_batch_against_the_naive_loops(kind, phases):
    base, offsets, lengths = trap_batch(kind)
    total, n = len(base), len(lengths)
    if kind == "validation":
        assert offsets[4] - offsets[3] == 35 and offsets[7] - offsets[6] == 70 and offsets[1] == 0       # 35 and 70 have no tail
    else:
        assert (np.diff(offsets) > lengths).all()
    retiled = tilings.retile_host(base, offsets, lengths, phases)
    assert len(retiled) == tilings.tiling_size(total, n, len(phases)) and len(retiled) % W == 0
    assert same_bits(retiled, naive_retile(base, offsets, lengths, phases))
    # every tiling window that holds no real sample is all zero; every real sample appears once per tiling
    for j in range(1, len(phases)):
        region = retiled[tilings.tiling_start(j, total, n):tilings.tiling_start(j + 1, total, n)]
        assert np.count_nonzero(region) == lengths.sum()
        real = np.zeros(len(region), dtype=bool)
        for r in range(n):
            real[offsets[r] + W * r + phases[j]:offsets[r] + W * r + phases[j] + lengths[r]] = True
        empty = ~real.reshape(-1, W).any(axis=1)
        assert empty.any() and not region.reshape(-1, W)[empty].any()
    rng = np.random.default_rng(11)
    probs, logits = special_values(rng, len(retiled))
    for weight in WEIGHTS:
        for values in (probs, logits):
            voted = tilings.vote_host(values, offsets, lengths, phases, weight)
            assert same_bits(voted, naive_vote(values, offsets, lengths, phases, weight))
            tail = np.ones(total, dtype=bool)
            for r in range(n):
                tail[offsets[r]:offsets[r] + lengths[r]] = False
            assert same_bits(voted[tail], values[:total][tail])                 # the zero tails keep the base value
        # a constant votes to itself exactly
        for c in (np.float32(0.3), np.float32(1.0), np.float32(1e-45)):
            assert same_bits(tilings.vote_host(np.full(len(retiled), c), offsets, lengths, phases, weight), np.full(total, c))


@pytest.mark.parametrize("kind", LAYOUTS)
def test_random_batches_against_the_naive_loops(kind):
    rng = np.random.default_rng(2024)
    for _ in range(6):
        base, offsets, lengths = random_batch(rng, kind)
        phases = tuple([0] + sorted(rng.choice(np.arange(1, W), int(rng.integers(1, 8)), replace=False).tolist()))
        weight = WEIGHTS[int(rng.integers(0, 2))]
        retiled = tilings.retile_host(base, offsets, lengths, phases)
        assert same_bits(retiled, naive_retile(base, offsets, lengths, phases))
        values, _ = special_values(rng, len(retiled))
        assert same_bits(tilings.vote_host(values, offsets, lengths, phases, weight), naive_vote(values, offsets, lengths, phases, weight))


@pytest.mark.parametrize("kind", LAYOUTS)
def test_one_phase_is_the_identity(kind):
    base, offsets, lengths = trap_batch(kind)
    assert same_bits(tilings.retile_host(base, offsets, lengths, (0,)), base)
    rng = np.random.default_rng(5)
    values, _ = special_values(rng, len(base))
    for weight in WEIGHTS:
        assert same_bits(tilings.vote_host(values, offsets, lengths, (0,), weight), values)


def test_unsound_table_entries_are_zero_and_unvoted():
    base, offsets, lengths = trap_batch("pipeline")
    total, n, phases = len(base), len(lengths), (0, 12, 23)
    rng = np.random.default_rng(6)
    values, _ = special_values(rng, tilings.tiling_size(total, n, 3))
    good_x, good_v = tilings.retile_host(base, offsets, lengths, phases), tilings.vote_host(values, offsets, lengths, phases, "centre")
    for r, bad_len in ((8, -1), (8, 736), (5, 71), (8, np.iinfo(np.int64).max), (8, np.iinfo(np.int64).min)):
        lens = lengths.copy()
        lens[r] = bad_len
        got_x = tilings.retile_host(base, offsets, lens, phases, total=total)
        got_v = tilings.vote_host(values, offsets, lens, phases, "centre", total=total)
        want_x = good_x.copy()
        for j in (1, 2):
            t_j = tilings.tiling_start(j, total, n)
            want_x[t_j + offsets[r] + W * r:t_j + offsets[r + 1] + W * (r + 1)] = 0
        want_v = good_v.copy()
        want_v[offsets[r]:offsets[r + 1]] = values[offsets[r]:offsets[r + 1]]
        assert same_bits(got_x, want_x) and same_bits(got_v, want_v)


# --------------------------------------------------------------------------- one read
def position_stub(raw_in):
    """A stand-in for ``model.infer``: the probability of a sample is its own value / 1000 plus its position in the window / 70, so
    every tiling answers differently for the same sample and a sample that moved to the wrong place shows."""
    raw_in = np.asarray(raw_in)
    assert raw_in.ndim == 3 and raw_in.shape[1:] == (W, 1)
    x = raw_in.reshape(-1, W)
    return (x / 1000.0 + np.arange(W)[None, :] / 70.0).reshape(-1).astype(np.float32)


@pytest.mark.parametrize("length", (1, 34, 35, 36, 700))
@pytest.mark.parametrize("weight", WEIGHTS)
def test_voted_probs_of_read(length, weight):
    raw = np.arange(1, length + 1, dtype=np.float64)
    pad = infer.padding_size_for(length)
    raw_in = np.concatenate([raw, np.zeros(pad)]).reshape(-1, W, 1)
    assert same_bits(tilings.voted_probs_of_read(raw_in, position_stub, length, (0,), weight), position_stub(raw_in))
    for phases in PHASE_SETS:
        got = tilings.voted_probs_of_read(raw_in, position_stub, length, phases, weight)
        assert got.dtype == np.float32 and len(got) == length + pad
        for i in range(length):
            num = den = 0.0
            for phi in phases:
                t = (i + phi) % W
                w = 1 if weight == "mean" else min(t + 1, W - t)
                num += w * float(np.float32(raw[i] / 1000.0 + t / 70.0))
                den += w
            assert got[i] == np.float32(num / den), (phases, i)
        assert same_bits(got[length:], position_stub(raw_in)[length:])


def test_infer_class_from_raw_without_an_engine():
    rng = np.random.default_rng(9)
    raw = rng.standard_normal(1000)
    probs = (0.5 + 0.49 * np.sin(np.arange(1015 + W) / 23.0) + rng.uniform(-0.2, 0.2, 1015 + W)).clip(0, 1).astype(np.float32)
    model = _HostModel(probs)
    plain = infer.infer_class_from_raw(raw, model)
    assert infer.infer_class_from_raw(raw, model, phases=(0,), vote_weight="centre") == plain
    differs = False
    for phases in ((0, 17), (0, 12, 23)):
        for weight in WEIGHTS:
            # the stub answers probs[k] for sample k of whatever it is given: tiling j holds sample i at i + phi_j
            values = np.concatenate([probs[:1015]] + [probs[:1015 + W]] * (len(phases) - 1))
            voted = naive_vote(values, np.array([0, 1015]), np.array([1000]), phases, weight)[:1000]
            want = infer.hp_in_pred(infer.correct_short(infer.class_from_threshold(voted)))
            assert infer.infer_class_from_raw(raw, model, phases=phases, vote_weight=weight) == (want, 1000)
            differs = differs or want != plain[0]
            want3 = infer.hp_in_pred(infer.correct_short(infer.bridge_gaps(infer.class_from_threshold(voted), 3)))
            assert infer.infer_class_from_raw(raw, model, phases=phases, vote_weight=weight, max_gap=3) == (want3, 1000)
            spans, length, rows = infer.infer_class_from_raw(raw, model, phases=phases, vote_weight=weight, scores=True)
            assert (spans, length) == (want, 1000) and rows.shape == (len(want), 6)
            for (s, e), row in zip(spans, rows):
                p = voted[s + 11:e - 16]
                assert row[0] == len(p) and row[2] == p.min() and row[3] == p.max() and abs(row[1] - p.astype(np.float64).mean()) < 1e-12
    assert differs
    with pytest.raises(ValueError, match="first phase must be 0"):
        infer.infer_class_from_raw(raw, model, phases=(3, 5))
    with pytest.raises(ValueError, match="vote weight"):
        infer.infer_class_from_raw(raw, model, phases=(0, 5), vote_weight="median")


# --------------------------------------------------------------------------- the environment
def test_env_parsers(monkeypatch):
    assert tilings.phases_from_env(None) == (0,) and tilings.phases_from_env("") == (0,) and tilings.phases_from_env("  ") == (0,)
    assert tilings.phases_from_env("0,12,23") == (0, 12, 23) and tilings.phases_from_env(" 0 , 17 ") == (0, 17)
    for bad in ("12,23", "0,35", "0,5,5", "0,a", "0;17", "0,1,2,3,4,5,6,7,8", "0,,5", "0.0,17"):
        with pytest.raises(ValueError):
            tilings.phases_from_env(bad)
    assert tilings.weight_from_env(None) == "mean" and tilings.weight_from_env("") == "mean" and tilings.weight_from_env("centre") == "centre"
    with pytest.raises(ValueError):
        tilings.weight_from_env("center")
    monkeypatch.delenv("CATFISH_TILINGS", raising=False)
    monkeypatch.delenv("CATFISH_TILING_WEIGHT", raising=False)
    assert cli.tilings_from_env() == ((0,), "mean")
    monkeypatch.setenv("CATFISH_TILINGS", "0,12,23")
    monkeypatch.setenv("CATFISH_TILING_WEIGHT", "centre")
    assert cli.tilings_from_env() == ((0, 12, 23), "centre")
    monkeypatch.setenv("CATFISH_TILINGS", "5,12")
    with pytest.raises(ValueError, match="CATFISH_TILINGS"):
        cli.tilings_from_env()
    monkeypatch.setenv("CATFISH_TILINGS", "0,12")
    monkeypatch.setenv("CATFISH_TILING_WEIGHT", "middle")
    with pytest.raises(ValueError, match="CATFISH_TILING_WEIGHT"):
        cli.tilings_from_env()


def test_the_command_line_refuses_a_bad_value_before_any_rank_starts(monkeypatch, tmp_path):
    click_testing = pytest.importorskip("click.testing")
    started = []
    monkeypatch.setattr(cli, "launch_ranks", lambda *a, **k: started.append("ranks") or 0)
    monkeypatch.setattr(cli, "run_pipeline", lambda *a, **k: started.append("pipeline"))
    monkeypatch.setenv("CATFISH_TILINGS", "0,40")
    res = click_testing.CliRunner().invoke(cli._build_click_main(), ["-i", str(tmp_path), "-s", str(tmp_path / "out"), "-g", "2"])
    assert isinstance(res.exception, ValueError) and "CATFISH_TILINGS" in str(res.exception) and started == []
    monkeypatch.setenv("CATFISH_TILINGS", "0,12")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res = click_testing.CliRunner().invoke(cli._build_click_main(), ["-i", str(tmp_path), "-s", str(tmp_path / "out")])
    assert res.exception is None and started == ["pipeline"]
