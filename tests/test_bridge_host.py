"""Bridging short gaps between called stretches, host logic: ``infer.bridge_gaps`` (the definition) against a per-sample statement
on planted traps and on the random batch the replay and the GPU tests share; ``max_gap=0`` changes nothing anywhere; the host
validation definitions with a gap; refused pairs.  No GPU."""
import json
import os

import numpy as np
import pytest

from catfish_amd import infer
from catfish_amd.device_validation import run_borders_host, run_states_host
from catfish_amd.span_scores import SCORE_COLUMNS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESHOLDS = (0.5, 0.75)
PAIRS = ((1, 15), (5, 15), (15, 15), (49, 15), (63, 1), (8, 1), (32, 32))        # (max_gap, min_run): the domain's corners among them
UNBRIDGED = ((0, 15), (0, 64))
REFUSED = ((50, 15), (1, 65))
HI, LO = np.float32(0.9), np.float32(0.1)


# ------------------------------------------------------------------------------------------------ batches
def planted(seed, lengths, pads):
    """Random reads: positive stretches of ~9 samples, gaps short (~4) or of up to 100 samples; padding planted HIGH."""
    rng = np.random.default_rng(seed)
    offs, out = [0], []
    for L, P in zip(lengths, pads):
        v = np.empty(L, np.float32)
        i = 0
        state = bool(rng.integers(2))
        while i < L:
            d = int(rng.geometric(1 / 9.)) if state else (int(rng.geometric(1 / 4.)) if rng.random() < .5 else int(rng.integers(1, 101)))
            d = min(d, L - i)
            v[i:i + d] = (.5 + .5 * rng.random(d)) if state else .4999 * rng.random(d)
            i += d
            state = not state
        out += [v, np.full(P, .99, np.float32)]
        offs.append(offs[-1] + L + P)
    return np.concatenate(out), np.array(offs), np.array(lengths)


RANDOM_LENGTHS = [4130, 63, 64, 65, 1, 3968, 3969, 7953, 200, 0, 129]
RANDOM_PADS = [35, 7, 0, 0, 34, 0, 31, 0, 0, 5, 1]

_cache = {}


def random_batch():
    """(probs float32 [20 655], offsets int64 [12], lengths int64 [11]): 323 words, two workgroups.  Built once, never written to."""
    if "random" not in _cache:
        probs, offs, lengths = planted(7, RANDOM_LENGTHS, RANDOM_PADS)
        assert len(probs) == 20655
        probs.setflags(write=False)
        _cache["random"] = (probs, offs.astype(np.int64), lengths.astype(np.int64))
    return _cache["random"]


def trap_batch():
    """Every trap of the feature in one packed batch -> (probs, offsets, lengths, notes).  ``notes``: name -> packed position(s)
    the tests look at.  Ones are 0.9, zeros 0.1, padding 0.99."""
    if "traps" in _cache:
        return _cache["traps"]
    reads, pads, notes = [], [], {}

    def read(length, ones=(), pad=0, fill=LO):
        v = np.full(length, fill, np.float32)
        for a, b in ones:
            v[a:b] = HI
        reads.append(v)
        pads.append(pad)
        return v

    # read 0 (packed 0 .. 4200): leading zeros, a gap at the word edge 63|64, the chain, 1010.., NaNs, the wave edge 3967|3968,
    # trailing zeros; then HIGH padding
    v = read(4200, [(2, 30), (33, 62), (66, 100), (200, 205), (208, 213), (216, 221), (400, 420), (422, 440), (500, 520),
                    (3940, 3966), (3970, 4000), (4150, 4198)], pad=10)
    v[300:340:2] = HI                                        # 1010...10
    v[420] = np.nan                                          # a NaN inside a gap of two
    v[520] = np.nan                                          # a NaN where the run would go on: its end
    v[521:540] = HI
    notes.update(leading=(0, 2), gap3=(30, 33), word_edge=(62, 66), chain=(200, 221), alternating=(300, 340), nan_gap=(420, 422),
                 nan_end=520, wave_edge=(3966, 3970), trailing=(4198, 4200))
    # read 1: a ladder of gaps of 1 .. 66 samples between stretches of 20 ones: a gap of exactly max_gap and one of max_gap + 1
    ladder, at = [], 3
    for g in range(1, 67):
        ladder.append((at, at + 20))
        at += 20 + g
    ladder.append((at, at + 20))
    read(at + 25, ladder, pad=3)
    # reads 2, 3: one ends with ones, HIGH padding, the next begins with ones
    read(100, [(60, 100)], pad=2)
    read(90, [(0, 40)], pad=35)
    # reads 4 .. 7, packed without padding: ...1 0 | 0 1...   ...1 | 0 1...   ...1 | 1...
    read(80, [(40, 79)])
    read(70, [(1, 70)])
    read(60, [(1, 60)])
    read(50, [(0, 30)], pad=4)
    # gaps within reach of a read's first and last sample: ones at the very ends must survive, the gaps next to them fill
    read(120, [(0, 4), (6, 40), (80, 114), (116, 120)], pad=1)
    read(120, [(3, 40), (80, 117)], pad=1)                   # zeros at both ends: never filled
    # lengths 0, 1, 63, 64, 65; an all-ones read and an all-zeros read
    read(0, pad=5)
    read(1, [(0, 1)], pad=34)
    read(63, [(0, 63)])
    read(64)
    read(65, [(0, 20), (23, 65)], pad=5)
    read(3968, [(0, 3968)])                                  # all ones, then a read right behind it
    # ... of 3969 samples, which covers the workgroup edge 15871|15872: a gap of four there
    start = int(sum(len(r) + p for r, p in zip(reads, pads)))
    a = 15870 - start
    assert 1100 < a < 3900
    read(3969, [(5, 1000), (1003, a), (a + 4, 3969)], pad=31)
    notes["workgroup_edge"] = (15870, 15874)
    offs = np.concatenate(([0], np.cumsum([len(r) + p for r, p in zip(reads, pads)]))).astype(np.int64)
    probs = np.concatenate([np.concatenate((r, np.full(p, .99, np.float32))) for r, p in zip(reads, pads)])
    probs.setflags(write=False)
    _cache["traps"] = (probs, offs, np.array([len(r) for r in reads], np.int64), notes)
    return _cache["traps"]


# ------------------------------------------------------------------------------------------------ definitions
def bits_of(p, threshold):
    with np.errstate(invalid="ignore"):
        return (np.asarray(p, np.float32) >= np.float32(threshold)).astype(np.int64)


def brute_bridge(bits, max_gap):
    """Per sample: a zero is filled iff the nearest one below and the nearest one above exist and have at most max_gap zeros
    between them."""
    b = [int(v) for v in bits]
    out = list(b)
    for i, v in enumerate(b):
        if v:
            continue
        lo = i - 1
        while lo >= 0 and not b[lo]:
            lo -= 1
        hi = i + 1
        while hi < len(b) and not b[hi]:
            hi += 1
        if lo >= 0 and hi < len(b) and hi - lo - 1 <= max_gap:
            out[i] = 1
    return np.array(out, np.int64)


def host_bridged(probs, offsets, lengths, threshold, max_gap, min_run):
    """The definition over a packed batch -> (labels uint8 [total], starts, ends (packed, sorted, ends exclusive), gaps filled, interior
    gaps kept)."""
    shared = not probs.flags.writeable                       # the two batches above live as long as the process: their id is a key
    key = (id(probs), threshold, max_gap, min_run)
    if shared and key in _cache:
        return _cache[key]
    labels = np.zeros(len(probs), np.uint8)
    starts, ends, filled, kept = [], [], 0, 0
    for r, n in enumerate(lengths.tolist()):
        if n == 0:
            continue
        beg = int(offsets[r])
        bits = bits_of(probs[beg:beg + n], threshold)
        bridged = infer.bridge_gaps(bits, max_gap)
        lab = np.asarray(infer.correct_short(bridged, min_run))
        labels[beg:beg + n] = lab
        d = np.diff(np.concatenate(([0], lab, [0])))
        starts += (np.flatnonzero(d == 1) + beg).tolist()
        ends += (np.flatnonzero(d == -1) + beg).tolist()
        z = np.diff(np.concatenate(([1], bits, [1])))        # zero runs of the raw bits
        for s, t in zip(np.flatnonzero(z == -1).tolist(), np.flatnonzero(z == 1).tolist()):
            if s > 0 and t < n:
                filled += int(bridged[s] == 1)
                kept += int(bridged[s] == 0)
    labels.setflags(write=False)
    out = (labels, np.array(starts, np.int64), np.array(ends, np.int64), filled, kept)
    if shared:
        _cache[key] = out
    return out


# ------------------------------------------------------------------------------------------------ bridge_gaps
def test_bridge_gaps_on_small_cases():
    f = lambda s, g: "".join(map(str, infer.bridge_gaps([int(c) for c in s], g).tolist()))      # noqa: E731
    assert f("0011001100", 2) == "0011111100" and f("0011001100", 1) == "0011001100"
    assert f("0110", 5) == "0110" and f("1001", 2) == "1111" and f("1001", 1) == "1001"
    assert f("0001000", 63) == "0001000" and f("", 3) == "" and f("0", 3) == "0" and f("1", 3) == "1"
    assert f("10101010", 1) == "11111110" and f("01010101", 1) == "01111111"
    assert f("1001", 0) == "1001" and f("1001", -3) == "1001"
    b = np.array([1, 0, 1])
    assert infer.bridge_gaps(b, 1).tolist() == [1, 1, 1] and b.tolist() == [1, 0, 1]        # a copy


@pytest.mark.parametrize("max_gap", [0, 1, 2, 3, 4, 8, 15, 49, 63])
def test_bridge_gaps_against_the_per_sample_statement(max_gap):
    rng = np.random.default_rng(max_gap)
    for _ in range(300):
        n = int(rng.integers(0, 90))
        bits = (rng.random(n) < rng.choice([0.2, 0.5, 0.8])).astype(np.int64)
        assert np.array_equal(infer.bridge_gaps(bits, max_gap), brute_bridge(bits, max_gap))
    for probs, offsets, lengths in (trap_batch()[:3], random_batch()):
        for r in range(len(lengths)):
            if lengths[r] <= 4200:
                bits = bits_of(probs[offsets[r]:offsets[r] + lengths[r]], 0.5)
                assert np.array_equal(infer.bridge_gaps(bits, max_gap), brute_bridge(bits, max_gap)), r


def test_the_traps_hold_what_they_say():
    probs, offsets, lengths, notes = trap_batch()
    assert sorted(lengths.tolist())[:5] == [0, 1, 50, 60, 63] and {64, 65, 3968, 3969} <= set(lengths.tolist())
    assert offsets[-1] > 15872 and np.isnan(probs[420]) and np.isnan(probs[520])
    lab = lambda g, m=15: host_bridged(probs, offsets, lengths, 0.5, g, m)[0]      # noqa: E731
    # leading and trailing zeros are never filled, ones near the ends are never eroded
    for g in (1, 5, 49):
        assert not lab(g)[0:2].any() and not lab(g)[4198:4200].any() and lab(g)[2:30].all() and lab(g)[4150:4198].all()
    # edges of a word, a wave, a workgroup: a gap of four fills at 4, not at 3
    for name in ("word_edge", "wave_edge", "workgroup_edge"):
        a, b = notes[name]
        assert b - a == 4 and not lab(3)[a:b].any() and lab(4)[a:b].all() and lab(3)[a - 1] and lab(3)[b], name
    # the chain 5 3 5 3 5 is a call only from max_gap 3 on
    assert not lab(2)[200:221].any() and lab(3)[200:221].all() and not lab(3)[199] and not lab(3)[221]
    # 1010...10 with max_gap 1: 39 ones
    assert not lab(0)[300:340].any() and lab(1)[300:339].all() and not lab(1)[339]
    # NaN: false inside a gap (filled), and the end of a run
    assert lab(0)[400:420].all() and not lab(0)[420:422].any() and lab(2)[400:440].all() and not lab(1)[420]
    assert lab(0)[500:520].all() and not lab(0)[520] and lab(1)[500:540].all()
    # padding planted HIGH is never a label and never a bridge
    for r in range(len(lengths)):
        assert not lab(49)[offsets[r] + lengths[r]:offsets[r + 1]].any()
    _l, starts, ends, _f, _k = host_bridged(probs, offsets, lengths, 0.5, 49, 15)
    assert int(offsets[2] + 100) in ends and int(offsets[3]) in starts
    # packed without padding: 1 0 | 0 1, 1 | 0 1 and 1 | 1 stay apart
    for r in (5, 6, 7):
        assert offsets[r] == offsets[r - 1] + lengths[r - 1]
    full = lab(49)
    assert not full[offsets[5] - 1] and not full[offsets[5]] and full[offsets[5] - 2] and full[offsets[5] + 1]
    assert full[offsets[6] - 1] and not full[offsets[6]] and full[offsets[6] + 1]
    assert full[offsets[7] - 1] and full[offsets[7]] and int(offsets[7]) in starts and int(offsets[7]) in ends
    # the ladder: a gap of exactly max_gap fills, one of max_gap + 1 stays
    at = int(offsets[1]) + 3
    for g in range(1, 67):
        gap = slice(at + 20, at + 20 + g)
        for max_gap in (1, 5, 15, 49):
            assert lab(max_gap)[gap].all() == (g <= max_gap) and lab(max_gap)[gap].any() == (g <= max_gap)
        at += 20 + g


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("max_gap,min_run", PAIRS)
def test_the_random_batch_shows_something(threshold, max_gap, min_run):
    probs, offsets, lengths = random_batch()
    labels, starts, ends, filled, kept = host_bridged(probs, offsets, lengths, threshold, max_gap, min_run)
    assert filled >= 50 and kept >= 50
    plain = host_bridged(probs, offsets, lengths, threshold, 0, min_run)[0]
    assert 100 <= int((labels != plain).sum())
    assert len(starts) == len(ends) and (ends - starts >= min_run).all()


# ------------------------------------------------------------------------------------------------ max_gap = 0 is the identity
class _HostModel(object):
    """A model without an engine: probabilities planted per window."""

    def __init__(self, probs):
        self.probs = probs

    def infer(self, raw_in):
        assert raw_in.shape[1:] == (35, 1)
        return self.probs[:raw_in.shape[0] * 35].astype(float)


def _planted_read():
    rng = np.random.default_rng(5)
    raw = rng.standard_normal(1000)
    probs = np.full(1015, 0.99, dtype=np.float32)
    probs[:1000] = (rng.random(1000) * 0.4).astype(np.float32)
    probs[100:110] = 0.93
    probs[114:124] = 0.93                                    # 10 ones, 4 zeros, 10 ones: no call without bridging
    probs[400:460] = 0.8
    probs[990:1000] = 0.71                                   # ends the read: the HIGH padding behind it must not help
    return raw, probs


def test_infer_class_from_raw_on_a_model_without_an_engine():
    raw, probs = _planted_read()
    model = _HostModel(probs)
    plain = infer.infer_class_from_raw(raw, model)
    assert plain == ([[389, 476]], 1000)
    assert infer.infer_class_from_raw(raw, model, max_gap=0) == plain
    assert infer.infer_class_from_raw(raw, model, max_gap=3) == plain
    assert infer.infer_class_from_raw(raw, model, max_gap=4) == ([[89, 140], [389, 476]], 1000)
    spans0, length0, rows0 = infer.infer_class_from_raw(raw, model, scores=True)
    spans, length, rows = infer.infer_class_from_raw(raw, model, scores=True, max_gap=0)
    assert (spans, length) == (spans0, length0) == plain and rows.tobytes() == rows0.tobytes()
    spans, length, rows = infer.infer_class_from_raw(raw, model, scores=True, max_gap=4)
    assert spans == [[89, 140], [389, 476]] and rows.shape == (2, len(SCORE_COLUMNS))
    p = probs[100:124].astype(np.float64)
    assert rows[0, 0] == 24 and abs(rows[0, 1] - p.mean()) < 1e-12 and rows[0, 2] == p.min() < 0.5 and rows[0, 3] == p.max()
    assert rows[1].tobytes() == rows0[0].tobytes()


def test_the_other_entry_points_on_a_model_without_an_engine(tmp_path, monkeypatch):
    """``infer_class_from_signal`` takes the host definition too; the batch routes, the pipeline's runner and the command line need
    an engine and say so as before, whatever the gap (a refused pair is looked at only where there is an engine to refuse it for)."""
    from catfish_amd import batching, cli, sharding
    _raw, probs = _planted_read()
    model = _HostModel(probs)
    path = str(tmp_path / "read.npy")
    np.save(path, np.random.default_rng(1).integers(300, 700, size=1000).astype(np.int16))
    plain = infer.infer_class_from_signal(path, model)
    assert plain == ([[389, 476]], 1000) and infer.infer_class_from_signal(path, model, max_gap=0) == plain
    assert infer.infer_class_from_signal(path, model, max_gap=4) == ([[89, 140], [389, 476]], 1000)
    spans, length, rows = infer.infer_class_from_signal(path, model, scores=True, max_gap=4)
    assert (spans, length) == ([[89, 140], [389, 476]], 1000) and rows[:, 0].tolist() == [24.0, 60.0]
    with pytest.raises(ValueError):
        infer.infer_class_from_signal(path, model, max_gap=50)

    class NoWeights(object):
        engine = None

    for gap in (0, 4, 50):
        for call in (lambda: batching.infer_reads(NoWeights(), [np.zeros(70)], max_gap=gap),
                     lambda: batching.infer_reads_dac(NoWeights(), [np.zeros(70, np.int16)], max_gap=gap),
                     lambda: sharding.EngineBatchRunner(NoWeights(), 12000, max_gap=gap)):
            with pytest.raises(RuntimeError, match="network has no weights"):
                call()
    # the command line's switch: unset, empty and 0 are "off"; anything but an integer in 0 .. 49 names the variable
    for text, want in ((None, 0), ("", 0), ("0", 0), ("7", 7), ("49", 49)):
        monkeypatch.delenv("CATFISH_BRIDGE_GAP", raising=False)
        if text is not None:
            monkeypatch.setenv("CATFISH_BRIDGE_GAP", text)
        assert cli.bridge_gap_from_env() == want
    for text in ("50", "-1", "four", "2.5"):
        monkeypatch.setenv("CATFISH_BRIDGE_GAP", text)
        with pytest.raises(ValueError, match="CATFISH_BRIDGE_GAP"):
            cli.bridge_gap_from_env()
    with pytest.raises(ValueError):                            # before a directory is made or a network loaded
        cli.run_pipeline(str(tmp_path / "none"), str(tmp_path / "out"), bridge_gap=50)
    assert not (tmp_path / "out").exists()


def test_max_gap_0_leaves_the_validation_goldens_as_they_are():
    """The reference's records (tests/golden/run_states_golden.*, run_borders_golden.json) through ``max_gap=0``."""
    import test_run_borders_host as borders
    import test_run_states_host as states
    scores, labels, offsets, cases = states.golden()
    assert len(cases) > 100
    for case in cases:
        a, b = int(offsets[case["stretch"]]), int(offsets[case["stretch"] + 1])
        got = run_states_host(scores[a:b], labels[a:b], [0, b - a], [b - a], [case["threshold"]], (), case["min_run"], max_gap=0)
        assert np.array_equal(got[0], states.table_of(case["runs"])), case
    with open(os.path.join(GOLDEN, "run_borders_golden.json")) as fh:
        cases = json.load(fh)["cases"]
    assert len(cases) > 100
    for case in cases:
        a, b = int(offsets[case["stretch"]]), int(offsets[case["stretch"] + 1])
        got = run_borders_host(scores[a:b], labels[a:b], [0, b - a], [b - a], [case["threshold"]], 64, case["min_run"], max_gap=0)
        assert np.array_equal(got[0], borders.table_of(case["runs"], 64)), case


def test_a_homopolymer_called_in_two_pieces_is_found_once_bridged():
    y = np.zeros(100, np.uint8)
    y[30:54] = 1
    p = np.full(100, 0.1, np.float32)
    p[30:40] = 0.9
    p[44:54] = 0.9                                           # 10 ones, 4 zeros, 10 ones
    bounds, lengths = np.array([0, 100]), np.array([100])
    plain = run_states_host(p, y, bounds, lengths, [0.5], (), 15)
    assert plain[0, 0, 0].tolist() == [0, 0, 1] and plain[0, 1].sum() == 0                  # absent; nothing called
    assert np.array_equal(run_states_host(p, y, bounds, lengths, [0.5], (), 15, max_gap=3), plain)
    bridged = run_states_host(p, y, bounds, lengths, [0.5], (), 15, max_gap=4)
    assert bridged[0, 0, 0].tolist() == [1, 0, 0] and bridged[0, 1, 0].tolist() == [1, 0, 0]
    reach = 8
    # in pieces of 15 and 16 with a gap of 4: one interruption of the true run at gap 0, none at gap 4
    y = np.zeros(100, np.uint8)
    y[30:65] = 1
    p = np.full(100, 0.1, np.float32)
    p[30:45] = 0.9
    p[49:65] = 0.9
    plain = run_borders_host(p, y, bounds, lengths, [0.5], reach, 15)
    assert plain[0, 0, 5 * reach + 2] == 1 and plain[0, 0, 4 * reach + 2 + 3] == 1
    bridged = run_borders_host(p, y, bounds, lengths, [0.5], reach, 15, max_gap=4)
    assert bridged[0, 0, 5 * reach + 2] == 0 and bridged[0, 0, 4 * reach + 2:5 * reach + 2].sum() == 0
    assert bridged[0, 0, reach] == 1 and bridged[0, 0, 2 * reach + 1 + reach] == 1          # both borders hit exactly


# ------------------------------------------------------------------------------------------------ refused pairs
@pytest.mark.parametrize("max_gap,min_run", REFUSED)
def test_refused_pairs_raise(max_gap, min_run):
    with pytest.raises(ValueError):
        infer.check_bridge(max_gap, min_run)
    p, y = np.full(50, 0.9, np.float32), np.ones(50, np.uint8)
    with pytest.raises(ValueError):
        run_states_host(p, y, [0, 50], [50], [0.5], (), min_run, max_gap=max_gap)
    with pytest.raises(ValueError):
        run_borders_host(p, y, [0, 50], [50], [0.5], 8, min_run, max_gap=max_gap)


def test_what_check_bridge_takes():
    for max_gap, min_run in PAIRS + UNBRIDGED + ((0, 200), (None, 15)):
        assert infer.check_bridge(max_gap, min_run) == (max_gap or 0)
    for bad in (-1, 2.5, True, 50):
        with pytest.raises(ValueError):
            infer.check_bridge(bad, 15)
    raw, probs = _planted_read()
    with pytest.raises(ValueError):
        infer.infer_class_from_raw(raw, _HostModel(probs), max_gap=50)
    from catfish_amd import train_validate
    with pytest.raises(ValueError):
        train_validate.threshold_sweep(None, None, [0.5], 1000, bridge_gap=50, run_edges=())
    with pytest.raises(ValueError):
        train_validate.threshold_sweep(None, None, [0.5], 1000, bridge_gap=3)          # nothing it could change
