"""The tiled training set on the host (no GPU): ``device_db.tiled_tables`` against a plain loop over every start, its miss quota
against ``centre_tables``' own selection rule, ``DeviceTiledDb``'s sampler contract, the CPU trainer on it, the environment of
``train_validate.main``, and the constants of tests/test_tiled_db_gpu.py against their profile."""
import os

import numpy as np
import pytest

from catfish_amd import device_db as ddb, train_validate as tv
from catfish_amd.device_db import DeviceExampleDb, DeviceTiledDb, WINDOW, tiled_tables

LENGTHS = (34, 35, 36, 69, 70, 71, 105)
STRIDES = (1, 7, 35, 36)


# ---------------------------------------------------------------------------------------------------- the reads
def _reads():
    """Label arrays, one per read, in one fixed order: every length of LENGTHS under every pattern that fits it, an empty read
    among them, and a read that ends in a run followed by a read that starts with one."""
    reads = []
    for n in LENGTHS:
        first_run = np.zeros(n, np.uint8); first_run[:min(n, 5)] = 1                 # a run at the read's first sample
        last_run = np.zeros(n, np.uint8); last_run[max(0, n - 5):] = 1               # a run at the read's last sample
        reads += [first_run, last_run, np.ones(n, np.uint8), np.zeros(n, np.uint8)]
        for at in (35, 34 + 35, 0, 34):                                             # a single 1 at sample 0 / 34 of a window of the grid
            if at < n:
                one = np.zeros(n, np.uint8); one[at] = 1
                reads.append(one)
        reads.append(np.zeros(0, np.uint8))                                         # an empty read among the others
    ends = np.zeros(71, np.uint8); ends[60:] = 1                                     # this read ends in a run ...
    starts = np.zeros(70, np.uint8); starts[:8] = 1                                  # ... and the next one starts with one
    return reads + [ends, starts]


def _layout(reads):
    offsets = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([r.size for r in reads], out=offsets[1:])
    return (np.concatenate(reads) if reads else np.zeros(0, np.uint8)), offsets


def _brute(reads, stride):
    """(read, start-in-read, number of ones) of every window, by a plain loop over every start."""
    out = []
    for rho, lab in enumerate(reads):
        k = 0
        while k * stride + WINDOW <= lab.size:
            ones = sum(int(v) for v in lab[k * stride:k * stride + WINDOW])
            out.append((rho, k * stride, ones))
            k += 1
    return out


@pytest.mark.parametrize("stride", STRIDES)
def test_tables_against_a_plain_loop(stride):
    reads = _reads()
    labels, offsets = _layout(reads)
    hit, miss = tiled_tables(labels, offsets, stride)
    windows = _brute(reads, stride)
    want_hit = [int(offsets[r]) + s for r, s, ones in windows if ones > 0]
    want_miss = [int(offsets[r]) + s for r, s, ones in windows if ones == 0]
    assert hit.dtype == miss.dtype == np.int64 and hit.tolist() == want_hit and miss.tolist() == want_miss
    assert want_hit and want_miss
    # no window straddles two reads, none is padded, a read shorter than 35 samples contributes nothing
    for start in hit.tolist() + miss.tolist():
        rho = int(np.searchsorted(offsets, start, side="right")) - 1
        assert start + WINDOW <= offsets[rho + 1] and (start - offsets[rho]) % stride == 0
    short = [r for r, lab in enumerate(reads) if lab.size < WINDOW]
    assert short and not any(r in short for r, _, _ in windows)
    # the pair of reads at the end: the last window of the first holds its run, none starts inside it and reaches the second
    a, b = int(offsets[-3]), int(offsets[-2])
    assert not any(a <= s < b and s + WINDOW > b for s in hit.tolist() + miss.tolist())


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("rule", [None, 0, 3, "hits"])
def test_miss_quota_is_centre_tables_rule(rule, stride):
    """Per read: q = m, min(m, it) or min(m, hits); candidate j of the read's m misses is kept iff q == m or
    keyed_permutation(j, m, key) < q with centre_tables' key -- stated here from the docstring, not through the module's helper."""
    reads = _reads()
    labels, offsets = _layout(reads)
    seed = 0x1234ABCD
    hit, miss = tiled_tables(labels, offsets, stride, rule, seed)
    all_hit, all_miss = tiled_tables(labels, offsets, stride)
    assert np.array_equal(hit, all_hit)
    want = []
    for rho in range(len(reads)):
        lo, hi = offsets[rho], offsets[rho + 1]
        cand = all_miss[(all_miss >= lo) & (all_miss < hi)]
        n_hit = int(((all_hit >= lo) & (all_hit < hi)).sum())
        m = cand.size
        q = m if rule is None else min(m, n_hit) if rule == "hits" else min(m, rule)
        if q < m:
            with np.errstate(over="ignore"):
                key = ddb.fmix32(np.uint32(seed) ^ ddb.fmix32(np.uint32(((rho + 1) * 0x9E3779B9) & 0xFFFFFFFF)))
            cand = cand[ddb.keyed_permutation(np.arange(m, dtype=np.uint32), m, key) < q]
        assert cand.size == q
        want += cand.tolist()
    assert miss.tolist() == want
    # the same rule keeps the same candidates in centre_tables: an all-zero read of 105 samples has the same 71 candidates at stride 1
    zeros, off = np.zeros(105, np.uint8), np.array([0, 105])
    if rule != "hits" and stride == 1:
        assert np.array_equal(tiled_tables(zeros, off, 1, rule, seed)[1], ddb.centre_tables(zeros, off, 1, rule, seed)[1])


def test_refusals():
    labels, offsets = _layout(_reads())
    for stride in (0, -1, 1.5, "35", None, True):
        with pytest.raises(ValueError):
            tiled_tables(labels, offsets, stride)
    for rule in (-1, 1.5, "positives", "all", True):
        with pytest.raises(ValueError):
            tiled_tables(labels, offsets, 35, rule)
    with pytest.raises(ValueError):
        tiled_tables(labels.astype(np.int64), offsets)
    with pytest.raises(ValueError):
        tiled_tables(labels, offsets[:-1])
    with pytest.raises(ValueError):
        DeviceTiledDb(np.zeros((2, 35)), np.zeros((2, 34), np.uint8), np.zeros((2, 35)), 0)
    with pytest.raises(ValueError):
        DeviceTiledDb(np.zeros((2, 35)), np.full((2, 35), 2, np.uint8), np.zeros((2, 35)), 0)


# ---------------------------------------------------------------------------------------------------- the sampler's contract
def _signals(reads, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1.2, size=r.size).astype(np.float32) for r in reads]


def _db(seed=11, stride=7, rule=None):
    reads = _reads()
    return DeviceTiledDb.from_arrays(_signals(reads), reads, seed, stride, rule), reads


def test_pools_hold_the_windows_of_the_tables():
    db, reads = _db()
    labels, offsets = _layout(reads)
    signal = np.concatenate(_signals(reads))
    hit, miss = tiled_tables(labels, offsets, 7, None, 11)
    span = np.arange(WINDOW)
    assert db.pos.dtype == db.neg.dtype == np.float32 and db.pos_labels.dtype == np.uint8
    assert (db.nb_pos, db.nb_neg) == (hit.size, miss.size) == (db.pos.shape[0], db.neg.shape[0])
    assert np.array_equal(db.pos, signal[hit[:, None] + span]) and np.array_equal(db.neg, signal[miss[:, None] + span])
    assert np.array_equal(db.pos_labels, labels[hit[:, None] + span]) and db.pos_labels.sum(1).min() >= 1
    mixed = (db.pos_labels.sum(1) < WINDOW).sum()
    assert 0 < mixed < db.nb_pos                                   # windows with a border inside AND all-ones windows


@pytest.mark.parametrize("size,ratio", [(32, 2), (33, 2), (7, 3), (6, 7), (5, 1)])
def test_contract(size, ratio):
    db, _ = _db()
    for d in (0, 1, 2 ** 32 - 1, 2 ** 32):
        x, y = db.gather(d, size, ratio)
        is_pos, row = db.batch_indices(d, size, ratio)
        assert x.dtype == np.float32 and x.shape == (size, WINDOW) and y.dtype == np.uint8 and y.shape == (size, WINDOW)
        assert int(is_pos.sum()) == size // ratio
        assert len(set(row[is_pos].tolist())) == size // ratio and len(set(row[~is_pos].tolist())) == size - size // ratio
        assert np.array_equal(x[is_pos], db.pos[row[is_pos]]) and np.array_equal(x[~is_pos], db.neg[row[~is_pos]])
        assert np.array_equal(y[is_pos], db.pos_labels[row[is_pos]]) and not y[~is_pos].any()


def test_the_draw_key_wraps_at_32_bits():
    """The draw number enters the key modulo 2^32 (as in the kernel): draw 2^32 is draw 0 again, 2^32 - 1 is not."""
    db, _ = _db()
    assert np.array_equal(db.gather(2 ** 32, 32)[0], db.gather(0, 32)[0])
    assert not np.array_equal(db.gather(2 ** 32 - 1, 32)[0], db.gather(0, 32)[0])


def test_get_training_set_skip_and_last_batch():
    for first in (0, 1, 2 ** 32 - 1):
        db, _ = _db()
        db.skip(first)
        with pytest.raises(RuntimeError):
            db.last_batch()
        for d in (first, first + 1):
            x, y, n_one = db.get_training_set(32)
            want_x, want_y = db.gather(d, 32)
            assert isinstance(x, tuple) and isinstance(y, tuple) and len(x) == len(y) == 32 and isinstance(y[0], list) and len(y[0]) == WINDOW
            assert np.array_equal(np.stack(x), want_x) and np.array_equal(np.asarray(y), want_y)
            assert n_one == int(want_y.sum()) == int(np.asarray(y).sum()) and db.draw == d + 1
            lx, ly = db.last_batch()
            assert np.array_equal(lx, want_x) and np.array_equal(ly, want_y) and ly.dtype == np.int64
    with pytest.raises(ValueError):
        db.skip(-1)


def test_a_pool_smaller_than_its_share_is_refused():
    db, _ = _db()
    with pytest.raises(ValueError):
        db.gather(0, 2 * db.nb_pos + 2, 2)
    with pytest.raises(ValueError):
        db.get_training_set(db.nb_neg + 1, db.nb_neg + 2)         # no hit, one miss too many
    assert db.draw == 0
    with pytest.raises(ValueError):
        db.gather(0, 0, 2)


def test_uniform_twin_draws_what_a_device_example_db_draws():
    rng = np.random.default_rng(5)
    pos, neg = rng.normal(size=(40, WINDOW)).astype(np.float32), rng.normal(size=(70, WINDOW)).astype(np.float32)
    tiled, old = DeviceTiledDb(pos, np.ones((40, WINDOW), np.uint8), neg, 99), DeviceExampleDb(pos, neg, 99)
    for d in (0, 1, 7, 2 ** 32 - 1, 2 ** 32):
        (x, y), (want_x, is_pos) = tiled.gather(d, 48), old.gather(d, 48)
        assert np.array_equal(x, want_x) and np.array_equal(y, np.repeat(is_pos.astype(np.uint8)[:, None], WINDOW, 1))
    a, b = tiled.get_training_set(48), old.get_training_set(48)
    assert np.array_equal(np.stack(a[0]), np.stack(b[0])) and a[1] == b[1] and a[2] == b[2]


def test_synthetic_sizes():
    """491 hits (210 of them all-ones, 281 mixed) and 4077 misses over the eight synthetic reads at stride 35; 491 misses under
    "hits" -- enough for a batch of 256 at ratio 2 either way."""
    db = ddb.synthetic_device_tiled_db()
    assert db.nb_pos >= 128 and db.nb_neg >= 128
    assert (db.nb_pos, db.nb_neg) == (491, 4077)
    full = int((db.pos_labels.sum(1) == WINDOW).sum())
    assert (full, db.nb_pos - full) == (210, 281)
    hits = ddb.synthetic_device_tiled_db(miss_per_read="hits")
    assert (hits.nb_pos, hits.nb_neg) == (491, 491) and np.array_equal(hits.pos, db.pos)
    x, y = hits.gather(0, 256)
    assert x.shape == (256, WINDOW) and 0 < y.sum() < 128 * WINDOW


def test_from_npz_and_from_source(tmp_path):
    from catfish_amd.labelling import LabelSource
    paths, raws, labs = [], [], []
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(3000 + i, seed=70 + i)
        path = str(tmp_path / ("r%d.npz" % i))
        np.savez(path, raw=raw, base_labels=lab)
        paths.append(path); raws.append(raw); labs.append(lab)
    want = DeviceTiledDb.from_arrays(raws, labs, 4, 35, "hits")
    for got in (DeviceTiledDb.from_npz(paths, 4, 35, "hits"), DeviceTiledDb.from_source(paths, LabelSource(), 4, 35, "hits", device="cpu")):
        assert np.array_equal(got.pos, want.pos) and np.array_equal(got.pos_labels, want.pos_labels) and np.array_equal(got.neg, want.neg)
        assert got.seed == 4


# ---------------------------------------------------------------------------------------------------- the CPU trainer
def test_cpu_trainer_steps_on_the_gathered_batches():
    """Trainer(device="cpu").train_steps runs get_training_set + train_step: three losses bit-equal to train_step on the same three
    gathered batches, per-sample labels included (a batch with every y set to its window's majority gives other losses)."""
    pytest.importorskip("torch")
    from catfish_amd.training import Trainer
    from oracle import catfish_oracle as oracle
    w = oracle.random_weights(seed=8, layer_size=16, n_layers=1, layer_size_res=16, n_layers_res=1)
    mk = lambda: Trainer(w, 1, 1, "Adam", 1e-3, 1.0, device="cpu", seed=2)      # noqa: E731
    db = ddb.synthetic_device_tiled_db(n_reads=2, read_len=6000, seed=1, miss_per_read="hits")
    twin = ddb.synthetic_device_tiled_db(n_reads=2, read_len=6000, seed=1, miss_per_read="hits")
    got = mk().train_steps(db, 3, 32)
    batches = [twin.gather(d, 32) for d in range(3)]
    assert any(0 < row.sum() < WINDOW for _, y in batches for row in y)
    host = mk()
    want = np.array([host.train_step(x, y.astype(np.float32)) for x, y in batches], np.float32)
    assert db.draw == 3 and got.dtype == np.float32 and np.array_equal(got, want)
    uniform = mk()
    other = np.array([uniform.train_step(x, np.repeat((y.sum(1) > 0).astype(np.float32)[:, None], WINDOW, 1)) for x, y in batches], np.float32)
    assert not np.array_equal(other, want)
    lx, ly = db.last_batch()
    assert np.array_equal(lx, batches[2][0]) and np.array_equal(ly, batches[2][1])
    assert not hasattr(db, "device_pools") and db._dev is None                     # a host database: nothing of it goes to a card


# ---------------------------------------------------------------------------------------------------- the environment
def test_environment_of_main(monkeypatch, tmp_path):
    for name in ("CATFISH_TILED_STRIDE", "CATFISH_TILED_MISSES", "CATFISH_LABEL_KMER", "CATFISH_LABEL_MOVES"):
        monkeypatch.delenv(name, raising=False)
    assert tv.tiled_options_from_env() == (35, "hits")
    for text, want in (("all", None), ("hits", "hits"), ("0", 0), ("12", 12)):
        monkeypatch.setenv("CATFISH_TILED_MISSES", text)
        assert tv.tiled_options_from_env() == (35, want)
    for text in ("-1", "positives", "1.5", ""):
        monkeypatch.setenv("CATFISH_TILED_MISSES", text)
        with pytest.raises(ValueError):
            tv.tiled_options_from_env()
    monkeypatch.setenv("CATFISH_TILED_MISSES", "all")
    for text, want in (("1", 1), ("7", 7), ("36", 36)):
        monkeypatch.setenv("CATFISH_TILED_STRIDE", text)
        assert tv.tiled_options_from_env() == (want, None)
    for text in ("0", "-35", "x", "3.5", ""):
        monkeypatch.setenv("CATFISH_TILED_STRIDE", text)
        with pytest.raises(ValueError):
            tv.tiled_options_from_env()
    raw, lab = tv.synthetic_labelled_read(3000, seed=9)
    path = str(tmp_path / "a.npz")
    np.savez(path, raw=raw, base_labels=lab)
    monkeypatch.setenv("CATFISH_TILED_STRIDE", "7")
    monkeypatch.setenv("CATFISH_TILED_MISSES", "5")
    got, want = tv.device_tiled_db_from_env([path]), DeviceTiledDb.from_arrays([raw], [lab], 0, 7, 5)
    assert isinstance(got, DeviceTiledDb) and got.nb_neg == 5 and np.array_equal(got.pos, want.pos) and np.array_equal(got.neg, want.neg)
    assert "CATFISH_DEVICE_DB=tiled" in tv.main.__doc__ and "CATFISH_TILED_STRIDE" in tv.main.__doc__ and "CATFISH_TILED_MISSES" in tv.main.__doc__


# ---------------------------------------------------------------------------------------------------- the GPU module's constants
def test_bounds_of_the_gpu_module_follow_from_its_profile():
    """Each bound of tests/test_tiled_db_gpu.py is at most 4 x the largest float32-torch error that profiles/tiled_db_parity.jsonl
    records for the quantity, at most the older bound, and not so far below (rounded down to three digits) that it is a different
    number -- the check tests/test_train_draws_host.py makes for its own module."""
    import test_tiled_db_gpu as m
    want = m.bounds_from_profile()
    assert sorted(want) == sorted(m.BOUNDS) == sorted(m.OLDER_BOUNDS)
    for k, b in m.BOUNDS.items():
        assert 0.99 * want[k] <= b <= want[k], (k, b, want[k])
