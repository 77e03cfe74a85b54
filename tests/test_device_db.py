"""DeviceExampleDb on the host: the stateless balanced sampler (catfish_amd/device_db.py) that cf_sample_batch reproduces on the
card, its drop-in surface for the per-step loop, and train_and_validate's choice between the two loops.  No GPU needed."""
import os

import numpy as np
import pytest

from catfish_amd import device_db as ddb, train_validate as tv
from catfish_amd.device_db import DeviceExampleDb

SIZES = (256, 255, 64, 4096)
RATIOS = (2, 3)


def pools(n_pos, n_neg, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n_pos, 35)).astype(np.float32), rng.normal(size=(n_neg, 35)).astype(np.float32)


def pool_shapes(size, ratio):
    """(n_pos, n_neg): exactly the needed size, a power of two, a power of two plus one, and a large odd pool."""
    k_pos = size // ratio
    k_neg = size - k_pos
    p2 = lambda k: 1 << (k - 1).bit_length()              # noqa: E731
    return [(k_pos, k_neg), (p2(k_pos), p2(k_neg)), (p2(k_pos) + 1, p2(k_neg) + 1), (7188, 32000)]


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("size", SIZES)
def test_draw_keeps_the_reference_samplers_contract(size, ratio):
    """ExampleDb.get_training_set: size // ratio distinct positives, the rest distinct negatives, every row in range."""
    k_pos = size // ratio
    for n_pos, n_neg in pool_shapes(size, ratio):
        db = DeviceExampleDb(*pools(n_pos, n_neg), seed=11)
        for d in (0, 1, 2, 77, 2 ** 32 + 5):
            is_pos, row = db.batch_indices(d, size, ratio)
            assert is_pos.shape == row.shape == (size,) and is_pos.dtype == bool and row.dtype == np.int64
            assert int(is_pos.sum()) == k_pos
            rp, rn = row[is_pos], row[~is_pos]
            assert len(set(rp.tolist())) == k_pos and len(set(rn.tolist())) == size - k_pos
            assert rp.min(initial=0) >= 0 and rp.max(initial=0) < n_pos and rn.min() >= 0 and rn.max() < n_neg


def test_short_pool_and_wrong_window_raise():
    pos, neg = pools(127, 128)
    with pytest.raises(ValueError):
        DeviceExampleDb(pos, neg, seed=0).batch_indices(0, 256, 2)
    with pytest.raises(ValueError):
        DeviceExampleDb(neg, pos, seed=0).get_training_set(256)
    with pytest.raises(ValueError):
        DeviceExampleDb(pos[:, :34], neg, seed=0)
    with pytest.raises(ValueError):
        DeviceExampleDb([np.zeros(35), np.zeros(36)], neg, seed=0)


def test_keyed_permutation_is_a_bijection():
    for n in (1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000):
        for key in (0, 1, 0xDEADBEEF):
            got = ddb.keyed_permutation(np.arange(n, dtype=np.uint32), n, np.uint32(key))
            assert sorted(got.tolist()) == list(range(n))


def test_determinism_and_drop_in_surface():
    pos, neg = pools(300, 500, seed=3)
    a, b, c = DeviceExampleDb(pos, neg, seed=5), DeviceExampleDb(pos, neg, seed=5), DeviceExampleDb(pos, neg, seed=6)
    for d in range(4):
        ia, ra = a.batch_indices(d, 64)
        ib, rb = b.batch_indices(d, 64)
        assert np.array_equal(ia, ib) and np.array_equal(ra, rb)
        ic, rc = c.batch_indices(d, 64)
        assert not (np.array_equal(ia, ic) and np.array_equal(ra, rc))           # another seed
        i1, r1 = a.batch_indices(d + 1, 64)
        assert not (np.array_equal(ia, i1) and np.array_equal(ra, r1))           # another draw
    # the per-step surface: today's types, the windows batch_indices names, the counter moves by one per batch
    for d in range(3):
        assert a.draw == d
        x_out, y_out, pos_count = a.get_training_set(64, ratio=2)
        is_pos, row = b.batch_indices(d, 64, 2)
        assert isinstance(x_out, tuple) and isinstance(y_out, tuple) and len(x_out) == len(y_out) == 64
        assert all(isinstance(y, list) and len(y) == 35 for y in y_out)
        assert pos_count == (64 // 2) * 35 == sum(y.count(1) for y in y_out)
        for j in range(64):
            want = pos[row[j]] if is_pos[j] else neg[row[j]]
            assert x_out[j].dtype == np.float32 and np.array_equal(x_out[j], want)
            assert y_out[j] == [int(is_pos[j])] * 35
        lx, ly = a.last_batch()
        assert np.array_equal(lx, np.stack(x_out)) and np.array_equal(ly, np.asarray(y_out))
    a.skip(4)
    assert a.draw == 7
    x7, _, _ = a.get_training_set(64)
    assert np.array_equal(np.stack(x7), b.gather(7, 64)[0])
    x3, y3, n3 = a.get_training_set(255, ratio=3)
    assert n3 == 85 * 35 and len(x3) == 255
    # the same pools through the WindowExampleDb constructor; train_validate's reshape_input takes the result as it is
    w = DeviceExampleDb.from_window_db(tv.WindowExampleDb(list(pos), list(neg), seed=1), seed=5)
    xs, ys, _ = w.get_training_set(64)
    assert np.array_equal(np.stack(xs), b.gather(0, 64)[0])
    assert tv.reshape_input(xs, 35, 1).shape == (64, 35, 1) and tv.reshape_input(ys, 35, 1).shape == (64, 35, 1)


def test_constructors_share_the_window_selection():
    syn = ddb.synthetic_device_db(n_reads=2, read_len=6000, seed=2)
    ref = tv.synthetic_example_db(n_reads=2, read_len=6000, seed=2)
    assert syn.nb_pos == ref.nb_pos and syn.nb_neg == ref.nb_neg and syn.seed == 2
    assert np.array_equal(syn.pos, np.asarray(ref.pos, dtype=np.float32))
    assert np.array_equal(syn.neg, np.asarray(ref.neg, dtype=np.float32))
    assert syn._dev is None                                                    # host-only until a trainer asks for the pools


def test_npz_constructor(tmp_path):
    files = []
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(5000, seed=30 + i)
        files.append(str(tmp_path / ("r%d.npz" % i)))
        np.savez(files[-1], raw=raw, base_labels=lab)
    got = ddb.device_db_from_npz(files, seed=4)
    ref = tv.example_db_from_npz(files, seed=4)
    assert np.array_equal(got.pos, np.asarray(ref.pos, dtype=np.float32))
    assert np.array_equal(got.neg, np.asarray(ref.neg, dtype=np.float32))
    with pytest.raises(ValueError):
        ddb.device_db_from_npz(files, width=33)                                # 34-sample windows


def test_uniformity_of_the_sampler():
    """20 000 draws of 256 from pools of 7 188 / 32 000.  For a uniform sampler each positive is picked with p = 128 / 7188 per
    draw, each negative with p = 128 / 32000 and each slot is positive with p = 1 / 2; the standardised counts must stay within
    |z| <= 6 (a false alarm of the order of 1e-4 over the 39 444 counts) and their mean z^2 within [0.9, 1.1].  The bounds are
    conditions set before the sampler was written, not measurements of it; the seed is fixed, so the test is deterministic."""
    draws, size, n_pos, n_neg = 20000, 256, 7188, 32000
    c_pos, c_neg, c_slot = np.zeros(n_pos), np.zeros(n_neg), np.zeros(size)
    for lo in range(0, draws, 2000):
        is_pos, row = ddb.draw_indices(12345, np.arange(lo, lo + 2000), size, 2, n_pos, n_neg)
        assert (is_pos.sum(1) == 128).all()
        srt = np.sort(np.where(is_pos, row, row + n_pos), axis=1)              # distinct rows in every batch
        assert (np.diff(srt, axis=1) > 0).all()
        c_pos += np.bincount(row[is_pos], minlength=n_pos)
        c_neg += np.bincount(row[~is_pos], minlength=n_neg)
        c_slot += is_pos.sum(0)
    z = lambda c, p: (c - draws * p) / np.sqrt(draws * p * (1 - p))           # noqa: E731
    for name, zz in (("positives", z(c_pos, 128 / n_pos)), ("negatives", z(c_neg, 128 / n_neg)), ("slots", z(c_slot, 0.5))):
        print("%s: max |z| %.3f, mean z^2 %.4f" % (name, np.abs(zz).max(), (zz ** 2).mean()))
        assert np.abs(zz).max() <= 6.0, name
        assert 0.9 <= (zz ** 2).mean() <= 1.1, name


# ---------------------------------------------------------------- train_and_validate: which loop runs
class _StepNetwork(object):
    """The surface train_and_validate uses, without a model behind it."""
    window, n_inputs, n_outputs, model_type, batch_size = 35, 1, 1, "ResNet-RNN", 16

    def __init__(self):
        self.tp = self.fp = self.tn = self.fn = 0
        self.batches, self.saved = [], []

    def train_network(self, x, y, step):
        self.batches.append((np.array(x), np.array(y), step))

    def save_network_to_model_path(self, step):
        self.saved.append(step)

    def evaluate(self, x, y):
        return float(np.mean(np.asarray(y))), float(np.mean(np.asarray(x, dtype=np.float64)))

    def score_windows(self, windows):
        z = np.asarray(windows, dtype=np.float32).reshape(-1)
        return (1.0 / (1.0 + np.exp(-z))).astype(np.float32), z


class _FedNetwork(_StepNetwork):
    def __init__(self):
        _StepNetwork.__init__(self)
        self.calls = []

    def train_network_steps(self, db, n_steps):
        self.calls.append((db.draw, n_steps))
        for _ in range(n_steps):
            db.get_training_set(self.batch_size)


def _run(network, db, tmp_path, name, checkpoint_every):
    raw, lab = tv.synthetic_labelled_read(1400, seed=9)
    np.savez(tmp_path / "val.npz", raw=raw, base_labels=lab)
    tv.train_and_validate(network, db, 7 * 16 + 5, [str(tmp_path / "val.npz")], 700, str(tmp_path / name), 0, 856,
                          checkpoint_every=checkpoint_every)
    return open(str(tmp_path / name) + ".txt").read(), open(name + ".txt").read()


def test_train_and_validate_keeps_todays_loop_without_train_network_steps(tmp_path, monkeypatch):
    """A DeviceExampleDb with a network that has no train_network_steps: the per-step loop, batch by batch, and its report --
    the same bytes a host database of the same batches gives."""
    monkeypatch.chdir(tmp_path)
    pos, neg = pools(40, 60, seed=8)

    class Replay(object):                                  # a plain database (not a DeviceExampleDb) handing out the same batches
        def __init__(self):
            self.db = DeviceExampleDb(pos, neg, seed=3)

        def get_training_set(self, size, ratio=2):
            return self.db.get_training_set(size, ratio)

    a, b = _StepNetwork(), _StepNetwork()
    got = _run(a, DeviceExampleDb(pos, neg, seed=3), tmp_path, "fed", 3)
    want = _run(b, Replay(), tmp_path, "host", 3)
    assert got == want
    assert "Training on 112 examples in 7 batches" in got[0] and "Training set had 50.00% HPs" in got[0]
    assert a.saved == b.saved == [3, 6, 7] and [s for _, _, s in a.batches] == list(range(1, 8))
    twin = DeviceExampleDb(pos, neg, seed=3)
    for x, y, _ in a.batches:
        wx, wy, _ = twin.get_training_set(16)
        assert x.shape == (16, 35, 1) and np.array_equal(x[:, :, 0], np.stack(wx)) and np.array_equal(y[:, :, 0], np.asarray(wy))


def test_train_and_validate_runs_the_steps_between_checkpoints_as_one_call(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pos, neg = pools(40, 60, seed=8)
    fed, host = _FedNetwork(), _StepNetwork()
    got = _run(fed, DeviceExampleDb(pos, neg, seed=3), tmp_path, "fed", 3)
    want = _run(host, DeviceExampleDb(pos, neg, seed=3), tmp_path, "host", 3)
    assert fed.calls == [(0, 3), (3, 3), (6, 1)] and fed.batches == [] and fed.saved == [3, 6, 7]
    assert got == want                                     # report text, checkpoint steps, HP share: unchanged
