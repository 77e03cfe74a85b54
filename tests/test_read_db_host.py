"""DeviceReadDb: the window selection (device_db.centre_tables) against a brute-force restatement of TrainingRead.get_pos / get_neg,
the drop-in surface against today's pools, and which loop train_and_validate runs with it.  No GPU needed."""
import numpy as np
import pytest

from catfish_amd import device_db as ddb, train_validate as tv
from catfish_amd.device_db import DeviceExampleDb, DeviceReadDb

LESSENS = (1, 2, 3)
NEG_RULES = (None, 0, 5, 10 ** 9, "positives")
STRIDE = 1024                                          # long reads: runs placed around every multiple of this


def _runs(*pairs):
    """(value, length), ... -> uint8 labels."""
    return np.concatenate([np.full(n, v, dtype=np.uint8) for v, n in pairs] + [np.zeros(0, np.uint8)])


def case_reads():
    """About 40 short reads: every edge of the selection rule at least once."""
    reads = []
    for n in (0, 34, 35, 36):                              # too short, and the shortest reads that hold a window
        reads += [_runs((1, n)), _runs((0, n))]
    reads += [_runs((0, 30), (1, 34), (0, 30)),            # a run of exactly 34 ones: no positive
              _runs((0, 30), (1, 35), (0, 30)),            # exactly 35: one
              _runs((1, 30), (0, 34), (1, 30)),            # the same for the candidates
              _runs((1, 30), (0, 35), (1, 30)),
              _runs((1, 50), (0, 60), (1, 50)),            # runs touching both ends of the read
              _runs((0, 50), (1, 60), (0, 50)),
              _runs((0, 90), (1, 20)), _runs((1, 20), (0, 90)),      # read r ends in 20 ones, read r + 1 begins with 20: no window across
              _runs((1, 90), (0, 20)), _runs((0, 20), (1, 90)),      # the same in zeros
              _runs((0, 600)), _runs((1, 300)),            # many candidates and no positive; many positives and no candidate
              _runs((1, 36), (0, 400)), _runs((1, 40), (0, 36), (1, 40), (0, 36))]
    rng = np.random.default_rng(5)
    while len(reads) < 40:                                 # runs of 1 .. 90 samples, either label first
        pairs, v = [], int(rng.integers(2))
        for _ in range(int(rng.integers(3, 14))):
            pairs.append((v, int(rng.integers(1, 91))))
            v = 1 - v
        reads.append(_runs(*pairs))
    return reads


def chunk_edge_reads(deltas=range(-17, 18)):
    """One read of 3 * STRIDE + 7 samples per delta: at every multiple E of STRIDE a run of 40 ones ends and a run of 40 zeros
    begins at E + delta; everything else alternates 1, 0 (label-1 centres that are never positives, so the number k of a
    positive counts hundreds of centres before it)."""
    reads = []
    for delta in deltas:
        lab = (np.arange(3 * STRIDE + 7) % 2 == 0).astype(np.uint8)
        for edge in (STRIDE, 2 * STRIDE, 3 * STRIDE):
            lab[edge + delta - 40:edge + delta] = 1
            lab[edge + delta:edge + delta + 40] = 0
        reads.append(lab)
    return reads


def pack(reads, seed=0):
    """-> (signal float32 [total], labels uint8 [total], offsets int64 [R + 1])."""
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in reads]))).astype(np.int64)
    labels = np.concatenate(list(reads) + [np.zeros(0, np.uint8)]).astype(np.uint8)
    signal = np.random.default_rng(seed).normal(size=labels.size).astype(np.float32)
    return signal, labels, offsets


def brute_force(labels, offsets, lessen, neg_per_read, seed):
    """The rule in plain loops over every centre: TrainingRead.get_pos (every lessen-th label-1 centre, kept when its 35 labels are
    all 1), the candidates (35 labels all 0), the quota, and the keyed subset.  -> (pos_start, neg_start, per-read (candidates, q)).
    The read key is restated here; the bijection itself is ``ddb.keyed_permutation``, the function centre_tables uses -- that it IS
    a bijection and what the kernels compute is tests/test_device_db.py's and tests/test_device_db_gpu.py's matter, not this file's."""
    pos, neg, per_read = [], [], []
    for rho in range(len(offsets) - 1):
        o = int(offsets[rho])
        lab = labels[o:int(offsets[rho + 1])].tolist()
        k, hits, cand = 0, [], []
        for c in range(17, len(lab) - 17):
            window = lab[c - 17:c + 18]
            if lab[c] == 1:
                if k % lessen == 0 and all(v == 1 for v in window):
                    hits.append(o + c - 17)
                k += 1
            if all(v == 0 for v in window):
                cand.append(o + c - 17)
        m = len(cand)
        q = m if neg_per_read is None else min(m, len(hits)) if neg_per_read == "positives" else min(m, neg_per_read)
        chosen = cand
        if q < m:
            key = ddb.fmix32(np.uint32(seed) ^ ddb.fmix32(np.uint32(((rho + 1) * 0x9E3779B9) & 0xFFFFFFFF)))
            image = ddb.keyed_permutation(np.arange(m, dtype=np.uint32), m, key).tolist()
            chosen = [cand[j] for j in range(m) if image[j] < q]
        pos += hits
        neg += chosen
        per_read.append((cand, q))
    return np.array(pos, dtype=np.int64), np.array(neg, dtype=np.int64), per_read


@pytest.mark.parametrize("lessen", LESSENS)
def test_centre_tables_against_the_brute_force_loop(lessen):
    _, labels, offsets = pack(case_reads())
    for rule in NEG_RULES:
        pos, neg = ddb.centre_tables(labels, offsets, lessen, rule, seed=9)
        want_pos, want_neg, _ = brute_force(labels, offsets, lessen, rule, 9)
        assert pos.dtype == neg.dtype == np.int64
        assert np.array_equal(pos, want_pos), (lessen, rule)
        assert np.array_equal(neg, want_neg), (lessen, rule)
    assert len(ddb.centre_tables(labels, offsets, 1)[0]) > len(ddb.centre_tables(labels, offsets, 3)[0]) > 0


def test_the_named_edges_of_the_rule():
    reads = case_reads()
    for i, (n_pos, n_neg) in {0: (0, 0), 1: (0, 0), 2: (0, 0), 3: (0, 0), 4: (1, 0), 5: (0, 1), 6: (2, 0), 7: (0, 2),
                              8: (0, 0), 9: (1, 0), 10: (0, 0), 11: (0, 1)}.items():
        pos, neg = ddb.centre_tables(reads[i], np.array([0, len(reads[i])]))
        assert (len(pos), len(neg)) == (n_pos, n_neg), i
    # read 14 ends in 20 ones and read 15 begins with 20: 40 ones in a row in the concatenation, and no window in either read
    signal, labels, offsets = pack(reads[14:16])
    assert labels[offsets[1] - 20:offsets[1] + 20].all()
    pos, neg = ddb.centre_tables(labels, offsets)
    assert len(pos) == 0 and all(s + 35 <= offsets[1] or s >= offsets[1] for s in neg.tolist())
    # every window lies inside one read
    _, labels, offsets = pack(reads)
    for table in ddb.centre_tables(labels, offsets):
        read = np.searchsorted(offsets, table, side="right") - 1
        assert np.all(table + 35 <= offsets[read + 1])


@pytest.mark.parametrize("deltas", [(-17, 0), (1, 17)])
def test_chunk_edge_reads_against_the_brute_force_loop(deltas):
    """Long reads (three times 1024 samples and seven) whose label-1 numbering runs far: the rule on them is the plain loop's."""
    _, labels, offsets = pack(chunk_edge_reads(deltas))
    for lessen, rule in ((1, None), (3, "positives")):
        pos, neg = ddb.centre_tables(labels, offsets, lessen, rule, seed=2)
        want_pos, want_neg, _ = brute_force(labels, offsets, lessen, rule, 2)
        assert np.array_equal(pos, want_pos) and np.array_equal(neg, want_neg) and len(pos) and len(neg)


def test_negatives_are_a_keyed_subset_of_the_candidates():
    _, labels, offsets = pack(case_reads())
    for rule in (5, "positives"):
        _, neg_a, per_read = brute_force(labels, offsets, 1, rule, 1)
        neg_a2 = ddb.centre_tables(labels, offsets, 1, rule, seed=1)[1]
        neg_b = ddb.centre_tables(labels, offsets, 1, rule, seed=2)[1]
        assert np.array_equal(neg_a2, ddb.centre_tables(labels, offsets, 1, rule, seed=1)[1])       # the same seed: the same subset
        assert np.array_equal(neg_a, neg_a2)
        assert len(neg_a) == len(neg_b) and not np.array_equal(neg_a, neg_b)                        # another seed: another subset
        read_of = np.searchsorted(offsets, neg_a2, side="right") - 1
        for rho, (cand, q) in enumerate(per_read):
            mine = neg_a2[read_of == rho]
            assert len(mine) == q and set(mine.tolist()) <= set(cand) and np.all(np.diff(mine) > 0), rho
        assert any(0 < q < len(cand) for cand, q in per_read)


def _twin_pools(db):
    """Today's pools from the same reads: windows_from_labelled_read with every negative, read by read."""
    pos, neg = [], []
    for a, b in zip(db.offsets[:-1].tolist(), db.offsets[1:].tolist()):
        p, n = tv.windows_from_labelled_read(db.signal[a:b], db.labels[a:b], 34, db.lessen, None)
        pos += p
        neg += n
    return DeviceExampleDb(pos, neg, seed=db.seed)


@pytest.mark.parametrize("lessen", LESSENS)
def test_gather_equals_todays_pools(lessen):
    signal, labels, offsets = pack(case_reads(), seed=3)
    db = DeviceReadDb(signal, labels, offsets, seed=11, lessen=lessen)
    twin = _twin_pools(db)
    assert (db.nb_pos, db.nb_neg) == (twin.nb_pos, twin.nb_neg) and db.nb_pos >= 32 and db.nb_neg >= 43
    assert np.array_equal(signal[db.pos_start[:, None] + np.arange(35)], twin.pos)
    for d in (0, 1, 77, 2 ** 32 - 1):
        for size in (1, 7, 64):
            for ratio in (2, 3):
                x, is_pos = db.gather(d, size, ratio)
                want_x, want_is_pos = twin.gather(d, size, ratio)
                assert x.dtype == np.float32 and x.shape == (size, 35)
                assert np.array_equal(x.view(np.uint32), want_x.view(np.uint32)) and np.array_equal(is_pos, want_is_pos)


def test_windows_from_labelled_read_is_the_brute_force_rule():
    """What makes the equivalence above a statement about the rule: on a 20 000-sample synthetic read today's selection with
    max_neg=None is the plain loop's positives and candidates."""
    raw, lab = tv.synthetic_labelled_read(20000, seed=4)
    lab8 = lab.astype(np.uint8)
    for lessen in LESSENS:
        pos, neg = tv.windows_from_labelled_read(raw, lab, 34, lessen, None)
        want_pos, want_neg, _ = brute_force(lab8, np.array([0, len(lab8)]), lessen, None, 0)
        assert np.array_equal(np.array(pos), raw[want_pos[:, None] + np.arange(35)])
        assert np.array_equal(np.array(neg), raw[want_neg[:, None] + np.arange(35)])


def test_drop_in_surface_and_constructors(tmp_path):
    db = ddb.synthetic_device_read_db(n_reads=2, read_len=6000, seed=2)
    again = ddb.synthetic_device_read_db(n_reads=2, read_len=6000, seed=2)
    assert db.seed == 2 and db.draw == 0 and db._dev is None and db.signal.dtype == np.float32
    x_out, y_out, pos_count = db.get_training_set(64)
    want_x, want_is_pos = again.gather(0, 64)
    assert db.draw == 1 and isinstance(x_out, tuple) and len(x_out) == len(y_out) == 64 and pos_count == 32 * 35
    assert np.array_equal(np.stack(x_out), want_x) and [y[0] for y in y_out] == want_is_pos.astype(int).tolist()
    lx, ly = db.last_batch()
    assert np.array_equal(lx, want_x) and np.array_equal(ly, np.asarray(y_out))
    db.skip(3)
    assert db.draw == 4
    is_pos, row = db.batch_indices(4, 64)
    assert row[is_pos].max() < db.nb_pos and row[~is_pos].max() < db.nb_neg
    files = []
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(6000, seed=2000 + i)
        files.append(str(tmp_path / ("r%d.npz" % i)))
        np.savez(files[-1], raw=raw, base_labels=lab)
    from_files = DeviceReadDb.from_npz(files, seed=2)
    assert np.array_equal(from_files.signal, db.signal) and np.array_equal(from_files.labels, db.labels)
    assert np.array_equal(from_files.pos_start, db.pos_start) and np.array_equal(from_files.neg_start, db.neg_start)
    ref = DeviceReadDb.from_npz(files, seed=2, neg_per_read="positives")
    assert ref.nb_pos == db.nb_pos and 0 < ref.nb_neg <= ref.nb_pos < db.nb_neg


def test_refusals():
    signal, labels, offsets = pack([_runs((0, 60), (1, 60))])
    bad = labels.copy()
    bad[7] = 2
    with pytest.raises(ValueError):
        ddb.centre_tables(bad, offsets)
    with pytest.raises(ValueError):
        DeviceReadDb(signal, bad, offsets, seed=0)
    with pytest.raises(ValueError):
        ddb.centre_tables(labels, offsets, lessen=0)
    with pytest.raises(ValueError):
        ddb.centre_tables(labels, offsets, neg_per_read="some")
    with pytest.raises(ValueError):
        ddb.centre_tables(labels, np.array([0, 50]))
    db = DeviceReadDb(signal, labels, offsets, seed=0)                          # 26 positives, 26 negatives
    assert (db.nb_pos, db.nb_neg) == (26, 26)
    db.batch_indices(0, 52, 2)
    with pytest.raises(ValueError):
        db.batch_indices(0, 54, 2)                                              # 27 positives of 26
    with pytest.raises(ValueError):
        db.get_training_set(64)
    assert db.draw == 0
    with pytest.raises(ValueError):
        ddb._table_sizes_fit(2 ** 31, 5)
    assert not hasattr(db, "device_pools")                                       # a host database: nothing to keep on a card


def test_read_db_from_the_environment(tmp_path, monkeypatch):
    files = []
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(6000, seed=40 + i)
        files.append(str(tmp_path / ("r%d.npz" % i)))
        np.savez(files[-1], raw=raw, base_labels=lab)
    monkeypatch.delenv("CATFISH_DEVICE_NEG", raising=False)
    ref = tv.device_read_db_from_env(files)
    assert isinstance(ref, DeviceReadDb) and ref.neg_per_read == "positives" and 0 < ref.nb_neg <= ref.nb_pos
    monkeypatch.setenv("CATFISH_DEVICE_NEG", "all")
    assert tv.device_read_db_from_env(files).nb_neg > ref.nb_neg
    monkeypatch.setenv("CATFISH_DEVICE_NEG", "7")
    assert tv.device_read_db_from_env(files).nb_neg == 14
    monkeypatch.setenv("CATFISH_DEVICE_NEG", "some")
    with pytest.raises(ValueError):
        tv.device_read_db_from_env(files)


# ---------------------------------------------------------------- train_and_validate: which loop runs
class _Network(object):
    """The surface train_and_validate uses, without a model behind it; it HAS train_network_steps, which a DeviceExampleDb would get."""
    window, n_inputs, n_outputs, model_type, batch_size = 35, 1, 1, "ResNet-RNN", 16

    def __init__(self):
        self.tp = self.fp = self.tn = self.fn = 0
        self.batches, self.saved, self.calls = [], [], []

    def train_network(self, x, y, step):
        self.batches.append((np.array(x), np.array(y), step))

    def train_network_steps(self, db, n_steps):
        self.calls.append(n_steps)

    def save_network_to_model_path(self, step):
        self.saved.append(step)

    def evaluate(self, x, y):
        return float(np.mean(np.asarray(y))), float(np.mean(np.asarray(x, dtype=np.float64)))

    def score_windows(self, windows):
        z = np.asarray(windows, dtype=np.float32).reshape(-1)
        return (1.0 / (1.0 + np.exp(-z))).astype(np.float32), z


def test_train_and_validate_feeds_a_read_db_through_the_per_step_loop(tmp_path, monkeypatch):
    """A DeviceReadDb is a host database: seven batches of 16 go through get_training_set + train_network one by one (never
    train_network_steps), they are the sampler's draws 0 .. 6, and the report is written."""
    monkeypatch.chdir(tmp_path)
    raw, lab = tv.synthetic_labelled_read(1400, seed=9)
    np.savez(tmp_path / "val.npz", raw=raw, base_labels=lab)
    db = ddb.synthetic_device_read_db(n_reads=1, read_len=6000, seed=5, neg_per_read="positives")
    net = _Network()
    acc = tv.train_and_validate(net, db, 7 * 16 + 5, [str(tmp_path / "val.npz")], 700, str(tmp_path / "reads"), 0, 856, checkpoint_every=3)
    assert net.calls == [] and net.saved == [3, 6, 7] and [s for _, _, s in net.batches] == list(range(1, 8)) and db.draw == 7
    twin = ddb.synthetic_device_read_db(n_reads=1, read_len=6000, seed=5, neg_per_read="positives")
    for d, (x, y, _) in enumerate(net.batches):
        want_x, is_pos = twin.gather(d, 16)
        assert np.array_equal(x[:, :, 0], want_x) and np.array_equal(y[:, :, 0], np.repeat(is_pos.astype(np.int64)[:, None], 35, 1))
    report = open(str(tmp_path / "reads") + ".txt").read()
    assert "Training on 112 examples in 7 batches" in report and "Training set had 50.00% HPs" in report and np.isfinite(acc)
    assert "---NEXT ROUND OF VALIDATION---" in open("reads.txt").read()
