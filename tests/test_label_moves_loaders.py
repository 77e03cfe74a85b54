"""Move files through the loaders: ``DeviceValidationSet.from_moves`` / ``from_move_npz`` and ``DeviceReadDb.from_move_npz`` on the
host, the ``CATFISH_LABEL_MOVES`` parse and the loaders ``train_validate.main`` hands out; and on the card (``gpu``): the same set
labelled by ``cf_label_moves``, and one seeded validation round scored on both."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import labelling  # noqa: E402
from catfish_amd.labelling import MoveBatch  # noqa: E402
from test_label_moves_host import write_move_npz  # noqa: E402

_reads = []


def move_reads():
    """Six synthetic reads with their move tables (float32 seconds) and some raw signal behind the events, made once."""
    if not _reads:
        for i in range(6):
            raw, states, lengths, moves = labelling.synthetic_move_read(3000 + 35 * i, 90 + i)
            _reads.append((np.concatenate([raw, np.zeros(7 * i)]), states, lengths, moves))
    return _reads


def move_files(tmp_path):
    return [write_move_npz(tmp_path / ("v%d.npz" % i), raw, s, l, m, (10, 10)) for i, (raw, s, l, m) in enumerate(move_reads())]


def test_validation_set_and_read_db_from_moves_on_the_cpu(tmp_path):
    from catfish_amd.device_db import DeviceReadDb
    from catfish_amd.device_validation import DeviceValidationSet
    reads = move_reads()
    batch = MoveBatch.from_reads([(s, l, m, (10, 10), len(raw)) for raw, s, l, m in reads])
    labels, basemap = batch.label_host(base_map=True)
    got = DeviceValidationSet.from_moves([raw for raw, _s, _l, _m in reads], batch, device="cpu")
    want = DeviceValidationSet.from_arrays([raw[:n] for (raw, _s, _l, _m), n in zip(reads, batch.final)], np.split(labels, batch.sample_offsets[1:-1]))
    assert np.array_equal(got.labels, want.labels) and np.array_equal(got.signal, want.signal) and np.array_equal(got.offsets, want.offsets)
    assert np.array_equal(got.basemap, basemap) and np.array_equal(got.lengths, batch.final) and got.uploads == 0 and got.labels.any()
    with pytest.raises(ValueError, match="signals but"):
        DeviceValidationSet.from_moves([raw for raw, _s, _l, _m in reads][:4], batch, device="cpu")
    with pytest.raises(ValueError, match="raw signal has"):
        DeviceValidationSet.from_moves([raw[:100] for raw, _s, _l, _m in reads], batch, device="cpu")
    paths = move_files(tmp_path)
    from_files = DeviceValidationSet.from_move_npz(paths, device="cpu")
    assert np.array_equal(from_files.labels, got.labels) and np.array_equal(from_files.signal, got.signal) and np.array_equal(from_files.basemap, basemap)
    db = DeviceReadDb.from_move_npz(paths, seed=4, device="cpu")
    want_db = DeviceReadDb.from_arrays([raw[:n] for (raw, _s, _l, _m), n in zip(reads, batch.final)], np.split(labels, batch.sample_offsets[1:-1]), seed=4)
    assert np.array_equal(db.labels, want_db.labels) and np.array_equal(db.signal, want_db.signal) and np.array_equal(db.offsets, want_db.offsets)
    assert np.array_equal(db.pos_start, want_db.pos_start) and np.array_equal(db.neg_start, want_db.neg_start) and db.nb_pos > 0 and db.nb_neg > 0


def test_train_validate_reads_move_directories_when_asked(tmp_path, monkeypatch):
    """``CATFISH_LABEL_MOVES=1``: the loaders ``main`` hands out read move files and give what ``load_npz`` gives for the labelled
    files made from them; unset, they are ``load_npz`` itself."""
    from catfish_amd import train_validate as tv
    raw, states, lengths, moves = move_reads()[1]
    path = write_move_npz(tmp_path / "m.npz", raw, states, lengths, moves, (10, 10))
    labels, _ = labelling.label_move_read_host(states, lengths, moves, (10, 10), len(raw))
    np.savez(tmp_path / "l.npz", raw=raw[:labels.size], base_labels=labels)
    monkeypatch.delenv("CATFISH_LABEL_KMER", raising=False)
    monkeypatch.delenv("CATFISH_LABEL_MOVES", raising=False)
    assert tv.npz_loader_from_env() is tv.load_npz
    monkeypatch.setenv("CATFISH_LABEL_MOVES", "0")
    assert tv.npz_loader_from_env() is tv.load_npz
    monkeypatch.setenv("CATFISH_LABEL_MOVES", "1")
    loader = tv.npz_loader_from_env()
    got, want = loader(path), tv.load_npz(str(tmp_path / "l.npz"))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].any()
    a = tv.example_db_from_npz([path], loader=loader)
    b = tv.example_db_from_npz([str(tmp_path / "l.npz")])
    assert a.nb_pos == b.nb_pos > 0 and a.nb_neg == b.nb_neg and np.array_equal(np.asarray(a.pos), np.asarray(b.pos))
    monkeypatch.setenv("CATFISH_DEVICE_NEG", "all")
    db = tv.device_read_db_from_env([path])
    assert np.array_equal(db.labels, labels) and db.nb_pos > 0
    monkeypatch.setenv("CATFISH_LABEL_KMER", "5")
    with pytest.raises(ValueError, match="exclude each other"):
        tv.npz_loader_from_env()
    monkeypatch.delenv("CATFISH_LABEL_KMER")
    monkeypatch.setenv("CATFISH_LABEL_MOVES", "true")
    with pytest.raises(ValueError, match="CATFISH_LABEL_MOVES"):
        tv.npz_loader_from_env()


@pytest.mark.gpu
def test_validation_set_from_move_files_on_the_card(tmp_path):
    from catfish_amd.device_db import DeviceReadDb
    from catfish_amd.device_validation import DeviceValidationSet
    paths = move_files(tmp_path)
    host = DeviceValidationSet.from_move_npz(paths, device="cpu")
    card = DeviceValidationSet.from_move_npz(paths, device="cuda")
    assert host.uploads == 0 and card.uploads == 1
    assert card.labels.dtype == np.uint8 and np.array_equal(card.labels, host.labels) and card.labels.any()
    assert np.array_equal(card.basemap, host.basemap) and np.array_equal(card.lengths, host.lengths)
    assert np.array_equal(card.signal, host.signal) and np.array_equal(card.offsets, host.offsets)
    signal, labels = card.device_arrays("cuda")
    assert card.uploads == 1                                          # the signal went up once, the labels never came from the host
    assert np.array_equal(labels.cpu().numpy(), host.labels) and np.array_equal(signal.cpu().numpy(), host.signal)
    db = DeviceReadDb.from_move_npz(paths, seed=2, device="cuda")
    want_db = DeviceReadDb.from_move_npz(paths, seed=2, device="cpu")
    assert np.array_equal(db.labels, host.labels) and db.nb_pos > 0
    assert np.array_equal(db.pos_start, want_db.pos_start) and np.array_equal(db.neg_start, want_db.neg_start)


@pytest.mark.gpu
def test_one_seeded_round_scores_equal_on_both(hp, tmp_path):
    from catfish_amd.device_validation import DeviceValidationSet
    from catfish_amd.resnet_class import ResNetRNN
    paths = move_files(tmp_path)
    host = DeviceValidationSet.from_move_npz(paths, device="cpu")
    card = DeviceValidationSet.from_move_npz(paths, device="cuda")
    selection = (np.int64([0, 2, 3, 5]), np.int64([0, 700, 35, 1]), np.int64([2500, 2000, 2501, 2400]))     # two start mid-read
    net = ResNetRNN(**hp)
    net.initialize_network(seed=5)
    a = net.score_validation_device(host, selection, (0.3, 0.5), run_edges=(), max_bases=16)
    b = net.score_validation_device(card, selection, (0.3, 0.5), run_edges=(), max_bases=16)
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a.run_bases[:, 0].sum() > 0                               # true homopolymers with their bases: the base map is in the round
