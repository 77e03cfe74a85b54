"""``labelling.LabelSource``: the one reader of ``CATFISH_LABEL_KMER`` / ``CATFISH_LABEL_MOVES``, the loaders it hands out, and
``DeviceValidationSet.from_source`` on the host against the per-kind constructors and the per-read definitions."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import labelling  # noqa: E402
from catfish_amd.labelling import LabelSource  # noqa: E402


def test_from_env_decides_the_kind_once():
    for env in ({}, {"CATFISH_LABEL_KMER": ""}, {"CATFISH_LABEL_KMER": "  "}, {"CATFISH_LABEL_MOVES": "0"}, {"CATFISH_LABEL_MOVES": ""},
                {"CATFISH_LABEL_KMER": "", "CATFISH_LABEL_MOVES": "0"}):
        source = LabelSource.from_env(env)
        assert (source.kind, source.kmer, source.has_tables) == ("labels", None, False), env
    source = LabelSource.from_env({"CATFISH_LABEL_KMER": "5"})
    assert (source.kind, source.kmer, source.has_tables) == ("events", 5, True)
    assert LabelSource.from_env({"CATFISH_LABEL_KMER": " 3 ", "CATFISH_LABEL_MOVES": "0"}).kmer == 3
    source = LabelSource.from_env({"CATFISH_LABEL_MOVES": "1"})
    assert (source.kind, source.kmer, source.has_tables) == ("moves", None, True)
    with pytest.raises(ValueError, match="exclude each other"):
        LabelSource.from_env({"CATFISH_LABEL_KMER": "5", "CATFISH_LABEL_MOVES": "1"})
    for bad in ("6", "17", "true"):
        with pytest.raises(ValueError, match="CATFISH_LABEL_KMER"):
            LabelSource.from_env({"CATFISH_LABEL_KMER": bad})
        with pytest.raises(ValueError, match="CATFISH_LABEL_MOVES"):
            LabelSource.from_env({"CATFISH_LABEL_MOVES": bad})
    with pytest.raises(ValueError, match="CATFISH_LABEL_KMER"):                  # a bad k is a bad k, whatever the other variable says
        LabelSource.from_env({"CATFISH_LABEL_KMER": "6", "CATFISH_LABEL_MOVES": "1"})


def test_from_env_reads_the_process_environment_by_default(monkeypatch):
    monkeypatch.delenv("CATFISH_LABEL_KMER", raising=False)
    monkeypatch.setenv("CATFISH_LABEL_MOVES", "1")
    assert LabelSource.from_env().kind == "moves"
    monkeypatch.setenv("CATFISH_LABEL_KMER", "7")
    with pytest.raises(ValueError, match="exclude each other"):
        LabelSource.from_env()
    from catfish_amd import train_validate as tv
    with pytest.raises(ValueError, match="exclude each other"):                  # the read database refuses both at once too
        tv.device_read_db_from_env([])


def test_a_source_checks_its_kind_and_k():
    assert LabelSource().kind == "labels" and LabelSource("moves", 6).kmer is None
    with pytest.raises(ValueError, match="label source"):
        LabelSource("tables")
    for bad in (6, 17, None, True):
        with pytest.raises(ValueError, match="kmer"):
            LabelSource("events", bad)
    with pytest.raises(ValueError, match="without tables"):
        LabelSource().load("x.npz")


def three_reads(tmp_path):
    """Three synthetic reads of a few hundred samples, each stored three ways: {kind: paths}; some raw signal lies behind the events."""
    paths = {"labels": [], "events": [], "moves": []}
    for i, length in enumerate((300, 411, 257)):
        raw, bases, samples = labelling.synthetic_event_read(length, 40 + i, hp_fraction=0.6)
        _raw, states, seconds, moves = labelling.synthetic_move_read(length, 40 + i)
        raw = np.concatenate([raw, np.zeros(5 * i)])
        labels, _ = labelling.label_read_host(bases, samples, (1, 2), 5)
        for kind, arrays in (("labels", {"base_labels": labels}),
                             ("events", {"event_base": bases.view("S1"), "event_length": samples, "clipped_start": np.int64(1), "clipped_end": np.int64(2)}),
                             ("moves", {"event_state": np.ascontiguousarray(states).view("S5").reshape(-1), "event_move": moves, "event_length": seconds,
                                        "clipped_start": np.int64(1), "clipped_end": np.int64(2)})):
            paths[kind].append(str(tmp_path / ("%s%d.npz" % (kind, i))))
            np.savez(paths[kind][-1], raw=raw[:labels.size] if kind == "labels" else raw, **arrays)
    return paths


def test_every_kinds_loader_is_the_loader_the_environment_names(tmp_path, monkeypatch):
    """``loader()`` per kind: ``load_npz`` itself, ``load_labelled_event_npz`` with the source's k, ``load_labelled_move_npz`` -- and what
    ``train_validate.npz_loader_from_env`` gives with the variables set to that kind."""
    from catfish_amd import train_validate as tv
    paths = three_reads(tmp_path)
    cases = (({}, "labels", tv.load_npz), ({"CATFISH_LABEL_KMER": "5"}, "events", lambda p: labelling.load_labelled_event_npz(p, 5)),
             ({"CATFISH_LABEL_KMER": "3"}, "events", lambda p: labelling.load_labelled_event_npz(p, 3)),
             ({"CATFISH_LABEL_MOVES": "1"}, "moves", labelling.load_labelled_move_npz))
    for env, kind, want in cases:
        monkeypatch.delenv("CATFISH_LABEL_KMER", raising=False)
        monkeypatch.delenv("CATFISH_LABEL_MOVES", raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        source = LabelSource.from_env(env)
        assert source.kind == kind
        if kind == "labels":
            assert source.loader() is tv.load_npz and tv.npz_loader_from_env() is tv.load_npz
        if kind == "moves":
            assert source.loader() is labelling.load_labelled_move_npz
        some = False
        for path in paths[kind]:
            raw, labels = want(path)
            for got_raw, got_labels in (source.loader()(path), tv.npz_loader_from_env()(path)):
                assert np.array_equal(got_raw, raw) and np.array_equal(got_labels, labels) and len(got_raw) == len(got_labels)
            some = some or bool(np.any(labels))
        assert some, kind
    a, b = (labelling.load_labelled_event_npz(paths["events"][0], k)[1] for k in (3, 5))
    assert not np.array_equal(a, b)                                              # the k reaches the loader
    assert np.array_equal(tv.load_npz(paths["labels"][0])[1], b)                 # the labelled files hold the k = 5 labels of the event files


def test_validation_set_from_source_on_the_host(tmp_path):
    from catfish_amd.base_votes import BaseTable
    from catfish_amd.device_db import DeviceReadDb
    from catfish_amd.device_validation import DeviceValidationSet
    paths = three_reads(tmp_path)

    def same(a, b):
        assert a.signal.dtype == np.float32 and a.labels.dtype == np.uint8 and a.uploads == 0 and a.labels.any()
        assert np.array_equal(a.signal, b.signal) and np.array_equal(a.labels, b.labels) and np.array_equal(a.offsets, b.offsets)
        assert (a.basemap is None) == (b.basemap is None) and (a.bases is None) == (b.bases is None)
        if a.basemap is not None:
            assert np.array_equal(a.basemap, b.basemap) and np.array_equal(a.bases.edges, b.bases.edges)
            assert np.array_equal(a.bases.base_offsets, b.bases.base_offsets)

    plain = DeviceValidationSet.from_source(paths["labels"], LabelSource(), device="cpu")
    same(plain, DeviceValidationSet.from_npz(paths["labels"]))
    assert plain.basemap is None and plain.bases is None and plain.n_reads == 3

    for kmer in (3, 5):
        events = DeviceValidationSet.from_source(paths["events"], LabelSource("events", kmer), device="cpu")
        same(events, DeviceValidationSet.from_event_npz(paths["events"], kmer, device="cpu"))
        reads = [labelling.load_event_npz(p) for p in paths["events"]]
        want = [labelling.label_read_host(r["bases"], r["lengths"], r["clipped"], kmer) for r in reads]         # the per-read definition
        assert np.array_equal(events.labels, np.concatenate([w[0] for w in want])) and np.array_equal(events.basemap, np.concatenate([w[1] for w in want]))
        assert np.array_equal(events.signal, np.concatenate([r["raw"][:w[0].size] for r, w in zip(reads, want)]).astype(np.float32))
        assert np.array_equal(events.bases.edges, np.concatenate([[0], np.cumsum(np.concatenate([r["lengths"] for r in reads]))]))
    same(events, DeviceValidationSet.from_events([r["raw"] for r in reads], labelling.EventBatch.from_reads(reads), 5, device="cpu"))
    assert np.array_equal(events.labels, plain.labels) and np.array_equal(events.signal, plain.signal)          # k = 5: the labelled files

    moves = DeviceValidationSet.from_source(paths["moves"], LabelSource("moves"), device="cpu")
    same(moves, DeviceValidationSet.from_move_npz(paths["moves"], device="cpu"))
    reads = [labelling.load_move_npz(p) for p in paths["moves"]]
    want = [labelling.label_move_read_host(r["states"], r["lengths"], r["moves"], r["clipped"], len(r["raw"])) for r in reads]
    assert np.array_equal(moves.labels, np.concatenate([w[0] for w in want])) and np.array_equal(moves.basemap, np.concatenate([w[1] for w in want]))
    assert np.array_equal(moves.offsets, np.concatenate([[0], np.cumsum([w[0].size for w in want])]))
    batch = labelling.MoveBatch.from_reads(reads)
    same(moves, DeviceValidationSet.from_moves([r["raw"] for r in reads], batch, device="cpu"))
    assert np.array_equal(moves.bases.edges, BaseTable.from_moves(batch).edges) and moves.bases.n_reads == 3
    marks = np.flatnonzero(moves.basemap & labelling.MARK)                       # at most one marked sample per base of the table
    assert 0 < marks.size <= moves.bases.n_bases and np.all(np.diff(np.searchsorted(moves.bases.edges, marks, side="right")) > 0)

    for kind, source in (("labels", LabelSource()), ("events", LabelSource("events", 5)), ("moves", LabelSource("moves"))):
        db = DeviceReadDb.from_source(paths[kind], source, seed=3, device="cpu")
        vset = DeviceValidationSet.from_source(paths[kind], source, device="cpu")
        assert np.array_equal(db.labels, vset.labels) and np.array_equal(db.signal, vset.signal) and np.array_equal(db.offsets, vset.offsets)
