"""Labels from event tables on the card: ``labelling.label_reads`` (``cf_label_events``: label_event_classes_kernel and
label_expand_kernel, csrc/label_events.hpp) against ``EventBatch.label_host``, byte for byte, labels and base map, on the golden
cases and on every size at which the kernels take another path.  Integers only: no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import labelling  # noqa: E402
from catfish_amd.labelling import EventBatch  # noqa: E402
from test_label_events_host import edge_batches, golden_cases, write_event_npz  # noqa: E402

pytestmark = pytest.mark.gpu
_host = {}


def host_labels(name, kmer):
    """``label_host`` of an edge batch, computed once."""
    if (name, kmer) not in _host:
        _host[(name, kmer)] = edge_batches_once()[name].label_host(kmer, base_map=True)
    return _host[(name, kmer)]


def edge_batches_once():
    if "batches" not in _host:
        _host["batches"] = edge_batches()
    return _host["batches"]


@pytest.mark.parametrize("kmer", (1, 5, 7))
def test_label_reads_equals_the_host_byte_for_byte(kmer):
    import torch
    for name, batch in edge_batches_once().items():
        want_labels, want_map = host_labels(name, kmer)
        labels, basemap = labelling.label_reads(batch, kmer, "cuda", base_map=True)
        assert labels.dtype == torch.uint8 and labels.is_cuda and tuple(labels.shape) == (batch.total,)
        assert np.array_equal(labels.cpu().numpy(), want_labels), name
        assert np.array_equal(basemap.cpu().numpy(), want_map), name


def test_the_golden_cases_each_with_its_own_kmer():
    cases = golden_cases()
    for kmer in sorted({c["kmer"] for c in cases}):
        some = [c for c in cases if c["kmer"] == kmer]
        batch = EventBatch.from_reads([(c["bases"], c["lengths"], c["clipped"]) for c in some])
        labels, basemap = labelling.label_reads(batch, kmer, base_map=True)
        assert np.array_equal(labels.cpu().numpy(), np.concatenate([c["labels"] for c in some]))
        assert np.array_equal(basemap.cpu().numpy(), np.concatenate([c["basemap"] for c in some]))


def test_no_base_map_equal_runs_and_the_empty_batch():
    batch = edge_batches_once()["synthetic reads"]
    want, _ = host_labels("synthetic reads", 5)
    alone = labelling.label_reads(batch, 5, "cuda")                  # basemap_out = NULL leaves the labels unchanged
    assert np.array_equal(alone.cpu().numpy(), want)
    first = [t.cpu().numpy() for t in labelling.label_reads(batch, 5, "cuda", base_map=True)]
    second = [t.cpu().numpy() for t in labelling.label_reads(batch, 5, "cuda", base_map=True)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))          # no atomics: equal inputs, equal bytes
    empty = EventBatch.from_reads([])
    assert empty.n_reads == 0 and empty.total == 0
    labels, basemap = labelling.label_reads(empty, 5, "cuda", base_map=True)       # total == 0: CF_OK, nothing launched
    assert labels.numel() == 0 and basemap.numel() == 0 and labels.is_cuda
    with pytest.raises(ValueError):
        labelling.label_reads(batch, 4, "cuda")
    with pytest.raises(ValueError):
        labelling.label_reads(batch, 5, "cpu")


def test_the_c_abi_refuses_what_the_header_says():
    import torch
    from catfish_amd import _native as N
    lib = N.lib()
    batch = edge_batches_once()["neighbouring reads"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    t = [up(batch.bases), up(batch.lengths), up(batch.event_offsets), up(batch.clipped.reshape(-1)), up(batch.sample_offsets)]
    out = torch.zeros(batch.total, dtype=torch.uint8, device="cuda")
    work_bytes = int(lib.cf_label_events_work_bytes(batch.n_events))
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    stream = N.current_stream_ptr(torch, out.device)

    def call(n_reads=batch.n_reads, n_events=batch.n_events, total=batch.total, kmer=5, bases=t[0], labels=out, work_at=work, bytes_=work_bytes):
        return lib.cf_label_events(None, N._p(bases) if bases is not None else None, N._p(t[1]), N._p(t[2]), N._p(t[3]), N._p(t[4]), n_reads,
                                   n_events, total, kmer, N._p(labels) if labels is not None else None, None,
                                   N._p(work_at) if work_at is not None else None, bytes_, stream)

    for change, text in ((dict(kmer=4), "kmer"), (dict(kmer=17), "kmer"), (dict(n_reads=-1), "negative"), (dict(total=2 ** 31), "2^31"),
                         (dict(n_events=2 ** 31, bytes_=2 ** 40), "2^31"), (dict(bytes_=5 * batch.n_events - 1), "work buffer"),
                         (dict(bases=None), "null"), (dict(labels=None), "null"), (dict(work_at=None), "null"),
                         (dict(n_reads=2 ** 23 + 1), "too many reads")):
        assert call(**change) == N.CF_ERR_INVALID, change
        assert text in lib.cf_last_error().decode(), (change, lib.cf_last_error())
    assert call(total=0) == N.CF_OK
    torch.cuda.synchronize()
    assert not out.any().item()                                      # nothing was launched by any of these
    assert call() == N.CF_OK
    assert np.array_equal(out.cpu().numpy(), batch.label_host(5))


def test_validation_set_from_event_files_on_the_card(tmp_path):
    from catfish_amd.device_db import DeviceReadDb
    from catfish_amd.device_validation import DeviceValidationSet
    reads = [labelling.synthetic_event_read(2000 + 35 * i, 90 + i) for i in range(6)]
    paths = [write_event_npz(tmp_path / ("v%d.npz" % i), np.concatenate([raw, np.zeros(i)]), b, l, (10, 10), starts=True)
             for i, (raw, b, l) in enumerate(reads)]
    host = DeviceValidationSet.from_event_npz(paths, kmer=5, device="cpu")
    card = DeviceValidationSet.from_event_npz(paths, kmer=5, device="cuda")
    assert host.uploads == 0 and card.uploads == 1
    assert card.labels.dtype == np.uint8 and np.array_equal(card.labels, host.labels) and card.labels.any()
    assert np.array_equal(card.signal, host.signal) and np.array_equal(card.offsets, host.offsets)
    signal, labels = card.device_arrays("cuda")
    assert card.uploads == 1                                          # the signal went up once, the labels never came from the host
    assert np.array_equal(labels.cpu().numpy(), host.labels) and np.array_equal(signal.cpu().numpy(), host.signal)
    db = DeviceReadDb.from_event_npz(paths, kmer=5, seed=2, device="cuda")
    assert np.array_equal(db.labels, host.labels) and db.nb_pos > 0
