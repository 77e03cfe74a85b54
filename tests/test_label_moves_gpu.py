"""Labels from a basecaller's move table on the card: ``labelling.label_moves`` (``cf_label_moves``: label_moves_merge_kernel,
label_moves_classes_kernel, csrc/label_moves.hpp, and label_expand_kernel behind them) against ``MoveBatch.label_host``, byte for
byte, labels and base map, on the golden cases and on every size at which the kernels take another path.  P = 1024 is the merge
kernel's piece, 4096 the tile.  No tolerance anywhere: the float sums are taken in the host's order with the host's roundings."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from catfish_amd import labelling  # noqa: E402
from catfish_amd.labelling import MoveBatch  # noqa: E402
from test_label_moves_host import edge_batches, golden_batches  # noqa: E402

pytestmark = pytest.mark.gpu
_host = {}


def edge_once(dtype):
    """The edge batches of one length dtype with their ``label_host``, computed once."""
    key = np.dtype(dtype).name
    if key not in _host:
        batches = edge_batches(dtype)
        _host[key] = {name: (batch, batch.label_host(base_map=True)) for name, batch in batches.items()}
    return _host[key]


def test_the_golden_cases():
    """One batch per k and length dtype (a batch has one of each): the reference's own labels."""
    import torch
    for (k, name), (batch, want) in golden_batches().items():
        _labels, want_map = batch.label_host(base_map=True)
        labels, basemap, offsets = labelling.label_moves(batch, "cuda", base_map=True)
        assert labels.dtype == torch.uint8 and labels.is_cuda and tuple(labels.shape) == (batch.total,)
        assert np.array_equal(labels.cpu().numpy(), want), (k, name)
        assert np.array_equal(basemap.cpu().numpy(), want_map), (k, name)
        assert offsets.dtype == torch.int64 and np.array_equal(offsets.cpu().numpy(), batch.sample_offsets)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_label_moves_equals_the_host_byte_for_byte(dtype):
    """Reads of P - 1, P and P + 1 events; stay runs over a piece border; heads that begin and end a piece; merged-event borders one
    sample before, on and one after a tile border; one merged event of 8 195 samples; 4 097 one-sample merged events; reads cut by
    n_raw inside the first tile and on a tile border; AAAAA at the end of one read and the start of the next; synthetic reads."""
    for name, (batch, (want_labels, want_map)) in edge_once(dtype).items():
        labels, basemap, _offsets = labelling.label_moves(batch, "cuda", base_map=True)
        assert np.array_equal(labels.cpu().numpy(), want_labels), name
        assert np.array_equal(basemap.cpu().numpy(), want_map), name


def test_one_table_as_float32_and_as_float64():
    """The same numbers in both dtypes, one call behind the other: each equals its own host answer, and the two differ -- the card
    neither widens the float32 table nor narrows the float64 one."""
    narrow, (narrow_labels, narrow_map) = edge_once(np.float32)["synthetic reads"]
    wide = MoveBatch.from_reads([(s, l.astype(np.float64), m, c, n) for s, l, m, c, n in (narrow.read(r) for r in range(narrow.n_reads))])
    assert wide.lengths.dtype == np.float64 and np.array_equal(wide.lengths, narrow.lengths.astype(np.float64))
    wide_labels, wide_map = wide.label_host(base_map=True)
    a = labelling.label_moves(narrow, "cuda", base_map=True)
    b = labelling.label_moves(wide, "cuda", base_map=True)
    assert np.array_equal(a[0].cpu().numpy(), narrow_labels) and np.array_equal(a[1].cpu().numpy(), narrow_map)
    assert np.array_equal(b[0].cpu().numpy(), wide_labels) and np.array_equal(b[1].cpu().numpy(), wide_map)
    assert not np.array_equal(narrow.final, wide.final) or not np.array_equal(narrow_labels, wide_labels)


def test_no_base_map_equal_runs_and_the_empty_batch():
    batch, (want, _map) = edge_once(np.float32)["synthetic reads"]
    alone, _offsets = labelling.label_moves(batch, "cuda")             # basemap_out = NULL leaves the labels unchanged
    assert np.array_equal(alone.cpu().numpy(), want)
    first = [t.cpu().numpy() for t in labelling.label_moves(batch, "cuda", base_map=True)]
    second = [t.cpu().numpy() for t in labelling.label_moves(batch, "cuda", base_map=True)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))          # no atomics: equal inputs, equal bytes
    empty = MoveBatch.from_reads([])
    assert empty.n_reads == 0 and empty.total == 0
    labels, basemap, offsets = labelling.label_moves(empty, "cuda", base_map=True)     # total == 0: CF_OK, nothing launched
    assert labels.numel() == 0 and basemap.numel() == 0 and labels.is_cuda and offsets.cpu().tolist() == [0]
    with pytest.raises(ValueError):
        labelling.label_moves(batch, "cpu")


def test_the_c_abi_refuses_what_the_header_says():
    import torch
    from catfish_amd import _native as N
    lib = N.lib()
    batch, (want, _map) = edge_once(np.float32)["neighbouring reads"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    t = [up(batch.states.reshape(-1)), up(batch.lengths), up(batch.moves), up(batch.event_offsets), up(batch.clipped.reshape(-1)), up(batch.n_raw),
         up(batch.sample_offsets)]
    out = torch.zeros(batch.total, dtype=torch.uint8, device="cuda")
    work_bytes = int(lib.cf_label_moves_work_bytes(batch.n_reads, batch.n_events))
    work = torch.zeros(work_bytes, dtype=torch.uint8, device="cuda")
    stream = N.current_stream_ptr(torch, out.device)
    p = lambda x: N._p(x) if x is not None else None                   # noqa: E731

    def call(n_reads=batch.n_reads, n_events=batch.n_events, total=batch.total, k=5, f64=0, states=t[0], lengths=t[1], n_raw=t[5], labels=out,
             work_at=work, bytes_=work_bytes):
        return lib.cf_label_moves(None, p(states), p(lengths), f64, p(t[2]), p(t[3]), p(t[4]), p(n_raw), p(t[6]), n_reads, n_events, total, k,
                                  p(labels), None, p(work_at), bytes_, stream)

    floor = 11 * batch.n_events + 8 * batch.n_reads
    for change, text in ((dict(k=0), "k must"), (dict(k=16), "k must"), (dict(n_reads=-1), "negative"), (dict(n_events=-1), "negative"),
                         (dict(total=-1), "negative"), (dict(total=2 ** 31), "2^31"), (dict(n_events=2 ** 31, bytes_=2 ** 40), "2^31"),
                         (dict(bytes_=floor - 1), "work buffer"), (dict(bytes_=-1), "work buffer"), (dict(f64=2), "lengths_f64"),
                         (dict(states=None), "null"), (dict(lengths=None), "null"), (dict(n_raw=None), "null"), (dict(labels=None), "null"),
                         (dict(work_at=None), "null"), (dict(n_reads=2 ** 23 + 1, bytes_=2 ** 40), "too many reads")):
        assert call(**change) == N.CF_ERR_INVALID, change
        assert text in lib.cf_last_error().decode(), (change, lib.cf_last_error())
    assert call(total=0) == N.CF_OK
    torch.cuda.synchronize()
    assert not out.any().item() and not work.any().item()            # nothing was launched by any of these
    assert call() == N.CF_OK
    assert np.array_equal(out.cpu().numpy(), want)
    counts = work[8 * batch.n_events:8 * batch.n_events + 8 * batch.n_reads].cpu().numpy().view(np.int32).reshape(-1, 2)
    assert np.array_equal(counts[:, 0], batch.merged) and np.array_equal(counts[:, 1], batch.final)     # M and final, as the header says
