"""The bodies of label_moves_merge_kernel, label_moves_classes_kernel and the label_expand_kernel behind them on the CPU under
AddressSanitizer + UBSan: tests/native/label_moves_replay.cpp walks the three grids serially through csrc/label_moves_rule.hpp and
csrc/label_events_rule.hpp -- the rules by which the kernels form their addresses and turn seconds into samples -- with every buffer
malloc'ed at exactly the size the Python layer allocates.  A stand-alone program run as its own process; nothing is preloaded.  Its
output must EQUAL ``MoveBatch.label_host`` on the golden cases and the edge batches of the GPU test; forged device tables (NaN,
negative and 1e30 lengths, event offsets outside the table) must be written inside the buffers only, with label 0 where nothing
vouches for a sample; refused arguments give the refusal; and the sanitizers must have nothing to say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd.labelling import MoveBatch
from test_label_moves_host import FILLER, edge_batches, golden_batches, kmers_with_runs, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xEE
SAT = 2 ** 31 - 1


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("label_moves") / "label_moves_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "label_moves_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def tables_of(batch):
    """[states, lengths, moves, event_offsets, clipped, n_raw, sample_offsets], copies."""
    return [batch.states.copy(), batch.lengths.copy(), batch.moves.copy(), batch.event_offsets.copy(), batch.clipped.copy(), batch.n_raw.copy(),
            batch.sample_offsets.copy()]


def replayed(exe, tmp_path, tables, base_map=True, lead=0, n_reads=None, n_events=None, total=None, k=None, work_bytes=-1, f64=None):
    """``tables`` as ``tables_of`` gives them, unchecked -> None when the arguments are refused, else (labels [total], basemap [total]
    or None, counts int32 [n_reads, 2]) as the program left them."""
    states, lengths, moves, event_offsets, clipped, n_raw, sample_offsets = tables
    n_reads = len(event_offsets) - 1 if n_reads is None else n_reads
    n_events = len(moves) if n_events is None else n_events
    total = int(sample_offsets[-1]) if total is None else total
    k = states.shape[1] if k is None else k
    f64 = int(lengths.dtype == np.float64) if f64 is None else f64
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as fh:
        np.array([n_reads, n_events, total, k, int(base_map), lead, work_bytes, f64], np.int64).tofile(fh)
        np.asarray(event_offsets, np.int64).tofile(fh)
        np.asarray(sample_offsets, np.int64).tofile(fh)
        np.asarray(n_raw, np.int64).tofile(fh)
        np.asarray(clipped, np.int32).tofile(fh)
        np.asarray(moves, np.int32).tofile(fh)
        np.ascontiguousarray(lengths).tofile(fh)
        np.asarray(states, np.uint8).tofile(fh)
    run = subprocess.run([exe, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    with open(out, "rb") as fh:
        refusal = int(np.fromfile(fh, np.int64, 1)[0])
        if refusal:
            assert fh.read() == b""
            return None
        labels = np.fromfile(fh, np.uint8, total)
        basemap = np.fromfile(fh, np.uint8, total) if base_map else None
        counts = np.fromfile(fh, np.int32, 2 * n_reads).reshape(-1, 2)
        assert fh.read() == b""
    return labels, basemap, counts


def test_the_library_asks_for_the_work_buffer_the_rule_header_sizes():
    """11 bytes per event and 8 per read, rounded up to 16, never 0: what the replay program mallocs is what ``label_moves``
    allocates."""
    from catfish_amd import _native
    lib = _native.lib()
    for (r, n), want in (((0, 0), 16), ((1, 1), 32), ((1, 0), 16), ((2, 0), 16), ((3, 1024), 11296), ((7, 1025), 11344),
                         ((2 ** 23, 2 ** 31 - 1), (11 * (2 ** 31 - 1) + 8 * 2 ** 23 + 15) // 16 * 16)):
        assert lib.cf_label_moves_work_bytes(r, n) == want
    assert lib.cf_label_moves_work_bytes(-1, 5) == -1 and lib.cf_label_moves_work_bytes(1, -1) == -1
    assert lib.cf_label_moves_work_bytes(1, 2 ** 31) == -1 and lib.cf_label_moves_work_bytes(2 ** 23 + 1, 1) == -1


def test_golden_cases_equal_the_reference(replay, tmp_path):
    for (k, name), (batch, want) in golden_batches().items():
        _labels, want_map = batch.label_host(base_map=True)
        for lead in (0, 4, 8, 5):
            labels, basemap, counts = replayed(replay, tmp_path, tables_of(batch), lead=lead)
            assert np.array_equal(labels, want), (k, name)
            assert np.array_equal(basemap, want_map), (k, name)
            assert np.array_equal(counts[:, 0], batch.merged) and np.array_equal(counts[:, 1], batch.final)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_edge_batches_equal_the_host(replay, tmp_path, dtype):
    for name, batch in edge_batches(dtype).items():
        want_labels, want_map = batch.label_host(base_map=True)
        for lead in ((0, 5) if name == "merged-event borders at a tile border" else (0,)):
            labels, basemap, counts = replayed(replay, tmp_path, tables_of(batch), lead=lead)
            assert np.array_equal(labels, want_labels), name
            assert np.array_equal(basemap, want_map), name
            assert np.array_equal(counts[:, 0], batch.merged) and np.array_equal(counts[:, 1], batch.final), name


def test_without_a_base_map_the_labels_are_the_same(replay, tmp_path):
    batch = edge_batches()["stays across a piece border"]
    labels, none, _counts = replayed(replay, tmp_path, tables_of(batch), base_map=False)
    assert none is None and np.array_equal(labels, batch.label_host())


def vouched(tables, n_events):
    """What forged tables must give: per read with a sound event range, every merged event's class (and middle byte) over the samples
    [start, start + n) that lie inside the read; n = ceil(sum * 4000) in the table's dtype where that is a finite number > 0 (at most
    2^31 - 1), else 0; start = the running sum; every other sample 0.  -> (labels, basemap, counts).  (Reads small enough that no
    tile meets more merged events than it stages.)"""
    states, lengths, moves, event_offsets, clipped, n_raw, sample_offsets = tables
    dt = lengths.dtype.type
    labels, basemap = np.zeros(int(sample_offsets[-1]), np.uint8), np.zeros(int(sample_offsets[-1]), np.uint8)
    counts = np.zeros((len(event_offsets) - 1, 2), np.int32)
    for r in range(len(event_offsets) - 1):
        e0, e1, s0, s1 = int(event_offsets[r]), int(event_offsets[r + 1]), int(sample_offsets[r]), int(sample_offsets[r + 1])
        if not 0 <= e0 <= e1 <= n_events or e0 == e1:
            counts[r, 1] = 0
            continue
        heads = [0] + [e for e in range(1, e1 - e0) if moves[e0 + e] != 0]
        ends = heads[1:] + [e1 - e0]
        n = []
        with np.errstate(all="ignore"):
            for h, end in zip(heads, ends):
                total = dt(lengths[e0 + h] + lengths[e0]) if h == 0 else lengths[e0 + h]
                for e in range(h + 1, end):
                    total = dt(total + lengths[e0 + e])
                product = dt(total * dt(4000))
                n.append(0 if not (product > 0) or not np.isfinite(product) else min(int(np.ceil(np.float64(product))), SAT))
        m, cs, ce = len(heads), int(clipped[r][0]), int(clipped[r][1])
        core = [int(cs <= j < m - ce and states[e0 + h][0] != ord("N") and (states[e0 + h] == states[e0 + h][0]).all()) for j, h in enumerate(heads)]
        at = 0
        for j, h in enumerate(heads):
            cls = int(any(core[max(0, j - 2):j + 3]))
            end = min(at + n[j], SAT)
            for q in range(at, min(end, s1 - s0)):
                labels[s0 + q] = cls
                basemap[s0 + q] = states[e0 + h][states.shape[1] // 2] | (0x80 if q == at + (end - at) // 2 else 0)
            at = end
        counts[r] = (m, min(at, max(int(n_raw[r]), 0)))
    return labels, basemap, counts


def test_forged_device_tables(replay, tmp_path):
    for dtype in (np.float32, np.float64):
        reads = [table_of([7, 3, 9, 2, 5, 8, 4, 6, 3, 7], kmers_with_runs(10, ((2, 4),)), dtype, [0, 1, 0, 2, 0, 0, 1, 0, 0, 3]),
                 table_of([1, 1, 300, 1, 1, 1, 1, 300, 1], kmers_with_runs(9, ((6, 9),)), dtype),
                 table_of([4] * 50, kmers_with_runs(50, ((0, 2), (47, 50))), dtype, [1] * 50, clipped=(1, 1)),
                 table_of([6] * 5, [b"AAAAA"] * 5, dtype), table_of([3] * 1100, kmers_with_runs(1100, ((1020, 1030), (500, 505))), dtype, [1] * 1100),
                 table_of([40] * 12, kmers_with_runs(12, ((4, 6),)), dtype, n_raw=300)]
        batch = MoveBatch.from_reads(reads)
        n_events, eo = batch.n_events, batch.event_offsets
        forgeries = []

        def forge(name, what, index, value):
            tables = tables_of(batch)
            tables[what][index] = value
            forgeries.append((name, tables))

        forge("a NaN length", 1, eo[0] + 4, np.nan)
        forge("a NaN length in the read's first event", 1, eo[2], np.nan)
        forge("an infinite length", 1, eo[2] + 7, np.inf)
        forge("a negative length", 1, eo[2] + 5, -5.0)
        forge("a negative length that leaves the sum negative", 1, eo[1] + 2, -1.0e9)
        forge("a zero length in a merged event of one", 1, eo[1] + 4, 0.0)
        forge("a 1e30 length", 1, eo[2] + 1, 1.0e30)
        forge("a 1e30 length at the read's last event", 1, eo[3] - 1, 1.0e30)
        forge("a 1e30 length at the read's first event", 1, eo[4], 1.0e30)
        forge("a length that sums short", 1, eo[1] + 2, 0.0001)
        forge("a length that sums past the read", 1, eo[5] + 3, 0.5)
        forge("a NaN length at the piece border", 1, eo[4] + 1023, np.nan)
        forge("an event_offsets entry past n_events", 3, 3, n_events + 5)
        forge("the last event_offsets entry past n_events", 3, 6, n_events + 1)
        forge("a negative event_offsets entry", 3, 0, -1)
        forge("a negative n_raw", 5, 2, -7)
        forge("negative clips", 4, 2, (-3, -1))
        forge("clips past the read", 4, 0, (2 ** 31 - 1, 2 ** 31 - 1))
        forge("a state byte with bit 7", 0, eo[1] + 3, 200)
        tables = tables_of(batch)
        tables[1][eo[4]:eo[5]] = 1.0e30                                # every length of a read huge: the running sum saturates
        forgeries.append(("all lengths 1e30", tables))
        tables = tables_of(batch)
        tables[1][:] = np.nan
        forgeries.append(("all lengths NaN", tables))
        tables = tables_of(batch)
        tables[2][:] = 0                                                # a forged all-zero move column: one thread walks each read
        forgeries.append(("no moves", tables))
        for name, tables in forgeries:
            for lead in (0, 3):
                labels, basemap, counts = replayed(replay, tmp_path, tables, lead=lead)  # ... and a silent sanitizer: nothing outside the buffers
                want_labels, want_map, want_counts = vouched(tables, n_events)
                assert np.array_equal(labels, want_labels), name     # 0 where nothing vouches for the sample, and no sample left unwritten
                assert np.array_equal(basemap, want_map), name
                assert np.array_equal(counts, want_counts), name
        untouched = batch.label_host()
        labels, _map, _counts = replayed(replay, tmp_path, forgeries[2][1])
        assert np.array_equal(labels[:batch.sample_offsets[2]], untouched[:batch.sample_offsets[2]])   # the other reads are whole
        assert np.array_equal(labels[batch.sample_offsets[3]:], untouched[batch.sample_offsets[3]:])
        assert not np.array_equal(labels, untouched)
        # sample_offsets that are not what the layout promises: that read is not written (the sentinel stays), nothing else is touched
        tables = tables_of(batch)
        tables[6][3] = tables[6][2] - 1
        labels, _map, _counts = replayed(replay, tmp_path, tables)
        assert set(np.unique(labels)) <= {0, 1, SENTINEL}
        assert np.array_equal(labels[:batch.sample_offsets[2] - 1], untouched[:batch.sample_offsets[2] - 1])
        tables = tables_of(batch)
        tables[6][6] = batch.total + 4096
        labels, _map, _counts = replayed(replay, tmp_path, tables, total=batch.total)
        assert (labels[batch.sample_offsets[5]:] == SENTINEL).all() and np.array_equal(labels[:batch.sample_offsets[5]], untouched[:batch.sample_offsets[5]])


def test_refused_arguments(replay, tmp_path):
    batch = edge_batches()["neighbouring reads"]
    assert replayed(replay, tmp_path, tables_of(batch)) is not None
    floor = 11 * batch.n_events + 8 * batch.n_reads
    for change in (dict(k=0), dict(k=16), dict(k=-1), dict(k=2 ** 32 + 5), dict(n_reads=-1), dict(n_events=-1), dict(total=-1), dict(n_events=2 ** 31),
                   dict(total=2 ** 31), dict(n_reads=2 ** 23 + 1), dict(work_bytes=floor - 1), dict(work_bytes=0), dict(f64=2), dict(f64=-1),
                   dict(f64=2 ** 32)):
        assert replayed(replay, tmp_path, tables_of(batch), **change) is None, change
    assert replayed(replay, tmp_path, tables_of(batch), work_bytes=floor) is not None
    empty = MoveBatch.from_reads([])
    labels, basemap, counts = replayed(replay, tmp_path, tables_of(empty))
    assert labels.size == 0 and basemap.size == 0 and counts.size == 0
    assert FILLER[0] == b"ACGTA"
