"""The bodies of label_event_classes_kernel and label_expand_kernel on the CPU under AddressSanitizer + UBSan:
tests/native/label_events_replay.cpp walks both grids serially through csrc/label_events_rule.hpp -- the rules by which the kernels
form their addresses -- with every buffer malloc'ed at exactly the size the Python layer allocates.  A stand-alone program run as its
own process; nothing is preloaded.  Its output must EQUAL ``EventBatch.label_host`` on the golden cases and the edge batches; forged
device tables must be written inside the buffers only, with label 0 where no event vouches for a sample; refused arguments give the
refusal; and the sanitizers must have nothing to say."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from catfish_amd import labelling
from catfish_amd.labelling import EventBatch
from test_label_events_host import edge_batches, golden_cases, run_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path_factory.mktemp("label_events") / "label_events_replay")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "native", "label_events_replay.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if build.returncode != 0 and "asan" in build.stdout.lower() and "cannot find" in build.stdout.lower():
        pytest.skip("g++ without the AddressSanitizer runtime")
    assert build.returncode == 0, build.stdout
    return exe


def replayed(exe, tmp_path, tables, kmer=5, base_map=True, lead=0, n_reads=None, n_events=None, total=None, work_bytes=-1):
    """``tables`` = (bases, lengths, event_offsets, clipped, sample_offsets), unchecked -> None when the arguments are refused, else
    (labels [total], basemap [total] or None) as the program left them."""
    bases, lengths, event_offsets, clipped, sample_offsets = tables
    n_reads = len(event_offsets) - 1 if n_reads is None else n_reads
    n_events = len(bases) if n_events is None else n_events
    total = int(sample_offsets[-1]) if total is None else total
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as fh:
        np.array([n_reads, n_events, total, kmer, int(base_map), lead, work_bytes, 0], np.int64).tofile(fh)
        np.asarray(event_offsets, np.int64).tofile(fh)
        np.asarray(sample_offsets, np.int64).tofile(fh)
        np.asarray(clipped, np.int32).tofile(fh)
        np.asarray(lengths, np.int32).tofile(fh)
        np.asarray(bases, np.uint8).tofile(fh)
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
        assert fh.read() == b""
    return labels, basemap


def tables_of(batch):
    return [batch.bases.copy(), batch.lengths.copy(), batch.event_offsets.copy(), batch.clipped.copy(), batch.sample_offsets.copy()]


def test_the_library_asks_for_the_work_buffer_the_rule_header_sizes():
    """5 bytes per event rounded up to 16, never 0: what the replay program mallocs is what ``label_reads`` allocates."""
    from catfish_amd import _native
    lib = _native.lib()
    for n, want in ((0, 16), (1, 16), (3, 16), (4, 32), (1024, 5120), (1025, 5136), (2 ** 31 - 1, (5 * (2 ** 31 - 1) + 15) // 16 * 16)):
        assert lib.cf_label_events_work_bytes(n) == want
    assert lib.cf_label_events_work_bytes(-1) == -1 and lib.cf_label_events_work_bytes(2 ** 31) == -1


@pytest.mark.parametrize("kmer", (1, 5, 7))
def test_golden_cases_and_edge_batches_equal_the_host(replay, tmp_path, kmer):
    for name, batch in edge_batches().items():
        want_labels, want_map = batch.label_host(kmer, base_map=True)
        for lead in ((0, 5) if name in ("golden", "event borders at a tile border") else (0,)):
            labels, basemap = replayed(replay, tmp_path, tables_of(batch), kmer, lead=lead)
            assert np.array_equal(labels, want_labels), name
            assert np.array_equal(basemap, want_map), name
    cases = golden_cases()
    for lead in (0, 4, 8):                                           # the golden cases, each labelled with the k it was made with
        for kmer_of in {c["kmer"] for c in cases} if kmer == 5 else ():
            some = [c for c in cases if c["kmer"] == kmer_of]
            batch = EventBatch.from_reads([(c["bases"], c["lengths"], c["clipped"]) for c in some])
            labels, basemap = replayed(replay, tmp_path, tables_of(batch), kmer_of, lead=lead)
            assert np.array_equal(labels, np.concatenate([c["labels"] for c in some]))
            assert np.array_equal(basemap, np.concatenate([c["basemap"] for c in some]))


def test_without_a_base_map_the_labels_are_the_same(replay, tmp_path):
    batch = edge_batches()["the piece border"]
    labels, none = replayed(replay, tmp_path, tables_of(batch), 5, base_map=False)
    assert none is None and np.array_equal(labels, batch.label_host(5))


def vouched(tables, n_events, kmer):
    """What forged tables must give: per read with a sound event range, every event's class (and base) over the samples
    [start, start + max(length, 0)) that lie inside the read, start = the running sum of the lengths that are >= 1; every other sample
    0.  (Reads small enough that no tile meets more events than it stages.)"""
    bases, lengths, event_offsets, clipped, sample_offsets = tables
    labels, basemap = np.zeros(int(sample_offsets[-1]), np.uint8), np.zeros(int(sample_offsets[-1]), np.uint8)
    for r in range(len(event_offsets) - 1):
        e0, e1, s0, s1 = int(event_offsets[r]), int(event_offsets[r + 1]), int(sample_offsets[r]), int(sample_offsets[r + 1])
        if not 0 <= e0 <= e1 <= n_events or e0 == e1:
            continue
        cls = labelling.event_classes_host(bases[e0:e1], int(clipped[r][0]), int(clipped[r][1]), kmer)
        at = 0
        for e in range(e1 - e0):
            n = max(int(lengths[e0 + e]), 0)
            for j in range(at, min(at + n, s1 - s0)):
                labels[s0 + j] = cls[e]
                basemap[s0 + j] = bases[e0 + e] | (0x80 if j == at + n // 2 else 0)
            at = min(at + n, 2 ** 31 - 1)
    return labels, basemap


def test_forged_device_tables(replay, tmp_path):
    reads = [run_read(30, np.arange(30) % 7 + 2, run_at=((3, 9), (20, 26))), run_read(9, [1, 1, 300, 1, 1, 1, 1, 300, 1], run_at=((2, 8),)),
             run_read(50, np.arange(50) % 4 + 1, run_at=((0, 6), (44, 50)), clipped=(2, 2)), run_read(5, [6] * 5, run_at=((0, 5),)),
             run_read(1100, np.arange(1100) % 9 + 1, run_at=((1020, 1030), (500, 505))), run_read(12, [40] * 12, run_at=((4, 10),))]
    batch = EventBatch.from_reads(reads)
    n_events, eo = batch.n_events, batch.event_offsets
    big, small = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    forgeries = []

    def forge(name, what, index, value):
        tables = tables_of(batch)
        tables[what][index] = value
        forgeries.append((name, tables))

    forge("lengths summing past the read", 1, eo[2] + 4, 500)
    forge("lengths summing past the read, at its last event", 1, eo[3] - 1, 9000)
    forge("lengths summing past the read, at its first event", 1, eo[4], 20000)
    forge("lengths summing short", 1, eo[1] + 2, 3)
    forge("lengths summing short, at the last event", 1, eo[6] - 1, 1)
    forge("a zero length", 1, eo[2] + 5, 0)
    forge("a zero length at the piece border", 1, eo[4] + 1023, 0)
    forge("a negative length", 1, eo[2] + 5, -5)
    forge("the most negative length", 1, eo[5] + 3, small)
    forge("a huge length", 1, eo[2] + 1, big)
    forge("an event_offsets entry past n_events", 2, 3, n_events + 5)
    forge("the last event_offsets entry past n_events", 2, 6, n_events + 1)
    forge("a negative event_offsets entry", 2, 0, -1)
    tables = tables_of(batch)
    tables[1][eo[4]:eo[5]] = big                                     # every length of a read huge: the running sum saturates
    forgeries.append(("all lengths huge", tables))
    tables = tables_of(batch)
    tables[1][:] = 0
    forgeries.append(("all lengths zero", tables))
    for name, tables in forgeries:
        for kmer, lead in ((5, 0), (3, 3)):
            labels, basemap = replayed(replay, tmp_path, tables, kmer, lead=lead)      # ... and a silent sanitizer: nothing outside the buffers
            want_labels, want_map = vouched(tables, n_events, kmer)
            assert np.array_equal(labels, want_labels), name         # 0 where no event vouches for the sample, and no sample left unwritten
            assert np.array_equal(basemap, want_map), name
    untouched = batch.label_host(5)
    labels, _ = replayed(replay, tmp_path, forgeries[0][1], 5)
    assert np.array_equal(labels[:batch.sample_offsets[2]], untouched[:batch.sample_offsets[2]])       # the other reads are whole
    assert np.array_equal(labels[batch.sample_offsets[3]:], untouched[batch.sample_offsets[3]:])
    # sample_offsets that are not what the layout promises: that read is not written (the sentinel stays), nothing else is touched
    tables = tables_of(batch)
    tables[4][3] = tables[4][2] - 1
    labels, basemap = replayed(replay, tmp_path, tables, 5)
    assert set(np.unique(labels)) <= {0, 1, SENTINEL}               # (read 3 now begins one sample early, inside read 1)
    assert np.array_equal(labels[:batch.sample_offsets[2] - 1], untouched[:batch.sample_offsets[2] - 1])
    tables = tables_of(batch)
    tables[4][6] = batch.total + 4096
    labels, basemap = replayed(replay, tmp_path, tables, 5, total=batch.total)
    assert (labels[batch.sample_offsets[5]:] == SENTINEL).all() and np.array_equal(labels[:batch.sample_offsets[5]], untouched[:batch.sample_offsets[5]])


def test_refused_arguments(replay, tmp_path):
    batch = edge_batches()["neighbouring reads"]
    assert replayed(replay, tmp_path, tables_of(batch)) is not None
    for change in (dict(kmer=4), dict(kmer=0), dict(kmer=17), dict(kmer=-1), dict(kmer=2 ** 32 + 5), dict(n_reads=-1), dict(n_events=-1),
                   dict(total=-1), dict(n_events=2 ** 31), dict(total=2 ** 31), dict(n_reads=2 ** 23 + 1),
                   dict(work_bytes=5 * batch.n_events - 1), dict(work_bytes=0)):
        assert replayed(replay, tmp_path, tables_of(batch), **change) is None, change
    empty = [np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32), np.zeros(1, np.int64)]
    labels, basemap = replayed(replay, tmp_path, empty)
    assert labels.size == 0 and basemap.size == 0
