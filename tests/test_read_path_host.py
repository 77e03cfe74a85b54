"""The read path's host rules (no GPU): how many windows a read occupies, the offset tables of a packed batch, the in-flight
driver, and the file-batch walk of ``sharding.EngineBatchRunner`` over a recording stand-in for ``ReadPipeline`` -- order of
results, at most one preload pending, none while the general loader runs, the re-cut of a refused batch, and every preload
launched or dropped however the walk ends.  The walk's tests were written against the code before it was gathered into one walk
and passed there unchanged."""
import os

import numpy as np
import pytest

from catfish_amd import batching, infer, sharding


# ------------------------------------------------------------------ the window rule, the tables of a batch, the in-flight driver
def test_windows_of_is_the_reference_padding_rule():
    ns = list(range(5001)) + [4095, 4096, 16384, 40000]
    want = [(n + infer.padding_size_for(n)) // 35 for n in ns]
    assert batching.windows_of(ns).tolist() == want
    assert [sharding.windows_of(n) for n in ns] == want and type(sharding.windows_of(70)) is int
    assert [sharding._padded(n) for n in (0, 34, 35, 36, 4096)] == [35, 35, 70, 70, 4130]
    # another window keeps going through padding_size_for, with its literal 35 for a multiple of ANY window
    assert [sharding.windows_of(n, 10) for n in (0, 9, 10, 11, 20)] == [3, 1, 4, 2, 5]
    packed = batching.pack_reads([np.ones(n) for n in (9, 11)], window=10)
    assert packed.win_offsets.tolist() == [0, 1, 3] and packed.x.shape == (3, 10)
    assert batching.length_buckets([9, 11, 21, 5], 3, window=10) == [[2], [1, 0], [3]]


def test_sample_hints_from_file_sizes():
    # computed once at the commit before the rule was gathered in one place
    assert sharding._sample_hints([0, 128, 129, 130, 198, 200, 8320]).tolist() == [35, 35, 35, 35, 70, 70, 4130]


@pytest.mark.parametrize("lengths, dac_off, win_off, s_off", [
    ([], [0], [0], [0]),
    ([0], [0, 0], [0, 1], [0, 35]),
    ([1], [0, 1], [0, 1], [0, 35]),
    ([34, 35, 36], [0, 34, 69, 105], [0, 1, 3, 5], [0, 35, 105, 175]),
    ([70, 0, 4096], [0, 70, 70, 4166], [0, 3, 4, 122], [0, 105, 140, 4270]),
])
def test_batch_tables(lengths, dac_off, win_off, s_off):
    t = batching.batch_tables(lengths)
    assert all(a.dtype == np.int64 for a in t[:4])
    assert [a.tolist() for a in t[:4]] == [dac_off, win_off, s_off, lengths]
    assert (t.n_windows, t.n_samples) == (win_off[-1], s_off[-1]) and type(t.n_windows) is int


@pytest.mark.parametrize("depth", (1, 2, 3))
def test_in_flight_finishes_in_order_and_holds_at_most_depth(depth):
    pulled, finished = [], []

    def items():
        for i in range(7):
            assert len(pulled) - len(finished) < depth          # never more than ``depth`` pulled and unfinished
            pulled.append(i)
            yield i

    def finish(i):
        finished.append(i)
        return 10 * i
    walk = batching.in_flight(items(), depth, finish)
    assert pulled == []                                          # lazy: nothing is submitted before the first result is asked for
    assert list(walk) == [10 * i for i in range(7)] and finished == list(range(7))
    assert list(batching.in_flight(iter(()), depth, finish)) == []


@pytest.mark.parametrize("depth", (1, 2, 3))
def test_in_flight_pulls_nothing_after_finish_raises(depth):
    pulled = []

    def items():
        for i in range(7):
            pulled.append(i)
            yield i

    def finish(i):
        if i == 2:
            raise RuntimeError("batch 2 failed")
        return i
    walk = batching.in_flight(items(), depth, finish)
    assert [next(walk), next(walk)] == [0, 1]
    with pytest.raises(RuntimeError, match="batch 2 failed"):
        next(walk)
    assert pulled == list(range(2 + depth))                      # what was in flight when batch 2 failed, and no more
    assert list(walk) == [] and pulled == list(range(2 + depth))


# ------------------------------------------------------------------ the file walk of EngineBatchRunner over a stand-in pipeline
MAX_SAMPLES = 1000
# five batches of files by read length; the stand-in pipeline refuses the third, whose reads (padded: 420, 420, 420, 1505) the
# general loader must re-cut into [400, 400], [400] and the single read that is larger than a batch on its own
BATCH_LENGTHS = ((100, 200), (300,), (400, 400, 400, 1500), (50, 60, 70), (800,))
REFUSED = 2


class _FakeListing(object):
    """What ``sharding.ListingPaths`` asks of a ``DirListing``."""

    def __init__(self, directory, names):
        self.directory, self._names = directory, names

    def __len__(self):
        return len(self._names)

    def names(self, lo, hi):
        return self._names[lo:hi]


class _FakePipeline(object):
    """Records every call; a ticket is the batch's result, ``[(first sample, length)]`` per read.  It checks what the real
    pipeline relies on: one preload at a time, nothing submitted while one is pending, at most ``depth`` batches uncollected."""

    def __init__(self, refuse, depth=2, fail_launch_of=None):
        self.depth, self.refuse, self.fail_launch_of = depth, refuse, fail_launch_of
        self.calls, self.pending, self.uncollected, self.preloads, self.settled = [], None, 0, [], []

    @staticmethod
    def _result(reads):
        return [(int(r[0]), len(r)) for r in reads]

    def _ticket(self, reads):
        self.uncollected += 1
        assert self.uncollected <= self.depth
        return {"result": self._result(reads)}

    def submit(self, reads):
        assert self.pending is None, "a batch was submitted while a preload was pending"
        self.calls.append(("submit", [len(r) for r in reads]))
        return self._ticket(reads)

    def submit_files(self, paths):
        assert self.pending is None
        self.calls.append(("submit_files", [os.path.basename(p) for p in paths]))
        if tuple(paths) in self.refuse:
            return None
        return self._ticket([np.load(p) for p in paths])

    def preload_listing(self, listing, lo, hi):
        assert self.pending is None, "two preloads pending"
        self.calls.append(("preload_listing", lo, hi))
        self.pending = (listing, lo, hi)
        self.preloads.append(self.pending)
        return self.pending

    def launch_preloaded(self, pre):
        assert pre is not None and pre is self.pending, "launched something other than the pending preload"
        listing, lo, hi = pre
        self.calls.append(("launch_preloaded", lo, hi))
        self.pending = None
        self.settled.append(pre)
        if self.fail_launch_of == (lo, hi):
            raise RuntimeError("launch failed")
        if (lo, hi) in self.refuse:
            return None
        return self._ticket([np.load(os.path.join(listing.directory, n)) for n in listing.names(lo, hi)])

    def drop_preloaded(self, pre):
        self.calls.append(("drop_preloaded", None if pre is None else pre[1:]))
        if pre is not None:
            assert pre is self.pending
            self.pending = None
            self.settled.append(pre)

    def collect(self, ticket):
        self.calls.append(("collect",))
        self.uncollected -= 1
        return ticket["result"]


@pytest.fixture()
def read_files(tmp_path):
    """The files of BATCH_LENGTHS (read i holds i + 1 everywhere) -> (directory, names, ranges, lengths)."""
    names, ranges, lengths = [], [], []
    for batch in BATCH_LENGTHS:
        lo = len(names)
        for n in batch:
            names.append("read_%02d.npy" % len(names))
            np.save(str(tmp_path / names[-1]), np.full(n, len(names), dtype=np.int16))
            lengths.append(n)
        ranges.append((lo, len(names)))
    return str(tmp_path), names, ranges, lengths


def _runner(pipe):
    runner = sharding.EngineBatchRunner.__new__(sharding.EngineBatchRunner)      # no engine, no GPU: only what the walk uses
    runner.pipe, runner.max_samples = pipe, MAX_SAMPLES
    return runner


def _watch_loader(monkeypatch, pipe):
    """``infer.load_dac`` with a look at the pipeline first: nothing may be preloading while the general loader runs."""
    real, loaded = infer.load_dac, []

    def load_dac(path):
        assert pipe.pending is None, "a preload was pending while the general loader ran"
        loaded.append(os.path.basename(path))
        return real(path)
    monkeypatch.setattr(infer, "load_dac", load_dac)
    return loaded


def _expected_results(ranges, lengths):
    """One item per submitted batch, in order: the refused range arrives as its re-cut pieces."""
    reads = [(i + 1, n) for i, n in enumerate(lengths)]
    out = []
    for k, (lo, hi) in enumerate(ranges):
        if k == REFUSED:
            out += [reads[lo:lo + 2], reads[lo + 2:lo + 3], reads[lo + 3:hi]]
        else:
            out.append(reads[lo:hi])
    return out


def _check_recut(pipe):
    submits = [c[1] for c in pipe.calls if c[0] == "submit"]
    assert submits == [[400, 400], [400], [1500]]
    for batch in submits:
        assert len(batch) == 1 or sum(sharding._padded(n) for n in batch) <= MAX_SAMPLES


def test_listing_walk_preloads_one_ahead_and_recuts_a_refused_batch(read_files, monkeypatch):
    directory, names, ranges, lengths = read_files
    pipe = _FakePipeline(refuse={ranges[REFUSED]})
    loaded = _watch_loader(monkeypatch, pipe)
    paths = sharding.ListingPaths(_FakeListing(directory, names))
    got = list(_runner(pipe).run_listing(paths, iter(ranges)))
    assert got == _expected_results(ranges, lengths)
    assert loaded == names[ranges[REFUSED][0]:ranges[REFUSED][1]]              # the general loader saw the refused batch only
    _check_recut(pipe)
    assert [p[1:] for p in pipe.preloads] == ranges                             # every range was preloaded, once, in order
    assert pipe.settled == pipe.preloads and pipe.pending is None and pipe.uncollected == 0
    # a preload starts right after the launch before it, ahead of that batch's collect; after a refused batch, after its re-cut
    order = [c for c in pipe.calls if c[0] in ("preload_listing", "launch_preloaded", "submit")]
    assert order == [("preload_listing",) + ranges[0], ("launch_preloaded",) + ranges[0],
                     ("preload_listing",) + ranges[1], ("launch_preloaded",) + ranges[1],
                     ("preload_listing",) + ranges[2], ("launch_preloaded",) + ranges[2],
                     ("submit", [400, 400]), ("submit", [400]), ("submit", [1500]),
                     ("preload_listing",) + ranges[3], ("launch_preloaded",) + ranges[3],
                     ("preload_listing",) + ranges[4], ("launch_preloaded",) + ranges[4]]


@pytest.mark.parametrize("stop_after", (1, 2))
def test_listing_walk_drops_its_preload_when_the_consumer_stops(read_files, monkeypatch, stop_after):
    """Closed after the first result the third range is being preloaded (and must be dropped); after the second the walk is in
    the middle of the refused batch's re-cut and nothing is."""
    directory, names, ranges, lengths = read_files
    pipe = _FakePipeline(refuse={ranges[REFUSED]})
    _watch_loader(monkeypatch, pipe)
    walk = _runner(pipe).run_listing(sharding.ListingPaths(_FakeListing(directory, names)), iter(ranges))
    got = [next(walk) for _ in range(stop_after)]
    walk.close()
    del walk
    assert got == _expected_results(ranges, lengths)[:stop_after]
    assert [p[1:] for p in pipe.preloads] == ranges[:3] and pipe.pending is None
    assert sorted(p[1:] for p in pipe.settled) == ranges[:3]
    if stop_after == 1:
        assert pipe.calls[-1] == ("drop_preloaded", ranges[2])


def test_listing_walk_leaves_no_preload_behind_when_a_launch_raises(read_files, monkeypatch):
    directory, names, ranges, lengths = read_files
    pipe = _FakePipeline(refuse={ranges[REFUSED]}, fail_launch_of=ranges[3])
    _watch_loader(monkeypatch, pipe)
    walk = _runner(pipe).run_listing(sharding.ListingPaths(_FakeListing(directory, names)), iter(ranges))
    got = []
    with pytest.raises(RuntimeError, match="launch failed"):
        for res in walk:
            got.append(res)
    assert got == _expected_results(ranges, lengths)[:len(got)] and len(got) >= 2
    assert [p[1:] for p in pipe.preloads] == ranges[:4] and pipe.settled == pipe.preloads and pipe.pending is None


def test_files_walk_recuts_a_refused_batch_and_never_preloads(read_files, monkeypatch):
    directory, names, ranges, lengths = read_files
    batches = [[os.path.join(directory, n) for n in names[lo:hi]] for lo, hi in ranges]
    pipe = _FakePipeline(refuse={tuple(batches[REFUSED])})
    loaded = _watch_loader(monkeypatch, pipe)
    got = list(_runner(pipe).run_files(iter(batches)))
    assert got == _expected_results(ranges, lengths)
    assert loaded == names[ranges[REFUSED][0]:ranges[REFUSED][1]]
    _check_recut(pipe)
    assert not pipe.preloads and pipe.uncollected == 0
    order = [c for c in pipe.calls if c[0] in ("submit_files", "submit")]
    assert order == [("submit_files", names[lo:hi]) for lo, hi in ranges[:3]] + [
        ("submit", [400, 400]), ("submit", [400]), ("submit", [1500])] + [("submit_files", names[lo:hi]) for lo, hi in ranges[3:]]
