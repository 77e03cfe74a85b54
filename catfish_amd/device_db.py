"""Device-resident training set: a balanced sampler a HIP kernel can evaluate per slot.

``train_validate.WindowExampleDb`` draws its batches with Python's generator, on the host, once per step.
``DeviceExampleDb`` keeps the reference sampler's contract (``ExampleDb.get_training_set``,
networks/trainingDB/ExampleDb.py:57-83: ``size // ratio`` DISTINCT positives, the rest DISTINCT negatives, shuffled over
the slots, every window's 35 labels uniform) with a generator of its own that needs no state, no atomics and no
communication, so that ``cf_sample_batch`` (csrc/sample_batch.hpp) draws the same batch inside a captured training step:

* draw number ``d`` (counted from 0, one per batch, whoever asks) and ``seed`` give a 32-bit base key
  ``fmix(seed ^ fmix(d * 0x85ebca6b))`` -- ``fmix`` is the murmur3 finaliser the dropout masks already use;
* ``P(i, n, key)``, a keyed bijection of ``[0, n)``: a balanced four-round Feistel network over ``2^b >= n`` (``b`` even, at
  least 2), round keys ``fmix(key + (r + 1) * 0x9E3779B9)``, round function ``fmix(R ^ k_r)`` masked to ``b / 2`` bits,
  cycle-walking until the value is below ``n``;
* ``rank = P(slot, size, base ^ 1)`` (the shuffle); ranks below ``size // ratio`` are positives, pool row
  ``P(rank, n_pos, base ^ 2)``, the others negatives, pool row ``P(rank - size // ratio, n_neg, base ^ 3)``.

Distinct rows follow from bijectivity.  ``batch_indices`` is this definition in numpy integer arithmetic and is normative: the
kernel reproduces it bit for bit (tests/test_device_db_gpu.py).

The object is host-only until a trainer asks for the pools on a card (``device_pools``); the host's draw counter and the
device's are one number -- whichever side drew last writes it through.

``DeviceReadDb`` is the same sampler over the labelled reads themselves: the reads stay concatenated (float32 signal, uint8 labels,
5 B per sample), a row is an entry of one of two ordered tables of window starts, and a window is ``signal[start : start + 35]``.
``centre_tables`` states in numpy which windows the tables hold -- the reference's selection (``TrainingRead.get_pos`` / ``get_neg``,
networks/trainingDB/TrainingRead.py:226-257; ``ExampleDb.add_training_read`` draws as many negatives as the read has positives),
with the random subset of negatives drawn by the keyed bijection above, so that it is reproducible and a kernel could repeat it.
It is a host database and feeds the per-step loop.  Building the tables and gathering on the card is not in the tree; the index rules
such kernels would follow are (csrc/read_tables_plan.hpp, pieces of ``TABLE_PIECE`` window starts), replayed on the CPU against
``centre_tables`` and ``DeviceReadDb.gather`` (tests/test_read_tables_replay.py).

``DeviceTiledDb`` (opt-in) departs from the reference's selection on purpose: it holds the windows a caller cuts -- every read cut into
consecutive 35-sample windows -- with their true per-sample labels, so that a homopolymer's border lies inside a training window as it
does inside a called one (``tiled_tables`` states which windows).  The sampler above is unchanged; the windows are copied into pools
like ``DeviceExampleDb``'s, with one label byte per sample next to the first pool.  Like ``DeviceReadDb`` it is a host database and
feeds the per-step loop: it has no ``device_pools``.
"""
from __future__ import annotations

import numpy as np

WINDOW = 35
ROUNDS = 4
TABLE_PIECE = 1024                       # window starts per piece of a read's walk (RT_PIECE, csrc/read_tables_plan.hpp)
_U = np.uint32


def fmix32(v):
    """murmur3's 32-bit finaliser (``cf_fmix32`` of the kernels) on a uint32 array."""
    v = np.array(v, dtype=np.uint32, copy=True)
    v ^= v >> _U(16)
    v *= _U(0x85EBCA6B)
    v ^= v >> _U(13)
    v *= _U(0xC2B2AE35)
    v ^= v >> _U(16)
    return v


def keyed_permutation(i, n, key):
    """``P(i, n, key)`` elementwise: ``i`` (values in ``[0, n)``) and ``key`` are uint32 arrays that broadcast against each other."""
    n = int(n)
    if not 0 < n < 2 ** 31:
        raise ValueError("keyed_permutation: n must be in [1, 2^31)")
    bits = max(2, (n - 1).bit_length())
    bits += bits & 1
    half = _U(bits // 2)
    mask = _U((1 << (bits // 2)) - 1)
    i, key = np.broadcast_arrays(np.asarray(i, dtype=np.uint32), np.asarray(key, dtype=np.uint32))
    v = i.reshape(-1).copy()
    key = key.reshape(-1)
    todo = np.arange(v.size)
    with np.errstate(over="ignore"):
        while todo.size:
            k = key[todo]
            cur = v[todo]
            left, right = cur >> half, cur & mask
            for r in range(ROUNDS):
                kr = fmix32(k + _U(((r + 1) * 0x9E3779B9) & 0xFFFFFFFF))
                left, right = right, left ^ (fmix32(right ^ kr) & mask)
            cur = (left << half) | right
            v[todo] = cur
            todo = todo[cur >= n]
    return v.reshape(i.shape)


def draw_indices(seed, draws, size, ratio, n_pos, n_neg):
    """The sampler for a vector of draw numbers: (is_pos bool [len(draws), size], row int64 [len(draws), size])."""
    size, ratio = int(size), int(ratio)
    if size <= 0 or ratio <= 0:
        raise ValueError("batch size and ratio must be positive")
    k_pos = size // ratio
    if k_pos > n_pos or size - k_pos > n_neg:
        raise ValueError("Sample larger than population: %d positives of %d, %d negatives of %d"
                         % (k_pos, n_pos, size - k_pos, n_neg))
    d = (np.asarray(draws, dtype=np.int64).reshape(-1, 1) & 0xFFFFFFFF).astype(np.uint32)
    with np.errstate(over="ignore"):
        base = fmix32(_U(int(seed) & 0xFFFFFFFF) ^ fmix32(d * _U(0x85EBCA6B)))
    slot = np.arange(size, dtype=np.uint32)[None, :]
    rank = keyed_permutation(slot, size, base ^ _U(1))
    is_pos = rank < k_pos
    row = np.zeros(rank.shape, dtype=np.int64)
    keys = np.broadcast_to(base, rank.shape)
    if is_pos.any():
        row[is_pos] = keyed_permutation(rank[is_pos], n_pos, keys[is_pos] ^ _U(2))
    if not is_pos.all():
        row[~is_pos] = keyed_permutation(rank[~is_pos] - _U(k_pos), n_neg, keys[~is_pos] ^ _U(3))
    return is_pos, row


def _pool(windows):
    rows = [np.asarray(w, dtype=np.float32).reshape(-1) for w in windows]
    for r in rows:
        if r.size != WINDOW:
            raise ValueError("DeviceExampleDb holds windows of %d samples, got one of %d" % (WINDOW, r.size))
    return np.stack(rows) if rows else np.zeros((0, WINDOW), np.float32)


class DeviceFedDb(object):
    """What the device-fed training loop needs of a database, whatever a "row" is: the stateless sampler over ``nb_pos`` /
    ``nb_neg`` rows, the per-step surface of ``WindowExampleDb`` and the draw counter shared with the card.  A subclass says
    what a row holds (``gather``) and, when it has a card side, what it keeps there (``device_pools``); one without
    ``device_pools`` is fed by the host."""

    def __init__(self, seed, device=None):
        self.seed = int(seed) & 0xFFFFFFFF
        self.draw = 0                    # number of the NEXT draw
        self.device = device
        self._dev = None                 # what lives on the card, uploaded once; holds "counter"
        self._dev_draw = None            # what the device counter holds once everything enqueued so far has run
        self._last = None                # ("host", x, y) | ("device", x tensor, y tensor, size)

    # ------------------------------------------------------------------ the sampler on the host
    def batch_indices(self, d, size, ratio=2):
        """Draw number ``d`` -> (is_pos bool [size], row int64 [size]): slot ``j`` holds positive row ``row[j]`` when
        ``is_pos[j]``, else negative row ``row[j]``.  Pure integer arithmetic; the sampling kernels compute the same."""
        is_pos, row = draw_indices(self.seed, [int(d)], size, ratio, self.nb_pos, self.nb_neg)
        return is_pos[0], row[0]

    def get_training_set(self, size, ratio=2):
        """``WindowExampleDb.get_training_set``'s shapes for the next draw: (tuple of windows, tuple of label lists, number
        of positive labels); advances the draw counter."""
        x, is_pos = self.gather(self.draw, size, ratio)
        self.draw += 1
        x_out = tuple(x)
        y_out = tuple([1] * WINDOW if p else [0] * WINDOW for p in is_pos.tolist())
        self._last = ("host", x, np.repeat(is_pos.astype(np.int64)[:, None], WINDOW, 1))
        return x_out, y_out, int(is_pos.sum()) * WINDOW

    def skip(self, k):
        """Advance the draw counter by ``k`` without drawing."""
        if int(k) < 0:
            raise ValueError("skip: k must not be negative")
        self.draw += int(k)

    # ------------------------------------------------------------------ the card's side (used by training.Trainer)
    def sync_counter(self):
        """Write the host's draw number through to the device counter when the host moved it (enqueued on the current stream)."""
        if self._dev is not None and self._dev_draw != self.draw:
            self._dev["counter"].fill_(self.draw)
            self._dev_draw = self.draw

    def device_drew(self, k, x, y, size):
        """``k`` draws were enqueued on the card into the static buffers ``x`` / ``y``: the counter moves on for both sides."""
        self.draw += int(k)
        self._dev_draw = self.draw
        self._last = ("device", x, y, int(size))

    def last_batch(self):
        """The batch of the latest draw: (x float32 [size, 35], y int64 [size, 35]); after a device-fed run this copies the
        step's static buffers back (one synchronising copy each)."""
        if self._last is None:
            raise RuntimeError("last_batch: nothing has been drawn yet")
        if self._last[0] == "host":
            return self._last[1], self._last[2]
        _, x, y, size = self._last
        return (x[:size].detach().cpu().numpy().astype(np.float32).reshape(size, WINDOW),
                y[:size].detach().cpu().numpy().astype(np.int64).reshape(size, WINDOW))


class DeviceExampleDb(DeviceFedDb):
    """Two pools of 35-sample windows (``pos``: all-ones labels, ``neg``: all-zeros), float32 ``[n, 35]`` each, and the
    stateless balanced sampler of the module docstring.  A drop-in for ``WindowExampleDb`` (``get_training_set``) and the
    source of ``Trainer.train_steps`` / ``RNN.train_network_steps``, which sample on the card."""

    def __init__(self, pos, neg, seed, device=None):
        DeviceFedDb.__init__(self, seed, device)
        self.pos = _pool(pos)
        self.neg = _pool(neg)
        self.nb_pos, self.nb_neg = int(self.pos.shape[0]), int(self.neg.shape[0])

    @classmethod
    def from_window_db(cls, db, seed, device=None):
        """The pools of a ``train_validate.WindowExampleDb``."""
        return cls(db.pos, db.neg, seed, device)

    def gather(self, d, size, ratio=2):
        """Draw ``d`` as arrays: (x float32 [size, 35], is_pos bool [size])."""
        is_pos, row = self.batch_indices(d, size, ratio)
        x = np.empty((int(size), WINDOW), np.float32)
        x[is_pos] = self.pos[row[is_pos]]
        x[~is_pos] = self.neg[row[~is_pos]]
        return x, is_pos

    def device_pools(self, device=None):
        """(pos tensor [max(n_pos, 1), 35], neg tensor, draw counter int64 [1]) on ``device``; uploaded on the first call."""
        import torch
        device = torch.device(self.device if device is None else device)
        if device.type != "cuda":
            raise ValueError("device_pools: the pools go to a GPU")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev["device"] != device:
            up = lambda a: torch.from_numpy(a if a.shape[0] else np.zeros((1, WINDOW), np.float32)).to(device)     # noqa: E731
            self._dev = {"device": device, "pos": up(self.pos), "neg": up(self.neg),
                         "counter": torch.zeros(1, dtype=torch.int64, device=device)}
            self._dev_draw = 0
        return self._dev["pos"], self._dev["neg"], self._dev["counter"]


def device_db_from_npz(npz_files, width=34, lessen=1, max_neg_per_read=2000, seed=0, device=None, loader=None):
    """``train_validate.example_db_from_npz``'s windows (the same selection code, the same ``loader``) in a ``DeviceExampleDb``."""
    from .train_validate import example_db_from_npz
    return DeviceExampleDb.from_window_db(example_db_from_npz(npz_files, width, lessen, max_neg_per_read, seed, loader), seed, device)


def synthetic_device_db(n_reads=8, read_len=20000, seed=0, device=None):
    """``train_validate.synthetic_example_db``'s windows in a ``DeviceExampleDb``."""
    from .train_validate import synthetic_example_db
    return DeviceExampleDb.from_window_db(synthetic_example_db(n_reads, read_len, seed), seed, device)


# --------------------------------------------------------------------------- the training set from the labelled reads themselves
def _neg_quota(neg_per_read, m, n_pos):
    """How many of a read's ``m`` candidates become negatives when the read has ``n_pos`` positives."""
    if neg_per_read is None:
        return m
    if isinstance(neg_per_read, str):
        if neg_per_read != "positives":
            raise ValueError("neg_per_read: None, an int or 'positives', got %r" % (neg_per_read,))
        return min(m, n_pos)
    if isinstance(neg_per_read, (bool, np.bool_)) or int(neg_per_read) != neg_per_read or int(neg_per_read) < 0:
        raise ValueError("neg_per_read: None, a non-negative int or 'positives', got %r" % (neg_per_read,))
    return min(m, int(neg_per_read))


def _read_layout(labels, offsets, lessen):
    labels = np.asarray(labels)
    if labels.dtype != np.uint8 or labels.ndim != 1:
        raise ValueError("labels: one uint8 array over all reads")
    if labels.size and labels.max() > 1:
        raise ValueError("labels must be 0 or 1")
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != labels.size or np.any(np.diff(offsets) < 0):
        raise ValueError("offsets: int64 [n_reads + 1], ascending from 0 to the number of samples")
    if int(lessen) != lessen or int(lessen) < 1:
        raise ValueError("lessen must be a positive int")
    return labels, offsets, int(lessen)


def centre_tables(labels, offsets, lessen=1, neg_per_read=None, seed=0):
    """Which windows of the concatenated reads (``labels`` uint8 [total], ``offsets`` int64 [R + 1], the layout of
    ``DeviceValidationSet.from_arrays``) are training examples -> (pos_start int64 [], neg_start int64 []): the index of each
    window's first sample, in (read, centre) order.

    For read ``rho`` of ``n`` samples the centres are ``c`` in ``[17, n - 17)``, ascending.  The centres with label 1 are
    numbered k = 0, 1, ...; centre k is a positive iff ``k % lessen == 0`` and all 35 labels of ``[c - 17, c + 17]`` are 1
    (``TrainingRead.get_pos``: the numbering runs over ALL label-1 centres).  The centres whose 35 labels are all 0 are the
    candidates, numbered j = 0 .. m - 1; the read contributes q of them: ``neg_per_read=None`` q = m, an int q = min(m, it),
    ``"positives"`` q = min(m, the read's positives) (the reference's rule).  Candidate j is a negative iff q == m or
    ``keyed_permutation(j, m, key) < q`` with ``key = fmix32(seed ^ fmix32((rho + 1) * 0x9E3779B9))`` -- a bijection, so exactly
    q are.  A read shorter than 35 samples contributes nothing."""
    labels, offsets, lessen = _read_layout(labels, offsets, lessen)
    _neg_quota(neg_per_read, 0, 0)                                       # a bad rule is refused even when no read has a candidate
    seed = _U(int(seed) & 0xFFFFFFFF)
    running = np.zeros(labels.size + 1, dtype=np.int64)
    np.cumsum(labels, out=running[1:])
    pos, neg = [], []
    for rho in range(offsets.size - 1):
        o, n = int(offsets[rho]), int(offsets[rho + 1] - offsets[rho])
        if n < WINDOW:
            continue
        first = o + np.arange(n - WINDOW + 1, dtype=np.int64)            # the window of centre c starts at o + c - 17
        ones = running[first + WINDOW] - running[first]
        hits = np.flatnonzero(labels[first + WINDOW // 2] == 1)[::lessen]       # every lessen-th label-1 centre ...
        hits = hits[ones[hits] == WINDOW]                                # ... whose whole window is ones
        pos.append(first[hits])
        cand = np.flatnonzero(ones == 0)
        neg.append(first[_quota_subset(cand, _neg_quota(neg_per_read, cand.size, hits.size), rho, seed)])
    empty = np.zeros(0, dtype=np.int64)
    return (np.concatenate(pos) if pos else empty), (np.concatenate(neg) if neg else empty)


def _quota_subset(cand, q, rho, seed):
    """Which of read ``rho``'s ``m`` candidates (in order) are kept when ``q`` of them are: all for q == m, else candidate j iff
    ``keyed_permutation(j, m, key) < q`` with ``key = fmix32(seed ^ fmix32((rho + 1) * 0x9E3779B9))`` (``seed`` a uint32)."""
    m = cand.size
    if q < m:
        with np.errstate(over="ignore"):
            key = fmix32(seed ^ fmix32(_U(((rho + 1) * 0x9E3779B9) & 0xFFFFFFFF)))
        cand = cand[keyed_permutation(np.arange(m, dtype=np.uint32), m, key) < q]
    return cand


def _table_sizes_fit(n_pos, n_neg, advice="raise lessen or cap neg_per_read"):
    """``keyed_permutation`` draws rows from [0, n) with n below 2^31."""
    if n_pos >= 2 ** 31 or n_neg >= 2 ** 31:
        raise ValueError("a table of 2^31 or more windows (%d positives, %d negatives): %s" % (n_pos, n_neg, advice))


class DeviceReadDb(DeviceFedDb):
    """The labelled reads themselves as the training set: ``signal`` float32 [total] (cast once), ``labels`` uint8 [total],
    ``offsets`` int64 [n_reads + 1], and two ordered tables of window starts (``centre_tables``).  The sampler and the public
    surface are ``DeviceExampleDb``'s; row ``i`` of the positives is the window ``signal[pos_start[i] : pos_start[i] + 35]``.

    The tables are computed on first use (``pos_start``, ``neg_start``, ``nb_pos``, ``nb_neg``, ``gather``).  Despite its
    place in this module this is a HOST database: nothing of it goes to a card.  It has no ``device_pools``, so
    ``Trainer.train_steps`` / ``RNN.train_network_steps`` and ``train_and_validate`` run it through ``get_training_set`` + one
    host-fed step per batch, on a GPU as on the CPU -- the same steps on the same batches, slower per step than a
    ``DeviceExampleDb``."""

    def __init__(self, signal, labels, offsets, seed, lessen=1, neg_per_read=None):
        DeviceFedDb.__init__(self, seed)
        self.labels, self.offsets, self.lessen = _read_layout(labels, offsets, lessen)
        self.signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1)
        if self.signal.size != self.labels.size:
            raise ValueError("%d samples but %d labels" % (self.signal.size, self.labels.size))
        _neg_quota(neg_per_read, 0, 0)
        self.neg_per_read = neg_per_read
        self._tables = None              # (pos_start, neg_start)

    @classmethod
    def from_arrays(cls, signals, labels, seed=0, lessen=1, neg_per_read=None):
        """One read per (signal, labels) pair, in that order."""
        from .device_validation import DeviceValidationSet
        v = DeviceValidationSet.from_arrays(signals, labels)
        return cls(v.signal, v.labels, v.offsets, seed, lessen, neg_per_read)

    @classmethod
    def from_npz(cls, paths, seed=0, lessen=1, neg_per_read=None, loader=None):
        """The reads of ``paths`` (``raw`` + ``base_labels``, ``train_validate.load_npz``), in that order."""
        from .device_validation import DeviceValidationSet
        v = DeviceValidationSet.from_npz(paths, loader)
        return cls(v.signal, v.labels, v.offsets, seed, lessen, neg_per_read)

    @classmethod
    def from_source(cls, paths, source, seed=0, lessen=1, neg_per_read=None, device=None):
        """The reads of ``paths``, in that order, as ``source`` (a ``labelling.LabelSource``) says they are stored, labelled through
        ``DeviceValidationSet.from_source`` (event and move files on the card where there is one)."""
        from .device_validation import DeviceValidationSet
        v = DeviceValidationSet.from_source(paths, source, device)
        return cls(v.signal, v.labels, v.offsets, seed, lessen, neg_per_read)

    @classmethod
    def from_event_npz(cls, paths, kmer=5, seed=0, lessen=1, neg_per_read=None, device=None):
        from .labelling import LabelSource
        return cls.from_source(paths, LabelSource("events", kmer), seed, lessen, neg_per_read, device)

    @classmethod
    def from_move_npz(cls, paths, seed=0, lessen=1, neg_per_read=None, device=None):
        from .labelling import LabelSource
        return cls.from_source(paths, LabelSource("moves"), seed, lessen, neg_per_read, device)

    # ------------------------------------------------------------------ the tables
    def host_tables(self):
        if self._tables is None:
            pos, neg = centre_tables(self.labels, self.offsets, self.lessen, self.neg_per_read, self.seed)
            _table_sizes_fit(pos.size, neg.size)
            self._tables = (pos, neg)
        return self._tables

    pos_start = property(lambda self: self.host_tables()[0])
    neg_start = property(lambda self: self.host_tables()[1])
    nb_pos = property(lambda self: int(self.host_tables()[0].size))
    nb_neg = property(lambda self: int(self.host_tables()[1].size))

    def gather(self, d, size, ratio=2):
        """Draw ``d`` as arrays: (x float32 [size, 35], is_pos bool [size])."""
        is_pos, row = self.batch_indices(d, size, ratio)
        pos, neg = self.host_tables()
        start = np.empty(int(size), dtype=np.int64)
        start[is_pos] = pos[row[is_pos]]
        start[~is_pos] = neg[row[~is_pos]]
        return self.signal[start[:, None] + np.arange(WINDOW)], is_pos


def synthetic_device_read_db(n_reads=8, read_len=20000, seed=0, lessen=1, neg_per_read=None):
    """``train_validate.synthetic_example_db``'s reads (the same squiggles) in a ``DeviceReadDb``."""
    from .train_validate import synthetic_labelled_read
    reads = [synthetic_labelled_read(read_len, seed * 1000 + r) for r in range(n_reads)]
    return DeviceReadDb.from_arrays([raw for raw, _ in reads], [lab for _, lab in reads], seed, lessen, neg_per_read)


# --------------------------------------------------------------------------- the windows the caller cuts, with their per-sample labels
def _miss_quota(miss_per_read, m, n_hit):
    """``_neg_quota`` with the tiled selection's name for the reference's rule: ``"hits"`` keeps as many misses as the read has hits."""
    if isinstance(miss_per_read, str):
        if miss_per_read != "hits":
            raise ValueError("miss_per_read: None, an int or 'hits', got %r" % (miss_per_read,))
        return min(m, n_hit)
    return _neg_quota(miss_per_read, m, n_hit)


def _check_stride(stride):
    if isinstance(stride, (bool, np.bool_)) or not isinstance(stride, (int, np.integer)) or int(stride) < 1:
        raise ValueError("stride must be an int of at least 1, got %r" % (stride,))
    return int(stride)


def tiled_tables(labels, offsets, stride=WINDOW, miss_per_read=None, seed=0):
    """Which windows of the concatenated reads (the layout of ``centre_tables``) a caller that cuts every read into consecutive
    windows would see -> (hit_start int64 [], miss_start int64 []): the index of each window's first sample, in (read, start) order.

    For read ``rho`` of ``n`` samples at offset ``o`` the windows start at ``o + k * stride``, k = 0, 1, ... while
    ``k * stride + 35 <= n``: none is padded, none straddles two reads, a read shorter than 35 samples contributes nothing.
    ``stride`` 35 is the caller's own grid, 1 gives every window.  A window with at least one label 1 is a hit, one with none a miss.
    Of a read's ``m`` misses q are kept: ``miss_per_read=None`` q = m, an int q = min(m, it), ``"hits"`` q = min(m, the read's hits);
    which ones is ``centre_tables``' rule for its negatives (``_quota_subset``: the same key, the same ``keyed_permutation``, ``< q``).
    Tables of 2^31 rows or more are refused.

    This is NOT the reference's selection (``TrainingRead.get_pos`` / ``get_neg`` keep only windows whose 35 labels are all equal):
    a hit here may hold a homopolymer's border, and the labels of a hit are the read's own, sample by sample."""
    labels, offsets, _ = _read_layout(labels, offsets, 1)
    stride = _check_stride(stride)
    _miss_quota(miss_per_read, 0, 0)                                      # a bad rule is refused even when no read has a candidate
    seed = _U(int(seed) & 0xFFFFFFFF)
    running = np.zeros(labels.size + 1, dtype=np.int64)
    np.cumsum(labels, out=running[1:])
    hit, miss = [], []
    for rho in range(offsets.size - 1):
        o, n = int(offsets[rho]), int(offsets[rho + 1] - offsets[rho])
        if n < WINDOW:
            continue
        first = o + np.arange(0, n - WINDOW + 1, stride, dtype=np.int64)
        ones = running[first + WINDOW] - running[first]
        hits = np.flatnonzero(ones > 0)
        hit.append(first[hits])
        cand = np.flatnonzero(ones == 0)
        miss.append(first[_quota_subset(cand, _miss_quota(miss_per_read, cand.size, hits.size), rho, seed)])
    empty = np.zeros(0, dtype=np.int64)
    hit, miss = (np.concatenate(hit) if hit else empty), (np.concatenate(miss) if miss else empty)
    _table_sizes_fit(hit.size, miss.size, "raise stride or cap miss_per_read")
    return hit, miss


class DeviceTiledDb(DeviceFedDb):
    """The windows of ``tiled_tables`` copied into pools, as ``DeviceExampleDb`` keeps its windows: ``pos`` float32 [n_hit, 35] with
    ``pos_labels`` uint8 [n_hit, 35] (the read's own labels: a hit may hold a border) and ``neg`` float32 [n_miss, 35], whose labels
    are all zero by construction.  The sampler is ``draw_indices``, unchanged: ``size // ratio`` distinct hits and the remaining
    distinct misses, shuffled over the slots.  A HOST database, like ``DeviceReadDb``: it has no ``device_pools``, so
    ``Trainer.train_steps`` / ``RNN.train_network_steps`` and ``train_and_validate`` run it through ``get_training_set`` + one
    host-fed step per batch, on a GPU as on the CPU, and the per-sample labels arrive through ``train_step``'s ``y``."""

    def __init__(self, pos, pos_labels, neg, seed, device=None):
        DeviceFedDb.__init__(self, seed, device)
        self.pos = _pool(pos)
        self.neg = _pool(neg)
        lab = np.asarray(pos_labels)
        if lab.dtype != np.uint8 or lab.shape != self.pos.shape:
            raise ValueError("pos_labels must be uint8 %s, got %s %s" % (self.pos.shape, lab.dtype, lab.shape))
        if lab.size and lab.max() > 1:
            raise ValueError("labels must be 0 or 1")
        self.pos_labels = np.ascontiguousarray(lab)
        self.nb_pos, self.nb_neg = int(self.pos.shape[0]), int(self.neg.shape[0])
        _table_sizes_fit(self.nb_pos, self.nb_neg, "raise stride or cap miss_per_read")

    @classmethod
    def from_layout(cls, signal, labels, offsets, seed=0, stride=WINDOW, miss_per_read=None, device=None):
        """The pools of concatenated reads (``signal`` [total], ``labels`` uint8 [total], ``offsets`` int64 [R + 1])."""
        hit, miss = tiled_tables(labels, offsets, stride, miss_per_read, seed)
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1)
        labels = np.asarray(labels)
        if signal.size != labels.size:
            raise ValueError("%d samples but %d labels" % (signal.size, labels.size))
        span = np.arange(WINDOW)
        return cls(signal[hit[:, None] + span], labels[hit[:, None] + span], signal[miss[:, None] + span], seed, device)

    @classmethod
    def from_arrays(cls, signals, labels, seed=0, stride=WINDOW, miss_per_read=None, device=None):
        """One read per (signal, labels) pair, in that order."""
        from .device_validation import DeviceValidationSet
        v = DeviceValidationSet.from_arrays(signals, labels)
        return cls.from_layout(v.signal, v.labels, v.offsets, seed, stride, miss_per_read, device)

    @classmethod
    def from_npz(cls, paths, seed=0, stride=WINDOW, miss_per_read=None, loader=None, device=None):
        """The reads of ``paths`` (``raw`` + ``base_labels``, ``train_validate.load_npz``), in that order."""
        from .device_validation import DeviceValidationSet
        v = DeviceValidationSet.from_npz(paths, loader)
        return cls.from_layout(v.signal, v.labels, v.offsets, seed, stride, miss_per_read, device)

    @classmethod
    def from_source(cls, paths, source, seed=0, stride=WINDOW, miss_per_read=None, device=None):
        """The reads of ``paths``, in that order, as ``source`` (a ``labelling.LabelSource``) says they are stored, labelled through
        ``DeviceValidationSet.from_source`` (event and move files on the card where there is one)."""
        from .device_validation import DeviceValidationSet
        v = DeviceValidationSet.from_source(paths, source, device)
        return cls.from_layout(v.signal, v.labels, v.offsets, seed, stride, miss_per_read, device)

    # ------------------------------------------------------------------ the sampler on the host
    def gather(self, d, size, ratio=2):
        """Draw ``d`` as arrays: (x float32 [size, 35], y uint8 [size, 35]) -- the labels are the windows' own."""
        is_pos, row = self.batch_indices(d, size, ratio)
        x = np.empty((int(size), WINDOW), np.float32)
        y = np.zeros((int(size), WINDOW), np.uint8)
        x[is_pos] = self.pos[row[is_pos]]
        y[is_pos] = self.pos_labels[row[is_pos]]
        x[~is_pos] = self.neg[row[~is_pos]]
        return x, y

    def get_training_set(self, size, ratio=2):
        """``WindowExampleDb.get_training_set``'s shapes for the next draw: (tuple of windows, tuple of label lists -- the true
        per-sample labels --, number of 1 labels); advances the draw counter."""
        x, y = self.gather(self.draw, size, ratio)
        self.draw += 1
        y = y.astype(np.int64)
        self._last = ("host", x, y)
        return tuple(x), tuple(y.tolist()), int(y.sum())


def synthetic_device_tiled_db(n_reads=8, read_len=20000, seed=0, stride=WINDOW, miss_per_read=None, device=None):
    """``train_validate.synthetic_example_db``'s reads (the same squiggles) in a ``DeviceTiledDb``."""
    from .train_validate import synthetic_labelled_read
    reads = [synthetic_labelled_read(read_len, seed * 1000 + r) for r in range(n_reads)]
    return DeviceTiledDb.from_arrays([raw for raw, _ in reads], [lab for _, lab in reads], seed, stride, miss_per_read, device)
