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
"""
from __future__ import annotations

import numpy as np

WINDOW = 35
ROUNDS = 4
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


class DeviceExampleDb(object):
    """Two pools of 35-sample windows (``pos``: all-ones labels, ``neg``: all-zeros), float32 ``[n, 35]`` each, and the
    stateless balanced sampler of the module docstring.  A drop-in for ``WindowExampleDb`` (``get_training_set``) and the
    source of ``Trainer.train_steps`` / ``RNN.train_network_steps``, which sample on the card."""

    def __init__(self, pos, neg, seed, device=None):
        self.pos = _pool(pos)
        self.neg = _pool(neg)
        self.nb_pos, self.nb_neg = int(self.pos.shape[0]), int(self.neg.shape[0])
        self.seed = int(seed) & 0xFFFFFFFF
        self.draw = 0                    # number of the NEXT draw
        self.device = device
        self._dev = None                 # {"pos", "neg", "counter"} on the card, uploaded once
        self._dev_draw = None            # what the device counter holds once everything enqueued so far has run
        self._last = None                # ("host", x, y) | ("device", x tensor, y tensor, size)

    @classmethod
    def from_window_db(cls, db, seed, device=None):
        """The pools of a ``train_validate.WindowExampleDb``."""
        return cls(db.pos, db.neg, seed, device)

    # ------------------------------------------------------------------ the sampler on the host
    def batch_indices(self, d, size, ratio=2):
        """Draw number ``d`` -> (is_pos bool [size], row int64 [size]): slot ``j`` holds ``pos[row[j]]`` when ``is_pos[j]``,
        else ``neg[row[j]]``.  Pure integer arithmetic; ``cf_sample_batch`` computes the same."""
        is_pos, row = draw_indices(self.seed, [int(d)], size, ratio, self.nb_pos, self.nb_neg)
        return is_pos[0], row[0]

    def gather(self, d, size, ratio=2):
        """Draw ``d`` as arrays: (x float32 [size, 35], is_pos bool [size])."""
        is_pos, row = self.batch_indices(d, size, ratio)
        x = np.empty((int(size), WINDOW), np.float32)
        x[is_pos] = self.pos[row[is_pos]]
        x[~is_pos] = self.neg[row[~is_pos]]
        return x, is_pos

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


def device_db_from_npz(npz_files, width=34, lessen=1, max_neg_per_read=2000, seed=0, device=None):
    """``train_validate.example_db_from_npz``'s windows (the same selection code) in a ``DeviceExampleDb``."""
    from .train_validate import example_db_from_npz
    return DeviceExampleDb.from_window_db(example_db_from_npz(npz_files, width, lessen, max_neg_per_read, seed), seed, device)


def synthetic_device_db(n_reads=8, read_len=20000, seed=0, device=None):
    """``train_validate.synthetic_example_db``'s windows in a ``DeviceExampleDb``."""
    from .train_validate import synthetic_example_db
    return DeviceExampleDb.from_window_db(synthetic_example_db(n_reads, read_len, seed), seed, device)
