"""Device-resident validation set: the reads of a run's checkpoint rounds, uploaded once, packed and scored on the card.

``train_validate.validate`` on a list of NPZ paths re-opens every file per round, packs the stretches in numpy, copies the batch
to the card, copies probabilities and logits back and scores them in numpy.  ``DeviceValidationSet`` keeps all reads on the
card (float32 signal, uint8 labels); a round then uploads three short int64 arrays (which stretch of which read), and two HIP
launches around the forward pass do the rest (csrc/validation.hpp): ``cf_validation_gather`` packs the window-major batch,
``cf_validation_score`` returns raw integer counts and double sums, and the host finishes with the divisions
``train_validate.score_validation_batch`` uses.

Every random draw stays on the host, on Python's global generator and in the reference's order
(networks/train_validate.py:214-249), so a seeded round selects the stretches the host route selects.

This module states both device steps in numpy and those statements are normative: ``DeviceValidationSet.pack`` is what the
gather kernel writes (bit for bit), ``score_host`` what the scoring kernel returns (counts exactly; the double sums up to the
summation order).  The object is host-only until ``device_arrays`` is called and usable without a GPU.
"""
from __future__ import annotations

import random

import numpy as np

SCORE_CHUNK = 2048          # samples one workgroup of the scoring kernel reduces (CF_SCORE_CHUNK, csrc/validation.hpp)
MAX_THRESHOLDS = 16         # thresholds per scoring launch (CF_SCORE_MAX_K)


def _as_labels(labels):
    """uint8 label values; anything that is not an integer in 0..255 is an error, not a wrap-around."""
    lab = np.asarray(labels)
    if lab.ndim != 1:
        lab = lab.reshape(-1)
    if lab.dtype == np.uint8:
        return lab
    if lab.dtype == np.bool_:
        return lab.astype(np.uint8)
    if not np.issubdtype(lab.dtype, np.number) or np.issubdtype(lab.dtype, np.complexfloating):
        raise ValueError("labels must be numbers, got dtype %s" % lab.dtype)
    if lab.size and not np.issubdtype(lab.dtype, np.integer) and not np.all(lab == np.rint(lab)):      # NaN fails too
        raise ValueError("labels must be integers")
    if lab.size and (lab.min() < 0 or lab.max() > 255):
        raise ValueError("labels must lie in 0..255")
    return lab.astype(np.uint8)


def layout(lengths, window):
    """Where the stretches sit in the packed batch: (bounds int64 [n + 1], tails int64 [n]) -- every stretch is followed by
    its zero tail up to the next multiple of the window (``train_validate.padding``: an exact multiple gets none)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_win = -(-lengths // int(window))
    tails = n_win * int(window) - lengths
    bounds = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(n_win * int(window), out=bounds[1:])
    return bounds, tails


def score_host(probs, logits, y, bounds, thresholds):
    """What ``cf_validation_score`` returns, in numpy: (right int64 [n], ce_sum float64 [n], counts int64 [K, 4]).

    With ``p``, ``z`` promoted to double and ``y`` the label value: ``right[r]`` counts read r's samples with
    ``round_half_even(p) == y``; ``ce_sum[r]`` sums ``max(z, 0) - z*y + log1p(exp(-|z|))`` over them; ``counts[k]`` =
    (tp, fp, tn_raw, fn) over ALL samples at ``thresholds[k]``: a sample is called when ``p >= t``, a called one is a true
    positive when its label is 1 and a false positive otherwise, an un-called one a true negative when its label is 0 and a
    false negative otherwise.  ``tn_raw`` still holds the zero tails (``finish`` takes them out)."""
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    z = np.asarray(logits, dtype=np.float64).reshape(-1)
    y = np.asarray(y).reshape(-1).astype(np.float64)
    bounds = np.asarray(bounds, dtype=np.int64)
    right_run = np.concatenate(([0], np.cumsum(np.round(p) == y))).astype(np.int64)
    right = right_run[bounds[1:]] - right_run[bounds[:-1]]
    ce = np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))
    ce_sum = np.array([np.sum(ce[a:b]) for a, b in zip(bounds[:-1].tolist(), bounds[1:].tolist())], dtype=np.float64)
    counts = np.zeros((len(thresholds), 4), dtype=np.int64)
    for k, t in enumerate(thresholds):
        called = p >= float(t)
        counts[k] = (np.count_nonzero(called & (y == 1)), np.count_nonzero(called & (y != 1)),
                     np.count_nonzero(~called & (y == 0)), np.count_nonzero(~called & (y != 0)))
    return right, ce_sum, counts


def finish(right, ce_sum, counts_k, bounds, tails):
    """The divisions of ``train_validate.score_validation_batch`` on the raw results: (acc float32 [n], loss float32 [n],
    (tp, fp, tn, fn)).  ``acc`` = count as float32 / size as float32; ``loss`` = ``ce_sum / size`` in double, then float32;
    every tail sample leaves the true negatives whether or not it was one (rnn_class.py:245-249)."""
    sizes = np.diff(np.asarray(bounds, dtype=np.int64))
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.asarray(right, dtype=np.int64).astype(np.float32) / sizes.astype(np.float32)
        loss = np.asarray(ce_sum, dtype=np.float64) / sizes
    tp, fp, tn, fn = (int(v) for v in counts_k)
    return acc, loss.astype(np.float32), (tp, fp, tn - int(np.sum(tails)), fn)


class DeviceValidationSet(object):
    """All validation reads of a run, concatenated: ``signal`` float32 [total] (cast once -- the values
    ``pack_validation_windows`` writes into its float32 batch), ``labels`` uint8 [total], ``offsets`` int64 [n_reads + 1],
    ``lengths`` int64 [n_reads]."""

    def __init__(self, signal, labels, offsets, device=None):
        self.signal = signal
        self.labels = labels
        self.offsets = offsets
        self.lengths = np.diff(offsets)
        self.device = device
        self._dev = None                 # {"device", "signal", "labels"} on the card, uploaded once
        self.uploads = 0                 # how often the reads went to a card

    @classmethod
    def from_arrays(cls, signals, labels, device=None):
        signals = [np.asarray(s).reshape(-1) for s in signals]
        labels = [_as_labels(l) for l in labels]
        if len(signals) != len(labels):
            raise ValueError("%d signals but %d label arrays" % (len(signals), len(labels)))
        for i, (s, l) in enumerate(zip(signals, labels)):
            if len(s) != len(l):
                raise ValueError("read %d: %d samples but %d labels" % (i, len(s), len(l)))
        offsets = np.zeros(len(signals) + 1, dtype=np.int64)
        np.cumsum(np.array([len(s) for s in signals], dtype=np.int64), out=offsets[1:])
        signal = np.zeros(int(offsets[-1]), dtype=np.float32)
        lab = np.zeros(int(offsets[-1]), dtype=np.uint8)
        for o, s, l in zip(offsets[:-1].tolist(), signals, labels):
            signal[o:o + len(s)] = s
            lab[o:o + len(l)] = l
        return cls(signal, lab, offsets, device)

    @classmethod
    def from_npz(cls, paths, loader=None, device=None):
        """The reads of ``paths`` (``raw`` + ``base_labels``, networks/reader.py:11-23), in that order."""
        if loader is None:
            from .train_validate import load_npz as loader
        signals, labels = [], []
        for path in paths:
            raw, lab = loader(path)
            signals.append(raw)
            labels.append(lab)
        return cls.from_arrays(signals, labels, device)

    @property
    def n_reads(self):
        return len(self.lengths)

    # ------------------------------------------------------------------ one round on the host
    def select(self, window, max_seq_length, validation_start, max_number):
        """``train_validate.select_validation_stretches`` from the lengths alone: (read_index, first, length) int64 arrays.
        Same skip rule for reads shorter than the stretch, same stop at ``max_number``, same ValueError, and for "random"
        the same ``random.randint(0, room)`` calls on Python's global generator: one per long-enough read, in file order,
        none after the stop."""
        whole = validation_start == "complete"
        if not whole and validation_start != "random" and type(validation_start) != int:
            raise ValueError("validation_start must be an int, 'random' or 'complete'")
        n = max_seq_length // window * window
        picked = []
        for index, size in enumerate(self.lengths.tolist()):
            first, length = 0, size
            if not whole:
                room = size - n - (0 if validation_start == "random" else validation_start)
                if room < 0:
                    continue
                first = random.randint(0, room) if validation_start == "random" else validation_start
                first, stop, _ = slice(first, first + n).indices(size)          # raw[first:first + n] as Python slices it
                length = max(0, stop - first)
            picked.append((index, first, length))
            if len(picked) >= max_number:
                break
        table = np.array(picked, dtype=np.int64).reshape(-1, 3)
        return table[:, 0].copy(), table[:, 1].copy(), table[:, 2].copy()

    def pack(self, selection, window):
        """What the gather kernel writes, in numpy: (x float32 [sum N_i, window, 1], y uint8 [sum N_i * window], bounds,
        tails) -- ``train_validate.pack_validation_windows`` on the selected slices, with the labels kept as uint8."""
        read_index, first, length = selection
        bounds, tails = layout(length, window)
        x = np.zeros(int(bounds[-1]), dtype=np.float32)
        y = np.zeros(int(bounds[-1]), dtype=np.uint8)
        src = self.offsets[read_index] + first
        for b, s, n in zip(bounds[:-1].tolist(), src.tolist(), np.asarray(length).tolist()):
            x[b:b + n] = self.signal[s:s + n]
            y[b:b + n] = self.labels[s:s + n]
        return x.reshape(-1, window, 1), y, bounds, tails

    def check_selection(self, selection):
        """Raise ValueError unless every stretch lies inside its read (the kernels index with these numbers)."""
        read_index, first, length = (np.asarray(a, dtype=np.int64) for a in selection)
        if not (read_index.shape == first.shape == length.shape and read_index.ndim == 1):
            raise ValueError("a selection is three int64 arrays of one length")
        if read_index.size and (read_index.min() < 0 or read_index.max() >= self.n_reads):
            raise ValueError("selection names a read that is not in the set")
        if np.any(first < 0) or np.any(length < 0) or np.any(first + length > self.lengths[read_index]):
            raise ValueError("selection reaches outside a read")
        return read_index, first, length

    score_host = staticmethod(score_host)
    finish = staticmethod(finish)
    layout = staticmethod(layout)

    # ------------------------------------------------------------------ the card's side
    def device_arrays(self, device=None):
        """(signal float32 [max(total, 1)], labels uint8 [max(total, 1)]) on ``device``; uploaded on the first call."""
        import torch
        device = torch.device((self.device or "cuda") if device is None else device)
        if device.type != "cuda":
            raise ValueError("device_arrays: the reads go to a GPU")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev["device"] != device:
            up = lambda a, dt: torch.from_numpy(a if a.size else np.zeros(1, dt)).to(device)     # noqa: E731
            self._dev = {"device": device, "signal": up(self.signal, np.float32), "labels": up(self.labels, np.uint8)}
            self.uploads += 1
        return self._dev["signal"], self._dev["labels"]
