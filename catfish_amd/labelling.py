"""Labels from event tables: a resquiggled read's base calls and event lengths -> the per-sample training labels.  This module is
the definition (numpy, host); ``cf_label_events`` (csrc/label_events.hpp, index rules in csrc/label_events_rule.hpp) computes the
same bytes on the card.

The rule is the reference's (``TrainingRead.events`` setter with ``use_tombo=True``, ``classify_events``, ``label_raws``;
``training_encodings.hp_class_number`` / ``extend_classification``; ``base_to_signal.get_base_new_signal``), restated over
integers.  A read has ``E >= 1`` events; event ``e`` has a base byte ``b[e]`` and ``len[e] >= 1`` samples; ``cs`` / ``ce`` events
are clipped at its ends and ``k`` is the odd k-mer size, ``oh = k // 2``:

    core[e] = cs <= e < E - ce,  e - oh >= 0,  e + oh < E,  b[e] != 'N'  and  b[e - oh .. e + oh] all the same byte
    cls[e]  = some core[e'] with |e' - e| <= 2 inside the read          (the widening ignores clipping and 'N')
    labels[start[e] .. start[e] + len[e]) = cls[e],   start = the exclusive sum of len,   final_signal = sum(len)
    basemap[j] = b[e] there, with bit 7 set on the one sample start[e] + len[e] // 2

A byte comparison: a lower-case base only equals itself.  What the reference leaves misaligned or undefined is refused with
ValueError (``check_read``); tests/golden/label_events_golden.npz holds the reference's own answers.
"""
from __future__ import annotations

import numpy as np

MAX_KMER = 15
WIDEN = 2                     # extend_classification: width 4, two events each way
TILE = 4096                   # CF_LABEL_TILE / LE_TILE: samples per workgroup of the expand kernel
DEFAULT_CLIPPED = 10          # the reference's --clipped-bases default
MARK = 0x80                   # the base map's "new base" bit


def check_kmer(kmer):
    if isinstance(kmer, (bool, np.bool_)) or not isinstance(kmer, (int, np.integer)):
        raise ValueError("kmer must be an int, got %r" % (kmer,))
    kmer = int(kmer)
    if kmer < 1 or kmer > MAX_KMER or kmer % 2 == 0:
        raise ValueError("kmer must be odd and in 1 .. %d, got %d" % (MAX_KMER, kmer))
    return kmer


def as_bases(bases):
    """Base calls as uint8 [E]: a uint8 array, ``bytes`` / ``str``, or an array of one-character ``S1`` / ``U1`` items (what h5py
    and ``astype(str)`` give).  ValueError for anything else and for a byte >= 128."""
    if isinstance(bases, str):
        try:
            bases = bases.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("bases must be ASCII (bytes below 128)")
    if isinstance(bases, (bytes, bytearray)):
        out = np.frombuffer(bytes(bases), dtype=np.uint8)
    else:
        arr = np.asarray(bases)
        if arr.dtype.kind == "U":
            if arr.dtype.itemsize != 4:
                raise ValueError("bases: one character per event, got dtype %s" % arr.dtype)
            try:
                arr = np.char.encode(arr.reshape(-1), "ascii")
            except UnicodeEncodeError:
                raise ValueError("bases must be ASCII (bytes below 128)")
            if arr.size == 0:
                arr = arr.astype("S1")
        if arr.dtype.kind == "S":
            if arr.dtype.itemsize != 1:
                raise ValueError("bases: one character per event, got dtype %s" % arr.dtype)
            out = np.ascontiguousarray(arr.reshape(-1)).view(np.uint8)
        elif arr.dtype == np.uint8:
            out = arr.reshape(-1)
        else:
            raise ValueError("bases must be uint8, bytes, str or one-character strings, got dtype %s" % arr.dtype)
    if out.size and out.max() >= 128:
        raise ValueError("bases must be bytes below 128 (bit 7 is the base map's mark)")
    return np.ascontiguousarray(out)


def _as_ints(values, what):
    arr = np.asarray(values)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.number) or np.issubdtype(arr.dtype, np.complexfloating):
        raise ValueError("%s must be integers, got dtype %s" % (what, arr.dtype))
    arr = arr.reshape(-1)
    if not np.issubdtype(arr.dtype, np.integer):
        if arr.size and not np.all(arr == np.rint(arr)):
            raise ValueError("%s must be integers" % what)
    if arr.size and (arr.min() < -2 ** 62 or arr.max() > 2 ** 62):
        raise ValueError("%s out of range" % what)
    return arr.astype(np.int64)


def _as_int(value, what):
    arr = _as_ints(value, what)
    if arr.size != 1:
        raise ValueError("%s must be one integer" % what)
    return int(arr[0])


def check_read(bases, lengths, clipped=(0, 0), starts=None, n_raw=None):
    """One read's table as (bases uint8 [E], lengths int64 [E], (cs, ce), final_signal), or ValueError where the reference's output is
    misaligned or undefined: no events, a length < 1, a negative clip or ``cs + ce > E``, a base byte >= 128, ``starts`` that are not
    the exclusive sum of the lengths (``TrainingRead`` cuts by start differences, ``base_to_signal`` by lengths: only contiguous
    tables make them agree), or more samples than the ``n_raw`` supplied."""
    bases = as_bases(bases)
    lengths = _as_ints(lengths, "event lengths")
    n = int(bases.size)
    if n == 0:
        raise ValueError("a read needs at least one event")
    if lengths.size != n:
        raise ValueError("%d bases but %d event lengths" % (n, lengths.size))
    if lengths.min() < 1:
        raise ValueError("every event length must be >= 1, got %d" % int(lengths.min()))
    if lengths.max() >= 2 ** 31:
        raise ValueError("an event of 2^31 or more samples")
    try:
        cs, ce = clipped
    except (TypeError, ValueError):
        raise ValueError("clipped must be (clipped_start, clipped_end), got %r" % (clipped,))
    cs, ce = _as_int(cs, "clipped_start"), _as_int(ce, "clipped_end")
    if cs < 0 or ce < 0 or cs + ce > n:
        raise ValueError("clipped (%d, %d) must be non-negative and leave %d events" % (cs, ce, n))
    final = int(lengths.sum())
    if starts is not None:
        starts = _as_ints(starts, "event starts")
        want = np.concatenate(([0], np.cumsum(lengths)[:-1]))
        if starts.size != n or not np.array_equal(starts, want):
            raise ValueError("event_start must be 0, len[0], len[0] + len[1], ...: the table is not contiguous")
    if n_raw is not None and final > int(n_raw):
        raise ValueError("the events cover %d samples, the raw signal has %d" % (final, int(n_raw)))
    return bases, lengths, (cs, ce), final


def event_classes_host(bases, clipped_start, clipped_end, kmer=5):
    """cls uint8 [E]: the k-mer test per event, widened by two events each way (the module's rule)."""
    kmer = check_kmer(kmer)
    b = as_bases(bases)
    n, oh = int(b.size), kmer // 2
    cs, ce = int(clipped_start), int(clipped_end)
    core = np.zeros(n, dtype=bool)
    if n >= kmer:
        windows = np.lib.stride_tricks.sliding_window_view(b, kmer)
        core[oh:n - oh] = (windows == windows[:, :1]).all(axis=1) & (b[oh:n - oh] != ord("N"))
    at = np.arange(n)
    core &= (at >= cs) & (at < n - ce)
    cls = core.copy()
    for d in range(1, WIDEN + 1):
        cls[d:] |= core[:-d]
        cls[:-d] |= core[d:]
    return cls.astype(np.uint8)


def expand_events_host(classes, lengths):
    """labels uint8 [sum(lengths)]: every event's class repeated over its samples."""
    return np.repeat(np.asarray(classes, dtype=np.uint8).reshape(-1), np.asarray(lengths, dtype=np.int64).reshape(-1))


def base_map_host(bases, lengths):
    """basemap uint8 [sum(lengths)]: every event's base over its samples, bit 7 set on the sample ``start + length // 2``."""
    b = as_bases(bases)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    out = np.repeat(b, lengths)
    if out.size:
        starts = np.cumsum(lengths) - lengths
        out[starts + lengths // 2] |= MARK
    return out


def label_read_host(bases, lengths, clipped=(0, 0), kmer=5, starts=None):
    """One read -> (labels uint8 [final_signal], basemap uint8 [final_signal]); ``check_read``'s refusals."""
    kmer = check_kmer(kmer)
    bases, lengths, (cs, ce), _final = check_read(bases, lengths, clipped, starts)
    return expand_events_host(event_classes_host(bases, cs, ce, kmer), lengths), base_map_host(bases, lengths)


def _read_fields(read):
    if isinstance(read, dict):
        return (read["bases"], read["lengths"], read.get("clipped", (0, 0)), read.get("starts"),
                read.get("n_raw", len(read["raw"]) if read.get("raw") is not None else None))
    read = tuple(read)
    if not 2 <= len(read) <= 5:
        raise ValueError("a read is (bases, lengths[, clipped[, starts[, n_raw]]]) or a dict with those keys")
    return read + ((0, 0), None, None)[len(read) - 2:]


class EventBatch(object):
    """Many reads' event tables, packed: ``bases`` uint8 [n_events], ``lengths`` int32 [n_events], ``event_offsets`` int64
    [n_reads + 1], ``clipped`` int32 [n_reads, 2], ``sample_offsets`` int64 [n_reads + 1] -- what ``cf_label_events`` takes."""

    def __init__(self, bases, lengths, event_offsets, clipped, sample_offsets):
        self.bases, self.lengths, self.event_offsets, self.clipped, self.sample_offsets = bases, lengths, event_offsets, clipped, sample_offsets

    n_reads = property(lambda self: len(self.event_offsets) - 1)
    n_events = property(lambda self: int(self.event_offsets[-1]))
    total = property(lambda self: int(self.sample_offsets[-1]))

    @classmethod
    def from_reads(cls, reads):
        """``reads``: one ``(bases, lengths[, clipped[, starts[, n_raw]]])`` tuple, or one dict with those keys (``load_event_npz``
        gives such dicts; their ``raw`` supplies ``n_raw``), per read.  Every refusal of ``check_read`` is made here, and a batch of
        2^31 or more events or samples is refused too."""
        checked = [check_read(b, l, c, s, n) for b, l, c, s, n in (_read_fields(read) for read in reads)]
        n_events = sum(len(b) for b, _l, _c, _f in checked)
        total = sum(f for _b, _l, _c, f in checked)
        if n_events >= 2 ** 31 or total >= 2 ** 31:
            raise ValueError("a batch of 2^31 or more events or samples (%d events, %d samples): label it in parts" % (n_events, total))
        event_offsets = np.zeros(len(checked) + 1, dtype=np.int64)
        sample_offsets = np.zeros(len(checked) + 1, dtype=np.int64)
        np.cumsum(np.array([len(b) for b, _l, _c, _f in checked], dtype=np.int64), out=event_offsets[1:])
        np.cumsum(np.array([f for _b, _l, _c, f in checked], dtype=np.int64), out=sample_offsets[1:])
        bases = np.concatenate([b for b, _l, _c, _f in checked]) if checked else np.zeros(0, np.uint8)
        lengths = (np.concatenate([l for _b, l, _c, _f in checked]) if checked else np.zeros(0, np.int64)).astype(np.int32)
        clipped = np.array([c for _b, _l, c, _f in checked], dtype=np.int32).reshape(-1, 2)
        return cls(bases, lengths, event_offsets, clipped, sample_offsets)

    def read(self, r):
        """Read ``r``'s (bases, lengths, (cs, ce))."""
        a, b = int(self.event_offsets[r]), int(self.event_offsets[r + 1])
        return self.bases[a:b], self.lengths[a:b], (int(self.clipped[r, 0]), int(self.clipped[r, 1]))

    def label_host(self, kmer=5, base_map=False):
        """labels uint8 [total] of the whole batch (and the base map with ``base_map=True``): ``label_read_host`` read by read."""
        kmer = check_kmer(kmer)
        labels = np.zeros(self.total, dtype=np.uint8)
        bmap = np.zeros(self.total, dtype=np.uint8) if base_map else None
        for r in range(self.n_reads):
            bases, lengths, (cs, ce) = self.read(r)
            o = int(self.sample_offsets[r])
            lab = expand_events_host(event_classes_host(bases, cs, ce, kmer), lengths)
            labels[o:o + lab.size] = lab
            if base_map:
                bmap[o:o + lab.size] = base_map_host(bases, lengths)
        return (labels, bmap) if base_map else labels


def label_reads(batch, kmer=5, device=None, base_map=False):
    """The batch's labels on the card through ``cf_label_events``: a torch uint8 tensor [total] on ``device`` (default: the current
    GPU), or (labels, basemap) with ``base_map=True`` -- ``EventBatch.label_host``'s bytes.  Asynchronous on torch's current stream.
    No GPU or no native library is an error: there is no fall-back here."""
    import torch
    from . import _native as N
    kmer = check_kmer(kmer)
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError("label_reads: the labels are made on a GPU (EventBatch.label_host is the host route)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    lib = N.lib()
    total, n_events = batch.total, batch.n_events
    labels = torch.empty(total, dtype=torch.uint8, device=device)
    bmap = torch.empty(total, dtype=torch.uint8, device=device) if base_map else None
    if total == 0:
        N.check(lib.cf_label_events(None, None, None, None, None, None, batch.n_reads, n_events, 0, kmer, None, None, None, 0, None))
        return (labels, bmap) if base_map else labels
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)     # noqa: E731
    tables = [up(batch.bases), up(batch.lengths), up(batch.event_offsets), up(batch.clipped.reshape(-1)), up(batch.sample_offsets)]
    work_bytes = int(lib.cf_label_events_work_bytes(n_events))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        N.check(lib.cf_label_events(None, *[N._p(t) for t in tables], batch.n_reads, n_events, total, kmer, N._p(labels),
                                    N._p(bmap) if base_map else None, N._p(work), work_bytes, N.current_stream_ptr(torch, device)))
    # (tables and work were allocated on the stream the launches run on, so the allocator hands them out again only behind them)
    return (labels, bmap) if base_map else labels


def load_event_npz(path):
    """One read with its event table: ``raw``, ``event_base`` (uint8, ``S1`` or ``U1``), ``event_length``, and optionally
    ``event_start``, ``clipped_start``, ``clipped_end`` (absent: 0) -> dict(raw, bases, lengths, clipped, starts) as
    ``EventBatch.from_reads`` takes it.  ``convert.convert_events`` writes such files."""
    with np.load(path, allow_pickle=False) as z:
        for key in ("raw", "event_base", "event_length"):
            if key not in z.files:
                raise ValueError("%s: no %r (an event .npz holds raw, event_base and event_length)" % (path, key))
        clip = lambda key: _as_int(z[key], key) if key in z.files else 0     # noqa: E731
        return {"raw": np.asarray(z["raw"]).reshape(-1), "bases": as_bases(z["event_base"]), "lengths": _as_ints(z["event_length"], "event_length"),
                "clipped": (clip("clipped_start"), clip("clipped_end")),
                "starts": _as_ints(z["event_start"], "event_start") if "event_start" in z.files else None}


def load_labelled_event_npz(path, kmer=5):
    """(raw[:final_signal], labels) of one event ``.npz``, labelled on the host: what ``train_validate.load_npz`` returns for the
    ``raw`` + ``base_labels`` file made from it."""
    read = load_event_npz(path)
    labels, _ = label_read_host(read["bases"], read["lengths"], read["clipped"], kmer, read["starts"])
    if labels.size > read["raw"].size:
        raise ValueError("%s: the events cover %d samples, the raw signal has %d" % (path, labels.size, read["raw"].size))
    return read["raw"][:labels.size], labels


def kmer_from_env(value):
    """``CATFISH_LABEL_KMER``: an odd k in 1 .. 15; unset (None) or empty means None: the directories hold labelled reads."""
    if value is None or not value.strip():
        return None
    try:
        return check_kmer(int(value.strip()))
    except ValueError:
        raise ValueError("CATFISH_LABEL_KMER must be an odd int in 1 .. %d, got %r" % (MAX_KMER, value))


def synthetic_event_read(length, seed, hp_fraction=0.06):
    """A normalised synthetic squiggle of ``length`` samples WITH its event table, built like
    ``train_validate.synthetic_labelled_read``: an event is a dwell at one level; a homopolymer is a run of five to nine events of
    one base at one level, the events between them single bases that differ from their predecessor.
    -> (raw float64 [length], bases uint8 [E], lengths int32 [E])."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    sig = np.empty(length, dtype=np.float64)
    bases, lengths = [], []
    i, last = 0, -1
    while i < length:
        if rng.random() < hp_fraction / 8.0:
            base = int(rng.integers(0, 4))
            level = rng.normal(500.0, 60.0)
            for _ in range(int(rng.integers(5, 10))):
                if i >= length:
                    break
                n = min(int(rng.integers(8, 21)), length - i)
                sig[i:i + n] = level
                bases.append(base)
                lengths.append(n)
                i += n
        else:
            base = int((last + 1 + rng.integers(0, 3)) % 4) if last >= 0 else int(rng.integers(0, 4))
            n = min(int(rng.geometric(1.0 / 9.0)), length - i)
            sig[i:i + n] = rng.normal(500.0, 60.0)
            bases.append(base)
            lengths.append(n)
            i += n
        last = base
    sig = np.clip(np.rint(sig + rng.normal(0.0, 8.0, size=length)), 0, 2047)
    shift = np.median(sig)
    scale = np.median(np.abs(sig - shift))
    return (sig - shift) / scale, letters[np.array(bases, dtype=np.int64)], np.array(lengths, dtype=np.int32)
