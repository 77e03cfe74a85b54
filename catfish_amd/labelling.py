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

import os

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


class TableBatch(object):
    """What ``EventBatch`` and ``MoveBatch`` share, and what the code that labels either asks of them: ``ENTRY`` and ``WORK_BYTES``, the
    names of its entry point in the library and of that entry point's work-buffer query; ``device_tables(up)``, the entry point's table
    arguments in its order (``up`` puts an array on the card; an int stays an int); ``work_args()``, the query's arguments;
    ``k_of(kmer)``, the k the labels are made with; ``read_labels_host(r, kmer, base_map)``, the definition for one read; and
    ``base_edges()``, where the bases begin -- ``(edges int64 [n_bases + 1], base_offsets int64 [n_reads + 1])`` as
    ``base_votes.BaseTable`` takes them."""

    n_reads = property(lambda self: len(self.event_offsets) - 1)
    n_events = property(lambda self: int(self.event_offsets[-1]))
    total = property(lambda self: int(self.sample_offsets[-1]))

    def label_host(self, kmer=5, base_map=False):
        """labels uint8 [total] of the whole batch (and the base map with ``base_map=True``): the definition, read by read.  A
        ``MoveBatch`` brings its k-mers with it and does not look at ``kmer`` (``k_of``)."""
        kmer = self.k_of(kmer)
        labels = np.zeros(self.total, dtype=np.uint8)
        bmap = np.zeros(self.total, dtype=np.uint8) if base_map else None
        for r in range(self.n_reads):
            lab, bm = self.read_labels_host(r, kmer, base_map)
            o = int(self.sample_offsets[r])
            labels[o:o + lab.size] = lab
            if base_map:
                bmap[o:o + bm.size] = bm
        return (labels, bmap) if base_map else labels


class EventBatch(TableBatch):
    """Many reads' event tables, packed: ``bases`` uint8 [n_events], ``lengths`` int32 [n_events], ``event_offsets`` int64
    [n_reads + 1], ``clipped`` int32 [n_reads, 2], ``sample_offsets`` int64 [n_reads + 1] -- what ``cf_label_events`` takes."""
    ENTRY, WORK_BYTES = "cf_label_events", "cf_label_events_work_bytes"

    def __init__(self, bases, lengths, event_offsets, clipped, sample_offsets):
        self.bases, self.lengths, self.event_offsets, self.clipped, self.sample_offsets = bases, lengths, event_offsets, clipped, sample_offsets

    k_of = staticmethod(check_kmer)

    def device_tables(self, up):
        return [up(self.bases), up(self.lengths), up(self.event_offsets), up(self.clipped.reshape(-1)), up(self.sample_offsets)]

    def work_args(self):
        return (self.n_events,)

    def base_edges(self):
        """A base per event: the running sum of the event lengths."""
        edges = np.zeros(self.n_events + 1, dtype=np.int64)
        np.cumsum(np.asarray(self.lengths, dtype=np.int64), out=edges[1:])
        return edges, np.asarray(self.event_offsets, dtype=np.int64)

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

    def read_labels_host(self, r, kmer, base_map):
        bases, lengths, (cs, ce) = self.read(r)
        return expand_events_host(event_classes_host(bases, cs, ce, kmer), lengths), base_map_host(bases, lengths) if base_map else None


def label_device(device, who=None):
    """The one decision "card or host": the CUDA device (with its index) the labels are made on, or None for the host route.
    ``who`` names a caller that has no host route (``label_reads``, ``label_moves``): ``device`` None is then the current GPU and
    anything but a CUDA device a ValueError.  Without ``who`` (``DeviceValidationSet.from_tables``) ``device`` None means the card
    where there is one to use -- a GPU and the built library -- and a device that is not CUDA means the host.  An explicit CUDA device
    is taken at its word: no GPU or no library is then an error of the launch, never a fall-back."""
    if device is not None and str(device).split(":")[0] != "cuda":
        if who is None:
            return None
        raise ValueError("%s: the labels are made on a GPU (%s.label_host is the host route)" % who)
    import torch
    if device is None and who is None:
        from . import _native
        if not torch.cuda.is_available() or not os.path.exists(_native.DEFAULT_LIB_PATH):
            return None
    device = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def label_on_card(batch, kmer, device, base_map):
    """Either kind of batch through its entry point, on ``device`` (a ``label_device``): (labels, basemap or None, the tables on the
    card) -- uint8 tensors [total] with ``batch.label_host``'s bytes.  Asynchronous on torch's current stream."""
    import torch
    from . import _native as N
    lib = N.lib()
    k, total = batch.k_of(kmer), batch.total
    labels = torch.empty(total, dtype=torch.uint8, device=device)
    bmap = torch.empty(total, dtype=torch.uint8, device=device) if base_map else None
    tables = batch.device_tables(lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device))
    work_bytes = int(getattr(lib, batch.WORK_BYTES)(*batch.work_args())) if total else 0
    work = torch.empty(work_bytes, dtype=torch.uint8, device=device)
    p = lambda t: N._p(t) if total else None     # noqa: E731   (an empty batch is a call without pointers)
    with torch.cuda.device(device):
        N.check(getattr(lib, batch.ENTRY)(None, *[t if isinstance(t, int) else p(t) for t in tables], batch.n_reads, batch.n_events, total, k,
                                          p(labels), p(bmap), p(work), work_bytes, N.current_stream_ptr(torch, device) if total else None))
    # (tables and work were allocated on the stream the launches run on, so the allocator hands them out again only behind them)
    return labels, bmap, tables


def label_reads(batch, kmer=5, device=None, base_map=False):
    """The batch's labels on the card through ``cf_label_events``: a torch uint8 tensor [total] on ``device`` (default: the current
    GPU), or (labels, basemap) with ``base_map=True`` -- ``EventBatch.label_host``'s bytes.  Asynchronous on torch's current stream.
    No GPU or no native library is an error: there is no fall-back here."""
    kmer = check_kmer(kmer)
    labels, bmap, _tables = label_on_card(batch, kmer, label_device(device, ("label_reads", "EventBatch")), base_map)
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


# ----------------------------------------------------------------------------------------------------- labels from a move table
# The other half of the reference's ``TrainingRead.events`` setter: ``use_tombo=False``, its default.  The basecaller's Events table
# holds, per event, ``model_state`` (a k-mer), ``move`` and ``length`` in SECONDS; consecutive events with ``move == 0`` ("stays")
# belong to the event before them.  One read has ``E >= 1`` events, ``n_raw`` samples of raw signal and clips ``(cs, ce)``:
#
#     heads    H = {0} u {n >= 1 : move[n] != 0} (move[0] is ignored), M = |H| merged events; merged event j has head h_j and the
#              stays behind it, up to h_{j+1} - 1 (E - 1 for the last)
#     length   L_j = length[h_j] + length[h_j + 1] + ..., summed left to right IN THE TABLE'S DTYPE (float32 or float64); for j = 0
#              the sum starts (length[0] + length[0]): the reference initialises its running length with length[0] and then adds
#              length[0] again, because it forces move[0] to 0.  n_j = ceil(L_j * 4000), the product in the same dtype
#     samples  merged event j owns [S_j, S_j + n_j), S the exclusive sum of n, cut at n_raw: final = min(sum n_j, n_raw) labels
#     class    core[j] = cs <= j < M - ce, and the k bytes of state[h_j] are one byte that is not 'N';
#              cls[j] = some core[j'] with |j' - j| <= 2 inside the read -- no sliding window: the k-mer comes with the event
#     base map state[h_j][k // 2] over the event's samples, bit 7 on the sample S_j + n_j // 2 where that lies below final
#
# In this branch the reference leaves ``final_signal`` None, so its ``get_pos`` / ``get_neg`` cannot run: it never trained from
# these labels.  ``classified`` is computed before that and is what tests/golden/label_moves_golden.npz holds.  ``cf_label_moves``
# (csrc/label_moves.hpp, rules in csrc/label_moves_rule.hpp) computes the same bytes on the card.
FREQUENCY = 4000              # samples per second: the reference's constant


def as_states(states):
    """The k-mers as uint8 [E, k]: an array of ``S<k>`` / ``U<k>`` items (what h5py and ``astype(str)`` give), or uint8 [E, k].
    ValueError for k outside 1 .. 15, a k-mer shorter than k (a NUL byte) and a byte >= 128."""
    arr = np.asarray(states)
    if arr.dtype.kind == "U":
        try:
            arr = np.char.encode(arr.reshape(-1), "ascii").astype("S%d" % max(arr.dtype.itemsize // 4, 1))
        except UnicodeEncodeError:
            raise ValueError("model states must be ASCII (bytes below 128)")
    if arr.dtype.kind == "S":
        k = arr.dtype.itemsize
        out = np.ascontiguousarray(arr.reshape(-1)).view(np.uint8).reshape(-1, k) if k else np.zeros((arr.size, 0), np.uint8)
    elif arr.dtype == np.uint8 and arr.ndim == 2:
        out = arr
    else:
        raise ValueError("model states must be k-character strings or uint8 [n_events, k], got dtype %s with %d axes" % (arr.dtype, arr.ndim))
    if out.shape[1] < 1 or out.shape[1] > MAX_KMER:
        raise ValueError("the k-mers must have 1 .. %d bytes, got %d" % (MAX_KMER, out.shape[1]))
    if out.size and (out.max() >= 128 or out.min() == 0):
        raise ValueError("every k-mer must be k bytes in 1 .. 127 (bit 7 is the base map's mark)")
    return np.ascontiguousarray(out)


def merge_moves_host(lengths, moves):
    """(heads int64 [M], n_signals int64 [M]): where the merged events begin, and ``ceil(L_j * 4000)`` with ``L_j`` summed left to
    right from the head in the dtype of ``lengths`` (float32 or float64), the first length counted twice.  A count the dtype cannot
    state as a finite number comes back as 2^63 - 1 (``check_move_read`` refuses it)."""
    lengths = np.asarray(lengths).reshape(-1)
    if lengths.dtype not in (np.float32, np.float64):
        raise ValueError("event lengths must be float32 or float64 (seconds), got dtype %s" % lengths.dtype)
    moves = np.asarray(moves).reshape(-1)
    n = int(lengths.size)
    if n == 0 or moves.size != n:
        raise ValueError("%d event lengths but %d moves" % (n, moves.size))
    flag = moves != 0
    flag[0] = True
    heads = np.flatnonzero(flag).astype(np.int64)
    count = np.diff(np.append(heads, n))
    with np.errstate(over="ignore", invalid="ignore"):
        total = lengths[heads]                                  # (a copy)
        total[0] = total[0] + lengths[0]
        active, d = np.flatnonzero(count > 1), 1
        while active.size:                                      # one stay further per round: every sum goes left to right
            total[active] = total[active] + lengths[heads[active] + d]
            d += 1
            active = active[count[active] > d]
        product = np.ceil(total * lengths.dtype.type(FREQUENCY))
    n_signals = np.full(heads.size, np.iinfo(np.int64).max, dtype=np.int64)
    fits = np.isfinite(product) & (product < 2.0 ** 62)
    n_signals[fits] = product[fits].astype(np.int64)
    return heads, n_signals


def check_move_read(states, lengths, moves, clipped=(0, 0), n_raw=None):
    """One read's move table as (states uint8 [E, k], lengths, moves int32 [E], (cs, ce), n_raw, heads, n_signals, final), or
    ValueError where the reference raises or misaligns: no events, a length that is not finite or not > 0, a merged event of 2^31
    or more samples, k outside 1 .. 15, a negative clip or ``cs + ce > M``, ``n_raw < 1``.  ``n_raw`` None: the raw signal is as
    long as the events."""
    states = as_states(states)
    lengths = np.asarray(lengths).reshape(-1)
    if lengths.dtype not in (np.float32, np.float64):
        raise ValueError("event lengths must be float32 or float64 (seconds), got dtype %s" % lengths.dtype)
    n = int(states.shape[0])
    if n == 0:
        raise ValueError("a read needs at least one event")
    moves = _as_ints(moves, "event moves")
    if lengths.size != n or moves.size != n:
        raise ValueError("%d model states but %d event lengths and %d moves" % (n, lengths.size, moves.size))
    if not np.all(np.isfinite(lengths)) or not np.all(lengths > 0):
        raise ValueError("every event length must be finite and > 0")
    heads, n_signals = merge_moves_host(lengths, moves)
    if n_signals.max() >= 2 ** 31:
        raise ValueError("a merged event of 2^31 or more samples")
    try:
        cs, ce = clipped
    except (TypeError, ValueError):
        raise ValueError("clipped must be (clipped_start, clipped_end), got %r" % (clipped,))
    cs, ce = _as_int(cs, "clipped_start"), _as_int(ce, "clipped_end")
    if cs < 0 or ce < 0 or cs + ce > heads.size:
        raise ValueError("clipped (%d, %d) must be non-negative and leave %d merged events" % (cs, ce, heads.size))
    covered = int(n_signals.sum())
    n_raw = covered if n_raw is None else _as_int(n_raw, "n_raw")
    if n_raw < 1:
        raise ValueError("n_raw must be >= 1, got %d" % n_raw)
    moves = np.clip(moves, -2 ** 31, 2 ** 31 - 1).astype(np.int32)             # only "zero or not" counts
    return states, np.ascontiguousarray(lengths), moves, (cs, ce), n_raw, heads, n_signals, min(covered, n_raw)


def move_classes_host(states, heads, clipped_start, clipped_end):
    """cls uint8 [M]: the merged event's own k-mer is one byte that is not 'N', outside the clips; widened by two each way."""
    at = states[heads]
    m = int(heads.size)
    core = (at == at[:, :1]).all(axis=1) & (at[:, 0] != ord("N"))
    j = np.arange(m)
    core &= (j >= int(clipped_start)) & (j < m - int(clipped_end))
    cls = core.copy()
    for d in range(1, WIDEN + 1):
        cls[d:] |= core[:-d]
        cls[:-d] |= core[d:]
    return cls.astype(np.uint8)


def _label_merged(states, heads, n_signals, clipped, final):
    cls = move_classes_host(states, heads, clipped[0], clipped[1])
    return expand_events_host(cls, n_signals)[:final], base_map_host(states[heads, states.shape[1] // 2], n_signals)[:final]


def label_move_read_host(states, lengths, moves, clipped=(0, 0), n_raw=None):
    """One read -> (labels uint8 [final], basemap uint8 [final]); ``check_move_read``'s refusals."""
    states, _lengths, _moves, clipped, _n_raw, heads, n_signals, final = check_move_read(states, lengths, moves, clipped, n_raw)
    return _label_merged(states, heads, n_signals, clipped, final)


def _move_fields(read):
    if isinstance(read, dict):
        return (read["states"], read["lengths"], read["moves"], read.get("clipped", (0, 0)),
                read.get("n_raw", len(read["raw"]) if read.get("raw") is not None else None))
    read = tuple(read)
    if not 3 <= len(read) <= 5:
        raise ValueError("a read is (states, lengths, moves[, clipped[, n_raw]]) or a dict with those keys")
    return read + ((0, 0), None)[len(read) - 3:]


class MoveBatch(TableBatch):
    """Many reads' move tables, packed -- what ``cf_label_moves`` takes: ``states`` uint8 [n_events, k], ``lengths`` float32 or
    float64 [n_events] (seconds, one dtype per batch), ``moves`` int32 [n_events], ``event_offsets`` int64 [n_reads + 1],
    ``clipped`` int32 [n_reads, 2], ``n_raw`` int64 [n_reads]; and what the host's own merge found: ``final`` int64 [n_reads]
    (labels per read), ``merged`` int64 [n_reads] (M) and ``sample_offsets`` int64 [n_reads + 1], the exclusive sum of ``final``."""
    ENTRY, WORK_BYTES = "cf_label_moves", "cf_label_moves_work_bytes"

    def __init__(self, states, lengths, moves, event_offsets, clipped, n_raw, final, merged):
        self.states, self.lengths, self.moves, self.event_offsets, self.clipped, self.n_raw = states, lengths, moves, event_offsets, clipped, n_raw
        self.final, self.merged = final, merged
        self.sample_offsets = np.zeros(len(final) + 1, dtype=np.int64)
        np.cumsum(final, out=self.sample_offsets[1:])

    kmer = property(lambda self: int(self.states.shape[1]))

    def k_of(self, kmer=None):
        """The k-mers come with the events: whatever k the caller has in mind, the labels are made with the tables' own."""
        return self.kmer

    def device_tables(self, up):
        return [up(self.states.reshape(-1)), up(self.lengths), int(self.lengths.dtype == np.float64), up(self.moves), up(self.event_offsets),
                up(self.clipped.reshape(-1)), up(self.n_raw), up(self.sample_offsets)]

    def work_args(self):
        return (self.n_reads, self.n_events)

    def base_edges(self):
        """A base per merged event of ``merge_moves_host``, cut at the read's ``final``; merged events left with no sample are dropped."""
        edges, base_offsets = [np.zeros(1, dtype=np.int64)], np.zeros(self.n_reads + 1, dtype=np.int64)
        for r in range(self.n_reads):
            _states, lengths, moves, _clipped, _n_raw = self.read(r)
            _heads, n_signals = merge_moves_host(lengths, moves)
            ends = np.minimum(np.cumsum(n_signals), int(self.final[r]))
            ends = ends[np.concatenate(([True], ends[1:] > ends[:-1])) & (ends > 0)]
            edges.append(ends + int(self.sample_offsets[r]))
            base_offsets[r + 1] = base_offsets[r] + ends.size
        return np.concatenate(edges), base_offsets

    @classmethod
    def from_reads(cls, reads):
        """``reads``: one ``(states, lengths, moves[, clipped[, n_raw]])`` tuple, or one dict with those keys (``load_move_npz``
        gives such dicts; their ``raw`` supplies ``n_raw``), per read.  Every refusal of ``check_move_read`` is made here; reads
        whose k or whose length dtype differ, and a batch of 2^31 or more events or samples, are refused too."""
        checked = [check_move_read(*_move_fields(read)) for read in reads]
        if len({c[0].shape[1] for c in checked}) > 1 or len({c[1].dtype for c in checked}) > 1:
            raise ValueError("the reads of one batch share one k and one length dtype")
        n_events = sum(c[0].shape[0] for c in checked)
        total = sum(c[7] for c in checked)
        if n_events >= 2 ** 31 or total >= 2 ** 31:
            raise ValueError("a batch of 2^31 or more events or samples (%d events, %d samples): label it in parts" % (n_events, total))
        event_offsets = np.zeros(len(checked) + 1, dtype=np.int64)
        np.cumsum(np.array([c[0].shape[0] for c in checked], dtype=np.int64), out=event_offsets[1:])
        if not checked:
            return cls(np.zeros((0, 5), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int32), event_offsets, np.zeros((0, 2), np.int32),
                       np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
        return cls(np.concatenate([c[0] for c in checked]), np.concatenate([c[1] for c in checked]), np.concatenate([c[2] for c in checked]),
                   event_offsets, np.array([c[3] for c in checked], dtype=np.int32).reshape(-1, 2),
                   np.array([c[4] for c in checked], dtype=np.int64), np.array([c[7] for c in checked], dtype=np.int64),
                   np.array([c[5].size for c in checked], dtype=np.int64))

    def read(self, r):
        """Read ``r``'s (states, lengths, moves, (cs, ce), n_raw)."""
        a, b = int(self.event_offsets[r]), int(self.event_offsets[r + 1])
        return self.states[a:b], self.lengths[a:b], self.moves[a:b], (int(self.clipped[r, 0]), int(self.clipped[r, 1])), int(self.n_raw[r])

    def read_labels_host(self, r, kmer, base_map):
        states, lengths, moves, clipped, n_raw = self.read(r)
        heads, n_signals = merge_moves_host(lengths, moves)
        return _label_merged(states, heads, n_signals, clipped, min(int(n_signals.sum()), n_raw))


def label_moves(batch, device=None, base_map=False):
    """The batch's labels on the card through ``cf_label_moves``: (labels, sample_offsets), or (labels, basemap, sample_offsets) with
    ``base_map=True`` -- torch tensors on ``device`` (default: the current GPU): uint8 [sum(final)] with ``MoveBatch.label_host``'s
    bytes, and the int64 [n_reads + 1] offsets of the reads in them.  Asynchronous on torch's current stream.  No GPU or no native
    library is an error: there is no fall-back here."""
    labels, bmap, tables = label_on_card(batch, None, label_device(device, ("label_moves", "MoveBatch")), base_map)
    return (labels, bmap, tables[-1]) if base_map else (labels, tables[-1])


def load_move_npz(path):
    """One read with its basecaller's move table: ``raw``, ``event_state`` (``S<k>``, ``U<k>`` or uint8 [E, k]), ``event_move``,
    ``event_length`` (float32 or float64 seconds, the dtype kept), and optionally ``clipped_start`` / ``clipped_end`` (absent: 0) ->
    dict(raw, states, lengths, moves, clipped) as ``MoveBatch.from_reads`` takes it.  ``convert.convert_moves`` writes such files."""
    with np.load(path, allow_pickle=False) as z:
        for key in ("raw", "event_state", "event_move", "event_length"):
            if key not in z.files:
                raise ValueError("%s: no %r (a move .npz holds raw, event_state, event_move and event_length)" % (path, key))
        clip = lambda key: _as_int(z[key], key) if key in z.files else 0     # noqa: E731
        return {"raw": np.asarray(z["raw"]).reshape(-1), "states": as_states(z["event_state"]), "lengths": np.asarray(z["event_length"]).reshape(-1),
                "moves": _as_ints(z["event_move"], "event_move"), "clipped": (clip("clipped_start"), clip("clipped_end"))}


def load_labelled_move_npz(path):
    """(raw[:final], labels) of one move ``.npz``, labelled on the host: what ``train_validate.load_npz`` returns for the ``raw`` +
    ``base_labels`` file made from it."""
    read = load_move_npz(path)
    labels, _ = label_move_read_host(read["states"], read["lengths"], read["moves"], read["clipped"], len(read["raw"]))
    return read["raw"][:labels.size], labels


def moves_from_env(value):
    """``CATFISH_LABEL_MOVES``: "1" -- the directories hold move files; unset (None), empty or "0" -- they do not."""
    if value is None or value.strip() in ("", "0"):
        return False
    if value.strip() != "1":
        raise ValueError("CATFISH_LABEL_MOVES must be 1 (or unset), got %r" % (value,))
    return True


class LabelSource(object):
    """What a run's ``.npz`` directories hold, decided once: ``kind`` "labels" (``raw`` + ``base_labels``), "events" (event files,
    labelled with the odd k-mer size ``kmer``) or "moves" (move files; ``kmer`` is None: the k-mers come with the events)."""
    KINDS = ("labels", "events", "moves")

    def __init__(self, kind="labels", kmer=None):
        if kind not in self.KINDS:
            raise ValueError("a label source is one of %s, got %r" % (", ".join(self.KINDS), kind))
        self.kind, self.kmer = kind, check_kmer(kmer) if kind == "events" else None

    @classmethod
    def from_env(cls, environ=os.environ):
        """The source ``CATFISH_LABEL_KMER`` / ``CATFISH_LABEL_MOVES`` name (``kmer_from_env``, ``moves_from_env``; neither set:
        "labels").  The package reads the two variables here and nowhere else; both at once is a ValueError."""
        kmer = kmer_from_env(environ.get("CATFISH_LABEL_KMER"))
        if not moves_from_env(environ.get("CATFISH_LABEL_MOVES")):
            return cls("labels") if kmer is None else cls("events", kmer)
        if kmer is not None:
            raise ValueError("CATFISH_LABEL_MOVES and CATFISH_LABEL_KMER exclude each other: a directory holds move files or event files")
        return cls("moves")

    has_tables = property(lambda self: self.kind != "labels")

    def _per_kind(self, events, moves):
        if not self.has_tables:
            raise ValueError("labelled reads come without tables (train_validate.load_npz reads them)")
        return events if self.kind == "events" else moves

    def load(self, path):
        """One file's read as ``batch`` takes it: the dict of ``load_event_npz`` / ``load_move_npz``."""
        return self._per_kind(load_event_npz, load_move_npz)(path)

    def batch(self, reads):
        """``EventBatch.from_reads`` / ``MoveBatch.from_reads``."""
        return self._per_kind(EventBatch, MoveBatch).from_reads(reads)

    def loader(self):
        """The ``path -> (raw, labels)`` loader of this kind of file: ``train_validate.load_npz`` itself, or one that labels each
        read on the host on the way in -- the ``(raw, labels)`` the ``raw`` + ``base_labels`` file made from it would give."""
        if self.kind == "moves":
            return load_labelled_move_npz
        if self.kind == "events":
            return lambda path: load_labelled_event_npz(path, self.kmer)
        from .train_validate import load_npz
        return load_npz


def synthetic_move_read(length, seed, stay=0.5, dtype=np.float32):
    """``synthetic_event_read`` with its event table as a basecaller would have written it: every event split into a head and, with
    probability ``stay`` each time, further stays; lengths in seconds as ``dtype``; 5-mers around each base.
    -> (raw float64 [length], states uint8 [E, 5], lengths dtype [E], moves int32 [E])."""
    raw, bases, samples = synthetic_event_read(length, seed)
    rng = np.random.default_rng(seed + 7919)
    padded = np.concatenate((bases[:1], bases[:1], bases, bases[-1:], bases[-1:]))
    kmers = np.lib.stride_tricks.sliding_window_view(padded, 5)
    states, lengths, moves = [], [], []
    for e in range(bases.size):
        parts = 1
        while parts < int(samples[e]) and rng.random() < stay:
            parts += 1
        cuts = np.sort(rng.choice(np.arange(1, int(samples[e])), size=parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
        for q, n in enumerate(np.diff(np.concatenate(([0], cuts, [int(samples[e])])))):
            states.append(kmers[e])
            lengths.append(n / float(FREQUENCY))
            moves.append(0 if q else 1)
    return raw, np.array(states, dtype=np.uint8), np.array(lengths, dtype=dtype), np.array(moves, dtype=np.int32)
