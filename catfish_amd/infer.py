"""Read-level inference -- the reference's catfish/infer.py surface on the MI355X engine.

Function names, arguments, return types and error behaviour follow the reference
(catfish/infer.py:12-198); the three per-sample Python loops of the reference's
post-processing (:138, :153-157, :186-190; ~2 M samples/s/core) are replaced by
vectorised run-length arithmetic with identical results (tests/golden/postproc_golden.json
holds outputs of the reference's own functions).
"""
from __future__ import annotations

import os

import numpy as np

from .tilings import check_phases, check_weight      # noqa: F401  (phases / vote_weight are accepted wherever max_gap is)

WINDOW_SIZE = 35


# --------------------------------------------------------------------------- raw signal
def normalize_raw_signal(raw, norm_method):
    """infer.py:96-105: (raw - median) / median(|raw - median|); unknown method -> ValueError."""
    if norm_method != "median":
        raise ValueError("norm_method not recognized")
    raw = np.asarray(raw)
    shift = np.median(raw)
    scale = np.median(np.abs(raw - shift))
    return (raw - shift) / scale


def _trimmed_fast5_signal(fast5_file):
    """infer.py:87-90: the raw DAC samples of the single read after the leader (``first_sample_template``)."""
    first_sample = fast5_file["Analyses/Segmentation_000/Summary/segmentation"].attrs["first_sample_template"]
    read_name = fast5_file["Raw/Reads/"].visit(str)
    raw_signal = fast5_file["Raw/Reads/" + read_name + "/Signal"][()]
    return raw_signal[first_sample:]


def process_signal(fast5_file, normalization="median"):
    """infer.py:77-93: trim the leader (``first_sample_template``) and normalise.

    ``fast5_file`` is an open h5py.File, exactly as in the reference.
    """
    return normalize_raw_signal(_trimmed_fast5_signal(fast5_file), normalization)


def _read_npy_int16(path):
    """Fast path for the common case of a directory of reads: a version-1/2 ``.npy`` holding a one-dimensional C-order
    little-endian int16 array, read with one ``read()`` and no literal_eval (np.load spends ~80 us per file in its
    header parser, which bounds a rank at ~50 M samples/s).  Anything else returns None and goes through np.load."""
    with open(path, "rb") as fh:
        buf = fh.read()
    if len(buf) < 12 or buf[:6] != b"\x93NUMPY" or buf[6] not in (1, 2):
        return None
    if buf[6] == 1:
        hlen, off = int.from_bytes(buf[8:10], "little"), 10
    else:
        hlen, off = int.from_bytes(buf[8:12], "little"), 12
    header = buf[off:off + hlen]
    if b"'descr': '<i2'" not in header or b"'fortran_order': False" not in header:
        return None
    a, b = header.find(b"'shape': ("), header.find(b")", header.find(b"'shape': ("))
    if a < 0 or b < 0:
        return None
    dims = [d for d in header[a + 10:b].split(b",") if d.strip()]
    if len(dims) != 1 or not dims[0].strip().isdigit():
        return None
    n = int(dims[0])
    if len(buf) != off + hlen + 2 * n:
        return None
    return np.frombuffer(buf, dtype="<i2", count=n, offset=off + hlen)


def load_dac(path):
    """Raw samples of one read after the leader trim, NOT normalised (what the device ingest path uploads).

    ``.fast5`` needs h5py (reference behaviour, infer.py:27-29); because h5py/libhdf5 are not
    part of the MI355X image, ``.npy`` (int16 DAC after the leader trim), ``.npz`` (key ``raw``
    or ``signal``; the reference's NPZ layout, networks/reader.py:11-23) and headerless
    little-endian int16 ``.bin``/``.raw`` files are accepted too.
    """
    if not os.path.exists(path):
        raise ValueError("path to FAST5 is not correct.")      # infer.py:25-26
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        raw = _read_npy_int16(path)
        if raw is None:
            raw = np.load(path, allow_pickle=False)
    elif ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            raw = z["raw"] if "raw" in z.files else z["signal"]
    elif ext in (".bin", ".raw"):
        raw = np.fromfile(path, dtype="<i2")
    else:
        try:
            import h5py
        except ImportError:
            raise ImportError("reading %s needs h5py, which is not installed; convert the read to "
                              ".npy/.npz/.bin (int16 DAC samples)" % path)
        with h5py.File(path, "r") as fast5:
            raw = _trimmed_fast5_signal(fast5)
    return np.asarray(raw).reshape(-1)


def is_dac(raw):
    """True when ``raw`` can go up as int16 DAC codes unchanged (the device normalisation is exact on those)."""
    raw = np.asarray(raw)
    if raw.dtype == np.int16:
        return True
    if raw.dtype.kind in "iu" and raw.size:
        return int(raw.min()) >= -32768 and int(raw.max()) <= 32767
    return raw.dtype.kind in "iu"


def load_raw(path):
    """One read, trimmed and normalised (process_signal's result for any of ``load_dac``'s formats)."""
    return normalize_raw_signal(load_dac(path), "median")


def padding_size_for(length, window_size=WINDOW_SIZE):
    """infer.py:32-36: pad to a multiple of the window; a multiple gets a FULL extra window."""
    if not (length / window_size).is_integer():
        return window_size - (length - (length // window_size * window_size))
    return 35


def reshape_input(data, window, n_inputs):
    """infer.py:108-124 (a failed reshape is printed and swallowed there; same here)."""
    try:
        data = np.reshape(data, (-1, window, n_inputs))
    except ValueError:
        print(len(data))
        print(len(data[0]))
    return data


# --------------------------------------------------------------------------- classified output
def class_from_threshold(predicted_scores, threshold=0.5):
    """infer.py:128-138 -> list of ints."""
    return (np.asarray(predicted_scores) >= threshold).astype(np.int64).tolist()


def _run_length(values):
    """values[n] -> (run values, run starts, run lengths)."""
    v = np.asarray(values)
    n = v.shape[0]
    if n == 0:
        raise IndexError("list index out of range")   # the reference indexes predictions[0]
    starts = np.concatenate(([0], np.flatnonzero(v[1:] != v[:-1]) + 1))
    lengths = np.diff(np.concatenate((starts, [n])))
    return v[starts], starts, lengths


def correct_short(predictions, threshold=15):
    """infer.py:174-198: non-zero runs shorter than ``threshold`` are set to 0."""
    vals, _starts, lengths = _run_length(predictions)
    vals = np.where((vals != 0) & (lengths < threshold), 0, vals)
    return np.repeat(vals, lengths)


def check_bridge(max_gap, min_run=15):
    """``max_gap`` as an int, after checking the pair against what the on-card post-processing takes: ``min_run >= 1``,
    ``max_gap >= 0`` and, when bridging is on, ``min_run + max_gap <= 64`` (its window has one 64-sample word of halo).  The same
    rule holds on the host route, so that a pair never gives results on one route and an error on the other."""
    if max_gap is None:
        return 0
    if isinstance(max_gap, bool) or int(max_gap) != max_gap:
        raise ValueError("max_gap must be an int, got %r" % (max_gap,))
    max_gap, min_run = int(max_gap), int(min_run)
    if max_gap < 0:
        raise ValueError("max_gap must be >= 0, got %d" % max_gap)
    if max_gap > 0 and (min_run < 1 or min_run + max_gap > 64):
        raise ValueError("bridging needs min_run >= 1 and min_run + max_gap <= 64, got min_run %d, max_gap %d" % (min_run, max_gap))
    return max_gap


def bridge_gaps(bits, max_gap):
    """The definition of bridging, over ONE read's real samples (``bits`` = float32 p >= float32 threshold, NaN is false): a maximal
    run of zeros of at most ``max_gap`` samples with a one directly before it and a one directly after it becomes ones.  Zeros that
    touch the read's first or last sample are never filled.  ``max_gap <= 0`` is the identity.  The labels of a read are
    ``correct_short(bridge_gaps(bits, max_gap), min_run)``; ``cf_postprocess_spans_bridged`` computes them on the card."""
    b = np.asarray(bits).astype(np.int64).copy()
    n = len(b)
    if max_gap <= 0 or n == 0:
        return b
    e = np.flatnonzero(np.diff(b)) + 1
    for s, t in zip(np.concatenate([[0], e]), np.concatenate([e, [n]])):
        if b[s] == 0 and s > 0 and t < n and t - s <= max_gap:
            b[s:t] = 1
    return b


def hp_in_pred(predictions, extension_left=11, extension_right=16, label=1):
    """infer.py:141-162: each run of ``label`` -> [start - 11, start + length + 16] (end exclusive;
    spans may start below 0 or end beyond the read, exactly like the reference)."""
    vals, starts, lengths = _run_length(predictions)
    sel = vals == label
    return [[int(s) - extension_left, int(s) + int(ln) + extension_right]
            for s, ln in zip(starts[sel], lengths[sel])]


# --------------------------------------------------------------------------- inference
def _engine_read(raw_in, engine, length, rule):
    """One padded, windowed read on the card: the shared chain of ``calling.py`` and the one-launch post-processing; neither the
    probabilities nor (with ``rule.scores``) the signal come down.  -> ``calling.results_of_runs``' entry of the read."""
    import torch
    from . import calling
    x_host = np.ascontiguousarray(np.asarray(raw_in, dtype=np.float32).reshape(-1, WINDOW_SIZE))
    total = x_host.size
    dev = torch.device("cuda", engine.device)
    x_all, x = calling.tiling_buffer(rule, x_host.shape[0], 1, dev)
    x.copy_(torch.from_numpy(x_host))
    s_off, lengths = np.array([0, total], dtype=np.int64), np.array([length], dtype=np.int64)
    off, lens = torch.from_numpy(s_off).to(dev), torch.from_numpy(lengths).to(dev)
    probs, _probs_all = calling.forward_voted(engine, rule, x_all, off, lens, total)
    out = engine.postprocess_spans_device(probs, off, lens, scores=rule.scores, signal=x.view(-1) if rule.scores else None,
                                          max_gap=rule.max_gap)
    return calling.results_of_runs(out[0], out[1], s_off, lengths, out[2] if rule.scores else None)[0]


def _host_read(raw_in, model, length, rule):
    """The same for a model without an engine, by the numpy definitions over ``model.infer``."""
    from .calling import results_of_runs
    from .span_scores import scores_of_runs
    from .tilings import voted_probs_of_read
    x = np.ascontiguousarray(np.asarray(raw_in, dtype=np.float32).reshape(-1))
    if rule.voted:
        probs = voted_probs_of_read(raw_in, model.infer, length, rule.phases, rule.vote_weight)
    else:
        probs = np.asarray(model.infer(raw_in)).reshape(-1)
    labels = np.asarray(correct_short(bridge_gaps(class_from_threshold(probs[:length]), rule.max_gap)))
    edges = np.diff(np.concatenate(([0], labels, [0])))
    starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    s_off, lengths = np.array([0, x.shape[0]], dtype=np.int64), np.array([length], dtype=np.int64)
    # the rows describe the runs that are returned: bridged runs hold samples below the threshold, and a probability may round across
    # the threshold on its way to float32 (``span_scores_host`` would find other runs then)
    flat = scores_of_runs(probs.astype(np.float32), x, starts, ends, s_off, 1) if rule.scores else None
    return results_of_runs(starts, ends, s_off, lengths, flat)[0]


def infer_class_from_raw(raw, model, label=1, window_size=WINDOW_SIZE, scores=False, max_gap=0, phases=(0,), vote_weight="mean"):
    """Body of infer_class_from_signal (infer.py:31-51) for an already normalised signal.

    ``max_gap > 0`` bridges gaps of at most that many samples between two called stretches before ``correct_short``
    (``bridge_gaps``); 0 changes nothing.

    ``scores=True`` returns a third value: a float64 array [n_spans, 6], one row per span in span order, columns n, mean_p,
    min_p, max_p, level, spread (``span_scores.SCORE_COLUMNS``).

    ``phases`` (``check_phases``; more than one needs the 35-sample window) asks the network once per tiling -- the read shifted
    right by that many samples before it is cut into windows -- and merges the per-sample probabilities by ``vote_weight``
    (``"mean"`` or ``"centre"``, ``tilings.vote_host``) before the threshold; ``(0,)`` changes nothing."""
    raw = np.asarray(raw)
    padding_size = padding_size_for(len(raw), window_size)
    length = len(raw)
    raw = np.hstack((raw, np.array(padding_size * [0])))
    raw_in = reshape_input(raw, window_size, 1)
    from .calling import CallRule
    rule = CallRule.of(max_gap=max_gap, phases=phases, vote_weight=vote_weight, scores=scores)
    if rule.voted and window_size != WINDOW_SIZE:
        raise ValueError("shifted-window voting needs window_size %d, got %r" % (WINDOW_SIZE, window_size))
    if rule.voted or rule.bridged or rule.scores:
        if hasattr(model, "_require_engine"):
            model._require_engine()
        engine = getattr(model, "engine", None)
        return _engine_read(raw_in, engine, length, rule) if engine is not None else _host_read(raw_in, model, length, rule)
    scores = model.infer(raw_in)
    scores = scores[:-padding_size]
    labels = correct_short(class_from_threshold(scores))
    predicted_hps = hp_in_pred(labels)
    return predicted_hps, len(labels)


def infer_class_from_signal(fast5_file, model, label=1, window_size=WINDOW_SIZE, scores=False, max_gap=0, phases=(0,), vote_weight="mean"):
    """infer.py:12-51.  Returns (list of [start, end] homopolymer spans, length of the read), and the score rows of
    ``infer_class_from_raw`` as a third value with ``scores=True``; ``max_gap``, ``phases`` and ``vote_weight`` as there."""
    raw = load_raw(fast5_file)
    return infer_class_from_raw(raw, model, label=label, window_size=window_size, scores=scores, max_gap=max_gap, phases=phases,
                                vote_weight=vote_weight)


def infer_class_from_npz(npz_file, model, label=1, window_size=WINDOW_SIZE):
    """infer.py:54-73: spans of the TRUE labels stored in an NPZ (no network involved)."""
    if not os.path.exists(npz_file):
        raise ValueError("path to NPZ is not correct.")
    with np.load(npz_file, allow_pickle=False) as z:
        labels = z["base_labels"]
    return hp_in_pred(labels, 0, 0), len(labels)
