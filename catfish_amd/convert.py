"""FAST5 reads -> the int16 ``.npy`` reads the MI355X path ingests natively.

The reference opens every read with h5py (catfish/infer.py:27-29) and keeps the DAC samples behind the leader
(``process_signal``, infer.py:77-93: ``Signal[first_sample_template:]``).  Neither image of this build holds h5py / libhdf5, so
the directory the CLI classifies is made of one-dimensional little-endian int16 ``.npy`` files holding exactly those samples (what
``infer.load_dac`` returns for the FAST5) -- the format the library's loader pool reads straight into pinned memory
(``cf_listing_load_npy_int16``) and the split step writes.  This module is the bridge, to be run once WHERE the FAST5 files and an
h5py live:

    python -m catfish_amd.convert -i fast5_dir -o npy_dir

``read_x.fast5`` becomes ``read_x.npy`` (the name up to its first dot -- what the split step names its pieces after -- is kept).
With h5py installed the CLI also takes FAST5 directly (``infer.load_dac``, one file at a time through the general loader).

``--events`` converts Tombo-resquiggled reads for TRAINING instead: ``read_x.fast5`` becomes ``read_x.npz`` with the normalised
signal and the corrected event table (``convert_events``), from which ``catfish_amd.labelling`` makes the per-sample labels for any
k-mer size.  ``--moves`` converts base-called reads that were NOT resquiggled: ``read_x.npz`` holds the normalised signal and the
basecaller's own Events table (``convert_moves``; ``CATFISH_LABEL_MOVES=1`` labels and trains from a directory of them).
"""
from __future__ import annotations

import os

import numpy as np

from . import infer
from .split import npy_header


def convert_read(src, dst):
    """One read: ``infer.load_dac(src)`` (leader trimmed, NOT normalised) written as an int16 ``.npy``; -> its length in samples.
    ValueError for a wrong path or samples that are not int16 codes, ImportError without h5py (``load_dac``'s own errors)."""
    dac = np.asarray(infer.load_dac(src)).reshape(-1)
    if not infer.is_dac(dac):
        raise ValueError("%s: the signal does not hold int16 DAC codes (dtype %s)" % (src, dac.dtype))
    dac = np.ascontiguousarray(dac, dtype="<i2")
    tmp = dst + ".part"
    with open(tmp, "wb") as fh:
        fh.write(npy_header(dac.shape[0]) + dac.tobytes())
    os.replace(tmp, dst)                                    # a reader of the directory never sees half a file
    return int(dac.shape[0])


TOMBO_PATH = "Analyses/RawGenomeCorrected_000/"


def _clipped_bases(fast5, end, default):
    """``TrainingRead.clipped_bases_start`` / ``_end``: the Alignment's ``clipped_bases_<end>``, else its ``trimmed_obs_<end>``,
    else the default (the reference's ``--clipped-bases``)."""
    alignment = TOMBO_PATH + "BaseCalled_template/Alignment"
    if alignment in fast5:
        attrs = fast5[alignment].attrs
        for name in ("clipped_bases_" + end, "trimmed_obs_" + end):
            if name in attrs:
                return int(attrs[name])
    return int(default)


def convert_events(src, dst_npz, clipped_bases=None):
    """One Tombo-resquiggled read -> an event ``.npz`` (``labelling.load_event_npz`` reads it; ``CATFISH_LABEL_KMER`` trains from a
    directory of them); -> its length in samples.  ``raw`` is the signal as ``TrainingRead.raw`` holds it --
    ``Signal[read_start_rel_to_raw:]``, median / MAD normalised -- cut to ``final_signal``; ``event_base``, ``event_length`` and
    ``event_start`` are the corrected Events table's columns; ``clipped_start`` / ``clipped_end`` come from the Alignment's
    attributes with the reference's fall-backs (``clipped_bases``: its default of 10).  No k-mer size goes in: the labels are made
    when the file is read.  ValueError for a wrong path or a table ``labelling.check_read`` refuses, ImportError without h5py."""
    from . import labelling
    if not os.path.exists(src):
        raise ValueError("path to FAST5 is not correct: %s" % src)
    try:
        import h5py
    except ImportError:
        raise ImportError("reading %s needs h5py, which is not installed" % src)
    default = labelling.DEFAULT_CLIPPED if clipped_bases is None else clipped_bases
    with h5py.File(src, "r") as fast5:
        events = fast5[TOMBO_PATH + "BaseCalled_template/Events"]
        first_sample = int(events.attrs["read_start_rel_to_raw"])
        lengths, bases, starts = np.asarray(events["length"]), np.asarray(events["base"]), np.asarray(events["start"])
        clipped = (_clipped_bases(fast5, "start", default), _clipped_bases(fast5, "end", default))
        read_name = fast5["Raw/Reads/"].visit(str)
        signal = np.asarray(fast5["Raw/Reads/" + read_name + "/Signal"][()]).reshape(-1)
    raw = infer.normalize_raw_signal(signal[first_sample:], "median")
    bases, lengths, clipped, final = labelling.check_read(bases, lengths, clipped, starts, n_raw=len(raw))
    tmp = dst_npz + ".part"
    with open(tmp, "wb") as fh:
        np.savez(fh, raw=raw[:final], event_base=bases.view("S1"), event_length=lengths, event_start=np.cumsum(lengths) - lengths,
                 clipped_start=np.int64(clipped[0]), clipped_end=np.int64(clipped[1]))
    os.replace(tmp, dst_npz)
    return final


BASECALL_PATH = "Analyses/Basecall_1D_000"     # the reference's --hdf-path for reads that were not resquiggled


def convert_moves(src, dst_npz, clipped_bases=None, hdf_path=BASECALL_PATH):
    """One base-called read -> a move ``.npz`` (``labelling.load_move_npz`` reads it; ``CATFISH_LABEL_MOVES=1`` trains from a
    directory of them); -> the number of labels it yields.  ``raw`` is the signal as ``TrainingRead.raw`` holds it with
    ``use_tombo=False`` -- ``Signal[first_sample_template:]`` of ``Analyses/Segmentation_000``, median / MAD normalised, whole: its
    length is where the labels are cut; ``event_state`` (``S<k>``), ``event_move`` and ``event_length`` (seconds, the table's own
    dtype) are the columns ``model_state``, ``move`` and ``length`` of ``<hdf_path>/BaseCalled_template/Events``;
    ``clipped_start`` / ``clipped_end`` as in ``convert_events``.  ValueError for a wrong path (the reference's words for a wrong
    ``hdf_path``) or a table ``labelling.check_move_read`` refuses, ImportError without h5py."""
    from . import labelling
    if not os.path.exists(src):
        raise ValueError("path to FAST5 is not correct: %s" % src)
    try:
        import h5py
    except ImportError:
        raise ImportError("reading %s needs h5py, which is not installed" % src)
    default = labelling.DEFAULT_CLIPPED if clipped_bases is None else clipped_bases
    hdf_path = hdf_path if hdf_path.endswith("/") else hdf_path + "/"
    with h5py.File(src, "r") as fast5:
        if hdf_path not in fast5:
            raise ValueError("hdf path not in hdf file!")
        if hdf_path + "BaseCalled_template" not in fast5:
            raise ValueError("hdf path in hdf file, but does not contain BaseCalled_template results!")
        events = fast5[hdf_path + "BaseCalled_template/Events"]
        lengths, states, moves = np.asarray(events["length"]), np.asarray(events["model_state"]), np.asarray(events["move"])
        first_sample = int(fast5["Analyses/Segmentation_000/Summary/segmentation"].attrs["first_sample_template"])
        clipped = (_clipped_bases(fast5, "start", default), _clipped_bases(fast5, "end", default))
        read_name = fast5["Raw/Reads/"].visit(str)
        signal = np.asarray(fast5["Raw/Reads/" + read_name + "/Signal"][()]).reshape(-1)
    raw = infer.normalize_raw_signal(signal[first_sample:], "median")
    checked = labelling.check_move_read(states, lengths, moves, clipped, n_raw=len(raw))
    states, lengths, moves, clipped, final = checked[0], checked[1], checked[2], checked[3], checked[7]
    tmp = dst_npz + ".part"
    with open(tmp, "wb") as fh:
        np.savez(fh, raw=raw, event_state=states.view("S%d" % states.shape[1]).reshape(-1), event_move=moves, event_length=lengths,
                 clipped_start=np.int64(clipped[0]), clipped_end=np.int64(clipped[1]))
    os.replace(tmp, dst_npz)
    return final


def convert_directory(input_dir, output_dir, keep_going=False, events=False, moves=False):
    """Every entry of ``input_dir`` (sorted) -> ``output_dir/<name without its last extension>.npy`` (``events``: ``.npz``, through
    ``convert_events``; ``moves``: ``.npz``, through ``convert_moves``).
    -> dict(converted, samples, failed = [(name, error text)]); the first failure raises unless ``keep_going``."""
    os.makedirs(output_dir, exist_ok=True)
    done = {"converted": 0, "samples": 0, "failed": []}
    for name in sorted(os.listdir(input_dir)):
        src = os.path.join(input_dir, name)
        if os.path.isdir(src):
            continue
        try:
            if events or moves:
                done["samples"] += (convert_events if events else convert_moves)(src, os.path.join(output_dir, os.path.splitext(name)[0] + ".npz"))
                done["converted"] += 1
                continue
            done["samples"] += convert_read(src, os.path.join(output_dir, os.path.splitext(name)[0] + ".npy"))
            done["converted"] += 1
        except Exception as exc:                            # noqa: BLE001 -- reported per file; the reference aborts on the first (infer.py:25-29)
            if not keep_going:
                raise
            done["failed"].append((name, "%s: %s" % (type(exc).__name__, exc)))
    return done


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="FAST5 (or .npz / .bin) reads -> int16 .npy reads for catfish_amd")
    ap.add_argument("-i", "--input-dir", required=True)
    ap.add_argument("-o", "--output-dir", required=True)
    ap.add_argument("--keep-going", action="store_true", help="report unreadable files at the end instead of stopping at the first")
    ap.add_argument("--events", action="store_true",
                    help="Tombo-resquiggled reads -> event .npz files (normalised signal + the corrected event table) to label and train from")
    ap.add_argument("--moves", action="store_true",
                    help="base-called reads that were not resquiggled -> move .npz files (normalised signal + the basecaller's Events table)")
    args = ap.parse_args(argv)
    if args.events and args.moves:
        ap.error("--events and --moves exclude each other")
    done = convert_directory(args.input_dir, args.output_dir, keep_going=args.keep_going,
                             **({"events": True} if args.events else {"moves": True} if args.moves else {}))
    print("converted %d reads (%d samples) into %s" % (done["converted"], done["samples"], args.output_dir))
    for name, err in done["failed"]:
        print("FAILED %s: %s" % (name, err))
    return 1 if done["failed"] else 0


if __name__ == "__main__":
    raise SystemExit(main())
