"""Thin host layer over the C ABI: owns one cf_model on one MI355X.

PyTorch is used only as plumbing (device buffers, the current HIP stream);
numpy callers go through ``cf_infer_host`` and need no torch at all.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

WINDOW = N.CF_WINDOW
DEFAULT_MAX_WINDOWS = 32768   # one pass covers 256 reads of 4096 samples (30 208 windows)


def device_identity(device):
    """-> (pci bus id ``"dddd:bb:dd.f"``, uuid as 32 hex digits) of HIP device ``device`` of this process (``cf_device_identity``):
    which card a rank drives, for ``placement.verify`` and the benchmark line.  Opens the HIP runtime."""
    bus, uuid = C.create_string_buffer(64), C.create_string_buffer(33)
    N.check(N.lib().cf_device_identity(int(device), bus, 64, uuid, 33))
    return bus.value.decode("ascii", "replace").lower(), uuid.value.decode("ascii", "replace")


class HipEngine(object):
    """The forward pass of one ResNetRNN checkpoint on one GPU."""

    def __init__(self, weights, layer_size=64, n_layers=3, layer_size_res=32, n_layers_res=2,
                 device=0, max_windows_per_pass=DEFAULT_MAX_WINDOWS, bn_epsilon=1e-3, n_streams=0,
                 precision="fp32", fuse_layers=None):
        self._lib = N.lib()
        self._handle = C.c_void_p()
        if precision not in N.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(N.PRECISIONS))
        self.precision = precision
        hp = N.cf_hparams(int(layer_size), int(n_layers), int(layer_size_res), int(n_layers_res),
                          WINDOW, float(bn_epsilon), int(max_windows_per_pass), int(n_streams),
                          N.PRECISIONS[precision], 0 if fuse_layers is None else (1 if fuse_layers else -1))
        w, keep = N.build_weight_structs(weights, int(n_layers), int(n_layers_res))
        N.check(self._lib.cf_model_create(C.byref(w), C.byref(hp), int(device), C.byref(self._handle)))
        del keep  # the library copied/re-tiled everything
        self.device = int(device)
        self.n_layers = int(n_layers)
        self.n_layers_res = int(n_layers_res)
        self.layer_size = int(layer_size)
        self.layer_size_res = int(layer_size_res)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.cf_model_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_identity(self):
        """(pci bus id, uuid hex) of the card this engine drives."""
        return device_identity(self.device)

    @property
    def workspace_bytes(self):
        return int(self._lib.cf_workspace_bytes(self._handle))

    def _tensors(self, what, rows):
        """The one check of tensor arguments; each row is ``(name, tensor, torch dtype[, minimum numel])``.  ValueError for
        whatever is not a contiguous CUDA tensor of that dtype, lives on another card than the model, or is too short.  It sits on
        the path of every call (``tools/bench_latency.py``): no torch import, no object made per row."""
        for row in rows:
            t, dtype = row[1], row[2]
            try:                                               # whatever is no torch.Tensor lacks one of these
                ok = t.dtype == dtype and t.is_cuda and t.is_contiguous()
            except AttributeError:
                ok = False
            if not ok:
                raise ValueError("%s: %s must be a contiguous %s CUDA tensor" % (what, row[0], str(dtype).replace("torch.", "")))
            if t.get_device() != self.device:
                raise ValueError("%s: %s lives on cuda:%d, model on cuda:%d" % (what, row[0], t.get_device(), self.device))
            if len(row) > 3 and t.numel() < row[3]:
                raise ValueError("%s: %s needs %d elements, has %d" % (what, row[0], row[3], t.numel()))

    # ------------------------------------------------------------------ device weights
    def param_count(self):
        """Values of the flat parameter vector of this engine's geometry (``cf_model_param_floats``): the checkpoint's inference
        tensors in ``torch_ops.tensor_names`` order, flattened -- ``pack_weights(...)`` without its header."""
        if getattr(self, "_param_count", None) is None:
            n = C.c_int64()
            N.check(self._lib.cf_model_param_floats(self._handle, C.byref(n)))
            self._param_count = int(n.value)
        return self._param_count

    def load_params_device(self, params, stream=None):
        """Replace the engine's weights by ``params`` (contiguous float32 CUDA tensor of ``param_count()`` values on the engine's
        device), folded and re-tiled on the device (``cf_model_load_params``), asynchronous on ``stream`` (default: the current
        stream).  Afterwards the engine computes exactly what ``HipEngine`` built from the same values computes.  The first call
        builds the gather map (host work, one upload); later calls only launch.  fp32 engines only: ValueError otherwise."""
        import torch
        self._tensors("load_params_device", [("params", params, torch.float32)])
        if params.numel() != self.param_count():
            raise ValueError("load_params_device: params must hold %d values, got %d" % (self.param_count(), params.numel()))
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_model_load_params(self._handle, N._p(params), N.stream_ptr(stream)))

    # ------------------------------------------------------------------ inference
    @staticmethod
    def _check_windows(shape):
        if len(shape) == 3 and shape[2] == 1:
            shape = shape[:2]
        if len(shape) != 2 or shape[1] != WINDOW:
            raise ValueError("input must be [n_windows, %d(, 1)], got %s" % (WINDOW, tuple(shape)))
        return int(shape[0])

    def infer_host(self, x, return_logits=False):
        """numpy [N,35(,1)] any float dtype -> numpy float32 [N*35] (H2D/D2H inside).

        ``return_logits=True`` -> (probs, logits): the pre-sigmoid values of rnn_class.py:178-183."""
        x = np.asarray(x)
        n = self._check_windows(x.shape)
        x32 = np.ascontiguousarray(x.reshape(n, WINDOW), dtype=np.float32)
        out = np.empty(n * WINDOW, dtype=np.float32)
        if return_logits:
            logits = np.empty(n * WINDOW, dtype=np.float32)
            N.check(self._lib.cf_infer_host_logits(self._handle, N.np_ptr(x32), n, N.np_ptr(out), N.np_ptr(logits)))
            return out, logits
        N.check(self._lib.cf_infer_host(self._handle, N.np_ptr(x32), n, N.np_ptr(out)))
        return out

    def check_error(self):
        """Raise if an earlier asynchronous launch of this model reported a device-side error (call after a sync)."""
        N.check(self._lib.cf_check_error(self._handle))

    def clear_error(self):
        """Reset the sticky device-side error after the results of the failed launch have been dropped (``cf_clear_error``):
        the engine is usable again."""
        N.check(self._lib.cf_clear_error(self._handle))

    def launch_regimes(self):
        """Switch points of the launcher (windows): dict(n_cu, hoist_max, coop_max, fuse_auto_min)."""
        out = (C.c_int64 * 4)()
        N.check(self._lib.cf_launch_regimes(self._handle, out))
        return dict(n_cu=int(out[0]), hoist_max=int(out[1]), coop_max=int(out[2]), fuse_auto_min=int(out[3]))

    def anysize_infer_shape(self, n_windows):
        """The launch of every biGRU layer of an any-size model in one pass of ``n_windows`` windows (``cf_anysize_infer_shape``;
        nothing is launched): a list of dict(kernel, waves, grid_x, lds_bytes, h_via_y), ``kernel`` one of "tuned" (the
        LDS-resident kernel: see ``launch_regimes``), "one_tile", "two_tile".  ValueError on the tuned 64 / 32 path."""
        out = (C.c_int64 * (5 * self.n_layers))()
        N.check(self._lib.cf_anysize_infer_shape(self._handle, int(n_windows), out, self.n_layers))
        return [dict(kernel=("tuned", "one_tile", "two_tile")[out[5 * l]], waves=int(out[5 * l + 1]), grid_x=int(out[5 * l + 2]),
                     lds_bytes=int(out[5 * l + 3]), h_via_y=int(out[5 * l + 4])) for l in range(self.n_layers)]

    def infer_device(self, x, out=None, stream=None, logits=None):
        """torch CUDA float32 tensor [N,35(,1)] -> torch CUDA float32 [N*35], async on the stream.

        ``logits``: optional float32 CUDA tensor of N*35 elements that receives the pre-sigmoid values."""
        import torch
        x = x.contiguous()                                     # any strides are fine for the input: it is copied here
        rows = [("x", x, torch.float32)]
        if out is not None:
            rows.append(("out", out, torch.float32))
        if logits is not None:
            rows.append(("logits", logits, torch.float32))
        self._tensors("infer_device", rows)
        n = self._check_windows(x.shape)
        if out is None:
            out = torch.empty(n * WINDOW, dtype=torch.float32, device=x.device)
        elif out.numel() != n * WINDOW:
            raise ValueError("infer_device: out must have %d elements, has %d" % (n * WINDOW, out.numel()))
        if logits is not None and logits.numel() != n * WINDOW:
            raise ValueError("infer_device: logits must have %d elements, has %d" % (n * WINDOW, logits.numel()))
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if logits is not None:
            N.check(self._lib.cf_infer_logits(self._handle, N._p(x), n, N._p(out), N._p(logits), N.stream_ptr(stream)))
            return out
        N.check(self._lib.cf_infer(self._handle, N._p(x), n, N._p(out), N.stream_ptr(stream)))
        return out

    def _check_packed(self, what, probs, read_offsets, read_lengths, own=()):
        """The packed layout every post-processing call takes: float32 ``probs``, int64 tables (and the call's ``own`` rows for
        ``_tensors``), ``n_reads + 1`` offsets -> (n_reads, total)."""
        import torch
        self._tensors(what, [("probs", probs, torch.float32), ("read_offsets", read_offsets, torch.int64),
                             ("read_lengths", read_lengths, torch.int64)] + list(own))
        n_reads = int(read_lengths.numel())
        if int(read_offsets.numel()) != n_reads + 1:
            raise ValueError("%s: read_offsets must have n_reads + 1 entries" % what)
        return n_reads, int(probs.numel())

    def postprocess_device(self, probs, read_offsets, read_lengths, threshold=0.5, min_run=15, out=None, stream=None):
        """Device threshold + correct_short over packed padded reads.

        probs: float32 CUDA [total]; read_offsets: int64 CUDA [n_reads+1] (padded sample offsets);
        read_lengths: int64 CUDA [n_reads] (real lengths) -> uint8 CUDA labels [total] (padding = 0).
        """
        import torch
        n_reads, total = self._check_packed("postprocess_device", probs, read_offsets, read_lengths)
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=probs.device)
        else:
            self._tensors("postprocess_device", [("out", out, torch.uint8, total)])
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_postprocess(self._handle, N._p(probs), N._p(read_offsets), N._p(read_lengths), n_reads, total,
                                         float(threshold), int(min_run), N._p(out), N.stream_ptr(stream)))
        return out

    def postprocess_spans_launch(self, probs, read_offsets, read_lengths, rule, signal=None, stream=None, want_labels=False, max_runs=None):
        """The asynchronous half of ``postprocess_spans_device``: threshold, bridging (``rule.bridged``), ``correct_short`` and the run
        boundaries in ONE launch (``cf_postprocess_spans`` / ``cf_postprocess_spans_bridged``), then the score rows of those runs when
        ``rule.scores`` (``span_scores_device``; by the labels when the runs are bridged).  ``rule``: a ``calling.CallRule``.  ->
        (starts, ends, counts, labels, rows), all on the card and not waited for: int64 [max_runs] (unsorted; default room
        ``rule.max_runs(total)``), int64 [2] = how many starts / ends there were (possibly more than the room), the uint8 labels
        [total] -- written only when ``want_labels`` or the scores need them, else None: the library never writes labels -- and the
        three score tensors or None."""
        import torch
        n_reads, total = self._check_packed("postprocess_spans_launch", probs, read_offsets, read_lengths)
        max_runs = rule.max_runs(total) if max_runs is None else int(max_runs)
        dev = probs.device
        labels = torch.empty(total, dtype=torch.uint8, device=dev) if want_labels or rule.scores_by_labels else None
        starts = torch.empty(max_runs, dtype=torch.int64, device=dev)
        ends = torch.empty(max_runs, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        head = (self._handle, N._p(probs), N._p(read_offsets), N._p(read_lengths), n_reads, total, rule.threshold)
        tail = (rule.min_run, N._p(labels), max_runs, N._p(starts), N._p(ends), N._p(counts), N.stream_ptr(stream))
        if rule.bridged:
            N.check(self._lib.cf_postprocess_spans_bridged(*head, rule.max_gap, *tail))
        else:
            N.check(self._lib.cf_postprocess_spans(*head, *tail))
        rows = None
        if rule.scores:
            rows = self.span_scores_device(probs, signal, read_offsets, read_lengths, starts, counts, rule.threshold, stream,
                                           labels=labels if rule.scores_by_labels else None)
        return starts, ends, counts, labels, rows

    def postprocess_spans_device(self, probs, read_offsets, read_lengths, threshold=0.5, min_run=15, max_runs=None, labels=False,
                                 stream=None, scores=False, signal=None, max_gap=0):
        """``postprocess_device`` + ``spans_device`` as ONE launch (``cf_postprocess_spans``) -> (starts, ends) numpy int64, sorted
        ascending (packed positions; ends exclusive), and the uint8 CUDA labels as a third value when ``labels=True``.

        ``scores=True`` appends the per-run score dict of ``span_scores.span_scores_host`` (``cf_span_scores`` on the same stream, its
        rows carried through the argsort of the starts; ``signal``: the float32 CUDA samples the network saw, None: ``sum_x`` and
        ``sum_x2`` are NaN).

        ``max_gap > 0`` bridges gaps of at most that many samples first (``cf_postprocess_spans_bridged``; ``infer.bridge_gaps`` is
        the definition); the score rows then come from ``cf_span_scores_labels`` over the labels of the same launch, so that they
        cover the samples of the bridged gaps.  A pair with ``min_run + max_gap > 64`` raises ValueError.

        ``postprocess_spans_launch`` and one wait; a run list that overflows is launched again with the true count."""
        from .calling import CallRule
        rule = CallRule.of(threshold, min_run, max_gap, scores=scores)
        starts, ends, counts, lab, rows = self.postprocess_spans_launch(probs, read_offsets, read_lengths, rule, signal, stream, labels, max_runs)
        n_s, n_e = (int(v) for v in counts.cpu().tolist())      # synchronises the stream
        self.check_error()
        if n_s != n_e:
            raise RuntimeError("cf_postprocess_spans: %d run starts but %d run ends" % (n_s, n_e))
        if n_s > int(starts.numel()):
            return self.postprocess_spans_device(probs, read_offsets, read_lengths, threshold, min_run, n_s, labels, stream, scores, signal,
                                                 max_gap)
        out = (np.sort(starts[:n_s].cpu().numpy()), np.sort(ends[:n_e].cpu().numpy()))
        if labels:
            out = out + (lab,)
        if scores:
            from .span_scores import scores_from_device_rows
            flat, _order = scores_from_device_rows(starts[:n_s].cpu().numpy(), rows[0][:n_s].cpu().numpy(), rows[1][:n_s].cpu().numpy(),
                                                   rows[2][:n_s].cpu().numpy(), read_offsets.cpu().numpy(), int(read_lengths.numel()),
                                                   signal is not None)
            if not np.array_equal(flat["end"], out[1]):
                raise RuntimeError("cf_span_scores: the paired ends differ from the sorted ends of cf_postprocess_spans")
            out = out + (flat,)
        return out

    def span_scores_device(self, probs, signal, read_offsets, read_lengths, starts, counts, threshold=0.5, stream=None, out=None,
                           labels=None):
        """``cf_span_scores``: for every run k < min(counts[0], len(starts)) of the start list ``cf_postprocess_spans`` wrote ->
        CUDA tensors (ends_paired int64 [max_runs], sums float64 [max_runs, 3] = sum p, sum x, sum x * x, extremes float32
        [max_runs, 2] = min p, max p); rows at and above the count are left as they were (``out``: the three tensors to write into).
        ``signal`` None: columns 1 and 2 of sums are not written.  Asynchronous on the stream: the count is read on the card.
        ``labels`` (uint8 CUDA [total], what ``cf_postprocess_spans_bridged`` wrote): a run lasts while its labels are non-zero
        instead of while ``p >= threshold`` (``cf_span_scores_labels``) -- bridged runs hold samples below the threshold."""
        import torch
        what = "span_scores_device"
        n_reads, total = self._check_packed(what, probs, read_offsets, read_lengths, [
            ("starts", starts, torch.int64), ("counts", counts, torch.int64, 1)]
            + [(name, t, dtype) for name, t, dtype in (("signal", signal, torch.float32), ("labels", labels, torch.uint8)) if t is not None])
        for name, t in (("signal", signal), ("labels", labels)):
            if t is not None and int(t.numel()) != total:
                raise ValueError("%s: %s must have as many samples as probs" % (what, name))
        max_runs = int(starts.numel())
        dev = probs.device
        if out is None:
            out = (torch.empty(max_runs, dtype=torch.int64, device=dev), torch.empty(max_runs, 3, dtype=torch.float64, device=dev),
                   torch.empty(max_runs, 2, dtype=torch.float32, device=dev))
        ends_paired, sums, extremes = out
        self._tensors(what, [("out[0]", ends_paired, torch.int64, max_runs), ("out[1]", sums, torch.float64, 3 * max_runs),
                             ("out[2]", extremes, torch.float32, 2 * max_runs)])
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if labels is not None:
            N.check(self._lib.cf_span_scores_labels(self._handle, N._p(probs), N._p(signal), N._p(labels), N._p(read_offsets),
                                                    N._p(read_lengths), n_reads, total, N._p(starts), N._p(counts), max_runs,
                                                    N._p(ends_paired), N._p(sums), N._p(extremes), N.stream_ptr(stream)))
            return out
        N.check(self._lib.cf_span_scores(self._handle, N._p(probs), N._p(signal), N._p(read_offsets), N._p(read_lengths), n_reads, total,
                                         float(threshold), N._p(starts), N._p(counts), max_runs, N._p(ends_paired), N._p(sums),
                                         N._p(extremes), N.stream_ptr(stream)))
        return out

    def spans_device(self, labels, max_runs=None, stream=None):
        """Device run-length pass over corrected labels -> (starts, ends) numpy int64, sorted ascending
        (packed positions; ends exclusive).  Only the two short lists cross PCIe."""
        import torch
        self._tensors("spans_device", [("labels", labels, torch.uint8)])
        total = int(labels.numel())
        if max_runs is None:
            max_runs = total // 15 + 16          # correct_short leaves runs of >= 15 samples
        dev = labels.device
        starts = torch.empty(max_runs, dtype=torch.int64, device=dev)
        ends = torch.empty(max_runs, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_spans(self._handle, N._p(labels), total, int(max_runs), N._p(starts), N._p(ends), N._p(counts),
                                   N.stream_ptr(stream)))
        n_s, n_e = (int(v) for v in counts.cpu().tolist())      # synchronises the stream
        self.check_error()                                        # the labels came from asynchronous launches
        if n_s != n_e:
            raise RuntimeError("cf_spans: %d run starts but %d run ends" % (n_s, n_e))
        if n_s > max_runs:
            return self.spans_device(labels, max_runs=n_s, stream=stream)
        return np.sort(starts[:n_s].cpu().numpy()), np.sort(ends[:n_e].cpu().numpy())

    def normalize_device(self, dac, dac_offsets, win_offsets, out=None, stream=None):
        """Device median/MAD normalisation + padding + window packing of many int16 reads.

        dac: int16 CUDA [total samples]; dac_offsets / win_offsets: int64 CUDA [n_reads + 1]
        -> float32 CUDA [n_windows, 35] (n_windows = win_offsets[-1], given by ``out`` or computed).
        """
        import torch
        self._tensors("normalize_device", [("dac", dac, torch.int16), ("dac_offsets", dac_offsets, torch.int64),
                                           ("win_offsets", win_offsets, torch.int64)])
        n_reads = int(dac_offsets.numel()) - 1
        if int(win_offsets.numel()) != n_reads + 1:
            raise ValueError("normalize_device: dac_offsets and win_offsets must have the same length")
        if out is None:
            out = torch.empty(int(win_offsets[-1].item()), WINDOW, dtype=torch.float32, device=dac.device)
        else:
            self._tensors("normalize_device", [("out", out, torch.float32)])
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_normalize(self._handle, N._p(dac), N._p(dac_offsets), N._p(win_offsets), n_reads, N._p(out),
                                       N.stream_ptr(stream)))
        return out

    # ------------------------------------------------------------------ shifted-window voting (csrc/tilings.hpp)
    def _check_tiling_tables(self, what, offsets, lengths, total, phases):
        import torch
        from .tilings import check_phases, tiling_size
        phases = check_phases(phases)
        self._tensors(what, [("offsets", offsets, torch.int64), ("lengths", lengths, torch.int64)])
        n, total = int(lengths.numel()), int(total)
        if int(offsets.numel()) != n + 1:
            raise ValueError("%s: offsets must have n_reads + 1 entries" % what)
        if total < 0:
            raise ValueError("%s: negative total" % what)
        return phases, n, total, tiling_size(total, n, len(phases)), (C.c_int32 * len(phases))(*phases)

    def retile_device(self, x_all, offsets, lengths, total, phases, stream=None):
        """``cf_retile_windows``: ``x_all`` (float32 CUDA, at least ``tilings.tiling_size(total, n, K)`` samples) holds the base
        layout in its first ``total`` samples; the call fills the K - 1 tiling regions behind it, zeros included
        (``tilings.retile_host`` is the definition).  ``offsets`` [n + 1] / ``lengths`` [n]: int64 CUDA tensors of the base layout.
        Asynchronous on the stream; one phase launches nothing.  Returns ``x_all``."""
        import torch
        phases, n, total, size, c_phases = self._check_tiling_tables("retile_device", offsets, lengths, total, phases)
        self._tensors("retile_device", [("x_all", x_all, torch.float32, size)])
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_retile_windows(self._handle, N._p(x_all), N._p(offsets), N._p(lengths), n, total, c_phases, len(phases),
                                            N.stream_ptr(stream)))
        return x_all

    def vote_device(self, probs_all, offsets, lengths, total, phases, weight="mean", logits_all=None, out=None, logits_out=None, stream=None):
        """``cf_vote_tilings``: the per-sample weighted mean over the K tilings of ``probs_all`` (float32 CUDA, at least
        ``tilings.tiling_size(total, n, K)`` samples: what the forward pass made of a retiled buffer) -> float32 CUDA [total]
        (``tilings.vote_host`` is the definition; ``weight``: ``"mean"`` or ``"centre"``).  ``out`` may be ``probs_all`` itself.
        ``logits_all`` (same size) is merged by the same formula on its own values -- the voted logit is the weighted mean of the
        logits, not the logit of the voted probability -- and the call then returns ``(voted, voted_logits)``.  Asynchronous on the
        stream; with one phase nothing is launched (the outputs are copies when they are other buffers)."""
        import torch
        from .tilings import check_weight
        phases, n, total, size, c_phases = self._check_tiling_tables("vote_device", offsets, lengths, total, phases)
        weight = check_weight(weight)
        self._tensors("vote_device", [("probs_all", probs_all, torch.float32, size)])
        if out is None:
            out = torch.empty(total, dtype=torch.float32, device=probs_all.device)
        self._tensors("vote_device", [("out", out, torch.float32, total)])
        if logits_all is not None:
            self._tensors("vote_device", [("logits_all", logits_all, torch.float32, size)])
            if logits_out is None:
                logits_out = torch.empty(total, dtype=torch.float32, device=probs_all.device)
            self._tensors("vote_device", [("logits_out", logits_out, torch.float32, total)])
        elif logits_out is not None:
            raise ValueError("vote_device: logits_out without logits_all")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_vote_tilings(self._handle, N._p(probs_all), N._p(logits_all), N._p(offsets), N._p(lengths), n, total, c_phases,
                                          len(phases), weight, N._p(out), N._p(logits_out), N.stream_ptr(stream)))
        return out if logits_all is None else (out, logits_out)

    # ------------------------------------------------------------------ validation rounds on the card (csrc/validation.hpp)
    @staticmethod
    def _check_validation_sizes(what, probs, y, bounds, length, total, longest):
        """What the run-state, border and curve steps ask of their tables: -> (n, total, longest) as ints."""
        n, total, longest = int(length.numel()), int(total), int(longest)
        if int(bounds.numel()) != n + 1:
            raise ValueError("%s: length needs n entries, bounds n + 1" % what)
        if total < 0 or min(int(probs.numel()), int(y.numel())) < total:
            raise ValueError("%s: probs and y need %d elements" % (what, total))
        return n, total, longest

    def gather_validation(self, signal, labels, src_first, length, bounds, total, longest, x_out, y_out, stream=None):
        """``cf_validation_gather``: packed sample ``bounds[r] + i`` of ``x_out`` / ``y_out`` (float32 / uint8, at least ``total``
        elements) becomes ``signal`` / ``labels`` ``[src_first[r] + i]`` for ``i < length[r]`` and 0 after it.  ``src_first``,
        ``length`` [n] and ``bounds`` [n + 1] are int64 CUDA tensors; ``total`` = bounds[n] and ``longest`` = the largest packed
        read are the caller's host copies of those numbers.  Asynchronous on the stream."""
        import torch
        self._tensors("gather_validation", [
            ("signal", signal, torch.float32), ("labels", labels, torch.uint8), ("src_first", src_first, torch.int64),
            ("length", length, torch.int64), ("bounds", bounds, torch.int64), ("x_out", x_out, torch.float32), ("y_out", y_out, torch.uint8)])
        n, total, longest = int(src_first.numel()), int(total), int(longest)
        if int(length.numel()) != n or int(bounds.numel()) != n + 1:
            raise ValueError("gather_validation: src_first and length need n entries, bounds n + 1")
        if int(labels.numel()) != int(signal.numel()):
            raise ValueError("gather_validation: signal and labels differ in length")
        if total < 0 or int(x_out.numel()) < total or int(y_out.numel()) < total:
            raise ValueError("gather_validation: x_out and y_out need %d elements" % total)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        N.check(self._lib.cf_validation_gather(self._handle, N._p(signal), N._p(labels), int(signal.numel()), N._p(src_first), N._p(length),
                                               N._p(bounds), n, total, longest, N._p(x_out), N._p(y_out), N.stream_ptr(stream)))

    def score_validation(self, probs, logits, y, bounds, total, longest, thresholds, right_out, ce_sum_out, counts_out, partials, stream=None):
        """``cf_validation_score``: per read the number of samples with ``rint(p) == y`` (``right_out`` int64 [n]) and the fp64 sum
        of the sigmoid cross-entropy of the logits (``ce_sum_out`` float64 [n]); per threshold (``thresholds`` float64 CUDA [K],
        1 <= K <= 16) tp / fp / raw tn / fn over all ``total`` samples (``counts_out`` int64 [K * 4]).  ``partials`` is float64
        work space of at least ``total // SCORE_CHUNK + n`` elements.  Asynchronous on the stream; equal inputs give equal bits."""
        import torch
        self._tensors("score_validation", [
            ("probs", probs, torch.float32), ("logits", logits, torch.float32), ("y", y, torch.uint8), ("bounds", bounds, torch.int64),
            ("thresholds", thresholds, torch.float64), ("right_out", right_out, torch.int64), ("ce_sum_out", ce_sum_out, torch.float64),
            ("counts_out", counts_out, torch.int64), ("partials", partials, torch.float64)])
        n, k, total, longest = int(bounds.numel()) - 1, int(thresholds.numel()), int(total), int(longest)
        if total < 0 or min(int(probs.numel()), int(logits.numel()), int(y.numel())) < total:
            raise ValueError("score_validation: probs, logits and y need %d elements" % total)
        if int(right_out.numel()) < n or int(ce_sum_out.numel()) < n or int(counts_out.numel()) < 4 * k:
            raise ValueError("score_validation: right_out and ce_sum_out need n entries, counts_out 4 per threshold")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        # n, K and the work space are refused by the library (CF_ERR_INVALID -> ValueError)
        N.check(self._lib.cf_validation_score(self._handle, N._p(probs), N._p(logits), N._p(y), N._p(bounds), n, total, longest,
                                              N._p(thresholds), k, N._p(right_out), N._p(ce_sum_out), N._p(counts_out), N._p(partials),
                                              int(partials.numel()), N.stream_ptr(stream)))

    def _run_step_arguments(self, what, probs, y, bounds, length, total, longest, thresholds, counts_out, work, stream, own=()):
        """What ``run_states_validation``, ``run_borders_validation`` and ``run_bases_validation`` check and convert alike (``own``:
        the step's own tensors, checked between ``y`` and ``bounds``) -> (n, total, longest, K, thresholds as a C array, stream).
        n, K, min_run, the (min_run, max_gap) pair and the work space are refused by the library (CF_ERR_INVALID -> ValueError)."""
        import torch
        self._tensors(what, [("probs", probs, torch.float32), ("y", y, torch.uint8)] + list(own) + [
            ("bounds", bounds, torch.int64), ("length", length, torch.int64), ("counts_out", counts_out, torch.int64),
            ("work", work, torch.uint8)])
        thresholds = [float(t) for t in thresholds]
        k = len(thresholds)
        n, total, longest = self._check_validation_sizes(what, probs, y, bounds, length, total, longest)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return n, total, longest, k, (C.c_double * max(k, 1))(*thresholds), stream

    def run_states_work_bytes(self, total, n_thresholds):
        """Bytes of work space ``run_states_validation`` needs for ``total`` packed samples and ``n_thresholds`` thresholds."""
        return int(self._lib.cf_validation_run_work_bytes(int(total), int(n_thresholds)))

    def run_states_validation(self, probs, y, bounds, length, total, longest, thresholds, edges, counts_out, work, min_run=15, stream=None,
                              max_gap=0):
        """``cf_validation_run_states``: per threshold (``thresholds``: 1..16 host floats), kind (0 = true runs judged against the
        corrected prediction, 1 = predicted runs judged against ``y``), length bin (``edges``: up to 7 ascending host ints) and
        state (complete / incomplete / absent) how many runs -- ``device_validation.run_states_host`` -- into ``counts_out``
        (int64 CUDA, ``K * 2 * (len(edges) + 1) * 3`` elements).  ``bounds`` [n + 1] and ``length`` [n] are int64 CUDA tensors;
        ``work`` is a uint8 CUDA tensor of at least ``run_states_work_bytes(total, K)`` bytes.  Asynchronous on the stream; equal
        inputs give equal bits."""
        n, total, longest, k, thresholds, stream = self._run_step_arguments("run_states_validation", probs, y, bounds, length, total, longest,
                                                                            thresholds, counts_out, work, stream)
        edges = [int(e) for e in edges]
        if int(counts_out.numel()) < k * 2 * (len(edges) + 1) * 3:
            raise ValueError("run_states_validation: counts_out needs 2 * (edges + 1) * 3 entries per threshold")
        # the edges are refused by the library too; ``max_gap`` 0 is ``cf_validation_run_states``, anything else bridges the
        # prediction first
        N.check(self._lib.cf_validation_run_states_bridged(self._handle, N._p(probs), N._p(y), N._p(bounds), N._p(length), n, total,
                                                           longest, thresholds, k, (C.c_int64 * max(len(edges), 1))(*edges), len(edges),
                                                           int(max_gap), int(min_run), N._p(counts_out), N._p(work), int(work.numel()),
                                                           N.stream_ptr(stream)))

    def run_scores_work_bytes(self, total, n_thresholds):
        """Bytes of work space ``run_scores_validation`` needs: the labels of ``run_states_work_bytes`` and a byte of paint per sample
        and threshold behind them."""
        return int(self._lib.cf_validation_run_scores_work_bytes(int(total), int(n_thresholds)))

    def run_scores_validation(self, probs, y, bounds, length, total, longest, thresholds, shift, table_out, work, min_run=15, stream=None,
                              max_gap=0):
        """``cf_validation_run_scores``: per threshold (``thresholds``: 1..16 host floats), kind and state of a run the histogram of the
        probabilities of the samples under those runs at ``shift`` (14 .. 22) and, in each row's last cell, their fixed-point sum --
        ``device_validation.run_scores_host`` -- into ``table_out`` (int64 CUDA, ``K * score_cells(shift)`` elements, zeroed and
        written by the call).  ``bounds`` [n + 1] and ``length`` [n] are int64 CUDA tensors; ``work`` is a uint8 CUDA tensor of at
        least ``run_scores_work_bytes(total, K)`` bytes.  Asynchronous on the stream; equal inputs give equal bits."""
        n, total, longest, k, thresholds, stream = self._run_step_arguments("run_scores_validation", probs, y, bounds, length, total, longest,
                                                                            thresholds, table_out, work, stream)
        if isinstance(shift, bool) or int(shift) != shift:
            raise ValueError("run_scores_validation: shift must be an int, got %r" % (shift,))
        # the shift, the room in table_out and the work space are refused by the library (CF_ERR_INVALID -> ValueError)
        N.check(self._lib.cf_validation_run_scores(self._handle, N._p(probs), N._p(y), N._p(bounds), N._p(length), n, total, longest,
                                                   thresholds, k, int(shift), int(max_gap), int(min_run), N._p(table_out),
                                                   int(table_out.numel()), N._p(work), int(work.numel()), N.stream_ptr(stream)))

    def run_borders_work_bytes(self, total, n_thresholds):
        """Bytes of work space ``run_borders_validation`` needs (``run_states_work_bytes``' rule: the two can share a buffer)."""
        return int(self._lib.cf_validation_run_borders_work_bytes(int(total), int(n_thresholds)))

    def run_borders_validation(self, probs, y, bounds, length, total, longest, thresholds, reach, counts_out, work, min_run=15, stream=None,
                               max_gap=0):
        """``cf_validation_run_borders``: per threshold (``thresholds``: 1..16 host floats) and kind the histograms of how far the
        other array reaches beyond a run's left and right border or falls short of it (clipped at ``reach``, an int in 1 .. 128),
        of the interruptions inside the runs, and the number of interrupted runs -- ``device_validation.run_borders_host`` -- into
        ``counts_out`` (int64 CUDA, ``K * 2 * (5 * reach + 3)`` elements).  ``bounds`` [n + 1] and ``length`` [n] are int64 CUDA
        tensors; ``work`` is a uint8 CUDA tensor of at least ``run_borders_work_bytes(total, K)`` bytes.  A label other than 1
        counts as 0 here (``RNN.score_validation_device`` refuses such sets).  Asynchronous on the stream; equal inputs give equal
        bits."""
        from .device_validation import check_border_reach
        n, total, longest, k, thresholds, stream = self._run_step_arguments("run_borders_validation", probs, y, bounds, length, total, longest,
                                                                            thresholds, counts_out, work, stream)
        reach = check_border_reach(reach)
        if int(counts_out.numel()) < k * 2 * (5 * reach + 3):
            raise ValueError("run_borders_validation: counts_out needs 2 * (5 * reach + 3) entries per threshold")
        # ``max_gap`` 0 is ``cf_validation_run_borders``, anything else bridges the prediction first
        N.check(self._lib.cf_validation_run_borders_bridged(self._handle, N._p(probs), N._p(y), N._p(bounds), N._p(length), n, total,
                                                            longest, thresholds, k, reach, int(max_gap), int(min_run), N._p(counts_out),
                                                            N._p(work), int(work.numel()), N.stream_ptr(stream)))

    def run_bases_validation(self, probs, y, basemap, src_first, bounds, length, total, longest, thresholds, max_bases, counts_out, work,
                             min_run=15, max_gap=0, stream=None):
        """``cf_validation_run_bases``: per threshold (``thresholds``: 1..16 host floats), kind, state, base class (A / C / G / T /
        other) and length in bases (``min(nb, max_bases)``, ``max_bases`` an int in 1 .. 32) how many runs --
        ``device_validation.run_bases_host`` -- into ``counts_out`` (int64 CUDA, ``K * 2 * 3 * 5 * (max_bases + 1)`` elements).
        ``basemap`` is the SET's base map (uint8 CUDA, read in place: packed sample ``bounds[r] + i`` is ``basemap[src_first[r] + i]``;
        an index outside it counts as no base); ``src_first`` [n], ``length`` [n] and ``bounds`` [n + 1] are int64 CUDA tensors;
        ``work`` is a uint8 CUDA tensor of at least ``run_states_work_bytes(total, K)`` bytes.  Asynchronous on the stream; equal
        inputs give equal bits."""
        import torch
        from .device_validation import BASE_CLASSES, check_max_bases
        n, total, longest, k, thresholds, stream = self._run_step_arguments(
            "run_bases_validation", probs, y, bounds, length, total, longest, thresholds, counts_out, work, stream,
            own=(("basemap", basemap, torch.uint8), ("src_first", src_first, torch.int64)))
        max_bases = check_max_bases(max_bases)
        if int(src_first.numel()) != n:
            raise ValueError("run_bases_validation: src_first needs n entries")
        if int(counts_out.numel()) < k * 2 * 3 * len(BASE_CLASSES) * (max_bases + 1):
            raise ValueError("run_bases_validation: counts_out needs 2 * 3 * 5 * (max_bases + 1) entries per threshold")
        # an empty base map is refused by the library too
        N.check(self._lib.cf_validation_run_bases(self._handle, N._p(probs), N._p(y), N._p(basemap), int(basemap.numel()), N._p(src_first),
                                                  N._p(bounds), N._p(length), n, total, longest, thresholds, k, max_bases, int(max_gap),
                                                  int(min_run), N._p(counts_out), N._p(work), int(work.numel()), N.stream_ptr(stream)))

    def base_votes_work_bytes(self, n_bases, n_thresholds):
        """Bytes of work space ``base_votes_validation`` needs for a set of ``n_bases`` bases and ``n_thresholds`` thresholds."""
        return int(self._lib.cf_base_votes_work_bytes(int(n_bases), int(n_thresholds)))

    def base_votes_validation(self, probs, labels, basemap, edges, src_first, bounds, length, ranges, total, longest_range, thresholds,
                              max_bases, confusion_out, runs_out, work, stream=None):
        """``cf_base_votes``: the samples of every base that lies wholly inside a stretch vote on it, and the voted bases are scored by
        base -- ``base_votes.vote_host``.  ``probs`` are the round's packed probabilities; ``labels`` / ``basemap`` (uint8) and
        ``edges`` (int64 [n_bases + 1]) the SET's arrays, read in place; ``src_first`` [n], ``length`` [n], ``bounds`` [n + 1] and
        ``ranges`` [2 n] (``base_votes.event_ranges``: every a, then every b) int64 CUDA tensors; ``thresholds`` 1..16 host floats.
        Into ``confusion_out`` (int64 CUDA, ``K * 5 * 2 * 2`` elements) and ``runs_out`` (``K * 2 * 3 * 5 * (max_bases + 1)``); ``work``
        (uint8 CUDA, at least ``base_votes_work_bytes(n_bases, K)`` bytes, 8-byte aligned) holds the per-base sums (uint64
        [n_bases]) and states (uint8 [K, n_bases]) afterwards.  Asynchronous on the stream; equal inputs give equal bits."""
        import torch
        from . import base_votes
        from .device_validation import BASE_CLASSES, check_max_bases
        self._tensors("base_votes_validation", [
            ("probs", probs, torch.float32), ("labels", labels, torch.uint8), ("basemap", basemap, torch.uint8), ("edges", edges, torch.int64),
            ("src_first", src_first, torch.int64), ("bounds", bounds, torch.int64), ("length", length, torch.int64),
            ("ranges", ranges, torch.int64), ("confusion_out", confusion_out, torch.int64), ("runs_out", runs_out, torch.int64),
            ("work", work, torch.uint8)])
        thresholds = [float(t) for t in thresholds]
        max_bases = check_max_bases(max_bases)
        k, n, total = len(thresholds), int(length.numel()), int(total)
        if int(bounds.numel()) != n + 1 or int(src_first.numel()) != n or int(ranges.numel()) != 2 * n:
            raise ValueError("base_votes_validation: src_first and length need n entries, bounds n + 1, ranges 2 n")
        if total < 0 or int(probs.numel()) < total:
            raise ValueError("base_votes_validation: probs needs %d elements" % total)
        if int(edges.numel()) < 1:
            raise ValueError("base_votes_validation: edges needs n_bases + 1 entries")
        if int(confusion_out.numel()) < k * base_votes.CONFUSION_CELLS or int(runs_out.numel()) < k * 2 * 3 * len(BASE_CLASSES) * (max_bases + 1):
            raise ValueError("base_votes_validation: confusion_out needs 20 entries per threshold, runs_out 2 * 3 * 5 * (max_bases + 1)")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        # K, the sizes and the work space are refused by the library (CF_ERR_INVALID -> ValueError)
        base_votes.launch(self._lib, self._handle, probs, total, labels, basemap, edges, int(edges.numel()) - 1, src_first, length, bounds,
                          ranges, longest_range, thresholds, max_bases, confusion_out, runs_out, work, stream)

    def curve_validation(self, probs, y, bounds, length, total, longest, shift, hist_out, stream=None):
        """``cf_validation_curve``: how many samples of label 1 / label 0 / any other label fall into every bin of
        ``device_validation.curve_bin`` at ``shift`` (10 .. 22) -- ``device_validation.curve_host`` -- into ``hist_out`` (int64 CUDA,
        at least ``3 * curve_bins(shift)`` elements, zeroed and written by the call).  ``bounds`` [n + 1] and ``length`` [n] are
        int64 CUDA tensors; the zero tails are not counted.  Asynchronous on the stream; equal inputs give equal bits."""
        import torch
        self._tensors("curve_validation", [
            ("probs", probs, torch.float32), ("y", y, torch.uint8), ("bounds", bounds, torch.int64), ("length", length, torch.int64),
            ("hist_out", hist_out, torch.int64)])
        n, total, longest = self._check_validation_sizes("curve_validation", probs, y, bounds, length, total, longest)
        if isinstance(shift, bool) or int(shift) != shift:
            raise ValueError("curve_validation: shift must be an int, got %r" % (shift,))
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        # n, the shift and the room in hist_out are refused by the library (CF_ERR_INVALID -> ValueError)
        N.check(self._lib.cf_validation_curve(self._handle, N._p(probs), N._p(y), N._p(bounds), N._p(length), n, total, longest, int(shift),
                                              N._p(hist_out), int(hist_out.numel()), N.stream_ptr(stream)))

    # ------------------------------------------------------------------ profiling / debug
    def profile_enable(self, on=True, every=1):
        """Per-kernel HIP-event timing of every ``every``-th call (events cost ~1.6 % when on every call)."""
        N.check(self._lib.cf_profile_enable(self._handle, int(every) if on else 0))

    def profile_reset(self):
        N.check(self._lib.cf_profile_reset(self._handle))

    def profile_read(self):
        """-> {kernel slot name: (total ms, launches)} since the last reset."""
        ms = (C.c_double * N.CF_PROF_SLOTS)()
        cnt = (C.c_int64 * N.CF_PROF_SLOTS)()
        N.check(self._lib.cf_profile_read(self._handle, ms, cnt))
        return {self._lib.cf_profile_slot_name(i).decode(): (float(ms[i]), int(cnt[i]))
                for i in range(N.CF_PROF_SLOTS) if cnt[i]}

    def debug_stage(self, stage, n_windows):
        """An intermediate activation of slot 0's last pass -> float32 [n_windows, 35, features] (tuned 64 / 32 path only).
        ``stage``: 0 .. n_layers_res - 1 the residual blocks' outputs, n_layers_res + l the output of biGRU layer l.  Only what
        survives a pass can be read: the last two blocks (block 0 not when blocks 0 and 1 ran as one fused launch), the two
        layers before the last one; the last layer's output exists as logits only.  In every precision: with ``precision="bf16"``
        the values are what the kernels stored, rounded to bf16; with ``"bf16x3"`` hi + lo of the stored split."""
        feats = self.layer_size_res if stage < self.n_layers_res else 2 * self.layer_size
        out = np.empty((n_windows, WINDOW, feats), dtype=np.float32)
        N.check(self._lib.cf_debug_stage(self._handle, int(stage), int(n_windows), N.np_ptr(out)))
        return out
