"""The backward of ``torch.ops.catfish.resnetrnn_forward`` on the HIP kernels (the autograd formula ``torch_ops`` registers).

The function differentiated is the operator's own: inference-mode BN on the moving statistics, no dropout, p = sigmoid(logit) per
sample.  Nothing is stashed by the forward: the backward re-runs the training forward of ``anysize_step`` (keep_prob 1) to get the
activations it needs, then walks the same launch sequence as ``AnySizeTrainStep.run`` backwards, with three differences:

    dense head            cf_gen_head_backward  (from the upstream d probability, not from labels)
    d signal              cf_gen_signal_grad    (block 0's two cin-1 units, or layer 0's gate gradients for the plain RNN)
    BN moving statistics  cf_gen_bn_stat_grads  (d mean, d var from the unit's d gamma, d beta: the step treats them as constants)

With only ``x`` requiring grad no weight-gradient reduction is launched (cf_gen_bn_backward_data, no dense / conv / GRU wgrad) and
nothing synchronises; the weight gradient ends in the one device-to-host copy of the flat gradient.

The operator's packed tensor is, after its 8-value header, exactly ``flat_layout``'s buffer (``tensor_names`` order), so the device
parameters are one upload of ``packed[HEADER:]``.  ``resnetrnn_forward_params`` passes that buffer itself, on the device: its
backward copies it into the state (``set_params``, stream-ordered) and returns the weight gradient on the device.  Windows are padded to a multiple of 16 and processed in slabs of at most
``BACKWARD_MAX_WINDOWS`` (None: as many as fit ``SLAB_BUDGET_BYTES`` of stash and workspace); the weight gradients of the slabs are
summed in slab order, so a call gives bit-identical gradients every time.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from .anysize_step import flat_layout, flat_pack_map
from .native_step import _p
from .native_train import T

BACKWARD_MAX_WINDOWS = None          # windows per slab (a multiple of 16); None: the most that fit SLAB_BUDGET_BYTES
SLAB_BUDGET_BYTES = 512 << 20        # stash + workspace of one slab


class OpGrad(object):
    """Per-engine backward state: device flat parameters, the GRU packs of ``flat_pack_map`` and the slab buffers."""

    def __init__(self, engine, packed=None, header=0, keep_buffers=False):
        """``packed``: the parameters (``header`` values, then the flat buffer) on the host or the device; None = set them with
        ``set_params`` before each backward.  ``keep_buffers``: never free a slab buffer set when a larger call needs a new one
        (a captured CUDA graph may still point at it)."""
        import torch
        self.torch = torch
        self.lib, self.handle = engine._lib, engine._handle
        self.dev = torch.device("cuda", engine.device)
        self.h, self.n_layers, self.n_blocks = engine.layer_size, engine.n_layers, engine.n_layers_res
        self.c = engine.layer_size_res if self.n_blocks > 0 else 0
        self.entries, self.units, self.layers, self.head_off, self.zero_off = flat_layout(self.h, self.c, self.n_layers, self.n_blocks)
        self.header = header
        self.pflat = torch.zeros(self.zero_off + 1, dtype=torch.float32, device=self.dev)
        idx, scale, self.per_layer = flat_pack_map(self.h, self.layers, self.zero_off)
        self._idx, self._scale = torch.from_numpy(idx).to(self.dev), torch.from_numpy(scale).to(self.dev)
        self.gru_packed = torch.empty(idx.shape[0], dtype=torch.float32, device=self.dev)
        self._bufs = None
        self._kept = [] if keep_buffers else None
        if packed is not None:
            if int(packed.numel()) != header + self.zero_off:
                raise ValueError("packed_weights has %d values, the engine's geometry needs %d" % (packed.numel(), header + self.zero_off))
            self.set_params(packed.detach()[header:])

    def set_params(self, params):
        """The flat parameters (``zero_off`` values, host or device) into ``pflat`` and the GRU packs gathered from them: a copy and
        two element-wise launches on the current stream."""
        torch = self.torch
        self.pflat[:self.zero_off].copy_(params.reshape(-1))
        torch.mul(self.pflat[self._idx], self._scale, out=self.gru_packed)

    # ------------------------------------------------------------------ slab buffers
    def _plane_features(self):
        """Feature counts of the fragment planes of one slab (each [tiles][35][F/16][64][4])."""
        c, h, nb = self.c, self.h, self.n_blocks
        feats = [c] * (4 * nb + 3 * nb + 1 + 4 + 2 + 2) if nb else [16]       # z, o1 / o2 / a, sc, dz, do1 / do2, dA | x_frag
        feats += [2 * h, 6 * h] * self.n_layers + [6 * h, 2 * h]              # y_frag, stash per layer; da, dy_head
        feats += [cin for _, cin in self.layers if cin >= 16]                 # dx per layer
        return feats

    def _ws_floats(self, npad):
        lib, h, c = self.lib, self.h, self.c
        rows = [kw * cin + 1 for _, kw, cin, _ in self.units] + [cin + h + 1 for _, cin in self.layers]
        cols = [c] * len(self.units) + [2 * h] * len(self.layers)
        wgrad = max(int(lib.cf_gen_train_workspace_floats(r, k, npad)) for r, k in zip(rows, cols))
        head = int(lib.cf_gen_head_backward_workspace_floats(2 * h, npad))
        bn = npad // 16 * 2 * c
        return wgrad, head, bn

    def slab_floats(self, npad):
        """Device floats of the buffers of a slab of ``npad`` windows (stash, gradients, workspaces, signal and upstream rows)."""
        return npad * T * (sum(self._plane_features()) + 3) + sum(self._ws_floats(npad)) + self.zero_off + 1

    def slab_windows(self, n):
        """Windows per slab for a call of ``n`` windows: a multiple of 16."""
        npad = (n + 15) // 16 * 16
        if BACKWARD_MAX_WINDOWS is not None:
            cap = int(BACKWARD_MAX_WINDOWS)
            if cap <= 0 or cap % 16:
                raise ValueError("op_grad.BACKWARD_MAX_WINDOWS must be a positive multiple of 16 or None")
            return min(npad, cap)
        lo, hi = 16, npad                                                   # largest multiple of 16 within the budget
        if self.slab_floats(hi) * 4 <= SLAB_BUDGET_BYTES:
            return hi
        while hi - lo > 16:
            mid = (lo + hi) // 32 * 16
            if self.slab_floats(mid) * 4 <= SLAB_BUDGET_BYTES:
                lo = mid
            else:
                hi = mid
        return lo

    def _buffers(self, npad):
        """Buffers for slabs of up to ``npad`` windows; planes are tile-major, so a smaller slab uses their prefix."""
        if self._bufs is not None and self._bufs["cap"] >= npad:
            return self._bufs
        torch = self.torch
        if self._kept is not None and self._bufs is not None:
            self._kept.append(self._bufs)
        self._bufs = None                                                  # free the old set before allocating the new one
        tiles, h, c = npad // 16, self.h, self.c
        f32 = dict(dtype=torch.float32, device=self.dev)
        plane = lambda f: torch.empty(tiles, T, f // 16, 64, 4, **f32)     # noqa: E731
        b = {"cap": npad}
        b["xpad"], b["g"], b["dx_sig"] = (torch.empty(npad, T, **f32) for _ in range(3))
        nb = self.n_blocks
        if nb > 0:
            b["z"] = [plane(c) for _ in range(4 * nb)]
            b["o1"], b["o2"], b["a"] = ([plane(c) for _ in range(nb)] for _ in range(3))
            b["sc"] = plane(c)
            b["dz"] = [plane(c) for _ in range(4)]
            b["do1"], b["do2"] = plane(c), plane(c)
            b["dA"] = [plane(c), plane(c)]
        else:
            b["x_frag"] = plane(16)
        b["y_frag"] = [plane(2 * h) for _ in range(self.n_layers)]
        b["stash"] = [plane(6 * h) for _ in range(self.n_layers)]
        b["da"] = plane(6 * h)
        b["dy_head"] = plane(2 * h)
        b["dx"] = [plane(cin) if cin >= 16 else None for _, cin in self.layers]
        wgrad, head, bn = self._ws_floats(npad)
        b["wgrad_ws"], b["head_ws"], b["bn_ws"] = torch.empty(wgrad, **f32), torch.empty(head, **f32), torch.empty(max(bn, 1), **f32)
        b["gslab"] = torch.zeros(self.zero_off + 1, **f32)                 # moving statistics and the zero slot stay 0
        self._bufs = b
        return b

    # ------------------------------------------------------------------ one slab (every launch on the current stream)
    def _slab(self, b, npad, gf, need_x, need_w, stream):
        lib, hd, h = self.lib, self.handle, self.h
        pf, packed, units = self.pflat, self.gru_packed, self.units
        ws, wsn = b["wgrad_ws"], int(b["wgrad_ws"].numel())
        # ---- training forward at keep_prob 1 (the stash the backward needs)
        a = b["xpad"]
        for k in range(self.n_blocks):
            j = 4 * k
            for u, src, res, relu, out in ((j, a, None, 0, b["sc"]), (j + 1, a, None, 1, b["o1"][k]), (j + 2, b["o1"][k], None, 1, b["o2"][k]),
                                           (j + 3, b["o2"][k], b["sc"], 1, b["a"][k])):
                off, kw, cin, cout = units[u]
                N.check(lib.cf_gen_conv_forward(hd, kw, cin, cout, _p(pf[off:]), _p(src), None if res is None else _p(res), relu,
                                                _p(b["z"][u]), _p(out), npad, stream))
            a = b["a"][k]
        if self.n_blocks == 0:
            N.check(lib.cf_gen_x_frag(hd, _p(b["xpad"]), _p(b["x_frag"]), npad, stream))
            a = b["x_frag"]
        inputs = []
        for layer, (off, cin) in enumerate(self.layers):
            (wo, _), (bo, _), _ = self.per_layer[layer]
            inputs.append(a)
            N.check(lib.cf_gru_anysize_train_forward(hd, h, (cin + 15) // 16, _p(packed[wo:]), _p(packed[bo:]), _p(a), _p(b["y_frag"][layer]),
                                                     _p(b["stash"][layer]), npad, stream))
            a = b["y_frag"][layer]
        # ---- head backward from d probability
        ho = self.head_off
        N.check(lib.cf_gen_head_backward(hd, 2 * h, _p(a), _p(pf[ho:]), _p(b["g"]), _p(b["dy_head"]), _p(b["head_ws"]),
                                         int(b["head_ws"].numel()), _p(gf[ho:]) if need_w else None, npad, stream))
        # ---- biGRU layers backward
        g = b["dy_head"]
        for layer in range(self.n_layers - 1, -1, -1):
            off, cin = self.layers[layer]
            _, _, (to, _) = self.per_layer[layer]
            N.check(lib.cf_gru_anysize_train_backward(hd, h, _p(packed[to:]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(g),
                                                      _p(b["da"]), npad, stream))
            if need_w:
                N.check(lib.cf_gen_gru_wgrad(hd, h, cin, _p(inputs[layer]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(b["da"]),
                                             _p(ws), wsn, _p(gf[off:]), npad, stream))
            if b["dx"][layer] is not None:
                N.check(lib.cf_gen_gru_dx(hd, h, cin, _p(pf[off:]), _p(b["da"]), _p(b["dx"][layer]), npad, stream))
                g = b["dx"][layer]
        if self.n_blocks == 0:
            if need_x:
                off, _ = self.layers[0]
                N.check(lib.cf_gen_signal_grad(hd, h, 0, _p(pf[off:]), _p(b["da"]), None, None, _p(b["dx_sig"]), npad, stream))
            return
        # ---- conv stack backward
        bws, bwsn = b["bn_ws"], int(b["bn_ws"].numel())
        dA = g
        dz = b["dz"]
        for k in range(self.n_blocks - 1, -1, -1):
            j = 4 * k
            a_in = b["xpad"] if k == 0 else b["a"][k - 1]

            def unit_bwd(u, grad, mask, relu, src):
                off, kw, cin, cout = units[u]
                msk = None if mask is None else _p(mask)
                if need_w:
                    N.check(lib.cf_gen_bn_backward(hd, kw, cin, cout, _p(pf[off:]), _p(grad), msk, relu, _p(b["z"][u]), _p(dz[u - j]),
                                                   _p(bws), bwsn, _p(gf[off:]), npad, stream))
                    N.check(lib.cf_gen_conv_wgrad(hd, kw, cin, cout, _p(src), _p(dz[u - j]), _p(ws), wsn, _p(gf[off:]), npad, stream))
                else:
                    N.check(lib.cf_gen_bn_backward_data(hd, kw, cin, cout, _p(pf[off:]), _p(grad), msk, relu, _p(b["z"][u]), _p(dz[u - j]),
                                                        npad, stream))

            def unit_dx(u, out, add=None):
                off, kw, cin, cout = units[u]
                N.check(lib.cf_gen_conv_backward_data(hd, kw, cin, cout, _p(pf[off:]), _p(dz[u - j]), None if add is None else _p(add),
                                                      _p(out), npad, stream))

            unit_bwd(j + 3, dA, b["a"][k], 1, b["o2"][k])
            unit_bwd(j, dA, b["a"][k], 0, a_in)
            unit_dx(j + 3, b["do2"])
            unit_bwd(j + 2, b["do2"], None, 1, b["o1"][k])
            unit_dx(j + 2, b["do1"])
            unit_bwd(j + 1, b["do1"], None, 1, a_in)
            if k > 0:
                nxt = b["dA"][k & 1]
                unit_dx(j, nxt)
                unit_dx(j + 1, nxt, add=nxt)
                dA = nxt
        if need_x:
            (o0, _, _, c), (o1, _, _, _) = units[0], units[1]
            N.check(lib.cf_gen_signal_grad(hd, 0, c, _p(pf[o0:]), _p(dz[0]), _p(pf[o1:]), _p(dz[1]), _p(b["dx_sig"]), npad, stream))

    # ------------------------------------------------------------------ the whole call
    def backward(self, x, grad, need_x, need_w, device_grad=False):
        """(d x shaped like ``x`` on its device or None, d packed_weights as a float32 CPU tensor or None).  ``device_grad``: the
        weight gradient is instead a fresh float32 tensor of the flat buffer's ``zero_off`` values on the device (no header, no
        synchronisation)."""
        torch = self.torch
        n = int(x.shape[0])
        xf = x.detach().reshape(n, T)
        gf_in = grad.detach().reshape(n, T)
        gx = torch.empty(n, T, dtype=torch.float32, device=self.dev) if need_x else None
        gacc = torch.zeros(self.zero_off + 1, dtype=torch.float32, device=self.dev) if need_w else None
        if n > 0 and (need_x or need_w):
            stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            slab = self.slab_windows(n)
            b = self._buffers(slab)
            for s, start in enumerate(range(0, n, slab)):
                m = min(slab, n - start)
                npad = (m + 15) // 16 * 16
                b["xpad"][:m].copy_(xf[start:start + m])
                b["xpad"][m:npad].zero_()
                b["g"][:m].copy_(gf_in[start:start + m])
                b["g"][m:npad].zero_()                                   # padding windows: zero upstream gradient
                dst = gacc if s == 0 else b["gslab"]
                self._slab(b, npad, dst, need_x, need_w, stream)
                if need_w and s > 0:
                    gacc += b["gslab"]                                   # slab order: the same sum on every call
                if need_x:
                    gx[start:start + m].copy_(b["dx_sig"][:m])
            if need_w:
                for off, kw, cin, cout in self.units:
                    N.check(self.lib.cf_gen_bn_stat_grads(self.handle, kw, cin, cout, _p(self.pflat[off:]), _p(gacc[off:]), stream))
        gw = None
        if need_w and device_grad:
            gw = gacc.narrow(0, 0, self.zero_off)                        # gacc is this call's own tensor
        elif need_w:
            gw = torch.zeros(self.header + self.zero_off, dtype=torch.float32)
            gw[self.header:].copy_(gacc[:self.zero_off])                 # the one synchronisation of the backward
        if need_x:
            gx = gx.reshape(x.shape)
        return gx, gw
