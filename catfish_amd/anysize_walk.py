"""The launch sequence of the any-size training kernels (``cf_gen_*``, ``cf_gru_anysize_train_*``), written once.

Two drivers walk it: the whole training step of ``anysize_step`` and the operator's backward of ``op_grad``.  Here is what they
share -- the flat parameter layout, the gather map of the biGRU packs, the table of a slab's fragment planes (allocation, float
count and workspace sizes all come from it) and the four walks

    conv_forward    cf_gen_conv_forward per unit (or cf_gen_x_frag for the plain RNN type)
    gru_forward     cf_gru_anysize_train_forward per layer, an optional hook after each (the step's output dropout)
    gru_backward    an optional hook before each layer (dropout of the incoming gradient), cf_gru_anysize_train_backward,
                    cf_gen_gru_wgrad if the weight gradients are wanted, cf_gen_gru_dx
    conv_backward   cf_gen_bn_backward + cf_gen_conv_wgrad, or cf_gen_bn_backward_data without weight gradients, and
                    cf_gen_conv_backward_data

The heads, the signal gradient, the optimizer and the slab loop stay with the drivers.  Every launch goes to the stream it is given.

With ``precision="bf16x3"`` the two recurrences run their ``_x3`` entry points on a second buffer of packs, ``packed_x3`` (per layer
the split wpack, then the split wtpack; ``repack_x3`` rebuilds it from ``packed`` with cf_gen_repack_x3).  The biases, the
GEMM-shaped kernels and everything else read what they read in fp32.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._native import _p
from .native_train import T, res_unit_names

STEP_ONLY = frozenset(("y_drop", "dy"))      # planes of the training step alone: dropped activations and their gradient


def flat_layout(layer_size, layer_size_res, n_layers, n_blocks):
    """(entries [(TF name, offset, shape)], units [(offset, kw, cin, cout)], layers [(offset, cin)], head offset, zero offset)."""
    h, c = int(layer_size), int(layer_size_res)
    entries, units, layers = [], [], []
    off = 0
    for j, unit in enumerate(res_unit_names(n_blocks)):
        kw = 3 if j % 4 == 2 else 1
        cin = 1 if j in (0, 1) else c
        units.append((off, kw, cin, c))
        for name, shape in zip(unit, [(kw, cin, c), (c,), (c,), (c,), (c,), (c,)]):
            entries.append((name, off, shape))
            off += int(np.prod(shape))
    for layer in range(n_layers):
        cin = (c if n_blocks > 0 else 1) if layer == 0 else 2 * h
        layers.append((off, cin))
        rows = cin + h
        for d in ("fw", "bw"):
            pre = N.gru_prefix(layer, d)
            for name, shape in ((pre + "/gates/kernel", (rows, 2 * h)), (pre + "/gates/bias", (2 * h,)),
                                (pre + "/candidate/kernel", (rows, h)), (pre + "/candidate/bias", (h,))):
                entries.append((name, off, shape))
                off += int(np.prod(shape))
    head = off
    entries += [("final_fully_connected/kernel", off, (2 * h, 1)), ("final_fully_connected/bias", off + 2 * h, (1,))]
    return entries, units, layers, head, off + 2 * h + 1


def flat_pack_map(layer_size, layers, zero_off):
    """The gather map of cf_opt_step over the flat buffer: per layer wpack [2] | bpack [2] | wtpack [2] (the layouts of
    cf_gru_anysize_train_forward / _backward), from anysize_train.pack_maps rebased from [wg | wc | bg | bc | 0.0] into the
    flat layout.  Returns (idx int64, scale float32, [(wpack, bpack, wtpack) (offset, floats) per layer]) as numpy."""
    from .anysize_train import pack_maps
    h = int(layer_size)
    idx, scale, per_layer = [], [], []
    pos = 0
    for off, cin in layers:
        rows = cin + h
        dir_floats = rows * 3 * h + 3 * h
        w_idx, w_scale, b_idx, b_scale, wt_idx = (t.cpu().numpy() for t in pack_maps(h, cin, "cpu"))
        parts = []
        for src_idx, src_scale in ((w_idx, w_scale), (b_idx, b_scale), (wt_idx, np.ones(wt_idx.shape, np.float32))):
            start = pos
            for d in range(2):
                base = off + d * dir_floats
                remap = np.concatenate([base + np.arange(rows * 2 * h),                              # gates kernel
                                        base + rows * 2 * h + 2 * h + np.arange(rows * h),           # candidate kernel
                                        base + rows * 2 * h + np.arange(2 * h),                      # gates bias
                                        base + rows * 3 * h + 2 * h + np.arange(h),                  # candidate bias
                                        [zero_off]])
                idx.append(remap[src_idx])
                scale.append(src_scale.astype(np.float32))
                pos += src_idx.size
            parts.append((start, pos - start))
        per_layer.append(tuple(parts))
    return np.concatenate(idx).astype(np.int64), np.concatenate(scale).astype(np.float32), per_layer


class AnySizeWalk(object):
    """One geometry's layout, plane table and launch walks.  ``b`` is a buffer dict of ``alloc``, ``pf`` / ``gf`` the flat parameters
    and gradients, ``packed`` the biGRU packs gathered through ``pack_idx`` / ``pack_scale`` (numpy, ``flat_pack_map``)."""

    def __init__(self, lib, handle, h, c, n_layers, n_blocks, precision="fp32"):
        from .anysize_train import check_precision, x3_pack_floats
        self.lib, self.handle = lib, handle
        self.precision = check_precision(precision)
        self.h, self.c, self.n_layers, self.n_blocks = int(h), int(c), int(n_layers), int(n_blocks)
        self.layout = flat_layout(h, c, n_layers, n_blocks)
        self.entries, self.units, self.layers, self.head_off, self.zero_off = self.layout
        self.pack_idx, self.pack_scale, self.per_layer = flat_pack_map(h, self.layers, self.zero_off)
        self.x3_layer, self.n_packed_x3 = [], 0              # per layer (offset of the split wpack, of the split wtpack) in packed_x3
        if self.precision == "bf16x3":
            for _, cin in self.layers:
                nw, nt = x3_pack_floats(lib, self.h, (cin + 15) // 16)
                self.x3_layer.append((self.n_packed_x3, self.n_packed_x3 + nw))
                self.n_packed_x3 += nw + nt

    def repack_x3(self, packed, packed_x3, stream):
        """Every layer's split packs from the fp32 packs in ``packed``: call after whatever rewrites ``packed``."""
        from .anysize_train import repack_x3
        for (_, cin), ((wo, _), _, (to, _)), (xw, xt) in zip(self.layers, self.per_layer, self.x3_layer):
            repack_x3(self.lib, self.handle, self.h, (cin + 15) // 16, packed[wo:], packed_x3[xw:], packed[to:], packed_x3[xt:], stream)

    # ------------------------------------------------------------------ the planes of one slab
    def plane_table(self):
        """The fragment planes of one slab, each [tiles][35][F/16][64][4], as (key, F, count): ``count`` planes of ``F`` features
        in a list, count None = one plane, no list; F a list = per plane, 0 for an entry that is None (a layer whose input is the
        one signal feature has no d input plane).  ``STEP_ONLY`` keys exist in the training step alone."""
        c, h, nb, nl = self.c, self.h, self.n_blocks, self.n_layers
        if nb > 0:
            table = [("z", c, 4 * nb), ("o1", c, nb), ("o2", c, nb), ("a", c, nb), ("sc", c, None), ("dz", c, 4), ("do1", c, None),
                     ("do2", c, None), ("dA", c, 2)]
        else:
            table = [("x_frag", 16, None)]
        return table + [("y_frag", 2 * h, nl), ("stash", 6 * h, nl), ("y_drop", 2 * h, nl), ("da", 6 * h, None), ("dy", 2 * h, None),
                        ("dx", [cin if cin >= 16 else 0 for _, cin in self.layers], nl), ("dy_head", 2 * h, None)]

    def _planes(self, step):
        for key, f, count in self.plane_table():
            if step or key not in STEP_ONLY:
                yield key, count, f if isinstance(f, list) else [f] * (count or 1)

    def plane_floats(self, npad, step=False):
        """Floats of the planes of a slab of ``npad`` windows."""
        return npad * T * sum(sum(feats) for _, _, feats in self._planes(step))

    def workspace_floats(self, npad):
        """(weight-gradient workspace, BN-backward workspace) floats: the largest reduction of any unit or layer."""
        h, c = self.h, self.c
        rows = [kw * cin + 1 for _, kw, cin, _ in self.units] + [cin + h + 1 for _, cin in self.layers]
        cols = [c] * len(self.units) + [2 * h] * len(self.layers)
        wgrad = max(int(self.lib.cf_gen_train_workspace_floats(r, k, npad)) for r, k in zip(rows, cols))
        return wgrad, npad // 16 * 2 * c

    def alloc(self, torch, dev, npad, zeroed, step=False):
        """The planes (``torch.zeros`` if ``zeroed``, else ``torch.empty``) and the two workspaces, as a dict by key."""
        f32 = dict(dtype=torch.float32, device=dev)
        new = torch.zeros if zeroed else torch.empty
        b = {}
        for key, count, feats in self._planes(step):
            planes = [new(npad // 16, T, f // 16, 64, 4, **f32) if f else None for f in feats]
            b[key] = planes[0] if count is None else planes
        wgrad, bn = self.workspace_floats(npad)
        b["wgrad_ws"], b["bn_ws"] = torch.empty(wgrad, **f32), torch.empty(max(bn, 1), **f32)
        return b

    # ------------------------------------------------------------------ forward
    def conv_forward(self, b, pf, npad, stream):
        """The conv stack over ``b["xpad"]``; per block  sc = BN(conv0 a), o1 = ReLU BN(conv1 a), o2 = ReLU BN(conv2 o1),
        a' = ReLU(ReLU BN(conv3 o2) + sc).  Returns the biGRU stack's input (the signal's fragment plane for the plain RNN)."""
        lib, hd = self.lib, self.handle
        a = b["xpad"]
        for k in range(self.n_blocks):
            j = 4 * k
            for u, src, res, relu, out in ((j, a, None, 0, b["sc"]), (j + 1, a, None, 1, b["o1"][k]), (j + 2, b["o1"][k], None, 1, b["o2"][k]),
                                           (j + 3, b["o2"][k], b["sc"], 1, b["a"][k])):
                off, kw, cin, cout = self.units[u]
                N.check(lib.cf_gen_conv_forward(hd, kw, cin, cout, _p(pf[off:]), _p(src), _p(res), relu,
                                                _p(b["z"][u]), _p(out), npad, stream))
            a = b["a"][k]
        if self.n_blocks == 0:
            N.check(lib.cf_gen_x_frag(hd, _p(b["xpad"]), _p(b["x_frag"]), npad, stream))
            a = b["x_frag"]
        return a

    def gru_forward(self, b, a, packed, npad, stream, after=None, packed_x3=None):
        """The biGRU layers over ``a``; ``after(layer, y)`` returns what the next layer reads in place of ``y``.  Returns (the last
        activation, [the input of each layer]).  ``packed_x3``: the split packs, with ``precision="bf16x3"``."""
        lib, hd, h = self.lib, self.handle, self.h
        x3 = self._x3(packed_x3)
        inputs = []
        for layer, (off, cin) in enumerate(self.layers):
            (wo, _), (bo, _), _ = self.per_layer[layer]
            inputs.append(a)
            if x3:
                N.check(lib.cf_gru_anysize_train_forward_x3(hd, h, (cin + 15) // 16, _p(packed_x3[self.x3_layer[layer][0]:]), _p(packed[bo:]),
                                                            _p(a), _p(b["y_frag"][layer]), _p(b["stash"][layer]), npad, stream))
            else:
                N.check(lib.cf_gru_anysize_train_forward(hd, h, (cin + 15) // 16, _p(packed[wo:]), _p(packed[bo:]), _p(a),
                                                         _p(b["y_frag"][layer]), _p(b["stash"][layer]), npad, stream))
            a = b["y_frag"][layer]
            if after is not None:
                a = after(layer, a)
        return a, inputs

    def _x3(self, packed_x3):
        if (self.precision == "bf16x3") != (packed_x3 is not None):
            raise ValueError("the split packs go with precision 'bf16x3', and only with it (this walk: %r)" % self.precision)
        return packed_x3 is not None

    # ------------------------------------------------------------------ backward
    def gru_backward(self, b, g, inputs, pf, gf, packed, npad, stream, need_w=True, before=None, packed_x3=None):
        """The biGRU layers from the gradient ``g`` of the last one's output; ``before(layer, g)`` returns the gradient the layer
        takes in place of ``g``.  Layer 0's gate gradients stay in ``b["da"]``.  Returns the gradient of the stack's input."""
        lib, hd, h = self.lib, self.handle, self.h
        x3 = self._x3(packed_x3)
        ws, wsn = b["wgrad_ws"], int(b["wgrad_ws"].numel())
        for layer in range(self.n_layers - 1, -1, -1):
            off, cin = self.layers[layer]
            _, _, (to, _) = self.per_layer[layer]
            if before is not None:
                g = before(layer, g)
            if x3:
                N.check(lib.cf_gru_anysize_train_backward_x3(hd, h, _p(packed_x3[self.x3_layer[layer][1]:]), _p(b["y_frag"][layer]),
                                                             _p(b["stash"][layer]), _p(g), _p(b["da"]), npad, stream))
            else:
                N.check(lib.cf_gru_anysize_train_backward(hd, h, _p(packed[to:]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(g),
                                                          _p(b["da"]), npad, stream))
            if need_w:
                N.check(lib.cf_gen_gru_wgrad(hd, h, cin, _p(inputs[layer]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(b["da"]),
                                             _p(ws), wsn, _p(gf[off:]), npad, stream))
            if b["dx"][layer] is not None:
                N.check(lib.cf_gen_gru_dx(hd, h, cin, _p(pf[off:]), _p(b["da"]), _p(b["dx"][layer]), npad, stream))
                g = b["dx"][layer]
        return g

    def conv_backward(self, b, dA, pf, gf, npad, stream, need_w=True):
        """The conv stack from the gradient ``dA`` of its output.  Block 0's pre-BN gradients stay in ``b["dz"]``."""
        lib, hd, units = self.lib, self.handle, self.units
        ws, wsn = b["wgrad_ws"], int(b["wgrad_ws"].numel())
        bws, bwsn = b["bn_ws"], int(b["bn_ws"].numel())
        dz = b["dz"] if self.n_blocks else None
        for k in range(self.n_blocks - 1, -1, -1):
            j = 4 * k
            a_in = b["xpad"] if k == 0 else b["a"][k - 1]

            def unit_bwd(u, grad, mask, relu, src):
                off, kw, cin, cout = units[u]
                msk = _p(mask)
                if need_w:
                    N.check(lib.cf_gen_bn_backward(hd, kw, cin, cout, _p(pf[off:]), _p(grad), msk, relu, _p(b["z"][u]), _p(dz[u - j]),
                                                   _p(bws), bwsn, _p(gf[off:]), npad, stream))
                    N.check(lib.cf_gen_conv_wgrad(hd, kw, cin, cout, _p(src), _p(dz[u - j]), _p(ws), wsn, _p(gf[off:]), npad, stream))
                else:
                    N.check(lib.cf_gen_bn_backward_data(hd, kw, cin, cout, _p(pf[off:]), _p(grad), msk, relu, _p(b["z"][u]), _p(dz[u - j]),
                                                        npad, stream))

            def unit_dx(u, out, add=None):
                off, kw, cin, cout = units[u]
                N.check(lib.cf_gen_conv_backward_data(hd, kw, cin, cout, _p(pf[off:]), _p(dz[u - j]), _p(add),
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
