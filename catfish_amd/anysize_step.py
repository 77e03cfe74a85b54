"""The whole training step of ANY geometry on the HIP kernels, without autograd (``Trainer(..., native=True)`` at every
geometry other than the shipped 64 / 32 one, RNN or ResNetRNN type).

    conv stack forward            cf_gen_conv_forward (BN as an epilogue affine of the step's gamma / beta, z stashed)
    biGRU layers forward          cf_gru_anysize_train_forward + cf_gen_dropout (the tuned kernels' in-kernel mask hash)
    dense head + loss, fwd + bwd  cf_gen_head
    biGRU layers backward         cf_gen_dropout + cf_gru_anysize_train_backward + cf_gen_gru_wgrad + cf_gen_gru_dx
    conv stack backward           cf_gen_bn_backward + cf_gen_conv_wgrad + cf_gen_conv_backward_data
    optimizer + re-tiling         cf_opt_step (one gather map rebuilds every layer's wpack | bpack | wtpack)

One flat layout (params | grads | two optimizer slots) for every geometry, as ``native_step.NativeTrainStep`` has for the
shipped one -- whose geometry-free parts (re-homing the variables into the flat buffers, batch loading, gradient views) this
class inherits:

    [ conv stack: per conv+BN unit  kernel | bias | gamma | beta | moving_mean | moving_variance ]
    [ biGRU layer 0: fw ( gates kernel | gates bias | candidate kernel | candidate bias ), bw ( ... ) ] [ layer 1 ] ...
    [ final_fully_connected kernel (2H) | bias (1) ] [ 0.0 ]
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .native_step import GRU_PRE, NativeTrainStep, _p
from .native_train import T, frag_to_nat, nat_to_frag, res_unit_names


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
            pre = GRU_PRE % (layer, d)
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


class AnySizeTrainStep(NativeTrainStep):
    def __init__(self, net, opt, engine, keep_prob, seed=None):
        import torch
        self.seed = int(np.random.SeedSequence(seed).generate_state(1)[0])      # 32-bit dropout seed (fresh entropy when seed is None)
        self.torch = torch
        self.net, self.opt, self.engine = net, opt, engine
        self.lib, self.handle = engine._lib, engine._handle
        self.keep_prob = float(keep_prob)
        self.dev = net.device
        self.n_layers, self.n_blocks = net.n_layers, net.n_layers_res
        p = net.params
        self.h = int(p[GRU_PRE % (0, "fw") + "/candidate/bias"].shape[0])
        self.c = int(p["conv1d/bias"].shape[0]) if self.n_blocks > 0 else 0
        self.kind = 1 if opt.choice == "Adam" else 0
        self._layout()
        self._rehome()
        self._bufs = None

    def _layout(self):
        self.entries, self.units, self.layers, self.head_off, self.zero_off = flat_layout(self.h, self.c, self.n_layers, self.n_blocks)
        for name, _, shape in self.entries:
            if tuple(self.net.params[name].shape) != tuple(shape):
                raise ValueError("%s: shape %s, the geometry needs %s" % (name, tuple(self.net.params[name].shape), shape))
        self.n_total = self.zero_off + 1
        idx, scale, self.per_layer = flat_pack_map(self.h, self.layers, self.zero_off)
        self.pack_idx = self.torch.from_numpy(idx.astype(np.int32)).to(self.dev)
        self.pack_scale = self.torch.from_numpy(scale).to(self.dev)
        self.n_packed = int(idx.size)

    # ------------------------------------------------------------------ buffers per batch size
    def _alloc(self, n):
        torch = self.torch
        lib, h, c = self.lib, self.h, self.c
        npad = (n + 15) // 16 * 16
        tiles = npad // 16
        f32 = dict(dtype=torch.float32, device=self.dev)
        plane = lambda f: torch.zeros(tiles, T, f // 16, 64, 4, **f32)          # noqa: E731
        b = {"n": n, "npad": npad, "tiles": tiles}
        b["xpad"] = torch.zeros(npad, T, **f32)
        b["x"] = b["xpad"][:n]                                 # load_batch writes the real windows; padding windows stay 0
        b["y"] = torch.zeros(npad, T, **f32)
        nb = self.n_blocks
        if nb > 0:
            b["z"] = [plane(c) for _ in range(4 * nb)]
            b["o1"], b["o2"], b["a"] = ([plane(c) for _ in range(nb)] for _ in range(3))
            b["sc"] = plane(c)
            b["dz"] = [plane(c) for _ in range(4)]
            b["do1"], b["do2"] = plane(c), plane(c)
            b["dA"] = [plane(c), plane(c)]
            b["bn_ws"] = torch.empty(tiles * 2 * c, **f32)
        else:
            b["x_frag"] = plane(16)
        b["y_frag"] = [plane(2 * h) for _ in range(self.n_layers)]
        b["stash"] = [plane(6 * h) for _ in range(self.n_layers)]
        b["y_drop"] = [plane(2 * h) for _ in range(self.n_layers)]
        b["da"] = plane(6 * h)
        b["dy"] = plane(2 * h)
        b["dx"] = [plane(cin) if cin >= 16 else None for _, cin in self.layers]
        b["dy_head"] = plane(2 * h)
        rows = [kw * cin + 1 for _, kw, cin, _ in self.units] + [cin + h + 1 for _, cin in self.layers]
        cols = [c] * len(self.units) + [2 * h] * len(self.layers)
        b["wgrad_ws"] = torch.empty(max(int(lib.cf_gen_train_workspace_floats(r, k, npad)) for r, k in zip(rows, cols)), **f32)
        b["head_ws"] = torch.empty(int(lib.cf_gen_head_workspace_floats(2 * h, npad)), **f32)
        b["loss"] = torch.zeros(1, **f32)
        return b

    def _scales(self, npad, kp, masks, layer):
        torch = self.torch
        m = torch.cat([torch.as_tensor(np.asarray(masks[(layer, d)]), dtype=torch.float32, device=self.dev) for d in ("fw", "bw")], 2)
        if m.shape[0] < npad:
            m = torch.cat([m, m.new_zeros(npad - m.shape[0], T, 2 * self.h)], 0)
        return nat_to_frag(m) / kp

    # ------------------------------------------------------------------ one step (all launches on the current stream)
    def run(self, b, keep_prob=None, masks=None, update=True):
        torch = self.torch
        lib, hd = self.lib, self.handle
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        n, npad, h = b["n"], b["npad"], self.h
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        pf, gf = self.pflat, self.gflat
        ws, wsn = b["wgrad_ws"], int(b["wgrad_ws"].numel())
        drop = kp < 1.0
        scales = [self._scales(npad, kp, masks, layer) for layer in range(self.n_layers)] if drop and masks is not None else None
        step_ptr = _p(self.opt.t)
        units = self.units
        # ---- conv stack forward: per block  sc = BN(conv0 a), o1 = ReLU BN(conv1 a), o2 = ReLU BN(conv2 o1), a' = ReLU(ReLU BN(conv3 o2) + sc)
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
        # ---- biGRU layers forward, output dropout after each
        inputs = []
        packed = self.packed
        for layer, (off, cin) in enumerate(self.layers):
            (wo, _), (bo, _), _ = self.per_layer[layer]
            inputs.append(a)
            N.check(lib.cf_gru_anysize_train_forward(hd, h, (cin + 15) // 16, _p(packed[wo:]), _p(packed[bo:]), _p(a), _p(b["y_frag"][layer]),
                                                     _p(b["stash"][layer]), npad, stream))
            a = b["y_frag"][layer]
            if drop:
                N.check(lib.cf_gen_dropout(hd, h, kp, self.seed, layer, step_ptr, None if scales is None else _p(scales[layer]), _p(a),
                                           _p(b["y_drop"][layer]), npad, stream))
                a = b["y_drop"][layer]
        # ---- dense head + loss, forward and backward
        ho = self.head_off
        N.check(lib.cf_gen_head(hd, 2 * h, _p(a), _p(pf[ho:]), _p(b["y"]), n, _p(b["dy_head"]), None, _p(b["head_ws"]),
                                int(b["head_ws"].numel()), _p(gf[ho:]), _p(b["loss"]), npad, stream))
        # ---- biGRU layers backward
        g = b["dy_head"]
        for layer in range(self.n_layers - 1, -1, -1):
            off, cin = self.layers[layer]
            _, _, (to, _) = self.per_layer[layer]
            if drop:
                N.check(lib.cf_gen_dropout(hd, h, kp, self.seed, layer, step_ptr, None if scales is None else _p(scales[layer]), _p(g),
                                           _p(b["dy"]), npad, stream))
                g = b["dy"]
            N.check(lib.cf_gru_anysize_train_backward(hd, h, _p(packed[to:]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(g),
                                                      _p(b["da"]), npad, stream))
            N.check(lib.cf_gen_gru_wgrad(hd, h, cin, _p(inputs[layer]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(b["da"]),
                                         _p(ws), wsn, _p(gf[off:]), npad, stream))
            if b["dx"][layer] is not None:
                N.check(lib.cf_gen_gru_dx(hd, h, cin, _p(pf[off:]), _p(b["da"]), _p(b["dx"][layer]), npad, stream))
                g = b["dx"][layer]
        # ---- conv stack backward
        bws, bwsn = b["bn_ws"] if self.n_blocks else None, int(b["bn_ws"].numel()) if self.n_blocks else 0
        dA = g
        for k in range(self.n_blocks - 1, -1, -1):
            j = 4 * k
            a_in = b["xpad"] if k == 0 else b["a"][k - 1]
            dz = b["dz"]

            def unit_bwd(u, grad, mask, relu, src):
                off, kw, cin, cout = units[u]
                N.check(lib.cf_gen_bn_backward(hd, kw, cin, cout, _p(pf[off:]), _p(grad), None if mask is None else _p(mask), relu,
                                               _p(b["z"][u]), _p(dz[u - j]), _p(bws), bwsn, _p(gf[off:]), npad, stream))
                N.check(lib.cf_gen_conv_wgrad(hd, kw, cin, cout, _p(src), _p(dz[u - j]), _p(ws), wsn, _p(gf[off:]), npad, stream))

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
        # ---- optimizer over every variable + re-tiling of the biGRU weights
        if update:
            N.check(lib.cf_opt_step(hd, self.kind, _p(pf), _p(gf), _p(self.s1), _p(self.s2), self.n_total - 1, float(self.opt.lr),
                                    _p(self.opt.t), _p(self.pack_idx), _p(self.pack_scale), _p(self.packed), self.n_packed, stream))
        return b["loss"]

    def dropout_scales(self, n, keep_prob=None):
        """The masks the kernels apply at the CURRENT optimizer step, as {(layer, "fw"|"bw"): 0/1 array [n, 35, H]}."""
        torch = self.torch
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        npad = (n + 15) // 16 * 16
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        ones = torch.ones(npad // 16, T, self.h // 8, 64, 4, dtype=torch.float32, device=self.dev)
        out = {}
        for layer in range(self.n_layers):
            sc = torch.empty_like(ones)
            N.check(self.lib.cf_gen_dropout(self.handle, self.h, kp, self.seed, layer, _p(self.opt.t), None, _p(ones), _p(sc), npad, stream))
            m = (frag_to_nat(sc)[:n] > 0).to(torch.float32).cpu().numpy()
            out[(layer, "fw")], out[(layer, "bw")] = m[:, :, :self.h], m[:, :, self.h:]
        return out
