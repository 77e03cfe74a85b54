"""The whole training step on the HIP kernels, without autograd (BASELINE config 5; reference ``RNN.train_network``,
catfish/models/rnn_class.py:201-210 = one ``optimizer.minimize(loss)``).

    conv stack forward            cf_res_train_forward
    biGRU layers forward          cf_gru_train_forward_dropout    (output dropout inside the kernels: no mask tensor)
    dense head + loss, fwd + bwd  cf_train_head                   (tf.losses.sigmoid_cross_entropy on the logits)
    biGRU layers backward         cf_gru_train_backward_dropout + cf_gru_train_wgrad
    conv stack backward           cf_res_train_backward
    optimizer + re-tiling         cf_opt_step                     (TF-1 RMSProp / Adam over ALL variables in one launch)
                                  or, with clip_norm / skip_nonfinite, cf_clip_norm + cf_opt_step_guarded

Every variable, its gradient and its two optimizer slots live in four flat device buffers of ONE layout
(``anysize_walk.flat_layout``), so the kernels write their gradients straight into the optimizer's input and nothing is copied,
concatenated or re-laid-out between them:

    [ conv stack: per conv+BN unit  kernel | bias | gamma | beta | moving_mean | moving_variance ]
    [ biGRU layer 0: fw ( gates kernel | gates bias | candidate kernel | candidate bias ), bw ( ... ) ] [ layer 1 ] ...
    [ final_fully_connected kernel (2H) | bias (1) ] [ 0.0 ]

The model's ``params`` dict (TF variable names) and the optimizer's slot dicts are VIEWS into these buffers, so checkpoint
I/O (``numpy_weights``, ``state_tf``) and the torch-autograd reference path keep working on the same storage.

``FlatTrainStep`` is what does not depend on the kernels: the constructor, re-homing the variables into the flat buffers, batch
loading, gradient views and the optimizer launch.  ``NativeTrainStep`` is the step of the shipped geometry (64 GRU units, 32 conv
channels, a conv stack of 1 .. ``TUNED_MAX_BLOCKS`` blocks) on the kernels tuned for it; ``anysize_step.AnySizeTrainStep`` is the
step of every other model.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from ._native import _p
from .anysize_walk import flat_layout
from .native_train import T, _stack_maps, dropout_scale_frag, frag_to_nat, nat_to_frag
from .train_mode import TUNED_MAX_BLOCKS


class FlatTrainStep(object):
    """A training step over the flat buffers.  A subclass gives ``_layout`` (which calls ``_set_layout`` and sets ``pack_idx``,
    ``pack_scale``, ``n_packed``: the gather map from the flat variables to its kernels' biGRU packs), ``alloc`` and ``run``."""

    def __init__(self, net, opt, engine, keep_prob, seed=None):
        import torch
        self.seed = int(np.random.SeedSequence(seed).generate_state(1)[0])      # 32-bit dropout seed (fresh entropy when seed is None)
        self.torch = torch
        self.net, self.opt, self.engine = net, opt, engine
        self.lib, self.handle = engine._lib, engine._handle
        self.keep_prob = float(keep_prob)
        self.dev = net.device
        self.n_layers, self.n_blocks = net.n_layers, net.n_layers_res
        self.kind = 1 if opt.choice == "Adam" else 0
        self._layout()
        self._rehome()

    def _set_layout(self, layout):
        """Adopt a ``flat_layout``, checked against the model's variables and, at 32 conv channels and a depth the tuned conv-stack
        kernels have, against the size of their parameter buffer, which is this layout's head."""
        self.entries, self.units, self.layers, self.head_off, self.zero_off = layout
        for name, _, shape in self.entries:
            if tuple(self.net.params[name].shape) != tuple(shape):
                raise ValueError("%s: shape %s, the geometry needs %s" % (name, tuple(self.net.params[name].shape), shape))
        if self.units and self.units[0][3] == 32 and self.n_blocks <= TUNED_MAX_BLOCKS:
            assert int(self.lib.cf_res_train_param_floats(self.n_blocks)) == self.layers[0][0]
        self.n_total = self.zero_off + 1

    def _rehome(self):
        """Move the variables and the optimizer slots into the flat buffers; the dicts become views."""
        torch = self.torch
        net, opt = self.net, self.opt
        self.pflat = torch.zeros(self.n_total, dtype=torch.float32, device=self.dev)
        self.gflat = torch.zeros_like(self.pflat)
        self.s1 = torch.ones_like(self.pflat) if self.kind == 0 else torch.zeros_like(self.pflat)   # TF: rms slot starts at 1
        self.s2 = torch.zeros_like(self.pflat)
        slots = (opt.ms, opt.mom) if self.kind == 0 else (opt.m, opt.v)
        with torch.no_grad():
            for name, off, shape in self.entries:
                n = int(np.prod(shape))
                old = net.params[name]
                view = self.pflat[off:off + n].view(shape)
                view.copy_(old.detach().reshape(shape))
                if old.requires_grad:
                    view.requires_grad_(True)
                    for flat, dic in zip((self.s1, self.s2), slots):
                        sv = flat[off:off + n].view(shape)
                        sv.copy_(dic[name].reshape(shape))
                        dic[name] = sv
                    opt.params[name] = view
                net.params[name] = view
        self.packed = torch.empty(self.n_packed, dtype=torch.float32, device=self.dev)
        self.norm_ws = None
        if opt.guarded:                                      # the norm's partial sums: allocated here, never inside a capture
            self.norm_ws = torch.empty(int(self.lib.cf_clip_workspace_doubles(self.n_total - 1)), dtype=torch.float64, device=self.dev)
        self.retile()

    def retile(self):
        """packed biGRU weights (forward and backward tilings of every layer) from the flat variables."""
        # (a gather without an optimizer update, e.g. after loading variables: done on the torch side)
        self.packed.copy_(self.pflat[self.pack_idx.long()] * self.pack_scale)

    @staticmethod
    def _npad(n):
        return (n + 15) // 16 * 16

    def _stream(self):
        return N.current_stream_ptr(self.torch, self.dev)

    def _opt_step(self, stream, loss=None):
        """The optimizer over every variable + re-tiling of the biGRU weights.  With ``clip_norm`` or ``skip_nonfinite`` the global
        norm of ``gflat`` and the decision for this step (which also looks at ``loss``) go in front, into ``opt.stats``, and the
        guarded optimizer reads them there: all on ``stream``, nothing comes back to the host."""
        opt = self.opt
        args = (self.handle, self.kind, _p(self.pflat), _p(self.gflat), _p(self.s1), _p(self.s2), self.n_total - 1, float(opt.lr),
                _p(opt.t), _p(self.pack_idx), _p(self.pack_scale), _p(self.packed), self.n_packed)
        if not opt.guarded:
            N.check(self.lib.cf_opt_step(*args, stream))
            return
        flags = (N.CF_CLIP_SCALE if opt.clip_norm is not None else 0) | (N.CF_CLIP_SKIP_NONFINITE if opt.skip_nonfinite else 0)
        N.check(self.lib.cf_clip_norm(self.handle, _p(self.gflat), self.n_total - 1, opt.clip_norm or 0.0, flags, _p(loss),
                                      _p(self.norm_ws), int(self.norm_ws.numel()), _p(opt.stats), stream))
        N.check(self.lib.cf_opt_step_guarded(*args, _p(opt.stats), stream))

    def load_batch(self, b, x, y):
        """The batch into the step's static device buffers.  (Pinned staging was measured in round 6 and dropped: 0.764-0.781 ms per
        256-window step against 0.754-0.762 with these plain copies, `profiles/r06_train_pinned_vs_pageable.log` -- the extra host copy
        and event cost more than the synchronous 36 KB copies.)"""
        torch = self.torch
        n = b["n"]
        b["x"].copy_(torch.as_tensor(np.asarray(x), dtype=torch.float32).reshape(n, T), non_blocking=True)
        b["y"][:n].copy_(torch.as_tensor(np.asarray(y), dtype=torch.float32).reshape(n, T), non_blocking=True)

    def grads(self):
        """{TF name: gradient view} of the last step (trainable variables only)."""
        return {name: self.gflat[off:off + int(np.prod(shape))].view(shape) for name, off, shape in self.entries
                if self.net.params[name].requires_grad}


class NativeTrainStep(FlatTrainStep):
    def __init__(self, net, opt, engine, keep_prob, seed=None):
        if net.n_layers_res < 1:
            raise ValueError("the native training step needs the ResNetRNN type (n_layers_res >= 1)")
        if net.n_layers_res > TUNED_MAX_BLOCKS:
            raise ValueError("the tuned training kernels take a conv stack of 1..%d blocks, not %d: anysize_step.AnySizeTrainStep "
                             "trains a deeper one" % (TUNED_MAX_BLOCKS, net.n_layers_res))
        super().__init__(net, opt, engine, keep_prob, seed=seed)
        # weight gradients of layer L on a second stream, next to the backward recurrence of layer L - 1 (which needs only dX of layer
        # L): at the reference's batch of 256 windows the step is a chain of launches of 16 tiles on 256 CUs, and the twelve-wave wgrad
        # workgroups fit beside the four-wave recurrence ones.  A fork / join per layer in the captured graph.
        self.overlap_wgrad = True
        self._side = None

    def _layout(self):
        self._set_layout(flat_layout(64, 32, self.n_layers, self.n_blocks))
        self.gru_off, self.cins = (list(v) for v in zip(*self.layers))
        # the gather map of native_train._stack_maps reads per (layer, direction) a block [wg | wc | bg | bc | 0.0]; in the flat
        # buffer a direction is wg | bg | wc | bc, and the one zero slot is the buffer's last float
        remap = []
        for off, cin in self.layers:
            rows = cin + 64
            for o in (off, off + rows * 192 + 192):
                remap += [np.arange(o, o + rows * 128), o + rows * 128 + 128 + np.arange(rows * 64), o + rows * 128 + np.arange(128),
                          o + rows * 192 + 128 + np.arange(64), [self.zero_off]]
        idx, scale, self.per_layer = _stack_maps(self.cins, self.dev)
        self.pack_idx = self.torch.from_numpy(np.concatenate(remap)[idx.cpu().numpy()].astype(np.int32)).to(self.dev)
        self.pack_scale = scale.contiguous()
        self.n_packed = int(self.pack_idx.numel())

    # ------------------------------------------------------------------ buffers per batch size
    def alloc(self, n):
        torch = self.torch
        dev = self.dev
        lib = self.lib
        npad = self._npad(n)
        tiles = npad // 16
        b = {"n": n, "npad": npad, "tiles": tiles}
        f32 = dict(dtype=torch.float32, device=dev)
        b["x"] = torch.zeros(n, T, **f32)
        b["y"] = torch.zeros(npad, T, **f32)
        b["z"] = torch.empty(4 * self.n_blocks, n * T, 32, **f32)
        b["res_out"] = torch.zeros(npad, T, 32, **f32)
        b["y_frag"] = [torch.empty(tiles, T, 8, 64, 4, **f32) for _ in range(self.n_layers)]
        b["stash"] = [torch.empty(tiles, T, 2, 12, 64, 4, **f32) for _ in range(self.n_layers)]
        b["y_drop"] = [torch.empty(tiles, T, 8, 64, 4, **f32) for _ in range(self.n_layers)] if self.keep_prob < 1.0 else None
        b["dy_head"] = torch.empty(tiles, T, 8, 64, 4, **f32)
        b["dx"] = [torch.empty(2, tiles, T, c // 16, 64, 4, **f32) for c in self.cins]
        # per layer: layer L's pre-activation gradients and partial sums are still being read (wgrad, side stream) while layer L - 1's are written
        b["da"] = [torch.empty(tiles, T, 2, 12, 64, 4, **f32) for _ in self.cins]
        b["head_ws"] = torch.empty(int(lib.cf_train_head_workspace_floats(self.handle, npad)), **f32)
        b["wgrad_ws"] = [torch.empty(int(lib.cf_gru_wgrad_workspace_floats(self.handle, c, npad)), **f32) for c in self.cins]
        b["res_ws"] = torch.empty(int(lib.cf_res_train_workspace_floats(self.n_blocks, n)), **f32)
        b["loss"] = torch.zeros(1, **f32)
        return b

    # ------------------------------------------------------------------ one step (all launches on the current stream)
    def run(self, b, keep_prob=None, masks=None, update=True):
        torch = self.torch
        lib, h = self.lib, self.handle
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        n, npad = b["n"], b["npad"]
        stream = self._stream()
        pf, gf = self.pflat, self.gflat
        # ---- forward
        N.check(lib.cf_res_train_forward(h, self.n_blocks, _p(pf), _p(b["x"]), _p(b["z"]), _p(b["res_out"]), n, stream))
        cur = nat_to_frag(b["res_out"])
        # output dropout: inside the kernels (hash of seed, layer, optimizer step, element) unless explicit masks are replayed
        drop = None
        in_kernel = kp < 1.0 and masks is None
        if kp < 1.0 and masks is not None:
            drop = [dropout_scale_frag(npad, kp, self.dev, masks, layer) for layer in range(self.n_layers)]
        if in_kernel and b.get("y_drop") is None:
            b["y_drop"] = [torch.empty_like(b["y_frag"][0]) for _ in range(self.n_layers)]
        step_ptr = _p(self.opt.t)
        inputs = []
        for layer in range(self.n_layers):
            fo, fn, _, _ = self.per_layer[layer]
            if in_kernel:
                N.check(lib.cf_gru_train_forward_dropout(h, self.cins[layer], _p(self.packed[fo:fo + fn]), _p(cur), _p(b["y_frag"][layer]),
                                                         _p(b["stash"][layer]), npad, _p(b["y_drop"][layer]), kp, self.seed, layer,
                                                         step_ptr, stream))
            else:
                N.check(lib.cf_gru_train_forward(h, self.cins[layer], _p(self.packed[fo:fo + fn]), _p(cur), _p(b["y_frag"][layer]),
                                                 _p(b["stash"][layer]), npad, stream))
            inputs.append(cur)
            if in_kernel:
                cur = b["y_drop"][layer]
            else:
                cur = b["y_frag"][layer] if drop is None else b["y_frag"][layer] * drop[layer]
        # ---- dense head + loss, forward and backward
        ho = self.head_off
        N.check(lib.cf_train_head(h, _p(cur), _p(pf[ho:ho + 128]), _p(pf[ho + 128:ho + 129]), _p(b["y"]), n, _p(b["dy_head"]), None,
                                  _p(b["head_ws"]), int(b["head_ws"].numel()), _p(gf[ho:ho + 129]), _p(b["loss"]), stream))
        # ---- backward through the biGRU layers
        main = torch.cuda.current_stream(self.dev)
        side = None
        if self.overlap_wgrad:
            if self._side is None:
                self._side = torch.cuda.Stream(self.dev)
            side = self._side
        g0, g1 = b["dy_head"], None
        for layer in range(self.n_layers - 1, -1, -1):
            cin = self.cins[layer]
            _, _, bo, bn = self.per_layer[layer]
            dx = b["dx"][layer]
            N.check(lib.cf_gru_train_backward_dropout(h, cin, _p(self.packed[bo:bo + bn]), _p(b["y_frag"][layer]), _p(b["stash"][layer]),
                                                      _p(g0), _p(g1), _p(drop[layer] if drop else None),
                                                      _p(dx), _p(b["da"][layer]), npad, kp if in_kernel else 1.0, self.seed, layer, step_ptr,
                                                      stream))
            go = self.gru_off[layer]
            wstream = stream
            if side is not None:
                side.wait_stream(main)                      # fork: everything up to this layer's backward recurrence
                wstream = N.stream_ptr(side)
            N.check(lib.cf_gru_train_wgrad(h, cin, _p(inputs[layer]), _p(b["y_frag"][layer]), _p(b["stash"][layer]), _p(b["da"][layer]), npad,
                                           _p(b["wgrad_ws"][layer]), int(b["wgrad_ws"][layer].numel()), _p(gf[go:]), wstream))
            g0, g1 = dx[0], dx[1]
        d_out = frag_to_nat(g0 + g1)[:n].contiguous()
        N.check(lib.cf_res_train_backward(h, self.n_blocks, _p(pf), _p(b["x"]), _p(b["z"]), _p(d_out), _p(b["res_ws"]),
                                          int(b["res_ws"].numel()), _p(gf), n, stream))
        if side is not None:
            main.wait_stream(side)                          # join: the optimizer reads every gradient
        if update:
            self._opt_step(stream, b["loss"])
        return b["loss"]

    def dropout_scales(self, n, keep_prob=None):
        """The mask / keep_prob tensors the kernels apply at the CURRENT optimizer step, as {(layer, "fw"|"bw"): 0/1 array
        [n, 35, 64]} (tests replay them through the torch reference path)."""
        torch = self.torch
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        npad = self._npad(n)
        stream = self._stream()
        out = {}
        for layer in range(self.n_layers):
            sc = torch.empty(npad // 16, T, 8, 64, 4, dtype=torch.float32, device=self.dev)
            N.check(self.lib.cf_dropout_scale(self.handle, kp, self.seed, layer, _p(self.opt.t), npad, _p(sc), stream))
            m = (frag_to_nat(sc)[:n] > 0).to(torch.float32).cpu().numpy()
            out[(layer, "fw")], out[(layer, "bw")] = m[:, :, :64], m[:, :, 64:]
        return out
