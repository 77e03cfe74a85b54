"""The whole training step of ANY geometry on the HIP kernels, without autograd (``Trainer(..., native=True)`` for every
model the tuned kernels do not take, RNN or ResNetRNN type: every size other than 64 / 32, 64 units without a conv stack, and 64 / 32
with more than ``train_mode.TUNED_MAX_BLOCKS`` blocks).

    conv stack forward            cf_gen_conv_forward (BN as an epilogue affine of the step's gamma / beta, z stashed)
    biGRU layers forward          cf_gru_anysize_train_forward + cf_gen_dropout (the tuned kernels' in-kernel mask hash)
    dense head + loss, fwd + bwd  cf_gen_head
    biGRU layers backward         cf_gen_dropout + cf_gru_anysize_train_backward + cf_gen_gru_wgrad + cf_gen_gru_dx
    conv stack backward           cf_gen_bn_backward + cf_gen_conv_wgrad + cf_gen_conv_backward_data
    optimizer + re-tiling         cf_opt_step (one gather map rebuilds every layer's wpack | bpack | wtpack); with clip_norm /
                                  skip_nonfinite cf_clip_norm + cf_opt_step_guarded (``FlatTrainStep._opt_step``)

The conv and biGRU launches, their buffers and the flat layout (params | grads | two optimizer slots, one layout for every
geometry) are ``anysize_walk``'s, shared with the operator's backward; this module adds the dropout hooks, the head and the
optimizer.  What does not depend on the kernels is ``native_step.FlatTrainStep``, shared with the step of the shipped geometry.

``precision="bf16x3"``: the two recurrences read split bf16 packs from ``packed_x3``, a second buffer beside ``packed``.  Whatever
rewrites ``packed`` -- ``retile`` and the optimizer launch, the latter inside the captured step -- is followed on the same stream
by ``AnySizeWalk.repack_x3``, so a split pack never lags behind its fp32 pack.
"""
from __future__ import annotations

from . import _native as N
from ._native import _p
from .anysize_walk import AnySizeWalk, flat_layout, flat_pack_map  # noqa: F401  (the layout's public home)
from .native_step import FlatTrainStep
from .native_train import T, dropout_scale_frag, frag_to_nat


class AnySizeTrainStep(FlatTrainStep):
    def __init__(self, net, opt, engine, keep_prob, seed=None, precision="fp32"):
        self.precision = precision                              # checked by AnySizeWalk
        self.packed_x3 = None
        super().__init__(net, opt, engine, keep_prob, seed=seed)

    def _layout(self):
        p = self.net.params
        self.h = int(p[N.gru_prefix(0, "fw") + "/candidate/bias"].shape[0])
        self.c = int(p["conv1d/bias"].shape[0]) if self.n_blocks > 0 else 0
        self.walk = w = AnySizeWalk(self.lib, self.handle, self.h, self.c, self.n_layers, self.n_blocks, precision=self.precision)
        self._set_layout(w.layout)
        self.pack_idx = self.torch.from_numpy(w.pack_idx.astype("int32")).to(self.dev)
        self.pack_scale = self.torch.from_numpy(w.pack_scale).to(self.dev)
        self.n_packed = int(w.pack_idx.size)

    # ------------------------------------------------------------------ the split packs follow the fp32 packs
    def retile(self):
        super().retile()
        if self.precision == "bf16x3":
            if self.packed_x3 is None:
                self.packed_x3 = self.torch.empty(self.walk.n_packed_x3, dtype=self.torch.float32, device=self.dev)
            self.walk.repack_x3(self.packed, self.packed_x3, self._stream())

    def _opt_step(self, stream, loss=None):
        super()._opt_step(stream, loss)
        if self.precision == "bf16x3":                          # (after a skipped step the repack sees unchanged weights)
            self.walk.repack_x3(self.packed, self.packed_x3, stream)

    # ------------------------------------------------------------------ buffers per batch size
    def alloc(self, n):
        torch = self.torch
        npad = self._npad(n)
        f32 = dict(dtype=torch.float32, device=self.dev)
        b = self.walk.alloc(torch, self.dev, npad, zeroed=True, step=True)
        b.update(n=n, npad=npad, tiles=npad // 16)
        b["xpad"] = torch.zeros(npad, T, **f32)
        b["x"] = b["xpad"][:n]                                 # load_batch writes the real windows; padding windows stay 0
        b["y"] = torch.zeros(npad, T, **f32)
        b["head_ws"] = torch.empty(int(self.lib.cf_gen_head_workspace_floats(2 * self.h, npad)), **f32)
        b["loss"] = torch.zeros(1, **f32)
        return b

    # ------------------------------------------------------------------ one step (all launches on the current stream)
    def run(self, b, keep_prob=None, masks=None, update=True):
        lib, hd, h, w = self.lib, self.handle, self.h, self.walk
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        n, npad = b["n"], b["npad"]
        stream = self._stream()
        pf, gf, packed, packed_x3 = self.pflat, self.gflat, self.packed, self.packed_x3
        # output dropout after each layer and on the gradient coming back into it: the kernel's own mask hash, or replayed masks
        after = before = None
        if kp < 1.0:
            scales = None if masks is None else [dropout_scale_frag(npad, kp, self.dev, masks, layer, 2 * h) for layer in range(self.n_layers)]
            step_ptr = _p(self.opt.t)

            def dropout(layer, src, dst):
                N.check(lib.cf_gen_dropout(hd, h, kp, self.seed, layer, step_ptr, _p(scales[layer] if scales else None), _p(src),
                                           _p(dst), npad, stream))
                return dst

            after = lambda layer, y: dropout(layer, y, b["y_drop"][layer])          # noqa: E731
            before = lambda layer, g: dropout(layer, g, b["dy"])                    # noqa: E731
        a, inputs = w.gru_forward(b, w.conv_forward(b, pf, npad, stream), packed, npad, stream, after=after, packed_x3=packed_x3)
        # ---- dense head + loss, forward and backward
        ho = self.head_off
        N.check(lib.cf_gen_head(hd, 2 * h, _p(a), _p(pf[ho:]), _p(b["y"]), n, _p(b["dy_head"]), None, _p(b["head_ws"]),
                                int(b["head_ws"].numel()), _p(gf[ho:]), _p(b["loss"]), npad, stream))
        g = w.gru_backward(b, b["dy_head"], inputs, pf, gf, packed, npad, stream, before=before, packed_x3=packed_x3)
        w.conv_backward(b, g, pf, gf, npad, stream)
        if update:
            self._opt_step(stream, b["loss"])
        return b["loss"]

    def dropout_scales(self, n, keep_prob=None):
        """The masks the kernels apply at the CURRENT optimizer step, as {(layer, "fw"|"bw"): 0/1 array [n, 35, H]}."""
        torch = self.torch
        kp = self.keep_prob if keep_prob is None else float(keep_prob)
        npad = self._npad(n)
        stream = self._stream()
        ones = torch.ones(npad // 16, T, self.h // 8, 64, 4, dtype=torch.float32, device=self.dev)
        out = {}
        for layer in range(self.n_layers):
            sc = torch.empty_like(ones)
            N.check(self.lib.cf_gen_dropout(self.handle, self.h, kp, self.seed, layer, _p(self.opt.t), None, _p(ones), _p(sc), npad, stream))
            m = (frag_to_nat(sc)[:n] > 0).to(torch.float32).cpu().numpy()
            out[(layer, "fw")], out[(layer, "bw")] = m[:, :, :self.h], m[:, :, self.h:]
        return out
