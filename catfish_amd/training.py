"""Training step (BASELINE config 5) -- the reference's ``train_network`` on PyTorch-ROCm autograd.

Reference: ``RNN.train_network`` (catfish/models/rnn_class.py:201-210) runs one
``optimizer.minimize(loss)`` step; loss = mean sigmoid cross-entropy over all B*35 outputs
(:74-79); optimizer = Adam or RMSProp with TF-1 defaults (:62-71); dropout with
``keep_prob`` on the GRU OUTPUTS only (:151-154); batch-norm stays in inference mode while
training (``training`` is never passed, resnet_class.py:61) so only gamma/beta learn and the
moving statistics never move.

The graph is restated with torch ops in the TF variable layout (same names/shapes as the
checkpoint), so trained weights go straight back into the HIP engine or a checkpoint-V2 bundle
(``checkpoint.write_checkpoint``).  The optimizer updates follow TF's formulas, not torch.optim's
(epsilon placement and slot initialisation differ).
"""
from __future__ import annotations

import gc

import numpy as np

from .batching import quiet_gc
from .train_mode import STEP_KINDS, TrainMode, geometry, tuned_geometry


def _names(n_layers, n_layers_res):
    conv = lambda j: "conv1d" if j == 0 else "conv1d_%d" % j            # noqa: E731
    bn = lambda j: "batch_normalization" if j == 0 else "batch_normalization_%d" % j   # noqa: E731
    return conv, bn


class TorchResNetRNN(object):
    """Differentiable restatement of the ResNetRNN graph; parameters are a dict of torch tensors."""

    def __init__(self, weights, n_layers, n_layers_res, device="cpu", dtype=None, precision="fp32"):
        import torch
        self.torch = torch
        self.precision = precision      # of the any-size HIP recurrences in _logits_anysize ("fp32" | "bf16x3"); pure torch ignores it
        self.dtype = dtype or torch.float32
        self.device = torch.device(device)
        self.n_layers = int(n_layers)
        self.n_layers_res = int(n_layers_res)
        self.params = {}
        for k, v in weights.items():
            t = torch.tensor(np.asarray(v), dtype=self.dtype, device=self.device)
            t.requires_grad_(not k.endswith(("moving_mean", "moving_variance")))
            self.params[k] = t

    def trainable(self):
        return {k: v for k, v in self.params.items() if v.requires_grad}

    def numpy_weights(self):
        return {k: v.detach().cpu().numpy().astype(np.float32) for k, v in self.params.items()}

    # ---- forward ---------------------------------------------------------------------------
    def _conv_bn(self, x, j):
        torch = self.torch
        F = torch.nn.functional
        conv, bn = _names(self.n_layers, self.n_layers_res)
        p = self.params
        k = p[conv(j) + "/kernel"]                       # [K, Cin, Cout]
        y = F.conv1d(x, k.permute(2, 1, 0), p[conv(j) + "/bias"], padding=(k.shape[0] - 1) // 2)
        inv = p[bn(j) + "/gamma"] * torch.rsqrt(p[bn(j) + "/moving_variance"] + 1e-3)
        return y * inv[None, :, None] + (p[bn(j) + "/beta"] - p[bn(j) + "/moving_mean"] * inv)[None, :, None]

    def logits(self, x, keep_prob=1.0, generator=None, engine=None, masks=None):
        """x [N, 35] or [N, 35, 1] -> logits [N, 35].

        With ``engine`` (a fp32 HipEngine on the same GPU) the biGRU layers run on the native HIP
        forward/backward kernels (catfish_amd/native_train.py); everything else stays torch autograd.
        ``masks`` ({(layer, "fw"|"bw"): 0/1 array [N, 35, 64]}) replaces the random dropout draws (tests)."""
        torch = self.torch
        p = self.params
        x = torch.as_tensor(x, dtype=self.dtype, device=self.device)
        if x.dim() == 3:
            x = x[:, :, 0]
        a = x[:, None, :]                                # [N, C, T]
        if engine is not None and not tuned_geometry(*geometry(p, self.n_layers_res)[:2], self.n_layers_res):
            return self._logits_anysize(a, keep_prob, generator, engine, masks)      # recurrence on the any-size HIP kernels
        native_res = engine is not None and self.n_layers_res > 0 and self.dtype == torch.float32
        if native_res:                                   # residual conv stack on the HIP training kernels
            from .native_train import native_res_stack, res_unit_names
            a = native_res_stack(x, [p[k] for unit in res_unit_names(self.n_layers_res) for k in unit], engine)
        for d in range(0 if native_res else self.n_layers_res):
            j0 = 4 * d
            sc = self._conv_bn(a, j0)
            o = torch.relu(self._conv_bn(a, j0 + 1))
            o = torch.relu(self._conv_bn(o, j0 + 2))
            o = torch.relu(self._conv_bn(o, j0 + 3))
            a = torch.relu(o + sc)
        if not native_res:
            a = a.permute(0, 2, 1)                       # [N, T, C]
        n, t_len, _ = a.shape
        if engine is not None:                           # all biGRU layers on the HIP training kernels
            from .native_train import native_gru_stack
            pre = "stack_bidirectional_rnn/cell_%d/bidirectional_rnn/%s/gru_cell"
            plist = [p[(pre % (layer, d)) + k] for layer in range(self.n_layers) for d in ("fw", "bw")
                     for k in ("/gates/kernel", "/gates/bias", "/candidate/kernel", "/candidate/bias")]
            a = native_gru_stack(a, plist, engine, keep_prob, masks)
        for layer in range(self.n_layers if engine is None else 0):
            outs = []
            for dname, rev in (("fw", False), ("bw", True)):
                pre = "stack_bidirectional_rnn/cell_%d/bidirectional_rnn/%s/gru_cell" % (layer, dname)
                wg, bg = p[pre + "/gates/kernel"], p[pre + "/gates/bias"]
                wc, bc = p[pre + "/candidate/kernel"], p[pre + "/candidate/bias"]
                hsz = wc.shape[1]
                h = torch.zeros(n, hsz, dtype=self.dtype, device=self.device)
                seq = [None] * t_len
                for s in (range(t_len - 1, -1, -1) if rev else range(t_len)):
                    xt = a[:, s, :]
                    g = torch.sigmoid(torch.cat([xt, h], 1) @ wg + bg)
                    r, u = g[:, :hsz], g[:, hsz:]
                    c = torch.tanh(torch.cat([xt, r * h], 1) @ wc + bc)
                    h = u * h + (1 - u) * c
                    seq[s] = h
                out = torch.stack(seq, 1)
                if keep_prob < 1.0:                      # DropoutWrapper(output_keep_prob): outputs only
                    if masks is not None:
                        mask = torch.as_tensor(masks[(layer, dname)], dtype=self.dtype, device=self.device)
                    else:
                        mask = torch.floor(keep_prob + torch.rand(out.shape, generator=generator, device=self.device,
                                                                  dtype=self.dtype))
                    out = out / keep_prob * mask
                outs.append(out)
            a = torch.cat(outs, 2)
        return (a.reshape(-1, a.shape[2]) @ p["final_fully_connected/kernel"] +
                p["final_fully_connected/bias"]).reshape(n, t_len)

    def _logits_anysize(self, a, keep_prob, generator, engine, masks):
        """Every model the tuned training kernels do not take (``train_mode.tuned_geometry``): conv stack, dropout and head in torch,
        every biGRU layer one forward and one backward launch of the any-size HIP kernels (catfish_amd/anysize_train.py)."""
        torch = self.torch
        p = self.params
        from .anysize_train import anysize_bigru
        for d in range(self.n_layers_res):
            j0 = 4 * d
            sc = self._conv_bn(a, j0)
            o = torch.relu(self._conv_bn(a, j0 + 1))
            o = torch.relu(self._conv_bn(o, j0 + 2))
            o = torch.relu(self._conv_bn(o, j0 + 3))
            a = torch.relu(o + sc)
        a = a.permute(0, 2, 1).contiguous()              # [N, T, C]
        n, t_len, _ = a.shape
        pre = "stack_bidirectional_rnn/cell_%d/bidirectional_rnn/%s/gru_cell"
        for layer in range(self.n_layers):
            params8 = [p[(pre % (layer, d)) + k] for d in ("fw", "bw")
                       for k in ("/gates/kernel", "/gates/bias", "/candidate/kernel", "/candidate/bias")]
            a = anysize_bigru(a, params8, engine, precision=self.precision)
            if keep_prob < 1.0:                          # DropoutWrapper(output_keep_prob), one draw per direction as in the torch path
                hsz = a.shape[2] // 2
                parts = []
                for dname in ("fw", "bw"):
                    if masks is not None:
                        parts.append(torch.as_tensor(masks[(layer, dname)], dtype=self.dtype, device=self.device))
                    else:
                        parts.append(torch.floor(keep_prob + torch.rand((n, t_len, hsz), generator=generator, device=self.device,
                                                                        dtype=self.dtype)))
                a = a / keep_prob * torch.cat(parts, 2)
        return (a.reshape(-1, a.shape[2]) @ p["final_fully_connected/kernel"] + p["final_fully_connected/bias"]).reshape(n, t_len)

    def loss(self, x, y, keep_prob=1.0, generator=None, engine=None, masks=None):
        """tf.losses.sigmoid_cross_entropy + reduce_mean (rnn_class.py:74-79)."""
        torch = self.torch
        z = self.logits(x, keep_prob, generator, engine, masks)
        y = torch.as_tensor(y, dtype=self.dtype, device=self.device).reshape(z.shape)
        return torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="mean")


def check_clip(clip_norm, skip_nonfinite):
    """The two options of gradient clipping, checked -> (clip_norm as a float or None, skip_nonfinite as a bool).  ``clip_norm`` is
    None or a finite number > 0 (anything else: ValueError); ``skip_nonfinite`` None means "on exactly when clipping is"."""
    if clip_norm is not None:
        if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float, np.integer, np.floating)):
            raise ValueError("clip_norm must be None or a finite number > 0, not %r" % (clip_norm,))
        clip_norm = float(clip_norm)
        if not (np.isfinite(clip_norm) and clip_norm > 0.0):
            raise ValueError("clip_norm must be None or a finite number > 0, not %r" % (clip_norm,))
    return clip_norm, (clip_norm is not None) if skip_nonfinite is None else bool(skip_nonfinite)


class TFOptimizer(object):
    """tf.train.AdamOptimizer / RMSPropOptimizer update rules with TF-1 defaults (rnn_class.py:62-71).

    ``clip_norm`` / ``skip_nonfinite`` (both off by default; ``check_clip``) put global-norm clipping and a non-finite-step guard
    in front of the update, for this class's own ``step`` and for the native steps, which read the options and share ``stats``:
    S = the float64 sum of the squared gradients, g = sqrt(S), s32 = float32(clip_norm / max(g, clip_norm))
    (``tf.clip_by_global_norm``; 1 without ``clip_norm``), the update consumes g_i * s32, and with ``skip_nonfinite`` a step whose S
    or loss is not finite changes nothing, ``t`` included.  ``stats``: device float64 [4] = g of the last step, the scale applied
    (-1 on a skipped step), steps clipped (s32 < 1), steps skipped."""

    def __init__(self, params, choice, lr, clip_norm=None, skip_nonfinite=None):
        import torch
        self.torch = torch
        if choice not in ("Adam", "RMSProp"):
            raise ValueError("Given optimizer choice is not known. Choose 'Adam' or 'RMSProp'.")
        self.choice = choice
        self.lr = float(lr)
        self.clip_norm, self.skip_nonfinite = check_clip(clip_norm, skip_nonfinite)
        self.guarded = self.clip_norm is not None or self.skip_nonfinite
        self.keep_grads = False      # graph mode: gradients live in the captured pool and are overwritten on replay
        self.params = params
        first = next(iter(params.values()))
        # step counter as a DEVICE tensor so that the bias correction is computed by captured ops (hipGraph replay)
        self.t = torch.zeros((), dtype=torch.float64, device=first.device)
        self._b1 = torch.tensor(0.9, dtype=torch.float64, device=first.device)      # created outside any capture
        self._b2 = torch.tensor(0.999, dtype=torch.float64, device=first.device)
        self.stats = torch.zeros(4, dtype=torch.float64, device=first.device)
        self._clip = torch.tensor(self.clip_norm or 0.0, dtype=torch.float64, device=first.device)
        if choice == "Adam":
            self.m = {k: torch.zeros_like(v) for k, v in params.items()}
            self.v = {k: torch.zeros_like(v) for k, v in params.items()}
        else:
            self.ms = {k: torch.ones_like(v) for k, v in params.items()}      # TF initialises the rms slot to 1
            self.mom = {k: torch.zeros_like(v) for k, v in params.items()}

    # ---- slot variables under their TensorFlow names (what tf.train.Saver writes next to the weights) ----------
    def state_tf(self):
        """{checkpoint name: ndarray}: ``<var>/RMSProp`` (rms), ``<var>/RMSProp_1`` (momentum) or ``<var>/Adam`` (m),
        ``<var>/Adam_1`` (v), ``optimizer/beta{1,2}_power`` (the optimizer is built under name_scope "optimizer",
        rnn_class.py:62-71)."""
        out = {}
        if self.choice == "Adam":
            t = float(self.t)
            for k in self.params:
                out[k + "/Adam"] = self.m[k].detach().cpu().numpy().astype(np.float32)
                out[k + "/Adam_1"] = self.v[k].detach().cpu().numpy().astype(np.float32)
            out["optimizer/beta1_power"] = np.float32(0.9 ** (t + 1))       # TF stores beta^(t+1): initial value beta
            out["optimizer/beta2_power"] = np.float32(0.999 ** (t + 1))
        else:
            for k in self.params:
                out[k + "/RMSProp"] = self.ms[k].detach().cpu().numpy().astype(np.float32)
                out[k + "/RMSProp_1"] = self.mom[k].detach().cpu().numpy().astype(np.float32)
        return out

    def load_state_tf(self, state):
        """Continue from restored slot variables (``saver.restore`` brings them back, rnn_class.py:191-198).
        Entries of the other optimizer, or missing ones, leave the fresh initial value in place."""
        torch = self.torch
        a, b = ("Adam", "Adam_1") if self.choice == "Adam" else ("RMSProp", "RMSProp_1")
        first, second = (self.m, self.v) if self.choice == "Adam" else (self.ms, self.mom)
        with torch.no_grad():
            for k, p in self.params.items():
                for slot, name in ((first, k + "/" + a), (second, k + "/" + b)):
                    if name in state:
                        slot[k].copy_(torch.as_tensor(np.asarray(state[name]), dtype=p.dtype).reshape(p.shape))
            if self.choice == "Adam":
                # TF stores beta^(t+1).  beta1_power = 0.9^(t+1) underflows fp32 after ~830 steps (denormal, then 0), so
                # the step count is read from beta2_power = 0.999^(t+1) (good for ~87 000 steps); when that is gone too
                # the bias corrections are 1 to fp32 precision anyway and a large count stands in.
                t_new = None
                for name, beta in (("optimizer/beta2_power", 0.999), ("beta2_power", 0.999),
                                   ("optimizer/beta1_power", 0.9), ("beta1_power", 0.9)):
                    if name in state:
                        v = float(state[name])
                        if 1e-30 < v < 1.0:
                            t_new = round(np.log(v) / np.log(beta)) - 1
                            break
                        if v <= 1e-30:
                            t_new = 1000000
                if t_new is not None:
                    self.t.fill_(max(0, t_new))

    def _guard(self, gs, loss):
        """The definition in the class docstring with device scalars only (graph-safe) -> (the scaled gradients, ok: a bool
        scalar tensor, False for a step to skip); updates ``stats``."""
        torch = self.torch
        S = torch.stack([(g.detach().to(torch.float64) ** 2).sum() for g in gs]).sum()
        gn = torch.sqrt(S)
        ok = torch.ones((), dtype=torch.bool, device=S.device)
        if self.skip_nonfinite:
            ok = torch.isfinite(S)
            if loss is not None:
                ok = ok & torch.isfinite(loss.detach()).all()
        one = torch.ones((), dtype=torch.float64, device=S.device)
        s32 = one
        if self.clip_norm is not None:
            # max(g, c) as fmax: a NaN norm leaves c (only met with skip_nonfinite switched off)
            s32 = (self._clip / torch.fmax(gn, self._clip)).to(torch.float32).to(torch.float64)
        self.stats[0] = gn
        self.stats[1] = torch.where(ok, s32, -one)
        self.stats[2] += (ok & (s32 < 1.0)).to(torch.float64)
        self.stats[3] += (~ok).to(torch.float64)
        # a skipped step's gradients are not used; zeros keep NaN / Inf out of the arithmetic whose result is discarded
        return [torch.where(ok, g * s32.to(g.dtype), torch.zeros_like(g)) for g in gs], ok

    def step(self, loss=None):
        """One update of every parameter with multi-tensor (``torch._foreach_*``) ops: a handful of launches
        instead of ~8 per parameter tensor (66 tensors).  ``loss``: the step's loss, which the non-finite guard also looks at."""
        torch = self.torch
        with torch.no_grad():
            keys = [k for k, p in self.params.items() if p.grad is not None]
            ps = [self.params[k] for k in keys]
            gs = [self.params[k].grad for k in keys]
            if self.guarded:
                gs, ok = self._guard(gs, loss)
                first, second = (self.m, self.v) if self.choice == "Adam" else (self.ms, self.mom)
                state = ps + [first[k] for k in keys] + [second[k] for k in keys] + [self.t]
                before = [a.clone() for a in state]
            self.t.add_(1.0)
            if self.choice == "Adam":
                b1, b2, eps = 0.9, 0.999, 1e-8
                lr_t = (self.lr * torch.sqrt(1.0 - torch.pow(self._b2, self.t)) / (1.0 - torch.pow(self._b1, self.t))).to(ps[0].dtype)
                ms = [self.m[k] for k in keys]
                vs = [self.v[k] for k in keys]
                torch._foreach_mul_(ms, b1)
                torch._foreach_add_(ms, gs, alpha=1 - b1)
                torch._foreach_mul_(vs, b2)
                torch._foreach_addcmul_(vs, gs, gs, value=1 - b2)
                den = torch._foreach_sqrt(vs)
                torch._foreach_add_(den, eps)
                upd = torch._foreach_div(ms, den)
                torch._foreach_mul_(upd, lr_t)                     # lr_t is a device scalar tensor: no host sync
                torch._foreach_sub_(ps, upd)
            else:
                decay, eps = 0.9, 1e-10
                rms = [self.ms[k] for k in keys]
                torch._foreach_mul_(rms, decay)
                torch._foreach_addcmul_(rms, gs, gs, value=1 - decay)
                den = torch._foreach_add(rms, eps)
                torch._foreach_sqrt_(den)
                upd = torch._foreach_div(gs, den)                  # momentum = 0: mom = lr * g / sqrt(ms + eps)
                torch._foreach_mul_(upd, self.lr)
                torch._foreach_sub_(ps, upd)
                torch._foreach_copy_([self.mom[k] for k in keys], upd)
            if self.guarded:                                       # a skipped step changes nothing, the counter included
                for a, old in zip(state, before):
                    a.copy_(torch.where(ok, a, old))
            if not self.keep_grads:
                for p in ps:
                    p.grad = None


class AutogradStep(object):
    """The step through torch autograd, behind the interface of ``native_step.FlatTrainStep`` (``alloc``, ``load_batch``, ``run``,
    ``grads``): pure torch without an ``engine``, else with the biGRU recurrences on the HIP kernels.

    A buffer set that the trainer marked ``captured`` runs inside a HIP graph: its dropout draws come from torch's default
    (graph-safe) CUDA generator instead of ``gen``, the gradients stay where the replays rewrite them (``opt.keep_grads``), and the
    loss, which autograd allocates, is also filed in the set's ``loss`` cell, where the device-fed graph's sampler looks for it."""

    def __init__(self, net, opt, engine, keep_prob, gen):
        self.net, self.opt, self.engine, self.gen = net, opt, engine, gen
        self.keep_prob = float(keep_prob)
        self._grads = {}

    def alloc(self, n):
        torch = self.net.torch
        x = torch.zeros((n, 35), dtype=self.net.dtype, device=self.net.device)
        return {"n": n, "x": x, "y": torch.zeros_like(x), "loss": torch.zeros(1, dtype=torch.float32, device=self.net.device)}

    def load_batch(self, b, x, y):
        torch = self.net.torch
        for name, a in (("x", x), ("y", y)):
            b[name].copy_(torch.as_tensor(np.asarray(a), dtype=self.net.dtype).reshape(b[name].shape), non_blocking=True)

    def _clear(self):
        for p in self.net.trainable().values():
            p.grad = None

    def run(self, b, keep_prob=None, masks=None, update=True):
        kp = self.keep_prob if keep_prob is None else keep_prob
        captured = b.get("captured", False)
        if captured:
            self.opt.keep_grads = True
        if not update:
            self._clear()                                   # whatever an earlier step kept would be added to
        loss = self.net.loss(b["x"], b["y"], kp, None if captured else self.gen, self.engine, masks)
        loss.backward()
        if update:
            self.opt.step(loss)
        else:
            self._grads = {k: p.grad for k, p in self.net.trainable().items()}
            self._clear()
        if captured:
            b["loss"].copy_(loss.detach().reshape(1))
        return loss

    def grads(self):
        """{TF name: gradient} of the last update-free step."""
        return self._grads


class Trainer(object):
    """One training step = forward + backward + optimizer update.

    On a GPU at 64 units, 32 channels and a conv stack of 1 .. ``train_mode.TUNED_MAX_BLOCKS`` blocks the step runs entirely on the
    tuned HIP training kernels through the C ABI
    (``catfish_amd/native_step.py``: conv stack, biGRU layers, dense head + loss, optimizer; no autograd), captured ONCE
    into a HIP graph (``torch.cuda.CUDAGraph``) and replayed per batch; batches are copied into static input buffers.
    Dropout masks inside the graph come from torch's default (graph-safe) CUDA generator.  ``native=False`` (and the CPU)
    run the torch-autograd restatement of the same graph -- the reference the native step is tested against.  Every other model
    on a GPU in float32 -- other sizes, 64 / 32 with a deeper stack and, with ``native=True``, 64 units without a conv stack -- trains
    on the any-size kernels: the whole step with ``native=True``, autograd around the recurrences with ``native=None`` (where the
    64-unit RNN type stays on torch).  Which of the four
    paths a trainer takes is one row of the table in ``catfish_amd/train_mode.py`` (``self.mode``); every path is one object
    with ``alloc`` / ``load_batch`` / ``run`` / ``grads`` (``self.step``), run eagerly, captured (``_capture_step``) or captured
    behind the on-card sampler (``_capture_fed``).  ``step_impl`` is that object where the whole step is native, else None.

    ``precision="bf16x3"`` (opt-in; the default "fp32" changes nothing) evaluates the matrix products on the serial chain of the
    any-size biGRU recurrences, forward and backward, as split bf16 products; everything else stays fp32.  It exists where those
    kernels train: on a GPU, in float32, in the two ``anysize_*`` rows of that table.

    ``clip_norm=c`` (opt-in) scales every step's gradients to a global norm of at most ``c`` (``tf.clip_by_global_norm`` in front of
    the reference's ``optimizer.minimize``), and ``skip_nonfinite`` (on with ``clip_norm`` unless switched off; may be switched on
    alone) skips a step whose gradients or loss are not finite: no variable, slot or packed weight changes and ``opt.t`` stays, so
    the next batch meets the same dropout masks.  Both hold in every mode (``TFOptimizer``'s docstring has the definition; the native
    steps run it as HIP kernels inside the captured step) and are orthogonal to ``train_mode``'s table.  ``step_stats()`` reads
    what happened.
    """

    def __init__(self, weights, n_layers, n_layers_res, optimizer_choice, learning_rate, keep_prob, device=None,
                 seed=None, use_graph=None, native=None, optimizer_state=None, dtype=None, loss_log_capacity=4096, precision="fp32",
                 clip_norm=None, skip_nonfinite=None):
        import torch
        from .anysize_train import check_precision
        self.precision = check_precision(precision)
        if int(loss_log_capacity) < 1:
            raise ValueError("loss_log_capacity must be at least 1")
        self.loss_log_capacity = int(loss_log_capacity)      # train_steps: losses kept on the card between two read-backs
        self._fed = None                                     # the device-fed capture (train_steps), next to train_step's
        if device is None:
            if not torch.cuda.is_available():
                # no silent CPU fallback: the torch-CPU mode exists as the reference for tests and is opt-in
                raise RuntimeError("Trainer: no HIP device visible; pass device='cpu' explicitly for the torch reference mode")
            device = "cuda"
        self.net = TorchResNetRNN(weights, n_layers, n_layers_res, device=device, dtype=dtype, precision=self.precision)
        self.opt = TFOptimizer(self.net.trainable(), optimizer_choice, learning_rate, clip_norm=clip_norm, skip_nonfinite=skip_nonfinite)
        self.clip_norm, self.skip_nonfinite = self.opt.clip_norm, self.opt.skip_nonfinite
        if optimizer_state:
            self.opt.load_state_tf(optimizer_state)
        self.keep_prob = float(keep_prob)
        self.gen = torch.Generator(device=self.net.device)
        if seed is not None:
            self.gen.manual_seed(int(seed))
        self.last_loss = None
        # the one decision of which path trains this model: train_mode's table
        h, c, _ = geometry(weights, n_layers_res)
        f32 = self.net.dtype == torch.float32
        mode = TrainMode.of(h, c, n_layers_res, self.net.device.type, f32, native, self.precision, dtype_name=str(self.net.dtype))
        self.mode, self.native, self.anysize = mode.kind, mode.native, mode.anysize
        self.engine = None
        if mode.engine_kwargs is not None:                   # for the autograd kinds only the C-ABI handle their recurrences launch through
            from .engine import HipEngine
            self.engine = HipEngine(weights, n_layers=n_layers, n_layers_res=n_layers_res, device=self.net.device.index or 0,
                                    max_windows_per_pass=256, **mode.engine_kwargs)
        if mode.kind == "anysize_step":
            from .anysize_step import AnySizeTrainStep
            self.step = AnySizeTrainStep(self.net, self.opt, self.engine, self.keep_prob, seed=seed, precision=self.precision)
        elif mode.kind == "tuned_step":
            from .native_step import NativeTrainStep
            self.step = NativeTrainStep(self.net, self.opt, self.engine, self.keep_prob, seed=seed)
        else:
            self.step = AutogradStep(self.net, self.opt, self.engine, self.keep_prob, self.gen)
        self.step_impl = self.step if mode.kind in STEP_KINDS else None      # the native step object, None in the autograd kinds
        self.use_graph = (self.net.device.type == "cuda") if use_graph is None else bool(use_graph)
        self._graph = None                                   # the host-fed capture (train_step) and its buffer set
        self._static = None
        self._eager_bufs = None                              # the buffer set of the steps that run uncaptured
        if seed is not None and self.net.device.type == "cuda":
            torch.cuda.manual_seed(int(seed))

    def _capture_step(self, n, prologue=None, rewind=None):
        """One step at batch ``n`` as a HIP graph -> (graph, its static buffer set).  ``prologue(b)`` is launched in front of the
        step, in the graph and in the warm-ups; ``rewind()`` undoes on the warm-up stream what the warm-up prologues moved.
        No warm-up result is kept: a live autograd loss would pin its gradient-accumulation nodes to the warm-up stream, and the
        captured backward would hop over to it."""
        import torch
        dev = self.net.device
        b = self.step.alloc(n)
        b["captured"] = True
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # warm-up off the capture stream (allocator, lazy init); no update
            for _ in range(2):
                if prologue:
                    prologue(b)
                self.step.run(b, update=False)
            if rewind:
                rewind()
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        # No finaliser may run while the stream captures: a dead cycle that still holds an earlier trainer's graph or engine
        # frees device objects when the cyclic collector reaches it, which a capture in progress does not allow (the process
        # aborts).  torch.cuda.graph collected on entry once and no longer does (torch.compiler.config.force_cudagraph_gc), so
        # collect here, before the capture, and keep the collector off until it ends.
        gc.collect()
        with quiet_gc(), torch.cuda.graph(g):
            if prologue:
                prologue(b)
            b["out"] = self.step.run(b)                     # the loss to read after a replay
        return g, b

    def _bufs(self, x, captured):
        """The buffer set of ``x``'s batch size: the captured step's (captured first, or again at a new size) or the eager one."""
        n = int(np.asarray(x).reshape(-1, 35).shape[0])
        if captured:
            if self._graph is None or self._static["n"] != n:
                self._graph, self._static = self._capture_step(n)
            return self._static
        if self._eager_bufs is None or self._eager_bufs["n"] != n:
            self._eager_bufs = self.step.alloc(n)
        return self._eager_bufs

    def train_step(self, x, y, keep_prob=None, masks=None):
        kp = self.keep_prob if keep_prob is None else keep_prob
        captured = self.use_graph and kp == self.keep_prob and masks is None
        b = self._bufs(x, captured)
        self.step.load_batch(b, x, y)
        if captured:
            self._graph.replay()
            loss = b["out"]
        else:
            loss = self.step.run(b, keep_prob=kp, masks=masks)
        self.last_loss = float(loss.detach())
        return self.last_loss

    # ------------------------------------------------------------------ device-fed loop
    def _capture_fed(self, db, n, ratio):
        """The device-fed step as ONE graph: cf_sample_batch_logged (draw + gather into the static input buffers; its
        one-thread launch then moves the draw counter on and files the previous step's loss in a device log) -> the step.
        Two launches more than the host-fed step.  A second capture next to ``train_step``'s: both work on the same variables,
        optimizer slots and ``opt.t``."""
        import torch
        from . import _native as N
        from ._native import _p
        dev = self.net.device
        lib = N.lib()
        handle = self.engine._handle if self.engine is not None else None
        pos, neg, counter = db.device_pools(dev)
        log = torch.zeros(self.loss_log_capacity, dtype=torch.float32, device=dev)
        log_pos = torch.zeros(1, dtype=torch.int64, device=dev)

        def sample(b):
            # the call's one-thread launch moves the draw counter on and files the PREVIOUS step's loss (still in b["loss"])
            N.check(lib.cf_sample_batch_logged(handle, _p(pos), db.nb_pos, _p(neg), db.nb_neg, n, ratio, db.seed, _p(counter),
                                               _p(b["x"]), _p(b["y"]), _p(b["loss"]), _p(log), self.loss_log_capacity, _p(log_pos),
                                               N.current_stream_ptr(torch, dev)))

        def rewind():                                        # the warm-ups leave no trace in the draw counter or the loss log
            counter.fill_(db.draw)
            db._dev_draw = db.draw
            log_pos.zero_()

        g, b = self._capture_step(n, sample, rewind)
        self._fed = {"key": (n, ratio), "db": db, "graph": g, "x": b["x"], "y": b["y"], "loss": b["loss"], "log": log, "log_pos": log_pos,
                     "pools": (pos, neg, counter)}

    def train_steps(self, db, n_steps, batch_size, ratio=2):
        """``n_steps`` optimizer steps on consecutive draws of a ``device_db.DeviceExampleDb`` -> float32 [n_steps] losses.

        On a GPU with graphs the example pools live on the card and every step is one replay of the device-fed graph
        (``_capture_fed``): no copy, no read-back and no synchronise between steps; the losses collect in a device log that is
        read back once per chunk of ``loss_log_capacity`` steps.  The CPU reference mode, ``use_graph=False`` and a database
        that keeps nothing on the card (``device_db.DeviceReadDb``) run ``db.get_training_set`` + ``train_step`` per step, on the
        same batches."""
        n_steps, n, ratio = int(n_steps), int(batch_size), int(ratio)
        out = np.zeros(max(n_steps, 0), dtype=np.float32)
        if n_steps <= 0:
            return out
        import torch
        on_card = hasattr(db, "device_pools")               # a database without a card side (DeviceReadDb) is fed by the host
        if not (on_card and self.use_graph and self.net.device.type == "cuda" and self.net.dtype == torch.float32):
            for i in range(n_steps):
                x, y, _ = db.get_training_set(n, ratio)
                out[i] = self.train_step(np.asarray(x, dtype=np.float32).reshape(n, 35), np.asarray(y, dtype=np.float32).reshape(n, 35))
            return out
        db.batch_indices(db.draw, n, ratio)                  # a pool smaller than its share: ValueError, before anything is enqueued
        f = self._fed
        if f is None or f["key"] != (n, ratio) or f["db"] is not db or f["pools"][0] is not db.device_pools(self.net.device)[0]:
            self._capture_fed(db, n, ratio)
            f = self._fed
        done = 0
        while done < n_steps:
            k = min(self.loss_log_capacity, n_steps - done)
            db.sync_counter()
            f["log_pos"].zero_()
            for _ in range(k):
                f["graph"].replay()
            db.device_drew(k, f["x"], f["y"], n)
            # losses 0 .. k-2 were filed by the following replays' samplers, the last one is still in the step's loss buffer
            out[done:done + k] = torch.cat([f["log"][:k - 1], f["loss"]]).cpu().numpy()     # the chunk's one synchronise
            done += k
        self.last_loss = float(out[-1])
        return out

    def step_stats(self):
        """{"grad_norm": g of the last step, "scale": the factor applied to its gradients (-1.0: the step was skipped),
        "clipped": steps clipped so far, "skipped": steps skipped so far}; all zero until a step with ``clip_norm`` or
        ``skip_nonfinite`` has run.  One synchronise: for the caller between chunks, never inside the loop."""
        g, scale, clipped, skipped = self.opt.stats.cpu().tolist()
        return {"grad_norm": g, "scale": scale, "clipped": int(clipped), "skipped": int(skipped)}

    def gradients(self, x, y, keep_prob=None, masks=None):
        """Loss and gradients of one batch WITHOUT an update: (loss, {TF name: ndarray}) -- what tests compare with the
        reference graph's gradient tensors."""
        kp = self.keep_prob if keep_prob is None else keep_prob
        b = self._bufs(x, False)
        self.step.load_batch(b, x, y)
        loss = float(self.step.run(b, keep_prob=kp, masks=masks, update=False).detach())
        return loss, {k: v.detach().cpu().numpy().copy() for k, v in self.step.grads().items()}
