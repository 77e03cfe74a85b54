"""``torch.ops.catfish.resnetrnn_forward(x, packed_weights) -> Tensor`` -- the one call this library replaces,

    confidences = self.sess.run(self.predictions, feed_dict={self.x: input_x, self.p_dropout: 1.0})
                                                                  (reference catfish/models/rnn_class.py:214-216)

registered as a PyTorch operator (SURVEY.md section 8b sketches exactly this name), for callers that live in torch: device tensor
in, device tensor out, asynchronous on PyTorch's current HIP stream, no host round trip.  It is a thin door to the same C ABI as
everything else (``cf_infer`` through ``HipEngine.infer_device``): there is NO CPU implementation -- a CPU tensor is refused, and
without the built library the call raises ``NativeLibraryMissing``.

``packed_weights``: ONE flat float32 CPU tensor made by ``pack_weights(weights, ...)`` -- a 8-value header
``[magic, n_layers, layer_size, n_layers_res, layer_size_res, n_tensors, 0, 0]`` followed by the checkpoint's inference tensors in
the fixed order of ``tensor_names`` (TF variable names, TF layouts), i.e. what ``checkpoint.read_inference_weights`` returns, flattened.
The engine built from it (BN folded, matrices re-tiled into MFMA fragment order, uploaded) is cached per (tensor storage, version,
device): the second call with the same tensor only launches.

The op is differentiable once, with respect to ``x`` and ``packed_weights`` (every tensor, the BN moving statistics included): its
autograd formula (``op_grad``) re-runs the training forward of the engine's geometry on the HIP kernels and walks it backwards.  The
``x`` gradient stays on the device, asynchronous; the ``packed_weights`` gradient is a float32 CPU tensor like ``packed_weights``
(header zero) and costs one device-to-host copy.  INTEGRATION.md, "The call as a PyTorch operator", has examples.

    import torch, catfish_amd.torch_ops as ops
    packed = ops.pack_weights(weights)                       # once
    probs = torch.ops.catfish.resnetrnn_forward(x, packed)   # x: float32 [N, 35] or [N, 35, 1] on an MI355X -> float32 [N * 35]

``torch.ops.catfish.resnetrnn_forward_params(x, params, n_layers, layer_size, n_layers_res, layer_size_res)`` is the same function
with the weights on the DEVICE: ``params`` is the flat float32 CUDA tensor ``packed[HEADER:]`` (``param_count(...)`` values), e.g. an
``nn.Parameter`` (``torch_module.CatfishModule``).  Its engine is cached per (device, geometry), not per content: every call folds
and re-tiles ``params`` into that engine on the device (``HipEngine.load_params_device``) and then infers, both on the current
stream, so a weight update never builds an engine and a training step through it can be captured in a CUDA graph.  Its gradient
with respect to ``params`` is a CUDA tensor (no host copy).  Threading: one engine serves every caller of a geometry on a device,
so calls from two streams on the same geometry must be ordered by the caller (the C ABI's one model per device per host thread).
"""
from __future__ import annotations

import functools

import numpy as np

from . import _native as N

MAGIC = 35064.0          # "catfish 35-sample windows, 64 units": any float32-exact constant would do
HEADER = 8
OP_NAME = "catfish::resnetrnn_forward"
OP_PARAMS_NAME = "catfish::resnetrnn_forward_params"


def tensor_names(n_layers=3, n_layers_res=2):
    """The inference tensors of a checkpoint in the operator's packing order (TF variable names)."""
    names = []
    for j in range(4 * n_layers_res):
        names += [N.conv_name(j) + "/kernel", N.conv_name(j) + "/bias"]
        names += [N.bn_name(j) + "/" + v for v in ("gamma", "beta", "moving_mean", "moving_variance")]
    for layer in range(n_layers):
        for d in ("fw", "bw"):
            p = N.gru_prefix(layer, d)
            names += [p + "/gates/kernel", p + "/gates/bias", p + "/candidate/kernel", p + "/candidate/bias"]
    names += ["final_fully_connected/kernel", "final_fully_connected/bias"]
    return names


def _shapes(n_layers, layer_size, n_layers_res, layer_size_res):
    """name -> shape for a geometry (resnet_class.py:44-82, rnn_class.py:142-183): needed to cut the flat tensor apart again."""
    shapes = {}
    for j in range(4 * n_layers_res):
        block, which = divmod(j, 4)
        cin = 1 if (block == 0 and which in (0, 1)) else layer_size_res          # shortcut and first conv of block 0 see the signal
        ksize = 3 if which == 2 else 1
        shapes[N.conv_name(j) + "/kernel"] = (ksize, cin, layer_size_res)
        shapes[N.conv_name(j) + "/bias"] = (layer_size_res,)
        for v in ("gamma", "beta", "moving_mean", "moving_variance"):
            shapes[N.bn_name(j) + "/" + v] = (layer_size_res,)
    feat = layer_size_res if n_layers_res else 1
    for layer in range(n_layers):
        cin = feat if layer == 0 else 2 * layer_size
        for d in ("fw", "bw"):
            p = N.gru_prefix(layer, d)
            shapes[p + "/gates/kernel"] = (cin + layer_size, 2 * layer_size)
            shapes[p + "/gates/bias"] = (2 * layer_size,)
            shapes[p + "/candidate/kernel"] = (cin + layer_size, layer_size)
            shapes[p + "/candidate/bias"] = (layer_size,)
    shapes["final_fully_connected/kernel"] = (2 * layer_size, 1)
    shapes["final_fully_connected/bias"] = (1,)
    return shapes


def pack_weights(weights, n_layers=3, layer_size=64, n_layers_res=2, layer_size_res=32):
    """dict {TF variable name: array} -> the operator's flat float32 CPU tensor (header + tensors in ``tensor_names`` order).
    A missing tensor or one of another shape raises ValueError naming it."""
    import torch
    names = tensor_names(n_layers, n_layers_res)
    shapes = _shapes(n_layers, layer_size, n_layers_res, layer_size_res)
    parts = [np.array([MAGIC, n_layers, layer_size, n_layers_res, layer_size_res, len(names), 0, 0], dtype=np.float32)]
    for name in names:
        if name not in weights:
            raise ValueError("checkpoint is missing tensor %r" % name)
        arr = np.asarray(weights[name], dtype=np.float32)
        if tuple(arr.shape) != shapes[name]:
            raise ValueError("tensor %r has shape %s, the geometry needs %s" % (name, tuple(arr.shape), shapes[name]))
        parts.append(arr.reshape(-1))
    return torch.from_numpy(np.concatenate(parts))


@functools.lru_cache(maxsize=64)
def param_count(n_layers=3, layer_size=64, n_layers_res=2, layer_size_res=32):
    """Values of the flat parameter tensor of ``resnetrnn_forward_params`` for a geometry: ``pack_weights(...).numel() - HEADER``."""
    shapes = _shapes(n_layers, layer_size, n_layers_res, layer_size_res)
    return sum(int(np.prod(shapes[name])) for name in tensor_names(n_layers, n_layers_res))


def _check_packed(packed):
    import torch
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.float32 or packed.dim() != 1 or packed.is_cuda:
        raise ValueError("packed_weights must be the flat float32 CPU tensor pack_weights() returns")


def unpack_weights(packed):
    """The inverse: flat tensor -> (dict of arrays, dict(n_layers, layer_size, n_layers_res, layer_size_res)); ValueError when the
    tensor is not one ``pack_weights`` made (dtype, device, magic, length)."""
    _check_packed(packed)
    flat = packed.detach().contiguous().numpy()
    if flat.shape[0] < HEADER or flat[0] != MAGIC:
        raise ValueError("packed_weights does not start with the catfish header")
    geom = dict(n_layers=int(flat[1]), layer_size=int(flat[2]), n_layers_res=int(flat[3]), layer_size_res=int(flat[4]))
    names = tensor_names(geom["n_layers"], geom["n_layers_res"])
    shapes = _shapes(**geom)
    if int(flat[5]) != len(names) or flat.shape[0] != HEADER + sum(int(np.prod(shapes[n])) for n in names):
        raise ValueError("packed_weights has %d values, its header describes %d tensors / %d values" % (
            flat.shape[0], len(names), HEADER + sum(int(np.prod(shapes[n])) for n in names)))
    out, pos = {}, HEADER
    for name in names:
        n = int(np.prod(shapes[name]))
        out[name] = flat[pos:pos + n].reshape(shapes[name])
        pos += n
    return out, geom


_ENGINES = {}            # (sha1 of the packed bytes, numel, device index) -> HipEngine; insertion order = age
_SEEN = {}               # id(tensor object) -> (weak reference to it, its version when hashed, (sha1, numel))
MAX_CACHED = 8


def _content_key(packed, device_index):
    """What identifies the weights is their CONTENT: an address says nothing (the allocator hands a freed packed tensor's block to
    the next one of the same size, version 0 again -- ADVICE r05: 9 of 10 trials), so the engines are keyed on a digest of the
    packed bytes (0.8 MB: under a millisecond).  The digest is taken once per tensor OBJECT and version: while the caller keeps
    passing the same live tensor, unmodified as far as torch's version counter sees, the look-up costs two dict reads."""
    import hashlib
    import weakref
    _check_packed(packed)                                     # (before anything is hashed: a CUDA or float64 tensor is a ValueError, as ever)
    seen = _SEEN.get(id(packed))
    if seen is not None and seen[0]() is packed and seen[1] == packed._version:
        return seen[2] + (int(device_index),)
    flat = packed.detach().contiguous().numpy()
    digest = (hashlib.sha1(memoryview(flat).cast("B")).digest(), int(flat.shape[0]))
    ident = id(packed)
    try:
        ref = weakref.ref(packed, lambda _r, ident=ident: _SEEN.pop(ident, None))      # the id may be reused once the object is gone
        _SEEN[ident] = (ref, packed._version, digest)
    except TypeError:                                          # an object that cannot be weakly referenced: hash it every time
        pass
    return digest + (int(device_index),)


def _engine_for(packed, device_index):
    from .engine import HipEngine
    key = _content_key(packed, device_index)
    eng = _ENGINES.get(key)
    if eng is None:
        weights, geom = unpack_weights(packed)
        eng = HipEngine(weights, device=int(device_index), **geom)
        eng.op_grad = None                                     # backward state (op_grad.OpGrad), built by the first backward
        if len(_ENGINES) >= MAX_CACHED:                       # oldest out: an engine holds device workspace
            _retire(_ENGINES.pop(next(iter(_ENGINES))))
        _ENGINES[key] = eng
    return eng


def _retire(eng):
    eng.op_grad = None                                         # device parameters, GRU packs and slab buffers of the backward
    eng.close()


def clear_engine_cache():
    """Free the engines (device weights + workspace, and the backward's state) the operator built so far."""
    _SEEN.clear()
    while _ENGINES:
        _retire(_ENGINES.popitem()[1])


_PARAM_ENGINES = {}      # (device index, n_layers, layer_size, n_layers_res, layer_size_res) -> HipEngine of resnetrnn_forward_params


def _placeholder_weights(n_layers, layer_size, n_layers_res, layer_size_res):
    """Zeros with unit moving variance: what the first engine of a geometry is created from before its first load."""
    shapes = _shapes(n_layers, layer_size, n_layers_res, layer_size_res)
    return {name: (np.ones if name.endswith("moving_variance") else np.zeros)(shapes[name], np.float32)
            for name in tensor_names(n_layers, n_layers_res)}


def _params_engine(device_index, geo):
    from .engine import HipEngine
    key = (int(device_index),) + tuple(geo)
    eng = _PARAM_ENGINES.get(key)
    if eng is None:
        n_layers, layer_size, n_layers_res, layer_size_res = geo
        eng = HipEngine(_placeholder_weights(*geo), device=int(device_index), n_layers=n_layers, layer_size=layer_size,
                        n_layers_res=n_layers_res, layer_size_res=layer_size_res)
        eng.op_grad = None
        _PARAM_ENGINES[key] = eng
    return eng


def _check_params(x, params, geo):
    """ValueError unless ``params`` is a contiguous float32 CUDA tensor on ``x``'s device with ``param_count(*geo)`` values."""
    import torch
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or not params.is_cuda:
        raise ValueError("params must be a float32 CUDA tensor (the flat parameters, packed_weights without its header)")
    if params.device != x.device:
        raise ValueError("params live on %s, x on %s" % (params.device, x.device))
    n = param_count(*geo)
    if not params.is_contiguous() or int(params.numel()) != n:
        raise ValueError("params must be a contiguous tensor of %d values for this geometry, got %d" % (n, params.numel()))


def clear_params_engine_cache():
    """Free the engines of ``resnetrnn_forward_params`` (and their backward state).  A CUDA graph captured through the operator
    points at them: drop such graphs first."""
    while _PARAM_ENGINES:
        _retire(_PARAM_ENGINES.popitem()[1])


def _backward_params_impl(x, params, grad, need_x, need_w, geo):
    """(d x, d params) of ``resnetrnn_forward_params``: ``op_grad`` over the engine of the geometry, its parameters set from
    ``params`` on the device; d params is a fresh CUDA tensor shaped like ``params``."""
    from .op_grad import OpGrad
    eng = _params_engine(x.device.index, geo)
    if eng.op_grad is None:
        eng.op_grad = OpGrad(eng, keep_buffers=True)
    eng.op_grad.set_params(params.detach())
    gx, gw = eng.op_grad.backward(x, grad, need_x, need_w, device_grad=True)
    return gx, (gw.view(params.shape) if gw is not None else None)


def _backward_impl(x, packed, grad, need_x, need_w):
    """(d x, d packed_weights) of the operator for the upstream gradient ``grad`` [N * 35] (``op_grad``)."""
    from .op_grad import OpGrad
    eng = _engine_for(packed, x.device.index)
    if eng.op_grad is None:
        eng.op_grad = OpGrad(eng, packed, HEADER)
    return eng.op_grad.backward(x, grad, need_x, need_w)


def _register():
    import torch

    @torch.library.custom_op(OP_NAME, mutates_args=(), schema="(Tensor x, Tensor packed_weights) -> Tensor")
    def resnetrnn_forward(x, packed_weights):
        # the C ABI behind it has no CPU path: a CPU tensor is an error, not a slow answer
        if not x.is_cuda:
            raise ValueError("catfish::resnetrnn_forward runs on an MI355X only: x must be a float32 CUDA tensor [N, 35(, 1)]")
        eng = _engine_for(packed_weights, x.device.index)
        return eng.infer_device(x)                            # asynchronous on torch.cuda.current_stream(x.device)

    @resnetrnn_forward.register_fake
    def _(x, packed_weights):
        n = x.shape[0]
        return x.new_empty((n * N.CF_WINDOW,), dtype=torch.float32)

    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(*inputs)                        # recompute, don't stash: torch catches an in-place edit of either

    def backward(ctx, grad):
        x, packed = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        gx, gw = _backward_impl(x, packed, grad, need_x, need_w)
        if torch.is_grad_enabled():                           # create_graph=True: the gradients are not differentiable again
            grads = [t.detach().requires_grad_(True) if t is not None else None for t in (gx, gw)]
            live = [t for t in grads if t is not None]
            err = torch._C._functions.DelayedError(b"catfish::resnetrnn_forward is once-differentiable: its backward has no "
                                                   b"autograd formula (double backward is not supported)", len(live) + 2)
            out = iter(err(*live, x, packed))                     # x, packed: the error node is reached from the op's inputs
            gx, gw = (next(out) if t is not None else None for t in grads)
        return gx, gw

    torch.library.register_autograd(OP_NAME, backward, setup_context=setup_context)
    return resnetrnn_forward


def _once_differentiable(torch, name, grads, inputs):
    """create_graph=True: the gradients come back through an error node, so that differentiating them again raises."""
    live = [t.detach().requires_grad_(True) for t in grads if t is not None]
    err = torch._C._functions.DelayedError(("%s is once-differentiable: its backward has no autograd formula (double backward is "
                                            "not supported)" % name).encode(), len(live) + len(inputs))
    out = iter(err(*(live + list(inputs))))
    return [next(out) if t is not None else None for t in grads]


def _register_params():
    import torch

    @torch.library.custom_op(OP_PARAMS_NAME, mutates_args=(), schema="(Tensor x, Tensor params, int n_layers, int layer_size, "
                                                                      "int n_layers_res, int layer_size_res) -> Tensor")
    def resnetrnn_forward_params(x, params, n_layers, layer_size, n_layers_res, layer_size_res):
        if not x.is_cuda:
            raise ValueError("catfish::resnetrnn_forward_params runs on an MI355X only: x must be a float32 CUDA tensor [N, 35(, 1)]")
        geo = (int(n_layers), int(layer_size), int(n_layers_res), int(layer_size_res))
        _check_params(x, params, geo)
        eng = _params_engine(x.device.index, geo)
        eng.load_params_device(params.reshape(-1))            # both on torch.cuda.current_stream(x.device)
        return eng.infer_device(x)

    @resnetrnn_forward_params.register_fake
    def _(x, params, n_layers, layer_size, n_layers_res, layer_size_res):
        return x.new_empty((x.shape[0] * N.CF_WINDOW,), dtype=torch.float32)

    def setup_context(ctx, inputs, output):
        x, params = inputs[:2]
        ctx.save_for_backward(x, params)
        ctx.geo = tuple(int(v) for v in inputs[2:])

    def backward(ctx, grad):
        x, params = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        gx, gw = _backward_params_impl(x, params, grad, need_x, need_w, ctx.geo)
        if torch.is_grad_enabled():
            gx, gw = _once_differentiable(torch, OP_PARAMS_NAME, [gx, gw], [x, params])
        return gx, gw, None, None, None, None

    torch.library.register_autograd(OP_PARAMS_NAME, backward, setup_context=setup_context)
    return resnetrnn_forward_params


resnetrnn_forward = _register()
resnetrnn_forward_params = _register_params()
