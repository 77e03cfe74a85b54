"""``CatfishModule``: the model as a ``torch.nn.Module`` with ONE flat trainable ``nn.Parameter``.

``params`` holds the checkpoint's inference tensors in the operator's order (``torch_ops.tensor_names``, TF layouts, flattened:
``pack_weights(...)`` without its header), so ``forward`` is one call of ``torch.ops.catfish.resnetrnn_forward_params`` and a
torch optimizer updates the weights in place on the device.  Every computation goes through that operator; this class only
holds the parameter and the geometry and converts between the flat tensor and ``{TF name: array}`` dicts.

    import torch
    from catfish_amd.torch_module import CatfishModule
    model = CatfishModule.from_weights(weights, device="cuda")     # weights: checkpoint.read_inference_weights(...)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    loss = torch.nn.functional.binary_cross_entropy(model(x), y)  # x: float32 [N, 35(, 1)] CUDA, y: [N * 35]
    loss.backward(); opt.step()
    net.set_weights(model.weights())                               # back into an RNN / ResNetRNN (or the checkpoint writer)
"""
from __future__ import annotations

import numpy as np
import torch

from . import torch_ops as ops


class CatfishModule(torch.nn.Module):
    def __init__(self, params, n_layers=3, layer_size=64, n_layers_res=2, layer_size_res=32):
        """``params``: the flat float32 parameters (``torch_ops.param_count(...)`` values), on any device."""
        super().__init__()
        self.n_layers, self.layer_size = int(n_layers), int(layer_size)
        self.n_layers_res, self.layer_size_res = int(n_layers_res), int(layer_size_res)
        n = ops.param_count(*self.geometry)
        params = torch.as_tensor(params)
        if params.dtype != torch.float32 or params.numel() != n:
            raise ValueError("params must be float32 with %d values for this geometry, got %s with %d" % (n, params.dtype, params.numel()))
        self.params = torch.nn.Parameter(params.detach().reshape(-1).clone())
        shapes = ops._shapes(*self.geometry)
        self._slices, off = {}, 0
        for name in ops.tensor_names(self.n_layers, self.n_layers_res):
            size = int(np.prod(shapes[name]))
            self._slices[name] = (off, size, tuple(shapes[name]))
            off += size

    @property
    def geometry(self):
        """(n_layers, layer_size, n_layers_res, layer_size_res): the operator's trailing arguments."""
        return (self.n_layers, self.layer_size, self.n_layers_res, self.layer_size_res)

    @classmethod
    def from_weights(cls, weights, n_layers=3, layer_size=64, n_layers_res=2, layer_size_res=32, device=None):
        """From a ``{TF variable name: array}`` dict such as ``checkpoint.read_inference_weights`` returns (ValueError naming a
        missing tensor or one of the wrong shape)."""
        flat = ops.pack_weights(weights, n_layers, layer_size, n_layers_res, layer_size_res)[ops.HEADER:]
        return cls(flat if device is None else flat.to(device), n_layers, layer_size, n_layers_res, layer_size_res)

    @classmethod
    def from_network(cls, net, device=None):
        """From an ``RNN`` / ``ResNetRNN`` of ``neural_network.load_network``: its current weights and geometry."""
        if net.weights is None:
            raise RuntimeError("network has no weights: call restore_network() or initialize_network() first")
        trainer = getattr(net, "_trainer", None)
        weights = trainer.net.numpy_weights() if trainer is not None else net.weights
        return cls.from_weights(weights, net.n_layers, net.layer_size, net.n_layers_res_, net.layer_size_res_, device=device)

    def tensor(self, name):
        """A view of ``params`` under a TF variable name, in its TF shape (shares storage: writes reach the parameter)."""
        if name not in self._slices:
            raise KeyError("no tensor %r in this geometry" % name)
        off, size, shape = self._slices[name]
        return self.params.narrow(0, off, size).view(shape)

    def weights(self):
        """``{TF variable name: float32 numpy array}`` of the current parameters (accepted by ``RNN.set_weights`` and the
        checkpoint writer)."""
        flat = self.params.detach().cpu().numpy()
        return {name: flat[off:off + size].reshape(shape).copy() for name, (off, size, shape) in self._slices.items()}

    def forward(self, x):
        """float32 CUDA [N, 35(, 1)] -> probabilities float32 [N * 35] (``resnetrnn_forward_params``)."""
        return torch.ops.catfish.resnetrnn_forward_params(x, self.params, *self.geometry)

    def extra_repr(self):
        return "n_layers=%d, layer_size=%d, n_layers_res=%d, layer_size_res=%d" % self.geometry
