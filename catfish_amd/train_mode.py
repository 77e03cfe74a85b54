"""Which training path a ``training.Trainer`` takes, decided once, on the host: ints, strings and bools only (no torch, no library).

``geometry(weights, n_layers_res)`` reads the two sizes; ``TrainMode.of`` maps them and the trainer's arguments to one row:

    geometry   device  dtype    native      type       kind              engine keywords          step class        fed by card  captured
    ---------  ------  -------  ----------  ---------  ----------------  -----------------------  ----------------  -----------  --------
    tuned      cuda    float32  None, True  ResNetRNN  tuned_step        fuse_layers=False        NativeTrainStep   yes          yes
    other      cuda    float32  True        either     anysize_step      layer_size, .._size_res  AnySizeTrainStep  yes          yes
    other      cuda    float32  None        either *   anysize_autograd  layer_size, .._size_res  AutogradStep      yes          yes
    everything else (the CPU, native=False, ...)       torch             no engine                AutogradStep      cuda float32 cuda

"ResNetRNN" is a model with a conv stack (``n_layers_res > 0``), "RNN" one without; an RNN's ``c`` counts as 32.  "tuned" is what
the tuned training kernels take (``tuned_geometry``): 64 GRU units, 32 conv channels and a conv stack of 1 .. ``TUNED_MAX_BLOCKS``
blocks.  "other" is every other model, so also 64 units without a conv stack and 64 / 32 with a deeper stack: the tuned biGRU
kernels take inputs of 32 or 128 features, not the RNN type's single one, and the tuned conv-stack kernels have no stack of five
blocks.  (*) One exception is recorded behaviour: a 64-unit RNN with ``native=None`` trains on ``torch``; only ``native=True`` moves
it to ``anysize_step``.  A tuned geometry that is not float32 trains on ``torch`` as well.
"fed by card" is ``Trainer.train_steps`` replaying the device-fed graph, "captured" is ``use_graph``.
``native`` is True in the rows of ``tuned_step`` and ``anysize_step``; ``anysize`` is True in the ``anysize_autograd`` row only.

``precision="bf16x3"`` exists in the two ``anysize_*`` rows.  Elsewhere it is refused, and so is ``native=True`` off the GPU or off
float32, with one ``ValueError`` each, in the order of ``TrainMode.of``'s body.  At 64 / 32 with at most ``TUNED_MAX_BLOCKS`` blocks
(the 64-unit RNN included) the refusal is the tuned kernels', whatever else is wrong with the request.
"""
from __future__ import annotations

from collections import namedtuple

KINDS = ("tuned_step", "anysize_step", "anysize_autograd", "torch")
STEP_KINDS = KINDS[:2]                                       # the whole step on the HIP kernels, no autograd
TUNED_MAX_BLOCKS = 4                                         # the deepest conv stack of the tuned training kernels (cf_res_train_param_floats)


def geometry(weights, n_layers_res):
    """(GRU units, conv channels, is it the shipped 64 / 32) of a {TF name: array or tensor}; without a conv stack ``c`` counts as 32."""
    h = len(weights["stack_bidirectional_rnn/cell_0/bidirectional_rnn/fw/gru_cell/candidate/bias"])
    c = len(weights["conv1d/bias"]) if n_layers_res > 0 else 32
    return h, c, (h == 64 and c == 32)


def tuned_geometry(h, c, n_layers_res):
    """Do the tuned training kernels take this model: 64 units, 32 channels, a conv stack of 1 .. ``TUNED_MAX_BLOCKS`` blocks."""
    return h == 64 and c == 32 and 1 <= n_layers_res <= TUNED_MAX_BLOCKS


class TrainMode(namedtuple("TrainMode", "kind engine_kwargs native anysize")):
    """One row of the module's table.  ``engine_kwargs``: None = no engine, else the keywords that size the trainer's ``HipEngine``."""
    __slots__ = ()

    @classmethod
    def of(cls, h, c, n_layers_res, device_type, float32, native, precision, dtype_name=""):
        """``h``, ``c`` as ``geometry`` gives them; ``float32``: the variables' dtype is; ``native``: None | bool as passed to the
        trainer; ``dtype_name`` only words the dtype refusal."""
        cuda = device_type == "cuda"
        tuned = tuned_geometry(h, c, n_layers_res)
        rnn64 = h == 64 and n_layers_res <= 0                    # trains on the any-size step when asked to, else as it always did
        other = not (tuned or rnn64) or (rnn64 and bool(native) and cuda and float32)
        if precision == "bf16x3":
            why = ("the tuned training kernels of the shipped 64 / 32 geometry are fp32" if not other else
                   "it runs on the HIP kernels: device='cpu' has none" if not cuda else
                   "native=False is the pure-torch reference" if native is not None and not native else
                   "the training kernels are float32 (dtype %s)" % dtype_name if not float32 else None)
            if why:
                raise ValueError("precision='bf16x3' is a mode of the any-size training recurrences; %s" % why)
        if native and not (cuda and float32):
            raise ValueError("native=True runs the fp32 HIP training kernels: it needs device='cuda' and dtype float32")
        sizes = dict(layer_size=h, layer_size_res=c)
        if native and other:
            return cls("anysize_step", sizes, True, False)
        if native is None and cuda and float32 and other:
            return cls("anysize_autograd", sizes, False, True)
        if tuned and cuda and float32 and (native or native is None):
            return cls("tuned_step", dict(fuse_layers=False), True, False)
        return cls("torch", None, False, False)
