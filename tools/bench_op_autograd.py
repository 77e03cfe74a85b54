"""Autograd through ``torch.ops.catfish.resnetrnn_forward`` (catfish_amd/op_grad.py): forward alone, forward + backward for ``x``
only, forward + backward for ``x`` and ``packed_weights``, and beside them forward + backward through the eager restatement
``TorchResNetRNN`` (float32, same GPU, every tensor requiring grad, the moving statistics included) for the same loss
(sigmoid(logits) . g).sum().  Device events, warm-up, the variants alternating in one process, median of the rounds; one JSON line
per geometry and window count.

    python tools/bench_op_autograd.py             # shipped checkpoint, 128 / 64, 256 / 128, plain RNN 128 units; 256 and 4096 windows
    python tools/bench_op_autograd.py --profile   # only the shipped geometry at 4096 windows, no restatement (for rocprofv3)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import catfish_amd.torch_ops as ops  # noqa: E402
from catfish_amd.training import TorchResNetRNN  # noqa: E402
from oracle import catfish_oracle as oracle  # noqa: E402

GEOMETRIES = [("checkpoint", 64, 32, 3, 2), ("random", 128, 64, 3, 2), ("random", 256, 128, 2, 1), ("random", 128, 32, 2, 0)]
ROUNDS = 3


def device_ms(fn, iters):
    """Mean device milliseconds per call of ``fn`` between two events on the current stream, after one warm-up call."""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def variants(packed, x, g, w, geo, with_torch):
    op = torch.ops.catfish.resnetrnn_forward
    xg = x.clone().requires_grad_(True)
    pw = packed.clone().requires_grad_(True)

    def forward():
        with torch.no_grad():
            op(x, packed)

    def backward_x():
        xg.grad = None
        (op(xg, packed) * g).sum().backward()

    def backward_xw():
        xg.grad, pw.grad = None, None
        (op(xg, pw) * g).sum().backward()

    out = {"forward_ms": forward, "fwd_bwd_x_ms": backward_x, "fwd_bwd_x_weights_ms": backward_xw}
    if with_torch:
        _, h, c, nl, nr = geo
        net = TorchResNetRNN(w, nl, nr, device="cuda", dtype=torch.float32)
        for t in net.params.values():
            t.requires_grad_(True)

        def restatement():
            for t in net.params.values():
                t.grad = None
            xg.grad = None
            (torch.sigmoid(net.logits(xg)).reshape(-1) * g).sum().backward()

        out["torch_restatement_fwd_bwd_ms"] = restatement
    return out


def main():
    profile = "--profile" in sys.argv
    rng = np.random.default_rng(0)
    geos = GEOMETRIES[:1] if profile else GEOMETRIES
    for geo in geos:
        kind, h, c, nl, nr = geo
        if kind == "checkpoint":
            with np.load(os.path.join(ROOT, "tests", "golden", "ckpnt-30000-inference.npz")) as z:
                w = {k: z[k] for k in z.files}
        else:
            w = oracle.random_weights(seed=3, layer_size=h, n_layers=nl, layer_size_res=c, n_layers_res=nr)
        packed = ops.pack_weights(w, nl, h, nr, c)
        for n in ((4096,) if profile else (256, 4096)):
            x = torch.tensor(rng.normal(0, 1, size=(n, 35)).astype(np.float32), device="cuda")
            g = torch.tensor(rng.normal(0, 1, size=n * 35).astype(np.float32), device="cuda")
            fns = variants(packed, x, g, w, geo, with_torch=not profile)
            times = {k: [] for k in fns}
            for _ in range(1 if profile else ROUNDS):
                for k, fn in fns.items():                 # alternate, so that clock and neighbour drift hit every variant alike
                    times[k].append(device_ms(fn, 5 if profile or k.startswith("torch") else 10))
            res = dict(weights=kind, layer_size=h, layer_size_res=c if nr else 0, n_layers=nl, n_layers_res=nr, windows=n)
            res.update({k: float(np.median(v)) for k, v in times.items()})
            print(json.dumps(res), flush=True)
        ops.clear_engine_cache()


if __name__ == "__main__":
    main()
