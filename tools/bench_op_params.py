"""Device-resident weights through ``torch.ops.catfish.resnetrnn_forward_params`` (``CatfishModule``) against the packed operator.

Per geometry and window count, ms per SGD step (forward + backward of x and the weights + ``torch.optim.SGD`` step, BCE loss):
    packed_cpu_step_ms   resnetrnn_forward with a CPU leaf ``packed``: every step builds a new engine (digest, folding, upload,
                         workspace) and copies the weight gradient to the host
    params_eager_step_ms resnetrnn_forward_params eagerly: one engine, a device load per call, gradients on the device
    params_graph_step_ms the same step captured once as a CUDA graph and replayed
At 256 windows also forward alone (no grad): the packed operator with a cached engine vs the params operator (the difference is
what a load costs per call), and per geometry the time of ``cf_model_load_params`` alone.  Device events on the current stream,
warm-up, variants alternating in one process, median of the rounds; one JSON line each.

    python tools/bench_op_params.py [--out FILE]   # 64/32 3+2 at 256 and 4096 windows, 128/64 3+2 and 256/128 2+1 at 256
    python tools/bench_op_params.py --profile      # 64/32 at 256 windows: params steps and loads only (for rocprofv3)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import catfish_amd.torch_ops as ops  # noqa: E402
from catfish_amd.torch_module import CatfishModule  # noqa: E402
from oracle import catfish_oracle as oracle  # noqa: E402

CONFIGS = [("checkpoint", 64, 32, 3, 2, 256), ("checkpoint", 64, 32, 3, 2, 4096), ("random", 128, 64, 3, 2, 256),
           ("random", 256, 128, 2, 1, 256)]
ROUNDS = 3
LR = 1e-3


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


def bce(probs, y):
    return torch.nn.functional.binary_cross_entropy(probs.clamp(1e-6, 1 - 1e-6), y)


def step_variants(w, geo, x, y, profile):
    op_geo = (geo[2], geo[0], geo[3], geo[1])                     # n_layers, layer_size, n_layers_res, layer_size_res
    fns = {}
    if not profile:
        packed = ops.pack_weights(w, *op_geo).requires_grad_(True)
        opt_a = torch.optim.SGD([packed], lr=LR)

        def packed_step():
            opt_a.zero_grad(set_to_none=True)
            x.grad = None
            bce(torch.ops.catfish.resnetrnn_forward(x, packed), y).backward()
            opt_a.step()
        fns["packed_cpu_step_ms"] = packed_step
    m_b = CatfishModule.from_weights(w, *op_geo, device="cuda")
    opt_b = torch.optim.SGD(m_b.parameters(), lr=LR)

    def params_step():
        opt_b.zero_grad(set_to_none=True)
        x.grad = None
        bce(m_b(x), y).backward()
        opt_b.step()
    fns["params_eager_step_ms"] = params_step
    if not profile:
        m_c = CatfishModule.from_weights(w, *op_geo, device="cuda")
        opt_c = torch.optim.SGD(m_c.parameters(), lr=LR)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                opt_c.zero_grad(set_to_none=True)
                x.grad = None
                bce(m_c(x), y).backward()
                opt_c.step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        opt_c.zero_grad(set_to_none=True)
        x.grad = None
        with torch.cuda.graph(graph):
            bce(m_c(x), y).backward()
            opt_c.step()
        fns["params_graph_step_ms"] = graph.replay
        fns["_graph"] = graph                                     # kept alive with the variants
    return fns


def main():
    profile = "--profile" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sink = open(out_path, "w") if out_path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    rng = np.random.default_rng(0)
    configs = CONFIGS[:1] if profile else CONFIGS
    for kind, h, c, nl, nr, n in configs:
        geo = (h, c, nl, nr)
        if kind == "checkpoint":
            with np.load(os.path.join(ROOT, "tests", "golden", "ckpnt-30000-inference.npz")) as z:
                w = {k: z[k] for k in z.files}
        else:
            w = oracle.random_weights(seed=3, layer_size=h, n_layers=nl, layer_size_res=c, n_layers_res=nr)
        x = torch.tensor(rng.normal(0, 1, size=(n, 35)).astype(np.float32), device="cuda").requires_grad_(True)
        y = torch.tensor(np.repeat((rng.random(n) < 0.3)[:, None], 35, axis=1).reshape(-1).astype(np.float32), device="cuda")
        fns = step_variants(w, geo, x, y, profile)
        graph = fns.pop("_graph", None)
        base = dict(weights=kind, layer_size=h, layer_size_res=c if nr else 0, n_layers=nl, n_layers_res=nr, windows=n)
        if n == 256:                                              # forward alone and the load alone
            op_geo = (nl, h, nr, c)
            packed = ops.pack_weights(w, *op_geo)
            params = packed[ops.HEADER:].cuda()
            xf = x.detach()
            eng = ops._params_engine(0, op_geo)

            def fwd_packed():
                with torch.no_grad():
                    torch.ops.catfish.resnetrnn_forward(xf, packed)

            def fwd_params():
                with torch.no_grad():
                    torch.ops.catfish.resnetrnn_forward_params(xf, params, *op_geo)
            if not profile:
                fns["forward_packed_ms"] = fwd_packed
                fns["forward_params_ms"] = fwd_params
            fns["load_params_ms"] = lambda: eng.load_params_device(params)
        times = {k: [] for k in fns}
        for _ in range(1 if profile else ROUNDS):
            for k, fn in fns.items():                             # alternate, so that clock and neighbour drift hit every variant alike
                iters = 3 if k.startswith("packed") else (100 if k.startswith("load") else 10)
                times[k].append(device_ms(fn, iters if not profile else 20))
        res = dict(base)
        res.update({k: float(np.median(v)) for k, v in times.items()})
        if n == 256:
            res["param_count"] = ops.param_count(nl, h, nr, c)
        emit(res)
        del fns, graph
        torch.cuda.synchronize()
        ops.clear_engine_cache()
        ops.clear_params_engine_cache()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
