"""Device-resident trainable weights: ``cf_model_load_params`` (``HipEngine.load_params_device``), the operator
``torch.ops.catfish.resnetrnn_forward_params`` and ``torch_module.CatfishModule``."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_C = 32                  # layer_size_res of a plain RNN model: recorded, unused
SCHEMA = ("catfish::resnetrnn_forward_params(Tensor x, Tensor params, int n_layers, int layer_size, int n_layers_res, "
          "int layer_size_res) -> Tensor")


def _ckpt():
    with np.load(os.path.join(ROOT, "tests", "golden", "ckpnt-30000-inference.npz")) as z:
        return {k: z[k] for k in z.files}


def _random(geo, seed):
    h, c, n_layers, n_blocks = geo
    return oracle.random_weights(seed=seed, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks)


def _op_geo(geo):
    """(layer_size, layer_size_res, n_layers, n_layers_res) -> the operator's (n_layers, layer_size, n_layers_res, layer_size_res)."""
    h, c, n_layers, n_blocks = geo
    return n_layers, h, n_blocks, c


# ---------------------------------------------------------------------------------------------------- CPU
def test_schema_of_the_params_operator():
    import torch
    import catfish_amd.torch_ops  # noqa: F401
    assert str(torch.ops.catfish.resnetrnn_forward_params.default._schema) == SCHEMA


def test_meta_shape_inference():
    import torch
    import catfish_amd.torch_ops as ops
    n = ops.param_count(3, 64, 2, 32)
    out = torch.ops.catfish.resnetrnn_forward_params(torch.empty(7, 35, device="meta"), torch.empty(n, device="meta"), 3, 64, 2, 32)
    assert out.shape == (7 * 35,) and out.dtype == torch.float32 and out.device.type == "meta"
    out = torch.ops.catfish.resnetrnn_forward_params(torch.empty(5, 35, 1, device="meta"), torch.empty(n, device="meta"), 3, 64, 2, 32)
    assert out.shape == (5 * 35,)


@pytest.mark.parametrize("geo", [(64, 32, 3, 2), (16, 16, 2, 2), (128, 32, 2, 0), (64, 32, 1, 0), (128, 128, 5, 5), (48, 80, 2, 1)])
def test_param_count_is_the_packed_length_without_header(geo):
    import catfish_amd.torch_ops as ops
    h, c, n_layers, n_blocks = geo
    packed = ops.pack_weights(_random(geo, 1), n_layers, h, n_blocks, c)
    assert ops.param_count(n_layers, h, n_blocks, c) == packed.numel() - 8 == packed.numel() - ops.HEADER


def test_cpu_x_is_refused():
    import torch
    import catfish_amd.torch_ops as ops
    n = ops.param_count(3, 64, 2, 32)
    with pytest.raises(ValueError, match="MI355X"):
        torch.ops.catfish.resnetrnn_forward_params(torch.zeros(2, 35), torch.zeros(n), 3, 64, 2, 32)


@pytest.mark.parametrize("geo", [(64, 32, 3, 2), (48, 80, 2, 1), (128, PLAIN_C, 2, 0)])
def test_module_round_trips_weights_and_views_share_storage(geo):
    import torch
    import catfish_amd.torch_ops as ops
    from catfish_amd.torch_module import CatfishModule
    w = _random(geo, 2)
    m = CatfishModule.from_weights(w, *_op_geo(geo))
    assert isinstance(m.params, torch.nn.Parameter) and m.params.dim() == 1 and m.params.numel() == ops.param_count(*_op_geo(geo))
    back = m.weights()
    assert sorted(back) == sorted(ops.tensor_names(geo[2], geo[3]))
    for k, v in back.items():
        assert v.dtype == np.float32 and v.shape == np.asarray(w[k]).shape
        np.testing.assert_array_equal(v, np.asarray(w[k], np.float32))
    name = "final_fully_connected/kernel"
    view = m.tensor(name)
    assert view.shape == (2 * geo[0], 1)
    assert view.untyped_storage().data_ptr() == m.params.untyped_storage().data_ptr()
    with torch.no_grad():
        view.fill_(0.25)
    assert (m.weights()[name] == 0.25).all()
    with pytest.raises(KeyError):
        m.tensor("no/such/tensor")
    with pytest.raises(ValueError):
        CatfishModule(torch.zeros(10), *_op_geo(geo))


def test_new_symbols_are_bound():
    from catfish_amd import _native as N
    assert "cf_model_param_floats" in N.SYMBOLS and "cf_model_load_params" in N.SYMBOLS
    assert N.CF_ABI_VERSION == 9


# ---------------------------------------------------------------------------------------------------- GPU
def _x(n, seed):
    import torch
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.normal(0, 1, size=(n, 35)).astype(np.float32), device="cuda")


def _flat(w, geo):
    import catfish_amd.torch_ops as ops
    return ops.pack_weights(w, *_op_geo(geo))[ops.HEADER:].cuda()


def _engine(w, geo, **kw):
    from catfish_amd.engine import HipEngine
    h, c, n_layers, n_blocks = geo
    return HipEngine(w, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks, device=0, **kw)


def _load_equals_create(geo, counts, max_windows):
    import torch
    a, b = _random(geo, 11), _random(geo, 12)
    eng = _engine(a, geo, max_windows_per_pass=max_windows)
    fresh_b = _engine(b, geo, max_windows_per_pass=max_windows)
    assert eng.param_count() == _flat(a, geo).numel()
    xs = [_x(n, n) for n in counts]
    want_a = [eng.infer_device(x).clone() for x in xs]
    want_b = [fresh_b.infer_device(x) for x in xs]
    eng.load_params_device(_flat(b, geo))
    for n, x, wb in zip(counts, xs, want_b):
        assert torch.equal(eng.infer_device(x), wb), (geo, n)
    eng.load_params_device(_flat(a, geo))
    for n, x, wa in zip(counts, xs, want_a):
        assert torch.equal(eng.infer_device(x), wa), (geo, n)
    torch.cuda.synchronize()
    eng.check_error()
    eng.close()
    fresh_b.close()


@pytest.mark.gpu
def test_load_equals_create_at_every_launch_regime_of_the_shipped_geometry():
    from catfish_amd.engine import HipEngine
    probe = HipEngine(_random((64, 32, 3, 2), 1), device=0, max_windows_per_pass=1024)
    r = probe.launch_regimes()
    probe.close()
    counts = [1, r["hoist_max"], r["coop_max"], r["coop_max"] + 1]
    if 0 < r["fuse_auto_min"] <= 32768:
        counts.append(r["fuse_auto_min"])
    counts.append(40000)                                    # several passes of 32768 windows
    _load_equals_create((64, 32, 3, 2), sorted(set(counts)), 32768)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(64, 32, 1, 0), (64, 128, 2, 1), (16, 16, 2, 2), (128, 64, 3, 2), (48, 80, 2, 1), (128, PLAIN_C, 2, 0),
                                 (128, 128, 5, 5)])
def test_load_equals_create(geo):
    _load_equals_create(geo, [1, 37, 300], 4096)


def _reference(w, geo, x, g):
    """d loss / d x and d loss / d every tensor of loss = (sigmoid(logits(x)) . g).sum(), float64 CPU (TorchResNetRNN)."""
    import torch
    from catfish_amd.training import TorchResNetRNN
    h, c, n_layers, n_blocks = geo
    net = TorchResNetRNN(w, n_layers, n_blocks, device="cpu", dtype=torch.float64)
    for t in net.params.values():
        t.requires_grad_(True)
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    probs = torch.sigmoid(net.logits(xt))
    (probs.reshape(-1) * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return probs.detach().reshape(-1).numpy(), xt.grad.numpy(), {k: v.grad.numpy() for k, v in net.params.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("geo", ["ckpt", (32, 16, 2, 1), (48, 80, 2, 1), (64, PLAIN_C, 2, 0)])
def test_params_operator_equals_the_packed_operator(geo):
    """Output, x gradient and weight gradient bit-identical to resnetrnn_forward with a CPU packed tensor; all three against the
    float64 restatement."""
    import torch
    import catfish_amd.torch_ops as ops
    if geo == "ckpt":
        w, geo = _ckpt(), (64, 32, 3, 2)
    else:
        w = _random(geo, 5)
    packed = ops.pack_weights(w, *_op_geo(geo))
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, size=(45, 35)).astype(np.float32)
    g = torch.tensor(rng.normal(0, 1, size=45 * 35).astype(np.float32), device="cuda")
    xa = torch.tensor(x, device="cuda", requires_grad=True)
    pa = packed.clone().requires_grad_(True)
    out_a = torch.ops.catfish.resnetrnn_forward(xa, pa)
    (out_a * g).sum().backward()
    xb = torch.tensor(x, device="cuda", requires_grad=True)
    pb = packed[ops.HEADER:].cuda().requires_grad_(True)
    out_b = torch.ops.catfish.resnetrnn_forward_params(xb, pb, *_op_geo(geo))
    (out_b * g).sum().backward()
    assert torch.equal(out_a, out_b)
    assert torch.equal(xa.grad, xb.grad)
    assert pb.grad.is_cuda and pb.grad.dtype == torch.float32 and pb.grad.shape == pb.shape
    assert torch.equal(pb.grad.cpu(), pa.grad[ops.HEADER:])
    rp, rx, rw = _reference(w, geo, x, g.cpu().numpy())
    assert np.abs(out_b.detach().cpu().numpy() - rp).max() < 1e-4
    assert np.abs(xb.grad.cpu().numpy() - rx).max() <= 1e-4 * max(1.0, np.abs(rx).max())
    flat = pb.grad.cpu().numpy()
    off, shapes = 0, ops._shapes(*_op_geo(geo))
    for name in ops.tensor_names(geo[2], geo[3]):
        size = int(np.prod(shapes[name]))
        got, want = flat[off:off + size].reshape(shapes[name]), rw[name]
        assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), name
        off += size
    ops.clear_engine_cache()
    ops.clear_params_engine_cache()


def _bce(probs, y):
    import torch
    return torch.nn.functional.binary_cross_entropy(probs.clamp(1e-6, 1 - 1e-6), y)


def _batch(n, seed):
    import torch
    rng = np.random.default_rng(seed)
    x = torch.tensor(rng.normal(0, 1, size=(n, 35)).astype(np.float32), device="cuda")
    y = torch.tensor(np.repeat((rng.random(n) < 0.3)[:, None], 35, axis=1).reshape(-1).astype(np.float32), device="cuda")
    return x, y


@pytest.mark.gpu
def test_training_loop_uses_one_engine():
    """20 SGD steps through CatfishModule: one engine in the per-geometry cache, none in the content-keyed one, the loss falls,
    and the parameters follow the same loop through the packed operator."""
    import torch
    import catfish_amd.torch_ops as ops
    from catfish_amd.torch_module import CatfishModule
    ops.clear_engine_cache()
    ops.clear_params_engine_cache()
    w = _ckpt()
    x, y = _batch(96, 9)
    model = CatfishModule.from_weights(w, device="cuda")
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = _bce(model(x), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert len(ops._PARAM_ENGINES) == 1 and not ops._ENGINES
    with torch.no_grad():
        final = float(_bce(model(x), y))
    assert final < losses[0], (losses, final)
    packed = ops.pack_weights(w).requires_grad_(True)
    opt2 = torch.optim.SGD([packed], lr=0.05)
    for _ in range(20):
        opt2.zero_grad()
        _bce(torch.ops.catfish.resnetrnn_forward(x, packed), y).backward()
        opt2.step()
    diff = (model.params.detach().cpu() - packed.detach()[ops.HEADER:]).abs().max().item()
    assert diff <= 1e-5, diff
    ops.clear_engine_cache()
    ops.clear_params_engine_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(64, 32, 3, 2), (128, 64, 3, 2)])
def test_cuda_graph_of_a_whole_training_step(geo):
    """Forward + backward (x and params) + SGD step of CatfishModule captured as one CUDA graph: 3 eager warm-up steps and 5
    replays leave the parameters bit-identical to an eager twin after 8 steps."""
    import torch
    import catfish_amd.torch_ops as ops
    from catfish_amd.torch_module import CatfishModule
    w = _ckpt() if geo == (64, 32, 3, 2) else _random(geo, 8)
    x, y = _batch(256, 4)
    x.requires_grad_(True)

    def make():
        m = CatfishModule.from_weights(w, *_op_geo(geo), device="cuda")
        return m, torch.optim.SGD(m.parameters(), lr=0.05)

    model, opt = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            x.grad = None
            _bce(model(x), y).backward()
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    x.grad = None
    with torch.cuda.graph(graph):
        static_loss = _bce(model(x), y)
        static_loss.backward()
        opt.step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    twin, opt_t = make()
    for _ in range(8):
        opt_t.zero_grad(set_to_none=True)
        _bce(twin(x), y).backward()
        opt_t.step()
    torch.cuda.synchronize()
    assert torch.equal(model.params.detach(), twin.params.detach())
    assert not torch.equal(model.params.detach(), make()[0].params.detach())      # the steps did move the weights
    del graph
    torch.cuda.synchronize()
    ops.clear_params_engine_cache()


@pytest.mark.gpu
def test_refusals():
    import torch
    import catfish_amd.torch_ops as ops
    from catfish_amd import _native as N
    for geo, precision in (((64, 32, 3, 2), "bf16x3"), ((128, 64, 3, 2), "bf16x3"), ((64, 32, 3, 2), "bf16")):
        w = _random(geo, 1)
        eng = _engine(w, geo, max_windows_per_pass=256, precision=precision)
        with pytest.raises(ValueError, match="CF_PREC_FP32"):
            eng.load_params_device(_flat(w, geo))
        eng.close()
    geo = (32, 16, 2, 1)
    w = _random(geo, 2)
    eng = _engine(w, geo, max_windows_per_pass=256)
    p = _flat(w, geo)
    bad = [p[:-1], p.double(), p.cpu(), torch.cat([p, p[:1]])]
    if torch.cuda.device_count() > 1:
        bad.append(p.to("cuda:1"))
    for t in bad:
        with pytest.raises(ValueError):
            eng.load_params_device(t)
    lib = eng._lib
    n = C.c_int64()
    assert lib.cf_model_param_floats(None, C.byref(n)) == N.CF_ERR_INVALID
    assert lib.cf_model_param_floats(eng._handle, None) == N.CF_ERR_INVALID
    assert lib.cf_model_load_params(None, C.c_void_p(p.data_ptr()), None) == N.CF_ERR_INVALID
    assert lib.cf_model_load_params(eng._handle, None, None) == N.CF_ERR_INVALID
    assert lib.cf_model_param_floats(eng._handle, C.byref(n)) == N.CF_OK and n.value == p.numel()
    eng.close()
    # the operator: bad params, double backward, opcheck
    x = torch.randn(20, 35, device="cuda", requires_grad=True)
    op_geo = _op_geo(geo)
    for t in (p[:-1], p.double(), p.cpu()):
        with pytest.raises(ValueError):
            torch.ops.catfish.resnetrnn_forward_params(x, t, *op_geo)
    params = p.clone().requires_grad_(True)
    out = torch.ops.catfish.resnetrnn_forward_params(x, params, *op_geo)
    gx, = torch.autograd.grad(out.pow(2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once-differentiable"):
        torch.autograd.grad(gx.sum(), x)
    torch.library.opcheck(torch.ops.catfish.resnetrnn_forward_params.default, (x, params) + tuple(op_geo),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    torch.cuda.synchronize()
    ops.clear_params_engine_cache()
