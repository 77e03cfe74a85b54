"""The whole training step of any geometry on the HIP kernels (catfish_amd/anysize_step.py, ``Trainer(..., native=True)``)."""
import numpy as np
import pytest

from oracle import catfish_oracle as oracle


def _batch(rng, n):
    x = rng.normal(0, 1.0, size=(n, 35)).astype(np.float32)
    y = np.repeat((rng.random(n) < 0.5)[:, None], 35, axis=1).astype(np.float32)
    return x, y


def _masks(rng, n, h, n_layers, kp):
    return {(layer, d): (rng.random((n, 35, h)) < kp).astype(np.float32) for layer in range(n_layers) for d in ("fw", "bw")}


# ---------------------------------------------------------------------------------------------------- CPU: layout and gather map
@pytest.mark.parametrize("geo", [(32, 16, 2, 1), (48, 32, 2, 0), (16, 80, 3, 2)])
def test_flat_layout_covers_every_variable_once_and_the_gather_map_matches_pack_maps(geo):
    from catfish_amd.anysize_step import flat_layout, flat_pack_map
    from catfish_amd.anysize_train import pack_maps
    h, c, n_layers, n_blocks = geo
    w = oracle.random_weights(seed=3, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks)
    entries, units, layers, head, zero = flat_layout(h, c, n_layers, n_blocks)
    assert sorted(name for name, _, _ in entries) == sorted(w)
    covered = np.zeros(zero + 1, np.int64)
    flat = np.zeros(zero + 1, np.float32)
    for name, off, shape in entries:
        assert tuple(shape) == tuple(w[name].shape), name
        n = int(np.prod(shape))
        covered[off:off + n] += 1
        flat[off:off + n] = np.asarray(w[name], np.float32).reshape(-1)
    assert (covered[:zero] == 1).all() and covered[zero] == 0
    idx, scale, per_layer = flat_pack_map(h, layers, zero)
    packed = flat[idx] * scale
    pre = "stack_bidirectional_rnn/cell_%d/bidirectional_rnn/%s/gru_cell"
    for layer, (_, cin) in enumerate(layers):
        w_idx, w_scale, b_idx, b_scale, wt_idx = (t.numpy() for t in pack_maps(h, cin, "cpu"))
        srcs = [np.concatenate([np.asarray(w[pre % (layer, d) + k], np.float32).reshape(-1)
                                for k in ("/gates/kernel", "/candidate/kernel", "/gates/bias", "/candidate/bias")] + [np.zeros(1, np.float32)])
                for d in ("fw", "bw")]
        for (start, count), (i, s) in zip(per_layer[layer], ((w_idx, w_scale), (b_idx, b_scale), (wt_idx, None))):
            want = np.concatenate([src[i] * (1.0 if s is None else s) for src in srcs])
            assert count == want.size
            np.testing.assert_array_equal(packed[start:start + count], want.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- GPU
def _trainers(w, geo, opt="Adam", kp=0.8, **kw):
    from catfish_amd.training import Trainer
    h, c, n_layers, n_blocks = geo
    a = Trainer(w, n_layers, n_blocks, opt, 1e-3, kp, seed=1, native=True, **kw)
    b = Trainer(w, n_layers, n_blocks, opt, 1e-3, kp, seed=1, native=False, use_graph=False)
    return a, b


def _close(ga, gb):
    assert sorted(ga) == sorted(gb)
    for k in gb:
        assert np.abs(ga[k] - gb[k]).max() <= 2e-4 * np.abs(gb[k]).max() + 1e-6, (k, np.abs(ga[k] - gb[k]).max(), np.abs(gb[k]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("geo,n", [((32, 16, 2, 1), 40), ((128, 64, 1, 1), 150), ((48, 32, 2, 0), 75), ((128, 32, 2, 0), 33),
                                   ((256, 32, 1, 1), 600), ((16, 80, 3, 2), 512), ((64, 64, 2, 1), 40), ((128, 128, 5, 5), 40),
                                   ((32, 16, 2, 1), 2100)])
def test_native_step_gradients_equal_the_torch_trainer(geo, n):
    """Every trainable variable's gradient and the loss, with explicit dropout masks at keep_prob 0.8, against the pure-torch
    restatement of the graph (bounds of the existing any-size tests); a second run of the same batch is bit-identical."""
    pytest.importorskip("torch")
    h, c, n_layers, n_blocks = geo
    w = oracle.random_weights(seed=7, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks)
    a, b = _trainers(w, geo)
    assert a.step_impl is not None and type(a.step_impl).__name__ == "AnySizeTrainStep"
    rng = np.random.default_rng(4)
    x, y = _batch(rng, n)
    masks = _masks(rng, n, h, n_layers, 0.8)
    la, ga = a.gradients(x, y, masks=masks)
    lb, gb = b.gradients(x, y, masks=masks)
    assert abs(la - lb) < 1e-5, (la, lb)
    _close(ga, gb)
    la2, ga2 = a.gradients(x, y, masks=masks)
    assert la2 == la and all(np.array_equal(ga[k], ga2[k]) for k in ga)
    a.engine.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(32, 16, 2, 1), (128, 32, 2, 0)])
def test_in_kernel_dropout_masks_replay_through_torch(geo):
    """The masks the kernels draw (written out by dropout_scales) replayed through torch give the same loss and gradients; they keep
    about keep_prob of the elements and change per layer and per optimizer step."""
    pytest.importorskip("torch")
    h, c, n_layers, n_blocks = geo
    w = oracle.random_weights(seed=8, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks)
    a, b = _trainers(w, geo, use_graph=False)
    rng = np.random.default_rng(5)
    x, y = _batch(rng, 70)
    m0 = a.step_impl.dropout_scales(70)
    la, ga = a.gradients(x, y)
    lb, gb = b.gradients(x, y, masks=m0)
    assert abs(la - lb) < 1e-5
    _close(ga, gb)
    frac = np.mean([m.mean() for m in m0.values()])
    assert abs(frac - 0.8) < 0.01
    assert not np.array_equal(m0[(0, "fw")], m0[(1, "fw")])
    a.train_step(x, y)
    m1 = a.step_impl.dropout_scales(70)
    assert not np.array_equal(m0[(0, "fw")], m1[(0, "fw")])
    a.engine.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geo,opt,n", [((128, 64, 3, 2), "Adam", 128), ((128, 32, 2, 0), "RMSProp", 512),
                                       ((128, 64, 3, 2), "RMSProp", 512), ((128, 32, 2, 0), "Adam", 128)])
def test_native_trainer_follows_the_torch_trajectory(geo, opt, n):
    """Ten graph-replayed native steps follow the native=False trainer's loss trajectory; the loss falls."""
    pytest.importorskip("torch")
    h, c, n_layers, n_blocks = geo
    w = oracle.random_weights(seed=9, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks)
    a, b = _trainers(w, geo, opt=opt, kp=1.0)
    assert a.native and not a.anysize and a.use_graph
    rng = np.random.default_rng(6)
    la, lb = [], []
    for _ in range(10):
        x, _ = _batch(rng, n)
        y = (x > 0).astype(np.float32)                       # a learnable target: the loss falls under either optimizer
        la.append(a.train_step(x, y))
        lb.append(b.train_step(x, y))
    assert np.isfinite(la).all() and np.allclose(la, lb, rtol=0, atol=2e-3), (la, lb)
    assert la[-1] < la[0]
    a.engine.close()


@pytest.mark.gpu
def test_graph_replay_equals_eager_with_dropout():
    pytest.importorskip("torch")
    from catfish_amd.training import Trainer
    geo = (128, 64, 2, 1)
    w = oracle.random_weights(seed=10, layer_size=128, n_layers=2, layer_size_res=64, n_layers_res=1)
    g = Trainer(w, 2, 1, "RMSProp", 1e-3, 0.8, seed=5, native=True, use_graph=True)
    e = Trainer(w, 2, 1, "RMSProp", 1e-3, 0.8, seed=5, native=True, use_graph=False)
    rng = np.random.default_rng(7)
    for _ in range(4):
        x, y = _batch(rng, 128)
        assert g.train_step(x, y) == e.train_step(x, y)
    gw, ew = g.net.numpy_weights(), e.net.numpy_weights()
    assert all(np.array_equal(gw[k], ew[k]) for k in gw), geo
    g.engine.close()
    e.engine.close()


@pytest.mark.gpu
def test_native_step_on_the_shipped_geometry_draws_the_tuned_steps_masks(ckpt_weights):
    """Built directly on the shipped 64 / 32 checkpoint, the any-size step draws the same dropout masks as NativeTrainStep and
    gives the same loss and gradients as it."""
    torch = pytest.importorskip("torch")
    from catfish_amd.anysize_step import AnySizeTrainStep
    from catfish_amd.engine import HipEngine
    from catfish_amd.training import Trainer, TFOptimizer, TorchResNetRNN
    tr = Trainer(ckpt_weights, 3, 2, "RMSProp", 1e-3, keep_prob=0.8, device="cuda", native=True, seed=5, use_graph=False)
    net = TorchResNetRNN(ckpt_weights, 3, 2, device="cuda")
    opt = TFOptimizer(net.trainable(), "RMSProp", 1e-3)
    eng = HipEngine(ckpt_weights, layer_size=64, n_layers=3, layer_size_res=32, n_layers_res=2, device=0, max_windows_per_pass=256)
    st = AnySizeTrainStep(net, opt, eng, 0.8, seed=5)
    assert st.seed == tr.step_impl.seed
    ma, mb = st.dropout_scales(50), tr.step_impl.dropout_scales(50)
    assert all(np.array_equal(ma[k], mb[k]) for k in mb)
    rng = np.random.default_rng(8)
    x, y = _batch(rng, 50)
    b = st.alloc(50)
    st.load_batch(b, x, y)
    la = float(st.run(b, update=False))
    ga = {k: v.detach().cpu().numpy() for k, v in st.grads().items()}
    lb, gb = tr.gradients(x, y)
    assert abs(la - lb) < 1e-5
    _close(ga, gb)
    eng.close()
    tr.engine.close()
    del torch


@pytest.mark.gpu
def test_round_trip_save_load_infer_and_resume(tmp_path):
    pytest.importorskip("torch")
    from catfish_amd.resnet_class import ResNetRNN
    hp = dict(batch_size=128, optimizer_choice="Adam", learning_rate=1e-3, layer_size=128, n_layers=2, keep_prob=1.0,
              layer_size_res=64, n_layers_res=1, native_training=True)
    net = ResNetRNN(**hp)
    net.initialize_network()
    rng = np.random.default_rng(9)
    for s in range(3):
        x, y = _batch(rng, 128)
        net.train_network(x, y, s)
    tr = net._trainer
    assert tr.native and type(tr.step_impl).__name__ == "AnySizeTrainStep"
    d = str(tmp_path)
    net.save_network(d, 3)
    x, y = _batch(rng, 32)
    want = tr.net.logits(x).detach().cpu().numpy()
    other = ResNetRNN(**hp)
    other.restore_network(d)
    probs = np.asarray(other.infer(x[:, :, None])).reshape(32, 35)
    assert np.abs(probs - 1.0 / (1.0 + np.exp(-want))).max() < 1e-4
    # resume: the restored network continues where the trainer stands
    xs = [_batch(rng, 128) for _ in range(3)]
    la = [net.train_network(*b, 4 + i) or net.train_loss for i, b in enumerate(xs)]
    lb = [other.train_network(*b, 4 + i) or other.train_loss for i, b in enumerate(xs)]
    assert np.allclose(la, lb, rtol=0, atol=1e-4), (la, lb)


@pytest.mark.gpu
def test_invalid_arguments_raise():
    torch = pytest.importorskip("torch")
    import ctypes as C
    from catfish_amd import _native as N
    from catfish_amd.engine import HipEngine
    from catfish_amd.training import Trainer
    w = oracle.random_weights(seed=11, layer_size=32, n_layers=1, layer_size_res=16, n_layers_res=1)
    with pytest.raises(ValueError):
        Trainer(w, 1, 1, "Adam", 1e-3, 1.0, device="cpu", native=True)
    with pytest.raises(ValueError):
        Trainer(w, 1, 1, "Adam", 1e-3, 1.0, device="cuda", native=True, dtype=torch.float64)
    eng = HipEngine(w, layer_size=32, n_layers=1, layer_size_res=16, n_layers_res=1, device=0, max_windows_per_pass=256)
    lib, hd = eng._lib, eng._handle
    buf = torch.zeros(1 << 20, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = [
        lambda: lib.cf_gen_conv_forward(hd, 2, 16, 16, p, p, None, 1, p, p, 16, s),            # kw
        lambda: lib.cf_gen_conv_forward(hd, 1, 16, 16, p, p, None, 1, p, p, 17, s),            # n_windows
        lambda: lib.cf_gen_conv_forward(hd, 1, 16, 16, None, p, None, 1, p, p, 16, s),         # null
        lambda: lib.cf_gen_conv_backward_data(hd, 3, 1, 16, p, p, None, p, 16, s),            # cin 1 has no dx
        lambda: lib.cf_gen_bn_backward(hd, 1, 16, 24, p, p, None, 1, p, p, p, 1 << 20, p, 16, s),
        lambda: lib.cf_gen_bn_backward(hd, 1, 16, 16, p, p, None, 1, p, p, p, 1, p, 16, s),    # workspace
        lambda: lib.cf_gen_conv_wgrad(hd, 1, 16, 16, p, p, p, 1, p, 16, s),                   # workspace
        lambda: lib.cf_gen_gru_dx(hd, 24, 16, p, p, p, 16, s),                                # layer_size
        lambda: lib.cf_gen_gru_wgrad(hd, 32, 16, p, p, p, p, p, 1 << 20, p, 0, s),            # n_windows
        lambda: lib.cf_gen_dropout(hd, 32, 1.0, 0, 0, None, None, p, p, 16, s),                # keep_prob without scale
        lambda: lib.cf_gen_head(hd, 64, p, p, p, 0, p, None, p, 1 << 20, p, p, 16, s),         # n_real
        lambda: lib.cf_gen_x_frag(hd, None, p, 16, s),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            N.check(call())
    torch.cuda.synchronize()
    eng.close()
