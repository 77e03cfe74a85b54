"""The device-fed training loop on the card: cf_sample_batch against the host sampler, Trainer.train_steps against the host-fed
Trainer.train_step on the same batches, and train_and_validate with a DeviceExampleDb against the per-step loop."""
import ctypes as C
import os

import numpy as np
import pytest

from catfish_amd import device_db as ddb, train_validate as tv
from catfish_amd.device_db import DeviceExampleDb
from oracle import catfish_oracle as oracle
from test_device_db import RATIOS, SIZES, pool_shapes, pools

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("size", SIZES)
def test_kernel_draws_what_the_host_function_draws(size, ratio):
    """Eight consecutive draws through ONE captured graph replayed eight times: x and the first ``size`` rows of y are the
    host-gathered rows bit for bit, rows of y past ``size`` stay zero, the device counter reads d + 1."""
    torch = pytest.importorskip("torch")
    from catfish_amd import _native as N
    lib = N.lib()
    dev = torch.device("cuda", 0)
    npad = (size + 15) // 16 * 16
    ptr = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    for n_pos, n_neg in pool_shapes(size, ratio):
        db = DeviceExampleDb(*pools(n_pos, n_neg, seed=size + ratio), seed=0x9E3779B9 + n_pos)
        pos, neg, counter = db.device_pools(dev)
        x = torch.full((size, 35), -7.0, dtype=torch.float32, device=dev)
        y = torch.zeros(npad, 35, dtype=torch.float32, device=dev)

        def launch():
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            N.check(lib.cf_sample_batch(None, ptr(pos), n_pos, ptr(neg), n_neg, size, ratio, db.seed, ptr(counter), ptr(x), ptr(y),
                                        stream))

        launch()                                           # module load outside the capture
        first = 2 ** 32 - 3                                # the draw number wraps at 32 bits inside the key, not in the counter
        counter.fill_(first)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launch()
        assert int(counter.item()) == first                # capturing runs nothing
        for d in range(first, first + 8):
            g.replay()
            want_x, is_pos = db.gather(d, size, ratio)
            got_x, got_y = x.cpu().numpy(), y.cpu().numpy()
            assert np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32)), (size, ratio, n_pos, n_neg, d)
            assert np.array_equal(got_y[:size], np.repeat(is_pos.astype(np.float32)[:, None], 35, 1))
            assert not got_y[size:].any()
            assert int(counter.item()) == d + 1


def test_kernel_refuses_a_short_pool():
    torch = pytest.importorskip("torch")
    from catfish_amd import _native as N
    dev = torch.device("cuda", 0)
    z = torch.zeros(64, 35, dtype=torch.float32, device=dev)
    c = torch.zeros(1, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    with pytest.raises(ValueError):
        N.check(N.lib().cf_sample_batch(None, p(z), 31, p(z), 64, 64, 2, 1, p(c), p(z), p(z), None))
    assert int(c.item()) == 0


# ---------------------------------------------------------------------------------------------------- the trainer
def _weights(geo, ckpt_weights):
    if geo == "shipped":
        return ckpt_weights, 3, 2
    h, c, n_layers, n_blocks = geo
    return oracle.random_weights(seed=21, layer_size=h, n_layers=n_layers, layer_size_res=c, n_layers_res=n_blocks), n_layers, n_blocks


def _trainer(geo, ckpt_weights, native, kp, **kw):
    from catfish_amd.training import Trainer
    w, n_layers, n_blocks = _weights(geo, ckpt_weights)
    return Trainer(w, n_layers, n_blocks, "RMSProp" if geo == "shipped" else "Adam", 1e-3, kp, seed=5, native=native, **kw)


def _state(tr):
    out = dict(tr.net.numpy_weights())
    out.update({"slot:" + k: np.asarray(v) for k, v in tr.opt.state_tf().items()})
    return out


def _assert_same(a, b, tol=0.0):
    assert sorted(a) == sorted(b)
    worst = max(float(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).max()) for k in a)
    print("largest difference over %d variables and slots: %.3g (tolerance %g)" % (len(a), worst, tol))
    for k in a:
        if tol:
            assert np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).max() <= tol, k
        else:
            assert np.array_equal(a[k], b[k]), k


def _db(seed=7):
    return DeviceExampleDb(*pools(500, 900, seed=12), seed=seed)


def _host_fed(tr, batches):
    return np.array([tr.train_step(x, y) for x, y, _ in batches], dtype=np.float32)


def _close(tr):
    if tr.engine is not None:
        tr.engine.close()


@pytest.mark.parametrize("geo,native,kp", [("shipped", None, 0.8), ((128, 64, 2, 1), True, 0.8),
                                           ((32, 32, 2, 0), None, 1.0), ((128, 64, 2, 1), None, 1.0)],
                         ids=["shipped-native", "128-64-native", "rnn32-autograd", "128-64-autograd"])
def test_device_fed_equals_host_fed(geo, native, kp, ckpt_weights):
    """train_steps(db, 12, 64) against train_step on the twin database's twelve batches: the inputs are the same float32 bits,
    the kernels and their fixed-order reductions the same, the dropout keys come from the same opt.t -- so losses, variables and
    optimizer slots are BIT-EQUAL.  The native steps hash their masks from (seed, layer, opt.t, element); the autograd path
    draws them from torch's process-wide CUDA generator, which every replay of either trainer advances, so it is compared
    without dropout.  For the autograd path only: should the library GEMMs turn out not to be run-to-run deterministic under
    replay (two host-fed runs differ), the comparison is made at the 1e-6 DESIGN section 4 documents for these trajectories.
    Seen on an MI355X: the 32-unit RNN repeats itself bit for bit and is compared bit for bit; 128 / 64 does not repeat itself
    (its host-fed runs already differ from each other) and is compared at 1e-6."""
    pytest.importorskip("torch")
    twin = _db()
    batches = [twin.get_training_set(64) for _ in range(12)]
    host = _trainer(geo, ckpt_weights, native, kp)
    want = _host_fed(host, batches)
    tol = 0.0
    if native is None and geo != "shipped":
        again = _trainer(geo, ckpt_weights, native, kp)
        repeat = _host_fed(again, batches)
        if not (np.array_equal(repeat, want) and all(np.array_equal(v, _state(host)[k]) for k, v in _state(again).items())):
            tol = 1e-6
        _close(again)
    fed = _trainer(geo, ckpt_weights, native, kp)
    db = _db()
    got = fed.train_steps(db, 12, 64)
    print("losses host-fed", want, "device-fed", got, "tolerance", tol)
    assert got.dtype == np.float32 and got.shape == (12,) and np.isfinite(got).all()
    assert db.draw == 12 and fed.last_loss == float(got[-1])
    if tol:
        assert np.abs(got.astype(np.float64) - want).max() <= tol
    else:
        assert np.array_equal(got, want)
    _assert_same(_state(fed), _state(host), tol)
    lx, ly = db.last_batch()                               # the static buffers hold the twelfth batch
    assert np.array_equal(lx, np.stack(batches[-1][0])) and np.array_equal(ly, np.asarray(batches[-1][1]))
    _close(fed), _close(host)


def test_first_replay_after_the_capture_trains_on_the_current_draw(ckpt_weights):
    """The warm-up launches before the capture leave the draw counter, opt.t and the variables where they were."""
    pytest.importorskip("torch")
    fed = _trainer("shipped", ckpt_weights, None, 0.8)
    before = _state(fed)
    db = _db()
    db.skip(4)
    fed._capture_fed(db, 64, 2)
    _assert_same(_state(fed), before)
    assert float(fed.opt.t) == 0.0 and int(db.device_pools(fed.net.device)[2].item()) == 4 and db.draw == 4
    got = fed.train_steps(db, 1, 64)
    host = _trainer("shipped", ckpt_weights, None, 0.8)
    twin = _db()
    twin.skip(4)
    x, y, _ = twin.get_training_set(64)
    assert got[0] == np.float32(host.train_step(x, y))
    _close(fed), _close(host)


def test_chunked_loss_log_and_mixing_with_train_step(ckpt_weights):
    pytest.importorskip("torch")
    # a loss log of 5 entries over 12 steps = 3 chunks
    whole, cut = _trainer("shipped", ckpt_weights, None, 0.8), _trainer("shipped", ckpt_weights, None, 0.8, loss_log_capacity=5)
    a, b = whole.train_steps(_db(), 12, 64), cut.train_steps(_db(), 12, 64)
    assert np.array_equal(a, b)
    _assert_same(_state(whole), _state(cut))
    # 6 steps device-fed, 3 host-fed on the twin's next three draws, 3 device-fed = 12 host-fed steps on the same batches
    twin = _db()
    batches = [twin.get_training_set(64) for _ in range(12)]
    host = _trainer("shipped", ckpt_weights, None, 0.8)
    want = _host_fed(host, batches)
    assert np.array_equal(a, want)
    mixed, db = _trainer("shipped", ckpt_weights, None, 0.8), _db()
    got = list(mixed.train_steps(db, 6, 64))
    got += [np.float32(mixed.train_step(x, y)) for x, y, _ in batches[6:9]]
    db.skip(3)
    got += list(mixed.train_steps(db, 3, 64))
    assert db.draw == 12
    assert np.array_equal(np.array(got, np.float32), want)
    _assert_same(_state(mixed), _state(host))
    for tr in (whole, cut, host, mixed):
        _close(tr)


def test_short_pool_raises_before_anything_runs(ckpt_weights):
    pytest.importorskip("torch")
    tr = _trainer("shipped", ckpt_weights, None, 0.8)
    db = DeviceExampleDb(*pools(31, 900), seed=1)
    with pytest.raises(ValueError):
        tr.train_steps(db, 3, 64)
    assert db.draw == 0 and float(tr.opt.t) == 0.0
    _close(tr)


def test_eager_trainer_falls_back_to_the_per_step_loop(ckpt_weights):
    """use_graph=False: get_training_set + train_step per step, the same batches and the same losses as the device-fed graph."""
    pytest.importorskip("torch")
    eager, fed = _trainer("shipped", ckpt_weights, None, 0.8, use_graph=False), _trainer("shipped", ckpt_weights, None, 0.8)
    da, db = _db(), _db()
    a, b = eager.train_steps(da, 4, 64), fed.train_steps(db, 4, 64)
    assert da.draw == db.draw == 4 and da._dev is None
    assert np.array_equal(a, b)
    _close(eager), _close(fed)


# ---------------------------------------------------------------------------------------------------- the loop
class _HostDb(object):
    """The twin's batches through today's per-step loop (not a DeviceExampleDb, so train_and_validate does not feed from the card)."""

    def __init__(self, db):
        self.db = db

    def get_training_set(self, size, ratio=2):
        return self.db.get_training_set(size, ratio)


def test_train_save_load_infer_loop_device_fed(hp, tmp_path, monkeypatch):
    """tests/test_gpu_pipeline.py::test_train_save_load_infer_loop's scenario (20 steps of 64, checkpoint, validation,
    load_network) with a DeviceExampleDb, beside the same run host-fed from its twin: equal model reports, equal validation
    reports, byte-identical ckpnt-20 data files."""
    pytest.importorskip("torch")
    from catfish_amd import neural_network
    val_dir = tmp_path / "val"
    val_dir.mkdir()
    squiggles = []
    for i in range(3):
        raw, lab = tv.synthetic_labelled_read(3000 + 35 * i, seed=50 + i)
        np.savez(val_dir / ("sq%d.npz" % i), raw=raw, base_labels=lab)
        squiggles.append(str(val_dir / ("sq%d.npz" % i)))
    out = {}
    for name in ("fed", "host"):
        (tmp_path / name).mkdir()
        monkeypatch.chdir(tmp_path / name)
        net = tv.build_model("ResNetRNN", save=True, **dict(hp, batch_size=64, train_seed=0))
        net.initialize_network(seed=4)
        db = ddb.synthetic_device_db(n_reads=2, read_len=12000, seed=2)
        acc = tv.train_and_validate(net, db if name == "fed" else _HostDb(db), 20 * 64, squiggles, 2000, net.model_path, 0, 856)
        assert 0.0 <= acc <= 1.0 and np.isfinite(net.train_loss) and db.draw == 20
        if name == "fed":
            assert net.train_losses.shape == (20,) and net.train_loss == float(net.train_losses[-1])
        report = open(net.model_path + ".txt").read()
        assert "Training on 1280 examples in 20 batches" in report and "Saved checkpoint at step 20" in report
        assert "Training set had 50.00% HPs" in report
        val_report = open(os.path.basename(net.model_path) + ".txt").read()
        assert "---NEXT ROUND OF VALIDATION---" in val_report
        data = open(os.path.join(net.model_path, "checkpoints", "ckpnt-20.data-00000-of-00001"), "rb").read()
        loaded = neural_network.load_network("ResNetRNN", net.model_path, checkpoint=20)
        x = np.random.default_rng(0).normal(0, 1.2, size=(40, 35, 1))
        got = loaded.infer(x)
        assert np.array_equal(got, net.infer(x))
        out[name] = (report, val_report, data, acc, got)
        loaded.engine.close(); net.engine.close()
    assert out["fed"][0] == out["host"][0]
    assert out["fed"][1] == out["host"][1]
    assert out["fed"][2] == out["host"][2]
    assert out["fed"][3] == out["host"][3] and np.array_equal(out["fed"][4], out["host"][4])
