"""bf16x3 on the any-size kernel family (csrc/generic.hpp: gen_dot_x3, v_mfma_f32_16x16x32_bf16 with the hi / lo operand
split): every geometry the family accepts -- ResNetRNN and plain RNN, 16 ... 256 units / channels, any depth -- keeps the
1e-4 gate against the fp64 oracle, is really computed in bf16x3 (not a silent fp32 fallback), does not depend on the call a
window travels in, and is reachable through the public surface (HipEngine, the model classes, load_network, the CLI tail)."""
import json
import os

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
from oracle.tolerances import GATE_MAX_ABS_DP

pytestmark = pytest.mark.gpu


def _weights(h, c, n_layers, n_layers_res, seed):
    return oracle.random_weights(seed=seed, layer_size=h, n_layers=n_layers, layer_size_res=max(c, 16), n_layers_res=n_layers_res)


def _engine(w, h, c, n_layers, n_layers_res, precision="bf16x3", max_windows_per_pass=16384):
    from catfish_amd.engine import HipEngine
    return HipEngine(w, layer_size=h, n_layers=n_layers, layer_size_res=max(c, 16), n_layers_res=n_layers_res, device=0,
                     max_windows_per_pass=max_windows_per_pass, precision=precision)


def _oracle_rows(x, w, n_layers, n_layers_res, idx):
    return oracle.forward(x[idx], w, np.float64, n_layers=n_layers, n_layers_res=n_layers_res).reshape(len(idx), 35)


# (units, channels (0: plain RNN), GRU layers, residual blocks, window counts, windows per pass).  The counts hit every launch
# shape of gen_run_pass: one wave per workgroup (1, 15, 17), a single 118-window read, several thousand windows (a full
# workgroup per tile group), more than 2 x CUs tiles in one pass (9000 windows), and multi-pass calls (3000 at 1024 per pass).
GEOMETRIES = [
    (16, 16, 2, 2, (1, 15, 17), 16384),
    (32, 64, 2, 1, (118,), 16384),
    (48, 48, 2, 1, (17, 3000), 1024),            # odd tile counts: 48 units and 48 channels padded to whole 32-deep blocks
    (64, 64, 2, 1, (15, 9000), 16384),           # 64-unit layers: formerly the tuned fp32 kernel's
    (64, 128, 1, 1, (118,), 16384),
    (64, 0, 1, 0, (17, 118), 16384),             # the plain RNN type at 64 units
    (64, 0, 2, 0, (3000,), 16384),
    (128, 64, 3, 2, (118, 4000), 16384),
    (128, 0, 2, 0, (1, 9000), 16384),
    (256, 128, 3, 2, (17, 3000), 16384),
    (256, 256, 5, 5, (15,), 16384),
]


@pytest.mark.parametrize("h,c,n_layers,n_layers_res,counts,per_pass", GEOMETRIES)
def test_bf16x3_any_size_matches_oracle(h, c, n_layers, n_layers_res, counts, per_pass):
    w = _weights(h, c, n_layers, n_layers_res, seed=300 + h + c + n_layers)
    rng = np.random.default_rng(h * 7 + c)
    eng = _engine(w, h, c, n_layers, n_layers_res, max_windows_per_pass=per_pass)
    try:
        for n in counts:
            x = rng.normal(0, 1.3, size=(n, 35)).astype(np.float32)
            got = eng.infer_host(x).reshape(n, 35)
            idx = np.arange(n) if n <= 4000 else np.unique(np.concatenate([np.arange(0, 300), np.arange(n - 300, n),
                                                                           rng.integers(0, n, size=600)]))
            err = np.abs(got[idx] - _oracle_rows(x, w, n_layers, n_layers_res, idx)).max()
            assert err < GATE_MAX_ABS_DP, (h, c, n_layers, n_layers_res, n, err)
        eng.check_error()
    finally:
        eng.close()


@pytest.mark.parametrize("h,c,n_layers,n_layers_res", [(128, 64, 3, 2), (64, 0, 2, 0)])
def test_bf16x3_any_size_is_not_fp32(h, c, n_layers, n_layers_res):
    """The same engine in fp32 and bf16x3 on a few thousand windows: both within the gate, NOT bit-equal (a silent fp32
    fallback would be), labels at the 0.5 threshold agree on at least 99.95 % of the samples."""
    w = _weights(h, c, n_layers, n_layers_res, seed=41 + h)
    x = np.random.default_rng(5).normal(0, 1.3, size=(3000, 35)).astype(np.float32)
    x3, f32 = _engine(w, h, c, n_layers, n_layers_res), _engine(w, h, c, n_layers, n_layers_res, precision="fp32")
    try:
        a, b = x3.infer_host(x), f32.infer_host(x)
    finally:
        x3.close(); f32.close()
    want = oracle.forward(x, w, np.float64, n_layers=n_layers, n_layers_res=n_layers_res)
    assert np.abs(a - want).max() < GATE_MAX_ABS_DP and np.abs(b - want).max() < GATE_MAX_ABS_DP
    assert not np.array_equal(a, b)
    assert np.mean((a >= 0.5) == (b >= 0.5)) >= 0.9995


def test_bf16x3_any_size_call_sizes_and_offsets_are_bit_identical():
    """Random sub-batches at random offsets reproduce, bit for bit, the slice of one full call (every launch shape)."""
    torch = pytest.importorskip("torch")
    h, c, n_layers, n_layers_res = 128, 64, 2, 1
    w = _weights(h, c, n_layers, n_layers_res, seed=77)
    n_all = 12000
    eng = _engine(w, h, c, n_layers, n_layers_res, max_windows_per_pass=10240)
    try:
        g = torch.Generator(device="cpu").manual_seed(13)
        x = torch.randn(n_all, 35, generator=g).mul_(1.4).cuda()
        full = eng.infer_device(x).view(n_all, 35).clone()
        rng = np.random.default_rng(14)
        sizes = np.unique(np.concatenate([np.exp(rng.uniform(0, np.log(n_all), size=14)).astype(int), [1, 15, 17, 118, 10241, n_all]]))
        for n in sizes:
            n = int(min(max(n, 1), n_all))
            o = int(rng.integers(0, n_all - n + 1))
            got = eng.infer_device(x[o:o + n].contiguous()).view(n, 35)
            assert torch.equal(got, full[o:o + n]), (n, o)
        eng.check_error()
    finally:
        eng.close()


@pytest.mark.parametrize("network_type,hpm", [
    ("ResNetRNN", dict(batch_size=64, optimizer_choice="Adam", learning_rate=0.001, layer_size=128, n_layers=2, keep_prob=0.7,
                       layer_size_res=64, n_layers_res=2)),
    ("RNN", dict(batch_size=64, optimizer_choice="RMSProp", learning_rate=0.001, layer_size=32, n_layers=1, keep_prob=0.8))])
def test_bf16x3_any_size_public_surface(network_type, hpm, tmp_path, monkeypatch):
    """precision="bf16x3" through the model classes: build, train a few steps (training is fp32), save, load_network in
    bf16x3, infer within the gate of the oracle on the saved weights; then the CLI tail on that model directory in bf16x3
    writes the same chunk documents as in fp32, except for reads with a probability within 1e-4 of the threshold."""
    pytest.importorskip("torch")
    import contextlib
    import io
    from catfish_amd import checkpoint, cli, neural_network, train_validate as tv
    monkeypatch.chdir(tmp_path)
    net = tv.build_model(network_type, save=True, precision="bf16x3", **dict(hpm, train_seed=0))
    net.initialize_network(seed=6)
    db = tv.synthetic_example_db(n_reads=2, read_len=12000, seed=3)
    for step in range(4):
        data, labels, _ = db.get_training_set(64, ratio=2)
        net.train_network(tv.reshape_input(data, 35, 1), tv.reshape_input(labels, 35, 1), step + 1)
    assert np.isfinite(net.train_loss)
    net.save_network_to_model_path(4)
    n_res = hpm.get("n_layers_res", 0)
    saved = checkpoint.read_inference_weights(os.path.join(net.model_path, "checkpoints"), "ckpnt-4")
    loaded = neural_network.load_network(network_type, net.model_path, checkpoint=4, precision="bf16x3")
    try:
        assert loaded.engine.precision == "bf16x3"
        x = np.random.default_rng(0).normal(0, 1.2, size=(300, 35, 1))
        got = loaded.infer(x)
        want = oracle.forward(x, saved, np.float64, n_layers=hpm["n_layers"], n_layers_res=n_res)
        assert np.abs(got - want).max() < GATE_MAX_ABS_DP
    finally:
        loaded.engine.close(); net.engine.close()
    reads = tmp_path / "reads"
    reads.mkdir()
    sigs = {}
    for i in range(6):
        d = oracle.synthetic_dac(1, 900 + 311 * i, seed=900 + i)[0]
        np.save(reads / ("read_%d.npy" % i), d)
        sigs["read_%d.npy" % i] = oracle.normalize_raw_signal(d)
    docs = {}
    for precision in ("fp32", "bf16x3"):
        out = tmp_path / ("out_" + precision)
        with contextlib.redirect_stdout(io.StringIO()):
            res = cli.run_pipeline(str(reads), str(out), chunk_size=300, network_type=network_type, network_path=net.model_path,
                                   checkpoint=4, device=0, precision=precision)
        assert res["reads"] == 6
        docs[precision] = [json.load(open(out / "TEMP" / name)) for name in ("hp_positions.json", "nonhp_positions.json")]
    for name, sig in sigs.items():
        windows, _ = oracle.pad_and_window(sig)
        scores = oracle.forward(windows, saved, np.float64, n_layers=hpm["n_layers"], n_layers_res=n_res)
        if np.abs(scores - 0.5).min() < 1e-4:
            continue                                                            # a label may flip at the threshold
        for a, b in zip(docs["fp32"], docs["bf16x3"]):
            assert a.get(name) == b.get(name), name


def test_bf16x3_shipped_geometry_on_the_any_size_path(ckpt_weights, monkeypatch):
    """CATFISH_GENERIC=1 sends the shipped 64 / 32 checkpoint through the any-size kernels: in bf16x3 they agree with the
    tuned bf16x3 engine within the gate, and both sit within the gate of the fp64 oracle."""
    from catfish_amd.engine import HipEngine
    x = np.random.default_rng(22).normal(0, 1.5, size=(1500, 35)).astype(np.float32)
    tuned = HipEngine(ckpt_weights, device=0, max_windows_per_pass=4096, precision="bf16x3")
    monkeypatch.setenv("CATFISH_DEBUG_KNOBS", "1")          # the library reads its A/B knobs only behind this switch
    monkeypatch.setenv("CATFISH_GENERIC", "1")
    try:
        generic = HipEngine(ckpt_weights, device=0, max_windows_per_pass=4096, precision="bf16x3")
    finally:
        monkeypatch.delenv("CATFISH_GENERIC")
    try:
        a, b = tuned.infer_host(x), generic.infer_host(x)
        want = oracle.forward(x, ckpt_weights, np.float64)
        assert np.abs(a - b).max() < GATE_MAX_ABS_DP
        assert np.abs(a - want).max() < GATE_MAX_ABS_DP and np.abs(b - want).max() < GATE_MAX_ABS_DP
        generic.check_error()
    finally:
        tuned.close(); generic.close()
