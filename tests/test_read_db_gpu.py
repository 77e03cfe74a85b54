"""A DeviceReadDb with the real network on the card: Trainer.train_steps takes it through the per-step loop, on the batches and with
the losses of the device-fed loop over the same windows, and train_validate.main with CATFISH_DEVICE_DB=reads trains, checkpoints,
validates and writes its reports."""
import os

import numpy as np
import pytest

from catfish_amd import device_db as ddb, train_validate as tv
from catfish_amd.device_db import DeviceReadDb
from test_read_db_host import _twin_pools

pytestmark = pytest.mark.gpu


def _state(tr):
    out = dict(tr.net.numpy_weights())
    out.update({"slot:" + k: np.asarray(v) for k, v in tr.opt.state_tf().items()})
    return out


def test_train_steps_from_reads_equals_the_device_fed_steps_from_their_windows(ckpt_weights):
    """Five steps of 64 on the shipped geometry from a DeviceReadDb (every negative kept; host-fed, one step per batch) and from a
    DeviceExampleDb holding the same reads' windows (drawn and gathered on the card): the batches are the same float32 bits and the
    step is the same native step, so losses, variables and optimizer slots are bit-identical -- what tests/test_device_db_gpu.py
    establishes between the host-fed and the device-fed loop.  Nothing of the reads goes to the card."""
    pytest.importorskip("torch")
    from catfish_amd.training import Trainer
    reads = ddb.synthetic_device_read_db(n_reads=2, read_len=6000, seed=3)
    pools = _twin_pools(reads)
    a, b = (Trainer(ckpt_weights, 3, 2, "RMSProp", 1e-3, 0.8, seed=5) for _ in range(2))
    got = np.concatenate([a.train_steps(reads, 3, 64), a.train_steps(reads, 2, 64)])
    want = b.train_steps(pools, 5, 64)
    print("losses from reads", got, "from pools", want)
    assert got.dtype == np.float32 and np.isfinite(got).all() and np.array_equal(got, want)
    sa, sb = _state(a), _state(b)
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert reads.draw == 5 and reads._dev is None and a._fed is None and a.last_loss == float(got[-1])
    lx, ly = reads.last_batch()
    px, py = pools.last_batch()
    assert np.array_equal(lx.view(np.uint32), px.view(np.uint32)) and np.array_equal(ly, py)
    for tr in (a, b):
        if tr.engine is not None:
            tr.engine.close()


def test_train_validate_main_from_reads(tmp_path, monkeypatch):
    """CATFISH_DEVICE_DB=reads: twenty steps of the shipped network from NPZ reads with the reference's quota (as many negatives as
    positives per read), through the per-step loop, one checkpoint round; finite losses, both reports written."""
    pytest.importorskip("torch")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("CATFISH_DEVICE_DB", "reads")
    monkeypatch.setenv("CATFISH_SHIPPED_HPARAMS", "1")
    monkeypatch.delenv("CATFISH_DEVICE_NEG", raising=False)
    (tmp_path / "train").mkdir()
    (tmp_path / "val").mkdir()
    for i in range(2):
        raw, lab = tv.synthetic_labelled_read(12000, seed=70 + i)
        np.savez(tmp_path / "train" / ("t%d.npz" % i), raw=raw, base_labels=lab)
        raw, lab = tv.synthetic_labelled_read(3000, seed=80 + i)
        np.savez(tmp_path / "val" / ("v%d.npz" % i), raw=raw, base_labels=lab)
    seen, losses = {}, []
    real = tv.train_and_validate

    def spy(network, db, *args, **kw):
        seen["network"], seen["db"] = network, db
        step = network.train_network

        def train_network(x, y, n):
            step(x, y, n)
            losses.append(network.train_loss)

        network.train_network = train_network
        return real(network, db, *args, **kw)

    monkeypatch.setattr(tv, "train_and_validate", spy)
    tv.main(["train_validate.py", "ResNetRNN", str(tmp_path / "train"), str(20 * 256), str(tmp_path / "val"), "1050", "0"])
    db, net = seen["db"], seen["network"]
    assert isinstance(db, DeviceReadDb) and db.neg_per_read == "positives" and db.draw == 20 and db._dev is None
    assert 128 <= db.nb_neg <= db.nb_pos
    assert len(losses) == 20 and np.isfinite(losses).all() and np.isfinite(net.train_loss)
    report = open(net.model_path + ".txt").read()
    assert "Training on 5120 examples in 20 batches" in report and "Saved checkpoint at step 20" in report
    assert "Training set had 50.00% HPs" in report and "Finished training!" in report
    assert "---NEXT ROUND OF VALIDATION---" in open(os.path.basename(net.model_path) + ".txt").read()
    net.engine.close()
