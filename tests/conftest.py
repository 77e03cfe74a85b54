import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def ckpt_weights():
    """The 74 inference tensors of ckpnt-30000 (exported fixture, see make_network_golden.py)."""
    with np.load(os.path.join(GOLDEN, "ckpnt-30000-inference.npz")) as z:
        return {k: z[k] for k in z.files}


def _with_crc(raw, masked_crc):
    """``raw`` (bytearray, >= 4 bytes) with its last four bytes chosen so that the masked CRC-32C of the whole is ``masked_crc``.
    CRC-32C is affine over GF(2) in those four bytes: solve the 32 x 32 system by elimination."""
    from catfish_amd import checkpoint
    state = checkpoint.crc32c(bytes(raw[:-4]))
    crc_of = lambda x: checkpoint.crc32c(x.to_bytes(4, "little"), state)      # noqa: E731
    base = crc_of(0)
    rows = []                                             # (column combination, the input bits that make it), leading bits distinct
    for i in range(32):
        col, bits = crc_of(1 << i) ^ base, 1 << i
        for v, b in rows:
            if col ^ v < col:
                col, bits = col ^ v, bits ^ b
        if col:
            rows.append((col, bits))
            rows.sort(reverse=True)
    want, x = checkpoint.unmask_crc(masked_crc) ^ base, 0
    for v, b in rows:
        if want ^ v < want:
            want, x = want ^ v, x ^ b
    assert want == 0
    raw[-4:] = x.to_bytes(4, "little")
    return raw


@pytest.fixture(scope="session")
def ckpt_tensors(ckpt_weights):
    """All 190 entries of the reference's ckpnt-30000 bundle: the 74 inference tensors, and for each of the 116 optimizer
    slots (not stored) a seeded stand-in of its dtype and shape whose bytes carry the CRC-32C TensorFlow recorded for the real
    slot (ckpt_table.json).  The .index of a bundle written from them depends on names, dtypes, shapes, offsets, sizes and
    CRCs only: it must be TensorFlow's own, byte for byte."""
    with open(os.path.join(GOLDEN, "ckpt_table.json")) as fh:
        table = json.load(fh)
    rng = np.random.default_rng(190)
    tensors = dict(ckpt_weights)
    for e in table:
        if e["name"] not in tensors:
            assert e["dtype"] == 1                          # DT_FLOAT
            raw = _with_crc(bytearray(rng.integers(0, 256, size=e["size"], dtype=np.uint8).tobytes()), e["crc32c"])
            tensors[e["name"]] = np.frombuffer(bytes(raw), dtype="<f4").reshape(e["shape"])
    return tensors


@pytest.fixture(scope="session")
def reference_checkpoints(tmp_path_factory, ckpt_tensors):
    """A directory holding ckpnt-30000.{index,data-00000-of-00001} written from ``ckpt_tensors``: the .index is checked against
    the size and SHA-256 of the reference's own (tests/golden/ckpnt-30000-files.json), the data file against its size."""
    import hashlib
    from catfish_amd import checkpoint
    path = tmp_path_factory.mktemp("checkpoints")
    checkpoint.write_checkpoint(str(path / "ckpnt-30000"), ckpt_tensors)
    with open(os.path.join(GOLDEN, "ckpnt-30000-files.json")) as fh:
        files = json.load(fh)
    index = (path / "ckpnt-30000.index").read_bytes()
    assert (len(index), hashlib.sha256(index).hexdigest()) == (files["index"]["bytes"], files["index"]["sha256"])
    assert (path / "ckpnt-30000.data-00000-of-00001").stat().st_size == files["data-00000-of-00001"]["bytes"]
    return str(path)


@pytest.fixture(scope="session")
def golden_read():
    with np.load(os.path.join(GOLDEN, "golden_read_4096_seed0.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="session")
def graph_golden():
    """Outputs of the reference's own MetaGraphDef, interpreted in numpy (make_graph_golden.py)."""
    with np.load(os.path.join(GOLDEN, "graph_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="session")
def hp():
    return dict(batch_size=256, optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64,
                n_layers=3, keep_prob=0.8, layer_size_res=32, n_layers_res=2)
