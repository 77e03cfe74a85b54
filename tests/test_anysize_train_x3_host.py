"""Training precision "bf16x3": what needs no GPU.  The kernels' tests are in tests/test_anysize_train_x3.py."""
import hashlib
import json

import numpy as np
import pytest

from oracle import catfish_oracle as oracle
import test_anysize_train_x3 as x3


def test_bounds_do_not_exceed_what_the_profile_gives():
    """``BOUNDS`` against profiles/anysize_train_x3_parity.jsonl: 4 x the largest (emulation + float32-torch) error of the
    quantity's section, never above the older bound; every asserted quantity has rows, every row has all three errors."""
    allowed = x3.bounds_from_profile()
    assert sorted(allowed) == sorted(x3.BOUNDS)
    for key, bound in x3.BOUNDS.items():
        assert 0 < bound <= allowed[key] <= x3.OLDER_BOUNDS[key], (key, bound, allowed[key])
    cases = set()
    with open(x3.PROFILE) as fh:
        for line in fh:
            row = json.loads(line)
            assert row["device"] and row["kernel"] >= 0 and row["torch_fp32"] >= 0 and row["emulation"] >= 0
            cases.add((row["section"], row["case"]))
    assert len([c for s, c in cases if s == "F"]) == len(x3.F_CASES) and len([c for s, c in cases if s == "H"]) == 3


def test_numpy_repack_reproduces_a_hand_worked_example():
    """One output tile, k = 1 padded to 4.  bf16 keeps 8 significant bits, ties go to the even neighbour:
        1 + 2^-8           -> hi 1.0       (0x3F80), lo  2^-8 (0x3B80)
        1 + 2^-7 + 2^-8    -> hi 1 + 2^-6  (0x3F82), lo -2^-8 (0xBB80)
        -0.0               -> hi -0.0      (0x8000), lo  0.0  (0x0000)     (a padded input row times the negative gate scale)
        3.0                -> hi 3.0       (0x4040), lo  0.0
    Tile b of pair 0 is past k, so elements 4..7 of both slots are zero; pair 1 (slots 2, 3) is padding: zero."""
    src = np.zeros((1, 1, 64, 4), np.float32)
    src[0, 0, :] = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -0.0, 3.0]
    got = x3.repack_x3_numpy(src, (1,))
    assert got.shape == (1, 4, 64, 8) and got.dtype == np.uint16
    assert (got[0, 0] == np.array([0x3F80, 0x3F82, 0x8000, 0x4040, 0, 0, 0, 0], np.uint16)).all()
    assert (got[0, 1] == np.array([0x3B80, 0xBB80, 0x0000, 0x0000, 0, 0, 0, 0], np.uint16)).all()
    assert not got[0, 2:].any()
    two = x3.repack_x3_numpy(np.concatenate([src, 2 * src], axis=1), (1, 1))          # two segments of one tile: each padded on its own
    assert two.shape == (1, 8, 64, 8) and (two[0, :4] == got[0]).all() and two[0, 4, 0, 0] == 0x4000 and not two[0, 6:].any()


def test_trainer_refuses_bf16x3_where_the_kernels_do_not_train():
    from catfish_amd.training import Trainer
    w = oracle.random_weights(seed=5, layer_size=16, n_layers=1, layer_size_res=16, n_layers_res=1)
    with pytest.raises(ValueError, match="cpu"):
        Trainer(w, 1, 1, "Adam", 1e-3, 1.0, device="cpu", precision="bf16x3")
    with pytest.raises(ValueError, match="unknown training precision"):
        Trainer(w, 1, 1, "Adam", 1e-3, 1.0, device="cpu", precision="bf16")
    with pytest.raises(ValueError, match="64 / 32"):
        Trainer(oracle.random_weights(seed=5), 3, 2, "Adam", 1e-3, 1.0, device="cpu", precision="bf16x3")
    tr = Trainer(w, 1, 1, "Adam", 1e-3, 1.0, device="cpu")                           # the default: as before
    assert tr.precision == "fp32" and tr.net.precision == "fp32" and not tr.anysize and tr.step_impl is None


def test_model_classes_carry_the_training_precision_beside_the_inference_one():
    from catfish_amd.train_validate import build_model
    hp = dict(batch_size=8, optimizer_choice="Adam", learning_rate=1e-3, layer_size=16, n_layers=1, keep_prob=1.0, layer_size_res=16,
              n_layers_res=1)
    m = build_model("ResNetRNN", save=False, **hp)
    assert m.training_precision == "fp32" and m.precision == "fp32"
    m = build_model("ResNetRNN", save=False, training_precision="bf16x3", **hp)
    assert m.training_precision == "bf16x3" and m.precision == "fp32"


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


PACK_MAPS_48_80 = "f616bd7133e151667757ccf7540611b99d46ec8d5b52440935e17903994863e5"
FLAT_PACK_MAP_48_32 = "0f53205b8451d1d307fc6c669c9d209b5a3bf6011405308cebfa61d51ca163aa"


def test_fp32_pack_maps_are_what_they_were():
    """The fp32 gather maps feed both precisions: ``pack_maps`` / ``flat_pack_map`` give what they gave before the mode existed
    (digests taken on the parent commit), and an ``AnySizeWalk`` carries the same maps whatever its precision."""
    from catfish_amd import _native as N
    from catfish_amd.anysize_train import pack_maps
    from catfish_amd.anysize_walk import AnySizeWalk, flat_layout, flat_pack_map
    assert _digest(*(t.numpy() for t in pack_maps(48, 80, "cpu"))) == PACK_MAPS_48_80
    _, _, layers, _, zero = flat_layout(48, 32, 2, 1)
    idx, scale, per_layer = flat_pack_map(48, layers, zero)
    assert _digest(idx, scale, np.asarray(per_layer)) == FLAT_PACK_MAP_48_32
    lib = N.lib()
    walks = [AnySizeWalk(lib, None, 48, 32, 2, 1), AnySizeWalk(lib, None, 48, 32, 2, 1, precision="fp32"),
             AnySizeWalk(lib, None, 48, 32, 2, 1, precision="bf16x3")]
    for w in walks:
        assert np.array_equal(w.pack_idx, idx) and np.array_equal(w.pack_scale, scale) and w.per_layer == per_layer
    assert walks[0].precision == "fp32" and walks[0].x3_layer == [] and walks[0].n_packed_x3 == 0
    # layer 0: 32 inputs (2 tiles -> 4) | 48 units (3 -> 4); layer 1: 96 inputs (6 -> 8); transposed: 3 -> 4 and 6 -> 8
    nw0, nw1, nt = 6 * 3 * (4 + 4) * 256, 6 * 3 * (8 + 4) * 256, 2 * 3 * (4 + 8) * 256
    assert walks[2].x3_layer == [(0, nw0), (nw0 + nt, nw0 + nt + nw1)] and walks[2].n_packed_x3 == nw0 + nw1 + 2 * nt
    with pytest.raises(ValueError, match="unknown training precision"):
        AnySizeWalk(lib, None, 48, 32, 2, 1, precision="bf16")
