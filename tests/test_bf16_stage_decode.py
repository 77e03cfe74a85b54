"""csrc/bf16_stage.hpp on the CPU: the host decode of the bf16 / bf16x3 activation layout that ``cf_debug_stage`` uses in those
precisions, compiled with g++ through tests/native/bf16_stage_shim.cpp and held to a fragment buffer that is built here, in numpy,
from the layout as gru_bf16.hpp documents it:

  [tile32][t][kb < F / 16][part < NP][lane < 64][8 bf16]; lane l holds window l & 31 of its tile; element j of lane-half hh = l >> 5
  of k-block kb is feature 32 (kb >> 1) + 16 (kb & 1) + 8 (j >> 2) + 4 hh + (j & 3); NP = 2 stores hi = bf16(v) and lo = bf16(v - hi).
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 35
POISON = 0x7FC0              # a bf16 NaN: what the lanes of windows past the end hold here


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("bf16_stage") / "libbf16_stage.so")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "bf16_stage_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    dll = ctypes.CDLL(lib)
    dll.shim_stage_elems.restype = ctypes.c_longlong
    dll.shim_stage_elems.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    dll.shim_stage_decode.restype = None
    dll.shim_stage_decode.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return dll


def _bf16_bits(v):
    """float32 -> bf16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _fragments(parts, n_windows):
    """parts: NP arrays of bf16 bit patterns [n_windows, T, F] -> the fragment buffer of the documented layout, every lane of a
    window past the end poisoned."""
    feats, n_parts = parts[0].shape[2], len(parts)
    tiles = (n_windows + 31) // 32
    frag = np.full((tiles, T, feats // 16, n_parts, 64, 8), POISON, dtype=np.uint16)
    for kb in range(feats // 16):
        for hh in range(2):
            for j in range(8):
                f = 32 * (kb >> 1) + 16 * (kb & 1) + 8 * (j >> 2) + 4 * hh + (j & 3)
                for p in range(n_parts):
                    for w in range(n_windows):
                        frag[w >> 5, :, kb, p, 32 * hh + (w & 31), j] = parts[p][w, :, f]
    return frag


def test_every_feature_has_one_place(shim):
    for feats in (32, 128):
        seen = sorted(shim.shim_frag_feature(kb, hh, j) for kb in range(feats // 16) for hh in range(2) for j in range(8))
        assert seen == list(range(feats))


@pytest.mark.parametrize("n_windows", [1, 32, 33, 70])
@pytest.mark.parametrize("n_parts", [1, 2])
@pytest.mark.parametrize("feats", [32, 128])
def test_decode_returns_the_natural_array(shim, feats, n_parts, n_windows):
    """One and two parts, 32 and 128 features, whole tiles and a ragged last tile (1, 33 and 70 windows): the decode is the natural
    [n_windows, 35, F] array, bit for bit (hi + lo is exact in a float), and reads nothing of the windows past the end."""
    rng = np.random.default_rng(1000 * feats + 10 * n_windows + n_parts)
    v = (rng.normal(size=(n_windows, T, feats)) * np.exp(rng.normal(size=(n_windows, T, feats)))).astype(np.float32)
    hi = _bf16_bits(v)
    parts = [hi] if n_parts == 1 else [hi, _bf16_bits(v - _bf16_value(hi))]
    want = _bf16_value(parts[0]) if n_parts == 1 else _bf16_value(parts[0]) + _bf16_value(parts[1])
    if n_parts == 2:
        assert np.array_equal(want.astype(np.float64), _bf16_value(parts[0]).astype(np.float64) + _bf16_value(parts[1]))   # exact
        assert np.abs(want - v).max() <= 2.0 ** -15 * np.abs(v).max()
    frag = np.ascontiguousarray(_fragments(parts, n_windows))
    assert frag.size == shim.shim_stage_elems(n_windows, T, feats, n_parts)
    out = np.full((n_windows, T, feats), -7.0, dtype=np.float32)
    shim.shim_stage_decode(frag.ctypes.data, n_windows, T, feats, n_parts, out.ctypes.data)
    assert np.isfinite(out).all()
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
