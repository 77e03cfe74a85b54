"""The launch shape of the any-size training recurrences (catfish_amd/csrc/anysize_launch.hpp), on the CPU.

``cf_gru_anysize_train_forward`` / ``_backward`` take waves per workgroup, grid, dynamic LDS bytes and ``h_via_y`` from that
header; ``cf_gru_anysize_train_shape`` reports them and tests/test_anysize_train_fp64.py asserts every case's regime through it.
Here the header itself, compiled with g++ through tests/native/anysize_launch_shim.cpp, is held to what the kernels of
csrc/generic.hpp need, for every layer size 16..256, 64 / 104 / 256 / 304 CUs and every tile count up to 4 n_cu + 9:

* waves in 1..max, every tile has a wave and no workgroup is empty;
* the LDS is waves x arrays x h16 KB (wave w's state sits at w * arrays * h16 * 64 f32x4) and at most 163 840 bytes;
* the forward reads h' back through y exactly when three arrays of eight waves do not fit;
* the class table of DESIGN.md "Any-size path" on 256 CUs, its three exact-limit launches included.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 163840
N_CUS = (64, 104, 256, 304)


@pytest.fixture(scope="module")
def shape(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("anysize_launch") / "libanysize_launch.so")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "anysize_launch_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    dll = ctypes.CDLL(lib)
    dll.shim_anysize_shape.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    dll.shim_anysize_shape.restype = None

    def call(backward, h16, n_tiles, n_cu):
        out = (ctypes.c_longlong * 6)()
        dll.shim_anysize_shape(int(backward), h16, n_tiles, n_cu, out)
        return dict(zip(("waves", "max_waves", "grid_x", "lds_bytes", "arrays", "h_via_y"), list(out)))
    return call


@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("backward", [0, 1])
def test_every_tile_has_a_wave_and_the_state_fits_the_lds(shape, backward, n_cu):
    for h16 in range(1, 17):
        three_fit = 8 * 3 * h16 * 1024 <= LDS_LIMIT
        seen = set()
        for tiles in range(1, 4 * n_cu + 10):
            s = shape(backward, h16, tiles, n_cu)
            key = (h16, tiles, s)
            assert 1 <= s["waves"] <= s["max_waves"] and s["max_waves"] in (1, 2, 4, 8), key
            assert s["grid_x"] * s["waves"] >= tiles > (s["grid_x"] - 1) * s["waves"], key
            assert s["lds_bytes"] == s["waves"] * s["arrays"] * h16 * 1024 <= LDS_LIMIT, key
            # max_waves is the largest power of two that fits, and twice as many would not (or is 8)
            assert s["max_waves"] * s["arrays"] * h16 * 1024 <= LDS_LIMIT, key
            assert s["max_waves"] == 8 or 2 * s["max_waves"] * s["arrays"] * h16 * 1024 > LDS_LIMIT, key
            # enough waves to give every CU two tiles, as far as they fit
            assert s["waves"] == max(1, min(s["max_waves"], -(-2 * tiles // n_cu))), key
            if backward:
                assert s["arrays"] == 4 and s["h_via_y"] == 0, key
            else:
                assert s["h_via_y"] == (0 if three_fit else 1) and s["arrays"] == (3 if three_fit else 2), key
            seen.add(s["waves"])
        assert seen == set(range(1, s["max_waves"] + 1)), (h16, seen)        # 4 n_cu + 9 tiles reach every count, 3 / 5 / 6 / 7 too


# layer size -> (forward arrays, forward max waves, backward max waves): the table of DESIGN.md "Any-size path"
CLASSES = {h: (3, 8, 8) for h in (16, 32, 48, 64, 80)}
CLASSES.update({96: (3, 8, 4)})
CLASSES.update({h: (2, 8, 4) for h in (112, 128, 144, 160)})
CLASSES.update({h: (2, 4, 2) for h in (176, 192, 208, 224, 240, 256)})


def test_class_table_on_256_cus_and_its_exact_limit_launches(shape):
    assert sorted(CLASSES) == list(range(16, 257, 16))
    full = 4 * 256          # tiles at which every class has reached its largest wave count (8 = ceil(2 * 1024 / 256))
    for h, (arrays, fwd_max, bwd_max) in CLASSES.items():
        f, b = shape(0, h // 16, full, 256), shape(1, h // 16, full, 256)
        assert (f["arrays"], f["h_via_y"], f["max_waves"], f["waves"]) == (arrays, int(arrays == 2), fwd_max, fwd_max), h
        assert (b["arrays"], b["max_waves"], b["waves"]) == (4, bwd_max, bwd_max), h
    at_limit = {(h, back) for h in CLASSES for back in (0, 1) if shape(back, h // 16, full, 256)["lds_bytes"] == LDS_LIMIT}
    assert at_limit == {(80, 1), (160, 0), (160, 1)}
    assert shape(1, 5, full, 256)["waves"] == 8 and shape(0, 10, full, 256)["waves"] == 8 and shape(1, 10, full, 256)["waves"] == 4


def test_wave_count_follows_tiles_per_cu_on_256_cus(shape):
    """The tile counts tests/test_anysize_train_fp64.py uses, C = 256: C/2 + 1 tiles -> 2 waves, C + 1 -> 3, 3C/2 + 1 -> 4,
    2C + 1 -> 5, 7C/2 + 1 -> 8; each leaves the last workgroup partly empty at the size's own wave count."""
    for tiles, want in ((1, 1), (3, 1), (129, 2), (257, 3), (385, 4), (513, 5), (897, 8)):
        s = shape(0, 1, tiles, 256)
        assert s["waves"] == want, (tiles, s)
        assert want == 1 or s["grid_x"] * s["waves"] > tiles, (tiles, s)
