"""The launch shape of the any-size training recurrences (catfish_amd/csrc/anysize_launch.hpp), on the CPU.

``cf_gru_anysize_train_forward`` / ``_backward`` take waves per workgroup, grid, dynamic LDS bytes and ``h_via_y`` from that
header; ``cf_gru_anysize_train_shape`` reports them and tests/test_anysize_train_fp64.py asserts every case's regime through it.
Here the header itself, compiled with g++ through tests/native/anysize_launch_shim.cpp, is held to what the kernels of
csrc/generic.hpp need, for every layer size 16..256, 64 / 104 / 256 / 304 CUs and every tile count up to 4 n_cu + 9:

* waves in 1..max, every tile has a wave and no workgroup is empty;
* the LDS is waves x arrays x h16 KB (wave w's state sits at w * arrays * h16 * 64 f32x4) and at most 163 840 bytes;
* the forward reads h' back through y exactly when three arrays of eight waves do not fit;
* the class table of DESIGN.md "Any-size path" on 256 CUs, its three exact-limit launches included.

The inference launches of the same kernels (catfish_amd/csrc/anysize_infer_launch.hpp: what ``gen_build`` / ``gen_run_pass`` launch
and ``cf_anysize_infer_shape`` reports) go through the same shim: the class table and its borders 96 / 112 and 160 / 176, every
wave switch point of the one-tile kernel, the two-tile kernel's threshold of 2 n_cu tiles and its conditions, tuned layers.
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
    dll.shim_anysize_infer_shape.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_longlong)]
    dll.shim_anysize_infer_shape.restype = None

    def call(backward, h16, n_tiles, n_cu):
        out = (ctypes.c_longlong * 6)()
        dll.shim_anysize_shape(int(backward), h16, n_tiles, n_cu, out)
        return dict(zip(("waves", "max_waves", "grid_x", "lds_bytes", "arrays", "h_via_y"), list(out)))

    def infer(h16, n_tiles, n_cu, kbx=1, x3=False, one_tile_only=False, waves_cap=0, tuned=False):
        out = (ctypes.c_longlong * 10)()
        dll.shim_anysize_infer_shape(h16, int(x3), int(one_tile_only), waves_cap, int(tuned), kbx, n_tiles, n_cu, out)
        vals = list(out)
        return (dict(zip(("h_via_y", "gru_waves", "gru_lds", "gru2_waves", "gru2_lds"), vals[:5])),
                dict(zip(("kernel", "waves", "grid_x", "lds_bytes", "h_via_y"), vals[5:])))
    call.infer = infer
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


# ------------------------------------------------------------------------------------------------ the inference launches
# csrc/anysize_infer_launch.hpp: what gen_build / gen_run_pass (csrc/generic_host.hpp) launch and cf_anysize_infer_shape reports.
TUNED, ONE_TILE, TWO_TILE = 0, 1, 2
# layer size -> (h_via_y, most waves of the one-tile kernel, waves of the two-tile kernel in fp32)
INFER_CLASSES = {h: (0, 8, 0) for h in (16, 32, 48, 80, 96)}
INFER_CLASSES.update({64: (0, 8, 8), 128: (1, 8, 4), 192: (1, 4, 0), 256: (1, 4, 0)})
INFER_CLASSES.update({h: (1, 8, 0) for h in (112, 144, 160)})
INFER_CLASSES.update({h: (1, 4, 0) for h in (176, 208, 224, 240)})


def test_inference_class_table_and_its_borders(shape):
    """96 / 112: the third state array goes (h' through y); 160 / 176: eight waves of two arrays stop fitting, 160 itself takes
    the whole LDS.  The two-tile kernel: fp32, layer sizes that are a multiple of 64 and fit four arrays of 8 or 4 waves."""
    assert sorted(INFER_CLASSES) == list(range(16, 257, 16))
    for h, (via_y, waves, waves2) in INFER_CLASSES.items():
        h16 = h // 16
        c, _ = shape.infer(h16, 1, 256)
        arrays = 2 if via_y else 3
        assert (c["h_via_y"], c["gru_waves"], c["gru_lds"]) == (via_y, waves, waves * arrays * h16 * 1024), h
        assert (c["gru2_waves"], c["gru2_lds"]) == (waves2, waves2 * 4 * h16 * 1024), h
        assert c["gru_lds"] <= LDS_LIMIT and c["gru2_lds"] <= LDS_LIMIT, h
        assert via_y == int(8 * 3 * h16 * 1024 > LDS_LIMIT), h
        assert waves == 8 or 8 * arrays * h16 * 1024 > LDS_LIMIT, h
        for variant in (dict(x3=True), dict(one_tile_only=True)):
            c2, _ = shape.infer(h16, 1, 256, **variant)
            assert c2["gru2_waves"] == 0 and c2["gru2_lds"] == 0 and (c2["h_via_y"], c2["gru_waves"]) == (via_y, waves), (h, variant)
    at_limit = [h for h in INFER_CLASSES if shape.infer(h // 16, 1, 256)[0]["gru_lds"] == LDS_LIMIT]
    assert at_limit == [160]
    assert shape.infer(6, 1, 256)[0]["gru_lds"] == 147456 and shape.infer(7, 1, 256)[0]["gru_lds"] == 114688
    assert shape.infer(11, 1, 256)[0]["gru_lds"] == 90112
    assert [shape.infer(8, 1, 256, waves_cap=cap)[0]["gru_waves"] for cap in (0, 1, 3, 8, 9)] == [8, 1, 3, 8, 8]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_inference_one_tile_launch_at_every_wave_switch_point(shape, n_cu):
    """waves = ceil(2 tiles / n_cu) between 1 and the class's count: the last tile count of every wave count and the first of
    the next, for every layer size; every tile has a wave, no workgroup is empty, the LDS is that of the launched waves."""
    for h16 in range(1, 17):
        c, _ = shape.infer(h16, 1, n_cu)
        arrays = 2 if c["h_via_y"] else 3
        for w in range(1, 10):
            for tiles in (w * n_cu // 2, w * n_cu // 2 + 1):
                if tiles < 1:
                    continue
                _, s = shape.infer(h16, tiles, n_cu, kbx=1)
                key = (h16, tiles, s)
                assert s["kernel"] == ONE_TILE and s["h_via_y"] == c["h_via_y"], key
                assert s["waves"] == max(1, min(c["gru_waves"], -(-2 * tiles // n_cu))), key
                assert s["grid_x"] * s["waves"] >= tiles > (s["grid_x"] - 1) * s["waves"], key
                assert s["lds_bytes"] == s["waves"] * arrays * h16 * 1024 <= LDS_LIMIT, key
        if n_cu % 2 == 0:
            assert [shape.infer(h16, t, n_cu)[1]["waves"] for t in (n_cu // 2, n_cu // 2 + 1, n_cu, n_cu + 1)] == [1, 2, 2, 3]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_inference_two_tile_threshold_and_tuned_layers(shape, n_cu):
    """The two-tile kernel takes a layer from 2 n_cu tiles on, when the model has it and the layer's input is a multiple of 64
    features; always at its full wave count, one wave per pair of tiles.  A layer with a tuned pack is the tuned path's."""
    for h16, waves2 in ((4, 8), (8, 4)):
        for kbx in (4, 8, 16):
            _, below = shape.infer(h16, 2 * n_cu - 1, n_cu, kbx=kbx)
            assert below["kernel"] == ONE_TILE and below["waves"] == min(4, shape.infer(h16, 1, n_cu)[0]["gru_waves"])
            for tiles in (2 * n_cu, 2 * n_cu + 1, 4 * n_cu + 9):
                _, s = shape.infer(h16, tiles, n_cu, kbx=kbx)
                pairs = (tiles + 1) // 2
                assert (s["kernel"], s["waves"], s["lds_bytes"], s["h_via_y"]) == (TWO_TILE, waves2, 131072, 0), (h16, kbx, tiles, s)
                assert s["grid_x"] * waves2 >= pairs > (s["grid_x"] - 1) * waves2
        for kbx in (1, 2, 3, 5, 6):                                   # an input that is no multiple of 64 features
            assert shape.infer(h16, 2 * n_cu + 1, n_cu, kbx=kbx)[1]["kernel"] == ONE_TILE
        for variant in (dict(x3=True), dict(one_tile_only=True)):
            assert shape.infer(h16, 2 * n_cu + 1, n_cu, kbx=4, **variant)[1]["kernel"] == ONE_TILE
    for h16 in (12, 16):                                              # 192 and 256 units: four arrays fit no 4 waves
        assert shape.infer(h16, 4 * n_cu, n_cu, kbx=4)[1]["kernel"] == ONE_TILE
    for tiles in (1, n_cu, 2 * n_cu + 1):
        _, s = shape.infer(4, tiles, n_cu, kbx=8, tuned=True)
        assert s == dict(kernel=TUNED, waves=0, grid_x=0, lds_bytes=0, h_via_y=0)
