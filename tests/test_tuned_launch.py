"""The launch plans of the tuned 64 / 32 path (catfish_amd/csrc/tuned_launch.hpp), on the CPU.

``run_pass``, the training entries, ``cf_launch_regimes``, the two ``*_workspace_floats`` queries and the workspace of
``cf_model_create`` take every kernel choice, wave count, grid, dynamic LDS size and chunk count from that header.  Here the header
itself, compiled with g++ through tests/native/tuned_launch_shim.cpp, is held to what the kernels need, on 64 / 104 / 256 / 304
CUs for every tile count from 1 to 4 n_cu + 9, and on 256 CUs for 1800..2100 tiles (the benchmark's 1888, 1024 and 2048 included):

* every tile has a wave, no workgroup is empty and no grid exceeds the bound the workspace is sized from;
* a plan that leaves raw per-lane dense partials has at most n_cu tiles (the raw buffer holds n_cu tiles);
* the dynamic LDS is at most 163 840 bytes;
* x-projection, dx and residual chunk counts lie in 1..35 and leave no empty chunk;
* the workspace-floats functions equal what the plan's launch writes;
* the figures the project has written down elsewhere (tests/test_gpu_parity.py, tests/test_gru_grid_balance.py).

The pack sizes are the kernels' (gru_pack_floats, gtb_pack_floats, gb_pack_bytes, res_pack_floats, rb_pack_bytes), restated below.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 163840
T = 35
N_CUS = (64, 104, 256, 304)
CAP_TILES = 8192                # max_windows_per_pass = 131 072: above every tile count of the sweep
RUN_ZERO = 4                    # CF_GRU_RUN_ZERO_PRODUCTS on top of the schedule in the balance word
XCH, BWD_XCH = (2 * 4 * 64 * 4 + 4 * 64) * 4, (3 * 4 * 64 * 4) * 4        # exchange areas of the cooperative kernels, bytes

KNOBS = ("coop", "waves", "gru_balance", "gru_gx", "gru_zero_products", "xproj_lds", "xproj_chunks", "hoist_tiles", "fuse",
         "bf16_waves", "bf16_wgs", "bf16_pipe", "res_fuse", "res_tpw", "res_chunks", "dx_chunks", "ablate_four_waves")


def gru_x_bytes(cin):
    return (cin // 4) * 3 * 256 * 4


def gru_pack_bytes(cin):         # x | h gates | h candidate | bias | dense
    return gru_x_bytes(cin) + (16 * 2 * 256 + 16 * 256 + 192 + 64) * 4


def gtb_pack_bytes(cin):
    return ((cin + 64) // 16 // 2) * 128 * 48 * 4


def gb_pack_bytes(cin, np):
    return ((cin // 16) * 6 + 16 + 8) * np * 1024 + 192 * 4 + 64 * 4


RES_FIRST, RES_OTHER = (4 * 1024 + 6 * 32) * 4, (6 * 1024 + 4 * 32) * 4


def rb_pack_bytes(first, np):
    return (4 if first else 6) * 2 * np * 1024 + (6 if first else 4) * 128


def gwg_partial_floats(cin):
    return (cin + 64 + 1) * 192


HEAD_PART = 132
RES_BF16_WAVES = 3


def whole(c):
    """c chunks of ceil(35 / c) steps leave no chunk empty."""
    return 1 <= c <= T and -(-T // -(-T // c)) == c


class Plans:
    def __init__(self, dll):
        self.dll = dll
        assert dll.shim_n_knobs() == len(KNOBS)
        self.unset = dll.shim_knob_unset()

    def _knobs(self, kn):
        assert set(kn) <= set(KNOBS), kn
        return (ctypes.c_int * len(KNOBS))(*[kn.get(name, 0 if name == "ablate_four_waves" else self.unset) for name in KNOBS])

    def _call(self, fn, n_out, names, *args, ctype=ctypes.c_int, **kn):
        out = (ctype * n_out)()
        getattr(self.dll, fn)(*args, self._knobs(kn), out)
        return dict(zip(names, list(out)))

    def bounds(self, n_cu, cap_tiles=CAP_TILES, **kn):
        out = (ctypes.c_longlong * 12)()
        self.dll.shim_bounds(n_cu, ctypes.c_longlong(cap_tiles), self._knobs(kn), out)
        return dict(zip(("hoist", "coop_max", "fuse_auto_min", "max_gx", "hand_bytes", "flag_bytes", "p_floats", "xp_floats", "fuse_mode",
                         "lds_limit", "T", "tile"), list(out)))

    def gru(self, n_tiles, n_cu, cin, hoist, has_hand=1, **kn):
        p = self._call("shim_gru_plan", 16, ("coop", "hoist", "waves", "gx", "per_dir", "wg_per_cu", "gx_one", "balance", "load", "lds", "raw",
                                             "_", "xp_lds_kernel", "xp_chunks", "xp_grid_x", "xp_lds"),
                       n_tiles, n_cu, cin, gru_pack_bytes(cin), gru_x_bytes(cin), hoist, has_hand, **kn)
        return p

    def gru_bf16(self, n_tiles32, n_cu, cin, np, **kn):
        return self._call("shim_gru_bf16_plan", 4, ("pipe", "waves", "gx", "lds"), n_tiles32, n_cu, np, gb_pack_bytes(cin, np), **kn)

    def res(self, n_tiles, n_cu, n_blocks=5, **kn):
        return self._call("shim_res_plan", 11, ("split", "chunks", "waves", "grid", "lds_first", "lds_other", "fused", "stack_chunks", "stack_waves",
                                                "stack_grid", "stack_lds"), n_tiles, n_cu, n_blocks, RES_FIRST, RES_OTHER, **kn)

    def res_bf16(self, n_tiles32, n_cu, np, n_blocks=5, **kn):
        return self._call("shim_res_bf16_plan", 10, ("fused", "np", "tpw", "chunks", "per_cu", "stack_grid", "stack_lds", "grid", "lds_first",
                                                     "lds_other"),
                          n_tiles32, n_cu, n_blocks, np, rb_pack_bytes(True, np), rb_pack_bytes(False, np), RES_BF16_WAVES, **kn)

    def train(self, backward, n_tiles, n_cu, cin, hoist, **kn):
        pack = gtb_pack_bytes(cin) if backward else gru_pack_bytes(cin)
        return self._call("shim_train_gru_plan", 11, ("coop", "hoist", "dx_chunks", "dx_grid_x", "waves", "gx", "lds", "xp_lds_kernel", "xp_chunks",
                                                      "xp_grid_x", "xp_lds"),
                          int(backward), n_tiles, n_cu, cin, pack, 0 if backward else gru_x_bytes(cin), hoist, **kn)

    def fused(self, n_tiles, n_cu, n_layers, pack_bytes):
        out = (ctypes.c_int * 4)()
        self.dll.shim_fused_plan(n_tiles, n_cu, n_layers, pack_bytes, out)
        return dict(zip(("groups", "grid", "threads", "lds"), list(out)))

    def wgrad(self, n_tiles, n_cu, cin):
        out = (ctypes.c_longlong * 3)()
        self.dll.shim_wgrad_plan(n_tiles, n_cu, gwg_partial_floats(cin), out)
        return dict(zip(("pairs_per_wg", "n_chunks", "workspace_floats"), list(out)))

    def head(self, n_tiles, n_cu):
        out = (ctypes.c_longlong * 3)()
        self.dll.shim_train_head_plan(ctypes.c_longlong(n_tiles), n_cu, HEAD_PART, out)
        return dict(zip(("waves", "grid", "workspace_floats"), list(out)))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    lib = str(tmp_path_factory.mktemp("tuned_launch") / "libtuned_launch.so")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-shared", "-fPIC", "-o", lib,
                            os.path.join(ROOT, "tests", "native", "tuned_launch_shim.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    return Plans(ctypes.CDLL(lib))


def _tile_counts(n_cu):
    return list(range(1, 4 * n_cu + 10)) + (list(range(1800, 2101)) if n_cu == 256 else [])


def _check_xproj(p, tiles, n_cu, cin, b, key):
    assert p["xp_lds_kernel"] == 1 and whole(p["xp_chunks"]) and p["xp_grid_x"] == tiles * p["xp_chunks"], key
    assert p["xp_lds"] == gru_x_bytes(cin) <= LDS_LIMIT, key
    assert tiles * T * 2 * 12 * 64 * 4 <= b["xp_floats"], key              # d_xp holds the projection of every hoisted call


@pytest.mark.parametrize("n_cu", N_CUS)
def test_fp32_bigru_inference_plans(plans, n_cu):
    b = plans.bounds(n_cu)
    assert b["hoist"] == max(1, 3 * n_cu // 16) and b["coop_max"] == n_cu and b["max_gx"] == 2 * (n_cu // 2)
    assert b["hand_bytes"] == 2 * b["max_gx"] * 8 * 4 * 64 * 16 and b["flag_bytes"] >= 2 * b["max_gx"] * 4 and b["flag_bytes"] % 16 == 0
    for tiles in _tile_counts(n_cu):
        for cin in (16, 32, 128):
            for has_hand in (1, 0):
                p = plans.gru(tiles, n_cu, cin, b["hoist"], has_hand)
                key = (n_cu, tiles, cin, has_hand, p)
                assert p["coop"] == int(tiles <= n_cu) == p["raw"], key           # raw partials only where the raw buffer holds them
                assert 1 <= p["gx"] <= b["max_gx"] and 1 <= p["waves"] <= 8 and p["lds"] <= LDS_LIMIT, key
                if p["coop"]:
                    assert p["waves"] == 4 and p["gx"] == min(tiles, n_cu // 2) and -(-tiles // p["gx"]) <= 2, key      # at most two rounds
                    assert p["lds"] == gru_pack_bytes(cin) + XCH, key
                    assert 2 * tiles * T * 256 <= b["p_floats"], key
                    assert p["hoist"] == int(cin >= 32 and tiles <= b["hoist"]), key
                    if p["hoist"]:
                        _check_xproj(p, tiles, n_cu, cin, b, key)
                    continue
                assert p["hoist"] == 0 and p["lds"] == gru_pack_bytes(cin) + 8 * 4, key
                assert p["waves"] == plans.dll.shim_pick_waves(2 * tiles, n_cu) and p["waves"] in (1, 2, 4, 8), key
                groups = -(-tiles // p["waves"])
                assert p["per_dir"] == (n_cu // 2) * (2 if gru_pack_bytes(cin) <= LDS_LIMIT // 2 else 1), key
                # every tile has a wave in one pass of the grid, or the grid is one of the two persistent ones; no workgroup is empty
                assert p["gx"] <= groups and (p["gx"] == groups or p["gx"] in (p["per_dir"], n_cu // 2)), key
                assert 2 * tiles * T * 16 <= plans.bounds(n_cu, cap_tiles=tiles)["p_floats"], key
                sched = p["balance"] & 3
                if not has_hand:
                    assert p["balance"] == RUN_ZERO and p["gx"] == min(groups, p["per_dir"]), key      # the kernel as it always was
                    continue
                assert p["balance"] == sched in (0, 1, 2) and p["load"] > 0, key                       # zero-state products skipped
                assert 2 * p["gx"] * 8 * 4 * 64 * 16 <= b["hand_bytes"] and 2 * p["gx"] * 4 <= b["flag_bytes"], key
                if sched == 2:
                    assert tiles >= p["gx"] * p["waves"], key        # grid-wide: no share shorter than a tile (cf_gru_gridwide_ok)


@pytest.mark.parametrize("n_cu", N_CUS)
def test_bf16_bigru_plans(plans, n_cu):
    for tiles in _tile_counts(n_cu):
        for cin in (32, 128):
            for np in (1, 2):
                for pipe in (1, 0):
                    p = plans.gru_bf16(tiles, n_cu, cin, np, **({} if pipe else {"bf16_pipe": 0}))
                    key = (n_cu, tiles, cin, np, p)
                    assert p["pipe"] == pipe and p["lds"] == gb_pack_bytes(cin, np) <= LDS_LIMIT, key
                    x3_pipe = np == 2 and pipe
                    assert p["waves"] == min(plans.dll.shim_pick_waves(2 * tiles, n_cu), 4 if x3_pipe else 8), key
                    cap = (n_cu // 2) * (2 if not x3_pipe and p["lds"] <= LDS_LIMIT // 2 else 1)     # x3 pipe: one workgroup per CU
                    assert p["gx"] == min(-(-tiles // p["waves"]), cap) >= 1, key


@pytest.mark.parametrize("n_cu", N_CUS)
def test_residual_stack_plans(plans, n_cu):
    for tiles in _tile_counts(n_cu):
        p = plans.res(tiles, n_cu)
        key = (n_cu, tiles, p)
        assert p["split"] == int(tiles <= n_cu) and p["fused"] == 1, key
        assert p["chunks"] == (4 if p["split"] else 1) and 1 <= p["waves"] <= 4 and (not p["split"] or p["waves"] == 4), key
        assert 1 <= p["grid"] <= 4 * n_cu and p["grid"] <= -(-tiles * p["chunks"] // p["waves"]), key
        assert p["lds_first"] == RES_FIRST + p["waves"] * 16 * T * 4 and p["lds_other"] == RES_OTHER, key
        assert whole(p["stack_chunks"]) and (p["split"] or p["stack_chunks"] == 1) and p["stack_waves"] == p["waves"], key
        assert 1 <= p["stack_grid"] <= 3 * n_cu and p["stack_grid"] <= -(-tiles * p["stack_chunks"] // p["stack_waves"]), key
        assert p["stack_lds"] == RES_FIRST + RES_OTHER + p["stack_waves"] * 16 * T * 4, key
        assert 3 * p["stack_lds"] <= LDS_LIMIT and max(p["lds_first"], p["lds_other"]) <= LDS_LIMIT, key     # three workgroups per CU fit
        for np in (1, 2):
            for tpw in ((1, 2) if np == 1 else (1,)):
                q = plans.res_bf16(tiles, n_cu, np, **({"res_tpw": 2} if tpw == 2 else {}))
                key = (n_cu, tiles, np, tpw, q)
                assert (q["fused"], q["np"], q["tpw"]) == (1, np, tpw) and whole(q["chunks"]), key
                assert q["stack_lds"] == rb_pack_bytes(True, np) + rb_pack_bytes(False, np) + 4 * tpw * 32 * T * 4, key
                assert 1 <= q["per_cu"] <= 3 and q["per_cu"] * q["stack_lds"] <= LDS_LIMIT, key
                assert 1 <= q["stack_grid"] <= n_cu * q["per_cu"] and q["stack_grid"] <= -(-(-(-tiles // tpw)) * q["chunks"] // 4), key
                assert 1 <= q["grid"] <= 4 * n_cu and q["grid"] <= -(-tiles // 4), key
                assert q["lds_first"] == rb_pack_bytes(True, np) + 4 * 32 * T * 4 <= LDS_LIMIT and q["lds_other"] == rb_pack_bytes(False, np), key
    assert plans.res(1, n_cu, n_blocks=1)["fused"] == 0 and plans.res(1, n_cu, res_fuse=0)["fused"] == 0
    assert plans.res_bf16(1, n_cu, 2, res_tpw=2)["tpw"] == 1         # two tiles per wave exist for one bf16 part only


@pytest.mark.parametrize("n_cu", N_CUS)
def test_training_plans_and_workspaces(plans, n_cu):
    b = plans.bounds(n_cu)
    for tiles in _tile_counts(n_cu):
        for cin in (32, 128):
            f, g = plans.train(False, tiles, n_cu, cin, b["hoist"]), plans.train(True, tiles, n_cu, cin, b["hoist"])
            key = (n_cu, tiles, cin, f, g)
            assert f["coop"] == g["coop"] == int(tiles <= n_cu) and f["hoist"] == g["hoist"] == int(tiles <= b["hoist"]), key
            assert (f["waves"], f["gx"]) == (g["waves"], g["gx"]) and 1 <= f["gx"] <= n_cu // 2 <= b["max_gx"], key
            if f["coop"]:
                assert f["waves"] == 4 and f["gx"] == min(tiles, n_cu // 2) and -(-tiles // f["gx"]) <= 2, key
                assert f["lds"] == gru_pack_bytes(cin) + XCH <= LDS_LIMIT and g["lds"] == gtb_pack_bytes(cin) + BWD_XCH <= LDS_LIMIT, key
                assert whole(g["dx_chunks"]), key
                if f["hoist"]:
                    _check_xproj(f, tiles, n_cu, cin, b, key)
                    assert g["dx_grid_x"] == tiles * g["dx_chunks"], key
            else:
                assert f["waves"] == plans.dll.shim_pick_waves(2 * tiles, n_cu) and f["gx"] == min(-(-tiles // f["waves"]), n_cu // 2), key
                assert f["lds"] == gru_pack_bytes(cin) <= LDS_LIMIT and g["lds"] == gtb_pack_bytes(cin) <= LDS_LIMIT, key
            w = plans.wgrad(tiles, n_cu, cin)
            assert w["pairs_per_wg"] >= 8 and (w["n_chunks"] - 1) * w["pairs_per_wg"] < tiles * T <= w["n_chunks"] * w["pairs_per_wg"], (key, w)
            assert w["workspace_floats"] == w["n_chunks"] * 2 * gwg_partial_floats(cin), (key, w)        # one partial per (chunk, direction)
        h = plans.head(tiles, n_cu)
        assert h["waves"] == 4 * h["grid"] and 1 <= h["grid"] <= 2 * n_cu and h["workspace_floats"] == h["waves"] * HEAD_PART, (tiles, h)
        assert h["grid"] == min(-(-tiles * T // 32), 2 * n_cu), (tiles, h)


def test_figures_written_down_elsewhere_on_256_cus(plans):
    b = plans.bounds(256)
    assert (b["lds_limit"], b["T"], b["tile"]) == (LDS_LIMIT, T, 16)
    # tests/test_gpu_parity.py: hoist_max = 16 (3 n_cu / 16), coop_max = 16 n_cu, fuse_auto_min = (8 * 6 (n_cu / 2) - 8) * 16 + 1
    assert 16 * b["hoist"] == 768 and 16 * b["coop_max"] == 4096 and b["fuse_auto_min"] == 98177 == (8 * 6 * (256 // 2) - 8) * 16 + 1
    assert b["fuse_mode"] == 2 and plans.bounds(256, fuse=0)["fuse_mode"] == 0 and plans.bounds(256, fuse=1)["fuse_mode"] == 1
    assert plans.dll.shim_fuse_now(2, 98177 // 16, 256) == 0 and plans.dll.shim_fuse_now(2, -(-98177 // 16), 256) == 1
    assert plans.bounds(256, cap_tiles=32)["hoist"] == 32 and plans.bounds(256, hoist_tiles=100)["hoist"] == 100
    f = plans.fused(8192, 256, 3, gru_pack_bytes(128))
    assert (f["groups"], f["grid"], f["threads"], f["lds"]) == (1024, 3 * 128 * 2, 512, gru_pack_bytes(128) + 16) and f["lds"] <= LDS_LIMIT
    # the training step at the reference's batch (256 windows): 18 dx chunks; DESIGN.md: 12 x-projection chunks for a single read
    assert plans.dll.shim_dx_chunks(16, 256, plans._knobs({})) == 18 and plans.train(True, 16, 256, 128, 48)["dx_chunks"] == 18
    assert plans.dll.shim_dx_chunks(48, 256, plans._knobs({})) == 7 and plans.dll.shim_dx_chunks(16, 256, plans._knobs({"dx_chunks": 5})) == 5
    assert plans.dll.shim_xproj_plan(8, 256, 128) == 12
    assert plans.gru(8, 256, 128, 48, xproj_chunks=8)["xp_chunks"] == 7 and plans.gru(8, 256, 128, 48, xproj_lds=0)["xp_chunks"] == 35
    assert all(plans.wgrad(t, 256, 128)["pairs_per_wg"] >= 8 for t in (1, 16, 48, 256, 1888))
    # tests/test_gru_grid_balance.py, DESIGN.md section 4: (schedule, workgroups per direction, worst SIMD load)
    def choice(tiles, cin, **kn):
        p = plans.gru(tiles, 256, cin, 48, **kn)
        assert p["coop"] == 0 and p["waves"] == 8
        return (p["balance"] & 3, p["gx"], p["load"])
    for tiles in (1887, 1888, 1889):
        assert choice(tiles, 32) == choice(tiles, 128) == (2, 128, 130)         # the grid-wide schedule, 130 steps on the worst SIMD
    for tiles, load in ((1024, 70), (2048, 140)):                               # divides evenly: round-robin, what it ran
        assert choice(tiles, 128) == (0, 128, load)
    assert choice(1024, 32) == (0, 128, 70) and choice(2048, 32) == (0, 256, 140)       # first layer: 128 groups at 1024, two per CU at 2048
    assert choice(1025, 128) == (2, 128, 71) and choice(4096 + 5, 32)[0] == 2
    p = plans.gru(257, 256, 128, 48)
    assert (p["waves"], p["balance"], p["gx"], p["load"]) == (4, 0, 65, 35)            # 4097 windows: 3 or 4 tiles on 4 waves
    assert choice(1888, 128, gru_balance=0) == (0, 128, 140) and choice(1888, 128, gru_balance=1) == (1, 128, 132)
    assert choice(1888, 128, gru_balance=2) == (1, 128, 132) and choice(1888, 128, gru_balance=3) == (2, 128, 130)
    # the first layer's usual grid at 1888 tiles is 236 workgroups of 8 whole tiles (two per CU): balanced there gains nothing
    assert choice(1888, 32, gru_balance=0) == (0, 236, 140) and choice(1888, 32, gru_balance=1) == (1, 236, 140)
    assert choice(1888, 32, gru_balance=2) == (1, 128, 132) and choice(1888, 32, gru_balance=3) == (2, 128, 130)
    assert choice(2048, 128, gru_balance=3) == (2, 128, 140)
    assert plans.gru(1888, 256, 128, 48, gru_zero_products=1)["balance"] == 2 | RUN_ZERO
    # CATFISH_GRU_GX: that many 8-wave workgroups whatever the size of the call, never the cooperative kernel, no second grid
    assert choice(40, 128, gru_gx=2, gru_balance=3) == (2, 2, 176) and choice(15, 128, gru_gx=2, gru_balance=3)[0] != 2
    for gx in (2, 3, 5):
        for tiles in range(16 * gx, 16 * gx + 12):
            for cin in (32, 128):
                p = plans.gru(tiles, 256, cin, 48, gru_gx=gx, gru_balance=3)
                assert (p["coop"], p["raw"], p["waves"], p["gx"], p["gx_one"], p["balance"]) == (0, 0, 8, gx, 0, 2), (gx, tiles, p)
    assert plans.gru(8192, 256, 32, 48, gru_gx=100000)["gx"] == 256 and plans.gru(16, 256, 32, 48, gru_gx=0)["coop"] == 1
    # CATFISH_COOP / CATFISH_WAVES and the four-wave ablation build
    assert plans.gru(16, 256, 32, 48, coop=0)["coop"] == 0 and plans.gru(257, 256, 32, 48, coop=1)["coop"] == 0
    assert plans.gru(16, 256, 32, 48, ablate_four_waves=1)["coop"] == 0 and plans.gru(1888, 256, 32, 48, ablate_four_waves=1)["waves"] == 4
    assert plans.gru(1888, 256, 128, 48, waves=2)["waves"] == 2 and plans.gru(1888, 256, 128, 48, waves=99)["waves"] == 8
    # the x3 pipe kernel: four waves, one workgroup per CU; CATFISH_BF16_WGS / CATFISH_BF16_WAVES
    assert plans.gru_bf16(944, 256, 128, 2) == dict(pipe=1, waves=4, gx=128, lds=gb_pack_bytes(128, 2))
    assert plans.gru_bf16(944, 256, 32, 1) == dict(pipe=1, waves=8, gx=118, lds=gb_pack_bytes(32, 1))
    assert plans.gru_bf16(944, 256, 128, 1, bf16_wgs=64, bf16_waves=4)["gx"] == 64 and plans.gru_bf16(944, 256, 128, 2, bf16_wgs=64)["gx"] == 64
