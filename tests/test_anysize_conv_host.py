"""tests/test_anysize_conv_fp64.py can see what it is there for, shown on the CPU.

The GPU module holds each ``cf_gen_*`` kernel to a float64 reference written out in torch.  Those references take ``departure=``,
a named way of being subtly wrong that the whole-network tests at 2e-4 of a tensor's maximum let through.  Here every departure is
evaluated in float64 at the smallest case of the module that has it, on the very inputs of the GPU run (they come from seeded
CPU generators), with the module's own error measures: each must exceed the committed bound of the quantities it touches by at
least 10 x.  Also here: the share of pre-activations ``settle`` moves away from the ReLU threshold for every case and seed, and the
fragment layout of ``nat_to_frag`` against ``gt_fi`` of csrc/gen_train.hpp."""
import numpy as np
import pytest
import torch

import test_anysize_conv_fp64 as m
from test_anysize_conv_fp64 import T

F64 = torch.float64
SMALLEST, SMALLEST_K3, FIRST_WITH_CIN, FIRST_WITH_A_PARTIAL_CHUNK = (1, 1, 16, 16), (3, 1, 16, 16), (1, 16, 48, 16), (3, 16, 16, 48)


def _clears(quantity, error, name):
    bound = m.BOUNDS[quantity]
    print("%s: %s %.3g, %.0f x its bound %.3g" % (name, quantity, error, error / bound, bound))
    assert error >= 10 * bound, (name, quantity, error, bound)


def _forward(case, departure):
    kw = case[0]
    x, u, sc = m.conv_forward_inputs(*case)
    out = {}
    for relu, short in ((0, None), (1, sc)):
        ref = m.conv_forward_ref(x, u, kw, relu, short, F64)
        got = m.conv_forward_ref(x, u, kw, relu, short, F64, departure=departure)
        out[relu] = (m.forward_errors(got, ref), m._rel(got[1][:, m.EDGE], ref[1][:, m.EDGE]))
    return out


def _wgrad(case, departure):
    x, dz = m.conv_wgrad_inputs(*case)
    return m.wgrad_errors(m.conv_wgrad_ref(x, dz, case[0], F64, departure=departure), m.conv_wgrad_ref(x, dz, case[0], F64))["wgrad"]


def test_cases_of_the_departures_are_cases_of_the_module():
    assert set(m.CHAIN_TERM) <= set(m.BOUNDS) and all(b < m.OLDER_BOUNDS[k] / 5 for k, b in m.BOUNDS.items())
    assert {SMALLEST, SMALLEST_K3, FIRST_WITH_CIN, FIRST_WITH_A_PARTIAL_CHUNK} <= set(m.I_CASES)
    assert m.I_CASES[0] == SMALLEST and m.I_CASES[1] == SMALLEST_K3
    assert FIRST_WITH_CIN == next(c for c in m.I_CASES if c[1] > 1)
    assert FIRST_WITH_A_PARTIAL_CHUNK == next(c for c in m.I_CASES if c[3] > m.CHUNK_WINDOWS and c[3] % m.CHUNK_WINDOWS)
    assert (16, 16, 0) in m.J_CASES


@pytest.mark.parametrize("case", [SMALLEST, SMALLEST_K3])
def test_taps_shifted_by_one_show_in_z_y_and_the_weight_gradient(case):
    for relu, (e, _) in _forward(case, "taps_shifted").items():
        for q in ("z", "y", "y_window"):
            _clears("I." + q, e[q], "taps shifted, %s, relu %d" % (case, relu))
    _clears("I.wgrad", _wgrad(case, "taps_shifted"), "taps shifted, %s" % (case,))


def test_padding_that_reads_the_neighbouring_window_shows_on_the_edge_steps_and_in_the_weight_gradient():
    for relu, (e, edge) in _forward(SMALLEST_K3, "neighbour_padding").items():
        _clears("I.y", edge, "neighbour padding, steps 0 and 34, relu %d" % relu)
        assert e["y"] >= edge
    _clears("I.wgrad", _wgrad(SMALLEST_K3, "neighbour_padding"), "neighbour padding")
    x, u, _ = m.conv_forward_inputs(*SMALLEST_K3)                   # ... and nowhere else: the inner steps are untouched
    ref, got = (m.conv_forward_ref(x, u, 3, 1, None, F64, departure=d) for d in (None, "neighbour_padding"))
    assert torch.equal(ref[1][:, 1:T - 1], got[1][:, 1:T - 1]) and not torch.equal(ref[1][1:, 0], got[1][1:, 0])


def test_a_dropped_bias_row_shows_in_the_weight_gradient():
    _clears("I.wgrad", _wgrad(SMALLEST, "bias_dropped"), "bias row dropped")


def test_a_dropped_partial_chunk_shows_in_the_weight_gradient():
    _clears("I.wgrad", _wgrad(FIRST_WITH_A_PARTIAL_CHUNK, "last_chunk_dropped"), "last partial chunk dropped")


def test_epsilon_outside_the_root_shows_in_y_and_in_the_statistics_gradients():
    for relu, (e, _) in _forward(SMALLEST, "eps_outside_root").items():
        _clears("I.y", e["y"], "epsilon outside the root, relu %d" % relu)
        _clears("I.y_window", e["y_window"], "epsilon outside the root, relu %d" % relu)
        assert e["z"] == 0.0
    u, dgamma, dbeta = m.bn_stat_inputs(16)
    ref, got = m.bn_stat_ref(u, dgamma, dbeta, F64), m.bn_stat_ref(u, dgamma, dbeta, F64, departure="eps_outside_root")
    _clears("K.dstat", max(m.elementwise_error(got[0], ref[0]), m.elementwise_error(got[1], ref[1])), "epsilon outside the root")
    keep = torch.arange(16) != 3                                   # ... also without the channel of zero variance
    _clears("K.dstat", max(m.elementwise_error(got[i][keep], ref[i][keep]) for i in (0, 1)), "epsilon outside the root, variance > 0.5")


@pytest.mark.parametrize("departure,relu", [("gate_from_a", 1), ("negative_zero_on", 0), ("negative_zero_on", 1)])
def test_a_wrong_gate_shows_in_dz(departure, relu):
    g, mask, z, u, _ = m.bn_backward_inputs(*SMALLEST)
    ref = m.bn_backward_ref(g, mask, relu, z, u, F64)
    e = m.bn_errors(m.bn_backward_ref(g, mask, relu, z, u, F64, departure=departure), ref)
    for q in ("dz", "dz_window", "bn"):
        _clears("I." + q, e[q], "%s, relu %d" % (departure, relu))


def test_n_real_off_by_one_shows_in_the_loss_and_in_dl():
    features, npad, n_real = 16, 16, 16
    x, w, b, labels = m.head_inputs(features, npad, n_real)
    ref = m.head_ref(x, w, b, labels, n_real, F64)
    e = m.head_errors(m.head_ref(x, w, b, labels, n_real, F64, departure="n_real_off_by_one"), ref, n_real)
    for q in ("loss", "dl", "din", "wgrad"):
        _clears("J." + q, e[q], "n_real off by one")
    assert e["logits"] == 0.0


def test_add_applied_twice_shows_in_dx():
    kw = FIRST_WITH_CIN[0]
    dz, u, add = m.conv_dx_inputs(*FIRST_WITH_CIN)
    ref = m.conv_dx_ref(dz, u, kw, add, F64)
    _clears("I.dx", m._rel(m.conv_dx_ref(dz, u, kw, add, F64, departure="add_twice"), ref), "add applied twice")


def test_swapped_direction_offsets_show_in_the_signal_gradient():
    h, npad = 16, 16
    gen = m._gen(8, h, npad)                                         # the draws of test_signal_grad_of_the_plain_rnn_matches_float64
    params, da = m.gru_layer0_flat(gen, h), m._randn(gen, npad, T, 6 * h)
    ref = m.signal_grad_rnn_ref(params, da, h, F64)
    _clears("K.dsignal", m._rel(m.signal_grad_rnn_ref(params, da, h, F64, departure="directions_swapped"), ref), "directions swapped")


@pytest.mark.parametrize("case", m.I_CASES)
def test_few_pre_activations_are_moved_off_the_relu_threshold(case):
    """``settle`` moves fewer than 1 % of a case's z, none of them by more than 3e-3 / |s|, and afterwards float32 takes every
    gate as float64 does; the three special channels are in every case."""
    g, mask, z, u, moved = m.bn_backward_inputs(*case)
    print("%s: %.3f %% moved" % (case, 100 * moved))
    assert moved < 0.01
    gen = m._gen(3, *case)                                           # the same draws, before settle
    m.unit_params(gen, case[0], case[1], case[2], special=True)
    m._randn(gen, case[3], T, case[2]), m.mask_plane(gen, case[3], T, case[2])
    z0 = 1.5 * m._randn(gen, case[3], T, case[2])
    s, t = m.bn_affine(u, F64)
    assert float(((z - z0).double().abs() * s.abs()).max()) <= 3 * m.GATE_MARGIN + 1e-6
    assert abs(float((z != z0).double().mean()) - moved) < 1e-12
    for relu in (0, 1):
        v64, v32 = (m.bn_gated(g, mask, relu, z, u, dt) for dt in (F64, torch.float32))
        assert torch.equal(v64 != 0, v32 != 0)
    assert float(s[1]) == 0.0 and float(t[1]) == 0.25 and float(s[2]) < 0 and float(u["var"][3]) == 0.0


def test_mask_planes_hold_all_four_kinds_of_value():
    mask = m.mask_plane(m._gen(1), 16, T, 16)
    zeros = mask[mask == 0]
    share = lambda sel: float(sel.double().sum()) / mask.numel()      # noqa: E731
    assert 0.5 < share(mask > 0) < 0.6 and 0.1 < share(mask < 0) < 0.2
    assert 0.1 < float(torch.signbit(zeros).sum()) / mask.numel() < 0.2 and 0.1 < float((~torch.signbit(zeros)).sum()) / mask.numel() < 0.2


def test_nat_to_frag_places_elements_where_gt_fi_reads_them():
    """gt_fi(n, t, f, F16) = ((((n >> 4) 35 + t) F16 + (f >> 4)) 64 + (((f >> 2) & 3) 16 + (n & 15))) 4 + (f & 3), as written in
    csrc/gen_train.hpp: two tiles, 48 features."""
    from catfish_amd.native_train import frag_to_nat, nat_to_frag
    n_win, feats = 32, 48
    x = np.arange(n_win * T * feats, dtype=np.float32).reshape(n_win, T, feats)
    frag = nat_to_frag(torch.from_numpy(x))
    assert tuple(frag.shape) == (2, T, 3, 64, 4)
    n, t, f = np.meshgrid(np.arange(n_win), np.arange(T), np.arange(feats), indexing="ij")
    idx = ((((n >> 4) * T + t) * (feats // 16) + (f >> 4)) * 64 + (((f >> 2) & 3) * 16 + (n & 15))) * 4 + (f & 3)
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(x.size))
    assert np.array_equal(frag.numpy().reshape(-1)[idx], x)
    assert torch.equal(frag_to_nat(frag), torch.from_numpy(x))


def test_the_restated_dropout_hash_is_the_scalar_recipe():
    """``drop_scale_plane`` (vectorised) against the recipe of cf_drop_key / cf_drop_scale4 one element at a time in Python
    integers; the step count enters modulo 2^32."""
    m32 = 0xFFFFFFFF

    def fmix(v):
        v ^= v >> 16
        v = (v * 0x85EBCA6B) & m32
        v ^= v >> 13
        v = (v * 0xC2B2AE35) & m32
        return v ^ (v >> 16)

    for keep_prob, seed, layer, step in ((0.8, 0xC0FFEE11, 0, 0), (0.5, 7, 2, 2 ** 32 + 3), (0.999999, 1, 1, 7)):
        key = fmix(seed ^ fmix((0x9E3779B9 * (layer + 1) + (step & m32) * 0x85EBCA6B) & m32))
        thresh = int(min(np.float32(keep_prob) * np.float32(2.0 ** 32), np.float32(4294967040.0)))
        want = [np.float32(1.0) / np.float32(keep_prob) if fmix(e ^ key) < thresh else np.float32(0.0) for e in range(4 * 500)]
        got = m.drop_scale_plane(500, keep_prob, seed, layer, step)
        assert got.dtype == np.float32 and np.array_equal(got.reshape(-1), np.array(want, dtype=np.float32))
    assert np.array_equal(m.drop_scale_plane(64, 0.8, 5, 1, 3), m.drop_scale_plane(64, 0.8, 5, 1, 2 ** 32 + 3))
    assert not np.array_equal(m.drop_scale_plane(64, 0.8, 5, 1, 3), m.drop_scale_plane(64, 0.8, 5, 1, 4))
