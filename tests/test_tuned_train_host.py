"""tests/test_tuned_train_fp64.py can see what it is there for, shown on the CPU.

The GPU module holds the tuned conv stack (csrc/res_train.hpp) and the head (csrc/train_step.hpp) to float64 references written
out in torch.  Those references take ``departure=``, a named way of being subtly wrong that the older gates (float32 torch at
1e-5 / 2e-5, one maximum over all gradients) let through or never met.  Here every departure is evaluated in float64 on the
very inputs of a case of the GPU module (they come from seeded CPU generators), with the module's own error measures: each must
exceed the committed bound of the quantities it names by at least 10 x.  Also here: the given-stash reference against plain
float64 autograd, the share of pre-activations ``settle_stash`` moves, the size of the block outputs, the gates float32 takes on
a settled stash, and the float32 emulations of the kernels' summation order against plain sums."""
import pytest
import torch

import test_tuned_train_fp64 as m
from test_tuned_train_fp64 import T

F64 = torch.float64
THREE_WINDOWS, TWO_BLOCKS, TAIL_OF_ONE = (3, 1), (17, 2), (1025, 4)


def _clears(quantity, error, name):
    bound = m.BOUNDS[quantity]
    print("%s: %s %.3g, %.0f x its bound %.3g" % (name, quantity, error, error / bound, bound))
    assert error >= 10 * bound, (name, quantity, error, bound)


_CACHE = {}


def _stack(case):
    """(x, units, d_out, float64 z per unit, block outputs, settled stash, share moved, float64 gradients given the stash)"""
    if case not in _CACHE:
        x, units, d_out = m.stack_inputs(*case)
        zs, outs = m.stack_forward(x, units, F64)
        stash, moved = m.settle_stash(zs, units)
        _CACHE[case] = (x, units, d_out, zs, outs, stash, moved, m.stack_backward(x, units, stash, d_out, F64))
    return _CACHE[case]


def _grads_with(case, departure):
    x, units, d_out, _, _, stash, _, ref = _stack(case)
    return m.grad_errors(m.stack_backward(x, units, stash, d_out, F64, departure=departure), ref)


def test_cases_of_the_departures_are_cases_of_the_module():
    assert {THREE_WINDOWS, TWO_BLOCKS, TAIL_OF_ONE} <= set(m.S_CASES)
    assert m.workgroups(1024) == (1024, 1) and m.workgroups(1025) == (513, 2) and 513 % 4 == 1 and 1024 % 16 == 0
    assert {(11, "mixed"), (16, "mixed"), (17, "mixed")} <= set(m.T_CASES)
    assert set(m.CHAIN_TERM) <= set(m.BOUNDS) and sorted(m.BOUNDS) == sorted(m.OLDER_BOUNDS)
    assert all(b <= m.OLDER_BOUNDS[k] for k, b in m.BOUNDS.items())
    assert m.capped_windows(256) == 7499 and m.head_waves(7499, 256) == 2048 and m.head_waves(7483, 256) == 4 * 512
    assert [m.head_waves(n, 256) for n in (1, 11, 16, 17, 48)] == [8, 8, 8, 12, 16]


# ------------------------------------------------------------------------------------------------ S. the reference itself
@pytest.mark.parametrize("case", [THREE_WINDOWS, TWO_BLOCKS])
def test_given_stash_reference_is_plain_autograd_when_the_stash_is_the_forwards_own(case):
    """``stack_backward`` on the unrounded, unsettled float64 z of ``stack_forward`` against autograd through
    ``TorchResNetRNN(dtype=float64)``: every kernel, bias, gamma and beta gradient to 1e-12 of its tensor's maximum; the forward
    to 1e-12 as well."""
    from catfish_amd.native_train import res_unit_names
    from catfish_amd.training import TorchResNetRNN
    n, n_blocks = case
    x, units, d_out, zs, outs = _stack(case)[:5]
    names = res_unit_names(n_blocks)
    weights = {}
    for u, unit_names in zip(units, names):
        for k, name in zip(m.UNIT_KEYS, unit_names):
            weights[name] = u[k].numpy()
    net = TorchResNetRNN(weights, 3, n_blocks, dtype=F64)
    a = x.double()[:, None, :]
    for d in range(n_blocks):
        sc = net._conv_bn(a, 4 * d)
        o = torch.relu(net._conv_bn(a, 4 * d + 1))
        o = torch.relu(net._conv_bn(o, 4 * d + 2))
        o = torch.relu(net._conv_bn(o, 4 * d + 3))
        a = torch.relu(o + sc)
    out = a.permute(0, 2, 1)
    assert m._rel(outs[-1], out.detach()) <= 1e-12
    train = [net.params[k] for unit_names in names for k in unit_names[:4]]
    auto = torch.autograd.grad(out, train, d_out.double())
    mine = m.stack_backward(x, units, zs, d_out, F64)
    for j, g in enumerate(mine):
        for i, k in enumerate(m.GRAD_KEYS):
            want = auto[4 * j + i]
            assert m._rel(g[k].reshape(want.shape), want) <= 1e-12, (j, k)


@pytest.mark.parametrize("case", m.S_CASES)
def test_few_pre_activations_are_moved_and_the_block_outputs_stay_small(case):
    """``settle_stash`` moves fewer than 1 % of a case's z; afterwards float32 takes every gate of the backward as float64 does
    (the gated gradients vanish at the same elements); no block output exceeds 100; the special channels are in every unit."""
    x, units, d_out, zs, outs, stash, moved, _ = _stack(case)
    print("%s: %.3f %% moved, block maxima %s" % (case, 100 * moved, ["%.1f" % float(o.abs().max()) for o in outs]))
    assert moved < 0.01
    assert all(float(o.abs().max()) < 100.0 for o in outs)
    changed = sum(float((a != b.float()).sum()) for a, b in zip(stash, zs)) / sum(z.numel() for z in zs)
    assert abs(changed - moved) < 1e-12
    for u in units:
        s, t = m.bn_affine(u, F64)
        assert float(s[1]) == 0.0 and float(t[1]) == 0.25 and float(s[2]) < 0 and float(u["var"][3]) == 0.0 and 0.9 < float(s[3]) < 1.0
    for d in range(case[1]):
        for dt in (F64, torch.float32):
            y, pre = m.block_from_stash(stash[4 * d:4 * d + 4], units[4 * d:4 * d + 4], dt)
            assert float(pre.abs().min()) > 0.5 * m.GATE_MARGIN and all(float(v.abs().min()) > 0.5 * m.GATE_MARGIN for v in y[1:])
    ops64, ops32 = [], []
    m.stack_backward(x, units, stash, d_out, F64, operands=ops64)
    m.stack_backward(x, units, stash, d_out, torch.float32, operands=ops32)
    for a, b in zip(ops64, ops32):
        assert torch.equal(a[1] != 0, b[1] != 0)


# ------------------------------------------------------------------------------------------------ S. departures
def test_a_width_3_unit_that_reads_its_neighbour_window_shows_on_the_edge_steps_and_in_its_weight_gradient():
    x, units, d_out, zs, outs = _stack(THREE_WINDOWS)[:5]
    got_z, got_outs = m.stack_forward(x, units, F64, departure="neighbour_padding")
    edge = m._rel(got_z[2][:, m.EDGE], zs[2][:, m.EDGE])
    _clears("S.edge", edge, "neighbour padding, Z[2] on steps 0 and 34")
    e = m.forward_errors((got_z, got_outs[-1]), (zs, outs[-1]))
    assert e["edge"] >= edge
    _clears("S.z", e["z"], "neighbour padding")
    assert torch.equal(got_z[2][:, 1:T - 1], zs[2][:, 1:T - 1]) and torch.equal(got_z[1], zs[1])       # ... and nowhere else
    assert torch.equal(got_z[2][0, 0], zs[2][0, 0]) and not torch.equal(got_z[2][1, 0], zs[2][1, 0])   # the first window has no neighbour
    g = _grads_with(THREE_WINDOWS, "neighbour_padding")
    _clears("S.wgrad_wide", g["wgrad_wide"], "neighbour padding")
    assert g["wgrad_first"] == 0.0 and g["wgrad_point"] == 0.0


def test_epsilon_outside_the_root_shows_in_out_and_in_the_gamma_and_beta_gradients():
    x, units, d_out, zs, outs = _stack(THREE_WINDOWS)[:5]
    got_z, got_outs = m.stack_forward(x, units, F64, departure="eps_outside_root")
    e = m.forward_errors((got_z, got_outs[-1]), (zs, outs[-1]))
    for q in ("out", "out_window", "edge"):
        _clears("S." + q, e[q], "epsilon outside the root")
    g = _grads_with(THREE_WINDOWS, "eps_outside_root")
    for q in ("bn_first", "bn_point", "bn_wide"):
        _clears("S." + q, g[q], "epsilon outside the root")


def test_the_last_partial_dropped_from_the_reduction_shows_in_every_gradient():
    """1025 windows: 513 partials, thread group 0 adds the last one alone in its tail loop."""
    g = _grads_with(TAIL_OF_ONE, "last_partial_dropped")
    for q in sorted(g):
        _clears("S." + q, g[q], "last partial dropped")


def test_a_gamma_gradient_through_the_magnitude_of_gamma_shows_only_in_the_negative_gamma_channel():
    x, units, d_out, _, _, stash, _, ref = _stack(TWO_BLOCKS)
    got = m.stack_backward(x, units, stash, d_out, F64, departure="abs_gamma")
    e = m.grad_errors(got, ref)
    for q in ("bn_first", "bn_point", "bn_wide"):
        _clears("S." + q, e[q], "|gamma| for gamma")
    assert e["wgrad_first"] == 0.0 and e["wgrad_point"] == 0.0 and e["wgrad_wide"] == 0.0
    for a, b, u in zip(got, ref, units):
        differs = a["gamma"] != b["gamma"]
        assert bool(differs[2]) and int(differs.sum()) == 1 and float(u["gamma"][2]) < 0
    # the units of ``oracle.random_weights`` (gamma in [0.5, 1.5]) cannot show it
    from oracle import catfish_oracle as oracle
    assert all(float(v.min()) > 0 for k, v in oracle.random_weights(seed=31).items() if k.endswith("/gamma"))


# ------------------------------------------------------------------------------------------------ T. departures
def _head(n, departure):
    x, w, b, lab = m.head_inputs(n, "mixed")
    ref = m.head_ref(x, w, b, lab, F64)
    return m.head_errors(m.head_ref(x, w, b, lab, F64, departure=departure), ref)


def test_a_mean_over_the_padded_window_count_shows_at_11_windows_and_not_at_16():
    e = _head(11, "padded_count")
    for q in ("loss", "din", "wgrad"):
        _clears("T." + q, e[q], "mean over the padded count, 11 windows of 16")
    assert e["logits"] == 0.0
    assert all(v == 0.0 for v in _head(16, "padded_count").values())


@pytest.mark.parametrize("n", [11, 17])
def test_a_label_read_one_window_off_shows_in_the_loss_and_every_gradient(n):
    e = _head(n, "label_one_window_off")
    for q in ("loss", "din", "wgrad"):
        _clears("T." + q, e[q], "label one window off, %d windows" % n)
    assert e["logits"] == 0.0


def test_padding_windows_of_the_input_are_no_part_of_the_reference():
    x, w, b, lab = m.head_inputs(11, "mixed")
    assert float(x[11:].min()) > 0.99 * m.PADDING_VALUE and x.shape[0] == 16
    x2 = x.clone()
    x2[11:] = 0.0
    a, c = m.head_ref(x, w, b, lab, F64), m.head_ref(x2, w, b, lab, F64)
    assert all(torch.equal(a[k], c[k]) for k in a)
    assert a["din"].shape == (11, T, m.FEATURES) and a["logits"].shape == (11, T)


def test_the_saturated_case_passes_100_under_both_labels():
    x, w, b, lab = m.head_inputs(48, "mixed", reach=100.0)
    ref, yard = m.head_ref(x, w, b, lab, F64), m.head_ref(x, w, b, lab, torch.float32)
    s, one = ref["logits"].reshape(-1), lab.reshape(-1) > 0
    for sel in (one, ~one):
        assert float(s[sel].max()) > 100.0 and float(s[sel].min()) < -100.0
    assert all(bool(torch.isfinite(v).all()) for v in yard.values())
    e = m.head_errors(yard, ref)
    assert all(v <= m.OLDER_BOUNDS["T." + q] for q, v in e.items()), e


# ------------------------------------------------------------------------------------------------ the emulations of the summation order
def test_reduce_parts_adds_every_part_once():
    """``reduce_parts`` on integer-valued parts (every float32 sum exact) is the plain sum, at the part counts of the cases: the
    tail loop alone, whole rounds of 16, a tail of one."""
    gen = m._gen(40)
    for n_parts in (1, 2, 3, 8, 12, 13, 16, 17, 513, 1024, 2048):
        parts = torch.randint(-8, 9, (n_parts, 5), generator=gen).float()
        assert torch.equal(m.reduce_parts(parts), parts.sum(0)), n_parts


@pytest.mark.parametrize("case", [THREE_WINDOWS, TWO_BLOCKS])
def test_the_emulated_stack_sums_are_the_reference_sums_to_float32_rounding(case):
    x, units, d_out, _, _, stash, _, ref = _stack(case)
    ops = []
    m.stack_backward(x, units, stash, d_out, F64, operands=ops)
    e = m.grad_errors(m.stack_chain_grads(units, ops, case[0]), ref)
    print(e)
    assert all(0 < v < 2e-6 for v in e.values()), e


@pytest.mark.parametrize("n", [1, 11, 17, 48])
def test_the_emulated_head_sums_are_the_reference_sums_to_float32_rounding(n):
    x, w, b, lab = m.head_inputs(n, "mixed")
    ref = m.head_ref(x, w, b, lab, F64)
    e = m.head_chain_errors(m.head_chain(x, w, b, ref, m.head_waves(n, 256)), ref)
    print(e)
    assert all(0 <= v < 2e-6 for v in e.values()), e
