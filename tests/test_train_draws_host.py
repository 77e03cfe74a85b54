"""Every network the reference's random search can draw resolves, through ``TrainMode.of`` alone, to a path that a GPU test steps.

``generate_random_hyperparameters`` draws type x ``layer_size`` {16 .. 256} x depth 1 .. 5 x ``layer_size_res`` {16 .. 256}; the trainer
adds ``native_training`` {None, True} and ``training_precision`` {fp32, bf16x3}.  A combination is mapped to a *cell* -- (kind,
type, is it 64 units, depth class of the conv stack, precision) -- and every cell that occurs must be the cell of a case in
``STEPPED_CELLS``, over which tests/test_train_draws_fp64.py parametrises: a cell nobody steps fails here, on the CPU.

No GPU, no native library, no torch.
"""
import itertools
from collections import namedtuple

import numpy as np

from catfish_amd import train_validate as tv
from catfish_amd.train_mode import KINDS, TUNED_MAX_BLOCKS, TrainMode

TYPES = ("RNN", "ResNetRNN")
SIZES = (16, 32, 64, 128, 256)
DEPTHS = (1, 2, 3, 4, 5)                                     # n_layers = randint(1, 6); the reference stores it under n_layers_res too
NATIVE = (None, True)
PRECISIONS = ("fp32", "bf16x3")

X3 = "precision='bf16x3' is a mode of the any-size training recurrences; "
# the one refusal in the search space: bf16x3 where no any-size recurrence trains -- the tuned step, and the 64-unit RNN that stays
# on torch without native_training (train_mode.py words both as the 64 / 32 geometry's)
REFUSED = X3 + "the tuned training kernels of the shipped 64 / 32 geometry are fp32"


def depth_class(network_type, depth):
    """Of the conv stack: "0" none (the RNN type), "1-4" what the tuned kernels have, "5" deeper."""
    return "0" if network_type == "RNN" else "1-4" if depth <= TUNED_MAX_BLOCKS else "5"


def resolve(network_type, layer_size, depth, layer_size_res, native, precision):
    """-> the cell (kind, type, 64 units?, depth class, precision), or the ValueError's text.  As ``Trainer`` sees the model that
    ``build_model(network_type, ...)`` makes on a card in float32."""
    blocks = depth if network_type == "ResNetRNN" else 0
    c = layer_size_res if blocks else 32
    try:
        mode = TrainMode.of(layer_size, c, blocks, "cuda", True, native, precision, dtype_name="torch.float32")
    except ValueError as e:
        return str(e)
    return (mode.kind, network_type, layer_size == 64, depth_class(network_type, depth), precision)


# name, the cell it stands for, then what builds it: build_model(network_type, layer_size=, n_layers=, [layer_size_res=, n_layers_res=
# n_layers, as the draw stores it]), native_training, training_precision, the other hyper-parameters (optimizer, rate, keep_prob).
Case = namedtuple("Case", "name cell network_type layer_size n_layers layer_size_res native precision optimizer learning_rate keep_prob")


def _case(name, kind, network_type, layer_size, n_layers, layer_size_res, native, precision="fp32", optimizer="Adam", learning_rate=1e-3,
          keep_prob=0.7):
    cell = (kind, network_type, layer_size == 64, depth_class(network_type, n_layers), precision)
    return Case(name, cell, network_type, layer_size, n_layers, layer_size_res, native, precision, optimizer, learning_rate, keep_prob)


def _others(prefix, network_type, layer_size, layer_size_res, depths):
    """The four any-size cells (autograd / step x fp32 / bf16x3) of one size and each depth class in ``depths``."""
    return tuple(_case("%s-x%d-%s-%s" % (prefix, depth, "step" if native else "autograd", precision),
                       "anysize_step" if native else "anysize_autograd", network_type, layer_size, depth, layer_size_res, native, precision)
                 for depth in depths for native in (None, True) for precision in PRECISIONS)


SEED_13 = {"learning_rate": 0.01, "optimizer_choice": "Adam", "layer_size": 64, "n_layers": 1, "batch_size": 512, "keep_prob": 0.7}
SEED_25 = {"learning_rate": 0.0001, "optimizer_choice": "Adam", "layer_size": 64, "n_layers": 5, "batch_size": 512, "keep_prob": 0.3,
           "layer_size_res": 32, "n_layers_res": 5}

STEPPED_CELLS = (
    # the cells at 64 units that the tuned kernels do not train: np.random.seed(13)'s RNN and seed(25)'s ResNetRNN, as drawn
    _case("rnn64-x1-step", "anysize_step", "RNN", 64, 1, None, True, learning_rate=0.01),
    _case("rnn64-x5-step", "anysize_step", "RNN", 64, 5, None, True),
    _case("rnn64-x2-step-bf16x3", "anysize_step", "RNN", 64, 2, None, True, "bf16x3"),
    _case("rnn64-x2-torch", "torch", "RNN", 64, 2, None, None),
    _case("res64-32-x5-autograd", "anysize_autograd", "ResNetRNN", 64, 5, 32, None, learning_rate=0.0001, keep_prob=0.3),
    _case("res64-32-x5-step", "anysize_step", "ResNetRNN", 64, 5, 32, True, learning_rate=0.0001, keep_prob=0.3),
    _case("res64-32-x5-autograd-bf16x3", "anysize_autograd", "ResNetRNN", 64, 5, 32, None, "bf16x3"),
    _case("res64-32-x5-step-bf16x3", "anysize_step", "ResNetRNN", 64, 5, 32, True, "bf16x3"),
    # the tuned step at its shallowest and its deepest stack
    _case("res64-32-x1-tuned", "tuned_step", "ResNetRNN", 64, 1, 32, None, optimizer="RMSProp"),
    _case("res64-32-x4-tuned", "tuned_step", "ResNetRNN", 64, 4, 32, None),
    # every other draw, at the smallest size of its cell: 64 units beside other channels, other units, the RNN type
    *_others("res64-16", "ResNetRNN", 64, 16, (1,)),           # (five blocks at 64 units is one cell whatever the channels: above)
    *_others("res16-16", "ResNetRNN", 16, 16, (1, 5)),
    *_others("rnn16", "RNN", 16, None, (1,)),
)


def hyperparameters(case, batch_size):
    """The keywords of ``build_model(case.network_type, **...)``, in the draw's own words."""
    hp = dict(batch_size=batch_size, optimizer_choice=case.optimizer, learning_rate=case.learning_rate, layer_size=case.layer_size,
              n_layers=case.n_layers, keep_prob=case.keep_prob)
    if case.network_type == "ResNetRNN":
        hp.update(layer_size_res=case.layer_size_res, n_layers_res=case.n_layers)
    if case.native is not None:
        hp["native_training"] = case.native
    if case.precision != "fp32":
        hp["training_precision"] = case.precision
    return hp


def _grid():
    return list(itertools.product(TYPES, SIZES, DEPTHS, SIZES, NATIVE, PRECISIONS))


def test_every_draw_resolves_to_a_kind_or_the_documented_refusal():
    grid = _grid()
    assert len(grid) == 2 * 5 * 5 * 5 * 2 * 2
    refused = []
    for combo in grid:
        got = resolve(*combo)
        if isinstance(got, str):
            assert got == REFUSED, combo
            refused.append(combo)
        else:
            assert got[0] in KINDS, combo
    # refused: bf16x3 at 64 / 32 with 1 .. 4 blocks, either way, and at the 64-unit RNN without native_training (any depth; the grid
    # carries a res size for the RNN type too, where it means nothing); nothing in fp32
    want = {c for c in grid if c[5] == "bf16x3" and c[1] == 64 and
            ((c[0] == "ResNetRNN" and c[3] == 32 and c[2] <= 4) or (c[0] == "RNN" and c[4] is None))}
    assert set(refused) == want and len(want) == 4 * 2 + 5 * 5


def search_space_cells():
    """{cell: one draw that lands in it} over the whole grid."""
    cells = {}
    for combo in _grid():
        got = resolve(*combo)
        if not isinstance(got, str):
            cells.setdefault(got, combo)
    return cells


def unstepped(cases):
    """{cell: a draw that lands in it} of the cells of the search space that no case of ``cases`` stands for."""
    stepped = {case.cell for case in cases}
    return {cell: combo for cell, combo in search_space_cells().items() if cell not in stepped}


def test_every_cell_of_the_search_space_is_stepped():
    missing = unstepped(STEPPED_CELLS)
    assert not missing, "cells no test steps (cell: a draw that lands in it): %r" % missing
    cells = search_space_cells()
    assert {case.cell for case in STEPPED_CELLS} == set(cells)        # and no case claims a cell that the search space does not have
    assert len(cells) == 24


def test_a_cell_taken_out_is_missed():
    """What the module is for: take a cell's cases out of ``STEPPED_CELLS`` and the check names that cell, and only it."""
    for gone in sorted({case.cell for case in STEPPED_CELLS}, key=repr):
        assert set(unstepped([case for case in STEPPED_CELLS if case.cell != gone])) == {gone}


def test_cases_are_in_the_cells_they_claim():
    names = [case.name for case in STEPPED_CELLS]
    assert len(set(names)) == len(names)
    for case in STEPPED_CELLS:
        got = resolve(case.network_type, case.layer_size, case.n_layers, case.layer_size_res or 32, case.native, case.precision)
        assert got == case.cell, case.name
        assert case.cell[0] in KINDS
        hp = hyperparameters(case, 64)
        assert hp.get("n_layers_res", case.n_layers) == case.n_layers


def test_the_two_seeds_draw_what_they_drew():
    """np.random.seed(13) -> the 64-unit RNN, seed(25) -> 64 / 32 with five blocks: the draws of the script test's two rows
    (tests/test_gpu_pipeline.py), so a change in the draw order shows here first."""
    np.random.seed(13)
    assert tv.generate_random_hyperparameters("RNN") == SEED_13
    np.random.seed(25)
    assert tv.generate_random_hyperparameters("ResNetRNN") == SEED_25
    assert resolve("RNN", 64, 1, 32, True, "fp32") == ("anysize_step", "RNN", True, "0", "fp32")
    assert resolve("RNN", 64, 1, 32, None, "fp32") == ("torch", "RNN", True, "0", "fp32")
    assert resolve("ResNetRNN", 64, 5, 32, None, "fp32") == ("anysize_autograd", "ResNetRNN", True, "5", "fp32")
    assert resolve("ResNetRNN", 64, 5, 32, True, "fp32") == ("anysize_step", "ResNetRNN", True, "5", "fp32")
    assert resolve("ResNetRNN", 64, 4, 32, None, "fp32") == ("tuned_step", "ResNetRNN", True, "1-4", "fp32")
    by_name = {case.name: case for case in STEPPED_CELLS}
    for name, drawn in (("rnn64-x1-step", SEED_13), ("res64-32-x5-autograd", SEED_25), ("res64-32-x5-step", SEED_25)):
        hp = hyperparameters(by_name[name], drawn["batch_size"])
        hp.pop("native_training", None)
        assert hp == drawn, name


def test_bounds_of_the_draws_parity_module_follow_from_its_profile():
    """Each bound of tests/test_train_draws_fp64.py is at most 4 x the largest yardstick that profiles/train_draws_fp64_parity.jsonl
    records for the quantity (float32 torch; for bf16x3 plus the scheme's float64 emulation), at most the older tests' bound, and
    not so far below (rounded down to three digits) that it is a different number."""
    import test_train_draws_fp64 as m
    want = m.bounds_from_profile()
    assert sorted(want) == sorted(m.BOUNDS) == sorted(m.OLDER_BOUNDS)
    for k, b in m.BOUNDS.items():
        assert 0.99 * want[k] <= b <= want[k], (k, b, want[k])
