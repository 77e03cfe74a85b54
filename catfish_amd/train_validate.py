"""Training / validation driver -- the reference's networks/train_validate.py on the MI355X model objects.

Same function names, arguments and report text as the reference (``train_and_validate``
networks/train_validate.py:114-185, ``validate`` :188-295, ``padding`` :50-63, ``reshape_input`` :15-31,
``build_model`` :34-48, ``generate_random_hyperparameters`` :66-111); the network methods it calls
(``train_network``, ``test_network``, the checkpoint save) run on the HIP training / inference kernels.

The reference samples its training windows from a ZODB database (``ExampleDb.get_training_set``,
networks/trainingDB/ExampleDb.py:50-83), which is outside this path; the two databases here
expose the same ``get_training_set(size, ratio=2) -> (x_out, y_out, pos_count)`` over NPZ reads
(``raw`` + ``base_labels``, networks/reader.py:11-23) or synthetic squiggles, with the sampler's shape kept:
``size // ratio`` all-positive windows + the rest all-negative, shuffled, every window's labels uniform
(TrainingRead.get_pos / get_neg, networks/trainingDB/TrainingRead.py:226-257).
"""
from __future__ import annotations

import datetime
import json
import os
import random
from collections import namedtuple

import numpy as np

from . import metrics
from .device_validation import (BASE_CLASSES, BORDER_REACH, MAX_BASES, RUN_SCORE_SHIFT, RUN_STATES, check_border_reach, check_max_bases,
                                curve_thresholds, curves_from_histogram, run_base_rates, run_border_summary, run_score_summary,
                                run_state_rates, split_run_borders)
from .neural_network import build_model as _build_model
from .validation_round import CHECK_ORDER, OPTIONS


def reshape_input(data, window, n_inputs):
    """networks/train_validate.py:15-31: ``[-1, window, n_inputs]`` view of the data.  Data that does not fill whole
    windows is NOT an error there: two lengths are printed and the data comes back as it was; same here."""
    try:
        flat = np.asarray(data)
        fits = flat.size % (window * n_inputs) == 0
    except ValueError:                                     # ragged rows
        fits = False
    if fits:
        return flat.reshape(-1, window, n_inputs)
    for what in (data, data[0]):
        print(len(what))
    return data


def build_model(network_type, **kwargs):
    """networks/train_validate.py:34-48 (``save=True`` is passed through as a keyword, :323)."""
    return _build_model(network_type, saving=kwargs.pop("save", False), **kwargs)


def padding(data, window=35, n_input=1):
    """networks/train_validate.py:51-64: integer zeros up to the next multiple of the window -> (windows, how many).
    Unlike catfish/infer.py:32-36 an exact multiple gets NO extra window here."""
    tail = -len(data) % window
    if tail:
        data = np.hstack((data, np.zeros(tail, dtype=np.int64)))
    return reshape_input(data, window, n_input), tail


def generate_random_hyperparameters(network_type, learning_rate_min=-4, learning_rate_max=0,
                                    optimizer_list=("Adam", "RMSProp"), layer_size_list=(16, 32, 64, 128, 256),
                                    n_layers_min=1, n_layers_max=6, batch_size_list=(128, 256, 512),
                                    dropout_min=0.2, dropout_max=0.8, n_layers_res_min=1, n_layers_res_max=12,
                                    size_layers_res_list=(16, 32, 64, 128, 256)):
    """networks/train_validate.py:66-111: one random-search draw from numpy's GLOBAL generator, in the reference's
    call order (so a seeded run draws the same network): learning-rate exponent, optimizer, layer size, depth, batch
    size, keep probability, and for ResNetRNN a residual depth that is drawn and then DROPPED -- the reference stores
    ``n_layers`` under ``n_layers_res`` (:109) -- and the residual width.

    Every draw builds and takes a step (tests/test_train_draws_host.py enumerates the grid): ``layer_size`` 64 / ``layer_size_res``
    32 at depths 1 .. 4 trains natively on the tuned HIP kernels; every other ResNetRNN draw -- other sizes, and 64 / 32 at depth 5,
    which the tuned conv-stack kernels do not have -- infers on the any-size HIP kernels (csrc/generic.hpp) and trains through torch
    autograd with the recurrence on the same kernel family (anysize_train.py), or natively on it with ``native_training=True``.
    The RNN type does the same, except that at 64 units it trains on plain torch unless ``native_training=True`` is given.
    """
    rs = np.random
    plan = [("learning_rate", lambda: float(10 ** rs.randint(learning_rate_min, learning_rate_max))),
            ("optimizer_choice", lambda: str(rs.choice(list(optimizer_list)))),
            ("layer_size", lambda: int(rs.choice(list(layer_size_list)))),
            ("n_layers", lambda: int(rs.randint(n_layers_min, n_layers_max))),
            ("batch_size", lambda: int(rs.choice(list(batch_size_list)))),
            ("keep_prob", lambda: round(rs.uniform(dropout_min, dropout_max), 1))]
    if network_type == "ResNetRNN":
        plan += [(None, lambda: rs.randint(n_layers_res_min, n_layers_res_max)),
                 ("layer_size_res", lambda: int(rs.choice(list(size_layers_res_list))))]
    drawn = {}
    for key, draw in plan:
        value = draw()
        if key is not None:
            drawn[key] = value
    if "layer_size_res" in drawn:
        drawn["n_layers_res"] = drawn["n_layers"]
    return drawn


# --------------------------------------------------------------------------- training databases
class WindowExampleDb(object):
    """Balanced sampler over two pools of uniform-label windows (ExampleDb.get_training_set's contract)."""

    def __init__(self, pos, neg, seed=None):
        self.pos = [np.asarray(p) for p in pos]
        self.neg = [np.asarray(n) for n in neg]
        self.nb_pos, self.nb_neg = len(self.pos), len(self.neg)
        self.rng = random.Random(seed)

    def get_training_set(self, size, ratio=2):
        """ExampleDb.py:50-83: ``size // ratio`` positives + the rest negatives, drawn without replacement per
        batch, shuffled; returns (tuple of windows, tuple of label lists, number of positive labels)."""
        nb_pos = size // ratio
        nb_neg = size - nb_pos
        ps = self.rng.sample(range(self.nb_pos), nb_pos)
        ns = self.rng.sample(range(self.nb_neg), nb_neg)
        data_out = [(self.pos[n], [1] * len(self.pos[n])) for n in ps] + [(self.neg[n], [0] * len(self.neg[n])) for n in ns]
        self.rng.shuffle(data_out)
        x_out, y_out = zip(*data_out)
        pos_count = sum(y.count(1) for y in y_out)
        return x_out, y_out, pos_count


def windows_from_labelled_read(raw, labels, width=34, lessen=1, max_neg=None, rng=None):
    """TrainingRead.get_pos / get_neg (TrainingRead.py:226-257): windows of ``width + 1`` samples centred on a point
    (one more sample right of the centre when the width is odd) whose labels are ALL 1 (positives, every
    ``lessen``-th hit) or ALL 0 (negatives, a random subset of ``max_neg`` centres)."""
    raw = np.asarray(raw)
    labels = np.asarray(labels).astype(np.int64)
    width_l = width // 2
    width_r = width - width_l
    n = len(labels)
    csum = np.concatenate(([0], np.cumsum(labels)))
    centres = np.arange(width_l, n - width_r)
    ones = csum[centres + width_r + 1] - csum[centres - width_l]          # label sum of [c - l, c + r]
    pos_c = centres[(labels[centres] == 1)][::lessen]
    pos_c = pos_c[(csum[pos_c + width_r + 1] - csum[pos_c - width_l]) == width + 1]
    neg_c = centres[(labels[centres] == 0) & (ones == 0)]
    if max_neg is not None and len(neg_c) > max_neg:
        rng = rng or np.random.default_rng(0)
        neg_c = np.sort(rng.choice(neg_c, size=max_neg, replace=False))
    pos = [raw[c - width_l:c + width_r + 1] for c in pos_c]
    neg = [raw[c - width_l:c + width_r + 1] for c in neg_c]
    return pos, neg


def load_npz(npz_file):
    """networks/reader.py:11-23: (raw signal, labels) of one NPZ read."""
    with np.load(npz_file, allow_pickle=False) as npz:
        return npz["raw"], npz["base_labels"]


def npz_loader_from_env():
    """The ``path -> (raw, labels)`` loader of the files ``CATFISH_LABEL_KMER`` / ``CATFISH_LABEL_MOVES`` name
    (``labelling.LabelSource``): ``load_npz`` itself when neither is set."""
    from . import labelling
    return labelling.LabelSource.from_env().loader()


def example_db_from_npz(npz_files, width=34, lessen=1, max_neg_per_read=2000, seed=0, loader=None):
    """A training database over NPZ reads (raw = normalised signal, base_labels = 0/1 per sample; ``loader``: ``load_npz``)."""
    rng = np.random.default_rng(seed)
    pos, neg = [], []
    for f in npz_files:
        raw, labels = (loader or load_npz)(f)
        p, n = windows_from_labelled_read(raw, labels, width, lessen, max_neg_per_read, rng)
        pos.extend(p)
        neg.extend(n)
    return WindowExampleDb(pos, neg, seed=seed)


def synthetic_labelled_read(length, seed, hp_fraction=0.06):
    """A normalised synthetic squiggle (SURVEY 8d generator) with a planted class: homopolymer stretches are long
    dwells at one level (what a homopolymer looks like in nanopore current), labelled 1."""
    rng = np.random.default_rng(seed)
    sig = np.empty(length, dtype=np.float64)
    lab = np.zeros(length, dtype=np.int64)
    i = 0
    while i < length:
        if rng.random() < hp_fraction / 8.0:
            n = int(rng.integers(40, 120))                 # homopolymer: one long flat event
            sig[i:i + n] = rng.normal(500.0, 60.0)
            lab[i:i + n] = 1
        else:
            n = int(rng.geometric(1.0 / 9.0))
            sig[i:i + n] = rng.normal(500.0, 60.0)
        i += n
    sig = np.clip(np.rint(sig + rng.normal(0.0, 8.0, size=length)), 0, 2047)
    shift = np.median(sig)
    scale = np.median(np.abs(sig - shift))
    return (sig - shift) / scale, lab


def synthetic_example_db(n_reads=8, read_len=20000, seed=0):
    pos, neg = [], []
    rng = np.random.default_rng(seed)
    for r in range(n_reads):
        raw, lab = synthetic_labelled_read(read_len, seed * 1000 + r)
        p, n = windows_from_labelled_read(raw, lab, 34, 1, 4000, rng)
        pos.extend(p)
        neg.extend(n)
    return WindowExampleDb(pos, neg, seed=seed)


# --------------------------------------------------------------------------- training loop
def _append(path, text):
    with open(path, "a+") as fh:
        fh.write(text)


def _json_line(record):
    """One JSON line; nan (an AUC without one of the classes) is written as null, at any depth."""
    def clean(value):
        if isinstance(value, dict):
            return {key: clean(v) for key, v in value.items()}
        if isinstance(value, float) and value != value:
            return None
        return value
    return json.dumps(clean(record), allow_nan=False) + "\n"


def border_report(row, reach):
    """One threshold's [2, 5 * reach + 3] border row -> (hp_borders, called_borders): ``device_validation.run_border_summary``'s two
    dicts, each with the four parts of its row as lists (``left``, ``right``, ``gaps``) and a number (``interrupted_runs``)."""
    out = []
    for kind, summary in enumerate(run_border_summary(row, reach)):
        part = split_run_borders(np.asarray(row)[kind], reach)
        out.append(dict(summary, left=part["left"].tolist(), right=part["right"].tolist(), gaps_by_length=part["gaps"].tolist(),
                        interrupted_runs=int(part["interrupted"])))
    return tuple(out)


def _state_fields(run_edges, table):
    complete, found, called_absent = run_state_rates(table)
    return {"hp_states": table[0].tolist(), "called_states": table[1].tolist(), "hp_complete": complete, "hp_found": found,
            "called_absent": called_absent}


def _base_fields(max_bases, table):
    return {"hp_bases": table[0].tolist(), "called_bases": table[1].tolist(), **run_base_rates(table)}


def _vote_fields(vote_bases, confusion, vote_runs):
    from .base_votes import base_vote_rates
    return {"base_confusion": confusion.tolist(), **base_vote_rates(confusion), "vote_runs": run_base_rates(vote_runs)}


def _vote_line(vote_bases, confusion, vote_runs):
    from .base_votes import base_vote_rates
    return {"threshold": 0.5, "max_bases": int(vote_bases), "classes": list(BASE_CLASSES), "states": list(RUN_STATES),
            "base_confusion": confusion.tolist(), **base_vote_rates(confusion), "hp_vote_runs": vote_runs[0].tolist(),
            "called_vote_runs": vote_runs[1].tolist(), **run_base_rates(vote_runs)}


def _curve_line(shift, histogram):
    curves = curves_from_histogram(histogram, shift)
    return {"shift": int(shift), **{key: curves[key] for key in ("roc_auc", "roc_auc_slack", "pr_auc", "best_f1", "n_pos", "n_neg", "n_other")}}


# How each optional result of a round (``validation_round.OPTIONS``, same keys in the same order) is reported.  The network carries the
# option as ``validation_<option>`` and ``validate`` leaves every result in ``validation_<result>`` ([0] of a per-threshold one).
#   refusal      why ``validate`` cannot count it over a list of paths
#   sweep        (value, one threshold's table or tables) -> what it adds to a ``threshold_sweep`` row; None: nothing
#   line         (value, the round's table or tables) -> its JSON line per checkpoint round, after ``step`` and before ``bridge_gap``
#   suffix       ... appended to ``<model path><suffix>.jsonl``
#   nan_as_null  ... through ``_json_line``; otherwise ``json.dumps``
Report = namedtuple("Report", "refusal sweep line suffix nan_as_null")
REPORTS = {
    "run_edges": Report(
        "validate: run_edges needs a DeviceValidationSet (the run states are counted on the card)", _state_fields,
        lambda edges, table: {"threshold": 0.5, "edges": list(edges), "states": list(RUN_STATES), **_state_fields(edges, table)},
        "_hp_states", False),
    "border_reach": Report(
        "validate: border_reach needs a DeviceValidationSet (the borders are compared on the card)",
        lambda reach, table: dict(zip(("hp_borders", "called_borders"), border_report(table, reach))),
        lambda reach, table: {"threshold": 0.5, "reach": int(reach), **dict(zip(("hp_borders", "called_borders"), border_report(table, reach)))},
        "_hp_borders", False),
    "curve_shift": Report(
        "validate: curve_shift needs a DeviceValidationSet (the probabilities are binned on the card)", None, _curve_line, "_curves", True),
    "max_bases": Report(
        "validate: max_bases needs a DeviceValidationSet with a base map (the bases are counted on the card)", _base_fields,
        lambda most, table: {"threshold": 0.5, "max_bases": int(most), "classes": list(BASE_CLASSES), "states": list(RUN_STATES),
                             **_base_fields(most, table)},
        "_hp_bases", False),
    "vote_bases": Report(
        "validate: vote_bases needs a DeviceValidationSet with a base table (the bases are voted on the card)", _vote_fields, _vote_line,
        "_base_votes", False),
    "score_shift": Report(
        "validate: score_shift needs a DeviceValidationSet (the scores under runs are binned on the card)",
        lambda shift, table: dict(zip(("hp_scores", "called_scores"), run_score_summary(table, shift))),
        lambda shift, table: {"threshold": 0.5, "shift": int(shift), "states": list(RUN_STATES),
                              **dict(zip(("hp_scores", "called_scores"), run_score_summary(table, shift)))},
        "_hp_scores", True)}
_REPORT_ORDER = tuple(sorted(OPTIONS, key=lambda row: not row.per_threshold))       # the files in the order the round launches: the curve last


def _given(**options):
    """The options that were given (not None), in the order of the tables: what a round is asked for, and nothing else."""
    return {option: options[option] for option in REPORTS if options.get(option) is not None}


def _bridged(given):
    """Whether ``bridge_gap`` changes any of the results asked for."""
    return any(row.bridged for row in OPTIONS if row.option in given)


def _checkpoint_round(network, step, batch_x, batch_y, report, validation):
    """What the reference does at a checkpoint step (networks/train_validate.py:154-175): save, score the batch just
    trained on, run one round of validation; the report lines go to ``report`` in that order.  Every optional result the network asks
    for (``network.validation_<option>``, a row of ``REPORTS``) is appended as one JSON line to its own file next to the report, which
    stays the reference's."""
    network.save_network_to_model_path(step)
    saved = "Saved checkpoint at step {}\n".format(step)
    print(saved)
    _append(report, "\n" + saved)
    clock = datetime.datetime.now()
    # the reference feeds the TRAINING keep_prob here (:163), so its two numbers carry dropout noise; the
    # deterministic inference pass is reported instead
    batch_acc, batch_loss = network.evaluate(batch_x, batch_y)
    print("Validated in {}".format(datetime.datetime.now() - clock))
    _append(report, "\nTraining accuracy: {}\nTraining loss: {}\n".format(batch_acc, batch_loss))
    clock = datetime.datetime.now()
    given = _given(**{option: getattr(network, "validation_" + option, None) for option in REPORTS})
    extra = dict(given)
    bridge_gap = int(getattr(network, "validation_bridge_gap", 0) or 0)
    if bridge_gap:
        extra["bridge_gap"] = bridge_gap
    if getattr(network, "validation_loader", None) is not None:
        extra["loader"] = network.validation_loader
    _acc, precision, recall = validate(network, *validation, **extra)
    for row in _REPORT_ORDER:
        if row.option in given:
            how = REPORTS[row.option]
            record = {"step": int(step), **how.line(given[row.option], *(np.asarray(getattr(network, "validation_" + name)) for name in row.names))}
            if bridge_gap and row.bridged:
                record["bridge_gap"] = bridge_gap
            _append(report[:-len(".txt")] + how.suffix + ".jsonl", _json_line(record) if how.nan_as_null else json.dumps(record) + "\n")
    print("Validated in {}".format(datetime.datetime.now() - clock))
    _append(report, "Validation precision: {}\nValidation recall: {}\n".format(precision, recall))
    return batch_acc


def _train_device_fed(network, db, n_steps, step, report):
    """``n_steps`` device-fed steps after step ``step`` -> (steps taken, whether the draw goes on).  A network that trains with
    ``clip_norm`` / ``skip_nonfinite`` takes them one read-back chunk at a time (``Trainer.loss_log_capacity``; the same steps as
    one call) and looks at the count of skipped steps after each: a chunk in which EVERY step was skipped ends the draw, with a
    line in the report -- the weights no longer change, and unchanged weights on a diverged forward pass never recover."""
    if getattr(network, "clip_norm", None) is None and not getattr(network, "skip_nonfinite", None):
        network.train_network_steps(db, n_steps)
        return n_steps, True
    chunk = network._require_trainer().loss_log_capacity
    skipped = network.step_stats()["skipped"]
    done = 0
    while done < n_steps:
        k = min(chunk, n_steps - done)
        network.train_network_steps(db, k)
        done += k
        before, skipped = skipped, network.step_stats()["skipped"]
        if skipped - before == k:
            _append(report, "\nDraw ended at step {}: all {} steps of the last chunk were skipped (non-finite gradients or loss)\n"
                    .format(step + done, k))
            return done, False
    return done, True


def train_and_validate(network, db, training_nr, squiggles, max_seq_length, file_path, validation_start, max_number,
                       checkpoint_every=10000):
    """networks/train_validate.py:114-185.  ``training_nr // batch_size`` optimizer steps on balanced batches from
    ``db.get_training_set``; after the last step and after every ``checkpoint_every``-th (10 000 in the reference):
    checkpoint + batch metrics + one validation round.  Report text appended to ``file_path + ".txt"`` as the
    reference writes it.  Returns the last batch accuracy (None when no step ran; the reference fails on its unbound
    local there)."""
    report = file_path + ".txt"
    steps = training_nr // network.batch_size
    seen = steps * network.batch_size
    banner = "\nTraining on {} examples in {} batches\n".format(seen, steps)
    print("Start training at {}".format(datetime.datetime.now()))
    print(banner)
    _append(report, banner)
    validation = (squiggles, max_seq_length, file_path, validation_start, max_number)
    hp_labels = 0
    batch_acc = None
    from .device_db import DeviceExampleDb
    device_fed = isinstance(db, DeviceExampleDb) and hasattr(network, "train_network_steps")
    if device_fed:
        # device-fed: the steps between two checkpoint rounds are ONE call (the batches are drawn on the card); the round then
        # scores the batch just trained on, copied back from the step's static buffers
        step = 0
        while step < steps:
            upto = min(steps, (step // checkpoint_every + 1) * checkpoint_every)
            took, alive = _train_device_fed(network, db, upto - step, step, report)
            hp_labels += took * (network.batch_size // 2) * network.window
            if not alive:                                        # diverged for good: no checkpoint of it, no further round
                seen = (step + took) * network.batch_size
                break
            step = upto
            if step == steps - 1:
                print("This was the final checkpoint\n")
            windows, labels = db.last_batch()
            batch_acc = _checkpoint_round(network, step, reshape_input(windows, network.window, network.n_inputs),
                                          reshape_input(labels, network.window, network.n_outputs), report, validation)
    for step in range(1, (0 if device_fed else steps) + 1):
        windows, labels, n_pos = db.get_training_set(network.batch_size, ratio=2)
        hp_labels += n_pos
        batch_x = reshape_input(windows, network.window, network.n_inputs)
        batch_y = reshape_input(labels, network.window, network.n_outputs)
        network.train_network(batch_x, batch_y, step)
        if step == steps or step % checkpoint_every == 0:
            if step == steps - 1:
                print("This was the final checkpoint\n")          # the reference's off-by-one message (:158)
            batch_acc = _checkpoint_round(network, step, batch_x, batch_y, report, validation)
    share = hp_labels / (network.window * seen) if seen else 0
    _append(report, "\nTraining set had {:.2%} HPs\n".format(share) + "\nFinished training!\n\n")
    return batch_acc


# --------------------------------------------------------------------------- validation: select, ONE packed launch, sums
_VALIDATION_REPORT = (
    "\n---NEXT ROUND OF VALIDATION---"
    "\nAverage performance of validation set:\n"
    "\tAccuracy: {mean_acc:.2%}\n"
    "\tLoss: {mean_loss:.4f}"
    "\nPerformance over whole set: \n"
    "\tDetected {tp} true positives, {fp} false positives, {tn} true negatives, {fn} false negatives in total.\n"
    "\tTrue number of HPs: {hp} \tTrue percentage: {hp_share:.2%}\t Predicted percentage HPs: {called_share:.2%}\n"
    "\tAccuracy: {acc:.2%}"
    "\n\tPrecision: {precision:.2%}\n\tRecall: {recall:.2%}"
    "\t\nF1 score: {f1:.4f}"
    "{closing}")
_VALIDATION_CLOSING = "\nFinished validation of model {} on {} raw signals of average length {}."


def select_validation_stretches(squiggles, window, max_seq_length, validation_start, max_number, loader=load_npz):
    """Which samples one validation round scores (networks/train_validate.py:214-249), in file order.

    ``validation_start``: "complete" = whole reads; an int = the stretch ``[start, start + n)``; "random" = a stretch
    at ``random.randint(0, len - n)`` (Python's global generator, one draw per read that is long enough, so a seeded
    run picks the reference's stretches); ``n`` = ``max_seq_length`` rounded down to whole windows.  Reads shorter
    than the stretch are skipped; the selection stops once ``max_number`` reads are in.
    -> (signals, labels): two lists of 1-D arrays."""
    whole = validation_start == "complete"
    if not whole and validation_start != "random" and type(validation_start) != int:
        raise ValueError("validation_start must be an int, 'random' or 'complete'")
    n = max_seq_length // window * window
    signals, labels = [], []
    for path in squiggles:
        raw, lab = loader(path)
        if not whole:
            room = len(raw) - n - (0 if validation_start == "random" else validation_start)
            if room < 0:
                continue
            first = random.randint(0, room) if validation_start == "random" else validation_start
            raw, lab = raw[first:first + n], lab[first:first + n]
        signals.append(np.asarray(raw))
        labels.append(np.asarray(lab))
        if len(signals) >= max_number:
            break
    return signals, labels


def pack_validation_windows(signals, labels, window):
    """All stretches as one window-major batch: x float32 [sum N_i, window, 1], y float64 [sum N_i * window], the first
    packed sample of every read (int64 [n_reads + 1]) and each read's zero tail.  The tail rule is the training
    driver's ``padding`` (:51-64): an exact multiple of the window gets none."""
    lengths = np.array([len(s) for s in signals], dtype=np.int64)
    n_win = -(-lengths // window)
    tails = n_win * window - lengths
    bounds = np.zeros(len(signals) + 1, dtype=np.int64)
    np.cumsum(n_win * window, out=bounds[1:])
    x = np.zeros(int(bounds[-1]), dtype=np.float32)
    y = np.zeros(int(bounds[-1]), dtype=np.float64)
    for b, s, l in zip(bounds[:-1].tolist(), signals, labels):
        x[b:b + len(s)] = s
        y[b:b + len(l)] = l
    return x.reshape(-1, window, 1), y, bounds, tails


def score_validation_batch(probs32, logits32, y, bounds, tails, threshold=0.5):
    """Per-read accuracy / loss and whole-batch confusion counts from ONE packed forward pass
    (what rnn_class.py:222-261 computes read by read):

    * accuracy_i = mean(round_half_even(p) == y) over the read's padded windows -- ``tf.round`` sends p = 0.5 to 0
      (rnn_class.py:85) -- as float32, an exact count divided once;
    * loss_i = mean sigmoid cross-entropy of the LOGITS (rnn_class.py:74-79), summed in double, float32;
    * counts: prediction = ``p >= threshold`` (so p = 0.5 counts as a call); a called sample is a true positive when
      its label is 1 and a false positive otherwise -- zero tails included --, an un-called one a true negative when
      its label is 0 and a false negative otherwise; then every tail sample is taken out of the true negatives whether
      or not it was one (rnn_class.py:245-249)."""
    p = np.asarray(probs32, dtype=np.float64).reshape(-1)
    z = np.asarray(logits32, dtype=np.float64).reshape(-1)
    called = p >= threshold
    counts = (int(np.count_nonzero(called & (y == 1))), int(np.count_nonzero(called & (y != 1))),
              int(np.count_nonzero(~called & (y == 0))) - int(tails.sum()), int(np.count_nonzero(~called & (y != 0))))
    right = np.concatenate(([0], np.cumsum(np.round(p) == y)))
    sizes = np.diff(bounds)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = (right[bounds[1:]] - right[bounds[:-1]]).astype(np.float32) / sizes.astype(np.float32)
        ce = np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))
        loss = np.array([np.sum(ce[a:b]) for a, b in zip(bounds[:-1].tolist(), bounds[1:].tolist())]) / sizes
    return acc, loss.astype(np.float32), counts


def validate(network, squiggles, max_seq_length, file_path, validation_start="random", max_number=856, run_edges=None, curve_shift=None,
             border_reach=None, bridge_gap=0, loader=None, max_bases=None, vote_bases=None, score_shift=None):
    """networks/train_validate.py:188-295 as one packed launch.

    The reference pushes every read through ``test_network`` (one ``sess.run`` each, up to 856 per round); windows are
    independent, so here the selected stretches of ALL reads form one ``[sum N_i, 35, 1]`` batch that goes through
    ``network.score_windows`` once, and the per-read numbers come out of array sums over the read boundaries.  Same
    report (appended to ``<basename of file_path>.txt`` in the current directory), prints, return value
    ``(accuracy, precision, recall)`` over the whole set, and the same bookkeeping: counts are added to the
    network's running ``tp/fp/tn/fn`` and those are reset afterwards.

    Kept behaviour of the loop being replaced: the read that reaches ``max_number`` is scored and counted but its
    accuracy / loss are left out of the averages, which still divide by the number of reads (:248-256); no read
    selected -> ZeroDivisionError.

    The optional results of a round on the card (a ``DeviceValidationSet`` only; a list of paths is refused with the row's text in
    ``REPORTS``), each counted at threshold 0.5 and left on the network -- ``RNN.score_validation_device`` has the ranges of the options
    and the definitions:

        ``run_edges``     the homopolymers found, per length bin           ``network.validation_run_states`` [2, B, 3]
        ``border_reach``  how far the called borders miss, interruptions   ``network.validation_run_borders`` [2, 5 * border_reach + 3]
        ``curve_shift``   the probabilities binned (no threshold)          ``network.validation_curve`` [3, NB]
        ``max_bases``     the runs by base and length in bases; needs a    ``network.validation_run_bases`` [2, 3, 5, max_bases + 1]
                          set with a base map
        ``vote_bases``    every base voted by its samples, scored by       ``network.validation_base_confusion`` [5, 2, 2] and
                          base; needs a set with a base table              ``network.validation_base_vote_runs`` [2, 3, 5, vote_bases + 1]
        ``score_shift``   the probabilities under the runs, by kind and    ``network.validation_run_scores`` [2, 3, NB + 1]
                          state of the run

    ``bridge_gap`` (with ``run_edges``, ``border_reach``, ``max_bases`` or ``score_shift``; 0 .. 49): those tables are counted on the
    prediction with its gaps of at most that many samples bridged (``infer.bridge_gaps``).
    ``loader`` (a list of paths only): what reads a path into ``(raw, labels)`` instead of ``load_npz``.
    Report, prints and return value stay as they are."""
    from .calling import CallRule
    bridge_gap = CallRule.of(max_gap=bridge_gap).max_gap
    given = _given(run_edges=run_edges, border_reach=border_reach, curve_shift=curve_shift, max_bases=max_bases, vote_bases=vote_bases,
                   score_shift=score_shift)
    if bridge_gap and not _bridged(given):
        raise ValueError("validate: bridge_gap changes the run states and the borders only: give run_edges or border_reach")
    print("Max length is {}".format(max_seq_length))
    print("Validation start is {}".format(validation_start))
    from .device_validation import DeviceValidationSet
    if isinstance(squiggles, DeviceValidationSet):
        # the reads live on the card: the same stretches (same draws), gathered and scored there; only raw counts and sums come back
        selection = squiggles.select(network.window, max_seq_length, validation_start, max_number)
        n_reads = len(selection[0])
        n_samples = int(selection[2].sum())
        if n_reads == 0:
            raise ZeroDivisionError("validation selected no read")
        if not given:
            right, ce_sum, counts_k = network.score_validation_device(squiggles, selection)
        else:
            got = network.score_validation_device(squiggles, selection, (0.5,), **given, **({"bridge_gap": bridge_gap} if bridge_gap else {}))
            right, ce_sum, counts_k = got[:3]
            for row in OPTIONS:
                for name in row.names if row.option in given else ():
                    setattr(network, "validation_" + name, getattr(got, name)[0] if row.per_threshold else getattr(got, name))
        acc, loss, counts = squiggles.finish(right, ce_sum, counts_k[0], *squiggles.layout(selection[2], network.window))
    else:
        for row in CHECK_ORDER:                            # what is counted on the card cannot be asked of paths
            if row.option in given:
                raise ValueError(REPORTS[row.option].refusal)
        signals, labels = select_validation_stretches(squiggles, network.window, max_seq_length, validation_start,
                                                      max_number, **({} if loader is None else {"loader": loader}))
        n_reads = len(signals)
        n_samples = sum(len(s) for s in signals)
        if n_reads == 0:
            raise ZeroDivisionError("validation selected no read")
        x, y, bounds, tails = pack_validation_windows(signals, labels, network.window)
        probs, logits = network.score_windows(x)
        acc, loss, counts = score_validation_batch(probs, logits, y, bounds, tails)
    averaged = n_reads - 1 if n_reads >= max_number else n_reads
    acc_sum = loss_sum = 0
    for a, l in zip(acc[:averaged].tolist(), loss[:averaged].tolist()):      # doubles holding float32 values, in order
        acc_sum += a
        loss_sum += l
    network.tp, network.fp, network.tn, network.fn = (have + new for have, new in
                                                      zip((network.tp, network.fp, network.tn, network.fn), counts))
    tp, fp, tn, fn = network.tp, network.fp, network.tn, network.fn
    whole_acc = metrics.calculate_accuracy(tp, fp, tn, fn)
    precision, recall = metrics.precision_recall(tp, fp, fn)
    closing = _VALIDATION_CLOSING.format(network.model_type, n_reads, n_samples / n_reads)
    _append(file_path.split("/")[-1] + ".txt", _VALIDATION_REPORT.format(
        mean_acc=acc_sum / n_reads, mean_loss=loss_sum / n_reads, tp=tp, fp=fp, tn=tn, fn=fn, hp=tp + fn,
        hp_share=(tp + fn) / n_samples, called_share=(tp + fp) / n_samples, acc=whole_acc, precision=precision,
        recall=recall, f1=metrics.f1(precision, recall), closing=closing))
    print(closing)
    network.tp = network.fp = network.tn = network.fn = 0
    print("Validation accuracy: ", whole_acc)
    print("Validation loss: ", loss_sum / n_reads)
    return whole_acc, precision, recall


def threshold_sweep(network, vset, thresholds, max_seq_length, validation_start="complete", max_number=856, run_edges=None,
                    border_reach=None, bridge_gap=0, phases=(0,), vote_weight="mean", max_bases=None, vote_bases=None, score_shift=None):
    """The reference's precision / recall sweep (networks/precision_recall_ROC.py:85-100: ``class_from_threshold`` --
    ``p >= t`` -- then ``compute_f1`` per threshold) over a ``DeviceValidationSet``: ONE forward pass, every threshold counted
    from its probabilities on the card.  The stretches are ``validate``'s (same selection, same tail rule for the true
    negatives).  -> a list of dicts {threshold, tp, fp, tn, fn, precision, recall, f1}, one per threshold, in order.

    Every optional result given adds its fields to every row (``REPORTS[option].sweep``; the options' ranges and what is counted:
    ``RNN.score_validation_device``; the reference does all of this offline, networks/process_output.py):

        ``run_edges``     ``hp_states`` and ``called_states`` -- per length bin [complete, incomplete, absent] of the true runs against the
                          corrected prediction and of the called runs against the truth --, ``hp_complete`` and ``hp_found`` (complete,
                          complete + incomplete over all true runs) and ``called_absent`` (called runs that hold no homopolymer sample over
                          all called runs); 0 for an empty denominator (:235-273)
        ``border_reach``  ``hp_borders`` and ``called_borders``, each ``border_report``'s dict: how far that threshold's borders miss (the
                          rest of ``check_hp``)
        ``max_bases``     ``hp_bases`` and ``called_bases`` -- per state, base class (A / C / G / T / other) and length in bases how many true
                          and called runs, ``[3][5][max_bases + 1]`` lists -- and the fields of ``device_validation.run_base_rates``
                          (``prediction_information``); a set with a base map
        ``vote_bases``    ``base_confusion`` -- per base class [truth][called] how many voted bases, a ``[5][2][2]`` list --, the fields of
                          ``base_votes.base_vote_rates`` (per-base precision / recall / F1, overall and per letter) and ``vote_runs``, the
                          fields of ``run_base_rates`` over the runs on the base axis; a set with a base table
        ``score_shift``   ``hp_scores`` and ``called_scores`` -- per state of the true and of the called runs
                          ``device_validation.run_score_summary``'s dict (n, mean, q1 / median / q3 as the edges of their bin), so
                          ``hp_scores[2]`` tells how close the missed homopolymers were to the threshold and ``called_scores[2]`` how
                          confident the calls that hold none (``check_for_false_neg``)

    ``bridge_gap`` (with ``run_edges``, ``border_reach``, ``max_bases`` or ``score_shift``; 0 .. 49): those tables are those of the prediction
    with its gaps of at most that many samples bridged (``infer.bridge_gaps``); tp / fp / tn / fn stay per-sample counts.

    ``phases`` / ``vote_weight`` (``infer.check_phases``): shifted-window voting -- every count is taken from the probabilities voted
    over those tilings (``tilings.vote_host``); ``(0,)`` changes nothing."""
    from .calling import CallRule
    rule = CallRule.of(max_gap=bridge_gap, phases=phases, vote_weight=vote_weight)
    bridge_gap = rule.max_gap
    voted = {"phases": rule.phases, "vote_weight": rule.vote_weight} if rule.voted else {}      # (0,): the call of before
    given = _given(run_edges=run_edges, border_reach=border_reach, max_bases=max_bases, vote_bases=vote_bases, score_shift=score_shift)
    if bridge_gap and not _bridged(given):
        raise ValueError("threshold_sweep: bridge_gap changes the run states and the borders only: give run_edges or border_reach")
    bridged = {"bridge_gap": bridge_gap} if bridge_gap else {}                                  # nothing given: the call of before
    thresholds = [float(t) for t in thresholds]
    selection = vset.select(network.window, max_seq_length, validation_start, max_number)
    if len(selection[0]) == 0:
        raise ZeroDivisionError("validation selected no read")
    got = network.score_validation_device(vset, selection, thresholds, **given, **bridged, **voted)
    counts = got[2]
    tail = int(vset.layout(selection[2], network.window)[1].sum())
    rows = []
    for k, (t, (tp, fp, tn_raw, fn)) in enumerate(zip(thresholds, np.asarray(counts).tolist())):
        precision, recall = metrics.precision_recall(tp, fp, fn)
        rows.append({"threshold": t, "tp": tp, "fp": fp, "tn": tn_raw - tail, "fn": fn, "precision": precision, "recall": recall,
                     "f1": metrics.f1(precision, recall)})
        for row in OPTIONS:
            if row.option in given and REPORTS[row.option].sweep is not None:
                rows[-1].update(REPORTS[row.option].sweep(given[row.option], *(getattr(got, name)[k] for name in row.names)))
    return rows


def _interrupted_shares(row):
    """Of a ``threshold_sweep`` row with borders: the share of the true (called) runs that are not absent and have at least one
    interruption in the other array."""
    out = {}
    for name, part in (("hp_interrupted", row["hp_borders"]), ("called_interrupted", row["called_borders"])):
        judged = int(np.sum(part["left"]))
        out[name] = part["interrupted_runs"] / judged if judged else 0
    return out


def bridge_sweep(network, vset, gaps, max_seq_length, threshold=0.5, validation_start="complete", max_number=856, run_edges=(),
                 border_reach=BORDER_REACH):
    """What bridging gaps of up to g samples does to the homopolymers a round finds, for every g of ``gaps`` (ints in 0 .. 49), over
    a ``DeviceValidationSet`` at one threshold: one ``threshold_sweep`` round per gap (same stretches; ``validation_start`` should
    not be "random").  -> a list of dicts {bridge_gap, hp_complete, hp_found, called_absent (``run_state_rates``), hp_states,
    called_states, hp_interrupted, called_interrupted}: the last two are the share of the true (called) runs that are not absent
    and have at least one interruption in the other array -- homopolymers found in pieces."""
    rows = []
    for gap in gaps:
        row = threshold_sweep(network, vset, [threshold], max_seq_length, validation_start, max_number, run_edges=run_edges,
                              border_reach=border_reach, bridge_gap=gap)[0]
        out = {"bridge_gap": int(gap)}
        out.update({key: row[key] for key in ("hp_complete", "hp_found", "called_absent", "hp_states", "called_states")})
        out.update(_interrupted_shares(row))
        rows.append(out)
    return rows


def tiling_sweep(network, vset, phase_sets, max_seq_length, weight="mean", threshold=0.5, validation_start="complete", max_number=856,
                 run_edges=(), border_reach=BORDER_REACH):
    """What shifted-window voting does to a round, for every phase set of ``phase_sets`` (each ``infer.check_phases``'s; ``(0,)`` is
    the network as it is), over a ``DeviceValidationSet`` at one threshold: one ``threshold_sweep`` round per phase set (same
    stretches; ``validation_start`` should not be "random"), merged by ``weight``.  -> a list of dicts {phases, weight, tp, fp, tn,
    fn, precision, recall, f1 (per sample), hp_complete, hp_found, called_absent (``run_state_rates``), hp_states, called_states,
    hp_interrupted, called_interrupted}: the last two are the share of the true (called) runs that are not absent and have at
    least one interruption in the other array -- homopolymers found in pieces.  Whether voting improves the calls on real reads
    is what this function is there to find out."""
    from .infer import check_phases
    rows = []
    for phases in phase_sets:
        phases = check_phases(phases)
        row = threshold_sweep(network, vset, [threshold], max_seq_length, validation_start, max_number, run_edges=run_edges,
                              border_reach=border_reach, phases=phases, vote_weight=weight)[0]
        out = {"phases": list(phases), "weight": weight}
        out.update({key: row[key] for key in ("tp", "fp", "tn", "fn", "precision", "recall", "f1", "hp_complete", "hp_found",
                                              "called_absent", "hp_states", "called_states")})
        out.update(_interrupted_shares(row))
        rows.append(out)
    return rows


def validation_curves(network, vset, max_seq_length, validation_start="complete", max_number=856, shift=14):
    """The reference's whole-curve evaluation (``roc_curve``, ``precision_recall_curve`` and ``auc``, networks/metrics.py:66-94;
    ``roc_auc_score`` and the marks on the curve, networks/precision_recall_ROC.py:14-82 -- offline there, from text dumps of every
    score) over a ``DeviceValidationSet``: ONE forward pass, the probabilities binned on the card at every ``1 << shift`` step of
    their float32 bits (``device_validation.curve_host``; 65 025 thresholds at shift 14), the curves drawn from that table on the
    host.  The stretches are ``threshold_sweep``'s (same selection; the zero tails are not counted).  ->
    ``device_validation.curves_from_histogram``'s dict (tp / fp / tn / fn, tpr / fpr, precision / recall per threshold, roc_auc
    with its quantisation slack, pr_auc, best_f1, n_pos / n_neg / n_other) plus ``shift`` and ``thresholds`` (float32 [NB])."""
    selection = vset.select(network.window, max_seq_length, validation_start, max_number)
    if len(selection[0]) == 0:
        raise ZeroDivisionError("validation selected no read")
    hist = network.score_validation_device(vset, selection, (0.5,), curve_shift=shift).curve
    curves = curves_from_histogram(hist, shift)
    curves.update({"shift": int(shift), "thresholds": curve_thresholds(shift)})
    return curves


VALIDATION_RUN_EDGES = (35, 70, 140)        # length bins of the per-round homopolymer table: one, two and four windows

VALIDATION_CURVE_SHIFT = 14                  # 65 025 threshold steps for the per-round curve line

_USAGE = ("The following arguments should be provided in this order:\n"
          "\t-network type\n\t-path to training db"
          "\n\t-number of training reads\n\t-path to validation db"
          "\n\t-max length of validation reads\n\nOptional:"
          "\n\t-start position for validation\n\t-maximum number of reads for validation")
_SHIPPED_HPARAMS = {
    "RNN": dict(batch_size=256, optimizer_choice="Adam", learning_rate=0.001, layer_size=64, n_layers=3, keep_prob=0.8),
    "ResNetRNN": dict(batch_size=256, optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64, n_layers=3,
                      keep_prob=0.8, layer_size_res=32, n_layers_res=2)}


def _npz_files(directory):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.endswith(".npz"))


def device_read_db_from_env(npz_files):
    """``CATFISH_DEVICE_DB=reads``: a ``device_db.DeviceReadDb`` over the NPZ reads.  CATFISH_DEVICE_NEG says how many negatives a
    read contributes: ``positives`` (the default: as many as it has positives, the reference's rule), an integer, or ``all``.
    A host database: it feeds the per-step loop (``get_training_set``)."""
    from .device_db import DeviceReadDb
    from . import labelling
    rule = os.environ.get("CATFISH_DEVICE_NEG", "positives")
    if rule not in ("positives", "all"):
        try:
            rule = int(rule)
        except ValueError:
            raise ValueError("CATFISH_DEVICE_NEG must be 'positives', 'all' or an integer, got %r" % rule)
    # (event and move files are labelled on the card where there is one)
    return DeviceReadDb.from_source(npz_files, labelling.LabelSource.from_env(), seed=0, neg_per_read=None if rule == "all" else rule)


def tiled_options_from_env():
    """CATFISH_TILED_STRIDE (an int of at least 1; default 35, the caller's grid) and CATFISH_TILED_MISSES (``hits``, the default: as
    many windows without a positive sample as the read has windows with one; an integer; or ``all``) -> (stride, miss_per_read) as
    ``device_db.tiled_tables`` takes them.  Anything else raises ValueError."""
    text = os.environ.get("CATFISH_TILED_STRIDE", "35")
    try:
        stride = int(text)
    except ValueError:
        stride = 0
    if stride < 1:
        raise ValueError("CATFISH_TILED_STRIDE must be an integer of at least 1, got %r" % text)
    rule = os.environ.get("CATFISH_TILED_MISSES", "hits")
    if rule not in ("hits", "all"):
        try:
            rule = int(rule)
        except ValueError:
            rule = -1
        if rule < 0:
            raise ValueError("CATFISH_TILED_MISSES must be 'hits', 'all' or a non-negative integer, got %r" % os.environ["CATFISH_TILED_MISSES"])
    return stride, None if rule == "all" else rule


def device_tiled_db_from_env(npz_files):
    """``CATFISH_DEVICE_DB=tiled``: a ``device_db.DeviceTiledDb`` over the NPZ reads, cut as ``tiled_options_from_env`` says; the reads
    are what ``labelling.LabelSource.from_env()`` says they are (event and move files are labelled on the card where there is one)."""
    from .device_db import DeviceTiledDb
    from . import labelling
    stride, misses = tiled_options_from_env()
    return DeviceTiledDb.from_source(npz_files, labelling.LabelSource.from_env(), seed=0, stride=stride, miss_per_read=misses)


def main(argv):
    """networks/train_validate.py:298-360: ``network_type train_npz_dir n_training_examples validation_npz_dir
    max_validation_length [validation_start [max_number]]``.  The training "database" argument is a directory of NPZ
    reads (the reference takes a ZODB file); hyper-parameters are a random draw as in the reference (:328) unless
    CATFISH_SHIPPED_HPARAMS=1 asks for the shipped network's (the reference's commented block :329-332).
    CATFISH_NATIVE_TRAINING=1 trains with ``native_training=True``: the whole step on the HIP kernels, the tuned ones at 64 / 32
    with a conv stack of 1 .. 4 blocks, the any-size ones for every other draw (64 units without a conv stack and 64 / 32 at depth 5
    among them).
    CATFISH_TRAINING_PRECISION=bf16x3 trains with ``training_precision="bf16x3"`` (every draw that trains on the any-size kernels;
    refused where the tuned ones or plain torch train).
    CATFISH_CLIP_NORM=<c> trains with ``clip_norm=c``: every step's gradients scaled to a global norm of at most c, and a step with
    non-finite gradients or loss skipped (``training.Trainer``); a device-fed draw whose steps were all skipped for a whole
    read-back chunk is ended, with a line in the report.
    CATFISH_DEVICE_DB=1 keeps the training windows on the card (``device_db.DeviceExampleDb``): the steps between two
    checkpoint rounds run back to back, each drawing its own batch.
    CATFISH_DEVICE_DB=reads trains from the labelled reads as they are (``device_db.DeviceReadDb``).  Despite the variable's name
    this is a HOST database -- nothing of it goes to the card, every batch is gathered in numpy and copied over, so a step costs
    more than with CATFISH_DEVICE_DB=1; what it offers is 5 B per sample and two tables of window starts instead of one array per
    window, the reference's negative rule and a reproducible selection.  CATFISH_DEVICE_NEG=positives|<int>|all sets the
    negatives a read contributes (``device_read_db_from_env``).
    CATFISH_DEVICE_DB=tiled trains on the windows the caller will cut (``device_db.DeviceTiledDb``): every read cut into consecutive
    35-sample windows from its first sample, each with its true per-sample labels, so that a homopolymer's border falls inside a
    window.  Like ``reads`` it is a HOST database: every batch is gathered in numpy and copied over.  This departs from the
    reference's selection (``TrainingRead.get_pos`` / ``get_neg`` keep only windows whose 35 labels are all equal), which never
    shows the network the mixed windows it meets when calling.  CATFISH_TILED_STRIDE=<int> (default 35) sets the distance between
    window starts, CATFISH_TILED_MISSES=hits|<int>|all (default ``hits``) how many windows without a positive sample a read
    contributes (``tiled_options_from_env``; a bad value raises ValueError).  CATFISH_LABEL_KMER / CATFISH_LABEL_MOVES apply as for
    ``reads``.
    CATFISH_DEVICE_VALIDATION=1 keeps the validation reads on the card too (``device_validation.DeviceValidationSet``, loaded
    once): a checkpoint round gathers and scores its stretches there instead of re-opening the files.
    CATFISH_VALIDATION_RUNS=1 (with CATFISH_DEVICE_VALIDATION=1) also counts, per round, the homopolymers found at threshold 0.5
    in the length bins ``VALIDATION_RUN_EDGES`` and appends them as one JSON line to ``<model path>_hp_states.jsonl``; the
    ``.txt`` report is unchanged.
    CATFISH_VALIDATION_CURVE=1 (with CATFISH_DEVICE_VALIDATION=1) also bins every round's probabilities on the card
    (``validation_curves``' histogram at shift ``VALIDATION_CURVE_SHIFT``) and appends step, shift, roc_auc, roc_auc_slack, pr_auc,
    best_f1, n_pos, n_neg and n_other as one JSON line to ``<model path>_curves.jsonl`` (nan as null); the ``.txt`` reports and the
    ``_hp_states.jsonl`` lines are unchanged.
    CATFISH_VALIDATION_BORDERS=1 (reach 64) or =<int> (that reach, 1 .. 128; with CATFISH_DEVICE_VALIDATION=1) also counts, per
    round, how far the called borders miss the true ones and the interruptions at threshold 0.5 and appends step, threshold,
    reach, ``hp_borders`` and ``called_borders`` (``border_report``; None as null) as one JSON line to
    ``<model path>_hp_borders.jsonl``; the ``.txt`` reports and the other ``.jsonl`` files are unchanged.
    CATFISH_VALIDATION_SCORES=1 (with CATFISH_DEVICE_VALIDATION=1) also bins, per round, the probabilities under the true and the
    called runs at threshold 0.5 by state of the run (``device_validation.run_scores_host`` at shift ``RUN_SCORE_SHIFT``, on the card)
    and appends step, threshold, shift, states, ``hp_scores`` and ``called_scores`` (``device_validation.run_score_summary``: n, mean
    and quartile bins per state; None as null) as one JSON line to ``<model path>_hp_scores.jsonl``: how close the missed
    homopolymers were to the threshold.  CATFISH_VALIDATION_BRIDGE applies to it too.  The ``.txt`` reports and the other ``.jsonl``
    files are unchanged.
    CATFISH_VALIDATION_BRIDGE=<int> (1 .. 49; with CATFISH_VALIDATION_RUNS or CATFISH_VALIDATION_BORDERS) counts those two on the
    prediction with its gaps of at most that many samples bridged (``infer.bridge_gaps``); their JSON lines then carry
    ``bridge_gap``.
    CATFISH_VALIDATION_BASES=1 (16 length bins) or =<int> (1 .. 32; needs CATFISH_DEVICE_VALIDATION=1 and CATFISH_LABEL_KMER: only
    reads that come with their event tables have a base map) also counts, per round, the true and the called runs at threshold 0.5
    by state, base (A / C / G / T / other) and length in bases and appends step, threshold, max_bases, classes, states,
    ``hp_bases``, ``called_bases`` and the rates of ``device_validation.run_base_rates`` as one JSON line to
    ``<model path>_hp_bases.jsonl``; CATFISH_VALIDATION_BRIDGE applies to it too.  The ``.txt`` reports and the other ``.jsonl``
    files are unchanged.
    CATFISH_VALIDATION_VOTES=1 (16 length bins) or =<int> (1 .. 32; needs what CATFISH_VALIDATION_BASES needs: only reads that come
    with their event or move tables have a base table) also lets, per round, the samples of every base vote on it at threshold 0.5
    (``base_votes.vote_host``, on the card) and appends step, threshold, max_bases, classes, states, ``base_confusion``, the rates of
    ``base_votes.base_vote_rates`` (per-base precision / recall / F1), ``hp_vote_runs``, ``called_vote_runs`` and the rates of
    ``device_validation.run_base_rates`` over them as one JSON line to ``<model path>_base_votes.jsonl``.  The ``.txt`` reports and
    the other ``.jsonl`` files are unchanged.
    CATFISH_LABEL_KMER=<odd k in 1 .. 15> or CATFISH_LABEL_MOVES=1 (never both): the two directories hold reads with their tables
    instead of labels -- event files (``raw`` + ``event_base`` / ``event_length``; ``python -m catfish_amd.convert --events`` writes
    them) or move files (``raw`` + ``event_state`` / ``event_move`` / ``event_length`` of reads that were base-called and not
    resquiggled; ``convert --moves``).  ``labelling.LabelSource.from_env`` reads the two variables, once, and everything below takes
    the source from it: every read is labelled on the way in (``source.loader()``; with CATFISH_DEVICE_VALIDATION=1 or
    CATFISH_DEVICE_DB=reads on the card, ``DeviceValidationSet.from_source`` -> ``cf_label_events`` / ``cf_label_moves``) -- the labels
    a directory of ``raw`` + ``base_labels`` files made from them would hold.  Unset, nothing changes."""
    args = list(argv[1:])
    if len(args) < 5:
        raise ValueError(_USAGE)
    kind, train_dir, val_dir = args[0], args[1], args[3]
    n_train, stretch = int(args[2]), int(args[4])
    start = int(args[5]) if len(args) > 5 else "random"
    most = int(args[6]) if len(args) > 6 else 856
    shipped = os.environ.get("CATFISH_SHIPPED_HPARAMS") == "1"
    hparams = dict(_SHIPPED_HPARAMS.get(kind, _SHIPPED_HPARAMS["ResNetRNN"])) if shipped \
        else generate_random_hyperparameters(kind)
    if os.environ.get("CATFISH_NATIVE_TRAINING") == "1":          # the whole training step on the HIP kernels at any geometry
        hparams["native_training"] = True
    if os.environ.get("CATFISH_TRAINING_PRECISION"):             # "bf16x3": split bf16 products in the any-size training recurrences
        hparams["training_precision"] = os.environ["CATFISH_TRAINING_PRECISION"]
    if os.environ.get("CATFISH_CLIP_NORM"):                      # global-norm gradient clipping + the non-finite-step guard
        hparams["clip_norm"] = float(os.environ["CATFISH_CLIP_NORM"])
    network = build_model(kind, save=True, **hparams)
    network.initialize_network()
    from . import labelling
    source = labelling.LabelSource.from_env()                    # what both directories hold: labelled reads, event files or move files
    bases = os.environ.get("CATFISH_VALIDATION_BASES") or "0"
    if bases != "0":                                             # ... which homopolymers by base and length in bases, one JSON line per round
        if os.environ.get("CATFISH_DEVICE_VALIDATION") != "1" or not source.has_tables:
            raise ValueError("CATFISH_VALIDATION_BASES needs CATFISH_DEVICE_VALIDATION=1 and CATFISH_LABEL_KMER (reads with event tables)")
        network.validation_max_bases = MAX_BASES if bases == "1" else check_max_bases(int(bases))
    votes = os.environ.get("CATFISH_VALIDATION_VOTES") or "0"
    if votes != "0":                                             # ... and the per-base calls, one JSON line per round
        if os.environ.get("CATFISH_DEVICE_VALIDATION") != "1" or not source.has_tables:
            raise ValueError("CATFISH_VALIDATION_VOTES needs CATFISH_DEVICE_VALIDATION=1 and CATFISH_LABEL_KMER or CATFISH_LABEL_MOVES "
                             "(reads with event or move tables)")
        network.validation_vote_bases = MAX_BASES if votes == "1" else check_max_bases(int(votes))
    loader = source.loader()                                     # load_npz, or event / move files labelled on the way in
    with_loader = {"loader": loader} if source.has_tables else {}
    print("Loading training database..")
    if os.environ.get("CATFISH_DEVICE_DB") == "1":               # the training set on the card, batches drawn by a HIP kernel
        from .device_db import device_db_from_npz
        db_train = device_db_from_npz(_npz_files(train_dir), **with_loader)
    elif os.environ.get("CATFISH_DEVICE_DB") == "reads":         # the labelled reads as they are, two tables of window starts: a HOST database
        db_train = device_read_db_from_env(_npz_files(train_dir))
    elif os.environ.get("CATFISH_DEVICE_DB") == "tiled":         # the windows the caller cuts, labels per sample: a HOST database
        db_train = device_tiled_db_from_env(_npz_files(train_dir))
    else:
        db_train = example_db_from_npz(_npz_files(train_dir), **with_loader)
    if source.has_tables:
        network.validation_loader = loader
    print("Loading validation database..")
    squiggles = _npz_files(val_dir)
    if os.environ.get("CATFISH_DEVICE_VALIDATION") == "1":       # the validation reads on the card, rounds scored by HIP kernels
        from .device_validation import DeviceValidationSet
        squiggles = DeviceValidationSet.from_source(squiggles, source)
        if os.environ.get("CATFISH_VALIDATION_RUNS") == "1":     # ... and the homopolymers found, one JSON line per round
            network.validation_run_edges = VALIDATION_RUN_EDGES
        if os.environ.get("CATFISH_VALIDATION_CURVE") == "1":    # ... and the round's ROC / PR areas and best F1, one JSON line per round
            network.validation_curve_shift = VALIDATION_CURVE_SHIFT
        borders = os.environ.get("CATFISH_VALIDATION_BORDERS") or "0"
        if borders != "0":                                       # ... and how far the called borders miss, one JSON line per round
            network.validation_border_reach = BORDER_REACH if borders == "1" else check_border_reach(int(borders))
        if os.environ.get("CATFISH_VALIDATION_SCORES") == "1":   # ... and what the samples under the runs scored, one JSON line per round
            network.validation_score_shift = RUN_SCORE_SHIFT
        bridge = int(os.environ.get("CATFISH_VALIDATION_BRIDGE") or "0")
        if bridge:                                               # ... both counted on the bridged prediction
            from .infer import check_bridge
            network.validation_bridge_gap = check_bridge(bridge, 15)
            if not _bridged(_given(**{option: getattr(network, "validation_" + option, None) for option in REPORTS})):
                raise ValueError("CATFISH_VALIDATION_BRIDGE needs CATFISH_VALIDATION_RUNS=1 or CATFISH_VALIDATION_BORDERS")
    began = datetime.datetime.now()
    train_and_validate(network, db_train, n_train, squiggles, stretch, network.model_path, start, most)
    print("Trained and validated network in {}".format(datetime.datetime.now() - began))
    print("Finished script at ", datetime.datetime.now())


if __name__ == "__main__":
    import sys
    main(sys.argv)
