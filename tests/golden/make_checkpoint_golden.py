"""Checkpoint fixtures that let the bundle tests run without the reference checkout.

usage: python tests/golden/make_checkpoint_golden.py <reference repository root>

Reads the reference's ``catfish/ResNetRNN/checkpoints/ckpnt-30000.*`` with catfish_amd.checkpoint (every tensor's CRC-32C
verified against the .index) and writes:

* ckpnt-30000-files.json -- size and SHA-256 of the reference's .index file and the size of its .data file.  The tests write
  the bundle from the 74 inference tensors (ckpnt-30000-inference.npz) and stand-ins for the 116 optimizer slots that carry
  the slots' recorded CRC-32Cs (ckpt_table.json); the .index they get must be this one, byte for byte.
* graph_restore_golden.npz -- one optimizer step of the reference's own gradient + ApplyRMSProp subgraph (ckpnt-30000.meta,
  interpreted in fp64 by oracle/tf_graph.py) from ckpnt-30000's variables with the seeded slots of ``synthetic_slots``
  restored, on the first batch of graph_train_golden.npz: ``names`` (the trainable variables), and per variable and result
  (weight change, RMSProp, RMSProp_1; ``RESULTS``) the values at 16 seeded positions (``samples`` [58, 3, 16], NaN past the end of a smaller variable) and the sum,
  the sum of magnitudes and the largest magnitude (``stats`` [58, 3, 3]).
* shipped_report.json -- the hyperparameter header of the report the reference ships beside the checkpoint
  (catfish/ResNetRNN/ResNetRNN.txt: every line before its first ``NEXT EPOCH``).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from catfish_amd import checkpoint  # noqa: E402

NAME = "ckpnt-30000"
SAMPLES = 16
RESULTS = ("delta", "ms", "mom")


def synthetic_slots(table):
    """Seeded RMSProp slots for every variable that has them in ``table`` (ckpt_table.json): ``<var>/RMSProp`` (ms, positive)
    and ``<var>/RMSProp_1`` (mom), float32, the shapes of the real slots."""
    rng = np.random.default_rng(30000)
    out = {}
    for e in sorted(table, key=lambda e: e["name"]):
        if e["name"].endswith("/RMSProp"):
            out[e["name"]] = rng.uniform(1e-6, 1e-3, size=e["shape"]).astype(np.float32)
            out[e["name"] + "_1"] = rng.normal(0.0, 1e-4, size=e["shape"]).astype(np.float32)
    return out


def sample_positions(name, size):
    """The seeded flat positions of variable ``name`` whose values graph_restore_golden.npz keeps."""
    rng = np.random.default_rng(int(hashlib.sha256(name.encode("utf-8")).hexdigest()[:8], 16))
    return np.sort(rng.choice(size, size=min(SAMPLES, size), replace=False))


def restore_step(nodes, variables, table, train_golden):
    from oracle import tf_graph
    variables = dict(variables)
    variables.update(synthetic_slots(table))
    x, y = train_golden["train_x"][0], train_golden["train_y"][0]
    gi = tf_graph.GraphInterpreter(nodes, variables, np.float64)
    applies = sorted(k for k, n in nodes.items() if n.op == "ApplyRMSProp")
    gi.run(applies, {"data/Placeholder": x.reshape(-1, 35, 1), "data/Placeholder_1": y.reshape(-1, 35, 1), "dropout": np.float32(1.0)})
    names, samples, stats = [], [], []
    for k in sorted(variables):
        if not (checkpoint.is_inference_tensor(k) and k + "/RMSProp" in variables):
            continue
        res = {"delta": gi.updates[k] - variables[k].astype(np.float64), "ms": gi.updates[k + "/RMSProp"],
               "mom": gi.updates[k + "/RMSProp_1"]}
        pos = sample_positions(k, variables[k].size)
        vals = [np.asarray(res[r], dtype=np.float64).reshape(-1) for r in RESULTS]
        names.append(k)
        samples.append([np.pad(v[pos], (0, SAMPLES - len(pos)), constant_values=np.nan) for v in vals])
        stats.append([[v.sum(), np.abs(v).sum(), np.abs(v).max()] for v in vals])
    return {"names": np.array(names), "samples": np.array(samples), "stats": np.array(stats)}


def main(ref_root):
    from oracle import tf_graph
    model = os.path.join(ref_root, "catfish", "ResNetRNN")
    prefix = os.path.join(model, "checkpoints", NAME)
    with open(prefix + ".index", "rb") as fh:
        index = fh.read()
    files = {"index": {"bytes": len(index), "sha256": hashlib.sha256(index).hexdigest()},
             "data-00000-of-00001": {"bytes": os.path.getsize(prefix + ".data-00000-of-00001")}}
    with open(os.path.join(HERE, NAME + "-files.json"), "w") as fh:
        json.dump(files, fh, indent=1, sort_keys=True)
        fh.write("\n")

    with open(os.path.join(HERE, "ckpt_table.json")) as fh:
        table = json.load(fh)
    with np.load(os.path.join(HERE, "graph_train_golden.npz")) as z:
        train_golden = {k: z[k] for k in z.files}
    nodes = tf_graph.load_meta_graph(prefix + ".meta")
    np.savez_compressed(os.path.join(HERE, "graph_restore_golden.npz"),
                        **restore_step(nodes, checkpoint.read_checkpoint(prefix), table, train_golden))

    with open(os.path.join(model, "ResNetRNN.txt")) as fh:
        report = fh.read()
    with open(os.path.join(HERE, "shipped_report.json"), "w") as fh:
        json.dump({"header": report[:report.index("NEXT EPOCH")]}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
