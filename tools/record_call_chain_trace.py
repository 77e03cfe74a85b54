"""Record tests/golden/call_chain_trace.json: what every route from raw reads to homopolymer spans asks of the C ABI, for every option
set of tests/call_chain_routes.py, on the tree this file is run in (an MI355X is needed).  tests/test_call_chain_trace_gpu.py
compares a later tree's calls with the file, entry for entry.

    python tools/record_call_chain_trace.py --commit $(git rev-parse HEAD) [--out FILE]

Record it from the commit whose behaviour is to be kept, i.e. BEFORE a change to the calling chain, never after it."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import call_chain_routes as routes
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", default=None, help="the commit of the tree (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=routes.TRACE_FILE)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, universal_newlines=True,
                                           check=True).stdout.strip()
    from catfish_amd.resnet_class import ResNetRNN
    model = ResNetRNN(batch_size=256, optimizer_choice="RMSProp", learning_rate=0.001, layer_size=64, n_layers=3, keep_prob=0.8,
                      layer_size_res=32, n_layers_res=2)
    with np.load(os.path.join(routes.GOLDEN, "ckpnt-30000-inference.npz")) as z:
        model.set_weights({k: z[k] for k in z.files})
    with np.load(os.path.join(routes.GOLDEN, "golden_read_4096_seed0.npz")) as z:
        dac = z["dac"]
    try:
        traces = routes.record(model, dac)
    finally:
        model.engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("{\n \"recorded_at_commit\": %s,\n \"traces\": {\n" % json.dumps(commit))
        fh.write(",\n".join("  %s: [\n%s\n  ]" % (json.dumps(k), ",\n".join("   " + json.dumps(e) for e in t)) for k, t in traces.items()))
        fh.write("\n }\n}\n")
    print("recorded %d traces, %d calls -> %s" % (len(traces), sum(len(t) for t in traces.values()), args.out))


if __name__ == "__main__":
    main()
