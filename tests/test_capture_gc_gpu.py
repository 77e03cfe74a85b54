"""No finaliser runs while ``Trainer._capture_step`` captures a step into a HIP graph.  ``torch.cuda.graph`` collects garbage on
entry only under ``torch.compiler.config.force_cudagraph_gc``; a dead cycle reached by the cyclic collector in the middle of a
capture is finalised there, and a finaliser that frees device objects (an earlier trainer's graph, an engine) aborts the process.
The test plants harmless garbage -- a cycle whose finaliser only notes whether the stream was capturing -- before and inside the
captured step, with the collector set to run at every allocation."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_no_finaliser_runs_inside_a_capture(ckpt_weights):
    import torch
    from catfish_amd.training import Trainer
    seen = []

    class Cycle(object):
        def __init__(self):
            self.me = self

        def __del__(self):
            seen.append(bool(torch.cuda.is_current_stream_capturing()))

    tr = Trainer(ckpt_weights, 3, 2, "RMSProp", 1e-3, 0.8, seed=5)
    assert tr.use_graph
    run = tr.step.run

    def littering(b, *args, **kw):                         # garbage born inside the warm-ups and inside the captured step
        Cycle()
        return run(b, *args, **kw)

    tr.step.run = littering
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((64, 35)).astype(np.float32), (rng.random((64, 35)) < 0.3).astype(np.float32)
    Cycle()                                                # ... and garbage that is already dead when the capture begins
    was = gc.get_threshold()
    gc.set_threshold(1, 10 ** 6, 10 ** 6)                  # a young collection at every allocation of a container object
    try:
        loss = tr.train_step(x, y)
    finally:
        gc.set_threshold(*was)
    gc.collect()
    if tr.engine is not None:
        tr.engine.close()
    assert np.isfinite(loss)
    assert len(seen) >= 4 and not any(seen), seen           # all four were finalised, none of them while the stream captured
