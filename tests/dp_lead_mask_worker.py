"""One data-parallel rank of tests/test_dp_lead_mask_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_augment_worker.py
does).

Two train steps with MODEL.lead_mask and DATA.aug_lead_drop 0.4 on this rank's shard of two global batches whose two halves are the SAME
samples -- the ranks read identical clean inputs, so whatever differs between their masks is the per-rank seed: once as an eager epoch of
the Solver, once as a graphed epoch (two graphs per step).  The parent compares the ranks and the two paths."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import ops, parallel, synth                  # noqa: E402
from test_lead_mask_gpu import ON, make_cfg                                  # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 8, 512, 5, 2
batches = []
for i in range(steps):
    half = synth.make_batch(B // 2, V, L, seed=seed + i, Q=5)
    batches.append({k: np.concatenate([v, v], axis=0) for k, v in half.items()})

for graph in (False, True):
    torch.manual_seed(1234)
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.1, data=ON["data"], make_cfg=lambda V_, lr: make_cfg(V_, lr=lr, model=ON["model"]))
    assert sol.lead_mask is True
    masks, real = [], ops.augment_mask
    if not graph:          # the eager path's masks (the replayed path launches inside its capture)
        ops.augment_mask = lambda *a, **k: (lambda y: (masks.append(y.clone()), y)[1])(real(*a, **k))
    random.seed(seed)
    try:
        rows = sol.run_one_epoch(parallel.ShardedLoader(batches), "train", opt, collect_views=False)[0]
    finally:
        ops.augment_mask = real
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    if graph:
        assert st.calls == steps and len(st.slots) == 1 and isinstance(next(iter(st.slots.values()))["graph"], tuple)      # the two-graph capture
        masks = [st.lead_mask.clone()]          # the last step's
    dpc.save("graph" if graph else "eager", **dpc.flats(opt, "p", "buf"), losses=np.array(rows), mask_last=masks[-1].cpu().numpy(),
             n_masks=np.array(len(masks)))
dpc.finish("DPLEADMASK")
