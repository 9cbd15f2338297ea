"""One data-parallel rank of tests/test_dp_device_noise_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_augment_worker.py
does).

Three train steps with DATA.device_noise on, on this rank's shard of three global batches whose two halves are the SAME samples -- the
ranks read identical targets and rois, so whatever differs between their noise rows is the per-rank seed: once as an eager epoch of the
Solver, once as a graphed epoch (two graphs per step).  The parent compares the ranks and the two paths."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import ops, parallel, synth                  # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_augment_gpu import make_cfg                                        # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 3
batches = []
for i in range(steps):
    half = synth.make_batch(B // 2, V, L, seed=seed + i, Q=5)
    batches.append({k: np.concatenate([v, v], axis=0) for k, v in half.items()})

for graph in (False, True):
    torch.manual_seed(1234)
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.1, data=dict(device_noise=True), make_cfg=make_cfg)
    rows_fed, real = [], ops.noise_row
    if not graph:          # the eager path's rows (the replayed path launches inside its capture)
        ops.noise_row = lambda *a, **k: (lambda y: (rows_fed.append(y.clone()), y)[1])(real(*a, **k))
    random.seed(seed)
    try:
        rows = sol.run_one_epoch(parallel.ShardedLoader(batches), "train", opt, collect_views=False)[0]
    finally:
        ops.noise_row = real
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    if graph:
        assert st.calls == steps and len(st.slots) == 1 and isinstance(next(iter(st.slots.values()))["graph"], tuple)      # the two-graph capture
        rows_fed = [st.noise.clone()]          # the last step's
    h0 = hw.hashed_params(V)
    moved = sum(not torch.equal(p.detach().cpu(), h0[n]) for n, p in sol.model.named_parameters())
    dpc.save("graph" if graph else "eager", **dpc.flats(opt, "p", "buf"), losses=np.array(rows), moved=np.array(moved),
             row_last=rows_fed[-1].reshape(B // 2, L).cpu().numpy(), n_rows=np.array(len(rows_fed)),
             target_last=batches[-1]["target_view"][rank * (B // 2):(rank + 1) * (B // 2)])
dpc.finish("DPDEVICENOISE")
