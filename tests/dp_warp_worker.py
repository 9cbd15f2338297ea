"""One data-parallel rank of tests/test_dp_warp_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_augment_worker.py does).

Three train steps with DATA.aug_warp and DATA.aug_roi_jitter on, on this rank's shard of three global batches whose two halves are the
SAME samples -- the ranks read identical batches, so whatever differs between their warped batches is the per-rank seed: once as an eager
epoch of the Solver, once as a graphed epoch.  The parent compares the ranks and the two paths."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import ops, parallel, synth, warp            # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_augment_gpu import make_cfg                                        # noqa: E402
from test_warp_gpu import WARP                                               # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 3
batches = []
for i in range(steps):
    half = synth.make_batch(B // 2, V, L, seed=seed + i, Q=5)
    batches.append({k: np.concatenate([v, v], axis=0) for k, v in half.items()})

for graph in (False, True):
    torch.manual_seed(1234)
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.1, data=WARP, make_cfg=make_cfg)
    fed, real = [], ops.warp
    ops.warp = lambda *a, **k: (lambda res: (fed.append((a[5], res[0].clone(), res[3].clone())), res)[1])(real(*a, **k))
    random.seed(seed)
    try:
        rows = sol.run_one_epoch(parallel.ShardedLoader(batches), "train", opt, collect_views=False)[0]
    finally:
        ops.warp = real
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    assert [s for s, _, _ in fed] == [warp.train_seed(cfg.seed, 0, i, rank) for i in range(steps)]
    h0 = hw.hashed_params(V)
    moved = sum(not torch.equal(p.detach().cpu(), h0[n]) for n, p in sol.model.named_parameters())
    dpc.save("graph" if graph else "eager", **dpc.flats(opt, "p", "buf"), losses=np.array(rows), moved=np.array(moved),
             fed_last=fed[-1][1].cpu().numpy(), rois_last=fed[-1][2].cpu().numpy(), n_fed=np.array(len(fed)),
             clean_last=batches[-1]["data"][rank * (B // 2):(rank + 1) * (B // 2)])
dpc.finish("DPWARP")
