"""One data-parallel rank of tests/test_dp_views_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_loss_term_worker.py does).

Two train steps with SOLVER.train_views 2 (of 5 supervised rest views) on this rank's shard of two global batches: once as an eager
epoch of the Solver, once as a graphed epoch (two graphs per step, the early bucket's all-reduce between the replays).  The parent compares
the ranks and the two paths."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import parallel, synth                       # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_views_gpu import make_cfg                                          # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, Q, seed = 3, 4, 512, 2, 5
batches = [synth.make_batch(B, V, L, seed=seed + i, Q=5) for i in range(2)]

for graph in (False, True):
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.1, solver=dict(train_views=Q), make_cfg=make_cfg)
    random.seed(seed)
    rows = sol.run_one_epoch(parallel.ShardedLoader(batches), "train", opt, collect_views=False)[0]
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    if graph:
        assert st.calls == 2 and len(st.slots) == 1 and isinstance(next(iter(st.slots.values()))["graph"], tuple)      # the two-graph capture
        assert st.q_theta.shape == (Q, B // world, 2)
    h0 = hw.hashed_params(V)
    moved = sum(not torch.equal(p.detach().cpu(), h0[n]) for n, p in sol.model.named_parameters())
    nbt = int(dict(sol.model.named_buffers())["decoder.1.double_conv.1.num_batches_tracked"])
    dpc.save("graph" if graph else "eager", **dpc.flats(opt, "p", "buf"), losses=np.array(rows), nbt=np.array(nbt), moved=np.array(moved))
dpc.finish("DPVIEWS")
