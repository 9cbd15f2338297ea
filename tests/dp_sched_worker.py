"""One data-parallel rank of tests/test_dp_sched_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_accum_worker.py does).

Per mode (eager, graphed): four updates of FusedSGD under the per-update schedule (W = 2, N = 6, cosine) through Solver.run_one_epoch on
this rank's shards; then a clamp counted on rank 1 ONLY in front of a fifth batch -- the summed taint word must skip the update, and with
it the schedule, on both ranks; then a clean sixth batch.  The parameters, the momentum, the count t and the rate word are recorded
behind each of the three."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import ops, parallel, synth                  # noqa: E402
from electrocardio_panorama_amd.solver import Solver                         # noqa: E402
from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD, get_optimizer  # noqa: E402
from test_model_gpu import make_cfg                                          # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, LR = 3, 4, 512, 5, 0.1
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(6)]


def solver(graph):          # (the default weights, not the hashed ones: not dpc.make_solver)
    cfg = make_cfg(V, lr=LR)
    cfg.SOLVER.update(graph=graph, warmup_updates=2, lr_shape="cosine", total_updates=6, lr_floor=0.1)
    torch.manual_seed(1234)                     # the same default weights on both ranks
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedSGD) and opt._sched_on
    return sol, opt


def record(opt, into, tag):
    t, lr = opt.lr_state()
    into.update({f"p_{tag}": dpc.flat(opt, "p"), f"buf_{tag}": dpc.flat(opt, "buf"), f"t_{tag}": np.array(t),
                 f"lr_{tag}": np.array(lr, dtype=np.float32)})


for graph in (False, True):
    sol, opt = solver(graph)
    z = {}
    random.seed(seed)
    sol.run_one_epoch(parallel.ShardedLoader(fulls[:4]), "train", opt, collect_views=False)
    assert (getattr(sol, "_graph_stepper", None) is not None) == graph
    record(opt, z, "four")
    ops.h2_clamped(), ops.h2_skipped()          # (reset the host's marks)
    if rank == 1:
        ops._amax_state(dev)["clamped"] += 1    # what a clamping split-fp16 launch on this rank alone does
    random.seed(seed + 1)
    sol.run_one_epoch(parallel.ShardedLoader(fulls[4:5]), "train", opt, collect_views=False)
    record(opt, z, "tainted")
    random.seed(seed + 2)
    sol.run_one_epoch(parallel.ShardedLoader(fulls[5:]), "train", opt, collect_views=False)
    record(opt, z, "clean")
    dpc.save("graph" if graph else "eager", base=np.array(LR), **z)
dpc.finish("DPSCHED")
