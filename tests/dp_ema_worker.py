"""One data-parallel rank of tests/test_dp_ema_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_wd_worker.py does).

part 1: two eager steps of FusedSGD with SOLVER.ema_decay (warm-up on, decay and exempt tensors on as well: one launch carries all of it)
on this rank's shard, saving the flat parameters after every step.  part 2: the same two steps through the graphed Solver."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import synth                                 # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 2
DECAY, WARMUP = 0.9, True
KEYS = dict(weight_decay=1e-2, no_decay=["*.bias", "decoder.*.double_conv.[14].weight"], ema_decay=DECAY, ema_warmup=WARMUP)
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]

for graph in (False, True):
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.1, solver=KEYS, check=lambda opt: opt.ema_decay == DECAY)
    traj = []
    dpc.one_batch_epochs(sol, opt, fulls, seed, graph, each=lambda res: traj.append(dpc.flat(opt, "p")))
    dpc.save("graph" if graph else "eager", traj=np.stack(traj), **dpc.flats(opt, "p", "buf", "ema", "ema_n"), p0=dpc.live_p0(opt, V),
             decay=np.array(DECAY), warmup=np.array(WARMUP))
dpc.finish("DPEMA")
