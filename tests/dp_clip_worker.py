"""One data-parallel rank of tests/test_dp_clip_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_adam_worker.py does).

part 1: two eager steps of FusedSGD with clip_grad_norm = 0.25 on this rank's shard, recording this rank's own gradients (the parent
checks the result against torch's clip_grad_norm_ + SGD on the mean of both ranks' gradients), the norm and coefficient of every step
and the sizes of the all-reduces inside each optimiser step (the early bucket consumed: no all-reduce of the whole buffer).
part 2: the same two steps through the graphed Solver."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import synth                                 # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 2
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]


def solver(graph):
    return dpc.make_solver(V, graph, lr=0.1, solver=dict(clip_grad_norm=0.25), check=lambda opt: opt.max_grad_norm == 0.25)


# ---------------------------------------------------------------- part 1: eager
cfg, sol, opt = solver(False)
clips = []
recorded = dpc.eager_steps(cfg, sol, opt, fulls, V, seed, after_step=lambda: clips.append(opt.clip_stats[:2].tolist()))
dpc.save("eager", **recorded, **dpc.flats(opt, "p", "buf"), clips=np.array(clips))

# ---------------------------------------------------------------- part 2: the same steps through the graphed Solver
cfg, sol_g, opt_g = solver(True)
clips = []
dpc.one_batch_epochs(sol_g, opt_g, fulls, seed, True, each=lambda res: clips.extend(sol_g.last_grad_norms))
dpc.save("graph", **dpc.flats(opt_g, "p", "buf"), clips=np.array(clips))
dpc.finish("DPCLIP")
