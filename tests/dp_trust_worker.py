"""One data-parallel rank of tests/test_dp_trust_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_wd_worker.py does).

part 1: two eager steps of FusedLAMB (SOLVER.optim lamb, the biases and BatchNorm affine parameters exempt from the decay and from the
trust ratio) on this rank's shard, recording this rank's own gradients (the parent checks the result against the fp64 oracle on the mean
of both ranks' gradients) and the sizes of the all-reduces inside each optimiser step (the early bucket consumed: no all-reduce of the
whole buffer).  part 2: the same two steps through the graphed Solver."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import synth                                 # noqa: E402
from electrocardio_panorama_amd.solver.optim_scheduler import FusedLAMB      # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 2
WD, NO_DECAY = 1e-2, ["*.bias", "decoder.*.double_conv.[14].weight"]
KEYS = dict(optim="lamb", weight_decay=WD, no_decay=NO_DECAY, trust_exempt=NO_DECAY)
STATE = ("p", "m", "v", "step", "ratio", "trust_stats")
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]

# ---------------------------------------------------------------- part 1: eager
cfg, sol, opt = dpc.make_solver(V, False, lr=1e-3, solver=KEYS, optim=FusedLAMB)
recorded = dpc.eager_steps(cfg, sol, opt, fulls, V, seed)
dpc.save("eager", **recorded, **dpc.flats(opt, *STATE, "seg_end", "seg_wd_mul", "seg_adapt"), wd=np.array(WD),
         no_decay=np.array(NO_DECAY), sizes=np.array([dict(sol.model.named_parameters())[k].numel() for k in recorded["live"]]))

# ---------------------------------------------------------------- part 2: the same steps through the graphed Solver
cfg, sol_g, opt_g = dpc.make_solver(V, True, lr=1e-3, solver=KEYS, optim=FusedLAMB)
dpc.one_batch_epochs(sol_g, opt_g, fulls, seed, True)
dpc.save("graph", **dpc.flats(opt_g, *STATE))
dpc.finish("DPTRUST")
