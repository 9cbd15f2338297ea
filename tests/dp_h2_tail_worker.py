"""One data-parallel rank of tests/test_dp_h2_tail_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_adam_worker.py
does).  Both ranks run ops.H2_TAIL_MODE = "fp32" with the split-fp16 kernels forced (ops._H2_MIN_WGS = 0); only rank 0 lowers
ops.H2_TAIL_FRAC below 0, so every weight-gradient site of rank 0 routes to the fp32 kernels (reading its census flag on the host in
the middle of the backward pass) and none of rank 1 does.  Two train steps of the Solver, eager and graphed; saved per rank: the
parameters, the sites routed during the run and the weight-gradient sites of the model."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import ops, synth                            # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 2
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]
ops._H2_MIN_WGS = 0
ops.H2_TAIL_MODE = "fp32"
if rank == 0:
    ops.H2_TAIL_FRAC = -1.0


def routed_total():
    """Sites routed so far in this process (the Solver's epoch check reads and resets h2_fallback_sites() itself)."""
    return sum(st["fallback"] for st in ops._AMAX.values())


for graph in (False, True):
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.05)
    n0 = routed_total()
    dpc.one_batch_epochs(sol, opt, fulls, seed, graph)
    blob = sol.model.h2_state()
    dpc.save("graph" if graph else "eager", p=torch.cat([p.detach().reshape(-1) for p in sol.model.parameters()]).cpu().numpy(),
             moved=np.array(routed_total() - n0), n_bww=np.array(sum(1 for k in blob["keys"] if k[2] == "conv_bwd_weight")),
             routed=np.array(sum(blob.get("fp32", []))))
dpc.finish("DPH2TAIL")
