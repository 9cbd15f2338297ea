"""One data-parallel rank of tests/test_dp_{ssim,slope,corr,seg}_loss_gpu.py: `dp_loss_term_worker.py <out> <term>` (two of these share
cuda:0 and talk over gloo, as tests/dp_accum_worker.py does).

One train step with the SOLVER keys of TERMS[term] on this rank's shard of the global batch.  part 1: eagerly by hand -- model,
losswrapper(rois=), backward, FusedSGD.step() -- recording this rank's own gradient, its prediction and loss row and the parameters behind
the update.  part 2: the same batch as one epoch of the graphed Solver.  The parent compares the ranks, the two paths, the update with the
mean of the two recorded gradients and each rank's term with the fp64 restatement on that rank's rows."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import parallel, synth                       # noqa: E402
from electrocardio_panorama_amd.network import build_loss                    # noqa: E402

# term: the SOLVER keys, the length of the loss row (the segment weights reweigh term 3: no fifth entry), the tag of the last line
TERMS = {
    "ssim": (dict(ssim_factor=0.5, ssim_crop=True), 5, "DPSSIM"),
    "slope": (dict(slope_factor=5.0, slope_loss="l1_loss", slope_crop=True), 5, "DPSLOPE"),
    "corr": (dict(corr_factor=5.0, corr_crop=True, corr_eps=1e-8), 5, "DPCORR"),
    "seg": (dict(seg_weights=[1.0, 1.0, 3.0, 2.0, 1.0, 1.0, 0.0]), 4, "DPSEG"),
}
keys, row_len, tag = TERMS[sys.argv[2]]
weights = keys.get("seg_weights")
rank, world, local, dev, out_dir = dpc.start()
# lr = 1: the displacement check against fp64 wants the update large beside the parameters' own fp32 rounding (tests/dp_accum_worker.py)
V, B, L, seed, LR = 3, 4, 512, 5, 1.0
full = synth.make_batch(B, V, L, seed=seed, Q=2)

# ---------------------------------------------------------------- part 1: eager, by hand
cfg, sol, opt = dpc.make_solver(V, False, lr=LR, solver=keys)
sol.model.train()
lossf = build_loss(cfg)
random.seed(seed)
b = dpc.shard_to_device(full, rank, world, dev)
o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
losses = lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg, rois=b["rois"])
assert len(losses) == row_len
losses[0].backward()
live, grad = dpc.live_grad(sol.model)
opt.step()
opt.zero_grad()
dpc.save("eager", grad=grad, p=dpc.flat(opt, "p"), buf=dpc.flat(opt, "buf"), lr=np.array(LR),
         losses=torch.stack([t.detach() for t in losses]).cpu().numpy(), pred=o[0].detach().cpu().numpy(),
         target=b["target_view"].cpu().numpy(), rois=b["rois"].cpu().numpy(), p0=dpc.live_p0(live, V),
         **({} if weights is None else {"weights": np.array(weights)}))

# ---------------------------------------------------------------- part 2: the same batch as one epoch of the graphed Solver
cfg, sol_g, opt_g = dpc.make_solver(V, True, lr=LR, solver=keys)
random.seed(seed)
rows = sol_g.run_one_epoch(parallel.ShardedLoader([full]), "train", opt_g, collect_views=False)[0]
st = sol_g._graph_stepper
assert st is not None and st.calls == 1 and len(st.slots) == 1 and st.losses.numel() == row_len
assert weights is None or st.seg_weights == tuple(weights)
dpc.save("graph", p=dpc.flat(opt_g, "p"), buf=dpc.flat(opt_g, "buf"), losses=np.array(rows))
dpc.finish(tag)
