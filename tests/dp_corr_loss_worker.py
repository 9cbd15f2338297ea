"""One data-parallel rank of tests/test_dp_corr_loss_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_accum_worker.py does).

One train step with SOLVER.corr_factor 5.0, corr_crop true on this rank's shard of the global batch.  part 1: eagerly by hand -- model,
losswrapper(rois=), backward, FusedSGD.step() -- recording this rank's own gradient, its prediction and loss row and the parameters behind
the update.  part 2: the same batch as one epoch of the graphed Solver.  The parent compares the ranks, the two paths, the update with the
mean of the two recorded gradients and each rank's term with the fp64 restatement on that rank's rows."""
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from electrocardio_panorama_amd import parallel, synth                       # noqa: E402
from electrocardio_panorama_amd.network import build_loss                    # noqa: E402
from electrocardio_panorama_amd.solver import Solver                         # noqa: E402
from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD, get_optimizer  # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_model_gpu import make_cfg                                          # noqa: E402

out_dir = sys.argv[1]
rank, world, local = parallel.init_from_env()
assert world == 2 and dist.is_initialized()
dev = torch.device("cuda", local)
# lr = 1: the displacement check against fp64 wants the update large beside the parameters' own fp32 rounding (tests/dp_accum_worker.py)
V, B, L, seed, LR, FACTOR = 3, 4, 512, 5, 1.0, 5.0
full = synth.make_batch(B, V, L, seed=seed, Q=2)


def solver(graph):
    cfg = make_cfg(V, lr=LR)
    cfg.SOLVER.update(graph=graph, corr_factor=FACTOR, corr_crop=True, corr_eps=1e-8)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedSGD)
    return cfg, sol, opt


def flat(opt, key):
    return opt._flat[0][key].detach().cpu().numpy().copy()


# ---------------------------------------------------------------- part 1: eager, by hand
cfg, sol, opt = solver(False)
sol.model.train()
lossf = build_loss(cfg)
random.seed(seed)
b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in parallel.shard_batch(full, rank, world).items()}
o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
losses = lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg, rois=b["rois"])
assert len(losses) == 5
losses[0].backward()
live = [n for n, p in sol.model.named_parameters() if p.grad is not None]
grad = torch.cat([p.grad.detach().reshape(-1) for p in sol.model.parameters() if p.grad is not None]).cpu().numpy()
opt.step()
opt.zero_grad()
np.savez(os.path.join(out_dir, f"eager_rank{rank}.npz"), grad=grad, p=flat(opt, "p"), buf=flat(opt, "buf"), lr=np.array(LR),
         losses=torch.stack([t.detach() for t in losses]).cpu().numpy(), pred=o[0].detach().cpu().numpy(),
         target=b["target_view"].cpu().numpy(), rois=b["rois"].cpu().numpy(),
         p0=torch.cat([hw.hashed_params(V)[n].reshape(-1) for n in live]).numpy())
dist.barrier()

# ---------------------------------------------------------------- part 2: the same batch as one epoch of the graphed Solver
cfg, sol_g, opt_g = solver(True)
random.seed(seed)
rows = sol_g.run_one_epoch(parallel.ShardedLoader([full]), "train", opt_g, collect_views=False)[0]
st = sol_g._graph_stepper
assert st is not None and st.calls == 1 and len(st.slots) == 1 and st.losses.numel() == 5
np.savez(os.path.join(out_dir, f"graph_rank{rank}.npz"), p=flat(opt_g, "p"), buf=flat(opt_g, "buf"), losses=np.array(rows))
dist.barrier()
dist.destroy_process_group()
print("DPCORR_OK", rank)
