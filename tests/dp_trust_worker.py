"""One data-parallel rank of tests/test_dp_trust_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_wd_worker.py does).

part 1: two eager steps of FusedLAMB (SOLVER.optim lamb, the biases and BatchNorm affine parameters exempt from the decay and from the
trust ratio) on this rank's shard, recording this rank's own gradients (the parent checks the result against the fp64 oracle on the mean
of both ranks' gradients) and the sizes of the all-reduces inside each optimiser step (the early bucket consumed: no all-reduce of the
whole buffer).  part 2: the same two steps through the graphed Solver."""
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
from electrocardio_panorama_amd.solver.optim_scheduler import FusedLAMB, get_optimizer  # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_model_gpu import make_cfg                                          # noqa: E402

out_dir = sys.argv[1]
rank, world, local = parallel.init_from_env()
assert world == 2 and dist.is_initialized()
dev = torch.device("cuda", local)
V, B, L, seed, steps = 3, 4, 512, 5, 2
WD, NO_DECAY = 1e-2, ["*.bias", "decoder.*.double_conv.[14].weight"]
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]


def solver(graph):
    cfg = make_cfg(V, lr=1e-3)
    cfg.SOLVER["optim"] = "lamb"
    cfg.SOLVER["weight_decay"] = WD
    cfg.SOLVER["no_decay"] = list(NO_DECAY)
    cfg.SOLVER["trust_exempt"] = list(NO_DECAY)
    cfg.SOLVER["graph"] = graph
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedLAMB)
    return cfg, sol, opt


def flat(opt, key):
    return opt._flat[0][key].detach().cpu().numpy().copy()


# ---------------------------------------------------------------- part 1: eager
cfg, sol, opt = solver(False)
sol.model.train()
lossf = build_loss(cfg)
names = [n for n, _ in sol.model.named_parameters()]
grads, reduced, early = [], [], []
real_all_reduce = dist.all_reduce
for s in range(steps):
    b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in parallel.shard_batch(fulls[s], rank, world).items()}
    random.seed(seed + s)
    o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
    lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
    live = [n for n, p in sol.model.named_parameters() if p.grad is not None]
    grads.append(torch.cat([p.grad.detach().reshape(-1) for p in sol.model.parameters() if p.grad is not None]).cpu().numpy())
    pend = parallel._EARLY["pending"]
    early.append(0 if pend is None else len(pend["names"]))
    sizes = []

    def counting(t, *a, **k):
        sizes.append(t.numel())
        return real_all_reduce(t, *a, **k)
    dist.all_reduce = counting
    try:
        opt.step()
    finally:
        dist.all_reduce = real_all_reduce
    opt.zero_grad()
    reduced.append(max(sizes) if sizes else 0)
np.savez(os.path.join(out_dir, f"eager_rank{rank}.npz"), grads=np.stack(grads), live=np.array(live), names=np.array(names),
         p=flat(opt, "p"), m=flat(opt, "m"), v=flat(opt, "v"), step=flat(opt, "step"), reduced=np.array(reduced),
         early=np.array(early), n=np.array(opt._flat[0]["p"].numel()), wd=np.array(WD), no_decay=np.array(NO_DECAY),
         sizes=np.array([dict(sol.model.named_parameters())[k].numel() for k in live]),
         seg_end=flat(opt, "seg_end"), seg_wd_mul=flat(opt, "seg_wd_mul"), seg_adapt=flat(opt, "seg_adapt"), ratio=flat(opt, "ratio"),
         trust_stats=flat(opt, "trust_stats"),
         p0=torch.cat([hw.hashed_params(V)[n].reshape(-1) for n in live]).numpy())
dist.barrier()

# ---------------------------------------------------------------- part 2: the same steps through the graphed Solver
cfg, sol_g, opt_g = solver(True)
for s in range(steps):
    random.seed(seed + s)
    sol_g.run_one_epoch(parallel.ShardedLoader([fulls[s]]), "train", opt_g, collect_views=False)
assert sol_g._graph_stepper is not None and sol_g._graph_stepper.calls == steps
np.savez(os.path.join(out_dir, f"graph_rank{rank}.npz"), p=flat(opt_g, "p"), m=flat(opt_g, "m"), v=flat(opt_g, "v"),
         step=flat(opt_g, "step"), ratio=flat(opt_g, "ratio"), trust_stats=flat(opt_g, "trust_stats"))
dist.barrier()
dist.destroy_process_group()
print("DPTRUST_OK", rank)
