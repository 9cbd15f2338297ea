"""One data-parallel rank of tests/test_dp_ema_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_wd_worker.py does).

part 1: two eager steps of FusedSGD with SOLVER.ema_decay (warm-up on, decay and exempt tensors on as well: one launch carries all of it)
on this rank's shard, saving the flat parameters after every step.  part 2: the same two steps through the graphed Solver."""
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
from electrocardio_panorama_amd.solver import Solver                         # noqa: E402
from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD, get_optimizer  # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_model_gpu import make_cfg                                          # noqa: E402

out_dir = sys.argv[1]
rank, world, local = parallel.init_from_env()
assert world == 2 and dist.is_initialized()
V, B, L, seed, steps = 3, 4, 512, 5, 2
DECAY, WARMUP = 0.9, True
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]


def solver(graph):
    cfg = make_cfg(V, lr=0.1)
    cfg.SOLVER["weight_decay"] = 1e-2
    cfg.SOLVER["no_decay"] = ["*.bias", "decoder.*.double_conv.[14].weight"]
    cfg.SOLVER["ema_decay"] = DECAY
    cfg.SOLVER["ema_warmup"] = WARMUP
    cfg.SOLVER["graph"] = graph
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedSGD) and opt.ema_decay == DECAY
    return cfg, sol, opt


def flat(opt, key):
    return opt._flat[0][key].detach().cpu().numpy().copy()


def run(graph):
    cfg, sol, opt = solver(graph)
    traj = []
    for s in range(steps):
        random.seed(seed + s)
        sol.run_one_epoch(parallel.ShardedLoader([fulls[s]]), "train", opt, collect_views=False)
        traj.append(flat(opt, "p"))
    assert (sol._graph_stepper is not None and sol._graph_stepper.calls == steps) if graph else getattr(sol, "_graph_stepper", None) is None
    live = [p._nef_name for p in opt._flat[0]["params"]]
    return dict(traj=np.stack(traj), p=flat(opt, "p"), buf=flat(opt, "buf"), ema=flat(opt, "ema"), ema_n=flat(opt, "ema_n"),
                p0=torch.cat([hw.hashed_params(V)[n].reshape(-1) for n in live]).numpy(), decay=np.array(DECAY), warmup=np.array(WARMUP))


np.savez(os.path.join(out_dir, f"eager_rank{rank}.npz"), **run(False))
dist.barrier()
np.savez(os.path.join(out_dir, f"graph_rank{rank}.npz"), **run(True))
dist.barrier()
dist.destroy_process_group()
print("DPEMA_OK", rank)
