"""One data-parallel rank of tests/test_dp_noise_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_clip_worker.py does).

Two train steps with cfg.DATA.noise on this rank's shard of the global batch -- the noise rows are sharded with the batch
(parallel.ShardedLoader) -- through the Solver, once eagerly and once through the graphed step; the parent compares the two paths, the
ranks, and each rank's first-step losses with the oracle on that rank's shard."""
import os
import random
import sys

import numpy as np
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
fulls = []
for s in range(steps):
    b = dict(synth.make_batch(B, V, L, seed=seed + s, Q=2))
    b["noise"] = np.random.default_rng(9000 + s).normal(0, 0.05, (B, L)).astype(np.float32)
    fulls.append(b)

for graph in (False, True):
    cfg = make_cfg(V, lr=0.1, noise=True)
    cfg.SOLVER["graph"] = graph
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedSGD)
    losses = []
    for s in range(steps):
        random.seed(seed + s)
        losses += sol.run_one_epoch(parallel.ShardedLoader([fulls[s]]), "train", opt, collect_views=False)[0]
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    if graph:
        assert st.calls == steps and len(st.slots) == 1
        slot = next(iter(st.slots.values()))
        mine = parallel.shard_batch(fulls[-1], rank, world)["noise"]
        assert np.array_equal(slot["noise"].cpu().numpy().reshape(mine.shape), mine)       # this rank's rows, not the other's
    fl = opt._flat[0]
    np.savez(os.path.join(out_dir, f"{'graph' if graph else 'eager'}_rank{rank}.npz"), p=fl["p"].detach().cpu().numpy(),
             buf=fl["buf"].detach().cpu().numpy(), losses=np.array(losses))
    dist.barrier()
dist.destroy_process_group()
print("DPNOISE_OK", rank)
