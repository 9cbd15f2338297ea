"""One data-parallel rank of tests/test_dp_augment_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_views_worker.py does).

Three train steps with all four DATA.aug_* corruptions on, on this rank's shard of three global batches whose two halves are the SAME
samples -- the ranks read identical clean inputs, so whatever differs between their corrupted inputs is the per-rank seed: once as an eager
epoch of the Solver, once as a graphed epoch (two graphs per step).  The parent compares the ranks and the two paths."""
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from electrocardio_panorama_amd import ops, parallel, synth                  # noqa: E402
from electrocardio_panorama_amd.solver import Solver                         # noqa: E402
from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD, get_optimizer  # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402
from test_augment_gpu import ALL, make_cfg                                   # noqa: E402

out_dir = sys.argv[1]
rank, world, local = parallel.init_from_env()
assert world == 2 and dist.is_initialized()
V, B, L, seed, steps = 3, 4, 512, 5, 3
batches = []
for i in range(steps):
    half = synth.make_batch(B // 2, V, L, seed=seed + i, Q=5)
    batches.append({k: np.concatenate([v, v], axis=0) for k, v in half.items()})


def run(graph):
    cfg = make_cfg(V, lr=0.1, graph=graph, data=ALL)
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedSGD)
    fed, real = [], ops.augment
    if not graph:          # the eager path's corrupted inputs (the replayed path launches inside its capture)
        ops.augment = lambda *a, **k: (lambda y: (fed.append(y.clone()), y)[1])(real(*a, **k))
    random.seed(seed)
    try:
        rows = sol.run_one_epoch(parallel.ShardedLoader(batches), "train", opt, collect_views=False)[0]
    finally:
        ops.augment = real
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    if graph:
        assert st.calls == steps and len(st.slots) == 1 and isinstance(next(iter(st.slots.values()))["graph"], tuple)      # the two-graph capture
        fed = [st.data_aug.clone()]          # the last step's
    fl = opt._flat[0]
    h0 = hw.hashed_params(V)
    moved = sum(not torch.equal(p.detach().cpu(), h0[n]) for n, p in sol.model.named_parameters())
    np.savez(os.path.join(out_dir, f"{'graph' if graph else 'eager'}_rank{rank}.npz"), p=fl["p"].detach().cpu().numpy(),
             buf=fl["buf"].detach().cpu().numpy(), losses=np.array(rows), moved=np.array(moved),
             fed_last=fed[-1].cpu().numpy(), n_fed=np.array(len(fed)), clean_last=batches[-1]["data"][rank * (B // 2):(rank + 1) * (B // 2)])
    dist.barrier()


run(False)
run(True)
dist.destroy_process_group()
print("DPAUGMENT_OK", rank)
