"""One data-parallel rank of tests/test_dp_views_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_ssim_loss_worker.py does).

Two train steps with SOLVER.train_views 2 (of 5 supervised rest views) on this rank's shard of two global batches: once as an eager
epoch of the Solver, once as a graphed epoch (two graphs per step, the early bucket's all-reduce between the replays).  The parent compares
the ranks and the two paths."""
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
from test_views_gpu import make_cfg                                          # noqa: E402

out_dir = sys.argv[1]
rank, world, local = parallel.init_from_env()
assert world == 2 and dist.is_initialized()
V, B, L, Q, seed = 3, 4, 512, 2, 5
batches = [synth.make_batch(B, V, L, seed=seed + i, Q=5) for i in range(2)]


def run(graph):
    cfg = make_cfg(V, lr=0.1, graph=graph, train_views=Q)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedSGD)
    random.seed(seed)
    rows = sol.run_one_epoch(parallel.ShardedLoader(batches), "train", opt, collect_views=False)[0]
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == graph
    if graph:
        assert st.calls == 2 and len(st.slots) == 1 and isinstance(next(iter(st.slots.values()))["graph"], tuple)      # the two-graph capture
        assert st.q_theta.shape == (Q, B // world, 2)
    fl = opt._flat[0]
    h0 = hw.hashed_params(V)
    moved = sum(not torch.equal(p.detach().cpu(), h0[n]) for n, p in sol.model.named_parameters())
    nbt = int(dict(sol.model.named_buffers())["decoder.1.double_conv.1.num_batches_tracked"])
    np.savez(os.path.join(out_dir, f"{'graph' if graph else 'eager'}_rank{rank}.npz"), p=fl["p"].detach().cpu().numpy(),
             buf=fl["buf"].detach().cpu().numpy(), losses=np.array(rows), nbt=np.array(nbt),
             moved=np.array(moved))
    dist.barrier()


run(False)
run(True)
dist.destroy_process_group()
print("DPVIEWS_OK", rank)
