"""What every data-parallel worker (tests/dp_*_worker.py: one rank of a two-rank test, started by tests/dp_launch.py) does around
the part it measures.  A worker begins with

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dp_common as dpc
    rank, world, local, dev, out_dir = dpc.start()

builds its solvers with make_solver, hands its arrays to save(mode, ...) -- the parent reads them with dp_launch.load_ranks -- and ends
with finish(tag)."""
import contextlib
import copy
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from electrocardio_panorama_amd import parallel                              # noqa: E402
from electrocardio_panorama_amd.network import build_loss                    # noqa: E402
from electrocardio_panorama_amd.solver import Solver                         # noqa: E402
from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD, get_optimizer  # noqa: E402
from oracle import hashweights as hw                                         # noqa: E402

_rank = _world = _dev = _out_dir = None


def start():
    """Join the process group of the launcher's environment: (rank, world, local rank, this rank's device, the output directory)."""
    global _rank, _world, _dev, _out_dir
    _out_dir = sys.argv[1]
    _rank, _world, local = parallel.init_from_env()
    assert _world == 2 and dist.is_initialized()
    _dev = torch.device("cuda", local)
    return _rank, _world, local, _dev, _out_dir


def make_solver(V, graph, *, lr, solver=None, data=None, optim=FusedSGD, make_cfg=None, check=None):
    """(cfg, Solver, optimiser) on the hashed weights without dropout: make_cfg(V, lr=lr) (tests/test_model_gpu.py's by default) with
    the SOLVER keys `solver`, SOLVER.graph and the DATA keys `data`.  The optimiser must be an `optim`, and `check(opt)` must hold."""
    if make_cfg is None:
        from test_model_gpu import make_cfg
    cfg = make_cfg(V, lr=lr)
    cfg.DATA.update(copy.deepcopy(data or {}))
    cfg.SOLVER.update(copy.deepcopy(solver or {}), graph=graph)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, optim) and (check is None or check(opt))
    return cfg, sol, opt


def flat(opt, key):
    return opt._flat[0][key].detach().cpu().numpy().copy()


def flats(opt, *keys):
    return {k: flat(opt, k) for k in keys}


def live_p0(opt_or_names, V):
    """The hashed initial values of the live parameters, flat in the optimiser's order (given the optimiser, or the live names)."""
    names = opt_or_names if isinstance(opt_or_names, list) else [p._nef_name for p in opt_or_names._flat[0]["params"]]
    h0 = hw.hashed_params(V)
    return torch.cat([h0[n].reshape(-1) for n in names]).numpy()


def live_grad(model):
    """(names of the parameters that have a gradient, those gradients as one flat host array) behind a backward pass."""
    live = [n for n, p in model.named_parameters() if p.grad is not None]
    return live, torch.cat([p.grad.detach().reshape(-1) for p in model.parameters() if p.grad is not None]).cpu().numpy()


def shard_to_device(full, rank, world, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in parallel.shard_batch(full, rank, world).items()}


@contextlib.contextmanager
def all_reduce_sizes():
    """The element count of every dist.all_reduce made inside the block, in order."""
    sizes, real = [], dist.all_reduce

    def counting(t, *a, **k):
        sizes.append(t.numel())
        return real(t, *a, **k)
    dist.all_reduce = counting
    try:
        yield sizes
    finally:
        dist.all_reduce = real


def eager_steps(cfg, sol, opt, fulls, V, seed, after_step=None):
    """One eager train step by hand per global batch -- model, losswrapper, backward, opt.step() on this rank's shard, lead choice seeded
    seed + s -- and what every optimiser worker records of them: this rank's own gradients, the size of the early bucket backward()
    started and the largest all-reduce inside each optimiser step."""
    sol.model.train()
    lossf = build_loss(cfg)
    names = [n for n, _ in sol.model.named_parameters()]
    grads, reduced, early = [], [], []
    for s, full in enumerate(fulls):
        b = shard_to_device(full, _rank, _world, _dev)
        random.seed(seed + s)
        o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
        lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
        live, grad = live_grad(sol.model)
        grads.append(grad)
        pend = parallel._EARLY["pending"]
        early.append(0 if pend is None else len(pend["names"]))
        with all_reduce_sizes() as sizes:
            opt.step()
        opt.zero_grad()
        if after_step is not None:
            after_step()
        reduced.append(max(sizes) if sizes else 0)
    return dict(grads=np.stack(grads), live=np.array(live), names=np.array(names), reduced=np.array(reduced),
                early=np.array(early), n=np.array(opt._flat[0]["p"].numel()), p0=live_p0(live, V))


def one_batch_epochs(sol, opt, fulls, seed, graph, each=None):
    """Solver.run_one_epoch once per global batch (lead choice seeded seed + s), each(its result) behind every one.  Returns the graph
    stepper, which must have run every batch when SOLVER.graph is on and must not exist when it is off."""
    for s, full in enumerate(fulls):
        random.seed(seed + s)
        res = sol.run_one_epoch(parallel.ShardedLoader([full]), "train", opt, collect_views=False)
        if each is not None:
            each(res)
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None and st.calls == len(fulls)) if graph else st is None
    return st


def save(mode, **arrays):
    np.savez(os.path.join(_out_dir, f"{mode}_rank{_rank}.npz"), **arrays)
    dist.barrier()


def finish(tag):
    dist.destroy_process_group()
    print(f"{tag}_OK", _rank)
