"""One data-parallel rank of tests/test_dp_accum_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_trust_worker.py does).

part 1: three eager micro-batches of FusedSGD with accum_steps = 2 on this rank's shards -- a window of two and a flushed window of one --
recording this rank's own gradients, the parameters behind the first update and the size of every all-reduce per micro-batch (none on
a micro-batch that does not close a window).  part 2: the same three batches as one epoch of the graphed Solver (two graphs per
micro-batch; the collectives of the window's last micro-batch only), every all-reduce recorded with the stepper's call count."""
import os
import random
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import parallel, synth                       # noqa: E402
from electrocardio_panorama_amd.network import build_loss                    # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
# The learning rate is this test's to choose, and the displacement check against fp64 decides it: fp32 parameters of rms 5.8e-2 carry a
# rounding of 2^-24 * |p| whatever the update computes, and the gradients of these batches have rms 2.7e-4, so the correctly rounded
# result alone sits at 4.5e-6 / lr of the displacement lr * mean(g).  lr = 1 puts that floor at half the 1e-5 bar (lr = 0.1 would put it
# at 4.5 times the bar, for any update that stores fp32 parameters); what the update's own arithmetic adds is ~1e-7.
V, B, L, seed, steps, K, LR = 3, 4, 512, 5, 3, 2, 1.0
fulls = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]


def solver(graph):
    return dpc.make_solver(V, graph, lr=LR, solver=dict(accum_steps=K), check=lambda opt: opt.accum_steps == K)


# ---------------------------------------------------------------- part 1: eager
cfg, sol, opt = solver(False)
sol.model.train()
lossf = build_loss(cfg)
grads, reduced, p_first = [], [], None
random.seed(seed)
for s in range(steps):
    b = dpc.shard_to_device(fulls[s], rank, world, dev)
    o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
    lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
    live, grad = dpc.live_grad(sol.model)
    grads.append(grad)
    assert parallel._EARLY["pending"] is None          # an accumulating optimiser does not opt in to the early bucket
    with dpc.all_reduce_sizes() as sizes:
        opt.step()
        if s == steps - 1:
            assert opt.window_open
            n_before = len(sizes)
            opt.flush()                                    # the epoch ends inside a window: one micro-batch, gscale 1 / (world * 1)
            flush_sizes = sizes[n_before:]
            del sizes[n_before:]
    opt.zero_grad()
    reduced.append(max(sizes) if sizes else 0)
    if s == K - 1:
        assert not opt.window_open
        p_first = dpc.flat(opt, "p")
dpc.save("eager", grads=np.stack(grads), live=np.array(live), p=dpc.flat(opt, "p"), buf=dpc.flat(opt, "buf"), p_first=p_first,
         reduced=np.array(reduced), flush_reduced=np.array(flush_sizes), n=np.array(opt._flat[0]["p"].numel()), lr=np.array(LR),
         p0=dpc.live_p0(live, V))

# ---------------------------------------------------------------- part 2: the same batches as one epoch of the graphed Solver
cfg, sol_g, opt_g = solver(True)
calls, real_all_reduce = [], dist.all_reduce


def counting_g(t, *a, **k):
    calls.append((sol_g._graph_stepper.calls, t.numel()))
    return real_all_reduce(t, *a, **k)


random.seed(seed)
dist.all_reduce = counting_g
try:
    sol_g.run_one_epoch(parallel.ShardedLoader(fulls), "train", opt_g, collect_views=False)
finally:
    dist.all_reduce = real_all_reduce
st = sol_g._graph_stepper
assert st is not None and st.calls == steps and len(st.slots) == 1 and not opt_g.window_open
assert isinstance(next(iter(st.slots.values()))["graph"], tuple)      # two graphs per micro-batch
assert sol_g.last_updates == (2, 3)
dpc.save("graph", p=dpc.flat(opt_g, "p"), buf=dpc.flat(opt_g, "buf"), calls=np.array(calls))
dpc.finish("DPACCUM")
