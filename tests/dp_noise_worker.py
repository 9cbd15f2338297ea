"""One data-parallel rank of tests/test_dp_noise_gpu.py (two of these share cuda:0 and talk over gloo, as tests/dp_clip_worker.py does).

Two train steps with cfg.DATA.noise on this rank's shard of the global batch -- the noise rows are sharded with the batch
(parallel.ShardedLoader) -- through the Solver, once eagerly and once through the graphed step; the parent compares the two paths, the
ranks, and each rank's first-step losses with the oracle on that rank's shard."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_common as dpc                                                      # noqa: E402
from electrocardio_panorama_amd import parallel, synth                       # noqa: E402

rank, world, local, dev, out_dir = dpc.start()
V, B, L, seed, steps = 3, 4, 512, 5, 2
fulls = []
for s in range(steps):
    b = dict(synth.make_batch(B, V, L, seed=seed + s, Q=2))
    b["noise"] = np.random.default_rng(9000 + s).normal(0, 0.05, (B, L)).astype(np.float32)
    fulls.append(b)

for graph in (False, True):
    cfg, sol, opt = dpc.make_solver(V, graph, lr=0.1, data=dict(noise=True))
    losses = []
    st = dpc.one_batch_epochs(sol, opt, fulls, seed, graph, each=lambda res: losses.extend(res[0]))
    if graph:
        assert len(st.slots) == 1
        slot = next(iter(st.slots.values()))
        mine = parallel.shard_batch(fulls[-1], rank, world)["noise"]
        assert np.array_equal(slot["noise"].cpu().numpy().reshape(mine.shape), mine)       # this rank's rows, not the other's
    dpc.save("graph" if graph else "eager", **dpc.flats(opt, "p", "buf"), losses=np.array(losses))
dpc.finish("DPNOISE")
