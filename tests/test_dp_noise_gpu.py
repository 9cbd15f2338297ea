"""cfg.DATA.noise with world_size 2 (two ranks sharing cuda:0 over gloo, the harness of tests/test_dp_clip_gpu.py): the noise rows are
sharded with the batch, the graphed step (two graphs with the early bucket's all-reduce between them) equals the eager one bit for
bit, and every rank's first-step losses are the oracle's on that rank's shard with that shard's noise."""
import os
import random

import numpy as np
import pytest
import torch

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_noise(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_noise"))
    run_ranks(os.path.join(TESTS, "dp_noise_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_noise_graphed_equals_eager_and_ranks_agree(dp_noise):
    eager, graph = dp_noise
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "losses"):
            assert np.array_equal(e[k], g[k]), k
    for pair in (eager, graph):
        for k in ("p", "buf"):
            assert np.array_equal(pair[0][k], pair[1][k]), k
        assert not np.array_equal(pair[0]["losses"], pair[1]["losses"])        # (each rank reports its own shard's losses)


def test_world2_noise_first_step_losses_vs_oracle_per_shard(dp_noise):
    """The bar of test_world2_step_8_leads_vs_per_shard_bn_oracle.  A rank that took the other rank's noise rows is 1e-2 away."""
    from electrocardio_panorama_amd import parallel, synth
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    V, B, L, seed = 3, 4, 512, 5
    full = dict(synth.make_batch(B, V, L, seed=seed, Q=2))
    full["noise"] = np.random.default_rng(9000).normal(0, 0.05, (B, L)).astype(np.float32)
    random.seed(seed)
    choice = (random.randint(0, V - 1), random.randint(0, V - 1))
    want = {}
    for r in range(2):
        for nr in (r, 1 - r):        # this shard with its own noise rows, and with the other rank's
            sh = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in parallel.shard_batch(full, r, 2).items()}
            nz = torch.from_numpy(np.ascontiguousarray(parallel.shard_batch(full, nr, 2)["noise"]))
            with torch.no_grad():
                o = orc.forward(hw.hashed_params(V), hw.hashed_buffers(), sh["data"], sh["input_theta"], sh["target_theta"], sh["rois"],
                                phase="train", training=True, p=0.0, lead_choice=choice)
                want[r, nr] = np.array([float(v) for v in orc.loss_v1(o[0] + nz.unsqueeze(1), o[1], o[2],
                                                                      sh["target_view"].unsqueeze(1))])
    for r in range(2):
        assert np.abs(want[r, r] - want[r, 1 - r]).max() > 1e-4          # the check can tell the rows apart
        for name, runs in zip(("eager", "graphed"), dp_noise):
            e = float(np.abs(runs[r]["losses"][0] - want[r, r]).max())
            print(f"rank {r} {name}: first-step losses {runs[r]['losses'][0]} vs oracle {want[r, r]}: max-abs {e:.2e}")
            assert e < 2e-6, (r, name, runs[r]["losses"][0], want[r, r])
