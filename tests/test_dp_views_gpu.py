"""SOLVER.train_views at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_ssim_loss_gpu.py):
two FusedSGD steps at train_views 2.  Both ranks end bit for bit alike, and the two-graph step equals the eager one bit for bit."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_views(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_views"))
    run_ranks(os.path.join(TESTS, "dp_views_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_views_ranks_agree(dp_views):
    for runs in dp_views:
        for k in ("p", "buf"):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        assert not np.array_equal(runs[0]["losses"], runs[1]["losses"])       # the ranks saw different shards
        for z in runs:
            assert z["losses"].shape == (2, 4) and np.isfinite(z["losses"]).all()
            assert int(z["nbt"]) == 2 * 2 * 3 and int(z["moved"]) > 40       # two steps x two views x three passes


def test_world2_views_two_graph_step_equals_eager(dp_views):
    eager, graph = dp_views
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "losses"):
            assert np.array_equal(e[k], g[k]), k
