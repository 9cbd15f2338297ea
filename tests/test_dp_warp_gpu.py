"""DATA.aug_warp / aug_roi_jitter at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of
tests/test_dp_augment_gpu.py): three FusedSGD steps with the warp on.  The ranks warp identical shards differently, end with identical
parameters, and the graphed step equals the eager one bit for bit."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_warp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_warp"))
    run_ranks(os.path.join(TESTS, "dp_warp_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_warp_ranks_warp_differently_and_agree_on_the_parameters(dp_warp):
    for runs in dp_warp:
        assert np.array_equal(runs[0]["clean_last"], runs[1]["clean_last"])      # the same samples on both ranks ...
        assert not np.array_equal(runs[0]["fed_last"], runs[1]["fed_last"])      # ... warped under the per-rank seed
        assert not np.array_equal(runs[0]["rois_last"], runs[1]["rois_last"])
        for z in runs:
            assert not np.array_equal(z["fed_last"], z["clean_last"]) and int(z["n_fed"]) == 3
        for k in ("p", "buf"):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        assert not np.array_equal(runs[0]["losses"], runs[1]["losses"])
        for z in runs:
            assert z["losses"].shape == (3, 4) and np.isfinite(z["losses"]).all() and int(z["moved"]) > 40


def test_world2_warp_graphed_step_equals_eager(dp_warp):
    eager, graph = dp_warp
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "losses", "fed_last", "rois_last"):
            assert np.array_equal(e[k], g[k]), k
