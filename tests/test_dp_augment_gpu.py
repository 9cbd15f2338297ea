"""DATA.aug_* at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_views_gpu.py): three
FusedSGD steps with all four corruptions on.  The ranks corrupt identical clean shards differently, end with identical parameters, and
the two-graph step equals the eager one bit for bit."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_augment(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_augment"))
    run_ranks(os.path.join(TESTS, "dp_augment_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_augment_ranks_corrupt_differently_and_agree_on_the_parameters(dp_augment):
    for runs in dp_augment:
        assert np.array_equal(runs[0]["clean_last"], runs[1]["clean_last"])      # the same clean samples on both ranks ...
        assert not np.array_equal(runs[0]["fed_last"], runs[1]["fed_last"])      # ... corrupted under the per-rank seed
        for z in runs:
            assert not np.array_equal(z["fed_last"], z["clean_last"])
        for k in ("p", "buf"):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        assert not np.array_equal(runs[0]["losses"], runs[1]["losses"])
        for z in runs:
            assert z["losses"].shape == (3, 4) and np.isfinite(z["losses"]).all() and int(z["moved"]) > 40
    assert all(int(z["n_fed"]) == 3 for z in dp_augment[0])


def test_world2_augment_two_graph_step_equals_eager(dp_augment):
    eager, graph = dp_augment
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "losses", "fed_last"):
            assert np.array_equal(e[k], g[k]), k
