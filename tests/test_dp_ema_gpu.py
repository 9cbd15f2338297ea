"""FusedSGD with SOLVER.ema_decay at world_size 2 (two ranks sharing cuda:0 over gloo, the test hooks of tests/test_dp_wd_gpu.py): every
rank computes the same average from the same parameters -- no collective is added --, the graphed step equals the eager one bit for bit,
and the average follows the recurrence over the saved per-step parameters inside the bar of tests/test_ema_gpu.py."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_ema(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_ema"))
    run_ranks(os.path.join(TESTS, "dp_ema_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_ema_ranks_agree(dp_ema):
    eager, graph = dp_ema
    for a, b in (eager, graph):
        for k in ("p", "buf", "ema", "ema_n", "traj"):
            assert np.array_equal(a[k], b[k]), k
        assert float(a["ema_n"][0]) == 2.0 and not np.array_equal(a["ema"], a["p"])


def test_world2_ema_graphed_equals_eager(dp_ema):
    eager, graph = dp_ema
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "ema", "ema_n", "traj"):
            assert np.array_equal(e[k], g[k]), k


def test_world2_ema_follows_the_recurrence(dp_ema):
    from test_ema_gpu import _check_ema
    for z in dp_ema[0]:
        _check_ema(z["ema"], z["p0"], list(z["traj"]), float(z["decay"]), bool(z["warmup"]), "world 2 ")
