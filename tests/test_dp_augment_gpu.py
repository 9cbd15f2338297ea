"""DATA.aug_* at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_views_gpu.py): three
FusedSGD steps with all four corruptions on.  The ranks corrupt identical clean shards differently, end with identical parameters, and
the two-graph step equals the eager one bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dp_augment(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_augment"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "dp_augment_worker.py")
    procs = [subprocess.Popen([sys.executable, script, out], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        logs = [p.communicate(timeout=600)[0] for p in procs]      # every child has its own time limit
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(lg[-3000:] for lg in logs)
    return [dict(np.load(os.path.join(out, f"eager_rank{r}.npz"))) for r in range(2)], \
        [dict(np.load(os.path.join(out, f"graph_rank{r}.npz"))) for r in range(2)]


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
