"""FusedSGD with SOLVER.ema_decay at world_size 2 (two ranks sharing cuda:0 over gloo, the test hooks of tests/test_dp_wd_gpu.py): every
rank computes the same average from the same parameters -- no collective is added --, the graphed step equals the eager one bit for bit,
and the average follows the recurrence over the saved per-step parameters inside the bar of tests/test_ema_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dp_ema(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_ema"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "dp_ema_worker.py")
    procs = [subprocess.Popen([sys.executable, script, out], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        logs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(lg[-3000:] for lg in logs)
    return [dict(np.load(os.path.join(out, f"eager_rank{r}.npz"))) for r in range(2)], \
        [dict(np.load(os.path.join(out, f"graph_rank{r}.npz"))) for r in range(2)]


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
