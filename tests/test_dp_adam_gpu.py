"""FusedAdam with world_size 2 (two ranks sharing cuda:0 over gloo, the test hooks of tests/test_dp_gpu.py): the early gradient
bucket is consumed, both ranks hold the same parameters, the update is torch.optim.Adam on the mean of the ranks' gradients, and the
graphed step equals the eager one bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import free_port, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dp_adam(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_adam"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "dp_adam_worker.py")
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


def test_world2_adam_ranks_agree_and_match_torch_adam_on_mean_gradient(dp_adam):
    eager, _ = dp_adam
    a, b = eager
    for k in ("p", "m", "v", "step"):
        assert np.array_equal(a[k], b[k]), k
    assert float(a["step"][0]) == 2.0
    p = torch.nn.Parameter(torch.from_numpy(a["p0"].copy()))
    ref = torch.optim.Adam([p], lr=1e-3, foreach=False)
    for s in range(a["grads"].shape[0]):
        p.grad = torch.from_numpy((a["grads"][s] + b["grads"][s]) / 2).float()
        ref.step()
    st = ref.state[p]
    assert rel(a["p"] - a["p0"], p.detach().numpy() - a["p0"]) <= 1e-5
    assert rel(a["m"], st["exp_avg"]) <= 1e-5 and rel(a["v"], st["exp_avg_sq"]) <= 1e-5


def test_world2_adam_consumes_the_early_bucket(dp_adam):
    eager, _ = dp_adam
    for z in eager:
        assert (z["early"] > 0).all()                      # engine.backward started the bucket every step ...
        assert (z["reduced"] > 0).all() and (z["reduced"] < int(z["n"])).all()     # ... and the step reduced only the rest


def test_world2_adam_graphed_equals_eager(dp_adam):
    eager, graph = dp_adam
    for e, g in zip(eager, graph):
        for k in ("p", "m", "v", "step"):
            assert np.array_equal(e[k], g[k]), k
