"""FusedAdam with world_size 2 (two ranks sharing cuda:0 over gloo, the test hooks of tests/test_dp_gpu.py): the early gradient
bucket is consumed, both ranks hold the same parameters, the update is torch.optim.Adam on the mean of the ranks' gradients, and the
graphed step equals the eager one bit for bit."""
import os

import numpy as np
import pytest
import torch

import dp_checks
from dp_launch import TESTS, load_ranks, run_ranks
from util import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_adam(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_adam"))
    run_ranks(os.path.join(TESTS, "dp_adam_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


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
    dp_checks.consumes_the_early_bucket(dp_adam[0])


def test_world2_adam_graphed_equals_eager(dp_adam):
    eager, graph = dp_adam
    for e, g in zip(eager, graph):
        for k in ("p", "m", "v", "step"):
            assert np.array_equal(e[k], g[k]), k
