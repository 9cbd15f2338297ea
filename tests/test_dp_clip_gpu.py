"""Gradient-norm clipping with world_size 2 (two ranks sharing cuda:0 over gloo, the harness of tests/test_dp_adam_gpu.py): the norm
clipped is that of the MEAN gradient, the same on both ranks; the early gradient bucket is still consumed; the graphed step equals the
eager one bit for bit."""
import os

import numpy as np
import pytest
import torch

import dp_checks
from dp_launch import TESTS, load_ranks, run_ranks
from util import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_clip(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_clip"))
    run_ranks(os.path.join(TESTS, "dp_clip_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_clip_ranks_agree_and_match_torch_clip_on_mean_gradient(dp_clip):
    """The torch replay runs on the device: on the CPU torch sums the squares of the one flat 7 M-element gradient in fp32 chunks and
    its norm is 1e-4 low, ten times the bar (measured: 0.8282758 against 0.8284231 on the device and in fp64)."""
    eager, _ = dp_clip
    a, b = eager
    for k in ("p", "buf", "clips"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["clips"][:, 1] < 1.0).all(), a["clips"]                  # every step clipped
    dev = torch.device("cuda", 0)
    p0 = torch.from_numpy(a["p0"].copy()).to(dev)
    p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.SGD([p], lr=0.1, momentum=0.9)
    for s in range(a["grads"].shape[0]):
        mean = (a["grads"][s].astype(np.float64) + b["grads"][s].astype(np.float64)) / 2
        p.grad = torch.from_numpy(mean).float().to(dev)
        total = float(torch.nn.utils.clip_grad_norm_([p], 0.25))
        exact = float(np.sqrt((mean * mean).sum()))
        print(f"step {s}: norm {a['clips'][s, 0]!r}, torch {total!r}, fp64 {exact!r}, coef {a['clips'][s, 1]!r}")
        assert abs(float(a["clips"][s, 0]) - exact) <= 1e-6 * exact, (s, a["clips"][s], exact)
        ref.step()
    pa = torch.from_numpy(a["p"]).to(dev)
    assert rel(pa - p0, p.detach() - p0) <= 1e-5, rel(pa - p0, p.detach() - p0)
    assert rel(a["buf"], ref.state[p]["momentum_buffer"]) <= 1e-5


def test_world2_clip_still_consumes_the_early_bucket(dp_clip):
    dp_checks.consumes_the_early_bucket(dp_clip[0])


def test_world2_clip_graphed_equals_eager(dp_clip):
    eager, graph = dp_clip
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "clips"):
            assert np.array_equal(e[k], g[k]), k
