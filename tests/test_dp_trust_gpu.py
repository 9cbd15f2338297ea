"""FusedLAMB at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_wd_gpu.py): the early
gradient bucket is consumed, both ranks hold the same parameters, state and ratio table, the update is the fp64 oracle of
tests/test_trust_gpu.py on the mean of the ranks' gradients (that module's bars), and the graphed step equals the eager one bit for bit."""
import os

import numpy as np
import pytest
import torch

import dp_checks
from dp_launch import TESTS, load_ranks, run_ranks
from util import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_trust(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_trust"))
    run_ranks(os.path.join(TESTS, "dp_trust_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_trust_ranks_agree_and_match_the_oracle_on_the_mean_gradient(dp_trust):
    from electrocardio_panorama_amd.solver.optim_scheduler import trust_segments
    from test_trust_gpu import _check, _restate
    eager, _ = dp_trust
    a, b = eager
    for k in ("p", "m", "v", "step", "seg_end", "seg_wd_mul", "seg_adapt", "ratio", "trust_stats"):
        assert np.array_equal(a[k], b[k]), k
    assert float(a["step"][0]) == 2.0 and a["trust_stats"].tolist()[2:] == [2.0, 0.0]
    # the table the optimiser built is the one of the live tensors' names: one segment each, some exempt
    pats = [str(k) for k in a["no_decay"]]
    ends, wd_muls, adapts = trust_segments([str(k) for k in a["live"]], [int(k) for k in a["sizes"]], pats, pats)
    assert a["seg_end"].tolist() == ends and a["seg_wd_mul"].tolist() == wd_muls and a["seg_adapt"].tolist() == adapts
    assert len(ends) == len(a["live"]) and 0.0 in adapts and 1.0 in adapts
    p0 = torch.from_numpy(a["p0"].copy())
    grads = [torch.from_numpy((a["grads"][s] + b["grads"][s]) / 2).float() for s in range(a["grads"].shape[0])]
    hyper = dict(gscale=1.0, lr=1e-3, wd=float(a["wd"]))
    want, q_want = _restate("lamb", p0, grads, ends, wd_muls, adapts, torch.float64, **hyper)
    f32, _ = _restate("lamb", p0, grads, ends, wd_muls, adapts, torch.float32, **hyper)
    bar = rel(f32[0].double() - p0.double(), want[0] - p0.double())
    got = [torch.from_numpy(a[k].copy()) for k in ("p", "m", "v")]
    _check(got, a["ratio"].astype(np.float64).tolist(), want, q_want, bar, p0, "world 2 lamb")
    assert all(q == 1.0 for q, ad in zip(a["ratio"].tolist(), adapts) if not ad)


def test_world2_trust_consumes_the_early_bucket(dp_trust):
    dp_checks.consumes_the_early_bucket(dp_trust[0])


def test_world2_trust_graphed_equals_eager(dp_trust):
    eager, graph = dp_trust
    for e, g in zip(eager, graph):
        for k in ("p", "m", "v", "step", "ratio", "trust_stats"):
            assert np.array_equal(e[k], g[k]), k
