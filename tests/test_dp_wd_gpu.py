"""FusedAdamW with weight decay and exempt tensors at world_size 2 (two ranks sharing cuda:0 over gloo, the test hooks of
tests/test_dp_adam_gpu.py): the early gradient bucket is consumed, both ranks hold the same parameters and state, the update is
torch.optim.AdamW -- the exempt tensors in a group without decay -- on the mean of the ranks' gradients, and the graphed step equals
the eager one bit for bit."""
import os

import numpy as np
import pytest
import torch

import dp_checks
from dp_launch import TESTS, load_ranks, run_ranks
from util import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_wd(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_wd"))
    run_ranks(os.path.join(TESTS, "dp_wd_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_wd_ranks_agree_and_match_torch_adamw_on_mean_gradient(dp_wd):
    from electrocardio_panorama_amd.solver.optim_scheduler import decay_runs
    eager, _ = dp_wd
    a, b = eager
    for k in ("p", "m", "v", "step", "run_end", "run_mul"):
        assert np.array_equal(a[k], b[k]), k
    assert float(a["step"][0]) == 2.0
    # the table the optimiser built is the one of the live tensors' names; more than one run, some exempt
    ends, muls = decay_runs([str(k) for k in a["live"]], [int(k) for k in a["sizes"]], [str(k) for k in a["no_decay"]])
    assert a["run_end"].tolist() == ends and a["run_mul"].tolist() == muls and 0.0 in muls and 1.0 in muls
    wd, p0 = float(a["wd"]), torch.from_numpy(a["p0"].copy())
    begs = [0] + ends[:-1]
    segs = [torch.nn.Parameter(p0[s:e].clone()) for s, e in zip(begs, ends)]
    ref = torch.optim.AdamW([dict(params=[s], weight_decay=wd * m) for s, m in zip(segs, muls)], lr=1e-3, foreach=False)
    for s in range(a["grads"].shape[0]):
        g = torch.from_numpy((a["grads"][s] + b["grads"][s]) / 2).float()
        for seg, s0, e in zip(segs, begs, ends):
            seg.grad = g[s0:e].clone()
        ref.step()
    p = torch.cat([s.detach() for s in segs]).numpy()
    m, v = (torch.cat([ref.state[s][k] for s in segs]) for k in ("exp_avg", "exp_avg_sq"))
    e_p, e_m, e_v = rel(a["p"] - a["p0"], p - a["p0"]), rel(a["m"], m), rel(a["v"], v)
    print(f"world 2 adamw: displacement {e_p:.3e}, m {e_m:.3e}, v {e_v:.3e}")
    assert e_p <= 1e-5 and e_m <= 1e-5 and e_v <= 1e-5
    # the decay is in the result: torch without it ends more than the bar away
    free = torch.nn.Parameter(p0.clone())
    ref0 = torch.optim.AdamW([free], lr=1e-3, weight_decay=0.0, foreach=False)
    for s in range(a["grads"].shape[0]):
        free.grad = torch.from_numpy((a["grads"][s] + b["grads"][s]) / 2).float()
        ref0.step()
    assert rel(a["p"] - a["p0"], free.detach().numpy() - a["p0"]) > 1e-4


def test_world2_wd_consumes_the_early_bucket(dp_wd):
    dp_checks.consumes_the_early_bucket(dp_wd[0])


def test_world2_wd_graphed_equals_eager(dp_wd):
    eager, graph = dp_wd
    for e, g in zip(eager, graph):
        for k in ("p", "m", "v", "step"):
            assert np.array_equal(e[k], g[k]), k
