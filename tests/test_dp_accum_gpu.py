"""Gradient accumulation at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_trust_gpu.py):
FusedSGD, accum_steps = 2, three batches -- a window of two and a flushed window of one.  Both ranks agree bit for bit, the graphed
step equals the eager one bit for bit, the first update is p0 - lr * mean of the four recorded gradients in fp64 (the displacement bar of
tests/test_dp_wd_gpu.py and an element-wise rounding bar), and no
collective runs on a micro-batch that does not close a window."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks
from util import rel

pytestmark = pytest.mark.gpu
GRAD_HDR = 4


@pytest.fixture(scope="module")
def dp_accum(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_accum"))
    run_ranks(os.path.join(TESTS, "dp_accum_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_accum_ranks_agree(dp_accum):
    eager, graph = dp_accum
    a, b = eager
    for k in ("p", "buf", "p_first", "p0"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("p", "buf"):
        assert np.array_equal(graph[0][k], graph[1][k]), k
    assert not np.array_equal(a["grads"], b["grads"])              # the ranks saw different shards
    assert not np.array_equal(a["p"], a["p_first"])                # the flushed window updated too


def _first_update(eager):
    a, b = eager
    g = np.stack([a["grads"][0], a["grads"][1], b["grads"][0], b["grads"][1]]).astype(np.float64)
    p0 = a["p0"].astype(np.float64)
    return a["p_first"].astype(np.float64), p0, p0 - float(a["lr"]) * g.mean(0), g


def test_world2_accum_first_update_is_the_mean_of_four_gradients(dp_accum):
    """The first update against p0 - lr * mean(g) of the four recorded gradients in fp64, displacement rel-L2 <= 1e-5 (the bar
    tests/test_dp_wd_gpu.py applies to the displacement).  The reference is fp64 here (there it is torch's fp32 AdamW, whose parameters
    round as ours do), so the parameters' own 2^-24 rounding is part of the distance: the worker's learning rate is chosen so that the
    fp64 result rounded once to fp32 -- printed beside the measured figure -- stays at half the bar (see dp_accum_worker.py)."""
    got, p0, want, _ = _first_update(dp_accum[0])
    e = rel(got - p0, want - p0)
    floor = rel(want.astype(np.float32).astype(np.float64) - p0, want - p0)
    print(f"world 2, accum_steps 2: displacement of the first update vs fp64 {e:.3e} (bar 1e-5); the fp64 result rounded to fp32 sits at "
          f"{floor:.3e}; displacement rms {np.sqrt(np.mean((want - p0) ** 2)):.3e}, parameter rms {np.sqrt(np.mean(p0 ** 2)):.3e}")
    # a mean over the wrong count is far outside: 1 / (world * K) is in the result
    assert rel(got - p0, 2.0 * (want - p0)) > 0.1
    assert e <= 1e-5


def test_world2_accum_first_update_within_fp32_rounding(dp_accum):
    """Element by element, the bar of the single-process K = 3 check with the four addends of world x K: lr * (4 + 1) * 2^-24 *
    sum_k |g_k| / 4 (three fp32 adds -- one on each rank, one in the all-reduce -- and the products with gscale and lr) + 2^-24 * |p|
    (the final subtract)."""
    got, p0, want, g = _first_update(dp_accum[0])
    lr = float(dp_accum[0][0]["lr"])
    tol = lr * 5 * 2.0 ** -24 * np.abs(g).sum(0) / 4 + 2.0 ** -24 * np.abs(want)
    err = np.abs(got - want)
    print(f"world 2, accum_steps 2: first update vs fp64, worst error / bar {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert bool((err <= tol).all())
    assert float(np.abs(got - p0).max()) > 1e-4


def test_world2_accum_no_collective_on_a_non_final_micro_batch(dp_accum):
    eager, graph = dp_accum
    for z in eager:
        n = int(z["n"])
        assert z["reduced"].tolist() == [0, n + GRAD_HDR, 0]       # one all-reduce of g_all, header included, at the window's end
        assert z["flush_reduced"].tolist() == [n + GRAD_HDR]
    for z, e in zip(graph, eager):
        n = int(e["n"])
        # (the two counters Solver._check_h2_range sums over the ranks at the end of the epoch are not a gradient collective)
        calls = [(int(c), int(k)) for c, k in z["calls"] if int(k) > 2]
        assert [k for c, k in calls if c == 1] == []               # the window's first micro-batch: both graphs, no collective
        last = [k for c, k in calls if c == 2]
        assert len(last) == 2 and sum(last) == n + GRAD_HDR        # the suffix bucket, then the encoder bucket with the header
        assert [k for c, k in calls if c == 3] == [n + GRAD_HDR]   # nothing at the replay; the flush reduces the whole buffer once
        assert len(calls) == 3


def test_world2_accum_graphed_equals_eager(dp_accum):
    eager, graph = dp_accum
    for e, g in zip(eager, graph):
        for k in ("p", "buf"):
            assert np.array_equal(e[k], g[k]), k
