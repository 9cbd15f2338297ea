"""SOLVER.corr_factor at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_ssim_loss_gpu.py):
one FusedSGD step with the correlation term on.  Both ranks end bit for bit alike, the graphed step equals the eager one, the update is
p0 - lr * mean of the two ranks' recorded gradients in fp64, and each rank's term is the per-shard mean of the fp64 restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import corr_ref
from util import free_port, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 5.0


@pytest.fixture(scope="module")
def dp_corr(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_corr"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "dp_corr_loss_worker.py")
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


def test_world2_corr_ranks_agree_and_graphed_equals_eager(dp_corr):
    eager, graph = dp_corr
    for k in ("p", "buf", "p0"):
        assert np.array_equal(eager[0][k], eager[1][k]), k
    for k in ("p", "buf"):
        assert np.array_equal(graph[0][k], graph[1][k]), k
    assert not np.array_equal(eager[0]["grad"], eager[1]["grad"])       # the ranks saw different shards
    for e, g in zip(eager, graph):
        for k in ("p", "buf"):
            assert np.array_equal(e[k], g[k]), k
        assert g["losses"].shape == (1, 5) and np.array_equal(g["losses"][0], e["losses"])


def test_world2_corr_update_is_the_mean_of_the_two_gradients(dp_corr):
    """The single-process step on the mean of the two shards' gradients, in fp64: displacement rel-L2 against p0 - lr * mean(g).  Bar
    4.5e-6: what tests/dp_accum_worker.py derives for this comparison at lr = 1 (the fp32 rounding of the stored parameters, 2^-24 * |p|
    at parameter rms 5.8e-2 against a displacement of rms 2.7e-4 there; the term's gradient only makes the displacement larger)."""
    a, b = dp_corr[0]
    p0 = a["p0"].astype(np.float64)
    want = p0 - float(a["lr"]) * np.stack([a["grad"], b["grad"]]).astype(np.float64).mean(0)
    got = a["p"].astype(np.float64)
    e = rel(got - p0, want - p0)
    floor = rel(want.astype(np.float32).astype(np.float64) - p0, want - p0)
    print(f"world 2, corr_factor 5: displacement of the update vs fp64 {e:.3e} (bar 4.5e-6); the fp64 result rounded to fp32 sits at "
          f"{floor:.3e}; displacement rms {np.sqrt(np.mean((want - p0) ** 2)):.3e}")
    assert rel(got - p0, 2.0 * (want - p0)) > 0.1              # a sum instead of the mean is far outside
    assert e <= 4.5e-6


def test_world2_corr_term_is_the_per_shard_mean(dp_corr):
    """Each rank's losses[4] against the fp64 restatement on that rank's own prediction, target and rois (one fp32 rounding, 2x
    headroom), and the total is the fp32 sum behind the three terms."""
    terms = []
    for z in dp_corr[0]:
        pred, tgt = torch.from_numpy(z["pred"]), torch.from_numpy(z["target"]).unsqueeze(1)
        B, _, L = pred.shape
        ends = corr_ref.row_ends(torch.from_numpy(z["rois"]), B, L)
        assert all(2 <= e < L for e in ends)                   # cropping matters on these rows
        ref = float(corr_ref.corr_term(pred, tgt, FACTOR, corr_ref.EPS, ends))
        got = float(z["losses"][4])
        assert abs(got - ref) <= 2.0 ** -22 * abs(ref) + 1e-12, (got, ref)
        assert abs(float(corr_ref.corr_term(pred, tgt, FACTOR, corr_ref.EPS)) - ref) > 1e-3
        r = z["losses"].astype(np.float32)
        assert r[0] == np.float32(np.float32(r[1] + r[2]) + r[3]) + r[4] and r[4] > 0.01
        terms.append(got)
    assert terms[0] != terms[1]
