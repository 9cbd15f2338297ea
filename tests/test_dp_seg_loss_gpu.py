"""SOLVER.seg_weights at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_ssim_loss_gpu.py):
one FusedSGD step with the segment weights on.  Both ranks end bit for bit alike, the graphed step equals the eager one, the update is
p0 - lr * mean of the two ranks' recorded gradients in fp64, and each rank's term 3 is the weighted mean of its own shard."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seg_ref
from util import free_port, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dp_seg(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_seg"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "dp_seg_loss_worker.py")
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


def test_world2_seg_ranks_agree_and_graphed_equals_eager(dp_seg):
    eager, graph = dp_seg
    for k in ("p", "buf", "p0"):
        assert np.array_equal(eager[0][k], eager[1][k]), k
    for k in ("p", "buf"):
        assert np.array_equal(graph[0][k], graph[1][k]), k
    assert not np.array_equal(eager[0]["grad"], eager[1]["grad"])       # the ranks saw different shards
    for e, g in zip(eager, graph):
        for k in ("p", "buf"):
            assert np.array_equal(e[k], g[k]), k
        assert g["losses"].shape == (1, 4) and np.array_equal(g["losses"][0], e["losses"])


def test_world2_seg_update_is_the_mean_of_the_two_gradients(dp_seg):
    """The single-process step on the mean of the two shards' gradients, in fp64: displacement rel-L2 against p0 - lr * mean(g).  Bar
    4.5e-6: what tests/dp_accum_worker.py derives for this comparison at lr = 1 (the fp32 rounding of the stored parameters, 2^-24 * |p|
    at parameter rms 5.8e-2 against a displacement of rms 2.7e-4 there)."""
    a, b = dp_seg[0]
    p0 = a["p0"].astype(np.float64)
    want = p0 - float(a["lr"]) * np.stack([a["grad"], b["grad"]]).astype(np.float64).mean(0)
    got = a["p"].astype(np.float64)
    e = rel(got - p0, want - p0)
    floor = rel(want.astype(np.float32).astype(np.float64) - p0, want - p0)
    print(f"world 2, seg_weights: displacement of the update vs fp64 {e:.3e} (bar 4.5e-6); the fp64 result rounded to fp32 sits at "
          f"{floor:.3e}; displacement rms {np.sqrt(np.mean((want - p0) ** 2)):.3e}")
    assert rel(got - p0, 2.0 * (want - p0)) > 0.1              # a sum instead of the mean is far outside
    assert e <= 4.5e-6


def test_world2_seg_term_is_the_per_shard_weighted_mean(dp_seg):
    """Each rank's losses[3] against the fp64 restatement on that rank's own prediction, target and rois: two fp32 roundings with 2x
    headroom (2^-22 relative); the total is the fp32 sum of the three terms in loss_final's association."""
    terms = []
    for z in dp_seg[0]:
        pred, tgt, rois = torch.from_numpy(z["pred"]), torch.from_numpy(z["target"]).unsqueeze(1), z["rois"]
        ref = float(seg_ref.seg_term(pred, tgt, rois, z["weights"], 1.0, False))
        flat = float(seg_ref.seg_term(pred, tgt, rois, [1.0] * 7, 1.0, False))
        got = z["losses"]
        assert abs(float(got[3]) - ref) <= 2.0 ** -22 * abs(ref), (float(got[3]), ref)
        assert abs(ref - flat) > 1e-2 * flat                    # the weights matter on these rows
        assert got[0] == np.float32(np.float32(got[1] + got[2]) + got[3])
        terms.append(float(got[3]))
    assert terms[0] != terms[1]
