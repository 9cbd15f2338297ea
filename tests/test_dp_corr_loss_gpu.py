"""SOLVER.corr_factor at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_ssim_loss_gpu.py):
one FusedSGD step with the correlation term on.  Both ranks end bit for bit alike, the graphed step equals the eager one, the update is
p0 - lr * mean of the two ranks' recorded gradients in fp64, and each rank's term is the per-shard mean of the fp64 restatement."""
import os

import numpy as np
import pytest
import torch

import corr_ref
import dp_checks
from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu
FACTOR = 5.0


@pytest.fixture(scope="module")
def dp_corr(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_corr"))
    run_ranks(os.path.join(TESTS, "dp_loss_term_worker.py"), out, extra_args=("corr",))
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_corr_ranks_agree_and_graphed_equals_eager(dp_corr):
    dp_checks.ranks_agree_and_graphed_equals_eager(*dp_corr, row_len=5)


def test_world2_corr_update_is_the_mean_of_the_two_gradients(dp_corr):
    """The single-process step on the mean of the two shards' gradients, in fp64: displacement rel-L2 against p0 - lr * mean(g).  Bar
    4.5e-6: what tests/dp_accum_worker.py derives for this comparison at lr = 1 (the fp32 rounding of the stored parameters, 2^-24 * |p|
    at parameter rms 5.8e-2 against a displacement of rms 2.7e-4 there; the term's gradient only makes the displacement larger)."""
    dp_checks.update_is_mean_of_gradients(dp_corr[0], "corr_factor 5", 4.5e-6)


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
