"""SOLVER.ssim_factor at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_accum_gpu.py): one
FusedSGD step with the SSIM term on.  Both ranks end bit for bit alike, the graphed step equals the eager one, the update is
p0 - lr * mean of the two ranks' recorded gradients in fp64, and each rank's term is the per-shard mean of the fp64 restatement."""
import os

import pytest
import torch

import dp_checks
import ssim_ref
from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_ssim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_ssim"))
    run_ranks(os.path.join(TESTS, "dp_loss_term_worker.py"), out, extra_args=("ssim",))
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_ssim_ranks_agree_and_graphed_equals_eager(dp_ssim):
    dp_checks.ranks_agree_and_graphed_equals_eager(*dp_ssim, row_len=5)


def test_world2_ssim_update_is_the_mean_of_the_two_gradients(dp_ssim):
    """The single-process step on the mean of the two shards' gradients, in fp64: displacement rel-L2 against p0 - lr * mean(g).  Bar
    4.5e-6: what tests/dp_accum_worker.py derives for this comparison at lr = 1 (the fp32 rounding of the stored parameters, 2^-24 * |p|
    at parameter rms 5.8e-2 against a displacement of rms 2.7e-4 there; the term's gradient only makes the displacement larger)."""
    dp_checks.update_is_mean_of_gradients(dp_ssim[0], "ssim_factor 0.5", 4.5e-6)


def test_world2_ssim_term_is_the_per_shard_mean(dp_ssim):
    """Each rank's losses[4] against the fp64 restatement on that rank's own prediction, target and rois (one fp32 rounding, 2x
    headroom), and the total is the fp32 sum behind the three terms."""
    terms = []
    for z in dp_ssim[0]:
        pred, tgt = torch.from_numpy(z["pred"]), torch.from_numpy(z["target"]).unsqueeze(1)
        B, _, L = pred.shape
        ends = ssim_ref.row_ends(torch.from_numpy(z["rois"]), B, L)
        assert all(7 <= e < L for e in ends)                   # cropping matters on these rows
        ref = float(ssim_ref.ssim_term(pred, tgt, 0.5, ends))
        got = float(z["losses"][4])
        assert abs(got - ref) <= 2.0 ** -23 * abs(ref) + 1e-12, (got, ref)
        assert abs(float(ssim_ref.ssim_term(pred, tgt, 0.5)) - ref) > 1e-3
        assert z["losses"][0] > z["losses"][4] > 0.1
        terms.append(got)
    assert terms[0] != terms[1]
