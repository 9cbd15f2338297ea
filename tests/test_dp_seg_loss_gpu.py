"""SOLVER.seg_weights at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_ssim_loss_gpu.py):
one FusedSGD step with the segment weights on.  Both ranks end bit for bit alike, the graphed step equals the eager one, the update is
p0 - lr * mean of the two ranks' recorded gradients in fp64, and each rank's term 3 is the weighted mean of its own shard."""
import os

import numpy as np
import pytest
import torch

import dp_checks
import seg_ref
from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_seg(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_seg"))
    run_ranks(os.path.join(TESTS, "dp_loss_term_worker.py"), out, extra_args=("seg",))
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_seg_ranks_agree_and_graphed_equals_eager(dp_seg):
    dp_checks.ranks_agree_and_graphed_equals_eager(*dp_seg, row_len=4)


def test_world2_seg_update_is_the_mean_of_the_two_gradients(dp_seg):
    """The single-process step on the mean of the two shards' gradients, in fp64: displacement rel-L2 against p0 - lr * mean(g).  Bar
    4.5e-6: what tests/dp_accum_worker.py derives for this comparison at lr = 1 (the fp32 rounding of the stored parameters, 2^-24 * |p|
    at parameter rms 5.8e-2 against a displacement of rms 2.7e-4 there)."""
    dp_checks.update_is_mean_of_gradients(dp_seg[0], "seg_weights", 4.5e-6)


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
