"""MODEL.lead_mask at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_augment_gpu.py): two
FusedSGD steps with aug_lead_drop 0.4.  The ranks mask identical clean shards differently (the seeds carry the rank), end with identical
parameters, and the two-graph step equals the eager one bit for bit."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_lead_mask(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_lead_mask"))
    run_ranks(os.path.join(TESTS, "dp_lead_mask_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_ranks_mask_differently_and_agree_on_the_parameters(dp_lead_mask):
    for runs in dp_lead_mask:
        assert runs[0]["mask_last"].shape == runs[1]["mask_last"].shape == (4, 3) and runs[0]["mask_last"].dtype == np.uint8
        assert not np.array_equal(runs[0]["mask_last"], runs[1]["mask_last"])        # the per-rank seed
        for z in runs:
            assert z["mask_last"].any(axis=1).all() and not z["mask_last"].all()     # every sample keeps a lead; some lead is gone
        for k in ("p", "buf"):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        for z in runs:
            assert z["losses"].shape == (2, 4) and np.isfinite(z["losses"]).all()
    assert all(int(z["n_masks"]) == 2 for z in dp_lead_mask[0])


def test_world2_two_graph_masked_step_equals_eager(dp_lead_mask):
    eager, graph = dp_lead_mask
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "losses", "mask_last"):
            assert np.array_equal(e[k], g[k]), k
