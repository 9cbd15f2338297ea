"""DATA.device_resident at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_views_gpu.py):
the ranks' batches of an epoch are disjoint in recording index and together cover the epoch's permutation, every field equals the
restatement of tests/resident_ref.py, and the next epoch is another order."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu
FIELDS = ("data", "target_view", "rest_view", "rois", "input_theta", "target_theta", "rest_theta")


@pytest.fixture(scope="module")
def dp_resident(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_resident"))
    run_ranks(os.path.join(TESTS, "dp_resident_worker.py"), out)
    return load_ranks(out, modes=("resident",))["resident"]


def test_world2_ranks_draw_disjoint_shards_that_cover_the_permutation(dp_resident):
    for epoch in (0, 1):
        a, b = (z[f"idx{epoch}"] for z in dp_resident)
        assert a.shape == b.shape == (3, 2)                                  # 12 entries: 6 per rank, three batches of 2 (global batch 4)
        assert not set(a.ravel()) & set(b.ravel()) and sorted(a.ravel().tolist() + b.ravel().tolist()) == list(range(12))
        oa, ob = (z[f"order{epoch}"] for z in dp_resident)
        assert a.ravel().tolist() == oa.tolist() and b.ravel().tolist() == ob.tolist()
        # rank r took every second element of one permutation, from r
        perm = np.stack([oa, ob], axis=1).ravel()
        assert sorted(perm.tolist()) == list(range(12)) and perm[0::2].tolist() == oa.tolist() and perm[1::2].tolist() == ob.tolist()


def test_world2_every_field_equals_the_restatement(dp_resident):
    for z in dp_resident:
        for epoch in (0, 1):
            for k in FIELDS:
                got, want = z[f"got{epoch}_{k}"], z[f"want{epoch}_{k}"]
                assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (epoch, k)
            assert z[f"got{epoch}_data"].shape == (3, 2, 3, 512) and np.isfinite(z[f"got{epoch}_data"]).all()


def test_world2_a_second_epoch_differs(dp_resident):
    for z in dp_resident:
        assert z["idx0"].tolist() != z["idx1"].tolist()
        assert z["got0_data"].tobytes() != z["got1_data"].tobytes()
    assert dp_resident[0]["got0_data"].tobytes() != dp_resident[1]["got0_data"].tobytes()
