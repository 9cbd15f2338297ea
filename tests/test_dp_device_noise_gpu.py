"""DATA.device_noise at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of tests/test_dp_augment_gpu.py): three
FusedSGD steps with the key on.  The ranks draw different rows for identical targets, end with identical parameters and optimiser state,
and the two-graph step equals the eager one bit for bit."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_device_noise(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_device_noise"))
    run_ranks(os.path.join(TESTS, "dp_device_noise_worker.py"), out)
    z = load_ranks(out)
    return z["eager"], z["graph"]


def test_world2_ranks_draw_different_rows_and_agree_on_the_parameters(dp_device_noise):
    for runs in dp_device_noise:
        assert np.array_equal(runs[0]["target_last"], runs[1]["target_last"])    # the same targets on both ranks ...
        assert not np.array_equal(runs[0]["row_last"], runs[1]["row_last"])      # ... a row each under the per-rank seed
        for z in runs:
            assert np.isfinite(z["row_last"]).all() and np.count_nonzero(z["row_last"]) > z["row_last"].size // 4
        for k in ("p", "buf"):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        assert not np.array_equal(runs[0]["losses"], runs[1]["losses"])
        for z in runs:
            assert z["losses"].shape == (3, 4) and np.isfinite(z["losses"]).all() and int(z["moved"]) > 40
    assert all(int(z["n_rows"]) == 3 for z in dp_device_noise[0])


def test_world2_two_graph_step_equals_eager(dp_device_noise):
    eager, graph = dp_device_noise
    for e, g in zip(eager, graph):
        for k in ("p", "buf", "losses", "row_last"):
            assert np.array_equal(e[k], g[k]), k
