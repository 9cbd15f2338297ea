"""The per-update learning-rate schedule at world_size 2 (two ranks sharing cuda:0 over gloo, the worker / fixture scheme of
tests/test_dp_accum_gpu.py): four updates, eagerly and through the two-graph data-parallel step -- both ranks hold bit-identical t, rate
and parameters, the graphed run equals the eager one, and a taint raised on rank 1 only skips the update on both ranks and advances the
schedule on neither."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu
POINTS = ("four", "tainted", "clean")
KEYS = ("p", "buf", "t", "lr")


@pytest.fixture(scope="module")
def dp_sched(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_sched"))
    run_ranks(os.path.join(TESTS, "dp_sched_worker.py"), out)
    return load_ranks(out)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_ranks_hold_the_same_count_rate_and_parameters(dp_sched, mode):
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    a, b = dp_sched[mode]
    for pt in POINTS:
        for k in KEYS:
            assert np.array_equal(a[f"{k}_{pt}"], b[f"{k}_{pt}"]), (pt, k)
    assert int(a["t_four"]) == 4 and int(a["t_clean"]) == 5
    for pt, t in (("four", 4), ("clean", 5)):
        want = float(np.float32(float(a["base"]) * lr_factor(t, 2, 0.01, "cosine", 6, lr_floor=0.1)))
        assert abs(float(a[f"lr_{pt}"]) - want) <= 2.0 ** -23 * want, (pt, float(a[f"lr_{pt}"]), want)
    assert a["lr_four"] != a["lr_clean"] and not np.array_equal(a["p_four"], a["p_clean"])


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_taint_on_one_rank_skips_and_advances_neither(dp_sched, mode):
    for z in dp_sched[mode]:
        for k in KEYS:
            assert np.array_equal(z[f"{k}_tainted"], z[f"{k}_four"]), k
        assert int(z["t_tainted"]) == 4


def test_world2_graphed_equals_eager(dp_sched):
    for e, g in zip(dp_sched["eager"], dp_sched["graph"]):
        for pt in POINTS:
            for k in KEYS:
                assert np.array_equal(e[f"{k}_{pt}"], g[f"{k}_{pt}"]), (pt, k)
