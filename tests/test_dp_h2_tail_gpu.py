"""The per-site fp32 route of split-fp16 weight gradients (ops.H2_TAIL_MODE = "fp32") with world_size 2 (two ranks sharing cuda:0
over gloo, the test hooks of tests/test_dp_gpu.py): routes are per rank and no collective decides them -- rank 0 routes every
weight-gradient site, rank 1 none -- and the parameters stay identical on both ranks after two steps, eager and graphed (the
gradients are all-reduced whichever kernel produced them)."""
import os

import numpy as np
import pytest

from dp_launch import TESTS, load_ranks, run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dp_tail(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_h2_tail"))
    run_ranks(os.path.join(TESTS, "dp_h2_tail_worker.py"), out)
    return load_ranks(out)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_routes_are_per_rank(dp_tail, mode):
    r0, r1 = dp_tail[mode]
    assert int(r0["n_bww"]) > 10 and int(r0["moved"]) == int(r0["routed"]) == int(r0["n_bww"]), r0
    assert int(r1["moved"]) == 0 and int(r1["routed"]) == 0 and int(r1["n_bww"]) == int(r0["n_bww"]), r1


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_parameters_identical_on_both_ranks(dp_tail, mode):
    r0, r1 = dp_tail[mode]
    assert np.array_equal(r0["p"], r1["p"])
