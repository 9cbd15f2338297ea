"""The per-site fp32 route of split-fp16 weight gradients (ops.H2_TAIL_MODE = "fp32") with world_size 2 (two ranks sharing cuda:0
over gloo, the test hooks of tests/test_dp_gpu.py): routes are per rank and no collective decides them -- rank 0 routes every
weight-gradient site, rank 1 none -- and the parameters stay identical on both ranks after two steps, eager and graphed (the
gradients are all-reduced whichever kernel produced them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dp_tail(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_h2_tail"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = os.path.join(ROOT, "tests", "dp_h2_tail_worker.py")
    procs = [subprocess.Popen([sys.executable, script, out], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        logs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(lg[-3000:] for lg in logs)
    return {mode: [dict(np.load(os.path.join(out, f"{mode}_rank{r}.npz"))) for r in range(2)] for mode in ("eager", "graph")}


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_routes_are_per_rank(dp_tail, mode):
    r0, r1 = dp_tail[mode]
    assert int(r0["n_bww"]) > 10 and int(r0["moved"]) == int(r0["routed"]) == int(r0["n_bww"]), r0
    assert int(r1["moved"]) == 0 and int(r1["routed"]) == 0 and int(r1["n_bww"]) == int(r0["n_bww"]), r1


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_world2_parameters_identical_on_both_ranks(dp_tail, mode):
    r0, r1 = dp_tail[mode]
    assert np.array_equal(r0["p"], r1["p"])
