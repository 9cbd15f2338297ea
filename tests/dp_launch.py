"""The one place that starts the rank processes of a multi-rank test: the rendezvous environment, the launch, the time limit, the
clean-up and the loading of what the ranks saved.  A two-rank test's fixture is

    out = str(tmp_path_factory.mktemp("dp_x"))
    run_ranks(os.path.join(TESTS, "dp_x_worker.py"), out)
    return load_ranks(out)

The group stops as a whole: at one deadline, or a grace period after the first rank fails (the survivor would otherwise wait inside
the collective, holding the GPU, until the deadline).  No path leaves a child behind, and nothing is ever started a second time."""
import os
import subprocess
import sys
import time

import numpy as np

from util import free_port

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def world2_env(share_gpu=True):
    """The environment of one of two ranks, RANK / LOCAL_RANK apart.  share_gpu: both ranks on cuda:0, gradients over gloo (the test
    hooks NEF_SHARE_GPU / NEF_DIST_BACKEND of parallel.init_from_env, honoured only under NEF_TEST_HOOKS=1); without it one rank per
    device over the production transport."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE="2", NEF_DIST_BACKEND="gloo",
               NEF_SHARE_GPU="1", NEF_TEST_HOOKS="1", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if not share_gpu:
        del env["NEF_DIST_BACKEND"], env["NEF_SHARE_GPU"]
    return env


def run_ranks(script_or_argv, out, *, world=2, timeout=600, env=None, extra_args=(), peer_grace=10.0):
    """Run `python <script_or_argv> <out> <extra_args...>` once per rank and return the ranks' logs (stdout and stderr, also kept as
    out/rank{r}.log) when every rank exits 0.  Otherwise AssertionError with every rank's return code and the end of every log:
    `timeout` seconds after the start every rank still running is killed ("time limit"); once a rank has failed the others get
    `peer_grace` seconds to end on their own -- their traceback reaches the log -- and are killed then."""
    argv = [script_or_argv] if isinstance(script_or_argv, str) else list(script_or_argv)
    argv = [sys.executable, *argv, str(out), *(str(a) for a in extra_args)]
    env = world2_env() if env is None else env
    paths = [os.path.join(out, f"rank{r}.log") for r in range(world)]
    procs, killed, why = [], [], "time limit"
    try:
        for r, path in enumerate(paths):
            with open(path, "wb") as log:        # a file, not a pipe: nobody drains a pipe while the parent polls
                procs.append(subprocess.Popen(argv, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=log, stderr=subprocess.STDOUT))
        deadline = time.monotonic() + timeout    # one for the group
        while time.monotonic() < deadline:
            codes = [p.poll() for p in procs]
            if None not in codes:
                break
            failed = [r for r, c in enumerate(codes) if c]
            if failed and why == "time limit":
                why, deadline = f"killed after rank {failed[0]} failed", min(deadline, time.monotonic() + peer_grace)
            time.sleep(0.05)
    finally:
        for r, p in enumerate(procs):
            if p.poll() is None:
                p.kill()
                killed.append(r)
            p.wait()
    logs = []
    for path in paths:
        with open(path, errors="replace") as log:
            logs.append(log.read())
    if any(p.returncode != 0 for p in procs):
        codes = ", ".join(f"rank {r}: exit code {p.returncode}" + (f" ({why})" if r in killed else "") for r, p in enumerate(procs))
        raise AssertionError(codes + "\n" + "\n".join(lg[-3000:] for lg in logs))
    return logs


def load_ranks(out, modes=("eager", "graph"), world=2):
    """{mode: [rank 0's arrays, rank 1's, ...]} of the {mode}_rank{r}.npz files the ranks saved (dp_common.save)."""
    return {mode: [dict(np.load(os.path.join(out, f"{mode}_rank{r}.npz"))) for r in range(world)] for mode in modes}
