"""Checks that several two-rank tests (tests/test_dp_*_gpu.py) make in the same words, on what dp_launch.load_ranks returns."""
import numpy as np

from util import rel


def ranks_agree_and_graphed_equals_eager(eager, graph, row_len):
    """One FusedSGD step: both ranks end bit for bit alike on different shards, and the graphed step is the eager one bit for bit."""
    for k in ("p", "buf", "p0"):
        assert np.array_equal(eager[0][k], eager[1][k]), k
    for k in ("p", "buf"):
        assert np.array_equal(graph[0][k], graph[1][k]), k
    assert not np.array_equal(eager[0]["grad"], eager[1]["grad"])       # the ranks saw different shards
    for e, g in zip(eager, graph):
        for k in ("p", "buf"):
            assert np.array_equal(e[k], g[k]), k
        assert g["losses"].shape == (1, row_len) and np.array_equal(g["losses"][0], e["losses"])


def update_is_mean_of_gradients(eager, label, bar):
    """The single-process step on the mean of the two shards' gradients, in fp64: displacement rel-L2 against p0 - lr * mean(g) <= bar."""
    a, b = eager
    p0 = a["p0"].astype(np.float64)
    want = p0 - float(a["lr"]) * np.stack([a["grad"], b["grad"]]).astype(np.float64).mean(0)
    got = a["p"].astype(np.float64)
    e = rel(got - p0, want - p0)
    floor = rel(want.astype(np.float32).astype(np.float64) - p0, want - p0)
    shown = f"{bar:.1e}".replace("e-0", "e-")
    print(f"world 2, {label}: displacement of the update vs fp64 {e:.3e} (bar {shown}); the fp64 result rounded to fp32 sits at "
          f"{floor:.3e}; displacement rms {np.sqrt(np.mean((want - p0) ** 2)):.3e}")
    assert rel(got - p0, 2.0 * (want - p0)) > 0.1              # a sum instead of the mean is far outside
    assert e <= bar


def consumes_the_early_bucket(eager):
    for z in eager:
        assert (z["early"] > 0).all()                      # engine.backward started the bucket every step ...
        assert (z["reduced"] > 0).all() and (z["reduced"] < int(z["n"])).all()     # ... and the step reduced only the rest
