"""Global gradient-norm clipping (SOLVER.clip_grad_norm): the nef_grad_clip kernels against an fp64 reference, the eager trajectory of
FusedSGD / FusedAdam against torch.nn.utils.clip_grad_norm_ + torch's optimisers, graph replay against the eager path, clipping off,
and a step with a non-finite norm."""
import math
import random

import numpy as np
import pytest
import torch

from test_adam_gpu import _grads
from test_model_gpu import DEV, make_cfg
from util import rel

pytestmark = pytest.mark.gpu

GSCALE = 0.5


def _buf(g, off):
    """`g` on the device at `off` floats behind an allocation's (16-byte aligned) start."""
    b = torch.zeros(g.numel() + off, device=DEV)
    b[off:].copy_(g)
    return b[off:]


def _norm64(g):
    a = g.double().numpy()
    return GSCALE * math.sqrt(float((a * a).sum()))


def _bits(t):
    return t.detach().cpu().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernels vs fp64
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", [1, 1000, 4099, (1 << 20) + 3])
def test_clip_kernel_vs_fp64(n, off):
    """ops.grad_clip with max_norm = a quarter of the norm.  Bars: the norm and every scaled element carry one fp32 rounding of the
    norm, one of the coefficient and one of the product (<= 2e-7 together): 1e-6 leaves 5x."""
    from electrocardio_panorama_amd import ops
    g = _grads(n, 1, n + 1)[0]
    if n == 1:
        g[0] = 0.75                   # (a lone exact zero has no norm to take a quarter of)
    norm = _norm64(g)
    assert norm > 0
    max_norm = 0.25 * norm
    coef = float(np.float32(max_norm)) / (norm + 1e-6)
    g_dev = _buf(g, off)
    assert (g_dev.data_ptr() % 16 == 0) == (off == 0)
    stats = torch.zeros(4, device=DEV)
    ops.grad_clip(g_dev, max_norm, GSCALE, stats)
    s = stats.tolist()
    print(f"n={n} off={off}: norm {s[0]!r} vs {norm!r}, coef {s[1]!r} vs {coef!r}, g rel-L2 {rel(g_dev, g.double() * coef):.2e}")
    assert abs(s[0] - norm) <= 1e-6 * norm, (s[0], norm)
    assert abs(s[1] - coef) <= 1e-6, (s[1], coef)
    assert rel(g_dev, g.double() * coef) <= 1e-6
    zero = g == 0
    assert bool((g_dev.cpu()[zero] == 0).all()) and int(zero.sum()) == int((g_dev == 0).sum())
    assert s[2] == 1.0 and s[3] == 0.0


# ------------------------------------------------------------------------------------------------ 2. nothing to clip
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("case", ["four_times_the_norm", "inf", "all_zero"])
def test_clip_leaves_the_gradient_bit_identical_when_nothing_clips(case, off):
    from electrocardio_panorama_amd import ops
    n = 4099
    g = torch.zeros(n) if case == "all_zero" else _grads(n, 1, 7)[0]
    norm = _norm64(g)
    max_norm = {"four_times_the_norm": 4 * norm, "inf": math.inf, "all_zero": 1.0}[case]
    g_dev = _buf(g, off)
    stats = torch.zeros(4, device=DEV)
    ops.grad_clip(g_dev, max_norm, GSCALE, stats)
    s = stats.tolist()
    assert torch.equal(g_dev.cpu(), g)
    assert s[1] == 1.0 and s[2] == 0.0 and s[3] == 0.0
    assert abs(s[0] - norm) <= 1e-6 * norm and (case != "all_zero" or s[0] == 0.0)
    assert not any(math.isnan(v) for v in s)


# ------------------------------------------------------------------------------------------------ 3. range
def test_clip_norm_of_elements_whose_squares_overflow_fp32():
    from electrocardio_panorama_amd import ops
    n = 4099
    g = torch.full((n,), 1e30)
    g[::2] = -1e30
    norm = _norm64(g)                                        # 3.2e31: finite in fp32, the squares are not
    g_dev = _buf(g, 0)
    stats = torch.zeros(4, device=DEV)
    ops.grad_clip(g_dev, 1.0, GSCALE, stats)
    s = stats.tolist()
    assert abs(s[0] - norm) <= 1e-6 * norm, (s[0], norm)
    assert s[2] == 1.0 and s[3] == 0.0
    assert rel(g_dev, g.double() * (1.0 / norm)) <= 1e-6


@pytest.mark.parametrize("bad", [math.inf, math.nan], ids=["inf", "nan"])
def test_clip_non_finite_norm_taints_the_step(bad):
    from electrocardio_panorama_amd import ops
    n = 4099
    g = _grads(n, 1, 11)[0]
    g[1234] = bad
    g_dev = _buf(g, 0)
    stats, taint = torch.zeros(4, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_clip(g_dev, 0.25, GSCALE, stats, taint=taint)
    assert torch.equal(_bits(g_dev), _bits(g))               # (bit patterns: NaN != NaN)
    s = stats.tolist()
    assert not math.isfinite(s[0]) and s[1] == 1.0 and s[2] == 0.0 and s[3] == 1.0
    assert float(taint.item()) == 1.0
    # the update behind it skips the step and counts it
    gen = torch.Generator().manual_seed(12)
    p, buf = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    p0, buf0 = p.clone(), buf.clone()
    ops.sgd_momentum(p, g_dev, buf, 0.1, 0.9, GSCALE, False)         # (the counters exist; reset the host's mark)
    p.copy_(p0), buf.copy_(buf0)
    ops.h2_skipped()
    ops.sgd_momentum(p, g_dev, buf, 0.1, 0.9, GSCALE, False, skip=taint)
    assert torch.equal(p, p0) and torch.equal(buf, buf0)
    assert ops.h2_skipped() == 1


def test_clip_leaves_an_already_tainted_step_alone():
    from electrocardio_panorama_amd import ops
    n = 4099
    g = _grads(n, 1, 13)[0]
    g_dev = _buf(g, 0)
    stats = torch.tensor([0.0, 0.0, 5.0, 7.0], device=DEV)
    taint = torch.ones(1, device=DEV)
    ops.grad_clip(g_dev, 0.25 * _norm64(g), GSCALE, stats, taint=taint)
    assert torch.equal(g_dev.cpu(), g)
    assert stats[2:].tolist() == [5.0, 7.0] and float(taint.item()) == 1.0


# ------------------------------------------------------------------------------------------------ Solver-level helpers
V, B, L = 3, 2, 512
CLIP = 0.25      # the unclipped norms of the first steps on these batches and weights are 0.8 .. 1.1 (CPU oracle): 3x headroom


def _solver(optim, graph, clip, reg="l1_loss"):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, reg=reg, lr={"sgd": 0.1, "adam": 1e-3}[optim])
    cfg.SOLVER["optim"] = optim
    cfg.SOLVER["graph"] = bool(graph)
    cfg.SOLVER["clip_grad_norm"] = clip
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


def _batches(n, seed0=40):
    from electrocardio_panorama_amd import synth
    return [synth.make_batch(B, V, L, seed=seed0 + i, Q=2) for i in range(n)]


_SLOTS = {"sgd": ("buf",), "adam": ("m", "v", "step")}


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + \
        [v.clone() for k, v in sol.model.named_buffers() if "running" in k]


# ------------------------------------------------------------------------------------------------ 4. eager trajectory vs torch
@pytest.mark.parametrize("optim", ["sgd", "adam"])
def test_clip_eager_trajectory_vs_torch(optim):
    """Three eager steps with clip_grad_norm = 0.25; the gradients of every step, cloned before opt.step(), replayed through
    torch.nn.utils.clip_grad_norm_ + torch's optimiser on shadow parameters.  Bar: test_adam_kernel_vs_torch's 1e-5 on the update."""
    from electrocardio_panorama_amd.network import build_loss
    cfg, sol, opt = _solver(optim, False, CLIP)
    sol.model.train()
    lossf = build_loss(cfg)
    params = list(sol.model.parameters())
    p0 = [p.detach().clone() for p in params]
    shadow = [torch.nn.Parameter(p.clone()) for p in p0]
    ropt = torch.optim.SGD(shadow, lr=0.1, momentum=0.9) if optim == "sgd" else torch.optim.Adam(shadow, lr=1e-3, foreach=False)
    for i, b in enumerate(_batches(3)):
        b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}
        random.seed(100 + i)
        o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
        lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
        for p, s in zip(params, shadow):
            s.grad = None if p.grad is None else p.grad.detach().clone()
        opt.step()
        opt.zero_grad()
        total, coef = opt.clip_stats[:2].tolist()
        ref_total = float(torch.nn.utils.clip_grad_norm_(shadow, CLIP))
        ropt.step()
        print(f"{optim} step {i}: norm {total!r} (torch {ref_total!r}), coef {coef!r}")
        assert coef < 1.0, (i, total, coef)                  # the test cannot pass without clipping
        assert abs(total - ref_total) <= 1e-5 * ref_total
    live = [i for i, s in enumerate(shadow) if s.grad is not None]
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])      # noqa: E731
    d0 = cat([p0[i] for i in live])
    e = rel(cat([params[i] for i in live]) - d0, cat([shadow[i] for i in live]) - d0)
    assert e <= 1e-5, e
    keys = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq")}[optim]
    for k in keys:
        e = rel(cat([opt.state[params[i]][k] for i in live]), cat([ropt.state[shadow[i]][k] for i in live]))
        assert e <= 1e-5, (k, e)
    assert opt.clip_stats[2:].tolist() == [3.0, 0.0]


# ------------------------------------------------------------------------------------------------ 5. graphed == eager
@pytest.mark.parametrize("optim", ["sgd", "adam"])
def test_clip_graphed_equals_eager_across_lr_milestone(optim):
    """Six clipped steps with a MultiStepLR milestone crossed after step 3: the replayed step equals the eager one bit for bit
    (parameters, optimiser state, BatchNorm statistics, the reported norms and coefficients) from one capture; a new max_grad_norm
    takes effect on the next step of both paths."""
    from torch.optim.lr_scheduler import MultiStepLR
    batches = _batches(7)
    out = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(optim, graph, CLIP)
        sched = MultiStepLR(opt, [3], gamma=0.1)
        norms, slot = [], None
        for i, b in enumerate(batches[:6]):
            random.seed(100 + i)
            sol.run_one_epoch([b], "train", opt, collect_views=False)
            sched.step()
            norms += sol.last_grad_norms
            if graph:
                st = sol._graph_stepper
                assert st is not None and len(st.slots) == 1
                slot = slot or next(iter(st.slots.values()))
                assert next(iter(st.slots.values())) is slot          # one capture only
        six = _state(sol, opt, optim)
        opt.max_grad_norm = 100.0
        random.seed(106)
        sol.run_one_epoch([batches[6]], "train", opt, collect_views=False)
        assert len(sol.last_grad_norms) == 1 and sol.last_grad_norms[0][1] == 1.0
        assert sol.last_clip_counts == (0, 0)
        out[graph] = (six, norms, _state(sol, opt, optim), sol.last_grad_norms, opt.clip_stats.tolist())
    assert len(out[True][1]) == 6 and all(c < 1.0 for _, c in out[True][1])
    assert out[False][1] == out[True][1] and out[False][3] == out[True][3] and out[False][4] == out[True][4]
    assert out[True][4][2:] == [6.0, 0.0]
    for k in (0, 2):
        for a, b in zip(out[False][k], out[True][k]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. off is off
def test_clip_off_is_off():
    """Three graphed SGD steps: a max_norm nothing reaches (100) gives the bits of clipping off; with it off the optimiser owns no
    stats words and the Solver reports no norms."""
    out = {}
    for clip in (0.0, 100.0):
        cfg, sol, opt = _solver("sgd", True, clip)
        norms = []
        for i, b in enumerate(_batches(3)):
            random.seed(100 + i)
            sol.run_one_epoch([b], "train", opt, collect_views=False)
            norms += sol.last_grad_norms
        assert sol._graph_stepper is not None
        out[clip] = _state(sol, opt, "sgd")
        if clip == 0.0:
            assert opt.clip_stats is None and norms == []
        else:
            assert len(norms) == 3 and all(c == 1.0 and 0.0 < t < 100.0 for t, c in norms)
            assert opt.clip_stats[2:].tolist() == [0.0, 0.0]
    for a, b in zip(out[0.0], out[100.0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. a non-finite step
def test_clip_non_finite_step_through_the_solver(monkeypatch):
    """An eager step whose target carries a NaN (reg_loss l2: the gradient of |d| at a NaN is 0, that of d^2 is NaN) has a non-finite
    gradient norm: parameters and momentum stay as they are and the epoch reports one skipped step.  On the fp32 kernels (ops.H2 False),
    so that it is the clip's rule that skips the step, not the split-fp16 taint."""
    from electrocardio_panorama_amd import ops
    monkeypatch.setattr(ops, "H2", False)
    cfg, sol, opt = _solver("sgd", False, CLIP, reg="l2_loss")
    good, bad = _batches(2)
    bad = dict(bad)
    tv = np.array(bad["target_view"], copy=True)
    tv.reshape(-1)[5] = np.nan
    bad["target_view"] = tv
    random.seed(100)
    sol.run_one_epoch([good], "train", opt, collect_views=False)
    assert sol.last_clip_counts[1] == 0 and math.isfinite(sol.last_grad_norms[0][0])
    before = _state(sol, opt, "sgd")[:2]
    random.seed(101)
    sol.run_one_epoch([bad], "train", opt, collect_views=False)
    assert sol.last_clip_counts == (0, 1)
    assert not math.isfinite(sol.last_grad_norms[0][0]) and sol.last_grad_norms[0][1] == 1.0
    for a, b in zip(before, _state(sol, opt, "sgd")[:2]):
        assert torch.equal(a, b)
