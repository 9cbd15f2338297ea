"""Layer-wise trust ratios on the device: nef_update_trust (LARS, LAMB; one norm pair per segment by a deterministic segmented reduction)
against an fp64 restatement of the formulas of include/nefnet_hip.h, written here as a plain torch-on-CPU loop over the segments --
neither optimiser exists in torch.optim.  Then its bit boundaries (nef_update, replay, the skip word, lr_dev, a non-finite gradient, the
average), FusedLARS / FusedLAMB, the model's eager step, graph replay against the eager path, and a checkpoint in a graphed run.

Bars.  Parameters and state buffers: rel-L2 <= 1e-6 (the project's bar in tests/test_wd_gpu.py).  Every ratio: within 1e-5 relative.
Displacement p - p0: no fixed number -- the same recurrences in plain fp32 on the CPU (fp64 norms) already sit at 1e-5 from the oracle
for LAMB (p's own rounding against a small displacement), so each case computes that fp32 restatement's distance, prints both figures
and demands kernel <= 4 x restatement (the margin covers multiply-add contraction and another operation order inside the Adam element;
a wrong ratio, a wrong segment or an ignored adapt flag is off by O(1)).  Sensitivity: with every adapt flag 0 the displacement and the
ratios are outside those bars by more than 100 x."""
import copy
import functools
import random

import numpy as np
import pytest
import torch

from test_model_gpu import DEV, make_cfg
from util import rel

pytestmark = pytest.mark.gpu

GSCALE = 0.5      # as after a two-rank all-reduce sum
COEF, TEPS = 1e-3, 1e-8
RULES = {      # rule -> (kind, nesterov, lr, weight_decay, eps)
    "lars": ("lars", False, 0.1, 0.05, 0.0),
    "lars-nesterov": ("lars", True, 0.1, 0.05, 0.0),
    "lamb": ("lamb", False, 1e-3, 0.01, 1e-6),
}
NO_DECAY = ["*.bias", "decoder.*.double_conv.[14].weight"]      # the model's biases and BatchNorm affine parameters: its 1-D tensors


def _grads(n, steps, seed):      # the recipe of tests/test_wd_gpu.py
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0          # exact zeros (dead units)
        out.append(g)
    return out


def _table_a():
    """One-element segments at the start and in the middle, ends inside a 16-byte vector (1, 6, 1030, 1031) and on a vector boundary."""
    return [1, 6, 1030, 1031, 2048, 4099], [1.0, 0.0, 1.0, 0.0, 0.5, 1.0], [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]


def _table_b():
    """256 segments (the cap): 255 of sizes cycling through 1, 2, 3, 5, 64, 129, 4, 7 and one of 1,200,003 elements at position 100 -- many
    segments per chunk and one segment across many blocks, whatever the chunk size."""
    cyc = (1, 2, 3, 5, 64, 129, 4, 7)
    sizes = [cyc[i % 8] for i in range(255)]
    sizes.insert(100, 1200003)
    ends = np.cumsum(sizes).tolist()
    return ends, [0.0 if i % 3 == 1 else 1.0 for i in range(256)], [0.0 if i % 4 == 2 else 1.0 for i in range(256)]


TABLES = {"A": _table_a, "B": _table_b}


@functools.lru_cache(maxsize=None)
def _inputs(table, steps=5):
    """p0 and the gradients of a table.  Table B scales both per segment so that the ratios span orders of magnitude."""
    ends = TABLES[table]()[0]
    n = ends[-1]
    gen = torch.Generator().manual_seed(n)
    p0, grads = torch.randn(n, generator=gen), _grads(n, steps, n + 1)
    if table == "B":
        ps, gs = torch.ones(n), torch.ones(n)
        for i, (b, e) in enumerate(zip([0] + ends[:-1], ends)):
            ps[b:e], gs[b:e] = 10.0 ** (i % 5 - 2), 10.0 ** (i % 3 - 1)
        p0, grads = p0 * ps, [g * gs for g in grads]
    return p0, grads


def _restate(rule, p0, grads, ends, wd_muls, adapts, dtype, gscale=GSCALE, lr=None, wd=None, coef=COEF, teps=TEPS):
    """The formulas of the header, over the segments one by one, with every element-wise operation in `dtype` (fp64: the oracle; fp32:
    the restatement the displacement bar is measured with) and the norms always fp64 sums of squares.  Returns the parameters, the state
    buffers and the ratios of the last step."""
    kind, nesterov, lr0, wd0, eps = RULES[rule]
    lr, wd = lr0 if lr is None else lr, wd0 if wd is None else wd
    p = p0.to(dtype).clone()
    s0, s1 = torch.zeros_like(p), torch.zeros_like(p)
    begs = [0] + list(ends[:-1])
    b1, b2, mu = 0.9, 0.999, 0.9
    q_last = []
    for t, g in enumerate(grads, 1):
        gp = g.to(dtype) * gscale
        q_last = []
        if kind == "lamb":
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for b, e, mul, ad in zip(begs, ends, wd_muls, adapts):
            ps, gs = p[b:e], gp[b:e]
            wd_s = wd * mul
            wn = float(ps.double().pow(2).sum().sqrt())
            if kind == "lars":
                gn = float(gs.double().pow(2).sum().sqrt())
                q = coef * wn / (gn + wd_s * wn + teps) if ad and wn > 0 and gn > 0 else 1.0
                if dtype == torch.float32:
                    q = float(np.float32(q))
                d = (gs + wd_s * ps) * q
                s0[b:e] = mu * s0[b:e] + d
                p[b:e] = ps - lr * (d + mu * s0[b:e] if nesterov else s0[b:e])
            else:
                m = s0[b:e] + (1.0 - b1) * (gs - s0[b:e])
                v = b2 * s1[b:e] + (1.0 - b2) * gs * gs
                s0[b:e], s1[b:e] = m, v
                u = (m / bc1) / ((v / bc2).sqrt() + eps) + wd_s * ps
                un = float(u.double().pow(2).sum().sqrt())
                q = wn / un if ad and wn > 0 and un > 0 else 1.0
                if dtype == torch.float32:
                    q = float(np.float32(q))
                p[b:e] = ps - lr * q * u
            q_last.append(q)
    state = [s0] if kind == "lars" else [s0, s1]
    return [p] + state, q_last


@functools.lru_cache(maxsize=None)
def _reference(rule, table):
    """Computed once per (rule, table): the oracle, its last ratios, and the fp32 restatement's displacement distance to it."""
    p0, grads = _inputs(table)
    tab = TABLES[table]()
    want, q = _restate(rule, p0, grads, *tab, torch.float64)
    f32, _ = _restate(rule, p0, grads, *tab, torch.float32)
    return want, q, rel(f32[0].double() - p0.double(), want[0] - p0.double())


def _dev_table(ends, wd_muls, adapts):
    return (torch.tensor(ends, device=DEV, dtype=torch.int64), torch.tensor(wd_muls, device=DEV, dtype=torch.float32),
            torch.tensor(adapts, device=DEV, dtype=torch.float32))


def _views(n, off, k):
    """k zeroed fp32 device buffers of n elements that start `off` floats behind a 16-byte boundary."""
    return [torch.zeros(n + off, device=DEV)[off:] for _ in range(k)]


def _aux(segs):
    """The caller-owned ratio table and stats words."""
    return torch.ones(segs[0].numel(), device=DEV), torch.tensor([1.0, 1.0, 0.0, 0.0], device=DEV)


def _call(rule, t, g, segs, ratio, stats, gscale=GSCALE, lr=None, coef=COEF, teps=TEPS, **kw):
    """One ops.update_lars / ops.update_lamb call of `rule` over t = (p, s0, s1, step)."""
    from electrocardio_panorama_amd import ops
    kind, nesterov, lr0, wd, eps = RULES[rule]
    lr = lr0 if lr is None else lr
    if kind == "lars":
        ops.update_lars(t[0], g, t[1], lr, 0.9, gscale, segs, ratio, stats, trust_coef=coef, trust_eps=teps, weight_decay=wd,
                        nesterov=nesterov, **kw)
    else:
        ops.update_lamb(t[0], g, t[1], t[2], t[3], lr, 0.9, 0.999, eps, wd, gscale, segs, ratio, stats, **kw)


def _kernel_steps(rule, p0, grads, table, off):
    kind = RULES[rule][0]
    n = p0.numel()
    p, g_dev, s0, s1 = _views(n, off, 4)
    p.copy_(p0)
    step = torch.zeros(1, device=DEV)
    segs = _dev_table(*table)
    ratio, stats = _aux(segs)
    for g in grads:
        g_dev.copy_(g)
        _call(rule, (p, s0, s1, step), g_dev, segs, ratio, stats)
    torch.cuda.synchronize()
    assert float(step.item()) == (0.0 if kind == "lars" else len(grads))
    return [p.cpu(), s0.cpu()] + ([] if kind == "lars" else [s1.cpu()]), ratio.cpu().double().tolist(), stats.cpu().tolist()


def _ratio_err(got, want):
    return max(abs(a - b) / abs(b) for a, b in zip(got, want))


def _check(got, q, want, q_want, bar_disp, p0, what=""):
    """The bars of the module docstring; every figure is printed before it is asserted."""
    p0 = p0.double()
    e_state = [rel(a.double(), b) for a, b in zip(got[1:], want[1:])]
    e_p = rel(got[0].double(), want[0])
    e_disp = rel(got[0].double() - p0, want[0] - p0)
    e_q = _ratio_err(q, q_want)
    print(f"{what}: state {e_state}, parameters {e_p:.3e}, ratios {e_q:.3e} (they span {min(q_want):.3e} .. {max(q_want):.3e}), "
          f"displacement {e_disp:.3e} against the fp32 restatement's {bar_disp:.3e}")
    assert all(e <= 1e-6 for e in e_state), e_state
    assert e_p <= 1e-6, e_p
    assert e_q <= 1e-5, e_q
    assert e_disp <= 4 * bar_disp, (e_disp, bar_disp)


# ------------------------------------------------------------------------------------------------ 1. the kernels against the oracle
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("table", ["A", "B"])
def test_trust_kernel_vs_oracle(table, rule, off):
    """Five steps with gscale = 0.5 and 10 % exact zeros in the gradients."""
    p0, grads = _inputs(table)
    tab = TABLES[table]()
    want, q_want, bar = _reference(rule, table)
    got, q, stats = _kernel_steps(rule, p0, grads, tab, off)
    _check(got, q, want, q_want, bar, p0, f"table {table}, {rule}, off {off}")
    adapted = [a for a, ad in zip(q, tab[2]) if ad]
    assert all(a == 1.0 for a, ad in zip(q, tab[2]) if not ad)                      # exempt segments step at the plain rate
    assert stats[0] == np.float32(min(adapted)) and stats[1] == np.float32(max(adapted)) and stats[2:] == [5.0, 0.0]
    if off == 0:      # the adapt flags matter: without them the result is far outside the bars
        flat, q1, _ = _kernel_steps(rule, p0, grads, (tab[0], tab[1], [0.0] * len(tab[0])), off)
        e_disp, e_q = rel(flat[0].double() - p0.double(), want[0] - p0.double()), _ratio_err(q1, q_want)
        print(f"all adapt = 0: displacement {e_disp:.3e}, ratios {e_q:.3e}")
        assert e_disp > 100 * 4 * bar and e_q > 100 * 1e-5


@pytest.mark.parametrize("rule", ["lars", "lamb"])
@pytest.mark.parametrize("zero", ["p", "g"])
def test_zero_norm_segments(rule, zero):
    """Table A with segment [1031, 2048) of p zeroed / segment [6, 1030) of every g zeroed, against the oracle.  Where the formulas give
    q = 1 it is exactly 1: a zero weight norm (both rules), a zero gradient norm (LARS).  (LAMB's direction in a decayed segment with zero
    gradients is wd_s * p, whose norm is not zero: its ratio is 1 / wd_s, as the oracle says.)"""
    p0, grads = _inputs("A")
    p0, grads = p0.clone(), [g.clone() for g in grads]
    if zero == "p":
        p0[1031:2048] = 0.0
        grads = grads[:1]          # (the segment has a norm again after the first step)
    else:
        for g in grads:
            g[6:1030] = 0.0
    tab = _table_a()
    if zero == "p":
        tab = (tab[0], tab[1], [1.0] * 6)      # (the table exempts that segment anyway: let the zero norm decide here)
    want, q_want = _restate(rule, p0, grads, *tab, torch.float64)
    f32, _ = _restate(rule, p0, grads, *tab, torch.float32)
    bar = rel(f32[0].double() - p0.double(), want[0] - p0.double())
    got, q, _ = _kernel_steps(rule, p0, grads, tab, 0)
    _check(got, q, want, q_want, bar, p0, f"{rule}, zero {zero}")
    if zero == "p":
        assert q[4] == 1.0 and q_want[4] == 1.0
    elif rule == "lars":
        assert q[2] == 1.0 and q_want[2] == 1.0
    else:
        assert q_want[2] == pytest.approx(1.0 / 0.01, rel=1e-6)


# ------------------------------------------------------------------------------------------------ 2. bit boundaries
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("rule", ["lars", "lars-nesterov"])
def test_lars_without_adapted_segments_is_update_sgd_bit_for_bit(rule, off):
    """Every adapt flag 0: q = 1 everywhere, and the multipliers of the segments are the run table of ops.update_sgd."""
    from electrocardio_panorama_amd import ops
    _, nesterov, lr, wd, _ = RULES[rule]
    ends, wd_muls, _ = _table_a()
    n = ends[-1]
    p0, grads = _inputs("A")
    segs = _dev_table(ends, wd_muls, [0.0] * len(ends))
    ratio, stats = _aux(segs)
    pa, ga, ba = _views(n, off, 3)
    pb, gb, bb = _views(n, off, 3)
    pa.copy_(p0), pb.copy_(p0)
    for g in grads[:3]:
        ga.copy_(g), gb.copy_(g)
        _call(rule, (pa, ba, None, None), ga, segs, ratio, stats)
        ops.update_sgd(pb, gb, bb, lr, 0.9, GSCALE, wd, nesterov, runs=(segs[0], segs[1]))
    assert torch.equal(pa, pb) and torch.equal(ba, bb) and not torch.equal(pa.cpu(), p0)
    assert ratio.tolist() == [1.0] * len(ends) and stats.tolist() == [1.0, 1.0, 3.0, 0.0]


@pytest.mark.parametrize("rule", ["lars-nesterov", "lamb"])
@pytest.mark.parametrize("table", ["A", "B"])
def test_two_calls_and_a_replay_give_equal_bits(table, rule):
    """Two calls on equal buffers give equal bits, and so do an eager call and a replayed capture of the same call."""
    p0, grads = _inputs(table)
    segs = _dev_table(*TABLES[table]())
    n = p0.numel()
    runs = []
    for _ in range(3):
        p, g_dev, s0, s1 = _views(n, 0, 4)
        p.copy_(p0)
        runs.append(((p, s0, s1, torch.zeros(1, device=DEV)), g_dev) + _aux(segs))
    (ta, ga, ra, sa), (tb, gb, rb, sb), (tc, gc, rc, sc) = runs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gc.copy_(grads[0])
        _call(rule, tc, gc, segs, rc, sc)              # (warm-up on the capture stream: its workspace exists before the capture)
        side.synchronize()
        tc[0].copy_(p0)
        for t in tc[1:]:
            t.zero_()
        rc.fill_(1.0), sc.copy_(torch.tensor([1.0, 1.0, 0.0, 0.0]))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _call(rule, tc, gc, segs, rc, sc)
    for g in grads[:3]:
        ga.copy_(g), gb.copy_(g), gc.copy_(g)
        _call(rule, ta, ga, segs, ra, sa)
        _call(rule, tb, gb, segs, rb, sb)
        graph.replay()
    torch.cuda.synchronize()
    for other, ro, so in ((tb, rb, sb), (tc, rc, sc)):
        for a, b in zip(ta + (ra, sa), other + (ro, so)):
            assert torch.equal(a, b)
    assert sa.tolist()[2:] == [3.0, 0.0] and not torch.equal(ta[0].cpu(), p0)


@pytest.mark.parametrize("rule", ["lars-nesterov", "lamb"])
def test_trust_skip_word_and_lr_dev(rule):
    """A positive skip word leaves p, the state, *step, the ratio table and the stats bit-identical and counts once; a zero word steps;
    lr_dev replaces lr."""
    from electrocardio_panorama_amd import ops
    kind, _, lr, _, _ = RULES[rule]
    p0, grads = _inputs("A")
    n = p0.numel()
    segs = _dev_table(*_table_a())
    ratio, stats = _aux(segs)
    p, s0, s1 = _views(n, 0, 3)
    p.copy_(p0)
    state = (p, s0, s1, torch.zeros(1, device=DEV))
    g1, g2 = (g.to(DEV) for g in grads[:2])
    _call(rule, state, g1, segs, ratio, stats)
    ops.h2_skipped()                                         # (reset the host's mark)
    before = [t.clone() for t in state + (ratio, stats)]
    _call(rule, state, g2, segs, ratio, stats, skip=torch.ones(1, device=DEV))
    for a, b in zip(state + (ratio, stats), before):
        assert torch.equal(a, b)
    assert ops.h2_skipped() == 1
    a = [t.clone() for t in before]
    b = [t.clone() for t in before]
    _call(rule, a[:4], g2, segs, a[4], a[5], skip=torch.zeros(1, device=DEV), lr_dev=torch.full((1,), 5 * lr, device=DEV))
    _call(rule, b[:4], g2, segs, b[4], b[5], lr=5 * lr)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], before[0]) and float(a[3].item()) == (0.0 if kind == "lars" else 2.0)
    assert a[5].tolist()[2:] == [2.0, 0.0] and not torch.equal(a[4], before[4])
    assert ops.h2_skipped() == 0


@pytest.mark.parametrize("rule", ["lars", "lamb"])
@pytest.mark.parametrize("table", ["A", "B"])
def test_one_inf_in_the_gradient_skips_the_step(table, rule):
    """stats[3] and the taint word advance by 1, nothing else moves, and the step counts in h2_skipped()."""
    from electrocardio_panorama_amd import ops
    p0, grads = _inputs(table)
    n = p0.numel()
    segs = _dev_table(*TABLES[table]())
    ratio, stats = _aux(segs)
    p, s0, s1 = _views(n, 0, 3)
    p.copy_(p0)
    state = (p, s0, s1, torch.zeros(1, device=DEV))
    taint = torch.zeros(4, device=DEV)
    _call(rule, state, grads[0].to(DEV), segs, ratio, stats, skip=taint[:1], taint=taint[:1])
    ops.h2_skipped()
    before = [t.clone() for t in state + (ratio,)]
    g = grads[1].clone()
    g[n // 2] = float("inf")
    _call(rule, state, g.to(DEV), segs, ratio, stats, skip=taint[:1], taint=taint[:1])
    for a, b in zip(state + (ratio,), before):
        assert torch.equal(a, b)
    assert stats.tolist()[2:] == [1.0, 1.0] and taint.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert ops.h2_skipped() == 1
    # without a taint word the step is skipped all the same
    _call(rule, state, g.to(DEV), segs, ratio, stats)
    for a, b in zip(state + (ratio,), before):
        assert torch.equal(a, b)
    assert stats.tolist()[2:] == [1.0, 2.0]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("rule", ["lars-nesterov", "lamb"])
def test_trust_with_the_average(rule, off):
    """With ema=: p and the state are bit-identical to the call without it; the average is within t * 3 * 2^-24 * max|p| of the fp64
    recurrence over the kernel's own parameters (the bar of tests/test_ema_gpu.py)."""
    decay, warmup = 0.9, True
    p0, grads = _inputs("A")
    n = p0.numel()
    segs = _dev_table(*_table_a())
    pa, ga, s0a, s1a, ema = _views(n, off, 5)
    pb, gb, s0b, s1b = _views(n, off, 4)
    stepa, stepb, ema_n = (torch.zeros(1, device=DEV) for _ in range(3))
    (ra, sa), (rb, sb) = _aux(segs), _aux(segs)
    pa.copy_(p0), pb.copy_(p0), ema.copy_(p0)
    traj = []
    for g in grads:
        ga.copy_(g), gb.copy_(g)
        _call(rule, (pa, s0a, s1a, stepa), ga, segs, ra, sa, ema=(ema, ema_n, decay, warmup))
        _call(rule, (pb, s0b, s1b, stepb), gb, segs, rb, sb)
        traj.append(pa.cpu().numpy())
    for a, b in ((pa, pb), (s0a, s0b), (s1a, s1b), (stepa, stepb), (ra, rb), (sa, sb)):
        assert torch.equal(a, b)
    assert float(ema_n.item()) == len(grads)
    e = p0.numpy().astype(np.float64)
    for t, p in enumerate(traj):
        w = float(np.float32(1.0 - min(decay, (1.0 + t) / (10.0 + t))))
        e = e + w * (p.astype(np.float64) - e)
    bar = len(traj) * 3 * 2.0 ** -24 * max(float(np.abs(p).max()) for p in [p0.numpy()] + traj)
    err = float(np.abs(ema.cpu().numpy().astype(np.float64) - e).max())
    print(f"{rule}, off {off}: max |ema - recurrence| {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    # a skipped step leaves the average and its count as they are
    before = [ema.clone(), ema_n.clone(), pa.clone()]
    _call(rule, (pa, s0a, s1a, stepa), ga, segs, ra, sa, ema=(ema, ema_n, decay, warmup), skip=torch.ones(1, device=DEV))
    assert torch.equal(ema, before[0]) and torch.equal(ema_n, before[1]) and torch.equal(pa, before[2])


# ------------------------------------------------------------------------------------------------ 3. the optimisers
_NAMED = (("a.bias", (1,)), ("b.weight", (3,)), ("c.bias", (128,)), ("d.weight", (64, 3)), ("e.weight", (130,)))


def _named_params(dev):
    gen = torch.Generator().manual_seed(50)
    out = []
    for name, shape in _NAMED:
        p = torch.nn.Parameter(torch.randn(*shape, generator=gen).to(dev))
        p._nef_name = name
        out.append(p)
    return out


def _cat(ts):
    return torch.cat([torch.as_tensor(t).detach().reshape(-1).cpu() for t in ts])


def _fused(kind, params, **kw):
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedLAMB, FusedLARS
    if kind == "lars":
        return FusedLARS(params, lr=0.1, momentum=0.9, weight_decay=0.05, nesterov=True, no_decay=["*.bias"], trust_exempt=["*.bias"], **kw)
    return FusedLAMB(params, lr=1e-3, weight_decay=0.01, no_decay=["*.bias"], trust_exempt=["*.bias"], **kw)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_fused_optimisers_vs_oracle(kind):
    """FusedLARS(nesterov) / FusedLAMB over named tensors of sizes [1], [3], [128], [64, 3], [130] with the biases exempt from decay and
    from the ratio: five steps against the oracle, trust_ratios(), and a state-dict round trip through a fresh instance."""
    from electrocardio_panorama_amd import ops
    ops.h2_rebase()      # no model runs here: clamps an earlier test left uncharged must not taint (skip) this test's first step
    ops.h2_skipped()
    rule, keys = ("lars-nesterov", ("momentum_buffer",)) if kind == "lars" else ("lamb", ("exp_avg", "exp_avg_sq"))
    params = _named_params(DEV)
    p0 = _cat(params)
    n = p0.numel()
    opt = _fused(kind, params)
    grads = _grads(n, 6, 51)

    def step(o, ps, g):
        off = 0
        for p in ps:
            p.grad = g[off:off + p.numel()].view_as(p).clone().to(p.device)
            off += p.numel()
        o.step()

    for g in grads[:5]:
        step(opt, params, g)
    assert ops.h2_skipped() == 0
    fl = opt._flat[0]
    ends, exempt = [1, 4, 132, 324, n], [0.0, 1.0, 0.0, 1.0, 1.0]
    assert fl["seg_end"].tolist() == ends and fl["seg_wd_mul"].tolist() == exempt and fl["seg_adapt"].tolist() == exempt
    assert "run_end" not in fl
    tab = (ends, exempt, exempt)
    want, q_want = _restate(rule, p0, grads[:5], *tab, torch.float64, gscale=1.0)
    f32, _ = _restate(rule, p0, grads[:5], *tab, torch.float32, gscale=1.0)
    bar = rel(f32[0].double() - p0.double(), want[0] - p0.double())
    got = lambda o, ps: [_cat(ps)] + [_cat([o.state[p][k] for p in ps]) for k in keys]      # noqa: E731
    ratios = opt.trust_ratios()
    assert list(ratios) == [name for name, _ in _NAMED]
    assert ratios["a.bias"] == 1.0 and ratios["c.bias"] == 1.0 and all(ratios[k] != 1.0 for k in ("b.weight", "d.weight", "e.weight"))
    _check(got(opt, params), list(ratios.values()), want, q_want, bar, p0, f"{kind}, 5 steps")
    assert opt.trust_stats.tolist()[2:] == [5.0, 0.0]
    # a fresh instance over equal parameters loads the state dict (torch's format plus the two group keys) and steps the same bits
    sd = copy.deepcopy(opt.state_dict())
    g0 = sd["param_groups"][0]
    assert g0["trust_coef"] == 1e-3 and g0["trust_eps"] == 1e-8 and "trust_exempt" not in g0
    if kind == "lamb":
        assert all(float(s["step"]) == 5.0 for s in sd["state"].values()) and g0["eps"] == 1e-6
    params2 = _named_params(DEV)
    for p, q in zip(params2, params):
        p.data.copy_(q.data)
    opt2 = _fused(kind, params2)
    opt2.load_state_dict(sd)
    step(opt, params, grads[5])
    step(opt2, params2, grads[5])
    for a, b in zip(got(opt, params), got(opt2, params2)):
        assert torch.equal(a, b)
    assert opt.trust_ratios() == opt2.trust_ratios()


def test_more_segments_than_the_cap_is_refused():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedLARS
    params = [torch.nn.Parameter(torch.ones(2, device=DEV)) for _ in range(257)]
    for p in params:
        p.grad = torch.ones_like(p)
    opt = FusedLARS(params, lr=0.1)
    with pytest.raises(ValueError, match="257"):
        opt.step()


# ------------------------------------------------------------------------------------------------ Solver-level helpers
V, B, L = 3, 2, 512
WD = 1e-2
_LR = {"lars": 0.1, "lamb": 1e-3, "sgd": 0.1, "adam": 1e-3}
_SLOTS = {"lars": ("buf",), "lamb": ("m", "v", "step")}


def _solver(optim, graph, clip=0.0, ema=0.0, bare=False):
    """`bare`: a config written before any of the keys existed."""
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr=_LR[optim])
    cfg.SOLVER["optim"] = optim
    cfg.SOLVER["graph"] = bool(graph)
    if bare:
        for k in ("trust_coef", "trust_eps", "trust_exempt"):
            cfg.SOLVER.pop(k, None)
    else:
        cfg.SOLVER["weight_decay"] = WD
        cfg.SOLVER["nesterov"] = optim == "lars"
        cfg.SOLVER["no_decay"] = list(NO_DECAY)
        cfg.SOLVER["trust_exempt"] = list(NO_DECAY)
        cfg.SOLVER["clip_grad_norm"] = clip
        cfg.SOLVER["ema_decay"] = ema
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


def _batches(n, seed0=40):
    from electrocardio_panorama_amd import synth
    return [synth.make_batch(B, V, L, seed=seed0 + i, Q=2) for i in range(n)]


def _state(sol, opt, optim, extra=()):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim] + ("ratio", "trust_stats") + tuple(extra)] + \
        [v.clone() for k, v in sol.model.named_buffers() if "running" in k]


def _run(sol, opt, batches, sched=None, seed0=100):
    for i, b in enumerate(batches):
        random.seed(seed0 + i)
        sol.run_one_epoch([b], "train", opt, collect_views=False)
        if sched is not None:
            sched.step()


# ------------------------------------------------------------------------------------------------ 4. the model's eager step
@pytest.mark.parametrize("optim", ["lars", "lamb"])
def test_model_eager_steps_vs_oracle(optim):
    """Three eager steps with SOLVER.weight_decay = 1e-2 and the biases and BatchNorm affine parameters exempt from the decay and from the
    ratio (lars: with Nesterov).  Every step's gradients, cloned before opt.step(), go through the oracle on the CPU."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedLAMB, FusedLARS
    ops.h2_rebase()       # (clamps of an earlier test are not this test's first step's)
    ops.h2_skipped()
    cfg, sol, opt = _solver(optim, False)
    assert type(opt) is {"lars": FusedLARS, "lamb": FusedLAMB}[optim]
    sol.model.train()
    lossf = build_loss(cfg)
    named = list(sol.model.named_parameters())
    params = [p for _, p in named]
    p0 = [p.detach().cpu().clone() for p in params]
    steps = []
    for i, b in enumerate(_batches(3)):
        b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}
        random.seed(100 + i)
        o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
        lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
        steps.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in params])
        opt.step()
        opt.zero_grad()
    assert ops.h2_skipped() == 0
    live = [i for i, g in enumerate(steps[0]) if g is not None]
    dead = [i for i, g in enumerate(steps[0]) if g is None]
    assert dead and len(live) + len(dead) == 53
    fl = opt._flat[0]
    assert fl["seg_end"].numel() == len(live) and int(fl["seg_end"][-1]) == fl["p"].numel() == sum(params[i].numel() for i in live)
    # the oracle over the live tensors in flat order
    rule = "lars-nesterov" if optim == "lars" else "lamb"
    hyper = dict(gscale=1.0, lr=_LR[optim], wd=WD)
    sizes = [params[i].numel() for i in live]
    ends = np.cumsum(sizes).tolist()
    flags = [0.0 if params[i].dim() == 1 else 1.0 for i in live]
    flat0 = _cat([p0[i] for i in live])
    grads = [_cat([st[i] for i in live]) for st in steps]
    want, q_want = _restate(rule, flat0, grads, ends, flags, flags, torch.float64, **hyper)
    f32, _ = _restate(rule, flat0, grads, ends, flags, flags, torch.float32, **hyper)
    keys = ("momentum_buffer",) if optim == "lars" else ("exp_avg", "exp_avg_sq")
    got_all = [_cat([params[i] for i in live])] + [_cat([opt.state[params[i]][k] for i in live]) for k in keys]
    ratios = opt.trust_ratios()
    assert list(ratios) == [named[i][0] for i in live]
    q = list(ratios.values())
    begs = [0] + ends[:-1]

    def pick(sel, what):
        idx = torch.cat([torch.arange(begs[j], ends[j]) for j in sel])
        cut = lambda ts: [t[idx] for t in ts]      # noqa: E731
        bar = rel(f32[0][idx].double() - flat0[idx].double(), want[0][idx] - flat0[idx].double())
        _check(cut(got_all), [q[j] for j in sel], cut(want), [q_want[j] for j in sel], bar, flat0[idx], f"model, {optim}, {what}")

    pick(list(range(len(live))), "all live tensors")
    exempt = [j for j, f in enumerate(flags) if not f]
    adapted = [j for j, f in enumerate(flags) if f]
    assert exempt and adapted and all(q[j] == 1.0 for j in exempt)
    pick(exempt, "exempt tensors")
    pick(adapted, "adapted tensors")
    for i in dead:      # parameters without a gradient are untouched
        assert torch.equal(params[i].detach().cpu(), p0[i]), named[i][0]


# ------------------------------------------------------------------------------------------------ 5. graphed == eager
@pytest.mark.parametrize("optim,clip", [("lars", 0.0), ("lamb", 0.25)], ids=["lars", "lamb-clip"])
def test_trust_graphed_equals_eager(optim, clip):
    """Four steps with a MultiStepLR milestone crossed after step 2 and trust_coef changed after step 3: the replayed step equals the
    eager one bit for bit (parameters, optimiser state, ratio table, stats, BatchNorm statistics); the new rate re-captures nothing, the
    new coefficient does."""
    from torch.optim.lr_scheduler import MultiStepLR
    batches = _batches(4)
    out = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(optim, graph, clip=clip)
        sched = MultiStepLR(opt, [2], gamma=0.1)
        _run(sol, opt, batches[:1], sched)
        st = slot = None
        if graph:
            st = sol._graph_stepper
            assert st is not None and len(st.slots) == 1
            slot = next(iter(st.slots.values()))
        _run(sol, opt, batches[1:3], sched, seed0=101)
        three = _state(sol, opt, optim)
        if graph:
            assert len(st.slots) == 1 and next(iter(st.slots.values())) is slot      # no re-capture for the new rate
            assert st.lr == pytest.approx(_LR[optim] * 0.1)
        opt.param_groups[0]["trust_coef"] = 5e-3
        _run(sol, opt, batches[3:], sched, seed0=103)
        if graph:
            assert len(st.slots) == 1 and next(iter(st.slots.values())) is not slot  # the captured scalar changed: a new capture
            assert st.opt_flat is opt._flat[0] and "seg_end" in st.opt_flat
        fl = opt._flat[0]
        assert fl["trust_stats"].tolist()[2:] == [4.0, 0.0] and float(fl["ratio"].min()) != float(fl["ratio"].max())
        # the Solver's read-back at the end of the epoch: the ratio table by name, (min, max) over the adapted tensors, steps skipped
        assert sol.last_trust_ratios == opt.trust_ratios() and len(sol.last_trust_ratios) == fl["ratio"].numel()
        assert sol.last_trust_stats == tuple(fl["trust_stats"].tolist()[:2]) + (0,)
        out[graph] = (three, _state(sol, opt, optim))
    for k in (0, 1):
        for a, b in zip(out[False][k], out[True][k]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. checkpoint
def test_trust_checkpoint_round_trip_graphed(tmp_path):
    """Graphed lamb with the average on: two steps, CheckPointer.save, load into a fresh Solver + FusedLAMB, two more steps == four
    uninterrupted steps, bit for bit."""
    from electrocardio_panorama_amd.utils import CheckPointer
    batches = _batches(4, seed0=60)
    extra = ("ema", "ema_n")
    _, sol_a, opt_a = _solver("lamb", True, ema=0.9)
    _run(sol_a, opt_a, batches)
    _, sol_b, opt_b = _solver("lamb", True, ema=0.9)
    _run(sol_b, opt_b, batches[:2])
    CheckPointer(sol_b.model, opt_b, None, str(tmp_path)).save("mid")
    _, sol_c, opt_c = _solver("lamb", True, ema=0.9)
    CheckPointer(sol_c.model, opt_c, None, str(tmp_path)).load()
    g = opt_c.param_groups[0]
    assert g["weight_decay"] == WD and g["trust_coef"] == 1e-3 and opt_c.trust_exempt == tuple(NO_DECAY)
    _run(sol_c, opt_c, batches[2:], seed0=102)
    assert sol_c._graph_stepper is not None and "seg_end" in opt_c._flat[0]
    assert float(opt_c._flat[0]["step"].item()) == 4.0 and float(opt_c._flat[0]["ema_n"].item()) == 4.0
    sa, sc = _state(sol_a, opt_a, "lamb", extra), _state(sol_c, opt_c, "lamb", extra)
    ts = 1 + len(_SLOTS["lamb"]) + 1      # trust_stats: its counters are THIS optimiser instance's steps, 4 against 2
    for i, (a, b) in enumerate(zip(sa, sc)):
        if i == ts:
            assert a.tolist()[:2] == b.tolist()[:2] and a.tolist()[2:] == [4.0, 0.0] and b.tolist()[2:] == [2.0, 0.0]
        else:
            assert torch.equal(a, b)
    assert "ema" in torch.load(str(tmp_path / "mid.pkl"), map_location="cpu")


# ------------------------------------------------------------------------------------------------ 7. defaults
@pytest.mark.parametrize("optim", ["sgd", "adam"])
def test_sgd_and_adam_issue_the_launches_they_issued(optim, monkeypatch):
    """A config without the new keys: the step's update launch is nef_sgd_momentum / nef_adam (the `hbm` tags of ops.PROFILE) and no
    update_l* one; SOLVER.optim lars / lamb issue exactly one update_lars / update_lamb."""
    from electrocardio_panorama_amd import ops
    batch = _batches(1)
    old = {"sgd": "sgd_momentum", "adam": "adam"}[optim]
    new = {"sgd": "lars", "adam": "lamb"}[optim]
    for name, bare, want in ((optim, True, old), (new, False, "update_" + new)):
        _, sol, opt = _solver(name, False, bare=bare)
        prof = []
        monkeypatch.setattr(ops, "PROFILE", prof)
        _run(sol, opt, batch)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "PROFILE", None)
        tags = [t[1] for t, _, _ in prof if isinstance(t, tuple) and t[0] == "hbm"]
        assert tags.count(want) == 1 and not any(t.startswith("update_") for t in tags if t != want), tags
        assert ("seg_end" in opt._flat[0]) == (not bare) and hasattr(opt, "trust_ratios") == (not bare)
