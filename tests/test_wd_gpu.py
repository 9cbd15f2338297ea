"""Weight decay on the device: the nef_update kernel (SGD with L2 decay / Nesterov, Adam with L2 decay, AdamW, a decay multiplier per
run of elements) against torch.optim on the CPU, its bit boundaries with nef_sgd_momentum / nef_adam, the skip word, FusedSGD /
FusedAdamW with `no_decay` against torch with two parameter groups, the model's eager step, graph replay against the eager path, and
a checkpoint in the middle of a graphed run.

Bars (the project's own): state buffers rel-L2 <= 1e-6; Adam / AdamW parameter displacement p - p0 <= 1e-5
(test_adam_kernel_vs_torch); SGD parameters and displacement <= 1e-6 (test_sgd_momentum).  The build contracts nothing; an fp32
restatement of these updates with EVERY multiply-add contracted sits at <= 7e-8 (momentum), <= 1e-7 (SGD displacement), 5e-8 (v) and
1.2e-6 (AdamW displacement) from torch.optim on the kernel tests' inputs, so the bars hold whatever a CPU build of torch contracts."""
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
RULES = {      # rule -> (kind, nesterov, lr, weight_decay)
    "sgd": ("sgd", False, 0.1, 0.05),
    "sgd-nesterov": ("sgd", True, 0.1, 0.05),
    "adam-L2": ("adam", False, 1e-3, 0.01),
    "adamw": ("adamw", False, 1e-3, 0.01),
}
# one-element runs at the start and in the middle, run ends inside a 16-byte vector (1, 6, 1030, 1031) and on a vector boundary (2048),
# a fractional multiplier
TABLE = ([1, 6, 1030, 1031, 2048, 4099], [1.0, 0.0, 1.0, 0.0, 0.5, 1.0])
NO_DECAY = ["*.bias", "decoder.*.double_conv.[14].weight"]      # the model's biases and BatchNorm affine parameters: its 1-D tensors


def _grads(n, steps, seed):      # the recipe of tests/test_adam_gpu.py
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0          # exact zeros (dead units)
        out.append(g)
    return out


def _table(n):
    """TABLE clipped at n."""
    ends, muls = [], []
    for e, m in zip(*TABLE):
        ends.append(min(e, n))
        muls.append(m)
        if e >= n:
            break
    assert ends[-1] == n
    return ends, muls


def _dev_table(ends, muls):
    return torch.tensor(ends, device=DEV, dtype=torch.int64), torch.tensor(muls, device=DEV, dtype=torch.float32)


def _torch_steps(rule, p0, grads, ends, muls, gscale=GSCALE):
    """torch.optim on the CPU (foreach=False) over the same tensors split per run into parameter groups with weight_decay * mul.
    Returns the flat parameters and state buffers."""
    kind, nesterov, lr, wd = RULES[rule]
    begs = [0] + list(ends[:-1])
    segs = [torch.nn.Parameter(p0[b:e].clone()) for b, e in zip(begs, ends)]
    groups = [dict(params=[s], weight_decay=wd * m) for s, m in zip(segs, muls)]
    if kind == "sgd":
        opt = torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=nesterov, foreach=False)
        keys = ("momentum_buffer",)
    else:
        opt = (torch.optim.Adam if kind == "adam" else torch.optim.AdamW)(groups, lr=lr, foreach=False)
        keys = ("exp_avg", "exp_avg_sq")
    for g in grads:
        gs = g * gscale
        for s, b, e in zip(segs, begs, ends):
            s.grad = gs[b:e].clone()
        opt.step()
    return [torch.cat([s.detach() for s in segs])] + [torch.cat([opt.state[s][k] for s in segs]) for k in keys]


def _inputs(n, steps):
    gen = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=gen), _grads(n, steps, n + 1)


@functools.lru_cache(maxsize=None)
def _reference(rule, n, steps):
    """Computed once per (rule, n): the aligned and the unaligned case share it."""
    p0, grads = _inputs(n, steps)
    return _torch_steps(rule, p0, grads, *_table(n))


def _kernel_steps(rule, p0, grads, runs, off, gscale=GSCALE):
    """ops.update_sgd / ops.update_adam over buffers that start `off` floats behind a 16-byte boundary."""
    from electrocardio_panorama_amd import ops
    kind, nesterov, lr, wd = RULES[rule]
    n = p0.numel()
    bufs = [torch.zeros(n + off, device=DEV) for _ in range(4)]
    p, g_dev, s0, s1 = (b[off:] for b in bufs)
    p.copy_(p0)
    step = torch.zeros(1, device=DEV)
    for g in grads:
        g_dev.copy_(g)
        if kind == "sgd":
            ops.update_sgd(p, g_dev, s0, lr, 0.9, gscale, wd, nesterov, runs=runs)
        else:
            ops.update_adam(p, g_dev, s0, s1, step, lr, 0.9, 0.999, 1e-8, wd, gscale, decoupled=kind == "adamw", runs=runs)
    torch.cuda.synchronize()
    assert kind == "sgd" or float(step.item()) == len(grads)
    return [p.cpu(), s0.cpu()] + ([] if kind == "sgd" else [s1.cpu()])


def _check(rule, got, want, p0, what=""):
    """The bars of the module docstring; every figure is printed before it is asserted."""
    kind = RULES[rule][0]
    e_state = [rel(a, b) for a, b in zip(got[1:], want[1:])]
    e_disp = rel(got[0] - p0, want[0] - p0)
    e_p = rel(got[0], want[0])
    print(f"{what}{rule}: state {e_state}, displacement {e_disp:.3e}, parameters {e_p:.3e}")
    assert all(e <= 1e-6 for e in e_state), e_state
    if kind == "sgd":
        assert e_p <= 1e-6 and e_disp <= 1e-6, (e_p, e_disp)
    else:
        assert e_disp <= 1e-5, e_disp


# ------------------------------------------------------------------------------------------------ 1. the kernel against torch
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("n", [1000, 4099])
def test_update_kernel_vs_torch(n, rule, off):
    """Five steps with gscale = 0.5 and 10 % exact zeros in the gradients, under the run table TABLE (clipped at n)."""
    p0, grads = _inputs(n, 5)
    want = _reference(rule, n, 5)
    got = _kernel_steps(rule, p0, grads, _dev_table(*_table(n)), off)
    _check(rule, got, want, p0)
    if n == 4099:      # the table matters: without it (about half of the elements decayed otherwise) the result is far outside the bars
        assert rel(_kernel_steps(rule, p0, grads, None, off)[0] - p0, want[0] - p0) > 1e-4


@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_update_kernel_grid_stride(rule):
    """n just above one pass of the capped grid's 16-byte body (4096 blocks x 256 lanes x 4 elements): one step; a run end 5 elements
    behind the pass boundary and a zero-multiplier run across it."""
    one_pass = 4 * 256 * 4096
    n = one_pass + 4099
    ends, muls = [1000, one_pass - 3, one_pass + 5, n], [1.0, 0.5, 0.0, 1.0]
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen)
    grads = _grads(n, 1, 8)
    want = _torch_steps(rule, p0, grads, ends, muls)
    got = _kernel_steps(rule, p0, grads, _dev_table(ends, muls), 0)
    _check(rule, got, want, p0, "grid-stride ")
    # ... and element by element around the boundary: the exempt run moved by the undecayed rule, its neighbours did not
    lo, hi = one_pass - 8, one_pass + 12
    assert rel(got[0][lo:hi] - p0[lo:hi], want[0][lo:hi] - p0[lo:hi]) <= 1e-5
    free = _torch_steps(rule, p0[lo:hi], [grads[0][lo:hi]], [hi - lo], [0.0])
    a, b = one_pass - 3 - lo, one_pass + 5 - lo
    assert rel(got[0][lo:hi][a:b] - p0[lo:hi][a:b], free[0][a:b] - p0[lo:hi][a:b]) <= 1e-5
    assert rel(got[0][lo:hi][:a] - p0[lo:hi][:a], free[0][:a] - p0[lo:hi][:a]) > 1e-4


# ------------------------------------------------------------------------------------------------ 2. bit boundaries
def _four(n, off, seed):
    gen = torch.Generator().manual_seed(seed)
    bufs = [torch.zeros(n + off, device=DEV) for _ in range(4)]
    views = [b[off:] for b in bufs]
    views[0].copy_(torch.randn(n, generator=gen))
    return views


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
def test_update_with_nothing_new_is_the_old_entries_bit_for_bit(off):
    from electrocardio_panorama_amd import ops
    n = 4099
    grads = [g.to(DEV) for g in _grads(n, 3, 21)]
    # SGD
    (pa, ga, ba, _), (pb, gb, bb, _) = _four(n, off, 20), _four(n, off, 20)
    for g in grads:
        ga.copy_(g), gb.copy_(g)
        ops.sgd_momentum(pa, ga, ba, 0.1, 0.9, GSCALE, False)
        ops.update_sgd(pb, gb, bb, 0.1, 0.9, GSCALE)
    assert torch.equal(pa, pb) and torch.equal(ba, bb) and not torch.equal(pa, _four(n, off, 20)[0])
    # Adam, without decay and with the scalar L2 decay nef_adam already had
    for wd in (0.0, 0.01):
        (pa, ga, ma, va), (pb, gb, mb, vb) = _four(n, off, 22), _four(n, off, 22)
        sa, sb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        for g in grads:
            ga.copy_(g), gb.copy_(g)
            ops.adam(pa, ga, ma, va, sa, 1e-3, 0.9, 0.999, 1e-8, wd, GSCALE)
            ops.update_adam(pb, gb, mb, vb, sb, 1e-3, 0.9, 0.999, 1e-8, wd, GSCALE)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(sa, sb)
        assert float(sb.item()) == 3.0


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("rule", list(RULES))
def test_all_multipliers_zero_is_decay_zero_bit_for_bit(rule, off):
    from electrocardio_panorama_amd import ops
    kind, nesterov, lr, wd = RULES[rule]
    n = 4099
    grads = [g.to(DEV) for g in _grads(n, 3, 31)]
    ends, _ = _table(n)
    zero = _dev_table(ends, [0.0] * len(ends))
    out = []
    for decay, runs in ((wd, zero), (0.0, None)):
        p, g_dev, s0, s1 = _four(n, off, 30)
        step = torch.zeros(1, device=DEV)
        for g in grads:
            g_dev.copy_(g)
            if kind == "sgd":
                ops.update_sgd(p, g_dev, s0, lr, 0.9, GSCALE, decay, nesterov, runs=runs)
            else:
                ops.update_adam(p, g_dev, s0, s1, step, lr, 0.9, 0.999, 1e-8, decay, GSCALE, decoupled=kind == "adamw", runs=runs)
        out.append((p, s0, s1, step))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. skip word and lr_dev
@pytest.mark.parametrize("rule", ["sgd-nesterov", "adam-L2", "adamw"])
def test_update_skip_word_and_lr_dev(rule):
    """tests/test_adam_gpu.py::test_adam_skip_word_and_lr_dev for the three rules, with decay and a table: a skipped step leaves the
    parameters bit-identical -- the (decoupled) decay is skipped too -- and the state and the step word as they are."""
    from electrocardio_panorama_amd import ops
    kind, nesterov, lr, wd = RULES[rule]
    n = 4099
    runs = _dev_table(*_table(n))
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=gen).to(DEV)
    s0, s1, step = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
    g1, g2 = (g.to(DEV) for g in _grads(n, 2, 4))

    def upd(t, g, lr, **kw):
        if kind == "sgd":
            ops.update_sgd(t[0], g, t[1], lr, 0.9, 1.0, wd, nesterov, runs=runs, **kw)
        else:
            ops.update_adam(t[0], g, t[1], t[2], t[3], lr, 0.9, 0.999, 1e-8, wd, 1.0, decoupled=kind == "adamw", runs=runs, **kw)

    state = (p, s0, s1, step)
    upd(state, g1, lr)
    ops.h2_skipped()                                         # (reset the host's mark)
    before = [t.clone() for t in state]
    upd(state, g2, lr, skip=torch.ones(1, device=DEV))
    for a, b in zip(state, before):
        assert torch.equal(a, b)
    assert ops.h2_skipped() == 1
    # a zero skip word steps; lr_dev replaces lr (in AdamW's decay factor as well)
    a = [t.clone() for t in before]
    b = [t.clone() for t in before]
    upd(a, g2, lr, skip=torch.zeros(1, device=DEV), lr_dev=torch.full((1,), 5 * lr, device=DEV))
    upd(b, g2, 5 * lr)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], before[0]) and float(a[3].item()) == (0.0 if kind == "sgd" else 2.0)
    assert ops.h2_skipped() == 0


# ------------------------------------------------------------------------------------------------ 4. the optimisers
_NAMED = (("a.bias", (1,)), ("b.weight", (3,)), ("c.bias", (128,)), ("d.weight", (64, 3)), ("e.weight", (130,)))


def _named_params(dev):
    gen = torch.Generator().manual_seed(50)
    out = []
    for name, shape in _NAMED:
        p = torch.nn.Parameter(torch.randn(*shape, generator=gen).to(dev))
        p._nef_name = name
        out.append(p)
    return out


def _two_groups(params, wd):
    decay = [p for (name, _), p in zip(_NAMED, params) if not name.endswith(".bias")]
    exempt = [p for (name, _), p in zip(_NAMED, params) if name.endswith(".bias")]
    return [dict(params=decay, weight_decay=wd), dict(params=exempt, weight_decay=0.0)]


def _split_group(sd, wd):
    """A fused optimiser's state dict (one group, torch's format) as the two-group dict of _two_groups."""
    sd = copy.deepcopy(sd)
    g, = sd["param_groups"]
    idx = {True: [i for i, (name, _) in enumerate(_NAMED) if name.endswith(".bias")],
           False: [i for i, (name, _) in enumerate(_NAMED) if not name.endswith(".bias")]}
    sd["param_groups"] = [dict(g, params=idx[False], weight_decay=wd), dict(g, params=idx[True], weight_decay=0.0)]
    return sd


def _cat(ts):
    return torch.cat([torch.as_tensor(t).detach().reshape(-1).cpu() for t in ts])


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fused_optimisers_with_no_decay_vs_torch_two_groups(kind):
    """FusedSGD(weight_decay=0.05, nesterov=True) / FusedAdamW over named tensors of sizes [1], [3], [128], [64, 3], [130] with
    no_decay=['*.bias']: five steps against torch with two parameter groups; then the state dict goes into torch optimisers (one group:
    the format; two groups: the reference) and back, and every side takes one more step that agrees."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdamW, FusedSGD
    # no model runs here: clamps an earlier test's split-fp16 launches left uncharged must not taint (skip) this test's first step
    ops.h2_rebase()
    ops.h2_skipped()
    wd = 0.05
    if kind == "sgd":
        rule, keys = "sgd-nesterov", ("momentum_buffer",)
        fused = lambda ps: FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=wd, nesterov=True, no_decay=["*.bias"])      # noqa: E731
        torch_opt = lambda groups: torch.optim.SGD(groups, lr=0.1, momentum=0.9, weight_decay=wd, nesterov=True, foreach=False)      # noqa: E731
    else:
        rule, keys = "adamw", ("exp_avg", "exp_avg_sq")
        fused = lambda ps: FusedAdamW(ps, lr=1e-3, weight_decay=wd, no_decay=["*.bias"])      # noqa: E731
        torch_opt = lambda groups: torch.optim.AdamW(groups, lr=1e-3, weight_decay=wd, foreach=False)      # noqa: E731
    params, shadow = _named_params(DEV), _named_params("cpu")
    p0 = _cat(shadow)
    opt, ropt = fused(params), torch_opt(_two_groups(shadow, wd))
    n = p0.numel()
    grads = _grads(n, 6, 51)

    def step(o, ps, g):
        off = 0
        for p in ps:
            p.grad = g[off:off + p.numel()].view_as(p).clone().to(p.device)
            off += p.numel()
        o.step()

    for g in grads[:5]:
        step(opt, params, g)
        step(ropt, shadow, g)
    assert ops.h2_skipped() == 0
    fl = opt._flat[0]
    assert fl["run_end"].tolist() == [1, 4, 132, n] and fl["run_mul"].tolist() == [0.0, 1.0, 0.0, 1.0]
    got = lambda o, ps: [_cat(ps)] + [_cat([o.state[p][k] for p in ps]) for k in keys]      # noqa: E731
    _check(rule, got(opt, params), got(ropt, shadow), p0, "5 steps, ")
    # the state dict in torch's format: a one-group torch optimiser loads it, and a fresh fused optimiser loads that one's
    sd = copy.deepcopy(opt.state_dict())
    assert "no_decay" not in sd["param_groups"][0]
    plain = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    t1 = torch_opt(plain)
    t1.load_state_dict(sd)
    for p, q in zip(params, plain):
        for k in keys:
            assert torch.equal(t1.state[q][k], opt.state[p][k].cpu())
        if kind != "sgd":
            assert float(t1.state[q]["step"]) == 5.0
    params2 = _named_params(DEV)
    for p, q in zip(params2, params):
        p.data.copy_(q.data)
    opt2 = fused(params2)
    opt2.load_state_dict(copy.deepcopy(t1.state_dict()))
    # ... and the two-group torch optimiser, over the fused parameters as they are now, loads it as well
    shadow2 = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    ropt2 = torch_opt(_two_groups(shadow2, wd))
    ropt2.load_state_dict(_split_group(sd, wd))
    p5 = _cat(params)
    step(opt, params, grads[5])
    step(opt2, params2, grads[5])
    step(ropt2, shadow2, grads[5])
    for a, b in zip(got(opt, params), got(opt2, params2)):
        assert torch.equal(a, b)                            # the round trip through torch's optimiser lost nothing
    _check(rule, got(opt, params), got(ropt2, shadow2), p5, "round trip + 1 step, ")


# ------------------------------------------------------------------------------------------------ Solver-level helpers
V, B, L = 3, 2, 512
WD = 1e-2
_LR = {"sgd": 0.1, "adam": 1e-3, "adamw": 1e-3}
_SLOTS = {"sgd": ("buf",), "adam": ("m", "v", "step"), "adamw": ("m", "v", "step")}


def _solver(optim, graph, wd=WD, no_decay=NO_DECAY, clip=0.0, bare=False):
    """`bare`: a config written before the keys existed."""
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr=_LR[optim])
    cfg.SOLVER["optim"] = optim
    cfg.SOLVER["graph"] = bool(graph)
    if not bare:
        cfg.SOLVER["weight_decay"] = wd
        cfg.SOLVER["nesterov"] = optim == "sgd"
        cfg.SOLVER["no_decay"] = list(no_decay)
        cfg.SOLVER["clip_grad_norm"] = clip
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


def _batches(n, seed0=40):
    from electrocardio_panorama_amd import synth
    return [synth.make_batch(B, V, L, seed=seed0 + i, Q=2) for i in range(n)]


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + \
        [v.clone() for k, v in sol.model.named_buffers() if "running" in k]


def _run(sol, opt, batches, sched=None, seed0=100):
    for i, b in enumerate(batches):
        random.seed(seed0 + i)
        sol.run_one_epoch([b], "train", opt, collect_views=False)
        if sched is not None:
            sched.step()


# ------------------------------------------------------------------------------------------------ 5. the model's eager step
@pytest.mark.parametrize("optim", ["sgd", "adamw"])
def test_model_eager_steps_vs_torch(optim):
    """Three eager steps with SOLVER.weight_decay = 1e-2 and the biases and BatchNorm affine parameters exempt (sgd: with Nesterov).  Every
    step's gradients, cloned before opt.step(), go through torch's optimiser on the CPU over cloned parameters in two groups (the scheme
    of tests/test_dp_adam_gpu.py: same gradients in, torch's update out)."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdamW, FusedSGD
    ops.h2_rebase()       # (clamps of an earlier test are not this test's first step's)
    ops.h2_skipped()
    cfg, sol, opt = _solver(optim, False)
    assert type(opt) is {"sgd": FusedSGD, "adamw": FusedAdamW}[optim]
    sol.model.train()
    lossf = build_loss(cfg)
    named = list(sol.model.named_parameters())
    params = [p for _, p in named]
    p0 = [p.detach().cpu().clone() for p in params]
    shadow = [torch.nn.Parameter(p.clone()) for p in p0]
    groups = [dict(params=[s for s in shadow if s.dim() > 1], weight_decay=WD),
              dict(params=[s for s in shadow if s.dim() == 1], weight_decay=0.0)]
    if optim == "sgd":
        ropt, keys, rule = torch.optim.SGD(groups, lr=0.1, momentum=0.9, nesterov=True, foreach=False), ("momentum_buffer",), "sgd-nesterov"
    else:
        ropt, keys, rule = torch.optim.AdamW(groups, lr=1e-3, foreach=False), ("exp_avg", "exp_avg_sq"), "adamw"
    for i, b in enumerate(_batches(3)):
        b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}
        random.seed(100 + i)
        o = sol.model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
        lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
        for p, s in zip(params, shadow):
            s.grad = None if p.grad is None else p.grad.detach().cpu().clone()
        opt.step()
        opt.zero_grad()
        ropt.step()
    assert ops.h2_skipped() == 0
    live = [i for i, s in enumerate(shadow) if s.grad is not None]
    dead = [i for i, s in enumerate(shadow) if s.grad is None]
    assert dead and len(live) + len(dead) == 53
    fl = opt._flat[0]
    assert "run_end" in fl and int(fl["run_end"][-1]) == fl["p"].numel() == sum(params[i].numel() for i in live)

    def both(idx):
        got = [_cat([params[i] for i in idx])] + [_cat([opt.state[params[i]][k] for i in idx]) for k in keys]
        want = [_cat([shadow[i] for i in idx])] + [_cat([ropt.state[shadow[i]][k] for i in idx]) for k in keys]
        return got, want, _cat([p0[i] for i in idx])

    _check(rule, *both(live), "model, all live tensors, ")
    # the exempt tensors alone moved by the weight_decay = 0 rule (torch's second group), the others by the decayed one
    exempt = [i for i in live if params[i].dim() == 1]
    assert exempt and len(exempt) < len(live)
    _check(rule, *both(exempt), "model, exempt tensors, ")
    _check(rule, *both([i for i in live if params[i].dim() > 1]), "model, decayed tensors, ")
    # parameters without a gradient are not decayed, as in torch
    for i in dead:
        assert torch.equal(params[i].detach().cpu(), p0[i]), named[i][0]
    msg = opt.decay_summary()
    assert "exempt: " in msg and named[exempt[0]][0] in msg


# ------------------------------------------------------------------------------------------------ 6. graphed == eager
@pytest.mark.parametrize("optim,clip", [("sgd", 0.0), ("adam", 0.0), ("adamw", 0.25)], ids=["sgd-nesterov", "adam-L2", "adamw-clip"])
def test_wd_graphed_equals_eager(optim, clip):
    """Four steps with a MultiStepLR milestone crossed after step 2 and weight_decay changed after step 3: the replayed step equals the
    eager one bit for bit (parameters, optimiser state, BatchNorm statistics); the new rate re-captures nothing, the new decay does."""
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
        opt.param_groups[0]["weight_decay"] = 5 * WD
        _run(sol, opt, batches[3:], sched, seed0=103)
        if graph:
            assert len(st.slots) == 1 and next(iter(st.slots.values())) is not slot  # the captured scalar changed: a new capture
            assert st.opt_flat is opt._flat[0] and "run_end" in st.opt_flat
        out[graph] = (three, _state(sol, opt, optim))
    for k in (0, 1):
        for a, b in zip(out[False][k], out[True][k]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. checkpoint
def test_wd_checkpoint_round_trip_graphed(tmp_path):
    """Graphed adamw with decay and exempt tensors: two steps, CheckPointer.save, load into a fresh Solver + FusedAdamW, two more steps
    == four uninterrupted steps, bit for bit."""
    from electrocardio_panorama_amd.utils import CheckPointer
    batches = _batches(4, seed0=60)
    _, sol_a, opt_a = _solver("adamw", True)
    _run(sol_a, opt_a, batches)
    _, sol_b, opt_b = _solver("adamw", True)
    _run(sol_b, opt_b, batches[:2])
    CheckPointer(sol_b.model, opt_b, None, str(tmp_path)).save("mid")
    _, sol_c, opt_c = _solver("adamw", True)
    CheckPointer(sol_c.model, opt_c, None, str(tmp_path)).load()
    g = opt_c.param_groups[0]
    assert g["weight_decay"] == WD and g["decoupled_weight_decay"] is True and opt_c.no_decay == tuple(NO_DECAY)
    _run(sol_c, opt_c, batches[2:], seed0=102)
    assert sol_c._graph_stepper is not None and "run_end" in opt_c._flat[0]
    assert float(opt_c._flat[0]["step"].item()) == 4.0
    for a, b in zip(_state(sol_a, opt_a, "adamw"), _state(sol_c, opt_c, "adamw")):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 8. defaults
@pytest.mark.parametrize("optim", ["sgd", "adam"])
def test_defaults_issue_the_launches_they_issued(optim, monkeypatch):
    """A config without the new keys: the step's update launch is nef_sgd_momentum / nef_adam (the `hbm` tags of ops.PROFILE) and none
    of the new ones; with decay on it is the new entry's."""
    from electrocardio_panorama_amd import ops
    batch = _batches(1)
    old = {"sgd": "sgd_momentum", "adam": "adam"}[optim]
    new = {"sgd": "update_sgd", "adam": "update_adam"}[optim]
    for bare, want, never in ((True, old, new), (False, new, old)):
        _, sol, opt = _solver(optim, False, bare=bare)
        prof = []
        monkeypatch.setattr(ops, "PROFILE", prof)
        _run(sol, opt, batch)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "PROFILE", None)
        tags = [t[1] for t, _, _ in prof if isinstance(t, tuple) and t[0] == "hbm"]
        assert tags.count(want) == 1 and never not in tags and not any(t.startswith("update_") for t in tags if t != want), tags
        assert ("run_end" in opt._flat[0]) == (not bare)
