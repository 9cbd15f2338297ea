"""The EMA of the weights on the device: the nef_update_ema kernel against nef_update (bit for bit on p, state and *step) and against the
fp64 recurrence over its own parameters, the skip word, FusedSGD / FusedAdamW with SOLVER.ema_decay in the eager and the graphed step, a
checkpoint in the middle of a graphed run, the ema_weights() context and the Solver's evaluation on the averaged weights.

The bar on the average (every element): t * 3 * 2^-24 * M after t steps, M = max |p| over the trajectory (the start included: e_0 = p_0).
One step computes fmaf(w, p - e, e) in fp32 with the same w = (float)(1.0 - d_t) as the recurrence: one rounding of p - e, whose magnitude
is at most 2M (an error of at most 2M * 2^-24, carried on with |w| <= 1), one rounding of the result, at most M (M * 2^-24); the errors of
earlier steps are carried with the factor 1 - w <= 1."""
import functools
import random

import numpy as np
import pytest
import torch

from test_model_gpu import DEV, make_cfg
from test_wd_gpu import B, GSCALE, L, NO_DECAY, RULES, V, WD, _LR, _SLOTS, _batches, _dev_table, _grads, _run, _table

pytestmark = pytest.mark.gpu

EMA_CASES = [(0.9, False), (0.9, True), (0.999, False), (0.999, True)]      # (decay, warm-up)


def _decay_at(decay, warmup, t):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def _recurrence(p0, traj, decay, warmup):
    """The fp64 recurrence over the kernel's own fp32 parameters after each step, with the kernel's fp32 weight."""
    e = p0.astype(np.float64)
    for t, p in enumerate(traj):
        w = float(np.float32(1.0 - _decay_at(decay, warmup, t)))
        e = e + w * (p.astype(np.float64) - e)
    return e


def _bound(p0, traj):
    return len(traj) * 3 * 2.0 ** -24 * max(float(np.abs(p).max()) for p in [p0] + list(traj))


def _check_ema(ema, p0, traj, decay, warmup, what=""):
    want, bar = _recurrence(p0, traj, decay, warmup), _bound(p0, traj)
    err = float(np.abs(ema.astype(np.float64) - want).max())
    print(f"{what}decay {decay} warm-up {warmup}: max |ema - recurrence| {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    return want


def _call(rule, t, g, runs, gscale=GSCALE, lr=None, ema=None, **kw):
    """One ops.update_* call of `rule` over t = (p, s0, s1, step)."""
    from electrocardio_panorama_amd import ops
    kind, nesterov, lr0, wd = RULES[rule]
    lr = lr0 if lr is None else lr
    if kind == "sgd":
        ops.update_sgd(t[0], g, t[1], lr, 0.9, gscale, wd, nesterov, runs=runs, ema=ema, **kw)
    else:
        ops.update_adam(t[0], g, t[1], t[2], t[3], lr, 0.9, 0.999, 1e-8, wd, gscale, decoupled=kind == "adamw", runs=runs, ema=ema, **kw)


def _views(n, off, k):
    """k zeroed fp32 device buffers of n elements that start `off` floats behind a 16-byte boundary."""
    return [torch.zeros(n + off, device=DEV)[off:] for _ in range(k)]


def _kernel_vs_plain(rule, p0, grads, runs, off, decay, warmup, what=""):
    """`len(grads)` steps of nef_update_ema next to nef_update on cloned inputs: p, the state buffers and *step bit-identical, the count
    right, the average inside the bar of the module docstring."""
    n = p0.numel()
    pa, ga, s0a, s1a, ema = _views(n, off, 5)
    pb, gb, s0b, s1b = _views(n, off, 4)
    stepa, stepb, ema_n = (torch.zeros(1, device=DEV) for _ in range(3))
    pa.copy_(p0), pb.copy_(p0), ema.copy_(p0)
    traj = []
    for g in grads:
        ga.copy_(g), gb.copy_(g)
        _call(rule, (pa, s0a, s1a, stepa), ga, runs, ema=(ema, ema_n, decay, warmup))
        _call(rule, (pb, s0b, s1b, stepb), gb, runs)
        traj.append(pa.cpu().numpy())
    for a, b in ((pa, pb), (s0a, s0b), (s1a, s1b), (stepa, stepb)):
        assert torch.equal(a, b)
    assert float(ema_n.item()) == len(grads)
    assert float(stepa.item()) == (0.0 if RULES[rule][0] == "sgd" else len(grads))
    e = ema.cpu().numpy()
    _check_ema(e, p0.numpy(), traj, decay, warmup, what)
    assert not np.array_equal(e, traj[-1]) and not np.array_equal(e, p0.numpy())       # an average, neither end


@functools.lru_cache(maxsize=None)
def _inputs(n, steps):
    gen = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=gen), _grads(n, steps, n + 1)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("table", [True, False], ids=["table", "no-table"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("rule", ["sgd-nesterov", "adam-L2", "adamw"])
@pytest.mark.parametrize("n", [1000, 4099])
def test_update_ema_kernel(n, rule, off, table):
    """Five steps (gscale 0.5, 10 % exact zeros in the gradients) for decay 0.9 / 0.999, warm-up off / on: the 16-byte body with its
    n % 4 tail (aligned) and the scalar path (one float off), with and without the decay run table."""
    p0, grads = _inputs(n, 5)
    runs = _dev_table(*_table(n)) if table else None
    for decay, warmup in EMA_CASES:
        _kernel_vs_plain(rule, p0, grads, runs, off, decay, warmup)


# ------------------------------------------------------------------------------------------------ 2. grid stride
@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_update_ema_kernel_grid_stride(rule):
    """The n of test_wd_gpu.py::test_update_kernel_grid_stride -- just above one pass of the capped grid's 16-byte body -- and its table:
    one step, warm-up on (the first weight is 1 - 1/10)."""
    one_pass = 4 * 256 * 4096
    n = one_pass + 4099
    ends, muls = [1000, one_pass - 3, one_pass + 5, n], [1.0, 0.5, 0.0, 1.0]
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen)
    _kernel_vs_plain(rule, p0, _grads(n, 1, 8), _dev_table(ends, muls), 0, 0.999, True, "grid-stride ")


# ------------------------------------------------------------------------------------------------ 3. skip word and lr_dev
@pytest.mark.parametrize("rule", ["sgd-nesterov", "adam-L2", "adamw"])
def test_update_ema_skip_word_and_lr_dev(rule):
    """A positive skip word leaves p, the state, the average and its count bit-identical and counts the step; a zero word with lr_dev
    steps at the device's rate."""
    from electrocardio_panorama_amd import ops
    n = 4099
    runs = _dev_table(*_table(n))
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=gen).to(DEV)
    s0, s1, step, ema_n = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ema = p.clone()
    g1, g2 = (g.to(DEV) for g in _grads(n, 2, 4))
    lr = RULES[rule][2]
    state = (p, s0, s1, step, ema, ema_n)

    def upd(t, g, lr, **kw):
        _call(rule, t[:4], g, runs, gscale=1.0, lr=lr, ema=(t[4], t[5], 0.9, True), **kw)

    upd(state, g1, lr)
    ops.h2_skipped()                                         # (reset the host's mark)
    before = [t.clone() for t in state]
    assert float(ema_n.item()) == 1.0 and not torch.equal(ema, p)
    upd(state, g2, lr, skip=torch.ones(1, device=DEV))
    for a, b in zip(state, before):
        assert torch.equal(a, b)
    assert ops.h2_skipped() == 1
    a = [t.clone() for t in before]
    b = [t.clone() for t in before]
    upd(a, g2, lr, skip=torch.zeros(1, device=DEV), lr_dev=torch.full((1,), 5 * lr, device=DEV))
    upd(b, g2, 5 * lr)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], before[0]) and not torch.equal(a[4], before[4]) and float(a[5].item()) == 2.0
    assert float(a[3].item()) == (0.0 if RULES[rule][0] == "sgd" else 2.0)
    assert ops.h2_skipped() == 0


# ------------------------------------------------------------------------------------------------ Solver-level helpers
EMA = 0.9


def _solver(optim, graph, ema=EMA, warmup=True, bare=False, out=None, ema_eval=None, lr=None):
    """tests/test_wd_gpu.py::_solver with the EMA keys (decay and exempt tensors stay on: the run table and the average share one launch).
    `bare`: a config written before any of the keys existed."""
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr=_LR[optim] if lr is None else lr)
    cfg.SOLVER["optim"] = optim
    cfg.SOLVER["graph"] = bool(graph)
    if not bare:
        cfg.SOLVER["weight_decay"] = WD
        cfg.SOLVER["nesterov"] = optim == "sgd"
        cfg.SOLVER["no_decay"] = list(NO_DECAY)
        cfg.SOLVER["ema_decay"] = ema
        cfg.SOLVER["ema_warmup"] = warmup
    if ema_eval is not None:
        cfg.SOLVER["ema_eval"] = ema_eval
    if out is not None:
        cfg["output_dir"] = str(out)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim] + ("ema", "ema_n")] + \
        [v.clone() for k, v in sol.model.named_buffers() if "running" in k]


# ------------------------------------------------------------------------------------------------ 4. graphed == eager
@pytest.mark.parametrize("optim", ["sgd", "adamw"])
def test_ema_graphed_equals_eager(optim):
    """Four steps with a MultiStepLR milestone crossed after step 2 and ema_decay changed after step 3: the replayed step equals the eager
    one bit for bit (parameters, optimiser state, BatchNorm statistics, the average and its count); the new rate re-captures nothing, the
    new decay does."""
    from torch.optim.lr_scheduler import MultiStepLR
    batches = _batches(4)
    out = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(optim, graph)
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
        opt.ema_decay = 0.5
        _run(sol, opt, batches[3:], sched, seed0=103)
        if graph:
            assert len(st.slots) == 1 and next(iter(st.slots.values())) is not slot  # the captured scalar changed: a new capture
            assert st.opt_flat is opt._flat[0] and "ema" in st.opt_flat
        fl = opt._flat[0]
        assert float(fl["ema_n"].item()) == 4.0 and not torch.equal(fl["ema"], fl["p"])
        out[graph] = (three, _state(sol, opt, optim))
    for k in (0, 1):
        for a, b in zip(out[False][k], out[True][k]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. checkpoint
@pytest.mark.parametrize("optim", ["sgd", "adamw"])
def test_ema_checkpoint_round_trip_graphed(optim, tmp_path):
    """Graphed: two steps, CheckPointer.save, load into a fresh Solver + optimiser, two more steps == four uninterrupted steps, bit for
    bit, the average and its count included.  The file's ema['model'] loads like its 'model'; its optimiser entry is torch's."""
    from electrocardio_panorama_amd.utils import CheckPointer
    batches = _batches(4, seed0=60)
    _, sol_a, opt_a = _solver(optim, True)
    _run(sol_a, opt_a, batches)
    _, sol_b, opt_b = _solver(optim, True)
    _run(sol_b, opt_b, batches[:2])
    CheckPointer(sol_b.model, opt_b, None, str(tmp_path)).save("mid")
    ema_b = opt_b._flat[0]["ema"].clone()
    _, sol_c, opt_c = _solver(optim, True)
    CheckPointer(sol_c.model, opt_c, None, str(tmp_path)).load()
    _run(sol_c, opt_c, batches[2:], seed0=102)
    assert sol_c._graph_stepper is not None and float(opt_c._flat[0]["ema_n"].item()) == 4.0
    for a, b in zip(_state(sol_a, opt_a, optim), _state(sol_c, opt_c, optim)):
        assert torch.equal(a, b)
    # the file
    ckpt = torch.load(str(tmp_path / "mid.pkl"), map_location="cpu")
    ema = ckpt["ema"]
    assert set(ema) == {"decay", "warmup", "n_averaged", "model"}
    assert ema["decay"] == EMA and ema["warmup"] is True and ema["n_averaged"] == 2.0
    assert list(ema["model"]) == list(sol_b.model.state_dict()) == list(ckpt["model"])
    _, sol_d, _ = _solver(optim, False)
    sol_d.model.load_state_dict(ema["model"], strict=True)
    got = torch.cat([dict(sol_d.model.named_parameters())[p._nef_name].detach().reshape(-1) for p in opt_b._flat[0]["params"]])
    assert torch.equal(got, ema_b)                                       # the covered parameters hold the average ...
    covered = {p._nef_name for p in opt_b._flat[0]["params"]}
    others = [k for k in ckpt["model"] if k not in covered]
    assert others and all(torch.equal(ema["model"][k], ckpt["model"][k]) for k in others)       # ... every other entry the live tensor
    assert any(not torch.equal(ema["model"][k], ckpt["model"][k]) for k in covered)
    plain = [torch.nn.Parameter(p.detach().cpu().clone()) for p in sol_b.model.parameters()]
    topt = torch.optim.SGD(plain, lr=0.1, momentum=0.9) if optim == "sgd" else torch.optim.AdamW(plain)
    topt.load_state_dict(ckpt["optimizer"])
    # ... and CheckPointer.load(ema=True) puts the averaged weights into the model
    _, sol_e, _ = _solver(optim, False)
    CheckPointer(sol_e.model, None, None, str(tmp_path)).load(ema=True)
    for k, v in sol_e.model.state_dict().items():
        assert torch.equal(v.cpu(), ema["model"][k]), k


# ------------------------------------------------------------------------------------------------ 6. ema_weights()
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_ema_weights_context(graph):
    """Inside, every live parameter equals its average bit for bit; after it, both are restored bit for bit; a train step taken
    afterwards (an evaluation ran inside the context) equals the step of a twin that never entered it."""
    from electrocardio_panorama_amd import synth
    batches = _batches(3, seed0=70)
    probe = [synth.make_batch(B, V, L, seed=75, Q=6)]
    _, sol, opt = _solver("sgd", graph)
    _, twin, topt = _solver("sgd", graph)
    with opt.ema_weights():                                  # before the first step: nothing to exchange
        pass
    _run(sol, opt, batches[:2])
    _run(twin, topt, batches[:2])
    fl = opt._flat[0]
    p0, e0 = fl["p"].clone(), fl["ema"].clone()
    assert not torch.equal(p0, e0)
    with opt.ema_weights():
        off = 0
        for p in fl["params"]:
            assert torch.equal(p.detach().reshape(-1), e0[off:off + p.numel()])
            off += p.numel()
        assert off == e0.numel() and torch.equal(fl["ema"], p0)
        sol.run_one_epoch(probe, "test", collect_views=False)      # an evaluation on the averaged weights, as Solver.train runs it
    twin.run_one_epoch(probe, "test", collect_views=False)         # (the twin's: on its live weights)
    assert torch.equal(fl["p"], p0) and torch.equal(fl["ema"], e0)
    _run(sol, opt, batches[2:], seed0=102)
    _run(twin, topt, batches[2:], seed0=102)
    for a, b in zip(_state(sol, opt, "sgd"), _state(twin, topt, "sgd")):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. the Solver, end to end
class _Seeded:
    """A loader that seeds Python's `random` (the model's two lead draws per call) whenever an epoch starts."""

    def __init__(self, batches, seed):
        self.batches, self.seed = batches, seed

    def __iter__(self):
        random.seed(self.seed)
        return iter(self.batches)


def test_solver_evaluates_and_saves_the_averaged_weights(tmp_path):
    """One epoch of two batches with a one-batch test loader, ema_decay 0.5: the checkpoint holds `ema`, and its psnr_gen is the
    averaged model's -- Solver.val on it from a fresh Solver lies at least ten times closer to it with ema_eval on than with it off."""
    from electrocardio_panorama_amd import synth
    train = _Seeded(_batches(2, seed0=80), 11)
    test = _Seeded([synth.make_batch(B, V, L, seed=90, Q=6)], 5)
    _, sol, _ = _solver("sgd", False, ema=0.5, warmup=False, out=tmp_path)
    sol.train(train, test)
    ckpt = torch.load(str(tmp_path / "debug" / "epoch_0.pkl"), map_location="cpu")
    assert "ema" in ckpt and ckpt["ema"]["n_averaged"] == 2.0 and ckpt["ema"]["decay"] == 0.5
    assert list(ckpt["ema"]["model"]) == list(ckpt["model"])
    saved = float(ckpt["psnr_gen"])
    vals = {}
    for ema_eval in (True, False):
        _, fresh, _ = _solver("sgd", False, ema=0.5, warmup=False, out=tmp_path, ema_eval=ema_eval)
        vals[ema_eval] = fresh.val(test, epoch=0)[0]
    d_on, d_off = abs(vals[True] - saved), abs(vals[False] - saved)
    print(f"psnr_gen: checkpoint {saved!r}, val with ema_eval {vals[True]!r} (|d| {d_on:.3e}), without {vals[False]!r} (|d| {d_off:.3e})")
    assert d_off > 0 and 10 * d_on <= d_off, (saved, vals)


# ------------------------------------------------------------------------------------------------ 8. defaults
@pytest.mark.parametrize("optim", ["sgd", "adam"])
def test_defaults_issue_the_launches_they_issued(optim, monkeypatch):
    """A config without the keys: the step's update launch is nef_sgd_momentum / nef_adam and no `*_ema` tag, and the flat buffers hold
    no average; with ema_decay on (and nothing else) it is the new entry's, its bytes two streams more."""
    from electrocardio_panorama_amd import ops
    batch = _batches(1)
    old = {"sgd": "sgd_momentum", "adam": "adam"}[optim]
    new = {"sgd": "update_sgd_ema", "adam": "update_adam_ema"}[optim]
    for bare, want, never in ((True, old, new), (False, new, old)):
        cfg, sol, opt = _solver(optim, False, bare=True)
        if not bare:
            opt.ema_decay = 0.99
        prof = []
        monkeypatch.setattr(ops, "PROFILE", prof)
        _run(sol, opt, batch)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "PROFILE", None)
        hbm = [t for t, _, _ in prof if isinstance(t, tuple) and t[0] == "hbm"]
        tags = [t[1] for t in hbm]
        assert tags.count(want) == 1 and never not in tags, tags
        assert any(t.endswith("_ema") for t in tags) == (not bare), tags
        fl = opt._flat[0]
        assert ("ema" in fl) == ("ema_n" in fl) == (not bare)
        streams = {"sgd": 5, "adam": 7}[optim] + (0 if bare else 2)
        assert next(t[2] for t in hbm if t[1] == want) == streams * 4 * fl["p"].numel()
        assert "ema" not in opt.state_dict() and set(opt.state_dict()) == {"state", "param_groups"}
