"""The per-update learning-rate schedule on the device (SOLVER.warmup_updates / lr_shape): the nef_lr_sched kernel alone against the host
fp64 restatement lr_factor (which test_sched_cpu.py pins to torch's schedulers); the five fused optimisers consuming exactly the
scheduled rate, counting updates (not micro-batches) and standing still on a skipped step; off is off; and the Solver: graphed against
eager bit for bit with a per-epoch MultiStep drop in between, no host write of the rate between replays, checkpoint and resume."""
import random

import numpy as np
import pytest
import torch

from test_model_gpu import DEV, make_cfg

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23          # one fp32 ulp, relative: both sides round an fp64 result once, the device's cos / pow may differ in the last fp64 bits
BASE = 0.1
T_GUARD, LR_GUARD = -(2 ** 40) - 5, -77.25


def _f32(x):
    return float(np.float32(x))


def _host(t, base, **kw):
    """fp32 rounding of the host fp64 value base * m(t)."""
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    return _f32(base * lr_factor(t, **kw))


def _within_ulp(got, want):
    return abs(got - want) <= ULP * abs(want)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
class _Words:
    """n independent (t, rate) word pairs, each between guard words: [guard, word, guard] triples in one int64 and one fp32 buffer."""

    def __init__(self, n):
        self.n = n
        self.t = torch.full((3 * n,), T_GUARD, device=DEV, dtype=torch.int64)
        self.lr = torch.full((3 * n,), LR_GUARD, device=DEV, dtype=torch.float32)

    def set(self, i, t, lr=-1.0):
        self.t[3 * i + 1] = t
        self.lr[3 * i + 1] = lr

    def words(self, i):
        return self.t[3 * i + 1:3 * i + 2], self.lr[3 * i + 1:3 * i + 2]

    def read(self):
        """(t values, rate values) -- after checking that every guard word is intact."""
        t, lr = self.t.cpu().view(self.n, 3), self.lr.cpu().view(self.n, 3)
        assert bool((t[:, [0, 2]] == T_GUARD).all()) and bool((lr[:, [0, 2]] == LR_GUARD).all())
        return t[:, 1].tolist(), lr[:, 1].tolist()


KERNEL_T = lambda W, N: sorted({0, 1, W - 1, W, W + 1, N - 1, N, N + 5} - {-1})      # noqa: E731


@pytest.mark.parametrize("shape", ["const", "cosine", "poly"])
def test_kernel_against_the_host_restatement(shape):
    """One launch per t: t in {0, 1, W-1, W, W+1, N-1, N, N+5} for W = 4, N = 12, p in {0.5, 1, 2}, f in {0, 0.1, 1}, s in {0, 0.01, 1},
    plus W = 0 and N = W.  t > 0 is reached by an advancing launch from t - 1 (so the count is checked too), t = 0 by an evaluation."""
    from electrocardio_panorama_amd import ops
    cases = []
    for W, N in ((4, 12), (0, 12), (4, 4)):
        for p in (0.5, 1.0, 2.0):
            for f in (0.0, 0.1, 1.0):
                for s in (0.0, 0.01, 1.0):
                    for t in KERNEL_T(W, N):
                        cases.append(dict(t=t, kw=dict(warmup_updates=W, warmup_start=s, total_updates=N, lr_floor=f, poly_power=p)))
    words = _Words(len(cases))
    base_dev = torch.tensor([BASE], device=DEV, dtype=torch.float64)
    for i, c in enumerate(cases):
        words.set(i, max(c["t"] - 1, 0))
    for i, c in enumerate(cases):
        tw, lw = words.words(i)
        # the base rate as a device word and as a scalar, alternating: the same bits either way
        ops.lr_sched(tw, lw, base_dev if i % 2 else BASE, shape, advance=c["t"] > 0, **c["kw"])
    ts, lrs = words.read()
    worst = 0.0
    for c, t, lr in zip(cases, ts, lrs):
        want = _host(c["t"], BASE, lr_shape=shape, **c["kw"])
        assert t == c["t"], c
        assert _within_ulp(lr, want), (c, lr, want)
        if want:
            worst = max(worst, abs(lr - want) / abs(want) / ULP)
    print(f"nef_lr_sched {shape}: {len(cases)} launches, worst distance {worst:.3f} fp32 ulp (bar 1)")
    # const, W = 0: the word equals the base exactly, at every t
    if shape == "const":
        exact = [lr for c, lr in zip(cases, lrs) if c["kw"]["warmup_updates"] == 0]
        assert len(exact) == 27 * len(KERNEL_T(0, 12)) and all(lr == _f32(BASE) for lr in exact)


def test_kernel_skip_flag_advance_and_a_large_count():
    from electrocardio_panorama_amd import ops
    kw = dict(warmup_updates=4, warmup_start=0.01, total_updates=12, lr_floor=0.1, poly_power=2.0)
    pos, zero = torch.tensor([2.0], device=DEV), torch.zeros(1, device=DEV)
    runs = [dict(skip=pos), dict(flag=pos), dict(skip=pos, flag=pos), dict(skip=zero, flag=pos), dict(skip=pos, flag=zero),   # 0-4: not applied
            dict(skip=zero), dict(flag=zero), dict(skip=zero, flag=zero), dict(),                                          # 5-8: applied
            dict(advance=False), dict(advance=False, skip=pos, flag=pos),                                                   # 9-10: re-evaluation
            dict(t0=2 ** 24 + 1), dict(t0=2 ** 40), dict(t0=2 ** 24 + 1, advance=False)]                                    # 11-13
    words = _Words(len(runs))
    for i, r in enumerate(runs):
        words.set(i, r.get("t0", 6), lr=-3.5)
        tw, lw = words.words(i)
        ops.lr_sched(tw, lw, BASE, "cosine", advance=r.get("advance", True), skip=r.get("skip"), flag=r.get("flag"), **kw)
    ts, lrs = words.read()
    for i in range(5):                 # a positive skip word or trust flag: the count and the word keep their bits
        assert ts[i] == 6 and lrs[i] == -3.5, i
    for i in range(5, 9):
        assert ts[i] == 7 and lrs[i] == lrs[8] and _within_ulp(lrs[i], _host(7, BASE, lr_shape="cosine", **kw)), i
    for i in (9, 10):                  # advance = 0 never moves t (and reads neither word)
        assert ts[i] == 6 and _within_ulp(lrs[i], _host(6, BASE, lr_shape="cosine", **kw)), i
    assert lrs[9] != lrs[8]
    # an int64 count: a float one would stop at 2^24
    assert ts[11] == 2 ** 24 + 2 and ts[12] == 2 ** 40 + 1 and ts[13] == 2 ** 24 + 1
    assert lrs[11] == lrs[12] == lrs[13] == _host(2 ** 30, BASE, lr_shape="cosine", **kw) == _f32(BASE * 0.1)
    # every launch is tagged for ops.PROFILE
    ops.PROFILE = []
    try:
        tw, lw = words.words(0)
        ops.lr_sched(tw, lw, BASE, "poly", **kw)
        ops.lr_sched(tw, lw, BASE, "poly", advance=False, **kw)
        assert [t for t, _, _ in ops.PROFILE] == [("lr_sched", "advance"), ("lr_sched", "evaluate")]
    finally:
        ops.PROFILE = None
    with pytest.raises(ValueError):
        ops.lr_sched(tw, lw, BASE, "none", **kw)


# ------------------------------------------------------------------------------------------------ 2. the optimisers
SIZES = (1030, 7, 4096)
NAMES = ("a.weight", "a.bias", "b.weight")
EXTRAS = dict(max_grad_norm=1.0, ema_decay=0.9, no_decay=("*.bias",))
OPTIMS = ["sgd", "adam", "adamw", "lars", "lamb"]


def _sched(W=3, N=8, shape="cosine", **kw):
    from electrocardio_panorama_amd.solver.optim_scheduler import LrSchedule
    return LrSchedule(warmup_updates=W, lr_shape=shape, total_updates=N, **kw)


def _make(name, **kw):
    """A few small tensors, as test_accum_gpu.py builds them."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.solver import optim_scheduler as osch
    ops.h2_rebase()      # no model runs here: clamps an earlier test left uncharged must not taint (skip) this test's first step
    gen = torch.Generator().manual_seed(5)
    params = []
    for k, n in zip(NAMES, SIZES):
        p = torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV))
        p._nef_name = k
        params.append(p)
    cls, args = {"sgd": (osch.FusedSGD, dict(lr=0.1, weight_decay=0.01)), "adam": (osch.FusedAdam, dict(lr=1e-3, weight_decay=0.01)),
                 "adamw": (osch.FusedAdamW, dict(lr=1e-3)), "lars": (osch.FusedLARS, dict(lr=0.1, weight_decay=0.01, trust_exempt=("*.bias",))),
                 "lamb": (osch.FusedLAMB, dict(lr=1e-3, weight_decay=0.01, trust_exempt=("*.bias",)))}[name]
    return params, cls(params, **{**args, **kw})


def _grad_sets(n, seed=70):
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(k, generator=gen).to(DEV) for k in SIZES] for _ in range(n)]


def _set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad = g.clone()


def _everything(opt):
    """Parameters, every state slot, the average, clip_stats and the ratio table of the one built group."""
    fl = opt._flat[0]
    keys = [k for k in ("p", "buf", "m", "v", "step", "ema", "ema_n", "ratio", "trust_stats") if k in fl]
    out = {k: fl[k].clone() for k in keys}
    if opt.clip_stats is not None:
        out["clip_stats"] = opt.clip_stats.clone()
    return out


def _rate_word(opt, params):
    """The float in the optimiser's rate word in front of its next update (the flat buffers and the words are made if they are not
    there yet: the step that follows reuses them)."""
    opt._current(0, params)
    return opt.lr_state()


def _same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", OPTIMS)
def test_update_consumes_exactly_the_scheduled_rate(name):
    """8 updates, W = 3, N = 8, cosine: parameters and state bit for bit those of a second optimiser with the schedule off whose
    group["lr"] the host sets, before every update, to the float read back from the first one's rate word."""
    sets = _grad_sets(8)
    sc = _sched(lr_floor=0.1)
    pa, a = _make(name, lr_schedule=sc, **EXTRAS)
    pb, b = _make(name, **EXTRAS)
    base = a.param_groups[0]["lr"]
    rates = []
    for i, gs in enumerate(sets):
        _set_grads(pa, gs)
        t, lr = _rate_word(a, pa)
        assert t == i and _within_ulp(lr, _f32(base * sc.factor(i))), (i, lr)
        assert a.param_groups[0]["lr"] == base          # the base rate is the host's, untouched
        rates.append(lr)
        a.step()
        b.param_groups[0]["lr"] = lr
        _set_grads(pb, gs)
        b.step()
        _same(_everything(a), _everything(b), (name, i))
    assert len(set(rates)) == 8 and rates[3] == _f32(base)
    t, lr = a.lr_state()
    assert t == 8 and lr == _f32(base * 0.1)
    assert a._sched[0]["t"].dtype == torch.int64 and a._sched[0]["lr"].dtype == torch.float32
    # the host changes the base rate (a per-epoch scheduler): re-evaluated without advancing, and the next update uses it
    a.param_groups[0]["lr"] = base * 0.5
    assert a.lr_state() == (8, _f32(base * 0.5 * 0.1))
    _set_grads(pa, sets[0]), _set_grads(pb, sets[0])
    b.param_groups[0]["lr"] = a.lr_state()[1]
    a.step(), b.step()
    _same(_everything(a), _everything(b), (name, "new base"))
    assert a.lr_state()[0] == 9


@pytest.mark.parametrize("name", OPTIMS)
def test_counts_updates_not_micro_batches(name):
    sets = _grad_sets(8)
    sc = _sched()
    pa, a = _make(name, lr_schedule=sc, accum_steps=2, **EXTRAS)
    for i, gs in enumerate(sets):
        _set_grads(pa, gs)
        a.step()
        assert a.lr_state()[0] == (i + 1) // 2
    t, lr = a.lr_state()
    assert t == 4 and _within_ulp(lr, _f32(a.param_groups[0]["lr"] * sc.factor(4)))
    # flush() on an incomplete window is an update too
    _set_grads(pa, sets[0])
    a.step()
    assert a.lr_state()[0] == 4
    a.flush()
    assert a.lr_state()[0] == 5


@pytest.mark.parametrize("name", OPTIMS)
def test_tainted_step_moves_nothing(name):
    """A clamp counted in front of the step (what a clamping split-fp16 launch does): t, the rate, parameters and state are untouched, and
    the next clean step uses the rate the skipped one would have used."""
    from electrocardio_panorama_amd import ops
    sets = _grad_sets(4, seed=74)
    sc = _sched()
    pa, a = _make(name, lr_schedule=sc, **EXTRAS)
    pb, b = _make(name, **EXTRAS)
    for gs in sets[:2]:
        _set_grads(pa, gs)
        rate = _rate_word(a, pa)[1]
        a.step()
        b.param_groups[0]["lr"] = rate
        _set_grads(pb, gs)
        b.step()
    st = ops._amax_state(pa[0].device)
    ops.h2_clamped(), ops.h2_skipped()                              # (reset the host's marks)
    before, (t0, lr0) = _everything(a), a.lr_state()
    assert t0 == 2
    st["clamped"] += 1
    _set_grads(pa, sets[2])
    a.step()
    assert ops.h2_skipped() == 1 and ops.h2_clamped() == 1
    after = _everything(a)
    # (the clip launch in front still measures: its norm and coefficient words are this call's, its two counters stay)
    assert torch.equal(after.pop("clip_stats")[2:], before.pop("clip_stats")[2:])
    _same(after, before, name)
    assert a.lr_state() == (t0, lr0)
    # the clean step behind it: the reference takes the rate of update 2
    _set_grads(pa, sets[3])
    a.step()
    b.param_groups[0]["lr"] = lr0
    _set_grads(pb, sets[3])
    b.step()
    _same(_everything(a), _everything(b), name)
    assert a.lr_state()[0] == 3 and a.lr_state()[1] != lr0 and ops.h2_skipped() == 0


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_non_finite_trust_norms_move_nothing(name):
    """No clipping in front: an infinite gradient reaches the trust norms, whose flag skips the update -- and the schedule."""
    sets = _grad_sets(2, seed=75)
    pa, a = _make(name, lr_schedule=_sched())
    _set_grads(pa, sets[0])
    a.step()
    before, state = _everything(a), a.lr_state()
    assert state[0] == 1
    _set_grads(pa, sets[1])
    pa[0].grad[3] = float("inf")
    a.step()
    after = _everything(a)
    assert after.pop("trust_stats").tolist()[3] == 1.0 and before.pop("trust_stats").tolist()[3] == 0.0
    _same(after, before, name)
    assert a.lr_state() == state
    _set_grads(pa, sets[1])
    a.step()
    assert a.lr_state()[0] == 2
    from electrocardio_panorama_amd import ops
    assert ops.h2_skipped() == 1                                    # (the skipped step is counted once; reading resets the host's mark)


def test_off_is_off():
    """With the defaults there is no lr_sched launch among ops' per-launch tags, no word, and the bits are those of an optimiser built
    without the keyword; W = 2 shows the tag once per update (and once when the words are made)."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.solver.optim_scheduler import LrSchedule
    sets = _grad_sets(3, seed=76)
    states, tags, opts = [], [], []
    for kw in ({}, dict(lr_schedule=None), dict(lr_schedule=LrSchedule()), dict(lr_schedule=LrSchedule(warmup_updates=2))):
        params, opt = _make("sgd", **kw, **EXTRAS)
        ops.PROFILE = []
        try:
            for gs in sets:
                _set_grads(params, gs)
                opt.step()
            tags.append([t for t, _, _ in ops.PROFILE])
        finally:
            ops.PROFILE = None
        states.append(_everything(opt))
        opts.append(opt)
    for i in (0, 1, 2):
        assert not any(t[0] == "lr_sched" for t in tags[i]) and tags[i] == tags[0]
        assert opts[i]._sched == {} and opts[i].lr_state() == (None, 0.1)
        _same(states[i], states[0])
    assert [t for t in tags[3] if t[0] == "lr_sched"] == [("lr_sched", "evaluate")] + [("lr_sched", "advance")] * 3
    assert [t for t in tags[3] if t[0] != "lr_sched"] == tags[0]              # and nothing else changed in what is launched
    assert not torch.equal(states[3]["p"], states[0]["p"])


# ------------------------------------------------------------------------------------------------ 3. the Solver
V, B, L = 3, 2, 512
_LR = {"sgd": 0.1, "lamb": 1e-3}
_SLOTS = {"sgd": ("buf",), "lamb": ("m", "v", "step", "ratio")}


def _batches(n=6, seed0=40):
    from electrocardio_panorama_amd import synth
    return [synth.make_batch(B, V, L, seed=seed0 + s, Q=2) for s in range(n)]


def _solver(optim, graph, out_dir=None, **solver_keys):
    """A Solver on seeded default weights with W = 2, N = 6, cosine, and a per-epoch MultiStep milestone behind the first epoch."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_lr_scheduler, get_optimizer
    ops.h2_rebase()      # (clamps of an earlier test are not this test's first step's)
    cfg = make_cfg(V, lr=_LR[optim])
    cfg.SOLVER.update(optim=optim, graph=bool(graph), lr_step=[1], warmup_updates=2, lr_shape="cosine", total_updates=6, lr_floor=0.1)
    cfg.SOLVER.update(solver_keys)
    if out_dir is not None:
        cfg["output_dir"] = str(out_dir)
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.dropout_p = 0.0
    opt = get_optimizer(cfg, sol.model.parameters())
    return cfg, sol, opt, get_lr_scheduler(cfg, opt)


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return ([fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + [opt._sched[0]["t"].clone(), opt._sched[0]["lr"].clone()] +
            [v.clone() for k, v in sol.model.named_buffers()])


def _epoch(sol, opt, batches, seed):
    random.seed(seed)
    sol.run_one_epoch(batches, "train", opt, collect_views=False)


@pytest.mark.parametrize("optim", ["sgd", "lamb"])
def test_graphed_equals_eager_and_nothing_writes_the_rate_between_replays(optim, monkeypatch):
    """Six batches, one per run_one_epoch call, the per-epoch MultiStep milestone crossed behind the third: parameters, optimiser state,
    t, the rate word and the BatchNorm buffers bit for bit.  The rate is base * m(t) before and behind the drop, t is undisturbed by it,
    and the graphed run neither re-captures nor issues a host write (fill_) or an lr_sched launch of its own between replays."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.solver.optim_scheduler import ScheduledLR
    batches = _batches()
    fills = []
    real_fill = torch.Tensor.fill_

    def counting_fill(self, *a, **k):
        fills.append((tuple(self.shape), self.dtype))
        return real_fill(self, *a, **k)

    out = {}
    for graph in (False, True):
        cfg, sol, opt, sch = _solver(optim, graph)
        assert type(sch) is ScheduledLR and opt.lr_schedule.total_updates == 6
        snaps, rates, tags = [], [], []
        for i, b in enumerate(batches):
            base = opt.param_groups[0]["lr"]
            watch = i not in (0, 3)                     # (0: build and capture; 3: the first step behind the per-epoch drop)
            if watch:
                ops.PROFILE = []
                monkeypatch.setattr(torch.Tensor, "fill_", counting_fill)
            try:
                _epoch(sol, opt, [b], 100 + i)
                if watch:
                    tags += [t for t, _, _ in ops.PROFILE if t[0] == "lr_sched"]
            finally:
                ops.PROFILE = None
                monkeypatch.setattr(torch.Tensor, "fill_", real_fill)
            t, lr = opt.lr_state()
            assert t == i + 1 and _within_ulp(lr, _f32(base * opt.lr_schedule.factor(i + 1))), (i, lr)
            assert opt.param_groups[0]["lr"] == base and sol.last_lr[1] == lr and sol.last_lr_updates == t
            assert _within_ulp(sol.last_lr[0], _f32(base * opt.lr_schedule.factor(i)))
            rates.append(lr)
            snaps.append(_state(sol, opt, optim))
            if i == 2:
                sch.step()                              # the per-epoch scheduler: the base rate drops tenfold
                assert opt.param_groups[0]["lr"] == pytest.approx(_LR[optim] * 0.1)
                # re-evaluated without advancing: the new base times m(t), t where it was
                assert opt.lr_state()[0] == 3 and _within_ulp(opt.lr_state()[1], _f32(opt.param_groups[0]["lr"] * opt.lr_schedule.factor(3)))
                assert opt.lr_state()[1] < 0.2 * rates[-1]
                assert sch.get_last_lr() == [opt.lr_state()[1]]
        assert len(set(rates)) == 6                     # the rate word changes from step to step while group["lr"] does not
        st = getattr(sol, "_graph_stepper", None)
        assert (st is not None) == graph
        one_word_fills = [f for f in fills if f[0] in ((1,), ()) and f[1].is_floating_point]
        if graph:
            assert len(st.slots) == 1 and st.calls == 6             # the drop re-captured nothing
            assert tags == [] and one_word_fills == []              # the launch is inside the replayed graph; no host write of a rate
        else:
            assert tags == [("lr_sched", "advance")] * 4 and one_word_fills == []
        fills.clear()
        out[graph] = snaps
    for i, (sa, sb) in enumerate(zip(out[False], out[True])):
        for a, b in zip(sa, sb):
            assert torch.equal(a, b), i
    assert not torch.equal(out[True][0][0], out[True][5][0])


@pytest.mark.parametrize("optim", ["sgd", "lamb"])
def test_checkpoint_and_resume_graphed(optim, tmp_path, capsys):
    """Checkpoint behind batch 3 (CheckPointer: model, optimiser, the scheduler entry with the count), a fresh Solver resuming from it:
    the remaining batches end bit-identical to the uninterrupted run.  An entry written with the schedule off loads with t = 0."""
    from electrocardio_panorama_amd.utils import CheckPointer
    batches = _batches(seed0=60)
    _, sol_a, opt_a, sch_a = _solver(optim, True)
    _epoch(sol_a, opt_a, batches[:3], 100)
    sch_a.step()
    _epoch(sol_a, opt_a, batches[3:], 101)
    _, sol_b, opt_b, sch_b = _solver(optim, True)
    _epoch(sol_b, opt_b, batches[:3], 100)
    sch_b.step()
    CheckPointer(sol_b.model, opt_b, sch_b, str(tmp_path)).save("mid")
    saved = torch.load(str(tmp_path / "mid.pkl"), map_location="cpu")["scheduler"]
    assert saved["per_update"]["t"] == 3 and saved["per_update"]["lr_shape"] == "cosine" and saved["last_epoch"] == 1
    _, sol_c, opt_c, sch_c = _solver(optim, True)
    capsys.readouterr()
    CheckPointer(sol_c.model, opt_c, sch_c, str(tmp_path)).load()
    assert capsys.readouterr().out == ""
    # the count waits for the flat buffers; the rate it implies is already the host's answer
    assert opt_c._sched == {} and opt_c.lr_state()[0] == 3 and _within_ulp(opt_c.lr_state()[1], opt_b.lr_state()[1])
    assert opt_c.param_groups[0]["lr"] == pytest.approx(_LR[optim] * 0.1) and sch_c.last_epoch == 1
    _epoch(sol_c, opt_c, batches[3:], 101)
    assert sol_c._graph_stepper is not None and opt_c.lr_state() == opt_a.lr_state() and opt_a.lr_state()[0] == 6
    for i, (a, c) in enumerate(zip(_state(sol_a, opt_a, optim), _state(sol_c, opt_c, optim))):
        assert torch.equal(a, c), i
    # a scheduler entry without a count (the schedule was off when it was written): t = 0, one line says so
    data = torch.load(str(tmp_path / "mid.pkl"), map_location="cpu")
    del data["scheduler"]["per_update"]
    torch.save(data, str(tmp_path / "mid.pkl"))
    CheckPointer(sol_c.model, opt_c, sch_c, str(tmp_path)).load()
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and "t = 0" in line
    assert opt_c.lr_state()[0] == 0


def test_solver_train_derives_total_updates_and_reports_the_rate(tmp_path, capsys):
    """SOLVER.total_updates 0: epochs * ceil(len(dl_train) / accum_steps), set before the first step; the epoch message and the train_lr
    scalar carry the effective rate."""
    cfg, sol, _, _ = _solver("sgd", True, out_dir=tmp_path, total_updates=0, epochs=2, accum_steps=2, lr_step=[50])
    batches = _batches(3)
    random.seed(100)
    scalars = []
    sol.summary_writer = type("W", (), {"add_scalar": lambda self, tag, v, global_step=None: scalars.append((tag, v, global_step))})()
    sol.train(batches)
    opt = sol._graph_stepper.optimizer
    assert opt.lr_schedule.total_updates == 4                       # 2 epochs * ceil(3 / 2) updates
    t, lr = opt.lr_state()
    assert t == 4 and lr == _f32(0.1 * 0.1)                         # the end value: lr_floor times the base rate
    assert sol.last_lr == (_f32(0.1 * opt.lr_schedule.factor(2)), lr) and sol.last_lr_updates == 4
    assert [(tag, step) for tag, _, step in scalars if tag == "train_lr"] == [("train_lr", 0), ("train_lr", 1)]
    assert [v for tag, v, _ in scalars if tag == "train_lr"][1] == lr
    out = capsys.readouterr().out
    assert out.count("\nlr: ") == 2 and "4 updates applied so far" in out
