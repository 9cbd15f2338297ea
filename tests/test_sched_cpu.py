"""CPU: the per-update learning-rate schedule (SOLVER.warmup_updates / lr_shape) -- the host restatement lr_factor pinned to torch's
own schedulers segment by segment, its edge cases, the config validation, the factory with the keys off, the wrapper's state dict and
the nef_lr_sched C-ABI entry's argument checks (no GPU work)."""
import ctypes
import math
import os
import re

import pytest
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, MultiStepLR, PolynomialLR, StepLR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, N, LR = 5, 40, 0.1
# torch's chained forms accumulate one fp64 rounding per step over at most 40 steps
BAR = 1e-12


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _torch_rates(make, steps):
    """group["lr"] of a CPU torch.optim.SGD in front of update 0, 1, ..., steps under the torch scheduler `make(opt)` builds."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR)
    sch = make(opt)
    out = []
    for _ in range(steps + 1):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return out


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("s", [0.01, 0.0, 0.5, 1.0])
def test_warmup_is_linearlr(s):
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    if s == 0.0:       # (LinearLR rejects start_factor 0: its chained form divides by the previous factor; the closed form is checked alone)
        for t in range(W):
            assert lr_factor(t, W, s, "cosine", N) == t / W
        return
    want = _torch_rates(lambda o: LinearLR(o, start_factor=s, end_factor=1.0, total_iters=W), W)
    for shape in ("none", "const", "cosine", "poly"):
        for t in range(W + 1):       # t == W: the warm-up has ended at 1, where every shape starts (x = 0)
            got = LR * lr_factor(t, W, s, shape, N)
            assert _rel(got, want[t]) <= BAR, (shape, t, got, want[t])
    assert lr_factor(0, W, s, "const", N) == s


@pytest.mark.parametrize("f", [0.0, 0.1, 1.0])
def test_cosine_is_cosineannealinglr(f):
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    want = _torch_rates(lambda o: CosineAnnealingLR(o, T_max=N - W, eta_min=f * LR), N - W)
    for t in range(W, N + 1):
        got = LR * lr_factor(t, W, 0.01, "cosine", N, lr_floor=f)
        assert _rel(got, want[t - W]) <= BAR, (t, got, want[t - W])
    assert lr_factor(N, W, 0.01, "cosine", N, lr_floor=f) == pytest.approx(f, abs=1e-16)


@pytest.mark.parametrize("p", [1.0, 2.0])
def test_poly_is_polynomiallr(p):
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    want = _torch_rates(lambda o: PolynomialLR(o, total_iters=N - W, power=p), N - W)
    for t in range(W, N + 1):
        got = LR * lr_factor(t, W, 0.01, "poly", N, lr_floor=0.0, poly_power=p)
        if want[t - W] == 0.0:
            assert got == 0.0
        else:
            assert _rel(got, want[t - W]) <= BAR, (t, got, want[t - W])


def test_every_t_is_covered_and_the_end_value_stays():
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    for shape, end in (("const", 1.0), ("none", 1.0), ("cosine", 0.25), ("poly", 0.25)):
        vals = [lr_factor(t, W, 0.01, shape, N, lr_floor=0.25, poly_power=2.0) for t in range(N + 1)]
        assert all(0.0 <= v <= 1.0 for v in vals)
        assert vals[:W + 1] == sorted(vals[:W + 1]) and vals[W] == 1.0          # the ramp, ending where the shape starts
        assert vals[W:] == sorted(vals[W:], reverse=True)                        # and no shape rises again
        for t in (N, N + 1, N + 5, 10 ** 12):
            assert lr_factor(t, W, 0.01, shape, N, lr_floor=0.25, poly_power=2.0) == pytest.approx(end, abs=1e-16), (shape, t)
    assert lr_factor(-3, W, 0.01, "const", N) == 0.01                            # (a negative count reads as 0)


def test_total_not_behind_the_warmup_and_no_warmup():
    from electrocardio_panorama_amd.solver.optim_scheduler import lr_factor
    # N <= W: nothing divides by zero -- the span counts as 1, so the shape is at its start at t == W and at its end behind it
    for n in (0, 3, W):
        for shape in ("cosine", "poly"):
            assert lr_factor(W - 1, W, 0.5, shape, n, lr_floor=0.1) == 0.5 + 0.5 * (W - 1) / W
            assert lr_factor(W, W, 0.5, shape, n, lr_floor=0.1) == 1.0
            assert lr_factor(W + 1, W, 0.5, shape, n, lr_floor=0.1) == pytest.approx(0.1, abs=1e-16)
        assert lr_factor(W + 1, W, 0.5, "const", n) == 1.0
    # W == 0: no warm-up branch, m(0) is the shape's start
    for shape in ("const", "cosine", "poly"):
        assert lr_factor(0, 0, 0.01, shape, 10) == 1.0
    assert lr_factor(5, 0, 0.01, "cosine", 10) == pytest.approx(0.5, abs=1e-16)
    assert lr_factor(5, 0, 0.01, "poly", 10, poly_power=2.0) == 0.25
    assert lr_factor(0, 0, 0.01, "cosine", 0) == 1.0 and lr_factor(1, 0, 0.01, "cosine", 0) == pytest.approx(0.0, abs=1e-16)
    with pytest.raises(ValueError):
        lr_factor(1, 0, 0.01, "linear", 10)


def _solver_cfg(**kw):
    return Cfg(SOLVER=Cfg(optim="sgd", lr=0.1, scheduler="MultiStep", lr_step=[2, 4], **kw))


def test_config_defaults_are_off():
    from electrocardio_panorama_amd.config import get_defaults
    from electrocardio_panorama_amd.solver.optim_scheduler import LrSchedule
    S = get_defaults().SOLVER
    assert (S.warmup_updates, S.warmup_start, S.lr_shape, S.total_updates, S.lr_floor, S.poly_power) == (0, 0.01, "none", 0, 0.0, 1.0)
    assert not LrSchedule.from_cfg(get_defaults()).on
    cfg = get_defaults()
    cfg.merge_from_list(["SOLVER.warmup_updates", "100", "SOLVER.lr_shape", "cosine"])
    sc = LrSchedule.from_cfg(cfg)
    assert sc.on and sc.warmup_updates == 100 and sc.lr_shape == "cosine"
    # 'none' with a warm-up behaves as 'const'
    sc = LrSchedule(warmup_updates=3)
    assert sc.on and sc.kwargs()["shape"] == "const" and sc.factor(3) == 1.0 and sc.factor(10 ** 6) == 1.0


@pytest.mark.parametrize("bad", [dict(warmup_updates=-1), dict(warmup_updates=1.5), dict(warmup_updates=True), dict(warmup_updates="3"),
                                 dict(total_updates=-1), dict(total_updates=2.0), dict(warmup_start=-0.1), dict(warmup_start=1.1),
                                 dict(warmup_start=float("nan")), dict(lr_floor=-1e-9), dict(lr_floor=1.5), dict(lr_floor=float("nan")),
                                 dict(lr_shape="linear"), dict(lr_shape=None), dict(poly_power=0.0), dict(poly_power=-1.0),
                                 dict(poly_power=float("nan")), dict(poly_power=float("inf"))])
def test_config_validation(bad):
    from electrocardio_panorama_amd.solver.optim_scheduler import LrSchedule, get_lr_scheduler, get_optimizer
    with pytest.raises(ValueError):
        LrSchedule(**bad)
    params = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):          # validated whether the schedule is on or off
        get_optimizer(_solver_cfg(**bad), params)
    with pytest.raises(ValueError):
        get_lr_scheduler(_solver_cfg(**bad), torch.optim.SGD(params, lr=0.1))


@pytest.mark.parametrize("name", ["sgd", "adam", "adamw", "lars", "lamb"])
def test_factory_off_is_what_it_was(name):
    from electrocardio_panorama_amd.solver.optim_scheduler import get_lr_scheduler, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    for extra in ({}, dict(warmup_updates=0, lr_shape="none", total_updates=7, lr_floor=0.5, poly_power=2.0)):
        opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=0.1, **extra)), params)
        assert opt.lr_schedule is None and not opt._sched_on and opt._sched == {}
        assert opt.lr_state() == (None, 0.1)
        assert "lr_schedule" not in opt.state_dict()["param_groups"][0] and "lr_schedule" not in opt.defaults
        sch = get_lr_scheduler(Cfg(SOLVER=Cfg(scheduler="steplr", lr_step=[2], **extra)), opt)
        assert type(sch) is StepLR and sch.step_size == 50 and sch.gamma == 0.1
        sch = get_lr_scheduler(Cfg(SOLVER=Cfg(scheduler="MultiStep", lr_step=[2, 4], **extra)), opt)
        assert type(sch) is MultiStepLR and dict(sch.milestones) == {2: 1, 4: 1}
        # the frozen scalars of a captured update carry nothing new
        assert len(opt._captured_scalars(opt.param_groups[0])) == {"sgd": 5, "adam": 6, "adamw": 6, "lars": 7, "lamb": 8}[name]


@pytest.mark.parametrize("name", ["sgd", "adam", "adamw", "lars", "lamb"])
def test_factory_on(name):
    from electrocardio_panorama_amd.solver.optim_scheduler import LrSchedule, ScheduledLR, get_lr_scheduler, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    keys = dict(warmup_updates=3, lr_shape="cosine", total_updates=8, lr_floor=0.1)
    cfg = Cfg(SOLVER=Cfg(optim=name, lr=0.1, scheduler="MultiStep", lr_step=[1], **keys))
    opt = get_optimizer(cfg, params)
    assert isinstance(opt.lr_schedule, LrSchedule) and opt._sched_on
    # an attribute like max_grad_norm: the state dict keeps torch's format
    assert "lr_schedule" not in opt.state_dict()["param_groups"][0] and "lr_schedule" not in opt.defaults
    base = len(get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=0.1)), params)._captured_scalars(opt.param_groups[0]))
    sc = opt._captured_scalars(opt.param_groups[0])
    assert len(sc) == base + 6 and "cosine" in sc                 # a change of a shape number re-captures
    sch = get_lr_scheduler(cfg, opt)
    assert type(sch) is ScheduledLR and type(sch.inner) is MultiStepLR and sch.last_epoch == 0
    assert opt.lr_state() == (0, float(torch.tensor(0.1 * 0.01, dtype=torch.float64).float()))
    assert sch.get_last_lr() == [opt.lr_state()[1]]
    sch.step()                                                     # the per-epoch scheduler's: the BASE rate drops
    assert opt.param_groups[0]["lr"] == pytest.approx(0.01) and sch.last_epoch == 1
    assert sch.get_last_lr()[0] == pytest.approx(0.01 * 0.01)
    # an optimiser that cannot carry the schedule is refused, not silently left unscheduled
    with pytest.raises(ValueError, match="fused"):
        get_lr_scheduler(cfg, torch.optim.SGD(params, lr=0.1))
    with pytest.raises(ValueError):
        type(opt)(params, lr=0.1, lr_schedule=dict(keys))


def test_wrapper_state_dict_round_trip(capsys):
    from electrocardio_panorama_amd.solver.optim_scheduler import get_lr_scheduler, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    keys = dict(warmup_updates=3, lr_shape="poly", total_updates=8, lr_floor=0.1, poly_power=2.0)
    cfg = Cfg(SOLVER=Cfg(optim="sgd", lr=0.1, scheduler="MultiStep", lr_step=[1, 3], **keys))

    def pair():
        opt = get_optimizer(cfg, params)
        return opt, get_lr_scheduler(cfg, opt)

    a_opt, a = pair()
    a.step(), a.step()
    a_opt.set_lr_updates(5)                          # no flat buffers yet: the count waits for them
    sd = a.state_dict()
    assert sd["per_update"] == dict(t=5, warmup_updates=3, warmup_start=0.01, lr_shape="poly", total_updates=8, lr_floor=0.1,
                                    poly_power=2.0)
    assert sd["last_epoch"] == 2 and "milestones" in sd            # the inner scheduler's own entries, in place
    b_opt, b = pair()
    b_opt.load_state_dict(a_opt.state_dict())
    b.load_state_dict(sd)
    assert capsys.readouterr().out == ""
    assert b.last_epoch == 2 and b_opt.lr_state()[0] == 5
    assert b_opt.param_groups[0]["lr"] == a_opt.param_groups[0]["lr"] == pytest.approx(0.01)
    assert b.state_dict() == sd and b.get_last_lr() == a.get_last_lr()
    # an entry written with the schedule off has no count: t = 0, and one line says so
    off_cfg = Cfg(SOLVER=Cfg(optim="sgd", lr=0.1, scheduler="MultiStep", lr_step=[1, 3]))
    off_opt = get_optimizer(off_cfg, params)
    off = get_lr_scheduler(off_cfg, off_opt)
    off.step()
    c_opt, c = pair()
    c_opt.set_lr_updates(9)
    c.load_state_dict(off.state_dict())
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "t = 0" in out
    assert c.last_epoch == 1 and c_opt.lr_state()[0] == 0
    # ... and the other way round: the plain scheduler takes an entry with a count
    off.load_state_dict(sd)
    assert off.last_epoch == 2
    # other shape numbers in the checkpoint: this run's stay, one line names the difference
    d_opt, d = pair()
    sd2 = dict(sd, per_update=dict(sd["per_update"], lr_floor=0.5))
    d.load_state_dict(sd2)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "lr_floor" in out
    assert d_opt.lr_schedule.lr_floor == 0.1 and d_opt.lr_state()[0] == 5
    with pytest.raises(ValueError):
        d_opt.set_lr_updates(-1)


def test_header_declares_the_entry_and_binding_mirrors_the_struct():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_lr_sched\s*\(\s*const nef_lr_sched_args\s*\*\s*a,\s*nef_stream_t stream\s*\)", hdr)
    assert re.search(r"\bsize_t nef_lr_sched_args_bytes\s*\(\s*void\s*\)", hdr)
    assert re.search(r"typedef struct nef_lr_sched_args\s*\{", hdr) and re.search(r"\}\s*nef_lr_sched_args\s*;", hdr)
    body = hdr[hdr.index("typedef struct nef_lr_sched_args"):hdr.index("} nef_lr_sched_args;")]
    fields = re.findall(r"(\w+);\s*/\*", body)
    assert fields == [n for n, _ in _lib.LrSchedArgs._fields_]
    assert "int64_t* t;" in body and "const double* base_dev;" in body and "float* lr_out;" in body
    L = _lib.load()
    assert ctypes.sizeof(_lib.LrSchedArgs) == L.nef_lr_sched_args_bytes() == 96
    for name in ("nef_lr_sched", "nef_lr_sched_args_bytes"):
        assert name in _lib.SIGNATURES and hasattr(L, name)


def test_a_library_without_the_entry_is_rejected(monkeypatch):
    """The stale-library check.  The ABI number did not move (the entry is an addition), so a library built before it is told by the
    missing symbol: a shared object that lacks a declared entry -- here CPython's own _ctypes module -- does not load as the extension."""
    import _ctypes
    from electrocardio_panorama_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", _ctypes.__file__)
    with pytest.raises(_lib.NefLibraryError, match="rebuild"):
        _lib.load()


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(t=64, base_dev=None, lr_out=64, skip_if_positive=None, flag=None, warmup_updates=3, total_updates=8, base=0.1,
             warmup_start=0.01, lr_floor=0.0, poly_power=1.0, shape=1, advance=1)
    a.update(kw)
    return _lib.LrSchedArgs(**a)


def test_nef_lr_sched_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the launch: nothing is launched and no address is read (non-NULL, never dereferenced pointers)."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    call = lambda **kw: L.nef_lr_sched(ctypes.byref(_args(**kw)), None)      # noqa: E731
    assert L.nef_lr_sched(None, None) == -2                                   # NEF_E_NULL
    assert call(t=None) == -2 and call(lr_out=None) == -2
    assert call(shape=3) == -4 and call(shape=-1) == -4                       # NEF_E_UNSUPPORTED
    assert call(advance=2) == -1 and call(advance=-1) == -1                   # NEF_E_SHAPE
    assert call(warmup_updates=-1) == -1 and call(total_updates=-1) == -1
    for key in ("warmup_start", "lr_floor"):
        for bad in (-0.1, 1.5, math.nan, math.inf):
            assert call(**{key: bad}) == -1, (key, bad)
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert call(poly_power=bad) == -1, bad
    for bad in (-0.1, math.nan, math.inf):
        assert call(base=bad) == -1, bad
