"""Gradient accumulation on the device (SOLVER.accum_steps): nef_flatten_acc bit for bit against torch.cat / add_ on every path of the
kernel; the fused optimisers' windows bit for bit against one step on the fp32 sum times 1/K (K a power of two: both sides exact) and,
for K = 3, against fp64; flush, an open window, the taint word; five batches of Solver.run_one_epoch against the CPU oracle looping
(loss / m).backward() per micro-batch and SGDState.step per window (bars of test_sgd_steps_golden); graph replay against the eager path
bit for bit; and accum_steps == 1 is the code that was there."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from test_model_gpu import DEV, make_cfg
from util import rel, sub

pytestmark = pytest.mark.gpu

GUARD_F, GUARD_B = 4, 8


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _kernel_tensors():
    """Every path of flatten_acc_kernel.  600 001: 16-byte body whose grid-stride loop iterates (150 000 vectors over 128 x 256
    threads) and a one-element tail; 7 and 1: shorter than one vector, on destinations the odd offset leaves misaligned (scalar path);
    0: an empty tensor; 4096 taken one float into its storage: a misaligned source; 3 pad elements put the next destination back on a
    16-byte boundary, so a small aligned tensor (12: body only, 13: body + tail) runs the vector path too; 65 tensors in all: two launches."""
    gen = torch.Generator().manual_seed(11)
    sizes = [600001, 7, 1, 0]
    ts = [torch.randn(n, generator=gen).to(DEV) for n in sizes]
    store = torch.randn(4097, generator=gen).to(DEV)
    ts.append(store[1:])
    assert ts[-1].data_ptr() % 16 == 4 and ts[-1].numel() == 4096
    ts.append(torch.randn(3, generator=gen).to(DEV))           # 600001 + 7 + 1 + 4096 + 3 = 604108 = 4 * 151027
    ts.append(torch.randn(12, generator=gen).to(DEV))
    ts.append(torch.randn(13, generator=gen).to(DEV))
    while len(ts) < 65:
        ts.append(torch.randn(1 + (5 * len(ts)) % 23, generator=gen).to(DEV))
    assert len(ts) == 65 and sum(t.numel() for t in ts[:6]) % 4 == 0
    return ts


def _guarded(n, fill):
    buf = torch.empty(GUARD_F + n + GUARD_B, device=DEV)
    buf[:GUARD_F] = torch.arange(1, GUARD_F + 1, device=DEV) * -7.0
    buf[GUARD_F + n:] = torch.arange(1, GUARD_B + 1, device=DEV) * 13.0
    out = buf[GUARD_F:GUARD_F + n]
    out.copy_(fill) if torch.is_tensor(fill) else out.fill_(fill)
    assert out.data_ptr() % 16 == 0
    return buf, out


def _guards_ok(buf, n):
    return (torch.equal(buf[:GUARD_F], torch.arange(1, GUARD_F + 1, device=DEV) * -7.0) and
            torch.equal(buf[GUARD_F + n:], torch.arange(1, GUARD_B + 1, device=DEV) * 13.0))


@pytest.mark.parametrize("via", ["host", "word"])
def test_flatten_acc_bit_for_bit(via):
    from electrocardio_panorama_amd import _lib, ops
    ts = _kernel_tensors()
    cat = torch.cat([t.reshape(-1) for t in ts])
    n = cat.numel()
    base = torch.randn(n, generator=torch.Generator().manual_seed(12)).to(DEV)

    def call(out, acc):
        if via == "host":
            if acc:
                return ops.flatten_into(ts, out, accumulate=True)
            # (ops' accumulate=False is the default call, nef_flatten: the assign form of the new entry is reached through the binding)
            srcs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            sizes = (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts])
            return _lib.check(_lib.load().nef_flatten_acc(srcs, sizes, len(ts), out.data_ptr(), 0, None,
                                                          torch.cuda.current_stream().cuda_stream), "nef_flatten_acc")
        # the device word decides, whatever the host integer says
        return ops.flatten_into(ts, out, accumulate=not acc, accumulate_dev=torch.full((1,), acc, device=DEV, dtype=torch.int32))

    # assign: right on an `out` full of NaN -- it is not read
    buf, out = _guarded(n, float("nan"))
    call(out, 0)
    assert torch.equal(out, cat) and _guards_ok(buf, n)
    # accumulate: one fp32 add per element, exact in both
    buf, out = _guarded(n, base)
    call(out, 1)
    want = base.clone().add_(cat)
    assert torch.equal(out, want) and _guards_ok(buf, n)
    assert not torch.equal(out, cat)
    # ... twice: the sum in call order
    call(out, 1)
    assert torch.equal(out, want.add_(cat)) and _guards_ok(buf, n)
    # accumulate = 0 is nef_flatten bit for bit (which takes no NULL source: the same list without the empty tensor)
    full = [t for t in ts if t.numel()]
    buf2, out2 = _guarded(n, 0.0)
    ops.flatten_into(full, out2)
    buf, out = _guarded(n, float("nan"))
    call(out, 0)
    assert torch.equal(out, out2) and torch.equal(buf, buf2)


def test_flatten_acc_one_tensor_and_slices():
    """One launch row, a destination slice that starts misaligned, and an n == 0 call that leaves `out` alone."""
    from electrocardio_panorama_amd import ops
    gen = torch.Generator().manual_seed(13)
    a, b = torch.randn(1030, generator=gen).to(DEV), torch.randn(9, generator=gen).to(DEV)
    buf, out = _guarded(1039, 1.0)
    ops.flatten_into([a], out[:1030], accumulate=True)
    ops.flatten_into([b], out[1030:], accumulate=True)           # destination 1030 floats in: 8-byte aligned only
    assert torch.equal(out, torch.cat([a, b]) + 1.0) and _guards_ok(buf, 1039)
    ops.flatten_into([], out, accumulate=True)
    assert torch.equal(out, torch.cat([a, b]) + 1.0)


# ------------------------------------------------------------------------------------------------ 2. the optimisers
SIZES = (1030, 7, 4096)
NAMES = ("a.weight", "a.bias", "b.weight")
EXTRAS = dict(max_grad_norm=1.0, ema_decay=0.9, no_decay=("*.bias",))


def _make(name, **kw):
    from electrocardio_panorama_amd.solver import optim_scheduler as osch
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


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("name", ["sgd", "adam", "adamw", "lars", "lamb"])
def test_window_equals_one_step_on_the_scaled_sum(name, K):
    """Two windows of K micro-batches against two accum_steps=1 steps on (g_1 + ... + g_K) * (1 / K), the sum built in fp32 in the same
    order.  1 / K is a power of two: the scaling commutes with every rounding, so the bits agree -- clipping (it clips: the norm is ~50),
    the average, the no_decay pattern and the trust ratios included."""
    sets = _grad_sets(2 * K)
    pa, acc = _make(name, accum_steps=K, **EXTRAS)
    pr, ref = _make(name, **EXTRAS)
    for w in range(2):
        window = sets[w * K:(w + 1) * K]
        for i, gs in enumerate(window):
            _set_grads(pa, gs)
            acc.step()
            assert acc.window_open == (i < K - 1)
        summed = [g.clone() for g in window[0]]
        for gs in window[1:]:
            for s, g in zip(summed, gs):
                s.add_(g)
        _set_grads(pr, [s * (1.0 / K) for s in summed])
        ref.step()
        a, r = _everything(acc), _everything(ref)
        assert set(a) == set(r) and {"p", "ema", "ema_n", "clip_stats"} <= set(a)
        for k in a:
            assert torch.equal(a[k], r[k]), (name, K, w, k)
    assert float(acc.clip_stats[2]) == 2.0                          # both updates clipped, counted once per update
    assert float(acc._flat[0]["ema_n"]) == 2.0
    if "step" in acc._flat[0]:
        assert float(acc._flat[0]["step"]) == 2.0                   # Adam's count: per update, not per micro-batch
    if name in ("lars", "lamb"):
        assert float(acc._flat[0]["trust_stats"][2]) == 2.0
        q = acc.trust_ratios()
        assert q["a.bias"] == 1.0 and q["a.weight"] != 1.0


def test_sgd_three_micro_batches_against_fp64():
    """K = 3, no momentum history: p1 = p0 - lr * mean(g).  Bar per element: lr * (K + 1) * 2^-24 * sum_k |g_k| / K (the K - 1 fp32 adds
    of the sum, the product with gscale and with lr) + 2^-24 * |p| (the final subtract)."""
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD
    K, lr = 3, 0.1
    sets = _grad_sets(K, seed=71)
    params, _ = _make("sgd")
    opt = FusedSGD(params, lr=lr, accum_steps=K)
    p0 = torch.cat([p.detach().reshape(-1) for p in params]).double().cpu()
    for gs in sets:
        _set_grads(params, gs)
        opt.step()
    g64 = torch.stack([torch.cat(gs).double().cpu() for gs in sets])
    want = p0 - lr * g64.mean(0)
    got = opt._flat[0]["p"].double().cpu()
    tol = lr * (K + 1) * 2.0 ** -24 * g64.abs().sum(0) / K + 2.0 ** -24 * want.abs()
    err = (got - want).abs()
    print(f"K=3 sgd vs fp64: worst error / bar {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), float((err / tol).max())
    assert float((got - p0).abs().max()) > 1e-3


def test_flush_open_window_and_untouched_state():
    """A call that does not close the window leaves parameters and state as they were; flush() after one of three micro-batches is an
    accum_steps=1 step on that gradient, bit for bit; flush() on an empty window does nothing."""
    gs, g0 = _grad_sets(1, seed=72)[0], _grad_sets(1, seed=73)[0]
    pa, acc = _make("adam", accum_steps=3, **EXTRAS)
    pr, ref = _make("adam", **EXTRAS)
    for _ in range(3):                                               # one full window first: a state with history ...
        _set_grads(pa, g0)
        acc.step()
    _set_grads(pr, g0)
    ref.step()                                                       # ... which the reference (built by a step of its own) takes over
    for k, v in _everything(acc).items():
        (ref.clip_stats if k == "clip_stats" else ref._flat[0][k]).copy_(v)
    before = _everything(acc)
    _set_grads(pa, gs)
    acc.step()
    assert acc.window_open
    for k, v in _everything(acc).items():
        assert torch.equal(v, before[k]), k
    acc.flush()
    assert not acc.window_open
    _set_grads(pr, gs)
    ref.step()
    a, r = _everything(acc), _everything(ref)
    for k in a:
        assert torch.equal(a[k], r[k]), k
    assert not torch.equal(a["p"], before["p"])
    acc.flush()
    for k, v in _everything(acc).items():
        assert torch.equal(v, a[k]), k


def test_taint_in_the_second_micro_batch_skips_the_whole_update():
    """A clamp counted while the window's second micro-batch ran: the one taint launch at the window's end sees it (the mark advances
    only when the launch runs) and the update is skipped -- parameters, state and the average untouched, the skip counted once."""
    from electrocardio_panorama_amd import ops
    sets = _grad_sets(4, seed=74)
    pa, acc = _make("sgd", accum_steps=2, ema_decay=0.9)
    for gs in sets[:2]:
        _set_grads(pa, gs)
        acc.step()
    st = ops._amax_state(pa[0].device)
    ops.h2_clamped(), ops.h2_skipped()                               # (reset the host's marks)
    before = _everything(acc)
    _set_grads(pa, sets[2])
    acc.step()
    st["clamped"] += 1                                               # what a clamping split-fp16 launch of this micro-batch does
    _set_grads(pa, sets[3])
    acc.step()
    assert not acc.window_open
    for k, v in _everything(acc).items():
        assert torch.equal(v, before[k]), k
    assert ops.h2_skipped() == 1 and ops.h2_clamped() == 1
    # the next window is clean again
    for gs in sets[:2]:
        _set_grads(pa, gs)
        acc.step()
    assert not torch.equal(acc._flat[0]["p"], before["p"]) and ops.h2_skipped() == 0


def test_changed_live_set_inside_a_window_raises():
    gs = _grad_sets(1, seed=75)[0]
    pa, acc = _make("sgd", accum_steps=2)
    _set_grads(pa, gs)
    acc.step()
    _set_grads(pa, gs)
    pa[1].grad = None
    with pytest.raises(RuntimeError, match="flush"):
        acc.step()
    _set_grads(pa, gs)
    pa[0].data = pa[0].data.clone()                                  # re-pointed from outside
    with pytest.raises(RuntimeError, match="flush"):
        acc.step()
    with pytest.raises(RuntimeError, match="flush"):
        acc.load_state_dict(acc.state_dict())


def test_off_is_off():
    """accum_steps=1: no flatten_acc launch among ops' per-launch tags and the bits of an optimiser built without the keyword; K = 2
    shows the tag is there to be seen."""
    from electrocardio_panorama_amd import ops
    sets = _grad_sets(3, seed=76)
    states, tags = [], []
    for kw in ({}, dict(accum_steps=1), dict(accum_steps=2)):
        params, opt = _make("sgd", **kw, **EXTRAS)
        ops.PROFILE = []
        try:
            for gs in sets:
                _set_grads(params, gs)
                opt.step()
            tags.append([t[1] for t, _, _ in ops.PROFILE if t[0] == "hbm"])
        finally:
            ops.PROFILE = None
        states.append(_everything(opt))
    assert "flatten_acc" not in tags[0] and "flatten_acc" not in tags[1] and tags[0] == tags[1]
    assert tags[2].count("flatten_acc") == 1        # (assign, add + update, assign: the assigning micro-batches are nef_flatten launches)
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
    assert not torch.equal(states[0]["p"], states[2]["p"])


# ------------------------------------------------------------------------------------------------ 3. Solver-level helpers
def _solver(V, optim, graph, K, lr=None):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr={"sgd": 0.1, "lamb": 1e-3}[optim] if lr is None else lr)
    cfg.SOLVER["optim"] = optim
    cfg.SOLVER["graph"] = bool(graph)
    cfg.SOLVER["accum_steps"] = K
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


_SLOTS = {"sgd": ("buf",), "lamb": ("m", "v", "step", "ratio", "trust_stats")}


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + [v.clone() for k, v in sol.model.named_buffers()]


# ------------------------------------------------------------------------------------------------ 4. trajectory against the oracle
N_BATCHES = 5


@pytest.fixture(scope="module", params=[2, 3], ids=["K2", "K3"])
def accum_oracle(request, golden_dir):
    """The recipe of sgd_B4_V3_L512.npz over five batches on the CPU oracle: (loss / m).backward() per micro-batch (torch sums into
    .grad), SGDState.step per window of m = min(K, what the epoch has left) micro-batches.  K = 2: 2 + 2 + 1; K = 3: 3 + 2."""
    from electrocardio_panorama_amd import synth
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    K = request.param
    z = np.load(os.path.join(golden_dir, "sgd_B4_V3_L512.npz"))
    B, V, L, seed = (int(z[k]) for k in ("B", "V", "L", "seed"))
    lr = float(z["lr"])
    assert (B, V, L, seed, lr) == (4, 3, 512, 21, 0.1)
    batches = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(N_BATCHES)]
    P, Bf, opt = orc.require_grad(hw.hashed_params(V)), hw.hashed_buffers(), orc.SGDState(lr)
    random.seed(seed)
    losses, i = [], 0
    while i < N_BATCHES:
        m = min(K, N_BATCHES - i)
        for b in batches[i:i + m]:
            choice = (random.randint(0, V - 1), random.randint(0, V - 1))
            bt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}
            out, out_p, out_l = orc.forward(P, Bf, bt["data"], bt["input_theta"], bt["target_theta"], bt["rois"], phase="train",
                                            training=True, masks=None, p=0.0, lead_choice=choice)
            ls = orc.loss_v1(out, out_p, out_l, bt["target_view"].unsqueeze(1))
            (ls[0] / m).backward()
            losses.append([float(v.detach()) for v in ls])
        opt.step(P)
        i += m
    return dict(K=K, V=V, seed=seed, lr=lr, batches=batches, losses=np.array(losses), P={k: v.detach() for k, v in P.items()}, Bf=Bf,
                every_batch_losses=z["losses"])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_accum_sgd_steps_vs_oracle(accum_oracle, graph):
    """Solver.run_one_epoch(phase='train') with SOLVER.accum_steps against the oracle, eagerly and through the captured graphs; the bars
    of test_sgd_steps_golden.  What they catch (CPU oracle): a path that ignores K is 2.0e-2 off the loss bar from the second batch on
    -- asserted below on the oracle's own two trajectories; one that sums without the 1 / K misses it from the first batch behind an
    update (1.8e-2 at K = 2, 3.2e-2 at K = 3); a flush scaled 1 / K instead of 1 / m leaves the losses alone and puts 19 (K = 2) or 17
    (K = 3) parameters beyond 2e-4."""
    from oracle import nefnet_oracle as orc
    t = accum_oracle
    K, V = t["K"], t["V"]
    # the trajectory that updates behind every batch (the fixture's own three steps) is far from the accumulated one at the second batch
    assert abs(t["losses"][1, 0] - t["every_batch_losses"][1, 0]) > 1e-2
    cfg, sol, opt = _solver(V, "sgd", graph, K, lr=t["lr"])
    random.seed(t["seed"])
    losses = sol.run_one_epoch(t["batches"], "train", opt, collect_views=False)[0]
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == bool(graph)
    if graph:
        assert st.calls == N_BATCHES and len(st.slots) == 1
    assert not opt.window_open
    assert sol.last_updates == (-(-N_BATCHES // K), N_BATCHES)
    assert len(losses) == N_BATCHES                                   # every micro-batch has its row
    dl = float(np.abs(np.array(losses) - t["losses"]).max())
    sd = sol.model.state_dict()
    worst, errs = (0.0, None), {}
    for k in orc.param_shapes(V):
        errs[k] = rel(sub(sd[k], 128), sub(t["P"][k], 128))
        if k not in orc.DEAD_PARAMS and errs[k] > worst[0]:
            worst = (errs[k], k)
    line = (f"5-batch SGD trajectory with accum_steps {K} vs the oracle ({'graphed' if graph else 'eager'}): losses max-abs {dl:.2e} "
            f"(bar 2e-5), worst parameter {worst[1]} rel-L2 {worst[0]:.2e} (bar 2e-4)")
    print(line)
    import conftest
    conftest.report(line)
    assert dl < 2e-5, (losses, t["losses"])
    for k, e in errs.items():
        assert e < (1e-6 if k in orc.DEAD_PARAMS else 2e-4), (k, e)
    for k in orc.buffer_shapes():
        if "running" in k:
            assert rel(sd[k], t["Bf"][k]) < 1e-4, k
    assert int(sd["decoder.1.double_conv.1.num_batches_tracked"]) == 3 * N_BATCHES      # per micro-batch, as in torch


# ------------------------------------------------------------------------------------------------ 5. graphed == eager
@pytest.mark.parametrize("optim", ["sgd", "lamb"])
@pytest.mark.parametrize("K", [2, 4])
def test_accum_graphed_equals_eager(optim, K):
    """Six batches, parameters / optimiser state / BatchNorm buffers bit for bit.  K = 2: three epochs of one window each with a
    MultiStepLR milestone crossed between the first and the second.  K = 4: one epoch whose six batches end in a flushed window of 2."""
    from torch.optim.lr_scheduler import MultiStepLR
    from electrocardio_panorama_amd import synth
    V, B, L = 3, 2, 512
    batches = [synth.make_batch(B, V, L, seed=40 + s, Q=2) for s in range(6)]
    out = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(V, optim, graph, K)
        if K == 2:
            sched = MultiStepLR(opt, [1], gamma=0.1)
            snaps = []
            for e in range(3):
                random.seed(100 + e)
                sol.run_one_epoch(batches[2 * e:2 * e + 2], "train", opt, collect_views=False)
                sched.step()
                assert sol.last_updates == (1, 2)
                snaps.append(_state(sol, opt, optim))
            assert opt.param_groups[0]["lr"] == pytest.approx(0.1 * {"sgd": 0.1, "lamb": 1e-3}[optim])
        else:
            random.seed(100)
            sol.run_one_epoch(batches, "train", opt, collect_views=False)
            assert sol.last_updates == (2, 6)
            snaps = [_state(sol, opt, optim)]
        st = getattr(sol, "_graph_stepper", None)
        assert (st is not None) == graph and not opt.window_open
        if graph:
            assert len(st.slots) == 1 and st.calls == 6
        out[graph] = snaps
    for sa, sb in zip(out[False], out[True]):
        for a, b in zip(sa, sb):
            assert torch.equal(a, b)
    if K == 2:
        assert not torch.equal(out[True][0][0], out[True][2][0])


def test_eager_and_replayed_micro_batches_share_a_window():
    """The window position lives in the optimiser: a window opened by an eager micro-batch and closed by a replayed one gives the bits
    of the all-eager window."""
    from electrocardio_panorama_amd import synth
    V, B, L = 3, 2, 512
    batches = [synth.make_batch(B, V, L, seed=40 + s, Q=2) for s in range(2)]
    out = []
    for mixed in (False, True):
        cfg, sol, opt = _solver(V, "sgd", False, 2)
        random.seed(100)
        for i, b in enumerate(batches):
            cfg.SOLVER["graph"] = bool(mixed and i == 1)
            # (one batch per call would flush: feed the Solver's loop body through a two-batch epoch by hand)
            if i == 0:
                sol.model.train()
                data, rois, in_t, tgt, q_t, _ = sol._to_device(b)
                o, sp, sl = sol.model(data, in_t, q_t, rois, phase="train")
                sol.loss(o, sp, sl, tgt, cfg)[0].backward()
                opt.step()
                opt.zero_grad()
                assert opt.window_open
            else:
                sol.run_one_epoch([b], "train", opt, collect_views=False)
                assert sol.last_updates == (1, 1) and not opt.window_open
        assert (getattr(sol, "_graph_stepper", None) is not None) == mixed
        out.append(_state(sol, opt, "sgd"))
    for a, b in zip(*out):
        assert torch.equal(a, b)
