"""cfg.DATA.noise on the device path (reference solver.py:185-186, `out = out + noise` between model and loss): the noise row as an
addend of the loss kernels against the CPU oracle's loss, bit for bit against the explicit add, through losswrapper's autograd, a
three-step trajectory against the oracle's train_step(add_noise=True) eagerly and replayed, graph replay against the eager path, and
DATA.noise off."""
import os
import random

import numpy as np
import pytest
import torch

from test_model_gpu import DEV, make_cfg
from util import maxabs, rel, rnd, sub

pytestmark = pytest.mark.gpu

FACTORS = (0.5, 0.5, 1.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g(t):
    return t.to(DEV).contiguous()


def noise_rows(s, B, L):
    return np.random.default_rng(9000 + s).normal(0, 0.05, (B, L)).astype(np.float32)


def _loss_inputs(shape):
    """test_loss's inputs (sigmoids of seeded normals) and a noise of std 0.05 in the prediction's layout."""
    pred, pp, pl, tgt = (torch.sigmoid(rnd(*shape, seed=s)) for s in (48, 49, 50, 51))
    nz = torch.from_numpy(np.random.default_rng(9000).normal(0, 0.05, shape).astype(np.float32))
    return pred, pp, pl, tgt, nz


# ------------------------------------------------------------------------------------------------ 1. the kernels vs the oracle's loss
@pytest.mark.parametrize("reg", ["l1_loss", "l2_loss"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 1, 500), (2, 1, 40000)], ids=["one", "B4_L500", "stride_loop"])
def test_noise_loss_kernels_vs_oracle(shape, reg):
    """(2, 1, 40000): 80000 elements are more than loss_partial's 65536 threads, so its stride loop runs.  Bars: test_loss's own."""
    from electrocardio_panorama_amd import ops
    from oracle import nefnet_oracle as orc
    pred, pp, pl, tgt, nz = _loss_inputs(shape)
    pr, ppr, plr = (t.clone().requires_grad_(True) for t in (pred, pp, pl))
    ref = orc.loss_v1(pr + nz, ppr, plr, tgt, FACTORS, (1, 2, 3), reg)
    L4 = ops.loss_fwd(g(pred), g(pp), g(pl), g(tgt), FACTORS, reg == "l2_loss", 7, noise=g(nz))
    e = maxabs(L4, torch.stack([r.detach() for r in ref]))
    ref[0].backward()
    g_pred, g_p, g_l = ops.loss_bwd(g(pred), g(pp), g(pl), g(tgt), torch.ones(4, device=DEV), FACTORS, reg == "l2_loss", 7,
                                    noise=g(nz))
    errs = (rel(g_pred, pr.grad), rel(g_p, ppr.grad), rel(g_l, plr.grad))
    print(f"{shape} {reg}: losses max-abs {e:.2e}, gradients rel-L2 {errs}")
    assert e < 1e-6
    assert all(x < 1e-5 for x in errs), errs
    # the noise is seen: the clean losses are not the noisy ones
    clean = ops.loss_fwd(g(pred), g(pp), g(pl), g(tgt), FACTORS, reg == "l2_loss", 7)
    assert not torch.equal(clean, L4)


# ------------------------------------------------------------------------------------------------ 2. the add is the reference's add
@pytest.mark.parametrize("use_mask", [7, 4])
@pytest.mark.parametrize("reg_l2", [False, True], ids=["l1_loss", "l2_loss"])
@pytest.mark.parametrize("shape", [(4, 1, 500), (2, 1, 40000)], ids=["B4_L500", "stride_loop"])
def test_noise_addend_equals_explicit_add_bit_for_bit(shape, reg_l2, use_mask):
    """One fp32 add has one result and nothing in (a + b) - c can contract: the kernels with noise= give the bits of the kernels on
    pred + noise; a null noise gives the bits of a noise of zeros."""
    from electrocardio_panorama_amd import ops
    pred, pp, pl, tgt, nz = (g(t) for t in _loss_inputs(shape))
    gs = torch.full((1,), 0.37, device=DEV)
    added = pred + nz
    assert torch.equal(ops.loss_fwd(pred, pp, pl, tgt, FACTORS, reg_l2, use_mask, noise=nz),
                       ops.loss_fwd(added, pp, pl, tgt, FACTORS, reg_l2, use_mask))
    got = ops.loss_bwd(pred, pp, pl, tgt, gs, FACTORS, reg_l2, use_mask, noise=nz)
    want = ops.loss_bwd(added, pp, pl, tgt, gs, FACTORS, reg_l2, use_mask)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert any(float(t.abs().max()) > 0 for t in got)
    zeros = torch.zeros_like(pred)
    assert torch.equal(ops.loss_fwd(pred, pp, pl, tgt, FACTORS, reg_l2, use_mask),
                       ops.loss_fwd(pred, pp, pl, tgt, FACTORS, reg_l2, use_mask, noise=zeros))
    none = ops.loss_bwd(pred, pp, pl, tgt, gs, FACTORS, reg_l2, use_mask)
    zero = ops.loss_bwd(pred, pp, pl, tgt, gs, FACTORS, reg_l2, use_mask, noise=zeros)
    assert all(torch.equal(a, b) for a, b in zip(none, zero))


# ------------------------------------------------------------------------------------------------ 3. losswrapper autograd
def test_losswrapper_noise_keyword_equals_the_users_own_add():
    """A loop that writes `out = out + noise` in front of losswrapper and one that passes noise= get the same bits: losses and the
    gradients of out, p, l; a [B, L] row after unsqueeze(1) and a [B, 1, L] tensor agree."""
    from electrocardio_panorama_amd.network import losswrapper
    cfg = make_cfg(3)
    B, L = 4, 512
    out0, p0, l0, tgt = (g(torch.sigmoid(rnd(B, 1, L, seed=s))) for s in (60, 61, 62, 63))
    rows = g(torch.from_numpy(noise_rows(0, B, L)))
    res = []
    for mode in ("keyword", "added", "keyword_B1L"):
        out, p, l_ = (t.clone().requires_grad_(True) for t in (out0, p0, l0))
        if mode == "added":
            losses = losswrapper(out + rows.unsqueeze(1), p, l_, tgt, cfg)
        else:
            nz = rows.unsqueeze(1) if mode == "keyword" else rows.reshape(B, 1, L).clone()
            losses = losswrapper(out, p, l_, tgt, cfg, noise=nz)
        assert len(losses) == 4
        losses[0].backward()
        res.append([x.detach().clone() for x in losses] + [out.grad, p.grad, l_.grad])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    assert float(res[0][4].abs().max()) > 0 and float(res[0][5].abs().max()) > 0
    # the noise is seen
    out, p, l_ = (t.clone().requires_grad_(True) for t in (out0, p0, l0))
    assert not torch.equal(losswrapper(out, p, l_, tgt, cfg)[0].detach(), res[0][0])


# ------------------------------------------------------------------------------------------------ Solver-level helpers
def _batches(n, B, V, L, seed0, first=0):
    """synth batches seed0 + s with the noise rows of step s (synth's own are zeros)."""
    from electrocardio_panorama_amd import synth
    out = []
    for s in range(first, first + n):
        b = dict(synth.make_batch(B, V, L, seed=seed0 + s, Q=2))
        b["noise"] = noise_rows(s, B, L)
        out.append(b)
    return out


def _solver(V, optim, graph, noise, lr=None):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr={"sgd": 0.1, "adam": 1e-3}[optim] if lr is None else lr, noise=noise)
    cfg.SOLVER["optim"] = optim
    cfg.SOLVER["graph"] = bool(graph)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


_SLOTS = {"sgd": ("buf",), "adam": ("m", "v", "step")}


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + \
        [v.clone() for k, v in sol.model.named_buffers() if "running" in k]


# ------------------------------------------------------------------------------------------------ 4. trajectory vs the oracle
@pytest.fixture(scope="module")
def noisy_oracle_trajectory(golden_dir):
    """Three steps of the oracle's train_step(add_noise=True) on the CPU: the recipe of sgd_B4_V3_L512.npz with the noise on."""
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    z = np.load(os.path.join(golden_dir, "sgd_B4_V3_L512.npz"))
    B, V, L, seed, steps = (int(z[k]) for k in ("B", "V", "L", "seed", "steps"))
    lr = float(z["lr"])
    assert (B, V, L, seed, steps, lr) == (4, 3, 512, 21, 3, 0.1)
    batches = _batches(steps, B, V, L, seed)
    P, Bf, opt = orc.require_grad(hw.hashed_params(V)), hw.hashed_buffers(), orc.SGDState(lr)
    random.seed(seed)
    losses = []
    for b in batches:
        choice = (random.randint(0, V - 1), random.randint(0, V - 1))
        bt = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}
        losses.append(orc.train_step(P, Bf, opt, bt, p=0.0, lead_choice=choice, add_noise=True))
    return dict(V=V, seed=seed, lr=lr, steps=steps, batches=batches, losses=np.array(losses),
                P={k: v.detach() for k, v in P.items()}, Bf=Bf, clean_losses=z["losses"])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_noisy_sgd_steps_vs_oracle(noisy_oracle_trajectory, graph):
    """Solver.run_one_epoch(phase='train') with DATA.noise against the oracle, eagerly and through the captured graph; the bars of
    test_sgd_steps_golden.  The noisy total loss is at least 1.8e-2 away from the clean one in every step (CPU oracle), so a path that
    ignores the noise, or adds it to the regression term only, misses the 2e-5 bar."""
    from oracle import nefnet_oracle as orc
    t = noisy_oracle_trajectory
    V, steps = t["V"], t["steps"]
    assert np.abs(t["losses"][:, 0] - t["clean_losses"][:, 0]).min() > 1e-2
    cfg, sol, opt = _solver(V, "sgd", graph, True, lr=t["lr"])
    random.seed(t["seed"])
    losses = sol.run_one_epoch(t["batches"], "train", opt, collect_views=False)[0]
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == bool(graph)
    if graph:
        assert st.calls == steps and len(st.slots) == 1
    dl = float(np.abs(np.array(losses) - t["losses"]).max())
    sd = sol.model.state_dict()
    worst = (0.0, None)
    errs = {}
    for k in orc.param_shapes(V):
        errs[k] = rel(sub(sd[k], 128), sub(t["P"][k], 128))
        if k not in orc.DEAD_PARAMS and errs[k] > worst[0]:
            worst = (errs[k], k)
    import conftest
    line = (f"3-step SGD trajectory with DATA.noise vs the oracle ({'graphed' if graph else 'eager'}): losses max-abs {dl:.2e} "
            f"(bar 2e-5), worst parameter {worst[1]} rel-L2 {worst[0]:.2e} (bar 2e-4)")
    print(line)
    conftest.report(line)
    assert dl < 2e-5, (losses, t["losses"])
    for k, e in errs.items():
        assert e < (1e-6 if k in orc.DEAD_PARAMS else 2e-4), (k, e)
    for k in orc.buffer_shapes():
        if "running" in k:
            assert rel(sd[k], t["Bf"][k]) < 1e-4, k
    assert int(sd["decoder.1.double_conv.1.num_batches_tracked"]) == 3 * steps


# ------------------------------------------------------------------------------------------------ 5. graphed == eager
@pytest.mark.parametrize("optim", ["sgd", "adam"])
def test_noise_graphed_equals_eager_across_lr_milestone(optim):
    """Six noisy steps with a MultiStepLR milestone crossed after step 3: the replayed step equals the eager one bit for bit
    (parameters, optimiser state, BatchNorm statistics) from one capture; a step of a second shape (B = 1) replays its own slot with
    its own noise buffer."""
    from torch.optim.lr_scheduler import MultiStepLR
    V, B, L = 3, 2, 512
    batches = _batches(6, B, V, L, 40)
    small = _batches(1, 1, V, L, 40, first=6)[0]
    out = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(V, optim, graph, True)
        sched = MultiStepLR(opt, [3], gamma=0.1)
        slot = None
        for i, b in enumerate(batches):
            random.seed(100 + i)
            sol.run_one_epoch([b], "train", opt, collect_views=False)
            sched.step()
            if graph:
                st = sol._graph_stepper
                assert st is not None and len(st.slots) == 1
                slot = slot or next(iter(st.slots.values()))
                assert next(iter(st.slots.values())) is slot          # one capture only
                assert torch.equal(slot["noise"].cpu().reshape(B, L), torch.from_numpy(b["noise"]))
        six = _state(sol, opt, optim)
        random.seed(106)
        sol.run_one_epoch([small], "train", opt, collect_views=False)
        if graph:
            st = sol._graph_stepper
            assert len(st.slots) == 2 and st.calls == 7
            bufs = [s_["noise"] for s_ in st.slots.values()]
            assert sorted(tuple(t.shape) for t in bufs) == [(1, 1, L), (B, 1, L)]
            assert bufs[0].data_ptr() != bufs[1].data_ptr()
            assert torch.equal(bufs[1].cpu().reshape(1, L), torch.from_numpy(small["noise"]))
            assert torch.equal(bufs[0].cpu().reshape(B, L), torch.from_numpy(batches[5]["noise"]))      # the first slot keeps its own
        else:
            assert getattr(sol, "_graph_stepper", None) is None
        out[graph] = (six, _state(sol, opt, optim))
    for k in (0, 1):
        for a, b in zip(out[False][k], out[True][k]):
            assert torch.equal(a, b)
    assert not torch.equal(out[True][0][0], out[True][1][0])


# ------------------------------------------------------------------------------------------------ 6. off is off
def test_noise_off_is_off():
    """DATA.noise False: three graphed SGD steps give the same bits whether the batches (Solver) or the call (stepper) carry a
    non-zero noise or none, and the slot holds no noise buffer.  DATA.noise True: a call without noise is an error."""
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    V, B, L = 3, 2, 512
    noisy = _batches(3, B, V, L, 40)
    quiet = [dict(b, noise=np.zeros((B, L), np.float32)) for b in noisy]
    out = {}
    for name, batches in (("solver_quiet", quiet), ("solver_noisy", noisy)):
        cfg, sol, opt = _solver(V, "sgd", True, False)
        for i, b in enumerate(batches):
            random.seed(100 + i)
            sol.run_one_epoch([b], "train", opt, collect_views=False)
        st = sol._graph_stepper
        assert st is not None and st.calls == 3 and len(st.slots) == 1
        assert "noise" not in next(iter(st.slots.values())) and st.noise is None
        out[name] = _state(sol, opt, "sgd")
    for name in ("stepper_none", "stepper_noisy"):
        cfg, sol, opt = _solver(V, "sgd", True, False)
        st = GraphedTrainStep(sol.model, cfg, optimizer=opt)
        for i, b in enumerate(noisy):
            t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}
            random.seed(100 + i)
            args = (t["data"], t["input_theta"], t["target_theta"], t["rois"], t["target_view"].unsqueeze(1))
            st(*args) if name == "stepper_none" else st(*args, noise=t["noise"].unsqueeze(1))
        assert "noise" not in next(iter(st.slots.values())) and st.noise is None
        out[name] = _state(sol, opt, "sgd")
    for one, other in (("solver_quiet", "solver_noisy"), ("stepper_none", "stepper_noisy")):
        for a, b in zip(out[one], out[other]):
            assert torch.equal(a, b), other
    cfg, sol, opt = _solver(V, "sgd", True, True)
    st = GraphedTrainStep(sol.model, cfg, optimizer=opt)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in noisy[0].items()}
    with pytest.raises(ValueError):
        st(t["data"], t["input_theta"], t["target_theta"], t["rois"], t["target_view"].unsqueeze(1))
    assert st.slots == {}
