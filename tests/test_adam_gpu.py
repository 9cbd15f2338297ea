"""FusedAdam: the nef_adam kernel against torch.optim.Adam, the reference Solver's Adam trajectory (eager and graphed), graph
replay against the eager path, checkpoints in both formats, and the pre-packed operand table after an update."""
import copy
import os
import random

import numpy as np
import pytest
import torch

from test_model_gpu import DEV, golden, hashed_model, make_cfg
from util import rel, sub

pytestmark = pytest.mark.gpu


def adam_cfg(V, lr=1e-3):
    cfg = make_cfg(V, lr=lr)
    cfg.SOLVER["optim"] = "adam"
    return cfg


def _grads(n, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0          # exact zeros (dead units)
        out.append(g)
    return out


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [1000, 4099])
def test_adam_kernel_vs_torch(n, wd, off):
    """Five steps of ops.adam (gradients scaled by gscale = 0.5, as after a two-rank all-reduce sum) == torch.optim.Adam on the averaged
    gradients (fp32, foreach=False): ragged tail, exact zeros, L2 weight decay, the 16-byte and the scalar path."""
    from electrocardio_panorama_amd import ops
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = _grads(n, 5, n + 1)
    ref = torch.nn.Parameter(p0.clone().to(DEV))
    ropt = torch.optim.Adam([ref], lr=1e-3, weight_decay=wd, foreach=False)
    for g in grads:
        ref.grad = (g * 0.5).to(DEV)
        ropt.step()
    bufs = [torch.zeros(n + off, device=DEV) for _ in range(4)]
    p, g_dev, m, v = (b[off:] for b in bufs)
    p.copy_(p0)
    step = torch.zeros(1, device=DEV)
    for g in grads:
        g_dev.copy_(g)
        ops.adam(p, g_dev, m, v, step, 1e-3, 0.9, 0.999, 1e-8, wd, 0.5)
    torch.cuda.synchronize()
    st = ropt.state[ref]
    assert rel(m, st["exp_avg"]) <= 1e-6 and rel(v, st["exp_avg_sq"]) <= 1e-6, (rel(m, st["exp_avg"]), rel(v, st["exp_avg_sq"]))
    d0 = p0.to(DEV)
    assert rel(p - d0, ref.detach() - d0) <= 1e-5, rel(p - d0, ref.detach() - d0)
    assert float(step.item()) == 5.0 == float(st["step"])


def test_adam_skip_word_and_lr_dev():
    from electrocardio_panorama_amd import ops
    n = 4099
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=gen).to(DEV)
    m, v, step = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
    g1, g2 = (g.to(DEV) for g in _grads(n, 2, 4))
    ops.adam(p, g1, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
    ops.h2_skipped()                                         # (reset the host's mark)
    before = [t.clone() for t in (p, m, v, step)]
    ops.adam(p, g2, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, skip=torch.ones(1, device=DEV))
    for a, b in zip((p, m, v, step), before):
        assert torch.equal(a, b)
    assert ops.h2_skipped() == 1
    # a zero skip word steps; lr_dev replaces lr
    a = [t.clone() for t in before]
    b = [t.clone() for t in before]
    ops.adam(a[0], g2, a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, skip=torch.zeros(1, device=DEV),
             lr_dev=torch.full((1,), 5e-3, device=DEV))
    ops.adam(b[0], g2, b[1], b[2], b[3], 5e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[3].item()) == 2.0 and not torch.equal(a[0], before[0])
    assert ops.h2_skipped() == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_adam_steps_golden(golden_dir, graph):
    """Three iterations of Solver.run_one_epoch(phase='train') with optim='adam' vs the reference Solver's own torch.optim.Adam
    trajectory (tools/make_golden_adam.py) -- eagerly, and through the captured hipGraph (FusedAdam's flat buffers stepped)."""
    from electrocardio_panorama_amd import synth
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, get_optimizer
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    z = np.load(golden(golden_dir, "adam_*.npz")[0])
    B, V, L, seed, steps = (int(z[k]) for k in ("B", "V", "L", "seed", "steps"))
    cfg = adam_cfg(V, lr=float(z["lr"]))
    cfg.SOLVER["graph"] = bool(graph)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    batches = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]
    opt = get_optimizer(cfg, sol.model.parameters())
    assert isinstance(opt, FusedAdam)
    random.seed(seed)
    losses = sol.run_one_epoch(batches, "train", opt, collect_views=not graph)[0]
    st = getattr(sol, "_graph_stepper", None)
    assert (st is not None) == bool(graph)
    if graph:      # the moments live in the optimiser's state (checkpoints see them), not in a private buffer
        fl = opt._flat[0]
        assert st.calls == steps and st.opt_flat is fl and st.flat_p is fl["p"]
        p0 = next(iter(opt.state))
        assert opt.state[p0]["exp_avg"].data_ptr() >= fl["m"].data_ptr() and opt.state[p0]["exp_avg_sq"].data_ptr() >= fl["v"].data_ptr()
    assert float(opt._flat[0]["step"].item()) == steps
    assert np.abs(np.array(losses) - z["losses"]).max() < 2e-5, (losses, z["losses"])
    # Sign flips, counted from the fixture.  Each Adam update moves an element by at most ~1.002 lr over these three steps (Cauchy-Schwarz
    # on the bias-corrected moments), so an element whose reference gradient sits below another fp32 computation's error can end at most
    # 2.02 * lr * steps from the reference.  Such elements: `gsmall` (0 < |g| < 1e-3 x RMS at some step; tools/make_golden_adam.py), and
    # every element of a parameter whose gradient is rounding noise -- RMS below 1e-3 of the median parameter's, which the fixture shows
    # for exactly the four conv biases in front of a train-mode BatchNorm (exact gradient zero; ~1e-9 against ~3e-4).  A parameter's bar
    # is 2e-4 plus what its flippable elements of the 128-element subsample can do; the running mean behind such a bias carries the
    # bias (0.1 x its offsets of steps 2 and 3: at most 0.61 lr per channel).
    lr = float(z["lr"])
    grms = {k: float(z["grms:" + k].max()) for k in orc.param_shapes(V) if "grms:" + k in z}
    noise = {k for k, r in grms.items() if r < 1e-3 * float(np.median(list(grms.values())))}
    assert noise == {f"decoder.{i}.double_conv.{j}.bias" for i in (1, 3) for j in (0, 3)}, sorted(noise)
    sd = sol.model.state_dict()
    worst, bad, loose = (0.0, None), [], []
    for k in orc.param_shapes(V):
        ref = z["psub:" + k]
        if k in orc.DEAD_PARAMS:
            tol = 1e-6
        else:
            f = 1.0 if k in noise else float(z["gsmall:" + k].max())
            tol = 2e-4 + 2.02 * lr * steps * np.sqrt(f * ref.size) / float(np.linalg.norm(ref))
        e = rel(sub(sd[k], 128), ref)
        if not e < tol:
            bad.append((k, e, tol))
        if e > 2e-4 and k not in orc.DEAD_PARAMS:
            loose.append((k, round(e, 6), round(tol, 6)))
        if k not in orc.DEAD_PARAMS and e > worst[0]:
            worst = (e, k)
    rm_noise = {k.replace(".0.bias", ".1.running_mean").replace(".3.bias", ".4.running_mean") for k in noise}
    for k in orc.buffer_shapes():
        if "running" in k:
            ref = z["buf:" + k]
            tol = 1e-4 + (0.61 * lr * np.sqrt(ref.size) / float(np.linalg.norm(ref)) if k in rm_noise else 0.0)
            e = rel(sd[k], ref)
            if not e < tol:
                bad.append((k, e, tol))
    assert not bad, (bad, loose)
    assert int(sd["decoder.1.double_conv.1.num_batches_tracked"]) == 3 * steps
    import conftest
    conftest.report(f"3-step Adam trajectory vs the reference Solver ({'graphed' if graph else 'eager'}): worst loss "
                    f"{np.abs(np.array(losses) - z['losses']).max():.1e} (bar 2e-5), worst parameter {worst[1]} rel-L2 {worst[0]:.2e}; "
                    f"above 2e-4, within their sign-flip bars: {loose}")


def _run_steps(sol, opt, batches, sched=None, seed0=100):
    for i, b in enumerate(batches):
        random.seed(seed0 + i)
        sol.run_one_epoch([b], "train", opt, collect_views=False)
        if sched is not None:
            sched.step()


def _adam_solver(V, graph, lr=1e-3):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = adam_cfg(V, lr=lr)
    cfg.SOLVER["graph"] = bool(graph)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return sol, get_optimizer(cfg, sol.model.parameters())


def _state(sol, opt):
    fl = opt._flat[0]
    return [fl["p"].clone(), fl["m"].clone(), fl["v"].clone(), fl["step"].clone()] + \
        [v.clone() for k, v in sol.model.named_buffers() if "running" in k]


def test_adam_graphed_equals_eager_across_lr_milestone():
    """Six steps at a launch-bound shape with a MultiStepLR milestone crossed after step 3: the replayed step equals the eager one bit
    for bit (parameters, both moments, step word, BatchNorm statistics), and the learning-rate change re-captures nothing."""
    from electrocardio_panorama_amd import synth
    from torch.optim.lr_scheduler import MultiStepLR
    V, B, L = 3, 2, 512
    batches = [synth.make_batch(B, V, L, seed=40 + i, Q=2) for i in range(6)]
    out = {}
    for graph in (False, True):
        sol, opt = _adam_solver(V, graph)
        sched = MultiStepLR(opt, [3], gamma=0.1)
        _run_steps(sol, opt, batches[:1], sched)
        slot = None
        if graph:
            st = sol._graph_stepper
            assert st is not None and len(st.slots) == 1
            slot = next(iter(st.slots.values()))
        _run_steps(sol, opt, batches[1:], sched, seed0=101)
        if graph:
            assert len(st.slots) == 1 and next(iter(st.slots.values())) is slot      # no re-capture for the new rate
            assert st.lr == pytest.approx(1e-4)
        out[graph] = _state(sol, opt)
    assert float(out[True][3].item()) == 6.0
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)


def test_adam_checkpoint_round_trip_graphed(tmp_path):
    """Graphed: two steps, CheckPointer.save, load into a fresh Solver + FusedAdam, two more steps == four uninterrupted steps, bit for
    bit (h2_state included)."""
    from electrocardio_panorama_amd import synth
    from electrocardio_panorama_amd.utils import CheckPointer
    V, B, L = 3, 2, 512
    batches = [synth.make_batch(B, V, L, seed=60 + i, Q=2) for i in range(4)]
    sol_a, opt_a = _adam_solver(V, True)
    _run_steps(sol_a, opt_a, batches)
    sol_b, opt_b = _adam_solver(V, True)
    _run_steps(sol_b, opt_b, batches[:2])
    CheckPointer(sol_b.model, opt_b, None, str(tmp_path)).save("mid")
    sol_c, opt_c = _adam_solver(V, True)
    CheckPointer(sol_c.model, opt_c, None, str(tmp_path)).load()
    _run_steps(sol_c, opt_c, batches[2:], seed0=102)
    assert sol_c._graph_stepper is not None
    for a, b in zip(_state(sol_a, opt_a), _state(sol_c, opt_c)):
        assert torch.equal(a, b)
    ha, hc = sol_a.model.h2_state(), sol_c.model.h2_state()
    assert sorted(zip(ha["keys"], ha["cur"], ha["nxt"])) == sorted(zip(hc["keys"], hc["cur"], hc["nxt"]))


def test_adam_checkpoint_torch_format():
    """torch.optim.Adam loads FusedAdam's state dict (same keys, shapes, step); FusedAdam resumes from a DataParallelAdam checkpoint."""
    from electrocardio_panorama_amd import synth
    from electrocardio_panorama_amd.solver.optim_scheduler import DataParallelAdam, FusedAdam
    V, B, L = 3, 2, 512
    batches = [synth.make_batch(B, V, L, seed=80 + i, Q=2) for i in range(3)]
    sol, opt = _adam_solver(V, False)
    _run_steps(sol, opt, batches[:2])
    sd = copy.deepcopy(opt.state_dict())
    live = [i for i, s in sd["state"].items() if s]
    assert live and all(set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} for i in live)
    params = list(sol.model.parameters())
    shadow = [torch.nn.Parameter(p.detach().clone()) for p in params]
    tadam = torch.optim.Adam(shadow, lr=1e-3)
    tadam.load_state_dict(sd)
    for i in live:
        s = tadam.state[shadow[i]]
        assert s["step"].dtype == torch.float32 and float(s["step"]) == 2.0
        assert s["exp_avg"].shape == params[i].shape == s["exp_avg_sq"].shape
        assert torch.equal(s["exp_avg"], opt.state[params[i]]["exp_avg"])
    # the other way: two steps of the unfused optimiser, its checkpoint into FusedAdam, one more step of each
    sol_t, opt_t = _adam_solver(V, False)
    opt_t = DataParallelAdam(sol_t.model.parameters(), lr=1e-3)
    _run_steps(sol_t, opt_t, batches[:2])
    sd_t = copy.deepcopy(opt_t.state_dict())
    sol_f, _ = _adam_solver(V, False)
    sol_f.model.load_state_dict(copy.deepcopy(sol_t.model.state_dict()))
    sol_f.model.load_h2_state(copy.deepcopy(sol_t.model.h2_state()))
    opt_f = FusedAdam(sol_f.model.parameters(), lr=1e-3)
    opt_f.load_state_dict(sd_t)
    _run_steps(sol_t, opt_t, batches[2:], seed0=102)
    _run_steps(sol_f, opt_f, batches[2:], seed0=102)
    assert float(opt_f._flat[0]["step"].item()) == 3.0
    pt, pf = dict(sol_t.model.named_parameters()), dict(sol_f.model.named_parameters())
    worst = max(rel(pf[k], pt[k]) for k in pt)
    assert worst <= 1e-5, worst
    for k, p in pt.items():
        s_t, s_f = opt_t.state[p], opt_f.state[pf[k]]
        if "exp_avg" in s_t:
            assert rel(s_f["exp_avg"], s_t["exp_avg"]) <= 1e-5 and rel(s_f["exp_avg_sq"], s_t["exp_avg_sq"]) <= 1e-5, k


def test_adam_step_drops_prepacked_operands():
    """A train-phase forward with no backward leaves pre-packed operands of the old weights in ops._PREPACKED; the FusedAdam update
    writes the weights through raw pointers (no version bump), so it must drop them: the next forward uses the updated weights."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam
    from test_model_gpu import batch_t
    V = 3
    cfg = adam_cfg(V)
    m = hashed_model(V).train()
    m.dropout_p = 0.0
    lossf = build_loss(cfg)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    b = batch_t(2, V, 512, 9, Q=2)

    def loss(model):
        random.seed(9)
        o = model(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
        return lossf(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)

    loss(m)[0].backward()
    loss(m)                         # a train-phase forward (save=True) whose backward never runs
    opt.step()
    assert not ops._PREPACKED
    opt.zero_grad()
    sd, h2 = copy.deepcopy(m.state_dict()), copy.deepcopy(m.h2_state())
    got = loss(m)
    fresh = hashed_model(V).train()
    fresh.dropout_p = 0.0
    fresh.load_state_dict(sd)
    fresh.load_h2_state(h2)
    want = loss(fresh)
    for a, w in zip(got, want):
        assert rel(a.detach(), w.detach()) < 1e-6, (a, w)
