"""GPU: the heavy-tail census of split-fp16 operands (nef_h2_tail_census) and the per-site fp32 route of flagged weight-gradient
sites (ops.H2_TAIL_MODE = "fp32"): census against fp64, the route's accuracy on log-normal operands (plain, affine + ReLU prologue,
polyphase), sites that stay on the split kernels, the whole model with every weight-gradient site routed (golden trajectory, graphed
== eager), and the routes through a checkpoint."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import rel, rnd, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


def g(t):
    return t.to(DEV).contiguous()


def _dist_operand(kind, shape, seed):
    """(tests/test_ops_gpu.py) `lognormal` = exp(4 N(0,1)) with random signs, else uniform [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "lognormal":
        return torch.exp(4.0 * torch.randn(*shape, generator=gen)) * torch.sign(torch.rand(*shape, generator=gen) - 0.5)
    return torch.rand(*shape, generator=gen) * 2 - 1


def _region_err(y, ref64):
    """(tests/test_ops_gpu.py) rel-L2 over all elements, and over the half whose reference magnitude is below the median."""
    y, ref64 = y.double().cpu().reshape(-1), ref64.reshape(-1)
    small = ref64.abs() <= ref64.abs().median()
    return rel(y, ref64), rel(y[small], ref64[small])


def _fringe(shape, seed):
    B, C, T = shape
    xf = rnd(B, C, T, seed=seed)
    xf[:, :, T // 4:] *= torch.pow(0.5, torch.arange(T - T // 4, dtype=torch.float32)).clamp_min(1e-30)
    return xf


@pytest.fixture
def tail_mode():
    """ops.H2_TAIL_MODE / H2_TAIL_FRAC / _H2_MIN_WGS as they were, whatever a test sets."""
    o = ops()
    saved = (o.H2_TAIL_MODE, o.H2_TAIL_FRAC, o._H2_MIN_WGS)
    o.h2_tail_sites(), o.h2_fallback_sites()
    yield o
    o.H2_TAIL_MODE, o.H2_TAIL_FRAC, o._H2_MIN_WGS = saved
    o.h2_tail_sites(), o.h2_fallback_sites()


def _want_census(v, amax):
    """fp64 census of the values `v` (the operand after its prologue / scale) against the fp32 word `amax`."""
    a = v.double().abs().reshape(-1)
    thr = float(torch.tensor(amax, dtype=torch.float32) * torch.tensor(2.0 ** -11, dtype=torch.float32))
    nz, small = a > 0, (a > 0) & (a < thr)
    e = a * a
    return int(nz.sum()), int(small.sum()), float(e[small].sum() / e.sum())


def test_census_matches_fp64():
    """nef_h2_tail_census against fp64 torch on the operand as a launch reads it: a dense view, a z1 / z2-style half view (the
    other half, 10^6 x larger and uniform, must not be seen), an in_scale operand and an affine + ReLU prologue (two passes).
    Counts equal, energy fractions within 1e-6, flag = count fraction > H2_TAIL_FRAC."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    B, G, C, T = 4, 2, 128, 384
    x = _dist_operand("lognormal", (B, G * C, T), 900)
    cases = []
    cases.append(("dense", GV.dense(g(x), G), None, None, x))
    V = 3      # half view: channels [64, 128) of every lead of a [B, 128 V, T] tensor
    full = _dist_operand("uniform", (B, 128 * V, T), 901) * 1e6
    lv = _dist_operand("lognormal", (B, V, 64, T), 902)
    full.view(B, V, 128, T)[:, :, 64:] = lv
    cases.append(("half", GV.half(g(full), V, 1), None, None, lv))
    s = torch.rand(B, G * C, generator=torch.Generator().manual_seed(903)) * 3 + 0.1
    cases.append(("in_scale", GV.dense(g(x), G), (g(s), G * C, C), None, x * s[:, :, None]))
    P = 2
    pa = torch.rand(P, G * C, generator=torch.Generator().manual_seed(904)) + 0.5
    pb = torch.randn(P, G * C, generator=torch.Generator().manual_seed(905)) * 1e-3
    xp = torch.relu(torch.addcmul(pb.repeat_interleave(B // P, 0)[:, :, None], x, pa.repeat_interleave(B // P, 0)[:, :, None]))
    cases.append(("affine", GV.dense(g(x), G), None, (1, g(pa), g(pb), B // P), xp))
    for name, xv, sc, pro, vals in cases:
        amax = float(vals.abs().max())
        rec = o.census_record(o.tail_census(xv, g(torch.tensor([amax])), in_scale=sc, pro=pro))
        nz, ns, ef = _want_census(vals, amax)
        assert (rec["n_nonzero"], rec["n_small"]) == (nz, ns), (name, rec, nz, ns)
        assert abs(rec["frac_energy"] - ef) < 1e-6, (name, rec, ef)
        assert abs(rec["e_small"] / rec["e_total"] - ef) < 1e-6, (name, rec, ef)
        assert rec["flag"] == int(ns / nz > o.H2_TAIL_FRAC), (name, rec)
        assert rec["flag"] == 1, name      # (log-normal values: 99 % below the window)
    # uniform operand: nothing below the window worth a flag
    u = _dist_operand("uniform", (B, G * C, T), 906)
    rec = o.census_record(o.tail_census(GV.dense(g(u), G), g(torch.tensor([float(u.abs().max())]))))
    nz, ns, ef = _want_census(u, float(u.abs().max()))
    assert (rec["n_nonzero"], rec["n_small"], rec["flag"]) == (nz, ns, 0) and abs(rec["frac_energy"] - ef) < 1e-6


def _affine(B, C, P, seed):
    pa = torch.rand(P, C, generator=torch.Generator().manual_seed(seed)) + 0.5
    pb = torch.randn(P, C, generator=torch.Generator().manual_seed(seed + 1)) * 1e-3
    return pa, pb


def _apply_affine(x, pa, pb, Bp):
    return torch.relu(x * pa.repeat_interleave(Bp, 0)[:, :, None] + pb.repeat_interleave(Bp, 0)[:, :, None])


@pytest.mark.parametrize("K,aff", [(3, False), (3, True), (7, False)], ids=["K3", "K3-affine", "K7"])
def test_fallback_fixes_heavy_tailed_weight_gradient(tail_mode, K, aff):
    """H2_TAIL_MODE = "fp32": a scoped weight-gradient site on log-normal operands is flagged at its measuring launch and runs on the
    direct fp32 kernel, conv_bwd_weight(h2=False, wino=False) -- bit for bit, at that launch and every later one; its small-half
    rel-L2 against fp64 is within 3 x torch fp32's own (the split kernels: ~5e-3; the transposed-Winograd fp32 form: 2.3e-4).
    h2_fallback_sites() counts the site.  (K = 7 has no split-fp16 form with a prologue.)"""
    o = tail_mode
    from electrocardio_panorama_amd.ops import GV
    o.H2_TAIL_MODE = "fp32"
    B, G, C, T, P = 6, 2, 128, 512, 2
    x = _dist_operand("lognormal", (B, G * C, T), 910 + K)
    gy = _dist_operand("lognormal", (B, G * C, T), 911 + K)
    w = rnd(G * C, C, K, seed=912, scale=0.05)
    pro, xe = None, x
    if aff:
        pa, pb = _affine(B, G * C, P, 913)
        pro, xe = (1, g(pa), g(pb), B // P), _apply_affine(x, pa, pb, B // P)
    w64 = torch.nn.grad.conv1d_weight(xe.double(), w.shape, gy.double(), padding=K // 2, groups=G)
    w32 = _region_err(torch.nn.grad.conv1d_weight(xe, w.shape, gy, padding=K // 2, groups=G), w64)
    xv, gv, wd = GV.dense(g(x), G), GV.dense(g(gy), G), g(w)
    with o.amax_scope((o.new_amax_scope(), True)):
        gw = o.conv_bwd_weight(xv, gv, K, pro=pro, site=wd.data_ptr(), h2=True)
        o.amax_roll()      # (next pass: the same site again)
        gw2 = o.conv_bwd_weight(xv, gv, K, pro=pro, site=wd.data_ptr(), h2=True)
    ref32 = o.conv_bwd_weight(xv, gv, K, pro=pro, h2=False, wino=False)
    assert torch.equal(gw, ref32) and torch.equal(gw2, ref32)
    assert o.h2_fallback_sites() == 1 and o.h2_tail_sites() == 1
    e = _region_err(gw, w64)
    import conftest
    conftest.report(f"fp32 route, log-normal weight gradient K={K}{' affine' if aff else ''}: flat / small-half rel-L2 {e[0]:.1e} / "
                    f"{e[1]:.1e} (torch fp32 {w32[0]:.1e} / {w32[1]:.1e})")
    assert e[0] <= 3 * w32[0] + 1e-12 and e[1] <= 3 * w32[1] + 1e-12, (e, w32)


def _upsample2(x):
    return F.interpolate(x, scale_factor=2, mode="linear", align_corners=False)


def test_fallback_polyphase_weight_gradient(tail_mode):
    """The polyphase weight gradient (conv_bwd_weight_poly, prologue mode 4 | affine: the half-resolution window continued with
    x'[0] / x'[T-1]) of a flagged site runs on the fp32 kernel + the row-end terms (nef_bwd_weight_clamp_ends), then the fold:
    flat and small-half error at fp32 level against fp64, and equal to the non-polyphase (direct) fp32 weight gradient of
    conv1d(upsample2(x), w) within 3 x fp32's error."""
    o = tail_mode
    from electrocardio_panorama_amd.ops import GV
    o.H2_TAIL_MODE = "fp32"
    B, G, Cog, Cig, T, P = 4, 1, 64, 128, 512, 2
    Th = T // 2
    x = _dist_operand("lognormal", (B, G * Cig, Th), 920)
    gy = _dist_operand("lognormal", (B, G * Cog, T), 921)
    pa, pb = _affine(B, G * Cig, P, 922)
    xp = _apply_affine(x, pa, pb, B // P)
    w_shape = (G * Cog, Cig, 3)
    w64 = torch.nn.grad.conv1d_weight(_upsample2(xp.double()), w_shape, gy.double(), padding=1, groups=G)
    w32 = _region_err(torch.nn.grad.conv1d_weight(_upsample2(xp), w_shape, gy, padding=1, groups=G), w64)
    gy_pm = gy.view(B, G * Cog, Th, 2).permute(0, 1, 3, 2).reshape(B, G * 2 * Cog, Th)     # row 2 co + p = positions 2 m + p
    xedge = torch.stack([xp[:, :, 0], xp[:, :, -1]], dim=2)
    pro = (3, g(pa), g(pb), B // P)
    site = g(torch.zeros(1))
    with o.amax_scope((o.new_amax_scope(), True)):
        gw = o.conv_bwd_weight_poly(GV.dense(g(x), G), g(gy_pm), Cog, pro, g(xedge), site=site.data_ptr())
    assert o.h2_fallback_sites() == 1
    e = _region_err(gw, w64)
    plain32 = o.conv_bwd_weight(GV.dense(g(x), G), GV.dense(g(gy), G), 3, pro=pro, h2=False, wino=False)
    d = rel(gw.double().cpu(), plain32.double().cpu())
    import conftest
    conftest.report(f"fp32 route, polyphase weight gradient on log-normal operands: flat / small-half rel-L2 {e[0]:.1e} / {e[1]:.1e} "
                    f"(torch fp32 {w32[0]:.1e} / {w32[1]:.1e}); vs the non-polyphase fp32 gradient {d:.1e}")
    assert e[0] <= 3 * w32[0] + 1e-12 and e[1] <= 3 * w32[1] + 1e-12, (e, w32)
    assert d <= 3 * w32[0] + 1e-12, (d, w32)


def test_unflagged_sites_do_not_move(tail_mode):
    """Uniform, ReLU and decaying-fringe operands in "fp32" mode: the same bits as in "warn" mode and no site routed.  In "warn" mode
    a log-normal site counts in h2_tail_sites(), not in h2_fallback_sites(), and keeps the split kernels."""
    o = tail_mode
    from electrocardio_panorama_amd.ops import GV
    B, G, C, T, K = 4, 1, 128, 512, 3
    w = g(rnd(G * C, C, K, seed=931, scale=0.05))

    def run(mode, x, gy):
        o.H2_TAIL_MODE = mode
        with o.amax_scope((o.new_amax_scope(), True)):
            return o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), K, site=w.data_ptr(), h2=True)

    for kind in ("uniform", "relu", "fringe"):
        if kind == "fringe":
            x = g(_fringe((B, G * C, T), 935))
        else:
            x = g(F.relu(rnd(B, G * C, T, seed=934)) if kind == "relu" else _dist_operand(kind, (B, G * C, T), 932))
        gy = g(_dist_operand("uniform", (B, G * C, T), 933))
        a, b = run("fp32", x, gy), run("warn", x, gy)
        assert torch.equal(a, b), kind
        assert o.h2_fallback_sites() == 0 and o.h2_tail_sites() == 0, kind
    x, gy = g(_dist_operand("lognormal", (B, G * C, T), 936)), g(_dist_operand("lognormal", (B, G * C, T), 937))
    gw = run("warn", x, gy)
    assert o.h2_tail_sites() == 1 and o.h2_fallback_sites() == 0
    assert not torch.equal(gw, o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), K, h2=False))      # (split kernels)
    o.H2_TAIL_MODE = "sometimes"
    with pytest.raises(ValueError):
        with o.amax_scope((o.new_amax_scope(), True)):
            o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), K, site=w.data_ptr(), h2=True)


def _force_every_route(o):
    """Split-fp16 kernels wherever their shapes allow (as test_model_gpu's `h2` param) and every weight-gradient site routed: the
    count-fraction bar below 0 flags every operand, even one without a single element below the window."""
    o._H2_MIN_WGS = 0
    o.H2_TAIL_MODE = "fp32"
    o.H2_TAIL_FRAC = -1.0


def _routed_total(o):
    """Sites routed since the start of the process (h2_fallback_sites() without the reset of its last reader)."""
    return sum(st["fallback"] for st in o._AMAX.values())


def _bww_sites(blob):
    return [k for k in blob["keys"] if k[2] == "conv_bwd_weight"]


def test_model_every_weight_gradient_site_routed(tail_mode, golden_dir):
    """The whole model with every weight-gradient site on the fp32 route: the 3-step SGD trajectory against the reference Solver's
    (tests/golden/sgd_*.npz) within test_sgd_steps_golden's bars, eagerly and through the captured step (routes decided by the
    stepper's eager first step), the two bit-identical; h2_fallback_sites() = the step's weight-gradient sites."""
    o = tail_mode
    from electrocardio_panorama_amd import synth
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    from test_model_gpu import golden, make_cfg
    _force_every_route(o)
    z = np.load(golden(golden_dir, "sgd_*.npz")[0])
    B, V, L, seed, steps = (int(z[k]) for k in ("B", "V", "L", "seed", "steps"))
    finals = []
    for graph in (False, True):
        cfg = make_cfg(V, lr=float(z["lr"]))
        cfg.SOLVER["graph"] = graph
        sol = Solver(cfg, use_tensorboardx=False)
        sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
        sol.model.dropout_p = 0.0
        batches = [synth.make_batch(B, V, L, seed=seed + s, Q=2) for s in range(steps)]
        opt = get_optimizer(cfg, sol.model.parameters())
        moved0 = _routed_total(o)
        random.seed(seed)
        losses = sol.run_one_epoch(batches, "train", opt, collect_views=not graph)[0]
        assert (getattr(sol, "_graph_stepper", None) is not None) == graph
        blob = sol.model.h2_state()
        n_bww = len(_bww_sites(blob))
        assert n_bww > 10 and all(r for k, r in zip(blob["keys"], blob["fp32"]) if k[2] == "conv_bwd_weight"), blob["fp32"]
        assert not any(r for k, r in zip(blob["keys"], blob["fp32"]) if k[2] != "conv_bwd_weight")
        moved = _routed_total(o) - moved0      # (Solver's epoch check has read h2_fallback_sites() already: the running total)
        assert moved == n_bww, (graph, moved, n_bww)      # (graphed: the stepper's eager probe decides them, the captures reuse them)
        assert np.abs(np.array(losses) - z["losses"]).max() < 2e-5, (losses, z["losses"])
        sd = sol.model.state_dict()
        for k in orc.param_shapes(V):
            tol = 1e-6 if k in orc.DEAD_PARAMS else 2e-4
            assert rel(sub(sd[k], 128), z["psub:" + k]) < tol, (graph, k)
        finals.append(({k: v.detach().clone() for k, v in sd.items()}, np.array(losses)))
    assert np.array_equal(finals[0][1], finals[1][1])
    for k in finals[0][0]:
        assert torch.equal(finals[0][0][k], finals[1][0][k]), k


def test_checkpoint_carries_routes(tail_mode, tmp_path):
    """CheckPointer.save / load (torch.load with its default weights_only) carries the routes (h2_state version 2): the restored
    graphed stepper equals the running one in losses and every parameter, bit for bit, with the same routes.  A version-1 blob
    still loads: its sites are ready and keep the split kernels.  A "warn" process loading a version-2 blob keeps the split
    kernels and counts the flagged sites in h2_tail_sites()."""
    o = tail_mode
    from electrocardio_panorama_amd import synth
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.utils.checkpointer import CheckPointer
    from test_model_gpu import hashed_model, make_cfg
    _force_every_route(o)
    V, B, L = 3, 4, 512
    cfg = make_cfg(V, lr=0.05)
    batches = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in synth.make_batch(B, V, L, seed=80 + i).items()}
               for i in range(4)]
    mg = hashed_model(V).train()
    mg.dropout_p = 0.0
    step = GraphedTrainStep(mg, cfg)
    random.seed(5)
    for b in batches[:3]:
        step(b["data"], b["input_theta"], b["target_theta"], b["rois"], b["target_view"])
    blob = mg.h2_state()
    assert blob["version"] == 2 and len(_bww_sites(blob)) > 10
    CheckPointer(mg, save_dir=str(tmp_path)).save("c")
    m2 = hashed_model(V).train()
    m2.dropout_p = 0.0
    CheckPointer(m2, save_dir=str(tmp_path)).load()
    assert m2.h2_state()["fp32"] == blob["fp32"] and m2.h2_state()["keys"] == blob["keys"]
    step2 = GraphedTrainStep(m2, cfg)
    step2.load_state_dict(step.state_dict())
    b = batches[3]
    st = random.getstate()
    l_a = step(b["data"], b["input_theta"], b["target_theta"], b["rois"], b["target_view"]).clone()
    random.setstate(st)
    l_b = step2(b["data"], b["input_theta"], b["target_theta"], b["rois"], b["target_view"]).clone()
    assert torch.equal(l_a, l_b), (l_a, l_b)
    p2 = dict(m2.named_parameters())
    for k, p in mg.named_parameters():
        assert torch.equal(p2[k], p), k
    # version 1: magnitudes only -- every site ready, none routed (split kernels, as before routes existed)
    v1 = {"version": 1, "keys": copy.deepcopy(blob["keys"]), "cur": copy.deepcopy(blob["cur"]), "nxt": copy.deepcopy(blob["nxt"])}
    m3 = hashed_model(V).train()
    m3.load_state_dict(copy.deepcopy(mg.state_dict()))
    assert m3.load_h2_state(v1) == len(blob["keys"])
    b3 = m3.h2_state()
    assert b3["version"] == 1 and b3["keys"] == blob["keys"] and not any(b3.get("fp32", []))
    # version 2 in a "warn" process: the routes are not taken up (split kernels), the flagged sites count in h2_tail_sites()
    o.H2_TAIL_MODE = "warn"
    o.h2_tail_sites(), o.h2_fallback_sites()
    m4 = hashed_model(V).train()
    m4.load_state_dict(copy.deepcopy(mg.state_dict()))
    assert m4.load_h2_state(copy.deepcopy(blob)) == len(blob["keys"])
    assert not any(m4.h2_state().get("fp32", [])) and o.h2_fallback_sites() == 0 and o.h2_tail_sites() == sum(blob["fp32"])
