"""Several target views per train step on the GPU (SOLVER.train_views): the nef_copy_many entry bit for bit against copy_ / add_, the
multi-view engine path against Q single-view steps of the existing path (outputs and BatchNorm buffers bit for bit, gradients against
their fp64 mean at the project's bars) and against the CPU oracle, the replayed step against the eager one, and Solver epochs."""
import random
import types

import numpy as np
import pytest
import torch

from decisions import FLAT_TOL, TENSOR_TOL, assert_grad_parity
from util import FWD_TOL, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Cfg(dict):
    __getattr__ = dict.__getitem__


def make_cfg(V, lr=0.1, **solver):
    cfg = Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""),
              DATA=Cfg(lead_num=V, noise=False, synthetic=True),
              SOLVER=Cfg(optim="sgd", lr=lr, scheduler="MultiStep", lr_step=[50, 100], reg_loss="l1_loss",
                         loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], epochs=1),
              output_dir="/tmp/nef_test", desc="debug", seed=7)
    cfg.SOLVER.update(solver)
    return cfg


# ------------------------------------------------------------------------------------------------ 1. nef_copy_many
SIZES = (0, 1, 3, 4, 5, 1023, 4097)


def _segments(sizes, s_off, d_off, seed):
    """Per segment: (source slice, destination slice, the destination's whole storage), each slice `off` elements behind a
    16-byte-aligned address."""
    g = torch.Generator().manual_seed(seed)
    segs = []
    for n in sizes:
        s = torch.randn(n + 12, generator=g).to(DEV)
        d = torch.randn(n + 12, generator=g).to(DEV)
        assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
        segs.append((s[4 + s_off:4 + s_off + n], d[4 + d_off:4 + d_off + n], d))
    return segs


@pytest.mark.parametrize("accumulate", [False, True], ids=["assign", "add"])
@pytest.mark.parametrize("s_off,d_off", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["aligned", "src+1", "dst+1", "both+1"])
def test_copy_many_matches_torch_bit_for_bit(s_off, d_off, accumulate):
    from electrocardio_panorama_amd import ops
    segs = _segments(SIZES, s_off, d_off, 3)
    want = []
    for s, d, whole in segs:
        w = whole.clone()
        view = w[4 + d_off:4 + d_off + s.numel()]
        view.add_(s) if accumulate else view.copy_(s)
        want.append(w)
    ops.copy_many([s for s, _, _ in segs], [d for _, d, _ in segs], accumulate=accumulate)
    torch.cuda.synchronize()
    for (s, d, whole), w in zip(segs, want):
        assert torch.equal(whole, w), (s.numel(), s_off, d_off)        # the segment's bits, and nothing beside it was touched


@pytest.mark.parametrize("accumulate", [False, True], ids=["assign", "add"])
def test_copy_many_130_segments_take_three_launches(accumulate, monkeypatch):
    from electrocardio_panorama_amd import _lib, ops
    sizes = [(7 * i) % 61 + (4097 if i in (3, 64, 129) else 0) for i in range(130)]
    segs = _segments(sizes, 1, 0, 5)
    want = []
    for s, d, whole in segs:
        w = whole.clone()
        view = w[4:4 + s.numel()]
        view.add_(s) if accumulate else view.copy_(s)
        want.append(w)
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what="": (calls.append(what), real(rc, what))[1])
    ops.copy_many([s for s, _, _ in segs], [d for _, d, _ in segs], accumulate=accumulate)
    torch.cuda.synchronize()
    assert calls == ["nef_copy_many"]                      # one entry call (the library splits it into ceil(130 / 64) = 3 launches)
    for (s, d, whole), w in zip(segs, want):
        assert torch.equal(whole, w)
    with pytest.raises(ValueError):
        ops.copy_many([segs[0][0]], [segs[1][1]])          # sizes differ
    with pytest.raises(ValueError):
        ops.copy_many([segs[0][0]], [])


# ------------------------------------------------------------------------------------------------ 2. the engine
def hashed_model(V):
    from electrocardio_panorama_amd.network import build_model
    from oracle import hashweights as hw
    m = build_model(make_cfg(V)).float()
    m.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    return m.to(DEV)


def batch_t(B, V, L, seed, Q):
    from electrocardio_panorama_amd import synth
    b = synth.make_batch(B, V, L, seed=seed, Q=Q)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}


def _views_of(b, Q):
    """The batch's first Q rest views as the step's targets [Q, B, 1, L] and query angles [Q, B, 2] (distinct angles per view)."""
    from electrocardio_panorama_amd.views import select_views
    return select_views(b["rest_view"], b["rest_theta"], list(range(Q)))


_REF = {}


def _single_view_reference(B, V, L, Q, seed, path):
    """Q single-view train steps of the EXISTING path at one set of dropout masks and one Standin draw, run in view order on one model:
    per-view outputs, the BatchNorm buffers behind the Q forwards, and the fp64 mean of the Q gradients.  Computed once per case and
    conv path, shared by the tests below and left unchanged."""
    key = (B, V, L, Q, seed, path)
    if key in _REF:
        return _REF[key]
    from electrocardio_panorama_amd.network import build_loss
    from oracle import hashweights as hw
    cfg = make_cfg(V)
    b = batch_t(B, V, L, seed, Q)
    tv, th = _views_of(b, Q)
    m = hashed_model(V).train()
    m.dropout_masks = {k: v.to(DEV) for k, v in hw.hashed_masks(V, B, L // 4).items()}
    outs, gsum = [], None
    for k in range(Q):
        random.seed(seed)                                  # the same Standin draw for every view
        o = m(b["data"], b["input_theta"], th[k], b["rois"], phase="train")
        losses = build_loss(cfg)(o[0], o[1], o[2], tv[k], cfg)
        m.zero_grad()
        losses[0].backward()
        g = {n: (p.grad.double().clone() if p.grad is not None else None) for n, p in m.named_parameters()}
        gsum = g if gsum is None else {n: (None if g[n] is None else gsum[n] + g[n]) for n in g}
        outs.append(tuple(t.detach().clone() for t in o))
    torch.cuda.synchronize()
    ref = dict(outs=outs, buffers={n: v.detach().clone() for n, v in m.named_buffers()},
               grads={n: (None if v is None else (v / Q).cpu()) for n, v in gsum.items()}, batch=b, tv=tv, th=th)
    _REF[key] = ref
    return ref


def _multi_view_step(B, V, L, Q, seed, ref):
    from electrocardio_panorama_amd.network import build_loss
    from oracle import hashweights as hw
    cfg = make_cfg(V)
    b = ref["batch"]
    m = hashed_model(V).train()
    m.dropout_masks = {k: v.to(DEV) for k, v in hw.hashed_masks(V, B, L // 4).items()}
    random.seed(seed)
    o = m(b["data"], b["input_theta"], ref["th"], b["rois"], phase="train")
    losses = build_loss(cfg)(o[0], o[1], o[2], ref["tv"], cfg)
    losses[0].backward()
    torch.cuda.synchronize()
    return m, o, losses


CASES = [(2, 3, 512, 3), (2, 1, 128, 2), (1, 3, 7808, 2)]
CASE_IDS = ["unpool_fused_B2_V3_L512_Q3", "unfused_decoder_B2_V1_L128_Q2", "two_pass_bwd_B1_V3_L7808_Q2"]


def _check_grads(m, ref, B, L, Q):
    named = {n: p.grad for n, p in m.named_parameters()}
    dead = [n for n, g in ref["grads"].items() if g is None]
    P_ref = {n: types.SimpleNamespace(grad=g) for n, g in ref["grads"].items()}
    for n in dead:
        P_ref[n] = types.SimpleNamespace(grad=None)
    assert_grad_parity(named, P_ref, dead=dead, flat_tol=FLAT_TOL, tensor_tol=TENSOR_TOL, n_terms=3.0 * Q * B * L)
    got = torch.cat([named[n].double().cpu().reshape(-1) for n in named if named[n] is not None])
    want = torch.cat([ref["grads"][n].reshape(-1) for n in named if named[n] is not None])
    return rel(got, want)


@pytest.mark.parametrize("B,V,L,Q", CASES, ids=CASE_IDS)
def test_multi_view_step_on_fp32_kernels(B, V, L, Q, monkeypatch):
    """fp32 kernels (ops.H2 off), fixed dropout masks and Standin draw: outs[k] and the BatchNorm buffers are bit-identical to Q single-view
    train forwards in view order (num_batches_tracked = 3Q), every gradient sits inside FLAT_TOL / TENSOR_TOL of the fp64 mean of the Q
    single-view gradients of the existing path."""
    from electrocardio_panorama_amd import ops
    monkeypatch.setattr(ops, "H2", False)
    seed = 11
    ref = _single_view_reference(B, V, L, Q, seed, "fp32")
    m, o, losses = _multi_view_step(B, V, L, Q, seed, ref)
    assert len(losses) == 4
    assert all(t.shape == (Q, B, 1, L) and t.is_contiguous() for t in o)
    assert o[1].data_ptr() == o[0].data_ptr() + 4 * o[0].numel() and o[2].data_ptr() == o[1].data_ptr() + 4 * o[1].numel()
    for k in range(Q):
        for got, want in zip(o, ref["outs"][k]):
            assert torch.equal(got[k], want), k
    if Q > 1:
        assert not torch.equal(o[0][0], o[0][1])           # the views differ
    bufs = dict(m.named_buffers())
    for n, v in ref["buffers"].items():
        assert torch.equal(bufs[n], v), n
    assert int(bufs["decoder.1.double_conv.1.num_batches_tracked"]) == 3 * Q
    flat = _check_grads(m, ref, B, L, Q)
    print(f"multi-view (B={B}, V={V}, L={L}, Q={Q}), fp32 kernels: flat gradient vs the fp64 mean of {Q} single-view steps {flat:.2e} (bar {FLAT_TOL:g})")


@pytest.mark.parametrize("B,V,L,Q", CASES, ids=CASE_IDS)
def test_multi_view_step_on_split_fp16_convs(B, V, L, Q, monkeypatch):
    """The same with the split-fp16 convs forced wherever their shape rules hold: outputs within FWD_TOL of the single-view outputs, the
    gradients inside the same two bars."""
    from electrocardio_panorama_amd import ops
    monkeypatch.setattr(ops, "_H2_MIN_WGS", 0)
    seed = 11
    ref = _single_view_reference(B, V, L, Q, seed, "h2")
    m, o, losses = _multi_view_step(B, V, L, Q, seed, ref)
    for k in range(Q):
        for got, want in zip(o, ref["outs"][k]):
            e = rel(got[k], want)
            assert e < FWD_TOL, (k, e)
    bufs = dict(m.named_buffers())
    assert int(bufs["decoder.1.double_conv.1.num_batches_tracked"]) == 3 * Q
    flat = _check_grads(m, ref, B, L, Q)
    print(f"multi-view (B={B}, V={V}, L={L}, Q={Q}), split-fp16 convs: flat gradient vs the fp64 mean of {Q} single-view steps {flat:.2e} (bar {FLAT_TOL:g})")


def test_multi_view_forward_against_the_oracle(monkeypatch):
    """outs[k] against oracle.forward with theta_k at the same masks and Standin draw (B=2, V=3, L=512, Q=3, fp32 kernels)."""
    from electrocardio_panorama_amd import ops
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    monkeypatch.setattr(ops, "H2", False)
    B, V, L, Q, seed = 2, 3, 512, 3, 11
    ref = _single_view_reference(B, V, L, Q, seed, "fp32")
    m, o, _ = _multi_view_step(B, V, L, Q, seed, ref)
    random.seed(seed)
    choice = (random.randint(0, V - 1), random.randint(0, V - 1))
    masks = hw.hashed_masks(V, B, L // 4)
    b = {k: v.cpu() for k, v in ref["batch"].items()}
    th = ref["th"].cpu()
    with torch.no_grad():
        for k in range(Q):
            want = orc.forward(hw.hashed_params(V), hw.hashed_buffers(), b["data"], b["input_theta"], th[k], b["rois"], phase="train",
                               training=True, masks=masks, p=0.2, lead_choice=choice)
            for got, w, name in zip(o, want, ("out", "shuffle_p", "shuffle_l")):
                e = rel(got[k], w)
                assert e < FWD_TOL, (k, name, e)


def test_3d_query_is_the_train_phase_of_model_nefnet_only():
    from electrocardio_panorama_amd.network.model_nefnet import Model_nefnet2
    b = batch_t(2, 3, 512, 1, 3)
    tv, th = _views_of(b, 2)
    m = hashed_model(3).eval()
    for phase in ("val", "test", "gen"):
        with pytest.raises(ValueError, match="query_theta"):
            m(b["data"], b["input_theta"], th, b["rois"], rest_theta=b["rest_theta"], phase=phase)
    m2 = Model_nefnet2(1, 3).to(DEV).train()
    with pytest.raises(ValueError, match="query_theta"):
        m2(b["data"], b["input_theta"], th, b["rois"], phase="train")


# ------------------------------------------------------------------------------------------------ 3. graphed == eager
def _batches(n, B, V, L, seed0, n_rest=5):
    from electrocardio_panorama_amd import synth
    return [dict(synth.make_batch(B, V, L, seed=seed0 + s, Q=n_rest)) for s in range(n)]


def _solver(V, optim, graph, accum=1, **keys):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr={"sgd": 0.1, "adam": 1e-3}[optim], optim=optim, graph=bool(graph), **keys)
    if accum > 1:
        cfg.SOLVER["accum_steps"] = accum
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


_SLOTS = {"sgd": ("buf",), "adam": ("m", "v", "step")}


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + [v.clone() for k, v in sol.model.named_buffers()]


@pytest.mark.parametrize("optim,ssim,accum", [("sgd", 0.0, 1), ("adam", 0.0, 1), ("sgd", 0.5, 1), ("sgd", 0.0, 2)],
                         ids=["sgd", "adam", "sgd_ssim_crop", "sgd_accum2"])
def test_views_graphed_equals_eager(optim, ssim, accum):
    """Three steps at (B=2, V=3, L=512) with train_views 3 of 5 supervised rest views: the replayed step equals the eager one bit for bit
    -- parameters, optimiser state, BatchNorm buffers, loss rows -- from one capture."""
    V, B, L, Q = 3, 2, 512, 3
    batches = _batches(3, B, V, L, 40)
    keys = dict(train_views=Q)
    if ssim:
        keys.update(ssim_factor=ssim, ssim_crop=True)
    out = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(V, optim, graph, accum=accum, **keys)
        random.seed(100)
        rows = np.array(sol.run_one_epoch(batches, "train", opt, collect_views=False)[0])
        assert rows.shape == (3, 5 if ssim else 4) and np.isfinite(rows).all()
        st = getattr(sol, "_graph_stepper", None)
        assert (st is not None) == graph
        if graph:
            assert len(st.slots) == 1 and st.calls == 3 and st.q_theta.shape == (Q, B, 2) and st.target.shape == (Q, B, 1, L)
        assert int(dict(sol.model.named_buffers())["decoder.1.double_conv.1.num_batches_tracked"]) == 3 * Q * 3
        out[graph] = (_state(sol, opt, optim), rows)
    for a, b in zip(out[False][0], out[True][0]):
        assert torch.equal(a, b)
    assert np.array_equal(out[False][1], out[True][1])


def test_collected_views_of_a_train_epoch_carry_all_views():
    V, B, L, Q = 3, 2, 512, 2
    cfg, sol, opt = _solver(V, "sgd", False, train_views=Q)
    random.seed(100)
    res = sol.run_one_epoch(_batches(2, B, V, L, 40), "train", opt, collect_views=True)
    gt, pred = res[1], res[2]
    assert len(gt) == len(pred) == 2 and all(a.shape == (Q, B, L) for a in gt) and all(a.shape == (Q, B, L) for a in pred)


# ------------------------------------------------------------------------------------------------ 4. Solver on SyntheticLoader
def _loader_solver(graph, tmp=None):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from electrocardio_panorama_amd.train_net import SyntheticLoader
    V = 3
    cfg = make_cfg(V, graph=bool(graph), train_views=3)
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters()), SyntheticLoader(cfg, batch_size=4, n_batches=2, length=512, seed=cfg.seed)


def _epoch(sol, opt, dl, epoch):
    sol.model.dropout_epoch = epoch
    random.seed(100 + epoch)
    return np.array(sol.run_one_epoch(dl, "train", opt, collect_views=False)[0])


def test_solver_epochs_on_the_synthetic_loader_and_a_resumed_epoch():
    """B=4, L=512, 2 batches, train_views 3 of the 9 rest views: an eager and a graphed epoch give the same 4-element rows and parameters;
    the parameters move; a second epoch run by a fresh Solver from the first epoch's state equals the uninterrupted second epoch bit for
    bit (the view draw is a function of (seed, epoch, batch index), not of any state)."""
    cfg, sol_e, opt_e, dl = _loader_solver(False)
    p0 = {n: p.detach().clone() for n, p in sol_e.model.named_parameters()}
    rows_e = _epoch(sol_e, opt_e, dl, 0)
    cfg, sol_g, opt_g, dl = _loader_solver(True)
    rows_g = _epoch(sol_g, opt_g, dl, 0)
    assert rows_e.shape == rows_g.shape == (2, 4) and np.array_equal(rows_e, rows_g)
    assert sol_g._graph_stepper is not None and getattr(sol_e, "_graph_stepper", None) is None
    moved = [n for n, p in sol_g.model.named_parameters() if not torch.equal(p.detach(), p0[n])]
    assert len(moved) > 40
    for (n, a), (_, b) in zip(sol_e.model.named_parameters(), sol_g.model.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    # the checkpoint's content behind epoch 0, then the uninterrupted epoch 1
    model_sd = {k: v.detach().clone() for k, v in sol_g.model.state_dict().items()}
    h2_blob = sol_g.model.h2_state()
    opt_sd = opt_g.state_dict()
    opt_sd = {"state": {k: {kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in opt_sd["state"].items()},
              "param_groups": opt_sd["param_groups"]}
    rows_1 = _epoch(sol_g, opt_g, dl, 1)
    cfg, sol_r, opt_r, dl = _loader_solver(True)
    sol_r.model.load_state_dict(model_sd)
    sol_r.model.load_h2_state(h2_blob)
    opt_r.load_state_dict(opt_sd)
    rows_r = _epoch(sol_r, opt_r, dl, 1)
    assert np.array_equal(rows_1, rows_r)
    for (n, a), (_, b) in zip(sol_g.model.state_dict().items(), sol_r.model.state_dict().items()):
        assert torch.equal(a, b), n
    # the draw differs between the epochs (3 of 9, two batches each): the resumed epoch did not replay epoch 0's views
    from electrocardio_panorama_amd.views import draw_views
    assert [draw_views(cfg.seed, 0, i, 3, 9) for i in range(2)] != [draw_views(cfg.seed, 1, i, 3, 9) for i in range(2)]
