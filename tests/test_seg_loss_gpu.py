"""The wave-segment weights of the reconstruction term (SOLVER.seg_weights; nef_loss_seg_fwd / nef_loss_seg_bwd) and the per-segment squared
error of the test phase (SOLVER.seg_eval; nef_view_seg_metrics) on the device: the three kernels against the restatement tests/seg_ref.py
on the golden rois and on adversarial rows, losswrapper through autograd on the model's own output, graph replay against the eager step
bit for bit, the Solver's per-segment PSNR against a host computation, and the keys off."""
import os
import random

import numpy as np
import pytest
import torch

import seg_ref
from test_model_gpu import DEV, Cfg, batch_t, hashed_model

pytestmark = pytest.mark.gpu

FACTORS = (0.5, 0.5, 0.75)
W_DISTINCT = (0.5, 1.25, 3.0, 2.0, 0.75, 1.5, 0.25)      # every bin its own weight: a position in the wrong bin shows
W_QRS = (1.0, 1.0, 3.0, 2.0, 1.0, 1.0, 0.0)
ONES = (1.0,) * 7
# losses[3] against the fp64 term: the fp64 sums differ by at most n * 2^-53, then (float)(S / n) and the fp32 product with f2 -- two
# fp32 roundings, 2^-23 relative, with 2x headroom
BAR = 2.0 ** -22


def g(t):
    return t.to(DEV).contiguous()


def _starts(rows):
    r = torch.zeros(len(rows), 7, 2, dtype=torch.int64)
    r[:, :, 0] = torch.tensor(rows, dtype=torch.int64)
    r[:, :, 1] = -77          # the second column is never read
    return r


_CASES = {}


def _case(name, golden_dir):
    """(rois int64 [B, 7, 2], L, pred, pp, pl, target, noise) on the host; made once per name and left unchanged.  Rows uniform in
    [0, 1/3] (the decoder's output range is sigmoid / 3), a noise of std 0.01; `real3_512` carries the real prediction / target rows."""
    if name in _CASES:
        return _CASES[name]
    real = np.load(os.path.join(golden_dir, "real_tianchi_B2_V3.npz"))
    cases = np.load(os.path.join(golden_dir, "roi_cases.npz"))
    if name == "real3_512":
        # the two real rows plus one adversarial row: non-monotonic starts, one negative, one beyond L
        rois = torch.cat([torch.from_numpy(real["rois"]), _starts([[0, 300, -5, 100, 700, 203, 401]])])
        L = 512
    elif name in ("mod4_512", "len1000", "len5000"):
        rois, L = torch.from_numpy(cases[f"{name}:rois"]), int(cases[f"{name}:L"])
    elif name == "synth_40000":
        rois = _starts([[0, 4001, 5003, 9999, 13001, 22222, 31337], [0, 1, 2, 1023, 1025, 39997, 39999]])
        L = 40000
    elif name == "edges_512":
        # end 0; end > L; negative and beyond-L starts; non-monotonic with the end in front of two starts; equal starts
        rois = _starts([[0, 3, 6, 9, 12, 15, 0], [0, 50, 100, 150, 200, 250, 900], [0, -9, -1, 2 ** 40, 600, 77, 500],
                        [0, 400, 100, 300, 50, 200, 350], [0, 64, 64, 64, 255, 255, 257]])
        L = 512
    else:
        raise KeyError(name)
    B = rois.shape[0]
    gen = torch.Generator().manual_seed(1000 * B + L)
    pred, pp, pl, tgt = (torch.rand(B, 1, L, generator=gen) / 3 for _ in range(4))
    if name == "real3_512":
        pred[:2], tgt[:2, 0] = torch.from_numpy(real["out"]), torch.from_numpy(real["target_view"])
        pp[:2], pl[:2] = torch.from_numpy(real["shuf_p"]), torch.from_numpy(real["shuf_l"])
    nz = torch.randn(B, 1, L, generator=gen) * 0.01
    _CASES[name] = (rois, L, pred, pp, pl, tgt, nz)
    return _CASES[name]


NAMES = ["real3_512", "mod4_512", "len1000", "len5000", "synth_40000", "edges_512"]


def test_cases_cover_every_segment_and_the_seams(golden_dir):
    """What the shapes are for: every bin occurs, boundaries that are no multiple of 4, empty and one-position segments, the 1024-position
    tile seams inside a segment and at a boundary, rows without padding and rows that are all padding."""
    from electrocardio_panorama_amd import ops
    assert ops.LOSS_SEG_TILE == 1024
    for name in NAMES:
        rois, L = _case(name, golden_dir)[:2]
        idx = seg_ref.seg_index(rois, L)
        assert set(np.unique(idx)) == set(range(7)), name
    idx = seg_ref.seg_index(*_case("mod4_512", golden_dir)[:2])
    assert (idx[0] == 0).sum() == 1 and (idx[1] == 1).sum() == 0 and (idx[1] == 6).sum() == 3
    assert _case("len1000", golden_dir)[1] % 1024 != 0 and _case("len5000", golden_dir)[0][1, 6, 0] == 4999
    idx = seg_ref.seg_index(*_case("edges_512", golden_dir)[:2])
    assert (idx[0] == 6).all() and (idx[1] != 6).all()
    idx = seg_ref.seg_index(*_case("synth_40000", golden_dir)[:2])
    assert idx[1, 1022] == 2 and idx[1, 1023] == 3 and idx[1, 1024] == 3 and idx[1, 1025] == 4 and idx[1, 39999] == 6


# ------------------------------------------------------------------------------------------------ 1. backward
@pytest.mark.parametrize("name", NAMES)
def test_backward_is_one_fp32_multiply_per_element(name, golden_dir):
    """g_pred is bit-identical to ops.loss_bwd(...)[0] * W with W built on the host from seg_ref.weight_map: both sides are one fp32
    multiply of the same operands.  All weights 1: bit-identical to ops.loss_bwd alone.  The Standin gradients keep their bits."""
    from electrocardio_panorama_amd import ops
    rois, L, pred, pp, pl, tgt, nz = _case(name, golden_dir)
    B = rois.shape[0]
    d_rois = g(rois)
    W = torch.from_numpy(seg_ref.weight_map(rois, L, W_DISTINCT)).reshape(B, 1, L)
    gs = torch.tensor([0.5, 0, 0, 0], device=DEV)
    for reg_l2 in (False, True):
        for noise in (None, g(nz)):
            args = (g(pred), g(pp), g(pl), g(tgt), gs, FACTORS, reg_l2, 7)
            plain = [t.clone() for t in ops.loss_bwd(*args, noise=noise)]
            g3 = ops.loss_bwd(*args, noise=noise)
            assert ops.loss_seg_bwd(g3[0], W_DISTINCT, d_rois) is g3[0]
            assert torch.equal(g3[0].cpu(), plain[0].cpu() * W), (name, reg_l2)
            assert torch.equal(g3[1], plain[1]) and torch.equal(g3[2], plain[2])
            assert float(plain[0].abs().max()) > 0 and not torch.equal(g3[0], plain[0])
            g1 = ops.loss_bwd(*args, noise=noise)
            ops.loss_seg_bwd(g1[0], ONES, d_rois)
            assert torch.equal(g1[0], plain[0])


# ------------------------------------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("name", NAMES)
def test_forward_vs_fp64_restatement(name, golden_dir):
    """losses[3] within 2^-22 relative of seg_ref.seg_term; losses[0] == (losses[1] + losses[2]) + losses[3] in fp32 exactly;
    losses[1:3] bit-identical to the key-off row; all weights 1 within one fp32 ulp of ops.loss_fwd's; the same bits from a second call;
    a fifth element (the SSIM term's place) is not touched."""
    from electrocardio_panorama_amd import ops
    rois, L, pred, pp, pl, tgt, nz = _case(name, golden_dir)
    d_rois = g(rois)
    for reg_l2 in (False, True):
        for noisy in (False, True):
            noise = g(nz) if noisy else None
            four = ops.loss_fwd(g(pred), g(pp), g(pl), g(tgt), FACTORS, reg_l2, 7, noise=noise).cpu()
            row = torch.full((4,), -3.0, device=DEV)
            ops.loss_fwd(g(pred), g(pp), g(pl), g(tgt), FACTORS, reg_l2, 7, out=row, noise=noise)
            assert ops.loss_seg_fwd(g(pred), g(tgt), row, W_DISTINCT, FACTORS[2], reg_l2, d_rois, noise=noise) is row
            got = row.cpu()
            ref = float(seg_ref.seg_term(pred, tgt, rois, W_DISTINCT, FACTORS[2], reg_l2, noise=nz if noisy else None))
            d = abs(float(got[3]) - ref)
            print(f"{name} {'l2' if reg_l2 else 'l1'} noise={noisy}: losses[3] {float(got[3]):.9g} vs fp64 {ref:.9g}, rel {d / abs(ref):.2e} "
                  f"(bar {BAR:.2e})")
            assert ref > 0 and d <= BAR * abs(ref)
            assert torch.equal(got[1:3], four[1:3])
            assert torch.equal(got[0], (got[1] + got[2]) + got[3])
            assert abs(float(got[3]) - float(four[3])) > 1e-3 * float(four[3])          # the weights matter on this case
            # all ones: the flat term, summed in another order
            one = four.clone().to(DEV)
            ops.loss_seg_fwd(g(pred), g(tgt), one, ONES, FACTORS[2], reg_l2, d_rois, noise=noise)
            ulp = float(np.spacing(np.float32(float(four[3]))))
            assert abs(float(one[3].cpu()) - float(four[3])) <= ulp, (float(one[3]), float(four[3]))
            # a 5-element row: [4] keeps its bits; a second call gives the same bits (fixed summation order, no atomics)
            five = torch.full((5,), -3.0, device=DEV)
            ops.loss_fwd(g(pred), g(pp), g(pl), g(tgt), FACTORS, reg_l2, 7, out=five, noise=noise)
            ops.loss_seg_fwd(g(pred), g(tgt), five, W_DISTINCT, FACTORS[2], reg_l2, d_rois, noise=noise)
            assert torch.equal(five[:4], row) and float(five[4]) == -3.0


def test_pad_zero_changes_the_term_on_the_real_rows(golden_dir):
    """With pad = 0 on the two real rows the term differs from the flat term by more than 10 %: the inputs exercise the weights."""
    from electrocardio_panorama_amd import ops
    rois, L, pred, pp, pl, tgt, _ = _case("real3_512", golden_dir)
    a = [g(t[:2]) for t in (pred, pp, pl, tgt)]
    flat = ops.loss_fwd(*a, FACTORS, False, 7)
    row = flat.clone()
    ops.loss_seg_fwd(a[0], a[3], row, (1, 1, 1, 1, 1, 1, 0), FACTORS[2], False, g(rois[:2]))
    f, w = float(flat[3]), float(row[3])
    print(f"real rows: flat term {f:.6g}, pad = 0 term {w:.6g} ({(f - w) / f:.1%} of it was padding)")
    assert abs(w - f) > 0.1 * f and w > 0


def test_ops_reject_malformed_calls(golden_dir):
    from electrocardio_panorama_amd import ops
    rois, L, pred, pp, pl, tgt, nz = _case("real3_512", golden_dir)
    row = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError):
        ops.loss_seg_fwd(g(pred), g(tgt), row, W_QRS[:6], 1.0, False, g(rois))
    with pytest.raises(ValueError):
        ops.loss_seg_fwd(g(pred), g(tgt), row, (1, 1, -1, 1, 1, 1, 1), 1.0, False, g(rois))
    with pytest.raises(ValueError):
        ops.loss_seg_fwd(g(pred), g(tgt), row, W_QRS, 1.0, False, g(rois[:2]))
    with pytest.raises(ValueError):
        ops.loss_seg_fwd(g(pred), g(tgt), row, W_QRS, 1.0, False, g(rois), noise=g(nz[:1]))
    with pytest.raises(ValueError):
        ops.loss_seg_fwd(g(pred[:, :, :510]), g(tgt[:, :, :510]), row, W_QRS, 1.0, False, g(rois))
    with pytest.raises(AssertionError):
        ops.loss_seg_fwd(g(pred), g(tgt), row[:3], W_QRS, 1.0, False, g(rois))
    with pytest.raises(AssertionError):
        ops.loss_seg_bwd(g(pred), W_QRS, g(rois).to(torch.int32))
    with pytest.raises(ValueError):
        ops.view_seg_metrics(g(pred), g(tgt), g(rois[:1]))


# ------------------------------------------------------------------------------------------------ 3. view_seg_metrics
@pytest.mark.parametrize("name", NAMES)
def test_view_seg_metrics_vs_restatement_and_view_metrics(name, golden_dir):
    """cnt equals seg_ref exactly, se within 1e-12 relative; the six wave segments together give ops.view_metrics' cropped PSNR within
    1e-12 relative on every row with end > 0."""
    from electrocardio_panorama_amd import ops
    rois, L = _case(name, golden_dir)[:2]
    B, Q = rois.shape[0], 3
    gen = torch.Generator().manual_seed(77 + L)
    x, y = (torch.rand(B, Q, L, generator=gen) / 3 for _ in range(2))
    x[0, 1] = y[0, 1]                                     # one exact row: se == 0 in every bin
    se, cnt = ops.view_seg_metrics(g(x), g(y), g(rois))
    assert se.dtype == torch.float64 and cnt.dtype == torch.int32 and se.shape == cnt.shape == (B, Q, 7)
    se, cnt = se.cpu().numpy(), cnt.cpu().numpy()
    se_ref, cnt_ref = seg_ref.seg_sums(x, y, rois)
    assert np.array_equal(cnt.astype(np.int64), cnt_ref)
    err = np.abs(se - se_ref)
    print(f"{name}: se worst relative error {float((err / np.maximum(se_ref, 1e-300)).max()):.2e} (bar 1e-12)")
    assert (err <= 1e-12 * se_ref).all() and (se[cnt_ref == 0] == 0.0).all() and (se[0, 1] == 0.0).all()
    psnr = ops.view_metrics(g(x), g(y), g(rois))[0].cpu().numpy()
    checked = 0
    for i in range(B):
        end = min(max(int(rois[i, 6, 0]), 0), L)
        assert cnt[i, 0, :6].sum() == end
        if end == 0:
            continue
        for q in range(Q):
            s = se[i, q, :6].sum()
            mine = 100.0 if s == 0 else 20.0 * np.log10(1.0 / np.sqrt(s / end))
            assert abs(mine - psnr[i, q]) <= 1e-12 * abs(psnr[i, q]), (i, q, mine, psnr[i, q])
            checked += 1
    assert checked >= Q
    se2, cnt2 = ops.view_seg_metrics(g(x), g(y), g(rois))
    assert torch.equal(se2.cpu(), torch.from_numpy(se)) and torch.equal(cnt2.cpu(), torch.from_numpy(cnt))


# ------------------------------------------------------------------------------------------------ through the model
def make_cfg(V, lr=0.1, noise=False, **solver):
    cfg = Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""),
              DATA=Cfg(lead_num=V, noise=noise, synthetic=True),
              SOLVER=Cfg(optim="sgd", lr=lr, scheduler="MultiStep", lr_step=[50, 100], reg_loss="l1_loss",
                         loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], epochs=1),
              output_dir="/tmp/nef_test", desc="debug", seed=7)
    cfg.SOLVER.update(solver)
    return cfg


@pytest.mark.parametrize("reg", ["l1_loss", "l2_loss"])
def test_autograd_on_the_models_own_output(reg):
    """B = 2, V = 3, L = 512: autograd.grad(loss_seg, out) equals W * autograd.grad(loss_plain, out) bit for bit, and the Standin
    outputs' gradients keep their bits."""
    from electrocardio_panorama_amd.network import losswrapper
    B, V, L = 2, 3, 512
    b = batch_t(B, V, L, 41)
    m = hashed_model(V).train()
    random.seed(5)
    out, sp, sl = m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
    tgt = b["target_view"].unsqueeze(1)
    cfg_p, cfg_s = make_cfg(V, reg_loss=reg), make_cfg(V, reg_loss=reg, seg_weights=list(W_QRS))
    plain = losswrapper(out, sp, sl, tgt, cfg_p)
    seg = losswrapper(out, sp, sl, tgt, cfg_s, rois=b["rois"])
    assert len(plain) == len(seg) == 4
    gp = torch.autograd.grad(plain[0], (out, sp, sl), retain_graph=True)
    gsg = torch.autograd.grad(seg[0], (out, sp, sl), retain_graph=True)
    W = torch.from_numpy(seg_ref.weight_map(b["rois"], L, W_QRS)).reshape(B, 1, L)
    assert torch.equal(gsg[0].cpu(), gp[0].cpu() * W)
    assert torch.equal(gsg[1], gp[1]) and torch.equal(gsg[2], gp[2])
    assert float(gsg[0][W.to(DEV) == 0].abs().sum()) == 0.0 and float((W == 0).sum()) > 100       # the padding sends nothing back
    ref = float(seg_ref.seg_term(out.detach().cpu(), tgt.cpu(), b["rois"], W_QRS, 1.0, reg == "l2_loss"))
    assert abs(float(seg[3]) - ref) <= BAR * ref
    assert torch.equal(seg[1], plain[1]) and torch.equal(seg[2], plain[2])
    assert torch.equal(seg[0].detach().cpu(), (seg[1].cpu() + seg[2].cpu()) + seg[3].cpu())


def _batches(n, B, V, L, seed0, noise=False, n_rest=5):
    from electrocardio_panorama_amd import synth
    out = []
    for s in range(seed0, seed0 + n):
        b = dict(synth.make_batch(B, V, L, seed=s, Q=n_rest))
        if noise:
            b["noise"] = np.random.default_rng(9000 + s).normal(0, 0.05, (B, L)).astype(np.float32)
        out.append(b)
    return out


def _solver(V, optim, graph, noise=False, **keys):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    cfg = make_cfg(V, lr={"sgd": 0.1, "adam": 1e-3}[optim], noise=noise, optim=optim, graph=bool(graph), **keys)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


_SLOTS = {"sgd": ("buf",), "adam": ("m", "v", "step")}


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + [v.clone() for k, v in sol.model.named_buffers()]


@pytest.mark.parametrize("optim,noise,keys", [("sgd", False, {}), ("adam", False, {}), ("sgd", False, dict(ssim_factor=0.5, ssim_crop=True)),
                                              ("sgd", True, {}), ("sgd", False, dict(accum_steps=2)), ("sgd", False, dict(train_views=2))],
                         ids=["sgd", "adam", "sgd_ssim", "sgd_noise", "sgd_accum2", "sgd_views2"])
def test_seg_graphed_equals_eager(optim, noise, keys):
    """Three steps at B = 2, V = 3, L = 512 with seg_weights [1, 1, 3, 2, 1, 1, 0]: the replayed step equals the eager one bit for bit --
    loss rows, parameters, optimiser state, BatchNorm buffers -- from one capture, and both differ from the key-off run."""
    V, B, L = 3, 2, 512
    batches = _batches(3, B, V, L, 40, noise=noise)
    out = {}
    for name, graph, seg in (("eager", False, True), ("graphed", True, True), ("off", False, False)):
        k = dict(keys, seg_weights=list(W_QRS)) if seg else dict(keys)
        cfg, sol, opt = _solver(V, optim, graph, noise=noise, **k)
        random.seed(100)
        rows = np.array(sol.run_one_epoch(batches, "train", opt, collect_views=False)[0])
        assert rows.shape == (3, 5 if "ssim_factor" in keys else 4) and np.isfinite(rows).all()
        st = getattr(sol, "_graph_stepper", None)
        assert (st is not None) == graph
        if graph:
            assert len(st.slots) == 1 and st.calls == 3
            assert (st.rois_q is not None) == ("train_views" in keys and (seg or "ssim_factor" in keys))
        out[name] = (_state(sol, opt, optim), rows)
    for a, b in zip(out["eager"][0], out["graphed"][0]):
        assert torch.equal(a, b)
    assert np.array_equal(out["eager"][1], out["graphed"][1])
    rows, off = out["graphed"][1], out["off"][1]
    assert np.array_equal(rows[0, 1:3], off[0, 1:3]) and rows[0, 3] != off[0, 3]       # the first step: same weights, another term 3
    r = rows.astype(np.float32)                           # (exact: the rows are fp32 values)
    total = (r[:, 1] + r[:, 2]) + r[:, 3]
    assert np.array_equal(r[:, 0], total + r[:, 4] if r.shape[1] == 5 else total)       # the association of loss_final, then the SSIM add
    assert not torch.equal(out["graphed"][0][0], out["off"][0][0])


def test_off_is_off(monkeypatch):
    """seg_weights [] and seg_eval False, or the keys absent: neither segment op is entered, the loss row has 4 elements, and losses and
    parameters after two steps are bit-identical to a config that never had the keys -- eagerly and replayed.  A test phase launches no
    nef_view_seg_metrics."""
    from electrocardio_panorama_amd import ops, synth
    V, B, L = 3, 2, 512
    batches = _batches(2, B, V, L, 40)
    test = [dict(synth.make_batch(B, V, L, seed=70, Q=5))]
    entered = []
    for fn in ("loss_seg_fwd", "loss_seg_bwd", "view_seg_metrics"):
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _r=real, _n=fn, **k: (entered.append(_n), _r(*a, **k))[1])
    res = {}
    for name, keys in (("absent", {}), ("off", dict(seg_weights=[], seg_eval=False)), ("on", dict(seg_weights=list(W_QRS), seg_eval=True))):
        for graph in (False, True):
            entered.clear()
            cfg, sol, opt = _solver(V, "sgd", graph, **keys)
            random.seed(100)
            rows = np.array(sol.run_one_epoch(batches, "train", opt, collect_views=False)[0])
            state = _state(sol, opt, "sgd")
            random.seed(101)
            with torch.no_grad():
                metrics = sol.run_one_epoch(test, "test", collect_views=False)[4]
            res[name, graph] = (rows, state, list(entered), sol.last_seg_psnr, metrics,
                                sol._graph_stepper.losses.numel() if graph else rows.shape[1])
    for graph in (False, True):
        a, z, on = res["absent", graph], res["off", graph], res["on", graph]
        assert a[2] == [] and z[2] == [] and a[3] is None and z[3] is None
        assert a[0].shape == z[0].shape == (2, 4) and a[5] == z[5] == 4
        assert np.array_equal(a[0], z[0]) and all(torch.equal(x, y) for x, y in zip(a[1], z[1]))
        assert a[4] == z[4]
        # on: both loss entries once per eager train step -- replayed: once in the probe, once under capture --, the forward one once
        # more in the test phase's losswrapper, and one metrics launch
        assert on[2].count("loss_seg_fwd") == 3 and on[2].count("loss_seg_bwd") == 2 and on[2].count("view_seg_metrics") == 1
        assert not np.array_equal(on[0], a[0]) and on[5] == 4
    assert np.array_equal(res["absent", False][0], res["absent", True][0])


def test_solver_test_phase_reports_psnr_per_segment():
    """Solver.run_one_epoch(phase='test') with seg_eval: six finite numbers per split that match a host computation from rest_out /
    rest_view within 1e-9; the clean metrics keep their bits; with `whole` both splits are the same."""
    from electrocardio_panorama_amd import synth
    V, B, L, Q = 3, 2, 512, 5
    test = [dict(synth.make_batch(B, V, L, seed=70 + s, Q=Q)) for s in range(2)]
    runs = {}
    for name, keys, data in (("off", {}, {}), ("on", dict(seg_eval=True), {}), ("whole", dict(seg_eval=True), dict(super_mode="all0"))):
        cfg, sol, _ = _solver(V, "sgd", False, **keys)
        cfg.DATA.update(data)
        random.seed(101)
        with torch.no_grad():
            res = sol.run_one_epoch(test, "test", collect_views=True)
        runs[name] = (res, sol.last_seg_psnr)
    assert runs["off"][1] is None
    assert runs["off"][0][4] == runs["on"][0][4] and runs["off"][0][0] == runs["on"][0][0]           # metrics and losses: the same bits
    res, seg = runs["on"]
    gen_num = 4
    rest_view, rest_out, rois = (np.stack(res[k]).reshape(2, B, *np.shape(res[k][0])) for k in (1, 2, 5))
    want = {"gen": [], "reg": []}
    for bi in range(2):
        se, cnt = seg_ref.seg_sums(rest_out[bi], rest_view[bi], rois[bi])
        for split, sl in (("gen", slice(Q - gen_num, Q)), ("reg", slice(0, Q - gen_num))):
            row = []
            for k in range(6):
                vals = [seg_ref.seg_psnr(se[i, q, k], cnt[i, q, k]) for i in range(B) for q in range(Q)[sl] if cnt[i, q, k] > 0]
                assert vals
                row.append(np.mean(vals))
            want[split].append(row)
    for split in ("gen", "reg"):
        w = np.mean(np.array(want[split]), axis=0)
        got = np.array(seg[split])
        print(f"psnr_{split}_seg: {got}")
        assert got.shape == (6,) and np.isfinite(got).all() and np.abs(got - w).max() <= 1e-9
    assert seg["gen"] != seg["reg"]
    names, vals = sol._seg_scalars()
    assert names[:2] == ["psnr_gen_seg_P", "psnr_gen_seg_PR"] and names[-1] == "psnr_reg_seg_TP" and len(names) == len(vals) == 12
    assert runs["whole"][1]["gen"] == runs["whole"][1]["reg"] and np.isfinite(runs["whole"][1]["gen"]).all()


def test_nefnet2_goes_through_the_same_losswrapper():
    """Model_nefnet2's eager step with seg_weights: the loss row's term 3 is the weighted one and the step runs."""
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    V, B, L = 3, 2, 512
    rows = {}
    for name, keys in (("off", {}), ("on", dict(seg_weights=list(W_QRS)))):
        cfg = make_cfg(V, **keys)
        cfg.MODEL["model"] = "model_nefnet2"
        torch.manual_seed(1234)
        sol = Solver(cfg, use_tensorboardx=False)
        sol.model.dropout_p = 0.0
        opt = get_optimizer(cfg, sol.model.parameters())
        random.seed(100)
        rows[name] = np.array(sol.run_one_epoch(_batches(1, B, V, L, 40), "train", opt, collect_views=False)[0])
    assert rows["on"].shape == rows["off"].shape == (1, 4) and np.isfinite(rows["on"]).all()
    assert np.array_equal(rows["on"][0, 1:3], rows["off"][0, 1:3]) and rows["on"][0, 3] != rows["off"][0, 3]
