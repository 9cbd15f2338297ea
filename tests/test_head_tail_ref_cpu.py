"""tests/head_tail_ref.py pinned without a GPU: every restatement against an independent fp64 computation (torch autograd
in double, or the oracle run on double inputs) to 1e-12 relative; the tie screen over the seed table of
tests/test_head_tail_gpu.py; and fp32 restatements with the kernels' summation order inside the per-element bounds of that
file, so that no bound there rests on what a kernel returned."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_tail_ref as R
from util import rnd

U = R.U
BAR = 1e-12


def close(a, b, bar=BAR):
    a, b = R.d(a).reshape(-1), R.d(b).reshape(-1)
    assert a.shape == b.shape
    return float((a - b).abs().max()) <= bar * max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------ against autograd / the oracle
@pytest.mark.parametrize("shape", [(2, 3, 1), (2, 3, 5), (3, 17, 260), (2, 3, 5, 37)], ids=str)
def test_outconv_against_autograd(shape):
    c = R.oc_case(shape, 31)
    x = R.d(c["x"])
    if c["pro"] is not None:
        a, b, Bp = c["pro"]
        x = F.relu(x * a.double().repeat_interleave(Bp, 0)[:, :, None] + b.double().repeat_interleave(Bp, 0)[:, :, None])
    act, w, bias = x.clone().requires_grad_(True), R.d(c["w"]).requires_grad_(True), R.d(c["b"]).requires_grad_(True)
    out = torch.sigmoid(F.conv1d(act, w, bias, 1, 1) / 3)
    out.backward(R.d(c["gy"]))
    assert close(R.outconv(c["x"], c["w"], c["b"], c["pro"]), out)
    # the backward restatements read `out` as an input: handed the fp64 forward they are autograd's gradients
    gx, gmag = R.outconv_bwd_data(c["gy"], out, c["w"])
    gw, gb, aw, ab = R.outconv_bwd_weight(c["gy"], out, c["x"], c["pro"])
    assert close(gx, act.grad) and close(gw, w.grad) and close(gb, bias.grad)
    assert bool((gmag >= gx.abs() * (1 - 1e-12)).all()) and bool((aw >= gw.abs() * (1 - 1e-12)).all()) and bool(ab >= gb.abs())
    S = R.outconv_S(c["x"], c["w"], c["b"], c["pro"])
    assert bool((S >= (F.conv1d(act, w, bias, 1, 1)).abs() * (1 - 1e-12)).all())
    # fed the rounded fp32 `out` instead, go moves by the rounding of out only
    assert close(R.outconv_bwd_data(c["gy"], c["out"], c["w"])[0], act.grad, 1e-6)


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("reg", ["l1_loss", "l2_loss"])
@pytest.mark.parametrize("mask", range(1, 8))
def test_loss_against_autograd_and_oracle(mask, reg, noisy):
    from oracle import nefnet_oracle as orc
    c = R.loss_case(255)
    pred, noise = c["pred"][noisy], (c["noise"] if noisy else None)
    f, gs = R.LOSS_FACTORS, torch.tensor([0.37])
    o = R.loss_o(pred, noise).requires_grad_(True)               # the fp32 sum, then double
    pp, pl = R.d(c["pp"]).requires_grad_(True), R.d(c["pl"]).requires_grad_(True)
    using = tuple(i + 1 for i in range(3) if mask >> i & 1)
    vals = orc.loss_v1(o, pp, pl, R.d(c["tgt"]), f, using, reg)
    ref = R.loss(pred, c["pp"], c["pl"], c["tgt"], f, reg == "l2_loss", mask, noise)
    assert close(ref, torch.stack([torch.as_tensor(v, dtype=torch.float64) for v in vals]))
    (vals[0] * float(np.float32(0.37))).backward()
    grads = R.loss_grads(pred, c["pp"], c["pl"], c["tgt"], gs, f, reg == "l2_loss", mask, noise)
    for got, want in zip(grads, (o.grad, pp.grad, pl.grad)):
        want = torch.zeros_like(got) if want is None else want
        assert close(got, want) and bool(((want == 0) == (got == 0)).all())
    if mask == 7:            # the planted ties are there and give exact zeros
        for i, gr in zip(c["idx"], grads):
            assert len(i) == R.PLANT and bool((gr.reshape(-1)[i] == 0).all())


def test_theta_against_autograd_and_oracle():
    from oracle import nefnet_oracle as orc
    th = torch.round(rnd(40, 2, seed=32, scale=3.0) * 1024) / 1024         # th +- ph exact in fp32: the oracle's double sum equals it
    assert close(R.theta_encode(th), orc.angular_encoding(th.double()))
    assert close(R.theta_encode(R.theta_grid()[:, None, :]).reshape(-1, 12), R.theta_encode(R.theta_grid()))
    th = rnd(40, 2, seed=33, scale=3.0)                                     # general angles: the sum and difference are fp32's
    e = R.theta_encode(th)
    assert torch.equal(e[:, 6], (th[:, 0] + th[:, 1]).double()) and torch.equal(e[:, 9], (th[:, 0] - th[:, 1]).double())
    assert close(e[:, 7], torch.sin(e[:, 6])) and close(e[:, 11], torch.cos(e[:, 9])) and torch.equal(e[:, 3], th[:, 1].double())
    W, b, gy = rnd(5, 12, seed=34).double().requires_grad_(True), rnd(5, seed=35).double().requires_grad_(True), rnd(40, 5, seed=36)
    y = F.linear(e, W, b)
    y.backward(gy.double())
    ref, A, Wabs = R.theta_mlp(th, W, b)
    gW, gb, AW, Ab = R.theta_mlp_grads(th, gy)
    assert close(ref, y) and close(gW, W.grad) and close(gb, b.grad)
    assert bool((A >= ref.abs() * (1 - 1e-12)).all()) and bool((AW >= gW.abs() * (1 - 1e-12)).all()) and close(Wabs, W.detach().abs().sum(1))
    assert close(Ab, gy.double().abs().sum(0))


def test_chscale_against_autograd():
    x, tab, gy = R.chscale_case((3, 5, 77), True)
    s = tab[:, 5:10]
    xr, sr = x.double().requires_grad_(True), s.double().requires_grad_(True)
    y = xr * sr[:, :, None]
    y.backward(gy.double())
    gx, gs, A = R.chscale_grads(gy, x, s, False)
    assert close(R.chscale(x, s), y) and close(gx, xr.grad) and close(gs, sr.grad) and bool((A >= gs.abs() * (1 - 1e-12)).all())
    ur = x.double().requires_grad_(True)                     # x as the output of a ReLU: its producer masks where not x > 0
    (F.relu(ur) * s.double()[:, :, None]).backward(gy.double())
    gxm = R.chscale_grads(gy, x, s, True)[0]
    assert close(gxm, ur.grad) and bool((gxm[~(x > 0)] == 0).all())


def _roi_tables(golden_dir):
    from electrocardio_panorama_amd import synth
    z = np.load(f"{golden_dir}/roi_cases.npz")
    out = [(n, torch.from_numpy(z[f"{n}:rois"]), int(z[f"{n}:L"]) // 4) for n in sorted({k.split(":")[0] for k in z.files})]
    return out + [(f"synth L={L}", torch.from_numpy(synth.make_rois(np.random.default_rng(3), 3, L)), L // 4) for L in R.ROI_L]


def test_roi_align_against_grid_sample_and_oracle(golden_dir):
    from oracle import nefnet_oracle as orc
    for name, rois, T in _roi_tables(golden_dir):
        B, C = rois.shape[0], 4
        z, gy = rnd(B, C, T, seed=37).double().requires_grad_(True), rnd(B, C, 7, 16, seed=38).double()
        gx = R.roi_grid(rois, T)
        grid = torch.stack([gx.double(), torch.zeros(gx.shape, dtype=torch.float64)], dim=3)
        out = F.grid_sample(z.unsqueeze(-1), grid, align_corners=False)          # fp64 on this file's fp32 grid
        out.backward(gy)
        ref, mag = R.roi_align(z, rois)
        gz, A = R.roi_align_transpose(gy, rois, T)
        assert close(ref, out), name
        assert close(gz, z.grad), name
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all()) and bool((A >= gz.abs() * (1 - 1e-12)).all())
        # the oracle builds its fp32 grid with torch's linspace: the one documented difference, a few ulps of the grid
        r = rois.to(torch.float32).mul(0.25).mul(2 / T).add(-1)
        gxo = torch.stack([torch.stack([torch.linspace(r[i, j, 0], r[i, j, 1], steps=16) for j in range(7)]) for i in range(B)])
        dg = float((gxo.double() - gx.double()).abs().max())
        assert dg <= 4 * 2.0 ** -23 * max(1.0, float(gx.abs().max())), (name, dg)
        oo = orc.roi_align_mid(z.detach(), rois)
        assert float((oo - ref).abs().max()) <= (BAR + dg / 2) * float(z.detach().abs().max()), name


# ------------------------------------------------------------------------------------------------ the tie screen
def gpu_file():
    """tests/test_head_tail_gpu.py: the owner of the SEEDS table and the shape lists this file screens (imported where it is
    needed only; everything else here stands on head_tail_ref alone)."""
    import test_head_tail_gpu as H
    return H


def case(shape):
    """An output-conv case with the seed the GPU file runs it with."""
    return gpu_file().oc_case(shape)


def test_seed_table_clears_the_tie_screen():
    H = gpu_file()
    assert set(H.SEEDS) == set(H.OC_PRO)
    for shape in H.OC_PRO:
        c = case(shape)
        assert c["seed"] == H.SEEDS[shape] and H.oc_screen(c) >= H.MARGIN, shape
    for shape in H.CHSCALE_SHAPES:       # relu_x decides on the input itself: the planted zeros of both signs and negatives are there
        x = R.chscale_case(shape, True)[0].reshape(-1)
        assert bool((x[0::7] == 0).all()) and bool((x[3::7] == 0).all()) and bool(torch.signbit(x[3::7]).all())
        assert not bool(torch.signbit(x[0::7]).any()) and (x.numel() < 3 or bool((x < 0).any()))


# ------------------------------------------------------------------------------------------------ fp32 restatements in the kernels' order
def fma32(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in fp64, the sum is rounded to fp64 and then to fp32."""
    return (a.double() * b.double() + c.double()).float()


def act32(c):
    if c["pro"] is None:
        return c["x"]
    a, b, Bp = c["pro"]
    return F.relu(fma32(c["x"], a.repeat_interleave(Bp, 0)[:, :, None], b.repeat_interleave(Bp, 0)[:, :, None]))


def tree64(v):
    """The 6-level wave sum of 64 lanes (last axis) in fp32."""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 64, 12), (2, 5, 257), (3, 17, 1028), (3, 2, 64, 260), (2, 3, 5, 1025)], ids=str)
def test_outconv_forward_fp32_restatement_is_inside_the_bound(shape):
    """The kernel's chain -- per channel fma(w0, x[t-1]), fma(w1, x[t]), fma(w2, x[t+1]), then + bias, / 3, the sigmoid --
    and torch's own fp32 conv: both inside (3C+2) u S/12 + 6u, torch's below 0.14 of it."""
    c = case(shape)
    C, L = c["C"], c["L"]
    ap = F.pad(act32(c), (1, 1))
    acc = torch.zeros(c["N"], L)
    for ch in range(C):
        for k in range(3):
            acc = fma32(c["w"][0, ch, k].expand_as(acc), ap[:, ch, k:k + L], acc)
    out = (1.0 / (1.0 + torch.exp(-((acc + c["b"][0]) / 3.0))))[:, None]
    bound = (3 * C + 2) * U * R.outconv_S(c["x"], c["w"], c["b"], c["pro"]) / 12 + 6 * U
    assert out.dtype == torch.float32 and R.frac(out, c["ref"], bound) <= 1.0
    t32 = torch.sigmoid(F.conv1d(act32(c), c["w"], c["b"], 1, 1) / 3)
    assert R.frac(t32, c["ref"], bound) <= 0.14


def weight_restatement(c):
    """outconv_bwd_weight_partial / _final in fp32 with the kernel's order: go = gout * (o * (1 - o)) / 3; block b takes the
    units b, b + nblk, ...; within a unit a lane chains 16 fmas per tap (positions (lane + 64 i) * 4 + e for L % 4 == 0,
    lane + 64 q otherwise); wave tree; fp64 over the blocks; one rounding."""
    N, C, L = c["N"], c["C"], c["L"]
    tiles = math.ceil(L / 1024)
    units, Lp = N * tiles, tiles * 1024
    nblk = min(units, 1024)
    o = c["out"]
    go = F.pad((c["gy"] * (o * (1.0 - o)) / 3.0)[:, 0], (1, Lp - L + 1))           # [N, Lp + 2], go[t] at column t + 1
    X = F.pad(act32(c), (0, Lp - L)).view(N, C, tiles, 1024).permute(0, 2, 1, 3).reshape(units, C, 1024)
    G = torch.stack([torch.stack([go[:, t * 1024 + 2 - k:t * 1024 + 2 - k + 1024] for t in range(tiles)], 1) for k in range(3)], 2)
    G = G.reshape(units, 3, 1024)                                                   # G[u, k, tl] = go[t0 + tl + 1 - k]
    lane = torch.arange(64)
    if L % 4 == 0:
        pos = torch.stack([(lane + 64 * i) * 4 + e for i in range(4) for e in range(4)], 1)
    else:
        pos = torch.stack([lane + 64 * q for q in range(16)], 1)
    acc, bsum = torch.zeros(nblk, C, 3, 64), torch.zeros(nblk, 64)
    for r in range(math.ceil(units / nblk)):
        us = slice(r * nblk, min((r + 1) * nblk, units))
        nu = us.stop - us.start
        for step in range(16):
            xv, gv = X[us][:, :, pos[:, step]], G[us][:, :, pos[:, step]]
            acc[:nu] = fma32(gv[:, None, :, :], xv[:, :, None, :], acc[:nu])
        for q in range(16):
            bsum[:nu] = bsum[:nu] + G[us][:, 1, lane + 64 * q]
    gw = tree64(acc).double().sum(0).float()[None]
    return gw, tree64(bsum).double().sum(0).float().reshape(1)


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 5, 257), (3, 17, 1028), (1, 3, 2052), (3, 2, 17, 1028), (2, 3, 5, 1025),
                                   (1030, 3, 4), (520, 3, 1028)], ids=str)
def test_outconv_weight_gradient_fp32_restatement_is_inside_the_bound(shape):
    """K = 12 + 16 ceil(units / 1024) of test_head_tail_gpu.py holds for the kernel's summation order run in fp32 here (and
    for torch's fp32 autograd, about 1 u): the constant comes from the derivation, not from a kernel's output."""
    c = case(shape)
    gw, gb = weight_restatement(c)
    rw, rb, aw, ab = R.outconv_bwd_weight(c["gy"], c["out"], c["x"], c["pro"])
    K = R.oc_weight_K(c["N"], c["L"])
    assert K == (44 if c["N"] * math.ceil(c["L"] / 1024) > 1024 else 28)
    fw, fb = R.frac(gw, rw, K * U * aw), R.frac(gb, rb, K * U * ab)
    assert fw <= 1.0 and fb <= 1.0, (fw, fb)
    a, w, b = act32(c).clone(), c["w"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    F.conv1d(a, w, b, 1, 1).backward((c["gy"] * (c["out"] * (1.0 - c["out"])) / 3.0))
    assert R.frac(w.grad, rw, K * U * aw) <= 1.0 and R.frac(b.grad, rb, K * U * ab) <= 1.0


def test_roi_align_fp32_restatement_is_inside_the_bounds(golden_dir):
    """roi.hip's col_weight, forward expression and backward chain (a lane fmas elements lane and lane + 64 of the 112,
    wave tree, times the row weight) in fp32 on this file's grid: inside 4u and (112/64 + 8)u of the magnitude sums."""
    f1, h = torch.tensor(1.0), torch.tensor(0.5)
    for name, rois, T in _roi_tables(golden_dir):
        B, C = rois.shape[0], 5
        z, gy = rnd(B, C, T, seed=39), rnd(B, C, 7, 16, seed=40)
        gx = R.roi_grid(rois, T)
        ix = ((gx + f1) * f1 - f1) * h
        x0 = torch.floor(ix)
        we = ix - x0
        wx = (torch.where(x0 == 0, f1 - we, torch.zeros_like(we)) + torch.where(x0 + f1 == 0, we, torch.zeros_like(we)))[:, None]
        r0, r1, w0, w1 = R.roi_rows(T)
        w0, w1 = torch.tensor(w0, dtype=torch.float32), torch.tensor(w1, dtype=torch.float32)
        out = z[:, :, r0, None, None] * (w0 * wx) + z[:, :, r1, None, None] * (w1 * wx)
        ref, mag = R.roi_align(z, rois)
        assert out.dtype == torch.float32 and R.frac(out, ref, 4 * U * mag) <= 1.0, name
        ge, we_ = gy.reshape(B, C, 112), wx.expand(B, C, 7, 16).reshape(B, C, 112)
        acc = fma32(ge[..., :64], we_[..., :64], torch.zeros(B, C, 64))
        acc[..., :48] = fma32(ge[..., 64:], we_[..., 64:], acc[..., :48])
        s = tree64(acc)
        gref, A = R.roi_align_transpose(gy, rois, T)
        got = torch.zeros(B, C, T)
        got[:, :, r0] = s * w0
        if float(w1) != 0.0:
            got[:, :, r1] = got[:, :, r1] + s * w1
        assert R.frac(got, gref, (112 / 64 + 8) * U * A) <= 1.0, name


@pytest.mark.parametrize("shape", [(2, 3, 1), (2, 3, 2), (2, 3, 5), (3, 64, 12), (2, 5, 257), (3, 17, 1028), (3, 2, 64, 260)], ids=str)
def test_outconv_data_gradient_fp32_restatement_is_inside_the_bound(shape):
    """outconv_bwd_data_kernel in fp32: go = gout * (o * (1 - o)) / 3 with zero padding, then (w0 go[t+1] + w1 go[t]) + w2 go[t-1],
    every operation rounded on its own (the library is built without fma contraction): inside 8u sum_k|w_k||go_k|."""
    c = case(shape)
    o, L = c["out"], c["L"]
    go = F.pad(c["gy"] * (o * (1.0 - o)) / 3.0, (1, 1))                     # [N, 1, L + 2], go[t] at column t + 1
    gm, g0, gp = go[:, :, 0:L], go[:, :, 1:L + 1], go[:, :, 2:L + 2]
    w = c["w"][0][None, :, :, None]                                          # [1, C, 3, 1]
    gx = (w[:, :, 0] * gp + w[:, :, 1] * g0) + w[:, :, 2] * gm
    gref, gmag = R.outconv_bwd_data(c["gy"], c["out"], c["w"])
    assert gx.dtype == torch.float32 and gx.shape == gref.shape and R.frac(gx, gref, 8 * U * gmag) <= 1.0


def check_rel_or_zero(got, ref, k):
    """The loss bars: exactly 0 where the reference is 0, within k u relative elsewhere; returns the worst fraction."""
    got, ref = R.d(got).reshape(-1), R.d(ref).reshape(-1)
    zero = ref == 0
    assert bool((got[zero] == 0).all())
    return R.frac(got[~zero], ref[~zero], k * U * ref[~zero].abs())


@pytest.mark.parametrize("n", [1, 255, 2000, 65536 + 257])
@pytest.mark.parametrize("reg_l2", [False, True], ids=["l1", "l2"])
def test_loss_fp32_restatement_is_inside_the_bounds(reg_l2, n):
    """loss_partial / loss_final / loss_bwd_kernel in fp32: each |o - p|, o - tgt and its square one fp32 rounding, the sums
    in fp64, (float)(s / n), * f, t1 + t2 + t3 left to right; inv_n = 1.0f / (float)n, ((gs * f) * inv_n) * sign or
    * (2 * d).  Values inside 4u, gradient elements inside 6u, exact zeros where the reference has them."""
    c = R.loss_case(n)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    f = [f32(v) for v in R.LOSS_FACTORS]
    inv_n = f32(1.0) / f32(float(n))
    for noisy in (False, True):
        pred, noise = c["pred"][noisy], (c["noise"] if noisy else None)
        o = pred + noise if noisy else pred
        dd = o - c["tgt"]
        s = [(o - c["pp"]).abs().double().sum(), (o - c["pl"]).abs().double().sum(), ((dd * dd) if reg_l2 else dd.abs()).double().sum()]
        for mask in range(1, 8):
            t = [(s[i] / n).float() * f[i] if mask >> i & 1 else f32(0.0) for i in range(3)]
            got = torch.stack([(t[0] + t[1]) + t[2]] + t)
            assert got.dtype == torch.float32
            assert check_rel_or_zero(got, R.loss(pred, c["pp"], c["pl"], c["tgt"], R.LOSS_FACTORS, reg_l2, mask, noise), 4) <= 1.0
            for gsv in (None, 0.37):
                gs = f32(1.0) if gsv is None else f32(gsv)
                z = torch.zeros_like(o)
                g_p = ((gs * f[0]) * inv_n) * torch.sign(c["pp"] - o) if mask & 1 else z
                g_l = ((gs * f[1]) * inv_n) * torch.sign(c["pl"] - o) if mask & 2 else z
                g_o = ((gs * f[2]) * inv_n) * (2.0 * dd if reg_l2 else torch.sign(dd)) if mask & 4 else z
                refs = R.loss_grads(pred, c["pp"], c["pl"], c["tgt"], None if gsv is None else gs.reshape(1), R.LOSS_FACTORS, reg_l2, mask, noise)
                for a, b in zip((g_o, g_p, g_l), refs):
                    assert a.dtype == torch.float32 and check_rel_or_zero(a, b, 6) <= 1.0


def encode32(th):
    """encode12 in fp32 (torch's fp32 sin / cos stand in for sinf / cosf: both are within the encoding's 2e-6 bar)."""
    t, p = th[..., 0], th[..., 1]
    a = torch.stack([t, p, t + p, t - p], -1)
    return torch.stack([a, torch.sin(a), torch.cos(a)], -1).reshape(*th.shape[:-1], 12)


@pytest.mark.parametrize("N,O", [(1, 5), (18, 128), (257, 256), (300, 5)])
def test_theta_mlp_fwd_fp32_restatement_is_inside_the_bound(N, O):
    """theta_mlp_fwd_kernel in fp32: the 12-fma chain over k, then + bias: inside 14u (sum|e_k W_k| + |bias|) + 2e-6 sum|W_k|."""
    th, W, b = rnd(N, 2, seed=2400, scale=3.0), rnd(O, 12, seed=2401), rnd(O, seed=2402)
    e = encode32(th)
    assert R.frac(e, R.theta_encode(th), 2e-6) <= 1.0 and R.frac(encode32(R.theta_grid()), R.theta_encode(R.theta_grid()), 2e-6) <= 1.0
    acc = torch.zeros(N, O)
    for k in range(12):
        acc = fma32(e[:, k, None].expand(N, O), W[None, :, k].expand(N, O), acc)
    y = acc + b[None, :]
    ref, A, Wabs = R.theta_mlp(th, W, b)
    assert y.dtype == torch.float32 and R.frac(y, ref, 14 * U * A + 2e-6 * Wabs[None, :]) <= 1.0


@pytest.mark.parametrize("N,O", [(1, 5), (255, 128), (257, 5), (700, 128)])
def test_theta_mlp_bwd_fp32_restatement_is_inside_the_bounds(N, O):
    """theta_mlp_bwd_kernel: each product g * e_k one fp32 rounding, summed in fp64, rounded once; gb the fp64 sum of g
    rounded once: gW inside 2u sum|g e_k| + 2e-6 sum|g|, gb inside 2u sum|g|."""
    th, gy = rnd(N, 2, seed=2410, scale=3.0), rnd(N, O, seed=2411)
    e = encode32(th)
    gW = (gy[:, :, None] * e[:, None, :]).double().sum(0).float()
    gb = gy.double().sum(0).float()
    rW, rb, AW, Ab = R.theta_mlp_grads(th, gy)
    assert R.frac(gW, rW, 2 * U * AW + 2e-6 * Ab[:, None]) <= 1.0 and R.frac(gb, rb, 2 * U * Ab) <= 1.0


@pytest.mark.parametrize("shape", [(3, 50, 77), (2, 5, 1), (2, 5, 63), (2, 5, 64), (2, 5, 65), (40, 130, 3)], ids=str)
def test_chscale_fp32_restatement_is_inside_the_bounds(shape):
    """chscale_fwd / chscale_bwd in fp32: y and gx one product each (u relative); gs a lane's fma chain over t = lane,
    lane + 64, ... and the 6-level wave tree: inside (T/64 + 8) u sum|gy x|."""
    B, C, T = shape
    x, tab, gy = R.chscale_case(shape, True)
    s = tab[:, C:2 * C]
    yref = R.chscale(x, s)
    rx, rs, A = R.chscale_grads(gy, x, s, True)
    assert R.frac(x * s[:, :, None], yref, U * yref.abs()) <= 1.0
    gx = torch.where(x > 0, gy * s[:, :, None], torch.zeros_like(x))
    assert R.frac(gx, rx, U * rx.abs()) <= 1.0 and bool((gx[~(x > 0)] == 0).all())
    trips = math.ceil(T / 64)
    gp, xp = F.pad(gy, (0, trips * 64 - T)).view(B, C, trips, 64), F.pad(x, (0, trips * 64 - T)).view(B, C, trips, 64)
    acc = torch.zeros(B, C, 64)
    for q in range(trips):
        acc = fma32(gp[:, :, q], xp[:, :, q], acc)
    assert R.frac(tree64(acc), rs, (T / 64 + 8) * U * A) <= 1.0


# ------------------------------------------------------------------------------------------------ the comparison itself
def test_the_comparisons_reject_what_is_not_a_number_inside_the_bound():
    """frac and the GPU file's rel_or_zero / elem fail on a NaN or an infinity and on any element outside its bound; a
    difference where the bound is 0 fails too."""
    H = gpu_file()
    saved = dict(H.WORST)            # elem keeps a family's worst fraction: this self-check must leave no trace in it
    try:
        _comparisons_reject(H)
    finally:
        H.WORST.clear()
        H.WORST.update(saved)


def _comparisons_reject(H):
    ref = torch.tensor([1.0, 2.0, 0.0])
    assert R.frac(torch.tensor([1.0, 2.0, 0.0]), ref, 1e-7) == 0.0
    assert R.frac(torch.tensor([1.0 + 5e-8, 2.0, 0.0], dtype=torch.float64), ref.double(), 1e-7) == pytest.approx(0.5, rel=1e-6)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for where in range(3):
            got = ref.clone()
            got[where] = bad
            with pytest.raises(AssertionError):
                R.frac(got, ref, 1e-7)
            with pytest.raises(AssertionError):
                H.rel_or_zero("B", "self-check", got, ref, 6)
            with pytest.raises(AssertionError):
                H.elem("B", "self-check", got, ref, torch.tensor([1e-7, 1e-7, 1e-7]))
    with pytest.raises(AssertionError):
        R.frac(torch.tensor([1.0, 2.0, 1e-9]), ref, torch.tensor([1e-7, 1e-7, 0.0]))          # a difference where the bound is 0
    with pytest.raises(AssertionError):
        H.rel_or_zero("B", "self-check", torch.tensor([1.0, 2.0, 1e-30]), ref, 6)              # not exactly 0 where the reference is
    with pytest.raises(AssertionError):
        H.rel_or_zero("B", "self-check", torch.tensor([1.0 + 1e-6, 2.0, 0.0]), ref, 6)
