"""tests/bn_ref.py (the fp64 reference that judges the BatchNorm kernels in test_bn_gpu.py) against torch.autograd in
float64: the closed forms are verified here, on any machine, before they are used as a yardstick."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref
from util import rel, rnd

TOL = 1e-12      # fp64 against fp64: a few hundred ulps of headroom over the summation-order differences


def _inputs(P, Bp, C, L, seed):
    x = (rnd(P * Bp, C, L, seed=seed) * 2 + 0.3).double()
    gamma, beta = (rnd(C, seed=seed + 1) + 1.5).double(), rnd(C, seed=seed + 2).double()
    rm, rv = (rnd(C, seed=seed + 3) * 0.1).double(), (rnd(C, seed=seed + 4).abs() + 0.5).double()
    return x, gamma, beta, rm, rv


def _autograd(x, gamma, beta, rm, rv, P):
    """relu(batch_norm(training=True)) pass by pass in float64; returns leaves, output and the updated running statistics."""
    Bp = x.shape[0] // P
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm.clone(), rv.clone()
    y = torch.cat([F.relu(F.batch_norm(xr[p * Bp:(p + 1) * Bp], rm, rv, gr, br, True, 0.1, 1e-5)) for p in range(P)], 0)
    return xr, gr, br, y, rm, rv


@pytest.mark.parametrize("P,Bp,C,L", [(3, 2, 3, 10), (2, 5, 4, 7)])
def test_stats_forward_backward_match_autograd(P, Bp, C, L):
    x, gamma, beta, rm, rv = _inputs(P, Bp, C, L, seed=700)
    xr, gr, br, y, rm1, rv1 = _autograd(x, gamma, beta, rm, rv, P)
    mean, invstd, a, b, rm2, rv2 = bn_ref.stats(x, gamma, beta, rm, rv, P)
    assert rel(rm2, rm1) < TOL and rel(rv2, rv1) < TOL
    xp = x.reshape(P, Bp, C, L)
    assert rel(mean, xp.mean(dim=(1, 3))) < TOL
    assert rel(invstd, 1 / torch.sqrt(xp.var(dim=(1, 3), unbiased=False) + 1e-5)) < TOL
    assert rel(bn_ref.fwd(x, a, b, P), y) < TOL
    gy = rnd(*y.shape, seed=705).double()
    y.backward(gy)
    gx, gg, gb, gs = bn_ref.bwd(gy, x, gamma, beta, P)
    assert rel(gx, xr.grad) < TOL and rel(gg, gr.grad) < TOL and rel(gb, br.grad) < TOL
    # the channel sum of gx is analytically zero: what is left is fp64 round-off of the O(1) terms
    assert torch.equal(gs, gx.sum(dim=(0, 2))) and float(gs.abs().max()) < 1e-13 * float(gx.abs().sum())
    # eval mode
    a1, b1 = bn_ref.eval_affine(gamma, beta, rm1, rv1)
    assert rel(bn_ref.fwd(x, a1, b1, 1), F.relu(F.batch_norm(x, rm1, rv1, gamma, beta, False, 0.1, 1e-5))) < TOL


@pytest.mark.parametrize("P,Bp,C,L", [(3, 2, 3, 8), (1, 3, 4, 12)])
def test_fused_form_wrappers_match_autograd(P, Bp, C, L):
    x, gamma, beta, rm, rv = _inputs(P, Bp, C, L, seed=710)
    N = P * Bp
    # through the x2 upsampling
    xr, gr, br, y, _, _ = _autograd(x, gamma, beta, rm, rv, P)
    gu = rnd(N, C, 2 * L, seed=715).double()
    F.interpolate(y, scale_factor=2, mode="linear", align_corners=False).backward(gu)
    gx, gg, gb, _ = bn_ref.bwd(bn_ref.upsample2_adjoint(gu), x, gamma, beta, P)
    assert rel(gx, xr.grad) < TOL and rel(gg, gr.grad) < TOL and rel(gb, br.grad) < TOL
    # through the last conv and its sigmoid
    xr, gr, br, y, _, _ = _autograd(x, gamma, beta, rm, rv, P)
    w, bias = rnd(1, C, 3, seed=716, scale=0.2).double(), rnd(1, seed=717).double()
    out = torch.sigmoid(F.conv1d(y, w, bias, 1, 1) / 3)
    gout = rnd(N, 1, L, seed=718).double()
    out.backward(gout)
    gx, gg, gb, _, act = bn_ref.bwd_g(lambda act: bn_ref.outconv_adjoint(gout, act, w, bias), x, gamma, beta, P)
    assert rel(bn_ref.outconv(act, w, bias), out) < TOL
    assert rel(gx, xr.grad) < TOL and rel(gg, gr.grad) < TOL and rel(gb, br.grad) < TOL


def test_pass_combine_and_phase_major():
    B, C, L = 2, 3, 6
    P2 = rnd(2 * B, 2 * C, L, seed=720).double().requires_grad_(True)
    bias = rnd(C, seed=721).double()
    c1 = bn_ref.pass_combine_fwd(P2.detach(), bias, B)
    # the three Standin passes, written out: (mean, mean), (pick, mean), (mean, pick) for the (A, B) halves
    for b in range(B):
        for p, (ia, ib) in enumerate([(b, b), (B + b, b), (b, B + b)]):
            assert torch.equal(c1[p * B + b], P2.detach()[ia, :C] + P2.detach()[ib, C:] + bias[:, None])
    am, bm, ap, bp = P2[:B, :C], P2[:B, C:], P2[B:, :C], P2[B:, C:]
    c1g = torch.cat([am + bm, ap + bm, am + bp], 0) + bias[None, :, None]
    g = rnd(3 * B, C, L, seed=722).double()
    c1g.backward(g)
    assert rel(bn_ref.combine3(g), P2.grad) < TOL
    pm = bn_ref.phase_major(g)
    assert pm.shape == (3 * B, 2 * C, L // 2)
    for c in range(C):
        for p in range(2):
            assert torch.equal(pm[:, 2 * c + p], g[:, c, p::2])


def test_relu_margin():
    x = torch.tensor([[[1.0, -0.5, 0.25]]])
    a, b = torch.tensor([[2.0]]), torch.tensor([[1.0]])
    # pre-activations 3, 0, 1.5 over |xa| + |b| = 3, 2, 1.5
    assert bn_ref.relu_margin(x, a, b, 1) == 0.0
    assert bn_ref.relu_margin(x[:, :, ::2], a, b, 1) == 1.0
    assert abs(bn_ref.relu_margin(torch.tensor([[[-0.25]]]), a, b, 1) - 0.5 / 1.5) < 1e-15
