"""fp64 reference of the BatchNorm family (csrc/elementwise.hip), plain torch on the CPU.

Every function takes the fp32 tensors a kernel was given, upcasts them to double and returns doubles.  The backward is
written from the closed form, not through autograd; tests/test_bn_ref_cpu.py checks it against torch.autograd in float64
before tests/test_bn_gpu.py lets it judge a kernel."""
import torch
import torch.nn.functional as F


def d(t):
    return torch.as_tensor(t).detach().cpu().double()


def _pc(v, Bp):
    """[P, C] per-pass constants -> [P*Bp, C, 1], broadcastable against [P*Bp, C, L]."""
    return v.repeat_interleave(Bp, 0)[:, :, None]


def stats(x, gamma, beta, rm, rv, P, eps=1e-5, mom=0.1):
    """Train-mode BatchNorm1d statistics of P stacked passes x [P*Bp, C, L]: (mean, invstd, a, b), each [P, C], with
    y = x*a + b, and the running statistics after the P passes in order (unbiased variance, n = Bp*L)."""
    x, gamma, beta, rm, rv = d(x), d(gamma), d(beta), d(rm).clone(), d(rv).clone()
    N, C, L = x.shape
    Bp = N // P
    n = Bp * L
    xp = x.reshape(P, Bp, C, L)
    mean = xp.mean(dim=(1, 3))
    var = ((xp - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    a = gamma[None, :] * invstd
    b = beta[None, :] - mean * a
    for p in range(P):
        rm = (1.0 - mom) * rm + mom * mean[p]
        rv = (1.0 - mom) * rv + mom * var[p] * (n / (n - 1.0))
    return mean, invstd, a, b, rm, rv


def eval_affine(gamma, beta, rm, rv, eps=1e-5):
    a = d(gamma) / torch.sqrt(d(rv) + eps)
    return a[None, :], (d(beta) - d(rm) * a)[None, :]


def fwd(x, a, b, P):
    """relu(x*a[p,c] + b[p,c])."""
    x = d(x)
    Bp = x.shape[0] // P
    return torch.relu(x * _pc(d(a), Bp) + _pc(d(b), Bp))


def bwd(gy, x, gamma, beta, P, eps=1e-5):
    """Backward of relu(batch_norm(x)) per pass from the closed form: g = gy*[x*a+b > 0], k1 = sum(g)/n,
    k2 = sum(g*xhat)/n, gx = a*(g - k1 - xhat*k2); ggamma = sum g*xhat and gbeta = sum g over all passes.
    Returns (gx, ggamma, gbeta, per-channel sum of gx)."""
    return bwd_g(lambda act: d(gy), x, gamma, beta, P, eps)[:4]


def bwd_g(g_of_act, x, gamma, beta, P, eps=1e-5):
    """bwd() with the gradient at the ReLU output supplied by `g_of_act(act)` (act = the fp64 forward): what the fused
    forms rebuild on the fly.  Returns (gx, ggamma, gbeta, chan sum, act)."""
    x = d(x)
    N, C, L = x.shape
    Bp = N // P
    n = Bp * L
    mean, invstd, a, b, _, _ = stats(x, gamma, beta, torch.zeros(C), torch.ones(C), P, eps)
    pre = x * _pc(a, Bp) + _pc(b, Bp)
    act = torch.relu(pre)
    g = g_of_act(act) * (pre > 0)
    xhat = (x - _pc(mean, Bp)) * _pc(invstd, Bp)
    s1 = g.reshape(P, Bp, C, L).sum(dim=(1, 3))
    s2 = (g * xhat).reshape(P, Bp, C, L).sum(dim=(1, 3))
    gx = _pc(a, Bp) * (g - _pc(s1 / n, Bp) - xhat * _pc(s2 / n, Bp))
    return gx, s2.sum(0), s1.sum(0), gx.sum(dim=(0, 2)), act


def upsample2(x):
    return F.interpolate(d(x), scale_factor=2, mode="linear", align_corners=False)


def upsample2_adjoint(gu):
    """Transpose of upsample2 applied to gu [N, C, 2L] -> [N, C, L] (the map is linear: its vector-Jacobian product)."""
    gu = d(gu)
    N, C, L2 = gu.shape
    z = torch.zeros(N, C, L2 // 2, dtype=torch.float64, requires_grad=True)
    F.interpolate(z, scale_factor=2, mode="linear", align_corners=False).backward(gu)
    return z.grad.detach()


def outconv(act, w, bias):
    """sigmoid(conv1d(act, w, bias, padding=1) / 3), act [N, C, L] -> [N, 1, L]."""
    return torch.sigmoid(F.conv1d(d(act), d(w), d(bias), 1, 1) / 3)


def outconv_adjoint(gout, act, w, bias):
    """Gradient of outconv() with respect to act for the cotangent gout: go = gout*o*(1-o)/3 through the conv's transpose."""
    o = outconv(act, w, bias)
    go = d(gout) * o * (1 - o) / 3
    return F.conv_transpose1d(go, d(w), None, 1, 1)


def pass_combine_fwd(P2, bias, B):
    """P2 [2B, 2C, L] (rows n < B: mean inputs, n >= B: picked inputs; channels < C: A half, >= C: B half) -> the three
    passes c1 [3B, C, L] = (A[mean] + B[mean], A[pick] + B[mean], A[mean] + B[pick]) + bias."""
    P2 = d(P2)
    C = P2.shape[1] // 2
    am, bm, ap, bp = P2[:B, :C], P2[:B, C:], P2[B:, :C], P2[B:, C:]
    return torch.cat([am + bm, ap + bm, am + bp], 0) + d(bias)[None, :, None]


def combine3(gx):
    """Adjoint of pass_combine_fwd on gx [3B, C, L] -> gP2 [2B, 2C, L]: A[mean] = g0 + g2, A[pick] = g1,
    B[mean] = g0 + g1, B[pick] = g2."""
    gx = d(gx)
    B = gx.shape[0] // 3
    g0, g1, g2 = gx[:B], gx[B:2 * B], gx[2 * B:]
    return torch.cat([torch.cat([g0 + g2, g0 + g1], 1), torch.cat([g1, g2], 1)], 0)


def phase_major(t):
    """[N, C, L] -> [N, 2C, L/2], row 2c + p holding positions p, p + 2, ... of channel c."""
    t = d(t)
    N, C, L = t.shape
    return t.reshape(N, C, L // 2, 2).permute(0, 1, 3, 2).reshape(N, 2 * C, L // 2)


def relu_margin(x, a, b, P):
    """min |x*a + b| / (|x*a| + |b|): how far the closest ReLU decision is from a tie, relative to its two terms."""
    x = d(x)
    Bp = x.shape[0] // P
    xa, bb = x * _pc(d(a), Bp), _pc(d(b), Bp)
    return float(((xa + bb).abs() / (xa.abs() + bb.abs())).min())
