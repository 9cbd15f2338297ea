"""fp64 restatements of the thin ops at the two ends of the network: the output conv, the loss, the angular encoding and
its linear layer, the channel scale and roi_align, each with the magnitude sums the per-element bounds of
tests/test_head_tail_gpu.py are stated against; then the per-element comparison `frac` and the seeded inputs of that
file's cases, which tests/test_head_tail_ref_cpu.py runs its fp32 restatements on.  Plain torch / numpy on the CPU.

Every function takes the fp32 inputs the kernel reads and works in float64 from there.  Three steps are fp32 by the
kernels' contract and are done in fp32 here too, everything behind them in fp64:
  - `th + ph` and `th - ph` of the angular encoding;
  - `pred + noise` in front of the loss terms;
  - the ROI grid positions: (float)roi * 0.25f, * (float)(2/T), + (-1), and torch.linspace's fp32 formula
    (start + step*s below the middle, end - step*(15 - s) above it), each operation rounded on its own."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from util import rnd

U = 2.0 ** -24          # fp32 unit round-off
MARGIN = 2.0 ** -16     # the tie screen: no ReLU decision closer to zero than this fraction of |x*a| + |b|
N_SEG, ROI_BINS = 7, 16


def d(t):
    return torch.as_tensor(t).detach().cpu().double()


# ------------------------------------------------------------------------------------------------ output conv
def act_of(x, pro=None):
    """The tensor the conv reads: x, or relu(x*a[pass] + b[pass]) with pro = (a [P, C], b [P, C], Bp)."""
    x = d(x)
    if pro is None:
        return x
    a, b, Bp = pro
    return F.relu(x * d(a).repeat_interleave(Bp, 0)[:, :, None] + d(b).repeat_interleave(Bp, 0)[:, :, None])


def pro_margin(x, pro):
    """min |x*a + b| / (|x*a| + |b|) over the prologue's ReLU decisions."""
    a, b, Bp = pro
    xa = d(x) * d(a).repeat_interleave(Bp, 0)[:, :, None]
    bb = d(b).repeat_interleave(Bp, 0)[:, :, None].expand_as(xa)
    return float(((xa + bb).abs() / (xa.abs() + bb.abs())).min())


def outconv(x, w, bias, pro=None):
    """sigmoid(conv1d(act, w, bias, padding=1) / 3): [N, C, L] -> [N, 1, L]."""
    return torch.sigmoid(F.conv1d(act_of(x, pro), d(w), d(bias), 1, 1) / 3)


def outconv_S(x, w, bias, pro=None):
    """S[n, 0, t] = sum_k |w_k||act_k| + |bias|: the magnitude the forward's rounding errors scale with."""
    return F.conv1d(act_of(x, pro).abs(), d(w).abs(), d(bias).abs(), 1, 1)


def outconv_go(gout, out):
    """go = gout * out * (1 - out) / 3 from the fp32 `out` the backward kernels read."""
    o = d(out)
    return d(gout) * o * (1 - o) / 3


def outconv_bwd_data(gout, out, w):
    """gx[n, c, t] = sum_k w[c, k] go[n, t - k + 1] and the magnitude sum_k |w[c, k]||go[n, t - k + 1]|."""
    go, w = outconv_go(gout, out), d(w)
    return F.conv_transpose1d(go, w, None, 1, 1), F.conv_transpose1d(go.abs(), w.abs(), None, 1, 1)


def outconv_bwd_weight(gout, out, x, pro=None):
    """gw[0, c, k] = sum_{n,t} go[n, t] act[n, c, t + k - 1], gb = sum go, and the sums of |go||act| and |go|."""
    go, act = outconv_go(gout, out), act_of(x, pro)

    def taps(g, a):
        ap = F.pad(a, (1, 1))
        L = a.shape[-1]
        return torch.stack([(g * ap[:, :, k:k + L]).sum(dim=(0, 2)) for k in range(3)], dim=1)[None]
    return taps(go, act), go.sum().reshape(1), taps(go.abs(), act.abs()), go.abs().sum().reshape(1)


# ------------------------------------------------------------------------------------------------ loss
def _f32(v):
    return float(np.float32(v))


def loss_o(pred, noise=None):
    """The prediction every term is taken at: pred, or the fp32 sum pred + noise."""
    pred = torch.as_tensor(pred).detach().cpu().float()
    return d(pred if noise is None else pred + torch.as_tensor(noise).detach().cpu().float().reshape(pred.shape))


def loss(pred, pp, pl, tgt, factors, reg_l2, use_mask, noise=None):
    """(total, f0*mean|o - pp|, f1*mean|o - pl|, f2*mean|o - tgt| or f2*mean (o - tgt)^2) as a float64 tensor [4]; a term
    whose bit of `use_mask` is clear is 0.  The factors are the fp32 values the kernel is handed."""
    o = loss_o(pred, noise)
    f = [_f32(v) for v in factors]
    dd = o - d(tgt)
    t = [(o - d(pp)).abs().mean() * f[0] if use_mask & 1 else torch.zeros((), dtype=torch.float64),
         (o - d(pl)).abs().mean() * f[1] if use_mask & 2 else torch.zeros((), dtype=torch.float64),
         ((dd * dd).mean() if reg_l2 else dd.abs().mean()) * f[2] if use_mask & 4 else torch.zeros((), dtype=torch.float64)]
    return torch.stack([t[0] + t[1] + t[2]] + t)


def loss_grads(pred, pp, pl, tgt, gscale, factors, reg_l2, use_mask, noise=None):
    """loss_bwd_kernel's closed forms with sign(0) = 0: (g_pred, g_p, g_l), g_p = gs*f0/n * sign(pp - o), g_l likewise,
    g_pred = gs*f2/n * (2(o - tgt) or sign(o - tgt)); zeros for a masked term."""
    o = loss_o(pred, noise)
    f = [_f32(v) for v in factors]
    gs = 1.0 if gscale is None else float(d(gscale).reshape(-1)[0])
    n = o.numel()
    z = torch.zeros_like(o)
    dd = o - d(tgt)
    g_p = gs * f[0] / n * torch.sign(d(pp) - o) if use_mask & 1 else z
    g_l = gs * f[1] / n * torch.sign(d(pl) - o) if use_mask & 2 else z
    g_o = gs * f[2] / n * (2 * dd if reg_l2 else torch.sign(dd)) if use_mask & 4 else z
    return g_o, g_p, g_l


# ------------------------------------------------------------------------------------------------ theta
def theta_encode(theta):
    """[..., 2] -> [..., 12]: (a, sin a, cos a) for a in (th, ph, th + ph, th - ph), the sum and the difference in fp32."""
    th32 = torch.as_tensor(theta).detach().cpu().float()
    t, p = th32[..., 0], th32[..., 1]
    a = torch.stack([t, p, t + p, t - p], dim=-1).double()
    return torch.stack([a, torch.sin(a), torch.cos(a)], dim=-1).reshape(*th32.shape[:-1], 12)


def theta_mlp(theta, W, bias):
    """y = e W^T + bias, A = sum_k |e_k W_k| + |bias| per output element, and sum_k |W_k| per output unit."""
    e, W, bias = theta_encode(theta), d(W), d(bias)
    return e @ W.t() + bias, e.abs() @ W.abs().t() + bias.abs(), W.abs().sum(dim=1)


def theta_mlp_grads(theta, gy):
    """gW [O, 12] = sum_n g[n, o] e[n, k], gb [O] = sum_n g[n, o], A [O, 12] = sum_n |g e_k| and sum_n |g| [O]."""
    e = theta_encode(theta).reshape(-1, 12)
    g = d(gy).reshape(e.shape[0], -1)
    return g.t() @ e, g.sum(0), g.abs().t() @ e.abs(), g.abs().sum(0)


# ------------------------------------------------------------------------------------------------ channel scale
def chscale(x, s):
    """y[b, c, t] = x[b, c, t] * s[b, c]."""
    return d(x) * d(s)[:, :, None]


def chscale_grads(gy, x, s, relu_x):
    """gx = gy * s (zero where relu_x and not x > 0: -0.0 and +0.0 both mask), gs[b, c] = sum_t gy x, A = sum_t |gy x|."""
    gy, x = d(gy), d(x)
    gx = gy * d(s)[:, :, None]
    if relu_x:
        gx = torch.where(x > 0, gx, torch.zeros_like(gx))
    return gx, (gy * x).sum(-1), (gy * x).abs().sum(-1)


# ------------------------------------------------------------------------------------------------ ROI align
def roi_grid(rois, T):
    """The fp32 grid x of (sample, segment, bin) [B, 7, 16]; every operation is one fp32 rounding (module docstring)."""
    f = np.float32
    r = np.asarray(torch.as_tensor(rois).cpu().numpy(), dtype=np.int64).astype(f)
    sc = f(2.0 / T)
    r = (r * f(0.25)) * sc + f(-1.0)
    r0, r1 = r[..., 0:1], r[..., 1:2]
    step = (r1 - r0) / f(ROI_BINS - 1)
    s = np.arange(ROI_BINS, dtype=f)[None, None, :]
    gx = np.where(s < ROI_BINS // 2, r0 + step * s, r1 - step * (f(ROI_BINS - 1) - s))
    assert gx.dtype == np.float32
    return torch.from_numpy(gx)


def roi_col_weight(gx):
    """grid_sample's bilinear weight of the single column (W = 1, zero padding, align_corners=False) at x = gx, in fp64."""
    ix = ((d(gx) + 1.0) - 1.0) * 0.5
    x0 = torch.floor(ix)
    we = ix - x0
    return torch.where(x0 == 0, 1.0 - we, torch.zeros_like(we)) + torch.where(x0 + 1 == 0, we, torch.zeros_like(we))


def roi_rows(T):
    """The two middle rows and their weights: iy = (T - 1)/2, rows floor(iy) and floor(iy) + 1 (the latter out of range
    or weightless for odd T: weight 0, row index folded back onto the first)."""
    iy = (T - 1) * 0.5
    r0 = int(np.floor(iy))
    w1 = iy - r0
    r1 = r0 + 1
    if r1 >= T or w1 == 0.0:
        return r0, r0, 1.0 - w1, 0.0
    return r0, r1, 1.0 - w1, w1


def roi_align(z, rois):
    """out[b, c, j, s] = (z[b, c, r0] w0 + z[b, c, r1] w1) wx[b, j, s] and |z0 w0 wx| + |z1 w1 wx|."""
    z = d(z)
    T = z.shape[2]
    r0, r1, w0, w1 = roi_rows(T)
    wx = roi_col_weight(roi_grid(rois, T))[:, None]                    # [B, 1, 7, 16]
    z0, z1 = z[:, :, r0, None, None], z[:, :, r1, None, None]
    return (z0 * w0 + z1 * w1) * wx, (z0.abs() * w0 + z1.abs() * w1) * wx.abs()


def roi_align_transpose(gout, rois, T):
    """gz [B, C, T]: w_row * sum_{j,s} gout wx on the two middle rows, zero elsewhere; and the magnitude w_row * sum |gout wx|."""
    g = d(gout)
    r0, r1, w0, w1 = roi_rows(T)
    wx = roi_col_weight(roi_grid(rois, T))[:, None]
    acc, mag = (g * wx).sum(dim=(2, 3)), (g * wx).abs().sum(dim=(2, 3))
    gz, A = torch.zeros(g.shape[0], g.shape[1], T, dtype=torch.float64), torch.zeros(g.shape[0], g.shape[1], T, dtype=torch.float64)
    gz[:, :, r0], A[:, :, r0] = acc * w0, mag * w0
    if w1 != 0.0:
        gz[:, :, r1] += acc * w1
        A[:, :, r1] += mag * w1
    return gz, A


# ------------------------------------------------------------------------------------------------ the comparison
def frac(got, ref, bound):
    """max over the elements of |got - ref| / bound.  Fails on anything that is not a finite value inside a finite
    comparison: a NaN or an infinity in `got`, or a difference where the bound is 0."""
    shape = torch.as_tensor(ref).shape
    got, ref = d(got).reshape(-1), d(ref).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} values are not finite"
    assert bool(torch.isfinite(ref).all())
    dlt = (got - ref).abs()
    b = d(bound).expand(shape).reshape(-1) if torch.is_tensor(bound) and bound.numel() > 1 else torch.full_like(dlt, float(bound))
    bad = (dlt > 0) & ~(b > 0)
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ where the bound is 0"
    f = torch.where(dlt > 0, dlt / b.clamp_min(1e-300), torch.zeros_like(dlt))
    return float(f.max())


# ------------------------------------------------------------------------------------------------ seeded inputs of the cases
OC_PLAIN_SEED = 2100
LOSS_FACTORS = (0.5, 0.25, 1.5)
PLANT = 16
CHSCALE_SEED = 2300
ROI_L = [4, 8, 12, 500, 1000]
_OC = {}


def oc_case(shape, seed):
    """Seeded fp32 inputs of one output-conv case and its fp64 forward.  shape (N, C, L): no prologue; (P, Bp, C, L): with
    one.  `out` is the fp32 rounding of the fp64 forward: the backward kernels read it as an input.  gout is rnd + 0.5: the
    bias gradient is ONE value, and a relative bar on it means something only where sum go does not cancel (with a
    zero-mean gout |sum go| / sum|go| is 2e-5 at (2,5,257), where torch's own fp32 sum misses 1e-5)."""
    key = (shape, seed)
    if key not in _OC:
        pro = len(shape) == 4
        N, C, L = (shape[0] * shape[1], shape[2], shape[3]) if pro else shape
        s = seed
        c = dict(N=N, C=C, L=L, seed=s, x=rnd(N, C, L, seed=s), w=rnd(1, C, 3, seed=s + 1, scale=0.2), b=rnd(1, seed=s + 2),
                 gy=rnd(N, 1, L, seed=s + 5) + 0.5, pro=None)
        if pro:
            c["pro"] = (rnd(shape[0], C, seed=s + 3) + 1.1, rnd(shape[0], C, seed=s + 4) * 0.4, shape[1])
        c["ref"] = outconv(c["x"], c["w"], c["b"], c["pro"])
        c["out"] = c["ref"].float()
        _OC[key] = c
    return _OC[key]


def oc_weight_K(N, L):
    """The constant of the weight-gradient bound (derived in test_head_tail_gpu.py's docstring)."""
    return 12 + 16 * math.ceil(N * math.ceil(L / 1024) / 1024)


def loss_case(n, seed=2200):
    """pred, pp, pl, tgt, noise of n elements.  PLANT elements each of pred are set so that o = pred (+ noise) equals tgt,
    pp and pl exactly: there everything involved sits on a 2^-10 lattice, so pred = v - noise and pred + noise are exact.
    n = 1 has room for one tie only, o == tgt."""
    pred, pp, pl, tgt = (rnd(n, 1, 1, seed=seed + i) for i in range(4))
    noise = rnd(n, 1, 1, seed=seed + 4, scale=0.1)
    k = min(PLANT, n // 3) if n >= 3 else 0
    idx = [torch.arange(k) * 3 + j + (n // 2 if n > 6 * PLANT else 0) for j in range(3)] if k else [torch.arange(1), [], []]
    q = lambda t: torch.round(t * 1024) / 1024
    plain, noisy = pred.clone(), pred.clone()
    for i, other in zip(idx, (tgt, pp, pl)):
        if len(i) == 0:
            continue
        other[i], noise[i] = q(other[i]), q(noise[i])
        plain[i], noisy[i] = other[i], other[i] - noise[i]
    return dict(n=n, pp=pp, pl=pl, tgt=tgt, noise=noise, pred={False: plain, True: noisy}, idx=idx)


def theta_grid():
    """(theta, phi) over [-pi, pi]^2: a 9-point linspace plus 0, +-pi, +-pi/2 in fp32, every pair (so th == ph too)."""
    pi = float(np.float32(np.pi))
    v = torch.cat([torch.linspace(-pi, pi, 9), torch.tensor([0.0, pi, -pi, pi / 2, -pi / 2, 1.0, -2.5])]).float()
    return torch.stack(torch.meshgrid(v, v, indexing="ij"), dim=-1).reshape(-1, 2)


def chscale_case(shape, relu_x):
    """x, the [B, 3C] scale table (its middle column block is `s`), gy; with relu_x, x carries +0.0, -0.0 and negatives."""
    B, C, T = shape
    x, tab, gy = rnd(B, C, T, seed=CHSCALE_SEED), rnd(B, 3 * C, seed=CHSCALE_SEED + 1), rnd(B, C, T, seed=CHSCALE_SEED + 2)
    if relu_x:
        f = x.reshape(-1)
        f[0::7], f[3::7] = 0.0, -0.0           # the rest keeps both signs
    return x, tab, gy
