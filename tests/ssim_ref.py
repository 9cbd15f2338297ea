"""The SSIM term of the training loss (cfg.SOLVER.ssim_factor, include/nefnet_hip.h: nef_loss_ssim_args) restated in torch fp64 for the tests:
`ssim_term` is autograd-able (unfold-based) and composes with oracle.nefnet_oracle's forward / loss_v1 / SGDState; `ssim_grad_closed` is the
closed-form gradient the backward kernel implements.  Row rule: row i is taken on [0, end_i); a row with end_i < 7 has no window and is
left out; R = rows with a window; term = factor * (1 - mean_i S_i), 0 with R = 0."""
import torch

WIN = 7
C1, C2 = 1e-4, 9e-4
COV_NORM = WIN / (WIN - 1.0)


def row_ends(rois, B, L):
    """end_i = clamp(rois[i, -1, 0], 0, L); None: whole rows."""
    if rois is None:
        return [L] * B
    return [min(max(int(rois[i, -1, 0]), 0), L) for i in range(B)]


def _window_ssim(x, y):
    """S_p of every full window of the 1-D fp64 rows x, y."""
    wx, wy = x.unfold(0, WIN, 1), y.unfold(0, WIN, 1)
    ux, uy = wx.mean(1), wy.mean(1)
    vx = COV_NORM * ((wx * wx).mean(1) - ux * ux)
    vy = COV_NORM * ((wy * wy).mean(1) - uy * uy)
    vxy = COV_NORM * ((wx * wy).mean(1) - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def row_ssim(x, y, ends=None):
    """[S_i or None] for the rows of x, y ([B, L] or [B, 1, L]; any float dtype, computed in fp64)."""
    L = x.shape[-1]
    x2, y2 = x.reshape(-1, L).double(), y.reshape(-1, L).double()
    ends = [L] * x2.shape[0] if ends is None else ends
    return [_window_ssim(x2[i, :e], y2[i, :e]).mean() if e >= WIN else None for i, e in enumerate(ends)]


def ssim_term(x, y, factor, ends=None):
    """factor * (1 - mean S_i) as a 0-dim fp64 tensor (differentiable in x); 0 when no row has a window."""
    rows = [s for s in row_ssim(x, y, ends) if s is not None]
    if not rows:
        return x.double().sum() * 0.0
    return factor * (1.0 - torch.stack(rows).mean())


def ssim_grad_closed(x, y, factor, ends=None, gscale=1.0):
    """d term / d x by the closed form: per window dS_p/dx_t = [dS/dux + 2n dS/dvx (x_t - ux) + n dS/dvxy (y_t - uy)] / 7, summed over the
    windows that hold t, times -factor * gscale / (R (end_i - 6)).  fp64, x's shape."""
    L = x.shape[-1]
    x2, y2 = x.detach().reshape(-1, L).double(), y.detach().reshape(-1, L).double()
    B = x2.shape[0]
    ends = [L] * B if ends is None else ends
    R = sum(1 for e in ends if e >= WIN)
    g = torch.zeros_like(x2)
    n = COV_NORM
    for i, e in enumerate(ends):
        if e < WIN:
            continue
        xi, yi = x2[i, :e], y2[i, :e]
        wx, wy = xi.unfold(0, WIN, 1), yi.unfold(0, WIN, 1)
        ux, uy = wx.mean(1), wy.mean(1)
        vx = n * ((wx * wx).mean(1) - ux * ux)
        vy = n * ((wy * wy).mean(1) - uy * uy)
        vxy = n * ((wx * wy).mean(1) - ux * uy)
        A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
        B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
        S = A1 * A2 / (B1 * B2)
        d_ux = 2 * (uy * A2 - ux * S * B2) / (B1 * B2)
        d_vx = -S / B2
        d_vxy = 2 * A1 / (B1 * B2)
        scale = -factor * gscale / (R * (e - (WIN - 1)))
        for p in range(e - (WIN - 1)):
            d = (d_ux[p] + 2 * n * d_vx[p] * (xi[p:p + WIN] - ux[p]) + n * d_vxy[p] * (yi[p:p + WIN] - uy[p])) / WIN
            g[i, p:p + WIN] += scale * d
    return g.reshape(x.shape)
