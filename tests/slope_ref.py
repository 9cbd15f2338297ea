"""The slope (first-difference) term of the training loss (cfg.SOLVER.slope_factor, include/nefnet_hip.h: nef_loss_slope_args) restated in
torch fp64 for the tests: `slope_term` is autograd-able and composes with oracle.nefnet_oracle's forward / loss_v1 / SGDState;
`slope_grad_closed` is the closed-form gradient the backward kernel implements; `slope_metrics` is nef_view_slope_metrics' table.  Row rule:
row i is taken on [0, end_i); d(i, t) = (x[t + 1] - x[t]) - (y[t + 1] - y[t]) for t in [0, end_i - 1); S_i = mean of |d| (or d^2); a row
with end_i < 2 has no difference and is left out; R = rows with a difference; term = factor * mean_i S_i, 0 with R = 0."""
import torch


def row_ends(rois, B, L):
    """end_i = clamp(rois[i, -1, 0], 0, L); None: whole rows."""
    if rois is None:
        return [L] * B
    return [min(max(int(rois[i, -1, 0]), 0), L) for i in range(B)]


def _diffs(x, y, e):
    """d(t), t in [0, e - 1), of the 1-D fp64 rows x, y -- in the order of the definition."""
    return (x[1:e] - x[:e - 1]) - (y[1:e] - y[:e - 1])


def _rows(x, y, ends):
    L = x.shape[-1]
    x2, y2 = x.reshape(-1, L).double(), y.reshape(-1, L).double()
    return x2, y2, ([L] * x2.shape[0] if ends is None else list(ends))


def row_slope(x, y, l2=False, ends=None):
    """[S_i or None] for the rows of x, y ([B, L], [B, 1, L] or [Q, B, 1, L]; any float dtype, computed in fp64)."""
    x2, y2, ends = _rows(x, y, ends)
    out = []
    for i, e in enumerate(ends):
        if e < 2:
            out.append(None)
            continue
        d = _diffs(x2[i], y2[i], e)
        out.append((d * d).mean() if l2 else d.abs().mean())
    return out


def slope_term(x, y, factor, l2=False, ends=None):
    """factor * mean_i S_i as a 0-dim fp64 tensor (differentiable in x); 0 when no row has a difference."""
    rows = [s for s in row_slope(x, y, l2, ends) if s is not None]
    if not rows:
        return x.double().sum() * 0.0
    return factor * torch.stack(rows).mean()


def slope_grad_closed(x, y, factor, l2=False, ends=None, gscale=1.0):
    """d term / d x by the closed form: g[t] = factor * gscale / (R (end_i - 1)) * (s(t - 1) - s(t)), s = sign(d) (sign(0) = 0) or 2 d,
    s = 0 outside [0, end_i - 1).  fp64, x's shape; exactly 0 at and behind a row's end and on rows without a difference."""
    x2, y2, ends = _rows(x.detach(), y.detach(), ends)
    R = sum(1 for e in ends if e >= 2)
    g = torch.zeros_like(x2)
    for i, e in enumerate(ends):
        if e < 2:
            continue
        d = _diffs(x2[i], y2[i], e)
        s = 2.0 * d if l2 else torch.sign(d)
        z = torch.zeros(1, dtype=torch.float64)
        g[i, :e] = factor * gscale / (R * (e - 1)) * (torch.cat([z, s]) - torch.cat([s, z]))
    return g.reshape(x.shape)


def slope_metrics(pred, gt, rois=None):
    """(se fp64 [B, Q], cnt int64 [B, Q]) of pred, gt [B, Q, L]: the sum of d^2 over the differences of row (b, q) on [0, end_b), and
    their number max(end_b - 1, 0)."""
    B, Q, L = pred.shape
    ends = row_ends(rois, B, L)
    se = torch.zeros(B, Q, dtype=torch.float64)
    cnt = torch.zeros(B, Q, dtype=torch.int64)
    for b in range(B):
        e = ends[b]
        cnt[b] = max(e - 1, 0)
        if e >= 2:
            for q in range(Q):
                d = _diffs(pred[b, q].double(), gt[b, q].double(), e)
                se[b, q] = (d * d).sum()
    return se, cnt
