"""The correlation term of the training loss (cfg.SOLVER.corr_factor, include/nefnet_hip.h: nef_loss_corr_args) restated in torch fp64
for the tests: `corr_term` is autograd-able and composes with oracle.nefnet_oracle's forward / loss_v1 / SGDState; `corr_grad_closed` is the
closed-form gradient the backward kernels implement; `corr_metrics` is nef_view_corr_metrics' table.  Row rule: row i is taken on
[0, n_i); moments on values shifted by the row's first sample, u = x - x[0], w = y - y[0]:
    mu = mean u;  mw = mean w;  vx = mean u^2 - mu^2;  vy = mean w^2 - mw^2;  c = mean u w - mu mw;
    D = sqrt((vx + eps) (vy + eps));  r_i = (c + eps) / D
a row with n_i < 2 is left out; R = rows that count; term = factor * mean_i (1 - r_i), 0 with R = 0.
`corr_term_centred` is a second formulation (two-pass, centred, numpy.longdouble) that the CPU tests use as a precondition check only."""
import numpy as np
import torch

EPS = 1e-8


def row_ends(rois, B, L):
    """n_i = clamp(rois[i, -1, 0], 0, L); None: whole rows."""
    if rois is None:
        return [L] * B
    return [min(max(int(rois[i, -1, 0]), 0), L) for i in range(B)]


def _rows(x, y, ends):
    L = x.shape[-1]
    x2, y2 = x.reshape(-1, L).double(), y.reshape(-1, L).double()
    return x2, y2, ([L] * x2.shape[0] if ends is None else list(ends))


def _moments(x, y, n):
    """(u, w, mu, mw, vx, vy, c) of the 1-D fp64 rows x, y on [0, n), n >= 1 -- one pass on shifted values, in the definition's order."""
    u, w = x[:n] - x[0], y[:n] - y[0]
    mu, mw = u.sum() / n, w.sum() / n
    vx = (u * u).sum() / n - mu * mu
    vy = (w * w).sum() / n - mw * mw
    c = (u * w).sum() / n - mu * mw
    return u, w, mu, mw, vx, vy, c


def corr_rows(x, y, eps=EPS, ends=None):
    """[r_i or None] for the rows of x, y ([B, L], [B, 1, L] or [Q, B, 1, L]; any float dtype, computed in fp64)."""
    x2, y2, ends = _rows(x, y, ends)
    out = []
    for i, n in enumerate(ends):
        if n < 2:
            out.append(None)
            continue
        _, _, _, _, vx, vy, c = _moments(x2[i], y2[i], n)
        out.append((c + eps) / torch.sqrt((vx + eps) * (vy + eps)))
    return out


def corr_term(x, y, factor, eps=EPS, ends=None):
    """factor * mean_i (1 - r_i) as a 0-dim fp64 tensor (differentiable in x); 0 when no row counts."""
    rows = [1.0 - r for r in corr_rows(x, y, eps, ends) if r is not None]
    if not rows:
        return x.double().sum() * 0.0
    return factor * (torch.stack(rows).sum() / len(rows))


def corr_grad_closed(x, y, factor, eps=EPS, ends=None, gscale=1.0):
    """(g, mag): d term / d x by the closed form, g[t] = gscale * a_i * ((w_t - mw) - k_i (u_t - mu)) with a_i = -factor / (R n_i D) and
    k_i = r_i D / (vx + eps), and the per-element magnitude mag[t] = |gscale a_i| (|w_t - mw| + |k_i| |u_t - mu|) that the rounding of
    g[t] scales with.  fp64, x's shape; exactly 0 at and behind a row's end and on rows that do not count."""
    x2, y2, ends = _rows(x.detach(), y.detach(), ends)
    R = sum(1 for n in ends if n >= 2)
    g, mag = torch.zeros_like(x2), torch.zeros_like(x2)
    for i, n in enumerate(ends):
        if n < 2:
            continue
        u, w, mu, mw, vx, vy, c = _moments(x2[i], y2[i], n)
        D = torch.sqrt((vx + eps) * (vy + eps))
        r = (c + eps) / D
        a = gscale * (-factor / (R * n * D))
        k = r * D / (vx + eps)
        g[i, :n] = a * ((w - mw) - k * (u - mu))
        mag[i, :n] = a.abs() * ((w - mw).abs() + k.abs() * (u - mu).abs())
    return g.reshape(x.shape), mag.reshape(x.shape)


def corr_metrics(pred, gt, rois=None):
    """(mom fp64 [B, Q, 3] = (vx, vy, c), cnt int64 [B, Q] = n_b) of pred, gt [B, Q, L]; zeros for an empty row."""
    B, Q, L = pred.shape
    ends = row_ends(rois, B, L)
    mom = torch.zeros(B, Q, 3, dtype=torch.float64)
    cnt = torch.zeros(B, Q, dtype=torch.int64)
    for b in range(B):
        n = ends[b]
        cnt[b] = n
        if n >= 1:
            for q in range(Q):
                mom[b, q] = torch.stack(_moments(pred[b, q].double(), gt[b, q].double(), n)[4:])
    return mom, cnt


def metrics_r(mom, cnt, eps=EPS):
    """r of the rows with cnt >= 2 from the table, as the host forms it: a 1-D fp64 tensor."""
    m = mom.reshape(-1, 3)[cnt.reshape(-1) >= 2]
    return (m[:, 2] + eps) / torch.sqrt((m[:, 0] + eps) * (m[:, 1] + eps))


# ---------------------------------------------------------------------------------------------- the inputs of the device tests
# They live here so that tests/test_corr_loss_cpu.py can assert the precondition of the device tests' bars on the very same tensors.
TILE = 1024         # ops.LOSS_CORR_TILE
FACTOR = 5.0
# (B, L, row ends or None for whole rows): rows that do not count, unaligned rows (odd L: every second row starts off a 16-byte boundary),
# a row that ends on the tile seam / one behind it, many tiles
SHAPES = [(1, 1, None), (1, 2, None), (2, 13, None), (4, 40, [33, 1, 0, 40]), (3, 500, [298, 2, 777]), (3, 500, [-7, 2, 500]),
          (2, TILE + 1, [TILE, TILE + 1]), (2, TILE + 2, [TILE + 1, 9]), (2, 3 * TILE + 5, [2 * TILE + 1, 3 * TILE + 5]),
          (2, 40000, [39999, 12345])]
IDS = [f"B{b}_L{l}" + ("_neg" if e and min(e) < 0 else "") for b, l, e in SHAPES]
KINDS = ["indep", "close"]      # independent uniform rows in [0, 1/3] (r near 0); pred = target + 0.02 * randn (r near 1)


def rois_of(ends):
    r = torch.zeros(len(ends), 7, 2, dtype=torch.int64)
    r[:, -1, 0] = torch.tensor(ends)
    r[:, :, 1] = 77          # (the other columns are not the row's end)
    return r


def variants(ends):
    """Each cropped shape is also run with whole rows."""
    return [ends] if ends is None else [ends, None]


_CASES = {}


def case(B, L, kind, noisy):
    """(pred, pred_p, pred_l, target, noise or None), fp32 [B, 1, L] on the CPU; made once per key and left unchanged.  The decoder's
    output range is sigmoid / 3; the noise row has std 0.01."""
    key = (B, L, kind, noisy)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * B + L + (500000 if kind == "close" else 0))
        pred, pp, pl, tgt = (torch.rand(B, 1, L, generator=gen) / 3 for _ in range(4))
        if kind == "close":
            pred = tgt + 0.02 * torch.randn(B, 1, L, generator=gen)
        nz = torch.randn(B, 1, L, generator=gen) * 0.01 if noisy else None
        _CASES[key] = (pred, pp, pl, tgt, nz)
    return _CASES[key]


def case_x(B, L, kind, noisy):
    """x of the definition for a case: fp32(pred + noise), the add the kernels make."""
    pred, _, _, _, nz = case(B, L, kind, noisy)
    return pred + nz if noisy else pred


def corr_term_centred(x, y, factor, eps=EPS, ends=None):
    """The same number by another route: two passes, centred on the row's mean, in numpy.longdouble.  A float."""
    L = x.shape[-1]
    x2 = x.detach().reshape(-1, L).double().numpy().astype(np.longdouble)
    y2 = y.detach().reshape(-1, L).double().numpy().astype(np.longdouble)
    ends = [L] * x2.shape[0] if ends is None else list(ends)
    e = np.longdouble(eps)
    vals = []
    for i, n in enumerate(ends):
        if n < 2:
            continue
        a, b = x2[i, :n], y2[i, :n]
        a, b = a - a.mean(), b - b.mean()
        vx, vy, c = (a * a).mean(), (b * b).mean(), (a * b).mean()
        vals.append(np.longdouble(1) - (c + e) / np.sqrt((vx + e) * (vy + e)))
    return float(np.longdouble(factor) * (sum(vals) / len(vals))) if vals else 0.0
