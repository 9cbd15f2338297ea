"""The panorama search (Model_nefnet.locate; include/nefnet_hip.h, nef_locate_score_args) restated in numpy fp64 for the tests: both
scores, the per-row bound of the 'corr' comparison, the best rule as a literal loop, the fp32 candidate formula, and the inputs of the
device tests (so that tests/test_locate_cpu.py can assert the precondition of the device bars on the very same arrays).

Score of view p against observed row y on [0, n): 'mse' = (1/n) sum (p - y)^2, +inf with n < 1; 'corr' = 1 - r, r by tests/corr_ref.py's
definition (sums on values shifted by each row's first sample), +inf with n < 2; NaN counts as +inf.  Lower is better."""
import math

import numpy as np

import corr_ref

EPS = corr_ref.EPS
INF = float("inf")


def row_ends(rois, B, L):
    return corr_ref.row_ends(rois, B, L)


def _corr_parts(p, y, n):
    """(score, bound-free moments) of the fp64 rows p [C, n] against y [n]: 1 - r per candidate and (vx, vy, mean u^2, mean w^2)."""
    u, w = p - p[:, :1], y - y[0]
    mu, mw = u.sum(-1) / n, w.sum() / n
    mu2, mw2 = (u * u).sum(-1) / n, (w * w).sum() / n
    vx, vy, c = mu2 - mu * mu, mw2 - mw * mw, (u * w).sum(-1) / n - mu * mw
    return vx, vy, c, mu2, mw2


def scores(pred, obs, ends, mode, eps=EPS, group=0, with_bound=False):
    """fp64 [B, R, A] (group 0: every candidate against every observed row) or [B, R, G] (group G: candidate a against row a // G) of
    pred [B, A, L], obs [B, R, L] (any float dtype, widened); `ends`: n_b per sample.  with_bound: also the per-row bound of the device
    comparison in 'corr' mode -- delta = n 2^-52 (mean u^2 + mean w^2) is what the rounding of n fp64 additions can move a moment by,
    three moments enter r, and 1 / min(vx + eps, vy + eps) is r's sensitivity to them: 3 delta / min(vx + eps, vy + eps); 0 where the
    score is +inf."""
    pred, obs = np.asarray(pred, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    B, A, L = pred.shape
    R = obs.shape[1]
    W = group if group else A
    out = np.full((B, R, W), INF)
    bound = np.zeros((B, R, W))
    for b in range(B):
        n = ends[b]
        if n < (1 if mode == "mse" else 2):
            continue
        for r in range(R):
            p = pred[b, r * group:(r + 1) * group, :n] if group else pred[b, :, :n]
            y = obs[b, r, :n]
            if mode == "mse":
                d = p - y
                v = (d * d).sum(-1) / n
            else:
                vx, vy, c, mu2, mw2 = _corr_parts(p, y, n)
                with np.errstate(invalid="ignore", divide="ignore"):
                    v = 1.0 - (c + eps) / np.sqrt((vx + eps) * (vy + eps))
                    bound[b, r] = 3.0 * (n * 2.0 ** -52 * (mu2 + mw2)) / np.minimum(vx + eps, vy + eps)
            out[b, r] = np.where(np.isnan(v), INF, v)
    return (out, bound) if with_bound else out


def mse_loop(p, y, n):
    """The 'mse' score, literally."""
    if n < 1:
        return INF
    s = 0.0
    for t in range(n):
        d = float(p[t]) - float(y[t])
        s += d * d
    return s / n


def best(row, cands, running=None, index_base=0, keep_index=False):
    """The best rule, literally: candidates in order, a strictly lower score replaces the running best (ties stay with the earliest), NaN
    counts as +inf.  row: scores [A]; cands: [A, 2] fp32; running: None (initialise) or (score, (t1, t2), index).  Returns (score,
    (t1, t2) as np.float32, index): (+inf, (nan, nan), -1) without a finite score.  keep_index: the index is left alone, and a running
    best at -1 stays as it is."""
    if running is None:
        bs, bt, bi = INF, (np.float32("nan"), np.float32("nan")), -1
    else:
        bs, bt, bi = running
        if keep_index and bi < 0:
            return running
        bs = INF if math.isnan(bs) else bs
    for j in range(len(row)):
        v = float(row[j])
        if math.isnan(v):
            v = INF
        if v < bs:
            bs, bt = v, (np.float32(cands[j][0]), np.float32(cands[j][1]))
            if not keep_index:
                bi = index_base + j
    return bs, bt, bi


def best_table(scores_, cands, running=None, index_base=0, keep_index=False):
    """`best` over scores [B, R, A]; cands [A, 2] shared or [B, R * A, 2] per pair.  (score [B, R], theta fp32 [B, R, 2], index [B, R])."""
    B, R, A = scores_.shape
    bs, bt, bi = np.empty((B, R)), np.empty((B, R, 2), dtype=np.float32), np.empty((B, R), dtype=np.int64)
    for b in range(B):
        for r in range(R):
            c = cands if cands.ndim == 2 else cands[b, r * A:(r + 1) * A]
            run = None if running is None else (float(running[0][b, r]), tuple(running[1][b, r]), int(running[2][b, r]))
            bs[b, r], bt[b, r], bi[b, r] = best(scores_[b, r], c, run, index_base, keep_index)
    return bs, bt, bi


def level_cands(best_theta, best_index, s1, s2, radius, placeholder):
    """fp32 [B, R * (2 radius + 1)^2, 2]: centre + (float32(i - radius) * s1, float32(k - radius) * s2), i-major, one rounded fp32
    multiply and one rounded fp32 add per coordinate; centre = best_theta[b, r], or the placeholder where best_index[b, r] < 0."""
    bt = np.asarray(best_theta, dtype=np.float32)
    B, R = bt.shape[:2]
    W = 2 * radius + 1
    centre = np.where(np.asarray(best_index)[..., None] >= 0, bt, np.asarray(placeholder, dtype=np.float32)[None, None]).astype(np.float32)
    off = np.arange(-radius, radius + 1).astype(np.float32)
    o1 = (off * np.float32(s1)).astype(np.float32)                # rounded multiply
    o2 = (off * np.float32(s2)).astype(np.float32)
    out = np.empty((B, R, W, W, 2), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        out[..., 0] = centre[:, :, None, None, 0] + o1[None, None, :, None]       # rounded add (float32 + float32)
        out[..., 1] = centre[:, :, None, None, 1] + o2[None, None, None, :]
    return out.reshape(B, R * W * W, 2)


# ---------------------------------------------------------------------------------------------- the inputs of the device tests
B = 2
SHAPES = [(R, A, L) for R in (1, 3) for A in (1, 5, 26) for L in (1, 2, 4, 7, 64, 257, 512, 1000, 5000)] + [(1, 2, 40000), (3, 2, 40000)]
IDS = [f"R{r}_A{a}_L{l}" for r, a, l in SHAPES]
BOUND_CAP = 1e-8          # the 'corr' bound of every counted row of every case stays below this (asserted on the CPU)


def end_variants(L):
    """Row ends of the two samples: None = without rois; then 0, 1, 2, L - 1, L, beyond L and negative, two at a time."""
    return [None, [0, L], [1, L - 1], [2, L + 5], [-3, L]]


_CASES = {}


def case(R, A, L):
    """(pred fp32 [B, A, L], obs fp32 [B, R, L]), made once per key and left unchanged.  Observed rows: uniform on [0, 1].  Even
    candidates: independent uniform rows (r near 0); odd candidates: 0.9 * (observed row a % R) + 0.1 * an independent row (r near 1)."""
    key = (R, A, L)
    if key not in _CASES:
        rng = np.random.default_rng(100000 * R + 1000 * A + L)
        obs = rng.random((B, R, L), dtype=np.float32)
        pred = rng.random((B, A, L), dtype=np.float32)
        for a in range(1, A, 2):
            pred[:, a] = np.float32(0.9) * obs[:, a % R] + np.float32(0.1) * pred[:, a]
        _CASES[key] = (pred, obs)
    return _CASES[key]
