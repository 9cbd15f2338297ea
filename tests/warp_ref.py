"""Numpy restatement of the time warp with jittered marks (DATA.aug_warp / aug_roi_jitter; the definition in include/nefnet_hip.h,
nef_warp_args): Python integers for the edges, uint64 wrap-around for the counter RNG's mix, IEEE fp64 operation by operation for the
resampling, one rounding to fp32.  Shares no code with the package."""
import os

import numpy as np

from augment_ref import mix

M64 = (1 << 64) - 1
SAMPLE_BASE = 1 << 62
TWO24 = 16777216.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_tianchi_B2_V3.npz")


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def draws(seed, sample):
    """The six words z_k of sample `sample` (= index0 + i) as Python ints."""
    ctr = np.array([(SAMPLE_BASE + 8 * int(sample) + k) & M64 for k in range(6)], dtype=np.uint64)
    return [int(z) for z in mix(seed, ctr)]


def uniform(z):
    return (z >> 40) / TWO24


def jitter_of(z, J):
    return (((2 * J + 1) * ((z >> 16) & 0xFFFFFF)) >> 24) - J


def tables(roi, L, seed, sample, amp, J):
    """One sample's tables from its [7, 2] rois: dict of c [7], n [6], m [6], d [7], e [7], jit [6] (Python ints)."""
    starts = [int(v) for v in np.asarray(roi)[:, 0]]
    c = [clamp(starts[0], 0, L)]
    for k in range(1, 7):
        c.append(clamp(max(starts[k], c[k - 1]), 0, L))
    n = [c[k + 1] - c[k] for k in range(6)]
    z = draws(seed, sample)
    m = []
    for k in range(6):
        s = np.float64(1.0) + np.float64(amp[k]) * (np.float64(2.0) * np.float64(uniform(z[k])) - np.float64(1.0))
        if n[k] == 0:
            m.append(0)
        elif c[6] == L:
            m.append(n[k])
        else:
            m.append(max(1, int(np.floor(np.float64(n[k]) * s + np.float64(0.5)))))
    d = [c[0]]
    for k in range(6):
        d.append(min(d[k] + m[k], L))
    jit = [jitter_of(z[k], J) for k in range(6)]
    e = [d[0]]
    for k in range(1, 6):
        e.append(clamp(d[k] + jit[k], e[k - 1], d[6]))
    e.append(d[6])
    return dict(c=c, n=n, m=m, d=d, e=e, jit=jit)


def warp_row(x, tb):
    """One float32 row resampled under the sample's tables."""
    L = x.shape[0]
    c, n, m, d = tb["c"], tb["n"], tb["m"], tb["d"]
    y = np.zeros(L, dtype=np.float32)
    y[:d[0]] = x[:d[0]]
    x64 = x.astype(np.float64)
    for k in range(6):
        if d[k + 1] <= d[k]:
            continue
        j = np.arange(d[k + 1] - d[k], dtype=np.float64)
        r = np.float64(n[k]) / np.float64(m[k])
        p = (j + 0.5) * r - 0.5
        p = np.minimum(np.maximum(p, 0.0), np.float64(n[k] - 1))
        fl = np.floor(p)
        i0 = fl.astype(np.int64)
        i1 = np.minimum(i0 + 1, n[k] - 1)
        f = p - fl
        x0, x1 = x64[c[k] + i0], x64[c[k] + i1]
        with np.errstate(invalid="ignore", over="ignore"):
            blend = (x0 + f * (x1 - x0)).astype(np.float32)
        y[d[k]:d[k + 1]] = np.where(f == 0.0, x[c[k] + i0], blend)
    return y


def warp(data, target, rest, rois, seed, amp, J, index0=0):
    """data [B, V, L], target [B, L] or [B, 1, L], rest [B, R, L] or None (float32), rois [B, 7, 2] integer ->
    (data, target, rest, rois int64, tables: the list of every sample's dict)."""
    data, target, rois = np.asarray(data), np.asarray(target), np.asarray(rois)
    assert data.dtype == np.float32 and target.dtype == np.float32 and (rest is None or np.asarray(rest).dtype == np.float32)
    B, V, L = data.shape
    assert L % 4 == 0 and rois.shape == (B, 7, 2)
    out_d, out_t = np.empty_like(data), np.empty_like(target)
    out_r = None if rest is None else np.empty_like(np.asarray(rest))
    out_rois = np.empty((B, 7, 2), dtype=np.int64)
    t2 = target.reshape(B, L)
    o2 = out_t.reshape(B, L)
    tbs = []
    for i in range(B):
        tb = tables(rois[i], L, seed, index0 + i, amp, J)
        tbs.append(tb)
        for v in range(V):
            out_d[i, v] = warp_row(data[i, v], tb)
        o2[i] = warp_row(t2[i], tb)
        if rest is not None:
            for q in range(out_r.shape[1]):
                out_r[i, q] = warp_row(np.asarray(rest)[i, q], tb)
        e = tb["e"]
        for k in range(6):
            out_rois[i, k] = (e[k], e[k + 1])
        out_rois[i, 6] = (e[6], int(rois[i, 6, 1]))
    return out_d, out_t, out_r, out_rois, tbs


# ------------------------------------------------------------------------------------------------ the cases both test files use
# name -> the seven starts of one sample's rois for L = 64 (ends: the next start, the last 64): every way a mark can be wrong
ADVERSARIAL = {
    "contiguous": [0, 6, 9, 20, 28, 40, 50],
    "from_3": [3, 6, 9, 20, 28, 40, 50],
    "negative": [-5, -2, 9, 20, 28, 40, 50],
    "huge": [0, 6, 9, 10 ** 12, 28, 40, 50],
    "non_monotone": [0, 30, 9, 20, 10, 40, 35],
    "beyond_L": [0, 6, 9, 20, 70, 80, 90],
    "all_beyond": [100, 200, 300, 400, 500, 600, 700],
    "all_negative": [-70, -60, -50, -40, -30, -20, -10],
    "empty_segments": [0, 0, 9, 9, 9, 40, 50],
    "cropped": [0, 6, 9, 20, 28, 40, 64],
    "int64_ends": [-2 ** 63, 6, 2 ** 63 - 1, 20, 28, 40, 50],
}


def adversarial_rois(name, L=64):
    s = ADVERSARIAL[name]
    r = np.zeros((1, 7, 2), dtype=np.int64)
    r[0, :, 0] = s
    r[0, :6, 1] = s[1:]
    r[0, 6, 1] = L
    if name == "non_monotone":
        r[0, :, 1] = [5, 3, 99, -4, 0, 7, 12345]          # ends are not read, apart from the last, which passes through
    return r


def golden():
    z = np.load(GOLDEN)
    return (z["data"].astype(np.float32), z["target_view"].astype(np.float32), z["rest_view"].astype(np.float32),
            z["rois"].astype(np.int64))
