"""Literal restatement of the rational polyphase resampler (include/nefnet_hip.h, nef_resample_args; electrocardio_panorama_amd/resample.py):
one Python statement per arithmetic step, in the order the header states, so that nef_resample can be held to it bit for bit.

`design` restates the table, `resample_loop` one row output by output; `resample` is the same sum with the outputs side by side in numpy --
every multiply and add still one IEEE fp64 operation, in the same order -- for the rows a loop would take seconds over (the CPU tests hold
the two to each other).  `rescale_marks` is the label rescale as a loop."""
import math

import numpy as np


def ratio(src, dst):
    g = math.gcd(int(src), int(dst))
    return int(dst) // g, int(src) // g


def out_len(length, up, down):
    return (int(length) * up + down - 1) // down


def prototype(up, down, zeros=16, beta=8.6):
    """(h float64 [2 c + 1], c, m)."""
    m = max(up, down)
    c = zeros * m
    N = 2 * c + 1
    w = np.kaiser(N, beta)
    h = np.empty(N, dtype=np.float64)
    for n in range(N):
        h[n] = np.sinc((n - c) / m) * w[n]
    return h, c, m


def design(up, down, zeros=16, beta=8.6, normalise=True):
    """(taps float64 [up, K], first int32 [up]); normalise False leaves raw[p, k]."""
    h, c, _ = prototype(up, down, zeros, beta)
    first = [-((c - p) // up) for p in range(up)]                  # ceil((p - c) / up)
    cnt = [(p + c) // up - first[p] + 1 for p in range(up)]
    K = max(cnt)
    taps = np.zeros((up, K), dtype=np.float64)
    for p in range(up):
        s = 0.0
        for k in range(K):
            taps[p, k] = h[p + c - (first[p] + k) * up] if k < cnt[p] else 0.0
            s = s + taps[p, k]
        if normalise:
            for k in range(K):
                taps[p, k] = taps[p, k] / s
    return taps, np.array(first, dtype=np.int32)


def resample_loop(x, taps, first, up, down):
    """x: one row (int16 or float32, any length >= 1).  float32 [out_len]."""
    x = np.asarray(x)
    n, K = x.shape[0], taps.shape[1]
    xs = [float(v) for v in x]
    tp = [[float(v) for v in row] for row in taps]
    y = np.empty(out_len(n, up, down), dtype=np.float32)
    for m in range(y.shape[0]):
        i0, p = (m * down) // up, (m * down) % up
        s = 0.0
        for k in range(K):
            i = min(max(i0 + int(first[p]) + k, 0), n - 1)
            t = tp[p][k] * xs[i]
            s = s + t
        y[m] = np.float32(s)
    return y


def resample(x, taps, first, up, down, keep_fp64=False):
    """x: [..., len] rows (int16 or float32).  float32 [..., out_len]: resample_loop's sums, the outputs of all rows side by side
    (keep_fp64: the sums before the store)."""
    x = np.asarray(x)
    n, K = x.shape[-1], taps.shape[1]
    xd = x.astype(np.float64)
    m = np.arange(out_len(n, up, down), dtype=np.int64)
    i0, p = (m * down) // up, (m * down) % up
    start = i0 + first.astype(np.int64)[p]
    s = np.zeros(x.shape[:-1] + m.shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            t = taps[p, k] * xd[..., np.clip(start + k, 0, n - 1)]
            s = s + t
        return s if keep_fp64 else s.astype(np.float32)


def rescale_marks(lab, up, down):
    """Six lists of one recording -> (six lists on the new axis, marks the strictly-increasing pass moved)."""
    out = [[(2 * int(v) * up + down) // (2 * down) for v in lst] for lst in lab]
    moved, last = 0, None
    for j in range(max(len(lst) for lst in out)):
        for k in range(6):
            if j < len(out[k]):
                if last is not None and out[k][j] < last + 1:
                    out[k][j] = last + 1
                    moved += 1
                last = out[k][j]
    return out, moved
