"""Literal-loop restatements of nef_mark_envelope, nef_mark_peaks (include/nefnet_hip.h) and dataset/marks.py's labels_from_peaks: one
Python statement per arithmetic step, in the order the header states, so that the device result can be held to them bit for bit.  Slow on
purpose; the tests run them once per module on short recordings."""
import math

import numpy as np


def envelope(x, D=2, H=20, lead_bits=255):
    """x: [8, len] stored values (int16 or float32).  float64 [len]."""
    x = np.asarray(x)
    n = x.shape[1]
    xs = [[float(v) for v in x[c]] for c in range(8)]
    e = [0.0] * n
    for t in range(n):
        s = 0.0
        for c in range(8):
            if (lead_bits >> c) & 1:
                d = xs[c][min(t + D, n - 1)] - xs[c][max(t - D, 0)]
                p = d * d
                s = s + p
        e[t] = s
    env = np.empty(n, dtype=np.float64)
    for t in range(n):
        s = 0.0
        for u in range(max(t - H, 0), min(t + H, n - 1) + 1):
            s = s + e[u]
        env[t] = s
    return env


def peaks(env, r=100, seg=1000, frac=0.125, max_peaks=256):
    """env: float64 [len].  (peaks int32 [max_peaks] with -1 behind the count, count, level)."""
    env = [float(v) for v in np.asarray(env, dtype=np.float64)]
    n = len(env)
    row = np.full(max_peaks, -1, dtype=np.int32)
    if any(math.isnan(v) or math.isinf(v) for v in env):
        return row, -1, float('nan')
    nseg = max(n // seg, 1)
    maxima = []
    for i in range(nseg):
        b, e = i * seg, (n if i == nseg - 1 else (i + 1) * seg)
        m = env[b]
        for t in range(b + 1, e):
            if env[t] > m:
                m = env[t]
        maxima.append(m)
    level = sorted(maxima)[(nseg - 1) // 2]
    thr = level * frac
    count = 0
    for t in range(n):
        v = env[t]
        if not (v > 0.0 and v >= thr):
            continue
        ok = True
        for u in range(max(t - r, 0), t):
            if not env[u] < v:
                ok = False
                break
        if ok:
            for u in range(t + 1, min(t + r, n - 1) + 1):
                if not env[u] <= v:
                    ok = False
                    break
        if ok:
            if count < max_peaks:
                row[count] = t
            count += 1
    return row, count, level


def labels_from_peaks(peaks, count, lengths, table):
    """The loop form of dataset/marks.py's labels_from_peaks.  peaks [N, max_peaks], count [N], lengths [N], table [6, 2] (a_k, b_k).
    Returns (six lists of per-recording int lists, dropped [N], adjusted [N])."""
    peaks, table = np.asarray(peaks), np.asarray(table, dtype=np.float64)
    N, max_peaks = peaks.shape
    out = [[[] for _ in range(N)] for _ in range(6)]
    dropped, adjusted = [0] * N, [0] * N
    for i in range(N):
        P, n = int(count[i]), int(lengths[i])
        dropped[i] = max(P, 0)
        if P < 2 or P > max_peaks:
            continue
        p = [int(v) for v in peaks[i, :P]]
        beats = []
        for j in range(P):
            rr_next = p[j + 1] - p[j] if j + 1 < P else p[j] - p[j - 1]
            rr_prev = p[j] - p[j - 1] if j > 0 else p[j + 1] - p[j]
            m = []
            for k in range(6):
                rr = rr_prev if k < 2 else rr_next
                m.append(p[j] + int(math.floor(float(table[k, 0]) + float(table[k, 1]) * float(rr) + 0.5)))
            beats.append(m)
        first = 0
        for j in range(P):
            if beats[j][0] < 0:
                first = j + 1
        last = P
        for j in range(P):
            if beats[j][5] > n - 1:
                last = j
                break
        before = [v for m in beats[first:last] for v in m]
        flat = list(before)
        for q in range(1, len(flat)):
            if flat[q] < flat[q - 1] + 1:
                flat[q] = flat[q - 1] + 1
        nb = len(flat) // 6
        while nb > 0 and flat[6 * nb - 1] > n - 1:
            nb -= 1
        if nb < 2:
            continue
        dropped[i] = P - nb
        adjusted[i] = sum(1 for q in range(6 * nb) if flat[q] != before[q])
        for b in range(nb):                            # the last beat is not drawable: its 'P on' closes the one before it
            for k in range(6):
                out[k][i].append(flat[6 * b + k])
    return out, dropped, adjusted
