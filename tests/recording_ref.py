"""numpy fp64 restatement, in literal loops, of the whole-recording path: the plan of all beats and its three tables
(dataset/resident.py recording_plan), a beat's range (nef_beat_range), the stitch in both fill modes (nef_beat_stitch) and the seven sums
with rmse / corr (nef_recording_stats, recording.metrics).  Definitions: include/nefnet_hip.h."""
import numpy as np

import resident_ref as rr

L = 512


def store_recording(store, i):
    """(signal [8, len] as stored, {key: list}) of recording i of a ResidentTianchi."""
    s8 = store.signal[int(store.offsets[i]):int(store.offsets[i + 1])].cpu().numpy().reshape(8, -1)
    lab = {k: store.labels[q][store.label_offsets[q][i]:store.label_offsets[q][i + 1]].tolist() for q, k in enumerate(rr.KEYS)}
    return s8, lab


def twelve(s8):
    s = np.asarray(s8).astype(np.float64)
    i, ii = s[0:1], s[1:2]
    return np.concatenate([s, ii - i, -0.5 * (i + ii), i - 0.5 * ii, ii - 0.5 * i], axis=0)


def plan_tables(store, indices, input_leads, A=12):
    """table [Bt, 3 + V + 1], rois [Bt, 7, 2], rec [Bt], beats [Bt], stitch [Bt, 4], recordings [N, 4], out_offsets [N + 1], ids."""
    table, rois, rec, beats, stitch, recs, ids = [], [], [], [], [], [], []
    offs, row = [0], 0
    for j, i in enumerate(indices):
        p = store.labels[0][store.label_offsets[0][i]:store.label_offsets[0][i + 1]].tolist()
        marks = [store.labels[q][store.label_offsets[q][i]:store.label_offsets[q][i + 1]].tolist() for q in range(6)]
        ln = int(store.lengths[i])
        recs.append([row, len(p) - 1, int(store.offsets[i]), ln])
        for k in range(len(p) - 1):
            p_on, end = p[k], p[k + 1]
            edges = [marks[q][k] for q in range(6)] + [end, L + p_on]
            table.append([int(store.offsets[i]) + p_on, ln, end - p_on] + list(input_leads) + [input_leads[0]])
            rois.append([[edges[q] - p_on, edges[q + 1] - p_on] for q in range(7)])
            rec.append(j)
            beats.append(k)
            stitch.append([offs[-1] + p_on, ln, end - p_on, 1 if k + 1 < len(p) - 1 else 0])
            ids.append(store.names[i])
            row += 1
        offs.append(offs[-1] + A * ln)
    as64 = lambda a, shape: np.array(a, dtype=np.int64).reshape(shape)      # noqa: E731
    V = len(input_leads)
    return dict(table=as64(table, (-1, 3 + V + 1)), rois=as64(rois, (-1, 7, 2)), rec=as64(rec, (-1,)), beats=as64(beats, (-1,)),
                stitch=as64(stitch, (-1, 4)), recordings=as64(recs, (-1, 4)), out_offsets=as64(offs, (-1,)), ids=ids)


def beat_range(signal, off, stride, n):
    """(lo, hi) of the beat at flat offset `off` of lead 0 over all 12 leads; signal: the store's flat numpy array."""
    s8 = np.stack([signal[off + k * stride:off + k * stride + n] for k in range(8)])
    s = twelve(s8)
    return np.min(s), np.max(s)


def ranges(signal, table):
    return np.array([beat_range(signal, int(r[0]), int(r[1]), int(r[2])) for r in table], dtype=np.float64).reshape(-1, 2)


def _denorm(v, lo, hi):
    span = hi - lo
    if not np.isfinite(span):
        return np.full(np.shape(v), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        return lo + np.asarray(v, dtype=np.float64) * span


def stitch(views, rng, table, out, fill):
    """views [Bt, A, 512] float32, rng [Bt, 2] fp64, table [Bt, 4] -> writes `out` (flat float32) in place, as nef_beat_stitch does."""
    Bt, A = views.shape[:2]
    for b in range(Bt):
        base, stride, n, link = (int(v) for v in table[b])
        if base < 0 or stride < 1 or n < 1 or n > stride or base + (A - 1) * stride + n > out.size:
            continue
        lo, hi = rng[b]
        m = min(n, L)
        for a in range(A):
            o = base + a * stride
            with np.errstate(invalid="ignore", over="ignore"):
                out[o:o + m] = _denorm(views[b, a, :m], lo, hi).astype(np.float32)
            if n <= L:
                continue
            if fill in ("nan", 0):
                out[o + L:o + n] = np.nan
                continue
            a0 = float(_denorm(views[b, a, L - 1], lo, hi))
            a1 = float(_denorm(views[b + 1, a, 0], rng[b + 1][0], rng[b + 1][1])) if link == 1 and b + 1 < Bt else a0
            for t in range(L, n):
                with np.errstate(invalid="ignore", over="ignore"):
                    out[o + t] = np.float32(a0 + (a1 - a0) * (np.float64(t - (L - 1)) / np.float64(n - (L - 1))))
    return out


def stats(out, signal, beat_table, rec_table, out_offsets, score_leads, fill):
    """([N, A, 7] sums, [N, A, 7] sums of the terms' magnitudes) -- count, d^2, u, w, u^2, w^2, u w -- in position order."""
    N, A = rec_table.shape[0], len(score_leads)
    res, mag = np.zeros((N, A, 7)), np.zeros((N, A, 7))
    for i in range(N):
        first, rows, soff, ln = (int(v) for v in rec_table[i])
        s12 = twelve(signal[soff:soff + 8 * ln].reshape(8, ln))
        for a, lead in enumerate(score_leads):
            if lead == -1 or rows == 0:
                continue
            xs, ys = [], []
            for b in range(first, first + rows):
                p = int(beat_table[b][0]) - int(out_offsets[i])
                n = int(beat_table[b][2])
                cover = n if fill in ("bridge", 1) else min(n, L)
                xs.append(out[int(out_offsets[i]) + a * ln + p:int(out_offsets[i]) + a * ln + p + cover].astype(np.float64))
                ys.append(s12[lead, p:p + cover])
            x, y = np.concatenate(xs), np.concatenate(ys)
            d, u, w = x - y, x - x[0], y - y[0]
            terms = [np.ones_like(x), d * d, u, w, u * u, w * w, u * w]
            res[i, a] = [np.sum(t) for t in terms]
            mag[i, a] = [np.sum(np.abs(t)) for t in terms]
    return res, mag


def metrics(st):
    """(rmse, corr) [N, A] from the seven sums."""
    st = np.asarray(st, dtype=np.float64)
    rmse, corr = np.full(st.shape[:-1], np.nan), np.full(st.shape[:-1], np.nan)
    for idx in np.ndindex(*st.shape[:-1]):
        cnt, se, su, sw, suu, sww, suw = st[idx]
        if not cnt >= 2:
            continue
        rmse[idx] = np.sqrt(se / cnt)
        vx, vy, c = suu - su * su / cnt, sww - sw * sw / cnt, suw - su * sw / cnt
        if vx * vy > 0:
            corr[idx] = c / np.sqrt(vx * vy)
    return rmse, corr
