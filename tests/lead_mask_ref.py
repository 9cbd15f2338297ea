"""Numpy restatement of the lead-mask head (MODEL.lead_mask; the definition in include/nefnet_hip.h, nef_lead_mask_mix_fwd_args): the
present-lead lists, the Standin picks, the mean and D in fp64 and in the defined fp32 order, the adjoint in fp64 with the magnitudes the
tolerances scale with, and the drop mask through tests/augment_ref.py's decisions.  Shares no code with the package."""
import numpy as np

import augment_ref

U24 = 2.0 ** -24


def present_lists(mask):
    """P_b for every sample: ascending v with mask[b, v] != 0."""
    mask = np.asarray(mask)
    return [[v for v in range(mask.shape[1]) if mask[b, v] != 0] for b in range(mask.shape[0])]


def picks(mask, c1, c2):
    """int64 [B, 2]: (P_b[c1 mod n_b], P_b[c2 mod n_b]); (-1, -1) for n_b = 0."""
    out = np.full((np.asarray(mask).shape[0], 2), -1, np.int64)
    for b, P in enumerate(present_lists(mask)):
        if P:
            out[b] = (P[c1 % len(P)], P[c2 % len(P)])
    return out


def _leads(z, V):
    z = np.asarray(z)
    B, Ct, T = z.shape
    assert Ct == 128 * V
    return z.reshape(B, V, 128, T)


def forward(z1, z2r, mask, q, c1, c2, dtype=np.float64):
    """(latent [B, 256, T], D [3B, 256, T] or None with q None, A [B, 256, T] = sum over the present leads of |z|) in `dtype`: float64 is
    the exact reference, float32 replays the defined order (first present lead, += in ascending order, one division by (float)n_b, one
    rounded multiply by q per D element).  Absent leads are never touched: NaNs there do not show."""
    mask = np.asarray(mask)
    B, V = mask.shape
    Z = np.concatenate([_leads(z1, V), _leads(z2r, V)], axis=2).astype(dtype)      # [B, V, 256, T]
    T = Z.shape[3]
    latent = np.zeros((B, 256, T), dtype)
    A = np.zeros((B, 256, T), np.float64)
    D = None if q is None else np.zeros((3, B, 256, T), dtype)
    pk = picks(mask, c1, c2)
    for b, P in enumerate(present_lists(mask)):
        if not P:
            continue
        s = Z[b, P[0]].copy()
        for v in P[1:]:
            s = s + Z[b, v]
        latent[b] = s / dtype(len(P))
        A[b] = sum(np.abs(Z[b, v].astype(np.float64)) for v in P)
        if D is not None:
            f = np.asarray(q)[b].astype(dtype)[:, None]
            D[0, b] = f * latent[b]
            D[1, b] = f * np.concatenate([Z[b, pk[b, 0], :128], latent[b, 128:]], axis=0)
            D[2, b] = f * np.concatenate([latent[b, :128], Z[b, pk[b, 1], 128:]], axis=0)
    return latent, (None if D is None else D.reshape(3 * B, 256, T)), A


def up2_matrix(T):
    """U [2T, T]: Upsample(x2, linear, align_corners=False) of a length-T row, in fp64."""
    U = np.zeros((2 * T, T))
    for i in range(2 * T):
        src = max(0.5 * (i + 0.5) - 0.5, 0.0)
        i0 = min(int(src), T - 1)
        i1 = i0 + (1 if i0 < T - 1 else 0)
        l1 = src - i0
        U[i, i0] += 1.0 - l1
        U[i, i1] += l1
    return U


def backward(gD, latent, z1, z2r, q, mask, c1, c2, relu_z1=False, up=False):
    """The adjoint in fp64, from the latent the forward left (an input of the backward entry): (gz1, gz2r [B, 128V, T], gq [B, 256],
    Mz [B, 256, T] = |q| (|gD0| + |gD1| + |gD2|), Mq [B, 256] = the sum of the |products| behind gq).  `up`: gD is [3B, 256, 2T] and goes
    through the upsampling's adjoint first (the magnitudes through the adjoint of |gD|)."""
    mask = np.asarray(mask)
    B, V = mask.shape
    g = np.asarray(gD).astype(np.float64)
    ga = np.abs(g)
    if up:
        U = up2_matrix(g.shape[2] // 2)
        g, ga = g @ U, ga @ U
    T = g.shape[2]
    g, ga = g.reshape(3, B, 256, T), ga.reshape(3, B, 256, T)
    Z = np.concatenate([_leads(z1, V), _leads(z2r, V)], axis=2).astype(np.float64)
    lat = np.asarray(latent).astype(np.float64)
    qq = np.asarray(q).astype(np.float64)
    gZ = np.zeros((B, V, 256, T))
    gq = np.zeros((B, 256))
    Mq = np.zeros((B, 256))
    Mz = np.abs(qq)[:, :, None] * (ga[0] + ga[1] + ga[2])
    pk = picks(mask, c1, c2)
    first = (np.arange(256) < 128)[:, None]
    for b, P in enumerate(present_lists(mask)):
        if not P:
            Mz[b] = 0.0
            continue
        g_pick = np.where(first, g[1, b], g[2, b])
        g_mean = np.where(first, g[0, b] + g[2, b], g[0, b] + g[1, b])
        zp = np.concatenate([Z[b, pk[b, 0], :128], Z[b, pk[b, 1], 128:]], axis=0)
        gq[b] = (g_mean * lat[b] + g_pick * zp).sum(axis=1)
        Mq[b] = ((ga[0, b] + np.where(first, ga[2, b], ga[1, b])) * np.abs(lat[b]) + np.where(first, ga[1, b], ga[2, b]) * np.abs(zp)).sum(axis=1)
        f = qq[b][:, None]
        for v in P:
            pv = np.where(first, v == pk[b, 0], v == pk[b, 1])
            o = f * g_mean / len(P) + np.where(pv, f * g_pick, 0.0)
            if relu_z1:
                o[:128] = np.where(Z[b, v, :128] > 0, o[:128], 0.0)
            gZ[b, v] = o
    return gZ[:, :, :128].reshape(B, 128 * V, T), gZ[:, :, 128:].reshape(B, 128 * V, T), gq, Mz, Mq


def drop_mask(seed, B, V, lead_drop):
    """uint8 [B, V]: 0 where the augmentation zeroes the row (augment_ref.dropped_rows: row draw, all-dropped test, fallback lead)."""
    if not lead_drop > 0:
        return np.ones((B, V), np.uint8)
    return (~augment_ref.dropped_rows(seed, B, V, lead_drop)[0]).astype(np.uint8)
