"""Numpy restatement of the input-lead augmentation (DATA.aug_*; the definition in include/nefnet_hip.h, nef_augment_args): uint64
wrap-around arithmetic for the counter RNG's mix, fp64 for everything else.  Shares no code with the package."""
import numpy as np

M64 = (1 << 64) - 1
ROW_BASE = 1 << 62
TWO24 = 16777216.0


def mix(seed, counter):
    """nef_rng_mix (csrc/nef_common.h) on uint64 arrays: `seed` a Python int, `counter` an array (or int) of counters."""
    with np.errstate(over="ignore"):
        c = np.asarray(counter, dtype=np.uint64)
        z = c + np.uint64((int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def k0(z):
    return (z >> np.uint64(40)).astype(np.int64)


def k1(z):
    return ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)


def normals(seed, n, first=0):
    """(values, r) of elements first .. first + n - 1 of the per-element Gaussian stream (first even)."""
    assert first % 2 == 0
    pairs = np.arange(first // 2, (first + n + 1) // 2, dtype=np.uint64)
    z = mix(seed, pairs)
    r = np.sqrt(-2.0 * np.log((k0(z) + 1) / TWO24))
    ang = 2.0 * np.pi * (k1(z) / TWO24)
    vals = np.stack([r * np.cos(ang), r * np.sin(ang)], 1).reshape(-1)[:n]
    return vals, np.repeat(r, 2)[:n]


def row_draws(seed, B, V):
    """The per-row words: dict of [B, V] arrays (k0 / k1 of j = 0, 1, 2) and the per-sample fallback lead [B]."""
    rows = np.arange(B * V, dtype=np.uint64).reshape(B, V)
    base = np.uint64(ROW_BASE) + np.uint64(4) * rows
    z = [mix(seed, base + np.uint64(j)) for j in range(3)]
    z3 = mix(seed, base[:, 0] + np.uint64(3))
    fallback = (V * k0(z3)) >> 24
    return z, fallback


def dropped_rows(seed, B, V, p):
    """(dropped [B, V] bool, drew [B, V] bool: the raw draws before the fallback)."""
    z, fallback = row_draws(seed, B, V)
    u_d = (k1(z[2]) / TWO24).astype(np.float32)
    drew = u_d < np.float32(p)
    dropped = drew.copy()
    for b in np.nonzero(drew.all(axis=1))[0]:
        dropped[b, fallback[b]] = False
    return dropped, drew


def augment(x, rois, seed, noise_std=0.0, wander_amp=0.0, wander_hz=(0.05, 0.7), hum_amp=0.0, hum_hz=50.0, lead_drop=0.0,
            sample_rate=500.0, crop=True):
    """x [B, V, L] float32, rois [B, R, 2] integer -> (y float64 [B, V, L], dropped [B, V] bool, M float64 [B, V, L]) with
    M = |x| + sigma r + A_w + A_h per element, the magnitude the tolerance of a comparison scales with."""
    x = np.asarray(x)
    B, V, L = x.shape
    assert x.dtype == np.float32 and L % 4 == 0
    x64 = x.astype(np.float64)
    z, _ = row_draws(seed, B, V)
    dropped = dropped_rows(seed, B, V, lead_drop)[0] if lead_drop > 0 else np.zeros((B, V), bool)
    end = np.clip(np.asarray(rois)[:, -1, 0].astype(np.int64), 0, L) if crop else np.full(B, L, np.int64)
    t = np.arange(L, dtype=np.float64)
    add = np.zeros((B, V, L))
    M = np.abs(x64)
    if noise_std > 0:
        sigma = float(np.float32(noise_std))
        n, r = normals(seed, B * V * L)
        add += sigma * n.reshape(B, V, L)
        M = M + sigma * r.reshape(B, V, L)
    if wander_amp > 0:
        lo, hi = wander_hz
        A = wander_amp * (k0(z[0]) / TWO24)
        f = lo + (hi - lo) * (k1(z[0]) / TWO24)
        phi = k0(z[1]) / TWO24
        add += A[..., None] * np.sin(2.0 * np.pi * (f[..., None] * t / sample_rate + phi[..., None]))
        M = M + A[..., None]
    if hum_amp > 0:
        A = hum_amp * (k1(z[1]) / TWO24)
        phi = k0(z[2]) / TWO24
        add += A[..., None] * np.sin(2.0 * np.pi * (hum_hz * t / sample_rate + phi[..., None]))
        M = M + A[..., None]
    live = t[None, None, :] < end[:, None, None]
    y = np.where(live, x64 + add, x64)
    y[dropped] = 0.0
    return y, dropped, M
