"""Resampling in time by a rational factor: the host half (DATA.source_rate).

Every count of samples in the project -- the 512-sample beat, the detector's windows, the timing table, the augmentation's frequencies, the
SSIM window -- is a count at DATA.sample_rate.  A recording stored at another rate enters through one polyphase FIR, run on the device
(ops.resample, nef_resample) from a table designed here in fp64: `design` makes the taps, `ratio` the two integers of a pair of rates,
`rescale_all` moves annotated label lists to the new time axis.  The device receives the table, so its result is defined bit for bit by
what `design` returns (include/nefnet_hip.h, nef_resample_args)."""
import math

import numpy as np

MAX_UP, MAX_K, MAX_RATIO = 1024, 512, 8          # NEF_RESAMPLE_MAX_UP, _MAX_K, _MAX_RATIO (include/nefnet_hip.h)


def check_rate(name, v):
    """A rate in Hz as a positive int: ints and integral floats pass (500.0 is 500), everything else is a ValueError naming `name`."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v or v in (float('inf'), float('-inf')) \
            or v != int(v):
        raise ValueError(f"{name} = {v!r}: a rate is a whole number of Hz")
    if v <= 0:
        raise ValueError(f"{name} = {v!r}: a rate is a positive number of Hz")
    return int(v)


def ratio(src_rate, dst_rate):
    """(up, down) that take `src_rate` Hz to `dst_rate` Hz: dst / g and src / g, g their gcd."""
    src, dst = check_rate("src_rate", src_rate), check_rate("dst_rate", dst_rate)
    g = math.gcd(src, dst)
    return dst // g, src // g


def out_len(length, up, down):
    """Samples a row of `length` gives: ceil(length * up / down) (an int, or an int64 array)."""
    return (length * up + down - 1) // down


def design(up, down, zeros=16, beta=8.6):
    """The polyphase table of a Kaiser-windowed sinc that cuts at the lower of the two rates: (taps float64 [up, K], first int32 [up]).
    m = max(up, down), c = zeros * m, h[n] = sinc((n - c) / m) * kaiser(2 c + 1, beta)[n]; phase p reads the inputs first[p] .. first[p] +
    cnt[p] - 1 relative to (m * down) // up, raw[p, k] = h[p + c - (first[p] + k) * up], padded with 0.0 to K = max cnt, and every row is
    divided by its sum (ascending k), so that a constant row comes out as that constant."""
    for name, v in (("up", up), ("down", down), ("zeros", zeros)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} = {v!r}: an integer >= 1")
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 <= float(beta) < float('inf'):
        raise ValueError(f"beta = {beta!r}: a finite number >= 0")
    up, down, zeros = int(up), int(down), int(zeros)
    m = max(up, down)
    c = zeros * m
    N = 2 * c + 1
    n = np.arange(N, dtype=np.float64)
    h = np.sinc((n - c) / m) * np.kaiser(N, float(beta))
    p = np.arange(up, dtype=np.int64)
    first = -((c - p) // up)                            # ceil((p - c) / up)
    cnt = (p + c) // up - first + 1
    K = int(cnt.max())
    k = np.arange(K, dtype=np.int64)
    idx = p[:, None] + c - (first[:, None] + k[None, :]) * up
    live = k[None, :] < cnt[:, None]
    raw = np.where(live, h[np.clip(idx, 0, N - 1)], 0.0)
    s = np.zeros(up, dtype=np.float64)
    for j in range(K):                                  # ascending k
        s = s + raw[:, j]
    return np.ascontiguousarray(raw / s[:, None]), np.ascontiguousarray(first.astype(np.int32))


def taps_per_phase(up, down, zeros=16):
    """K of design(up, down, zeros): the most inputs a phase reads."""
    c = zeros * max(up, down)
    p = np.arange(up, dtype=np.int64)
    return int(((p + c) // up + (c - p) // up + 1).max())


def check_ratio(up, down, zeros=None, src_rate=None, dst_rate=None):
    """The limits of nef_resample: up <= 1024, down <= 8 up and, with `zeros`, at most 512 taps a phase; a ValueError naming the two
    rates otherwise."""
    what = f"{src_rate} Hz -> {dst_rate} Hz" if src_rate is not None else f"up {up}, down {down}"
    if up > MAX_UP:
        raise ValueError(f"{what}: up = {up} is above {MAX_UP}; nef_resample does not take the ratio")
    if down > MAX_RATIO * up:
        raise ValueError(f"{what}: down = {down} is above {MAX_RATIO} x up = {up}; nef_resample does not take the ratio")
    if zeros is not None and taps_per_phase(up, down, zeros) > MAX_K:
        raise ValueError(f"{what}: {zeros} zero crossings a side make {taps_per_phase(up, down, zeros)} taps a phase, above {MAX_K}; "
                         "nef_resample does not take the filter")


def increasing(values, groups):
    """Make flat int64 `values` strictly increasing within every run of equal `groups` (non-decreasing ids below 2^22) by
    v_i = max(v_i, v_{i-1} + 1); returns (fixed, changed mask).  |values| stays below 2^40."""
    v, g = np.asarray(values, dtype=np.int64).reshape(-1), np.asarray(groups, dtype=np.int64).reshape(-1)
    i = np.arange(v.size, dtype=np.int64)
    fixed = np.maximum.accumulate(v - i + g * _BIG) - g * _BIG + i        # v_i - i is made non-decreasing; _BIG keeps the groups apart
    return fixed, fixed != v


_BIG = 1 << 40


def rescale_all(labs, up, down):
    """The label lists of N recordings (`labs`: per recording six integer lists) on the resampled time axis, all recordings in one pass:
    mark' = (2 mark up + down) // (2 down) -- mark * up / down rounded half up -- and then, per recording in time order (P on, P off, R on,
    R off, T on, T off of beat 0, then beat 1 ...; a list may be shorter than another), made strictly increasing by
    m_i = max(m_i, m_{i-1} + 1).  Returns (six int64 arrays, each concatenated over the recordings, six int64 [N + 1] offsets into them
    -- ResidentTianchi's `labels` / `label_offsets` -- and the number of marks the fix-up moved)."""
    N = len(labs)
    cols = [[np.asarray(lab[k], dtype=np.int64).reshape(-1) for lab in labs] for k in range(6)]
    sizes = np.array([[v.size for v in col] for col in cols], dtype=np.int64).reshape(6, N)
    offsets = [np.concatenate([[0], np.cumsum(sizes[k])]).astype(np.int64) for k in range(6)]
    vals = [(2 * (np.concatenate(col) if N else np.zeros(0, dtype=np.int64)) * up + down) // (2 * down) for col in cols]
    rec = [np.repeat(np.arange(N, dtype=np.int64), sizes[k]) for k in range(6)]
    key = [(np.arange(vals[k].size, dtype=np.int64) - offsets[k][rec[k]]) * 6 + k for k in range(6)]
    flat, frec = np.concatenate(vals), np.concatenate(rec)
    order = np.lexsort((np.concatenate(key), frec))
    fixed, changed = increasing(flat[order], frec[order])
    flat[order] = fixed
    return np.split(flat, np.cumsum([v.size for v in vals])[:-1]), offsets, int(changed.sum())


def rescale_marks(lab, up, down):
    """One recording's six label lists through rescale_all: (six int64 arrays, number of marks the fix-up moved)."""
    labels, _, moved = rescale_all([lab], up, down)
    return labels, moved
