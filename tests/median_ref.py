"""Restatement of the sliding median (include/nefnet_hip.h, nef_sliding_median_args) and of the store's cleaning chain
(electrocardio_panorama_amd/clean.py), so that nef_sliding_median can be held to it with exact comparisons: the median of
an odd window is one of its elements, nothing is summed.

`sliding_median` is numpy.median over every window of the edge-padded float32 row (NaN if the window holds one: numpy's rule);
`sliding_median_loop` is the literal sort-and-pick form for short rows; `subtract` is the minuend form's one rounding; `notch_apply` runs a
clean.notch_taps row through tests/resample_ref.py at 1/1; `clean` chains them as ResidentTianchi._clean does."""
import math
import warnings

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import resample_ref


def sliding_median(x, h):
    """x: [..., len] rows (int16 or float32), h >= 0.  float32 [..., len]: the (h + 1)-th smallest of x[clamp(t - h .. t + h)]."""
    x = np.asarray(x).astype(np.float32)
    pad = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(h, h)], mode="edge")
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # "invalid value" of a window that holds a NaN
        return np.median(sliding_window_view(pad, 2 * h + 1, axis=-1), axis=-1).astype(np.float32)


def sliding_median_loop(x, h):
    """One row, one window at a time: clamp, sort, pick element h; NaN if the window holds a NaN."""
    x = [float(np.float32(v)) for v in np.asarray(x)]
    n = len(x)
    out = np.empty(n, dtype=np.float32)
    for t in range(n):
        win = [x[min(max(t + j, 0), n - 1)] for j in range(-h, h + 1)]
        out[t] = np.float32(float("nan") if any(math.isnan(v) for v in win) else sorted(win)[h])
    return out


def subtract(minuend, m):
    """The minuend form: float32(float64(minuend) - float64(m)), one rounding."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(minuend).astype(np.float64) - np.asarray(m).astype(np.float64)).astype(np.float32)


def notch_apply(x, taps, first):
    """x: [..., len] rows through the one-phase table of clean.notch_taps: float32 [..., len], resample_ref's sums at 1/1."""
    return resample_ref.resample(x, taps, first, 1, 1)


def baseline_remove(x, h1, h2):
    """x - median_h2(median_h1(x)) as the store forms it: float32 at every stage."""
    return subtract(x, sliding_median(sliding_median(x, h1), h2))


def clean(x, plan, notch=None):
    """A recording [8, len] through the CleanPlan's stages; `notch` = clean.notch_taps(...) when plan.mains_hz > 0."""
    y = np.asarray(x)
    if plan.mains_hz > 0:
        y = notch_apply(y, notch[0], notch[1])
    if plan.h1 > 0:
        y = baseline_remove(y, plan.h1, plan.h2)
    return y.astype(np.float32)
