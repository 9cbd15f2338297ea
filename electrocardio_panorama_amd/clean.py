"""Cleaning recordings of baseline wander and mains hum: the host half (DATA.baseline_ms, DATA.mains_hz).

Recordings from other sources arrive as they were recorded.  The store removes the two artefacts the augmentation adds (DATA.aug_wander_*,
DATA.aug_hum_*) on the device, behind the resampling and in front of the detector: a narrow band-stop at the mains frequency -- a
linear-phase FIR designed here in fp64 (`notch_taps`) and run by nef_resample at 1/1, so its result is defined bit for bit by the row --
and then the two-stage sliding-median baseline estimate of de Chazal et al. (200 ms, then 600 ms), subtracted (ops.sliding_median,
nef_sliding_median; `median_half` turns a window in milliseconds into the kernel's half width).  `clean_plan` reads the keys."""
import math
from typing import NamedTuple

import numpy as np

MAX_H = 512                 # NEF_MEDIAN_MAX_H (include/nefnet_hip.h)
MAX_TAPS = 511              # odd, and within NEF_RESAMPLE_MAX_K


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


def median_half(ms, rate, key="DATA.baseline_ms"):
    """The half width h of a sliding median of `ms` milliseconds at `rate` Hz: floor(ms * rate / 2000 + 0.5), the window being 2 h + 1
    samples (200 ms at 500 Hz: 50).  ValueError naming `key` and the rate for anything outside 1..512."""
    if not _number(ms) or not _number(rate) or ms <= 0 or rate <= 0:
        raise ValueError(f"{key} = {ms!r} ms at {rate!r} Hz: a window is a positive finite number of milliseconds at a positive rate")
    h = int(math.floor(float(ms) * float(rate) / 2000.0 + 0.5))
    if not 1 <= h <= MAX_H:
        raise ValueError(f"{key} = {ms!r} ms at {rate!r} Hz is a half width of {h} samples; nef_sliding_median takes 1..{MAX_H}")
    return h


def notch_taps(rate, hz, width_hz=6.0, taps=511, beta=8.6):
    """The band-stop [hz - width_hz / 2, hz + width_hz / 2] at `rate` Hz as a one-phase table for ops.resample(..., up=1, down=1), in
    resample.design's format: (taps float64 [1, K], first int32 [1]).  K = `taps`, c = (K - 1) / 2, n = -c .. c, f1 and f2 the band's
    edges over the rate: h[n] = -(2 f2 sinc(2 f2 n) - 2 f1 sinc(2 f1 n)) * kaiser(K, beta)[n], 1.0 added at n = 0, and the row divided by
    its sum (ascending n), so that a constant row comes out as that constant; first = [-c].  ValueError: K not odd or outside 3..511, a
    band that does not lie inside (0, rate / 2)."""
    if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not 3 <= taps <= MAX_TAPS or taps % 2 == 0:
        raise ValueError(f"taps = {taps!r}: an odd integer in 3..{MAX_TAPS}")
    if not _number(beta) or beta < 0:
        raise ValueError(f"beta = {beta!r}: a finite number >= 0")
    if not _number(rate) or not _number(hz) or not _number(width_hz) or rate <= 0 or width_hz <= 0:
        raise ValueError(f"rate {rate!r}, hz {hz!r}, width_hz {width_hz!r}: finite numbers, rate and width positive")
    rate, hz, width = float(rate), float(hz), float(width_hz)
    if not (0.0 < hz - width / 2 and hz + width / 2 < rate / 2):
        raise ValueError(f"the stop band {hz - width / 2} .. {hz + width / 2} Hz does not lie inside (0, {rate / 2}) Hz, half the rate {rate}")
    K = int(taps)
    c = (K - 1) // 2
    n = np.arange(-c, c + 1, dtype=np.float64)
    f1, f2 = (hz - width / 2) / rate, (hz + width / 2) / rate
    h = -(2 * f2 * np.sinc(2 * f2 * n) - 2 * f1 * np.sinc(2 * f1 * n)) * np.kaiser(K, float(beta))
    h[c] = h[c] + 1.0
    s = 0.0
    for v in h.tolist():                                # ascending n
        s = s + v
    return np.ascontiguousarray((h / s)[None, :]), np.array([-c], dtype=np.int32)


class CleanPlan(NamedTuple):
    """DATA.baseline_ms / DATA.mains_hz read: the medians' half widths (0, 0: no baseline stage) and the notch (mains_hz 0: none)."""
    h1: int
    h2: int
    mains_hz: float
    width: float
    taps: int
    beta: float
    rate: float


def clean_plan(cfg, need_resident=True):
    """None with DATA.baseline_ms [] and DATA.mains_hz 0, else the CleanPlan.  ValueError: a key without DATA.device_resident (the loaders;
    the store itself does not ask), a baseline_ms that is not [] or two positive finite numbers w1 <= w2 with half widths in 1..512 at
    DATA.sample_rate, a mains_hz that is negative or not finite, a band or a tap count notch_taps does not take."""
    base = cfg.DATA.get('baseline_ms', [])
    hz = cfg.DATA.get('mains_hz', 0.0)
    if not isinstance(base, (list, tuple)) or len(base) not in (0, 2) or not all(_number(v) and v > 0 for v in base) or \
            (len(base) == 2 and base[0] > base[1]):
        raise ValueError(f"DATA.baseline_ms = {base!r}: [] for off, or two positive finite numbers of milliseconds [w1, w2] with w1 <= w2")
    if not _number(hz) or hz < 0:
        raise ValueError(f"DATA.mains_hz = {hz!r}: a finite number of Hz >= 0; 0 for off, 50 or 60")
    if not base and hz == 0:
        return None
    if need_resident and not cfg.DATA.get('device_resident', False):
        raise ValueError("DATA.baseline_ms / DATA.mains_hz clean the recordings of the device-resident store: set DATA.device_resident (the "
                         "host loader stays file based; `python -m electrocardio_panorama_amd.mark_net --clean DIR` writes files for it)")
    rate = cfg.DATA.get('sample_rate', 500.0)
    if not _number(rate) or rate <= 0:
        raise ValueError(f"DATA.sample_rate = {rate!r}: a positive finite number of Hz")
    rate = float(rate)
    h1 = h2 = 0
    if base:
        h1, h2 = median_half(base[0], rate), median_half(base[1], rate)
    width, taps, beta = cfg.DATA.get('mains_width_hz', 6.0), cfg.DATA.get('mains_taps', 511), cfg.DATA.get('mains_beta', 8.6)
    if hz > 0:
        try:
            notch_taps(rate, hz, width, taps, beta)
        except ValueError as e:
            raise ValueError(f"DATA.mains_hz = {hz!r} (mains_width_hz {width!r}, mains_taps {taps!r}, mains_beta {beta!r}) at "
                             f"DATA.sample_rate {rate}: {e}") from None
    return CleanPlan(h1, h2, float(hz), float(width), int(taps), float(beta), rate)
