"""Cleaning recordings of baseline wander and mains hum without a device (DATA.baseline_ms, DATA.mains_hz): the
restatement (tests/median_ref.py) against a literal sort-and-pick loop, clean.median_half / notch_taps / clean_plan and their errors, the
band-stop's gains from the DFT of its row, what the two-stage median leaves of a planted wander on the two bundled recordings, the
detector (tests/marks_ref.py) on the corrupted and on the cleaned signal, the argument checks of ops.sliding_median and of the entry, and
the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import marks_ref as mref
import median_ref as mr
import resident_ref as rr
from electrocardio_panorama_amd import clean
from electrocardio_panorama_amd.dataset import resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = np.arange(5000, dtype=np.float64)


def wander(hz, amp=200.0, phase=0.7):
    return amp * np.sin(2 * np.pi * hz * T / 500 + phase)


def hum(hz=50.0, amp=40.0, phase=0.3):
    return amp * np.sin(2 * np.pi * hz * T / 500 + phase)


def corrupt(sig, addend):
    """The addend on every stored lead, rounded to int16."""
    return np.rint(sig.astype(np.float64) + addend).astype(np.int16)


@pytest.fixture(scope="module")
def recs():
    return rr.recordings()


@pytest.fixture(scope="module")
def cleaned(recs):
    """Per bundled recording: the clean recording's peaks, the corrupted signal (0.3 Hz wander + 50 Hz hum) and its cleaned form."""
    notch = clean.notch_taps(500, 50)
    out = []
    for _, sig, lab in recs:
        bad = corrupt(sig, wander(0.3) + hum())
        out.append(dict(sig=sig, lab=lab, bad=bad, clean=mr.baseline_remove(mr.notch_apply(bad, *notch), 50, 150)))
    return out


def test_restatement_is_the_sort_and_pick_loop():
    rng = np.random.default_rng(11)
    for n, h in ((1, 0), (1, 3), (2, 1), (5, 2), (7, 3), (8, 4), (40, 0), (40, 1), (40, 7), (40, 19), (40, 20), (40, 60), (130, 50)):
        for x in (rng.integers(-300, 300, n).astype(np.int16), (rng.standard_normal(n) * 50).astype(np.float32),
                  rng.integers(-2, 3, n).astype(np.float32)):
            assert np.array_equal(mr.sliding_median(x, h), mr.sliding_median_loop(x, h)), (n, h)
    x = (rng.standard_normal(60) * 50).astype(np.float32)
    x[7], x[30], x[31], x[50] = np.inf, -np.inf, np.inf, np.nan
    for h in (0, 1, 4, 11):
        got, want = mr.sliding_median(x, h), mr.sliding_median_loop(x, h)
        assert np.array_equal(np.isnan(got), np.abs(np.arange(60) - 50) <= h) and np.array_equal(got, want, equal_nan=True)
    # rows side by side are the rows one by one; the minuend form is one rounding of the fp64 difference
    x = rng.integers(-3000, 3000, (3, 200)).astype(np.int16)
    m = mr.sliding_median(x, 9)
    assert all(np.array_equal(m[r], mr.sliding_median_loop(x[r], 9)) for r in range(3))
    big = np.array([16777217, -32768, 3], dtype=np.float64)
    assert mr.subtract(np.array([1, -32768, 3], dtype=np.int16), np.array([-16777216.0, 0.5, 0.1], dtype=np.float32)).tolist() == \
        [float(np.float32(big[0])), float(np.float32(-32768.5)), float(np.float32(3.0 - float(np.float32(0.1))))]


def test_median_half_and_the_plans_errors(tmp_path):
    assert clean.median_half(200, 500) == 50 and clean.median_half(600, 500) == 150 and clean.median_half(200, 360) == 36
    assert clean.median_half(3, 500) == 1 and clean.median_half(2048, 500.0) == 512 and clean.median_half(101, 500) == 25
    for ms, rate in ((1, 500), (2050, 500), (0, 500), (-200, 500), (float("nan"), 500), (float("inf"), 500), (200, 0), (True, 500)):
        with pytest.raises(ValueError, match="DATA.baseline_ms") as e:
            clean.median_half(ms, rate)
        assert "Hz" in str(e.value)
    cfg = rr.make_cfg(rr.write_listing(tmp_path))
    assert cfg.DATA.baseline_ms == [] and cfg.DATA.mains_hz == 0.0 and cfg.DATA.mains_width_hz == 6.0 and cfg.DATA.mains_taps == 511 \
        and cfg.DATA.mains_beta == 8.6
    assert clean.clean_plan(cfg) is None
    cfg.DATA.device_resident = True
    assert clean.clean_plan(cfg) is None
    resident.check_cfg(cfg)
    cfg.DATA.baseline_ms, cfg.DATA.mains_hz = [200, 600], 50.0
    assert clean.clean_plan(cfg) == clean.CleanPlan(50, 150, 50.0, 6.0, 511, 8.6, 500.0)
    resident.check_cfg(cfg)
    cfg.DATA.mains_hz = 0.0
    assert clean.clean_plan(cfg)[:3] == (50, 150, 0.0)
    cfg.DATA.baseline_ms, cfg.DATA.mains_hz = [], 60.0
    assert clean.clean_plan(cfg)[:3] == (0, 0, 60.0)
    # the keys without the resident store: the message names the tool that writes files for the host loader
    cfg.DATA.device_resident = False
    for base, hz in (([200, 600], 0.0), ([], 50.0)):
        cfg.DATA.baseline_ms, cfg.DATA.mains_hz = base, hz
        with pytest.raises(ValueError, match="device_resident.*mark_net --clean"):
            clean.clean_plan(cfg)
        assert clean.clean_plan(cfg, need_resident=False) is not None
        from electrocardio_panorama_amd import train_net
        with pytest.raises(ValueError, match="device_resident"):
            train_net.build_loaders(cfg, batch_size=2)
    cfg.DATA.device_resident, cfg.DATA.mains_hz = True, 0.0
    for bad in ([200], [200, 600, 900], [600, 200], [0, 600], [-200, 600], [200, float("inf")], [float("nan"), 600], [True, 600], ["a", "b"]):
        cfg.DATA.baseline_ms = bad
        with pytest.raises(ValueError, match="DATA.baseline_ms"):
            resident.check_cfg(cfg)
    cfg.DATA.baseline_ms = [200, 2100]                                      # 525 samples of half width
    with pytest.raises(ValueError, match="DATA.baseline_ms.*500.0 Hz.*525"):
        resident.check_cfg(cfg)
    cfg.DATA.baseline_ms = []
    for bad in (-50.0, float("nan"), float("inf")):
        cfg.DATA.mains_hz = bad
        with pytest.raises(ValueError, match="DATA.mains_hz"):
            resident.check_cfg(cfg)
    cfg.DATA.mains_hz = 50.0
    for key, bad in (("mains_taps", 510), ("mains_taps", 513), ("mains_taps", 1), ("mains_width_hz", 100.0), ("mains_width_hz", 0.0),
                     ("mains_beta", -1.0)):
        good = cfg.DATA[key]
        cfg.DATA[key] = bad
        with pytest.raises(ValueError, match="DATA.mains_hz"):
            resident.check_cfg(cfg)
        cfg.DATA[key] = good
    cfg.DATA.mains_hz = 249.0                                               # the band's upper edge is above half the rate
    with pytest.raises(ValueError, match="half the rate"):
        resident.check_cfg(cfg)
    # a host store cannot clean: the error says so; off is the store the keys' absence gives
    cfg.DATA.mains_hz, cfg.DATA.baseline_ms = 50.0, [200, 600]
    with pytest.raises(RuntimeError, match="HIP device"):
        resident.ResidentTianchi(cfg, "train")
    cfg.DATA.mains_hz, cfg.DATA.baseline_ms = 0.0, []
    st = resident.ResidentTianchi(cfg, "train")
    assert st.clean is None and st.clean_report is None and st.signal.dtype == torch.int16


def _gain(row, rate):
    K = row.size
    n = np.arange(K, dtype=np.float64) - (K - 1) // 2
    return lambda hz: float(abs(np.sum(row * np.exp(-2j * np.pi * hz / rate * n))))


def _ascending_sum(row):
    s = 0.0
    for v in row.tolist():
        s = s + v
    return s


def test_notch_taps_gains_at_500_hz():
    """Measured: 3.9e-5 at 50 Hz, 0.00927 at 49 and 51 Hz, the pass band within 1.1e-5 of 1."""
    taps, first = clean.notch_taps(500, 50)
    assert taps.dtype == np.float64 and taps.shape == (1, 511) and first.dtype == np.int32 and first.tolist() == [-255]
    assert np.array_equal(taps[0], taps[0][::-1])                           # linear phase
    assert abs(_ascending_sum(taps[0]) - 1.0) <= 1e-15
    g = _gain(taps[0], 500.0)
    assert g(50) <= 1e-3 and g(49) <= 0.02 and g(51) <= 0.02
    for hz in (1, 5, 15, 40, 44, 56, 60, 100, 150, 249):
        assert abs(g(hz) - 1.0) <= 1e-3, hz


def test_notch_taps_gains_at_360_hz():
    """The same bars at (360, 60).  Measured on the restatement: 4.9e-5 at 60 Hz, 5.4e-5 and 5.3e-5 at 59 and 61 Hz; the pass band at 1, 5,
    15, 40, 44, 50, 54, 66, 70, 100, 150 and 179 Hz within 2.5e-5 of 1 (worst: 54 Hz, 2.4e-5; 66 Hz: 2.3e-5).  The 500 Hz list's 56, 60 and
    249 Hz are no pass band here: 60 Hz is the stop itself, 249 Hz is above half the rate, and 56 Hz lies inside the transition (the band's
    edge is 57 Hz and the 511-tap Kaiser window's transition is 4.0 Hz wide at 360 Hz; measured gain 0.9395).  The list keeps the other
    seven frequencies and takes 54 and 66 Hz -- the mains frequency -+ 6 Hz, as 44 and 56 Hz are at 50 -- 50, 70 and 179 Hz in their place."""
    taps, first = clean.notch_taps(360, 60)
    assert taps.shape == (1, 511) and first.tolist() == [-255]
    assert abs(_ascending_sum(taps[0]) - 1.0) <= 1e-15
    g = _gain(taps[0], 360.0)
    assert g(60) <= 1e-3 and g(59) <= 0.02 and g(61) <= 0.02
    for hz in (1, 5, 15, 40, 44, 50, 54, 66, 70, 100, 150, 179):
        assert abs(g(hz) - 1.0) <= 1e-3, hz
    assert abs(g(56) - 0.9395) < 1e-3                                       # recorded, not a bar: inside the transition
    # a short row and the errors
    t3, f3 = clean.notch_taps(500, 50, taps=3)
    assert t3.shape == (1, 3) and f3.tolist() == [-1] and abs(_ascending_sum(t3[0]) - 1.0) <= 1e-15
    for kw in (dict(taps=512), dict(taps=2), dict(taps=513), dict(taps=5.0), dict(hz=3.0), dict(hz=2.0), dict(hz=178.0), dict(width_hz=0.0),
               dict(beta=float("nan")), dict(rate=0)):
        with pytest.raises(ValueError):
            clean.notch_taps(**{**dict(rate=360, hz=60), **kw})


@pytest.mark.parametrize("hz,bar", [(0.3, 21.0), (0.05, 8.5)])
def test_two_stage_median_removes_a_planted_wander(recs, hz, bar):
    """A = 200, phase 0.7 on every lead, rounded to int16, windows 101 / 301: the cleaned corrupted signal against the cleaned original over
    [300, len - 300).  Measured rms: 12.02 (11315) and 12.01 (40723) at 0.3 Hz, 4.57 and 4.14 at 0.05 Hz; the corruption's own is 141.4."""
    for name, sig, _ in recs:
        bad = corrupt(sig, wander(hz))
        d = mr.baseline_remove(bad, 50, 150).astype(np.float64) - mr.baseline_remove(sig, 50, 150).astype(np.float64)
        rms = float(np.sqrt((d[:, 300:-300] ** 2).mean()))
        print(name, hz, "residual rms", rms)
        assert rms <= bar, (name, rms)


def _peaks(sig):
    row, count, _ = mref.peaks(mref.envelope(sig))
    return row[:count].astype(np.int64), count


def test_detector_finds_the_clean_recordings_peaks_again(cleaned):
    """40723: 16 peaks, 19 on the corrupted signal, 16 again on the cleaned one (measured shift 2 at most); 11315: 19, 19 and 19 (shift 1)."""
    for c, (n_clean, n_bad) in zip(cleaned, ((19, 19), (16, 19))):
        want, count = _peaks(c["sig"])
        assert count == n_clean and _peaks(c["bad"])[1] == n_bad
        got, count = _peaks(c["clean"])
        print("peaks", count, "largest shift", int(np.abs(got - want).max()) if count == n_clean else None)
        assert count == n_clean and int(np.abs(got - want).max()) <= 4


def test_cleaned_lists_pass_the_stores_checks_and_the_recording_plan(cleaned, tmp_path):
    """Cleaning moves no sample in time: the annotated lists go with the cleaned signals through _check_labels and recording_plan as they are."""
    listing = rr.write_tree(tmp_path, [(n, c["clean"], c["lab"]) for n, c in zip(rr.NAMES, cleaned)])
    cfg = rr.make_cfg(listing, data_root=tmp_path / "npy", label_root=tmp_path / "json")
    st = resident.ResidentTianchi(cfg, "train")
    base = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp_path)), "train")
    assert st.signal.dtype == torch.float32 and np.array_equal(st.lengths, base.lengths) and np.array_equal(st.offsets, base.offsets)
    for i, c in enumerate(cleaned):
        lab = [np.asarray(c["lab"][k], dtype=np.int64) for k in rr.KEYS]
        resident.ResidentTianchi._check_labels(rr.NAMES[i], lab, 5000)
        assert all(np.array_equal(st.labels[k][st.label_offsets[k][i]:st.label_offsets[k][i + 1]], lab[k]) for k in range(6))
    a, b = resident.recording_plan(st, [0, 1], [1, 3, 6]), resident.recording_plan(base, [0, 1], [1, 3, 6])
    assert np.array_equal(a.plan.table, b.plan.table) and np.array_equal(a.stitch, b.stitch) and np.array_equal(a.plan.rois, b.plan.rois)


def test_ops_sliding_median_checks_its_arguments_in_front_of_the_library():
    from electrocardio_panorama_amd import ops
    table = torch.tensor([[0, 10, 1]], dtype=torch.int64)
    with pytest.raises(TypeError, match="int16 or float32"):
        ops.sliding_median(torch.zeros(16, dtype=torch.float64), table, torch.zeros(16), 3)
    with pytest.raises(ValueError, match="1-D"):
        ops.sliding_median(torch.zeros((2, 8), dtype=torch.int16), table, torch.zeros(16), 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sliding_median(torch.zeros(16, dtype=torch.int16), table, torch.zeros(16), 3)
    assert ops.MEDIAN_MAX_H == clean.MAX_H == 512 and ops.MEDIAN_TILE == 1024


def test_abi_surface():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    assert "median.hip" in build.SOURCES
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    L, raw = _lib.load(), ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint nef_sliding_median\(const nef_sliding_median_args\* a, nef_stream_t stream\);", hdr)
    assert re.search(r"\bsize_t nef_sliding_median_args_bytes\s*\(\s*void\s*\)", hdr)
    assert "nef_sliding_median" in _lib.SIGNATURES and "nef_sliding_median_args_bytes" in _lib.SIGNATURES and hasattr(raw, "nef_sliding_median")
    assert ctypes.sizeof(_lib.SlidingMedianArgs) == L.nef_sliding_median_args_bytes() == 4 * 8 + 4 * 8 + 6 * 4
    assert L.nef_abi_version() == 22                           # the entry is an addition
    assert int(re.search(r"#define NEF_MEDIAN_MAX_H (\d+)", hdr).group(1)) == clean.MAX_H
    assert int(re.search(r"#define NEF_MEDIAN_TILE (\d+)", hdr).group(1)) == 1024
    # malformed calls are refused in front of any launch (dummy non-null pointers)
    ok = dict(src=16, table=8, dst=4, minuend=None, src_elems=80, dst_elems=80, minuend_elems=0, max_len=10, N=1, max_rows=8, h=50, dtype=0,
              minuend_dtype=1, reserved0=0)
    for bad, code in ((dict(src=None), -2), (dict(table=None), -2), (dict(dst=None), -2), (dict(N=0), -1), (dict(N=65536), -1),
                      (dict(max_rows=0), -1), (dict(max_rows=65536), -1), (dict(max_len=0), -1), (dict(max_len=1 << 31), -1), (dict(h=-1), -1),
                      (dict(h=513), -1), (dict(dtype=2), -1), (dict(minuend_dtype=2), -1), (dict(src_elems=0), -1), (dict(dst_elems=0), -1),
                      (dict(minuend=4, minuend_elems=0), -1), (dict(src=24), -4), (dict(table=4), -4), (dict(dst=2), -4),
                      (dict(minuend=2, minuend_elems=80), -4), (dict(minuend=1, minuend_elems=80, minuend_dtype=0), -4)):
        assert L.nef_sliding_median(ctypes.byref(_lib.SlidingMedianArgs(**{**ok, **bad})), None) == code, bad
