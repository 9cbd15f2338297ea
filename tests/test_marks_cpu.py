"""Marks for unannotated recordings, without a device: the literal-loop restatement of the two kernels (tests/marks_ref.py) on the bundled
recordings -- the peak counts, one peak per annotated QRS, the timing table's distance to the annotator -- and dataset/marks.py's host half
(labels_from_peaks against the loop form, fit_table, the table file, the errors), the new config keys and the C ABI surface."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import marks_ref as mref
import resident_ref as rr
from electrocardio_panorama_amd.dataset import marks, resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLED_BAR, CROSS_BAR = 12, 16       # samples: the measured worst pooled plus one, and the cross-fitted worst -- the first within aug_roi_jitter's range


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    """The annotated host store of the two bundled recordings and the restatement's peaks of each."""
    store = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp_path_factory.mktemp("real"))), "train")
    rows = [mref.peaks(mref.envelope(sig)) for _, sig, _ in rr.recordings()]
    found = marks.Peaks(np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.int32), np.array([r[2] for r in rows]))
    return store, found


def _one(store, found, i):
    """Recording i alone: a one-recording view of the store and its peaks."""
    st = copy.copy(store)
    st.names, st.lengths = [store.names[i]], store.lengths[i:i + 1]
    st.labels = [store.labels[k][store.label_offsets[k][i]:store.label_offsets[k][i + 1]] for k in range(6)]
    st.label_offsets = [np.array([0, v.size], dtype=np.int64) for v in st.labels]
    return st, marks.Peaks(found.peaks[i:i + 1], found.count[i:i + 1], found.level[i:i + 1])


def test_restatement_finds_every_annotated_qrs_of_the_bundled_recordings_once(real):
    store, found = real
    assert found.count.tolist() == [19, 16]
    assert (found.peaks[0, 0], found.peaks[0, 18], found.peaks[1, 0], found.peaks[1, 15]) == (20, 4902, 113, 4735)
    assert (found.peaks[0, 19:] == -1).all() and (found.peaks[1, 16:] == -1).all()
    for i, (_, sig, lab) in enumerate(rr.recordings()):
        p = found.peaks[i, :found.count[i]]
        inside = [int(((p >= a) & (p <= b)).sum()) for a, b in zip(lab["R on"], lab["R off"])]
        assert len(inside) == (17, 15)[i] and inside == [1] * len(inside)           # no beat is left out of this check
        ratio = mref.envelope(sig)[p] / found.level[i]
        print("recording", i, "peak / level", ratio.min(), ratio.max())
        assert 0.84 <= ratio.min() and ratio.max() <= 1.05


def test_ratio_table_stays_within_the_bars_pooled_and_cross_fitted(real):
    store, found = real
    fit = marks.fit_table(store, found, "ratio")
    assert (fit.matched, fit.left_out) == (32, 0) and not fit.table[:, 0].any()
    auto = marks.labels_from_peaks(found.peaks, found.count, store.lengths, fit.table)
    rows = marks.compare(store, auto)
    worst = [rows[k]["max"] for k in marks.LABEL_KEYS]
    print("pooled, largest differences", worst)
    assert rows["share"] == 1.0 and rows["matched"] == 32
    assert max(worst) <= POOLED_BAR
    assert all(rows[k]["mean"] <= rows[k]["max"] and rows[k]["median"] <= rows[k]["max"] for k in marks.LABEL_KEYS)
    cross = []
    for a, b in ((0, 1), (1, 0)):
        sa, fa = _one(store, found, a)
        sb, fb = _one(store, found, b)
        got = marks.compare(sb, marks.labels_from_peaks(fb.peaks, fb.count, sb.lengths, marks.fit_table(sa, fa).table))
        assert got["share"] == 1.0
        cross.append([got[k]["max"] for k in marks.LABEL_KEYS])
    print("cross-fitted, largest differences", cross)
    assert max(max(c) for c in cross) <= CROSS_BAR
    # 'affine' fits both coefficients and is no worse on its own data
    aff = marks.fit_table(store, found, "affine")
    rows2 = marks.compare(store, marks.labels_from_peaks(found.peaks, found.count, store.lengths, aff.table))
    assert aff.table[:, 0].any() and max(rows2[k]["max"] for k in marks.LABEL_KEYS) <= POOLED_BAR


def test_auto_lists_pass_the_stores_checks_and_plan_whole_recordings(real):
    store, found = real
    auto = marks.labels_from_peaks(found.peaks, found.count, store.lengths, marks.fit_table(store, found).table)
    st = copy.copy(store)
    st.labels, st.label_offsets, st.n_p_on = auto.labels, auto.label_offsets, np.diff(auto.label_offsets[0])
    assert st.n_p_on.tolist() == [17, 16] and auto.dropped.tolist() == [2, 0] and auto.adjusted.tolist() == [0, 0]
    for i, name in enumerate(st.names):
        lab = [st.labels[k][st.label_offsets[k][i]:st.label_offsets[k][i + 1]] for k in range(6)]
        resident.ResidentTianchi._check_labels(name, lab, 5000)
        flat = np.stack(lab, axis=1).reshape(-1)
        assert (np.diff(flat) >= 1).all() and flat[0] >= 0 and flat[-1] <= 4999
    rp = resident.recording_plan(st, [0, 1], [1, 3, 6])
    assert rp.rec.size == 16 + 15 and (rp.plan.rois[:, :6, 1] >= rp.plan.rois[:, :6, 0]).all()
    assert (rp.stitch[:, 2] >= 1).all() and (rp.stitch[:, 2] <= 512).all()


def _same_lists(got, want):
    for k in range(6):
        for i, lst in enumerate(want[0][k]):
            if got.labels[k][got.label_offsets[k][i]:got.label_offsets[k][i + 1]].tolist() != lst:
                return False
    return got.dropped.tolist() == want[1] and got.adjusted.tolist() == want[2]


def test_labels_from_peaks_is_the_literal_loop_on_hand_made_peaks():
    table = np.array([[0, -0.34], [0, -0.15], [0, -0.085], [0, 0.087], [0, 0.22], [0, 0.5]])
    rows = [
        [20, 289, 558, 828, 1100],          # 'P on' of the first beat is negative: dropped
        [300, 600, 900, 1200, 1490],        # len 1300: 'T off' of the last two beats lies behind the end
        [500, 520, 1000, 1500],             # RR of 20 next to one of 480: overlapping marks, the fix-up moves some
        [],                                 # P = 0
        [700],                              # P = 1
        [400, 800],                         # P = 2
        [100, 200, 300],                    # count -1
        [100, 400, 700, 1000, 1300],        # count above max_peaks
        [60, 90, 4000, 4030, 4990],         # negative 'P on' in front, a second one behind a good beat: all up to it go
        [1000, 1001, 1002, 1003, 1004, 1500, 2000],     # RR of 1: every mark of five beats collides
    ]
    max_peaks = 8
    peaks = np.full((len(rows), max_peaks), -1, dtype=np.int32)
    for i, r in enumerate(rows):
        peaks[i, :len(r)] = r
    count = np.array([5, 5, 4, 0, 1, 2, -1, 9, 5, 7], dtype=np.int32)
    lengths = np.array([5000, 1300, 5000, 5000, 5000, 1100, 5000, 5000, 5000, 2600], dtype=np.int64)
    got = marks.labels_from_peaks(peaks, count, lengths, table)
    want = mref.labels_from_peaks(peaks, count, lengths, table)
    assert _same_lists(got, want)
    n = np.diff(got.label_offsets[0]).tolist()
    assert n[0] == 4 and n[1] == 3 and n[3] == n[4] == n[6] == n[7] == 0 and n[5] == 2 and got.adjusted[2] > 0 and got.adjusted[9] > 0
    assert got.dropped.tolist()[3:8] == [0, 1, 0, 0, 9]
    assert all(np.array_equal(got.label_offsets[0], o) for o in got.label_offsets)
    # an affine table with offsets, and one that pushes the end out so that trailing beats leave behind the fix-up
    for tab in (table + np.array([[-6.0, 0]] * 2 + [[3.0, 0]] * 4), table * np.array([[1.0, 1.0]] * 5 + [[1.0, 1.9]])):
        assert _same_lists(marks.labels_from_peaks(peaks, count, lengths, tab), mref.labels_from_peaks(peaks, count, lengths, tab))
    rng = np.random.default_rng(3)
    for _ in range(20):                      # random rhythms, short recordings: every rule fires somewhere
        P = rng.integers(0, 9, size=6)
        pk = np.full((6, 8), -1, dtype=np.int32)
        for i in range(6):
            pk[i, :P[i]] = np.sort(rng.choice(np.arange(0, 1200), size=P[i], replace=False))
        ln = rng.integers(900, 1400, size=6)
        assert _same_lists(marks.labels_from_peaks(pk, P.astype(np.int32), ln, table), mref.labels_from_peaks(pk, P, ln, table))


def test_errors_params_and_the_table_file(real, tmp_path):
    store, found = real
    assert marks.MarkParams.from_rate(500.0) == marks.MarkParams() == marks.MarkParams(2, 20, 100, 1000, 0.125, 255, 256)
    assert marks.MarkParams.from_rate(250)[:4] == (1, 10, 50, 500) and marks.MarkParams.from_rate(1000, max_peaks=64)[:4] == (4, 40, 200, 2000)
    with pytest.raises(ValueError, match="sample_rate"):
        marks.MarkParams.from_rate(0)
    with pytest.raises(ValueError, match="form"):
        marks.fit_table(store, found, "cubic")
    same = marks.Peaks(np.array([[100, 400, 700, 1000] + [-1] * 4], dtype=np.int32), np.array([4], dtype=np.int32), np.array([1.0]))
    st = copy.copy(store)
    st.names, st.lengths = ["x"], np.array([1500])
    st.labels = [np.array([100 + d, 400 + d, 700 + d]) for d in (-90, -40, -20, 20, 60, 150)]
    st.label_offsets = [np.array([0, 3])] * 6
    with pytest.raises(ValueError, match="all equal"):
        marks.fit_table(st, same, "affine")
    flat = marks.fit_table(st, same, "ratio")
    assert np.allclose(flat.table[:, 1], np.array([-90, -40, -20, 20, 60, 150]) / 300.0, rtol=1e-15) and flat.matched == 3
    none = marks.Peaks(same.peaks, np.array([-1], dtype=np.int32), np.array([np.nan]))
    with pytest.raises(ValueError, match="nothing to fit"):
        marks.fit_table(st, none)
    with pytest.raises(ValueError, match="six finite"):
        marks.labels_from_peaks(same.peaks, same.count, st.lengths, np.zeros((5, 2)))
    with pytest.raises(ValueError, match="max_peaks"):
        marks.labels_from_peaks(same.peaks, same.count, np.array([1500, 1500]), flat.table)
    with pytest.raises(RuntimeError, match="HIP device"):
        marks.detect(store)                                   # a host store: no CPU path
    with pytest.raises(TypeError, match="MarkParams"):
        marks.detect(store, params=(2, 20))
    # the file round trip
    fit = marks.fit_table(store, found, "affine")
    path = tmp_path / "table.json"
    params = marks.MarkParams.from_rate(500, max_peaks=64)
    marks.save_table(path, fit.table, "affine", params)
    table, form, back = marks.load_table(path)
    assert np.array_equal(table, fit.table) and form == "affine" and back == params and isinstance(back, marks.MarkParams)
    (tmp_path / "bad.json").write_text('{"table": [[0, 1]]}')
    with pytest.raises(ValueError):
        marks.load_table(tmp_path / "bad.json")
    assert marks._chunks([5, 5, 5, 20, 5], 10) == [(0, 2), (2, 3), (3, 4), (4, 5)] and marks._chunks([5, 5], 100) == [(0, 2)]


def test_keys_default_off_and_are_rejected_off_the_resident_path(tmp_path):
    from electrocardio_panorama_amd import train_net
    from electrocardio_panorama_amd.config import get_defaults
    d = get_defaults()
    assert d.DATA.auto_marks is False and d.DATA.mark_table == "" and d.DATA.auto_marks_skip is False
    cfg = rr.make_cfg(rr.write_listing(tmp_path))
    assert marks.check_cfg(cfg) is False
    cfg.DATA.auto_marks = True
    with pytest.raises(ValueError, match="device_resident"):
        train_net.build_loaders(cfg, batch_size=2)             # the host DataLoader path stays label-file based
    cfg.DATA.device_resident = True
    with pytest.raises(ValueError, match="mark_table"):
        resident.check_cfg(cfg)
    cfg.DATA.mark_table = str(tmp_path / "t.json")
    resident.check_cfg(cfg)
    cfg.DATA.weighted_sample = True
    with pytest.raises(ValueError, match="weighted_sample"):
        resident.check_cfg(cfg)


def test_load_signal_opens_no_label_file(tmp_path):
    from electrocardio_panorama_amd.dataset.tianchi import EcgTianChiInterval
    os.makedirs(tmp_path / "npy")
    recs = rr.recordings()
    np.save(tmp_path / "npy" / "11315.npy", recs[0][1])
    np.savez(tmp_path / "npy" / "40723.npz", signal=recs[1][1])
    (tmp_path / "list.txt").write_text("11315.json\n40723.json\n")
    cfg = rr.make_cfg(tmp_path / "list.txt", data_root=tmp_path / "npy", label_root=tmp_path / "none")
    ds = EcgTianChiInterval(cfg, "train")
    for name, (_, sig, _) in zip(ds.dataset, recs):
        got = ds._load_signal(name)
        assert got.dtype == np.float64 and np.array_equal(got, sig)
    with pytest.raises(FileNotFoundError):
        ds._load("11315.json")
    # on the host (no device) the signal-only store cannot mark: the error says so, and still no label file was asked for
    with pytest.raises(RuntimeError, match="HIP device"):
        resident.ResidentTianchi(cfg, "train", marks=np.zeros((6, 2)))


def test_abi_surface():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    assert "marks.hip" in build.SOURCES
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    L, raw = _lib.load(), ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nef_mark_envelope", "nef_mark_peaks"):
        assert re.search(r"\bint %s\(const %s_args\* a, nef_stream_t stream\);" % (name, name), hdr)
        assert re.search(r"\bsize_t %s_args_bytes\s*\(\s*void\s*\)" % name, hdr)
        assert name in _lib.SIGNATURES and name + "_args_bytes" in _lib.SIGNATURES and hasattr(raw, name)
    assert ctypes.sizeof(_lib.MarkEnvelopeArgs) == L.nef_mark_envelope_args_bytes() == 3 * 8 + 3 * 8 + 6 * 4
    assert ctypes.sizeof(_lib.MarkPeaksArgs) == L.nef_mark_peaks_args_bytes() == 5 * 8 + 3 * 8 + 4 * 4
    assert L.nef_abi_version() == 22                           # the entries are additions
    # malformed calls are refused in front of any launch (dummy non-null pointers)
    ok = dict(signal=16, table=8, env=8, signal_elems=80, env_elems=10, max_len=10, N=1, D=2, H=20, lead_bits=255, dtype=0, reserved0=0)
    for bad, code in ((dict(signal=None), -2), (dict(N=0), -1), (dict(N=65536), -1), (dict(H=257), -1), (dict(D=-1), -1), (dict(lead_bits=0), -1),
                      (dict(lead_bits=256), -1), (dict(dtype=2), -1), (dict(max_len=0), -1), (dict(signal=24), -4), (dict(env=4), -4)):
        assert L.nef_mark_envelope(ctypes.byref(_lib.MarkEnvelopeArgs(**{**ok, **bad})), None) == code, bad
    ok = dict(env=8, table=8, peaks=4, count=4, level=8, env_elems=10, max_len=10, frac=0.125, N=1, seg=1000, r=100, max_peaks=8)
    for bad, code in ((dict(level=None), -2), (dict(N=0), -1), (dict(seg=0), -1), (dict(max_len=4097 * 1000), -1), (dict(r=513), -1),
                      (dict(max_peaks=0), -1), (dict(frac=-1.0), -1), (dict(frac=float("nan")), -1), (dict(frac=float("inf")), -1),
                      (dict(peaks=2), -4), (dict(level=4), -4)):
        assert L.nef_mark_peaks(ctypes.byref(_lib.MarkPeaksArgs(**{**ok, **bad})), None) == code, bad
