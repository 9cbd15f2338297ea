"""The rational polyphase resampler without a device (DATA.source_rate): resample.design against a brute-force enumeration of
every phase's inputs, the restatement (tests/resample_ref.py) against scipy's upfirdn, its exactness properties, its distance to analytic
sinusoids and over a 500 -> 1000 -> 500 round trip of the bundled recordings, the label rescale against a loop, every ValueError of the new
keys, the argument checks of ops.resample and of the entry, and the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import resample_ref as ref
import resident_ref as rr
from electrocardio_panorama_amd import resample
from electrocardio_panorama_amd.dataset import resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ((1, 2), (2, 1), (25, 18), (18, 25), (500, 257), (125, 32), (1, 1))
EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("up,down", PAIRS)
def test_design_reads_exactly_the_inputs_under_the_prototype_and_sums_to_one(up, down):
    taps, first = resample.design(up, down)
    assert taps.dtype == np.float64 and first.dtype == np.int32 and taps.shape[0] == up and first.shape == (up,)
    zeros = 16
    c = zeros * max(up, down)
    N = 2 * c + 1
    K = taps.shape[1]
    assert K == resample.taps_per_phase(up, down, zeros)
    counts = []
    for p in range(up):
        m = next(q for q in range(up) if (q * down) % up == p)          # an output of phase p (up and down are coprime)
        i0 = (m * down) // up
        hit = [i for i in range(i0 - 2 * c - 2, i0 + 2 * c + 3) if 0 <= m * down - i * up + c < N]
        assert hit == list(range(i0 + int(first[p]), i0 + int(first[p]) + len(hit))) and 1 <= len(hit) <= K
        assert not taps[p, len(hit):].any()                               # the padding is 0.0
        counts.append(len(hit))
        s = 0.0
        for k in range(K):
            s = s + float(taps[p, k])
        assert abs(s - 1.0) <= 4 * EPS
    assert max(counts) == K
    # the literal restatement of the table: the same integers, the same doubles
    rt, rf = ref.design(up, down)
    assert np.array_equal(rf, first) and np.array_equal(rt, taps)
    assert resample.ratio(down * 7, up * 7) == (up, down) == ref.ratio(down * 7, up * 7)


@pytest.mark.parametrize("up,down", ((1, 2), (2, 1), (25, 18), (18, 25), (125, 32)))
def test_restatement_is_upfirdn_in_the_interior(up, down):
    from scipy.signal import upfirdn
    h, c, _ = ref.prototype(up, down)
    raw, first = ref.design(up, down, normalise=False)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(700).astype(np.float32)
    y = ref.resample(x, raw, first, up, down, keep_fp64=True)
    loop = ref.resample_loop(x, raw, first, up, down)
    assert np.array_equal(loop, y.astype(np.float32)) and np.array_equal(loop, ref.resample(x, raw, first, up, down))
    # ^ the two forms of the restatement: the same bits
    # y[m] = conv[m down + c], conv the up-sampled x through h; d leading zeros put that on upfirdn's grid of multiples of `down`
    d = (-c) % down
    full = upfirdn(np.concatenate([np.zeros(d), h]), x.astype(np.float64), up, down)
    shift = (c + d) // down
    K = raw.shape[1]
    edge = (K * up) // down + K + 2                                       # outputs whose window meets a clamped sample
    m = np.arange(edge, y.size - edge)
    bound = 1e-12 * np.abs(h).sum() * np.abs(x).max()
    assert m.size > 100 and np.abs(y[m] - full[m + shift]).max() <= bound


def test_constants_and_pass_through_positions_are_exact():
    t, f = resample.design(25, 18)
    x = np.full(300, -32768, dtype=np.int16)
    assert np.array_equal(ref.resample(x, t, f, 25, 18), np.full(ref.out_len(300, 25, 18), -32768.0, dtype=np.float32))
    t, f = resample.design(18, 25)
    x = np.full(300, np.float32(0.1), dtype=np.float32)
    assert np.array_equal(ref.resample(x, t, f, 18, 25), np.full(ref.out_len(300, 18, 25), np.float32(0.1), dtype=np.float32))
    rng = np.random.default_rng(11)
    for up in (1, 2, 5):
        t, f = resample.design(up, 1)
        for x in (rng.integers(-32768, 32768, 257).astype(np.int16), (rng.standard_normal(257) * 300).astype(np.float32)):
            y = ref.resample(x, t, f, up, 1)
            assert y.shape == (257 * up,) and np.array_equal(y[::up], x.astype(np.float32))


# the worst interior error against the analytic sinusoid of amplitude 1, measured on the restatement (zeros 16, beta 8.6)
SINE_MEASURED = {1000: 1.76e-5, 360: 3.19e-5, 250: 3.15e-5}


@pytest.mark.parametrize("src", sorted(SINE_MEASURED))
def test_sinusoids_come_out_as_sinusoids(src):
    up, down = resample.ratio(src, 500)
    taps, first = resample.design(up, down)
    K = taps.shape[1]
    edge = int(np.ceil(K * max(1.0, up / down))) + 1
    worst = 0.0
    for hz in (1.0, 5.0, 15.0, 40.0, 0.2 * min(src, 500)):
        x = np.sin(2 * np.pi * hz * np.arange(4 * src) / src).astype(np.float32)
        y = ref.resample(x, taps, first, up, down).astype(np.float64)
        truth = np.sin(2 * np.pi * hz * np.arange(y.size) / 500.0)
        worst = max(worst, float(np.abs(y - truth)[edge:-edge].max()))
    print(f"{src} Hz -> 500 Hz: worst interior error {worst:.3e}")
    assert worst <= 2 * SINE_MEASURED[src]                                # measured: 1.752e-5, 3.182e-5, 3.149e-5
    assert worst <= 1e-3                                                  # a wrong phase or centre misses this by orders of magnitude


# 500 -> 1000 -> 500 of the bundled recordings against the original on [K, len - K): measured 0.9784 and 0.2004 (int16 units)
ROUND_TRIP_MEASURED = {"11315.json": 0.9785, "40723.json": 0.2004}


def test_round_trip_of_the_bundled_recordings():
    ut, uf = resample.design(2, 1)
    dt, df = resample.design(1, 2)
    K = max(ut.shape[1], dt.shape[1])
    for name, sig, _ in rr.recordings():
        twice = ref.resample(sig, ut, uf, 2, 1)
        back = ref.resample(twice, dt, df, 1, 2)
        assert twice.shape == (8, 10000) and back.shape == sig.shape
        err = float(np.abs(back.astype(np.float64) - sig)[:, K:-K].max())
        print(f"{name}: round trip error {err:.4f} of a span of {int(sig.max()) - int(sig.min())}")
        assert err <= 2 * ROUND_TRIP_MEASURED[name]
        assert err <= 0.01 * (int(sig.max()) - int(sig.min()))


def test_label_rescale_is_the_literal_loop_and_separates_collisions():
    for _, sig, lab in rr.recordings():
        lists = [lab[k] for k in rr.KEYS]
        for src in (250, 360, 1000):
            up, down = resample.ratio(src, 500)
            got, moved = resample.rescale_marks(lists, up, down)
            want, wmoved = ref.rescale_marks(lists, up, down)
            assert [g.tolist() for g in got] == want and moved == wmoved and all(g.dtype == np.int64 for g in got)
            assert got[0][0] == (2 * lists[0][0] * up + down) // (2 * down)
            resident.ResidentTianchi._check_labels("x", got, ref.out_len(sig.shape[1], up, down))
    # 4 : 1 decimation: marks one and two samples apart collide, and a 'P on' list one longer than the others closes the last beat
    lab = [[10, 50, 90], [11, 60], [12, 61], [13, 62], [14, 70], [40, 80]]
    got, moved = resample.rescale_marks(lab, 1, 4)
    want, wmoved = ref.rescale_marks(lab, 1, 4)
    assert [g.tolist() for g in got] == want == [[3, 13, 23], [4, 15], [5, 16], [6, 17], [7, 18], [10, 20]]
    assert moved == wmoved == 6
    flat = [got[k][j] for j in range(3) for k in range(6) if j < got[k].size]
    assert all(b > a for a, b in zip(flat, flat[1:]))
    # every recording in one pass (what the store runs): the per-recording loop, laid out as the store keeps its lists
    many = [[r[2][k] for k in rr.KEYS] for r in rr.recordings()] + [lab, [[], [], [], [], [], []], [[7], [7], [7], [7], [7], [7]]]
    labels, offsets, total = resample.rescale_all(many, 1, 4)
    each = [ref.rescale_marks(one, 1, 4) for one in many]
    assert total == sum(m for _, m in each) and total >= 6 + 5
    for k in range(6):
        assert offsets[k].tolist() == np.concatenate([[0], np.cumsum([len(one[k]) for one in many])]).tolist()
        assert labels[k].tolist() == [v for w, _ in each for v in w[k]] and labels[k].dtype == np.int64
    # the fix-up is the one labels_from_peaks uses
    from electrocardio_panorama_amd.dataset import marks
    assert marks.increasing is resample.increasing
    fixed, changed = resample.increasing([5, 5, 5, 1, 1, 9], [0, 0, 0, 1, 1, 1])
    assert fixed.tolist() == [5, 6, 7, 1, 2, 9] and changed.tolist() == [False, True, True, False, True, False]


def test_keys_default_off_and_every_error(tmp_path):
    from electrocardio_panorama_amd import train_net
    from electrocardio_panorama_amd.config import get_defaults
    d = get_defaults()
    assert d.DATA.source_rate == 0 and d.DATA.resample_zeros == 16 and d.DATA.resample_beta == 8.6
    cfg = rr.make_cfg(rr.write_listing(tmp_path))
    assert resident.source_plan(cfg) is None
    cfg.DATA.source_rate = 1000
    with pytest.raises(ValueError, match="device_resident"):
        train_net.build_loaders(cfg, batch_size=2)                        # the host loader stays file based
    with pytest.raises(ValueError, match="device_resident"):
        resident.source_plan(cfg)
    cfg.DATA.device_resident = True
    plan = resident.source_plan(cfg)
    assert plan == resident.SourcePlan(1000, 500, 1, 2, 16, 8.6)
    resident.check_cfg(cfg)
    cfg.DATA.source_rate = 500                                            # the model's own rate: off
    assert resident.source_plan(cfg) is None
    for bad in (360.5, -360, True, "360"):
        cfg.DATA.source_rate = bad
        with pytest.raises(ValueError, match="DATA.source_rate"):
            resident.check_cfg(cfg)
    cfg.DATA.source_rate = 360
    cfg.DATA.sample_rate = 499.5
    with pytest.raises(ValueError, match="integer DATA.sample_rate"):
        resident.check_cfg(cfg)
    cfg.DATA.sample_rate = 500.0
    assert resident.source_plan(cfg)[:4] == (360, 500, 25, 18)
    for src, words in ((4001, "down = 4001 is above 8 x up = 500"), (5003, "down = 5003 is above 8 x up = 500")):
        cfg.DATA.source_rate = src
        with pytest.raises(ValueError, match=words) as e:
            resident.check_cfg(cfg)
        assert f"DATA.source_rate {src} Hz" in str(e.value) and "DATA.sample_rate 500 Hz" in str(e.value)
    cfg.DATA.source_rate, cfg.DATA.sample_rate = 500, 1031                # up = 1031
    with pytest.raises(ValueError, match="up = 1031 is above 1024"):
        resident.check_cfg(cfg)
    cfg.DATA.source_rate, cfg.DATA.sample_rate = 1000, 500
    cfg.DATA.resample_zeros = 300                                         # 2 * 300 * 2 + 1 taps a phase
    with pytest.raises(ValueError, match="1201 taps a phase, above 512"):
        resident.check_cfg(cfg)
    cfg.DATA.resample_zeros = 0
    with pytest.raises(ValueError, match="resample_zeros"):
        resident.check_cfg(cfg)
    cfg.DATA.resample_zeros, cfg.DATA.resample_beta = 16, -1.0
    with pytest.raises(ValueError, match="resample_beta"):
        resident.check_cfg(cfg)
    cfg.DATA.resample_beta = 8.6
    # a host store cannot resample: the error says so
    with pytest.raises(RuntimeError, match="HIP device"):
        resident.ResidentTianchi(cfg, "train")
    # off: the store is the one the key's absence gives, field for field
    cfg.DATA.source_rate = 0
    base = resident.ResidentTianchi(cfg, "train")
    cfg.DATA.source_rate = 500
    same = resident.ResidentTianchi(cfg, "train")
    for st in (base, same):
        assert st.source is None and st.source_rate == 0 and st.resample_report is None and st.raw_lengths is st.lengths
        assert st.signal.dtype == torch.int16
    assert torch.equal(base.signal, same.signal) and np.array_equal(base.offsets, same.offsets)
    assert all(np.array_equal(a, b) for a, b in zip(base.labels, same.labels))
    with pytest.raises(ValueError, match="whole number"):
        resample.ratio(360.5, 500)
    with pytest.raises(ValueError, match="positive"):
        resample.ratio(0, 500)
    with pytest.raises(ValueError, match="zeros"):
        resample.design(1, 2, zeros=0)


def test_ops_resample_checks_its_arguments_in_front_of_the_library():
    from electrocardio_panorama_amd import ops
    taps, first = resample.design(1, 2)
    table = torch.tensor([[0, 10, 0, 1]], dtype=torch.int64)
    with pytest.raises(TypeError, match="int16 or float32"):
        ops.resample(torch.zeros(16, dtype=torch.float64), table, torch.zeros(8), taps, first, 1, 2)
    with pytest.raises(ValueError, match="1-D"):
        ops.resample(torch.zeros((2, 8), dtype=torch.int16), table, torch.zeros(8), taps, first, 1, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.resample(torch.zeros(16, dtype=torch.int16), table, torch.zeros(8), taps, first, 1, 2)


def test_abi_surface():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    assert "resample.hip" in build.SOURCES
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    L, raw = _lib.load(), ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint nef_resample\(const nef_resample_args\* a, nef_stream_t stream\);", hdr)
    assert re.search(r"\bsize_t nef_resample_args_bytes\s*\(\s*void\s*\)", hdr)
    assert "nef_resample" in _lib.SIGNATURES and "nef_resample_args_bytes" in _lib.SIGNATURES and hasattr(raw, "nef_resample")
    assert ctypes.sizeof(_lib.ResampleArgs) == L.nef_resample_args_bytes() == 5 * 8 + 3 * 8 + 6 * 4
    assert L.nef_abi_version() == 22                           # the entry is an addition
    for name, macro in (("MAX_UP", "NEF_RESAMPLE_MAX_UP"), ("MAX_K", "NEF_RESAMPLE_MAX_K"), ("MAX_RATIO", "NEF_RESAMPLE_MAX_RATIO")):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == getattr(resample, name)
    # malformed calls are refused in front of any launch (dummy non-null pointers)
    ok = dict(src=16, table=8, dst=4, taps=8, first=4, src_elems=80, dst_elems=40, max_out_len=5, N=1, max_rows=8, up=1, down=2, K=65, dtype=0)
    for bad, code in ((dict(src=None), -2), (dict(first=None), -2), (dict(N=0), -1), (dict(N=65536), -1), (dict(max_rows=0), -1),
                      (dict(max_rows=65536), -1), (dict(max_out_len=0), -1), (dict(max_out_len=1 << 31), -1), (dict(up=0), -1),
                      (dict(up=1025), -1), (dict(K=0), -1), (dict(K=513), -1), (dict(down=0), -1), (dict(down=9), -1), (dict(dtype=2), -1),
                      (dict(src_elems=0), -1), (dict(dst_elems=0), -1), (dict(src=24), -4), (dict(table=4), -4), (dict(taps=4), -4),
                      (dict(dst=2), -4), (dict(first=2), -4)):
        assert L.nef_resample(ctypes.byref(_lib.ResampleArgs(**{**ok, **bad})), None) == code, bad
