"""DATA.device_noise without a GPU: the restatement the GPU tests compare against (tests/noise_row_ref.py) against numpy.std and a literal
loop, the statistical condition of the GPU test evaluated on the restatement for the seeds it uses, the key and its one rejection, the
three DATA.noise rejections that stay, the seed words, and the argument checks of ops.noise_row and of the entry nef_noise_row, which
need no device."""
import ctypes

import numpy as np
import pytest
import torch

import noise_row_ref as ref


def _cfg(solver=None, **data):
    from electrocardio_panorama_amd.config.default import get_defaults
    cfg = get_defaults()
    cfg.MODEL.model = "model_nefnet"
    cfg.DATA.lead_num = 3
    for k, v in data.items():
        cfg.DATA[k] = v
    for k, v in (solver or {}).items():
        cfg.SOLVER[k] = v
    return cfg


# ------------------------------------------------------------------------------------------------ the restatement
def _roi(s, e, end):
    r = np.zeros((7, 2), np.int64)
    r[5], r[6, 0] = (s, e), end
    return r


def test_sigma_is_numpy_std_of_the_slice():
    rng = np.random.default_rng(3)
    row = rng.random(64, dtype=np.float32)
    for s, e, end in ((0, 64, 64), (10, 30, 64), (11, 30, 64), (40, 60, 55), (60, 64, 64), (-20, 40, 64)):
        q0 = max((s + e) // 2, 0)
        q1 = min(e, end)
        want = np.std(row[q0:q1].astype(np.float64))
        got = ref.sigma(row, _roi(s, e, end))
        assert want > 0 and abs(got - want) <= 1e-15, (s, e, end, got, want)
    assert ref.sigma(np.full(64, 0.3, np.float32), _roi(0, 64, 64)) == 0.0          # two passes: a constant segment is exactly 0
    assert ref.sigma(row, _roi(63, 64, 64)) == 0.0                                  # one element
    assert ref.sigma(row, _roi(70, 70, 64)) == 0.0 and ref.sigma(row, _roi(20, 10, 64)) == 0.0      # empty: 0 where numpy.std warns
    bad = row.copy()
    bad[40] = np.nan
    assert np.isnan(ref.sigma(bad, _roi(20, 60, 64))) and not np.isnan(ref.sigma(bad, _roi(50, 60, 64)))


def test_clamping_against_a_literal_loop():
    """(end, q0, q1, m) for marks around and far outside a row of 16: the members of the quiet segment are found by walking the integers."""
    L = 16
    vals = [-(1 << 63), -1000, -33, -17, -16, -9, -2, -1, 0, 1, 2, 7, 8, 15, 16, 17, 31, 40, (1 << 63) - 1]
    for end_raw in [-(1 << 63), -3, 0, 1, 7, 15, 16, 21, (1 << 63) - 1]:
        for s in vals:
            for e in vals:
                end, q0, q1, m = ref.segment(_roi(0, 0, 0).tolist()[:5] + [[s, e], [end_raw, 0]], L)
                want_end = 0 if end_raw < 0 else (L if end_raw > L else end_raw)
                total = s + e
                half = total // 2 if total >= 0 else -((-total + 1) // 2)                 # the floor, spelled out for a negative sum
                members = [t for t in range(want_end) if half <= t < e]
                assert end == want_end and m == len(members), (s, e, end_raw)
                if members:
                    assert (q0, q1) == (members[0], members[-1] + 1)
                assert 0 <= q0 <= end and 0 <= q1 <= end


def test_rows_are_zero_behind_the_end_and_scale_with_sigma():
    Rw, L, names, target, rois, seed = [c for c in ref.launches(1) if c[:2] == (4, 1028)][0]
    noise, sig, r, end = ref.noise_rows(target, rois, seed)
    n, _ = __import__("augment_ref").normals(seed, Rw * L)
    for i in range(Rw):
        assert not noise[i, end[i]:].any()
        if sig[i] > 0:
            assert np.array_equal(noise[i, :end[i]], float(np.float32(sig[i])) * n.reshape(Rw, L)[i, :end[i]])
            assert np.all(np.abs(noise[i]) <= float(np.float32(sig[i])) * r[i] + 1e-15)
        else:
            assert not noise[i].any()
    assert (sig > 0).any()


def test_the_cases_cover_what_they_name():
    for Rw, L in ref.SHAPES:
        seg = {name: ref.segment(_roi(s, e, end), L) for name, (s, e), end in ref.case_rows(L)}
        assert seg["seg_0"][3] == 0 and seg["seg_1"][3] == 1 and seg["seg_2"][3] == 2
        assert seg["from_0"][1:] == (0, L, L) and seg["negative_start"][1:] == (0, 2, 2)
        assert seg["cross_end"][0] % 2 == 1 and seg["cross_end"][2] == seg["cross_end"][0] < L and seg["cross_end"][3] >= 1
        for name in ("behind_end", "non_monotonic", "negative_both", "int64_top", "int64_bottom", "end_0", "end_negative", "end_int64_bottom"):
            assert seg[name][3] == 0, name
        assert seg["int64_span"][1:] == (0, L, L)
        assert seg["end_0"][0] == 0 and seg["end_1"][0] == 1 and seg["end_odd"][0] == L - 1 and seg["end_above_L"][0] == L
        assert seg["end_int64_top"][0] == L and seg["end_negative"][0] == 0
    assert len(ref.launches(1)) == sum(-(-len(ref.case_rows(L)) // Rw) for Rw, L in ref.SHAPES)


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_the_screened_seeds_pass_on_the_restatement(seed):
    """The statistical condition of tests/test_device_noise_gpu.py, on the restatement: z = noise / sigma pooled over all rows with
    sigma > 0 of the seed's launches has mean within 4 / sqrt(N) of 0 and variance within 4 sqrt(2 / N) of 1."""
    res = [ref.noise_rows(t, r, s) for _, _, _, t, r, s in ref.launches(seed)]
    z = ref.pooled_z([x[0] for x in res], [x[1] for x in res], [x[3] for x in res])
    mean, mean_bar, var, var_bar, N = ref.stat_bars(z)
    print(f"seed {seed}: N = {N}, |mean| = {mean:.3e} (bar {mean_bar:.3e}), |var - 1| = {var:.3e} (bar {var_bar:.3e})")
    assert N > 300000 and mean <= mean_bar and var <= var_bar


# ------------------------------------------------------------------------------------------------ the key
def test_the_key_defaults_to_off_and_is_rejected_with_data_noise():
    from electrocardio_panorama_amd import device_noise
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.network import build_model
    cfg = _cfg()
    assert cfg.DATA.device_noise is False and device_noise.on(cfg) is False
    m = build_model(cfg)
    st = GraphedTrainStep(m, cfg)
    assert st.device_noise is False and st.use_noise is False and st.noise is None
    cfg = _cfg(device_noise=True)
    assert device_noise.on(cfg) is True
    st = GraphedTrainStep(m, cfg)
    assert st.device_noise and st.use_noise
    assert GraphedTrainStep(m, _cfg(noise=True)).use_noise and not GraphedTrainStep(m, _cfg(noise=True)).device_noise
    both = _cfg(device_noise=True, noise=True)
    with pytest.raises(ValueError, match="DATA.device_noise with DATA.noise"):
        device_noise.on(both)
    with pytest.raises(ValueError, match="DATA.device_noise with DATA.noise"):
        GraphedTrainStep(m, both)
    with pytest.raises(ValueError, match="DATA.device_noise"):
        device_noise.on(_cfg(device_noise=1))


def test_the_solver_rejects_both_keys(monkeypatch):
    from electrocardio_panorama_amd.solver import Solver
    monkeypatch.setattr(Solver, "_init_model_device", lambda self: None)
    with pytest.raises(ValueError, match="DATA.device_noise with DATA.noise"):
        Solver(_cfg(device_noise=True, noise=True), use_tensorboardx=False)
    sol = Solver(_cfg(device_noise=True), use_tensorboardx=False)
    assert sol.device_noise is True
    assert Solver(_cfg(), use_tensorboardx=False).device_noise is False


def test_the_three_data_noise_rejections_keep_their_words():
    from electrocardio_panorama_amd import views, warp
    from electrocardio_panorama_amd.dataset import resident
    with pytest.raises(ValueError, match="the noise row needs the quiet segment's sigma and a host draw"):
        resident.check_cfg(_cfg(noise=True, device_resident=True, dataset="tianchi"))
    with pytest.raises(ValueError, match="the noise row is padded to the unwarped beat"):
        warp.from_cfg(_cfg(noise=True, aug_roi_jitter=2))
    with pytest.raises(ValueError, match="the batch carries noise for the target lead only"):
        views.train_views(_cfg(solver=dict(train_views=2), noise=True))
    # ... and none of them looks at the new key
    resident.check_cfg(_cfg(device_noise=True, device_resident=True, dataset="tianchi"))
    assert warp.from_cfg(_cfg(device_noise=True, aug_roi_jitter=2)).jitter == 2
    assert views.train_views(_cfg(solver=dict(train_views=2), device_noise=True)) == 2


def test_seed_words():
    """The eager word is the step's seed plus the site word (what a replayed launch adds up from its host word and seed_dev); the site is
    no dropout site, not nef_augment's and not nef_warp's."""
    from electrocardio_panorama_amd import augment, device_noise, engine, warp
    n = len(engine.DROPOUT_SITES)
    assert device_noise.site_word() == (n + 4) * 0x85EBCA6B + 1
    for step in (0, 1, 0x7FFFFFFFFFFF):
        assert device_noise.train_seed(step) == step + device_noise.site_word()
    taken = {k * 0x85EBCA6B + 1 for k in range(n)} | {augment.site_word(), augment.site_word(read_out=True), warp._site_word(),
                                                      warp._site_word(read_out=True)}
    assert device_noise.site_word() not in taken and len(taken) == n + 4


# ------------------------------------------------------------------------------------------------ argument checks
def test_ops_noise_row_checks_its_arguments_before_the_library(monkeypatch):
    from electrocardio_panorama_amd import _lib, ops

    def touched():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)
    x = torch.zeros(2, 1, 8)
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    with pytest.raises(TypeError, match="float32"):
        ops.noise_row(x.double(), rois, 1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.noise_row(torch.zeros(8, 2).t(), rois, 1)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.noise_row(torch.zeros(2, 1, 6), rois, 1)
    with pytest.raises(TypeError, match="int64"):
        ops.noise_row(x, rois.to(torch.int32), 1)
    with pytest.raises(TypeError, match="int64"):
        ops.noise_row(x, None, 1)
    with pytest.raises(ValueError, match="rois"):
        ops.noise_row(x, rois[:1], 1)
    with pytest.raises(ValueError, match="rois"):
        ops.noise_row(torch.zeros(3, 2, 1, 8), rois, 1)            # a multi-view target takes Q * B rois
    with pytest.raises(ValueError, match="out"):
        ops.noise_row(x, rois, 1, out=torch.zeros(2, 1, 4))
    with pytest.raises(ValueError, match="out of place"):
        ops.noise_row(x, rois, 1, out=x)
    with pytest.raises(ValueError, match="sigma_out"):
        ops.noise_row(x, rois, 1, sigma_out=torch.zeros(2))
    with pytest.raises(ValueError, match="sigma_out"):
        ops.noise_row(x, rois, 1, sigma_out=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="seed_dev"):
        ops.noise_row(x, rois, 1, seed_dev=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.noise_row(x, rois, 1)                                  # a CPU tensor, everything else right: still in front of the library


def test_the_entry_rejects_bad_calls_without_touching_the_gpu():
    """nef_noise_row with dummy pointers: every refusal sits in front of the launch."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    assert L.nef_noise_row_args_bytes() == ctypes.sizeof(_lib.NoiseRowArgs) == 56

    def call(**kw):
        a = dict(target=1 << 20, rois=1 << 12, out=1 << 21, sigma=None, seed_dev=None, seed=1, Rw=2, L=8)
        a.update(kw)
        return L.nef_noise_row(ctypes.byref(_lib.NoiseRowArgs(**a)), None)
    assert L.nef_noise_row(None, None) == -2                       # NEF_E_NULL
    assert call(target=None) == -2 and call(rois=None) == -2 and call(out=None) == -2
    assert call(L=6) == -1 and call(L=0) == -1 and call(L=-4) == -1 and call(Rw=0) == -1 and call(Rw=-1) == -1      # NEF_E_SHAPE
    assert call(target=(1 << 20) + 4) == -4 and call(out=(1 << 21) + 8) == -4          # NEF_E_UNSUPPORTED: misaligned bases
    assert call(rois=(1 << 12) + 4) == -4 and call(sigma=(1 << 13) + 4) == -4 and call(seed_dev=(1 << 14) + 2) == -4
    assert call(out=1 << 20) == -4 and call(out=(1 << 20) + 48) == -4 and call(out=(1 << 20) - 48) == -4            # overlapping
