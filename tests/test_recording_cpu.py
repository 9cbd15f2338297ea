"""The whole-recording path without a device: the plan of all beats and its tables (dataset/resident.py recording_plan) against the literal
loops of tests/recording_ref.py and against resident_ref.beat_item, the argument errors, and the round trip on the restatement alone --
normalise the bundled recordings beat by beat, stitch them back, and land within two fp32 roundings of the stored signal."""
import random

import numpy as np
import pytest
import torch

import recording_ref as ref
import resident_ref as rr
from electrocardio_panorama_amd import recording
from electrocardio_panorama_amd.dataset import resident
from test_resident_gpu import _synthetic


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    return resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp_path_factory.mktemp("real"))), "train")


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    return _synthetic(tmp_path_factory.mktemp("syn16"), 0)


def check_plan(store, indices, leads, A):
    before = (random.getstate(), np.random.get_state()[1].copy())
    rp = resident.recording_plan(store, indices, leads, angles=A)
    assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
    want = ref.plan_tables(store, indices, leads, A)
    for got, key in ((rp.plan.table, "table"), (rp.plan.rois, "rois"), (rp.rec, "rec"), (rp.plan.beats, "beats"), (rp.stitch, "stitch"),
                     (rp.recordings, "recordings"), (rp.out_offsets, "out_offsets")):
        assert got.dtype == np.int64 and got.shape == want[key].shape and np.array_equal(got, want[key]), key
    assert rp.plan.id == want["ids"] and rp.plan.V == len(leads) and rp.plan.R == 0 and rp.A == A
    assert rp.plan.rest_theta.shape == (rp.rec.size, 0, 2) and rp.plan.unsupervision_lead_name == [[]] * rp.rec.size
    # every row's item fields are those of the per-beat dataset for that beat
    items = rr.plan_items(store, rp.plan)
    assert np.array_equal(items["rois"], rp.plan.rois) and items["rois"].dtype == rp.plan.rois.dtype
    assert np.array_equal(items["input_theta"], rp.plan.input_theta) and rp.plan.input_theta.dtype == np.float32
    assert np.array_equal(items["target_theta"], rp.plan.target_theta) and rp.plan.target_theta.dtype == np.float32
    assert np.array_equal(rp.plan.input_theta[0], rr.lead_theta()[list(leads)].astype(np.float32))      # no jitter
    for j in range(rp.rec.size):
        s8, lab = ref.store_recording(store, indices[rp.rec[j]])
        it = rr.beat_item(s8, lab, int(rp.plan.beats[j]), list(leads), leads[0], [])
        assert np.array_equal(it["rois"], rp.plan.rois[j]) and it["data"].shape == (len(leads), 512)
    return rp


def test_plan_of_the_bundled_recordings(real):
    rp = check_plan(real, [0, 1], [1, 3, 6], 12)
    assert rp.recordings[:, 1].tolist() == [16, 14] and rp.out_offsets.tolist() == [0, 60000, 120000]
    assert rp.stitch[15].tolist()[3] == 0 and rp.stitch[14].tolist()[3] == 1 and rp.stitch[-1, 3] == 0
    rp = check_plan(real, [1, 0, 1], [7], 5)                 # any order, a recording twice, one lead, five angles
    assert rp.recordings[:, 1].tolist() == [14, 16, 14] and rp.rec.tolist() == [0] * 14 + [1] * 16 + [2] * 14


def test_plan_of_the_synthetic_tree(synthetic):
    rp = check_plan(synthetic, [0, 1, 2, 3, 4], list(range(12)), 13)
    assert rp.stitch[:, 2].tolist() == [1, 2, 511, 183, 512, 513, 1300, 2677, 5000] + [9] * 9 + [290, 290]
    assert rp.out_offsets.tolist() == np.concatenate([[0], np.cumsum(13 * np.array([700, 5003, 5000, 1000, 600]))]).tolist()
    check_plan(synthetic, [3, 1], [0, 8], 1)


def test_recording_plan_rejects_bad_arguments(real):
    for leads in ([], list(range(12)) + [0], [1, 1], [12], [-1], [1.0], [True]):
        with pytest.raises(ValueError, match="input_leads"):
            resident.recording_plan(real, [0], leads)
    for idx in ([2], [-1], []):
        with pytest.raises(ValueError, match="indices"):
            resident.recording_plan(real, idx, [1])
    with pytest.raises(ValueError, match="angles"):
        resident.recording_plan(real, [0], [1], angles=0)


def test_synthesize_rejects_bad_arguments(real):
    with pytest.raises(ValueError, match="fill"):
        recording.synthesize(None, real, [0], [1, 3, 6], fill="zero")
    with pytest.raises(ValueError, match="score_leads"):
        recording.synthesize(None, real, [0], [1, 3, 6], score_leads=[0] * 11)
    with pytest.raises(ValueError, match="score_leads"):
        recording.synthesize(None, real, [0], [1, 3, 6], score_leads=[12] + [0] * 11)
    with pytest.raises(ValueError, match="score_leads"):
        recording.synthesize(None, real, [0], [1, 3, 6], score_leads=[-2] + [0] * 11)
    with pytest.raises(ValueError, match="input_leads"):
        recording.synthesize(None, real, [0], [1, 1, 6])
    with pytest.raises(ValueError, match="beats_per_pass"):
        recording.synthesize(None, real, [0], [1, 3, 6], beats_per_pass=0)
    with pytest.raises(ValueError, match="query_thetas"):
        recording.synthesize(None, real, [0], [1, 3, 6], query_thetas=np.zeros((3, 3)))
    assert real.signal.device.type == "cpu"
    with pytest.raises(ValueError, match="store is on the CPU"):
        recording.synthesize(None, real, [0], [1, 3, 6])


def test_chunks_are_whole_recordings(real, synthetic):
    rp = resident.recording_plan(real, [0, 1, 0], [1])
    assert recording.chunks(rp, 256) == [(0, 46)] and recording.chunks(rp, 30) == [(0, 30), (30, 46)]
    assert recording.chunks(rp, 16) == [(0, 16), (16, 30), (30, 46)] and recording.chunks(rp, 1) == [(0, 16), (16, 30), (30, 46)]
    rp = resident.recording_plan(synthetic, [0, 1, 2, 3, 4], [1])          # 4, 4, 1, 9 and 2 beats
    assert recording.chunks(rp, 7) == [(0, 4), (4, 9), (9, 18), (18, 20)]     # the nine-beat recording is a chunk alone


def test_round_trip_on_the_restatement(real):
    """Stitch the restatement's own normalised 12 leads of the bundled recordings: every covered element within (span + |s|) * 2^-24 of the
    stored signal -- one fp32 rounding of v, scaled by span, plus one fp32 rounding of the result.  Measured here: the worst ratio is 0.52 of
    that bound, the RMSE at most 8.2e-6 signal units, 1 - r at most 2.6e-13."""
    rp = resident.recording_plan(real, [0, 1], list(range(12)))
    sig = real.signal.numpy()
    views = rr.plan_items(real, rp.plan)["data"]
    assert views.shape == (30, 12, 512) and views.dtype == np.float32
    rng = ref.ranges(sig, rp.plan.table)
    out = np.full(int(rp.out_offsets[-1]), np.nan, dtype=np.float32)
    ref.stitch(views, rng, rp.stitch, out, "nan")
    worst = 0.0
    for j in range(2):
        s12 = ref.twelve(ref.store_recording(real, j)[0])
        got = out[rp.out_offsets[j]:rp.out_offsets[j + 1]].reshape(12, -1)
        p = real.labels[0][real.label_offsets[0][j]:real.label_offsets[0][j + 1]]
        covered = np.zeros(5000, dtype=bool)
        covered[p[0]:p[-1]] = True                            # no bundled beat is longer than 512
        assert covered.sum() == (4352, 4315)[j]
        assert np.isnan(got[:, ~covered]).all() and np.isfinite(got[:, covered]).all()
        for b in np.nonzero(rp.rec == j)[0]:
            q, n = int(rp.stitch[b, 0] - rp.out_offsets[j]), int(rp.stitch[b, 2])
            span = rng[b, 1] - rng[b, 0]
            err = np.abs(got[:, q:q + n].astype(np.float64) - s12[:, q:q + n])
            bound = (span + np.abs(s12[:, q:q + n])) * 2.0 ** -24
            assert (err <= bound).all()
            worst = max(worst, float((err / bound).max()))
    print("worst ratio to the bound", worst)
    st, _ = ref.stats(out, sig, rp.stitch, rp.recordings, rp.out_offsets, list(range(12)), "nan")
    assert np.array_equal(st[:, :, 0], np.array([[4352.0] * 12, [4315.0] * 12]))
    rmse, corr = ref.metrics(st)
    print("rmse max", rmse.max(), "1 - r max", (1 - corr).max())
    assert rmse.max() <= 8.2e-6 and (1 - corr).max() <= 2.6e-13 and corr.max() <= 1 + 1e-15
    # recording.metrics is the same arithmetic, vectorised
    r2, c2 = recording.metrics(st)
    assert np.allclose(r2, rmse, rtol=1e-15, atol=0) and np.allclose(c2, corr, rtol=1e-14, atol=0)
    zero = recording.metrics(np.zeros((1, 2, 7)))
    assert np.isnan(zero[0]).all() and np.isnan(zero[1]).all()


def test_bridge_and_hold_in_the_restatement():
    """The fill modes on a hand-made case: a 600-sample beat bridged into the next one, a 530-sample last beat held."""
    views = np.zeros((2, 1, 512), dtype=np.float32)
    views[0, 0, 511], views[1, 0, 0], views[1, 0, 511] = 1.0, 0.5, 0.25
    rng = np.array([[0.0, 10.0], [100.0, 300.0]])
    table = np.array([[5, 2000, 600, 1], [605, 2000, 530, 0]], dtype=np.int64)
    out = np.full(2000, -7.0, dtype=np.float32)
    ref.stitch(views, rng, table, out, "bridge")
    assert (out[:5] == -7).all() and (out[1135:] == -7).all() and out[5 + 511] == 10.0 and out[605] == 200.0
    t = np.arange(512, 600)
    assert np.array_equal(out[5 + 512:605], (10.0 + 190.0 * ((t - 511) / 89.0)).astype(np.float32))
    assert (out[605 + 511:1135] == 150.0).all()
    out2 = np.full(2000, -7.0, dtype=np.float32)
    ref.stitch(views, rng, table, out2, "nan")
    assert np.isnan(out2[5 + 512:605]).all() and np.isnan(out2[605 + 512:1135]).all() and np.array_equal(out2[5:517], out[5:517])


def test_gen_net_names_the_scheme_leads_or_asks_for_them():
    from electrocardio_panorama_amd import gen_net
    state = random.getstate()
    cfg = rr.make_cfg("unused", scheme=(3, "IIv2v5_v4I_372", "input_fix"))
    assert gen_net.scheme_leads(cfg) == [1, 3, 6]
    assert gen_net.scheme_leads(rr.make_cfg("unused", scheme=(2, "_228", "normal"))) == [1, 6]
    with pytest.raises(ValueError, match="--leads"):
        gen_net.scheme_leads(rr.make_cfg("unused", scheme=(3, "normal", "normal")))
    assert random.getstate() == state


def test_gen_net_is_one_rank_only(monkeypatch):
    from electrocardio_panorama_amd import gen_net
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one rank"):
        gen_net.main(rr.make_cfg("unused"))


def test_the_bindings_mirror_the_three_entries():
    from electrocardio_panorama_amd import _lib
    lib = _lib.load()
    for name, mirror in (("nef_beat_range", _lib.BeatRangeArgs), ("nef_beat_stitch", _lib.BeatStitchArgs),
                         ("nef_recording_stats", _lib.RecordingStatsArgs)):
        assert name in _lib.SIGNATURES and getattr(lib, name + "_args_bytes")() == __import__("ctypes").sizeof(mirror)
    assert lib.nef_abi_version() == 22


def test_ops_check_their_arguments_in_front_of_the_library():
    from electrocardio_panorama_amd import ops
    sig = torch.zeros(64, dtype=torch.int16)
    with pytest.raises(ValueError, match="leaves the signal"):
        ops.beat_range(sig, torch.tensor([[0, 8, 9, 0, 0]]), 1, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.beat_range(sig, torch.tensor([[0, 8, 8, 0, 0]]), 1, 0)
    with pytest.raises(ValueError, match="fill"):
        ops.beat_stitch(torch.zeros(1, 1, 512), torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(8), "hold")
    with pytest.raises(TypeError, match="views"):
        ops.beat_stitch(torch.zeros(1, 1, 511), torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(8), "nan")
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.beat_stitch(torch.zeros(1, 1, 512), torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(8), "nan")
    with pytest.raises(ValueError, match="score_leads"):
        ops.recording_stats(torch.zeros(8), sig, torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int64), [12], "nan",
                            torch.zeros(1, dtype=torch.int64))
