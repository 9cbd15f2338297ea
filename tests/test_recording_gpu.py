"""Whole recordings on the device: nef_beat_range, nef_beat_stitch and nef_recording_stats against the fp64 restatement of
tests/recording_ref.py -- the range and every stitched element bit for bit, the sums within 1e-12 of their terms' magnitudes -- the round
trip through nef_beat_batch on the bundled recordings, recording.synthesize end to end on both models and both panorama dtypes, and the
gen_net tool on a checkpoint a short training run wrote."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

import recording_ref as ref
import resident_ref as rr
from electrocardio_panorama_amd import ops, recording
from electrocardio_panorama_amd.dataset import resident
from test_resident_gpu import _cfg, _synthetic, on_device, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = ["int16", "float32"]


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    host = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp_path_factory.mktemp("real"))), "train")
    return {"int16": on_device(host, "real16"), "float32": on_device(host, "real32", float32=True)}


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    a, b = _synthetic(tmp_path_factory.mktemp("syn16"), 0), _synthetic(tmp_path_factory.mktemp("syn32"), 1)
    return {"int16": on_device(a, "syn16"), "float32": on_device(b, "syn32")}


_CASE = {}          # (store tag, A) -> the plan, its reference ranges, seeded views and a seeded output buffer, made once and never written


def case(store, A):
    key = (store.tag, A)
    if key not in _CASE:
        rp = resident.recording_plan(store, list(range(len(store))), [1, 3, 6], angles=A)
        sig = store.signal.cpu().numpy()
        g = np.random.default_rng(11 + A)
        Bt = rp.rec.size
        _CASE[key] = dict(rp=rp, sig=sig, rng=ref.ranges(sig, rp.plan.table), views=g.random((Bt, A, 512), dtype=np.float32),
                          init=g.normal(size=int(rp.out_offsets[-1])).astype(np.float32))
    return _CASE[key]


def same_f64(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


# ------------------------------------------------------------------------------------------------ nef_beat_range
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["real", "synthetic"])
def test_beat_range_is_the_restatements_and_beat_batchs(real, synthetic, which, dtype):
    store = {"real": real, "synthetic": synthetic}[which][dtype]
    rp = resident.recording_plan(store, list(range(len(store))), list(range(12)))
    sig = store.signal.cpu().numpy()
    ns = rp.stitch[:, 2].tolist()
    if which == "real":
        assert len(ns) == 30 and min(ns) == 265 and max(ns) == 315
    else:
        assert ns == [1, 2, 511, 183, 512, 513, 1300, 2677, 5000] + [9] * 9 + [290, 290]
        assert {int(v) % 8 for v in rp.plan.table[9:18, 0]} == set(range(8))
    table = torch.from_numpy(rp.plan.table)
    got = ops.beat_range(store.signal, table, 12, 0)                    # a host plan: checked and copied
    assert got.shape == (len(ns), 2) and got.dtype == torch.float64
    want = ref.ranges(sig, rp.plan.table)
    assert same_f64(got.cpu().numpy(), want)
    assert same_f64(ops.beat_range(store.signal, table.to(DEV), 12, 0).cpu().numpy(), want)
    # ... and the lo / hi behind beat_batch's rows: (float)((s - lo) / span) is reproduced from them
    data = ops.beat_batch(store.signal, table, 12, 0)[0].cpu().numpy()
    lo, hi = got.cpu().numpy().T
    for b, (off, stride, n) in enumerate(rp.plan.table[:, :3].tolist()):
        m = min(n, 512)
        s12 = ref.twelve(np.stack([sig[off + k * stride:off + k * stride + m] for k in range(8)]))
        with np.errstate(invalid="ignore", divide="ignore"):
            assert same_bits(data[b, :, :m], ((s12 - lo[b]) / (hi[b] - lo[b])).astype(np.float32)), b


def test_beat_range_of_a_device_row_outside_the_signal_is_nan(real):
    store = real["int16"]
    rp = resident.recording_plan(store, [0], [1, 3, 6])
    t = rp.plan.table[:4].copy()
    t[1, 5] = 12                      # a lead outside 0..11
    t[2, 1], t[2, 2] = 100, 101       # n > stride
    t[3, 0] = store.signal.numel()    # behind the signal
    got = ops.beat_range(store.signal, torch.from_numpy(t).to(DEV), 3, 0).cpu().numpy()
    assert same_f64(got[:1], ref.ranges(store.signal.cpu().numpy(), t[:1])) and np.isnan(got[1:]).all()
    with pytest.raises(ValueError, match="leaves the signal"):
        ops.beat_range(store.signal, torch.from_numpy(t), 3, 0)


# ------------------------------------------------------------------------------------------------ nef_beat_stitch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", ["nan", "bridge"])
@pytest.mark.parametrize("A", [1, 12, 13])
def test_stitch_matches_the_restatement_bit_for_bit(synthetic, A, fill, dtype):
    """Every beat length and P onset residue of the synthetic store, the odd-length recording (5003: angle rows not 16-byte aligned), the
    last beat of a recording (hold), n = 1300 bridged into n = 2677, the constant beat, and every position outside a beat keeping its bits."""
    c = case(synthetic[dtype], A)
    rp = c["rp"]
    want = ref.stitch(c["views"], c["rng"], rp.stitch, c["init"].copy(), fill)
    out = torch.from_numpy(c["init"]).to(DEV)
    back = ops.beat_stitch(torch.from_numpy(c["views"]).to(DEV), torch.from_numpy(c["rng"]), torch.from_numpy(rp.stitch), out, fill)
    assert back is out
    got = out.cpu().numpy()
    assert same_bits(got, want)
    for j, (first, rows, _, ln) in enumerate(rp.recordings.tolist()):
        sigs = got[rp.out_offsets[j]:rp.out_offsets[j + 1]].reshape(A, ln)
        p0, p1 = int(rp.stitch[first, 0] - rp.out_offsets[j]), int(rp.stitch[first + rows - 1, 0] - rp.out_offsets[j] + rp.stitch[first + rows - 1, 2])
        keep = c["init"][rp.out_offsets[j]:rp.out_offsets[j + 1]].reshape(A, ln)
        assert np.array_equal(sigs[:, :p0], keep[:, :p0]) and np.array_equal(sigs[:, p1:], keep[:, p1:])
    # the constant beat (recording 4, beat 0: hi == lo) is the constant lo
    b = int(rp.recordings[4, 0])
    assert c["rng"][b, 0] == c["rng"][b, 1]
    q = int(rp.stitch[b, 0])
    assert (got[q:q + 290] == np.float32(c["rng"][b, 0])).all()
    tail = got[int(rp.stitch[6, 0]) + 512:int(rp.stitch[6, 0]) + 1300]              # n = 1300, followed by n = 2677
    assert np.isnan(tail).all() if fill == "nan" else np.isfinite(tail).all()


@pytest.mark.parametrize("fill", ["nan", "bridge"])
def test_stitch_of_strided_views_two_launches_and_a_row_that_leaves_the_output(synthetic, fill):
    c = case(synthetic["int16"], 12)
    rp, Bt = c["rp"], c["rp"].rec.size
    want = ref.stitch(c["views"], c["rng"], rp.stitch, c["init"].copy(), fill)
    big = torch.zeros((Bt, 15, 516), dtype=torch.float32, device=DEV)
    rng, table = torch.from_numpy(c["rng"]).to(DEV), torch.from_numpy(rp.stitch).to(DEV)
    for shift in (0, 1):              # rows 16-byte aligned, and rows at an odd 4-byte address
        views = big[:, 2:14, shift:shift + 512]
        views.copy_(torch.from_numpy(c["views"]))
        assert not views.is_contiguous()
        out = torch.from_numpy(c["init"]).to(DEV)
        cut = int(rp.recordings[2, 0])                                    # two launches into one buffer, cut between recordings
        ops.beat_stitch(views[:cut], rng[:cut], table[:cut], out, fill)
        ops.beat_stitch(views[cut:], rng[cut:], table[cut:], out, fill)
        assert same_bits(out.cpu().numpy(), want)
    # an output buffer at an odd 4-byte address
    buf = torch.zeros(c["init"].size + 1, dtype=torch.float32, device=DEV)
    out = buf[1:]
    out.copy_(torch.from_numpy(c["init"]))
    ops.beat_stitch(torch.from_numpy(c["views"]).to(DEV), rng, table, out, fill)
    assert same_bits(out.cpu().numpy(), want)
    # device rows that would leave the output write nothing; the other rows are written
    bad = rp.stitch.copy()
    bad[0, 0] = c["init"].size                                   # behind the buffer
    bad[5, 0] = c["init"].size - 11 * 5003 - 512                 # its last angle row ends one element behind the buffer
    bad[9, 2] = bad[9, 1] + 1                                    # n > stride
    bad[12, 0] = -1
    want_bad = ref.stitch(c["views"], c["rng"], bad, c["init"].copy(), fill)
    for b in (0, 5, 9, 12):
        q = int(rp.stitch[b, 0])
        assert np.array_equal(want_bad[q:q + 1], c["init"][q:q + 1])
    out = torch.from_numpy(c["init"]).to(DEV)
    ops.beat_stitch(torch.from_numpy(c["views"]).to(DEV), rng, torch.from_numpy(bad).to(DEV), out, fill)
    assert same_bits(out.cpu().numpy(), want_bad)
    with pytest.raises(ValueError, match="leaves the output"):
        ops.beat_stitch(torch.from_numpy(c["views"]).to(DEV), rng, torch.from_numpy(bad), out, fill)


def test_fill_leaves_beats_of_up_to_512_samples_alone(synthetic):
    c = case(synthetic["float32"], 12)
    rp = c["rp"]
    outs = []
    for fill in ("nan", "bridge"):
        out = torch.from_numpy(c["init"]).to(DEV)
        ops.beat_stitch(torch.from_numpy(c["views"]).to(DEV), torch.from_numpy(c["rng"]), torch.from_numpy(rp.stitch), out, fill)
        outs.append(out.cpu().numpy())
    differ = np.zeros(outs[0].size, dtype=bool)
    for base, stride, n, _ in rp.stitch.tolist():
        for a in range(12):
            differ[base + a * stride + 512:base + a * stride + max(n, 512)] = True
    assert differ.sum() == 12 * (1 + 788 + 2165 + 4488)
    assert outs[0][~differ].tobytes() == outs[1][~differ].tobytes() and np.isnan(outs[0][differ]).all() and np.isfinite(outs[1][differ]).all()


# ------------------------------------------------------------------------------------------------ nef_recording_stats
SCORE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]


def stitched(c, fill):
    rp = c["rp"]
    return ref.stitch(c["views"], c["rng"], rp.stitch, c["init"].copy(), fill)


def within(got, want, mag):
    return bool((np.abs(got - want) <= 1e-12 * mag).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", ["nan", "bridge"])
def test_stats_match_the_restatement_and_do_not_depend_on_the_launch(synthetic, fill, dtype):
    store = synthetic[dtype]
    c = case(store, 12)
    rp = c["rp"]
    host = stitched(c, fill)
    score = [0, 9, 2, -1, 11, 5, 6, 7, 8, 1, 10, 3]
    want, mag = ref.stats(host, c["sig"], rp.stitch, rp.recordings, rp.out_offsets, score, fill)
    out = torch.from_numpy(host).to(DEV)
    bt, rt, oo = torch.from_numpy(rp.stitch), torch.from_numpy(rp.recordings), torch.from_numpy(rp.out_offsets[:-1].copy())
    got_t = ops.recording_stats(out, store.signal, bt, rt, score, fill, oo)
    assert got_t.shape == (5, 12, 7) and got_t.dtype == torch.float64
    got = got_t.cpu().numpy()
    cover = [sum(n if fill == "bridge" else min(n, 512) for n in rp.stitch[f:f + r, 2].tolist()) for f, r in rp.recordings[:, :2].tolist()]
    assert np.array_equal(got[:, :, 0], np.array([[0.0 if s == -1 else float(n) for s in score] for n in cover]))
    assert np.array_equal(got[:, :, 0], want[:, :, 0]) and within(got, want, mag)
    assert not got[:, 3].any() and np.isfinite(got).all()
    # a recording launched alone, device tables, other N: the same bits
    for j in (1, 4):
        alone = ops.recording_stats(out, store.signal, bt.to(DEV), rt[j:j + 1].to(DEV), score, fill, oo[j:j + 1].to(DEV)).cpu().numpy()
        assert alone.shape == (1, 12, 7) and alone.tobytes() == got[j:j + 1].tobytes()
    # one angle a launch (A = 1): the output's layout is the tables', not the launch's
    one = ops.recording_stats(out, store.signal, bt, rt, [score[0]], fill, oo).cpu().numpy()
    assert one.shape == (5, 1, 7) and one.tobytes() == np.ascontiguousarray(got[:, :1]).tobytes()
    # a NaN in one prediction: the sums of that (recording, angle) that see x are NaN, nothing else moves
    pos = int(rp.stitch[5, 0]) + 4 * 5003 + 17               # recording 1, angle 4, inside the n = 513 beat
    out[pos] = float("nan")
    hit = ops.recording_stats(out, store.signal, bt, rt, score, fill, oo).cpu().numpy()
    assert np.isnan(hit[1, 4, [1, 2, 4, 6]]).all() and np.array_equal(hit[1, 4, [0, 3, 5]], got[1, 4, [0, 3, 5]])
    hit[1, 4] = got[1, 4]
    assert hit.tobytes() == got.tobytes()


def test_stats_of_tables_that_leave_the_buffers(synthetic):
    store = synthetic["int16"]
    c = case(store, 12)
    rp = c["rp"]
    out = torch.from_numpy(stitched(c, "nan")).to(DEV)
    bt, rt, oo = torch.from_numpy(rp.stitch), torch.from_numpy(rp.recordings.copy()), torch.from_numpy(rp.out_offsets[:-1].copy())
    good = ops.recording_stats(out, store.signal, bt, rt, SCORE, "nan", oo).cpu().numpy()
    rt[0, 2] = store.signal.numel() - 8 * 700 + 1            # recording 0 would end one element behind the signal
    oo[2] = out.numel() - 12 * 5000 + 1                      # recording 2 one element behind the output
    rt[3, 0] = 12                                            # recording 3's nine rows would run past the beat table
    with pytest.raises(ValueError, match="leaves the signal"):
        ops.recording_stats(out, store.signal, bt, rt, SCORE, "nan", oo)
    got = ops.recording_stats(out, store.signal, bt.to(DEV), rt.to(DEV), SCORE, "nan", oo.to(DEV)).cpu().numpy()
    assert np.isnan(got[[0, 2, 3]]).all() and got[[1, 4]].tobytes() == good[[1, 4]].tobytes()
    lead13 = ops.recording_stats(out, store.signal, bt, torch.from_numpy(rp.recordings), torch.tensor([0, 12], dtype=torch.int32).to(DEV),
                                 "nan", torch.from_numpy(rp.out_offsets[:-1].copy())).cpu().numpy()
    assert np.isnan(lead13[:, 1]).all() and lead13[:, 0].tobytes() == np.ascontiguousarray(good[:, 0]).tobytes()


# ------------------------------------------------------------------------------------------------ the round trip on the device
@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip_of_the_bundled_recordings(real, dtype):
    """beat_batch on all 12 leads, beat_range, beat_stitch, recording_stats: the stored signal comes back within the bounds
    tests/test_recording_cpu.py derives, and the device's signals are the restatement's bit for bit."""
    store = real[dtype]
    rp = resident.recording_plan(store, [0, 1], list(range(12)))
    table = torch.from_numpy(rp.plan.table).to(DEV)
    views = ops.beat_batch(store.signal, table, 12, 0)[0]
    rng = ops.beat_range(store.signal, table, 12, 0)
    out = torch.full((int(rp.out_offsets[-1]),), float("nan"), dtype=torch.float32, device=DEV)
    ops.beat_stitch(views, rng, torch.from_numpy(rp.stitch), out, "nan")
    st = ops.recording_stats(out, store.signal, torch.from_numpy(rp.stitch), torch.from_numpy(rp.recordings), SCORE, "nan",
                             torch.from_numpy(rp.out_offsets[:-1].copy())).cpu().numpy()
    sig = store.signal.cpu().numpy()
    want = np.full(int(rp.out_offsets[-1]), np.nan, dtype=np.float32)
    ref.stitch(rr.plan_items(store, rp.plan)["data"], ref.ranges(sig, rp.plan.table), rp.stitch, want, "nan")
    assert same_bits(out.cpu().numpy(), want)
    assert np.array_equal(st[:, :, 0], np.array([[4352.0] * 12, [4315.0] * 12]))
    rmse, corr = recording.metrics(st)
    print("rmse max", rmse.max(), "1 - r max", (1 - corr).max())
    assert rmse.max() <= 8.2e-6 and (1 - corr).max() <= 2.6e-13
    want_st, mag = ref.stats(want, sig, rp.stitch, rp.recordings, rp.out_offsets, SCORE, "nan")
    assert within(st, want_st, mag)


# ------------------------------------------------------------------------------------------------ end to end
def _model(kind):
    import test_model_gpu as tm
    return tm.hashed_model(3).eval() if kind == "nefnet" else tm.hashed_model2(3)


@pytest.mark.parametrize("half", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["nefnet", "nefnet2"])
def test_synthesize_end_to_end(synthetic, kind, half):
    store = synthetic["int16"]
    model = _model(kind)
    model.panorama_dtype = half
    mode = model.training
    assert mode == (kind == "nefnet2")
    before, state = store.signal.clone(), random.getstate()
    sig = store.signal.cpu().numpy()
    for bpp, fill in ((256, "bridge"), (7, "nan")):
        syn = recording.synthesize(model, store, range(5), [1, 3, 6], fill=fill, beats_per_pass=bpp, return_views=True)
        rp = syn.plan
        assert recording.chunks(rp, bpp) == ([(0, 20)] if bpp == 256 else [(0, 4), (4, 9), (9, 18), (18, 20)])
        assert model.training == mode and random.getstate() == state and torch.equal(store.signal, before)
        views, rng = syn.views.cpu().numpy(), syn.range.cpu().numpy()
        assert views.shape == (20, 12, 512) and same_f64(rng, ref.ranges(sig, rp.plan.table))
        want = ref.stitch(views, rng, rp.stitch, np.full(int(rp.out_offsets[-1]), np.nan, dtype=np.float32), fill)
        assert same_bits(syn.out.cpu().numpy(), want)
        sigs = syn.signals
        assert [tuple(s.shape) for s in sigs] == [(12, 700), (12, 5003), (12, 5000), (12, 1000), (12, 600)]
        assert sigs[1].data_ptr() == syn.out.data_ptr() + 4 * 12 * 700
        # the constant beat (row 18) went in as zeros: no NaN in any view, its own included, so none reached the chunk's shared scales
        assert rng[18, 0] == rng[18, 1] and np.isfinite(views).all()
        q = int(rp.stitch[18, 0])
        assert (want[q:q + 290] == np.float32(rng[18, 0])).all()
        st = syn.stats.cpu().numpy()
        want_st, mag = ref.stats(want, sig, rp.stitch, rp.recordings, rp.out_offsets, SCORE, fill)
        assert np.array_equal(st[:, :, 0], want_st[:, :, 0]) and within(st, want_st, mag)
        rmse, corr = syn.rmse, syn.corr
        assert rmse.shape == corr.shape == (5, 12) and np.isfinite(rmse).all()
        assert np.allclose(rmse, ref.metrics(want_st)[0], rtol=1e-9, equal_nan=True)
    with pytest.raises(ValueError, match="the model is on"):
        recording.synthesize(copy.deepcopy(model).cpu(), store, [0], [1, 3, 6])


def test_panorama_takes_shared_or_per_sample_angles(synthetic):
    store = synthetic["int16"]
    model = _model("nefnet")
    rp = resident.recording_plan(store, [3], [1, 3, 6])
    data = ops.beat_batch(store.signal, torch.from_numpy(rp.plan.table), 3, 0)[0]
    th, rois = torch.from_numpy(rp.plan.input_theta).to(DEV), torch.from_numpy(rp.plan.rois).to(DEV)
    q = torch.from_numpy(rr.lead_theta()[[0, 7]].astype(np.float32)).to(DEV)
    shared = model.panorama(data, th, rois, q)
    each = model.panorama(data, th, rois, q.unsqueeze(0).expand(9, 2, 2))
    # the same decoder on the same latent; the split-fp16 convs may re-measure their operand scales between two calls: 2^-22 relative
    assert shared.shape == (9, 2, 512) and torch.allclose(shared, each, rtol=0, atol=1e-5) and not model.training
    z1, z2 = model(data, th, th[:, 0], rois, phase="gen")
    assert torch.allclose(shared, model.gen_ecg(z1, z2, q.unsqueeze(0).expand(9, 2, 2).contiguous(), rois), rtol=0, atol=1e-5)
    with pytest.raises(ValueError, match="query_thetas"):
        model.panorama(data, th, rois, q.unsqueeze(0).expand(8, 2, 2))


def test_gen_net_on_a_trained_checkpoint(tmp_path, capsys, monkeypatch):
    """Two epochs of Solver.train on the bundled listing write epoch_1.pkl; gen_net.run prints the four numbers, writes [12, 5000] float32
    files and a metrics.json that holds what synthesize gives for the same weights."""
    from electrocardio_panorama_amd import gen_net, train_net
    from electrocardio_panorama_amd.prefetch import DevicePrefetcher
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.utils import CheckPointer
    cfg = _cfg(tmp_path, repeat=1, epochs=2)
    run_cfg = cfg.clone()                        # what the tool sees: it appends the description to the output directory itself
    cfg.output_dir = os.path.join(str(tmp_path), "resident")
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    random.seed(100)
    sol.train(DevicePrefetcher(train, sol.device), DevicePrefetcher(test, sol.device))
    assert os.path.exists(os.path.join(str(tmp_path), "resident", "resident", "epoch_1.pkl"))
    monkeypatch.setattr(gen_net, "cfg", run_cfg)
    out_dir = tmp_path / "strips"
    capsys.readouterr()
    result = gen_net.run(["--epoch", "1", "--out", str(out_dir)])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("rec_rmse_reg:")]
    assert len(line) == 1 and [p.split(":")[0].strip() for p in line[0].split(",")] == ["rec_rmse_reg", "rec_corr_reg", "rec_rmse_gen", "rec_corr_gen"]
    assert [float(p.split(":")[1]) for p in line[0].split(",")] == [result[k] for k in ("rec_rmse_reg", "rec_corr_reg", "rec_rmse_gen", "rec_corr_gen")]
    assert all(np.isfinite(v) for v in result.values())
    files = {n: np.load(out_dir / (n + ".npy")) for n in rr.NAMES}
    assert all(a.shape == (12, 5000) and a.dtype == np.float32 for a in files.values())
    doc = json.loads((out_dir / "metrics.json").read_text())
    assert doc["input_leads"] == [1, 3, 6] and doc["ids"] == [n + ".json" for n in rr.NAMES] and doc["fill"] == "nan"
    # the same weights through synthesize
    sol2 = Solver(cfg, use_tensorboardx=False)
    CheckPointer(sol2.model, save_dir=sol2.output_dir).load(os.path.join(sol2.output_dir, "epoch_1.pkl"))
    store = resident.ResidentTianchi(cfg, "test", sol2.device)
    syn = recording.synthesize(sol2.model, store, range(2), [1, 3, 6])
    assert np.allclose(np.array(doc["rmse"]), syn.rmse, rtol=1e-12, atol=0) and np.allclose(np.array(doc["corr"]), syn.corr, rtol=1e-12, atol=0)
    for j, n in enumerate(rr.NAMES):
        assert same_bits(files[n], syn.signals[j].cpu().numpy())
    rest = [k for k in range(12) if k not in (1, 3, 6)]
    assert result["rec_rmse_gen"] == float(np.mean(syn.rmse[:, rest])) and result["rec_corr_reg"] == float(np.mean(syn.corr[:, [1, 3, 6]]))
