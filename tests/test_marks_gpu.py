"""Marks for unannotated recordings on the device: nef_mark_envelope and nef_mark_peaks against the literal loops of tests/marks_ref.py,
bit for bit on whole buffers (the untouched gaps and the -1 tails included), and cfg.DATA.auto_marks end to end in a directory that holds
the two bundled signals and no label file: the loader, one Solver.train run, the round trip of whole recordings, gen_net and mark_net."""
import json
import os
import random

import numpy as np
import pytest
import torch

import marks_ref as mref
import resident_ref as rr
from electrocardio_panorama_amd import ops, train_net
from electrocardio_panorama_amd.dataset import marks, resident

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
D, H, R, SEG = 2, 20, 100, 1000
LENGTHS = [1, 2, D, 2 * H, SEG - 1, SEG, SEG + 1, 1023, 1024, 1025, 2100, 2100, 2100]
SENTINEL = -7.25


class Store:
    """What marks.detect reads of a resident store."""

    def __init__(self, signal, offsets, lengths):
        self.signal, self.offsets, self.lengths = signal, np.asarray(offsets, dtype=np.int64), np.asarray(lengths, dtype=np.int64)

    def __len__(self):
        return self.lengths.size


def _recordings(floats):
    """One [8, len] recording per entry of LENGTHS: noise with QRS-like bursts every ~300 samples; the last two are silent but for impulses
    that put an envelope plateau's first position on the tile seam (t = 1024, and t = 1023) with a lower one within r in front of it."""
    g = np.random.default_rng(17 + floats)
    out = []
    for n in LENGTHS[:-2]:
        x = g.normal(0, 12, size=(8, n))
        for q in range(37, n, 293):
            w = min(9, n - q)
            x[:, q:q + w] += g.normal(0, 900, size=(8, 1)) * np.hanning(11)[1:1 + w]
        out.append(x.astype(np.float32) if floats else np.rint(x).astype(np.int16))
    for first in (1024, 1023):
        x = np.zeros((8, 2100))
        x[0, first - D + H] = 100.0            # e = 100^2 at q - D and q + D: the plateau of 2 * 100^2 starts at q + D - H = first
        x[3, first - D + H - 80] = 90.0        # a lower plateau 80 in front: suppressed across the seam
        x[5, 300], x[5, 300 + R + 2 * D] = 50.0, 50.0
        out.append(x.astype(np.float32) if floats else x.astype(np.int16))
    return out


_BUILT = {}


@pytest.fixture(scope="module", params=["int16", "float32"])
def synthetic(request):
    return _build(request.param == "float32")


def _build(floats):
    """A flat signal whose recordings start at every residue mod 8, the device table with gaps in `env` too, and the restatement's envelope
    of every recording -- computed once per dtype and never written."""
    if floats not in _BUILT:
        _BUILT[floats] = _build_once(floats)
    return _BUILT[floats]


def _build_once(floats):
    recs = _recordings(floats)
    parts, offsets, pos = [], [], 0
    for i, x in enumerate(recs):
        gap = i % 8 if i else 0
        parts.append(np.zeros(gap, dtype=x.dtype))
        offsets.append(pos + gap)
        parts.append(x.reshape(-1))
        pos += gap + x.size
    flat = np.concatenate(parts)
    assert {o % 8 for o in offsets} == set(range(8))
    lengths = np.array(LENGTHS, dtype=np.int64)
    eoff = np.concatenate([[0], np.cumsum(lengths + 3)[:-1]]) + 1          # three untouched doubles between two envelopes, one in front
    env = [mref.envelope(x, D, H) for x in recs]
    return dict(recs=recs, signal=torch.from_numpy(flat).to(DEV), offsets=np.array(offsets), lengths=lengths, eoff=eoff, env=env,
                env_elems=int(eoff[-1] + lengths[-1] + 2), floats=floats)


def _want_env(c, envs, rows=None):
    want = np.full(c["env_elems"], SENTINEL)
    for i in (range(len(envs)) if rows is None else rows):
        want[c["eoff"][i]:c["eoff"][i] + c["lengths"][i]] = envs[i]
    return torch.from_numpy(want)


def _table(c, rows=None):
    t = np.stack([c["offsets"], c["lengths"], c["eoff"]], axis=1).astype(np.int64)
    return torch.from_numpy(np.ascontiguousarray(t if rows is None else t[list(rows)]))


def _same_level(got, want):
    got, want = got.cpu(), torch.as_tensor(want, dtype=torch.float64)
    nan = torch.isnan(want)
    return got.dtype == torch.float64 and torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan])


def _want_peaks(envs, lengths=None, **kw):
    rows = [mref.peaks(e, **kw) for e in envs]
    return torch.from_numpy(np.stack([r[0] for r in rows])), torch.tensor([r[1] for r in rows], dtype=torch.int32), [r[2] for r in rows]


# ------------------------------------------------------------------------------------------------ nef_mark_envelope
def test_envelope_is_the_restatement_bit_for_bit(synthetic):
    c = synthetic
    env = torch.full((c["env_elems"],), SENTINEL, dtype=torch.float64, device=DEV)
    back = ops.mark_envelope(c["signal"], _table(c), env, D=D, H=H)                       # a host table: checked and copied
    assert back is env and torch.equal(env.cpu(), _want_env(c, c["env"]))
    if not c["floats"]:
        assert all(float(e.max()) < 2.0 ** 41 and np.array_equal(e, np.rint(e)) for e in c["env"])
    # a device table (max_len given), two launches over disjoint rows, a recording alone: the same bits, nothing else touched
    env2 = torch.full_like(env, SENTINEL)
    ops.mark_envelope(c["signal"], _table(c, range(0, 5)).to(DEV), env2, D=D, H=H, max_len=1000)
    ops.mark_envelope(c["signal"], _table(c, range(5, 13)).to(DEV), env2, D=D, H=H, max_len=2100)
    assert torch.equal(env2, env)
    alone = torch.full_like(env, SENTINEL)
    ops.mark_envelope(c["signal"], _table(c, [10]), alone, D=D, H=H)
    assert torch.equal(alone.cpu(), _want_env(c, c["env"], rows=[10]))


@pytest.mark.parametrize("bits,d,h", [(0b00100101, 2, 20), (0b10000000, 1, 0), (255, 7, 256), (1, 0, 3)])
def test_envelope_of_a_lead_subset_and_other_windows(synthetic, bits, d, h):
    c = synthetic
    rows = [0, 1, 3, 7, 9, 11]
    env = torch.full((c["env_elems"],), SENTINEL, dtype=torch.float64, device=DEV)
    ops.mark_envelope(c["signal"], _table(c, rows), env, D=d, H=h, lead_bits=bits)
    envs = {i: mref.envelope(c["recs"][i], d, h, bits) for i in rows}
    assert torch.equal(env.cpu(), _want_env(c, envs, rows=rows))


def test_envelope_rows_that_leave_a_buffer_write_nothing_and_bad_arguments_raise(synthetic):
    c = synthetic
    t = _table(c, [4, 5, 6, 7, 8]).clone()
    t[0, 0] = c["signal"].numel() - 8 * 999 + 1        # one element behind the signal
    t[1, 2] = c["env_elems"] - 1000 + 1                # one element behind env
    t[2, 1] = 0                                        # no positions
    t[3, 0] = -1
    env = torch.full((c["env_elems"],), SENTINEL, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="leaves the signal"):
        ops.mark_envelope(c["signal"], t, env)
    ops.mark_envelope(c["signal"], t.to(DEV), env, max_len=1024)
    assert torch.equal(env.cpu(), _want_env(c, c["env"], rows=[8]))
    ops.mark_envelope(c["signal"], _table(c, [8, 9]).to(DEV), env.fill_(SENTINEL), max_len=1024)      # 1025 > max_len: that row is left out
    assert torch.equal(env.cpu(), _want_env(c, c["env"], rows=[8]))
    for kw, exc in ((dict(D=-1), ValueError), (dict(H=257), ValueError), (dict(lead_bits=0), ValueError), (dict(lead_bits=256), ValueError)):
        with pytest.raises(exc):
            ops.mark_envelope(c["signal"], _table(c), env, **kw)
    with pytest.raises(ValueError, match="max_len"):
        ops.mark_envelope(c["signal"], _table(c).to(DEV), env)
    with pytest.raises(TypeError):
        ops.mark_envelope(c["signal"], _table(c), env.float())
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mark_envelope(c["signal"].cpu(), _table(c), env)


# ------------------------------------------------------------------------------------------------ nef_mark_peaks
def test_peaks_of_the_synthetic_store_are_the_restatements(synthetic):
    c = synthetic
    env = torch.full((c["env_elems"],), SENTINEL, dtype=torch.float64, device=DEV)
    ops.mark_envelope(c["signal"], _table(c), env, D=D, H=H)
    peaks, count, level = ops.mark_peaks(env, _table(c), max_peaks=16)
    wp, wc, wl = _want_peaks(c["env"], max_peaks=16)
    assert peaks.dtype == count.dtype == torch.int32 and torch.equal(peaks.cpu(), wp) and torch.equal(count.cpu(), wc) and _same_level(level, wl)
    assert wc.tolist()[-2:] == [2, 2] and wp[-2, :2].tolist() == [300 + D - H, 1024] and wp[-1, :2].tolist() == [300 + D - H, 1023]
    assert int(wc[10]) >= 6 and int(wc[:4].min()) >= 0
    # more peaks than a small max_peaks: the first ones, the true count
    few = ops.mark_peaks(env, _table(c, [10]), max_peaks=3)
    assert torch.equal(few[0].cpu(), wp[10:11, :3]) and torch.equal(few[1].cpu(), wc[10:11]) and int(wc[10]) > 3
    # a recording alone, a device table, other launch sizes: the same bits
    for rows in ([10], [12, 3, 10]):
        got = ops.mark_peaks(env, _table(c, rows).to(DEV), max_peaks=16, max_len=2100)
        assert torch.equal(got[0].cpu(), wp[rows]) and torch.equal(got[1].cpu(), wc[rows]) and _same_level(got[2], [wl[i] for i in rows])
    # other parameters
    for kw in (dict(r=0, seg=7, frac=0.0), dict(r=512, seg=100000, frac=1.0), dict(r=5, seg=333, frac=0.5)):
        got = ops.mark_peaks(env, _table(c), max_peaks=64, **kw)
        wp2, wc2, wl2 = _want_peaks(c["env"], max_peaks=64, **kw)
        assert torch.equal(got[0].cpu(), wp2) and torch.equal(got[1].cpu(), wc2) and _same_level(got[2], wl2), kw


def test_peaks_of_hand_made_envelopes_ties_plateaus_ends_zeros_and_non_finite():
    n = 2600
    base = np.zeros(n)
    cases = {}
    e = base.copy(); e[[400, 400 + R]] = 5.0; cases["tie at r"] = (e, [400])                      # the later of two equals within r is out
    e = base.copy(); e[[400, 400 + R + 1]] = 5.0; cases["tie at r + 1"] = (e, [400, 401 + R])
    e = base.copy(); e[700:720] = 3.0; e[720 + R - 20] = 3.0; cases["plateau"] = (e, [700])        # ... its earliest position, and it hides an equal
    e = base.copy(); e[0], e[n - 1] = 2.0, 2.0; cases["ends"] = (e, [0, n - 1])
    e = base.copy(); e[1023], e[1023 + R] = 4.0, 4.5; cases["across the seam"] = (e, [1023 + R])
    e = base.copy(); e[1024], e[1023 - R] = 4.0, 3.5; cases["seam"] = (e, [923, 1024])
    cases["zeros"] = (base.copy(), [])
    e = base.copy(); e[::150] = 1.0; e[1500] = 80.0; cases["level"] = (e, None)                    # one tall segment does not lift the median
    e = base.copy(); e[300] = 1.0; e[1700] = float("nan"); cases["nan"] = (e, None)
    e = base.copy(); e[300] = 1.0; e[2599] = float("inf"); cases["inf"] = (e, None)
    names = list(cases)
    envs = [cases[k][0] for k in names]
    env = torch.from_numpy(np.concatenate(envs)).to(DEV)
    table = torch.tensor([[0, n, i * n] for i in range(len(names))], dtype=torch.int64)
    peaks, count, level = ops.mark_peaks(env, table, max_peaks=32)
    wp, wc, wl = _want_peaks(envs, max_peaks=32)
    assert torch.equal(peaks.cpu(), wp) and torch.equal(count.cpu(), wc) and _same_level(level, wl)
    for i, k in enumerate(names):
        if cases[k][1] is not None:
            assert wp[i, :int(wc[i])].tolist() == cases[k][1], k
    assert wc[names.index("zeros")] == 0 and wl[names.index("zeros")] == 0.0 and wl[names.index("level")] == 1.0
    for k in ("nan", "inf"):
        i = names.index(k)
        assert int(count[i]) == -1 and bool(torch.isnan(level[i])) and bool((peaks[i] == -1).all())
    # rows that would leave env, or are longer than max_len: count -1, NaN, -1s; the others keep their bits
    bad = table.clone()
    bad[0, 2], bad[1, 1], bad[2, 1] = env.numel() - n + 1, 0, n + 1
    got = ops.mark_peaks(env, bad.to(DEV), max_peaks=32, max_len=n)
    assert got[1][:3].tolist() == [-1, -1, -1] and bool(torch.isnan(got[2][:3]).all()) and bool((got[0][:3] == -1).all())
    assert torch.equal(got[0][3:].cpu(), wp[3:]) and torch.equal(got[1][3:].cpu(), wc[3:])
    with pytest.raises(ValueError, match="leaves"):
        ops.mark_peaks(env, bad, max_peaks=32)
    for kw in (dict(r=513), dict(seg=0), dict(max_peaks=0), dict(frac=-0.5), dict(frac=float("nan")), dict(seg=1, max_len=5000)):
        with pytest.raises(ValueError):
            ops.mark_peaks(env, table.to(DEV), **{"max_len": n, **kw})


def test_a_planted_nan_marks_its_recording_only():
    c = _build(True)
    sig = c["signal"].clone()
    sig[int(c["offsets"][9]) + 3 * 1025 + 500] = float("nan")
    store = Store(sig, c["offsets"], c["lengths"])
    got = marks.detect(store, params=marks.MarkParams(max_peaks=16))
    wp, wc, wl = _want_peaks(c["env"], max_peaks=16)
    assert got.count[9] == -1 and np.isnan(got.level[9]) and (got.peaks[9] == -1).all()
    keep = [i for i in range(13) if i != 9]
    assert np.array_equal(got.peaks[keep], wp.numpy()[keep]) and np.array_equal(got.count[keep], wc.numpy()[keep])
    assert np.array_equal(got.level[keep], np.array(wl)[keep])


def test_detect_in_chunks_and_on_a_subset_gives_the_same_rows(synthetic):
    c = synthetic
    store = Store(c["signal"], c["offsets"], c["lengths"])
    p = marks.MarkParams(max_peaks=16)
    whole = marks.detect(store, params=p)
    wp, wc, wl = _want_peaks(c["env"], max_peaks=16)
    assert np.array_equal(whole.peaks, wp.numpy()) and np.array_equal(whole.count, wc.numpy()) and np.array_equal(whole.level, np.array(wl))
    assert len(marks._chunks(c["lengths"].tolist(), 3000)) > 4
    for budget in (3000, 1):                      # several recordings a chunk, and every recording a chunk of its own
        cut = marks.detect(store, params=p, budget=budget)
        assert all(np.array_equal(a, b) for a, b in zip(cut, whole))
    some = marks.detect(store, indices=[12, 4, 10], params=p, budget=2500)
    assert all(np.array_equal(a, b[[12, 4, 10]]) for a, b in zip(some, whole))


# ------------------------------------------------------------------------------------------------ the bundled recordings, end to end
@pytest.fixture(scope="module")
def bundled(tmp_path_factory):
    """A directory with the two bundled signals as .npy and NO label file, its cfg, the annotated store on the device, and the table fitted
    on that store -- by the device's own peaks, which are the restatement's."""
    tmp = tmp_path_factory.mktemp("signals")
    os.makedirs(tmp / "npy")
    recs = rr.recordings()
    for name, sig, _ in recs:
        np.save(tmp / "npy" / name.replace(".json", ".npy"), sig)
    (tmp / "list.txt").write_text("".join(name + "\n" for name, _, _ in recs))
    annotated = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp)), "train", DEV)
    found = marks.detect(annotated)
    rows = [mref.peaks(mref.envelope(sig)) for _, sig, _ in recs]
    assert np.array_equal(found.peaks, np.stack([r[0] for r in rows])) and found.count.tolist() == [19, 16] == [r[1] for r in rows]
    assert np.array_equal(found.level, np.array([r[2] for r in rows]))
    fit = marks.fit_table(annotated, found)
    marks.save_table(tmp / "table.json", fit.table)
    want = mref.labels_from_peaks(found.peaks, found.count, annotated.lengths, fit.table)
    return dict(tmp=tmp, annotated=annotated, found=found, table=fit.table, want=want)


def _auto_cfg(b, tmp_path, repeat=1, **solver):
    names = [n + ".json" for n in rr.NAMES]
    (tmp_path / "list.txt").write_text("\n".join(names * repeat) + "\n")
    cfg = rr.make_cfg(tmp_path / "list.txt", scheme=(3, "IIv2v5_v4I_372", "input_fix"), data_root=b["tmp"] / "npy", label_root=b["tmp"] / "none")
    cfg.DATA.device_resident, cfg.DATA.auto_marks, cfg.DATA.mark_table = True, True, str(b["tmp"] / "table.json")
    cfg.SOLVER.update(solver)
    cfg.output_dir, cfg.desc = str(tmp_path), "auto"
    return cfg


def test_bundled_envelope_on_the_device_is_exact_integer_arithmetic(bundled):
    st = bundled["annotated"]
    env = torch.empty(10000, dtype=torch.float64, device=DEV)
    table = torch.tensor([[0, 5000, 0], [40000, 5000, 5000]], dtype=torch.int64)
    ops.mark_envelope(st.signal, table, env)
    want = np.concatenate([mref.envelope(sig) for _, sig, _ in rr.recordings()])
    assert torch.equal(env.cpu(), torch.from_numpy(want))
    few = ops.mark_peaks(env, table, max_peaks=4)
    assert few[1].tolist() == [19, 16] and few[0].tolist() == bundled["found"].peaks[:, :4].tolist()


def test_build_loaders_with_auto_marks_yields_the_batches_of_the_auto_labels(bundled, tmp_path):
    from test_resident_gpu import same_bits
    cfg = _auto_cfg(bundled, tmp_path, repeat=3)
    assert not os.path.exists(bundled["tmp"] / "none")
    train, test = train_net.build_loaders(cfg, batch_size=2)
    assert isinstance(train, resident.ResidentLoader) and len(train) == len(test) == 3
    for ld in (train, test):
        store = ld.store
        assert store.auto_report == dict(recordings=6, marked=6, skipped=[], peaks=105, dropped=6, adjusted=0)
        for i in range(6):                               # the store's lists are the literal loop's
            for k in range(6):
                assert store.labels[k][store.label_offsets[k][i]:store.label_offsets[k][i + 1]].tolist() == bundled["want"][0][k][i % 2]
        assert store.n_p_on.tolist() == [17, 16] * 3
        n = 0
        for (_, idx, plan), meta in zip(ld.plans(), ld):
            # a plan made by hand from the auto labels: beat_batch of its table is the batch
            rows = []
            for j, beat in zip(idx, plan.beats.tolist()):
                lab = bundled["want"][0]
                p_on, end = lab[0][j % 2][beat], lab[0][j % 2][beat + 1]
                rows.append([int(store.offsets[j]) + p_on, 5000, end - p_on] + plan.table[len(rows), 3:].tolist())
                assert meta["rois"][len(rows) - 1, :, 0].tolist() == [lab[k][j % 2][beat] - p_on for k in range(6)] + [end - p_on]
            data, target, rest = ops.beat_batch(store.signal, torch.tensor(rows, dtype=torch.int64), plan.V, plan.R)
            assert torch.equal(meta["data"], data) and torch.equal(meta["target_view"], target) and torch.equal(meta["rest_view"], rest)
            want = rr.plan_items(store, plan)
            assert same_bits(meta["data"].cpu().numpy(), want["data"]) and np.array_equal(meta["rois"].cpu().numpy(), want["rois"])
            n += 1
        assert n == 3


def test_key_off_the_store_is_the_annotated_one_field_for_field(bundled, tmp_path):
    st = bundled["annotated"]
    recs = rr.recordings()
    assert st.auto_report is None and st.names == [n for n, _, _ in recs] and st.lengths.tolist() == [5000, 5000]
    assert st.offsets.tolist() == [0, 40000, 80000] and st.signal.dtype == torch.int16
    assert torch.equal(st.signal.cpu(), torch.from_numpy(np.concatenate([s.reshape(-1) for _, s, _ in recs])))
    for k, key in enumerate(rr.KEYS):
        assert st.labels[k].tolist() == recs[0][2][key] + recs[1][2][key] and st.label_offsets[k].tolist() == [0, 17, 32]
    assert st.n_p_on.tolist() == [17, 15]
    # a recording without labels: an error naming it, or dropped and counted with DATA.auto_marks_skip
    os.makedirs(tmp_path / "npy")
    np.save(tmp_path / "npy" / "flat.npy", np.zeros((8, 700), dtype=np.int16))
    np.save(tmp_path / "npy" / "11315.npy", recs[0][1])
    (tmp_path / "list.txt").write_text("flat.json\n11315.json\n")
    cfg = rr.make_cfg(tmp_path / "list.txt", data_root=tmp_path / "npy", label_root=tmp_path / "none")
    with pytest.raises(ValueError, match="recording flat.json"):
        resident.ResidentTianchi(cfg, "train", DEV, marks=bundled["table"])
    cfg.DATA.auto_marks_skip = True
    with pytest.warns(UserWarning, match="1 of 2 recordings"):
        got = resident.ResidentTianchi(cfg, "train", DEV, marks=(bundled["table"], marks.MarkParams()))
    assert got.names == ["11315.json"] and got.auto_report["skipped"] == ["flat.json"] and got.auto_report["marked"] == 1
    assert got.lengths.tolist() == [5000] and got.offsets.tolist() == [0, 40000] and torch.equal(got.signal, st.signal[:40000])
    assert [got.labels[k].tolist() for k in range(6)] == [bundled["want"][0][k][0] for k in range(6)] and got.n_p_on.tolist() == [17]


def test_round_trip_of_whole_recordings_on_the_auto_marked_store(bundled, tmp_path):
    """beat_batch on all 12 leads, beat_range, beat_stitch over the auto-marked store: every covered element within (span + |s|) * 2^-24 of
    the stored signal -- the bound tests/test_recording_cpu.py derives for the annotated one; then recording.synthesize runs on it."""
    import recording_ref as ref
    from electrocardio_panorama_amd import recording
    store = resident.ResidentTianchi(_auto_cfg(bundled, tmp_path), "test", DEV)
    rp = resident.recording_plan(store, [0, 1], list(range(12)))
    assert rp.rec.size == 16 + 15 and int(rp.stitch[:, 2].max()) <= 512
    table = torch.from_numpy(rp.plan.table).to(DEV)
    views = ops.beat_batch(store.signal, table, 12, 0)[0]
    rng = ops.beat_range(store.signal, table, 12, 0)
    out = torch.full((int(rp.out_offsets[-1]),), float("nan"), dtype=torch.float32, device=DEV)
    ops.beat_stitch(views, rng, torch.from_numpy(rp.stitch), out, "nan")
    got_all, rng = out.cpu().numpy(), rng.cpu().numpy()
    worst = 0.0
    for j in range(2):
        s12 = ref.twelve(rr.recordings()[j][1].astype(np.float64))
        got = got_all[rp.out_offsets[j]:rp.out_offsets[j + 1]].reshape(12, -1)
        p = store.labels[0][store.label_offsets[0][j]:store.label_offsets[0][j + 1]]
        covered = np.zeros(5000, dtype=bool)
        covered[p[0]:p[-1]] = True
        assert np.isnan(got[:, ~covered]).all() and np.isfinite(got[:, covered]).all() and covered.sum() > 4000
        for b in np.nonzero(rp.rec == j)[0]:
            q, n = int(rp.stitch[b, 0] - rp.out_offsets[j]), int(rp.stitch[b, 2])
            span = rng[b, 1] - rng[b, 0]
            err = np.abs(got[:, q:q + n].astype(np.float64) - s12[:, q:q + n])
            bound = (span + np.abs(s12[:, q:q + n])) * 2.0 ** -24
            assert (err <= bound).all()
            worst = max(worst, float((err / bound).max()))
    print("worst ratio to the bound", worst)
    import test_model_gpu as tm
    syn = recording.synthesize(tm.hashed_model(3).eval(), store, range(2), [1, 3, 6])
    assert [tuple(s.shape) for s in syn.signals] == [(12, 5000), (12, 5000)] and np.isfinite(syn.rmse).all() and np.isfinite(syn.corr).all()


def test_train_gen_net_and_mark_net_on_signals_alone(bundled, tmp_path, capsys, monkeypatch):
    """Two epochs of Solver.train on the auto-marked loaders; gen_net --auto-marks on the checkpoint with the key off in its config;
    mark_net --write, whose files the unchanged host dataset loads; mark_net --fit / --compare on the annotated listing."""
    from electrocardio_panorama_amd import gen_net, mark_net
    from electrocardio_panorama_amd.dataset.tianchi import EcgTianChiInterval
    from electrocardio_panorama_amd.prefetch import DevicePrefetcher
    from electrocardio_panorama_amd.solver import Solver
    cfg = _auto_cfg(bundled, tmp_path, repeat=1, epochs=2)
    run_cfg = cfg.clone()
    run_cfg.DATA.auto_marks, run_cfg.DATA.mark_table = False, ""
    cfg.output_dir = os.path.join(str(tmp_path), "auto")
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    random.seed(100)
    capsys.readouterr()
    sol.train(DevicePrefetcher(train, sol.device), DevicePrefetcher(test, sol.device))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 2 and all(np.isfinite(float(ln.split("train_loss: ")[1].split(",")[0])) for ln in lines)
    assert os.path.exists(os.path.join(str(tmp_path), "auto", "auto", "epoch_1.pkl"))
    monkeypatch.setattr(gen_net, "cfg", run_cfg)
    result = gen_net.run(["--epoch", "1", "--auto-marks", str(bundled["tmp"] / "table.json")])
    out = capsys.readouterr().out
    assert "auto marks: 2 of 2 recordings marked" in out and all(np.isfinite(v) for v in result.values()) and len(result) == 4
    # label files for the host loader
    monkeypatch.setattr(mark_net, "cfg", run_cfg)
    report = mark_net.run(["--write", str(tmp_path / "labels"), str(bundled["tmp"] / "table.json"), "--phase", "train"])
    assert report["marked"] == 2 and sorted(os.listdir(tmp_path / "labels")) == ["11315.json", "40723.json"]
    host_cfg = run_cfg.clone()
    host_cfg.DATA.train_label_root = str(tmp_path / "labels")
    ds = EcgTianChiInterval(host_cfg, "train")
    for i, name in enumerate(ds.dataset):
        doc = json.loads((tmp_path / "labels" / name).read_text())
        assert list(doc) == list(rr.KEYS) and [doc[k] for k in rr.KEYS] == [bundled["want"][0][k][i] for k in range(6)]
        random.seed(i)
        np.random.seed(i)
        item = ds[i]
        assert item["data"].shape == (3, 512) and np.isfinite(item["data"]).all() and item["rois"].shape == (7, 2)
    host = resident.ResidentTianchi(host_cfg, "train")              # ... and the annotated store path reads them as any label files
    assert host.n_p_on.tolist() == [17, 16] and host.auto_report is None
    # fit and compare on the annotated listing
    ann = rr.make_cfg(rr.write_listing(tmp_path))
    monkeypatch.setattr(mark_net, "cfg", ann)
    fit = mark_net.run(["--fit", str(tmp_path / "fit.json"), "--form", "ratio"])
    assert np.array_equal(fit.table, bundled["table"]) and np.array_equal(marks.load_table(tmp_path / "fit.json")[0], bundled["table"])
    rows = mark_net.run(["--compare", str(tmp_path / "fit.json")])
    assert rows["share"] == 1.0 and [rows[k]["max"] for k in rr.KEYS] == [4, 6, 2, 3, 9, 11]
    assert "matched 32 of 32" in capsys.readouterr().out
