"""nef_sliding_median on the device against the restatement of tests/median_ref.py with exact comparisons on whole buffers (the gaps
between the rows included; NaN positions as masks), and cfg.DATA.baseline_ms / cfg.DATA.mains_hz end to end on the two bundled recordings
with a wander and a hum added: the store, the labels, the loaders, the auto marks, one Solver.train epoch, recording.synthesize, gen_net
and mark_net --clean."""
import os
import random

import numpy as np
import pytest
import torch

import marks_ref as mref
import median_ref as mr
import resident_ref as rr
from electrocardio_panorama_amd import clean, ops, train_net
from electrocardio_panorama_amd.dataset import marks, resident

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = -7.25
HS = (0, 1, 3, 50, 150, 512)


def same(got, want):
    """Equal values on whole buffers (-0.0 is +0.0), a NaN exactly where the restatement has one."""
    got, want = got.cpu(), torch.from_numpy(want) if isinstance(want, np.ndarray) else want.cpu()
    nan = torch.isnan(want)
    if not bool(nan.any()):
        return torch.equal(got, want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))


def _data(rng, dtype, shape):
    if dtype == "int16":
        return rng.integers(-300, 300, shape).astype(np.int16)          # a narrow range: many ties
    return (rng.standard_normal(shape) * 400.0).astype(np.float32)


class Case:
    """Signals packed into one source buffer -- row i starts at an element index that is i mod 8, behind a gap -- their table, and the
    restatement's whole output buffer, the sentinel wherever no row lies.  `sigs`: ready [rows, len] arrays, or None for random ones of
    `lengths`, 8 signals in every fourth row and 1 elsewhere."""

    def __init__(self, h, dtype, lengths=None, sigs=None, seed=0, minuend=None):
        rng = np.random.default_rng([seed, h])
        if sigs is None:
            sigs = [_data(rng, dtype, (8 if i % 4 == 1 else 1, n)) for i, n in enumerate(lengths)]
        self.h, self.sigs, table, parts, pos = h, sigs, [], [], 0
        for i, sig in enumerate(sigs):
            pad = (i - pos) % 8 + 8 * (i % 3 == 2)
            parts.append(_data(rng, dtype, pad))
            pos += pad
            parts.append(sig.reshape(-1))
            table.append([pos, sig.shape[1], sig.shape[0]])
            pos += sig.size
        parts.append(_data(rng, dtype, 5))
        self.table = np.array(table, dtype=np.int64)
        assert sorted(set((self.table[:, 0] % 8).tolist())) == list(range(min(8, len(sigs))))
        flat = np.concatenate(parts)
        self.elems = flat.size
        self.src = torch.from_numpy(flat).to(DEV)
        self.minuend = None
        if minuend is not None:
            self.minuend_host = _data(np.random.default_rng([seed, h, 1]), minuend, flat.size)
            self.minuend = torch.from_numpy(self.minuend_host).to(DEV)
        self.want = np.full(self.elems, SENTINEL, dtype=np.float32)
        for (off, n, rows), sig in zip(self.table.tolist(), sigs):
            m = mr.sliding_median(sig, h).reshape(-1)
            self.want[off:off + m.size] = m if minuend is None else mr.subtract(self.minuend_host[off:off + m.size], m)

    def run(self, rows=None, table=None, dst=None, **kw):
        dst = torch.full((self.elems,), SENTINEL, dtype=torch.float32, device=DEV) if dst is None else dst
        table = torch.from_numpy(np.ascontiguousarray(self.table if rows is None else self.table[rows])) if table is None else table
        return ops.sliding_median(self.src, table, dst, self.h, minuend=self.minuend, **kw)


def _lengths(h):
    return sorted({n for n in (1, 2, h, h + 1, 2 * h, 2 * h + 1, 2 * h + 2, 1023, 1024, 1025, 2100) if n >= 1}) + [5000]


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("h", HS)
def test_sliding_median_is_the_restatement(h, dtype):
    """Row lengths 1, 2, h, h + 1, 2 h, 2 h + 1, 2 h + 2, 1023 .. 1025, 2100 and 5000; every offset residue mod 8; 1 and 8 signals a row;
    the gaps keep their bits."""
    c = Case(h, dtype, _lengths(h))
    got = c.run()
    assert same(got, c.want)
    n_rows = c.table.shape[0]
    # a row alone against the same row among the others
    for i in (1, n_rows - 4, n_rows - 1):
        off, n, rows = c.table[i].tolist()
        alone = c.run(rows=[i])
        assert torch.equal(alone[off:off + rows * n], got[off:off + rows * n])
        assert bool((alone[:off] == SENTINEL).all()) and bool((alone[off + rows * n:] == SENTINEL).all())
    # two chunks against one
    dst = c.run(rows=slice(0, 4))
    assert torch.equal(c.run(rows=slice(4, None), dst=dst), got)
    # a device table with the launch's extents given
    dev_table = torch.from_numpy(c.table).to(DEV)
    assert torch.equal(c.run(table=dev_table, max_len=5000, max_rows=8), got)
    assert torch.equal(c.run(table=dev_table, max_len=9000, max_rows=20), got)


@pytest.mark.parametrize("h", [3, 50, 150])
def test_ties_zeros_and_infinities(h):
    """A row of all-equal values, a staircase whose steps are longer than the window and cross the 1024-output seam, +-0.0 mixed (compared
    by value), +-inf among numbers and in runs longer than half a window."""
    rng = np.random.default_rng(h)
    const = np.full((1, 2500), np.float32(-3.5))
    stairs = (np.arange(3000) // 400).astype(np.float32)[None, :] * np.float32(2.5)
    zeros = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), (8, 1500))
    infs = (rng.standard_normal((1, 2300)) * 10).astype(np.float32)
    infs[0, rng.integers(0, 2300, 300)] = np.inf
    infs[0, rng.integers(0, 2300, 300)] = -np.inf
    infs[0, 1000:1000 + h + 5] = np.inf
    infs[0, 1600:1600 + h + 5] = -np.inf
    c = Case(h, "float32", sigs=[const, stairs, zeros, infs])
    got = c.run()
    assert same(got, c.want)
    off, n, _ = c.table[0].tolist()
    assert bool((got[off:off + n] == -3.5).all())
    off, n, _ = c.table[3].tolist()
    assert bool(torch.isinf(got[off:off + n]).any()) and not bool(torch.isnan(got).any())
    ci = Case(h, "int16", sigs=[np.full((8, 1100), -32768, dtype=np.int16), (np.arange(2200) // 300).astype(np.int16)[None, :]])
    assert same(ci.run(), ci.want)


def test_a_planted_nan_reaches_exactly_the_outputs_within_h():
    for h, at in ((0, 700), (1, 0), (50, 1030), (150, 1023), (512, 2999)):
        sig = (np.random.default_rng(h).standard_normal((3, 3000)) * 100).astype(np.float32)
        sig[1, at] = np.nan
        c = Case(h, "float32", sigs=[sig[:1, :40].copy(), sig])
        got = c.run()
        assert same(got, c.want)
        off, n, rows = c.table[1].tolist()
        hit = torch.isnan(got[off:off + rows * n]).cpu().numpy().reshape(rows, n)
        # edge replication: a NaN in the first or the last sample is in every window that reaches over that end
        want = np.abs(np.arange(n) - at) <= h
        assert np.array_equal(hit[1], want) and not hit[[0, 2]].any() and int(torch.isnan(got).sum()) == int(want.sum())


@pytest.mark.parametrize("minuend", ["int16", "float32"])
def test_minuend_form_and_dst_is_minuend(minuend):
    for h, dtype in ((0, "int16"), (50, "float32"), (150, "int16")):
        c = Case(h, dtype, [1, 300, 1025, 2100, 17], minuend=minuend)
        got = c.run()
        assert same(got, c.want)
        if minuend == "float32":
            # in place: the rows become the differences, the gaps keep the minuend's bits
            want = c.minuend_host.copy()
            for off, n, rows in c.table.tolist():
                want[off:off + rows * n] = c.want[off:off + rows * n]
            buf = c.minuend.clone()
            c.minuend = buf
            assert c.run(dst=buf) is buf and same(buf, want)
    # h = 0 with the source as the minuend: zeros
    x = torch.from_numpy(_data(np.random.default_rng(2), minuend, 4000)).to(DEV)
    out = ops.sliding_median(x, torch.tensor([[0, 500, 8]]), torch.full((4000,), SENTINEL, device=DEV), 0, minuend=x)
    assert bool((out == 0).all())


def test_rows_that_leave_a_buffer_write_nothing_and_bad_arguments_raise():
    c = Case(50, "int16", [40, 300, 50])
    good = c.run()
    assert same(good, c.want)
    t, E = c.table.copy(), c.elems
    for bad in ([E - 100, 300, 1], [-1, 300, 1], [t[1, 0], 0, 8], [t[1, 0], -5, 8], [t[1, 0], 300, 0], [t[1, 0], 300, 9], [t[1, 0], 300, -1],
                [t[1, 0], 1 << 40, 8], [1 << 60, 300, 8], [t[1, 0], 300, 1 << 40]):
        tab = t.copy()
        tab[1] = bad
        got = c.run(table=torch.from_numpy(tab).to(DEV), max_len=300, max_rows=8)
        want = c.want.copy()
        o, size = int(t[1, 0]), 8 * 300
        want[o:o + size] = SENTINEL
        assert same(got, want), bad
        with pytest.raises(ValueError, match="table row 1"):
            c.run(table=torch.from_numpy(tab))
    # the launch covers max_len outputs and max_rows signals: a row above either writes nothing; a shorter dst or minuend bounds the rows too
    dev_table = torch.from_numpy(t).to(DEV)
    want = c.want.copy()
    o, size = int(t[1, 0]), 8 * 300
    want[o:o + size] = SENTINEL
    assert same(c.run(table=dev_table, max_len=299, max_rows=8), want)
    assert same(c.run(table=dev_table, max_len=300, max_rows=7), want)
    short = int(t[2, 0]) + 10
    got = c.run(table=dev_table, max_len=300, max_rows=8, dst=torch.full((short,), SENTINEL, dtype=torch.float32, device=DEV))
    assert same(got, np.concatenate([c.want[:int(t[2, 0])], np.full(10, SENTINEL, dtype=np.float32)]))
    c.minuend = torch.zeros(short, dtype=torch.int16, device=DEV)
    want = np.full(E, SENTINEL, dtype=np.float32)                           # 0 - m in rows 0 and 1, nothing in row 2
    for off, n, rows in t[:2].tolist():
        want[off:off + rows * n] = -c.want[off:off + rows * n]
    assert same(c.run(table=dev_table, max_len=300, max_rows=8), want)
    with pytest.raises(ValueError, match="table row 2"):
        c.run()
    c.minuend = None
    with pytest.raises(ValueError, match="max_len and max_rows"):
        c.run(table=dev_table)
    with pytest.raises(ValueError, match="max_len and max_rows"):
        c.run(table=dev_table, max_len=300)
    with pytest.raises(ValueError, match="table row 1"):
        c.run(max_len=100)
    with pytest.raises(ValueError, match="table row 1"):
        c.run(max_rows=7)
    host = torch.from_numpy(t)
    dst = torch.full((E,), SENTINEL, dtype=torch.float32, device=DEV)
    fsrc = torch.zeros(E, dtype=torch.float32, device=DEV)
    for kw, exc, words in ((dict(h=-1), ValueError, "h ="), (dict(h=513), ValueError, "h ="), (dict(h=1.0), ValueError, "h ="),
                           (dict(dst=dst.double()), TypeError, "float32"), (dict(dst=dst.cpu()), ValueError, "dst is on"),
                           (dict(table=host.int()), TypeError, "int64"), (dict(table=host[:, :2].contiguous()), ValueError, "contiguous"),
                           (dict(src=c.src.cpu()), RuntimeError, "HIP device"), (dict(src=fsrc, dst=fsrc), ValueError, "overlaps src"),
                           (dict(src=fsrc, dst=fsrc[8:]), ValueError, "overlaps src"), (dict(src=fsrc[16:], dst=fsrc[:24]), ValueError, "overlaps src"),
                           (dict(minuend=dst.double()), TypeError, "minuend"), (dict(minuend=dst.cpu()), ValueError, "minuend is on"),
                           (dict(minuend=dst[4:]), ValueError, "overlaps minuend"), (dict(minuend=dst.view(-1, 1)), ValueError, "1-D")):
        args = dict(src=c.src, table=host, dst=dst, h=50)
        args.update(kw)
        with pytest.raises(exc, match=words):
            ops.sliding_median(**args)
    assert bool((dst == SENTINEL).all())
    # adjoining buffers do not overlap
    ops.sliding_median(fsrc[:16], torch.tensor([[0, 16, 1]]), fsrc[16:32], 3)


def test_capturable_with_a_device_table():
    c = Case(50, "int16", [1500, 700])
    table = torch.from_numpy(c.table).to(DEV)
    dst = torch.full((c.elems,), SENTINEL, dtype=torch.float32, device=DEV)
    c.run(table=table, dst=dst, max_len=1500, max_rows=8)                   # the library is loaded and warm
    dst.fill_(SENTINEL)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.run(table=table, dst=dst, max_len=1500, max_rows=8)
    dst.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert same(dst, c.want)


# ------------------------------------------------------------------------------------------------ the keys, end to end
SCHEME = (3, "IIv2v5_v4I_372", "input_fix")
T = np.arange(5000, dtype=np.float64)
ADDEND = 200 * np.sin(2 * np.pi * 0.3 * T / 500 + 0.7) + 40 * np.sin(2 * np.pi * 50 * T / 500 + 0.3)


def _cfg(tmp, listing, on=True, **data):
    cfg = rr.make_cfg(listing, scheme=SCHEME, data_root=tmp / "npy", label_root=tmp / "json")
    cfg.DATA.device_resident = True
    if on:
        cfg.DATA.baseline_ms, cfg.DATA.mains_hz = [200, 600], 50.0
    cfg.DATA.update(data)
    return cfg


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The two bundled recordings with the wander and the hum added, as a .npy + .json tree; the restatement's notched and cleaned signals;
    the timing table fitted on the clean recordings."""
    tmp = tmp_path_factory.mktemp("clean")
    recs = rr.recordings()
    bad = [np.rint(s.astype(np.float64) + ADDEND).astype(np.int16) for _, s, _ in recs]
    listing = rr.write_tree(tmp, [(n.replace(".json", ""), b, lab) for (n, _, lab), b in zip(recs, bad)])
    notch = clean.notch_taps(500.0, 50.0)
    notched = [mr.notch_apply(b, *notch) for b in bad]
    cleaned = [mr.baseline_remove(x, 50, 150) for x in notched]
    orig = tmp / "orig"
    os.makedirs(orig)
    annotated = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(orig)), "train", DEV)
    fit = marks.fit_table(annotated, marks.detect(annotated))
    marks.save_table(tmp / "table.json", fit.table)
    return dict(tmp=tmp, listing=listing, recs=recs, bad=bad, notched=notched, cleaned=cleaned, table=fit.table, notch=notch)


def test_two_stage_chain_on_the_bundled_recordings(tree):
    for (_, sig, _), bad in zip(tree["recs"], tree["bad"]):
        for x in (sig, bad, bad.astype(np.float32)):
            src = torch.from_numpy(x.reshape(-1)).to(DEV)
            table = torch.tensor([[0, 5000, 8]])
            tmp = ops.sliding_median(src, table, torch.empty(40000, device=DEV), 50)
            out = ops.sliding_median(tmp, table, torch.empty(40000, device=DEV), 150, minuend=src)
            assert same(tmp, mr.sliding_median(x, 50).reshape(-1)) and same(out, mr.baseline_remove(x, 50, 150).reshape(-1))


def _flat(sigs, repeat=1):
    return torch.from_numpy(np.concatenate([s.reshape(-1) for s in sigs] * repeat))


def _check_batches(ld):
    store, n, recs = ld.store, 0, rr.recordings()
    for (_, idx, plan), meta in zip(ld.plans(), ld):
        rows = []
        for j, beat in zip(idx, plan.beats.tolist()):        # a plan made by hand from the files' labels
            lab = [recs[j % 2][2][k] for k in rr.KEYS]
            p_on, end = lab[0][beat], lab[0][beat + 1]
            rows.append([int(store.offsets[j]) + p_on, int(store.lengths[j]), end - p_on] + plan.table[len(rows), 3:].tolist())
        data, target, rest = ops.beat_batch(store.signal, torch.tensor(rows, dtype=torch.int64), plan.V, plan.R)
        assert torch.equal(meta["data"], data) and torch.equal(meta["target_view"], target) and torch.equal(meta["rest_view"], rest)
        n += 1
    return n


def test_store_and_loaders_with_both_keys_on(tree, tmp_path):
    names = [n + ".json" for n in rr.NAMES]
    (tmp_path / "list.txt").write_text("\n".join(names * 3) + "\n")
    cfg = _cfg(tree["tmp"], tmp_path / "list.txt")
    off = resident.ResidentTianchi(_cfg(tree["tmp"], tmp_path / "list.txt", on=False), "train", DEV)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    assert isinstance(train, resident.ResidentLoader) and len(train) == len(test) == 3
    for ld in (train, test):
        st = ld.store
        assert st.signal.dtype == torch.float32 and same(st.signal, _flat(tree["cleaned"], 3))
        assert st.clean == clean.CleanPlan(50, 150, 50.0, 6.0, 511, 8.6, 500.0)
        assert st.clean_report == dict(recordings=6, h1=50, h2=150, taps=511, launches=3)
        assert np.array_equal(st.lengths, off.lengths) and np.array_equal(st.offsets, off.offsets) and st.raw_lengths is st.lengths
        assert all(np.array_equal(a, b) for a, b in zip(st.labels, off.labels)) and np.array_equal(st.n_p_on, off.n_p_on)
        assert all(np.array_equal(a, b) for a, b in zip(st.label_offsets, off.label_offsets)) and st.names == off.names
        assert _check_batches(ld) == 3
    # each stage alone: the notch bit for bit, the baseline by value; in chunks of one recording
    only = resident.ResidentTianchi(_cfg(tree["tmp"], tmp_path / "list.txt", baseline_ms=[]), "train", DEV)
    assert torch.equal(only.signal.cpu(), _flat(tree["notched"], 3)) and only.clean_report == dict(recordings=6, h1=0, h2=0, taps=511, launches=1)
    only = resident.ResidentTianchi(_cfg(tree["tmp"], tmp_path / "list.txt", mains_hz=0.0), "train", DEV)
    assert same(only.signal, _flat([mr.baseline_remove(b, 50, 150) for b in tree["bad"]], 3))
    assert only.clean_report == dict(recordings=6, h1=50, h2=150, taps=0, launches=2)
    raw = resident.ResidentTianchi(_cfg(tree["tmp"], tmp_path / "list.txt", on=False), "train", DEV)
    raw.clean = train.store.clean
    raw._clean(budget=1)
    assert raw.clean_report["launches"] == 18 and torch.equal(raw.signal, train.store.signal)


def test_notch_row_through_resample_on_short_rows(tree):
    """The 511-tap row at 1/1 on rows of 1, 2, 510 .. 512 and 1025 samples, bit for bit."""
    taps, first = tree["notch"]
    rng = np.random.default_rng(9)
    for n in (1, 2, 510, 511, 512, 1025):
        x = rng.integers(-3000, 3000, (8, n)).astype(np.int16)
        got = ops.resample(torch.from_numpy(x.reshape(-1)).to(DEV), torch.tensor([[0, n, 0, 8]]), torch.empty(8 * n, device=DEV), taps, first, 1, 1)
        assert torch.equal(got.cpu(), torch.from_numpy(mr.notch_apply(x, taps, first).reshape(-1))), n


def test_auto_marks_run_on_the_cleaned_store(tree):
    cfg = _cfg(tree["tmp"], tree["listing"], auto_marks=True, mark_table=str(tree["tmp"] / "table.json"))
    cfg.DATA.train_label_root = str(tree["tmp"] / "none")              # no label file is opened
    train, test = train_net.build_loaders(cfg, batch_size=2)
    st = train.store
    assert same(st.signal, _flat(tree["cleaned"]))
    sigs = [st.signal[st.offsets[i]:st.offsets[i + 1]].cpu().numpy().reshape(8, -1) for i in range(2)]
    rows = [mref.peaks(mref.envelope(s)) for s in sigs]
    assert [r[1] for r in rows] == [19, 16]                              # the counts of the clean recordings; the raw tree gives 19 and 19
    want, dropped, adjusted = mref.labels_from_peaks(np.stack([r[0] for r in rows]), [r[1] for r in rows], st.lengths, tree["table"])
    for i in range(2):
        for k in range(6):
            assert st.labels[k][st.label_offsets[k][i]:st.label_offsets[k][i + 1]].tolist() == want[k][i]
    assert st.auto_report["peaks"] == 35 and st.auto_report["marked"] == 2
    raw = resident.ResidentTianchi(_cfg(tree["tmp"], tree["listing"], on=False, auto_marks=True, mark_table=str(tree["tmp"] / "table.json")), "train", DEV)
    assert raw.auto_report["peaks"] == 38 and raw.signal.dtype == torch.int16
    assert sum(1 for _ in test) == 1


def test_keys_off_is_the_store_without_the_keys(tree):
    cfg = _cfg(tree["tmp"], tree["listing"], on=False)
    bare = cfg.clone()
    for key in ("baseline_ms", "mains_hz", "mains_width_hz", "mains_taps", "mains_beta"):
        del bare.DATA[key]
    base = resident.ResidentTianchi(bare, "train", DEV)
    for over in (dict(), dict(baseline_ms=[], mains_hz=0), dict(mains_taps=7, mains_width_hz=1.0)):
        st = resident.ResidentTianchi(_cfg(tree["tmp"], tree["listing"], on=False, **over), "train", DEV)
        assert st.clean is None and st.clean_report is None and base.clean is None
        assert st.signal.dtype == torch.int16 and torch.equal(st.signal, base.signal) and st.names == base.names
        assert torch.equal(st.signal.cpu(), _flat(tree["bad"]))
        assert np.array_equal(st.lengths, base.lengths) and np.array_equal(st.offsets, base.offsets) and np.array_equal(st.n_p_on, base.n_p_on)
        assert all(np.array_equal(a, b) for a, b in zip(st.labels, base.labels))
        assert all(np.array_equal(a, b) for a, b in zip(st.label_offsets, base.label_offsets))


def test_synthesize_and_source_rate_go_with_the_cleaning(tree):
    import test_model_gpu as tm
    from electrocardio_panorama_amd import recording
    store = resident.ResidentTianchi(_cfg(tree["tmp"], tree["listing"]), "test", DEV)
    model = tm.hashed_model(3).eval()
    syn = recording.synthesize(model, store, range(2), [1, 3, 6])
    assert len(syn.signals) == 2 and tuple(syn.signals[0].shape) == (12, 5000) and syn.rmse.shape == (2, 12)
    # the files declared as 1000 Hz: resampled to 2500 samples, then cleaned at 500 Hz
    st = resident.ResidentTianchi(_cfg(tree["tmp"], tree["listing"], source_rate=1000), "train", DEV)
    assert st.lengths.tolist() == [2500, 2500] and st.raw_lengths.tolist() == [5000, 5000] and st.signal.dtype == torch.float32
    assert st.resample_report["launches"] == 1 and st.clean_report == dict(recordings=2, h1=50, h2=150, taps=511, launches=3)
    import resample_ref as rref
    from electrocardio_panorama_amd import resample
    taps, first = resample.design(1, 2)
    want = [mr.baseline_remove(mr.notch_apply(rref.resample(b, taps, first, 1, 2), *tree["notch"]), 50, 150) for b in tree["bad"]]
    assert same(st.signal, _flat(want))
    assert sum(1 for _ in resident.ResidentLoader(st, st.cfg, "test", 2)) == 1


def test_train_gen_net_and_mark_net_on_a_cleaned_store(tree, tmp_path, capsys, monkeypatch):
    """One epoch of Solver.train with a checkpoint; gen_net on it; mark_net --clean, whose files the unchanged host dataset and the key-off
    store read."""
    from electrocardio_panorama_amd import gen_net, mark_net
    from electrocardio_panorama_amd.dataset.tianchi import EcgTianChiInterval
    from electrocardio_panorama_amd.prefetch import DevicePrefetcher
    from electrocardio_panorama_amd.solver import Solver
    cfg = _cfg(tree["tmp"], tree["listing"])
    cfg.SOLVER.epochs = 1
    cfg.output_dir, cfg.desc = str(tmp_path), "clean"
    run_cfg = cfg.clone()                                           # gen_net.run appends the description itself
    cfg.output_dir = os.path.join(str(tmp_path), "clean")
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    random.seed(100)
    capsys.readouterr()
    sol.train(DevicePrefetcher(train, sol.device), DevicePrefetcher(test, sol.device))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 1 and np.isfinite(float(lines[0].split("train_loss: ")[1].split(",")[0]))
    assert os.path.exists(os.path.join(sol.output_dir, "epoch_0.pkl"))
    monkeypatch.setattr(gen_net, "cfg", run_cfg)
    result = gen_net.run(["--epoch", "0", "--out", str(tmp_path / "strips")])
    assert len(result) == 4
    for name in rr.NAMES:
        assert np.load(tmp_path / "strips" / (name + ".npy")).shape == (12, 5000)
    run_cfg.output_dir = str(tmp_path)                               # run() appended the description to it
    # mark_net --clean: files for the host loader
    monkeypatch.setattr(mark_net, "cfg", run_cfg)
    report = mark_net.run(["--clean", str(tmp_path / "files"), "--phase", "train"])
    assert report == train.store.clean_report and "cleaned 2 recordings" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "files")) == ["11315.json", "11315.npy", "40723.json", "40723.npy"]
    host_cfg = run_cfg.clone()
    host_cfg.DATA.baseline_ms, host_cfg.DATA.mains_hz, host_cfg.DATA.device_resident = [], 0.0, False
    host_cfg.DATA.train_data_root = host_cfg.DATA.train_label_root = str(tmp_path / "files")
    ds = EcgTianChiInterval(host_cfg, "train")
    for i, name in enumerate(ds.dataset):
        sig, lab = ds._load(name)
        assert list(lab) == list(rr.KEYS) and [lab[k] for k in rr.KEYS] == [tree["recs"][i][2][k] for k in rr.KEYS]
        assert np.load(tmp_path / "files" / name.replace(".json", ".npy")).dtype == np.float32
        assert np.array_equal(sig, train.store.signal[train.store.offsets[i]:train.store.offsets[i + 1]].cpu().numpy().reshape(8, -1).astype(np.float64))
        random.seed(i)
        np.random.seed(i)
        item = ds[i]
        assert item["data"].shape == (3, 512) and np.isfinite(item["data"]).all() and item["rois"].shape == (7, 2)
    host = resident.ResidentTianchi(host_cfg, "train", DEV)        # the key-off store of those files is the cleaned store
    assert host.signal.dtype == torch.float32 and torch.equal(host.signal, train.store.signal) and host.clean is None
    with pytest.raises(ValueError, match="nothing to clean"):
        monkeypatch.setattr(mark_net, "cfg", host_cfg)
        mark_net.run(["--clean", str(tmp_path / "again")])
