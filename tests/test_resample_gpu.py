"""nef_resample on the device against the literal restatement of tests/resample_ref.py, bit for bit on whole buffers (the gaps between the
outputs included), and cfg.DATA.source_rate end to end on the two bundled recordings declared as 1000 Hz and 360 Hz files: the store, the
rescaled and the auto labels, the loaders, one Solver.train epoch, recording.synthesize at the source rate, gen_net and mark_net."""
import json
import os
import random

import numpy as np
import pytest
import torch

import marks_ref as mref
import resample_ref as ref
import resident_ref as rr
from electrocardio_panorama_amd import ops, resample, train_net
from electrocardio_panorama_amd.dataset import marks, resident

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = -7.25
# the taps in LDS: 1/2, 2/1, 25/18, 18/25, 1/1 and -- the tile worked in two halves -- 1/8; from global memory: 500/257
RATIOS = ((1, 2), (2, 1), (25, 18), (18, 25), (500, 257), (1, 1), (1, 8))
ROWS = (1, 8, 12, 13)


def same(got, want):
    """Equal floats on whole buffers, a NaN exactly where the restatement has one (torch.equal alone where it has none)."""
    got, want = got.cpu(), torch.from_numpy(want) if isinstance(want, np.ndarray) else want.cpu()
    nan = torch.isnan(want)
    if not bool(nan.any()):
        return torch.equal(got, want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))


def _len_for(out, up, down):
    """The shortest row that gives `out` outputs -- or, where up / down steps over `out` (2 / 1 gives even counts only), the next count."""
    n = max(1, (out * down) // up - down - 1)
    while ref.out_len(n, up, down) < out:
        n += 1
    assert out <= ref.out_len(n, up, down) < out + max(1, -(-up // down))
    return n


def _data(rng, dtype, shape):
    if dtype == "int16":
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return (rng.standard_normal(shape) * 400.0).astype(np.float32)


class Case:
    """Rows of signals packed into one source buffer -- row i starts at an element index that is i mod 8 -- their table, the output buffer
    with a gap of 3 + i floats in front of row i's results, and the restatement's whole output buffer."""

    def __init__(self, up, down, dtype, lengths, seed=0, taps=None, first=None, plant=None):
        self.up, self.down = up, down
        self.taps, self.first = resample.design(up, down) if taps is None else (taps, first)
        rng = np.random.default_rng([seed, up, down])
        self.sigs, table, src_parts, pos, opos = [], [], [], 0, 0
        for i, n in enumerate(lengths):
            rows = ROWS[i % 4]
            pad = (i - pos) % 8
            src_parts.append(_data(rng, dtype, pad))
            pos += pad
            sig = _data(rng, dtype, (rows, n))
            if plant is not None and plant[0] == i:
                sig[plant[1], plant[2]] = np.nan
            self.sigs.append(sig)
            src_parts.append(sig.reshape(-1))
            opos += 3 + i
            table.append([pos, n, opos, rows])
            pos += rows * n
            opos += rows * ref.out_len(n, up, down)
        self.table = np.array(table, dtype=np.int64)
        assert sorted(set((self.table[:, 0] % 8).tolist())) == list(range(min(8, len(lengths))))
        self.src = torch.from_numpy(np.concatenate(src_parts)).to(DEV)
        self.dst_elems = opos + 5
        self.want = np.full(self.dst_elems, SENTINEL, dtype=np.float32)
        for (off, n, ooff, rows), sig in zip(self.table.tolist(), self.sigs):
            y = ref.resample(sig, self.taps, self.first, up, down)
            self.want[ooff:ooff + y.size] = y.reshape(-1)

    def run(self, rows=None, table=None, dst=None, **kw):
        dst = torch.full((self.dst_elems,), SENTINEL, dtype=torch.float32, device=DEV) if dst is None else dst
        table = torch.from_numpy(np.ascontiguousarray(self.table if rows is None else self.table[rows])) if table is None else table
        return ops.resample(self.src, table, dst, self.taps, self.first, self.up, self.down, **kw)


def _lengths(up, down, long=20000):
    K = resample.taps_per_phase(up, down)
    return [1, 2, K - 1, K, K + 1, _len_for(1023, up, down), _len_for(1024, up, down), _len_for(1025, up, down), long]


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_is_the_restatement_bit_for_bit(up, down, dtype):
    """Row lengths 1, 2, K - 1, K, K + 1, those whose out_len is 1023, 1024 and 1025 and one of 20 000; every in_offset residue mod 8; 1, 8,
    12 and 13 signals a row; the gaps in dst keep their bits."""
    c = Case(up, down, dtype, _lengths(up, down))
    assert (c.taps.size <= 4096) == ((up, down) != (500, 257))
    got = c.run()
    assert same(got, c.want)
    # a row alone against the same row among the others
    for i in (3, 7, 8):
        off, n, ooff, rows = c.table[i].tolist()
        alone = c.run(rows=[i])
        size = rows * ref.out_len(n, up, down)
        assert torch.equal(alone[ooff:ooff + size], got[ooff:ooff + size])
        assert bool((alone[:ooff] == SENTINEL).all()) and bool((alone[ooff + size:] == SENTINEL).all())
    # two chunks against one
    dst = c.run(rows=slice(0, 4))
    assert torch.equal(c.run(rows=slice(4, None), dst=dst), got)
    # a device table with the launch's extents given
    n_max = int(max(ref.out_len(n, up, down) for n in c.table[:, 1]))
    dev_table = torch.from_numpy(c.table).to(DEV)
    assert torch.equal(c.run(table=dev_table, max_out_len=n_max, max_rows=13), got)
    assert torch.equal(c.run(table=dev_table, max_out_len=n_max + 5000, max_rows=20), got)


def test_rows_that_leave_a_buffer_write_nothing_and_bad_arguments_raise():
    c = Case(25, 18, "int16", [40, 300, 50])
    good = c.run()
    assert same(good, c.want)
    src_n, dst_n = c.src.numel(), c.dst_elems
    t = c.table.copy()
    # row 1 is replaced in turn by rows that leave src or dst, are empty, hold no or too many signals, or are longer than the launch covers
    for bad in ([src_n - 100, 300, t[1, 2], 8], [-1, 300, t[1, 2], 8], [t[1, 0], 300, dst_n - 100, 8], [t[1, 0], 300, -1, 8],
                [t[1, 0], 0, t[1, 2], 8], [t[1, 0], -5, t[1, 2], 8], [t[1, 0], 300, t[1, 2], 0], [t[1, 0], 300, t[1, 2], 14],
                [t[1, 0], 1 << 40, t[1, 2], 8], [1 << 60, 300, t[1, 2], 8], [t[1, 0], 300, 1 << 60, 8]):
        tab = t.copy()
        tab[1] = bad
        got = c.run(table=torch.from_numpy(tab).to(DEV), max_out_len=ref.out_len(300, 25, 18), max_rows=13)
        want = c.want.copy()
        o, size = int(t[1, 2]), 8 * ref.out_len(300, 25, 18)
        want[o:o + size] = SENTINEL
        assert same(got, want), bad
        with pytest.raises(ValueError, match="table row 1"):
            c.run(table=torch.from_numpy(tab))
    # the launch covers max_out_len outputs and max_rows signals: a row above either writes nothing
    dev_table = torch.from_numpy(t).to(DEV)
    want = c.want.copy()
    o, size = int(t[1, 2]), 8 * ref.out_len(300, 25, 18)
    want[o:o + size] = SENTINEL
    assert same(c.run(table=dev_table, max_out_len=ref.out_len(300, 25, 18) - 1, max_rows=13), want)
    with pytest.raises(ValueError, match="max_out_len"):
        c.run(table=dev_table)
    with pytest.raises(ValueError, match="table row 1"):
        c.run(max_out_len=100)
    host = torch.from_numpy(t)
    dst = torch.full((dst_n,), SENTINEL, dtype=torch.float32, device=DEV)
    for kw, exc, words in ((dict(up=0), ValueError, "up"), (dict(up=1025), ValueError, "up"), (dict(down=18 * 25), ValueError, "above 8 x up"),
                           (dict(taps=c.taps[:, :0]), ValueError, "taps"), (dict(taps=c.taps.astype(np.float32)), ValueError, "taps"),
                           (dict(taps=c.taps[:24]), ValueError, "taps"), (dict(first=c.first.astype(np.int64)), ValueError, "first"),
                           (dict(first=c.first[:24]), ValueError, "first"), (dict(dst=dst.double()), TypeError, "float32"),
                           (dict(dst=dst.cpu()), ValueError, "dst is on"), (dict(table=host.int()), TypeError, "int64"),
                           (dict(table=host[:, :3].contiguous()), ValueError, "contiguous"), (dict(src=c.src.cpu()), RuntimeError, "HIP device")):
        args = dict(src=c.src, table=host, dst=dst, taps=c.taps, first=c.first, up=25, down=18)
        args.update(kw)
        with pytest.raises(exc, match=words):
            ops.resample(**args)
    assert bool((dst == SENTINEL).all())


def test_a_planted_nan_reaches_exactly_the_outputs_the_formula_says():
    for up, down in ((25, 18), (1, 2), (500, 257)):
        K = resample.taps_per_phase(up, down)
        c = Case(up, down, "float32", [3000, 10, 2500], plant=(2, 5, 1500))
        got = c.run()
        assert same(got, c.want)
        off, n, ooff, rows = c.table[2].tolist()
        L = ref.out_len(n, up, down)
        hit = np.isnan(c.want[ooff:ooff + rows * L].reshape(rows, L))
        # the outputs whose K-sample window holds input 1500 of signal 5 -- zero-padded taps included -- and nothing else
        m = np.arange(L)
        start = (m * down) // up + c.first.astype(np.int64)[(m * down) % up]
        assert np.array_equal(hit[5], (start <= 1500) & (1500 < start + K)) and not hit[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]].any()
        assert 1 <= hit[5].sum() <= (K * up) // down + 1 and int(np.isnan(c.want).sum()) == int(hit.sum())
    # a NaN in the first sample is replicated over the left edge
    c = Case(2, 1, "float32", [100], plant=(0, 0, 0))
    assert same(c.run(), c.want) and np.isnan(c.want[3:3 + 16]).all()


def test_constant_rows_and_pass_through_positions_are_exact():
    for up, down, value, dtype in ((25, 18, -32768, np.int16), (18, 25, np.float32(0.1), np.float32)):
        taps, first = resample.design(up, down)
        src = torch.from_numpy(np.full(2 * 3000, value, dtype=dtype)).to(DEV)
        L = ref.out_len(3000, up, down)
        dst = ops.resample(src, torch.tensor([[0, 3000, 0, 2]]), torch.empty(2 * L, device=DEV), taps, first, up, down)
        assert torch.equal(dst.cpu(), torch.full((2 * L,), float(np.float32(value)), dtype=torch.float32))
    rng = np.random.default_rng(3)
    for up in (1, 2, 5):
        taps, first = resample.design(up, 1)
        for x in (rng.integers(-32768, 32768, 1500).astype(np.int16), (rng.standard_normal(1500) * 300).astype(np.float32)):
            dst = ops.resample(torch.from_numpy(x).to(DEV), torch.tensor([[0, 1500, 0, 1]]), torch.empty(1500 * up, device=DEV), taps, first, up, 1)
            assert torch.equal(dst.cpu()[::up], torch.from_numpy(x.astype(np.float32)))
            assert torch.equal(dst.cpu(), torch.from_numpy(ref.resample(x, taps, first, up, 1)))


def test_a_first_table_no_design_gives_is_still_the_formula():
    """The kernel places its staged stretch by the smallest entry of `first`; an output whose window lies elsewhere takes its samples from
    global memory, clamped.  Any table gives the restatement's sums."""
    taps, first = resample.design(25, 18)
    for f in (first + np.arange(25, dtype=np.int32) * 7, np.where(np.arange(25) % 3 == 0, -100000, first).astype(np.int32),
              np.full(25, 2 ** 31 - 1, dtype=np.int32), np.full(25, -2 ** 31, dtype=np.int32)):
        c = Case(25, 18, "int16", [700, 3, 1200], taps=taps, first=np.ascontiguousarray(f))
        assert same(c.run(), c.want)


# ------------------------------------------------------------------------------------------------ DATA.source_rate, end to end
SCHEME = (3, "IIv2v5_v4I_372", "input_fix")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The two bundled recordings as a .npy + .json tree, the timing table fitted on them at 500 Hz, and per declared rate the restatement's
    resampled signals and rescaled labels."""
    tmp = tmp_path_factory.mktemp("rates")
    recs = rr.recordings()
    listing = rr.write_tree(tmp, [(n.replace(".json", ""), s, lab) for n, s, lab in recs])
    annotated = resident.ResidentTianchi(_cfg(tmp, listing, 0), "train", DEV)
    fit = marks.fit_table(annotated, marks.detect(annotated))
    marks.save_table(tmp / "table.json", fit.table)
    want = {}
    for src in (1000, 360):
        up, down = ref.ratio(src, 500)
        taps, first = resample.design(up, down)
        sigs = [ref.resample(s, taps, first, up, down) for _, s, _ in recs]
        labs = [ref.rescale_marks([lab[k] for k in rr.KEYS], up, down) for _, _, lab in recs]
        want[src] = dict(up=up, down=down, sigs=sigs, labels=[l for l, _ in labs], moved=sum(m for _, m in labs))
    return dict(tmp=tmp, listing=listing, annotated=annotated, table=fit.table, want=want)


def _cfg(tmp, listing, source_rate, **data):
    cfg = rr.make_cfg(listing, scheme=SCHEME, data_root=tmp / "npy", label_root=tmp / "json")
    cfg.DATA.device_resident, cfg.DATA.source_rate = True, source_rate
    cfg.DATA.update(data)
    return cfg


def _check_batches(ld, labels):
    from test_resident_gpu import same_bits
    store, n = ld.store, 0
    for (_, idx, plan), meta in zip(ld.plans(), ld):
        rows = []
        for j, beat in zip(idx, plan.beats.tolist()):        # a plan made by hand from the expected labels
            lab = labels[j % 2]
            p_on, end = lab[0][beat], lab[0][beat + 1]
            rows.append([int(store.offsets[j]) + p_on, int(store.lengths[j]), end - p_on] + plan.table[len(rows), 3:].tolist())
            assert meta["rois"][len(rows) - 1, :, 0].tolist() == [lab[k][beat] - p_on for k in range(6)] + [end - p_on]
        data, target, rest = ops.beat_batch(store.signal, torch.tensor(rows, dtype=torch.int64), plan.V, plan.R)
        assert torch.equal(meta["data"], data) and torch.equal(meta["target_view"], target) and torch.equal(meta["rest_view"], rest)
        want = rr.plan_items(store, plan)
        assert same_bits(meta["data"].cpu().numpy(), want["data"]) and np.array_equal(meta["rois"].cpu().numpy(), want["rois"])
        n += 1
    return n


@pytest.mark.parametrize("src", [1000, 360])
def test_store_and_loaders_at_a_declared_source_rate(tree, tmp_path, src):
    w = tree["want"][src]
    names = [n + ".json" for n in rr.NAMES]
    (tmp_path / "list.txt").write_text("\n".join(names * 3) + "\n")
    cfg = _cfg(tree["tmp"], tmp_path / "list.txt", src)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    assert isinstance(train, resident.ResidentLoader) and len(train) == len(test) == 3
    for ld in (train, test):
        st = ld.store
        L = [ref.out_len(5000, w["up"], w["down"])] * 2
        assert st.source_rate == src and st.raw_lengths.tolist() == [5000] * 6 and st.lengths.tolist() == L * 3
        assert st.offsets.tolist() == np.concatenate([[0], np.cumsum([8 * v for v in L * 3])]).tolist() and st.signal.dtype == torch.float32
        assert torch.equal(st.signal.cpu(), torch.from_numpy(np.concatenate([s.reshape(-1) for s in w["sigs"]] * 3)))
        assert st.resample_report == dict(recordings=6, source_rate=src, sample_rate=500, up=w["up"], down=w["down"],
                                          taps=resample.taps_per_phase(w["up"], w["down"]), launches=1, adjusted=3 * w["moved"])
        for i in range(6):
            for k in range(6):
                assert st.labels[k][st.label_offsets[k][i]:st.label_offsets[k][i + 1]].tolist() == w["labels"][i % 2][k]
        assert _check_batches(ld, w["labels"]) == 3
    # the same store resampled in chunks of one recording
    st = train.store
    raw = resident.ResidentTianchi(_cfg(tree["tmp"], tmp_path / "list.txt", 0), "train", DEV)
    raw.source = st.source
    raw._resample(budget=1)
    assert raw.resample_report["launches"] == 6 and torch.equal(raw.signal, st.signal) and np.array_equal(raw.offsets, st.offsets)


@pytest.mark.parametrize("src", [1000, 360])
def test_auto_marks_run_on_the_resampled_store(tree, tmp_path, src):
    w = tree["want"][src]
    cfg = _cfg(tree["tmp"], tree["listing"], src, auto_marks=True, mark_table=str(tree["tmp"] / "table.json"))
    cfg.DATA.train_label_root = str(tree["tmp"] / "none")              # no label file is opened
    train, test = train_net.build_loaders(cfg, batch_size=2)
    st = train.store
    assert torch.equal(st.signal.cpu(), torch.from_numpy(np.concatenate([s.reshape(-1) for s in w["sigs"]])))
    rows = [mref.peaks(mref.envelope(s)) for s in w["sigs"]]
    want, dropped, adjusted = mref.labels_from_peaks(np.stack([r[0] for r in rows]), [r[1] for r in rows], st.lengths, tree["table"])
    for i in range(2):
        for k in range(6):
            assert st.labels[k][st.label_offsets[k][i]:st.label_offsets[k][i + 1]].tolist() == want[k][i]
    assert st.auto_report["peaks"] == sum(r[1] for r in rows) and st.auto_report["dropped"] == sum(dropped) and st.auto_report["marked"] == 2
    assert st.resample_report["adjusted"] == 0 and st.source_rate == src
    assert _check_batches(test, [[want[k][i] for k in range(6)] for i in range(2)]) == 1


def test_source_rate_off_is_the_key_off_store_field_for_field(tree):
    base = tree["annotated"]
    for rate in (0, 500, 500.0):
        st = resident.ResidentTianchi(_cfg(tree["tmp"], tree["listing"], rate), "train", DEV)
        assert st.source is None and st.source_rate == 0 and st.resample_report is None and st.raw_lengths is st.lengths
        assert st.signal.dtype == torch.int16 and torch.equal(st.signal, base.signal) and st.names == base.names
        assert np.array_equal(st.lengths, base.lengths) and np.array_equal(st.offsets, base.offsets) and np.array_equal(st.n_p_on, base.n_p_on)
        assert all(np.array_equal(a, b) for a, b in zip(st.labels, base.labels))
        assert all(np.array_equal(a, b) for a, b in zip(st.label_offsets, base.label_offsets))


def _native_want(sig, src_plan, raw_len):
    taps, first = resample.design(src_plan.down, src_plan.up, src_plan.zeros, src_plan.beta)
    return ref.resample(sig, taps, first, src_plan.down, src_plan.up)[:, :raw_len]


@pytest.mark.parametrize("src", [1000, 360])
def test_synthesize_hands_the_strips_back_at_the_source_rate(tree, src):
    import test_model_gpu as tm
    from electrocardio_panorama_amd import recording
    from test_resident_gpu import same_bits
    store = resident.ResidentTianchi(_cfg(tree["tmp"], tree["listing"], src), "test", DEV)
    model = tm.hashed_model(3).eval()
    syn = recording.synthesize(model, store, range(2), [1, 3, 6], native_rate=True)
    plain = recording.synthesize(model, store, range(2), [1, 3, 6])
    assert plain.native is None and np.array_equal(plain.stats.cpu().numpy(), syn.stats.cpu().numpy(), equal_nan=True)    # the model rate's
    assert same_bits(plain.out.cpu().numpy(), syn.out.cpu().numpy())
    assert syn.native_offsets.tolist() == [0, 12 * 5000, 24 * 5000]
    K = resample.taps_per_phase(store.source.down, store.source.up)
    for j, (got, at_model_rate) in enumerate(zip(syn.native_signals, syn.signals)):
        assert tuple(got.shape) == (12, 5000) and tuple(at_model_rate.shape) == (12, int(store.lengths[j]))
        want = _native_want(at_model_rate.cpu().numpy(), store.source, 5000)
        assert same_bits(got.cpu().numpy(), want)
        # NaN outside [p_0, p_last), spread by at most K samples; numbers inside
        p = store.labels[0][store.label_offsets[0][j]:store.label_offsets[0][j + 1]]
        lo, hi = int(p[0]) * store.source.down // store.source.up, int(p[-1]) * store.source.down // store.source.up
        nan = np.isnan(want)
        assert nan[:, :max(lo - 2 * K, 0)].all() and nan[:, hi + 2 * K:].all() and not nan[:, lo + 2 * K:hi - 2 * K].any() and hi - lo > 3000
    assert plain.native_signals[0] is not None and torch.equal(plain.native_signals[0], plain.signals[0])


def test_train_gen_net_and_mark_net_at_a_source_rate(tree, tmp_path, capsys, monkeypatch):
    """One epoch of Solver.train on the loaders of a 360 Hz tree; gen_net --native-rate --out on the checkpoint; mark_net --resample, whose
    files the unchanged host dataset and the key-off store read."""
    from electrocardio_panorama_amd import gen_net, mark_net
    from electrocardio_panorama_amd.dataset.tianchi import EcgTianChiInterval
    from electrocardio_panorama_amd.prefetch import DevicePrefetcher
    from electrocardio_panorama_amd.solver import Solver
    from test_resident_gpu import same_bits
    w = tree["want"][360]
    cfg = _cfg(tree["tmp"], tree["listing"], 360)
    cfg.SOLVER.epochs = 1
    cfg.output_dir, cfg.desc = str(tmp_path), "rate"
    run_cfg = cfg.clone()                                           # gen_net.run appends the description itself
    cfg.output_dir = os.path.join(str(tmp_path), "rate")
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    random.seed(100)
    capsys.readouterr()
    sol.train(DevicePrefetcher(train, sol.device), DevicePrefetcher(test, sol.device))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch ")]
    assert len(lines) == 1 and np.isfinite(float(lines[0].split("train_loss: ")[1].split(",")[0]))
    assert os.path.exists(os.path.join(sol.output_dir, "epoch_0.pkl"))
    # gen_net: the strips on the recordings' own time axis
    monkeypatch.setattr(gen_net, "cfg", run_cfg)
    result = gen_net.run(["--epoch", "0", "--native-rate", "--out", str(tmp_path / "strips")])
    out = capsys.readouterr().out
    assert "resampled 2 recordings from 360 Hz to 500 Hz (25/18, 33 taps a phase)" in out and len(result) == 4
    doc = json.loads((tmp_path / "strips" / "metrics.json").read_text())
    assert doc["native_rate"] is True and doc["source_rate"] == 360
    for name in rr.NAMES:
        assert np.load(tmp_path / "strips" / (name + ".npy")).shape == (12, 5000)
    run_cfg.output_dir = str(tmp_path)                               # run() appended the description to it
    gen_net.run(["--epoch", "0", "--out", str(tmp_path / "model_rate")])
    for name in rr.NAMES:
        at_model_rate = np.load(tmp_path / "model_rate" / (name + ".npy"))
        assert at_model_rate.shape == (12, 6945)
        assert same_bits(np.load(tmp_path / "strips" / (name + ".npy")), _native_want(at_model_rate, train.store.source, 5000))
    # mark_net --resample: files for the host loader
    monkeypatch.setattr(mark_net, "cfg", run_cfg)
    report = mark_net.run(["--resample", str(tmp_path / "files"), "--phase", "train"])
    assert report == train.store.resample_report
    assert sorted(os.listdir(tmp_path / "files")) == ["11315.json", "11315.npy", "40723.json", "40723.npy"]
    host_cfg = run_cfg.clone()
    host_cfg.DATA.source_rate, host_cfg.DATA.device_resident = 0, False
    host_cfg.DATA.train_data_root = host_cfg.DATA.train_label_root = str(tmp_path / "files")
    ds = EcgTianChiInterval(host_cfg, "train")
    for i, name in enumerate(ds.dataset):
        sig, lab = ds._load(name)
        assert list(lab) == list(rr.KEYS) and [lab[k] for k in rr.KEYS] == w["labels"][i]
        assert np.load(tmp_path / "files" / name.replace(".json", ".npy")).dtype == np.float32 and np.array_equal(sig, w["sigs"][i].astype(np.float64))
        random.seed(i)
        np.random.seed(i)
        item = ds[i]
        assert item["data"].shape == (3, 512) and np.isfinite(item["data"]).all() and item["rois"].shape == (7, 2)
    host = resident.ResidentTianchi(host_cfg, "train", DEV)        # the key-off store of those files is the resampled store
    assert host.signal.dtype == torch.float32 and torch.equal(host.signal, train.store.signal) and host.source_rate == 0
    assert all(np.array_equal(a, b) for a, b in zip(host.labels, train.store.labels))
    with pytest.raises(ValueError, match="nothing to resample"):
        monkeypatch.setattr(mark_net, "cfg", host_cfg)
        mark_net.run(["--resample", str(tmp_path / "again")])
