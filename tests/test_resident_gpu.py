"""DATA.device_resident on the device: nef_beat_batch against the fp64 restatement of tests/resident_ref.py, bit for bit on every output
element (tests/test_resident_cpu.py ties that restatement to EcgTianChiInterval.__getitem__), and the loader end to end through
train_net.build_loaders and the Solver."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import resident_ref as rr
from electrocardio_panorama_amd import ops, train_net
from electrocardio_panorama_amd.dataset import resident
from electrocardio_panorama_amd.dataset.tianchi import _lead_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_FULL = {}          # (store tag, recording, beat) -> the restatement's 12 normalised leads [12, 512] float32, computed once


def same_bits(got, want):
    """Equal bit patterns wherever the reference is a number, NaN exactly where it is NaN (a NaN's sign and payload are not numpy's to fix)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def on_device(store, tag, float32=False):
    st = copy.copy(store)
    st.signal = (store.signal.float() if float32 else store.signal).to(DEV)
    st.tag = tag
    return st


def full12(store, rec, beat):
    key = (store.tag, rec, beat)
    if key not in _FULL:
        s8 = store.signal[store.offsets[rec]:store.offsets[rec + 1]].cpu().numpy().reshape(8, -1)
        lab = {k: store.labels[q][store.label_offsets[q][rec]:store.label_offsets[q][rec + 1]].tolist() for q, k in enumerate(rr.KEYS)}
        _FULL[key] = rr.beat_item(s8, lab, beat, list(range(12)), 0, [])["data"]
    return _FULL[key]


def table_row(store, rec, beat, leads):
    p_on = int(store.labels[0][store.label_offsets[0][rec] + beat])
    end = int(store.labels[0][store.label_offsets[0][rec] + beat + 1])
    return [int(store.offsets[rec]) + p_on, int(store.lengths[rec]), end - p_on] + list(leads)


def check_batch(store, picks, V, R, device_plan=False):
    """picks: [(recording, beat, [V input leads, target, R rest leads])] -> one launch, every output element against the restatement."""
    table = torch.tensor([table_row(store, r, b, leads) for r, b, leads in picks], dtype=torch.int64)
    data, target, rest = ops.beat_batch(store.signal, table.to(DEV) if device_plan else table, V, R)
    assert data.shape == (len(picks), V, 512) and target.shape == (len(picks), 512) and rest.shape == (len(picks), R, 512)
    data, target, rest = data.cpu().numpy(), target.cpu().numpy(), rest.cpu().numpy()
    for j, (r, b, leads) in enumerate(picks):
        ref = full12(store, r, b)
        assert same_bits(data[j], ref[leads[:V]]), ("data", j, r, b)
        assert same_bits(target[j], ref[leads[V]]), ("target_view", j, r, b)
        assert same_bits(rest[j], ref[leads[V + 1:]].reshape(R, 512)), ("rest_view", j, r, b)
    return data, target, rest


def all_beats(store):
    return [(r, b) for r in range(len(store)) for b in range(int(store.n_p_on[r]) - 1)]


def scheme_leads(scheme, rng):
    sel, sup, unsup, keep = _lead_plan(*scheme, rng=rng)
    rest = list(sup) if keep else [x for x in sup if x not in sel]
    return list(sel) + [rng.sample(rest, 1)[0]] + rest + list(unsup), len(sel), len(rest) + len(unsup)


# ------------------------------------------------------------------------------------------------ the bundled recordings
@pytest.fixture(scope="module")
def real(tmp_path_factory):
    host = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp_path_factory.mktemp("real"))), "train")
    assert host.signal.dtype == torch.int16
    return {"int16": on_device(host, "real16"), "float32": on_device(host, "real32", float32=True)}


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("scheme", rr.SCHEMES, ids=lambda s: f"V{s[0]}{s[1]}")
def test_all_thirty_real_beats_every_lead_scheme(real, dtype, scheme):
    store, rng = real[dtype], random.Random(3)
    beats = all_beats(store)
    assert len(beats) == 30
    ns = [table_row(store, r, b, [])[2] for r, b in beats]
    assert min(ns) == 265 and max(ns) == 315 and {table_row(store, r, b, [])[0] % 8 for r, b in beats} == set(range(8))
    picks, V, R = [], None, None
    for r, b in beats:
        leads, V, R = scheme_leads(scheme, rng)
        picks.append((r, b, leads))
    check_batch(store, picks, V, R)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("B", [1, 67])
def test_real_beats_other_batch_sizes(real, dtype, B):
    store, rng = real[dtype], random.Random(B)
    beats = all_beats(store)
    picks = []
    for j in range(B):
        leads, V, R = scheme_leads(rr.SCHEMES[0], rng)
        picks.append(beats[(7 * j) % 30] + (leads,))
    check_batch(store, picks, V, R, device_plan=True)


# ------------------------------------------------------------------------------------------------ the edges, on a synthetic store
def _synthetic(tmp, floats):
    """Recordings of lengths 700, 5003, 5000, 1000 and 600 whose beats have n = 1, 2, 511, 183 / 512, 513, 1300, 2677 / 5000 / nine of 9
    samples at every p_on residue mod 8 / a constant beat and one whose extremes are in derived leads only."""
    rng = np.random.default_rng(5 + floats)
    draw = (lambda n: (rng.normal(0, 300, size=(8, n))).astype(np.float32).astype(np.float64)) if floats else \
           (lambda n: rng.integers(-2000, 2000, size=(8, n)).astype(np.float64))
    r0, r1, r2, r3, r4 = draw(700), draw(5003), draw(5000), draw(1000), draw(600)
    r1[5, 1026 + 900] = 30000.0                   # the maximum of the n = 1300 beat sits at position 900 >= 512
    r2[7, 4999] = -30000.0                        # the minimum of the n = 5000 beat at its last position
    r4[:, 10:300] = 0.0                           # a constant beat: hi == lo
    r4[:, 300:590] = np.clip(r4[:, 300:590], -40, 40)    # derived leads of these stay within +-80
    r4[0, 400], r4[1, 400] = 100.0, -100.0        # III = -200 and aVL = 150 there: both extremes are in derived leads only
    recs = [("r0", r0, rr.labels_for([3, 4, 6, 517, 700])), ("r1", r1, rr.labels_for([1, 513, 1026, 2326, 5003])),
            ("r2", r2, rr.labels_for([0, 5000])), ("r3", r3, rr.labels_for([8 + 9 * i for i in range(10)])),
            ("r4", r4, rr.labels_for([10, 300, 590]))]
    lst = rr.write_tree(tmp, recs)
    return resident.ResidentTianchi(rr.make_cfg(lst, data_root=tmp / "npy", label_root=tmp / "json"), "train")


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    a, b = _synthetic(tmp_path_factory.mktemp("syn16"), 0), _synthetic(tmp_path_factory.mktemp("syn32"), 1)
    assert a.signal.dtype == torch.int16 and b.signal.dtype == torch.float32
    assert a.lengths.tolist() == [700, 5003, 5000, 1000, 600]
    return {"int16": on_device(a, "syn16"), "float32": on_device(b, "syn32")}


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_edges_every_length_alignment_and_no_rest_views(synthetic, dtype):
    store = synthetic[dtype]
    beats = all_beats(store)
    ns = [table_row(store, r, b, [])[2] for r, b in beats]
    assert {1, 2, 511, 512, 513, 1300, 5000} <= set(ns)
    assert {table_row(store, 3, b, [])[0] % 8 for b in range(9)} == set(range(8))
    # all 12 leads as inputs, R = 0: lead strides 700 and 5003 put the eight rows of a beat at different alignments
    check_batch(store, [(r, b, list(range(12)) + [9]) for r, b in beats], 12, 0)
    # one input lead, a derived target, every other lead as a rest view
    check_batch(store, [(r, b, [1, 11, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10]) for r, b in beats], 1, 10, device_plan=True)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_edges_constant_beat_derived_extremes_and_extremes_past_512(synthetic, dtype):
    store = synthetic[dtype]
    leads = [0, 1, 8, 10, 5, 7, 9]                # V = 4, target lead 5, rest 7 and 9
    data, target, rest = check_batch(store, [(4, 0, leads), (4, 1, leads), (1, 2, leads), (2, 0, leads)], 4, 2)
    # the constant beat: NaN where numpy gives NaN (t < n = 290), zeros in the padding
    assert np.isnan(data[0][:, :290]).all() and (data[0][:, 290:] == 0).all() and np.isnan(target[0][:290]).all() and (target[0][290:] == 0).all()
    # extremes in derived leads only: III reaches 0.0 and aVL 1.0 at position 100 of the beat, no stored lead does
    assert data[1][2, 100] == 0.0 and data[1][3, 100] == 1.0 and 0.0 < data[1][:2, :290].min() and data[1][:2, :290].max() < 1.0
    # the n = 1300 beat's maximum is at position 900: the 512 samples written never reach 1.0 but were scaled by it
    assert target[2].max() < 0.2 and np.isfinite(target[2]).all()
    assert rest[3][0].min() > 0.8                 # lead 7 of the n = 5000 beat: its minimum of -30000 sits at position 4999


def test_two_launches_in_a_row_into_fresh_buffers(real):
    store, beats = real["int16"], all_beats(real["int16"])
    p1 = [(r, b, [1, 3, 6, 0, 2]) for r, b in beats[:7]]
    p2 = [(r, b, [6, 3, 1, 11, 8]) for r, b in beats[7:20]]
    t1 = torch.tensor([table_row(store, *p) for p in p1], dtype=torch.int64).to(DEV)
    t2 = torch.tensor([table_row(store, *p) for p in p2], dtype=torch.int64).to(DEV)
    o1 = ops.beat_batch(store.signal, t1, 3, 1)
    o2 = ops.beat_batch(store.signal, t2, 3, 1)
    assert len({t.data_ptr() for t in o1 + o2}) == 6
    for outs, picks in ((o1, p1), (o2, p2)):
        for j, (r, b, leads) in enumerate(picks):
            ref = full12(store, r, b)
            assert same_bits(outs[0][j].cpu().numpy(), ref[leads[:3]]) and same_bits(outs[1][j].cpu().numpy(), ref[leads[3]])
            assert same_bits(outs[2][j].cpu().numpy(), ref[leads[4:]])


def test_a_device_plan_row_outside_the_signal_reads_nothing(real):
    """A plan that is on the device already is not seen by the host: the kernel answers a bad row with NaNs.  (Both bad rows here stay
    inside the signal even if they were read.)"""
    store = real["int16"]
    good = table_row(store, 0, 0, [1, 3, 6, 0, 2])
    bad_lead = table_row(store, 0, 1, [1, 3, 12, 0, 2])
    bad_n = table_row(store, 0, 2, [1, 3, 6, 0, 2])
    bad_n[1], bad_n[2] = 100, 101                 # n > stride
    data, target, rest = ops.beat_batch(store.signal, torch.tensor([good, bad_lead, bad_n], dtype=torch.int64).to(DEV), 3, 1)
    ref = full12(store, 0, 0)
    assert same_bits(data[0].cpu().numpy(), ref[[1, 3, 6]]) and same_bits(target[0].cpu().numpy(), ref[0])
    for t in (data[1:], target[1:], rest[1:]):
        assert bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------ end to end
def _cfg(tmp_path, repeat=3, **solver):
    cfg = rr.make_cfg(rr.write_listing(tmp_path, repeat=repeat), scheme=(3, "IIv2v5_v4I_372", "input_fix"))
    cfg.DATA.device_resident = True
    cfg.SOLVER.update(solver)
    cfg.output_dir, cfg.desc = str(tmp_path), "resident"
    return cfg


def _host(meta):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in meta.items()}


def test_build_loaders_yields_the_restatement_of_the_loaders_own_plan(tmp_path):
    cfg = _cfg(tmp_path)
    train, test = train_net.build_loaders(cfg, batch_size=2)
    assert isinstance(train, resident.ResidentLoader) and isinstance(test, resident.ResidentLoader) and len(train) == len(test) == 3
    for ld in (train, test):
        store, n = ld.store, 0
        seen = []
        for (i, idx, plan), meta in zip(ld.plans(), ld):
            want = rr.plan_items(store, plan)
            for k in ("data", "target_view", "rest_view"):
                assert meta[k].is_cuda and meta[k].dtype == torch.float32 and same_bits(meta[k].cpu().numpy(), want[k]), k
            for k in ("rois", "input_theta", "target_theta", "rest_theta"):
                assert meta[k].is_cuda and np.array_equal(meta[k].cpu().numpy(), want[k]) and meta[k].cpu().numpy().dtype == want[k].dtype, k
            assert meta["rois"].dtype == torch.int64 and meta["noise"].shape == (2, 512) and not bool(meta["noise"].any())
            assert meta["id"] == plan.id and meta["unsupervision_lead_name"] == [[5, 0], [5, 0]] and meta["rest_view"].shape == (2, 9, 512)
            seen += idx
            n += 1
        assert n == 3 and sorted(seen) == list(range(6))
    cfg.DATA.device_resident = False
    from torch.utils.data import DataLoader
    assert all(isinstance(dl, DataLoader) for dl in train_net.build_loaders(cfg, batch_size=2))


class _Recorder:
    """A loader that keeps a host copy of what it hands on, per epoch."""

    def __init__(self, loader):
        self.loader, self.sampler, self.seen = loader, loader.sampler, {}

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for meta in self.loader:
            self.seen.setdefault(self.sampler.epoch, []).append(_host(meta))
            yield meta


def test_solver_trains_checkpoints_and_a_resumed_epoch_gets_the_same_batches(tmp_path, capsys):
    """Two epochs at batch 2 through Solver.train with finite losses and a checkpoint; a second Solver resumes from it -- like the reference
    the saved epoch index is re-run -- and the loader hands the re-run epoch the batches of the uninterrupted one, bit for bit."""
    from electrocardio_panorama_amd.prefetch import DevicePrefetcher
    from electrocardio_panorama_amd.solver import Solver

    def run(epochs):
        cfg = _cfg(tmp_path, epochs=epochs)
        torch.manual_seed(1234)
        sol = Solver(cfg, use_tensorboardx=False)
        train, test = train_net.build_loaders(cfg, batch_size=2)
        rec = _Recorder(train)
        random.seed(100)
        capsys.readouterr()
        sol.train(DevicePrefetcher(rec, sol.device), DevicePrefetcher(test, sol.device))
        return rec.seen, capsys.readouterr().out

    seen, out = run(2)
    lines = [ln for ln in out.splitlines() if ln.startswith("Epoch ")]
    assert [ln.split(":")[0] for ln in lines] == ["Epoch 0", "Epoch 1"]
    assert all(np.isfinite(float(ln.split("train_loss: ")[1].split(",")[0])) and np.isfinite(float(ln.split("test_loss: ")[1])) for ln in lines)
    assert os.path.exists(os.path.join(str(tmp_path), "resident", "epoch_1.pkl"))
    assert sorted(seen) == [0, 1] and len(seen[0]) == len(seen[1]) == 3
    assert not all(np.array_equal(a["data"], b["data"], equal_nan=True) for a, b in zip(seen[0], seen[1]))      # a new order and new draws
    seen2, out2 = run(3)
    assert [ln.split(":")[0] for ln in out2.splitlines() if ln.startswith("Epoch ")] == ["Epoch 1", "Epoch 2"]
    for a, b in zip(seen[1], seen2[1]):
        assert a["id"] == b["id"]
        for k in ("data", "rois", "input_theta", "target_view", "target_theta", "rest_view", "rest_theta", "noise"):
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graphed"])
def test_a_step_fed_by_the_loader_equals_a_step_fed_from_the_host(tmp_path, graph):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    cfg = _cfg(tmp_path, repeat=2, graph=graph)
    train, = train_net.build_loaders(cfg, batch_size=2, phases=("train",))[:1]
    batches = list(train)
    assert len(batches) == 2
    hosted = [{k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in _host(m).items()} for m in batches]
    got = []
    for feed in (batches, hosted):
        torch.manual_seed(1234)
        sol = Solver(cfg, use_tensorboardx=False)
        sol.model.dropout_p = 0.0
        opt = get_optimizer(cfg, sol.model.parameters())
        random.seed(7)
        rows = sol.run_one_epoch(feed, "train", opt, collect_views=False)[0]
        assert (getattr(sol, "_graph_stepper", None) is not None) == graph
        got.append((np.array(rows), opt._flat[0]["p"].detach().cpu().numpy().copy()))
    assert np.isfinite(got[0][0]).all() and got[0][0].shape[0] == 2
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


def test_train_views_and_input_augmentation_run_with_the_key_on(tmp_path):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    cfg = _cfg(tmp_path, repeat=2, train_views=2)
    cfg.DATA.aug_noise_std = 0.05
    train, = train_net.build_loaders(cfg, batch_size=2, phases=("train",))[:1]
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    opt = get_optimizer(cfg, sol.model.parameters())
    random.seed(7)
    rows = np.array(sol.run_one_epoch(train, "train", opt, collect_views=False)[0])
    assert rows.shape[0] == 2 and np.isfinite(rows).all() and sol.augment is not None and sol.train_views == 2
