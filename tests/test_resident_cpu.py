"""DATA.device_resident without a device: the fp64 restatement against the product dataset, the store's packing, the loader's order and
the argument errors (tests/test_resident_gpu.py holds the kernel against the same restatement)."""
import os
import random

import numpy as np
import pytest
import torch

import resident_ref as rr
from electrocardio_panorama_amd import ops, train_net
from electrocardio_panorama_amd.dataset import build_dataset, resident

FIELDS = ("data", "rois", "input_theta", "target_view", "target_theta", "rest_theta")


@pytest.mark.parametrize("scheme", rr.SCHEMES, ids=lambda s: f"V{s[0]}{s[1]}")
def test_plan_and_restatement_reproduce_the_dataset_items(tmp_path, scheme):
    """Same seeds, rng=random: the plan makes the dataset's choices, and the restatement of the planned items equals the dataset's bit for bit."""
    cfg = rr.make_cfg(rr.write_listing(tmp_path), scheme)
    order, s = [0, 1, 0, 1, 1, 0], 11
    ds = build_dataset(cfg, "train")
    random.seed(s)
    np.random.seed(s)
    items = [ds[i] for i in order]
    after = random.getstate()
    store = resident.ResidentTianchi(cfg, "train")
    random.seed(s)
    np.random.seed(s)
    plan = resident.draw_plan(store, order, cfg, "train", random)
    assert random.getstate() == after                       # the same number of draws, in the same order
    got = rr.plan_items(store, plan)
    host = {"rois": plan.rois, "input_theta": plan.input_theta, "target_theta": plan.target_theta, "rest_theta": plan.rest_theta}
    for k in FIELDS:
        want = np.stack([it[k] for it in items])
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert np.array_equal(got[k], want, equal_nan=True), k
        if k in host:                                       # the loader's host arrays are the plan's, not the restatement's
            assert host[k].dtype == want.dtype and np.array_equal(host[k], want), k
    assert np.array_equal(got["rest_view"], np.stack([it["rest_view"].astype(np.float32) for it in items]))
    assert plan.id == [it["id"] for it in items]
    assert plan.unsupervision_lead_name == [it["unsupervision_lead_name"] for it in items]
    assert plan.table.dtype == np.int64 and plan.table.shape == (6, 3 + plan.V + 1 + plan.R) and plan.V == scheme[0]
    assert (plan.rois[:, 6, 1] == 512).all() and (plan.rois[:, 6, 0] == plan.table[:, 2]).all()


def test_jitter_comes_from_the_generator_handed_in(tmp_path):
    cfg = rr.make_cfg(rr.write_listing(tmp_path))
    cfg.MODEL.jitter_factor = 2.5
    store = resident.ResidentTianchi(cfg, "train")
    with pytest.raises(ValueError, match="jitter"):
        resident.draw_plan(store, [0, 1], cfg, "train", random.Random(1))
    state = np.random.get_state()
    a = resident.draw_plan(store, [0, 1], cfg, "train", random.Random(1), np.random.default_rng(7))
    b = resident.draw_plan(store, [0, 1], cfg, "train", random.Random(1), np.random.default_rng(7))
    c = resident.draw_plan(store, [0, 1], cfg, "train", random.Random(1), np.random.default_rng(8))
    t = resident.draw_plan(store, [0, 1], cfg, "test", random.Random(1))                 # the test phase never jitters
    assert np.array_equal(a.input_theta, b.input_theta) and not np.array_equal(a.input_theta, c.input_theta)
    assert np.array_equal(a.table, t.table) and not np.array_equal(a.input_theta, t.input_theta)
    assert np.abs(a.input_theta - t.input_theta).max() < 0.5
    assert all(np.array_equal(x, y) for x, y in zip(state[1:2], np.random.get_state()[1:2]))


def _tree(tmp_path, sigs, p_ons):
    return rr.write_tree(tmp_path, [(f"r{i}", s, rr.labels_for(p)) for i, (s, p) in enumerate(zip(sigs, p_ons))])


def test_store_packs_int16_or_float32_and_keeps_mixed_lengths(tmp_path):
    rng = np.random.default_rng(0)
    a = rng.integers(-3000, 3000, size=(8, 700)).astype(np.float64)
    b = rng.integers(-32768, 32768, size=(8, 5003)).astype(np.int16)
    lst = _tree(tmp_path, [a, b], [[5, 300, 650], [0, 2000, 5003]])
    cfg = rr.make_cfg(lst, data_root=tmp_path / "npy", label_root=tmp_path / "json")
    st = resident.ResidentTianchi(cfg, "train")
    assert st.signal.dtype == torch.int16 and st.signal.device.type == "cpu" and len(st) == 2
    assert st.lengths.tolist() == [700, 5003] and st.offsets.tolist() == [0, 5600, 5600 + 8 * 5003] and st.offsets.dtype == np.int64
    assert np.array_equal(st.signal[:5600].numpy().reshape(8, 700), a) and np.array_equal(st.signal[5600:].numpy().reshape(8, 5003), b)
    assert st.n_p_on.tolist() == [3, 3] and st.labels[0].tolist() == [5, 300, 650, 0, 2000, 5003]
    assert st.label_offsets[0].tolist() == [0, 3, 6] and st.device_bytes == 2 * 8 * 5703
    # one value that is no int16 (but a float32): the whole store is float32, the int16 recording exactly so
    a32 = a.copy()
    a32[3, 77] = 0.5
    os.makedirs(tmp_path / "f", exist_ok=True)
    lst = _tree(tmp_path / "f", [a32, b], [[5, 300, 650], [0, 2000, 5003]])
    st = resident.ResidentTianchi(rr.make_cfg(lst, data_root=tmp_path / "f" / "npy", label_root=tmp_path / "f" / "json"), "train")
    assert st.signal.dtype == torch.float32 and st.signal[3 * 700 + 77].item() == 0.5
    assert np.array_equal(st.signal[5600:].numpy().astype(np.float64).reshape(8, 5003), b.astype(np.float64))
    # a value past int16's range stays exact as float32 too
    assert resident._pack("x", np.full((8, 4), 40000.0)).dtype == np.float32


def test_store_rejects_a_lossy_recording_and_a_one_beat_recording(tmp_path):
    ok = np.zeros((8, 700))
    bad = ok.copy()
    bad[0, 3] = 0.1                                           # neither an int16 nor a float32
    lst = _tree(tmp_path, [ok, bad, bad], [[5, 300, 650]] * 3)
    with pytest.raises(ValueError, match=r"r1\.json"):       # the first offender in list order
        resident.ResidentTianchi(rr.make_cfg(lst, data_root=tmp_path / "npy", label_root=tmp_path / "json"), "train")
    os.makedirs(tmp_path / "one", exist_ok=True)
    lst = rr.write_tree(tmp_path / "one", [("a", ok, rr.labels_for([5, 300])), ("b", ok, {k: [7] for k in rr.KEYS})])
    with pytest.raises(ValueError, match=r"b\.json.*no drawable beat"):
        resident.ResidentTianchi(rr.make_cfg(lst, data_root=tmp_path / "one" / "npy", label_root=tmp_path / "one" / "json"), "train")
    os.makedirs(tmp_path / "end", exist_ok=True)
    lst = rr.write_tree(tmp_path / "end", [("a", ok, rr.labels_for([5, 300, 701]))])      # a beat that leaves the recording
    with pytest.raises(ValueError, match=r"a\.json"):
        resident.ResidentTianchi(rr.make_cfg(lst, data_root=tmp_path / "end" / "npy", label_root=tmp_path / "end" / "json"), "train")


def test_store_reads_the_bundled_npz_recordings(tmp_path):
    st = resident.ResidentTianchi(rr.make_cfg(rr.write_listing(tmp_path)), "test")
    assert st.signal.dtype == torch.int16 and st.lengths.tolist() == [5000, 5000] and (st.n_p_on - 1).sum() == 30
    for i, (name, sig, lab) in enumerate(rr.recordings()):
        assert st.names[i] == name and np.array_equal(st.signal[st.offsets[i]:st.offsets[i + 1]].numpy().reshape(8, 5000), sig)
        assert st.labels[0][st.label_offsets[0][i]:st.label_offsets[0][i + 1]].tolist() == lab["P on"]


def test_loader_order_shards_epochs_and_global_rng_state(tmp_path):
    cfg = rr.make_cfg(rr.write_listing(tmp_path, repeat=11))          # 22 list entries
    store = resident.ResidentTianchi(cfg, "train")
    ranks = [resident.ResidentLoader(store, cfg, "train", 3, seed=5, rank=r, world=2) for r in range(2)]
    assert [len(ld) for ld in ranks] == [3, 3]                         # 11 per rank, batches of 3, the short one dropped
    py, npy = random.getstate(), np.random.get_state()
    seen = [[i for _, idx, _ in ld.plans() for i in idx] for ld in ranks]
    assert random.getstate() == py and all(np.array_equal(a, b) for a, b in zip(npy, np.random.get_state()) if isinstance(a, np.ndarray))
    assert len(seen[0]) == len(seen[1]) == 9 and len(set(seen[0] + seen[1])) == 18 and set(seen[0] + seen[1]) <= set(range(22))
    both = sorted(ranks[0].order() + ranks[1].order())
    assert both == list(range(22))                                     # before drop_last the two shards are the whole permutation
    tables = [np.concatenate([p.table for _, _, p in ld.plans()]) for ld in ranks]
    again = [np.concatenate([p.table for _, _, p in ld.plans()]) for ld in ranks]
    assert all(np.array_equal(a, b) for a, b in zip(tables, again))    # the same (seed, epoch) repeats
    for ld in ranks:
        ld.sampler.set_epoch(1)
    seen1 = [[i for _, idx, _ in ld.plans() for i in idx] for ld in ranks]
    assert seen1 != seen and sorted(ranks[0].order() + ranks[1].order()) == list(range(22))
    assert not np.array_equal(np.concatenate([p.table for _, _, p in ranks[0].plans()]), tables[0])
    for ld in ranks:
        ld.sampler.set_epoch(0)
    assert [[i for _, idx, _ in ld.plans() for i in idx] for ld in ranks] == seen
    other = resident.ResidentLoader(store, cfg, "train", 3, seed=6, rank=0, world=2)
    assert [i for _, idx, _ in other.plans() for i in idx] != seen[0]
    # odd list under two ranks: the permutation's tail is dropped, as the DistributedSampler's drop_last does
    cfg21 = rr.make_cfg(rr.write_listing(tmp_path, names=["11315.json"] * 21))
    st21 = resident.ResidentTianchi(cfg21, "train")
    o = [resident.ResidentLoader(st21, cfg21, "train", 5, seed=1, rank=r, world=2).order() for r in range(2)]
    assert len(o[0]) == len(o[1]) == 10 and not set(o[0]) & set(o[1])
    # the test phase: the list in order, whole
    test = resident.ResidentLoader(store, cfg, "test", 4, seed=5)
    assert [idx for _, idx, _ in test.plans()] == [list(range(i, i + 4)) for i in range(0, 20, 4)] and len(test) == 5


def test_the_key_rejects_what_it_does_not_build(tmp_path):
    base = rr.make_cfg(rr.write_listing(tmp_path))
    for key, val, word in (("dataset", "ptbv2", "ptbv2"), ("noise", True, "DATA.noise"), ("weighted_sample", True, "weighted_sample"),
                           ("synthetic", True, "synthetic")):
        cfg = rr.make_cfg(rr.write_listing(tmp_path))
        cfg.DATA.device_resident = True
        cfg.DATA[key] = val
        with pytest.raises(ValueError, match=word):
            train_net.build_loaders(cfg, batch_size=2)
        with pytest.raises(ValueError, match=word):
            train_net.build_loaders(cfg, batch_size=2, phases=("test",))     # val_net's call
    assert base.DATA.device_resident is False


def test_beat_batch_argument_checks_need_no_device():
    sig = torch.zeros(8 * 100, dtype=torch.int16)
    row = [10, 100, 50, 1, 3, 6, 0, 2, 4]                    # V = 3, R = 2: offset, stride, n, leads
    good = torch.tensor([row], dtype=torch.int64)
    with pytest.raises(TypeError, match="signal"):
        ops.beat_batch(sig.double(), good, 3, 2)
    with pytest.raises(ValueError, match="signal"):
        ops.beat_batch(sig.reshape(8, 100), good, 3, 2)
    with pytest.raises(TypeError, match="plan"):
        ops.beat_batch(sig, good.int(), 3, 2)
    with pytest.raises(ValueError, match="plan"):
        ops.beat_batch(sig, good, 3, 4)                      # W does not fit
    with pytest.raises(ValueError, match="V = 0"):
        ops.beat_batch(sig, good, 0, 2)
    with pytest.raises(ValueError, match="R = 65"):
        ops.beat_batch(sig, good, 3, 65)
    for col, val in ((0, -1), (0, 60), (2, 0), (2, 101), (1, 0), (4, 12), (8, -1)):      # leaves the signal / names no lead
        bad = good.clone()
        bad[0, col] = val
        with pytest.raises(ValueError, match="plan row 0"):
            ops.beat_batch(sig, torch.cat([bad, good]), 3, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):  # everything checked, and then there is no device
        ops.beat_batch(sig, good, 3, 2)
