"""DATA.aug_warp / aug_roi_jitter without a GPU: the properties of the numpy restatement the GPU tests compare against
(tests/warp_ref.py), the keys and their rejections (warp.from_cfg), the seeds, ops.warp's argument checks, which sit in front of the
library, and the agreement of header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import warp_ref as ref
from warp_ref import ADVERSARIAL, adversarial_rois, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = (0.0,) * 6
A03 = (0.3,) * 6


def _cfg(**data):
    from electrocardio_panorama_amd.config.default import get_defaults
    cfg = get_defaults()
    for k, v in data.items():
        cfg.DATA[k] = v
    return cfg


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_identity_on_the_golden_rows():
    data, target, rest, rois = golden()
    d, t, r, ro, _ = ref.warp(data, target, rest, rois, 5, ZERO, 0)
    assert np.array_equal(bits(d), bits(data)) and np.array_equal(bits(t), bits(target)) and np.array_equal(bits(r), bits(rest))
    assert np.array_equal(ro, rois)


def test_golden_rows_at_03_end_at_265_and_334():
    data, target, rest, rois = golden()
    d, t, r, ro, tbs = ref.warp(data, target, rest, rois, 5, A03, 0)
    assert [tb["d"][6] for tb in tbs] == [265, 334]
    assert ro[:, 6, 0].tolist() == [265, 334] and ro[:, 6, 1].tolist() == [512, 512]
    for i, tb in enumerate(tbs):
        assert tb["m"] != tb["n"]
        assert not d[i, :, tb["d"][6]:].any() and not t[i, tb["d"][6]:].any() and not r[i, :, tb["d"][6]:].any()
        # values stay inside each segment's own range
        for k in range(6):
            src = data[i, 0, tb["c"][k]:tb["c"][k + 1]]
            out = d[i, 0, tb["d"][k]:tb["d"][k + 1]]
            assert out.min() >= src.min() and out.max() <= src.max()


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
@pytest.mark.parametrize("J", [0, 3, 64])
def test_any_rois_give_contiguous_monotone_marks(name, J):
    L = 64
    rng = np.random.default_rng(1)
    data = rng.random((1, 2, L), dtype=np.float32) + 1.0      # in [1, 2): a written zero is told from a copied sample
    target = rng.random((1, L), dtype=np.float32) + 1.0
    rois = adversarial_rois(name, L)
    for seed in range(8):
        d, t, _, ro, tbs = ref.warp(data, target, None, rois, seed, A03, J)
        tb = tbs[0]
        e = ro[0, :, 0].tolist()
        assert all(0 <= v <= L for v in e) and e == sorted(e)
        assert ro[0, :6, 1].tolist() == e[1:] and ro[0, 6, 1] == rois[0, 6, 1]
        assert e[0] == tb["d"][0] and e[6] == tb["d"][6]
        assert all(abs(e[k] - tb["d"][k]) <= J for k in range(1, 6))
        if J == 0:
            assert e == tb["d"]
        assert not d[0, :, e[6]:].any() and not t[0, e[6]:].any()
        live = np.concatenate([d[0].reshape(-1), t[0]])
        assert live.min() >= 0.0 and live.max() <= max(data.max(), target.max())
        assert np.array_equal(d[0, :, :e[0]], data[0, :, :e[0]])
        if tb["c"][6] == L:                                    # a cropped beat keeps its samples bit for bit
            assert tb["m"] == tb["n"]
            assert np.array_equal(bits(d[0, :, tb["c"][0]:]), bits(data[0, :, tb["c"][0]:]))


def test_long_beat_is_sometimes_cut_at_the_row_end():
    L = 512
    rois = np.zeros((1, 7, 2), dtype=np.int64)
    rois[0, :, 0] = [0, 80, 110, 190, 260, 400, 500]
    rois[0, :6, 1] = rois[0, 1:, 0]
    rois[0, 6, 1] = L
    x = np.linspace(0.0, 1.0, L, dtype=np.float32)[None, None]
    cut = 0
    for seed in range(300):
        tb = ref.tables(rois[0], L, seed, 0, A03, 0)
        uncut = tb["c"][0] + sum(tb["m"])
        assert tb["d"][6] == min(uncut, L)
        cut += uncut > L
    assert 0 < cut < 300, cut
    seed = next(s for s in range(300) if sum(ref.tables(rois[0], L, s, 0, A03, 0)["m"]) > L)
    d, _, _, ro, tbs = ref.warp(x, x[:, 0], None, rois, seed, A03, 0)
    assert ro[0, 6, 0] == L and np.all(np.diff(d[0, 0]) >= 0) and d[0, 0, -1] < x[0, 0, 499]   # the mapping uses the uncut lengths


@pytest.mark.parametrize("L,starts", [(4, [0, 1, 1, 2, 3, 3, 4]), (4, [0, 1, 2, 3, 3, 3, 3]), (8, [0, 1, 2, 3, 4, 5, 6]),
                                      (8, [2, 2, 2, 2, 2, 2, 2]), (8, [0, 0, 0, 7, 7, 8, 8])])
def test_tiny_rows_one_sample_and_empty_segments(L, starts):
    rois = np.zeros((1, 7, 2), dtype=np.int64)
    rois[0, :, 0] = starts
    rois[0, :6, 1] = starts[1:]
    rois[0, 6, 1] = L
    x = (np.arange(L, dtype=np.float32) + 1.0)[None, None]
    for seed in range(16):
        d, t, _, ro, tbs = ref.warp(x, x[:, 0], None, rois, seed, (0.9,) * 6, 2)
        tb = tbs[0]
        assert all(m == 0 for m, n in zip(tb["m"], tb["n"]) if n == 0) and all(m >= 1 for m, n in zip(tb["m"], tb["n"]) if n > 0)
        e = ro[0, :, 0].tolist()
        assert e == sorted(e) and 0 <= e[0] and e[6] <= L and not d[0, 0, e[6]:].any()
        assert np.array_equal(d[0, 0], t[0])
        for k in range(6):                                    # a one-sample segment is that sample, however long it becomes
            if tb["n"][k] == 1:
                assert np.all(d[0, 0, tb["d"][k]:tb["d"][k + 1]] == x[0, 0, tb["c"][k]])
    d, _, _, ro, _ = ref.warp(x, x[:, 0], None, rois, 0, ZERO, 0)
    c6 = min(starts[6], L)
    assert np.array_equal(d[0, 0, :c6], x[0, 0, :c6]) and not d[0, 0, c6:].any()


def test_draw_statistics():
    J = 5
    z = np.array([ref.draws(77, i) for i in range(4096)], dtype=object)
    u = np.array([[ref.uniform(w) for w in row] for row in z], dtype=np.float64)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert np.all(np.abs(u.mean(axis=0) - 0.5) < 0.02), u.mean(axis=0)
    for k in range(1, 6):
        assert {ref.jitter_of(w, J) for w in z[:, k]} == set(range(-J, J + 1))
    assert {ref.jitter_of(w, 64) for w in z.reshape(-1)} == set(range(-64, 65))
    assert {ref.jitter_of(w, 0) for w in z[:64, 1]} == {0}


def test_a_sample_depends_on_seed_index_and_its_own_rows():
    data, target, rest, rois = golden()
    full = ref.warp(data, target, rest, rois, 9, A03, 3, index0=10)
    one = ref.warp(data[1:], target[1:], rest[1:], rois[1:], 9, A03, 3, index0=11)
    for a, b in zip(full[:4], one[:4]):
        assert np.array_equal(a[1:], b)
    other = ref.warp(data[1:], target[1:], rest[1:], rois[1:], 9, A03, 3, index0=12)
    assert not np.array_equal(other[3], one[3])


def test_defaults_are_off():
    from electrocardio_panorama_amd import warp
    cfg = _cfg()
    assert cfg.DATA["aug_warp"] == [] and cfg.DATA["aug_roi_jitter"] == 0 and cfg.DATA["aug_warp_eval"] is False
    assert warp.from_cfg(cfg) is None
    assert warp.from_cfg(_cfg(aug_warp=[0, 0, 0, 0, 0, 0], aug_warp_eval=True)) is None
    assert warp.from_cfg(_cfg(aug_warp=[0.0] * 6, noise=True)) is None            # nothing on: DATA.noise is not in the way


def test_from_cfg_carries_the_keys():
    from electrocardio_panorama_amd import warp
    w = warp.from_cfg(_cfg(aug_warp=[0.1, 0.2, 0, 0.3, 0.9, 0.05], aug_roi_jitter=4, aug_warp_eval=True))
    assert w == warp.Warp((0.1, 0.2, 0.0, 0.3, 0.9, 0.05), 4, True)
    assert warp.from_cfg(_cfg(aug_roi_jitter=64)) == warp.Warp((0.0,) * 6, 64, False)
    assert warp.from_cfg(_cfg(aug_warp=(0.3,) * 6)).jitter == 0
    assert "aug_warp" in w.describe() and "aug_roi_jitter 4" in w.describe()


@pytest.mark.parametrize("key,data", [
    ("aug_warp", dict(aug_warp=[0.1] * 5)),
    ("aug_warp", dict(aug_warp=[0.1] * 7)),
    ("aug_warp", dict(aug_warp=0.3)),
    ("aug_warp", dict(aug_warp=[0.1, True, 0.1, 0.1, 0.1, 0.1])),
    ("aug_warp", dict(aug_warp=[0.1, float("nan"), 0.1, 0.1, 0.1, 0.1])),
    ("aug_warp", dict(aug_warp=[0.1, -0.1, 0.1, 0.1, 0.1, 0.1])),
    ("aug_warp", dict(aug_warp=[0.1, 0.91, 0.1, 0.1, 0.1, 0.1])),
    ("aug_warp", dict(aug_warp=[0.1, float("inf"), 0.1, 0.1, 0.1, 0.1])),
    ("aug_warp", dict(aug_warp=[0.1, "0.2", 0.1, 0.1, 0.1, 0.1])),
    ("aug_roi_jitter", dict(aug_roi_jitter=-1)),
    ("aug_roi_jitter", dict(aug_roi_jitter=65)),
    ("aug_roi_jitter", dict(aug_roi_jitter=True)),
    ("aug_roi_jitter", dict(aug_roi_jitter=2.0)),
    ("noise", dict(aug_warp=[0.3] * 6, noise=True)),
    ("noise", dict(aug_roi_jitter=1, noise=True)),
], ids=["five", "seven", "scalar", "bool", "nan", "negative", "above_09", "inf", "string", "J_neg", "J_65", "J_bool", "J_float",
        "noise_warp", "noise_jitter"])
def test_rejections_name_the_key(key, data):
    from electrocardio_panorama_amd import warp
    with pytest.raises(ValueError, match="DATA." + key):
        warp.from_cfg(_cfg(**data))


def test_seeds():
    from electrocardio_panorama_amd import augment, engine, warp
    n = len(engine.DROPOUT_SITES)
    assert warp.train_seed(0, 0, 0, 0) == (n + 2) * 0x85EBCA6B + 1
    assert warp.eval_seed(0, 0, 0) == (n + 3) * 0x85EBCA6B + 1 + augment._EVAL_BIT
    seen = set()
    for epoch in range(3):
        for index in range(4):
            for rank in range(3):
                seen.add(warp.train_seed(123, epoch, index, rank))
                seen.add(warp.eval_seed(123, index, rank) if epoch == 0 else warp.train_seed(124, epoch, index, rank))
    assert len(seen) == 3 * 4 * 3 * 2
    assert warp.train_seed(123, 2, 3, 1) == warp.train_seed(123, 2, 3, 1)
    assert warp.eval_seed(123, 0) >> 48 == 1 and warp.train_seed(2 ** 40, 10 ** 6, 10 ** 6, 7) >> 48 == 0
    # under sites of their own: neither a dropout site's word, nor nef_augment's two
    words = {k * 0x85EBCA6B + 1 for k in range(n)} | {augment.site_word(), augment.site_word(read_out=True)}
    assert warp.train_seed(0, 0, 0) not in words and warp.eval_seed(0, 0) not in words


def test_seeds_leave_the_global_random_states_alone():
    import random
    from electrocardio_panorama_amd import warp
    s0, n0 = random.getstate(), np.random.get_state()[1].copy()
    warp.train_seed(1, 2, 3, 0), warp.eval_seed(1, 2, 0), warp.from_cfg(_cfg(aug_roi_jitter=2))
    assert random.getstate() == s0 and np.array_equal(np.random.get_state()[1], n0)


def test_ops_warp_checks_its_arguments_before_the_library(monkeypatch):
    from electrocardio_panorama_amd import _lib, ops, warp

    def touched():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)
    w = warp.Warp((0.3,) * 6, 2, False)
    d, t, r = torch.zeros(2, 3, 8), torch.zeros(2, 8), torch.zeros(2, 9, 8)
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    out = ops.warp(d, t, r, rois, None, 0)
    assert out[0] is d and out[1] is t and out[2] is r and out[3] is rois     # off: the tensors themselves
    assert ops.warp(d.double(), t, None, rois, None, 0)[0].dtype == torch.float64 and ops.warp(d, t, None, rois, None, 0)[2] is None
    with pytest.raises(TypeError, match="data must be a float32"):
        ops.warp(d.double(), t, r, rois, w, 0)
    with pytest.raises(TypeError, match="target must be a float32"):
        ops.warp(d, t.double(), r, rois, w, 0)
    with pytest.raises(TypeError, match="rest must be a float32"):
        ops.warp(d, t, r.double(), rois, w, 0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.warp(d.transpose(0, 1), t, r, rois, w, 0)
    with pytest.raises(ValueError, match=r"\[B, V, L\]"):
        ops.warp(d[0], t, r, rois, w, 0)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.warp(torch.zeros(2, 3, 6), torch.zeros(2, 6), None, rois, w, 0)
    with pytest.raises(ValueError, match="V in 1..12"):
        ops.warp(torch.zeros(2, 13, 8), t, None, rois, w, 0)
    with pytest.raises(ValueError, match="target"):
        ops.warp(d, torch.zeros(2, 2, 8), r, rois, w, 0)
    with pytest.raises(ValueError, match="target"):
        ops.warp(d, torch.zeros(2, 4), r, rois, w, 0)
    with pytest.raises(ValueError, match="rest"):
        ops.warp(d, t, torch.zeros(1, 9, 8), rois, w, 0)
    with pytest.raises(ValueError, match="rest"):
        ops.warp(d, t, torch.zeros(2, 65, 8), rois, w, 0)
    with pytest.raises(TypeError, match="integer"):
        ops.warp(d, t, r, rois.float(), w, 0)
    with pytest.raises(TypeError, match="integer"):
        ops.warp(d, t, r, None, w, 0)
    with pytest.raises(ValueError, match="rois"):
        ops.warp(d, t, r, torch.zeros(2, 6, 2, dtype=torch.int64), w, 0)
    with pytest.raises(ValueError, match="rois"):
        ops.warp(d, t, r, rois[:1], w, 0)
    with pytest.raises(ValueError, match="amp"):
        ops.warp(d, t, r, rois, warp.Warp((0.3,) * 5 + (1.0,), 0, False), 0)
    with pytest.raises(ValueError, match="jitter"):
        ops.warp(d, t, r, rois, warp.Warp((0.3,) * 6, 65, False), 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.warp(d, t, r, rois, w, 0)                          # CPU tensors, everything else right: still in front of the library
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.warp(d, t.unsqueeze(1), None, rois.to(torch.int32), w, 0)


def test_header_binding_and_library_agree():
    from electrocardio_panorama_amd import _lib
    text = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    body = re.search(r"typedef struct nef_warp_args \{(.*?)\} nef_warp_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = decl.split(",")
        names.append(re.sub(r"\[\d+\]", "", first.split()[-1].lstrip("*")))
        names += [m.strip() for m in more]
    assert names == [f[0] for f in _lib.WarpArgs._fields_]
    assert "int nef_warp(const nef_warp_args* a, nef_stream_t stream);" in text and "size_t nef_warp_args_bytes(void);" in text
    for name in ("nef_warp", "nef_warp_args_bytes"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.nef_warp_args_bytes() == ctypes.sizeof(_lib.WarpArgs) == 8 * 8 + 16 + 48 + 6 * 4
    assert lib.nef_abi_version() == 22                        # an addition: the number stays


def test_library_rejects_in_front_of_the_launch():
    """No device is touched: every call is turned away by a check in front of the launch."""
    from electrocardio_panorama_amd import _lib
    lib = _lib.load()

    def call(**kw):
        base = dict(data=0x1000, target=0x2000, rest=0x3000, rois=0x4000, data_out=0x11000, target_out=0x12000, rest_out=0x13000,
                    rois_out=0x14000, seed=1, index0=0, amp=(ctypes.c_double * 6)(*[0.3] * 6), jitter=2, B=1, V=3, R=9, L=8)
        base.update(kw)
        return lib.nef_warp(ctypes.byref(_lib.WarpArgs(**base)), None)

    assert lib.nef_warp(None, None) == -2
    for ptr in ("data", "target", "rois", "data_out", "target_out", "rois_out", "rest", "rest_out"):
        assert call(**{ptr: None}) == -2, ptr
    for kw in (dict(L=6), dict(L=0), dict(L=(1 << 24) + 4), dict(V=0), dict(V=13), dict(R=-1), dict(R=65), dict(B=0), dict(jitter=-1),
               dict(jitter=65), dict(amp=(ctypes.c_double * 6)(0.3, 0.3, 0.91, 0.3, 0.3, 0.3)),
               dict(amp=(ctypes.c_double * 6)(0.3, -0.1, 0.3, 0.3, 0.3, 0.3)),
               dict(amp=(ctypes.c_double * 6)(0.3, 0.3, 0.3, 0.3, 0.3, float("nan")))):
        assert call(**kw) == -1, list(kw)
    for kw in (dict(data=0x1004), dict(rois_out=0x14008), dict(target_out=0x12004), dict(data_out=0x1000), dict(data_out=0x1010),
               dict(target_out=0x1000 + 32), dict(rois_out=0x4000 + 16), dict(rest_out=0x2000)):
        assert call(**kw) == -4, kw
