"""CPU: the wave-segment weights of the reconstruction term (SOLVER.seg_weights) and the per-segment read-out (SOLVER.seg_eval) -- the
restatement tests/seg_ref.py pinned to the interval definition on every golden rois array and to a literal per-position loop on hand-made
ones, its autograd gradient against the closed form the backward kernel implements, seg_settings' accept / reject rules, the C-ABI
entries in the header, the binding table and the library, and their argument checks (no GPU work)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import seg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nef_loss_seg_fwd", "nef_loss_seg_bwd", "nef_view_seg_metrics", "nef_loss_seg_ws_bytes", "nef_loss_seg_args_bytes")
WEIGHTS = (0.5, 1.25, 3.0, 2.0, 0.75, 1.5, 0.25)


class Cfg(dict):
    __getattr__ = dict.__getitem__


# ------------------------------------------------------------------------------------------------ the segment of a position
def _golden_rois(golden_dir):
    """(name, rois [B, 7, 2], L) of every rois array under tests/golden."""
    out = []
    z = np.load(os.path.join(golden_dir, "real_tianchi_B2_V3.npz"))
    out.append(("real_tianchi_B2_V3", z["rois"], int(z["data"].shape[-1])))
    z = np.load(os.path.join(golden_dir, "roi_cases.npz"))
    for name in ("real512", "mod4_512", "len5000", "len1000"):
        out.append((f"roi_cases:{name}", z[f"{name}:rois"], int(z[f"{name}:L"])))
    z = np.load(os.path.join(golden_dir, "ptb_synth.npz"))
    for c in range(5):
        out.append((f"ptb_synth:cfg{c}", z[f"cfg{c}/rois"], int(z[f"cfg{c}/data"].shape[-1])))
    return out


def test_seg_index_equals_the_interval_definition_on_every_golden_rois(golden_dir):
    """Contiguous rois with non-decreasing starts: the segment of t is the one k with rois[i, k, 0] <= t < rois[i, k, 1]."""
    cases = _golden_rois(golden_dir)
    assert len(cases) == 10 and sum(r.shape[0] for _, r, _ in cases) == 2 + 2 + 2 + 2 + 1 + 5 * 12
    for name, rois, L in cases:
        assert rois.dtype == np.int64 and rois.shape[1:] == (7, 2)
        assert (rois[:, 0, 0] == 0).all() and (rois[:, 6, 1] == L).all(), name
        assert (rois[:, 1:, 0] == rois[:, :-1, 1]).all() and (np.diff(rois[:, :, 0], axis=1) >= 0).all(), name      # contiguous
        got = seg_ref.seg_index(rois, L)
        assert got.shape == (rois.shape[0], L) and got.dtype == np.int64
        for i in range(rois.shape[0]):
            for t in range(L):
                ks = [k for k in range(7) if rois[i, k, 0] <= t < rois[i, k, 1]]
                assert len(ks) == 1 and got[i, t] == ks[0], (name, i, t, ks, got[i, t])


HAND_L = 40
HAND = {
    "plain": [0, 5, 9, 14, 20, 27, 33],
    "negative_starts": [0, -7, -1, 3, 8, 12, 30],
    "beyond_L": [0, 10, 20, 45, 1000, 2 ** 40, 39],
    "non_monotonic": [0, 30, 10, 25, 5, 15, 36],
    "equal_starts": [0, 8, 8, 8, 20, 20, 20],
    "end_zero": [0, 3, 6, 9, 12, 15, 0],
    "end_negative": [0, 3, 6, 9, 12, 15, -4],
    "end_beyond_L": [0, 3, 6, 9, 12, 15, 77],
    "end_in_front_of_starts": [0, 30, 32, 34, 36, 38, 10],
    "all_beyond": [0, 50, 60, 70, 80, 90, 100],
    "int64_extremes": [0, -2 ** 62, 2 ** 62, -1, 40, 39, 40],
}


def _hand_rois():
    r = np.zeros((len(HAND), 7, 2), dtype=np.int64)
    r[:, :, 0] = np.array(list(HAND.values()), dtype=np.int64)
    r[:, :, 1] = -123           # the second column is never read
    return r


def test_seg_index_equals_a_literal_loop_on_hand_made_rois():
    rois, L = _hand_rois(), HAND_L
    got = seg_ref.seg_index(rois, L)
    seen = set()
    for i, name in enumerate(HAND):
        end = min(max(int(rois[i, 6, 0]), 0), L)
        for t in range(L):
            want = 6 if t >= end else sum(1 for k in range(1, 6) if int(rois[i, k, 0]) <= t)
            assert got[i, t] == want, (name, t, got[i, t], want)
            seen.add(want)
    assert seen == set(range(7))
    assert (got[list(HAND).index("end_zero")] == 6).all() and (got[list(HAND).index("end_negative")] == 6).all()
    assert (got[list(HAND).index("all_beyond")] == 0).all()
    # torch rois are taken too, and the weight map is the weights at that index, in fp32
    assert np.array_equal(seg_ref.seg_index(torch.from_numpy(rois), L), got)
    W = seg_ref.weight_map(rois, L, WEIGHTS)
    assert W.dtype == np.float32 and np.array_equal(W, np.asarray(WEIGHTS, dtype=np.float32)[got])


# ------------------------------------------------------------------------------------------------ the weighted term and its gradient
@pytest.mark.parametrize("reg_l2", [False, True], ids=["l1", "l2"])
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noise"])
def test_autograd_of_seg_term_equals_the_closed_form(reg_l2, noisy):
    """d term / d pred = f2 * w * sign(d) / n (l1) and f2 * w * 2 d / n (l2): what nef_loss_seg_bwd's multiply makes of loss_bwd's
    gradient.  fp64 inputs: the bar is 1e-12."""
    rois, L = _hand_rois(), HAND_L
    B = rois.shape[0]
    gen = torch.Generator().manual_seed(3)
    pred, tgt = (torch.rand(B, 1, L, generator=gen, dtype=torch.float64) / 3 for _ in range(2))
    nz = torch.randn(B, 1, L, generator=gen, dtype=torch.float64) * 0.01 if noisy else None
    x = pred.clone().requires_grad_(True)
    f2 = 0.75
    term = seg_ref.seg_term(x, tgt, rois, WEIGHTS, f2, reg_l2, noise=nz)
    assert term.dtype == torch.float64 and term.dim() == 0
    term.backward()
    d = (pred + nz if noisy else pred) - tgt
    W = torch.from_numpy(seg_ref.weight_map(rois, L, WEIGHTS).astype(np.float64)).reshape(B, 1, L)
    n = B * L
    want = f2 * W * (2.0 * d if reg_l2 else torch.sign(d)) / n
    assert float((x.grad - want).abs().max()) <= 1e-12
    assert float(x.grad.abs().max()) > 0
    # all ones is the flat mean; a weight of 3 counts a position three times; no renormalisation
    e = d * d if reg_l2 else d.abs()
    assert abs(float(seg_ref.seg_term(pred, tgt, rois, [1.0] * 7, 1.0, reg_l2, noise=nz)) - float(e.mean())) <= 1e-15
    assert abs(float(seg_ref.seg_term(pred, tgt, rois, [3.0] * 7, 1.0, reg_l2, noise=nz)) - 3.0 * float(e.mean())) <= 1e-15
    # multi-view rows: [Q, B, 1, L] with the rois tiled per view is the mean over all Q * B * L elements
    two = seg_ref.seg_term(torch.stack([pred, pred]), torch.stack([tgt, tgt]), np.concatenate([rois, rois]), WEIGHTS, f2, reg_l2,
                           noise=None if nz is None else torch.stack([nz, nz]))
    assert abs(float(two) - float(term.detach())) <= 1e-15


def test_seg_sums_add_up_to_the_row():
    rois, L = _hand_rois(), HAND_L
    B = rois.shape[0]
    gen = torch.Generator().manual_seed(4)
    x, y = (torch.rand(B, 3, L, generator=gen) / 3 for _ in range(2))
    se, cnt = seg_ref.seg_sums(x, y, rois)
    assert se.shape == cnt.shape == (B, 3, 7) and (cnt.sum(-1) == L).all()
    d2 = (x.double() - y.double()) ** 2
    assert np.abs(se.sum(-1) - d2.sum(-1).numpy()).max() <= 1e-12
    idx = seg_ref.seg_index(rois, L)
    for k in range(7):
        assert (cnt[:, 0, k] == (idx == k).sum(-1)).all() and (cnt[:, 0] == cnt[:, 2]).all()
    assert seg_ref.seg_psnr(0.0, 5) == 100.0 and abs(seg_ref.seg_psnr(0.04, 4) - 20.0) <= 1e-12


# ------------------------------------------------------------------------------------------------ config
def _cfg(using=(1, 2, 3), **solver):
    base = dict(optim="sgd", lr=0.1, reg_loss="l1_loss", loss_using=list(using), loss_factor=[0.5, 0.5, 1])
    base.update(solver)
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=3, noise=False), SOLVER=Cfg(**base))


def test_config_defaults_are_off():
    from electrocardio_panorama_amd.config import get_defaults
    cfg = get_defaults()
    assert list(cfg.SOLVER.seg_weights) == [] and cfg.SOLVER.seg_eval is False


def test_seg_settings_accepts_and_rejects():
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.network.loss.losses import SEG_NAMES, seg_settings
    assert SEG_NAMES == ('P', 'PR', 'QRS', 'ST', 'T', 'TP', 'pad')
    assert seg_settings(_cfg()) is None                                     # a config written before the key existed
    assert seg_settings(_cfg(seg_weights=[])) is None and seg_settings(_cfg(seg_weights=())) is None
    assert seg_settings(_cfg(using=(1, 2), seg_weights=[])) is None         # off: loss_using is not looked at
    w = seg_settings(_cfg(seg_weights=[1, 1, 3, 2, 1, 1, 0]))
    assert w == (1.0, 1.0, 3.0, 2.0, 1.0, 1.0, 0.0) and all(isinstance(x, float) for x in w)
    assert seg_settings(_cfg(seg_weights=(0, 0, 0, 0, 0, 0, 1e-3))) == (0.0,) * 6 + (1e-3,)
    assert seg_settings(_cfg(using=(3,), seg_weights=[1] * 7)) == (1.0,) * 7
    bad = {"length 6": [1] * 6, "length 8": [1] * 8, "length 1": [2.0], "negative": [1, 1, -0.5, 1, 1, 1, 1], "nan": [1, 1, math.nan, 1, 1, 1, 1],
           "inf": [1, 1, math.inf, 1, 1, 1, 1], "all zero": [0] * 7}
    for name, v in bad.items():
        with pytest.raises(ValueError, match="seg_weights"):
            seg_settings(_cfg(seg_weights=v))
        with pytest.raises(ValueError, match="seg_weights"):
            build_loss(_cfg(seg_weights=v))                                  # rejected where the loss is built, not at the first batch
    with pytest.raises(ValueError, match="seg_weights.*loss_using|loss_using.*seg_weights"):
        seg_settings(_cfg(using=(1, 2), seg_weights=[1] * 7))
    assert build_loss(_cfg()) is build_loss(_cfg(seg_weights=[1, 1, 3, 2, 1, 1, 0]))


def test_losswrapper_needs_rois_with_the_key_on_before_any_device_work():
    """CPU tensors: the ValueError comes before the first launch (which would reject them)."""
    from electrocardio_panorama_amd.network import losswrapper
    t = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="seg_weights"):
        losswrapper(t, t, t, t, _cfg(seg_weights=[1, 1, 3, 2, 1, 1, 0]))
    with pytest.raises(ValueError, match="seg_weights"):
        losswrapper(t, t, t, t, _cfg(seg_weights=[1] * 6), rois=torch.zeros(2, 7, 2, dtype=torch.int64))


def test_losswrapper_call_order_and_tuple_lengths(monkeypatch):
    """Key off or absent: only ops.loss_fwd is called, on its own 4-element row.  Key on: loss_seg_fwd sits behind loss_fwd on the same
    row and in front of loss_ssim_fwd; the tuple keeps its length; [B, 7, 2] rois are tiled once per view, [Q * B, 7, 2] taken as is."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.network import losswrapper
    calls = []

    def fake_fwd(pred, pp, pl, tgt, factors, reg_l2, use_mask, out=None, noise=None):
        calls.append(("loss_fwd", None if out is None else out.numel()))
        row = torch.zeros(4) if out is None else out
        row[:4] = torch.arange(4, dtype=torch.float32)
        return row

    def fake_seg(pred, tgt, losses, weights, f2, reg_l2, rois, noise=None):
        calls.append(("loss_seg_fwd", losses.numel(), tuple(weights), f2, bool(reg_l2), tuple(rois.shape), rois.dtype))
        losses[3] = 7.0
        return losses

    def fake_ssim(pred, tgt, losses, factor, rois=None, noise=None):
        calls.append(("loss_ssim_fwd", losses.numel()))
        losses[4] = 9.0
        return losses

    monkeypatch.setattr(ops, "loss_fwd", fake_fwd)
    monkeypatch.setattr(ops, "loss_seg_fwd", fake_seg)
    monkeypatch.setattr(ops, "loss_ssim_fwd", fake_ssim)
    t = torch.zeros(2, 1, 16)
    rois = torch.zeros(2, 7, 2, dtype=torch.int32)
    for cfg in (_cfg(), _cfg(seg_weights=[], seg_eval=False)):
        for kw in ({}, {"rois": rois}):
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, **kw)) == 4
            assert calls == [("loss_fwd", None)]
    W = [1, 1, 3, 2, 1, 1, 0]
    Wf = tuple(float(x) for x in W)
    calls.clear()
    row = losswrapper(t, t, t, t, _cfg(seg_weights=W), rois=rois)
    assert len(row) == 4 and float(row[3]) == 7.0
    assert calls == [("loss_fwd", 4), ("loss_seg_fwd", 4, Wf, 1.0, False, (2, 7, 2), torch.int64)]
    calls.clear()
    assert len(losswrapper(t, t, t, t, _cfg(seg_weights=W), t, t, rois=rois)) == 5          # the test form: + loss_unsperv
    assert calls[:2] == [("loss_fwd", 4), ("loss_seg_fwd", 4, Wf, 1.0, False, (2, 7, 2), torch.int64)] and calls[2:] == [("loss_fwd", None)]
    calls.clear()
    row = losswrapper(t, t, t, t, _cfg(seg_weights=W, ssim_factor=0.5, reg_loss="l2_loss"), rois=rois)
    assert len(row) == 5 and float(row[3]) == 7.0 and float(row[4]) == 9.0
    assert calls == [("loss_fwd", 5), ("loss_seg_fwd", 5, Wf, 1.0, True, (2, 7, 2), torch.int64), ("loss_ssim_fwd", 5)]
    # multi-view
    q = torch.zeros(3, 2, 1, 16)
    for r in (rois, rois.repeat(3, 1, 1)):
        calls.clear()
        losswrapper(q, q, q, q, _cfg(seg_weights=W), rois=r)
        assert calls[1][5] == (6, 7, 2)


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    from electrocardio_panorama_amd import _lib, ops
    from electrocardio_panorama_amd.csrc import build
    assert "loss_seg.hip" in build.SOURCES
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    for fn in ("nef_loss_seg_fwd", "nef_loss_seg_bwd"):
        assert re.search(r"\bint " + fn + r"\s*\(\s*const nef_loss_seg_args\s*\*\s*a,\s*nef_stream_t stream\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_seg_ws_bytes\s*\(\s*int B,\s*int L\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_seg_args_bytes\s*\(\s*void\s*\)", hdr)
    assert re.search(r"\bint nef_view_seg_metrics\s*\(\s*const float\s*\*\s*pred,\s*const float\s*\*\s*gt,\s*const int64_t\s*\*\s*rois,\s*"
                     r"double\s*\*\s*se,\s*int32_t\s*\*\s*cnt,\s*int B,\s*int Q,\s*int L,\s*nef_stream_t stream\s*\)", hdr)
    body = hdr[hdr.index("typedef struct nef_loss_seg_args"):hdr.index("} nef_loss_seg_args;")]
    assert re.findall(r"(\w+)(?:\[7\])?;\s*/\*", body) == [n for n, _ in _lib.LossSegArgs._fields_]
    L = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert L.nef_abi_version() == 22                                       # additions only
    assert ctypes.sizeof(_lib.LossSegArgs) == L.nef_loss_seg_args_bytes() == 112
    tile = int(re.search(r"#define NEF_LOSS_SEG_TILE (\d+)", hdr).group(1))
    assert tile == ops.LOSS_SEG_TILE == 1024
    assert L.nef_loss_seg_ws_bytes(4, tile) == 4 * 8 and L.nef_loss_seg_ws_bytes(4, tile + 4) == 4 * 2 * 8
    assert L.nef_loss_seg_ws_bytes(256, 5000) == 256 * 5 * 8
    assert L.nef_loss_seg_ws_bytes(0, 16) == 0 and L.nef_loss_seg_ws_bytes(3, -4) == 0


def test_a_binding_with_another_struct_size_is_rejected(monkeypatch):
    """The struct-size check of _lib.load: a library whose nef_loss_seg_args is not the mirror's size is told to rebuild."""
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)

    class Long(ctypes.Structure):
        _fields_ = _lib.LossSegArgs._fields_ + [("more", ctypes.c_void_p)]

    assert ctypes.sizeof(Long) != ctypes.sizeof(_lib.LossSegArgs)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LossSegArgs", Long)
    with pytest.raises(_lib.NefLibraryError, match="nef_loss_seg_args"):
        _lib.load()


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(pred=64, target=64, noise=None, rois=64, losses=64, g_pred=64, ws=64, ws_bytes=1 << 20, B=4, L=512, reg_l2=0, f2=1.0)
    w = kw.pop("w", (1, 1, 3, 2, 1, 1, 0))
    a.update(kw)
    return _lib.LossSegArgs(w=(ctypes.c_float * 7)(*w), **a)


def test_entries_reject_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the launches: nothing is launched and no address is read (non-NULL, never dereferenced pointers)."""
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)
    lib = _lib.load()
    fwd = lambda **kw: lib.nef_loss_seg_fwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    bwd = lambda **kw: lib.nef_loss_seg_bwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    NULL, SHAPE, WS, UNSUPPORTED = -2, -1, -3, -4
    assert lib.nef_loss_seg_fwd(None, None) == NULL and lib.nef_loss_seg_bwd(None, None) == NULL
    assert fwd(pred=None) == NULL and fwd(target=None) == NULL and fwd(losses=None) == NULL and bwd(g_pred=None) == NULL
    for call in (fwd, bwd):
        assert call(rois=None) == NULL
        for key in ("B", "L"):
            for bad in (0, -4):
                assert call(**{key: bad}) == SHAPE, (key, bad)
        assert call(B=65536) == SHAPE
        for bad in (510, 511, 513, 2):
            assert call(L=bad) == SHAPE, bad
        for bad in (-0.5, math.nan, math.inf):
            assert call(w=(1, 1, bad, 1, 1, 1, 1)) == SHAPE, bad
    need = lib.nef_loss_seg_ws_bytes(4, 512)
    assert need == 32
    assert fwd(ws_bytes=need - 1) == WS and fwd(ws_bytes=0, ws=None) == WS
    assert fwd(ws=None) == NULL
    # a NULL pointer wins over a bad shape, a bad shape over a small workspace, the workspace over the alignment
    assert fwd(pred=None, B=0) == NULL and fwd(B=0, ws_bytes=0) == SHAPE and fwd(pred=68, ws_bytes=0) == WS
    assert fwd(pred=68) == UNSUPPORTED and fwd(target=72) == UNSUPPORTED and fwd(noise=8) == UNSUPPORTED and bwd(g_pred=68) == UNSUPPORTED

    def vm(pred=64, gt=64, rois=64, se=64, cnt=64, B=2, Q=3, L=512):
        return lib.nef_view_seg_metrics(pred, gt, rois, se, cnt, B, Q, L, None)

    for key in ("pred", "gt", "rois", "se", "cnt"):
        assert vm(**{key: None}) == NULL, key
    for key in ("B", "Q", "L"):
        for bad in (0, -4):
            assert vm(**{key: bad}) == SHAPE, (key, bad)
    assert vm(B=65536) == SHAPE and vm(L=510) == SHAPE and vm(L=513) == SHAPE
    assert vm(pred=68) == UNSUPPORTED and vm(gt=72) == UNSUPPORTED
    assert vm(pred=None, B=0) == NULL


def test_ops_wrappers_reject_malformed_weights_before_any_launch():
    from electrocardio_panorama_amd import ops
    for bad in ([1] * 6, [1] * 8, [1, 1, -1, 1, 1, 1, 1], [1, 1, math.nan, 1, 1, 1, 1], [1, 1, math.inf, 1, 1, 1, 1]):
        with pytest.raises(ValueError):
            ops._seg_weights(bad)
    assert list(ops._seg_weights([1, 1, 3, 2, 1, 1, 0])) == [1.0, 1.0, 3.0, 2.0, 1.0, 1.0, 0.0]
