"""CPU: the slope term of the training loss (SOLVER.slope_factor) -- the fp64 restatement tests/slope_ref.py pinned to a literal Python
loop and its autograd gradient to the closed form the backward kernel implements, the C-ABI entries in the header, the binding table and
the library, their argument checks (no GPU work), the config keys and their ValueErrors, and losswrapper's tuple with the keys off."""
import ctypes
import math
import os
import re

import pytest
import torch

import slope_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fp64 throughout; the restatements differ in the order of a row's sum only
BAR = 1e-12
ENTRIES = ("nef_loss_slope_fwd", "nef_loss_slope_bwd", "nef_loss_slope_ws_bytes", "nef_loss_slope_args_bytes", "nef_view_slope_metrics")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _rows(B, L, seed):
    """Uniform in [0, 1/3]: the decoder's output range is sigmoid / 3."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, L, generator=g, dtype=torch.float64) / 3, torch.rand(B, L, generator=g, dtype=torch.float64) / 3)


CASES = [(1, 1, [1]), (1, 2, [2]), (2, 13, [13, 13]), (4, 40, [33, 1, 0, 40]), (3, 500, [298, 2, 500]), (1, 512, [440])]
IDS = [f"B{b}_L{l}" for b, l, _ in CASES]


def _loop_term(x, y, factor, l2, ends):
    """The definition, literally."""
    total, R = 0.0, 0
    for i, e in enumerate(ends):
        if e < 2:
            continue
        s = 0.0
        for t in range(e - 1):
            d = (float(x[i, t + 1]) - float(x[i, t])) - (float(y[i, t + 1]) - float(y[i, t]))
            s += d * d if l2 else abs(d)
        total += s / (e - 1)
        R += 1
    return factor * total / R if R else 0.0


@pytest.mark.parametrize("l2", [False, True], ids=["l1", "l2"])
@pytest.mark.parametrize("B,L,ends", CASES, ids=IDS)
def test_restatement_equals_the_literal_loop(B, L, ends, l2):
    x, y = _rows(B, L, 7 * L + B)
    want = _loop_term(x, y, 5.0, l2, ends)
    got = float(slope_ref.slope_term(x, y, 5.0, l2, ends))
    assert abs(got - want) <= BAR * max(1.0, abs(want)), (got, want)
    rows = slope_ref.row_slope(x, y, l2, ends)
    assert [r is None for r in rows] == [e < 2 for e in ends]
    # [B, 1, L] is the same rows; float32 inputs are widened, not computed in fp32
    assert float(slope_ref.slope_term(x.unsqueeze(1), y.unsqueeze(1), 5.0, l2, ends)) == got
    xf, yf = x.float(), y.float()
    assert float(slope_ref.slope_term(xf, yf, 5.0, l2, ends)) == float(slope_ref.slope_term(xf.double(), yf.double(), 5.0, l2, ends))
    # the metrics table is the squared form, unnormalised
    rois = torch.zeros(B, 7, 2, dtype=torch.int64)
    rois[:, -1, 0] = torch.tensor(ends)
    se, cnt = slope_ref.slope_metrics(x.unsqueeze(1), y.unsqueeze(1), rois)
    assert cnt.reshape(-1).tolist() == [max(e - 1, 0) for e in ends]
    if l2 and any(e >= 2 for e in ends):
        mean = sum(float(se[i, 0]) / (e - 1) for i, e in enumerate(ends) if e >= 2) / sum(e >= 2 for e in ends)
        assert abs(5.0 * mean - got) <= BAR * max(1.0, got)


@pytest.mark.parametrize("l2", [False, True], ids=["l1", "l2"])
@pytest.mark.parametrize("B,L,ends", CASES, ids=IDS)
def test_autograd_gradient_equals_the_closed_form(B, L, ends, l2):
    x, y = _rows(B, L, 11 * L + B)
    xr = x.clone().requires_grad_(True)
    slope_ref.slope_term(xr, y, 5.0, l2, ends).backward()
    g = slope_ref.slope_grad_closed(x, y, 5.0, l2, ends)
    d = float((xr.grad - g).abs().max())
    print(f"B={B} L={L} l2={l2}: autograd vs closed form max-abs {d:.2e}")
    assert d <= BAR
    for i, e in enumerate(ends):
        assert float(xr.grad[i, e:].abs().sum()) == 0.0 and float(g[i, e:].abs().sum()) == 0.0        # beyond the end: exactly zero
        if e < 2:
            assert float(g[i].abs().sum()) == 0.0
    assert (float(g.abs().max()) > 0) == any(e >= 2 for e in ends)
    # gscale is a plain factor
    assert torch.equal(slope_ref.slope_grad_closed(x, y, 5.0, l2, ends, gscale=0.25), slope_ref.slope_grad_closed(x, y, 5.0, l2, ends) * 0.25)


def test_the_closed_form_by_hand():
    """One row of four samples, L1: d = (+, -, 0) -> s = (1, -1, 0); g = F / 3 * (0 - 1, 1 + 1, -1 - 0, 0 - 0)."""
    x = torch.tensor([[0.0, 0.3, 0.1, 0.1]], dtype=torch.float64)
    y = torch.zeros_like(x)
    g = slope_ref.slope_grad_closed(x, y, 3.0)
    assert g.tolist() == [[-1.0, 2.0, -1.0, 0.0]]
    assert abs(float(slope_ref.slope_term(x, y, 3.0)) - (0.3 + 0.2 + 0.0)) <= BAR
    g2 = slope_ref.slope_grad_closed(x, y, 3.0, l2=True)
    assert float((g2 - torch.tensor([[-0.6, 0.6 + 0.4, -0.4, 0.0]], dtype=torch.float64)).abs().max()) <= BAR


def test_no_row_with_a_difference_gives_zero():
    x, y = _rows(2, 40, 3)
    for l2 in (False, True):
        xr = x.clone().requires_grad_(True)
        t = slope_ref.slope_term(xr, y, 5.0, l2, [1, 0])
        t.backward()
        assert float(t.detach()) == 0.0 and float(xr.grad.abs().sum()) == 0.0
        assert float(slope_ref.slope_grad_closed(x, y, 5.0, l2, [1, 0]).abs().sum()) == 0.0


def test_row_ends_clamp():
    rois = torch.zeros(4, 7, 2, dtype=torch.int64)
    rois[:, -1, 0] = torch.tensor([-5, 0, 33, 900])
    assert slope_ref.row_ends(rois, 4, 40) == [0, 0, 33, 40]
    assert slope_ref.row_ends(None, 2, 40) == [40, 40]


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)
    assert "loss_slope.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    for fn in ("nef_loss_slope_fwd", "nef_loss_slope_bwd"):
        assert re.search(r"\bint " + fn + r"\s*\(\s*const nef_loss_slope_args\s*\*\s*a,\s*nef_stream_t stream\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_slope_ws_bytes\s*\(\s*int B,\s*int L\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_slope_args_bytes\s*\(\s*void\s*\)", hdr)
    assert re.search(r"\bint nef_view_slope_metrics\s*\(\s*const float\s*\*\s*pred,\s*const float\s*\*\s*gt,\s*const int64_t\s*\*\s*rois,\s*"
                     r"double\s*\*\s*se,\s*int32_t\s*\*\s*cnt,\s*int B,\s*int Q,\s*int L,\s*nef_stream_t stream\s*\)", hdr)
    body = hdr[hdr.index("typedef struct nef_loss_slope_args"):hdr.index("} nef_loss_slope_args;")]
    fields = ["pred", "target", "noise", "rois", "losses", "ws", "ws_bytes", "gscale", "g_pred", "B", "L", "factor", "l2", "slot", "reserved0"]
    assert re.findall(r"(\w+);\s*/\*", body) == [n for n, _ in _lib.LossSlopeArgs._fields_] == fields
    L = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert L.nef_abi_version() == 22
    assert ctypes.sizeof(_lib.LossSlopeArgs) == L.nef_loss_slope_args_bytes() == 96
    from electrocardio_panorama_amd import ops
    tile = int(re.search(r"#define NEF_LOSS_SLOPE_TILE (\d+)", hdr).group(1))
    assert tile == ops.LOSS_SLOPE_TILE == 1024
    assert L.nef_loss_slope_ws_bytes(4, tile) == 4 * 8 and L.nef_loss_slope_ws_bytes(4, tile + 1) == 4 * 2 * 8
    assert L.nef_loss_slope_ws_bytes(256, 5000) == 256 * 5 * 8
    assert L.nef_loss_slope_ws_bytes(0, 10) == 0 and L.nef_loss_slope_ws_bytes(3, -1) == 0


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(pred=64, target=64, noise=None, rois=None, losses=64, ws=64, ws_bytes=1 << 20, gscale=None, g_pred=64, B=4, L=512, factor=5.0,
             l2=0, slot=4)
    a.update(kw)
    return _lib.LossSlopeArgs(**a)


def test_entries_reject_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the launches: nothing is launched and no address is read (non-NULL, never dereferenced pointers)."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    fwd = lambda **kw: L.nef_loss_slope_fwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    bwd = lambda **kw: L.nef_loss_slope_bwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    assert L.nef_loss_slope_fwd(None, None) == -2 and L.nef_loss_slope_bwd(None, None) == -2      # NEF_E_NULL
    for call in (fwd, bwd):
        assert call(pred=None) == -2 and call(target=None) == -2
        for key in ("B", "L"):
            for bad in (0, -1):
                assert call(**{key: bad}) == -1, (key, bad)                                        # NEF_E_SHAPE
        assert call(B=65536) == -1
        for bad in (-0.5, math.nan):
            assert call(factor=bad) == -1, bad
    assert fwd(losses=None) == -2 and bwd(g_pred=None) == -2
    for bad in (3, 6, 0, -1):
        assert fwd(slot=bad) == -1, bad
    need = L.nef_loss_slope_ws_bytes(4, 512)
    assert need == 32
    assert fwd(ws_bytes=need - 1) == -3 and fwd(ws_bytes=0, ws=None) == -3                        # NEF_E_WORKSPACE
    assert fwd(ws=None) == -2
    # a NULL pointer wins over a bad shape, a bad shape over a small workspace
    assert fwd(pred=None, B=0) == -2 and fwd(B=0, ws_bytes=0) == -1 and fwd(slot=7, ws_bytes=0) == -1
    L_ = L
    met = lambda pred=64, gt=64, rois=None, se=64, cnt=64, B=2, Q=3, L=16: L_.nef_view_slope_metrics(pred, gt, rois, se, cnt, B, Q, L, None)  # noqa: E731
    for key in ("pred", "gt", "se", "cnt"):
        assert met(**{key: None}) == -2, key
    for key in ("B", "Q", "L"):
        for bad in (0, -1):
            assert met(**{key: bad}) == -1, (key, bad)
    assert met(B=1 << 16, Q=1 << 15) == -1                                                         # B * Q is a grid's x extent
    assert met(pred=None, B=0) == -2


def test_a_library_without_the_entries_is_rejected(monkeypatch):
    """The ABI number stays 22 (the entries are additions): a library built before them is told by the missing symbol, and one whose
    struct differs by the size check."""
    import _ctypes
    from electrocardio_panorama_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", _ctypes.__file__)
    with pytest.raises(_lib.NefLibraryError, match="rebuild"):
        _lib.load()
    # the entries' names are what a stale library of this project lacks
    for name in ENTRIES:
        assert name in _lib.SIGNATURES


def test_a_struct_of_another_size_is_rejected(monkeypatch):
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)

    class Short(ctypes.Structure):
        _fields_ = _lib.LossSlopeArgs._fields_[:-2]

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LossSlopeArgs", Short)
    with pytest.raises(_lib.NefLibraryError, match="nef_loss_slope_args is 96 bytes"):
        _lib.load()


# ------------------------------------------------------------------------------------------------ config and losswrapper
def test_config_defaults_are_off():
    from electrocardio_panorama_amd.config import get_defaults
    cfg = get_defaults()
    assert cfg.SOLVER.slope_factor == 0.0 and cfg.SOLVER.slope_loss == "l1_loss" and cfg.SOLVER.slope_crop is True
    assert cfg.SOLVER.slope_eval is False
    cfg.merge_from_list(["SOLVER.slope_factor", "5.0", "SOLVER.slope_crop", "False", "SOLVER.slope_loss", "l2_loss", "SOLVER.slope_eval", "True"])
    assert cfg.SOLVER.slope_factor == 5.0 and cfg.SOLVER.slope_crop is False and cfg.SOLVER.slope_loss == "l2_loss"
    assert cfg.SOLVER.slope_eval is True
    cfg.merge_from_list(["SOLVER.slope_factor", 1])
    assert cfg.SOLVER.slope_factor == 1.0 and isinstance(cfg.SOLVER.slope_factor, float)


def _cfg(**solver):
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=3, noise=False),
               SOLVER=Cfg(optim="sgd", lr=0.1, reg_loss="l1_loss", loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], **solver))


@pytest.mark.parametrize("bad", [-0.5, -1e-9, math.nan])
def test_a_negative_factor_raises_where_the_loss_is_built(bad):
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.network.loss.losses import slope_settings
    with pytest.raises(ValueError, match="slope_factor"):
        build_loss(_cfg(slope_factor=bad))
    with pytest.raises(ValueError, match="slope_factor"):
        slope_settings(_cfg(slope_factor=bad), rois=torch.zeros(1, 7, 2, dtype=torch.int64))
    assert build_loss(_cfg()) is build_loss(_cfg(slope_factor=5.0))       # keys absent (an older config) or valid: the same losswrapper


@pytest.mark.parametrize("bad", ["l3_loss", "", "L1", None, 2])
def test_an_unknown_norm_raises_where_the_loss_is_built(bad):
    from electrocardio_panorama_amd.network import build_loss, losswrapper
    with pytest.raises(ValueError, match="slope_loss"):
        build_loss(_cfg(slope_factor=5.0, slope_loss=bad))
    t = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="slope_loss"):
        losswrapper(t, t, t, t, _cfg(slope_factor=5.0, slope_loss=bad), rois=torch.zeros(2, 7, 2, dtype=torch.int64))
    build_loss(_cfg(slope_factor=0.0, slope_loss=bad))                    # off: the other keys are not looked at


def test_crop_without_rois_raises_before_any_device_work():
    """CPU tensors: the ValueError comes before the first launch (which would reject them)."""
    from electrocardio_panorama_amd.network import losswrapper
    from electrocardio_panorama_amd.network.loss.losses import slope_settings
    t = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="slope_crop"):
        losswrapper(t, t, t, t, _cfg(slope_factor=5.0, slope_crop=True))
    with pytest.raises(ValueError, match="slope_crop"):
        losswrapper(t, t, t, t, _cfg(slope_factor=5.0))                  # the key's default is True
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    assert slope_settings(_cfg(slope_factor=5.0), rois)[2] is rois
    assert slope_settings(_cfg(slope_factor=5.0), rois)[:2] == (5.0, False)
    assert slope_settings(_cfg(slope_factor=5.0, slope_loss="l2_loss", slope_crop=False), rois) == (5.0, True, None)
    assert slope_settings(_cfg(slope_factor=0.0, slope_crop=True, slope_loss="l2_loss")) == (0.0, False, None)      # off: nothing asked for
    assert slope_settings(_cfg()) == (0.0, False, None)
    assert slope_settings(_cfg(slope_factor=5.0), need_rois=False) == (5.0, False, None)


def test_losswrapper_tuple_lengths_with_the_keys_off(monkeypatch):
    """4 (train) and 5 (test) elements with the key off or absent, rois= given or not, and only ops.loss_fwd is called -- checked on the
    host with the ops replaced by recorders; with the key on the term is the last element of both forms, behind the SSIM term when that
    is on, and the SSIM op keeps being handed five elements."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.network import losswrapper
    calls = []

    def fake_fwd(pred, pp, pl, tgt, factors, reg_l2, use_mask, out=None, noise=None):
        calls.append(("loss_fwd", None if out is None else out.numel()))
        row = torch.arange(4, dtype=torch.float32) if out is None else out
        if out is not None:
            out[:4] = torch.arange(4, dtype=torch.float32)
        return row

    def fake_ssim(pred, tgt, losses, factor, rois=None, noise=None):
        calls.append(("loss_ssim_fwd", losses.numel(), factor, rois is not None))
        losses[4] = 9.0
        return losses

    def fake_slope(pred, tgt, losses, factor, l2, rois=None, noise=None):
        calls.append(("loss_slope_fwd", losses.numel(), factor, bool(l2), rois is not None))
        losses[-1] = 7.0
        return losses

    monkeypatch.setattr(ops, "loss_fwd", fake_fwd)
    monkeypatch.setattr(ops, "loss_ssim_fwd", fake_ssim)
    monkeypatch.setattr(ops, "loss_slope_fwd", fake_slope)
    t = torch.zeros(2, 1, 16)
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    for cfg in (_cfg(), _cfg(slope_factor=0.0, slope_crop=True, slope_loss="l2_loss", slope_eval=True)):
        for kw in ({}, {"rois": rois}):
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, **kw)) == 4
            assert calls == [("loss_fwd", None)]
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, t, t, **kw)) == 5
            assert calls == [("loss_fwd", None), ("loss_fwd", None)]
    on = _cfg(slope_factor=5.0)
    calls.clear()
    train = losswrapper(t, t, t, t, on, rois=rois)
    assert len(train) == 5 and float(train[-1]) == 7.0 and [float(v) for v in train[:4]] == [0.0, 1.0, 2.0, 3.0]
    assert calls == [("loss_fwd", 5), ("loss_slope_fwd", 5, 5.0, False, True)]
    test = losswrapper(t, t, t, t, on, t, t, rois=rois)
    assert len(test) == 6 and float(test[-1]) == 7.0 and float(test[4]) == 3.0          # loss_unsperv keeps index 4
    calls.clear()
    assert len(losswrapper(t, t, t, t, _cfg(slope_factor=5.0, slope_crop=False, slope_loss="l2_loss"))) == 5
    assert calls[-1] == ("loss_slope_fwd", 5, 5.0, True, False)
    # both tail terms: (loss, l1, l2, l3[, unsup], ssim, slope)
    both = _cfg(slope_factor=5.0, ssim_factor=0.5)
    calls.clear()
    train = losswrapper(t, t, t, t, both, rois=rois)
    assert len(train) == 6 and float(train[4]) == 9.0 and float(train[5]) == 7.0
    assert calls == [("loss_fwd", 6), ("loss_ssim_fwd", 5, 0.5, True), ("loss_slope_fwd", 6, 5.0, False, True)]
    test = losswrapper(t, t, t, t, both, t, t, rois=rois)
    assert len(test) == 7 and [float(test[k]) for k in (4, 5, 6)] == [3.0, 9.0, 7.0]
    # the SSIM term alone is what it was
    calls.clear()
    assert len(losswrapper(t, t, t, t, _cfg(ssim_factor=0.5), rois=rois)) == 5
    assert calls == [("loss_fwd", 5), ("loss_ssim_fwd", 5, 0.5, True)]
