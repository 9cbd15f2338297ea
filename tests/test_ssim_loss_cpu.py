"""CPU: the SSIM term of the training loss (SOLVER.ssim_factor) -- the fp64 restatement tests/ssim_ref.py pinned to utils.metric.ssim_1d and
its autograd gradient to the closed form the backward kernel implements, the four C-ABI entries in the header, the binding table and the
library, their argument checks (no GPU work), the config keys and their ValueErrors, and losswrapper's tuple with the key off."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fp64 throughout; the two restatements order ~30 operations per window differently
BAR = 1e-12
ENTRIES = ("nef_loss_ssim_fwd", "nef_loss_ssim_bwd", "nef_loss_ssim_ws_bytes", "nef_loss_ssim_args_bytes")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _rows(B, L, seed):
    """Uniform in [0, 1/3]: the decoder's output range is sigmoid / 3."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, L, generator=g, dtype=torch.float64) / 3, torch.rand(B, L, generator=g, dtype=torch.float64) / 3)


CASES = [(1, 7, [7]), (1, 8, [8]), (2, 13, [13, 13]), (3, 40, [33, 7, 40]), (4, 500, [298, 6, 0, 500]), (1, 512, [440])]


@pytest.mark.parametrize("B,L,ends", CASES, ids=[f"B{b}_L{l}" for b, l, _ in CASES])
def test_restatement_equals_ssim_1d(B, L, ends):
    from electrocardio_panorama_amd.utils.metric import ssim_1d
    x, y = _rows(B, L, 7 * L + B)
    rows = ssim_ref.row_ssim(x, y, ends)
    want = []
    for i, e in enumerate(ends):
        if e < 7:
            assert rows[i] is None
            continue
        w = ssim_1d(x[i, :e].numpy(), y[i, :e].numpy())
        assert abs(float(rows[i]) - w) <= BAR, (i, float(rows[i]), w)
        want.append(w)
    term = float(ssim_ref.ssim_term(x, y, 0.5, ends))
    assert abs(term - 0.5 * (1.0 - float(np.mean(want)))) <= BAR
    # float32 inputs are widened, not computed in fp32
    assert abs(float(ssim_ref.ssim_term(x.float(), y.float(), 0.5, ends)) - float(ssim_ref.ssim_term(x.float().double(), y.float().double(), 0.5, ends))) == 0.0


@pytest.mark.parametrize("B,L,ends", CASES, ids=[f"B{b}_L{l}" for b, l, _ in CASES])
def test_autograd_gradient_equals_the_closed_form(B, L, ends):
    x, y = _rows(B, L, 11 * L + B)
    xr = x.clone().requires_grad_(True)
    ssim_ref.ssim_term(xr, y, 0.5, ends).backward()
    g = ssim_ref.ssim_grad_closed(x, y, 0.5, ends)
    d = float((xr.grad - g).abs().max())
    print(f"B={B} L={L}: autograd vs closed form max-abs {d:.2e}")
    assert d <= BAR
    for i, e in enumerate(ends):
        assert float(xr.grad[i, e:].abs().sum()) == 0.0 and float(g[i, e:].abs().sum()) == 0.0        # beyond the end: exactly zero
        if e < 7:
            assert float(g[i].abs().sum()) == 0.0
    assert float(g.abs().max()) > 0
    # gscale is a plain factor
    assert torch.equal(ssim_ref.ssim_grad_closed(x, y, 0.5, ends, gscale=0.25), ssim_ref.ssim_grad_closed(x, y, 0.5, ends) * 0.25)


def test_no_row_with_a_window_gives_zero():
    x, y = _rows(2, 40, 3)
    xr = x.clone().requires_grad_(True)
    t = ssim_ref.ssim_term(xr, y, 0.5, [6, 0])
    t.backward()
    assert float(t.detach()) == 0.0 and float(xr.grad.abs().sum()) == 0.0
    assert float(ssim_ref.ssim_grad_closed(x, y, 0.5, [6, 0]).abs().sum()) == 0.0


def test_row_ends_clamp():
    rois = torch.zeros(4, 7, 2, dtype=torch.int64)
    rois[:, -1, 0] = torch.tensor([-5, 0, 33, 900])
    assert ssim_ref.row_ends(rois, 4, 40) == [0, 0, 33, 40]
    assert ssim_ref.row_ends(None, 2, 40) == [40, 40]


def test_identical_constant_rows_and_zero_target():
    """x == y constant: every window is 1 and the gradient vanishes; a zero target (the padded region) stays finite."""
    x = torch.full((1, 20), 0.2, dtype=torch.float64)
    assert abs(float(ssim_ref.ssim_term(x, x.clone(), 1.0)) - 0.0) <= BAR
    assert float(ssim_ref.ssim_grad_closed(x, x.clone(), 1.0).abs().max()) <= BAR
    x, _ = _rows(1, 20, 5)
    g = ssim_ref.ssim_grad_closed(x, torch.zeros_like(x), 1.0)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    for fn in ("nef_loss_ssim_fwd", "nef_loss_ssim_bwd"):
        assert re.search(r"\bint " + fn + r"\s*\(\s*const nef_loss_ssim_args\s*\*\s*a,\s*nef_stream_t stream\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_ssim_ws_bytes\s*\(\s*int B,\s*int L\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_ssim_args_bytes\s*\(\s*void\s*\)", hdr)
    body = hdr[hdr.index("typedef struct nef_loss_ssim_args"):hdr.index("} nef_loss_ssim_args;")]
    assert re.findall(r"(\w+);\s*/\*", body) == [n for n, _ in _lib.LossSsimArgs._fields_]
    L = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert L.nef_abi_version() == 22
    assert ctypes.sizeof(_lib.LossSsimArgs) == L.nef_loss_ssim_args_bytes() == 88
    from electrocardio_panorama_amd import ops
    tile = int(re.search(r"#define NEF_LOSS_SSIM_TILE (\d+)", hdr).group(1))
    assert tile == ops.LOSS_SSIM_TILE
    assert L.nef_loss_ssim_ws_bytes(4, tile) == 4 * 8 and L.nef_loss_ssim_ws_bytes(4, tile + 1) == 4 * 2 * 8
    assert L.nef_loss_ssim_ws_bytes(256, 5000) == 256 * 10 * 8
    assert L.nef_loss_ssim_ws_bytes(0, 10) == 0 and L.nef_loss_ssim_ws_bytes(3, -1) == 0


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(pred=64, target=64, noise=None, rois=None, losses=64, ws=64, ws_bytes=1 << 20, gscale=None, g_pred=64, B=4, L=512, factor=0.5)
    a.update(kw)
    return _lib.LossSsimArgs(**a)


def test_entries_reject_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the launches: nothing is launched and no address is read (non-NULL, never dereferenced pointers)."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    fwd = lambda **kw: L.nef_loss_ssim_fwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    bwd = lambda **kw: L.nef_loss_ssim_bwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    assert L.nef_loss_ssim_fwd(None, None) == -2 and L.nef_loss_ssim_bwd(None, None) == -2      # NEF_E_NULL
    for call in (fwd, bwd):
        assert call(pred=None) == -2 and call(target=None) == -2
        for key in ("B", "L"):
            for bad in (0, -1):
                assert call(**{key: bad}) == -1, (key, bad)                                      # NEF_E_SHAPE
        assert call(B=65536) == -1
        for bad in (-0.5, math.nan):
            assert call(factor=bad) == -1, bad
    assert fwd(losses=None) == -2 and bwd(g_pred=None) == -2
    need = L.nef_loss_ssim_ws_bytes(4, 512)
    assert need == 32
    assert fwd(ws_bytes=need - 1) == -3 and fwd(ws_bytes=0, ws=None) == -3                      # NEF_E_WORKSPACE
    assert fwd(ws=None) == -2
    # a NULL pointer wins over a bad shape, a bad shape over a small workspace
    assert fwd(pred=None, B=0) == -2 and fwd(B=0, ws_bytes=0) == -1


def test_a_library_without_the_entries_is_rejected(monkeypatch):
    """The ABI number stays 22 (the entries are additions): a library built before them is told by the missing symbol."""
    import _ctypes
    from electrocardio_panorama_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", _ctypes.__file__)
    with pytest.raises(_lib.NefLibraryError, match="rebuild"):
        _lib.load()


# ------------------------------------------------------------------------------------------------ config and losswrapper
def test_config_defaults_are_off():
    from electrocardio_panorama_amd.config import get_defaults
    cfg = get_defaults()
    assert cfg.SOLVER.ssim_factor == 0.0 and cfg.SOLVER.ssim_crop is True
    cfg.merge_from_list(["SOLVER.ssim_factor", "0.5", "SOLVER.ssim_crop", "False"])
    assert cfg.SOLVER.ssim_factor == 0.5 and cfg.SOLVER.ssim_crop is False
    cfg.merge_from_list(["SOLVER.ssim_factor", 1])
    assert cfg.SOLVER.ssim_factor == 1.0 and isinstance(cfg.SOLVER.ssim_factor, float)


def _cfg(**solver):
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=3, noise=False),
               SOLVER=Cfg(optim="sgd", lr=0.1, reg_loss="l1_loss", loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], **solver))


@pytest.mark.parametrize("bad", [-0.5, -1e-9, math.nan])
def test_a_negative_factor_raises_where_the_loss_is_built(bad):
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.network.loss.losses import ssim_settings
    with pytest.raises(ValueError, match="ssim_factor"):
        build_loss(_cfg(ssim_factor=bad))
    with pytest.raises(ValueError, match="ssim_factor"):
        ssim_settings(_cfg(ssim_factor=bad), rois=torch.zeros(1, 7, 2, dtype=torch.int64))
    assert build_loss(_cfg()) is build_loss(_cfg(ssim_factor=0.5))        # keys absent (an older config) or valid: the same losswrapper


def test_crop_without_rois_raises_before_any_device_work():
    """CPU tensors: the ValueError comes before the first launch (which would reject them)."""
    from electrocardio_panorama_amd.network import losswrapper
    from electrocardio_panorama_amd.network.loss.losses import ssim_settings
    t = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="ssim_crop"):
        losswrapper(t, t, t, t, _cfg(ssim_factor=0.5, ssim_crop=True))
    with pytest.raises(ValueError, match="ssim_crop"):
        losswrapper(t, t, t, t, _cfg(ssim_factor=0.5))                  # the key's default is True
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    assert ssim_settings(_cfg(ssim_factor=0.5), rois)[1] is rois
    assert ssim_settings(_cfg(ssim_factor=0.5, ssim_crop=False), rois) == (0.5, None)
    assert ssim_settings(_cfg(ssim_factor=0.0, ssim_crop=True)) == (0.0, None)          # off: rois are not asked for
    assert ssim_settings(_cfg()) == (0.0, None)


def test_losswrapper_tuple_lengths_with_the_key_off(monkeypatch):
    """4 (train) and 5 (test) elements with the key off or absent, rois= given or not, and only ops.loss_fwd is called -- checked on the
    host with the two ops replaced by recorders; with the key on the term is the last element of both forms."""
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

    monkeypatch.setattr(ops, "loss_fwd", fake_fwd)
    monkeypatch.setattr(ops, "loss_ssim_fwd", fake_ssim)
    t = torch.zeros(2, 1, 16)
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    for cfg in (_cfg(), _cfg(ssim_factor=0.0, ssim_crop=True)):
        for kw in ({}, {"rois": rois}):
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, **kw)) == 4
            assert calls == [("loss_fwd", None)]
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, t, t, **kw)) == 5
            assert calls == [("loss_fwd", None), ("loss_fwd", None)]
    on = _cfg(ssim_factor=0.5)
    calls.clear()
    train = losswrapper(t, t, t, t, on, rois=rois)
    assert len(train) == 5 and float(train[-1]) == 9.0 and [float(v) for v in train[:4]] == [0.0, 1.0, 2.0, 3.0]
    assert calls == [("loss_fwd", 5), ("loss_ssim_fwd", 5, 0.5, True)]
    test = losswrapper(t, t, t, t, on, t, t, rois=rois)
    assert len(test) == 6 and float(test[-1]) == 9.0 and float(test[4]) == 3.0          # loss_unsperv keeps index 4
    calls.clear()
    assert len(losswrapper(t, t, t, t, _cfg(ssim_factor=0.5, ssim_crop=False))) == 5
    assert calls[-1] == ("loss_ssim_fwd", 5, 0.5, False)
