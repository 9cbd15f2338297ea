"""CPU: the correlation term of the training loss (SOLVER.corr_factor) -- the fp64 restatement tests/corr_ref.py pinned to a literal Python
loop and to numpy.corrcoef, its autograd gradient to the closed form the backward kernels implement, the exactness and range properties of
the definition, the C-ABI entries in the header, the binding table and the library, their argument checks (no GPU work), the config keys
and their ValueErrors, losswrapper's tuple with the keys off, and the precondition of the device tests' bars on the device tests' inputs."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import corr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12
EPS = corr_ref.EPS
ENTRIES = ("nef_loss_corr_fwd", "nef_loss_corr_bwd", "nef_loss_corr_ws_bytes", "nef_loss_corr_args_bytes", "nef_view_corr_metrics")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _rows(B, L, seed):
    """Uniform in [0, 1/3]: the decoder's output range is sigmoid / 3."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, L, generator=g, dtype=torch.float64) / 3, torch.rand(B, L, generator=g, dtype=torch.float64) / 3)


CASES = [(1, 1, [1]), (1, 2, [2]), (2, 13, [13, 13]), (4, 40, [33, 1, 0, 40]), (3, 500, [298, 2, 500]), (1, 512, [440])]
IDS = [f"B{b}_L{l}" for b, l, _ in CASES]


def _loop_term(x, y, factor, eps, ends):
    """The definition, literally."""
    total, R = 0.0, 0
    for i, n in enumerate(ends):
        if n < 2:
            continue
        su = sw = suu = sww = suw = 0.0
        x0, y0 = float(x[i, 0]), float(y[i, 0])
        for t in range(n):
            u, w = float(x[i, t]) - x0, float(y[i, t]) - y0
            su, sw, suu, sww, suw = su + u, sw + w, suu + u * u, sww + w * w, suw + u * w
        mu, mw = su / n, sw / n
        vx, vy, c = suu / n - mu * mu, sww / n - mw * mw, suw / n - mu * mw
        total += 1.0 - (c + eps) / math.sqrt((vx + eps) * (vy + eps))
        R += 1
    return factor * total / R if R else 0.0


@pytest.mark.parametrize("B,L,ends", CASES, ids=IDS)
def test_restatement_equals_the_literal_loop_and_corrcoef(B, L, ends):
    x, y = _rows(B, L, 7 * L + B)
    want = _loop_term(x, y, 5.0, EPS, ends)
    got = float(corr_ref.corr_term(x, y, 5.0, EPS, ends))
    assert abs(got - want) <= BAR * max(1.0, abs(want)), (got, want)
    rows = corr_ref.corr_rows(x, y, EPS, ends)
    assert [r is None for r in rows] == [n < 2 for n in ends]
    # eps = 0 is numpy's coefficient (n == 2 is +-1 there too; a longer row is a generic one)
    for i, n in enumerate(ends):
        if n >= 2:
            r0 = float(corr_ref.corr_rows(x[i:i + 1], y[i:i + 1], 0.0, [n])[0])
            assert abs(r0 - float(np.corrcoef(x[i, :n].numpy(), y[i, :n].numpy())[0, 1])) <= BAR
    # [B, 1, L] is the same rows; float32 inputs are widened, not computed in fp32
    assert float(corr_ref.corr_term(x.unsqueeze(1), y.unsqueeze(1), 5.0, EPS, ends)) == got
    xf, yf = x.float(), y.float()
    assert float(corr_ref.corr_term(xf, yf, 5.0, EPS, ends)) == float(corr_ref.corr_term(xf.double(), yf.double(), 5.0, EPS, ends))
    # the second formulation agrees
    assert abs(corr_ref.corr_term_centred(x, y, 5.0, EPS, ends) - got) <= BAR * max(1.0, abs(got))
    # the metrics table holds the same moments: r from it is the term's r
    rois = corr_ref.rois_of(ends)
    mom, cnt = corr_ref.corr_metrics(x.unsqueeze(1), y.unsqueeze(1), rois)
    assert cnt.reshape(-1).tolist() == [max(n, 0) for n in ends]
    r = corr_ref.metrics_r(mom, cnt, EPS)
    assert r.numel() == sum(n >= 2 for n in ends)
    if r.numel():
        assert abs(5.0 * float((1.0 - r).mean()) - got) <= BAR * max(1.0, got)


@pytest.mark.parametrize("n", [2, 3, 7, 512, 5000, 40000])
def test_autograd_gradient_equals_the_closed_form(n):
    """Within 1e-10 of the largest gradient element (3.6e-11 was measured when the closed form was derived)."""
    x, y = _rows(2, n + 3, 11 * n)
    ends = [n, n + 3]
    xr = x.clone().requires_grad_(True)
    corr_ref.corr_term(xr, y, 5.0, EPS, ends).backward()
    g, mag = corr_ref.corr_grad_closed(x, y, 5.0, EPS, ends)
    top = float(g.abs().max())
    d = float((xr.grad - g).abs().max())
    print(f"n={n}: autograd vs closed form max-abs {d:.2e}, relative to the largest element {d / top:.2e}")
    assert top > 0 and d <= 1e-10 * top
    assert float(xr.grad[0, n:].abs().sum()) == 0.0 and float(g[0, n:].abs().sum()) == 0.0         # beyond the end: exactly zero
    assert bool((mag >= g.abs() * (1 - 1e-12)).all()) and float(mag[0, n:].abs().sum()) == 0.0
    # gscale is a plain factor
    g4, mag4 = corr_ref.corr_grad_closed(x, y, 5.0, EPS, ends, gscale=0.25)
    assert torch.equal(g4, g * 0.25) and torch.equal(mag4, mag * 0.25)


def test_rows_that_do_not_count_have_zero_gradient():
    x, y = _rows(3, 40, 3)
    xr = x.clone().requires_grad_(True)
    corr_ref.corr_term(xr, y, 5.0, EPS, [1, 0, 40]).backward()
    g = corr_ref.corr_grad_closed(x, y, 5.0, EPS, [1, 0, 40])[0]
    assert float(xr.grad[:2].abs().sum()) == 0.0 and float(g[:2].abs().sum()) == 0.0 and float(g[2].abs().max()) > 0
    xr = x.clone().requires_grad_(True)
    t = corr_ref.corr_term(xr, y, 5.0, EPS, [1, 0, 1])
    t.backward()
    assert float(t.detach()) == 0.0 and float(xr.grad.abs().sum()) == 0.0
    assert float(corr_ref.corr_grad_closed(x, y, 5.0, EPS, [1, 0, 1])[0].abs().sum()) == 0.0


@pytest.mark.parametrize("eps", [1e-8, 1e-3, 0.37])
def test_identical_and_constant_rows_give_exactly_one(eps):
    """x == y: vx, vy and c are the same bits a, so D = sqrt(fl(a * a)) == a and r == 1.0 exactly; two constant rows: the shifted moments
    are exact zeros and r = eps / sqrt(fl(eps * eps)) == 1.0.  The gradients are exact zeros."""
    x = _rows(3, 777, 5)[0].float().double()
    assert [float(r) for r in corr_ref.corr_rows(x, x.clone(), eps)] == [1.0] * 3
    assert float(corr_ref.corr_term(x, x.clone(), 5.0, eps)) == 0.0
    g, mag = corr_ref.corr_grad_closed(x, x.clone(), 5.0, eps)
    assert float(g.abs().max()) == 0.0 and float(mag.abs().max()) > 0
    cx, cy = torch.full((2, 40), 0.1234567, dtype=torch.float64), torch.full((2, 40), -7.25, dtype=torch.float64)
    assert [float(r) for r in corr_ref.corr_rows(cx, cy, eps)] == [1.0] * 2
    assert float(corr_ref.corr_grad_closed(cx, cy, 5.0, eps)[0].abs().max()) == 0.0
    mom, cnt = corr_ref.corr_metrics(cx.unsqueeze(1), cy.unsqueeze(1))
    assert float(mom.abs().max()) == 0.0 and cnt.tolist() == [[40], [40]]


def test_r_lies_in_the_half_open_interval():
    x, y = _rows(64, 300, 9)
    r = torch.stack(corr_ref.corr_rows(x, y))
    assert bool((r > -1).all()) and bool((r <= 1).all()) and float(r.abs().max()) < 0.5           # independent rows: near 0
    anti = torch.stack(corr_ref.corr_rows(x, 0.2 - 0.5 * x))
    assert bool((anti > -1).all()) and bool((anti < -0.999).all())
    # gain and offset of the prediction do not change it (beyond eps' share)
    moved = torch.stack(corr_ref.corr_rows(3.0 * x + 0.7, y))
    assert float((moved - r).abs().max()) < 1e-5
    # n == 2, the shortest row that counts
    short = torch.stack(corr_ref.corr_rows(x, y, EPS, [2] * 64))
    assert bool((short > -1).all()) and bool((short <= 1).all())


def test_row_ends_clamp():
    rois = torch.zeros(4, 7, 2, dtype=torch.int64)
    rois[:, -1, 0] = torch.tensor([-5, 0, 33, 900])
    assert corr_ref.row_ends(rois, 4, 40) == [0, 0, 33, 40]
    assert corr_ref.row_ends(None, 2, 40) == [40, 40]


# ------------------------------------------------------------------------------------------------ precondition of the device bars
@pytest.mark.parametrize("B,L,ends", corr_ref.SHAPES, ids=corr_ref.IDS)
def test_the_device_tests_inputs_are_well_conditioned(B, L, ends):
    """The device tests hold the kernels to 2^-22 of the fp64 restatement.  That is a statement about the kernels only if the restatement
    itself is good to far below it on the same inputs: the shifted one-pass fp64 form and the centred two-pass longdouble form of
    1 - mean r agree within 2^-30 relative, on every input of tests/test_corr_loss_gpu.py."""
    for kind in corr_ref.KINDS:
        for noisy in (False, True):
            x, tgt = corr_ref.case_x(B, L, kind, noisy), corr_ref.case(B, L, kind, noisy)[3]
            for e in corr_ref.variants(ends):
                n = corr_ref.row_ends(None if e is None else corr_ref.rois_of(e), B, L)
                a = float(corr_ref.corr_term(x, tgt, 1.0, EPS, n))
                b = corr_ref.corr_term_centred(x, tgt, 1.0, EPS, n)
                print(f"B={B} L={L} {kind} noise={noisy} ends={e}: 1 - mean r = {a:.12g}, |one-pass - centred| {abs(a - b):.2e}")
                assert abs(a - b) <= 2.0 ** -30 * abs(b), (kind, noisy, e, a, b)
                if any(v >= 2 for v in n) and L > 13:
                    assert (a > 0.5) if kind == "indep" else (0 < a < 0.2), a


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_agree():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)
    assert "loss_corr.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    for fn in ("nef_loss_corr_fwd", "nef_loss_corr_bwd"):
        assert re.search(r"\bint " + fn + r"\s*\(\s*const nef_loss_corr_args\s*\*\s*a,\s*nef_stream_t stream\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_corr_ws_bytes\s*\(\s*int B,\s*int L\s*\)", hdr)
    assert re.search(r"\bsize_t nef_loss_corr_args_bytes\s*\(\s*void\s*\)", hdr)
    assert re.search(r"\bint nef_view_corr_metrics\s*\(\s*const float\s*\*\s*pred,\s*const float\s*\*\s*gt,\s*const int64_t\s*\*\s*rois,\s*"
                     r"double\s*\*\s*mom,\s*int32_t\s*\*\s*cnt,\s*int B,\s*int Q,\s*int L,\s*nef_stream_t stream\s*\)", hdr)
    body = hdr[hdr.index("typedef struct nef_loss_corr_args"):hdr.index("} nef_loss_corr_args;")]
    fields = ["pred", "target", "noise", "rois", "losses", "ws", "ws_bytes", "gscale", "g_pred", "eps", "B", "L", "factor", "slot"]
    assert re.findall(r"(\w+);\s*/\*", body) == [n for n, _ in _lib.LossCorrArgs._fields_] == fields
    L = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert L.nef_abi_version() == 22
    assert ctypes.sizeof(_lib.LossCorrArgs) == L.nef_loss_corr_args_bytes() == 96
    from electrocardio_panorama_amd import ops
    tile = int(re.search(r"#define NEF_LOSS_CORR_TILE (\d+)", hdr).group(1))
    assert tile == ops.LOSS_CORR_TILE == corr_ref.TILE == 1024
    # five sums per (row, tile) and four numbers per row
    assert L.nef_loss_corr_ws_bytes(4, tile) == 4 * (5 + 4) * 8 and L.nef_loss_corr_ws_bytes(4, tile + 1) == 4 * (2 * 5 + 4) * 8
    assert L.nef_loss_corr_ws_bytes(256, 5000) == 256 * (5 * 5 + 4) * 8
    assert L.nef_loss_corr_ws_bytes(0, 10) == 0 and L.nef_loss_corr_ws_bytes(3, -1) == 0


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(pred=64, target=64, noise=None, rois=None, losses=64, ws=64, ws_bytes=1 << 20, gscale=None, g_pred=64, eps=1e-8, B=4, L=512,
             factor=5.0, slot=4)
    a.update(kw)
    return _lib.LossCorrArgs(**a)


def test_entries_reject_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the launches: nothing is launched and no address is read (non-NULL, never dereferenced pointers)."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    fwd = lambda **kw: L.nef_loss_corr_fwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    bwd = lambda **kw: L.nef_loss_corr_bwd(ctypes.byref(_args(**kw)), None)      # noqa: E731
    assert L.nef_loss_corr_fwd(None, None) == -2 and L.nef_loss_corr_bwd(None, None) == -2         # NEF_E_NULL
    need = L.nef_loss_corr_ws_bytes(4, 512)
    assert need == 4 * 9 * 8
    for call in (fwd, bwd):
        assert call(pred=None) == -2 and call(target=None) == -2
        for key in ("B", "L"):
            for bad in (0, -1):
                assert call(**{key: bad}) == -1, (key, bad)                                        # NEF_E_SHAPE
        assert call(B=65536) == -1
        for key in ("factor", "eps"):
            for bad in (-0.5, math.nan):
                assert call(**{key: bad}) == -1, (key, bad)
        assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0, ws=None) == -3                   # NEF_E_WORKSPACE
        assert call(ws=None) == -2
        # a NULL pointer wins over a bad shape, a bad shape over a small workspace
        assert call(pred=None, B=0) == -2 and call(B=0, ws_bytes=0) == -1
    assert fwd(losses=None) == -2 and bwd(g_pred=None) == -2
    for bad in (3, 7, 0, -1):
        assert fwd(slot=bad) == -1, bad
    assert fwd(slot=7, ws_bytes=0) == -1
    L_ = L
    met = lambda pred=64, gt=64, rois=None, mom=64, cnt=64, B=2, Q=3, L=16: L_.nef_view_corr_metrics(pred, gt, rois, mom, cnt, B, Q, L, None)  # noqa: E731
    for key in ("pred", "gt", "mom", "cnt"):
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
    for name in ENTRIES:
        assert name in _lib.SIGNATURES


def test_a_struct_of_another_size_is_rejected(monkeypatch):
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)

    class Short(ctypes.Structure):
        _fields_ = _lib.LossCorrArgs._fields_[:-2]

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LossCorrArgs", Short)
    with pytest.raises(_lib.NefLibraryError, match="nef_loss_corr_args is 96 bytes"):
        _lib.load()


# ------------------------------------------------------------------------------------------------ config and losswrapper
def test_config_defaults_are_off():
    from electrocardio_panorama_amd.config import get_defaults
    cfg = get_defaults()
    assert cfg.SOLVER.corr_factor == 0.0 and cfg.SOLVER.corr_crop is True and cfg.SOLVER.corr_eps == 1e-8
    assert cfg.SOLVER.corr_eval is False
    cfg.merge_from_list(["SOLVER.corr_factor", "5.0", "SOLVER.corr_crop", "False", "SOLVER.corr_eps", "1e-6", "SOLVER.corr_eval", "True"])
    assert cfg.SOLVER.corr_factor == 5.0 and cfg.SOLVER.corr_crop is False and cfg.SOLVER.corr_eps == 1e-6
    assert cfg.SOLVER.corr_eval is True
    cfg.merge_from_list(["SOLVER.corr_factor", 1])
    assert cfg.SOLVER.corr_factor == 1.0 and isinstance(cfg.SOLVER.corr_factor, float)


def _cfg(**solver):
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=3, noise=False),
               SOLVER=Cfg(optim="sgd", lr=0.1, reg_loss="l1_loss", loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], **solver))


@pytest.mark.parametrize("bad", [-0.5, -1e-9, math.nan])
def test_a_negative_factor_raises_where_the_loss_is_built(bad):
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.network.loss.losses import corr_settings
    with pytest.raises(ValueError, match="corr_factor"):
        build_loss(_cfg(corr_factor=bad))
    with pytest.raises(ValueError, match="corr_factor"):
        corr_settings(_cfg(corr_factor=bad), rois=torch.zeros(1, 7, 2, dtype=torch.int64))
    assert build_loss(_cfg()) is build_loss(_cfg(corr_factor=5.0))        # keys absent (an older config) or valid: the same losswrapper


@pytest.mark.parametrize("bad", [0.0, -1e-8, math.nan, math.inf, "small", None])
def test_a_bad_eps_raises_where_the_loss_is_built(bad):
    from electrocardio_panorama_amd.network import build_loss, losswrapper
    with pytest.raises(ValueError, match="corr_eps"):
        build_loss(_cfg(corr_factor=5.0, corr_eps=bad))
    t = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="corr_eps"):
        losswrapper(t, t, t, t, _cfg(corr_factor=5.0, corr_eps=bad), rois=torch.zeros(2, 7, 2, dtype=torch.int64))
    build_loss(_cfg(corr_factor=0.0, corr_eps=bad))                       # off: the other keys are not looked at


def test_crop_without_rois_raises_before_any_device_work():
    """CPU tensors: the ValueError comes before the first launch (which would reject them)."""
    from electrocardio_panorama_amd.network import losswrapper
    from electrocardio_panorama_amd.network.loss.losses import check_corr_rows, corr_settings
    t = torch.zeros(2, 1, 16)
    with pytest.raises(ValueError, match="corr_crop"):
        losswrapper(t, t, t, t, _cfg(corr_factor=5.0, corr_crop=True))
    with pytest.raises(ValueError, match="corr_crop"):
        losswrapper(t, t, t, t, _cfg(corr_factor=5.0))                   # the key's default is True
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    assert corr_settings(_cfg(corr_factor=5.0), rois)[2] is rois
    assert corr_settings(_cfg(corr_factor=5.0), rois)[:2] == (5.0, 1e-8)
    assert corr_settings(_cfg(corr_factor=5.0, corr_eps=1e-6, corr_crop=False), rois) == (5.0, 1e-6, None)
    assert corr_settings(_cfg(corr_factor=0.0, corr_crop=True, corr_eps=-1.0)) == (0.0, 1e-8, None)      # off: nothing asked for
    assert corr_settings(_cfg()) == (0.0, 1e-8, None)
    assert corr_settings(_cfg(corr_factor=5.0), need_rois=False) == (5.0, 1e-8, None)
    check_corr_rows(65535)
    with pytest.raises(ValueError, match="corr_factor"):
        check_corr_rows(65536)
    with pytest.raises(ValueError, match="65535"):
        losswrapper(torch.zeros(65536, 1, 4), t, t, t, _cfg(corr_factor=5.0, corr_crop=False))


def test_losswrapper_tuple_lengths_with_the_keys_off(monkeypatch):
    """4 (train) and 5 (test) elements with the key off or absent, rois= given or not, and only ops.loss_fwd is called -- checked on the
    host with the ops replaced by recorders; with the key on the term is the last element of both forms, behind the SSIM and slope terms
    when they are on, and those keep being handed the part of the row that ends at their own element."""
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

    def fake_corr(pred, tgt, losses, factor, eps, rois=None, noise=None):
        calls.append(("loss_corr_fwd", losses.numel(), factor, eps, rois is not None))
        losses[-1] = 6.0
        return losses

    monkeypatch.setattr(ops, "loss_fwd", fake_fwd)
    monkeypatch.setattr(ops, "loss_ssim_fwd", fake_ssim)
    monkeypatch.setattr(ops, "loss_slope_fwd", fake_slope)
    monkeypatch.setattr(ops, "loss_corr_fwd", fake_corr)
    t = torch.zeros(2, 1, 16)
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    for cfg in (_cfg(), _cfg(corr_factor=0.0, corr_crop=True, corr_eps=1e-3, corr_eval=True)):
        for kw in ({}, {"rois": rois}):
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, **kw)) == 4
            assert calls == [("loss_fwd", None)]
            calls.clear()
            assert len(losswrapper(t, t, t, t, cfg, t, t, **kw)) == 5
            assert calls == [("loss_fwd", None), ("loss_fwd", None)]
    on = _cfg(corr_factor=5.0)
    calls.clear()
    train = losswrapper(t, t, t, t, on, rois=rois)
    assert len(train) == 5 and float(train[-1]) == 6.0 and [float(v) for v in train[:4]] == [0.0, 1.0, 2.0, 3.0]
    assert calls == [("loss_fwd", 5), ("loss_corr_fwd", 5, 5.0, 1e-8, True)]
    test = losswrapper(t, t, t, t, on, t, t, rois=rois)
    assert len(test) == 6 and float(test[-1]) == 6.0 and float(test[4]) == 3.0          # loss_unsperv keeps index 4
    calls.clear()
    assert len(losswrapper(t, t, t, t, _cfg(corr_factor=5.0, corr_crop=False, corr_eps=1e-6))) == 5
    assert calls[-1] == ("loss_corr_fwd", 5, 5.0, 1e-6, False)
    # all three tail terms: (loss, l1, l2, l3[, unsup], ssim, slope, corr)
    three = _cfg(corr_factor=5.0, slope_factor=2.0, ssim_factor=0.5)
    calls.clear()
    train = losswrapper(t, t, t, t, three, rois=rois)
    assert len(train) == 7 and [float(train[k]) for k in (4, 5, 6)] == [9.0, 7.0, 6.0]
    assert calls == [("loss_fwd", 7), ("loss_ssim_fwd", 5, 0.5, True), ("loss_slope_fwd", 6, 2.0, False, True),
                     ("loss_corr_fwd", 7, 5.0, 1e-8, True)]
    test = losswrapper(t, t, t, t, three, t, t, rois=rois)
    assert len(test) == 8 and [float(test[k]) for k in (4, 5, 6, 7)] == [3.0, 9.0, 7.0, 6.0]
    # slope + corr, SSIM + corr
    calls.clear()
    train = losswrapper(t, t, t, t, _cfg(corr_factor=5.0, slope_factor=2.0), rois=rois)
    assert len(train) == 6 and [float(train[k]) for k in (4, 5)] == [7.0, 6.0]
    assert calls == [("loss_fwd", 6), ("loss_slope_fwd", 5, 2.0, False, True), ("loss_corr_fwd", 6, 5.0, 1e-8, True)]
    calls.clear()
    train = losswrapper(t, t, t, t, _cfg(corr_factor=5.0, ssim_factor=0.5), rois=rois)
    assert len(train) == 6 and [float(train[k]) for k in (4, 5)] == [9.0, 6.0]
    assert calls == [("loss_fwd", 6), ("loss_ssim_fwd", 5, 0.5, True), ("loss_corr_fwd", 6, 5.0, 1e-8, True)]
    # the other terms alone are what they were
    calls.clear()
    assert len(losswrapper(t, t, t, t, _cfg(ssim_factor=0.5, slope_factor=2.0), rois=rois)) == 6
    assert calls == [("loss_fwd", 6), ("loss_ssim_fwd", 5, 0.5, True), ("loss_slope_fwd", 6, 2.0, False, True)]


def test_solver_names_the_tail_terms_in_row_order():
    from electrocardio_panorama_amd.solver.solver import Solver, corr_pairs
    s = Solver.__new__(Solver)
    s.cfg = _cfg(corr_factor=5.0, ssim_factor=0.5)
    assert s._tail_terms() == ["ssim", "corr"]
    s.cfg = _cfg(corr_factor=5.0, slope_factor=1.0, ssim_factor=0.5)
    assert s._tail_terms() == ["ssim", "slope", "corr"]
    s.cfg = _cfg()
    assert s._tail_terms() == []
    # the host's r: pairs with fewer than two samples are left out; no pair at all is an empty array (logged as NaN)
    mom = np.array([[[0.01, 0.04, 0.01]], [[0.0, 0.0, 0.0]], [[0.5, 0.5, 0.5]]])
    r = corr_pairs(mom, np.array([[40], [40], [1]]), 1e-8)
    assert r.shape == (2,) and abs(r[0] - (0.01 + 1e-8) / math.sqrt((0.01 + 1e-8) * (0.04 + 1e-8))) < 1e-15 and r[1] == 1.0
    assert corr_pairs(mom, np.array([[1], [0], [1]]), 1e-8).size == 0
