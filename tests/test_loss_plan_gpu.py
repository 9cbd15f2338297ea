"""LossPlan on the device with every term on at once (SOLVER.seg_weights + ssim_factor + slope_factor + corr_factor) -- the one combination
the per-term suites leave out: losswrapper + backward against the ten ops issued by hand in the documented order, bit for bit, and the
graphed multi-view step against the eager one (the helper scheme of tests/test_corr_loss_gpu.py)."""
import random

import numpy as np
import pytest
import torch

from corr_ref import EPS, case, rois_of
from test_corr_loss_gpu import _batches, _solver, _state
from test_model_gpu import DEV, make_cfg

pytestmark = pytest.mark.gpu

FACTORS = (0.5, 0.5, 1.0)
SEG = [1, 1, 3, 2, 1, 1, 0]
KEYS = dict(seg_weights=SEG, ssim_factor=0.5, ssim_crop=True, slope_factor=2.0, slope_loss="l1_loss", slope_crop=True, corr_factor=5.0,
            corr_crop=True, corr_eps=EPS)


@pytest.mark.parametrize("views", [0, 2], ids=["B3", "Q2xB3"])
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noise"])
def test_all_four_on_equals_the_ops_by_hand(noisy, views):
    """B, L = 3, 500 with row ends [298, 2, 777]: a row too short for an SSIM window (one difference, two samples) and an end beyond L.
    [2, 3, 1, 500]: the same rois, tiled per view by losswrapper and by hand here."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.network import losswrapper
    B, L = 3, 500
    rois = rois_of([298, 2, 777]).to(DEV)
    shape = (views, B, 1, L) if views else (B, 1, L)
    out0, p0, l0, tgt, nz = (None if t is None else t.to(DEV).reshape(shape).contiguous() for t in case(B * max(views, 1), L, "close", noisy))
    cfg = make_cfg(3)
    cfg.SOLVER.update(KEYS)
    out, p, l_ = (t.clone().requires_grad_(True) for t in (out0, p0, l0))
    losses = losswrapper(out, p, l_, tgt, cfg, noise=nz, rois=rois)
    assert len(losses) == 7 and all(t.dim() == 0 for t in losses)
    (losses[0] * 0.5).backward()
    r = rois.repeat(views, 1, 1) if views else rois
    row = torch.zeros(7, device=DEV)
    ops.loss_fwd(out0, p0, l0, tgt, FACTORS, False, 7, out=row, noise=nz)
    ops.loss_seg_fwd(out0, tgt, row[:5], SEG, FACTORS[2], False, r, noise=nz)
    ops.loss_ssim_fwd(out0, tgt, row[:5], 0.5, rois=r, noise=nz)
    ops.loss_slope_fwd(out0, tgt, row[:6], 2.0, False, rois=r, noise=nz)
    ops.loss_corr_fwd(out0, tgt, row, 5.0, EPS, rois=r, noise=nz)
    gs = torch.zeros(7, device=DEV)
    gs[0] = 0.5
    g3 = ops.loss_bwd(out0, p0, l0, tgt, gs, FACTORS, False, 7, noise=nz)
    ops.loss_seg_bwd(g3[0], SEG, r)
    ops.loss_ssim_bwd(out0, tgt, g3[0], 0.5, rois=r, noise=nz, gscale=gs)
    ops.loss_slope_bwd(out0, tgt, g3[0], 2.0, False, rois=r, noise=nz, gscale=gs)
    ops.loss_corr_bwd(out0, tgt, g3[0], 5.0, EPS, rois=r, noise=nz, gscale=gs)
    assert torch.equal(torch.stack([t.detach() for t in losses]), row)
    for a, b in zip((out.grad, p.grad, l_.grad), g3):
        assert torch.equal(a, b)
    assert all(float(row[k]) > 0 for k in range(3, 7))


def test_graphed_equals_eager_all_four_on_two_views():
    """Three SGD steps of the multi-view step with every term on: parameters, momentum, BatchNorm statistics and the seven-element loss
    rows of the replayed step equal the eager ones bit for bit, from one capture on the rois tiled per view."""
    V, B, L = 3, 2, 512
    batches = _batches(3, B, V, L, 40)
    res = {}
    for graph in (False, True):
        cfg, sol, opt = _solver(V, "sgd", graph, train_views=2, **KEYS)
        rows = []
        for i, b in enumerate(batches):
            random.seed(100 + i)
            rows.append(np.array(sol.run_one_epoch([b], "train", opt, collect_views=False)[0]))
        rows = np.concatenate(rows)
        assert rows.shape == (3, 7) and (rows[:, 3:] > 0).all()
        if graph:
            st = sol._graph_stepper
            assert st is not None and len(st.slots) == 1 and st.calls == 3 and st.losses.numel() == 7 and st.rois_q is not None
        else:
            assert getattr(sol, "_graph_stepper", None) is None
        res[graph] = (_state(sol, opt, "sgd"), rows)
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    assert np.array_equal(res[False][1], res[True][1])
