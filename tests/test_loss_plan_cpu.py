"""CPU: network.loss.losses.LossPlan -- the one owner of the order, the row layout and the launch sequence of the loss terms behind the
reference's four (SOLVER.seg_weights, ssim_factor, slope_factor, corr_factor).  All 16 on/off combinations against a literal table of what
the eager loss and the graphed step issued before the plan existed, with the ops replaced by recorders (no device); the rois tiled once
for a multi-view prediction; MSELead; the row limits."""
import itertools

import pytest
import torch

SEG = (1.0, 1.0, 3.0, 2.0, 1.0, 1.0, 0.0)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(seg=False, ssim=False, slope=False, corr=False, crop=True):
    solver = dict(optim="sgd", lr=0.1, reg_loss="l1_loss", loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], ssim_crop=crop, slope_crop=crop,
                  corr_crop=crop)
    if seg:
        solver["seg_weights"] = list(SEG)
    if ssim:
        solver["ssim_factor"] = 0.5
    if slope:
        solver.update(slope_factor=2.0, slope_loss="l2_loss")
    if corr:
        solver.update(corr_factor=5.0, corr_eps=1e-6)
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=3, noise=False), SOLVER=Cfg(**solver))


# (seg, ssim, slope, corr) -> names, row_len, the forward launches behind loss_fwd with the elements of the row each is handed
TABLE = {
    (0, 0, 0, 0): ([], 4, []),
    (0, 0, 0, 1): (["corr"], 5, [("corr", 5)]),
    (0, 0, 1, 0): (["slope"], 5, [("slope", 5)]),
    (0, 0, 1, 1): (["slope", "corr"], 6, [("slope", 5), ("corr", 6)]),
    (0, 1, 0, 0): (["ssim"], 5, [("ssim", 5)]),
    (0, 1, 0, 1): (["ssim", "corr"], 6, [("ssim", 5), ("corr", 6)]),
    (0, 1, 1, 0): (["ssim", "slope"], 6, [("ssim", 5), ("slope", 6)]),
    (0, 1, 1, 1): (["ssim", "slope", "corr"], 7, [("ssim", 5), ("slope", 6), ("corr", 7)]),
    (1, 0, 0, 0): ([], 4, [("seg", 4)]),
    (1, 0, 0, 1): (["corr"], 5, [("seg", 4), ("corr", 5)]),
    (1, 0, 1, 0): (["slope"], 5, [("seg", 4), ("slope", 5)]),
    (1, 0, 1, 1): (["slope", "corr"], 6, [("seg", 4), ("slope", 5), ("corr", 6)]),
    (1, 1, 0, 0): (["ssim"], 5, [("seg", 5), ("ssim", 5)]),
    (1, 1, 0, 1): (["ssim", "corr"], 6, [("seg", 5), ("ssim", 5), ("corr", 6)]),
    (1, 1, 1, 0): (["ssim", "slope"], 6, [("seg", 5), ("ssim", 5), ("slope", 6)]),
    (1, 1, 1, 1): (["ssim", "slope", "corr"], 7, [("seg", 5), ("ssim", 5), ("slope", 6), ("corr", 7)]),
}
# what every call of a term carries behind the row: factor and extras (seg: weights, f2, reg_l2; its backward: the weights)
SCALARS = {"seg": (SEG, 1.0, False), "ssim": (0.5,), "slope": (2.0, True), "corr": (5.0, 1e-6)}
COMBOS = list(itertools.product((0, 1), repeat=4))
assert sorted(TABLE) == COMBOS


def _fwd(term, n, crop=True):
    return (f"loss_{term}_fwd", n) + SCALARS[term] + (term == "seg" or crop,)


def _bwd(term, crop=True, gscale=True):
    if term == "seg":
        return ("loss_seg_bwd", SEG, True)
    return (f"loss_{term}_bwd",) + SCALARS[term] + (crop, gscale)


@pytest.fixture
def recorded(monkeypatch):
    """ops.loss_* replaced by recorders: (op, row elements handed in, scalars, whether rois came; backward: whether gscale came)."""
    from electrocardio_panorama_amd import ops
    calls, rois_seen = [], []

    def loss_fwd(pred, pp, pl, tgt, factors, reg_l2, use_mask, out=None, noise=None):
        calls.append(("loss_fwd", None if out is None else out.numel()))
        row = torch.zeros(4) if out is None else out
        row[:4] = torch.arange(4, dtype=torch.float32)
        return row

    def loss_bwd(pred, pp, pl, tgt, gscale, factors, reg_l2, use_mask, noise=None):
        calls.append(("loss_bwd",))
        return torch.zeros_like(pred), torch.zeros_like(pp), torch.zeros_like(pl)

    def seg_fwd(pred, tgt, losses, weights, f2, reg_l2, rois, noise=None):
        calls.append(("loss_seg_fwd", losses.numel(), tuple(weights), f2, reg_l2, rois is not None))
        rois_seen.append(rois)

    def seg_bwd(g_pred, weights, rois):
        calls.append(("loss_seg_bwd", tuple(weights), rois is not None))
        rois_seen.append(rois)

    def tail(name):
        def fwd(pred, tgt, losses, factor, *extra, rois=None, noise=None):
            calls.append((f"loss_{name}_fwd", losses.numel(), factor) + extra + (rois is not None,))
            rois_seen.append(rois)
            losses[-1] = 9.0

        def bwd(pred, tgt, g_pred, factor, *extra, rois=None, noise=None, gscale=None):
            calls.append((f"loss_{name}_bwd", factor) + extra + (rois is not None, gscale is not None))
            rois_seen.append(rois)
        return fwd, bwd

    for name, fn in (("loss_fwd", loss_fwd), ("loss_bwd", loss_bwd), ("loss_seg_fwd", seg_fwd), ("loss_seg_bwd", seg_bwd)):
        monkeypatch.setattr(ops, name, fn)
    for name in ("ssim", "slope", "corr"):
        fwd, bwd = tail(name)
        monkeypatch.setattr(ops, f"loss_{name}_fwd", fwd)
        monkeypatch.setattr(ops, f"loss_{name}_bwd", bwd)
    return calls, rois_seen


def _eager(cfg, shape=(2, 1, 16), rois_rows=2):
    from electrocardio_panorama_amd.network import losswrapper
    pred = torch.zeros(shape, requires_grad=True)
    t = torch.zeros(shape)
    out = losswrapper(pred, t, t, t, cfg, rois=torch.zeros(rois_rows, 7, 2, dtype=torch.int32))
    out[0].backward()
    return out


@pytest.mark.parametrize("combo", COMBOS, ids=["".join(map(str, c)) for c in COMBOS])
def test_the_eager_loss_issues_what_the_table_says(recorded, combo):
    calls, _ = recorded
    names, row_len, fwd = TABLE[combo]
    out = _eager(_cfg(*combo))
    assert len(out) == row_len
    assert calls == ([("loss_fwd", row_len if fwd else None)] + [_fwd(t, n) for t, n in fwd] +
                     [("loss_bwd",)] + [_bwd(t) for t, _ in fwd])


@pytest.mark.parametrize("combo", COMBOS, ids=["".join(map(str, c)) for c in COMBOS])
def test_the_plan_holds_what_the_table_says(recorded, combo):
    from electrocardio_panorama_amd.network.loss.losses import LossPlan
    calls, _ = recorded
    names, row_len, fwd = TABLE[combo]
    plan = LossPlan.from_cfg(_cfg(*combo))
    assert (plan.names, plan.row_len, plan.any_on, plan.needs_rois) == (names, row_len, any(combo), any(combo))
    assert plan.seg_weights == (SEG if combo[0] else None)
    assert [(t.name, t.factor, t.crop) + t.extra for t in plan.tail] == [(n, SCALARS[n][0], True) + SCALARS[n][1:] for n in names]
    # driven as the captured step drives it: per term its forward, then its backward (no gscale: the captured backward's is 1)
    x, rois, row = torch.zeros(2, 1, 16), torch.zeros(2, 7, 2, dtype=torch.int64), torch.zeros(row_len)
    for step in plan:
        step.fwd(x, x, row, rois, None)
        step.bwd(x, x, x, rois, None)
    assert calls == [c for t, n in fwd for c in (_fwd(t, n), _bwd(t, gscale=False))]


def test_everything_off_is_the_empty_plan():
    from electrocardio_panorama_amd.network.loss.losses import LossPlan
    off = LossPlan()
    assert (off.names, off.row_len, off.any_on, off.needs_rois, off.seg_weights, list(off)) == ([], 4, False, False, None, [])


def test_crop_flags_off(recorded):
    """Whole rows: the tail terms are handed no rois, the segment weights always are; any_on does not look at the crop flags."""
    from electrocardio_panorama_amd.network.loss.losses import LossPlan
    calls, _ = recorded
    fwd = TABLE[(1, 1, 1, 1)][2]
    _eager(_cfg(1, 1, 1, 1, crop=False))
    assert calls == ([("loss_fwd", 7)] + [_fwd(t, n, crop=False) for t, n in fwd] + [("loss_bwd",)] + [_bwd(t, crop=False) for t, _ in fwd])
    plan = LossPlan.from_cfg(_cfg(1, 1, 1, 1, crop=False))
    assert plan.any_on and plan.needs_rois and [t.crop for t in plan.tail] == [False] * 3
    calls.clear()
    x, rois, row = torch.zeros(2, 1, 16), torch.zeros(2, 7, 2, dtype=torch.int64), torch.zeros(7)
    for step in plan:
        step.fwd(x, x, row, rois, None)
        step.bwd(x, x, x, rois, None)
    assert calls == [c for t, n in fwd for c in (_fwd(t, n, crop=False), _bwd(t, crop=False, gscale=False))]
    tails = LossPlan.from_cfg(_cfg(0, 1, 1, 1, crop=False))
    assert tails.any_on and not tails.needs_rois
    # ... and without rois the loss runs: nothing asks for them
    from electrocardio_panorama_amd.network import losswrapper
    t = torch.zeros(2, 1, 16)
    assert len(losswrapper(t, t, t, t, _cfg(0, 1, 1, 1, crop=False))) == 7


def test_multi_view_rois_are_tiled_once(recorded):
    """[Q, B, 1, L] with rois [B, 7, 2]: one int64 [Q * B, 7, 2] tensor, the same object in every launch of the forward and the backward."""
    calls, rois_seen = recorded
    out = _eager(_cfg(1, 1, 1, 1), shape=(2, 3, 1, 16), rois_rows=3)
    assert len(out) == 7 and len(calls) == 10 and len(rois_seen) == 8
    first = rois_seen[0]
    assert tuple(first.shape) == (6, 7, 2) and first.dtype == torch.int64
    assert all(r is first for r in rois_seen)


def test_mselead_is_one_loss_launch(recorded):
    from electrocardio_panorama_amd.network import MSELead
    calls, _ = recorded
    x = torch.zeros(2, 3, 16)
    MSELead()(x, x)
    assert calls == [("loss_fwd", None)]


@pytest.mark.parametrize("combo,key", [((1, 0, 0, 0), "seg_weights"), ((0, 0, 1, 0), "slope_factor"), ((0, 0, 0, 1), "corr_factor")])
def test_row_limit_of_each_term(combo, key):
    from electrocardio_panorama_amd.network.loss.losses import LossPlan
    plan = LossPlan.from_cfg(_cfg(*combo))
    plan.check_rows(65535)
    plan.check_rows(65535, views=3)
    with pytest.raises(ValueError, match=key):
        plan.check_rows(65536)
    with pytest.raises(ValueError, match="65535"):
        plan.check_rows(65536, views=2)


def test_row_limit_of_the_ssim_term_is_the_multi_view_steps(recorded):
    from electrocardio_panorama_amd.network import losswrapper
    from electrocardio_panorama_amd.network.loss.losses import LossPlan
    plan = LossPlan.from_cfg(_cfg(0, 1, 0, 0))
    plan.check_rows(65536)                       # a single-view step: the batch is the SSIM op's own affair
    plan.check_rows(65535, views=3)
    with pytest.raises(ValueError, match="ssim_factor"):
        plan.check_rows(65536, views=2)
    big = torch.zeros(65536, 1, 4)
    assert len(losswrapper(big, big, big, big, _cfg(0, 1, 0, 0, crop=False))) == 5      # 3-dim prediction: no check fires
    with pytest.raises(ValueError, match="ssim_factor"):
        losswrapper(big.reshape(2, 32768, 1, 4), big, big, big, _cfg(0, 1, 0, 0, crop=False))
    LossPlan().check_rows(1 << 20, views=2)      # nothing on: nothing to check
