"""`losswrapper` of reference codes/network/loss/losses.py:21-50 on the HIP loss kernels, and `LossPlan`: the one owner of the terms behind
the reference's four -- their order, the loss row's layout and the launch sequence the eager loss, the graphed step and the solver share."""
from typing import NamedTuple

import torch

from ... import ops

def _tail_rule(cfg, key):
    """(SOLVER.<key>_factor, whether the term crops its rows at rois[i, -1, 0]).  A negative (or NaN) factor raises ValueError; factor 0:
    (0.0, False), whatever else is set."""
    factor = float(cfg.SOLVER.get(key + '_factor', 0.0))       # (.get: configs written before the key existed)
    if not factor >= 0.0:
        raise ValueError(f"Invalid SOLVER.{key}_factor: {factor} (it must be >= 0)")
    return factor, factor > 0 and bool(cfg.SOLVER.get(key + '_crop', True))


def _crop_rois(key, crop, rois, need_rois=True):
    """The rois a term crops its rows with, or None for whole rows; ValueError when it crops and the batch's rois are missing."""
    if crop and rois is None and need_rois:
        raise ValueError(f"SOLVER.{key}_crop is set: {TAIL[key][0]} needs this batch's rois (losswrapper(..., rois=)); "
                         f"set SOLVER.{key}_crop False to take whole rows")
    return rois if crop else None


def _slope_l2(cfg):
    norm = cfg.SOLVER.get('slope_loss', 'l1_loss')
    if norm not in ('l1_loss', 'l2_loss'):
        raise ValueError(f"Invalid SOLVER.slope_loss: {norm!r} ('l1_loss' or 'l2_loss')")
    return norm == 'l2_loss'


CORR_EPS = 1e-8            # SOLVER.corr_eps' default


def _corr_eps(cfg):
    try:
        eps = float(cfg.SOLVER.get('corr_eps', CORR_EPS))
    except (TypeError, ValueError):
        raise ValueError(f"Invalid SOLVER.corr_eps: {cfg.SOLVER.get('corr_eps')!r} (a number is needed)") from None
    if not 0.0 < eps < float('inf'):                           # (NaN fails <)
        raise ValueError(f"Invalid SOLVER.corr_eps: {eps} (it must be positive and finite)")
    return eps


# The terms behind the reference's four, in the row's order (and the order of their launches): name -> (what the messages call it, its
# scalars behind the factor in the order its two ops take them -- read only while the term is on)
TAIL = {'ssim': ('the SSIM term', lambda cfg: ()),
        'slope': ('the slope term', lambda cfg: (_slope_l2(cfg),)),
        'corr': ('the correlation term', lambda cfg: (_corr_eps(cfg),))}


def ssim_settings(cfg, rois=None, need_rois=True):
    """(SOLVER.ssim_factor, the rois the SSIM term crops its rows with or None for whole rows).  A negative (or NaN) factor and
    ssim_crop without rois raise ValueError; factor 0: (0.0, None), whatever else is set."""
    factor, crop = _tail_rule(cfg, 'ssim')
    return factor, _crop_rois('ssim', crop, rois, need_rois)


def slope_settings(cfg, rois=None, need_rois=True):
    """(SOLVER.slope_factor, whether SOLVER.slope_loss is 'l2_loss', the rois the slope term crops its rows with or None for whole rows).
    A negative (or NaN) factor, an unknown slope_loss and slope_crop without rois raise ValueError; factor 0: (0.0, False, None), whatever
    else is set."""
    factor, crop = _tail_rule(cfg, 'slope')
    return factor, factor > 0 and _slope_l2(cfg), _crop_rois('slope', crop, rois, need_rois)


def corr_settings(cfg, rois=None, need_rois=True):
    """(SOLVER.corr_factor, SOLVER.corr_eps, the rois the correlation term crops its rows with or None for whole rows).  A negative (or
    NaN) factor, a corr_eps that is not positive and finite, and corr_crop without rois raise ValueError; factor 0: (0.0, corr_eps' default,
    None), whatever else is set."""
    factor, crop = _tail_rule(cfg, 'corr')
    return factor, _corr_eps(cfg) if factor > 0 else CORR_EPS, _crop_rois('corr', crop, rois, need_rois)


SEG_NAMES = ('P', 'PR', 'QRS', 'ST', 'T', 'TP', 'pad')


def seg_settings(cfg):
    """SOLVER.seg_weights as a 7-tuple of floats [P, PR, QRS, ST, T, TP, pad], or None when the key is empty (off).  ValueError for a
    wrong length, a negative or non-finite entry, all zeros, or the key on while the reconstruction term (3) is not in SOLVER.loss_using."""
    raw = cfg.SOLVER.get('seg_weights', None)               # (.get: configs written before the key existed)
    if raw is None or len(raw) == 0:
        return None
    if len(raw) != len(SEG_NAMES):
        raise ValueError(f"Invalid SOLVER.seg_weights: {list(raw)} ({len(SEG_NAMES)} numbers are needed: {list(SEG_NAMES)}, or [] for off)")
    try:
        w = tuple(float(x) for x in raw)
    except (TypeError, ValueError):
        raise ValueError(f"Invalid SOLVER.seg_weights: {list(raw)} (numbers are needed)") from None
    if not all(0.0 <= x < float('inf') for x in w):         # (NaN fails <=)
        raise ValueError(f"Invalid SOLVER.seg_weights: {list(w)} (every weight must be finite and >= 0)")
    if not any(x > 0.0 for x in w):
        raise ValueError(f"Invalid SOLVER.seg_weights: {list(w)} (not all weights may be zero; [] switches the key off)")
    if 3 not in cfg.SOLVER.loss_using:
        raise ValueError("SOLVER.seg_weights weighs the reconstruction term, which SOLVER.loss_using leaves out: add 3 to "
                         "SOLVER.loss_using or set SOLVER.seg_weights []")
    return w


SSIM_MAX_ROWS = 65535      # every term's launches take the (view, sample) rows as a grid's y extent


def _check_rows(rows, name, what=None):
    """The one row limit, worded for the key `name` ('seg' or one of TAIL) that ran into it."""
    if rows > SSIM_MAX_ROWS:
        takes, off = (("the segment weights (SOLVER.seg_weights) take", "SOLVER.seg_weights []") if name == 'seg' else
                      (f"{TAIL[name][0]} (SOLVER.{name}_factor) takes", f"SOLVER.{name}_factor 0"))
        raise ValueError(f"{what or f'{rows} rows (SOLVER.train_views x the batch)'} is more than the {SSIM_MAX_ROWS} {takes}: "
                         f"lower SOLVER.train_views or the batch size, or set {off}")


def check_view_rows(Q, B):
    """The SSIM term of a multi-view step takes its Q * B (view, sample) pairs as rows."""
    _check_rows(Q * B, 'ssim', f"SOLVER.train_views ({Q}) x the batch ({B}) = {Q * B} rows")


def check_corr_rows(rows):
    """The correlation term's launches take every (view, sample) row as one y index of their grid."""
    _check_rows(rows, 'corr')


class _SegStep(NamedTuple):
    """SOLVER.seg_weights: the reconstruction term and the total rewritten in front of the tail terms; the gradient scaled in place."""
    weights: tuple
    f2: float          # the reconstruction term's SOLVER.loss_factor
    reg_l2: bool
    n_row: int         # the row's elements the forward is handed: up to the SSIM term's
    name = 'seg'

    def fwd(self, pred, target, row, rois, noise):
        ops.loss_seg_fwd(pred, target, row[:self.n_row], self.weights, self.f2, self.reg_l2, rois, noise=noise)

    def bwd(self, pred, target, g_pred, rois, noise, gscale=None):
        ops.loss_seg_bwd(g_pred, self.weights, rois)


class _TailStep(NamedTuple):
    """One term of TAIL that is on: ops.loss_<name>_fwd writes the row's element n_row - 1 and adds it into the total, ops.loss_<name>_bwd
    accumulates onto the reconstruction term's gradient.  The ops are looked up when the step runs."""
    name: str
    factor: float
    crop: bool
    extra: tuple       # behind the factor: slope (l2,), corr (eps,)
    n_row: int         # the row's elements the forward is handed: up to the term's own

    def fwd(self, pred, target, row, rois, noise):
        getattr(ops, f'loss_{self.name}_fwd')(pred, target, row[:self.n_row], self.factor, *self.extra,
                                              rois=rois if self.crop else None, noise=noise)

    def bwd(self, pred, target, g_pred, rois, noise, gscale=None):
        getattr(ops, f'loss_{self.name}_bwd')(pred, target, g_pred, self.factor, *self.extra,
                                              rois=rois if self.crop else None, noise=noise, gscale=gscale)


class LossPlan:
    """What follows ops.loss_fwd / ops.loss_bwd: the segment weights, then the TAIL terms that are on.  Iterating yields the steps in launch
    order; the eager loss runs every `fwd` in its forward and every `bwd` in its backward, the captured step `fwd` then `bwd` per step.
    The loss row is (loss, l1, l2, l3) + one element per tail term in `names` order.  LossPlan() is everything off."""

    def __init__(self, seg_weights=None, f2=0.0, reg_l2=False, tail=()):
        """`tail`: (name, factor, crop, extra) of the terms that are on, in TAIL's order."""
        self.seg_weights = seg_weights
        self.tail = [_TailStep(*t, n_row=5 + k) for k, t in enumerate(tail)]
        self.names = [t.name for t in self.tail]
        self.row_len = 4 + len(self.tail)
        seg = [] if seg_weights is None else [_SegStep(seg_weights, f2, reg_l2, n_row=5 if 'ssim' in self.names else 4)]
        self.steps = seg + self.tail
        self.any_on = bool(self.steps)
        self.needs_rois = seg_weights is not None or any(t.crop for t in self.tail)

    @classmethod
    def from_cfg(cls, cfg):
        """The plan `cfg` asks for; every key's ValueError is its settings rule's."""
        tail = []
        for name in TAIL:
            factor, crop = _tail_rule(cfg, name)
            if factor > 0:
                tail.append((name, factor, crop, TAIL[name][1](cfg)))
        seg = seg_settings(cfg)
        if seg is None:
            return cls(tail=tail)
        return cls(seg, float(cfg.SOLVER.loss_factor[2]), cfg.SOLVER.reg_loss == 'l2_loss', tail)

    def __iter__(self):
        return iter(self.steps)

    def require_rois(self, rois):
        """ValueError when a term needs the batch's rois and there are none."""
        for t in self.tail:
            _crop_rois(t.name, t.crop, rois)
        if self.seg_weights is not None and rois is None:
            raise ValueError("SOLVER.seg_weights is set: the loss needs this batch's rois (losswrapper(..., rois=)); "
                             "set SOLVER.seg_weights [] to switch the weights off")

    def check_rows(self, rows, views=None):
        """Every term that is on takes at most SSIM_MAX_ROWS (view, sample) rows.  `views`: Q of a multi-view step; the SSIM term is
        checked for those only (a single-view step's rows are the batch, which ops.loss_ssim_fwd takes as it comes)."""
        for step in self.steps:
            if step.name != 'ssim':
                _check_rows(rows, step.name)
            elif views is not None:
                check_view_rows(views, rows // views)


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, pred_p, pred_l, target, factors, reg_l2, use_mask, noise, plan, rois):
        pred, pred_p, pred_l, target = (t.contiguous() for t in (pred, pred_p, pred_l, target))
        ctx.save_for_backward(pred, pred_p, pred_l, target, noise, rois)
        ctx.cfg = (factors, reg_l2, use_mask, plan)
        if not plan.any_on:
            return ops.loss_fwd(pred, pred_p, pred_l, target, factors, reg_l2, use_mask, noise=noise)
        row = torch.empty(plan.row_len, device=pred.device, dtype=torch.float32)
        ops.loss_fwd(pred, pred_p, pred_l, target, factors, reg_l2, use_mask, out=row, noise=noise)
        for step in plan:           # each term added into the total by its own finish launch
            step.fwd(pred, target, row, rois, noise)
        return row

    @staticmethod
    def backward(ctx, g):
        pred, pred_p, pred_l, target, noise, rois = ctx.saved_tensors
        factors, reg_l2, use_mask, plan = ctx.cfg
        g = g.contiguous()
        g_pred, g_p, g_l = ops.loss_bwd(pred, pred_p, pred_l, target, g, factors, reg_l2, use_mask, noise=noise)
        for step in plan:           # onto the reconstruction term's gradient, in the same stream behind it
            step.bwd(pred, target, g_pred, rois, noise, g)
        return g_pred, g_p, g_l, None, None, None, None, None, None, None


def _rows_rois(rois, predict):
    """int64 contiguous rois for the rows of `predict`: [B, 7, 2] tiled once per view for a multi-view prediction [Q, B, 1, L];
    [Q * B, 7, 2] is taken as it is."""
    if predict.dim() == 4 and rois.shape[0] == predict.shape[1]:
        rois = rois.repeat(predict.shape[0], 1, 1)
    return rois.detach().to(torch.int64).contiguous()


def losswrapper(predict, predict_shuffle_p, predict_shuffle_l, target, cfg, rest_out=None, rest_view=None,
                loss1_gt=None, loss2_gt=None, noise=None, rois=None):
    """Returns (loss, f0*loss1, f1*loss2, f2*loss3[, loss_unsperv][, loss_ssim][, loss_slope][, loss_corr]) as 0-dim tensors; `loss` supports
    .backward().  The Standin terms compare against the detached prediction (OurLoss1, losses.py:5-18).  The elements behind loss_unsperv
    are LossPlan's tail terms that are on, in its order; `loss` includes them.
    `noise` (behind the reference's signature): cfg.DATA.noise's per-sample row, [B, 1, L] or anything that expands to the prediction's
    shape.  Every term is taken at predict + noise inside the loss kernels -- the reference's `out = out + noise` between model and loss
    (solver.py:185-186), bit for bit, without a kernel of its own; the rest_out / rest_view term never sees it.
    `rois` (behind `noise`; no counterpart in the reference): the batch's int64 [B, 7, 2] rois, required by cfg.SOLVER.seg_weights and by a
    tail term with its `*_crop` key set (rows end at rois[i, -1, 0]); not looked at otherwise.
    Multi-view steps (SOLVER.train_views; Model_nefnet.forward with query_theta [Q, B, 2]): predictions and target are [Q, B, 1, L], every
    term's rows are the Q * B (view, sample) pairs and `rois` [B, 7, 2] is tiled once per view here ([Q * B, 7, 2] is taken as it is).
    cfg.SOLVER.seg_weights: the reconstruction term becomes f2 * (1/n) * sum w[seg(i, t)] * e(i, t) (nef_loss_seg_args); the tuple keeps its length.
    cfg.SOLVER.ssim_factor > 0: + ssim_factor * (1 - mean SSIM(predict (+ noise), target)) (nef_loss_ssim_args).
    cfg.SOLVER.slope_factor > 0: + slope_factor * the mean |d| or d^2 of the first differences' difference (nef_loss_slope_args).
    cfg.SOLVER.corr_factor > 0: + corr_factor * the mean of 1 - Pearson's r with cfg.SOLVER.corr_eps (nef_loss_corr_args)."""
    plan = LossPlan.from_cfg(cfg)
    plan.require_rois(rois)
    plan.check_rows(predict.numel() // predict.shape[-1], predict.shape[0] if predict.dim() == 4 else None)
    rois = _rows_rois(rois, predict) if plan.needs_rois else None
    if cfg.SOLVER.reg_loss == 'l2_loss':
        reg_l2 = True
    elif cfg.SOLVER.reg_loss == 'l1_loss':
        reg_l2 = False
    else:
        raise NotImplementedError
    if loss1_gt is not None or loss2_gt is not None:
        raise NotImplementedError("loss1_gt / loss2_gt are only produced by model variants outside Nef-Net")
    using = cfg.SOLVER.loss_using
    use_mask = (1 if 1 in using else 0) | (2 if 2 in using else 0) | (4 if 3 in using else 0)
    factors = tuple(float(f) for f in cfg.SOLVER.loss_factor)
    target = target.to(torch.float32).expand_as(predict)
    if noise is not None:
        noise = noise.detach().to(torch.float32).expand_as(predict).contiguous()
    row = _LossFn.apply(predict, predict_shuffle_p, predict_shuffle_l, target, factors, reg_l2, use_mask, noise, plan, rois)
    result = (row[0],) + tuple(row[k].detach() for k in range(1, 4))
    tail = tuple(row[k].detach() for k in range(4, plan.row_len))
    if rest_out is not None and rest_view is not None:
        ro = rest_out.detach().to(torch.float32).contiguous()
        rv = rest_view.detach().to(torch.float32).contiguous()
        unsup = ops.loss_fwd(ro, ro, ro, rv, (0.0, 0.0, 1.0), reg_l2, 4)[3]
        return result + (unsup,) + tail
    return result + tail


class MSELead(torch.nn.Module):
    """Reference losses.py:53-64: the mean over leads of the per-lead MSE (unused by the Nef-Net path).  Every lead has
    the same number of elements, so this is the MSE over the whole tensor -- one pass of the loss kernels."""

    def forward(self, input, target):
        target = target.to(torch.float32).expand_as(input)
        # element [0] (the total) is the one _LossFn back-propagates through; with factors (0, 0, 1) and only the
        # reconstruction term enabled it IS the MSE (element [3] carries the same number but no gradient)
        return _LossFn.apply(input, input, input, target, (0.0, 0.0, 1.0), True, 4, None, LossPlan(), None)[0]
