"""`losswrapper` of reference codes/network/loss/losses.py:21-50 on the HIP loss kernels."""
import torch

from ... import ops


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, pred_p, pred_l, target, factors, reg_l2, use_mask, noise=None, ssim_factor=0.0, rois=None, seg_weights=None,
                seg_rois=None, slope_factor=0.0, slope_l2=False, slope_rois=None, corr_factor=0.0, corr_eps=1e-8, corr_rois=None):
        pred, pred_p, pred_l, target = (t.contiguous() for t in (pred, pred_p, pred_l, target))
        ctx.save_for_backward(pred, pred_p, pred_l, target, noise, rois, seg_rois, slope_rois, corr_rois)
        ctx.cfg = (factors, reg_l2, use_mask, ssim_factor, seg_weights, slope_factor, slope_l2, corr_factor, corr_eps)
        if not ssim_factor > 0 and seg_weights is None and not slope_factor > 0 and not corr_factor > 0:
            return ops.loss_fwd(pred, pred_p, pred_l, target, factors, reg_l2, use_mask, noise=noise)
        # SOLVER.ssim_factor / SOLVER.slope_factor / SOLVER.corr_factor: one more element each -- the SSIM term behind the four, then the
        # slope term, the correlation term last, each added into the total by its own finish launch
        n_front = 5 if ssim_factor > 0 else 4
        n_slope = n_front + (1 if slope_factor > 0 else 0)
        row = torch.empty(n_slope + (1 if corr_factor > 0 else 0), device=pred.device, dtype=torch.float32)
        ops.loss_fwd(pred, pred_p, pred_l, target, factors, reg_l2, use_mask, out=row, noise=noise)
        if seg_weights is not None:     # SOLVER.seg_weights: the reconstruction term and the total rewritten, in front of the SSIM term
            ops.loss_seg_fwd(pred, target, row[:n_front], seg_weights, factors[2], reg_l2, seg_rois, noise=noise)
        if ssim_factor > 0:
            ops.loss_ssim_fwd(pred, target, row[:5], ssim_factor, rois=rois, noise=noise)
        if slope_factor > 0:
            ops.loss_slope_fwd(pred, target, row[:n_slope], slope_factor, slope_l2, rois=slope_rois, noise=noise)
        if corr_factor > 0:
            ops.loss_corr_fwd(pred, target, row, corr_factor, corr_eps, rois=corr_rois, noise=noise)
        return row

    @staticmethod
    def backward(ctx, g):
        pred, pred_p, pred_l, target, noise, rois, seg_rois, slope_rois, corr_rois = ctx.saved_tensors
        factors, reg_l2, use_mask, ssim_factor, seg_weights, slope_factor, slope_l2, corr_factor, corr_eps = ctx.cfg
        g = g.contiguous()
        g_pred, g_p, g_l = ops.loss_bwd(pred, pred_p, pred_l, target, g, factors, reg_l2, use_mask, noise=noise)
        if seg_weights is not None:     # the reconstruction term's gradient times its position's weight, in place
            ops.loss_seg_bwd(g_pred, seg_weights, seg_rois)
        if ssim_factor > 0:         # accumulated onto the reconstruction term's gradient, in the same stream behind it
            ops.loss_ssim_bwd(pred, target, g_pred, ssim_factor, rois=rois, noise=noise, gscale=g)
        if slope_factor > 0:        # ... and the slope term's behind both
            ops.loss_slope_bwd(pred, target, g_pred, slope_factor, slope_l2, rois=slope_rois, noise=noise, gscale=g)
        if corr_factor > 0:         # ... and the correlation term's last
            ops.loss_corr_bwd(pred, target, g_pred, corr_factor, corr_eps, rois=corr_rois, noise=noise, gscale=g)
        return g_pred, g_p, g_l, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None


def ssim_settings(cfg, rois=None, need_rois=True):
    """(SOLVER.ssim_factor, the rois the SSIM term crops its rows with or None for whole rows).  A negative (or NaN) factor and
    ssim_crop without rois raise ValueError; factor 0: (0.0, None), whatever else is set."""
    factor = float(cfg.SOLVER.get('ssim_factor', 0.0))         # (.get: configs written before the key existed)
    if not factor >= 0.0:
        raise ValueError(f"Invalid SOLVER.ssim_factor: {factor} (it must be >= 0)")
    if factor == 0.0:
        return 0.0, None
    if not cfg.SOLVER.get('ssim_crop', True):
        return factor, None
    if rois is None and need_rois:
        raise ValueError("SOLVER.ssim_crop is set: the SSIM term needs this batch's rois (losswrapper(..., rois=)); "
                         "set SOLVER.ssim_crop False to take whole rows")
    return factor, rois


def slope_settings(cfg, rois=None, need_rois=True):
    """(SOLVER.slope_factor, whether SOLVER.slope_loss is 'l2_loss', the rois the slope term crops its rows with or None for whole rows).
    A negative (or NaN) factor, an unknown slope_loss and slope_crop without rois raise ValueError; factor 0: (0.0, False, None), whatever
    else is set."""
    factor = float(cfg.SOLVER.get('slope_factor', 0.0))        # (.get: configs written before the key existed)
    if not factor >= 0.0:
        raise ValueError(f"Invalid SOLVER.slope_factor: {factor} (it must be >= 0)")
    if factor == 0.0:
        return 0.0, False, None
    norm = cfg.SOLVER.get('slope_loss', 'l1_loss')
    if norm not in ('l1_loss', 'l2_loss'):
        raise ValueError(f"Invalid SOLVER.slope_loss: {norm!r} ('l1_loss' or 'l2_loss')")
    l2 = norm == 'l2_loss'
    if not cfg.SOLVER.get('slope_crop', True):
        return factor, l2, None
    if rois is None and need_rois:
        raise ValueError("SOLVER.slope_crop is set: the slope term needs this batch's rois (losswrapper(..., rois=)); "
                         "set SOLVER.slope_crop False to take whole rows")
    return factor, l2, rois


CORR_EPS = 1e-8            # SOLVER.corr_eps' default


def corr_settings(cfg, rois=None, need_rois=True):
    """(SOLVER.corr_factor, SOLVER.corr_eps, the rois the correlation term crops its rows with or None for whole rows).  A negative (or
    NaN) factor, a corr_eps that is not positive and finite, and corr_crop without rois raise ValueError; factor 0: (0.0, corr_eps' default,
    None), whatever else is set."""
    factor = float(cfg.SOLVER.get('corr_factor', 0.0))         # (.get: configs written before the key existed)
    if not factor >= 0.0:
        raise ValueError(f"Invalid SOLVER.corr_factor: {factor} (it must be >= 0)")
    if factor == 0.0:
        return 0.0, CORR_EPS, None
    try:
        eps = float(cfg.SOLVER.get('corr_eps', CORR_EPS))
    except (TypeError, ValueError):
        raise ValueError(f"Invalid SOLVER.corr_eps: {cfg.SOLVER.get('corr_eps')!r} (a number is needed)") from None
    if not 0.0 < eps < float('inf'):                           # (NaN fails <)
        raise ValueError(f"Invalid SOLVER.corr_eps: {eps} (it must be positive and finite)")
    if not cfg.SOLVER.get('corr_crop', True):
        return factor, eps, None
    if rois is None and need_rois:
        raise ValueError("SOLVER.corr_crop is set: the correlation term needs this batch's rois (losswrapper(..., rois=)); "
                         "set SOLVER.corr_crop False to take whole rows")
    return factor, eps, rois


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


SSIM_MAX_ROWS = 65535      # nef_loss_ssim_fwd / _bwd: the rows are a grid's y extent


def check_view_rows(Q, B):
    """The SSIM term of a multi-view step takes its Q * B (view, sample) pairs as rows."""
    if Q * B > SSIM_MAX_ROWS:
        raise ValueError(f"SOLVER.train_views ({Q}) x the batch ({B}) = {Q * B} rows is more than the {SSIM_MAX_ROWS} the SSIM term "
                         "(SOLVER.ssim_factor) takes: lower SOLVER.train_views or the batch size, or set SOLVER.ssim_factor 0")


def check_slope_rows(rows):
    """The slope term's launches take every (view, sample) row as one y index of their grid."""
    if rows > SSIM_MAX_ROWS:
        raise ValueError(f"{rows} rows (SOLVER.train_views x the batch) is more than the {SSIM_MAX_ROWS} the slope term "
                         "(SOLVER.slope_factor) takes: lower SOLVER.train_views or the batch size, or set SOLVER.slope_factor 0")


def check_corr_rows(rows):
    """The correlation term's launches take every (view, sample) row as one y index of their grid."""
    if rows > SSIM_MAX_ROWS:
        raise ValueError(f"{rows} rows (SOLVER.train_views x the batch) is more than the {SSIM_MAX_ROWS} the correlation term "
                         "(SOLVER.corr_factor) takes: lower SOLVER.train_views or the batch size, or set SOLVER.corr_factor 0")


def check_seg_rows(rows):
    """The segment-weight launches take every (view, sample) row as one y index of their grid."""
    if rows > SSIM_MAX_ROWS:
        raise ValueError(f"{rows} rows (SOLVER.train_views x the batch) is more than the {SSIM_MAX_ROWS} the segment weights "
                         "(SOLVER.seg_weights) take: lower SOLVER.train_views or the batch size, or set SOLVER.seg_weights []")


def _rows_rois(rois, predict):
    """int64 contiguous rois for the rows of `predict`: [B, 7, 2] tiled once per view for a multi-view prediction [Q, B, 1, L];
    [Q * B, 7, 2] is taken as it is."""
    if predict.dim() == 4 and rois.shape[0] == predict.shape[1]:
        rois = rois.repeat(predict.shape[0], 1, 1)
    return rois.detach().to(torch.int64).contiguous()


def losswrapper(predict, predict_shuffle_p, predict_shuffle_l, target, cfg, rest_out=None, rest_view=None,
                loss1_gt=None, loss2_gt=None, noise=None, rois=None):
    """Returns (loss, f0*loss1, f1*loss2, f2*loss3[, loss_unsperv][, loss_ssim][, loss_slope][, loss_corr]) as 0-dim tensors; `loss` supports .backward().
    The Standin terms compare against the detached prediction (OurLoss1, losses.py:5-18).
    `noise` (behind the reference's signature): cfg.DATA.noise's per-sample row, [B, 1, L] or anything that expands to the prediction's
    shape.  The three terms are taken at predict + noise inside the loss kernels -- the reference's `out = out + noise` between model
    and loss (solver.py:185-186), bit for bit, without a kernel of its own; the rest_out / rest_view term never sees it.
    `rois` (behind `noise`; no counterpart in the reference): the batch's int64 [B, 7, 2] rois.  With cfg.SOLVER.ssim_factor > 0 the tuple
    gains the SSIM term ssim_factor * (1 - mean SSIM(predict (+ noise), target)) as its LAST element and `loss` includes it; with
    cfg.SOLVER.ssim_crop the rows end at rois[i, -1, 0] as the test phase's ssim_gen does (rois is required then).  Factor 0: `rois` is
    not looked at and the tuple, the launches and the bits are what they were.
    Multi-view steps (SOLVER.train_views; Model_nefnet.forward with query_theta [Q, B, 2]): predictions and target are [Q, B, 1, L] and
    every term is the mean over all Q * B * L elements -- the mean over views, which have equal size.  The SSIM term's rows are the
    Q * B (view, sample) pairs; `rois` [B, 7, 2] is tiled once per view here ([Q * B, 7, 2] is taken as it is).
    cfg.SOLVER.seg_weights [P, PR, QRS, ST, T, TP, pad]: the reconstruction term becomes f2 * (1/n) * sum w[seg(i, t)] * e(i, t) over all
    n elements, seg(i, t) from `rois` (required then; tiled per view in the same way) by the definition of nef_loss_seg_args
    (include/nefnet_hip.h).  No renormalisation: all ones is the flat mean.  The tuple keeps its length; the Standin terms, the rest_out /
    rest_view term and the SSIM term are untouched.  []: `rois` is not looked at for it.
    cfg.SOLVER.slope_factor > 0: the tuple gains the slope term slope_factor * (mean over rows of the row's mean |d| or d^2, d the
    difference of the first differences of predict (+ noise) and target; nef_loss_slope_args, include/nefnet_hip.h) as its LAST element,
    behind the SSIM term when both are on, and `loss` includes it.  With cfg.SOLVER.slope_crop the rows end at rois[i, -1, 0] (rois is
    required then; tiled per view in the same way).  The term does not depend on SOLVER.seg_weights, loss_using or loss_factor.  Factor 0:
    nothing changes.
    cfg.SOLVER.corr_factor > 0: the tuple gains the correlation term corr_factor * (mean over rows of 1 - r_i, r_i the Pearson correlation
    coefficient of predict (+ noise) and target with cfg.SOLVER.corr_eps; nef_loss_corr_args, include/nefnet_hip.h) as its LAST element,
    behind the SSIM and slope terms, and `loss` includes it.  With cfg.SOLVER.corr_crop the rows end at rois[i, -1, 0] (rois is required
    then; tiled per view in the same way).  Independent of SOLVER.seg_weights, loss_using and loss_factor.  Factor 0: nothing changes."""
    ssim_factor, ssim_rois = ssim_settings(cfg, rois)
    slope_factor, slope_l2, slope_rois = slope_settings(cfg, rois)
    if slope_factor > 0:
        check_slope_rows(predict.numel() // predict.shape[-1])
        if slope_rois is not None:
            slope_rois = _rows_rois(slope_rois, predict)
    corr_factor, corr_eps, corr_rois = corr_settings(cfg, rois)
    if corr_factor > 0:
        check_corr_rows(predict.numel() // predict.shape[-1])
        if corr_rois is not None:
            corr_rois = _rows_rois(corr_rois, predict)
    seg_weights = seg_settings(cfg)
    seg_rois = None
    if seg_weights is not None:
        if rois is None:
            raise ValueError("SOLVER.seg_weights is set: the loss needs this batch's rois (losswrapper(..., rois=)); "
                             "set SOLVER.seg_weights [] to switch the weights off")
        check_seg_rows(predict.numel() // predict.shape[-1])
        seg_rois = _rows_rois(rois, predict)
    if ssim_factor > 0 and predict.dim() == 4:
        check_view_rows(predict.shape[0], predict.shape[1])
        if ssim_rois is not None and ssim_rois.shape[0] == predict.shape[1]:
            ssim_rois = ssim_rois.repeat(predict.shape[0], 1, 1)
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
    if ssim_rois is not None:
        ssim_rois = ssim_rois.detach().to(torch.int64).contiguous()
    L4 = _LossFn.apply(predict, predict_shuffle_p, predict_shuffle_l, target, factors, reg_l2, use_mask, noise, ssim_factor, ssim_rois,
                       seg_weights, seg_rois, slope_factor, slope_l2, slope_rois, corr_factor, corr_eps, corr_rois)
    result = (L4[0], L4[1].detach(), L4[2].detach(), L4[3].detach())
    tail = (L4[4].detach(),) if ssim_factor > 0 else ()
    if slope_factor > 0:
        tail += (L4[4 + len(tail)].detach(),)
    if corr_factor > 0:
        tail += (L4[-1].detach(),)
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
        return _LossFn.apply(input, input, input, target, (0.0, 0.0, 1.0), True, 4, None, 0.0, None, None, None, 0.0, False, None, 0.0, CORR_EPS,
                             None)[0]
