"""The wave-segment weights of the reconstruction term (cfg.SOLVER.seg_weights) and the per-segment squared error of the test phase
(cfg.SOLVER.seg_eval) restated in numpy / torch fp64 for the tests.  The segment of position t of row i (include/nefnet_hip.h,
nef_loss_seg_args): end_i = clamp(rois[i, 6, 0], 0, L); t >= end_i is segment 6 (pad); otherwise the number of k in 1..5 with
rois[i, k, 0] <= t."""
import numpy as np
import torch

N_SEG = 7


def seg_index(rois, L):
    """int64 [B, L]: the segment 0..6 of every position, from int rois [B, 7, 2] (numpy or torch)."""
    r = np.asarray(rois.cpu() if torch.is_tensor(rois) else rois).astype(np.int64)
    assert r.ndim == 3 and r.shape[1:] == (N_SEG, 2), r.shape
    t = np.arange(L, dtype=np.int64)[None, :]
    end = np.clip(r[:, 6, 0], 0, L)[:, None]
    idx = np.zeros((r.shape[0], L), dtype=np.int64)
    for k in range(1, 6):
        idx += (r[:, k, 0][:, None] <= t).astype(np.int64)
    return np.where(t >= end, 6, idx)


def weight_map(rois, L, weights, dtype=np.float32):
    """[B, L]: the weight of every position, weights = [P, PR, QRS, ST, T, TP, pad] rounded to `dtype` as the kernels hold them."""
    w = np.asarray(weights, dtype=dtype)
    assert w.shape == (N_SEG,)
    return w[seg_index(rois, L)]


def seg_term(pred, target, rois, weights, f2=1.0, reg_l2=False, noise=None):
    """f2 * (1/n) * sum w[seg(i, t)] * e(i, t) as a 0-dim fp64 tensor (differentiable in pred); n = every element of pred.  The element
    e = |d| or d * d, d = (pred (+ noise)) - target, is formed in the dtype of the inputs -- fp32 inputs give the fp32 element the loss
    kernels form, fp64 inputs the exact term -- and is weighed and summed in fp64.  The weights are the fp32 values the kernel holds.
    pred: [B, L], [B, 1, L] or [Q, B, 1, L] with rois [rows, 7, 2]."""
    L = pred.shape[-1]
    x = pred.reshape(-1, L)
    if noise is not None:
        x = x + noise.reshape(-1, L)
    d = x - target.reshape(-1, L)
    e = (d * d if reg_l2 else d.abs()).double()
    W = torch.from_numpy(weight_map(rois, L, weights).astype(np.float64))
    assert W.shape == e.shape, (W.shape, e.shape)
    return float(f2) * (W * e).sum() / e.numel()


def seg_sums(pred, gt, rois):
    """(se fp64 [B, Q, 7], cnt int64 [B, Q, 7]) of pred, gt [B, Q, L]: the sum of ((double)x - (double)y)^2 over the positions of segment
    k of sample b, and their number."""
    x = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred).astype(np.float64)
    y = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt).astype(np.float64)
    B, Q, L = x.shape
    idx = seg_index(rois, L)
    d2 = (x - y) ** 2
    se = np.zeros((B, Q, N_SEG), dtype=np.float64)
    cnt = np.zeros((B, Q, N_SEG), dtype=np.int64)
    for k in range(N_SEG):
        m = idx == k                                    # [B, L]
        se[:, :, k] = (d2 * m[:, None, :]).sum(-1)
        cnt[:, :, k] = m.sum(-1)[:, None]
    return se, cnt


def seg_psnr(se, cnt):
    """PSNR of one (row, view, segment): 100 for se == 0, else 20 log10(1 / sqrt(se / cnt)); cnt > 0."""
    if se == 0:
        return 100.0
    return float(20.0 * np.log10(1.0 / np.sqrt(se / cnt)))
