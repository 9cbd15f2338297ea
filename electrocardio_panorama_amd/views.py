"""SOLVER.train_views: which target views a multi-view train step supervises (host side; no counterpart in the reference, whose
train step takes the one `target_view` its dataset drew, codes/dataset/tianchi.py:186-190).

The batch carries every lead that is not an input as `rest_view` / `rest_theta`, supervised ones first (dataset/tianchi.py).  A step
with Q = SOLVER.train_views >= 2 takes Q of those S supervised rest views -- ONE draw per step, shared by the batch and identical on
every rank -- and hands them to the model as `query_theta` [Q, B, 2] with targets [Q, B, 1, L]."""
import random


def train_views(cfg):
    """Q = SOLVER.train_views (1 = off; configs written before the key existed have none).  Q < 1, and DATA.noise with Q >= 2 -- the
    batch carries noise for the target lead only -- raise ValueError."""
    Q = cfg.SOLVER.get('train_views', 1)
    if isinstance(Q, bool) or int(Q) != Q or int(Q) < 1:
        raise ValueError(f"Invalid SOLVER.train_views: {Q!r} (an integer >= 1; 1 = one target view per step)")
    Q = int(Q)
    if Q >= 2 and cfg.DATA.get('noise', False):
        raise ValueError("DATA.noise with SOLVER.train_views >= 2: the batch carries noise for the target lead only (meta['noise']); "
                         "switch one of them off (DATA.device_noise draws a row per view)")
    return Q


def supervised_views(cfg, n_rest):
    """S: how many of the batch's `n_rest` rest views are supervised leads (they come first; the unsupervised leads of the configured
    lead scheme come last).  DATA.synthetic: all of them.  Python's global `random` stream is left as it was (the lead plan of the
    3-lead schemes draws from it)."""
    if cfg.DATA.get('synthetic', False):
        return int(n_rest)
    from .dataset.tianchi import _lead_plan
    state = random.getstate()
    try:
        unsup = _lead_plan(cfg.DATA.lead_num, cfg.DATA.super_mode, cfg.DATA.train_data_mode)[2]
    finally:
        random.setstate(state)
    return int(n_rest) - len(unsup)


def planned_views(cfg):
    """(rest views per item, S of them supervised) of the configured lead scheme, as dataset/tianchi.py builds `rest_view`; the global
    `random` stream is left as it was."""
    from .dataset.tianchi import _lead_plan
    state = random.getstate()
    try:
        sel, sup, unsup, keep = _lead_plan(cfg.DATA.lead_num, cfg.DATA.super_mode, cfg.DATA.train_data_mode)
    finally:
        random.setstate(state)
    S = len(sup) if keep else len([x for x in sup if x not in sel])
    return S + len(unsup), S


def check_views(Q, S):
    if Q > S:
        raise ValueError(f"SOLVER.train_views = {Q} but the batch carries only {S} supervised rest views")


def draw_views(seed, epoch, index, Q, S):
    """The Q rest-view indices (sorted, no repeats, all < S) of train batch `index` of `epoch`: a function of (seed, epoch, index)
    alone -- a private random.Random, so a resumed run continues bit for bit, every rank draws the same views and Python's global
    `random` stream is consumed exactly as without the key.  Q == S: all views in order, no draw."""
    check_views(Q, S)
    if Q == S:
        return list(range(S))
    rng = random.Random((int(seed) * 1000003 + int(epoch)) * 1000003 + int(index))
    return sorted(rng.sample(range(S), Q))


def select_views(rest_view, rest_theta, idx):
    """(targets [Q, B, 1, L] float32, query_theta [Q, B, 2] float32), view-major and contiguous, of rest views `idx`."""
    import torch
    # (slices stacked on the device: an index tensor would be a blocking host-to-device copy in every step)
    tv = torch.stack([rest_view[:, i] for i in idx], 0).to(torch.float32).unsqueeze(2).contiguous()
    th = torch.stack([rest_theta[:, i] for i in idx], 0).to(torch.float32).contiguous()
    return tv, th
