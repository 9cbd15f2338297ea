"""DATA.device_noise: the train step's label-noise row, drawn on the device (host side: the key, its one rejection, the seeds; no
counterpart in the reference, whose DATA.noise row is a host draw of its dataset, codes/dataset/tianchi.py, added in front of the loss,
codes/solver/solver.py:185-186).

DATA.noise's row is made in the loader workers from the UNWARPED beat of the TARGET lead, so every feature that builds, moves or multiplies
the target on the device rejects it (dataset/resident.py, warp.py, views.py).  With DATA.device_noise the train step makes the row
itself -- ops.noise_row (nef_noise_row, include/nefnet_hip.h, where the row is defined) on the step's final target rows and rois, behind
the warp and the view selection -- and hands it to the loss where DATA.noise's row goes: the `noise=` argument of ops.loss_fwd /
ops.loss_bwd and of every tail term.  meta['noise'] is not read; the test phase adds no noise, as in the reference.

Seeds.  The row draws from the counter RNG of the dropout epilogues under a seed word of its own, built as augment.py builds the
corruption's: the step's seed (Model_nefnet._drop_cfg / GraphedTrainStep._stage: initial seed, call counter, epoch, rank) plus the site
word four behind the last entry of engine.DROPOUT_SITES (nef_augment holds the first two behind it, nef_warp the next two).  The eager
step adds the two on the host (`train_seed`), the replayed step holds its seed in the `seed_dev` word the launch adds to `site_word()`
when it runs: one row on both paths, another one on every step and every rank, and -- the step counters restart with every train epoch
when the key is on, as with DATA.aug_* -- the same rows in a resumed epoch."""
from . import augment


def on(cfg):
    """DATA.device_noise (configs written before the key existed have none: off).  Together with DATA.noise: ValueError -- two sources for
    one addend."""
    v = cfg.DATA.get("device_noise", False)
    if not isinstance(v, bool):
        raise ValueError(f"Invalid DATA.device_noise: {v!r} (True or False)")
    if v and cfg.DATA.get("noise", False):
        raise ValueError("DATA.device_noise with DATA.noise: two sources for the one noise addend of the loss (the loader's row and the "
                         "step's own); switch one of them off")
    return v


def site_word():
    """The host word of a launch whose step seed arrives through `seed_dev` (the replayed step)."""
    return (augment._site() + 4) * augment._SITE_MUL + 1


def train_seed(step_seed):
    """ops.noise_row's `seed` of the eager train step whose dropout seed (DropCfg.seed) is `step_seed`."""
    return (int(step_seed) + site_word()) & augment._M64


def rows(target, rois):
    """(target rows, rois per row) as ops.noise_row takes them: float32 contiguous targets, and int64 rois tiled once per view for a
    multi-view target [Q, B, 1, L] ([Q * B, 7, 2] is taken as it is)."""
    import torch
    target = target.detach().to(torch.float32).contiguous()
    rois = rois.detach().to(torch.int64)
    if target.dim() == 4 and rois.shape[0] == target.shape[1]:
        rois = rois.repeat(target.shape[0], 1, 1)
    return target, rois.contiguous()
