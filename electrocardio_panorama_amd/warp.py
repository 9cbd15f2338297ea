"""DATA.aug_warp / DATA.aug_roi_jitter: time warp of a whole train batch with jittered marks, on the device (host side: the keys, the
seeds, the log line; no counterpart in the reference, whose only augmentation is the angle jitter of its dataset).

DATA.aug_* (augment.py) corrupts the input leads additively and never changes a beat's timing; this stretches or shrinks each of the six
wave segments of every beat by a drawn factor -- inputs, target, rest views and the marks in `rois` together -- and then moves each
interior mark by a drawn integer, the signal staying where it is: the first gives a run timing diversity, the second prepares it for marks
that are a few samples off.  (DATA.noise's host row belongs to the unwarped beat and is rejected; DATA.device_noise draws the row from the
warped target and its jittered marks, device_noise.py.)  `from_cfg` turns the keys into a `Warp` (None when nothing is on); ops.warp applies it (nef_warp,
include/nefnet_hip.h, where every step is defined), in Solver.run_one_epoch right behind the batch's arrival on the device: one launch
into fresh tensors, outside the replayed graph, so every later stage of the step receives a batch that is already consistent.

Seeds.  A launch's seed is a function of (cfg.seed, epoch, batch index, rank) alone (`train_seed`; `eval_seed` of (cfg.seed, batch index,
rank)): no counter, no global random state, so a resumed epoch repeats the uninterrupted one.  They are built as augment.eval_seed is, under
the site words two and three behind the last entry of engine.DROPOUT_SITES (nef_augment holds the two in between), the read-out's with
augment._EVAL_BIT: no draw coincides with a dropout mask's or with nef_augment's."""
from typing import NamedTuple, Optional, Tuple

from . import augment

MAX_AMP = 0.9        # NEF_WARP_MAX_AMP (include/nefnet_hip.h)
MAX_JITTER = 64      # NEF_WARP_MAX_JITTER
SEG_NAMES = ("P", "PR", "QRS", "ST", "T", "TP")
_EPOCH_MUL = 0x3D4D51CB


class Warp(NamedTuple):
    amp: Tuple[float, float, float, float, float, float]
    jitter: int
    eval: bool

    def describe(self):
        return "time warp on the device: aug_warp {} ({}), aug_roi_jitter {}, aug_warp_eval {}".format(
            ", ".join("{} {:g}".format(n, a) for n, a in zip(SEG_NAMES, self.amp)), "a segment's length times 1 +- its amplitude",
            self.jitter, self.eval)


def from_cfg(cfg) -> Optional[Warp]:
    """The run's Warp, or None when every amplitude is 0 (or DATA.aug_warp is empty) and DATA.aug_roi_jitter is 0 (configs written before
    the keys existed have none).  Raises ValueError, naming the key: aug_warp not empty and not six numbers, a bool, a NaN or a value
    outside [0, 0.9] in it; aug_roi_jitter not an integer in 0..64; DATA.noise with a warp or a jitter on."""
    amp = cfg.DATA.get("aug_warp", [])
    if amp is None:
        amp = []
    if not isinstance(amp, (list, tuple)) or len(amp) not in (0, 6):
        raise ValueError(f"Invalid DATA.aug_warp: {amp!r} (empty, or six amplitudes [P, PR, QRS, ST, T, TP])")
    for a in amp:
        if isinstance(a, bool) or not isinstance(a, (int, float)) or a != a or not 0 <= a <= MAX_AMP:
            raise ValueError(f"Invalid DATA.aug_warp: {amp!r} (every amplitude a number in [0, {MAX_AMP}])")
    J = cfg.DATA.get("aug_roi_jitter", 0)
    if isinstance(J, bool) or not isinstance(J, int) or not 0 <= J <= MAX_JITTER:
        raise ValueError(f"Invalid DATA.aug_roi_jitter: {J!r} (an integer in 0..{MAX_JITTER})")
    amp = tuple(float(a) for a in amp) if amp else (0.0,) * 6
    if not any(amp) and J == 0:
        return None
    if cfg.DATA.get("noise", False):
        raise ValueError("DATA.noise with DATA.aug_warp / DATA.aug_roi_jitter on: the noise row is padded to the unwarped beat "
                         "(DATA.device_noise draws the row from the warped target)")
    return Warp(amp, int(J), bool(cfg.DATA.get("aug_warp_eval", False)))


def _site_word(read_out=False):
    site = augment._site() + (3 if read_out else 2)
    return site * augment._SITE_MUL + 1 + (augment._EVAL_BIT if read_out else 0)


def train_seed(cfg_seed, epoch, index, rank=0):
    """ops.warp's `seed` of train batch `index` of epoch `epoch` on rank `rank`."""
    step = (int(cfg_seed) * 0x1000003 + int(epoch) * _EPOCH_MUL + int(index) + int(rank) * 0x9E3779B1) & 0x7FFFFFFFFFFF
    return (step + _site_word()) & augment._M64


def eval_seed(cfg_seed, index, rank=0):
    """ops.warp's `seed` of test batch `index` of the read-out on warped beats (DATA.aug_warp_eval): every epoch and every resumed run
    judges the same warped test set, under a site of its own and a bit no train seed has."""
    step = (int(cfg_seed) * 0x1000003 + int(index) + int(rank) * 0x9E3779B1) & 0x7FFFFFFFFFFF
    return (step + _site_word(read_out=True)) & augment._M64
