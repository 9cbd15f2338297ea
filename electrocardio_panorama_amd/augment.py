"""DATA.aug_*: corruption of the input leads of a train step, on the device (host side: the keys, the seeds, the log line; no
counterpart in the reference, whose only augmentation is the angle jitter of its dataset, codes/dataset/tianchi.py).

The model synthesises clean views from few real electrodes, whose signals carry measurement noise, baseline wander, mains hum and the
odd detached electrode: a run trains on corrupted INPUTS against the clean targets.  `from_cfg` turns the keys into an `Augment` (None
when nothing is on); ops.augment applies it (nef_augment, include/nefnet_hip.h, where the corruption is defined draw by draw), in front of
the stem in Model_nefnet.forward and as the first launch of the graphed step.

Seeds.  The corruption draws from the counter RNG of the dropout epilogues under a seed word of its own: the step's seed -- the one
Model_nefnet._drop_cfg / GraphedTrainStep._stage form from (initial seed, call counter, epoch, rank) -- plus SITE * 0x85EBCA6B + 1 with
SITE one behind the last entry of engine.DROPOUT_SITES.  The step's seed is ADDED (`train_seed`), on both paths: the replayed step holds
it in its `seed_dev` word, which the launch adds to the host word `site_word()` when it runs, so an eager and a replayed step at one
step seed draw the same corruption.  (DropCfg.args multiplies the eager step's seed by 0x9E3779B1, which a device word added at run time
cannot reproduce: the dropout masks of the two paths are equally distributed, not equal.)  The robustness read-out (`eval_seed`) uses
the next site and a bit no train seed has."""
from typing import NamedTuple, Optional

_M64 = 0xFFFFFFFFFFFFFFFF
_SITE_MUL = 0x85EBCA6B        # engine.DropCfg.args
_EVAL_BIT = 1 << 48           # a step seed is below 2^47 and the site words below 2^36: no train seed has this bit


class Augment(NamedTuple):
    noise_std: float
    wander_amp: float
    wander_lo: float
    wander_hi: float
    hum_amp: float
    hum_hz: float
    lead_drop: float
    sample_rate: float
    crop: bool
    eval: bool

    def active(self):
        """The keys that are on, as the log line names them."""
        out = []
        if self.noise_std > 0:
            out.append(f"aug_noise_std {self.noise_std:g}")
        if self.wander_amp > 0:
            out.append(f"aug_wander_amp {self.wander_amp:g} at {self.wander_lo:g}-{self.wander_hi:g} Hz")
        if self.hum_amp > 0:
            out.append(f"aug_hum_amp {self.hum_amp:g} at {self.hum_hz:g} Hz")
        if self.lead_drop > 0:
            out.append(f"aug_lead_drop {self.lead_drop:g}")
        return out

    def describe(self):
        return "input-lead augmentation on the device: {} (sample_rate {:g} Hz, aug_crop {}, aug_eval {})".format(
            ", ".join(self.active()), self.sample_rate, self.crop, self.eval)


def _number(cfg, key, default):
    v = cfg.DATA.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError(f"Invalid DATA.{key}: {v!r} (a number)")
    return float(v)


def lead_mask_on(cfg):
    """MODEL.lead_mask: the train step (and the aug_eval read-out) tell the head which leads DATA.aug_lead_drop zeroed, so the lead mean
    and the Standin picks run over the present leads only (include/nefnet_hip.h, nef_lead_mask_mix_fwd_args).  Configs written before
    the key existed have none: off."""
    model = cfg.get("MODEL") or {}
    v = model.get("lead_mask", False)
    if not isinstance(v, bool):
        raise ValueError(f"Invalid MODEL.lead_mask: {v!r} (True or False)")
    return v


def from_cfg(cfg) -> Optional[Augment]:
    """The run's Augment, or None when aug_noise_std, aug_wander_amp, aug_hum_amp and aug_lead_drop are all 0 (configs written before the
    keys existed have none).  Raises ValueError, naming the key: a negative value, aug_lead_drop >= 1, aug_wander_hz with lo > hi,
    sample_rate <= 0, a wander or hum frequency at or above sample_rate / 2, MODEL.lead_mask on with aug_lead_drop 0 (nothing to mask)."""
    noise, wander, hum, drop = (_number(cfg, k, 0.0) for k in ("aug_noise_std", "aug_wander_amp", "aug_hum_amp", "aug_lead_drop"))
    hz = cfg.DATA.get("aug_wander_hz", [0.05, 0.7])
    if not isinstance(hz, (list, tuple)) or len(hz) != 2 or any(isinstance(f, bool) or not isinstance(f, (int, float)) or f != f for f in hz):
        raise ValueError(f"Invalid DATA.aug_wander_hz: {hz!r} ([lo, hi] in Hz)")
    lo, hi = float(hz[0]), float(hz[1])
    hum_hz, fs = _number(cfg, "aug_hum_hz", 50.0), _number(cfg, "sample_rate", 500.0)
    for key, v in (("aug_noise_std", noise), ("aug_wander_amp", wander), ("aug_hum_amp", hum), ("aug_lead_drop", drop),
                   ("aug_wander_hz", lo), ("aug_wander_hz", hi), ("aug_hum_hz", hum_hz)):
        if v < 0 or v == float("inf"):
            raise ValueError(f"Invalid DATA.{key}: {v!r} (negative or not finite)")
    if drop >= 1:
        raise ValueError(f"Invalid DATA.aug_lead_drop: {drop!r} (a probability below 1: every sample keeps a lead)")
    if lo > hi:
        raise ValueError(f"Invalid DATA.aug_wander_hz: {hz!r} (lo > hi)")
    if not 0 < fs < float("inf"):
        raise ValueError(f"Invalid DATA.sample_rate: {fs!r} (Hz, > 0)")
    if hi >= fs / 2:
        raise ValueError(f"Invalid DATA.aug_wander_hz: {hz!r} reaches sample_rate / 2 = {fs / 2:g} Hz")
    if hum_hz >= fs / 2:
        raise ValueError(f"Invalid DATA.aug_hum_hz: {hum_hz!r} reaches sample_rate / 2 = {fs / 2:g} Hz")
    if lead_mask_on(cfg) and drop == 0:
        raise ValueError("MODEL.lead_mask is on with DATA.aug_lead_drop 0: no lead is ever dropped, there is nothing to mask")
    if noise == 0 and wander == 0 and hum == 0 and drop == 0:
        return None
    return Augment(noise, wander, lo, hi, hum, hum_hz, drop, fs, bool(cfg.DATA.get("aug_crop", True)), bool(cfg.DATA.get("aug_eval", False)))


def _site():
    from .engine import DROPOUT_SITES
    return len(DROPOUT_SITES)


def site_word(read_out=False):
    """The host word of a launch whose step seed arrives through `seed_dev` (the replayed step); `read_out`: the robustness read-out's."""
    return ((_site() + 1) * _SITE_MUL + 1 + _EVAL_BIT) if read_out else (_site() * _SITE_MUL + 1)


def train_seed(step_seed):
    """ops.augment's `seed` of the eager train step whose dropout seed (DropCfg.seed) is `step_seed`."""
    return (int(step_seed) + site_word()) & _M64


def eval_seed(cfg_seed, index, rank=0):
    """ops.augment's `seed` of test batch `index` of the robustness read-out (DATA.aug_eval): a function of (cfg.seed, batch index, rank)
    alone -- every epoch and every resumed run judges the same corrupted test set -- under a site of its own and a bit no train seed
    has."""
    step = (int(cfg_seed) * 0x1000003 + int(index) + int(rank) * 0x9E3779B1) & 0x7FFFFFFFFFFF
    return (step + site_word(read_out=True)) & _M64
