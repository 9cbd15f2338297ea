"""Training driver with the surface of reference codes/solver/solver.py:16-245 (`Solver.train`, `Solver.val`,
`Solver.run_one_epoch`, `write_tensorboardx`).

Scope.  The train-phase body of `run_one_epoch` -- H2D of the meta dict, model
call, losswrapper, backward, optimiser step -- runs on the device with NO per-iteration host synchronisation: the
reference issues ~10 blocking D2H copies per step (solver.py:179,189,236-240); here the loss scalars, the predicted
views and the metric tables are copied to pinned host memory asynchronously and read once at the end of the epoch,
so the returned lists are the reference's while the launch queue never drains.  The test phase reproduces the
reference's bookkeeping (solver.py:190-230): `loss_unsperv` on the last four rest views, PSNR / SSIM split into
generated (`gen`, the last `gen_num` rest views) and regressed (`reg`) leads plus per-lead numbers -- computed on the
device by `nef_view_metrics`, one launch per batch.

Data parallelism replaces `nn.DataParallel` (solver.py:32-34) with one process per GPU (`parallel.py`): the loaders
hand every rank its shard, FusedSGD all-reduces the flat gradient, rank 0 owns the BatchNorm running statistics,
the scalar log and the checkpoints.

`SOLVER.train_views = Q >= 2` (no counterpart in the reference): a train step supervises Q of the batch's supervised rest views on one
encoder pass -- the targets are drawn per step by `views.draw_views(seed, epoch, batch index, Q, S)` and handed to the model as
`query_theta` [Q, B, 2] with `[Q, B, 1, L]` targets, eagerly or through the graphed step; `target_view` / `target_theta` are not used.

`DATA.aug_*` (no counterpart in the reference; augment.py): the train step corrupts its INPUT leads on the device -- inside the model's
train-phase forward or as the first launch of the graphed step -- against the clean targets; with a corruption on, the step counters
restart with every train epoch, so the step's seed is a function of (seed, epoch, batch index, rank) and a resumed epoch draws what the
uninterrupted one drew.  `DATA.aug_eval`: `train` and `val` run the test phase a second time on one fixed corrupted test set and report
psnr_gen_aug / psnr_reg_aug / ssim_gen_aug / ssim_reg_aug beside the clean numbers, which decide best_valid as before.

`DATA.aug_warp` / `DATA.aug_roi_jitter` (no counterpart in the reference; warp.py): the train phase warps every batch in time on the device
right behind its arrival there -- inputs, target, rest views and rois in one launch (ops.warp) under warp.train_seed(seed, epoch, batch
index, rank) -- so the eager step, the replayed step and everything inside them receive a batch that is already consistent.
`DATA.aug_warp_eval`: `train` and `val` run the test phase once more on one fixed warped and jittered test set and report psnr_gen_warp /
psnr_reg_warp / ssim_gen_warp / ssim_reg_warp beside the unwarped numbers, which decide best_valid as before.

`DATA.device_noise` (no counterpart in the reference; device_noise.py): the train step draws DATA.noise's addend itself on the device --
ops.noise_row on the step's final target rows and rois, behind the warp and the view selection, eagerly right behind the model call or as
a captured launch of the graphed step -- and hands it to the loss as `noise=`; meta['noise'] is not read and the test phase adds no
noise.  The step counters restart with every train epoch then, as with DATA.aug_*.

`SOLVER.seg_weights` / `SOLVER.seg_eval` (no counterpart in the reference): the loss takes the batch's rois and weighs the reconstruction
term by wave segment; the test phase reports the PSNR of each of the six wave segments (`nef_view_seg_metrics`, one more launch per
batch) as psnr_gen_seg_* / psnr_reg_seg_*, in `Solver.last_seg_psnr`.
`SOLVER.slope_factor` / `SOLVER.slope_eval` (no counterpart in the reference): the loss gains the first-difference term, logged as
train_loss_slope / test_loss_slope; the test phase reports the PSNR of the first differences (`nef_view_slope_metrics`, one more launch per
batch) as psnr_slope_gen / psnr_slope_reg, in `Solver.last_slope_psnr`.
`SOLVER.corr_factor` / `SOLVER.corr_eval` (no counterpart in the reference): the loss gains 1 - the Pearson correlation coefficient, logged
as train_loss_corr / test_loss_corr; the test phase reports the mean coefficient (`nef_view_corr_metrics`, one more launch per batch) as
corr_gen / corr_reg, in `Solver.last_corr`.
`SOLVER.locate_eval` (no counterpart in the reference; locate.py): `Solver.val` also locates every rest view of every test batch from the
batch's input leads (`Solver.locate`: Model_nefnet.locate with observed = rest_view, truth = rest_theta) and prints the angular error
as locate_err1_* / locate_err2_* / locate_hit_* with the gen / reg view split, in `Solver.last_locate`."""
import contextlib
import json
import os
import random

import numpy as np
import torch
from .. import _env
import torch.distributed as dist

from .. import augment, engine, ops, parallel, views
from .. import warp as _warp
from .. import locate as _locate
from .. import device_noise as _device_noise
from ..network import build_model, build_loss
from ..utils import CheckPointer
from .optim_scheduler import get_optimizer, get_lr_scheduler


class JsonlScalarWriter:
    """`add_scalar(tag, value, global_step)` sink used when neither tensorboardX nor torch.utils.tensorboard is
    installed (solver.py:8,24): one JSON object per scalar in `<logdir>/scalars.jsonl`."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, 'scalars.jsonl')

    def add_scalar(self, tag, scalar_value, global_step=None):
        with open(self.path, 'a') as f:
            f.write(json.dumps({'tag': tag, 'value': float(scalar_value), 'step': global_step}) + '\n')

    def close(self):
        pass


def make_summary_writer(logdir):
    try:
        import tensorboardX
        return tensorboardX.SummaryWriter(logdir=logdir)
    except ImportError:
        pass
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(log_dir=logdir)
    except ImportError:
        return JsonlScalarWriter(logdir)


class _HostSink:
    """Device tensors queued for the host without a per-iteration synchronisation: each is copied into a pinned staging
    buffer on the current stream; the staging buffers form a bounded ring (RING entries per sink), and a buffer is drained
    into pageable numpy memory -- after waiting for ITS copy event only -- when the ring comes round to it again.  The
    pinned footprint is therefore RING tensors per sink, not an epoch's worth, and after the first RING adds no
    hipHostMalloc happens (buffers are reused when the shape matches)."""
    RING = 4

    def __init__(self):
        self.done = []           # pageable numpy arrays, in order
        self.ring = []           # [pinned buffer, event, filled?]
        self.pos = 0

    def _drain(self, slot):
        if slot[2]:
            slot[1].synchronize()
            self.done.append(slot[0].numpy().copy())
            slot[2] = False

    def add(self, t):
        t = t.detach()
        if len(self.ring) < self.RING:
            self.ring.append([torch.empty(t.shape, dtype=t.dtype, pin_memory=True), torch.cuda.Event(), False])
            slot = self.ring[-1]
        else:
            slot = self.ring[self.pos]
            self._drain(slot)
            if slot[0].shape != t.shape or slot[0].dtype != t.dtype:       # e.g. the final partial batch
                slot[0] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        self.pos = (self.pos + 1) % self.RING
        slot[0].copy_(t, non_blocking=True)
        slot[1].record()
        slot[2] = True

    def arrays(self):
        n = len(self.ring)
        start = self.pos if n == self.RING else 0
        for i in range(n):           # oldest first
            self._drain(self.ring[(start + i) % n])
        return self.done

    def rows(self):
        return [x for a in self.arrays() for x in a]


def seg_psnr(se, cnt):
    """PSNR per wave segment from nef_view_seg_metrics' tables of one batch: se, cnt [B, Q', 7] -> the mean over the (row, view) pairs
    that own positions of the segment of 100 (se == 0) or 20 log10(1 / sqrt(se / cnt)), for the six segments in front of the padding.  NaN
    where no pair has a position."""
    out = []
    for k in range(6):
        s, c = se[..., k].reshape(-1), cnt[..., k].reshape(-1)
        has = c > 0
        s, c = s[has], c[has].astype(np.float64)
        if s.size == 0:
            out.append(float('nan'))
            continue
        rmse = np.sqrt(s / c)
        out.append(float(np.mean(np.where(rmse == 0.0, 100.0, 20.0 * np.log10(1.0 / np.where(rmse == 0.0, 1.0, rmse))))))
    return out


def slope_psnr(se, cnt):
    """PSNR of the first differences from nef_view_slope_metrics' tables of one batch: se, cnt [B, Q'] -> the mean over the (row, view)
    pairs that have a difference of 100 (se == 0) or 20 log10(1 / sqrt(se / cnt)).  NaN where no pair has one."""
    s, c = np.asarray(se, dtype=np.float64).reshape(-1), np.asarray(cnt).reshape(-1)
    has = c > 0
    s, c = s[has], c[has].astype(np.float64)
    if s.size == 0:
        return float('nan')
    rmse = np.sqrt(s / c)
    return float(np.mean(np.where(rmse == 0.0, 100.0, 20.0 * np.log10(1.0 / np.where(rmse == 0.0, 1.0, rmse)))))


def corr_pairs(mom, cnt, eps):
    """The correlation coefficients from nef_view_corr_metrics' tables of one batch: mom [B, Q', 3] = (vx, vy, c), cnt [B, Q'] -> the 1-D
    array of r = (c + eps) / sqrt((vx + eps) (vy + eps)) of the (row, view) pairs with at least two samples."""
    m, n = np.asarray(mom, dtype=np.float64).reshape(-1, 3), np.asarray(cnt).reshape(-1)
    m = m[n >= 2]
    return (m[:, 2] + eps) / np.sqrt((m[:, 0] + eps) * (m[:, 1] + eps))


def _is_main():
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


class Solver:
    def __init__(self, cfg, use_tensorboardx=True, collect_views=True):
        self.cfg = cfg
        self.output_dir = os.path.join(cfg.output_dir, cfg.desc)
        self.desc = cfg.desc
        self.collect_views = collect_views       # False: skip the per-view host lists (benchmarks)
        # SOLVER.train_views = Q >= 2: a train step supervises Q of the batch's supervised rest views on one encoder pass (views.py);
        # 1: the reference's step on target_view / target_theta.  Invalid values and DATA.noise with Q >= 2 are rejected here
        self.train_views = views.train_views(cfg)
        # DATA.device_noise: the train step draws its own noise row on the device (device_noise.py); with DATA.noise it is rejected here
        self.device_noise = _device_noise.on(cfg)
        self.model = build_model(cfg).float()
        # DATA.aug_*: the train step corrupts its input leads on the device (augment.py); invalid keys are rejected here.  None = off
        self.augment = self.model.augment = augment.from_cfg(cfg)
        # MODEL.lead_mask (from_cfg has rejected it without DATA.aug_lead_drop): the train step's head reads the mask of the dropped leads
        self.lead_mask = self.model.lead_mask_from_aug = augment.lead_mask_on(cfg)
        # DATA.aug_warp / aug_roi_jitter: the train phase warps every batch in time on the device (warp.py); invalid keys are rejected
        # here.  None = off
        self.warp = _warp.from_cfg(cfg)
        self.loss = build_loss(cfg)
        # SOLVER.seg_eval: the test phase also fills last_seg_psnr = {'gen': [6 numbers], 'reg': [6 numbers]} (P, PR, QRS, ST, T, TP)
        self.seg_eval = bool(cfg.SOLVER.get('seg_eval', False))
        self.last_seg_psnr = None
        # SOLVER.slope_eval: the test phase also fills last_slope_psnr = {'gen': number, 'reg': number}
        self.slope_eval = bool(cfg.SOLVER.get('slope_eval', False))
        self.last_slope_psnr = None
        # SOLVER.corr_eval: the test phase also fills last_corr = {'gen': number, 'reg': number}
        self.corr_eval = bool(cfg.SOLVER.get('corr_eval', False))
        self.last_corr = None
        # SOLVER.locate_eval: val() also fills last_locate = {'locate_err1_gen': ..., ...} (Solver.locate); invalid keys are rejected here
        self.locate_eval = _locate.from_cfg(cfg) is not None
        self.last_locate = None
        self._init_model_device()
        if self.desc != 'debug' and use_tensorboardx and _is_main():       # solver.py:23-26
            self.summary_writer = make_summary_writer(os.path.join(cfg.output_dir, 'tf_logs'))
        else:
            self.summary_writer = None

    def _init_model_device(self):
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device: this build has no CPU path (use the oracle for CPU runs)")
        self.device = torch.device('cuda', parallel.local_rank() if dist.is_available() and dist.is_initialized() else 0)
        self.model.to(self.device)

    def write_tensorboardx(self, scalars, names, epoch):
        for i in range(len(scalars)):
            self.summary_writer.add_scalar(names[i], scalars[i], global_step=epoch)

    def train(self, dl_train, dl_test=None):
        optimizer = get_optimizer(self.cfg, self.model.parameters())
        scheduler = get_lr_scheduler(self.cfg, optimizer)
        checkpointer = CheckPointer(self.model, optimizer, scheduler, self.output_dir)
        extra = checkpointer.load(self.cfg.MODEL.resume)
        max_epochs = self.cfg.SOLVER.epochs
        start_epoch = extra.get('epoch', 0)
        best_test_psnr_gen = extra.get('best_test_psnr_gen', 0.)
        self.model.dropout_epoch = start_epoch          # a resumed run must not replay epoch 0's dropout masks
        print('the latest best_test_psnr_gen is {:06f}'.format(best_test_psnr_gen))
        save_arguments = {}
        sched = getattr(optimizer, 'lr_schedule', None)
        if sched is not None and sched.on and sched.total_updates == 0:
            # SOLVER.total_updates 0: the run's updates, known here -- before the first step, so nothing is re-captured for it
            sched.total_updates = max_epochs * -(-len(dl_train) // getattr(optimizer, 'accum_steps', 1))
        if self.augment is not None:
            print(self.augment.describe())                # once: the DATA.aug_* keys that are on
        if self.warp is not None:
            print(self.warp.describe())                   # once: DATA.aug_warp / aug_roi_jitter / aug_warp_eval
        if self.device_noise:                             # once: DATA.device_noise
            print("noise row on the device: per target row, sigma of the quiet second half of its T-P segment (device_noise)")
        seg_w = self._seg_weights()
        if seg_w is not None:                             # once: SOLVER.seg_weights
            from ..network.loss.losses import SEG_NAMES
            print('seg_weights: ' + ', '.join('{} {:g}'.format(n, w) for n, w in zip(SEG_NAMES, seg_w)))
        for epoch in range(start_epoch, max_epochs):
            print('---------------------------------{}---{}-------------------------------------'.format(self.cfg.desc, epoch))
            if hasattr(getattr(dl_train, 'sampler', None), 'set_epoch'):
                dl_train.sampler.set_epoch(epoch)         # DistributedSampler: a new shuffle per epoch
            self.model.dropout_epoch = epoch
            train_losses = self.run_one_epoch(dl_train, phase='train', optim=optimizer, collect_views=False)[0]
            if epoch == start_epoch and hasattr(optimizer, 'decay_summary') and (
                    optimizer.no_decay or any(g.get('weight_decay', 0) for g in optimizer.param_groups)):
                # once: which live tensors SOLVER.no_decay exempts and how many elements decay (known after the first step)
                print(optimizer.decay_summary())
            scheduler.step()
            parallel.broadcast_buffers(self.model)        # rank 0's BatchNorm running statistics are the model's
            tl = np.mean(train_losses, axis=0)
            train_loss_all = float(tl[0])
            scalars, names = [train_loss_all, float(tl[1]), float(tl[2]), float(tl[3])], \
                ['train_loss_all', 'train_loss_1', 'train_loss_2', 'train_3']
            psnr_gen = psnr_reg = 0.
            msg = 'Epoch {}: train_loss: {}'.format(epoch, train_loss_all)
            if dl_test is not None:
                # SOLVER.ema_decay with ema_eval: the test phase -- and with it psnr_gen and best_valid -- sees the averaged weights
                with optimizer.ema_weights() if self._ema_eval(optimizer) else contextlib.nullcontext():
                    test_losses, _, _, _, mertics_all, _, single = self.run_one_epoch(dl_test, phase='test', collect_views=False)
                te = np.mean(test_losses, axis=0)
                psnr_gen, psnr_reg, ssim_gen, ssim_reg = (float(v) for v in np.mean(mertics_all, axis=0))
                # the reference's scalar set and names (solver.py:82-100)
                scalars = [train_loss_all, float(te[0]), float(tl[1]), float(te[1]), float(tl[2]), float(te[2]),
                           float(tl[3]), float(te[3]), float(te[4]), psnr_gen, psnr_reg, ssim_gen, ssim_reg]
                names = ['train_loss_all', 'test_loss_all', 'train_loss_1', 'test_loss_1', 'train_loss_2', 'test_loss_2',
                         'train_3', 'test_3', 'test_unsuperv', 'psnr_gen', 'psnr_reg', 'ssim_gen', 'ssim_reg']
                if len(single) != 0:
                    single = np.array(single)
                    for i in range(single.shape[1]):
                        names += ['psnr_reg_lead_{}'.format(i), 'ssim_reg_lead_{}'.format(i)]
                        scalars += [float(np.mean(single[:, i, 0])), float(np.mean(single[:, i, 1]))]
                msg += ', test_loss: {}'.format(float(te[0]))
                msg += '\npsnr_gen: {}, psnr_reg: {}, ssim_gen:{}, ssim_reg:{}'.format(psnr_gen, psnr_reg, ssim_gen, ssim_reg)
                if self.seg_eval:                 # SOLVER.seg_eval: the clean test phase's PSNR per wave segment
                    seg_names, seg_vals = self._seg_scalars()
                    scalars += seg_vals
                    names += seg_names
                    msg += '\n' + self._seg_message()
                if self.slope_eval:               # SOLVER.slope_eval: the clean test phase's PSNR of the first differences
                    scalars += [self.last_slope_psnr['gen'], self.last_slope_psnr['reg']]
                    names += ['psnr_slope_gen', 'psnr_slope_reg']
                    msg += '\n' + self._slope_message()
                if self.corr_eval:                # SOLVER.corr_eval: the clean test phase's mean correlation coefficient
                    scalars += [self.last_corr['gen'], self.last_corr['reg']]
                    names += ['corr_gen', 'corr_reg']
                    msg += '\n' + self._corr_message()
                if self.augment is not None and self.augment.eval:
                    # DATA.aug_eval: the same weights on the fixed corrupted test set; best_valid stays on the clean psnr_gen
                    with optimizer.ema_weights() if self._ema_eval(optimizer) else contextlib.nullcontext():
                        aug_metrics = self._aug_eval(dl_test)
                    scalars += list(aug_metrics)
                    names += ['psnr_gen_aug', 'psnr_reg_aug', 'ssim_gen_aug', 'ssim_reg_aug']
                    msg += '\npsnr_gen_aug: {}, psnr_reg_aug: {}, ssim_gen_aug:{}, ssim_reg_aug:{}'.format(*aug_metrics)
                if self.warp is not None and self.warp.eval:
                    # DATA.aug_warp_eval: the same weights on the fixed warped test set; best_valid stays on the unwarped psnr_gen
                    with optimizer.ema_weights() if self._ema_eval(optimizer) else contextlib.nullcontext():
                        warp_metrics = self._warp_eval(dl_test)
                    scalars += list(warp_metrics)
                    names += ['psnr_gen_warp', 'psnr_reg_warp', 'ssim_gen_warp', 'ssim_reg_warp']
                    msg += '\npsnr_gen_warp: {}, psnr_reg_warp: {}, ssim_gen_warp:{}, ssim_reg_warp:{}'.format(*warp_metrics)
            # the plan's tail terms that are on sit behind the four (train) / five (test: the rest_out term) elements of every loss row
            for k, term in enumerate(self._plan().tail):
                key = term.name
                scalars.append(float(tl[4 + k]))
                names.append('train_loss_' + key)
                msg += '\nloss_{} (factor {}): train {}'.format(key, term.factor, float(tl[4 + k]))
                if dl_test is not None:
                    scalars.append(float(te[5 + k]))
                    names.append('test_loss_' + key)
                    msg += ', test {}'.format(float(te[5 + k]))
            if self.last_grad_norms:              # SOLVER.clip_grad_norm is on
                norms = [t for t, _ in self.last_grad_norms if np.isfinite(t)]
                scalars.append(float(np.mean(norms)) if norms else float('nan'))
                names.append('train_grad_norm')
                msg += '\ngrad_norm: {} (max_norm {}): {} of {} steps clipped, {} skipped for a non-finite norm'.format(
                    scalars[-1], optimizer.max_grad_norm, self.last_clip_counts[0], len(self.last_grad_norms), self.last_clip_counts[1])
            if getattr(optimizer, 'accum_steps', 1) > 1:
                msg += '\naccum_steps {}: {} updates from {} batches'.format(optimizer.accum_steps, *self.last_updates)
            if getattr(self, 'last_lr', None) is not None:                # SOLVER.warmup_updates / lr_shape
                scalars.append(self.last_lr[1])
                names.append('train_lr')
                msg += '\nlr: {:.6e} at the first update, {:.6e} behind the last ({} updates applied so far)'.format(
                    *self.last_lr, self.last_lr_updates)
            if getattr(self, 'last_trust_stats', None) is not None:      # SOLVER.optim is lars or lamb
                msg += '\ntrust ratio: min {:.3e}, max {:.3e} over the adapted tensors; {} steps skipped for non-finite norms'.format(
                    *self.last_trust_stats)
            if self.summary_writer is not None:
                self.write_tensorboardx(scalars, names, epoch)
            print(msg)
            save_arguments['psnr_gen'] = psnr_gen
            save_arguments['psnr_reg'] = psnr_reg
            save_arguments['epoch'] = epoch
            if _is_main():
                checkpointer.save('epoch_{}'.format(epoch), **save_arguments)
                if psnr_gen > best_test_psnr_gen:
                    best_test_psnr_gen = psnr_gen
                    save_arguments['best_test_psnr_gen'] = best_test_psnr_gen
                    save_arguments['epoch'] = epoch
                    checkpointer.save('best_valid', **save_arguments)

    def _ema_eval(self, optimizer=None):
        """Whether evaluation runs on the averaged weights: SOLVER.ema_decay > 0 and SOLVER.ema_eval (and, when an optimiser is given,
        that optimiser keeps the average)."""
        on = float(self.cfg.SOLVER.get('ema_decay', 0.0)) > 0 and bool(self.cfg.SOLVER.get('ema_eval', True))
        return on and (optimizer is None or getattr(optimizer, 'ema_decay', 0.0) > 0)

    def _plan(self):
        """The loss's LossPlan as `self.cfg` says now; everything off unless the loss is losswrapper."""
        from ..network.loss.losses import LossPlan
        return LossPlan.from_cfg(self.cfg) if self.cfg.MODEL.loss == 'v1' else LossPlan()

    def _seg_weights(self):
        """SOLVER.seg_weights as the loss reads it (a 7-tuple, or None for off)."""
        return self._plan().seg_weights

    def _tail_terms(self):
        """The names of the loss terms behind the reference's elements of a loss row, in the row's order."""
        return self._plan().names

    def _slope_message(self):
        return 'psnr_slope_gen: {}, psnr_slope_reg: {}'.format(self.last_slope_psnr['gen'], self.last_slope_psnr['reg'])

    def _corr_message(self):
        return 'corr_gen: {}, corr_reg: {}'.format(self.last_corr['gen'], self.last_corr['reg'])

    def _seg_scalars(self):
        """(names, values) of last_seg_psnr: psnr_gen_seg_P .. psnr_gen_seg_TP, psnr_reg_seg_P .. psnr_reg_seg_TP."""
        from ..network.loss.losses import SEG_NAMES
        names = ['psnr_{}_seg_{}'.format(split, n) for split in ('gen', 'reg') for n in SEG_NAMES[:6]]
        return names, list(self.last_seg_psnr['gen']) + list(self.last_seg_psnr['reg'])

    def _seg_message(self):
        from ..network.loss.losses import SEG_NAMES
        return '\n'.join('psnr_{}_seg: '.format(split) + ', '.join('{} {}'.format(n, v) for n, v in zip(SEG_NAMES, self.last_seg_psnr[split]))
                         for split in ('gen', 'reg'))

    def _aug_eval(self, dl_test):
        """DATA.aug_eval: (psnr_gen, psnr_reg, ssim_gen, ssim_reg) of the test phase on corrupted inputs -- batch i under
        augment.eval_seed(cfg.seed, i, rank), so every epoch and every resumed run judges the same corrupted test set and no seed is a
        train step's.  The run goes on as if this pass had not happened: Python's `random` stream (the Standin draws), the model's
        forward counter and the eval-mode operand magnitudes of the split-fp16 call sites are put back."""
        state, calls, amax0 = random.getstate(), getattr(self.model, '_drop_calls', 0), ops.amax_snapshot(self.device)
        try:
            with torch.no_grad():
                metrics = self.run_one_epoch(dl_test, phase='test', collect_views=False, aug_eval=True)[4]
        finally:
            random.setstate(state)
            self.model._drop_calls = calls
            ops.amax_restore(self.device, amax0)
        self.last_aug_metrics = tuple(float(v) for v in np.mean(metrics, axis=0))
        return self.last_aug_metrics

    def _warp_eval(self, dl_test):
        """DATA.aug_warp_eval: (psnr_gen, psnr_reg, ssim_gen, ssim_reg) of the test phase on warped and jittered batches -- batch i under
        warp.eval_seed(cfg.seed, i, rank), so every epoch and every resumed run judges the same warped test set and no seed is a train
        batch's.  The run goes on as if this pass had not happened, as after `_aug_eval`; the read-outs of the unwarped pass
        (last_seg_psnr, last_slope_psnr, last_corr) stay."""
        state, calls, amax0 = random.getstate(), getattr(self.model, '_drop_calls', 0), ops.amax_snapshot(self.device)
        try:
            with torch.no_grad():
                metrics = self.run_one_epoch(dl_test, phase='test', collect_views=False, warp_eval=True)[4]
        finally:
            random.setstate(state)
            self.model._drop_calls = calls
            ops.amax_restore(self.device, amax0)
        self.last_warp_metrics = tuple(float(v) for v in np.mean(metrics, axis=0))
        return self.last_warp_metrics

    def val(self, dl_test, epoch=-1):
        """solver.py:118-137: load `best_valid.pkl` (epoch == -1) or `epoch_<n>.pkl`, run the test phase, print and
        return (psnr_gen, psnr_reg, ssim_gen, ssim_reg).  DATA.aug_eval with a corruption on: the corrupted test set's four numbers are
        printed behind them and kept in `last_aug_metrics`; the return value is the clean one."""
        self.model.eval()
        optimizer = get_optimizer(self.cfg, self.model.parameters())
        scheduler = get_lr_scheduler(self.cfg, optimizer)
        checkpointer = CheckPointer(self.model, optimizer, scheduler, self.output_dir)
        if epoch == -1:
            extra = checkpointer.load(best_valid=True, ema=self._ema_eval())
        else:
            extra = checkpointer.load(os.path.join(self.output_dir, 'epoch_{}.pkl'.format(epoch)), ema=self._ema_eval())
        print('the latest best_test_psnr_gen is {:06f} of epoch {}'.format(extra.get('best_test_psnr_gen', 0.),
                                                                           extra.get('epoch', 0)))
        with torch.no_grad():
            mertics_all = self.run_one_epoch(dl_test, phase='test', collect_views=False)[4]
        psnr_gen, psnr_reg, ssim_gen, ssim_reg = (float(v) for v in np.mean(mertics_all, axis=0))
        print('psnr_gen:{}, psnr_reg:{}, ssim_gen:{}, ssim_reg:{}'.format(psnr_gen, psnr_reg, ssim_gen, ssim_reg))
        if self.seg_eval:
            print(self._seg_message())
        if self.slope_eval:
            print(self._slope_message())
        if self.corr_eval:
            print(self._corr_message())
        if self.augment is not None and self.augment.eval:
            print('psnr_gen_aug:{}, psnr_reg_aug:{}, ssim_gen_aug:{}, ssim_reg_aug:{}'.format(*self._aug_eval(dl_test)))
        if self.warp is not None and self.warp.eval:
            print('psnr_gen_warp:{}, psnr_reg_warp:{}, ssim_gen_warp:{}, ssim_reg_warp:{}'.format(*self._warp_eval(dl_test)))
        if self.locate_eval:
            self.locate(dl_test)
            print(self._locate_message())
        return psnr_gen, psnr_reg, ssim_gen, ssim_reg

    def _locate_message(self):
        return '\n'.join(', '.join('{}:{}'.format(k, v) for k, v in self.last_locate.items() if k.endswith(split)) for split in ('_gen', '_reg'))

    def locate(self, dl_test):
        """SOLVER.locate_*: locate every rest view of every test batch from the batch's input leads -- observed = rest_view, the truth is
        rest_theta; one encoder pass and one level-0 panorama per batch, for all rest views together (Model_nefnet.locate), rows cropped as
        the test phase's metrics crop them.  Fills and returns last_locate: the mean (locate_err1_*, locate_err2_*) and median
        (locate_err1_med_*, locate_err2_med_*) of |theta - truth| on both axes in degrees, and locate_hit_*, the share of views found
        within one level-0 step on both axes, for the view split of psnr_gen / psnr_reg (`*` = gen, reg); a view without a finite score
        counts as a miss and is left out of the errors.  The settings are the config's whether or not locate_eval is on.  The run goes on
        as if this pass had not happened: Python's `random` stream, the model's forward counter, its mode and the eval-mode operand
        magnitudes of the split-fp16 call sites are put back.  One rank only."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("SOLVER.locate_eval under data parallelism: the located views are not gathered over the ranks")
        kw = _locate.from_cfg(self.cfg, force=True)
        gen_num, whole = self._gen_num()
        found_s, truth_s = _HostSink(), _HostSink()
        state, calls, amax0 = random.getstate(), getattr(self.model, '_drop_calls', 0), ops.amax_snapshot(self.device)
        was_training = self.model.training
        try:
            with torch.no_grad():
                for meta in dl_test:
                    source_data, rois, input_theta = self._to_device(meta)[:3]
                    rest_view = torch.as_tensor(meta['rest_view']).to(self.device, torch.float32).contiguous()
                    res = self.model.locate(source_data, input_theta, rois, rest_view, crop=not whole, **kw)
                    found_s.add(res.theta)
                    truth_s.add(torch.as_tensor(meta['rest_theta']).to(self.device, torch.float32).contiguous())
        finally:
            random.setstate(state)
            self.model._drop_calls = calls
            ops.amax_restore(self.device, amax0)
            self.model.train(was_training)
        found = [a.astype(np.float64) for a in found_s.arrays()]
        truth = [a.astype(np.float64) for a in truth_s.arrays()]
        d1, d2 = (np.degrees(d) for d in kw['grid'].steps)
        self.last_locate = {}
        for split in ('gen', 'reg'):
            sl = slice(None) if whole else (slice(-gen_num, None) if split == 'gen' else slice(None, -gen_num))
            err = [np.degrees(np.abs(f[:, sl] - t[:, sl])).reshape(-1, 2) for f, t in zip(found, truth)]
            err = np.concatenate(err) if err else np.zeros((0, 2))
            ok = ~np.isnan(err).any(axis=1)
            good = err[ok]
            nan = float('nan')
            self.last_locate['locate_err1_' + split] = float(good[:, 0].mean()) if good.size else nan
            self.last_locate['locate_err1_med_' + split] = float(np.median(good[:, 0])) if good.size else nan
            self.last_locate['locate_err2_' + split] = float(good[:, 1].mean()) if good.size else nan
            self.last_locate['locate_err2_med_' + split] = float(np.median(good[:, 1])) if good.size else nan
            hit = ok & (np.nan_to_num(err[:, 0], nan=np.inf) <= d1) & (np.nan_to_num(err[:, 1], nan=np.inf) <= d2)
            self.last_locate['locate_hit_' + split] = float(hit.mean()) if err.shape[0] else nan
        return self.last_locate

    def _to_device(self, meta):
        dev = self.device
        t = lambda v: torch.as_tensor(v).to(dev, non_blocking=True)   # noqa: E731
        return (t(meta['data']), t(meta['rois']), t(meta['input_theta']), t(meta['target_view']).unsqueeze(1),
                t(meta['target_theta']), t(meta['noise']).unsqueeze(1))

    def _warp_batch(self, source_data, target_view, rest_view, rois, seed):
        """The batch warped under `seed` (ops.warp: one launch on the current stream into fresh tensors); float32 rows, as the model
        takes them."""
        f = lambda v: None if v is None else v.to(torch.float32).contiguous()   # noqa: E731
        return ops.warp(f(source_data), f(target_view), f(rest_view), rois.contiguous(), self.warp, seed)

    def _gen_num(self):
        """How many trailing rest views are 'generated' (never supervised), and whether the split applies at all
        (solver.py:197-203)."""
        gen_num = 6 if self.cfg.DATA.lead_num == 336 else 4
        super_mode = str(self.cfg.DATA.get('super_mode', 'normal'))
        whole = self.cfg.DATA.get('dataset', 'tianchi') == 'mit' or super_mode[-1] == '0' or super_mode == '_mit'
        # the reference eval()s the last character before it looks at `whole` (solver.py:198) and would crash on '_mit';
        # the split count is only consumed when `whole` is false, so it is only parsed then
        if super_mode != 'normal' and not whole:
            if not super_mode[-1].isdigit():
                raise ValueError(f"DATA.super_mode {super_mode!r}: the last character must be the number of generated views")
            gen_num = int(super_mode[-1])
        return gen_num, whole

    def _loss_rois(self, rois):
        """`rois=` for the loss when a term of its plan is on (losswrapper takes it then); nothing otherwise."""
        return {'rois': rois} if self._plan().any_on else {}

    def _graphed_step(self, optim, data, keep):
        """The hipGraph stepper for this batch, or None when the step runs eagerly: `cfg.SOLVER.graph` False, the per-view host lists are wanted (the graph returns losses only), the
        model is not the plain Model_nefnet train path, or the optimiser is not a fused one (FusedSGD, FusedAdam) with one
        parameter group."""
        mode = self.cfg.SOLVER.get('graph', None)
        mode = 'auto' if mode is None or mode == 'auto' else bool(mode)
        if mode is False or keep:
            return None
        if not hasattr(optim, '_flat') or len(optim.param_groups) != 1:
            return None
        if type(self.model).__name__ != 'Model_nefnet' or _env.get('NEF_SOLVER_GRAPH', '1') == '0':
            return None
        # 'auto' = wherever the conditions above hold, at every batch size: with the convs on the fp16 matrix cores even the
        # full-size step (configs[1]: ~290 launches, 36 ms) loses 2.5-4.5 ms to launch gaps when a busy host issues it from Python
        # (bench.py --no-graph against the default); rounds 1-3 replayed launch-bound shapes only
        st = getattr(self, '_graph_stepper', None)
        if st is None or st.optimizer is not optim:
            from ..graph import GraphedTrainStep
            st = self._graph_stepper = GraphedTrainStep(self.model, self.cfg, optimizer=optim)
        return st

    def _check_h2_range(self, phase, optim):
        """The split-fp16 convs count a launch whose operand is out of fp16's range even after the in-launch range rescue: non-finite
        data (finite operands beyond ops.H2_HEADROOM x of growth are redone with their own scale inside the launch), or any
        clamp of the opt-in producer / consumer kernel form (fp16 ends at 65504; the reference's fp32 nn.Conv1d,
        model_nefnet.py:18-21, has no such limit).  A train step that contained such a launch was SKIPPED on the device when the
        optimiser is a fused one, FusedSGD or FusedAdam (ops.h2_taint): that is reported; counts nothing protected against -- a test-phase forward,
        another optimiser -- mean wrong results were used: raise, unless NEF_H2_ALLOW_CLAMP=1 (then warn).  NEF_H2=0 runs the
        fp32 kernels instead.  Data parallel: the counters are per rank, so they are SUMMED over the process group before anything
        is decided -- every rank raises (or warns) together; a rank that alone saw the bad operand must not leave the others
        blocking in their next collective."""
        clamped, skipped = parallel.sum_counts([ops.h2_clamped(), ops.h2_skipped()], self.device)
        ops.h2_rebase(self.device)       # clamps of this (test / val) phase are not charged to the next train step's taint word
        tails, moved = ops.h2_tail_sites(), ops.h2_fallback_sites()
        if tails and ops.H2_TAIL_MODE == 'fp32':      # (per rank: a report only)
            print('NOTE: {} split-fp16 call site(s) measured a heavy-tailed operand (more than {:.0%} of its nonzero elements below 2^-11 of '
                  'its largest); {} weight-gradient site(s) of them now run on the fp32 kernels (NEF_H2_TAIL=fp32), the forward / '
                  'backward-data ones keep the split kernels'.format(tails, ops.H2_TAIL_FRAC, moved))
        elif tails:
            print('WARNING: {} split-fp16 call site(s) measured an operand with more than {:.0%} of its nonzero elements below 2^-11 of its '
                  'largest: practically the whole tensor is outside the format\'s full-precision window (DESIGN.md 3.0); NEF_H2_TAIL=fp32 '
                  'runs those weight-gradient sites on the fp32 kernels, NEF_H2=0 every conv'.format(tails, ops.H2_TAIL_FRAC))
        if not clamped and not skipped:
            return
        msg = ('{} waves of split-fp16 conv launches met an operand outside fp16\'s range in this {} phase (non-finite data; finite '
               'operands are rescaled inside the launch); {} train step(s) were skipped on the device'.format(clamped, phase, skipped))
        protected = phase == 'train' and hasattr(optim, '_flat') and skipped > 0
        if protected or _env.get('NEF_H2_ALLOW_CLAMP') == '1':
            print('WARNING: ' + msg + ('' if protected else ' -- results of those launches are wrong (NEF_H2_ALLOW_CLAMP=1)'))
            return
        raise RuntimeError(msg + '; their results are wrong.  Set NEF_H2=0 (fp32 kernels), or NEF_H2_ALLOW_CLAMP=1 to continue')

    def run_one_epoch(self, dl, phase, optim=None, collect_views=None, aug_eval=False, warp_eval=False):
        """solver.py:139-246.  `collect_views` (default: the Solver's setting) = also return the per-view host lists the
        reference returns (inputs, ground truth, predictions, rois); train() / val() only consume losses and metrics and
        pass False, so an epoch stages nothing but a few scalars per step.  With DATA.aug_* on, the inputs in those lists are the CLEAN
        ones the loader delivered: the corrupted copy lives inside the step.  `aug_eval` (test phase, DATA.aug_* on): the model reads
        batch i corrupted under augment.eval_seed(cfg.seed, i, rank) -- the robustness read-out of `_aug_eval`.  With DATA.aug_warp /
        aug_roi_jitter on, the train phase's lists hold the WARPED batch: what the step saw.  `warp_eval` (test phase, a warp on): batch i
        is warped under warp.eval_seed(cfg.seed, i, rank) -- inputs, target, rest views and rois -- the read-out of `_warp_eval`."""
        if warp_eval and (phase != 'test' or self.warp is None):
            raise ValueError('warp_eval is the test phase with DATA.aug_warp / DATA.aug_roi_jitter on')
        if aug_eval and (phase != 'test' or self.augment is None):
            raise ValueError('aug_eval is the test phase with a DATA.aug_* corruption on')
        if phase == 'train' and (self.augment is not None or self.device_noise):
            # the step's seed counts from the start of the epoch: a function of (seed, epoch, batch index, rank) on the eager and the
            # replayed path alike, whatever ran in between (test phases, a resume)
            self.model._drop_calls = 0
            if getattr(self, '_graph_stepper', None) is not None:
                self._graph_stepper.calls = 0
        if phase == 'train':
            self.model.train()
        elif phase == 'test':
            self.model.eval()
        else:
            raise ValueError('phase param not found.')
        keep = self.collect_views if collect_views is None else bool(collect_views)
        losses_s, pred_s, gt_s, in_s, rest_s, rois_s, psnr_s, ssim_s = (_HostSink() for _ in range(8))
        clean = phase == 'test' and not (aug_eval or warp_eval)         # the read-out passes fill none of the three below
        seg_s = (_HostSink(), _HostSink()) if clean and self.seg_eval else None          # (se, cnt) per clean batch
        slope_s = (_HostSink(), _HostSink()) if clean and self.slope_eval else None      # (se, cnt) per clean batch
        corr_s = (_HostSink(), _HostSink()) if clean and self.corr_eval else None        # (mom, cnt) per clean batch
        gen_num, whole = self._gen_num() if phase == 'test' else (0, True)
        # gradient-norm clipping (SOLVER.clip_grad_norm): [norm, coefficient] of every train step travel like the losses
        clip_s = _HostSink() if phase == 'train' and getattr(optim, 'max_grad_norm', 0.0) > 0 else None
        # the optimiser's counters (steps clipped, steps with a non-finite norm) before this epoch: nothing is in flight here
        clip_0 = optim.clip_stats[2:].tolist() if clip_s is not None and optim.clip_stats is not None else [0.0, 0.0]
        # SOLVER.optim lars / lamb: the count of steps skipped for non-finite norms before this epoch
        trust = phase == 'train' and hasattr(optim, 'trust_ratios')
        trust_0 = float(optim.trust_stats[3].item()) if trust and optim.trust_stats is not None else 0.0
        # SOLVER.accum_steps: an update closes every window of K train batches; clip_stats are recorded per UPDATE, not per batch
        accum = phase == 'train' and getattr(optim, 'accum_steps', 1) > 1
        # the per-update learning-rate schedule: the count the epoch starts from is the host's (the previous epoch's read; before the first
        # step: the loaded or zero count, no device word exists yet) and so is the rate of its first update
        lr_on = phase == 'train' and getattr(optim, '_sched_on', False)
        if lr_on and (getattr(self, '_lr_seen', None) is None or self._lr_seen[0] is not optim):
            self._lr_seen = (optim, optim.lr_state()[0])
        lr_first = float(np.float32(float(optim.param_groups[0]['lr']) * optim.lr_schedule.factor(self._lr_seen[1]))) if lr_on else None
        n_batches = n_updates = 0
        n_views = self.train_views if phase == 'train' else 1
        warp_rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        if n_views >= 2 and type(self.model).__name__ != 'Model_nefnet':
            raise ValueError("SOLVER.train_views >= 2 is Model_nefnet's multi-view train step; {} takes one view".format(type(self.model).__name__))
        for meta in dl:
            source_data, rois, input_theta, target_view, target_theta, noise = self._to_device(meta)
            rest_theta = torch.as_tensor(meta['rest_theta']).to(self.device) if 'rest_theta' in meta else None
            if n_views >= 2:
                # this step's targets: Q of the S supervised rest views -- one draw from (seed, epoch, batch index), the same on every
                # rank and in a resumed run; target_view / target_theta are not used.  [Q, B, 1, L] and [Q, B, 2], view-major
                if rest_theta is None or 'rest_view' not in meta:
                    raise KeyError("SOLVER.train_views >= 2 needs the batch's rest_view / rest_theta (train_net.build_loaders ships them)")
                rest_view = torch.as_tensor(meta['rest_view']).to(self.device, non_blocking=True)
                if self.warp is not None:         # the views are drawn from the warped rest views
                    source_data, target_view, rest_view, rois = self._warp_batch(
                        source_data, target_view, rest_view, rois,
                        _warp.train_seed(self.cfg.get('seed', 0), int(getattr(self.model, 'dropout_epoch', 0)), n_batches, warp_rank))
                n_sup = views.supervised_views(self.cfg, rest_theta.shape[1])
                views.check_views(n_views, min(n_sup, rest_view.shape[1]))
                picked = views.draw_views(self.cfg.get('seed', 0), int(getattr(self.model, 'dropout_epoch', 0)), n_batches, n_views, n_sup)
                target_view, target_theta = views.select_views(rest_view, rest_theta, picked)
            elif phase == 'train' and self.warp is not None:
                source_data, target_view, _, rois = self._warp_batch(
                    source_data, target_view, None, rois,
                    _warp.train_seed(self.cfg.get('seed', 0), int(getattr(self.model, 'dropout_epoch', 0)), n_batches, warp_rank))
            stepper = self._graphed_step(optim, source_data, keep) if phase == 'train' else None
            if stepper is not None:
                # forward + losswrapper + backward + SGD as ONE replayed hipGraph (one graph per batch shape: the final partial
                # batch has its own; a learning-rate change re-captures); data parallel: the flat gradient travels as one
                # all-reduce behind the replay (no early bucket under capture)
                losses_s.add(stepper(source_data, input_theta, target_theta, rois, target_view,
                                     noise=noise if self.cfg.DATA.noise else None))
            elif phase == 'train':
                out, shuf_p, shuf_l = self.model(source_data, input_theta, target_theta, rois, rest_theta=rest_theta,
                                                 phase='train')
                if keep:       # solver.py:179 (before the optional noise); multi-view: one [Q, B, L] entry per batch
                    pred_s.add(out.squeeze(1) if n_views < 2 else out.squeeze(2).unsqueeze(0))
                # DATA.noise (solver.py:185-186): the loss kernels add the row to the prediction, no launch of its own
                step_noise = noise if self.cfg.DATA.noise else None
                if self.device_noise:
                    # DATA.device_noise: the row from this step's final target rows and rois (behind the warp and the view selection),
                    # under the seed of the forward that has just run -- the captured launch of the graphed step at the same step seed
                    step_noise = ops.noise_row(*_device_noise.rows(target_view, rois),
                                               seed=_device_noise.train_seed(self.model.last_step_seed))
                losses = self.loss(out, shuf_p, shuf_l, target_view, self.cfg, noise=step_noise, **self._loss_rois(rois))
                losses_s.add(torch.stack([l_.detach() for l_ in losses]))
                losses[0].backward()
                optim.step()
                optim.zero_grad()
            else:
                rest_view = torch.as_tensor(meta['rest_view']).to(self.device, torch.float32).contiguous()
                mask_kw = {}                # the clean test phase passes no mask
                if warp_eval:
                    source_data, target_view, rest_view, rois = self._warp_batch(
                        source_data, target_view, rest_view, rois, _warp.eval_seed(self.cfg.get('seed', 0), n_batches, warp_rank))
                if aug_eval:
                    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
                    source_data = ops.augment(source_data.to(torch.float32).contiguous(), rois, self.augment,
                                              seed=augment.eval_seed(self.cfg.get('seed', 0), n_batches, rank))
                    if self.lead_mask:      # MODEL.lead_mask: the read-out's head is told which leads its own fixed seed dropped
                        mask_kw = dict(lead_mask=ops.augment_mask(source_data.shape[0], source_data.shape[1], self.augment.lead_drop,
                                                                  seed=augment.eval_seed(self.cfg.get('seed', 0), n_batches, rank),
                                                                  device=source_data.device))
                out, shuf_p, shuf_l, rest_out = self.model(source_data, input_theta, target_theta, rois,
                                                           rest_theta=rest_theta, phase='test', **mask_kw)
                losses = self.loss(out, shuf_p, shuf_l, target_view, self.cfg, rest_out[:, -4:, :].contiguous(),
                                   rest_view[:, -4:, :].contiguous(), **self._loss_rois(rois))
                losses_s.add(torch.stack([l_.detach() for l_ in losses]))
                ps, ss = ops.view_metrics(rest_out.contiguous(), rest_view, None if whole else rois.contiguous())
                psnr_s.add(ps)
                ssim_s.add(ss)
                if seg_s is not None:
                    se, cnt = ops.view_seg_metrics(rest_out.contiguous(), rest_view, rois.to(torch.int64).contiguous())
                    seg_s[0].add(se)
                    seg_s[1].add(cnt)
                if slope_s is not None:           # the rows of view_metrics: cropped at rois[i, -1, 0] unless the split is off
                    se, cnt = ops.view_slope_metrics(rest_out.contiguous(), rest_view,
                                                     None if whole else rois.to(torch.int64).contiguous())
                    slope_s[0].add(se)
                    slope_s[1].add(cnt)
                if corr_s is not None:            # the same rows
                    mom, cnt = ops.view_corr_metrics(rest_out.contiguous(), rest_view,
                                                     None if whole else rois.to(torch.int64).contiguous())
                    corr_s[0].add(mom)
                    corr_s[1].add(cnt)
                if keep:
                    pred_s.add(rest_out)                           # solver.py:182
                    rest_s.add(rest_view)
            updated = phase == 'train' and not (accum and optim.window_open)
            n_batches += 1
            n_updates += int(updated)
            if updated and clip_s is not None and optim.clip_stats is not None:
                clip_s.add(optim.clip_stats[:2])
            if keep:
                gt_s.add(target_view.squeeze(1) if n_views < 2 else target_view.squeeze(2).unsqueeze(0))
                in_s.add(source_data)
                rois_s.add(rois)
        if accum and optim.window_open:
            # a window never crosses an epoch: the incomplete last one is flushed on the micro-batches it has (issued eagerly, also behind
            # replayed micro-batches: the stepper and the optimiser share the window)
            optim.flush()
            n_updates += 1
            if clip_s is not None and optim.clip_stats is not None:
                clip_s.add(optim.clip_stats[:2])
        losses = [a.tolist() for a in losses_s.arrays()]
        self._check_h2_range(phase, optim)       # same cadence as the loss read-back above: the device has been waited for anyway
        if phase == 'train':
            # [norm, coefficient] of every step and this epoch's (steps clipped, steps skipped for a non-finite norm); clipping off: empty
            self.last_grad_norms, self.last_clip_counts = [], (0, 0)
            self.last_updates = (n_updates, n_batches)      # (equal unless SOLVER.accum_steps > 1)
            if clip_s is not None and optim.clip_stats is not None:
                self.last_grad_norms = [a.tolist() for a in clip_s.arrays()]
                clip_1 = optim.clip_stats[2:].tolist()
                self.last_clip_counts = (int(clip_1[0] - clip_0[0]), int(clip_1[1] - clip_0[1]))
            # the schedule's (first, last) effective rate of this epoch and the count behind it: ONE read, here
            self.last_lr = self.last_lr_updates = None
            if lr_on:
                t_now, lr_now = optim.lr_state()
                self.last_lr, self.last_lr_updates, self._lr_seen = (lr_first, lr_now), t_now, (optim, t_now)
            # trust ratios (SOLVER.optim lars / lamb) of the last updating step: name -> q, (min, max) over the adapted tensors and this
            # epoch's steps skipped for non-finite norms -- read once, here, where the device has been waited for anyway
            self.last_trust_ratios, self.last_trust_stats = {}, None
            if trust and optim.trust_stats is not None:
                st = optim.trust_stats.tolist()
                self.last_trust_ratios = optim.trust_ratios()
                self.last_trust_stats = (st[0], st[1], int(st[3] - trust_0))
            return losses, gt_s.rows(), pred_s.rows(), in_s.rows(), [], rois_s.rows()
        mertics_all, mertics_gen_singlelead = [], []
        for ps, ss in zip(psnr_s.arrays(), ssim_s.arrays()):
            if np.isnan(ss).any():
                raise ValueError("win_size exceeds signal extent (a test row is shorter than the 7-tap SSIM window)")
            if whole:
                pg = pr = float(ps.mean())
                sg = sr = float(ss.mean())
            else:
                pg, pr = float(ps[:, -gen_num:].mean()), float(ps[:, :-gen_num].mean())
                sg, sr = float(ss[:, -gen_num:].mean()), float(ss[:, :-gen_num].mean())
                Q = ps.shape[1]
                mertics_gen_singlelead.append([[float(ps[:, Q - gen_num + i].mean()), float(ss[:, Q - gen_num + i].mean())]
                                               for i in range(gen_num)])
            mertics_all.append([pg, pr, sg, sr])
        if seg_s is not None:
            # per batch the mean over the split's (row, view) pairs that own positions of the segment, then the mean over batches as
            # psnr_gen / psnr_reg are formed (a batch without any such pair is left out)
            per_batch = {'gen': [], 'reg': []}
            for se, cnt in zip(seg_s[0].arrays(), seg_s[1].arrays()):
                per_batch['gen'].append(seg_psnr(se, cnt) if whole else seg_psnr(se[:, -gen_num:], cnt[:, -gen_num:]))
                per_batch['reg'].append(seg_psnr(se, cnt) if whole else seg_psnr(se[:, :-gen_num], cnt[:, :-gen_num]))
            self.last_seg_psnr = {}
            for split, rows in per_batch.items():
                a = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
                ok = ~np.isnan(a)
                self.last_seg_psnr[split] = [float(a[ok[:, k], k].mean()) if ok[:, k].any() else float('nan') for k in range(6)]
        if slope_s is not None:
            # per batch the mean over the split's (row, view) pairs that have a difference, then the mean over batches, as psnr_gen /
            # psnr_reg are formed (a batch without any such pair is left out)
            per_batch = {'gen': [], 'reg': []}
            for se, cnt in zip(slope_s[0].arrays(), slope_s[1].arrays()):
                per_batch['gen'].append(slope_psnr(se, cnt) if whole else slope_psnr(se[:, -gen_num:], cnt[:, -gen_num:]))
                per_batch['reg'].append(slope_psnr(se, cnt) if whole else slope_psnr(se[:, :-gen_num], cnt[:, :-gen_num]))
            self.last_slope_psnr = {}
            for split, vals in per_batch.items():
                a = np.asarray(vals, dtype=np.float64)
                ok = ~np.isnan(a)
                self.last_slope_psnr[split] = float(a[ok].mean()) if ok.any() else float('nan')
        if corr_s is not None:
            # the mean coefficient over the split's (row, view) pairs of the whole phase that have at least two samples; NaN without one
            from ..network.loss.losses import CORR_EPS
            eps = float(self.cfg.SOLVER.get('corr_eps', CORR_EPS))
            pairs = {'gen': [], 'reg': []}
            for mom, cnt in zip(corr_s[0].arrays(), corr_s[1].arrays()):
                pairs['gen'].append(corr_pairs(mom, cnt, eps) if whole else corr_pairs(mom[:, -gen_num:], cnt[:, -gen_num:], eps))
                pairs['reg'].append(corr_pairs(mom, cnt, eps) if whole else corr_pairs(mom[:, :-gen_num], cnt[:, :-gen_num], eps))
            self.last_corr = {}
            for split, vals in pairs.items():
                a = np.concatenate(vals) if vals else np.zeros(0)
                self.last_corr[split] = float(a.mean()) if a.size else float('nan')
        return losses, rest_s.rows(), pred_s.rows(), in_s.rows(), mertics_all, rois_s.rows(), mertics_gen_singlelead
