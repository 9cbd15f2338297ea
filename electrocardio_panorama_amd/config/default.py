"""Default configuration tree.  Key names and default values follow reference codes/config/default.py:4-55 (they are
the drop-in surface: `cfg.SOLVER.lr`, `cfg.DATA.lead_num`, ...); the tree is declared once as a nested literal."""
from .cfgnode import CfgNode

_DEFAULTS = {
    "seed": 123,
    "fit_msg": "None",
    "output_dir": "{your folder}",
    "latent_save_dir": "{your folder}",
    "desc": "model_v2_tianchi",
    "DATA": {
        "dataset": "tianchi",
        "train_label_path": "data/tianchi/tianchi_train_jsons.txt",
        "test_label_path": "data/tianchi/tianchi_test_jsons.txt",
        "train_data_root": "data/tianchi/npy_data/tianchi_train_round1",
        "train_label_root": "data/tianchi/tianchi_interval",
        "train_pkl_path": "data/PTB/pkl_data/train_heartbeats.pkl",
        "test_pkl_path": "data/PTB/pkl_data/test_heartbeats.pkl",
        "noise_std": [4.37258895, 4.73799667, 5.00643047, 6.7582663, 6.57354042, 6.31023917, 6.05944371, 7.05612394],
        "lead_num": 1,                 # V: number of input leads (views)
        "noise": False,                # add the per-lead noise sample to the prediction before the loss
        "train_data_mode": "normal",
        "super_mode": "normal",
        "weighted_sample": False,
        "synthetic": False,            # (not in the reference) train / validate on seeded synthetic `meta` batches
        # (not in the reference) corruption of the INPUT leads of every train step, on the device (nef_augment: one launch in front of
        # the stem, in the eager and the graphed step; targets and rest views stay clean; augment.py).  Every draw comes from the step's
        # counter-RNG seed, so a resumed run and a replayed step see the same corruption, and shards differ.  The four amplitude /
        # probability keys at 0 = off: no launch, no buffer, the graphs and bits are what they were before the keys existed
        "aug_noise_std": 0.0,          # sigma of white Gaussian noise on every input lead, in signal units (the loaders' rows are in [0, 1])
        "aug_wander_amp": 0.0,         # largest amplitude of ONE baseline-wander sinusoid per (sample, lead): amplitude, frequency, phase drawn
        "aug_wander_hz": [0.05, 0.7],  # its frequency range [lo, hi], Hz
        "aug_hum_amp": 0.0,            # largest amplitude of ONE mains-hum sinusoid per (sample, lead): amplitude and phase drawn
        "aug_hum_hz": 50.0,            # its frequency, Hz
        "aug_lead_drop": 0.0,          # probability that an input lead of a sample is zeroed (in [0, 1)); every sample keeps at least one lead
        "sample_rate": 500.0,          # Hz: turns the two frequencies into turns per sample
        "aug_crop": True,              # corrupt positions t < rois[i, -1, 0] only (the row's valid extent, as SOLVER.ssim_crop); padding stays
        # with any corruption on: Solver.train / Solver.val run the test phase a second time on corrupted inputs -- one fixed corrupted
        # test set per (seed, batch index, rank) -- and log psnr_gen_aug / psnr_reg_aug / ssim_gen_aug / ssim_reg_aug; best_valid stays on
        # the clean psnr_gen
        "aug_eval": False,
        # (not in the reference) time warp of the whole train batch on the device, in front of everything else in the step (warp.py;
        # nef_warp): inputs, target, rest views and rois change together, DATA.aug_* then corrupts the warped inputs.  Every draw is a
        # function of (seed, epoch, batch index, rank, sample).  Not with DATA.noise (its row is padded to the unwarped beat)
        "aug_warp": [],                # off when empty; else six amplitudes [P, PR, QRS, ST, T, TP], each in [0, 0.9]: segment k of every
                                       # train beat is resampled to 1 + a_k (2 u - 1) times its length, u uniform per (sample, segment)
        "aug_roi_jitter": 0,           # J in 0..64: each of the five interior marks of the warped beat moves by an integer drawn
                                       # uniformly from [-J, J]; the signal does not move
        # with a warp or a jitter on: Solver.train / Solver.val run the test phase once more on one fixed warped and jittered test set
        # per (seed, batch index, rank) and log psnr_gen_warp / psnr_reg_warp / ssim_gen_warp / ssim_reg_warp; best_valid stays on the
        # unwarped psnr_gen
        "aug_warp_eval": False,
        # (not in the reference) keep the phase's Tianchi recordings in device memory and build every batch there: the host draws a small
        # integer plan per batch, one launch of nef_beat_batch crops, derives, normalises and pads (dataset/resident.py; the bits of the
        # host loader's items).  train_net.build_loaders and val_net hand out ResidentLoaders instead of DataLoaders: no worker processes.
        # Deliberately not on this path, ValueError with the key on: DATA.noise (it needs the quiet segment's sigma and a device draw, a
        # different random stream from the host's), every dataset but tianchi (PTB), DATA.weighted_sample, DATA.synthetic.
        # False: the DataLoaders, launches and bits are what they were before the key existed
        "device_resident": False,
        # (not in the reference) with device_resident: the store reads the SIGNALS of the label list's recordings only -- no <id>.json is
        # opened -- and makes the six 'P on' .. 'T off' lists itself: a QRS detector on the device (nef_mark_envelope, nef_mark_peaks) and
        # the timing table of mark_table, which `python -m electrocardio_panorama_amd.mark_net --fit` fits on an annotated list
        # (dataset/marks.py).  Rejected without device_resident -- `mark_net --write` writes label files for the host
        # loader -- and DATA.weighted_sample stays rejected.  False: no launch, no buffer, the loaders, graphs and bits are what they were
        # before the key existed
        "auto_marks": False,
        "mark_table": "",              # the JSON table file; required with auto_marks
        # a recording that gets no labels (fewer than two beats left) is an error; True: it is dropped from the store, one warning counts them
        "auto_marks_skip": False,
        # (not in the reference) DATA.noise's addend drawn by the TRAIN step itself on the device (device_noise.py; nef_noise_row): per
        # target row a Gaussian draw whose sigma is the standard deviation of the quiet second half of the row's T-P segment, taken from
        # the step's final target rows and rois -- behind the warp and the view selection -- and handed to the loss where DATA.noise's row
        # goes, in the eager and the graphed step; meta['noise'] is not read, the test phase adds no noise.  Goes with everything
        # DATA.noise is rejected with (device_resident, auto_marks, aug_warp / aug_roi_jitter, SOLVER.train_views >= 2) and with synthetic
        # batches; ValueError together with DATA.noise.  A segment without a sample inside the row gives sigma 0 and a row of zeros (the
        # host row is NaN there).  Every draw comes from the step's counter-RNG seed: a resumed run and a replayed step see the same row,
        # steps and shards differ.  False: no launch, no buffer, the graphs and bits are what they were before the key existed
        "device_noise": False,
        # (not in the reference) with device_resident: the files hold recordings at source_rate Hz, not at sample_rate.  The store uploads
        # them as they are and resamples them on the device to sample_rate -- a rational polyphase FIR, Kaiser-windowed sinc, per-phase
        # normalised (resample.py; nef_resample) -- into a float32 store; annotated label lists are rescaled on the host,
        # auto_marks detects on the resampled signal, and everything that counts samples (the 512-sample beat, the detector, the timing
        # table, aug_wander_hz / aug_hum_hz, the SSIM window) keeps counting them at sample_rate.  Whole positive rates only, sample_rate
        # too with the key on; up <= 1024, down <= 8 up, at most 512 taps a phase: ValueError otherwise, and without device_resident
        # (`mark_net --resample DIR` writes resampled files for the host loader).  0, or sample_rate itself: no launch, no buffer, the store
        # stays int16 / float32 and the loaders, graphs and bits are what they were before the key existed
        "source_rate": 0,
        "resample_zeros": 16,          # zero crossings of the sinc on each side of its centre, at the lower of the two rates
        "resample_beta": 8.6,          # the Kaiser window's beta
        # (not in the reference) with device_resident: clean the recordings on the device behind the resampling and in front of the
        # detector (clean.py).  baseline_ms = [w1, w2] removes the baseline wander: the signal minus the w2-ms sliding
        # median of its w1-ms sliding median (nef_sliding_median; [200, 600] is the usual pair, 101 and 301 samples at 500 Hz; windows
        # in milliseconds at sample_rate, half widths 1..512 samples).  mains_hz = 50 or 60 removes the mains hum: a linear-phase
        # band-stop mains_width_hz wide, a Kaiser-windowed FIR of mains_taps taps with unit gain at 0 Hz, run first through nef_resample
        # at 1/1.  Either key makes the store float32, in the cleaned signal's units; lengths, offsets and annotated labels stay,
        # auto_marks detects on the cleaned signal.  ValueError without device_resident (`mark_net --clean DIR` writes cleaned files for
        # the host loader).  [] and 0: no launch, no buffer, the store stays int16 / float32 and the loaders, graphs and bits are what
        # they were before the keys existed
        "baseline_ms": [],
        "mains_hz": 0.0,
        "mains_width_hz": 6.0,         # the stop band's width: mains_hz -+ half of it
        "mains_taps": 511,             # odd, 3..511
        "mains_beta": 8.6,             # the Kaiser window's beta
    },
    "MODEL": {
        "model": "modelv2",            # 'model_nefnet' selects Nef-Net
        "resume": "",
        "loss": "v1",                  # 'v1' = losswrapper (L1/L2 + Standin terms)
        "jitter_factor": 0.0,          # view-angle jitter in degrees (dataset side)
        "theta_L": 1,
        # True (needs DATA.aug_lead_drop > 0): the train step -- and the DATA.aug_eval read-out -- hand the head a per-sample lead mask of the
        # leads aug_lead_drop zeroed, so the lead mean and the Standin picks run over the present leads only and a dropped lead's encoder
        # output is never averaged in (include/nefnet_hip.h, nef_lead_mask_mix_fwd_args).  The masked head runs the
        # un-fused three-pass route.  The clean test phase passes no mask.  Inference: the `lead_mask=` keyword of Model_nefnet.forward /
        # gen_ecg / panorama / locate.  False: the launches, graphs and bits are what they were before the key existed
        "lead_mask": False,
    },
    "SOLVER": {
        # 'sgd' (FusedSGD: torch.optim.SGD, momentum 0.9), 'adam' (FusedAdam: torch.optim.Adam) or 'adamw' (FusedAdamW: torch.optim.AdamW)
        "optim": "sgd",
        "scheduler": "steplr",
        "lr_step": [150, 350],
        "lr": 1e-3,
        "epochs": 500,
        "OurLoss1_version": "v2",
        "reg_loss": "l1_loss",         # 'l1_loss' | 'l2_loss' for the reconstruction term
        "loss_using": [1, 2, 3],
        "part_loss_no_grad": False,
        "loss_factor": [1, 1, 1],
        # train step as one captured hipGraph (graph.GraphedTrainStep): None / 'auto' = replay at EVERY batch size wherever the step
        # qualifies (plain Model_nefnet train path, a fused optimiser -- FusedSGD, FusedAdam -- with one parameter group, per-view host
        # lists not wanted: Solver._graphed_step; DATA.noise replays too, its row is an addend of the loss kernels; rounds 1-3 replayed
        # launch-bound shapes only); False = always issue eagerly; True = as auto
        "graph": None,
        # global gradient-norm clipping on the device (ops.grad_clip: torch.nn.utils.clip_grad_norm_ semantics on the mean gradient,
        # in the eager and the graphed step): 0 = off (no launch, no allocation); inf = measure and report the norm, never scale;
        # a step whose norm is not finite is skipped
        "clip_grad_norm": 0.0,
        # weight decay inside the one update launch (nef_update), with torch's semantics per optimiser: 'sgd' and 'adam' give L2 decay
        # (weight_decay * p is added to the gradient, behind the clipping), 'adamw' gives decoupled decay (p *= 1 - lr * weight_decay in
        # front of Adam's update).  0 = off: the optimisers issue the launches they issued before the key existed
        "weight_decay": 0.0,
        # 'sgd' only: Nesterov momentum (torch.optim.SGD(nesterov=True))
        "nesterov": False,
        # fnmatch patterns on the state_dict keys of the parameters that are EXEMPT from weight_decay, e.g. ['*.bias', '*.double_conv.[14].*']
        # for the biases and the BatchNorm affine parameters; the exemption is a per-run multiplier inside the one flat launch, not a
        # second parameter group (the graphed step and the clipping take one group)
        "no_decay": [],
        # an exponential moving average (EMA) of the weights, kept inside the one update launch (nef_update_ema) of the eager and the
        # graphed step: e += (1 - ema_decay) * (p - e) after every update that is not skipped, e starting as a copy of the weights;
        # BatchNorm statistics stay the live ones.  0 = off: no buffer, no 'ema' checkpoint entry, the launches issued before the key existed
        "ema_decay": 0.0,
        # the decay of EMA update t (counted from 0) is min(ema_decay, (1 + t) / (10 + t)): the average forgets its start quickly
        "ema_warmup": False,
        # with ema_decay > 0: the per-epoch test phase (psnr_gen, best_valid) and Solver.val run on the averaged weights
        "ema_eval": True,
        # optim 'lars' / 'lamb': layer-wise trust ratios inside the update (nef_update_trust; one norm pair per parameter tensor).
        # 'lars' multiplies every tensor's decayed gradient by trust_coef * ||p|| / (||g|| + weight_decay * ||p|| + trust_eps) in front of
        # the momentum; 'lamb' scales Adam's direction u by ||p|| / ||u|| and uses neither number
        "trust_coef": 1e-3,
        "trust_eps": 1e-8,
        # fnmatch patterns on the state_dict keys of the parameters whose trust ratio stays 1 (they step at the plain learning rate),
        # e.g. ['*.bias', '*.double_conv.[14].*'] for the biases and the BatchNorm affine parameters
        "trust_exempt": [],
        # gradient accumulation on the device: an update every accum_steps train batches (micro-batches).  Every micro-batch runs forward,
        # loss and backward as a step does -- its own BatchNorm statistics, Standin draws, dropout seed and loss row -- and its gradients
        # are summed in fp32 into the one flat gradient buffer (nef_flatten_acc); taint word, all-reduce, clipping and the update run once
        # per window on the mean over its micro-batches (and ranks), in the eager and the graphed step.  A window never crosses an epoch:
        # the last, incomplete one is flushed on the micro-batches it has.  1 = off: the launches and graphs are what they were
        "accum_steps": 1,
        # a per-update learning-rate schedule on the device, behind every fused optimiser's update (nef_lr_sched: one single-wave launch,
        # in the eager and the graphed step): the update's rate is group lr -- what the per-epoch `scheduler` sets -- times m(t), t the
        # number of updates APPLIED so far (a skipped step does not count; with accum_steps, updates, not micro-batches).
        # t < warmup_updates: m = warmup_start + (1 - warmup_start) * t / warmup_updates (torch's LinearLR).  Behind it, with
        # x = clamp((t - warmup_updates) / max(1, total_updates - warmup_updates), 0, 1), lr_shape 'const': m = 1; 'cosine':
        # m = lr_floor + (1 - lr_floor) * (1 + cos(pi * x)) / 2 (CosineAnnealingLR); 'poly': m = lr_floor + (1 - lr_floor) * (1 - x)^poly_power
        # (PolynomialLR at lr_floor 0); 'none' with a warm-up behaves as 'const'.  warmup_updates 0 and lr_shape 'none' = off: no device
        # word, no launch, the scheduler object and the bits are what they were before the keys existed
        "warmup_updates": 0,
        "warmup_start": 0.01,       # in [0, 1]
        "lr_shape": "none",         # 'none', 'const', 'cosine' or 'poly'
        # the update at which the shape reaches its end value (kept from there on); 0 = Solver.train derives it before the first step as
        # epochs * ceil(len(dl_train) / accum_steps)
        "total_updates": 0,
        "lr_floor": 0.0,            # in [0, 1]: the end value as a fraction of group lr
        "poly_power": 1.0,          # > 0
        # a structural-similarity term in the training loss, on the device (nef_loss_ssim_fwd / nef_loss_ssim_bwd behind the loss launches,
        # in the eager and the graphed step): loss += ssim_factor * (1 - mean SSIM(prediction (+ DATA.noise), target)) with the SSIM the test
        # phase reports as ssim_gen (7-tap window, utils/metric.py:ssim_1d); the loss tuple and the graphed step's loss row gain the term as
        # their LAST element, logged as train_loss_ssim / test_loss_ssim.  0 = off: the 4-element rows, launches, graphs and bits are what
        # they were before the key existed; a negative value is rejected where the loss is built
        "ssim_factor": 0.0,
        # True: every row ends at rois[i, -1, 0] as in the test phase's metrics (a row shorter than the window is left out); False: whole rows
        "ssim_crop": True,
        # target views supervised per train step.  The batch carries every lead that is not an input (rest_view / rest_theta, supervised
        # ones first); with train_views = Q >= 2 a step draws Q of the S supervised ones -- one draw per step from (seed, epoch, batch
        # index), shared by the batch and the ranks; Q == S takes all in order -- runs the encoder ONCE and the head (mlp2, Standin mixes,
        # three decoder passes) once per view, each with its own BatchNorm batch statistics, and minimises the mean of the Q per-view
        # losses: the gradient is the mean of Q single-view steps at one dropout seed and Standin draw.  target_view / target_theta are not
        # used then; the loss row keeps its elements (each the mean over views).  Q > S and DATA.noise with Q >= 2 are rejected.
        # 1 = off: the launches, graphs, loader fields and bits are what they were before the key existed
        "train_views": 1,
        # weights of the reconstruction term by wave segment, on the device (nef_loss_seg_fwd / nef_loss_seg_bwd behind the loss launches, in
        # the eager and the graphed step): [P, PR, QRS, ST, T, TP, pad] -- seven finite numbers >= 0, not all zero.  Term 3 becomes
        # f2 * (1/n) * sum w[segment of (i, t)] * e(i, t) over ALL n elements (no renormalisation: 3 counts a position three times, all ones
        # is the flat mean, pad = 0 takes the zero padding out).  The segment of a position comes from the batch's rois: t >= rois[i, 6, 0]
        # is pad, otherwise the number of k in 1..5 with rois[i, k, 0] <= t.  Needs 3 in loss_using.  [] = off: the launches, graphs, loss
        # rows and bits are what they were before the key existed
        "seg_weights": [],
        # True: the test phase also reports the PSNR of each wave segment (nef_view_seg_metrics beside nef_view_metrics), logged as
        # psnr_gen_seg_{P,PR,QRS,ST,T,TP} / psnr_reg_seg_* with the view split of psnr_gen / psnr_reg.  False: no launch, no buffer
        "seg_eval": False,
        # a slope (first-difference) term in the training loss, on the device (nef_loss_slope_fwd / nef_loss_slope_bwd behind the loss, segment
        # and SSIM launches, in the eager and the graphed step): loss += slope_factor * mean over rows of the row's mean |d| (or d^2),
        # d = (x[t + 1] - x[t]) - (y[t + 1] - y[t]) at x = prediction (+ DATA.noise), y = target; the loss tuple and the graphed step's loss
        # row gain the term as their LAST element (behind the SSIM term when both are on), logged as train_loss_slope / test_loss_slope.
        # Independent of seg_weights, loss_using and loss_factor.  0 = off: the rows, launches, graphs and bits are what they were before the
        # key existed; a negative value is rejected where the loss is built
        "slope_factor": 0.0,
        # 'l1_loss': |d|, 'l2_loss': d^2; anything else is rejected where the loss is built
        "slope_loss": "l1_loss",
        # True: every row ends at rois[i, -1, 0] as in the test phase's metrics (a row with fewer than 2 samples is left out); False: whole rows
        "slope_crop": True,
        # True: the test phase also reports the PSNR of the first differences (nef_view_slope_metrics beside nef_view_metrics), logged as
        # psnr_slope_gen / psnr_slope_reg with the view split of psnr_gen / psnr_reg; best_valid stays on psnr_gen.  False: no launch, no buffer
        "slope_eval": False,
        # a correlation term in the training loss, on the device (nef_loss_corr_fwd / nef_loss_corr_bwd behind the loss, segment, SSIM and slope
        # launches, in the eager and the graphed step): loss += corr_factor * mean over rows of 1 - r_i, r_i the Pearson correlation coefficient
        # of the row's prediction (+ DATA.noise) and target -- no gain and no baseline offset of the prediction changes it; the loss tuple and
        # the graphed step's loss row gain the term as their LAST element (behind the SSIM and slope terms), logged as train_loss_corr /
        # test_loss_corr.  Independent of seg_weights, loss_using and loss_factor.  0 = off: the rows, launches, graphs and bits are what they
        # were before the key existed; a negative value is rejected where the loss is built
        "corr_factor": 0.0,
        # True: every row ends at rois[i, -1, 0] as in the test phase's metrics (a row with fewer than 2 samples is left out); False: whole rows
        "corr_crop": True,
        # r_i = (c + eps) / sqrt((vx + eps) (vy + eps)): keeps a constant row finite (two constant rows give exactly 1); > 0 and finite
        "corr_eps": 1e-8,
        # True: the test phase also reports the mean correlation coefficient (nef_view_corr_metrics beside nef_view_metrics), logged as
        # corr_gen / corr_reg with the view split of psnr_gen / psnr_reg; best_valid stays on psnr_gen.  False: no launch, no buffer
        "corr_eval": False,
        # True: Solver.val also locates every rest view of every test batch from the batch's input leads (Solver.locate: one encoder pass and
        # one level-0 panorama per batch, scored against all rest views on the device, then coarse-to-fine refinement) and prints the mean and
        # median angular error in degrees and the share of views found within one level-0 step on both axes -- locate_err1_gen /
        # locate_err2_gen / locate_hit_gen and the _reg forms, with the view split of psnr_gen / psnr_reg; best_valid and every other number
        # keep their bits.  One rank only.  False: no launch, no buffer, the keys below are not looked at
        "locate_eval": False,
        # level 0: locate_grid[0] x locate_grid[1] angles over locate_range_deg (degrees; the default is the span of the nominal lead table,
        # in steps of 15 and 10 degrees); an axis with one point is pinned at the range's start
        "locate_grid": [9, 19],
        "locate_range_deg": [[60, 180], [-90, 90]],
        # 'corr': 1 - the correlation coefficient (eps: corr_eps) -- no gain or offset of the located lead changes it; 'mse'
        "locate_score": "corr",
        # refinement levels behind level 0, each (2 locate_radius + 1)^2 candidates around the running best at half the previous step
        "locate_levels": 3,
        "locate_radius": 2,
    },
}


def get_defaults():
    """A fresh, mutable copy of the default tree."""
    return CfgNode(_DEFAULTS).clone()


cfg = get_defaults()
