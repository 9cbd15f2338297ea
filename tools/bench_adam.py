"""Adam against SGD on the train step of BASELINE config 2 (B=256, 3 leads, L=5000), one GPU; prints one JSON line.

    python tools/bench_adam.py [--steps 10] [--warmup 3] [--reps 3] [--out profiles/adam_bench_line.json]
    python tools/bench_adam.py --clip MAX_NORM [--parent-tree DIR] [--out profiles/clip_bench_line.json]
    python tools/bench_adam.py --weight-decay X [--no-decay PATTERN...] [--parent-tree DIR] [--out profiles/wd_bench_line.json]
    python tools/bench_adam.py --ema D [--parent-tree DIR] [--out profiles/ema_bench_line.json]
    python tools/bench_adam.py --trust lars|lamb [--parent-tree DIR] [--out profiles/r11_trust_bench_line.json]
    python tools/bench_adam.py --accum K [--parent-tree DIR] [--out profiles/r12_accum_bench_line.json]
    python tools/bench_adam.py --sched const|cosine|poly --warmup W [--parent-tree DIR] [--out profiles/r14_sched_bench_line.json]
    python tools/bench_adam.py --ssim F [--parent-tree DIR] [--out profiles/r15_ssim_bench_line.json]
    python tools/bench_adam.py --views Q [Q ...] [--parent-tree DIR] [--out profiles/r16_views_bench_line.json]
    python tools/bench_adam.py --augment [--parent-tree DIR] [--out profiles/r17_augment_bench_line.json]
    python tools/bench_adam.py --augment --lead-mask [--parent-tree DIR] [--out profiles/r28_lead_mask_bench_line.json]
    python tools/bench_adam.py --seg W0 W1 W2 W3 W4 W5 W6 [--parent-tree DIR] [--out profiles/r18_seg_bench_line.json]
    python tools/bench_adam.py --slope F [--parent-tree DIR] [--out profiles/r19_slope_bench_line.json]
    python tools/bench_adam.py --corr F [--parent-tree DIR] [--out profiles/r20_corr_bench_line.json]
    python tools/bench_adam.py --warp A0 A1 A2 A3 A4 A5 [--roi-jitter J] [--parent-tree DIR] [--out profiles/r25_warp_bench_line.json]
    python tools/bench_adam.py --device-noise [--parent-tree DIR] [--out profiles/r30_device_noise_bench_line.json]

Each measurement runs in a child process of its own under `timeout` (nothing more is started once one fails), `--reps` rounds of
the three children; every figure is reported as [min, median, max] over the rounds:
  sgd-graph   the graphed step (GraphedTrainStep) with FusedSGD -- what bench.py times;
  adam-graph  the graphed step with FusedAdam, then the nef_adam launch alone on the same flat buffers, COLD: before every timed
              launch a 512 MiB scratch buffer (twice the 256 MiB Infinity Cache) is written, as the backward pass in front of the
              update does in the train step; HIP events around each launch, median of 30 (seven fp32 streams per parameter = the
              algorithmic bytes).  The warm figure (50 back-to-back launches, the 115 MB working set cache-resident) is listed too;
  adam-eager  the eager step with DataParallelAdam (torch.optim.Adam: ATen kernels, no graph) -- the path 'adam' took before.
Every child warms up before it times.

--clip MAX_NORM measures gradient-norm clipping instead: per round the graphed FusedSGD step with clipping off (sgd-graph) and with
max_grad_norm = MAX_NORM (sgd-graph-clip: also the three nef_grad_clip launches alone on the flat gradient buffer, cold as above, with
a max_norm that clips), and -- with --parent-tree DIR -- the sgd-graph child of DIR/tools/bench_adam.py, in the same rounds on the same
device.  DIR is a checkout of the commit to compare against; its library must already be built (nothing is built here) and its
tools/bench_adam.py must accept `--child sgd-graph --steps N --warmup W`.

--weight-decay X measures weight decay inside the update launch (nef_update): per round the graphed step with FusedSGD and FusedAdam as
they are without decay (sgd-graph, adam-graph), with FusedSGD(weight_decay=X, no_decay=PATTERNS) (sgd-graph-wd) and with
FusedAdamW(weight_decay=X, no_decay=PATTERNS) (adamw-graph), and -- with --parent-tree DIR -- DIR's own sgd-graph child.  The two decay
children also time their update launch alone on the flat buffers with the model's real run table, cold as above and alternating with
the entry it stands beside (nef_sgd_momentum, nef_adam) in the same process: same bytes, the table lookup on top.

--ema D measures the EMA of the weights inside the update launch (nef_update_ema), at config 2 AND at the reference's own training shape
(B=32, L=512): per round and shape the graphed FusedSGD step with the average off (sgd-graph) and with ema_decay = D (sgd-graph-ema), and
-- with --parent-tree DIR -- DIR's own sgd-graph step at that shape (DIR/tools/bench_adam.py's `child` function, called in a fresh
process).  The config-2 EMA child also times the update launch alone on the flat buffers, cold as above: nef_update_ema beside nef_update
in one process (rule 0, no table: five fp32 streams per parameter against seven).

--trust lars|lamb measures the layer-wise trust ratios (nef_update_trust), at the same two shapes: per round and shape the graphed step with
FusedSGD / FusedAdam (sgd-graph for lars, adam-graph for lamb), the graphed step with FusedLARS / FusedLAMB (lars-graph / lamb-graph: one
segment per live tensor, nothing exempt), and -- with --parent-tree DIR -- DIR's own sgd-graph / adam-graph step.  The config-2 trust child
also times the entry's launches alone on the flat buffers with the model's real segment table, cold as above, beside nef_update (same rule,
no table) in one process.  Writes profiles/r11_trust_bench_line.json unless --out says otherwise.

--accum K measures gradient accumulation (SOLVER.accum_steps), at the same two shapes: per round and shape the graphed FusedSGD step with
accum_steps = 1 (sgd-graph: the parent's code path) and with accum_steps = K (sgd-graph-accum: ms per MICRO-batch, an update every K-th),
and -- with --parent-tree DIR -- DIR's own sgd-graph step.  The config-2 accumulating child also times the flatten launch alone on the
model's real gradient tensors, cold as above: nef_flatten_acc (accumulate form) beside nef_flatten in one process (3 fp32 streams per
parameter against 2).  Writes profiles/r12_accum_bench_line.json unless --out says otherwise.

--sched SHAPE --warmup W measures the per-update learning-rate schedule (SOLVER.warmup_updates / lr_shape), at the same two shapes: per
round and shape the graphed FusedSGD step with the keys off (sgd-graph: the parent's code path) and with the schedule on (sgd-graph-sched:
warmup_updates = W, lr_shape = SHAPE, total_updates = W + 1000, so the timed steps sit on the ramp or the shape), and -- with --parent-tree
DIR -- DIR's own sgd-graph step.  Beside --sched, --warmup is the SCHEDULE's W; every child then runs 3 untimed steps in front of the
timed ones (the default of the other measurements).  The config-2 schedule child also times the nef_lr_sched launch alone: cold as above
and warm (back-to-back launches).  Writes profiles/r14_sched_bench_line.json unless --out says otherwise.

--ssim F measures the SSIM term of the training loss (SOLVER.ssim_factor = F, ssim_crop true), at the same two shapes: per round and
shape the graphed FusedSGD step with the key off (sgd-graph: the parent's code path) and on (sgd-graph-ssim), and -- with --parent-tree
DIR -- DIR's own sgd-graph step.  The config-2 child with the term on also times the term's launches alone, cold: nef_loss_ssim_fwd
(two launches) and nef_loss_ssim_bwd.  Writes profiles/r15_ssim_bench_line.json unless --out says otherwise.

--views Q [Q ...] measures several target views per train step (SOLVER.train_views), at the same two shapes: per round and shape the graphed
FusedSGD step with the key off (sgd-graph: the parent's code path) and one child per Q (sgd-graph-views: query_theta [Q, B, 2], targets
[Q, B, 1, L]; ms per step, and per supervised view = step / Q, beside the FLOP model 1 + 0.31 (Q - 1) steps), and -- with --parent-tree DIR
-- DIR's own sgd-graph step.  Every child reports torch.cuda.max_memory_allocated; the config-2 views children also time the step's four
nef_copy_many launches alone, cold: the outputs into the loss's layout, the loss gradient back out, one view's latent gradients and one view's
head parameter gradients summed into the first view's.  Writes profiles/r16_views_bench_line.json unless --out says otherwise.

--augment measures the input-lead augmentation of the train step (DATA.aug_*), at the same two shapes: per round and shape the graphed
FusedSGD step with the keys off (sgd-graph: the parent's code path) and with all four corruptions on (sgd-graph-augment: aug_noise_std 0.05,
aug_wander_amp 0.2, aug_hum_amp 0.1, aug_lead_drop 0.1, aug_crop true), and -- with --parent-tree DIR -- DIR's own sgd-graph step.  The
config-2 child with the keys on also times the nef_augment launch alone on the batch's inputs and rois, cold.  Writes
profiles/r17_augment_bench_line.json unless --out says otherwise.

--augment --lead-mask adds the masked head (MODEL.lead_mask, which needs --augment's aug_lead_drop) as a third child per round and shape
(sgd-graph-lead-mask: the same four corruptions, the head over the present leads on the un-fused three-pass route).  The config-2 child
with the key on also times the two mix entries alone, cold, beside the launches they stand in for: nef_lead_mask_mix_fwd against
nef_lead_mean + nef_mix_fwd, nef_lead_mask_mix_bwd against nef_mix_bwd (three passes, gradient at the latent's resolution).  Writes
profiles/r28_lead_mask_bench_line.json unless --out says otherwise.

--seg W0 .. W6 measures the wave-segment weights of the reconstruction term (SOLVER.seg_weights = [P, PR, QRS, ST, T, TP, pad]), at the
same two shapes: per round and shape the graphed FusedSGD step with the key off (sgd-graph: the parent's code path) and on (sgd-graph-seg),
and -- with --parent-tree DIR -- DIR's own sgd-graph step.  The config-2 child with the key on also times the three new entries alone,
cold: nef_loss_seg_fwd and nef_loss_seg_bwd on the batch's prediction-sized tensors and rois, nef_view_seg_metrics on [B, 9, L] rows.
Writes profiles/r18_seg_bench_line.json unless --out says otherwise.

--slope F measures the slope term of the training loss (SOLVER.slope_factor = F, slope_loss l1_loss, slope_crop true), at the same two
shapes: per round and shape the graphed FusedSGD step with the key off (sgd-graph: the parent's code path) and on (sgd-graph-slope), and
-- with --parent-tree DIR -- DIR's own sgd-graph step.  The config-2 child with the term on also times the three entries alone, cold:
nef_loss_slope_fwd (two launches) and nef_loss_slope_bwd on the batch's prediction-sized tensors and rois, nef_view_slope_metrics on
[B, 9, L] rows.  Writes profiles/r19_slope_bench_line.json unless --out says otherwise.

--corr F measures the correlation term of the training loss (SOLVER.corr_factor = F, corr_crop true, corr_eps at its default), at the same
two shapes: per round and shape the graphed FusedSGD step with the key off (sgd-graph: the parent's code path) and on (sgd-graph-corr), and
-- with --parent-tree DIR -- DIR's own sgd-graph step.  The config-2 child with the term on also times the three entries alone, cold:
nef_loss_corr_fwd (two launches) and nef_loss_corr_bwd (three) on the batch's prediction-sized tensors and rois, nef_view_corr_metrics on
[B, 9, L] rows.  Writes profiles/r20_corr_bench_line.json unless --out says otherwise.

--warp A0 .. A5 [--roi-jitter J] measures the time warp of the train batch (DATA.aug_warp = [P, PR, QRS, ST, T, TP], DATA.aug_roi_jitter =
J), at the same two shapes: per round and shape the graphed FusedSGD step with the keys off (sgd-graph: the parent's code path) and on
(sgd-graph-warp: one nef_warp launch on the stream in front of every replay, into fresh tensors, as Solver.run_one_epoch places it), and --
with --parent-tree DIR -- DIR's own sgd-graph step.  The config-2 child with the keys on also times the nef_warp launch alone on the batch's
inputs, target and rois, cold.  Writes profiles/r25_warp_bench_line.json unless --out says otherwise.

--device-noise measures the train step's own noise row (DATA.device_noise), at the same two shapes: per round and shape the graphed FusedSGD
step with the keys off (sgd-graph: the parent's code path) and with the key on (sgd-graph-device-noise: one captured nef_noise_row launch in
front of the loss launches, the loss kernels with the addend), and -- with --parent-tree DIR -- DIR's own sgd-graph step and DIR's graphed
step with DATA.noise on and a host row staged per step (sgd-graph-noise, this tool's child importing DIR's package: the like-for-like step the
key-on step is compared with).  The config-2 child with the key on also times the nef_noise_row launch alone on the batch's target and
rois, cold, beside its bytes (the quiet segments read, the row written).  Writes profiles/r30_device_noise_bench_line.json unless --out
says otherwise."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"sgd-graph": 900, "adam-graph": 900, "adam-eager": 1200}      # child -> its time limit (s)
CLIP_MODES = {"sgd-graph": 900, "sgd-graph-clip": 900}
WD_MODES = {"sgd-graph": 900, "sgd-graph-wd": 900, "adam-graph": 900, "adamw-graph": 900}
EMA_MODES = {"sgd-graph": 900, "sgd-graph-ema": 900}
TRUST_BASE = {"lars": "sgd-graph", "lamb": "adam-graph"}
EMA_SHAPES = {"config2": (256, 5000), "reference": (32, 512)}      # (B, L) at 3 leads
ONES7 = (1.0,) * 7      # the cold timing of nef_loss_seg_bwd scales its buffer in place: by 1, so that 30 calls leave it as it was
AUGMENT_KEYS = {"aug_noise_std": 0.05, "aug_wander_amp": 0.2, "aug_hum_amp": 0.1, "aug_lead_drop": 0.1, "aug_crop": True}


def cold_ms(launches, dev, reps=30):
    """Median device time (ms) of each callable in `launches`, cold: a 512 MiB buffer is written before every timed call, and the
    callables take turns so that none of them always meets the same cache state."""
    import numpy as np
    import torch
    flush = torch.empty(512 << 18, device=dev, dtype=torch.float32)        # 512 MiB
    for fn in launches:
        fn()
    evs = [[] for _ in launches]
    for i in range(reps):
        for k, fn in enumerate(launches):
            flush.fill_(float(i))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize(dev)
    return [float(np.median([a.elapsed_time(b) for a, b in ev])) for ev in evs]


def child(mode, steps, warmup, V=3, B=256, L=5000, clip=0.0, wd=0.0, no_decay=(), ema=0.0, accum=1, sched=None, ssim=0.0, views=1,
          seg=None, slope=0.0, corr=0.0, warp=None, roi_jitter=0):
    import numpy as np
    import torch
    from electrocardio_panorama_amd import ops, synth
    from electrocardio_panorama_amd.config import get_defaults, resolve_config_path
    from electrocardio_panorama_amd.network import build_loss, build_model
    from electrocardio_panorama_amd.solver.optim_scheduler import DataParallelAdam, FusedAdam, FusedSGD
    from electrocardio_panorama_amd.solver import optim_scheduler
    from electrocardio_panorama_amd.utils import seed_torch
    cfg = get_defaults()
    cfg.merge_from_file(resolve_config_path("config/nef_net.yml"))
    cfg.DATA.lead_num = V
    if mode == "sgd-graph-ssim":
        cfg.SOLVER.ssim_factor, cfg.SOLVER.ssim_crop = float(ssim), True
    if mode in ("sgd-graph-augment", "sgd-graph-lead-mask"):
        for k, v in AUGMENT_KEYS.items():
            cfg.DATA[k] = v
    if mode == "sgd-graph-lead-mask":
        cfg.MODEL.lead_mask = True
    if mode == "sgd-graph-seg":
        cfg.SOLVER.seg_weights = [float(w) for w in seg]
    if mode == "sgd-graph-warp":
        cfg.DATA.aug_warp, cfg.DATA.aug_roi_jitter = [float(a) for a in warp], int(roi_jitter)
    if mode == "sgd-graph-noise":
        cfg.DATA.noise = True
    if mode == "sgd-graph-device-noise":
        cfg.DATA.device_noise = True
    if mode == "sgd-graph-slope":
        cfg.SOLVER.slope_factor, cfg.SOLVER.slope_loss, cfg.SOLVER.slope_crop = float(slope), "l1_loss", True
    if mode == "sgd-graph-corr":
        cfg.SOLVER.corr_factor, cfg.SOLVER.corr_crop = float(corr), True
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    seed_torch(cfg.seed)
    model = build_model(cfg).float().to(dev).train()
    lossf = build_loss(cfg)
    if mode in ("sgd-graph", "sgd-graph-ssim", "sgd-graph-views", "sgd-graph-augment", "sgd-graph-seg", "sgd-graph-slope", "sgd-graph-corr",
                "sgd-graph-warp", "sgd-graph-lead-mask", "sgd-graph-noise", "sgd-graph-device-noise"):
        optim = FusedSGD(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9)
    elif mode == "sgd-graph-clip":
        optim = FusedSGD(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9, max_grad_norm=clip)
    elif mode == "sgd-graph-wd":
        optim = FusedSGD(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9, weight_decay=wd, no_decay=no_decay)
    elif mode == "sgd-graph-ema":
        optim = FusedSGD(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9, ema_decay=ema)
    elif mode == "sgd-graph-accum":
        optim = FusedSGD(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9, accum_steps=accum)
    elif mode == "sgd-graph-sched":
        shape, W = sched
        optim = FusedSGD(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9,
                         lr_schedule=optim_scheduler.LrSchedule(warmup_updates=W, lr_shape=shape, total_updates=W + 1000))
    elif mode == "adam-graph":
        optim = FusedAdam(model.parameters(), lr=1e-3)
    elif mode == "lars-graph":
        optim = optim_scheduler.FusedLARS(model.parameters(), lr=cfg.SOLVER.lr, momentum=0.9)
    elif mode == "lamb-graph":
        optim = optim_scheduler.FusedLAMB(model.parameters(), lr=1e-3)
    elif mode == "adamw-graph":
        optim = optim_scheduler.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=wd, no_decay=no_decay)
    else:
        optim = DataParallelAdam(model.parameters(), lr=1e-3)
    meta = synth.make_batch(B, V, L, seed=123)
    data, rois, in_theta, tgt_view, tgt_theta = (torch.from_numpy(np.ascontiguousarray(meta[k])).to(dev) for k in
                                                 ("data", "rois", "input_theta", "target_view", "target_theta"))
    tgt_view = tgt_view.unsqueeze(1)
    if mode == "sgd-graph-views":
        # SOLVER.train_views = Q: the step's targets are Q rest views of the batch -- [Q, B, 1, L] and [Q, B, 2], view-major
        from electrocardio_panorama_amd.views import select_views
        meta = synth.make_batch(B, V, L, seed=123, Q=views)
        data, rois, in_theta, rest_view, rest_theta = (torch.from_numpy(np.ascontiguousarray(meta[k])).to(dev) for k in
                                                       ("data", "rois", "input_theta", "rest_view", "rest_theta"))
        tgt_view, tgt_theta = select_views(rest_view, rest_theta, list(range(views)))
    graphed = None
    if "-graph" in mode:
        from electrocardio_panorama_amd.graph import GraphedTrainStep
        graphed = GraphedTrainStep(model, cfg, optimizer=optim)

    warp_cfg, warped = None, []
    if mode == "sgd-graph-warp":
        # DATA.aug_warp / aug_roi_jitter as Solver.run_one_epoch places it: one launch on the stream into fresh tensors in front of the
        # replayed step, batch i under warp.train_seed(seed, 0, i, 0)
        from electrocardio_panorama_amd import warp as _warp
        warp_cfg = _warp.from_cfg(cfg)
        assert warp_cfg is not None

    # DATA.noise: a host row per sample as the loaders make it (sigma 0.01 in front of the row end, zeros behind it)
    host_noise = None
    if mode == "sgd-graph-noise":
        live = torch.arange(L, device=dev)[None, :] < rois[:, 6, 0].clamp(0, L)[:, None]
        host_noise = (0.01 * torch.randn(B, L, device=dev) * live).unsqueeze(1).contiguous()

    def step():
        if warp_cfg is not None:
            d, t, _, r = ops.warp(data, tgt_view, None, rois, warp_cfg, _warp.train_seed(cfg.seed, 0, len(warped), 0))
            warped.append((d, r) if not warped else None)      # (the first step's, for the result line)
            return graphed(d, in_theta, tgt_theta, r, t)
        if host_noise is not None:       # DATA.noise: the loader's row, staged with the other inputs
            return graphed(data, in_theta, tgt_theta, rois, tgt_view, noise=host_noise)
        if graphed is not None:
            return graphed(data, in_theta, tgt_theta, rois, tgt_view)
        out, sp, sl = model(data, in_theta, tgt_theta, rois, phase="train")
        losses = lossf(out, sp, sl, tgt_view, cfg)
        losses[0].backward()
        optim.step()
        optim.zero_grad()
        return losses

    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    res = {"mode": mode, "ms_per_step": round((time.perf_counter() - t0) * 1e3 / steps, 3), "steps": steps, "warmup": warmup, "B": B, "L": L,
           "max_memory_allocated_GiB": round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 3)}
    if mode == "sgd-graph-views":
        res.update(train_views=views, ms_per_view=round(res["ms_per_step"] / views, 3),
                   loss_row=[round(float(v), 6) for v in graphed.losses.tolist()])
    if mode == "sgd-graph-views" and (B, L) == EMA_SHAPES["config2"]:
        # the step's nef_copy_many launches alone, cold, on tensors of the step's own sizes
        Q, T = views, L // 4
        out3 = [torch.randn(3 * B, 1, L, device=dev) for _ in range(Q)]
        buf = torch.empty(3, Q, B, 1, L, device=dev)
        scat = ([o[j * B:(j + 1) * B] for o in out3 for j in range(3)], [buf[j, k] for k in range(Q) for j in range(3)])
        lat = [torch.randn(B, 128 * V, T, device=dev), torch.randn(B, 128 * V, 7, 32, device=dev), torch.randn(128 * V, device=dev)]
        lat0 = [torch.zeros_like(t) for t in lat]
        head = [p_ for n_, p_ in model.named_parameters() if n_.startswith(("decoder.", "mlp2."))]
        hg, hg0 = [torch.randn_like(p_) for p_ in head], [torch.zeros_like(p_) for p_ in head]
        ms = cold_ms([lambda: ops.copy_many(scat[0], scat[1]), lambda: ops.copy_many(scat[1], scat[0]),
                      lambda: ops.copy_many(lat, lat0, accumulate=True), lambda: ops.copy_many(hg, hg0, accumulate=True)], dev)
        nb = [2 * 4 * buf.numel(), 2 * 4 * buf.numel(), 3 * 4 * sum(t.numel() for t in lat), 3 * 4 * sum(t.numel() for t in hg)]
        res.update(copy_many_cold_ms=dict(zip(("outputs_to_loss_layout", "loss_gradient_to_views", "latent_gradient_sum", "head_parameter_gradient_sum"),
                                              [round(m_, 4) for m_ in ms])),
                   copy_many_cold_GBps=dict(zip(("outputs_to_loss_layout", "loss_gradient_to_views", "latent_gradient_sum", "head_parameter_gradient_sum"),
                                                [round(b_ / (m_ * 1e-3) / 1e9, 1) for b_, m_ in zip(nb, ms)])),
                   copy_many_head_tensors=len(hg))
    if mode == "sgd-graph-accum":
        graphed.flush()      # (a window the timed micro-batches left open)
        res.update(accum_steps=accum, ms_per_step_note="per micro-batch; an update behind every accum_steps-th")
    if mode == "sgd-graph-accum" and (B, L) == EMA_SHAPES["config2"]:
        fl = optim._flat[0]
        srcs = [torch.randn_like(p_) for p_ in fl["params"]]      # the model's gradient tensors: their sizes and count
        out_, n = torch.zeros_like(fl["g"]), fl["g"].numel()
        old_ms, new_ms = cold_ms([lambda: ops.flatten_into(srcs, out_), lambda: ops.flatten_into(srcs, out_, accumulate=True)], dev)
        res.update(flatten_tensors=len(srcs), flatten_params=n, nef_flatten_cold_ms=round(old_ms, 4), nef_flatten_acc_cold_ms=round(new_ms, 4),
                   nef_flatten_cold_GBps=round(2 * 4 * n / (old_ms * 1e-3) / 1e9, 1),
                   nef_flatten_acc_cold_GBps=round(3 * 4 * n / (new_ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-sched":
        t, lr = optim.lr_state()
        res.update(lr_shape=sched[0], warmup_updates=sched[1], updates_applied=t, effective_lr=lr)
    if mode == "sgd-graph-sched" and (B, L) == EMA_SHAPES["config2"]:
        sc = optim.lr_schedule
        t_w, lr_w = torch.zeros(1, device=dev, dtype=torch.int64), torch.zeros(1, device=dev)
        skip = torch.zeros(1, device=dev)
        launch = lambda: ops.lr_sched(t_w, lr_w, float(cfg.SOLVER.lr), skip=skip, **sc.kwargs())      # noqa: E731
        cold = cold_ms([launch], dev)[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 200
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        e1.synchronize()
        res.update(nef_lr_sched_cold_ms=round(cold, 4), nef_lr_sched_warm_ms=round(e0.elapsed_time(e1) / reps, 4))
    if mode == "sgd-graph-ssim":
        res.update(ssim_factor=ssim, loss_row=[round(float(v), 6) for v in graphed.losses.tolist()])
    if mode == "sgd-graph-ssim" and (B, L) == EMA_SHAPES["config2"]:
        pred, g_pred, row = torch.rand(B, 1, L, device=dev) / 3, torch.zeros(B, 1, L, device=dev), torch.zeros(5, device=dev)
        fwd_ms, bwd_ms = cold_ms([lambda: ops.loss_ssim_fwd(pred, tgt_view, row, ssim, rois=rois),
                                  lambda: ops.loss_ssim_bwd(pred, tgt_view, g_pred, ssim, rois=rois)], dev)
        n = pred.numel()
        res.update(nef_loss_ssim_fwd_cold_ms=round(fwd_ms, 4), nef_loss_ssim_bwd_cold_ms=round(bwd_ms, 4),
                   nef_loss_ssim_bwd_cold_GBps=round(4 * 4 * n / (bwd_ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-augment":
        res.update(augment=dict(AUGMENT_KEYS), loss_row=[round(float(v), 6) for v in graphed.losses.tolist()],
                   input_elements_changed=round(float((graphed.data_aug != graphed.data).float().mean().item()), 4))
    if mode == "sgd-graph-augment" and (B, L) == EMA_SHAPES["config2"]:
        from electrocardio_panorama_amd import augment as _augment
        y = torch.empty_like(data)
        ms = cold_ms([lambda: ops.augment(data, rois, graphed.augment, seed=_augment.train_seed(1), out=y)], dev)[0]
        res.update(nef_augment_cold_ms=round(ms, 4), nef_augment_cold_GBps=round(2 * 4 * data.numel() / (ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-lead-mask":
        res.update(augment=dict(AUGMENT_KEYS), loss_row=[round(float(v), 6) for v in graphed.losses.tolist()],
                   leads_masked=round(float((graphed.lead_mask == 0).float().mean().item()), 4))
    if mode == "sgd-graph-lead-mask" and (B, L) == EMA_SHAPES["config2"]:
        T = L // 4
        z1, z2r = torch.randn(B, 128 * V, T, device=dev), torch.randn(B, 128 * V, T, device=dev)
        q, gD = torch.randn(B, 256, device=dev), torch.randn(3 * B, 256, T, device=dev)
        mask, c = graphed.lead_mask, (1, 2)
        latent = ops.lead_mean(z1, z2r, V)
        ms = cold_ms([lambda: ops.lead_mask_mix_fwd(z1, z2r, mask, q, c),
                      lambda: ops.mix_fwd(ops.lead_mean(z1, z2r, V), z1, z2r, q, V, c),
                      lambda: ops.lead_mask_mix_bwd(gD, latent, z1, z2r, q, mask, c, relu_z1=True),
                      lambda: ops.mix_bwd(gD, latent, z1, z2r, q, V, c, relu_z1=True)], dev)
        res.update(mix_cold_ms=dict(zip(("lead_mask_mix_fwd", "lead_mean_plus_mix_fwd", "lead_mask_mix_bwd", "mix_bwd"), [round(m_, 4) for m_ in ms])))
    if mode == "sgd-graph-warp":
        d0, r0 = warped[0]
        res.update(aug_warp=[float(a) for a in warp], aug_roi_jitter=int(roi_jitter), loss_row=[round(float(v), 6) for v in graphed.losses.tolist()],
                   input_elements_changed=round(float((d0 != data).float().mean().item()), 4),
                   marks_moved=round(float((r0 != rois).float().mean().item()), 4))
    if mode == "sgd-graph-warp" and (B, L) == EMA_SHAPES["config2"]:
        ms = cold_ms([lambda: ops.warp(data, tgt_view, None, rois, warp_cfg, 1)], dev)[0]
        nbytes = 2 * 4 * (data.numel() + tgt_view.numel()) + 2 * 8 * rois.numel()
        res.update(nef_warp_cold_ms=round(ms, 4), nef_warp_bytes=nbytes, nef_warp_cold_GBps=round(nbytes / (ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-noise":
        res.update(loss_row=[round(float(v), 6) for v in graphed.losses.tolist()])
    if mode == "sgd-graph-device-noise":
        res.update(loss_row=[round(float(v), 6) for v in graphed.losses.tolist()],
                   noise_elements_nonzero=round(float((graphed.noise != 0).float().mean().item()), 4),
                   noise_abs_mean=float(graphed.noise.abs().mean().item()))
    if mode == "sgd-graph-device-noise" and (B, L) == EMA_SHAPES["config2"]:
        from electrocardio_panorama_amd import device_noise as _dn
        t_rows, r_rows = _dn.rows(tgt_view, rois)
        y = torch.empty_like(t_rows)
        ms = cold_ms([lambda: ops.noise_row(t_rows, r_rows, _dn.train_seed(1), out=y)], dev)[0]
        end = r_rows[:, 6, 0].clamp(0, L)
        q0 = torch.div(r_rows[:, 5, 0] + r_rows[:, 5, 1], 2, rounding_mode="floor").clamp(min=0)
        seg = (torch.minimum(r_rows[:, 5, 1].clamp(min=0), end) - torch.minimum(q0, end)).clamp(min=0)
        nbytes = 4 * y.numel() + 2 * 4 * int(seg.sum().item()) + 8 * r_rows.numel()      # the row written, the segments read twice, the rois
        res.update(nef_noise_row_cold_ms=round(ms, 4), nef_noise_row_bytes=nbytes, nef_noise_row_cold_GBps=round(nbytes / (ms * 1e-3) / 1e9, 1),
                   nef_noise_row_segment_elements=int(seg.sum().item()))
    if mode == "sgd-graph-seg":
        res.update(seg_weights=[float(w) for w in seg], loss_row=[round(float(v), 6) for v in graphed.losses.tolist()])
    if mode == "sgd-graph-seg" and (B, L) == EMA_SHAPES["config2"]:
        Qm = 9
        pred, g_pred, row = torch.rand(B, 1, L, device=dev) / 3, torch.rand(B, 1, L, device=dev), torch.zeros(4, device=dev)
        xs, ys = torch.rand(B, Qm, L, device=dev) / 3, torch.rand(B, Qm, L, device=dev) / 3
        fwd_ms, bwd_ms, met_ms = cold_ms([lambda: ops.loss_seg_fwd(pred, tgt_view, row, seg, 1.0, False, rois),
                                          lambda: ops.loss_seg_bwd(g_pred, ONES7, rois),
                                          lambda: ops.view_seg_metrics(xs, ys, rois)], dev)
        n = pred.numel()
        res.update(nef_loss_seg_fwd_cold_ms=round(fwd_ms, 4), nef_loss_seg_bwd_cold_ms=round(bwd_ms, 4),
                   nef_view_seg_metrics_cold_ms=round(met_ms, 4),
                   nef_loss_seg_fwd_cold_GBps=round(2 * 4 * n / (fwd_ms * 1e-3) / 1e9, 1),
                   nef_loss_seg_bwd_cold_GBps=round(2 * 4 * n / (bwd_ms * 1e-3) / 1e9, 1),
                   nef_view_seg_metrics_cold_GBps=round(2 * 4 * xs.numel() / (met_ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-slope":
        res.update(slope_factor=slope, loss_row=[round(float(v), 6) for v in graphed.losses.tolist()])
    if mode == "sgd-graph-slope" and (B, L) == EMA_SHAPES["config2"]:
        Qm = 9
        pred, g_pred, row = torch.rand(B, 1, L, device=dev) / 3, torch.zeros(B, 1, L, device=dev), torch.zeros(5, device=dev)
        xs, ys = torch.rand(B, Qm, L, device=dev) / 3, torch.rand(B, Qm, L, device=dev) / 3
        fwd_ms, bwd_ms, met_ms = cold_ms([lambda: ops.loss_slope_fwd(pred, tgt_view, row, slope, False, rois=rois),
                                          lambda: ops.loss_slope_bwd(pred, tgt_view, g_pred, slope, False, rois=rois),
                                          lambda: ops.view_slope_metrics(xs, ys, rois)], dev)
        n = pred.numel()
        res.update(nef_loss_slope_fwd_cold_ms=round(fwd_ms, 4), nef_loss_slope_bwd_cold_ms=round(bwd_ms, 4),
                   nef_view_slope_metrics_cold_ms=round(met_ms, 4),
                   nef_loss_slope_fwd_cold_GBps=round(2 * 4 * n / (fwd_ms * 1e-3) / 1e9, 1),
                   nef_loss_slope_bwd_cold_GBps=round(4 * 4 * n / (bwd_ms * 1e-3) / 1e9, 1),
                   nef_view_slope_metrics_cold_GBps=round(2 * 4 * xs.numel() / (met_ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-corr":
        res.update(corr_factor=corr, loss_row=[round(float(v), 6) for v in graphed.losses.tolist()])
    if mode == "sgd-graph-corr" and (B, L) == EMA_SHAPES["config2"]:
        Qm = 9
        eps = float(cfg.SOLVER.corr_eps)
        pred, g_pred, row = torch.rand(B, 1, L, device=dev) / 3, torch.zeros(B, 1, L, device=dev), torch.zeros(5, device=dev)
        xs, ys = torch.rand(B, Qm, L, device=dev) / 3, torch.rand(B, Qm, L, device=dev) / 3
        fwd_ms, bwd_ms, met_ms = cold_ms([lambda: ops.loss_corr_fwd(pred, tgt_view, row, corr, eps, rois=rois),
                                          lambda: ops.loss_corr_bwd(pred, tgt_view, g_pred, corr, eps, rois=rois),
                                          lambda: ops.view_corr_metrics(xs, ys, rois)], dev)
        n = pred.numel()
        res.update(nef_loss_corr_fwd_cold_ms=round(fwd_ms, 4), nef_loss_corr_bwd_cold_ms=round(bwd_ms, 4),
                   nef_view_corr_metrics_cold_ms=round(met_ms, 4),
                   nef_loss_corr_fwd_cold_GBps=round(2 * 4 * n / (fwd_ms * 1e-3) / 1e9, 1),
                   nef_loss_corr_bwd_cold_GBps=round(6 * 4 * n / (bwd_ms * 1e-3) / 1e9, 1),
                   nef_view_corr_metrics_cold_GBps=round(2 * 4 * xs.numel() / (met_ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-ema":
        fl = optim._flat[0]
        p, g, buf, e, e_n = (fl[k].clone() for k in ("p", "g", "buf", "ema", "ema_n"))
        n = p.numel()
        old_ms, new_ms = cold_ms([lambda: ops.update_sgd(p, g, buf, 0.1, 0.9, 1.0),
                                  lambda: ops.update_sgd(p, g, buf, 0.1, 0.9, 1.0, ema=(e, e_n, ema, False))], dev)
        res.update(ema_decay=ema, ema_updates=float(fl["ema_n"].item()), update_params=n, nef_update_cold_ms=round(old_ms, 4),
                   nef_update_ema_cold_ms=round(new_ms, 4), nef_update_cold_GBps=round(5 * 4 * n / (old_ms * 1e-3) / 1e9, 1),
                   nef_update_ema_cold_GBps=round(7 * 4 * n / (new_ms * 1e-3) / 1e9, 1))
    if mode in ("lars-graph", "lamb-graph") and (B, L) == EMA_SHAPES["config2"]:
        fl = optim._flat[0]
        n, segs = fl["p"].numel(), optim._segs(fl)
        ratio, stats = fl["ratio"].clone(), fl["trust_stats"].clone()
        if mode == "lars-graph":
            p, g, buf = (fl[k].clone() for k in ("p", "g", "buf"))
            old_ms, new_ms = cold_ms([lambda: ops.update_sgd(p, g, buf, 0.1, 0.9, 1.0),
                                      lambda: ops.update_lars(p, g, buf, 0.1, 0.9, 1.0, segs, ratio, stats)], dev)
            old_streams, new_streams = 5, 7
        else:
            p, g, m, v, s = (fl[k].clone() for k in ("p", "g", "m", "v", "step"))
            old_ms, new_ms = cold_ms([lambda: ops.update_adam(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-6, 0.0, 1.0),
                                      lambda: ops.update_lamb(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-6, 0.0, 1.0, segs, ratio, stats)], dev)
            old_streams, new_streams = 7, 11
        q = [x for x in fl["ratio"].tolist()]
        res.update(segments=int(segs[0].numel()), update_params=n, ratio_min=min(q), ratio_max=max(q),
                   steps_skipped_non_finite=int(fl["trust_stats"][3].item()), nef_update_cold_ms=round(old_ms, 4),
                   nef_update_trust_cold_ms=round(new_ms, 4), nef_update_cold_GBps=round(old_streams * 4 * n / (old_ms * 1e-3) / 1e9, 1),
                   nef_update_trust_cold_GBps=round(new_streams * 4 * n / (new_ms * 1e-3) / 1e9, 1))
    if mode == "adam-graph":
        fl = optim._flat[0]
        p, g, m, v, s = (fl[k].clone() for k in ("p", "g", "m", "v", "step"))
        n = p.numel()
        for _ in range(5):
            ops.adam(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 50
        e0.record()
        for _ in range(reps):
            ops.adam(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
        e1.record()
        e1.synchronize()
        warm = e0.elapsed_time(e1) / reps
        flush = torch.empty(512 << 18, device=dev, dtype=torch.float32)        # 512 MiB
        cold = []
        for i in range(30):
            flush.fill_(float(i))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.adam(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
            b.record()
            cold.append((a, b))
        torch.cuda.synchronize(dev)
        ms = float(np.median([a.elapsed_time(b) for a, b in cold]))
        res.update(nef_adam_cold_ms=round(ms, 4), nef_adam_warm_ms=round(warm, 4), nef_adam_params=n,
                   nef_adam_cold_GBps=round(7 * 4 * n / (ms * 1e-3) / 1e9, 1))
    if mode in ("sgd-graph-wd", "adamw-graph"):
        fl = optim._flat[0]
        runs = optim._runs(fl)
        n = fl["p"].numel()
        if mode == "sgd-graph-wd":
            p, g, buf = (fl[k].clone() for k in ("p", "g", "buf"))
            old_ms, new_ms = cold_ms([lambda: ops.sgd_momentum(p, g, buf, 0.1, 0.9, 1.0, False),
                                      lambda: ops.update_sgd(p, g, buf, 0.1, 0.9, 1.0, wd, False, runs=runs)], dev)
            streams, old = 5, "nef_sgd_momentum"
        else:
            p, g, m, v, s = (fl[k].clone() for k in ("p", "g", "m", "v", "step"))
            old_ms, new_ms = cold_ms([lambda: ops.adam(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0),
                                      lambda: ops.update_adam(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-8, wd, 1.0, decoupled=True, runs=runs)], dev)
            streams, old = 7, "nef_adam"
        res.update(weight_decay=wd, no_decay=list(no_decay), runs=0 if runs is None else int(runs[0].numel()), update_params=n,
                   old_entry=old, old_entry_cold_ms=round(old_ms, 4), nef_update_cold_ms=round(new_ms, 4),
                   nef_update_cold_GBps=round(streams * 4 * n / (new_ms * 1e-3) / 1e9, 1))
    if mode == "sgd-graph-clip":
        total, coef, clipped, bad = optim.clip_stats.tolist()
        g = optim._flat[0]["g"].clone()
        g0, n = g.clone(), g.numel()
        quarter = 0.25 * float(g0.double().norm().item())     # a quarter of this buffer's norm: the scale pass runs
        assert quarter > 0 and quarter == quarter and quarter != float("inf"), quarter
        stats = torch.zeros(4, device=dev)
        flush = torch.empty(512 << 18, device=dev, dtype=torch.float32)        # 512 MiB
        cold = []
        for i in range(30):
            g.copy_(g0)
            flush.fill_(float(i))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.grad_clip(g, quarter, 1.0, stats)
            b.record()
            cold.append((a, b))
        torch.cuda.synchronize(dev)
        ms = float(np.median([a.elapsed_time(b) for a, b in cold]))
        res.update(max_grad_norm=clip, last_norm=total, last_coef=coef, steps_clipped=int(clipped), steps_non_finite=int(bad),
                   steps_run=steps + warmup, nef_grad_clip_cold_ms=round(ms, 4), nef_grad_clip_params=n,
                   nef_grad_clip_launches_clipped=int(stats[2].item()))
    print("RESULT " + json.dumps(res), flush=True)


def run_child(cmd, tree, mode):
    """One measurement in a fresh process; its RESULT line.  A failure ends the whole run: nothing more is started."""
    r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-3000:])
        raise SystemExit(f"{mode}: exit status {r.returncode}; nothing more is started")
    return json.loads(line[0][len("RESULT "):])


def ema_rounds(args):
    """--ema D: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict(EMA_MODES, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool has no --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-ema":
                        cmd += ["--ema", str(args.ema)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    e2 = results[("config2", "sgd-graph-ema")][0]
    out = {"metric": "ms per train step, graphed FusedSGD with and without the EMA of the weights in the update launch "
                     "([min, median, max] over rounds)", "rounds": args.reps, "ema_decay": args.ema,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_ema_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_ema_on_ms"] = spread(shape, "sgd-graph-ema", "ms_per_step")
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # the two conditions: the EMA-off median inside the parent's own min-max spread; the EMA-on median <= parent median + 0.3 ms
            out[shape + "_ema_off_median_inside_parent_spread"] = par[0] <= out[shape + "_ema_off_ms"][1] <= par[2]
            out[shape + "_ema_on_median_minus_parent_median_ms"] = round(out[shape + "_ema_on_ms"][1] - par[1], 3)
    out.update(update_params=e2["update_params"], nef_update_cold_ms=spread("config2", "sgd-graph-ema", "nef_update_cold_ms"),
               nef_update_ema_cold_ms=spread("config2", "sgd-graph-ema", "nef_update_ema_cold_ms"),
               nef_update_cold_GBps=spread("config2", "sgd-graph-ema", "nef_update_cold_GBps"),
               nef_update_ema_cold_GBps=spread("config2", "sgd-graph-ema", "nef_update_ema_cold_GBps"),
               update_note="the update launch alone on the flat buffers (rule 0, no table), nef_update_ema alternating with nef_update in one "
                           "process; cold = a 512 MiB buffer written before each launch; 5 and 7 fp32 streams per parameter",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def accum_rounds(args):
    """--accum K: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-accum": 900}, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool may lack --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-accum":
                        cmd += ["--accum", str(args.accum)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    a2 = results[("config2", "sgd-graph-accum")][0]
    out = {"metric": "ms per train batch, graphed FusedSGD with accum_steps 1 and %d (per micro-batch) ([min, median, max] over rounds)" % args.accum,
           "rounds": args.reps, "accum_steps": args.accum,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_accum_1_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_accum_%d_ms_per_micro_batch" % args.accum] = spread(shape, "sgd-graph-accum", "ms_per_step")
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # the condition: accum_steps 1 is the parent's code path -- its median inside the parent's own min-max spread
            out[shape + "_accum_1_median_inside_parent_spread"] = par[0] <= out[shape + "_accum_1_ms"][1] <= par[2]
    out.update(flatten_tensors=a2["flatten_tensors"], flatten_params=a2["flatten_params"],
               nef_flatten_cold_ms=spread("config2", "sgd-graph-accum", "nef_flatten_cold_ms"),
               nef_flatten_acc_cold_ms=spread("config2", "sgd-graph-accum", "nef_flatten_acc_cold_ms"),
               nef_flatten_cold_GBps=spread("config2", "sgd-graph-accum", "nef_flatten_cold_GBps"),
               nef_flatten_acc_cold_GBps=spread("config2", "sgd-graph-accum", "nef_flatten_acc_cold_GBps"),
               flatten_note="the flatten launch alone on tensors of the model's gradient sizes, nef_flatten_acc (accumulate form) alternating "
                            "with nef_flatten in one process; cold = a 512 MiB buffer written before each launch; 3 and 2 fp32 streams per parameter",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r12_accum_bench_line.json"), "w") as f:
        f.write(line + "\n")


def sched_rounds(args):
    """--sched SHAPE --warmup W: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one
    JSON line."""
    W, untimed = args.warmup, 3
    modes = dict({"sgd-graph": 900, "sgd-graph-sched": 900}, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool may lack --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, untimed, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(untimed), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-sched":
                        cmd += ["--sched", args.sched, "--sched-warmup", str(W)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the per-update learning-rate schedule off and on ([min, median, max] over rounds)",
           "rounds": args.reps, "lr_shape": args.sched, "warmup_updates": W,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_sched_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_sched_on_ms"] = spread(shape, "sgd-graph-sched", "ms_per_step")
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # to be read against each other: the keys-off median and the parent's own min-max spread
            out[shape + "_sched_off_median_inside_parent_spread"] = par[0] <= out[shape + "_sched_off_ms"][1] <= par[2]
            out[shape + "_sched_on_median_minus_parent_median_ms"] = round(out[shape + "_sched_on_ms"][1] - par[1], 3)
    out.update(nef_lr_sched_cold_ms=spread("config2", "sgd-graph-sched", "nef_lr_sched_cold_ms"),
               nef_lr_sched_warm_ms=spread("config2", "sgd-graph-sched", "nef_lr_sched_warm_ms"),
               launch_note="the single-wave nef_lr_sched launch (advance form) alone; cold = a 512 MiB buffer written before each launch, warm = "
                           "200 back-to-back launches issued from Python (host-issue bound)",
               steps=args.steps, untimed_steps=untimed)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r14_sched_bench_line.json"), "w") as f:
        f.write(line + "\n")


def ssim_rounds(args):
    """--ssim F: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-ssim": 900}, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool may lack --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-ssim":
                        cmd += ["--ssim", str(args.ssim)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the SSIM term of the loss off and on ([min, median, max] over rounds)",
           "rounds": args.reps, "ssim_factor": args.ssim,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_ssim_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_ssim_on_ms"] = spread(shape, "sgd-graph-ssim", "ms_per_step")
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # to be read against each other: the key-off median and the parent's own min-max spread; the bar with the key on: + 0.3 ms
            out[shape + "_ssim_off_median_inside_parent_spread"] = par[0] <= out[shape + "_ssim_off_ms"][1] <= par[2]
            out[shape + "_ssim_on_median_minus_parent_median_ms"] = round(out[shape + "_ssim_on_ms"][1] - par[1], 3)
    out.update(nef_loss_ssim_fwd_cold_ms=spread("config2", "sgd-graph-ssim", "nef_loss_ssim_fwd_cold_ms"),
               nef_loss_ssim_bwd_cold_ms=spread("config2", "sgd-graph-ssim", "nef_loss_ssim_bwd_cold_ms"),
               launch_note="the term's launches alone at config 2 on the batch's rois (forward: partial sums + finish; backward: one launch); "
                           "cold = a 512 MiB buffer written before each call",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r15_ssim_bench_line.json"), "w") as f:
        f.write(line + "\n")


def augment_rounds(args):
    """--augment: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-augment": 900}, **({"sgd-graph-lead-mask": 900} if args.lead_mask else {}),
                 **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool may lack --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the input-lead augmentation off and on ([min, median, max] over rounds of "
                     "fresh processes)", "rounds": args.reps, "augment": dict(AUGMENT_KEYS),
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_augment_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_augment_on_ms"] = spread(shape, "sgd-graph-augment", "ms_per_step")
        out[shape + "_input_elements_changed"] = spread(shape, "sgd-graph-augment", "input_elements_changed")[1]
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # to be read against each other: the keys-off median and the parent's own min-max spread; the bar with the keys on: + 0.3 ms
            out[shape + "_augment_off_median_inside_parent_spread"] = par[0] <= out[shape + "_augment_off_ms"][1] <= par[2]
            out[shape + "_augment_on_median_minus_parent_median_ms"] = round(out[shape + "_augment_on_ms"][1] - par[1], 3)
            out[shape + "_augment_off_median_minus_parent_median_ms"] = round(out[shape + "_augment_off_ms"][1] - par[1], 3)
        if args.lead_mask:
            out[shape + "_lead_mask_on_ms"] = on = spread(shape, "sgd-graph-lead-mask", "ms_per_step")
            out[shape + "_leads_masked"] = spread(shape, "sgd-graph-lead-mask", "leads_masked")[1]
            out[shape + "_lead_mask_over_augment_median"] = round(on[1] / out[shape + "_augment_on_ms"][1], 4)
    if args.lead_mask:
        cold = [x["mix_cold_ms"] for x in results[("config2", "sgd-graph-lead-mask")]]
        out.update(lead_mask=True, mix_cold_ms={k: sorted(c[k] for c in cold)[len(cold) // 2] for k in cold[0]},
                   mix_note="medians over the rounds; the two mix entries alone at config 2 (a mask with aug_lead_drop's share of leads "
                            "absent) beside nef_lead_mean + nef_mix_fwd and nef_mix_bwd(shared = 0, up = 0), cold")
    out.update(nef_augment_cold_ms=spread("config2", "sgd-graph-augment", "nef_augment_cold_ms"),
               nef_augment_cold_GBps=spread("config2", "sgd-graph-augment", "nef_augment_cold_GBps"),
               launch_note="the nef_augment launch alone at config 2 on the batch's inputs and rois, all four corruptions on; cold = a 512 MiB "
                           "buffer written before each call; bytes counted: x read, y written",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    default = "r28_lead_mask_bench_line.json" if args.lead_mask else "r17_augment_bench_line.json"
    with open(args.out or os.path.join(ROOT, "profiles", default), "w") as f:
        f.write(line + "\n")


def warp_rounds(args):
    """--warp A0 .. A5 [--roi-jitter J]: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and
    writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-warp": 900}, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool lacks --warp: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L),
                           "--warp"] + [repr(float(a)) for a in args.warp] + ["--roi-jitter", str(args.roi_jitter)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the time warp off and on -- on: one nef_warp launch per step in front of the "
                     "replay ([min, median, max] over rounds of fresh processes)", "rounds": args.reps,
           "aug_warp": [float(a) for a in args.warp], "aug_roi_jitter": args.roi_jitter,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_warp_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_warp_on_ms"] = spread(shape, "sgd-graph-warp", "ms_per_step")
        out[shape + "_input_elements_changed"] = spread(shape, "sgd-graph-warp", "input_elements_changed")[1]
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # to be read against each other: the keys-off median and the parent's own min-max spread; the bar with the keys on: + 0.3 ms
            out[shape + "_warp_off_median_inside_parent_spread"] = par[0] <= out[shape + "_warp_off_ms"][1] <= par[2]
            out[shape + "_warp_on_median_minus_parent_median_ms"] = round(out[shape + "_warp_on_ms"][1] - par[1], 3)
    out.update(nef_warp_cold_ms=spread("config2", "sgd-graph-warp", "nef_warp_cold_ms"),
               nef_warp_cold_GBps=spread("config2", "sgd-graph-warp", "nef_warp_cold_GBps"),
               nef_warp_bytes=results[("config2", "sgd-graph-warp")][0]["nef_warp_bytes"],
               launch_note="the nef_warp launch alone at config 2 on the batch's inputs, target and rois (no rest views); cold = a 512 MiB "
                           "buffer written before each call; bytes counted: every input read once, every output written",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r25_warp_bench_line.json"), "w") as f:
        f.write(line + "\n")


def device_noise_rounds(args):
    """--device-noise: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-device-noise": 900}, **({"parent": 900, "parent-noise": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                tree = os.path.abspath(args.parent_tree) if mode.startswith("parent") else ROOT
                if mode == "parent":
                    # the parent's tool lacks --device-noise: its `child` function is called directly, in a fresh process of its own tree
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    # parent-noise: this tool's DATA.noise child on the parent's package (--parent-tree puts DIR in front of the path)
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child",
                           "sgd-graph-noise" if mode == "parent-noise" else mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "parent-noise":
                        cmd += ["--parent-tree", tree]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with DATA.device_noise off and on -- on: one captured nef_noise_row launch in front "
                     "of the loss launches ([min, median, max] over rounds of fresh processes)", "rounds": args.reps,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on, synthetic batches" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_device_noise_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_device_noise_on_ms"] = spread(shape, "sgd-graph-device-noise", "ms_per_step")
        out[shape + "_noise_elements_nonzero"] = spread(shape, "sgd-graph-device-noise", "noise_elements_nonzero")[1]
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            out[shape + "_parent_data_noise_ms"] = pn = spread(shape, "parent-noise", "ms_per_step")
            # to be read against each other: the keys-off median and the parent's own min-max spread; the key-on median and the parent's
            # like-for-like step with a host row (DATA.noise), the bar: + 0.3 ms
            out[shape + "_device_noise_off_median_inside_parent_spread"] = par[0] <= out[shape + "_device_noise_off_ms"][1] <= par[2]
            out[shape + "_device_noise_off_median_minus_parent_median_ms"] = round(out[shape + "_device_noise_off_ms"][1] - par[1], 3)
            out[shape + "_device_noise_on_median_minus_parent_data_noise_median_ms"] = round(out[shape + "_device_noise_on_ms"][1] - pn[1], 3)
    out.update(nef_noise_row_cold_ms=spread("config2", "sgd-graph-device-noise", "nef_noise_row_cold_ms"),
               nef_noise_row_cold_GBps=spread("config2", "sgd-graph-device-noise", "nef_noise_row_cold_GBps"),
               nef_noise_row_bytes=results[("config2", "sgd-graph-device-noise")][0]["nef_noise_row_bytes"],
               nef_noise_row_segment_elements=results[("config2", "sgd-graph-device-noise")][0]["nef_noise_row_segment_elements"],
               launch_note="the nef_noise_row launch alone at config 2 on the batch's target and rois; cold = a 512 MiB buffer written before "
                           "each call; bytes counted: the row written, the quiet segments read twice, the rois",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r30_device_noise_bench_line.json"), "w") as f:
        f.write(line + "\n")


def seg_rounds(args):
    """--seg W0 .. W6: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-seg": 900}, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool has no --seg: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-seg":
                        cmd += ["--seg"] + [repr(float(w)) for w in args.seg]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the wave-segment weights of the reconstruction term off and on ([min, median, "
                     "max] over rounds of fresh processes)", "rounds": args.reps, "seg_weights": [float(w) for w in args.seg],
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_seg_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_seg_on_ms"] = spread(shape, "sgd-graph-seg", "ms_per_step")
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # the bars: key off, the median not above the parent's slowest round; key on, the median at most 0.3 ms above the parent's
            out[shape + "_seg_off_median_not_above_parent_max"] = out[shape + "_seg_off_ms"][1] <= par[2]
            out[shape + "_seg_off_median_inside_parent_spread"] = par[0] <= out[shape + "_seg_off_ms"][1] <= par[2]
            out[shape + "_seg_on_median_minus_parent_median_ms"] = round(out[shape + "_seg_on_ms"][1] - par[1], 3)
    for k in ("nef_loss_seg_fwd", "nef_loss_seg_bwd", "nef_view_seg_metrics"):
        out[k + "_cold_ms"] = spread("config2", "sgd-graph-seg", k + "_cold_ms")
        out[k + "_cold_GBps"] = spread("config2", "sgd-graph-seg", k + "_cold_GBps")
    out.update(launch_note="the three entries alone at config 2 (B=256, L=5000; the metrics on 9 views per sample); cold = a 512 MiB buffer "
                           "written before each call; bytes counted: prediction and target read (fwd), the gradient read and written "
                           "(bwd), prediction and ground truth read (metrics)",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r18_seg_bench_line.json"), "w") as f:
        f.write(line + "\n")


def slope_rounds(args):
    """--slope F: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-slope": 900}, **({"parent": 900} if args.parent_tree else {}))
    shapes = {k: v for k, v in EMA_SHAPES.items() if args.only_shape in (None, k)}
    results = {(shape, mode): [] for shape in shapes for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in shapes.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool has no --slope: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-slope":
                        cmd += ["--slope", repr(float(args.slope))]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the slope term of the loss off and on ([min, median, max] over rounds of "
                     "fresh processes)", "rounds": args.reps, "slope_factor": args.slope, "slope_loss": "l1_loss", "slope_crop": True,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in shapes.items()}}
    for shape in shapes:
        out[shape + "_slope_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_slope_on_ms"] = spread(shape, "sgd-graph-slope", "ms_per_step")
        out[shape + "_slope_on_loss_row"] = results[(shape, "sgd-graph-slope")][0]["loss_row"]
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # the bar: key on, the median at most 0.3 ms above the parent's.  Key off (the parent's launches): where the median lies
            # against the parent's own spread is reported, not judged
            out[shape + "_slope_on_median_minus_parent_median_ms"] = round(out[shape + "_slope_on_ms"][1] - par[1], 3)
            out[shape + "_slope_off_median_inside_parent_spread"] = par[0] <= out[shape + "_slope_off_ms"][1] <= par[2]
            out[shape + "_slope_off_median_minus_parent_median_ms"] = round(out[shape + "_slope_off_ms"][1] - par[1], 3)
    if "config2" in shapes:
        for k in ("nef_loss_slope_fwd", "nef_loss_slope_bwd", "nef_view_slope_metrics"):
            out[k + "_cold_ms"] = spread("config2", "sgd-graph-slope", k + "_cold_ms")
            out[k + "_cold_GBps"] = spread("config2", "sgd-graph-slope", k + "_cold_GBps")
        out.update(launch_note="the three entries alone at config 2 (B=256, L=5000; the metrics on 9 views per sample); cold = a 512 MiB "
                               "buffer written before each call; bytes counted: prediction and target read (fwd), prediction and target "
                               "read, the gradient read and written (bwd), prediction and ground truth read (metrics)")
    out.update(steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r19_slope_bench_line.json"), "w") as f:
        f.write(line + "\n")


def corr_rounds(args):
    """--corr F: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON line."""
    modes = dict({"sgd-graph": 900, "sgd-graph-corr": 900}, **({"parent": 900} if args.parent_tree else {}))
    shapes = {k: v for k, v in EMA_SHAPES.items() if args.only_shape in (None, k)}
    results = {(shape, mode): [] for shape in shapes for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in shapes.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool has no --corr: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                    if mode == "sgd-graph-corr":
                        cmd += ["--corr", repr(float(args.corr))]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD with the correlation term of the loss off and on ([min, median, max] over rounds "
                     "of fresh processes)", "rounds": args.reps, "corr_factor": args.corr, "corr_crop": True,
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in shapes.items()}}
    for shape in shapes:
        out[shape + "_corr_off_ms"] = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_corr_on_ms"] = spread(shape, "sgd-graph-corr", "ms_per_step")
        out[shape + "_corr_on_loss_row"] = results[(shape, "sgd-graph-corr")][0]["loss_row"]
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            # the bar: key on, the median at most 0.3 ms above the parent's.  Key off (the parent's launches): where the median lies
            # against the parent's own spread is reported, not judged
            out[shape + "_corr_on_median_minus_parent_median_ms"] = round(out[shape + "_corr_on_ms"][1] - par[1], 3)
            out[shape + "_corr_off_median_inside_parent_spread"] = par[0] <= out[shape + "_corr_off_ms"][1] <= par[2]
            out[shape + "_corr_off_median_minus_parent_median_ms"] = round(out[shape + "_corr_off_ms"][1] - par[1], 3)
    if "config2" in shapes:
        for k in ("nef_loss_corr_fwd", "nef_loss_corr_bwd", "nef_view_corr_metrics"):
            out[k + "_cold_ms"] = spread("config2", "sgd-graph-corr", k + "_cold_ms")
            out[k + "_cold_GBps"] = spread("config2", "sgd-graph-corr", k + "_cold_GBps")
        out.update(launch_note="the three entries alone at config 2 (B=256, L=5000; the metrics on 9 views per sample); cold = a 512 MiB "
                               "buffer written before each call; bytes counted: prediction and target read (fwd), prediction and target "
                               "read twice, the gradient read and written (bwd), prediction and ground truth read (metrics)")
    out.update(steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r20_corr_bench_line.json"), "w") as f:
        f.write(line + "\n")


def views_rounds(args):
    """--views Q [Q ...]: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON
    line."""
    qs = list(args.views)
    modes = dict({"sgd-graph": 900}, **{f"views{q}": 900 for q in qs}, **({"parent": 900} if args.parent_tree else {}))
    shapes = {k: v for k, v in EMA_SHAPES.items() if args.only_shape in (None, k)}
    results = {(shape, mode): [] for shape in shapes for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in shapes.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool may lack --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child('sgd-graph', %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child",
                           "sgd-graph" if mode == "sgd-graph" else "sgd-graph-views", "--steps", str(args.steps), "--warmup", str(args.warmup),
                           "--shape", str(B), str(L)]
                    if mode != "sgd-graph":
                        cmd += ["--views", mode[len("views"):]]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    out = {"metric": "ms per train step, graphed FusedSGD, one target view per step (key off) and SOLVER.train_views = Q ([min, median, max] over "
                     "rounds of fresh processes)",
           "rounds": args.reps, "train_views": qs, "flop_model": "a Q-view step costs 1 + 0.31 (Q - 1) single-view steps (SURVEY.md 8(d))",
           "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in shapes.items()}}
    for shape in shapes:
        out[shape + "_views_off_ms"] = off = spread(shape, "sgd-graph", "ms_per_step")
        out[shape + "_views_off_max_memory_GiB"] = spread(shape, "sgd-graph", "max_memory_allocated_GiB")[1]
        base = off
        if args.parent_tree:
            out[shape + "_parent_ms"] = par = spread(shape, "parent", "ms_per_step")
            out[shape + "_views_off_median_inside_parent_spread"] = par[0] <= off[1] <= par[2]
            out[shape + "_views_off_median_minus_parent_max_ms"] = round(off[1] - par[2], 3)
            base = par
        for q in qs:
            out[f"{shape}_views{q}_ms"] = st = spread(shape, f"views{q}", "ms_per_step")
            out[f"{shape}_views{q}_ms_per_view"] = spread(shape, f"views{q}", "ms_per_view")
            out[f"{shape}_views{q}_steps_measured_vs_model"] = [round(st[1] / base[1], 3), round(1 + 0.31 * (q - 1), 2)]
            out[f"{shape}_views{q}_max_memory_GiB"] = spread(shape, f"views{q}", "max_memory_allocated_GiB")[1]
        # the one speed condition: ms per supervised view at the largest Q below the single-view step of the same session
        q = max(qs)
        out[f"{shape}_ms_per_view_at_{q}_below_single_view_step"] = out[f"{shape}_views{q}_ms_per_view"][1] < base[1]
    if "config2" in shapes:
        q = max(qs)
        out.update(copy_many_cold_ms={f"views{q_}": results[("config2", f"views{q_}")][0]["copy_many_cold_ms"] for q_ in qs},
                   copy_many_cold_GBps={f"views{q_}": results[("config2", f"views{q_}")][0]["copy_many_cold_GBps"] for q_ in qs},
                   copy_many_note="the step's four nef_copy_many launches alone at config 2 (first round's child): 3Q output segments into the "
                                  "[3, Q, B, 1, L] layout, the same back, one view's (gz1, gz2b, chan_sum) and one view's %d head parameter "
                                  "gradients summed into the first view's (the last two run Q - 1 times per step); cold = a 512 MiB buffer "
                                  "written before each call" % results[("config2", f"views{q}")][0]["copy_many_head_tensors"])
    out.update(steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r16_views_bench_line.json"), "w") as f:
        f.write(line + "\n")


def trust_rounds(args):
    """--trust lars|lamb: `--reps` alternating rounds of fresh children per shape (see the module docstring); prints and writes one JSON
    line."""
    base, new = TRUST_BASE[args.trust], args.trust + "-graph"
    modes = dict({base: 900, new: 900}, **({"parent": 900} if args.parent_tree else {}))
    results = {(shape, mode): [] for shape in EMA_SHAPES for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))
        for shape, (B, L) in EMA_SHAPES.items():
            for mode in order:
                if mode == "parent":
                    # the parent's tool may lack --shape: its `child` function is called directly, in a fresh process of its own tree
                    tree = os.path.abspath(args.parent_tree)
                    code = ("import importlib.util as u; s = u.spec_from_file_location('parent_bench', %r); m = u.module_from_spec(s); "
                            "s.loader.exec_module(m); m.child(%r, %d, %d, B=%d, L=%d)"
                            % (os.path.join(tree, "tools", "bench_adam.py"), base, args.steps, args.warmup, B, L))
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, "-c", code]
                else:
                    tree = ROOT
                    cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(ROOT, "tools", "bench_adam.py"), "--child", mode,
                           "--steps", str(args.steps), "--warmup", str(args.warmup), "--shape", str(B), str(L)]
                results[(shape, mode)].append(run_child(cmd, tree, mode))
                sys.stderr.write(f"round {rnd + 1}/{args.reps} {shape} {mode}: {results[(shape, mode)][-1]['ms_per_step']} ms/step\n")
                sys.stderr.flush()

    def spread(shape, mode, key):
        v = sorted(x[key] for x in results[(shape, mode)])
        return [v[0], v[len(v) // 2], v[-1]]

    t2 = results[("config2", new)][0]
    out = {"metric": "ms per train step, graphed: %s beside %s ([min, median, max] over rounds)" % (new, base), "rounds": args.reps,
           "trust": args.trust, "shapes": {k: "B=%d, 3 leads, L=%d, one GPU, dropout on" % v for k, v in EMA_SHAPES.items()}}
    for shape in EMA_SHAPES:
        out[shape + "_" + base.replace("-", "_") + "_ms"] = spread(shape, base, "ms_per_step")
        out[shape + "_" + new.replace("-", "_") + "_ms"] = spread(shape, new, "ms_per_step")
        if args.parent_tree:
            out[shape + "_parent_" + base.replace("-", "_") + "_ms"] = par = spread(shape, "parent", "ms_per_step")
            # the bar: the trust median <= the parent's median of the plain optimiser + 0.3 ms
            out[shape + "_trust_median_minus_parent_median_ms"] = round(out[shape + "_" + new.replace("-", "_") + "_ms"][1] - par[1], 3)
    out.update(update_params=t2["update_params"], segments=t2["segments"], ratio_min=t2["ratio_min"], ratio_max=t2["ratio_max"],
               nef_update_cold_ms=spread("config2", new, "nef_update_cold_ms"),
               nef_update_trust_cold_ms=spread("config2", new, "nef_update_trust_cold_ms"),
               nef_update_cold_GBps=spread("config2", new, "nef_update_cold_GBps"),
               nef_update_trust_cold_GBps=spread("config2", new, "nef_update_trust_cold_GBps"),
               update_note="the entry's launches alone on the flat buffers with the model's segment table, nef_update_trust alternating with "
                           "nef_update (same rule, no table) in one process; cold = a 512 MiB buffer written before each call; bytes counted: "
                           "lars 2 + 5 fp32 streams per parameter against 5, lamb 4 + 7 against 7",
               steps=args.steps, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    with open(args.out or os.path.join(ROOT, "profiles", "r11_trust_bench_line.json"), "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="rounds of the three children")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--clip", type=float, default=None, metavar="MAX_NORM", help="measure gradient-norm clipping (see above)")
    ap.add_argument("--weight-decay", type=float, default=None, metavar="X", help="measure weight decay in the update launch (see above)")
    ap.add_argument("--no-decay", nargs="*", default=[], metavar="PATTERN", help="with --weight-decay: fnmatch patterns of exempt tensors")
    ap.add_argument("--ema", type=float, default=None, metavar="D", help="measure the EMA of the weights in the update launch (see above)")
    ap.add_argument("--trust", choices=sorted(TRUST_BASE), default=None, help="measure the layer-wise trust ratios (see above)")
    ap.add_argument("--accum", type=int, default=None, metavar="K", help="measure gradient accumulation, accum_steps = K (see above)")
    ap.add_argument("--sched", choices=("const", "cosine", "poly"), default=None,
                    help="measure the per-update learning-rate schedule of this shape; --warmup is then the schedule's W (see above)")
    ap.add_argument("--sched-warmup", type=int, default=None, metavar="W", help="with --child sgd-graph-sched: the schedule's W")
    ap.add_argument("--ssim", type=float, default=None, metavar="F", help="measure the SSIM term of the loss, ssim_factor = F (see above)")
    ap.add_argument("--views", type=int, nargs="+", default=None, metavar="Q",
                    help="measure SOLVER.train_views = Q for every Q given (see above); with --child sgd-graph-views: the one Q")
    ap.add_argument("--augment", action="store_true", help="measure the input-lead augmentation of the train step, DATA.aug_* (see above)")
    ap.add_argument("--lead-mask", action="store_true", help="with --augment: also measure the masked head, MODEL.lead_mask (see above)")
    ap.add_argument("--seg", type=float, nargs=7, default=None, metavar="W",
                    help="measure the wave-segment weights of the reconstruction term, SOLVER.seg_weights = W0 .. W6 (see above)")
    ap.add_argument("--slope", type=float, default=None, metavar="F", help="measure the slope term of the loss, slope_factor = F (see above)")
    ap.add_argument("--corr", type=float, default=None, metavar="F", help="measure the correlation term of the loss, corr_factor = F (see above)")
    ap.add_argument("--warp", type=float, nargs=6, default=None, metavar="A",
                    help="measure the time warp of the train batch, DATA.aug_warp = A0 .. A5 (see above)")
    ap.add_argument("--roi-jitter", type=int, default=0, metavar="J", help="with --warp: DATA.aug_roi_jitter = J")
    ap.add_argument("--device-noise", action="store_true", help="measure the train step's own noise row, DATA.device_noise (see above)")
    ap.add_argument("--only-shape", choices=sorted(EMA_SHAPES), default=None, help="with --views, --slope or --corr: measure this shape only")
    ap.add_argument("--shape", type=int, nargs=2, default=(256, 5000), metavar=("B", "L"), help="with --child: batch size and length")
    ap.add_argument("--parent-tree", default=None,
                    help="with --clip / --weight-decay / --ema: a built checkout whose own sgd-graph child runs in every round")
    ap.add_argument("--child", choices=sorted({**MODES, **CLIP_MODES, **WD_MODES, **EMA_MODES, "lars-graph": 900, "lamb-graph": 900, "sgd-graph-accum": 900,
                                             "sgd-graph-sched": 900, "sgd-graph-ssim": 900, "sgd-graph-views": 900, "sgd-graph-augment": 900, "sgd-graph-lead-mask": 900,
                                             "sgd-graph-seg": 900, "sgd-graph-slope": 900, "sgd-graph-corr": 900, "sgd-graph-warp": 900,
                                             "sgd-graph-noise": 900, "sgd-graph-device-noise": 900}),
                    default=None)
    args = ap.parse_args()
    if args.child == "sgd-graph-ema" and not (args.ema is not None and 0.0 < args.ema < 1.0):
        ap.error("--child sgd-graph-ema needs --ema D in (0, 1)")
    if args.ema is not None and (args.clip is not None or args.weight_decay is not None):
        ap.error("--ema is a measurement of its own")
    if args.child == "sgd-graph-clip" and not (args.clip is not None and args.clip > 0):
        ap.error("--child sgd-graph-clip needs --clip MAX_NORM > 0")
    if args.child in ("sgd-graph-wd", "adamw-graph") and args.weight_decay is None:
        ap.error(f"--child {args.child} needs --weight-decay X")
    if args.clip is not None and args.weight_decay is not None:
        ap.error("--clip and --weight-decay are two measurements")
    if args.trust is not None and (args.clip is not None or args.weight_decay is not None or args.ema is not None):
        ap.error("--trust is a measurement of its own")
    if args.accum is not None and (args.accum < 2 or args.clip is not None or args.weight_decay is not None or args.ema is not None
                                   or args.trust is not None):
        ap.error("--accum K >= 2 is a measurement of its own")
    if args.child == "sgd-graph-accum" and args.accum is None:
        ap.error("--child sgd-graph-accum needs --accum K")
    if args.sched is not None and not args.child and (args.clip is not None or args.weight_decay is not None or args.ema is not None
                                                      or args.trust is not None or args.accum is not None or args.warmup < 0):
        ap.error("--sched SHAPE --warmup W >= 0 is a measurement of its own")
    if args.child == "sgd-graph-sched" and (args.sched is None or args.sched_warmup is None):
        ap.error("--child sgd-graph-sched needs --sched SHAPE and --sched-warmup W")
    if args.ssim is not None and (not args.ssim > 0 or (not args.child and (
            args.clip is not None or args.weight_decay is not None or args.ema is not None or args.trust is not None
            or args.accum is not None or args.sched is not None))):
        ap.error("--ssim F > 0 is a measurement of its own")
    if args.child == "sgd-graph-ssim" and args.ssim is None:
        ap.error("--child sgd-graph-ssim needs --ssim F")
    if args.views is not None and (min(args.views) < 2 or (args.child == "sgd-graph-views" and len(args.views) != 1) or (not args.child and (
            args.clip is not None or args.weight_decay is not None or args.ema is not None or args.trust is not None
            or args.accum is not None or args.sched is not None or args.ssim is not None))):
        ap.error("--views Q >= 2 is a measurement of its own (one Q with --child sgd-graph-views)")
    if args.child == "sgd-graph-views" and args.views is None:
        ap.error("--child sgd-graph-views needs --views Q")
    if args.augment and not args.child and (args.views is not None or args.clip is not None or args.weight_decay is not None
                                            or args.ema is not None or args.trust is not None or args.accum is not None
                                            or args.sched is not None or args.ssim is not None):
        ap.error("--augment is a measurement of its own")
    if args.lead_mask and not args.child and not args.augment:
        ap.error("--lead-mask goes with --augment: MODEL.lead_mask needs its aug_lead_drop")
    if args.seg is not None and not args.child and (args.augment or args.views is not None or args.clip is not None
                                                    or args.weight_decay is not None or args.ema is not None or args.trust is not None
                                                    or args.accum is not None or args.sched is not None or args.ssim is not None):
        ap.error("--seg is a measurement of its own")
    if args.child == "sgd-graph-seg" and args.seg is None:
        ap.error("--child sgd-graph-seg needs --seg W0 .. W6")
    if args.slope is not None and (not args.slope > 0 or (not args.child and (
            args.seg is not None or args.augment or args.views is not None or args.clip is not None or args.weight_decay is not None
            or args.ema is not None or args.trust is not None or args.accum is not None or args.sched is not None
            or args.ssim is not None))):
        ap.error("--slope F > 0 is a measurement of its own")
    if args.child == "sgd-graph-slope" and args.slope is None:
        ap.error("--child sgd-graph-slope needs --slope F")
    if args.corr is not None and (not args.corr > 0 or (not args.child and (
            args.slope is not None or args.seg is not None or args.augment or args.views is not None or args.clip is not None
            or args.weight_decay is not None or args.ema is not None or args.trust is not None or args.accum is not None
            or args.sched is not None or args.ssim is not None))):
        ap.error("--corr F > 0 is a measurement of its own")
    if args.child == "sgd-graph-corr" and args.corr is None:
        ap.error("--child sgd-graph-corr needs --corr F")
    if args.warp is not None and not args.child and (
            args.corr is not None or args.slope is not None or args.seg is not None or args.augment or args.views is not None
            or args.clip is not None or args.weight_decay is not None or args.ema is not None or args.trust is not None
            or args.accum is not None or args.sched is not None or args.ssim is not None):
        ap.error("--warp is a measurement of its own")
    if args.child == "sgd-graph-warp" and args.warp is None:
        ap.error("--child sgd-graph-warp needs --warp A0 .. A5")
    if args.device_noise and not args.child and (
            args.warp is not None or args.corr is not None or args.slope is not None or args.seg is not None or args.augment
            or args.views is not None or args.clip is not None or args.weight_decay is not None or args.ema is not None
            or args.trust is not None or args.accum is not None or args.sched is not None or args.ssim is not None):
        ap.error("--device-noise is a measurement of its own")
    if (args.parent_tree and not args.device_noise and not args.child and args.warp is None and args.corr is None and args.slope is None and args.seg is None and not args.augment and args.views is None and args.clip is None and args.weight_decay is None and args.ema is None and args.trust is None
            and args.accum is None and args.sched is None and args.ssim is None):
        ap.error("--parent-tree goes with --clip, --weight-decay, --ema, --trust, --accum, --sched, --ssim, --views, --augment, --seg, --slope, --corr, --warp or --device-noise")
    if args.child:
        if args.parent_tree:       # the child imports DIR's package (and loads DIR's library) instead of this tree's
            sys.path.insert(0, os.path.abspath(args.parent_tree))
        return child(args.child, args.steps if args.child != "adam-eager" else max(3, args.steps // 2), args.warmup,
                     B=args.shape[0], L=args.shape[1], clip=args.clip or 0.0, wd=args.weight_decay or 0.0,
                     no_decay=tuple(args.no_decay), ema=args.ema or 0.0, accum=args.accum or 1,
                     sched=(args.sched, args.sched_warmup) if args.child == "sgd-graph-sched" else None, ssim=args.ssim or 0.0,
                     views=args.views[0] if args.views else 1, seg=args.seg, slope=args.slope or 0.0, corr=args.corr or 0.0, warp=args.warp, roi_jitter=args.roi_jitter)
    if args.device_noise:
        return device_noise_rounds(args)
    if args.warp is not None:
        return warp_rounds(args)
    if args.corr is not None:
        return corr_rounds(args)
    if args.slope is not None:
        return slope_rounds(args)
    if args.seg is not None:
        return seg_rounds(args)
    if args.augment:
        return augment_rounds(args)
    if args.views is not None:
        return views_rounds(args)
    if args.ssim is not None:
        return ssim_rounds(args)
    if args.sched is not None:
        return sched_rounds(args)
    if args.ema is not None:
        return ema_rounds(args)
    if args.trust is not None:
        return trust_rounds(args)
    if args.accum is not None:
        return accum_rounds(args)
    modes = dict(MODES)
    if args.clip is not None:
        modes = dict(CLIP_MODES, **({"parent": 900} if args.parent_tree else {}))
    if args.weight_decay is not None:
        modes = dict(WD_MODES, **({"parent": 900} if args.parent_tree else {}))
    results = {mode: [] for mode in modes}
    for rnd in range(args.reps):
        order = list(modes) if rnd % 2 == 0 else list(reversed(modes))       # no mode always runs first on a fresh box
        for mode in order:
            tree = os.path.abspath(args.parent_tree) if mode == "parent" else ROOT
            cmd = ["timeout", "-k", "10", str(modes[mode]), sys.executable, os.path.join(tree, "tools", "bench_adam.py"), "--child",
                   "sgd-graph" if mode == "parent" else mode, "--steps", str(args.steps), "--warmup", str(args.warmup)]
            if mode == "sgd-graph-clip":
                cmd += ["--clip", str(args.clip)]
            if mode in ("sgd-graph-wd", "adamw-graph"):
                cmd += ["--weight-decay", str(args.weight_decay), "--no-decay"] + list(args.no_decay)
            r = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-3000:])
                raise SystemExit(f"{mode}: exit status {r.returncode}; nothing more is started")
            results[mode].append(json.loads(line[0][len("RESULT "):]))
            sys.stderr.write(f"round {rnd + 1}/{args.reps} {mode}: {results[mode][-1]['ms_per_step']} ms/step\n")
            sys.stderr.flush()

    def spread(mode, key):
        v = sorted(x[key] for x in results[mode])
        return [v[0], v[len(v) // 2], v[-1]]

    if args.weight_decay is not None:
        sw, aw = results["sgd-graph-wd"][0], results["adamw-graph"][0]
        out = {"metric": "ms per train step, graphed, with and without weight decay in the update launch ([min, median, max] over rounds)",
               "config": "BASELINE config 2: B=256, 3 leads, L=5000, one GPU, dropout on", "rounds": args.reps,
               "weight_decay": args.weight_decay, "no_decay": list(args.no_decay), "runs": aw["runs"],
               "sgd_graphed_decay_off_ms": spread("sgd-graph", "ms_per_step"), "sgd_graphed_decay_on_ms": spread("sgd-graph-wd", "ms_per_step"),
               "adam_graphed_decay_off_ms": spread("adam-graph", "ms_per_step"), "adamw_graphed_decay_on_ms": spread("adamw-graph", "ms_per_step"),
               "update_params": aw["update_params"],
               "nef_adam_cold_ms": spread("adamw-graph", "old_entry_cold_ms"),
               "nef_update_adamw_cold_ms": spread("adamw-graph", "nef_update_cold_ms"),
               "nef_update_adamw_cold_GBps": spread("adamw-graph", "nef_update_cold_GBps"),
               "nef_sgd_momentum_cold_ms": spread("sgd-graph-wd", "old_entry_cold_ms"),
               "nef_update_sgd_cold_ms": spread("sgd-graph-wd", "nef_update_cold_ms"),
               "nef_update_sgd_cold_GBps": spread("sgd-graph-wd", "nef_update_cold_GBps"),
               "update_note": "the update launch alone on the flat buffers with the model's real run table (%d runs), alternating with the entry "
                              "beside it in one process; cold = a 512 MiB buffer written before each launch" % sw["runs"],
               "steps": args.steps, "warmup": args.warmup}
        if args.parent_tree:
            out["parent_sgd_graphed_ms"] = spread("parent", "ms_per_step")
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    if args.clip is not None:
        cg = results["sgd-graph-clip"]
        out = {"metric": "ms per train step, graphed FusedSGD with and without gradient-norm clipping ([min, median, max] over rounds)",
               "config": "BASELINE config 2: B=256, 3 leads, L=5000, one GPU, dropout on", "rounds": args.reps,
               "max_grad_norm": args.clip, "sgd_graphed_clip_off_ms": spread("sgd-graph", "ms_per_step"),
               "sgd_graphed_clip_on_ms": spread("sgd-graph-clip", "ms_per_step"),
               "steps_clipped_of_run": [[x["steps_clipped"], x["steps_run"]] for x in cg],
               "nef_grad_clip_cold_ms": spread("sgd-graph-clip", "nef_grad_clip_cold_ms"),
               "nef_grad_clip_params": cg[0]["nef_grad_clip_params"],
               "nef_grad_clip_note": "the three launches alone on the flat gradient buffer, every launch clipping (read, read + write); "
                                     "cold = a 512 MiB buffer written before each call",
               "steps": args.steps, "warmup": args.warmup}
        if args.parent_tree:
            out["parent_sgd_graphed_ms"] = spread("parent", "ms_per_step")
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    ag = results["adam-graph"]
    out = {"metric": "ms per train step, Adam vs SGD ([min, median, max] over rounds)",
           "config": "BASELINE config 2: B=256, 3 leads, L=5000, one GPU, dropout on", "rounds": args.reps,
           "sgd_graphed_ms": spread("sgd-graph", "ms_per_step"), "adam_graphed_ms": spread("adam-graph", "ms_per_step"),
           "data_parallel_adam_eager_ms": spread("adam-eager", "ms_per_step"),
           "nef_adam_cold_ms": spread("adam-graph", "nef_adam_cold_ms"), "nef_adam_cold_GBps": spread("adam-graph", "nef_adam_cold_GBps"),
           "nef_adam_warm_ms": spread("adam-graph", "nef_adam_warm_ms"), "nef_adam_params": ag[0]["nef_adam_params"],
           "nef_adam_note": "cold = a 512 MiB buffer written before each launch (the 115 MB working set is evicted, as behind the "
                            "backward pass); warm = back-to-back launches, working set in the 256 MiB Infinity Cache",
           "steps": args.steps, "warmup": args.warmup, "eager_steps": results["adam-eager"][0]["steps"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
