"""hipGraph-captured train step.

At the reference's own training shape (batch 32, 512-sample beats, `train_net.py:27`) a step is ~250 short launches
and the host cannot issue them as fast as the GPU retires them.  `GraphedTrainStep` captures forward + losswrapper +
backward + the optimiser update once per input shape (torch.cuda.CUDAGraph on the stream the C ABI launches into) and replays
it: inputs are copied into static buffers, and the only per-step host decisions -- the two Standin lead choices
(reference model_nefnet.py:154,156, drawn from Python's `random` in the reference's order) and the dropout seed --
travel through device words that the kernels read at run time.  Same arithmetic as the eager path.  `cfg.DATA.noise`: the
per-sample noise row is one more static input, added to the prediction inside the loss kernels (ops.loss_fwd / loss_bwd, noise=).
`cfg.SOLVER.seg_weights`, `ssim_factor`, `slope_factor`, `corr_factor`: the launches of the terms that are on sit behind them in the same
graph, in the order and on the loss row that network.loss.losses.LossPlan lays out (per term its forward, then its backward), on the same
static rois and noise buffer; their weights, factors and other scalars are config constants, frozen into the capture.

One graph (with its own static input buffers) is kept per input shape, so a final partial batch or alternating shapes
replay instead of re-capturing; the flat parameter / gradient / momentum buffers are shared by all of them and survive
every re-capture (shape change); the learning rate lives in a device word the captured update launch reads, so a scheduler step costs
one small copy and no re-capture.  With a fused optimiser (solver.optim_scheduler: FusedSGD, FusedAdam) the graph steps that
optimiser's own flat buffers through its `_device_update`.  `state_dict()` / `load_state_dict()` carry the momentum buffer
for checkpoints.

Data parallel (world > 1): the step is captured as TWO graphs cut at the early-bucket point of the backward pass; the all-reduce
of the bucket that is final there runs between the replays, under the second graph (`_capture_split`; NEF_GRAPH_SPLIT=0 keeps one
graph and one exposed all-reduce).

Gradient accumulation (the optimiser's accum_steps = K > 1): the per-shape graphs hold forward, backward and the accumulating flatten
(ops.flatten_into(accumulate_dev=): a device word says "assign" on the first micro-batch of a window and "add" on the later ones, so every
micro-batch replays the same graph and shapes share the window); the taint word, the all-reduces, the clip and the update are issued
eagerly behind the window's last replay -- a handful of launches the host queues while the device is still inside the replay, with
the window's own gscale, which a captured update would have frozen.  The window position is the optimiser's (`_acc_n`), so eager and
replayed micro-batches mix.  K == 1: nothing of this runs.

The per-update learning-rate schedule (the optimiser's lr_schedule): `_device_update` reads the optimiser's own rate word and issues the
single-wave nef_lr_sched launch behind the update -- inside the graph where the update is (single process), behind the all-reduces where
it is issued eagerly (data parallel, accumulation).  The rate changes from replay to replay with no host write between them; the
schedule's numbers are among the frozen scalars.  The stepper with private buffers (optimizer=None) has no schedule.

Several target views per step (cfg.SOLVER.train_views; the call signature does not change, the shapes decide): a `q_theta` of
[Q, B, 2] with a target of [Q, B, 1, L] selects engine.forward's multi-view form -- one graph per (shape, Q), its slot holding static
[Q, B, 2] angles, [Q, B, 1, L] targets and, for the cropped SSIM term, the rois tiled once per view, all staged outside the graph with
the other inputs.  The sums over views are ops.copy_many launches inside the graph; both capture forms are otherwise as above.

Input-lead augmentation (cfg.DATA.aug_*; augment.py): every shape slot owns one more static [B, V, L] buffer, and ops.augment from the
staged inputs into it is the FIRST launch of the captured forward -- it reads the step's seed through the `seed_dev` word the dropout
epilogues read, so every replay (every micro-batch of an accumulation window; once per multi-view step) draws its own corruption with no
host write of its own.  Off: no buffer, no launch.

Lead masks (cfg.MODEL.lead_mask, with DATA.aug_lead_drop): every shape slot owns a static uint8 [B, V] buffer, filled by
ops.augment_mask directly behind the captured ops.augment from the same host word and `seed_dev`, and handed to engine.forward, whose
head then averages and picks among the leads the corruption left (the backward finds the mask in the saved state).  Two library
launches in the graph, no torch kernel, no host write between replays.  Off: no buffer, no launch, today's graph.

The step's own noise row (cfg.DATA.device_noise; device_noise.py): the slot's static noise buffer is [Rw, 1, L] -- one row per (view,
sample), also for Q >= 2, whose rois are then tiled per view whatever the plan needs -- and ops.noise_row from the static target and rois
fills it directly in front of ops.loss_fwd, at device_noise.site_word() + `seed_dev`: every replay draws its own row, the eager step's at
the same step seed, with no staged copy and no `noise=` from the caller.  Off: no buffer, no launch.
"""
import random

import torch
from . import _env
import torch.distributed as dist

from . import engine, ops


class GraphedTrainStep:
    def __init__(self, model, cfg, lr=None, momentum=0.9, optimizer=None):
        """`optimizer`: a fused optimiser of solver.optim_scheduler (FusedSGD, FusedAdam) over model.parameters() -- the graph then
        steps THAT optimiser's flat parameter / state buffers through its `_device_update` (so checkpoints, a learning-rate scheduler
        and eager steps in between see one state) and takes its scalars from its parameter group; without it the stepper owns its
        buffers and runs momentum SGD (lr / momentum arguments)."""
        self.model, self.cfg = model, cfg
        # cfg.DATA.noise (reference solver.py:185-186): every shape slot owns a static [B, 1, L] noise buffer, staged with the other inputs
        # and added inside the loss kernels; off: no buffer, no copy
        # cfg.DATA.device_noise (device_noise.py): the buffer is [Rw, 1, L], one row per (view, sample), and a captured ops.noise_row on the
        # static target and rois fills it in front of the loss launches -- nothing is staged, the caller hands no noise.  Both keys: ValueError
        from . import device_noise as _device_noise
        self.device_noise = _device_noise.on(cfg)
        self.use_noise = bool(cfg.DATA.noise) or self.device_noise
        self.noise = None
        self.rois_q = None       # multi-view steps whose plan needs rois (a cropped term, segment weights): the rois tiled Q times
        # the terms behind the four of ops.loss_fwd: their launches behind the loss launches, one more element of the loss row per tail term
        from .network.loss.losses import LossPlan
        self.plan = LossPlan.from_cfg(cfg)
        self.seg_weights = self.plan.seg_weights      # None, or the seven weights of the reconstruction term's positions
        # cfg.DATA.aug_*: every shape slot owns a static [B, V, L] buffer the captured ops.augment writes and the forward reads; None: neither
        from . import augment as _augment
        self.augment = _augment.from_cfg(cfg)
        self.data_aug = None
        # cfg.MODEL.lead_mask: every shape slot owns a static uint8 [B, V] mask the captured ops.augment_mask writes and the head reads
        self.lead_mask_on = self.augment is not None and _augment.lead_mask_on(cfg)
        self.lead_mask = None
        self.optimizer = optimizer
        if optimizer is not None:
            if len(optimizer.param_groups) != 1 or not hasattr(optimizer, "_device_update"):
                raise NotImplementedError("the graphed step drives a fused optimiser (FusedSGD, FusedAdam) with one parameter group")
            g0 = optimizer.param_groups[0]
            lr, momentum = g0["lr"], g0.get("momentum", momentum)
        self.lr = float(cfg.SOLVER.lr if lr is None else lr)
        self.mu = float(momentum)
        self.factors = tuple(float(f) for f in cfg.SOLVER.loss_factor)
        self.reg_l2 = {"l1_loss": False, "l2_loss": True}[cfg.SOLVER.reg_loss]
        u = cfg.SOLVER.loss_using
        self.use_mask = (1 if 1 in u else 0) | (2 if 2 in u else 0) | (4 if 3 in u else 0)
        self.slots = {}          # input shape -> static input buffers + captured graph
        self.flat_p = self.flat_g = self.flat_buf = None
        self.opt_flat = None     # the optimiser's flat buffers (optimizer mode)
        self.live = None
        self.choice_dev = None
        self.lr_dev = None
        self.acc_dev = None      # accum_steps > 1: the int32 device word the captured flatten reads (0: assign, 1: add)
        self._acc_word = None    # ... and what it holds
        self.calls = 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # dp: the step sums its gradients through torch.distributed.  True for more than one rank -- and for a ONE-rank group under the
        # NEF_DIST_FORCE test hook, so that the collectives between the two graph replays run on the real backend (RCCL) of a one-GPU box
        from . import parallel as _par
        self.dp = self.world > 1 or (dist.is_available() and dist.is_initialized() and _par._hook("NEF_DIST_FORCE") == "1")
        # data parallel: capture the step as two graphs with the early gradient bucket's all-reduce between them (_capture_split)
        self.split_capture = _env.get("NEF_GRAPH_SPLIT", "1") != "0"
        if optimizer is not None:
            self._captured = self._frozen()     # frozen into the captured launches: a change re-captures
        # bench.py --dry-collective: a parallel.DryCollective standing in for dist.all_reduce on a one-GPU box (set `dp` with it)
        self.dry = None

    def _all_reduce(self, t, async_op=False):
        if self.dry is not None:
            return self.dry(t, async_op)
        return dist.all_reduce(t, async_op=async_op)

    # -------------------------------------------------------------------------------------------------
    def _flatten(self, live):
        """Parameters become views of one flat buffer.  Done once: the live-parameter set does not depend on the input
        shape, so later captures reuse the buffers -- and with them the momentum."""
        named = dict(self.model.named_parameters())
        if self.optimizer is not None:
            # the optimiser's own flat buffers (its _build: parameters become views of fl["p"], the views of its state buffers -- FusedSGD's
            # momentum fl["buf"], FusedAdam's moments fl["m"] / fl["v"] -- live in optimizer.state): nothing to copy, nothing to keep in sync
            fl = self.optimizer._current(0, [named[k] for k in live])
            self.live = live
            self.opt_flat = fl
            self.flat_p, self.flat_g, self.flat_buf, self.flat_g_all = fl["p"], fl["g"], fl.get("buf"), fl["g_all"]
            return
        if self.live == live and self.flat_p is not None and all(
                named[k].data.data_ptr() >= self.flat_p.data_ptr() and
                named[k].data.data_ptr() < self.flat_p.data_ptr() + 4 * self.flat_p.numel() for k in live):
            return
        old_buf, old_live = self.flat_buf, self.live
        self.live = live
        n = sum(named[k].numel() for k in live)
        dev = self.data.device
        self.flat_p = torch.empty(n, device=dev, dtype=torch.float32)
        from .solver.optim_scheduler import GRAD_HDR
        self.flat_g_all = torch.zeros(n + GRAD_HDR, device=dev, dtype=torch.float32)      # [header: taint word + 3 zeros | gradients] (FusedSGD._build)
        self.flat_g = self.flat_g_all[GRAD_HDR:]
        self.flat_buf = torch.zeros(n, device=dev, dtype=torch.float32)
        if old_buf is not None and old_live == live:       # parameters were re-pointed from outside: keep the momentum
            self.flat_buf.copy_(old_buf)
        off = 0
        for k in live:
            p = named[k]
            m = p.numel()
            self.flat_p[off:off + m].copy_(p.data.reshape(-1))
            old_ptr = p.data.data_ptr()
            p.data = self.flat_p[off:off + m].view_as(p.data)       # parameters become views of the flat buffer
            ops.amax_move(old_ptr, p.data.data_ptr())
            off += m

    def _fwd_bwd(self):
        m = self.model
        P = {k: v.detach() for k, v in m.named_parameters()}
        drop = engine.DropCfg(True, m.dropout_p, m.dropout_masks, seed=0, seed_dev=self.seed_dev)
        data = self.data
        if self.augment is not None:
            # the step's first launch: the corrupted leads into the slot's buffer, at host word + seed_dev = the eager step's seed word
            from . import augment as _augment
            data = ops.augment(self.data, self.rois, self.augment, seed=_augment.site_word(), seed_dev=self.seed_dev, out=self.data_aug)
        mask_kw = {}
        if self.lead_mask_on:
            # ... and directly behind it the mask of the leads it zeroed, from the same two seed words
            ops.augment_mask(self.data.shape[0], self.data.shape[1], self.augment.lead_drop, seed=_augment.site_word(),
                             seed_dev=self.seed_dev, out=self.lead_mask)
            mask_kw = dict(lead_mask=self.lead_mask)
        with ops.amax_scope((m._nef_scope, True)):        # the train-mode call sites of the model (Model_nefnet._engine_fwd)
            outs, sv = engine.forward(P, dict(m.named_buffers()), data, self.in_theta, self.q_theta, self.rois,
                                      phase="train", training=True, drop=drop, lead_choice=self.choice_dev, save=True,
                                      status=self.status, **mask_kw)
            o, p_, l_ = (t.contiguous() for t in outs)
            if self.device_noise:
                # this step's noise row from its own target rows, at host word + seed_dev = the eager step's seed word
                from . import device_noise as _device_noise
                ops.noise_row(self.target, self.rois if self.rois_q is None else self.rois_q, seed=_device_noise.site_word(),
                              seed_dev=self.seed_dev, out=self.noise)
            ops.loss_fwd(o, p_, l_, self.target, self.factors, self.reg_l2, self.use_mask, out=self.losses, noise=self.noise)
            g3 = ops.loss_bwd(o, p_, l_, self.target, None, self.factors, self.reg_l2, self.use_mask, noise=self.noise)
            rois = self.rois if self.rois_q is None else self.rois_q      # (multi-view: the rows are the Q * B (view, sample) pairs)
            for step in self.plan:
                step.fwd(o, self.target, self.losses, rois, self.noise)
                step.bwd(o, self.target, g3[0], rois, self.noise)
            return engine.backward(P, sv, g3)

    def _frozen(self):
        """The optimiser's scalars that the captured launches freeze: those of its update and -- single process, where the clip launches
        sit inside the graph -- its max_grad_norm (data parallel they are issued behind the all-reduces, outside the graphs)."""
        opt = self.optimizer
        return opt._captured_scalars(opt.param_groups[0]) + (() if self.dp else (float(opt.max_grad_norm),)) + (
            (int(opt.accum_steps),) if opt.accum_steps > 1 else ())      # (what the graphs hold differs between K == 1 and K > 1)

    @property
    def accum(self):
        """Micro-batches per update: the optimiser's accum_steps (the stepper with private buffers does not accumulate)."""
        return getattr(self.optimizer, "accum_steps", 1)

    def _into_flat(self, tensors, out):
        """This backward pass's gradients into (a slice of) the flat gradient buffer: assigned, or -- accumulating -- assigned or added as
        the window word says when the launch runs."""
        if self.accum > 1:
            ops.flatten_into(tensors, out, accumulate_dev=self.acc_dev)
        else:
            ops.flatten_into(tensors, out)

    def _clip(self):
        """The optimiser's global gradient-norm clipping (its own clip_stats), between the summed gradients and the update; the stepper
        with private buffers does not clip."""
        if self.optimizer is not None and self.optimizer.max_grad_norm > 0:
            self.optimizer._clip(self.opt_flat, 1.0 / self.world)

    def _update(self):
        # the learning rate travels through a device word (a captured launch freezes its scalars): a scheduler step updates the word,
        # nothing is re-captured
        if self.optimizer is not None:
            self.optimizer._device_update(self.opt_flat, self.optimizer.param_groups[0], 1.0 / self.world, skip=self.flat_g_all[:1],
                                          lr_dev=self.lr_dev)
            return
        ops.sgd_momentum(self.flat_p, self.flat_g, self.flat_buf, self.lr, self.mu, 1.0 / self.world, False,
                         skip=self.flat_g_all[:1], lr_dev=self.lr_dev)

    def _body(self):
        grads = self._fwd_bwd()
        self._into_flat([grads[k] for k in self.live], self.flat_g)
        if self.accum > 1:
            return                             # taint word, clip and update: once per window, behind its last replay (_accum_replay)
        ops.h2_taint(self.flat_g_all[:1])      # this step's clamped split-fp16 launches: the update is skipped (on every rank)
        if not self.dp:
            self._clip()
            self._update()

    def _capture_split(self):
        """Data parallel: the step as TWO graphs, cut where engine.backward would start the early gradient bucket (everything
        behind the per-lead encoder: a suffix of the parameter order, 71 % of the bytes at 3 leads).  Between the two replays the
        suffix bucket's all-reduce is started on a side stream and runs under the second graph -- the encoder blocks' backward
        pass, ~10 ms at configs[1] -- so that only the encoder bucket (+ the taint word in front of it) is summed behind the
        replay: the overlap the eager path has had since round 3 (parallel.early_reduce), bit for bit the same buffer."""
        import gc
        gA, gB = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        info = {}

        def hook(P, grads, side):
            side.join()                                      # nothing forked may be open when a capture ends
            early = [k for k in self.live if grads.get(k) is not None]
            k0 = len(self.live) - len(early)
            if self.live[k0:] != early:
                raise RuntimeError("early gradient bucket is not a suffix of the live parameters")
            named = dict(self.model.named_parameters())
            info["k0"], info["split"] = k0, sum(named[k].numel() for k in self.live[:k0])
            self._into_flat([grads[k] for k in early], self.flat_g[info["split"]:])
            gA.capture_end()
            gB.capture_begin(pool=gA.pool())

        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            gA.capture_begin()
            engine.EARLY_HOOK = hook
            try:
                grads = self._fwd_bwd()
            finally:
                engine.EARLY_HOOK = None
            if "split" not in info:
                raise RuntimeError("engine.backward never reached its early-bucket point")
            if info["k0"]:
                self._into_flat([grads[k] for k in self.live[:info["k0"]]], self.flat_g[:info["split"]])
            if self.accum == 1:                # (accumulating: the taint word is taken once per window, behind its last replay)
                ops.h2_taint(self.flat_g_all[:1])
            gB.capture_end()
        torch.cuda.current_stream().wait_stream(cap)
        self._comm = getattr(self, "_comm", None) or torch.cuda.Stream()
        return (gA, gB, info["split"])

    def _state_tensors(self):
        """Everything the update writes: the parameters and the optimiser state (momentum; Adam's moments and step word)."""
        if self.opt_flat is None:
            return [self.flat_p, self.flat_buf]
        return [self.flat_p] + [v for k, v in self.opt_flat.items() if k not in ("ids", "params", "p", "g", "g_all")]

    def _use(self, slot):
        self.data, self.in_theta, self.q_theta, self.rois, self.target = (slot[k] for k in
                                                                          ("data", "in_theta", "q_theta", "rois", "target"))
        self.noise = slot.get("noise")
        self.rois_q = slot.get("rois_q")
        self.data_aug = slot.get("data_aug")
        self.lead_mask = slot.get("lead_mask")

    def _build(self, data, in_theta, q_theta, rois, target, noise=None):
        dev = data.device
        # static input buffers: contiguous whatever the caller's strides are (a sharded loader hands out slices)
        slot = dict(data=torch.empty(data.shape, device=dev, dtype=torch.float32),
                    in_theta=torch.empty(in_theta.shape, device=dev, dtype=torch.float32),
                    q_theta=torch.empty(q_theta.shape, device=dev, dtype=torch.float32),
                    rois=torch.empty(rois.shape, device=dev, dtype=torch.int64),
                    target=torch.empty(data.shape[0], 1, data.shape[2], device=dev, dtype=torch.float32))
        if q_theta.dim() == 3:
            # SOLVER.train_views: q_theta [Q, B, 2] selects the multi-view step (engine.forward) -- the targets are [Q, B, 1, L], and the
            # SSIM term's rows are the Q * B (view, sample) pairs, cropped by the rois tiled once per view
            Q = q_theta.shape[0]
            if self.use_noise and not self.device_noise:
                raise ValueError("DATA.noise with SOLVER.train_views >= 2: the batch carries noise for the target lead only")
            slot["target"] = torch.empty(Q, data.shape[0], 1, data.shape[2], device=dev, dtype=torch.float32)
            self.plan.check_rows(Q * data.shape[0], views=Q)
            if self.plan.needs_rois or self.device_noise:      # (the noise row's quiet segment is read per (view, sample) row too)
                slot["rois_q"] = torch.empty(Q * rois.shape[0], rois.shape[1], rois.shape[2], device=dev, dtype=torch.int64)
        if self.device_noise:
            slot["noise"] = torch.empty(slot["target"].numel() // data.shape[2], 1, data.shape[2], device=dev, dtype=torch.float32)
        elif self.use_noise:
            slot["noise"] = torch.empty(data.shape[0], 1, data.shape[2], device=dev, dtype=torch.float32)
        if self.augment is not None:
            slot["data_aug"] = torch.empty(data.shape, device=dev, dtype=torch.float32)
        if self.lead_mask_on:
            slot["lead_mask"] = torch.empty(data.shape[0], data.shape[1], device=dev, dtype=torch.uint8)
        self._use(slot)
        if self.choice_dev is None:
            self.choice_dev = torch.zeros(2, device=dev, dtype=torch.int32)
            self.seed_dev = torch.zeros(1, device=dev, dtype=torch.int64)
            self.status = torch.zeros(1, device=dev, dtype=torch.int32)
            self.losses = torch.zeros(self.plan.row_len, device=dev, dtype=torch.float32)
            self.lr_dev = torch.full((1,), self.lr, device=dev, dtype=torch.float32)
        if self.accum > 1 and self.acc_dev is None:
            self.acc_dev, self._acc_word = torch.zeros(1, device=dev, dtype=torch.int32), 0
        # the probe runs THIS step's inputs, Standin choices and dropout seed (drawn by __call__ before it builds): the split-fp16
        # convs measure their operands in it, and what they measure must be what the eager path measures on the same step
        self._stage(data, in_theta, q_theta, rois, target, noise, draw=False)
        self.model.train()
        # eager probe (no update): which parameters are live, and every kernel variant gets its one-time setup
        saved = {k: v.clone() for k, v in self.model.named_buffers()}
        # ... and no history either: the probe rolls and re-measures the operand magnitudes of the split-fp16 call sites; the sites
        # that existed before it get back what they held, so the step that follows rolls them exactly once -- as the eager path and
        # an already captured shape do.  (Without this a stepper restored from a checkpoint rolled twice on its first step and was
        # not bit-identical to the uninterrupted run; a fresh run is unaffected: rolling the same pair twice is rolling it once.)
        amax0 = ops.amax_snapshot(dev)
        grads = self._fwd_bwd()
        ops.amax_restore(dev, amax0)
        if self.dp:                          # the eager probe may have started an early gradient bucket: retire it
            from . import parallel
            pend = parallel.take_early()
            if pend is not None:
                pend["work"].wait()
        self._flatten([k for k, _ in self.model.named_parameters() if grads.get(k) is not None])
        for k, v in self.model.named_buffers():
            v.copy_(saved[k])
        if self.optimizer is not None and self.optimizer.max_grad_norm > 0:
            self.optimizer._clip_ready(dev)      # the stats words exist before the capture: a tensor made inside it would belong to the graph
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        saved = {k: v.clone() for k, v in self.model.named_buffers()}
        state = self._state_tensors()
        saved_state = [t.clone() for t in state]
        if self.dp and self.split_capture:
            graph = self._capture_split()
        else:
            with torch.cuda.graph(graph):
                self._body()
        # capture does not execute, but keep state exactly as before the capture regardless
        for k, v in self.model.named_buffers():
            v.copy_(saved[k])
        for t, t0 in zip(state, saved_state):
            t.copy_(t0)
        slot["graph"] = graph
        # The graph bakes in the pointers of every scratch buffer its launches used (ops.workspace, incl. the side
        # stream's, which the eager probe allocated from the general pool).  ops.workspace() REPLACES a buffer when a later
        # probe of a larger shape outgrows it; holding the buffers here keeps the replaced ones alive for as long as this
        # graph can be replayed.
        slot["workspaces"] = list(ops._WS.values())
        return slot

    def _draw(self):
        """This step's host decisions: Python `random` consumed exactly twice, z1 choice first (model_nefnet.py:154,156)."""
        V = self.model.lead_num
        self.calls += 1
        self._draws = (random.randint(0, V - 1), random.randint(0, V - 1))

    def _stage(self, data, in_theta, q_theta, rois, target, noise=None, draw=True):
        self.data.copy_(data, non_blocking=True)
        self.in_theta.copy_(in_theta, non_blocking=True)
        self.q_theta.copy_(q_theta, non_blocking=True)
        self.rois.copy_(rois, non_blocking=True)
        if self.rois_q is not None:
            self.rois_q.view((-1,) + tuple(self.rois.shape)).copy_(self.rois.unsqueeze(0).expand(self.rois_q.shape[0] // self.rois.shape[0], -1, -1, -1))
        self.target.copy_(target.reshape(self.target.shape), non_blocking=True)
        if self.noise is not None and not self.device_noise:
            self.noise.copy_(noise.reshape(self.noise.shape), non_blocking=True)
        if draw:
            self._draw()
        rank = dist.get_rank() if self.world > 1 else 0
        # same ingredients as the eager path (model_nefnet.py: initial seed + call counter + epoch + rank): a resumed run
        # (Solver sets model.dropout_epoch; `calls` travels in state_dict) does not replay the masks of step 1
        seed = (torch.initial_seed() + self.calls + int(getattr(self.model, "dropout_epoch", 0)) * 0x1000003
                + rank * 0x9E3779B1) & 0x7FFFFFFFFFFF
        c1, c2 = getattr(self, "_draws", (0, 0))
        # one asynchronous launch carrying the three values as kernel arguments (rounds 1-5: two BLOCKING host-to-device copies,
        # which made the host wait for the previous step's replay before it could stage this one)
        from . import _lib
        _lib.check(_lib.load().nef_step_words(self.choice_dev.data_ptr(), self.seed_dev.data_ptr(), int(c1), int(c2), int(seed),
                                              torch.cuda.current_stream().cuda_stream), "nef_step_words")

    # -------------------------------------------------------------------------------------------------
    def set_lr(self, lr):
        """The captured SGD launch reads its learning rate from a device word: a new value is one small copy, no re-capture."""
        if float(lr) != self.lr:
            self.lr = float(lr)
            if getattr(self, "lr_dev", None) is not None:
                self.lr_dev.fill_(self.lr)

    def flush(self):
        """Close an incomplete accumulation window (the optimiser's flush(): taint word, all-reduce, clip and update on the micro-batches
        summed so far); nothing to do on an empty window, with accum_steps == 1 or without an optimiser."""
        if self.optimizer is not None:
            self.optimizer.flush()

    def _accum_replay(self, slot):
        """One micro-batch of an accumulation window: the window word, the replay (data parallel: both graphs, with NO collective), and
        behind the window's last micro-batch the taint word, the all-reduces (the suffix bucket under graph B, the encoder bucket with the
        header behind it), the clip and the update -- issued eagerly, with gscale = 1 / (world * micro-batches)."""
        opt = self.optimizer
        word = 1 if opt._acc_n else 0
        if word != self._acc_word:
            self.acc_dev.fill_(word)
            self._acc_word = word
        last = opt._acc_n + 1 >= opt.accum_steps
        split = isinstance(slot["graph"], tuple)
        if not self.dp:
            slot["graph"].replay()
        elif not last:
            for g in (slot["graph"][:2] if split else (slot["graph"],)):
                g.replay()
        else:
            from . import parallel
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if parallel.TIMING is not None else None
            if split:
                gA, gB, cut = slot["graph"]
                gA.replay()
                cur = torch.cuda.current_stream()
                self._comm.wait_stream(cur)
                with torch.cuda.stream(self._comm):        # the window's suffix bucket travels while graph B runs
                    work = self._all_reduce(self.flat_g[cut:], async_op=True)
                gB.replay()
                ops.h2_taint(self.flat_g_all[:1])          # the clamps of every micro-batch of the window
                if ev is not None:
                    ev[0].record()
                self._all_reduce(self.flat_g_all[:self.flat_g_all.numel() - self.flat_g.numel() + cut])
                work.wait()
                cur.wait_stream(self._comm)
            else:
                slot["graph"].replay()
                ops.h2_taint(self.flat_g_all[:1])
                if ev is not None:
                    ev[0].record()
                self._all_reduce(self.flat_g_all)
            if ev is not None:
                ev[1].record()
                parallel.TIMING.append(ev)
        opt._acc_groups = (0,)
        opt._acc_n += 1
        if last:
            opt._close_window(taint=not self.dp, reduce=False)
        return self.losses

    def state_dict(self):
        """The optimiser state of the graphed path: the flat momentum buffer and the parameter order it refers to."""
        return {"lr": self.lr, "momentum": self.mu, "live": list(self.live or []), "calls": int(self.calls),
                "momentum_buffer": None if self.flat_buf is None else self.flat_buf.detach().cpu().clone()}

    def load_state_dict(self, sd):
        self.set_lr(sd["lr"])
        self.mu = float(sd["momentum"])
        self.calls = int(sd.get("calls", 0))        # the dropout seed's step counter
        self._pending_momentum = (list(sd["live"]), sd["momentum_buffer"])
        if self.flat_buf is not None:
            self._restore_momentum()

    def _restore_momentum(self):
        pend = getattr(self, "_pending_momentum", None)
        if pend is None or pend[1] is None:
            return
        live, buf = pend
        if live != self.live or buf.numel() != self.flat_buf.numel():
            raise ValueError("momentum buffer does not match this model's live parameters")
        self.flat_buf.copy_(buf.to(self.flat_buf.device))
        self._pending_momentum = None

    def __call__(self, data, in_theta, q_theta, rois, target, noise=None):
        """One train step; returns the device tensor [loss, f0*l1, f1*l2, f2*l3] + one element per tail term of `self.plan` that is on
        (valid in stream order; `loss` includes them all).  `noise`: the batch's [B, L] or [B, 1, L] noise rows, required when
        cfg.DATA.noise is set and ignored when it is not (as the reference ignores meta['noise'] then; cfg.DATA.device_noise: the step
        makes its own)."""
        self.model._check_inputs(data, rois)       # what Model_nefnet.forward rejects (float rois, L % 4, CPU tensors) is rejected here too
        if self.use_noise and not self.device_noise and noise is None:
            raise ValueError("cfg.DATA.noise is set: the step needs this batch's noise")
        if self.optimizer is not None:
            g = self.optimizer.param_groups[0]
            cap = self._frozen()
            if cap != self._captured:                          # (momentum; Adam's betas / eps / weight_decay; max_grad_norm: re-capture)
                self._captured = cap
                self.mu = float(g.get("momentum", self.mu))
                self.slots.clear()
            self.set_lr(g["lr"])                               # a scheduler stepped: the device word follows, nothing is re-captured
            # the per-update schedule (optimizer.lr_schedule): the captured update reads the optimiser's rate word and the captured
            # nef_lr_sched launch behind it writes the next rate -- nothing to do here unless the host changed the base rate
            self.optimizer._sched_sync()
            fl = self.optimizer._flat.get(0)
            if self.flat_p is not None and (fl is None or fl["p"] is not self.flat_p):   # e.g. optimizer.load_state_dict
                self.slots.clear()
        gen = ops.amax_generation(data.device)
        if getattr(self, "_amax_gen", gen) != gen:        # the split-fp16 site table started over: captured launches hold stale slots
            self.slots.clear()
        self._amax_gen = gen
        if getattr(self, "_scope", None) != self.model._nef_scope:       # the model loaded other weights: its split-fp16 call sites
            self._scope = self.model._nef_scope                            # start over (ops.amax_scope), and the captures hold the old slots
            self.slots.clear()
        self._draw()
        shape = (tuple(data.shape), tuple(in_theta.shape)) + ((q_theta.shape[0],) if q_theta.dim() == 3 else ())      # one graph per (shape, Q)
        slot = self.slots.get(shape)
        if slot is None:
            slot = self.slots[shape] = self._build(data, in_theta, q_theta, rois, target, noise)
            self._restore_momentum()
        self._use(slot)
        self._stage(data, in_theta, q_theta, rois, target, noise, draw=False)
        if self.accum > 1:
            return self._accum_replay(slot)
        if not self.dp:
            slot["graph"].replay()
            return self.losses
        from . import parallel
        timing = parallel.TIMING is not None       # bench.py: HIP events around what the launching stream waits for
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if timing else None
        if isinstance(slot["graph"], tuple):
            gA, gB, split = slot["graph"]
            gA.replay()
            cur = torch.cuda.current_stream()
            self._comm.wait_stream(cur)
            with torch.cuda.stream(self._comm):        # the suffix bucket travels while graph B (the encoder's backward pass) runs
                work = self._all_reduce(self.flat_g[split:], async_op=True)
            gB.replay()
            if ev is not None:
                ev[0].record()
            self._all_reduce(self.flat_g_all[:self.flat_g_all.numel() - self.flat_g.numel() + split])       # the encoder bucket, the header (taint word) in front of it
            work.wait()
            cur.wait_stream(self._comm)
        else:
            slot["graph"].replay()
            if ev is not None:
                ev[0].record()
            self._all_reduce(self.flat_g_all)                  # one fully exposed all-reduce (NEF_GRAPH_SPLIT=0)
        if ev is not None:
            ev[1].record()
            parallel.TIMING.append(ev)
        self._clip()
        self._update()
        return self.losses
