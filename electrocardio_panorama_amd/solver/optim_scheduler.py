"""Optimiser / scheduler factory of reference codes/solver/optim_scheduler.py:5-18.

'sgd' returns FusedSGD: torch.optim.SGD(lr, momentum=0.9) semantics, but one HIP launch over a flat
parameter buffer, and -- when torch.distributed is initialised -- one RCCL all-reduce of the flat
gradient buffer per step (data-parallel training, one process per GPU).
'adam' returns FusedAdam: torch.optim.Adam(lr) semantics on the same flat-buffer machinery (one nef_adam launch).
'adamw' returns FusedAdamW: torch.optim.AdamW.  SOLVER.weight_decay reaches all three (sgd, adam: L2, added to the gradient; adamw:
decoupled), SOLVER.nesterov the first, and SOLVER.no_decay exempts tensors by name inside the one flat launch (decay_runs).
SOLVER.ema_decay keeps an exponential moving average of the flat parameters inside that same launch (nef_update_ema): ema_state_dict,
load_ema_state_dict and the ema_weights() context are its surface.
'lars' / 'lamb' return FusedLARS / FusedLAMB: the layer-wise trust ratios of large-batch training on the same machinery (nef_update_trust:
one norm pair per parameter tensor by a deterministic segmented reduction, then the update), with SOLVER.trust_coef, SOLVER.trust_eps and
SOLVER.trust_exempt (tensors whose ratio stays 1).
SOLVER.accum_steps = K > 1 makes every fused optimiser accumulate: step() sums p.grad into the flat gradient buffer (nef_flatten_acc) and its
K-th call -- or flush() on an incomplete window -- takes the taint word, all-reduces, clips and updates once, on the mean over the window.
SOLVER.warmup_updates / SOLVER.lr_shape put a per-update learning-rate schedule behind every fused optimiser (LrSchedule, lr_factor): the
update reads its rate from a device word, and one single-wave launch behind it (nef_lr_sched) advances the device-side count of APPLIED
updates and writes base * m(t) for the next one -- no host work per update, a skipped step moves neither.  get_lr_scheduler then wraps
the per-epoch scheduler in ScheduledLR, whose state dict carries the count.
DataParallelAdam (torch Adam behind a separate all-reduce) is kept as the unfused comparison."""
import contextlib
import fnmatch
import math
from collections import OrderedDict

import torch
import torch.distributed as dist
from torch.optim import Adam
from torch.optim.lr_scheduler import StepLR, MultiStepLR

from .. import ops, parallel
from ..parallel import reduce_flat_grads


# The flat gradient buffer starts with a 4-word header (16 bytes: word 0 = the taint word of ops.h2_taint, words 1..3 zero) so that
# the gradients behind it, the encoder bucket's all-reduce (header + bucket) and the SGD kernel's reads stay 16-byte aligned.
GRAD_HDR = 4
MAX_RUNS = 256      # NEF_UPDATE_MAX_RUNS (include/nefnet_hip.h): runs of one nef_update launch


def decay_runs(names, sizes, patterns):
    """The decay run table of nef_update for tensors laid out one behind the other: `names[i]` (None: unnamed, never exempt) holds
    `sizes[i]` elements and is exempt from weight decay -- multiplier 0 -- when it matches one of the fnmatch `patterns`, else it decays
    in full (multiplier 1).  Neighbours with equal multipliers merge into one run.  Returns (ends, muls): the exclusive end of every run
    in flat order and its multiplier; two empty lists when nothing is exempt (no table: multiplier 1 everywhere)."""
    ends, muls, off = [], [], 0
    for name, k in zip(names, sizes):
        if k <= 0:
            continue
        mul = 0.0 if name is not None and any(fnmatch.fnmatchcase(name, pat) for pat in patterns) else 1.0
        off += int(k)
        if muls and muls[-1] == mul:
            ends[-1] = off
        else:
            ends.append(off)
            muls.append(mul)
    if all(m == 1.0 for m in muls):
        return [], []
    return ends, muls


MAX_SEGS = 256      # NEF_TRUST_MAX_SEGS (include/nefnet_hip.h): segments of one nef_update_trust call


def trust_segments(names, sizes, no_decay, trust_exempt):
    """The segment table of nef_update_trust for tensors laid out one behind the other: one segment per non-empty tensor, nothing
    merged (a trust ratio belongs to ONE tensor).  `names[i]` (None: unnamed, never exempt from anything) holds `sizes[i]` elements; its
    decay multiplier is 0 when it matches one of the fnmatch patterns `no_decay`, else 1, and it adapts (1) unless it matches one of
    `trust_exempt` (0: its ratio is 1).  Returns (ends, wd_muls, adapts): the exclusive end of every segment in flat order and its two
    numbers."""
    ends, wd_muls, adapts, off = [], [], [], 0
    for name, k in zip(names, sizes):
        if k <= 0:
            continue
        off += int(k)
        ends.append(off)
        wd_muls.append(0.0 if name is not None and any(fnmatch.fnmatchcase(name, pat) for pat in no_decay) else 1.0)
        adapts.append(0.0 if name is not None and any(fnmatch.fnmatchcase(name, pat) for pat in trust_exempt) else 1.0)
    return ends, wd_muls, adapts


LR_SHAPES = ('none', 'const', 'cosine', 'poly')


def lr_factor(t, warmup_updates=0, warmup_start=0.01, lr_shape='const', total_updates=0, lr_floor=0.0, poly_power=1.0):
    """m(t) of the per-update schedule in Python floats (fp64), in the operation order of the device's lr_sched_factor
    (csrc/elementwise.hip): the host restatement the tests pin to torch's LinearLR / CosineAnnealingLR / PolynomialLR and compare the
    kernel against.  `t`: updates applied so far (the first update uses m(0)).  t < W: s + (1 - s) * t / W.  Behind the warm-up, with
    x = clamp((t - W) / max(1, N - W), 0, 1): 'const' (and 'none') 1; 'cosine' f + (1 - f) * (1 + cos(pi * x)) / 2; 'poly'
    f + (1 - f) * (1 - x)^p -- the end value is kept for t >= N."""
    t, W, N = max(int(t), 0), int(warmup_updates), int(total_updates)
    s, f, p = float(warmup_start), float(lr_floor), float(poly_power)
    if t < W:
        return s + (1.0 - s) * float(t) / float(W)
    if lr_shape in ('none', 'const'):
        return 1.0
    x = min(max(float(t - W) / float(max(1, N - W)), 0.0), 1.0)
    if lr_shape == 'cosine':
        return f + (1.0 - f) * (1.0 + math.cos(math.pi * x)) / 2.0
    if lr_shape == 'poly':
        return f + (1.0 - f) * (1.0 - x) ** p
    raise ValueError(f"Invalid lr_shape value: {lr_shape!r}")


class LrSchedule:
    """The validated numbers of the per-update schedule (SOLVER.warmup_updates, warmup_start, lr_shape, total_updates, lr_floor,
    poly_power).  `on`: warmup_updates > 0 or lr_shape != 'none'; 'none' with a warm-up behaves as 'const'.  total_updates may be
    assigned later (Solver.train derives it before the first step); the optimiser re-evaluates its rate word when a number changed."""

    def __init__(self, warmup_updates=0, warmup_start=0.01, lr_shape='none', total_updates=0, lr_floor=0.0, poly_power=1.0):
        for key, v in (("warmup_updates", warmup_updates), ("total_updates", total_updates)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"Invalid {key} value: {v!r}")
        if lr_shape not in LR_SHAPES:
            raise ValueError(f"Invalid lr_shape value: {lr_shape!r} (one of {', '.join(LR_SHAPES)})")
        for key, v in (("warmup_start", warmup_start), ("lr_floor", lr_floor)):
            if isinstance(v, (bool, str)) or not 0.0 <= float(v) <= 1.0:      # (NaN fails the comparison too)
                raise ValueError(f"Invalid {key} value: {v!r}")
        if isinstance(poly_power, (bool, str)) or not 0.0 < float(poly_power) < math.inf:
            raise ValueError(f"Invalid poly_power value: {poly_power!r}")
        self.warmup_updates, self.total_updates = warmup_updates, total_updates
        self.warmup_start, self.lr_floor, self.poly_power = float(warmup_start), float(lr_floor), float(poly_power)
        self.lr_shape = lr_shape

    @classmethod
    def from_cfg(cls, cfg):
        S = cfg.SOLVER      # (.get: configs written before the keys existed)
        return cls(S.get('warmup_updates', 0), S.get('warmup_start', 0.01), S.get('lr_shape', 'none'), S.get('total_updates', 0),
                       S.get('lr_floor', 0.0), S.get('poly_power', 1.0))

    @property
    def on(self):
        return self.warmup_updates > 0 or self.lr_shape != 'none'

    def kwargs(self):
        """The keyword arguments of ops.lr_sched / lr_factor's keywords under ops' names."""
        return dict(shape='const' if self.lr_shape == 'none' else self.lr_shape, warmup_updates=self.warmup_updates,
                    warmup_start=self.warmup_start, total_updates=self.total_updates, lr_floor=self.lr_floor, poly_power=self.poly_power)

    def scalars(self):
        k = self.kwargs()
        return (k["shape"], k["warmup_updates"], k["warmup_start"], k["total_updates"], k["lr_floor"], k["poly_power"])

    def state_dict(self):
        return dict(warmup_updates=self.warmup_updates, warmup_start=self.warmup_start, lr_shape=self.lr_shape,
                    total_updates=self.total_updates, lr_floor=self.lr_floor, poly_power=self.poly_power)

    def factor(self, t):
        return lr_factor(t, **self.state_dict())


class _FusedFlat(torch.optim.Optimizer):
    """Flat-buffer machinery of the fused optimisers: the live parameters of a group become views of one flat fp32 buffer, the
    per-element state (`_SLOTS`: flat key -> torch state key) views of flat buffers of the same layout, and a step is ONE
    device-update launch (`_device_update`) over them -- behind, in data-parallel runs, the flat gradient all-reduce that consumes
    engine.backward's early bucket (`_reduce`).  The same `_device_update` is what GraphedTrainStep captures.

    A tainted step (a split-fp16 launch met non-finite data, on any rank) leaves parameters and optimiser state untouched; the
    BatchNorm running statistics its forward pass already updated are NOT rolled back (DESIGN.md 3.0 "Range")."""
    _SLOTS = ()

    def __init__(self, params, defaults, max_grad_norm=0.0, no_decay=(), ema_decay=0.0, ema_warmup=False, accum_steps=1, lr_schedule=None):
        super().__init__(params, defaults)
        # the per-update learning-rate schedule (LrSchedule; None or one that is not `on`: off -- no word, no launch, lr travels as it
        # did).  On: every _device_update reads its rate from the group's device word (eagerly as well) and the nef_lr_sched launch
        # behind it advances the count of applied updates and writes the next rate.  An attribute like max_grad_norm, NOT a param_groups
        # key.  The words live outside `_flat`: they survive a rebuild and load_state_dict, and captured launches keep their addresses
        if lr_schedule is not None and not isinstance(lr_schedule, LrSchedule):
            raise ValueError(f"Invalid lr_schedule value: {lr_schedule!r}")
        self.lr_schedule = lr_schedule
        self._sched = {}             # group index -> dict(t int64 word, base fp64 word, lr fp32 word, host: what the lr word was evaluated for)
        self._sched_pending = None   # set_lr_updates() before the words exist: the count they start from
        # gradient accumulation: step() folds p.grad into the flat gradient buffer (the first micro-batch of a window assigns, the later
        # ones add: ops.flatten_into(accumulate=)) and only its accum_steps-th call takes the taint word, all-reduces, clips and updates,
        # with gscale = 1 / (world * accum_steps); flush() closes an incomplete window.  1 = off: step() is what it was.  An attribute like
        # max_grad_norm, NOT a param_groups key.  The window position lives here, so eager and replayed micro-batches share a window
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
            raise ValueError(f"Invalid accum_steps value: {accum_steps!r}")
        self.accum_steps = accum_steps
        self._acc_n = 0          # micro-batches summed into the open window (0: no window is open)
        self._acc_groups = ()    # the parameter groups that window covers
        # an exponential moving average of the parameters, kept by the update launch itself (ops.update_*(ema=)): e += (1 - d_t) * (p - e)
        # after every update that is not skipped, d_t = ema_decay or (ema_warmup) min(ema_decay, (1 + t) / (10 + t)) over the t completed
        # EMA updates.  0 = off: no buffer, no other launch.  Attributes like max_grad_norm, NOT param_groups keys
        if not 0.0 <= float(ema_decay) < 1.0:      # (NaN fails the comparison too)
            raise ValueError(f"Invalid ema_decay value: {ema_decay}")
        self.ema_decay = float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._ema_pending = None     # load_ema_state_dict: {"model": name -> tensor, "n_averaged"} until the flat buffers are built
        # fnmatch patterns on a parameter's `_nef_name` (Model_nefnet: its state_dict key): a match is exempt from weight decay.  An
        # attribute like max_grad_norm, NOT a param_groups key; read when the flat buffers are built
        if isinstance(no_decay, str):
            no_decay = (no_decay,)
        self.no_decay = tuple(str(pat) for pat in no_decay)
        self._flat = {}      # group index -> dict(ids, params, p, g_all, g, one flat buffer per _SLOTS key)
        # global gradient-norm clipping (ops.grad_clip on the mean gradient; 0 = off, inf = measure only).  An attribute, NOT a
        # param_groups key: the state dict stays in torch's format
        if not float(max_grad_norm) >= 0.0:      # (NaN fails the comparison too)
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm}")
        self.max_grad_norm = float(max_grad_norm)
        self._clip_stats = None      # 4 device words [norm, coefficient, steps clipped, steps with a non-finite norm]: made at first use
        if accum_steps == 1:                    # (accumulating: one all-reduce per window, no early bucket)
            parallel.enable_early_reduce()      # this optimiser consumes engine.backward's early gradient bucket (see _reduce)

    def _build(self, gi, live):
        n = sum(p.numel() for p in live)
        dev = live[0].device
        old = self._flat.get(gi)
        # the averages of the parameters that survive a rebuild, cut out of the old flat buffer (as the state slots are carried in state[p])
        old_ema, off = {}, 0
        for p in (old["params"] if old is not None and "ema" in old else ()):
            old_ema[id(p)] = old["ema"][off:off + p.numel()]
            off += p.numel()
        flat_p = torch.empty(n, device=dev, dtype=torch.float32)
        slots = {fk: torch.zeros(n, device=dev, dtype=torch.float32) for fk, _ in self._SLOTS}
        off = 0
        for p in live:
            k = p.numel()
            flat_p[off:off + k].copy_(p.data.reshape(-1))
            old_ptr = p.data.data_ptr()
            p.data = flat_p[off:off + k].view_as(p.data)          # parameters become views of the flat buffer
            ops.amax_move(old_ptr, p.data.data_ptr())
            st = self.state[p]
            for fk, sk in self._SLOTS:
                if sk in st and st[sk] is not None:
                    slots[fk][off:off + k].copy_(st[sk].reshape(-1))
                st[sk] = slots[fk][off:off + k].view_as(p.data)
            off += k
        # gradients: [header (taint word, 3 zero words) | n gradients] -- the word in front (ops.h2_taint: clamps of this step's
        # split-fp16 launches) is summed by the same all-reduce as the gradients, so a clamp on any rank makes every rank skip the update
        g_all = torch.zeros(n + GRAD_HDR, device=dev, dtype=torch.float32)
        self._flat[gi] = dict(ids=[id(p) for p in live], params=live, p=flat_p, g_all=g_all, g=g_all[GRAD_HDR:], **slots)
        # the decay run table over this layout (device tensors: the update launch reads them); nothing exempt: no table, no key
        ends, muls = decay_runs([getattr(p, "_nef_name", None) for p in live], [p.numel() for p in live], self.no_decay)
        if len(ends) > MAX_RUNS:
            raise ValueError(f"no_decay splits the flat parameters into {len(ends)} runs; one update launch takes {MAX_RUNS}")
        if ends:
            self._flat[gi]["run_end"] = torch.tensor(ends, device=dev, dtype=torch.int64)
            self._flat[gi]["run_mul"] = torch.tensor(muls, device=dev, dtype=torch.float32)
        if self.ema_decay > 0:
            # the average starts as a copy of the parameters (timm's ModelEmaV2); what a rebuild or a checkpoint carries replaces it
            ema = flat_p.clone()
            ema_n = old["ema_n"].clone() if old_ema else torch.zeros(1, device=dev, dtype=torch.float32)
            off = 0
            for p in live:
                if id(p) in old_ema:
                    ema[off:off + p.numel()].copy_(old_ema[id(p)])
                off += p.numel()
            self._flat[gi]["ema"], self._flat[gi]["ema_n"] = ema, ema_n
            if self._ema_pending is not None:
                self._import_ema(self._flat[gi], self._ema_pending, skip=old_ema)
                if len(self.param_groups) == 1:      # (more groups: step() drops it behind the last one)
                    self._ema_pending = None

    @staticmethod
    def _runs(fl):
        return (fl["run_end"], fl["run_mul"]) if "run_end" in fl else None

    @staticmethod
    def _import_ema(fl, pend, skip=()):
        """The loaded average `pend` (load_ema_state_dict) into the flat buffers `fl`, by parameter name; parameters in `skip` (ids:
        they carried their average over a rebuild) keep theirs, and so does the count when there are any."""
        off = 0
        for p in fl["params"]:
            k, name = p.numel(), getattr(p, "_nef_name", None)
            if id(p) not in skip and name in pend["model"]:
                src = pend["model"][name]
                if src.numel() != k:
                    raise ValueError(f"the loaded EMA of {name} has {src.numel()} elements, the parameter {k}")
                fl["ema"][off:off + k].copy_(src.reshape(-1))
            off += k
        if not skip:
            fl["ema_n"].fill_(float(pend["n_averaged"]))

    def _ema(self, fl):
        """The `ema=` argument of ops.update_* for these flat buffers; None when the average is off."""
        return (fl["ema"], fl["ema_n"], self.ema_decay, self.ema_warmup) if self.ema_decay > 0 else None

    def _ema_scalars(self):
        """The part of `_captured_scalars` every fused optimiser shares: a captured update freezes the decay and the warm-up flag (the
        count of EMA updates lives on the device: a replay needs nothing), and the learning-rate schedule's numbers when it is on."""
        return (float(self.ema_decay), bool(self.ema_warmup)) + self._sched_scalars()

    def ema_state_dict(self, model):
        """The averaged model for a checkpoint: {"decay", "warmup", "n_averaged", "model"}; "model" has exactly the keys of
        `model.state_dict()` -- the parameters the flat buffers cover hold their average, every other entry (parameters that never had a
        gradient, BatchNorm statistics and the other buffers) the live tensor -- so `model.load_state_dict(sd["model"])` gives the
        averaged model anywhere.  One synchronisation (the count), at checkpoint time only."""
        avg, n_avg = {}, 0.0
        if self._ema_pending is not None:          # loaded, not yet imported (no step since)
            n_avg = float(self._ema_pending["n_averaged"])
        for fl in self._flat.values():
            if "ema" not in fl:
                continue
            n_avg, off = float(fl["ema_n"].item()), 0
            for p in fl["params"]:
                avg[id(p)] = fl["ema"][off:off + p.numel()].view_as(p.data)
                off += p.numel()
        out = OrderedDict(model.state_dict())
        for name, p in model.named_parameters():
            if id(p) in avg:
                out[name] = avg[id(p)].detach().clone()
            elif self._ema_pending is not None and getattr(p, "_nef_name", None) in self._ema_pending["model"]:
                out[name] = self._ema_pending["model"][p._nef_name].detach().clone().view_as(p.data)
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "n_averaged": n_avg, "model": out}

    def load_ema_state_dict(self, sd):
        """What ema_state_dict() returned.  The tensors are kept per parameter name (the parameters' `_nef_name`) and imported when the
        flat buffers are built -- the next step: `load_state_dict` drops them -- or, where they exist, at once.  The decay and the
        warm-up flag stay this optimiser's own; with the average off nothing is kept."""
        if not self.ema_decay > 0:
            return
        pend = {"model": {(k[7:] if k.startswith("module.") else k): v.detach() for k, v in sd["model"].items()},
                "n_averaged": float(sd.get("n_averaged", 0.0))}
        built = [fl for fl in self._flat.values() if "ema" in fl]
        for fl in built:
            self._import_ema(fl, pend)
        self._ema_pending = None if built else pend

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the model's parameters ARE the averaged ones (evaluation, export): the CONTENTS of fl["p"] and fl["ema"] are
        exchanged and exchanged back on exit -- contents, not pointers, because captured graphs and the split-fp16 call sites are keyed
        by address.  Plain torch copies through a temporary (this is outside the step).  Nothing happens before the first step or with
        the average off."""
        def swap():
            for fl in self._flat.values():
                if "ema" in fl:
                    tmp = fl["p"].clone()
                    fl["p"].copy_(fl["ema"])
                    fl["ema"].copy_(tmp)
            ops._PREPACKED.clear()      # an operand packed from the weights of the other side must not be served
        swap()
        try:
            yield self
        finally:
            swap()

    def decay_summary(self):
        """One line per built parameter group: the exempt live tensors and how many elements decay; None before the first step."""
        out = []
        for gi, fl in sorted(self._flat.items()):
            wd = float(self.param_groups[gi].get("weight_decay", 0.0))
            names = [getattr(p, "_nef_name", None) for p in fl["params"]]
            ends, muls = decay_runs(names, [p.numel() for p in fl["params"]], self.no_decay)
            n = fl["p"].numel()
            decayed = n if not ends else sum(e - b for b, e, m in zip([0] + ends[:-1], ends, muls) if m)
            exempt = [k for k in names if k is not None and any(fnmatch.fnmatchcase(k, pat) for pat in self.no_decay)]
            out.append("weight_decay {:g} on {} of {} elements ({} run(s)); exempt: {}".format(
                wd, decayed if wd else 0, n, max(len(ends), 1), ", ".join(exempt) if exempt else "none"))
        return "\n".join(out) if out else None

    def _current(self, gi, live):
        """The flat buffers of group `gi` for these live parameters, (re)built when the set changed or a parameter was re-pointed."""
        fl = self._flat.get(gi)
        if fl is None or fl["ids"] != [id(p) for p in live] or ("ema" in fl) != (self.ema_decay > 0) or any(
                p.data.data_ptr() < fl["p"].data_ptr() or
                p.data.data_ptr() >= fl["p"].data_ptr() + fl["p"].numel() * 4 for p in live):
            if self._acc_n:      # a rebuild would drop the partial sum of the open window
                raise RuntimeError(f"the live parameters of group {gi} changed or were re-pointed after {self._acc_n} of {self.accum_steps} "
                                   "accumulated micro-batches; flush() the window first")
            self._build(gi, live)
            fl = self._flat[gi]
        if self._sched_on:
            self._sched_words(gi, fl["p"].device)      # made (and brought up to date) before anything can be captured
        return fl

    # ---------------------------------------------------------------- the per-update learning-rate schedule
    @property
    def _sched_on(self):
        return self.lr_schedule is not None and self.lr_schedule.on

    def _sched_scalars(self):
        """The part of `_captured_scalars` the schedule adds: a captured nef_lr_sched launch freezes its shape numbers (off: nothing)."""
        return self.lr_schedule.scalars() if self._sched_on else ()

    def _sched_gi(self, group):
        return next(i for i, g in enumerate(self.param_groups) if g is group)

    def _sched_words(self, gi, device=None):
        """The schedule's device words of group `gi`, made at first use (the count starts at what set_lr_updates left, else 0) and
        brought up to date: when group["lr"] (the per-epoch scheduler), a shape number or the count was changed by the host, the base
        word is refreshed and the rate re-evaluated WITHOUT advancing.  Never inside a capture: _current and GraphedTrainStep.__call__
        come here first."""
        sc, group = self.lr_schedule, self.param_groups[gi]
        w = self._sched.get(gi)
        if w is None:
            # one count for every group: a group built later starts where the others are (a device copy, nothing is read)
            t = next(iter(self._sched.values()))["t"].clone() if self._sched else torch.full(
                (1,), int(self._sched_pending or 0), device=device, dtype=torch.int64)
            w = self._sched[gi] = dict(t=t, base=torch.zeros(1, device=device, dtype=torch.float64),
                                       lr=torch.zeros(1, device=device, dtype=torch.float32), host=None)
            self._sched_pending = None
        key = (float(group["lr"]),) + sc.scalars()
        if w["host"] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the learning-rate schedule's base rate changed inside a graph capture")
            w["base"].fill_(float(group["lr"]))
            ops.lr_sched(w["t"], w["lr"], w["base"], advance=False, **sc.kwargs())
            w["host"] = key
        return w

    def _sched_sync(self):
        """Every existing rate word follows a host change of group["lr"] or of the schedule's numbers (no launch when nothing changed)."""
        if self._sched_on:
            for gi in self._sched:
                self._sched_words(gi)

    def _sched_lr(self, fl, group, lr_dev):
        """The rate word `_device_update` hands to its launch: the schedule's when it is on, else the caller's (None: the scalar)."""
        if not self._sched_on:
            return lr_dev
        return self._sched_words(self._sched_gi(group), fl["p"].device)["lr"]

    def _sched_advance(self, group, skip, flag=None):
        """Behind the update launch: the count advances and the next rate is written, unless the update was not applied (the skip word;
        lars / lamb: the trust flag) -- the words adam_step_kernel / trust_step_kernel decide on."""
        if self._sched_on:
            w = self._sched[self._sched_gi(group)]
            ops.lr_sched(w["t"], w["lr"], w["base"], advance=True, skip=skip, flag=flag, **self.lr_schedule.kwargs())

    def set_lr_updates(self, t):
        """The count of applied updates (a checkpoint's): into the device words where they exist -- the rate is re-evaluated at the next
        use -- else kept until they are made, as `_ema_pending` waits for the flat buffers."""
        t = int(t)
        if t < 0:
            raise ValueError(f"Invalid count of applied updates: {t}")
        self._sched_pending = t
        for w in self._sched.values():
            w["t"].fill_(t)
            w["host"] = None

    def lr_state(self):
        """(t, effective lr) of the first parameter group: the updates applied so far and the rate the next one uses.  One synchronising
        read (none before the first step, where both come from the host's numbers).  Schedule off: (None, group["lr"])."""
        if not self._sched_on:
            return None, float(self.param_groups[0]["lr"])
        if 0 not in self._sched:
            t = int(self._sched_pending or 0)
            return t, float(torch.tensor(float(self.param_groups[0]["lr"]) * self.lr_schedule.factor(t), dtype=torch.float64).float())
        w = self._sched_words(0)
        t, lr = torch.cat([w["t"].double(), w["lr"].double()]).tolist()
        return int(t), lr

    @property
    def clip_stats(self):
        """The 4 device words ops.grad_clip writes for this optimiser; None until a step has clipped (clipping off: never made)."""
        return self._clip_stats

    def _clip_ready(self, device):
        if self._clip_stats is None:
            self._clip_stats = torch.zeros(4, device=device, dtype=torch.float32)

    def _clip(self, fl, gscale):
        """Clip the global norm of the flat gradients `fl["g"]` (summed over the ranks: the norm is that of the mean, the same on every
        rank) in front of `_device_update`; a non-finite norm taints the step."""
        self._clip_ready(fl["g"].device)
        ops.grad_clip(fl["g"], self.max_grad_norm, gscale, self._clip_stats, taint=fl["g_all"][:1])

    def load_state_dict(self, state_dict):
        """The loaded state replaces the flat buffers: drop the flat views so the next step() re-imports them."""
        if self._acc_n:
            raise RuntimeError(f"load_state_dict inside an accumulation window ({self._acc_n} of {self.accum_steps} micro-batches); flush() first")
        super().load_state_dict(state_dict)
        self._flat = {}

    def _captured_scalars(self, group):
        """The scalar arguments of `_device_update` that a captured launch freezes (a change re-captures); lr travels in a device word."""
        raise NotImplementedError

    def _device_update(self, fl, group, gscale, skip=None, lr_dev=None):
        """One update launch over the flat buffers `fl` of `group` (gradients already summed over the ranks: scaled by `gscale`)."""
        raise NotImplementedError

    @staticmethod
    def _reduce(live, flat, world, flat_all=None):
        """Sum of the flat gradient buffer across ranks (RCCL over xGMI).  When engine.backward already started the
        all-reduce of the gradients that were final early (parallel.early_reduce: a SUFFIX of the parameter order --
        everything behind the per-lead encoder), only the encoder bucket is reduced here and the early bucket's result
        is copied in behind it; otherwise one all-reduce of the whole buffer."""
        early = parallel.take_early() if world > 1 else None
        names = [getattr(p, "_nef_name", None) for p in live]
        split = None
        if early is not None:
            k = len(names) - len(early["names"])
            # the bucket is the raw gradient of ONE backward pass: it stands in for p.grad only while p.grad is still that
            # gradient -- a fresh tensor nobody has written to since autograd set it (clip_grad_norm_, loss-scale unscaling or
            # accumulation into an existing .grad bump its version counter; parallel.take_early already dropped a bucket that
            # saw two backward passes)
            if (k >= 0 and names[k:] == early["names"] and [p.numel() for p in live[k:]] == early["sizes"]
                    and all(p.grad._version == 0 for p in live[k:])):
                split = sum(p.numel() for p in live[:k])
        if split is None:
            if early is not None:
                early["work"].wait()          # a bucket that does not line up with this optimiser's parameters: drop it
            ev = None
            if parallel.TIMING is not None and world > 1:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            ops.flatten_into([p.grad for p in live], flat)
            if world > 1:
                dist.all_reduce(flat if flat_all is None else flat_all)      # one RCCL sum all-reduce over xGMI (+ the taint word)
            if ev is not None:
                ev[1].record()
                parallel.TIMING.append(ev)
            return
        k = len(names) - len(early["names"])
        if k:
            ops.flatten_into([p.grad for p in live[:k]], flat[:split])
        ev = None
        if parallel.TIMING is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if flat_all is not None:
            dist.all_reduce(flat_all[:GRAD_HDR + split])       # the encoder bucket, with the header (taint word) in front of it
        elif k:
            dist.all_reduce(flat[:split])
        early["work"].wait()                  # the launching stream now waits for the early bucket's collective
        if ev is not None:
            ev[1].record()
            parallel.TIMING.append(ev)
        flat[split:].copy_(early["flat"])

    @property
    def window_open(self):
        """Whether micro-batches are summed in the flat gradient buffer that no update has consumed yet (accum_steps > 1 only)."""
        return self._acc_n > 0

    def _accumulate(self):
        """step() with accum_steps > 1: this micro-batch's p.grad into the flat gradient buffers -- assigned by the first micro-batch of a
        window, added by the later ones, in call order -- and the window closed behind the accum_steps-th."""
        if self.max_grad_norm > 0 and sum(any(p.grad is not None for p in g["params"]) for g in self.param_groups) > 1:
            raise NotImplementedError("max_grad_norm clips the global norm of ONE parameter group")
        groups = []
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            fl = self._current(gi, live)      # (raises inside a window where it would have to rebuild)
            ops.flatten_into([p.grad for p in live], fl["g"], accumulate=self._acc_n > 0)
            groups.append(gi)
        if not groups:
            return
        if self._acc_n and tuple(groups) != self._acc_groups:
            raise RuntimeError(f"parameter groups {groups} have gradients, the open accumulation window covers {list(self._acc_groups)}")
        early = parallel.take_early() if dist.is_available() and dist.is_initialized() else None
        if early is not None:
            early["work"].wait()      # somebody else opted in: a bucket of ONE backward pass, retired like one that does not line up
        self._acc_groups = tuple(groups)
        self._acc_n += 1
        if self._acc_n >= self.accum_steps:
            self._close_window()

    @torch.no_grad()
    def flush(self):
        """Close an incomplete window: the update on the m < accum_steps micro-batches summed so far, gscale = 1 / (world * m).  Nothing
        happens on an empty window (and with accum_steps == 1, where no window is ever open)."""
        if self._acc_n:
            self._close_window()

    def _close_window(self, taint=True, reduce=True):
        """What step() does behind its flatten, once per window of `_acc_n` micro-batches: the taint word (h2_taint advances its mark only
        when it runs, so this one launch covers every micro-batch), ONE all-reduce of g_all (header included), the clip and the update,
        with gscale = 1 / (world * _acc_n).  GraphedTrainStep passes taint / reduce False where it has issued them itself."""
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        gscale = 1.0 / (world * self._acc_n)
        word = None
        for gi in self._acc_groups:
            fl, group = self._flat[gi], self.param_groups[gi]
            if taint:
                if word is None:
                    ops.h2_taint(fl["g_all"][:1])
                else:
                    fl["g_all"][:1].zero_()
            if reduce and world > 1:
                dist.all_reduce(fl["g_all"])
            if taint:
                if word is None:
                    word = fl["g_all"][:1]
                else:
                    fl["g_all"][:1].copy_(word)       # (already summed over the ranks)
            if self.max_grad_norm > 0:
                self._clip(fl, gscale)
            self._device_update(fl, group, gscale, skip=fl["g_all"][:1])
        ops._PREPACKED.clear()
        self._ema_pending = None
        self._acc_n, self._acc_groups = 0, ()

    @torch.no_grad()
    def step(self, closure=None):
        if self.accum_steps > 1:
            return self._accumulate()
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        taint = None           # ONE taint word per step: h2_taint advances its mark, so later groups reuse the first group's (summed) word
        clip = self.max_grad_norm > 0
        if clip and sum(any(p.grad is not None for p in g["params"]) for g in self.param_groups) > 1:
            raise NotImplementedError("max_grad_norm clips the global norm of ONE parameter group")
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]      # torch skips grad=None
            if not live:
                continue
            fl = self._current(gi, live)
            if taint is None:
                ops.h2_taint(fl["g_all"][:1])      # clamps of this step's split-fp16 launches -> the word in front of the gradients
            else:
                fl["g_all"][:1].zero_()
            self._reduce(live, fl["g"], world, fl["g_all"])
            if taint is None:
                taint = fl["g_all"][:1]
            else:
                fl["g_all"][:1].copy_(taint)       # (already summed over the ranks)
            if clip:
                self._clip(fl, 1.0 / world)
            self._device_update(fl, group, 1.0 / world, skip=fl["g_all"][:1])      # a tainted step is skipped on the device
        # the update wrote the parameters through raw pointers (no version bump): an operand pre-packed from the old weights by a forward
        # pass that no backward consumed (ops.pack_many) must not be served to the next one
        ops._PREPACKED.clear()
        self._ema_pending = None      # a loaded average has been imported by every group that was built
        return None


class FusedSGD(_FusedFlat):
    """torch.optim.SGD semantics (momentum > 0, dampening 0, L2 weight_decay, Nesterov), one launch per parameter group: nef_sgd_momentum
    while the group uses neither decay nor Nesterov nor a no_decay table, nef_update (rule 0) otherwise.  The group carries torch's keys,
    so state_dict() goes both ways with torch.optim.SGD."""
    _SLOTS = (("buf", "momentum_buffer"),)

    def __init__(self, params, lr, momentum=0.9, dampening=0, weight_decay=0, nesterov=False, *, no_decay=(), max_grad_norm=0.0,
                 ema_decay=0.0, ema_warmup=False, accum_steps=1, lr_schedule=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if dampening != 0:      # torch's first step takes buf = grad undamped: that needs a device step word
            raise NotImplementedError("FusedSGD implements dampening=0")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                                      maximize=False, foreach=None, differentiable=False, fused=None),
                         max_grad_norm=max_grad_norm, no_decay=no_decay, ema_decay=ema_decay, ema_warmup=ema_warmup, accum_steps=accum_steps,
                         lr_schedule=lr_schedule)

    @staticmethod
    def _check_group(group):
        if group.get("dampening", 0) != 0 or group.get("maximize"):
            raise NotImplementedError("FusedSGD implements dampening=0, maximize=False")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)

    def _captured_scalars(self, group):      # (.get: a group loaded from a checkpoint written before the keys existed)
        return (float(group["momentum"]), float(group.get("weight_decay", 0.0)), bool(group.get("nesterov", False))) + self._ema_scalars()

    def _device_update(self, fl, group, gscale, skip=None, lr_dev=None):
        # buf starts at zero, so mu*buf + g reproduces torch's first-step "buf = g" exactly
        self._check_group(group)
        mu, wd, nesterov = self._captured_scalars(group)[:3]
        runs, ema = self._runs(fl), self._ema(fl)
        lr_dev = self._sched_lr(fl, group, lr_dev)
        if wd == 0.0 and not nesterov and runs is None and ema is None:
            ops.sgd_momentum(fl["p"], fl["g"], fl["buf"], float(group["lr"]), mu, gscale, False, skip=skip, lr_dev=lr_dev)
        else:
            ops.update_sgd(fl["p"], fl["g"], fl["buf"], float(group["lr"]), mu, gscale, wd, nesterov, runs=runs, skip=skip,
                           lr_dev=lr_dev, ema=ema)
        self._sched_advance(group, skip)


class FusedAdam(_FusedFlat):
    """torch.optim.Adam semantics (amsgrad=False, maximize=False, L2 weight_decay folded into the gradient), one nef_adam launch per
    parameter group.  The state is torch's: state[p] = {"step", "exp_avg", "exp_avg_sq"} with the moments as views of the flat
    buffers, so checkpoints go both ways between this optimiser and torch.optim.Adam / DataParallelAdam.  The step count of a group
    lives in ONE device word (the kernel reads it for the bias corrections and advances it: a captured update stays right on every
    replay); it is imported from the parameters' state["step"] when the flat buffers are built, and state_dict() writes it back into
    each parameter's state["step"] -- one synchronisation, at checkpoint time only.  Between two state_dict() calls state["step"] is
    not kept current."""
    _SLOTS = (("m", "exp_avg"), ("v", "exp_avg_sq"))

    _DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 no_decay=(), max_grad_norm=0.0, ema_decay=0.0, ema_warmup=False, accum_steps=1, lr_schedule=None):
        if amsgrad or maximize:
            raise NotImplementedError(f"{type(self).__name__} implements amsgrad=False, maximize=False")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, self._defaults(lr, (float(betas[0]), float(betas[1])), eps, weight_decay),
                         max_grad_norm=max_grad_norm, no_decay=no_decay, ema_decay=ema_decay, ema_warmup=ema_warmup, accum_steps=accum_steps,
                         lr_schedule=lr_schedule)

    @staticmethod
    def _defaults(lr, betas, eps, weight_decay):
        return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)

    @staticmethod
    def _check_group(group):
        if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
            raise NotImplementedError("FusedAdam implements amsgrad=False, maximize=False, L2 weight_decay")

    def _export_steps(self):
        """The device step words -> state["step"] of every parameter (torch's float32 scalar tensor)."""
        for fl in self._flat.values():
            s = float(fl["step"].item())
            for p in fl["params"]:
                self.state[p]["step"] = torch.tensor(s, dtype=torch.float32)

    def _build(self, gi, live):
        old = self._flat.get(gi)
        if old is not None:         # the old buffers' step word is the current count of their parameters
            s = float(old["step"].item())
            for p in old["params"]:
                self.state[p]["step"] = torch.tensor(s, dtype=torch.float32)
        steps = {}
        for i, p in enumerate(live):
            v = self.state[p].get("step", 0.0)
            steps.setdefault(float(v), []).append(getattr(p, "_nef_name", None) or f"param {i}")
        if len(steps) > 1:
            raise ValueError("FusedAdam keeps one step count per parameter group; the live parameters carry different ones: " +
                             "; ".join(f"step {s:g}: {', '.join(names)}" for s, names in sorted(steps.items())))
        super()._build(gi, live)
        self._flat[gi]["step"] = torch.full((1,), next(iter(steps)), device=live[0].device, dtype=torch.float32)

    def state_dict(self):
        self._export_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)

    def _captured_scalars(self, group):
        b1, b2 = group["betas"]
        return (float(b1), float(b2), float(group["eps"]), float(group["weight_decay"])) + self._ema_scalars()

    def _device_update(self, fl, group, gscale, skip=None, lr_dev=None):
        self._check_group(group)
        b1, b2, eps, wd = self._captured_scalars(group)[:4]
        runs, ema = self._runs(fl), self._ema(fl)
        lr_dev = self._sched_lr(fl, group, lr_dev)
        if not self._DECOUPLED and runs is None and ema is None:
            ops.adam(fl["p"], fl["g"], fl["m"], fl["v"], fl["step"], float(group["lr"]), b1, b2, eps, wd, gscale, skip=skip, lr_dev=lr_dev)
        else:
            ops.update_adam(fl["p"], fl["g"], fl["m"], fl["v"], fl["step"], float(group["lr"]), b1, b2, eps, wd, gscale,
                            decoupled=self._DECOUPLED, runs=runs, skip=skip, lr_dev=lr_dev, ema=ema)
        self._sched_advance(group, skip)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW semantics on FusedAdam's machinery: the decay is decoupled -- p *= 1 - lr * weight_decay in front of Adam's
    update on the undecayed gradient -- and defaults to 1e-2; one nef_update launch (rule 2) per parameter group.  The group carries
    torch's keys (decoupled_weight_decay = True), so state_dict() goes both ways with torch.optim.AdamW."""
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 no_decay=(), max_grad_norm=0.0, ema_decay=0.0, ema_warmup=False, accum_steps=1, lr_schedule=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         no_decay=no_decay, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup, accum_steps=accum_steps,
                         lr_schedule=lr_schedule)

    @staticmethod
    def _defaults(lr, betas, eps, weight_decay):
        return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                    capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)

    @staticmethod
    def _check_group(group):
        if group.get("amsgrad") or group.get("maximize") or not group.get("decoupled_weight_decay", True):
            raise NotImplementedError("FusedAdamW implements amsgrad=False, maximize=False, decoupled weight_decay")


class _TrustMixin:
    """What FusedLARS and FusedLAMB share: the segment table (one segment per live tensor), the ratio table and the stats words of
    ops.update_lars / ops.update_lamb, built with the flat buffers -- before any capture, because a tensor made inside a capture belongs
    to the graph.  `trust_exempt`: fnmatch patterns on a parameter's `_nef_name`, an attribute like no_decay."""

    def _trust_init(self, trust_exempt):
        if isinstance(trust_exempt, str):
            trust_exempt = (trust_exempt,)
        self.trust_exempt = tuple(str(pat) for pat in trust_exempt)
        self._trust_names = {}      # group index -> the segments' names (kept out of _flat: the graphed step clones every tensor in there)

    @staticmethod
    def _check_trust(trust_coef, trust_eps):
        if not 0.0 <= trust_coef:      # (NaN fails the comparison too)
            raise ValueError(f"Invalid trust_coef value: {trust_coef}")
        if not 0.0 <= trust_eps:
            raise ValueError(f"Invalid trust_eps value: {trust_eps}")

    def _build(self, gi, live):
        ends, wd_muls, adapts = trust_segments([getattr(p, "_nef_name", None) for p in live], [p.numel() for p in live], self.no_decay,
                                               self.trust_exempt)
        if len(ends) > MAX_SEGS:
            raise ValueError(f"{len(ends)} live parameter tensors; one trust-ratio update takes {MAX_SEGS} segments")
        super()._build(gi, live)
        fl, dev = self._flat[gi], live[0].device
        fl.pop("run_end", None), fl.pop("run_mul", None)      # the decay multipliers travel per segment
        fl["seg_end"] = torch.tensor(ends, device=dev, dtype=torch.int64)
        fl["seg_wd_mul"] = torch.tensor(wd_muls, device=dev, dtype=torch.float32)
        fl["seg_adapt"] = torch.tensor(adapts, device=dev, dtype=torch.float32)
        fl["ratio"] = torch.ones(len(ends), device=dev, dtype=torch.float32)
        # [smallest, largest ratio over the adapted tensors, steps updated, steps skipped for non-finite norms]
        fl["trust_stats"] = torch.tensor([1.0, 1.0, 0.0, 0.0], device=dev, dtype=torch.float32)
        self._trust_names[gi] = [getattr(p, "_nef_name", None) or f"param {i}" for i, p in enumerate(live) if p.numel() > 0]

    @staticmethod
    def _segs(fl):
        return fl["seg_end"], fl["seg_wd_mul"], fl["seg_adapt"]

    @property
    def trust_stats(self):
        """The 4 device words of the first built group; None before the first step."""
        for _, fl in sorted(self._flat.items()):
            return fl["trust_stats"]
        return None

    def trust_ratios(self):
        """name -> the trust ratio the last updating step applied to that tensor (1.0: exempt, or a zero norm); empty before the first
        step.  One synchronisation, on demand."""
        out = OrderedDict()
        for gi, fl in sorted(self._flat.items()):
            out.update(zip(self._trust_names[gi], (float(q) for q in fl["ratio"].tolist())))
        return out


class FusedLARS(_TrustMixin, FusedSGD):
    """LARS on FusedSGD's machinery (You, Gitman, Ginsburg 2017): momentum SGD whose decayed gradient of every parameter tensor is
    multiplied by q = trust_coef * ||p|| / (||g|| + wd * ||p|| + trust_eps) -- norms per tensor, on the averaged (and clipped) gradient;
    q = 1 for the tensors matching `trust_exempt` and where a norm is zero.  One nef_update_trust call per parameter group.  The state is
    torch.optim.SGD's (momentum_buffer); `trust_coef` and `trust_eps` are group keys."""

    def __init__(self, params, lr, momentum=0.9, dampening=0, weight_decay=0, nesterov=False, trust_coef=1e-3, trust_eps=1e-8, *,
                 no_decay=(), trust_exempt=(), max_grad_norm=0.0, ema_decay=0.0, ema_warmup=False, accum_steps=1, lr_schedule=None):
        self._check_trust(trust_coef, trust_eps)
        self._trust_init(trust_exempt)
        super().__init__(params, lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         no_decay=no_decay, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup, accum_steps=accum_steps,
                         lr_schedule=lr_schedule)
        for group in self.param_groups:
            group.setdefault("trust_coef", float(trust_coef))
            group.setdefault("trust_eps", float(trust_eps))
        self.defaults.update(trust_coef=float(trust_coef), trust_eps=float(trust_eps))

    def _captured_scalars(self, group):
        return super()._captured_scalars(group) + (float(group.get("trust_coef", self.defaults["trust_coef"])),
                                                   float(group.get("trust_eps", self.defaults["trust_eps"])))

    def _device_update(self, fl, group, gscale, skip=None, lr_dev=None):
        self._check_group(group)
        sc = self._captured_scalars(group)
        mu, wd, nesterov = sc[:3]
        coef, teps = sc[-2:]
        self._check_trust(coef, teps)
        lr_dev = self._sched_lr(fl, group, lr_dev)
        flag = ops.update_lars(fl["p"], fl["g"], fl["buf"], float(group["lr"]), mu, gscale, self._segs(fl), fl["ratio"], fl["trust_stats"],
                               trust_coef=coef, trust_eps=teps, weight_decay=wd, nesterov=nesterov, skip=skip, lr_dev=lr_dev, taint=skip,
                               ema=self._ema(fl))
        self._sched_advance(group, skip, flag)


class FusedLAMB(_TrustMixin, FusedAdam):
    """LAMB on FusedAdam's machinery (You et al. 2020): Adam's direction u = m_hat / (sqrt(v_hat) + eps) + wd * p, scaled per parameter
    tensor by q = ||p|| / ||u|| (1 for the tensors matching `trust_exempt` and where a norm is zero): p -= lr * q * u.  One
    nef_update_trust call per parameter group.  The state is torch.optim.Adam's (step, exp_avg, exp_avg_sq); `trust_coef` and `trust_eps`
    are group keys as in FusedLARS (LAMB's ratio uses neither)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, amsgrad=False, trust_coef=1e-3, trust_eps=1e-8, *,
                 maximize=False, no_decay=(), trust_exempt=(), max_grad_norm=0.0, ema_decay=0.0, ema_warmup=False, accum_steps=1, lr_schedule=None):
        self._check_trust(trust_coef, trust_eps)
        self._trust_init(trust_exempt)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         no_decay=no_decay, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup, accum_steps=accum_steps,
                         lr_schedule=lr_schedule)
        for group in self.param_groups:
            group.setdefault("trust_coef", float(trust_coef))
            group.setdefault("trust_eps", float(trust_eps))
        self.defaults.update(trust_coef=float(trust_coef), trust_eps=float(trust_eps))

    def _captured_scalars(self, group):
        return super()._captured_scalars(group) + (float(group.get("trust_coef", self.defaults["trust_coef"])),
                                                   float(group.get("trust_eps", self.defaults["trust_eps"])))

    def _device_update(self, fl, group, gscale, skip=None, lr_dev=None):
        self._check_group(group)
        b1, b2, eps, wd = self._captured_scalars(group)[:4]
        lr_dev = self._sched_lr(fl, group, lr_dev)
        flag = ops.update_lamb(fl["p"], fl["g"], fl["m"], fl["v"], fl["step"], float(group["lr"]), b1, b2, eps, wd, gscale, self._segs(fl),
                               fl["ratio"], fl["trust_stats"], skip=skip, lr_dev=lr_dev, taint=skip, ema=self._ema(fl))
        self._sched_advance(group, skip, flag)


class DataParallelAdam(Adam):
    """torch Adam (the reference's other optimiser choice, optim_scheduler.py:8) whose step first averages the
    gradients over the data-parallel ranks with the same single flat all-reduce FusedSGD uses -- without it the
    ranks' parameters would silently diverge."""

    @torch.no_grad()
    def step(self, closure=None):
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world > 1:
            early = parallel.take_early()          # this optimiser reduces everything itself: retire the early bucket
            if early is not None:
                early["work"].wait()
            live = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
            if live:
                flat = torch.empty(sum(p.numel() for p in live), device=live[0].device, dtype=torch.float32)
                reduce_flat_grads([p.grad for p in live], flat)
                flat.mul_(1.0 / world)
                off = 0
                for p in live:
                    p.grad.copy_(flat[off:off + p.numel()].view_as(p.grad))
                    off += p.numel()
        return super().step(closure)


def get_optimizer(cfg, model_params):
    optim_name = cfg.SOLVER.optim
    clip = float(cfg.SOLVER.get('clip_grad_norm', 0.0))      # (.get: configs written before the key existed)
    wd = float(cfg.SOLVER.get('weight_decay', 0.0))          # sgd, adam: L2 (added to the gradient); adamw: decoupled
    no_decay = tuple(cfg.SOLVER.get('no_decay', None) or ())
    # (what every fused optimiser takes: the weight average and SOLVER.accum_steps, the micro-batches per update)
    ema = dict(ema_decay=float(cfg.SOLVER.get('ema_decay', 0.0)), ema_warmup=bool(cfg.SOLVER.get('ema_warmup', False)),
               accum_steps=cfg.SOLVER.get('accum_steps', 1))
    sched = LrSchedule.from_cfg(cfg)      # (validated whether on or off)
    if sched.on:
        ema["lr_schedule"] = sched        # SOLVER.warmup_updates / lr_shape: the per-update schedule behind the update launch
    if optim_name == 'adam':
        return FusedAdam(model_params, lr=cfg.SOLVER.lr, weight_decay=wd, no_decay=no_decay, max_grad_norm=clip, **ema)
    elif optim_name == 'adamw':
        return FusedAdamW(model_params, lr=cfg.SOLVER.lr, weight_decay=wd, no_decay=no_decay, max_grad_norm=clip, **ema)
    elif optim_name == 'sgd':
        return FusedSGD(model_params, lr=cfg.SOLVER.lr, momentum=0.9, weight_decay=wd, nesterov=bool(cfg.SOLVER.get('nesterov', False)),
                        no_decay=no_decay, max_grad_norm=clip, **ema)
    elif optim_name in ('lars', 'lamb'):
        trust = dict(trust_coef=float(cfg.SOLVER.get('trust_coef', 1e-3)), trust_eps=float(cfg.SOLVER.get('trust_eps', 1e-8)),
                     trust_exempt=tuple(cfg.SOLVER.get('trust_exempt', None) or ()))
        if optim_name == 'lars':
            return FusedLARS(model_params, lr=cfg.SOLVER.lr, momentum=0.9, weight_decay=wd, nesterov=bool(cfg.SOLVER.get('nesterov', False)),
                             no_decay=no_decay, max_grad_norm=clip, **trust, **ema)
        return FusedLAMB(model_params, lr=cfg.SOLVER.lr, weight_decay=wd, no_decay=no_decay, max_grad_norm=clip, **trust, **ema)


class ScheduledLR:
    """What get_lr_scheduler returns with the per-update schedule on: the per-epoch scheduler `inner` (it still sets group["lr"], the
    BASE rate) beside the optimiser's device-side schedule.  step() is the per-epoch scheduler's; get_last_lr() gives the effective
    rate base * m(t) per group.  state_dict() is the inner scheduler's own dict plus one key, "per_update" = {"t", the schedule's
    numbers}: a scheduler of the other kind reads it too (torch's load_state_dict keeps unknown keys as attributes), and a dict without
    the key -- written with the schedule off -- loads here with t = 0."""

    def __init__(self, optimizer, inner):
        if not getattr(optimizer, "_sched_on", False):
            raise ValueError("ScheduledLR needs a fused optimiser whose lr_schedule is on")
        self.optimizer, self.inner = optimizer, inner

    def step(self, *args, **kwargs):
        return self.inner.step(*args, **kwargs)

    def get_last_lr(self):
        opt = self.optimizer
        t, lr = opt.lr_state()
        if len(opt.param_groups) == 1:
            return [lr]
        # (more groups: one count, each group's own base rate -- the host's restatement of the words)
        return [float(torch.tensor(float(g["lr"]) * opt.lr_schedule.factor(t), dtype=torch.float64).float()) for g in opt.param_groups]

    def state_dict(self):
        sd = dict(self.inner.state_dict()) if self.inner is not None else {}
        sd["per_update"] = dict(self.optimizer.lr_schedule.state_dict(), t=int(self.optimizer.lr_state()[0]))
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        per = sd.pop("per_update", None)
        if self.inner is not None:
            self.inner.load_state_dict(sd)
        if per is None:
            print("the checkpoint's scheduler entry carries no count of applied updates (written with the per-update schedule off): "
                  "the schedule starts at t = 0")
            self.optimizer.set_lr_updates(0)
            return
        mine = self.optimizer.lr_schedule.state_dict()
        diff = {k: (per[k], v) for k, v in mine.items() if k in per and per[k] != v and not (k == "total_updates" and 0 in (per[k], v))}
        if diff:
            print("the checkpoint's per-update schedule differs from this run's, which is kept: " +
                  ", ".join(f"{k} {a!r} -> {b!r}" for k, (a, b) in sorted(diff.items())))
        self.optimizer.set_lr_updates(per.get("t", 0))

    def __getattr__(self, name):         # last_epoch, milestones, ...: the per-epoch scheduler's
        if name in ("inner", "optimizer"):
            raise AttributeError(name)
        return getattr(self.inner, name)


def get_lr_scheduler(cfg, optim=None):
    sche_name = cfg.SOLVER.scheduler
    inner = None
    if sche_name == 'steplr':
        inner = StepLR(optim, 50, gamma=0.1)
    elif sche_name == 'MultiStep':
        inner = MultiStepLR(optim, cfg.SOLVER.lr_step, gamma=0.1)
    sched = LrSchedule.from_cfg(cfg)
    if not sched.on:          # exactly what it returned before the keys existed
        return inner
    if not hasattr(optim, "_sched"):
        raise ValueError("SOLVER.warmup_updates / SOLVER.lr_shape need a fused optimiser (SOLVER.optim sgd, adam, adamw, lars or lamb)")
    if not optim._sched_on:
        optim.lr_schedule = sched
    return ScheduledLR(optim, inner)
