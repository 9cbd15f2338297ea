"""Thin tensor-level wrappers over the C ABI (include/nefnet_hip.h).

PyTorch is used only for device memory and streams: every function takes contiguous fp32 (int64 for
ROIs) tensors on a HIP device, allocates the outputs, and enqueues the library call on the current
stream.  Nothing here computes on the host and nothing falls back to torch ops.
"""
import ctypes as C
import contextlib
import itertools
import os
from typing import NamedTuple, Optional

import numpy as np
import torch
from . import _env

from . import _lib

N_SEG, ROI_BINS = 7, 16


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype=torch.float32):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return t


_WS = {}

# bench.py sets this to a list to collect (tag, start_event, end_event) around selected launches; the events are
# recorded on the stream the kernel is launched on, so their difference is that kernel's device time.
PROFILE = None
PROFILE_ONLY = None     # optional predicate(tag): bracket only these launches (every event pair costs ~3 us of GPU idle)
# matrix-core multiplies EXECUTED per algorithmic multiply of a tagged conv launch (tag -> fraction), filled while PROFILE
# is on: 1 direct; K=3: 2/3 through F(2,3), 1/2 through F(4,3) / the transposed F(3,4); K=7: 9/14 forward (F(2,4)+F(2,3)),
# 13/28 backward-data (F(4,4)+F(4,3)) and weight gradient (transposed F(4,4)+F(3,4)), 10/14 for the 3+3+1 forms
EXEC_FRAC = {}
# ... and fp16 matrix-core multiplies executed per algorithmic multiply (the split-fp16 kernels: 3; every other form: 0)
EXEC_FP16 = {}


def _exec_frac(K, form):
    """form: 0 direct, 1 the F(2,.) family, 2 the F(4,.) family (forward / backward-data: nef_conv_args.wino; weight
    gradient: 1 = transposed F(3,2), 2 = the round-2/3 forms ops.conv_bwd_weight calls `wino=4`)."""
    if not form or K == 1:
        return 1.0
    if K == 3:
        return 2.0 / 3.0 if form == 1 else 0.5
    return 9.0 / 14.0 if form == 1 else 13.0 / 28.0


def _timed(tag):
    if PROFILE is None or (PROFILE_ONLY is not None and not PROFILE_ONLY(tag)):
        return None
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    PROFILE.append((tag, s, e))
    s.record()
    return e


def _hbm(name, *tensors):
    """bench.py hook for the HBM-bound passes: the tag carries the launch's ALGORITHMIC bytes (its external inputs and
    outputs, each counted once), so bytes / event time is the pass's achieved bandwidth."""
    if PROFILE is None:
        return None
    return _timed(("hbm", name, sum(t.numel() * t.element_size() for t in tensors if t is not None)))


def _done(ev):
    if ev is not None:
        ev.record()


def workspace(nbytes, device):
    """Caller-owned scratch, grown on demand, reused by stream-ordered calls (one buffer per stream)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    cur = _WS.get(key)
    if cur is None or cur.numel() < nbytes:
        cur = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = cur
    return cur


class SideStream:
    """A second HIP stream for work that is off the critical dependency chain of the backward pass (weight and bias
    gradients are only needed by the optimiser).  The MFMA-bound bwd-weight kernels then overlap with the HBM-bound
    elementwise kernels of the main chain instead of queueing behind them.

    Memory safety without `record_stream` (which makes the caching allocator hoard memory: blocks with pending
    cross-stream uses cannot be recycled, so it keeps reserving new ones): the inputs of a side-stream launch are kept
    referenced here until an event recorded behind that launch has completed, or until `join()` has made the main
    stream wait for the side stream -- in both cases any later reuse of their memory is ordered after the side
    kernel.  Outputs are allocated from the side stream's pool and are only reused by side-stream work of a later
    step, which starts with `wait_stream(main)` and therefore after their last reader."""

    _cache = {}

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device)
        self.pending = []          # (event, tensors kept alive)

    @classmethod
    def get(cls, device):
        key = (device.type, device.index)
        if key not in cls._cache:
            cls._cache[key] = cls(device)
        return cls._cache[key]

    def run(self, fn, *inputs):
        """Run fn() on the side stream once everything enqueued so far on the current stream is done."""
        main = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(main)
        capturing = torch.cuda.is_current_stream_capturing()
        with torch.cuda.stream(self.stream):
            out = fn()
            if not capturing:
                ev = torch.cuda.Event()
                ev.record(self.stream)
        if capturing:
            # inside a hipGraph capture the fork / join become graph edges (the side kernels are parallel branches of the
            # captured step); events cannot be polled there, so the inputs simply stay referenced until join()
            self.pending.append((None, inputs))
            return out
        self.pending.append((ev, inputs))
        while self.pending and self.pending[0][0] is not None and self.pending[0][0].query():
            self.pending.pop(0)
        return out

    def join(self):
        """Make the current stream wait for everything issued on the side stream."""
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        self.pending.clear()


class _Inline:
    """Same interface, everything on the current stream (NEF_SIDE_STREAM=0)."""

    def run(self, fn, *inputs):
        return fn()

    def join(self):
        pass


class GV:
    """Grouped view of an activation: element (b, g, c, t) at base + b*bs + g*gs + c*T + t (in floats)."""
    __slots__ = ("t", "B", "G", "Cg", "T", "bs", "gs", "off")

    def __init__(self, t, B, G, Cg, T, bs, gs, off=0):
        self.t, self.B, self.G, self.Cg, self.T, self.bs, self.gs, self.off = t, B, G, Cg, T, bs, gs, off

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    @staticmethod
    def dense(t, G):
        _chk(t)
        B, Ct, T = t.shape
        return GV(t, B, G, Ct // G, T, Ct * T, (Ct // G) * T, 0)

    @staticmethod
    def half(t, V, which):
        """Channels [which*64, which*64+64) of every lead of a [B, 128V, T] tensor (the z1/z2 split,
        reference codes/network/model_nefnet.py:127-131)."""
        _chk(t)
        B, Ct, T = t.shape
        return GV(t, B, V, 64, T, Ct * T, 128 * T, which * 64 * T)


# ------------------------------------------------------------------ stem
def stem_fwd(x, w):
    L = _lib.load()
    _chk(x), _chk(w)
    B, V, Ln = x.shape
    y = torch.empty(B, 128 * V, Ln // 4, device=x.device, dtype=torch.float32)
    ev = _hbm("stem_fwd", x, y)
    _lib.check(L.nef_stem_fwd(_p(x), _p(w), _p(y), B, V, Ln, _stream()), "nef_stem_fwd")
    _done(ev)
    return y


# Live extents: the convs behind the bias-free stem skip the column tiles that lie in a beat's all-zero tail.  Off: every
# launch goes through the plain entry points, as if no table had been handed over (same bits either way).
_LV = _env.get("NEF_LIVE", "1")
if _LV not in ("0", "1", "fwd"):
    raise ValueError(f"NEF_LIVE={_LV!r}: expected 0, 1 or fwd")
LIVE = _LV != "0"
LIVE_WGRAD = _LV == "1"       # ... the weight gradients too (needs LIVE)
_LIVE_HOST = [None, None]     # (table, its host copy): one read-back per profiled step, for bench.py's executed-work figures
_LIVE_ACC = {}                # tag -> [sum of live-tile fractions, launches] over the launches of ONE profile (PROFILE list)
_LIVE_ACC_OF = [None]         # the PROFILE list _LIVE_ACC belongs to


def live_extent(x):
    """int32 [B, V]: from which position on ops.stem_fwd(x, .)'s output row (b, v) is exactly zero (nef_live_extent).  No host read."""
    L = _lib.load()
    _chk(x)
    B, V, Ln = x.shape
    live = torch.empty(B, V, device=x.device, dtype=torch.int32)
    ev = _hbm("live_extent", x)
    _lib.check(L.nef_live_extent(_p(x), _p(live), B, V, Ln, _stream()), "nef_live_extent")
    _done(ev)
    return live


def _live_note(tag, frac):
    """Executed-work figure of a profiled launch: EXEC_FP16[tag] = 3 x the mean live fraction of the tag's launches in this profile."""
    if _LIVE_ACC_OF[0] is not PROFILE:
        _LIVE_ACC.clear()
        _LIVE_ACC_OF[0] = PROFILE
    acc = _LIVE_ACC.setdefault(tag, [0.0, 0])
    acc[0] += frac
    acc[1] += 1
    EXEC_FP16[tag] = 3.0 * acc[0] / acc[1]


def _live_frac(live, pad, T, tile=256):
    """Mean fraction of `tile`-column tiles a split-fp16 launch with this promise multiplies: tile t0 is live iff t0 < table + addend
    + pad (profiled launches only: the one place a table is read back, once per table, BEFORE the launch's start event)."""
    if _LIVE_HOST[0] is not live[0]:
        _LIVE_HOST[0], _LIVE_HOST[1] = live[0], live[0].to("cpu", torch.int64)
    tps = (T + tile - 1) // tile
    bound = _LIVE_HOST[1] + int(live[1]) + pad
    return float(((bound + tile - 1) // tile).clamp(0, tps).double().mean()) / tps


def stem_bwd_weight(x, w, gy, live=None):
    """`live`: ops.live_extent(x) -- the matrix-core kernel then stops every row at its extent (same bits; part of ops.LIVE, and like the
    other weight gradients of ops.LIVE_WGRAD)."""
    L = _lib.load()
    _chk(x), _chk(w), _chk(gy)
    B, V, Ln = x.shape
    gw = torch.empty_like(w)
    n = L.nef_stem_bwd_ws_bytes(V)
    ws = workspace(n, x.device)
    ev = _hbm("stem_bwd_weight", x, gy)
    if live is not None and LIVE and LIVE_WGRAD:
        assert live.shape == (B, V) and live.dtype == torch.int32
        _lib.check(L.nef_stem_bwd_weight_live(_p(x), _p(w), _p(gy), _p(gw), _p(ws), n, B, V, Ln, _p(live), _stream()), "nef_stem_bwd_weight_live")
    else:
        _lib.check(L.nef_stem_bwd_weight(_p(x), _p(w), _p(gy), _p(gw), _p(ws), n, B, V, Ln, _stream()), "nef_stem_bwd_weight")
    _done(ev)
    return gw


# ------------------------------------------------------------------ grouped conv
# K = 3 convs through Winograd F(2,3), K = 7 convs through F(2,4) + F(2,3) on the taps split 4 + 3 (conv_mfma.hip:
# conv_wino_kernel; "F(2,3)" below stands for this F(2,.) family) wherever a whole output tile of one
# sample exists; NEF_WINOGRAD=0 keeps every conv on the direct kernel.
_WV = _env.get("NEF_WINOGRAD", "4")
WINOGRAD = _WV != "0"
# Forward / backward-data form where the caller allows the larger tile (`f4=True`: the decoder convs): 2 = F(4,3)
# (default), 1 = F(2,3) everywhere (NEF_WINOGRAD=2).  The encoder-side convs always take F(2,3), for two measured reasons:
# (1) their inputs end in the all-zero tail of a beat; F(2,3) reproduces the reference's exact 0.0 there (every product
# feeding an output only sees that output's own receptive field), F(4,3) leaves +-1e-9 of residue whose sign then
# opens ReLU gates the reference keeps closed (705 of 512 k decisions in one block); (2) with that repaired by an
# exact-zero fix-up in the kernel (built, 255 VGPRs), the larger rounding of F(4,3) still moved the stem's weights --
# a heavily cancelling gradient -- by 3.7e-4 over the 3-step reference trajectory (bar 2e-4), and the fixed-up kernel
# was no faster than F(2,3) (1.31 vs 1.33 ms on the K=7 conv).
WINO_FWD = 1 if _WV in ("1", "2") else 2
# Winograd weight gradients (nef_bww_args form 4): K=3 through the transposed F(3,4), K=7 with the taps split 4 + 3 over
# two launches (transposed F(4,4) + F(3,4)).
WINO_BW4 = _WV not in ("1", "2")
WINO_BW7 = _WV not in ("1", "2")


# Split-fp16 direct convolution (csrc/conv_h2.hip, conv args wino = 3): both fp32 operands split into two fp16 terms each (22-23 bits kept),
# three fp16 matrix instructions per 16 channels and tap, fp32 accumulation -- fp32-class results at 3/16 of the fp32 matrix
# instructions' pipe time.  NEF_H2=0 keeps the fp32 Winograd forms; NEF_H2=1 takes it wherever the shape allows
# (128-channel output tiles, 16-channel input chunks, T even and >= 128; K = 7 without an input prologue).
H2 = _env.get("NEF_H2", "1") == "1"


# Small problems stay on the fp32 kernels: the split-fp16 kernels tile a sample in 256 outputs x 128 (64) channels, and below
# ~one workgroup per CU the half-empty tiles and the per-launch setup cost more than the matrix time they save (reference-native
# batch 32 x L 512: 3.11 ms per captured step with them, 2.72 without).  The engine announces the batch of the pass it is about
# to run (BATCH_HINT); without a hint (bare ops calls) the shape rules alone decide.
BATCH_HINT = None
_H2_MIN_WGS = 256       # fewest workgroups a split-fp16 launch must fill


def _h2_packed(K, T_out, pro=0):
    """Short rows (8 <= T <= 64, T % 4 == 0) of plain K = 1 / K = 3 launches: several samples per tile of conv_h2_kernel
    (csrc/conv_h2.hip, PACK)."""
    return K in (1, 3) and not pro and 8 <= T_out <= 64 and T_out % 4 == 0


def _h2_fills(G, Cout_g, T_out, tile_t, tile_c):
    if BATCH_HINT is None:
        return True
    if T_out < 128:       # packed short rows: (256 + 4) // (T + 4) samples per tile, 64-channel tiles
        spt = (256 + 4) // (T_out + 4)
        return G * ((Cout_g + 63) // 64) * ((BATCH_HINT + spt - 1) // spt) >= _H2_MIN_WGS
    return G * ((Cout_g + tile_c - 1) // tile_c) * BATCH_HINT * ((T_out + tile_t - 1) // tile_t) >= _H2_MIN_WGS


def h2_ok(K, Cin_g, Cout_g, T_out, pro=0):
    return (H2 and (K == 3 or (K in (1, 7) and not pro)) and T_out % 2 == 0 and
            (T_out >= 128 or _h2_packed(K, T_out, pro)) and Cin_g % 16 == 0 and Cout_g % 64 == 0)


# Input magnitudes of the split-fp16 launches, per call site (= per weight tensor and direction): `cur` is what a launch derives
# its power-of-two input scale from, `nxt` is what it max-accumulates its own operand's magnitude into; amax_roll() -- once per
# forward pass -- moves nxt into cur.  A site's FIRST launch runs twice: once to measure, once with the measured scale.  Nothing is
# read back by the host, so the launches stay capturable.
# Range, in ONE place (bench.py and Solver quote these): the scale puts `cur` at [2^8, 2^9); amax_roll follows a
# measurement UP as soon as it exceeds H2_FOLLOW_UP x cur and DOWN only once it is H2_FOLLOW_DOWN x smaller (sticky: repeated
# passes split their operands identically), so the operand a launch meets is below 2^10 as long as it grew less than
# H2_HEADROOM = 2^16 / 2^10 = 64 x since the previous pass.  Beyond that the kernels RESCUE the launch: a workgroup whose tile (weight
# gradient: share) does not fit redoes it with the scale its own data asks for (conv_h2.hip / conv_h2w.hip), so finite operands are
# never clamped; a launch that meets non-finite data (or the opt-in producer / consumer form, which still clamps) counts itself in
# `clamped`, and the train step that contains it is SKIPPED on the device (h2_taint / sgd_momentum).
H2_FOLLOW_UP = 2.0
H2_FOLLOW_DOWN = 64.0
H2_HEADROOM = 64
# Heavy-tail guard (round 6): the format keeps 22-23 bits of an element only down to H2_TAIL_WINDOW = 2^-11 of its tensor's largest
# (one power-of-two scale per tensor).  A call site counts itself in `tail` when more than H2_TAIL_FRAC = 90 % of its operand's
# nonzero elements lie below that line: practically the whole tensor sits outside the full-precision window, and the products of two
# such operands (a weight gradient) lose per-element precision (test_conv_h2_operand_distributions[lognormal]: exp(4 N(0,1)) has
# 99.4 % there; profiles/r06_h2_scale_granularity.md).  There is no sharp line -- the format is fp32-class on the NORM whatever the
# distribution -- and this model's own tensors are not far from it: the worst site of configs[1] (a gradient: a few large entries, a
# long tail) has 74 % of its nonzero elements below the window, carrying 0.26 % of its energy (`h2_tail_worst` in the bench line;
# full-size gradient parity 3.3e-5 on the flat norm, every tensor <= 1e-3).  An amax / rms ratio (the review's suggestion) fires on
# neither: the rms of a heavy-tailed sample is dominated by its largest elements (log-normal: 100-500, not > 2048).  Checked ONCE per
# site, where it measures its operand (its first launch; never inside a captured step); bench.py and Solver report the count
# (h2_tail_sites) -- a model that counts here wants NEF_H2=0, or NEF_H2_TAIL=fp32 below.
# The measurement is a HIP census of the operand as the launch splits it (csrc/h2_tail.hip: the view, the affine + ReLU prologue,
# the channel scale), not of the tensor behind the view.
H2_TAIL_WINDOW = 2.0 ** -11
H2_TAIL_FRAC = 0.9
# What a flagged WEIGHT-GRADIENT site does (NEF_H2_TAIL; tests set the attribute): "warn" (default) only counts it; "fp32" reads its
# census flag on the host once, at its measuring launch (eager, never captured), and routes the site to the direct fp32
# weight-gradient kernel, conv_bwd_weight(h2=False, wino=False) for the same operands, for the site's lifetime (h2_fallback_sites).  Forward and
# backward-data sites keep the split kernels either way.
H2_TAIL_MODES = ("warn", "fp32")
H2_TAIL_MODE = _env.get("NEF_H2_TAIL", "warn")
if H2_TAIL_MODE not in H2_TAIL_MODES:
    raise ValueError(f"NEF_H2_TAIL={H2_TAIL_MODE!r}: expected one of {H2_TAIL_MODES}")
AMAX_SITES = 16384
_AMAX = {}
# A call site = (scope, weight address, direction, role, batch, length).  The scope is the owning model's token
# (Model_nefnet sets it around every engine call; a fresh model or a loaded checkpoint gets a fresh token, so nothing is inherited
# from whatever lived at the same addresses before).  Without a scope (bare engine / ops calls) every launch measures first.
AMAX_SCOPE = None
_SCOPE_IDS = itertools.count(1)


def new_amax_scope():
    return next(_SCOPE_IDS)


@contextlib.contextmanager
def amax_scope(token):
    global AMAX_SCOPE
    prev, AMAX_SCOPE = AMAX_SCOPE, token
    try:
        yield
    finally:
        AMAX_SCOPE = prev


def _amax_state(dev):
    st = _AMAX.get(dev)
    if st is None:
        st = _AMAX[dev] = dict(cur=torch.zeros(AMAX_SITES, device=dev, dtype=torch.float32),
                               nxt=torch.zeros(AMAX_SITES, device=dev, dtype=torch.float32), index={}, ready=set(), used=False, occ={}, n=0,
                               clamped=torch.zeros(1, device=dev, dtype=torch.int32),       # waves that clamped (device total, never reset)
                               mark=torch.zeros(1, device=dev, dtype=torch.int32),          # ... at the last step boundary (h2_taint)
                               skipped=torch.zeros(1, device=dev, dtype=torch.int32),       # train steps skipped because of a clamp
                               tail=torch.zeros(1, device=dev, dtype=torch.int32),          # call sites whose operand is heavy-tailed (H2_TAIL_*)
                               tail_stat=torch.zeros(2, device=dev, dtype=torch.float32),   # diagnostics: largest (count, energy) fraction below the window seen at a site
                               fp32=set(),                                                  # slots of weight-gradient sites routed to the fp32 kernels (H2_TAIL_MODE)
                               seen=0, seen_skipped=0, seen_tail=0, fallback=0, seen_fallback=0)          # ... as of the host's last h2_clamped() / h2_skipped()
    return st


def h2_clamped(reset=True):
    """Waves of split-fp16 launches (sited ones: measuring launches are not counted) that had to clamp an operand element at
    fp16's range since the last call: since round 5 that means NON-FINITE data (finite operands beyond the headroom are rescued
    inside the launch), or the opt-in producer / consumer form, which has no rescue.  Those launches' results are off; a train step
    that contains one is skipped (h2_taint).  Reading synchronises: call it at a logging interval, not per step."""
    n = 0
    for st in _AMAX.values():
        tot = int(st["clamped"].item())
        n += tot - st["seen"]
        if reset:
            st["seen"] = tot
    return n


def h2_skipped(reset=True):
    """Train steps whose parameter update was skipped on the device because a split-fp16 launch of the step clamped (on this or,
    data parallel, on any rank) since the last call.  Synchronises like h2_clamped()."""
    n = 0
    for st in _AMAX.values():
        tot = int(st["skipped"].item())
        n += tot - st["seen_skipped"]
        if reset:
            st["seen_skipped"] = tot
    return n


def h2_tail_sites(reset=True):
    """Split-fp16 call sites whose operand, when the site measured it, had more than H2_TAIL_FRAC of its nonzero elements below
    H2_TAIL_WINDOW x its largest (since the last call).  Synchronises like h2_clamped()."""
    n = 0
    for st in _AMAX.values():
        tot = int(st["tail"].item())
        n += tot - st["seen_tail"]
        if reset:
            st["seen_tail"] = tot
    return n


def h2_fallback_sites(reset=True):
    """Split-fp16 weight-gradient call sites routed to the fp32 kernels (H2_TAIL_MODE = "fp32": their census flagged an operand)
    since the last call.  A host count: nothing synchronises."""
    n = 0
    for st in _AMAX.values():
        n += st["fallback"] - st["seen_fallback"]
        if reset:
            st["seen_fallback"] = st["fallback"]
    return n


def tail_census(xv, amax, in_scale=None, pro=None, site_flag=None, tail_stat=None):
    """nef_h2_tail_census of the operand a split-fp16 launch splits: the GV `xv`, `in_scale` = (tensor, batch stride, group stride)
    and `pro` = (mode, a, b, Bp) as conv() / conv_bwd_weight() get them; `amax` a one-element device tensor (the slot).  Returns the
    record as a 12-word int32 device tensor (census_record() reads it); `site_flag` / `tail_stat`: device words the launch also
    updates.  Two stream-ordered launches, nothing read by the host."""
    L = _lib.load()
    dev = xv.t.device
    rec = torch.zeros(12, device=dev, dtype=torch.int32)
    n = L.nef_h2_tail_census_ws_bytes(xv.B, xv.G, xv.Cg)
    ws = torch.empty(max(n, 8) // 8, device=dev, dtype=torch.float64)
    sc, sc_bs, sc_gs = (None, 0, 0) if in_scale is None else (_p(in_scale[0]), in_scale[1], in_scale[2])
    pm = pro[0] if pro is not None else 0
    pa, pb, pbp = (_p(pro[1]), _p(pro[2]), pro[3]) if pm & 1 else (None, None, 1)
    _lib.check(L.nef_h2_tail_census(xv.ptr, xv.bs, xv.gs, xv.B, xv.G, xv.Cg, xv.T, sc, sc_bs, sc_gs, pa, pb, int(pm), int(pbp),
                                    amax.data_ptr(), H2_TAIL_WINDOW, H2_TAIL_FRAC, _p(ws), ws.numel() * 8, _p(rec), _p(site_flag),
                                    _p(tail_stat), _stream()), "nef_h2_tail_census")
    return rec


def census_record(rec):
    """The host's view of a tail_census() record (synchronises)."""
    r = rec.cpu()
    n = r[0:4].view(torch.int64).tolist()
    e = r[4:8].view(torch.float64).tolist()
    f = r[8:10].view(torch.float32).tolist()
    return dict(n_nonzero=n[0], n_small=n[1], e_small=e[0], e_total=e[1], frac_count=f[0], frac_energy=f[1], flag=int(r[10]))


def _note_tail(st, i, operands):
    """At a site's measuring launch (eager, once per site): slots i, i + 1, .. of `nxt` hold the amax of `operands` -- (GV,
    in_scale, pro) each, as the launch reads them; the census (tail_census) counts the site in `tail` if an operand has more than
    H2_TAIL_FRAC of its nonzero elements below H2_TAIL_WINDOW x that amax, and keeps the largest fractions in `tail_stat`.  Returns
    the site's device flag word; nothing read by the host."""
    flag = torch.zeros(1, device=st["nxt"].device, dtype=torch.int32)
    for k, (xv, in_scale, pro) in enumerate(operands):
        if xv is None or xv.B * xv.G * xv.Cg * xv.T == 0:
            continue
        tail_census(xv, st["nxt"][i + k:i + k + 1], in_scale, pro, site_flag=flag, tail_stat=st["tail_stat"])
    st["tail"] += flag
    return flag


def h2_tail_stats():
    """Diagnostics: the largest (count fraction, energy fraction) below the window any site's operand had when it was measured."""
    out = [0.0, 0.0]
    for st in _AMAX.values():
        v = st["tail_stat"].tolist()
        out = [max(out[0], v[0]), max(out[1], v[1])]
    return out


def h2_taint(out):
    """out[0] (a one-element fp32 device view, e.g. the word in front of the flat gradient buffer) = the number of waves that clamped
    since the previous call (or h2_rebase); stream-ordered, capturable.  The optimiser passes the word to sgd_momentum(skip=...).
    ONE call per optimiser step: the call advances the mark, so a second parameter group must reuse the first one's word."""
    st = _amax_state(out.device)
    _lib.check(_lib.load().nef_h2_taint(_p(st["clamped"]), _p(st["mark"]), _p(out), _stream()), "nef_h2_taint")


def h2_rebase(device=None):
    """The taint mark := the clamp counter (stream-ordered): clamps counted so far -- a test-phase forward, gen_ecg between train
    steps -- are not charged to the next train step.  Solver calls it where it has just read (and judged) the counters."""
    for dev, st in _AMAX.items():
        if device is None or torch.device(device) == dev:
            st["mark"].copy_(st["clamped"])


def _amax_index(st, site, n):
    """First of the `n` consecutive magnitude slots of a call site (allocated on first use)."""
    i = st["index"].get(site)
    if i is None:
        if st["n"] + n > AMAX_SITES:       # models come and go (tests): start over
            assert not torch.cuda.is_current_stream_capturing()
            st["index"].clear(), st["ready"].clear(), st["fp32"].clear(), st["cur"].zero_(), st["nxt"].zero_()
            st["n"] = 0
            st["gen"] = st.get("gen", 0) + 1       # captured graphs hold the old slots: GraphedTrainStep re-captures (amax_generation)
        i = st["index"][site] = st["n"]
        st["n"] += n
    return i


def h2_export(scope_id, ptr_names):
    """The operand-magnitude slots of a model's call sites as a checkpointable blob (CPU tensors and plain tuples): the keys of
    _amax_index with the owning model's scope token dropped and the weight ADDRESSES replaced by parameter names (`ptr_names`:
    {data_ptr: name}).  With it a restored run splits its operands with the scales the uninterrupted run would have used, i.e.
    continues bit for bit (h2_import); without it a restored model measures again (equal arithmetic, a different power-of-two operand
    scale wherever a magnitude sits near a binade edge).  Sites through tensors that are not parameters (BatchNorm-folded
    panorama weights) are left out: they measure again.  Version 2 also carries each site's route (`fp32`: a weight-gradient site
    on the fp32 kernels, H2_TAIL_MODE); a blob without a routed site stays version 1 (same meaning: every site on the split
    kernels, and readable by releases before routes).  Reads the device (synchronises)."""
    keys, cur, nxt, fp32 = [], [], [], []
    for st in _AMAX.values():
        c_, n_ = st["cur"].cpu(), st["nxt"].cpu()
        for key, i in st["index"].items():
            if i not in st["ready"] or len(key) != 6 or not isinstance(key[0], tuple) or key[0][0] != scope_id:
                continue
            name = ptr_names.get(key[1][0])
            if name is None:
                continue
            n = 2 if key[2] == "conv_bwd_weight" else 1
            keys.append((bool(key[0][1]), (name, key[1][1]), key[2], int(key[3]), int(key[4]), int(key[5])))
            cur.append([float(c_[i + j]) for j in range(n)])
            nxt.append([float(n_[i + j]) for j in range(n)])
            fp32.append(i in st["fp32"])
    if not any(fp32):
        return {"version": 1, "keys": keys, "cur": cur, "nxt": nxt}
    return {"version": 2, "keys": keys, "cur": cur, "nxt": nxt, "fp32": fp32}


def h2_import(scope_id, name_ptrs, blob, device):
    """Hands the slots of h2_export back to the call sites of the model that now owns `scope_id` (`name_ptrs`: {name: data_ptr});
    entries whose parameter is gone are skipped (they measure).  Routes (version 2) follow THIS process's H2_TAIL_MODE: in "fp32"
    mode a site the checkpointed run had routed is routed again and counted in h2_fallback_sites(); in "warn" mode it stays on the
    split kernels.  Either way it counts in h2_tail_sites() (its census flagged it; imported sites do not measure again).  A
    version-1 blob (no routes) leaves every site on the split kernels."""
    if not blob or blob.get("version") not in (1, 2):
        return 0
    st = _amax_state(torch.device(device))
    done = 0
    routes = blob["fp32"] if blob["version"] == 2 else [False] * len(blob["keys"])
    fp32, flagged = _tail_mode() == "fp32", 0
    for key, c_, n_, r_ in zip(blob["keys"], blob["cur"], blob["nxt"], routes):
        ptr = name_ptrs.get(key[1][0])
        if ptr is None:
            continue
        full = ((scope_id, bool(key[0])), (ptr, key[1][1])) + tuple(key[2:])
        i = _amax_index(st, full, len(c_))
        st["cur"][i:i + len(c_)] = torch.tensor(c_, dtype=torch.float32)
        st["nxt"][i:i + len(n_)] = torch.tensor(n_, dtype=torch.float32)
        st["ready"].add(i)
        st["fp32"].discard(i)
        if r_:
            flagged += 1
            if fp32:
                st["fp32"].add(i)
                st["fallback"] += 1
        done += 1
    if done:
        st["used"] = True
    if flagged:
        st["tail"] += flagged
    return done


def amax_roll():
    """Once per pass (stream-ordered, a handful of tiny launches): a site's reference magnitude `cur` follows what its last launch
    measured (`nxt`) UP as soon as that exceeds H2_FOLLOW_UP x cur and DOWN once it fell below cur / H2_FOLLOW_DOWN -- the scale is
    STICKY inside that window, so passes over data of similar magnitude (a repeated step, train after eval, eager and captured
    steps of one run) split their operands identically and stay bit-reproducible, and never lags a growing operand by more than
    H2_FOLLOW_UP: H2_HEADROOM x of growth per pass is absorbed whatever the history (round 4 followed up only at 64 x, which left
    2 x in the worst case).  Elements within 2^-9 / H2_FOLLOW_DOWN of the largest keep full precision."""
    for st in _AMAX.values():
        st["occ"].clear()
        if st["used"]:
            # one launch over the slots handed out so far (rounds 4-5: ~10 torch elementwise launches per pass)
            with torch.cuda.device(st["cur"].device):
                _lib.check(_lib.load().nef_amax_roll(_p(st["cur"]), _p(st["nxt"]), int(st["n"]), H2_FOLLOW_UP, H2_FOLLOW_DOWN, 0,
                                                     _stream()), "nef_amax_roll")
            st["used"] = False


def amax_snapshot(dev):
    """The magnitudes of the call sites handed out so far (GraphedTrainStep: around its eager probe)."""
    st = _amax_state(torch.device(dev))
    n = int(st["n"])
    return n, st["cur"][:n].clone(), st["nxt"][:n].clone(), st.get("gen", 0)


def amax_restore(dev, snap):
    """Puts the sites that existed at amax_snapshot() back to what they held then (sites created since keep what they measured)."""
    n, cur, nxt, gen = snap
    st = _amax_state(torch.device(dev))
    if n == 0 or st.get("gen", 0) != gen:
        return
    st["cur"][:n].copy_(cur)
    st["nxt"][:n].copy_(nxt)
    st["used"] = True


def amax_generation(dev):
    """Bumped whenever the site table of `dev` started over: pointers a captured launch baked in may now belong to other sites."""
    return _amax_state(dev).get("gen", 0)


def amax_move(old_ptr, new_ptr):
    """A weight tensor moved (an optimiser re-pointed its parameters into a flat buffer): its call sites keep their history."""
    for st in _AMAX.values():
        for site in [k for k in st["index"] if k[0] is not None and k[1][0] == old_ptr]:
            st["index"][(site[0], (new_ptr, site[1][1])) + site[2:]] = st["index"].pop(site)


def _pack_desc(wino, K, G, Cog, Cig, flip, src=None):
    """The nef_pack_desc of one operand, pointers left NULL."""
    d = _lib.PackDesc(G=G, Cog=Cog, Cig=Cig, K=K, transpose_flip=int(flip), wino=int(wino))
    if src is not None:
        d.src_mode, d.src_Cr = 1, int(src[1])
    return d


def _packed_floats(wino, K, G, Cog, Cig, flip):
    """fp32 words of a packed operand (nef_pack_bytes: include/nefnet_hip.h has the formulas)."""
    return _lib.load().nef_pack_bytes(C.byref(_pack_desc(wino, K, G, Cog, Cig, flip))) // 4


def wino_ok(K, Cin_g, Cout_g, T_out, pro=0):
    return (WINOGRAD and (K == 3 or (K == 7 and not pro)) and T_out % 2 == 0 and Cin_g % 16 == 0 and
            ((Cout_g % 128 == 0 and T_out >= 128) or (Cout_g % 128 != 0 and Cout_g % 64 == 0 and T_out >= 256)))


_PREPACKED = {}     # (weight data_ptr, G, flip, wino, src) -> operand packed by pack_many(), consumed by the next pack_weight()


_PACK_KEEP = False


@contextlib.contextmanager
def pack_keep(on=True):
    """Inside (with `on`): pack_weight() hands a pre-packed operand out WITHOUT taking it from the table, so the next pass through the
    same weights finds it again -- the multi-view train step runs its head once per view on one step-level pack_many.  The operand is
    a function of the weight alone, so who packed it never shows in a result."""
    global _PACK_KEEP
    prev, _PACK_KEEP = _PACK_KEEP, bool(on)
    try:
        yield
    finally:
        _PACK_KEEP = prev


def _logical_shape(w, src):
    """Shape of the weight tensor that is packed: w's own, or -- src = ("poly", Cr) -- the PHASE weights of conv1d(upsample2(x), w)
    (twice the rows, formed inside the pack kernel: nef_pack_desc.src_mode 1)."""
    if src is None:
        return tuple(w.shape)
    assert src[0] == "poly" and w.shape[2] == 3, src
    return (2 * w.shape[0], w.shape[1], 3)


def _pack_shape(w, G, flip, T, f4=False, plain=True, src=None):
    """`plain`: the launch has no prologue, channel scale, statistics or BatchNorm-backward sums -- the only launches the packed
    short-row form of the split-fp16 kernel (8 <= T <= 64) takes; pass False for the others so that they fall back to the fp32 kernels."""
    shp = _logical_shape(w, src)
    Cog, Cig, K = shp[0] // G, shp[1], shp[2]
    cin_g, cout_g = (Cog, Cig) if flip else (Cig, Cog)          # roles in the launch that consumes the operand
    wino = (WINO_FWD if f4 else 1) if (T is not None and wino_ok(K, cin_g, cout_g, T)) else 0
    if (T is not None and (T >= 128 or plain) and h2_ok(K, cin_g, cout_g, T) and
            _h2_fills(G, cout_g, T, 256, 128 if cout_g % 128 == 0 else 64)):
        wino = 3
    return Cog, Cig, K, wino


class PackReq(NamedTuple):
    """One operand for pack_many(): the arguments of the pack_weight(w, G, flip=, T=, f4=, src=, plain=, site=) call that will ask for it."""
    w: torch.Tensor
    G: int
    flip: bool
    T: Optional[int]
    f4: bool = False
    src: Optional[tuple] = None
    plain: bool = True
    site: object = None


def _pack(reqs, who, align=1):
    """`reqs`: [(w, G, Cog, Cig, K, flip, wino, src, site)], forms resolved -> their packed operands, written by ONE
    nef_pack_weights call.  The operands are slices of one allocation, each starting at a multiple of `align` words; a Winograd or
    split-fp16 operand carries its form (`nef_wino`) and the identity of its call site for the split-fp16 input-magnitude slots
    (`nef_site`; `site` stands in for w's address when `w` is a temporary)."""
    L = _lib.load()
    descs = (_lib.PackDesc * len(reqs))()
    offs, off = [], 0
    for i, (w, G, Cog, Cig, K, flip, wino, src, site) in enumerate(reqs):
        if src is not None and wino != 3:
            raise _lib.NefLibraryError(who + ": a synthesized (polyphase) operand outside the split-fp16 kernel")
        descs[i] = _pack_desc(wino, K, G, Cog, Cig, flip, src)
        offs.append((off, L.nef_pack_bytes(C.byref(descs[i])) // 4))
        off += (offs[-1][1] + align - 1) // align * align
    arena = torch.empty(off, device=reqs[0][0].device, dtype=torch.float32)
    out = []
    for d, (o, n), (w, G, Cog, Cig, K, flip, wino, src, site) in zip(descs, offs, reqs):
        wp = arena[o:o + n]
        if wino:
            wp.nef_wino = wino
            wp.nef_site = (w.data_ptr() if site is None else site, flip)
        d.w, d.wp = w.data_ptr(), wp.data_ptr()
        out.append(wp)
    _lib.check(L.nef_pack_weights(descs, len(reqs), _stream()), "nef_pack_weights")
    return out


def pack_many(requests):
    """All operands of a pass -- or, from engine.forward(save=True), of a whole train step: forward AND backward-data operands,
    the polyphase ones included -- in ONE launch.  `requests`: iterable of PackReq (or its fields as a plain tuple), exactly as
    the later pack_weight(w, G, flip=flip, T=T, f4=f4, src=src, plain=plain, site=site) calls will ask for them; those calls then
    return the pre-packed operand instead of launching.  Anything not pre-packed still packs on demand, so a missing or surplus
    request costs time, never correctness.  A call whose requests are ALL still waiting in the table (a pass-level call inside a
    step whose step-level call has already packed everything) does nothing; any other call resets the table first."""
    reqs, keys = [], []
    for r in requests:
        r = PackReq(*r)
        w, flip = _chk(r.w), bool(r.flip)
        Cog, Cig, K, wino = _pack_shape(w, r.G, flip, r.T, bool(r.f4), bool(r.plain), r.src)
        key = (w.data_ptr(), r.G, flip, wino, r.src)
        if key not in keys:
            keys.append(key)
            reqs.append((w, r.G, Cog, Cig, K, flip, wino, r.src, r.site))
    if keys and all(_PREPACKED.get(k) is not None and _PREPACKED[k][1] is r_[0] and _PREPACKED[k][2] == r_[0]._version
                    for k, r_ in zip(keys, reqs)):
        return
    _PREPACKED.clear()
    if not reqs:
        return
    for key, r_, wp in zip(keys, reqs, _pack(reqs, "pack_many", align=4)):      # 16-byte aligned operands
        _PREPACKED[key] = (wp, r_[0], r_[0]._version)          # keep the source alive while its pointer is the key


def pack_weight(w, G, flip=False, T=None, f4=False, site=None, shared=False, plain=True, src=None):
    """w [G*Cog, Cig, K] -> packed operand (forward: [G][K][Cig][Cog]; flip: [G][K][Cog][Cig], taps reversed).
    `T`: output length of the conv launch this operand is for; when the Winograd F(2,3) path applies to that launch
    the operand is packed for it (marked with `.nef_wino`) and `conv()` takes that path; `f4` allows the F(4,3) form.
    `src` = ("poly", Cr): pack the phase weights of conv1d(upsample2(x), w) instead of w itself (split-fp16 operands only)."""
    _chk(w)
    Cog, Cig, K, wino = _pack_shape(w, G, flip, T, f4, plain, src)
    key = (w.data_ptr(), G, bool(flip), wino, src)
    hit = _PREPACKED.get(key) if _PACK_KEEP else _PREPACKED.pop(key, None)
    if hit is not None and hit[1] is w and hit[2] == w._version:
        return hit[0]
    wp, = _pack([(w, G, Cog, Cig, K, bool(flip), wino, src, site)], "pack_weight")
    if shared:
        # every launch of a pass through this operand is ONE call site (a loop over chunks of one tensor family, e.g.
        # the panorama sweep's angle chunks) instead of one site per occurrence
        wp.nef_shared = True
    return wp


def conv_stats_buffer(wp, B, G, Cog, T_out, device):
    """(slots tensor, slots per sample) for conv(..., stats=...) -- or None when the conv would not run on the F(4,3)
    kernel, whose epilogue is the one that leaves the BatchNorm slot sums."""
    wino = int(getattr(wp, "nef_wino", 0))
    if wino not in (2, 3) or (wino == 3 and T_out < 128):      # (packed short rows leave no statistics)
        return None
    # a slot = one wave's 128 columns; the split-fp16 kernel tiles a sample in 256-column workgroups (2 slots each)
    nslot = 2 * ((T_out + 255) // 256) if wino == 3 else _lib.load().nef_conv_stats_slots(T_out, Cog)
    if nslot <= 0:
        return None
    return torch.empty(G * Cog, B * nslot, 2, device=device, dtype=torch.float32), nslot


def bn_stats_from_slots(stats, gamma, beta, running_mean, running_var, P, N, Ln, eps=1e-5, momentum=0.1, nbt=None):
    """bn_train_stats from the slot sums a conv epilogue left (x [N, C, Ln] itself is not read).  `nbt`: the BatchNorm's
    num_batches_tracked (int64[]), incremented by P in the same launch."""
    L = _lib.load()
    slots, nslot = stats
    Ct = slots.shape[0]
    mean, invstd, a, b = (torch.empty(P, Ct, device=slots.device, dtype=torch.float32) for _ in range(4))
    n = L.nef_bn_ws_bytes(P, Ct)
    ws = workspace(n, slots.device)
    _lib.check(L.nef_bn_stats_from_slots(_p(slots), nslot, _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(mean),
                                         _p(invstd), _p(a), _p(b), _p(ws), n, P, N // P, Ct, Ln, eps, momentum, _p(nbt), _stream()),
               "nef_bn_stats_from_slots")
    return mean, invstd, a, b


def _operand(a, xv, in_scale, pro):
    """The input operand of a ConvArgs / BwwArgs (same field names): the view, the channel scale and the input prologue."""
    a.x, a.x_bs, a.x_gs = xv.ptr, xv.bs, xv.gs
    if in_scale is not None:
        a.in_scale, a.sc_bs, a.sc_gs = _p(in_scale[0]), in_scale[1], in_scale[2]
    if pro is not None and pro[0]:
        a.pro_mode, a.pro_a, a.pro_b, a.pro_Bp = pro[0], _p(pro[1]), _p(pro[2]), pro[3]


def conv(xv, wp, Cog, K, out=None, bias=None, in_scale=None, res=None, gate=None, gate_scale=1.0, relu=False,
         mask=None, drop_p=0.0, drop_scale=1.0, seed=0, role="conv_fwd", pro=None, seed_dev=None, stats=None, bnb=None,
         x_scale=0.0, tag_extra="", res_scale=None, gate_rowscale=None, stats_mode=0, live=None, res_live=None):
    """out = epilogue(conv1d(prologue(x) * in_scale, w) + bias + res * res_scale).  `xv`, `res`, `gate`, `out` are GV views;
    `in_scale` / `res_scale` are (tensor, batch_stride, group_stride).  `pro` = (mode, a, b, Bp): input prologue applied while
    staging -- bit0 BatchNorm affine + ReLU with a/b [P, C_in], bit1 x2 linear upsampling of a half-resolution input
    (the output is then 2*xv.T long).  `stats`: a conv_stats_buffer() the epilogue fills with the per-slot sum and sum
    of squares of the outputs; `bnb` = (x, mean, invstd, a, b, Bp, conv_stats_buffer()[, up]): the epilogue leaves the
    BatchNorm-backward sums sum(g*m), sum(g*m*xhat) of the layer this backward-data launch propagates into.
    `live` = (int32 table [B, G], addend): the caller's promise that the operand, after in_scale, is exactly zero at every
    t >= table[b, g] + addend (ops.live_extent + the bias-free convs in between, never configuration): nef_conv_fwd_live, same bits.
    `res_live` = the addend of the same promise for `res` (after res_scale), over the same table: a dead tile behind it as well only
    stores its zeros (nef_conv_fwd_live_res).  None: no promise, such a tile runs the whole epilogue.
    Returns the output tensor."""
    L = _lib.load()
    if live is not None and not LIVE:
        live = None

    def launch():
        if live is not None and res is not None and res_live is not None:
            _lib.check(L.nef_conv_fwd_live_res(C.byref(a), _p(live[0]), int(live[1]), int(res_live), _stream()), "nef_conv_fwd_live_res")
        elif live is not None:
            _lib.check(L.nef_conv_fwd_live(C.byref(a), _p(live[0]), int(live[1]), _stream()), "nef_conv_fwd_live")
        else:
            _lib.check(L.nef_conv_fwd(C.byref(a), _stream()), "nef_conv_fwd")
    T_out = xv.T * 2 if (pro is not None and pro[0] & 2) else xv.T
    if out is None:
        y = torch.empty(xv.B, xv.G * Cog, T_out, device=xv.t.device, dtype=torch.float32)
        out = GV.dense(y, xv.G)
    a = _lib.ConvArgs()
    _operand(a, xv, in_scale, pro)
    a.wp, a.y, a.y_bs, a.y_gs = _p(wp), out.ptr, out.bs, out.gs
    a.bias = _p(bias)
    a.res = res.ptr if res is not None else None
    a.gate = gate.ptr if gate is not None else None
    a.mask = _p(mask)
    if res is not None:
        a.res_bs, a.res_gs = res.bs, res.gs
    if gate_rowscale is not None:      # y = gate > 0 ? y * gate_scale * gate_rowscale[b, g, c] : 0 (split-fp16 launches only)
        assert gate is not None
        a.gate_rowscale, a.gr_bs, a.gr_gs = _p(gate_rowscale[0]), gate_rowscale[1], gate_rowscale[2]
    a.stats_mode = int(stats_mode)      # 1: `stats` receives sum_t (ungated output) x gate per slot (chscale_bwd's per-channel sums)
    if res_scale is not None:      # (tensor, batch stride, group stride) like in_scale: y += res * res_scale[b, g, c]; split-fp16 launches only
        assert res is not None
        a.res_scale, a.rs_bs, a.rs_gs = _p(res_scale[0]), res_scale[1], res_scale[2]
    if gate is not None:
        a.gate_bs, a.gate_gs = gate.bs, gate.gs
    a.B, a.T, a.G, a.Cin_g, a.Cout_g, a.K = xv.B, T_out, xv.G, xv.Cg, Cog, K
    a.relu = int(relu)
    a.gate_scale, a.drop_scale, a.drop_p, a.rng_seed = gate_scale, drop_scale, drop_p, seed
    a.rng_seed_dev = _p(seed_dev)
    a.wino = int(getattr(wp, "nef_wino", 0))
    a.x_scale = float(x_scale)
    a.stats = _p(stats[0]) if stats is not None else None
    if bnb is not None:      # (x, mean, invstd, a, b, Bp, slots buffer): BatchNorm-backward sums of the layer below
        a.bnb_x, a.bnb_mean, a.bnb_invstd, a.bnb_a, a.bnb_b = (_p(t) for t in bnb[:5])
        a.bnb_Bp, a.bnb_slots = bnb[5], _p(bnb[6][0])
        a.bnb_up = int(bnb[7]) if len(bnb) > 7 else 0
    if a.wino == 3 and not x_scale:
        st = _amax_state(xv.t.device)
        ws = getattr(wp, "nef_site", None)
        site = None
        if AMAX_SCOPE is not None and ws is not None:
            # + the occurrence within the pass: the k-th launch through one weight keeps its own history, so a step repeated on
            # the same data finds the scales it left (bit-identical results)
            occ = st["occ"]
            k = occ[(AMAX_SCOPE, ws, role, xv.B, T_out)] = occ.get((AMAX_SCOPE, ws, role, xv.B, T_out), 0) + 1
            site = (AMAX_SCOPE, ws, role, xv.B, T_out, 0 if getattr(wp, "nef_shared", False) else k)
        i = _amax_index(st, site if site is not None else (None, "conv"), 1)      # (unscoped launches: a slot of their own, never a site's)
        a.x_amax_next = st["nxt"].data_ptr() + 4 * i
        if i not in st["ready"] or site is None:      # first launch of the site (or no scope): measure, then run
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("split-fp16 conv: a call site's first launch (it measures its operand) cannot be captured; "
                                   "run the step once eagerly first (GraphedTrainStep does)")
            st["nxt"][i] = 0.0
            launch()
            st["cur"][i] = st["nxt"][i]
            if site is not None:
                _note_tail(st, i, [(xv, in_scale, pro)])
            st["ready"].add(i)
        a.x_amax = st["cur"].data_ptr() + 4 * i
        a.x_clamped = st["clamped"].data_ptr()
        st["used"] = True
    # bench.py prices a launch by its tag; the optional 8th element says which operands are NOT at the output's resolution / are extra:
    # "up" = the input is the half-resolution tensor (x2-upsampling prologue), "bnb" / "bnbup" = the epilogue also reads the
    # BatchNorm input of the layer below (full / half resolution) for the backward sums
    extra = ("up" if (pro is not None and pro[0] & 2) else "") + ("ph" if (pro is not None and pro[0] == 4) else "") + ("pf" if (pro is not None and pro[0] & 8) else "") + tag_extra + ("bnb" + ("up" if len(bnb) > 7 and bnb[7] else "") if bnb is not None else "")
    tag = (role, K, xv.G, xv.Cg, Cog, xv.B, T_out) + ((extra,) if extra else ())
    frac = 1.0      # executed work: the plain forms skip the dead tiles of a launch that carries a promise (the table's read-back
    if PROFILE is not None and live is not None and a.wino == 3 and not a.pro_mode and T_out >= 128:      # stays outside the events)
        frac = _live_frac(live, (K - 1) // 2, T_out)
    ev = _timed(tag)
    if ev is not None:
        EXEC_FRAC[tag] = 0.0 if a.wino == 3 else _exec_frac(K, a.wino)
        EXEC_FP16[tag] = 3.0 if a.wino == 3 else 0.0
        if a.wino == 3 and LIVE:
            _live_note(tag, frac)
    launch()
    if ev is not None:
        ev.record()
    return out.t


# ------------------------------------------------------------------ polyphase form of conv1d(upsample2(x)), K = 3
def poly_weights(w, tile_Cr=0):
    """w [R, Cig, 3] -> [2R, Cig, 3]: row 2r + p = the phase-p weights of row r (csrc/elementwise.hip poly_weights_kernel): output
    2m + p of conv1d(upsample2(x), w) is the K = 3 conv of the half-resolution x with them.  `tile_Cr` (channels per group): rows in
    the tile order the polyphase FORWARD launch wants instead."""
    _chk(w)
    ws = torch.empty(2 * w.shape[0], w.shape[1], 3, device=w.device, dtype=torch.float32)
    _lib.check(_lib.load().nef_poly_weights(_p(w), _p(ws), w.shape[0], w.shape[1], int(tile_Cr), _stream()), "nef_poly_weights")
    return ws


def poly_fwd_ok(G, Cog, Cig, T):
    """Can y = conv1d(upsample2(x [.., G*Cig, T/2]), w [G*Cog, Cig, 3]) run in polyphase form?  (a split-fp16 conv with Cig reduction
    channels, 2 Cog output rows in 128-row tiles, T / 2 columns)"""
    Th = T // 2
    return (H2 and T % 2 == 0 and Th >= 128 and Cog % 64 == 0 and Cig % 16 == 0 and h2_ok(3, Cig, 2 * Cog, Th, 1) and
            _h2_fills(G, 2 * Cog, Th, 256, 128))


def conv_poly_fwd(xv, w, Cog, bias=None, pro=None, stats=False, site=None, save_edge=False):
    """y [B, G*Cog, 2T] = conv1d(upsample2(prologue(x)), w) + bias in polyphase form: one split-fp16 conv over the half-resolution
    x (`xv`, a GV) whose rows are the two phases of each channel (conv args pro_mode 8 | affine bit), written interleaved, + the two
    row-end columns (nef_poly_fwd_edge).  `pro` = (mode, a, b, Bp) as conv() gets it for this layer (bit1 = the upsampling itself,
    bit0 the BatchNorm affine + ReLU of the layer below); `stats`: also leave the BatchNorm slot sums -> (y, (slots, nslot)).
    Reference: codes/network/model_nefnet.py:102-105 (nn.Upsample + the DoubleConv's first conv).  Summation order differs from
    the upsampling-prologue form (fp32-class either way)."""
    L = _lib.load()
    G, Cig, Th = xv.G, xv.Cg, xv.T
    assert w.shape == (G * Cog, Cig, 3) and xv.bs == G * Cig * Th and xv.gs == Cig * Th, "conv_poly_fwd: dense input rows"
    aff = pro is not None and bool(pro[0] & 1)
    # the phase weights are formed inside the pack (nef_pack_desc.src_mode 1): no poly_weights launch, no fp32 phase tensor
    wp = pack_weight(w, G, T=Th, site=w.data_ptr() if site is None else site, plain=False, src=("poly", Cog))
    if int(getattr(wp, "nef_wino", 0)) != 3:
        raise _lib.NefLibraryError("conv_poly_fwd: shape outside the split-fp16 kernel (ask poly_fwd_ok first)")
    y = torch.empty(xv.B, G * Cog, 2 * Th, device=xv.t.device, dtype=torch.float32)
    slots = conv_stats_buffer(wp, xv.B, G, Cog, Th, xv.t.device) if stats else None
    out = GV(y, xv.B, G, 2 * Cog, Th, G * Cog * 2 * Th, Cog * 2 * Th, 0)      # (strides of the real tensor; Cg / T as the launch counts them)
    conv(xv, wp, 2 * Cog, 3, out=out, bias=bias, pro=(8 | int(aff), pro[1] if aff else None, pro[2] if aff else None, pro[3] if aff else 1),
         stats=slots)
    pa, pb, pbp = (_p(pro[1]), _p(pro[2]), pro[3]) if aff else (None, None, 1)
    xedge = torch.empty(xv.B, G * Cig, 2, device=xv.t.device, dtype=torch.float32) if save_edge else None
    _lib.check(L.nef_poly_fwd_edge(xv.ptr, _p(w), _p(y), xv.B, G, Cog, Cig, 2 * Th, pa, pb, pbp,
                                   _p(slots[0]) if slots is not None else None, slots[1] if slots is not None else 0, _p(xedge),
                                   _stream()), "nef_poly_fwd_edge")
    y.nef_xedge = xedge      # (the prologue's output at both row ends: what the polyphase weight gradient's row-end terms need)
    return (y, slots) if stats else y


def poly_bwd_ok(G, Cog, Cig, T):
    """Can the backward-data pass of conv1d(upsample2(x) [.., G*Cig, T], w [G*Cog, Cig, 3]) run in polyphase form?  (the launch is a
    split-fp16 conv with 2 Cog reduction channels, Cig outputs, T / 2 columns)"""
    Th = T // 2
    return (H2 and T % 2 == 0 and Th >= 128 and Cig % 64 == 0 and (2 * Cog) % 16 == 0 and h2_ok(3, 2 * Cog, Cig, Th) and
            _h2_fills(G, Cig, Th, 256, 128 if Cig % 128 == 0 else 64))


def conv_bwd_data_poly(gyv, w, Cig, bnb=None, site=None, phase_major=False):
    """Gradient wrt the HALF-resolution input x of y = conv1d(upsample2(x), w) (K = 3, zero padding 1), from gy [B, G*Cog, T]
    (`gyv`, a GV): one split-fp16 conv at half resolution over the 2 Cog phase channels of gy (conv args pro_mode 4) + the row-end
    terms (nef_poly_bwd_edge) -- the full-resolution gradient wrt upsample2(x) is never formed.  `w` [G*Cog, Cig, 3] is the conv's
    own weight; `bnb` as in conv() (plain form: its x at the half resolution).  Reference semantics: autograd through
    codes/network/model_nefnet.py:102-105.  Summation order differs from conv + upsample2_bwd (fp32-class either way)."""
    L = _lib.load()
    if phase_major:      # `gyv`: the gradient as [B, G * 2 Cog, T/2] (bn_relu_bwd(..., phase_major=True)): a plain conv over it
        G, Cog, T = gyv.G, gyv.Cg // 2, 2 * gyv.T
    else:
        G, Cog, T = gyv.G, gyv.Cg, gyv.T
    Th = T // 2
    assert w.shape == (G * Cog, Cig, 3) and gyv.gs == Cog * T, "conv_bwd_data_poly: dense gradient rows"
    wp = pack_weight(w, G, flip=True, T=Th, site=w.data_ptr() if site is None else site, src=("poly", 0))
    if int(getattr(wp, "nef_wino", 0)) != 3:
        raise _lib.NefLibraryError("conv_bwd_data_poly: shape outside the split-fp16 kernel (ask poly_bwd_ok first)")
    xv = GV(gyv.t, gyv.B, G, 2 * Cog, Th, gyv.bs, gyv.gs, gyv.off)
    if bnb is not None and len(bnb) == 6:      # (x, mean, invstd, a, b, Bp): the slot buffer is made here (returned as g.nef_slots)
        slots = conv_stats_buffer(wp, gyv.B, G, Cig, Th, gyv.t.device)
        bnb = None if slots is None else (*bnb, slots)
    g = conv(xv, wp, Cig, 3, role="conv_bwd_data", bnb=bnb, pro=None if phase_major else (4, None, None, 1),
             tag_extra="pm" if phase_major else "")      # (bench.py: "pm" = plain conv over the phase-major gradient)
    g.nef_slots = bnb[6] if bnb is not None else None
    ba = [None] * 5 + [1, None, 0]
    if bnb is not None:
        ba = [_p(t) for t in bnb[:5]] + [bnb[5], _p(bnb[6][0]), bnb[6][1]]
    _lib.check(L.nef_poly_bwd_edge(gyv.ptr, _p(w), _p(g), gyv.B, G, Cog, Cig, T, *ba, int(phase_major), _stream()), "nef_poly_bwd_edge")
    return g


def poly_w_ok(B, G, Cog, Cig, T):
    """Weight gradient of conv1d(upsample2(x), w) in polyphase form: a split-fp16 weight gradient over the half-resolution x and
    the phase-major gradient (2 Cog rows), producer / consumer form (2 Cog % 128 == 0), then nef_poly_wgrad_fold."""
    Th = T // 2
    return (T % 4 == 0 and Cog % 64 == 0 and h2w_ok(3, Cig, 2 * Cog, Th, 1) and
            (BATCH_HINT is None or B * ((Th + 63) // 64) >= 8 * _H2_MIN_WGS))


def conv_bwd_weight_poly(xv, gy_pm, Cog, pro, xedge, site=None):
    """gw [G*Cog, Cig, 3] of y = conv1d(upsample2(prologue(x)), w) from the half-resolution x (`xv`), the PHASE-MAJOR gradient
    gy_pm [B, G*2Cog, T/2] and `xedge` [B, G*Cig, 2] (the prologue's output at both row ends, conv_poly_fwd(..., save_edge=True)).
    `pro` as the forward got it (bit0 = affine + ReLU prologue; the upsampling bit is what the polyphase form replaces)."""
    L = _lib.load()
    G, Cig = xv.G, xv.Cg
    aff = pro is not None and bool(pro[0] & 1)
    gyv = GV.dense(gy_pm, G)
    gw2 = conv_bwd_weight(xv, gyv, 3, pro=(4 | int(aff), pro[1] if aff else None, pro[2] if aff else None, pro[3] if aff else 1),
                          site=site, h2=True, xedge=xedge)
    gw = torch.empty(G * Cog, Cig, 3, device=gy_pm.device, dtype=torch.float32)
    n = L.nef_poly_wgrad_fold_ws_bytes(xv.B, G, Cog, Cig)
    ws = torch.empty(n // 4, device=gy_pm.device, dtype=torch.float32)
    _lib.check(L.nef_poly_wgrad_fold(_p(gw2), _p(gy_pm), _p(xedge), _p(gw), _p(ws), n, xv.B, G, Cog, Cig, 2 * xv.T, _stream()),
               "nef_poly_wgrad_fold")
    return gw


def h2w_ok(K, Cig, Cog, T, pro_mode=0, in_scale=False):
    return (H2 and T % 2 == 0 and T >= 64 and Cig % 64 == 0 and Cog % 64 == 0 and
            (K == 3 or not pro_mode) and not (pro_mode and in_scale))


def conv_bwd_weight(xv, gyv, K, in_scale=None, pro=None, wino=None, site=None, h2=None, x_scale=0.0, gy_scale=0.0, xedge=None, live=None):
    """gw [G*Cog, Cig, K] for y = conv(prologue(x) * in_scale, w); `pro` as in conv().  Default path: the split-fp16 kernel
    (csrc/conv_h2w.hip) wherever its shape rules hold (h2w_ok; `h2=False` forbids it, giving `wino` forbids it too); `site`: the
    identity of the call site for its operand-magnitude slots (the engine passes the weight's address; None = measure at every
    call), `x_scale` / `gy_scale`: explicit powers of two instead.  `wino`: force (True / 4) or forbid
    (False) the transposed-Winograd form -- F(3,4) for K == 3, the 4 + 3 split through F(4,4) + F(3,4) for K == 7; default:
    wherever it applies (see WINOGRAD, WINO_BW4, WINO_BW7).  `xedge` [B, G*Cig, 2]: the prologue's output at both row ends, which
    pro_mode bit 2 needs on the fp32 kernels (conv_bwd_weight_poly passes it).  `live` = (int32 table [B, G], addend): the caller's
    promise that every product of a (sample, 64-column tile) item with t0 >= table[b, g] + addend is zero -- the gradient's bound, or
    the input's bound + (K-1)/2 (split-fp16 kernel only: nef_conv_bwd_weight_live, same gw bits; the fp32 forms ignore it).  The launch's
    magnitude words are taken over the live items: they are unchanged only where BOTH operands are zero in the dead ones."""
    L = _lib.load()
    B, T, G, Cig, Cog = xv.B, gyv.T, xv.G, xv.Cg, gyv.Cg
    dev = xv.t.device
    gw = torch.empty(G * Cog, Cig, K, device=dev, dtype=torch.float32)
    pm0 = pro[0] if pro is not None else 0
    a = _lib.BwwArgs()
    _operand(a, xv, in_scale, pro)
    a.gy, a.gy_bs, a.gy_gs, a.gw = gyv.ptr, gyv.bs, gyv.gs, _p(gw)
    a.B, a.T, a.G, a.Cin_g, a.Cout_g, a.K = B, T, G, Cig, Cog, K
    a.x_scale, a.gy_scale = float(x_scale), float(gy_scale)
    routed = False
    if h2 is None:
        h2 = (wino is None and h2w_ok(K, Cig, Cog, T, pm0, in_scale is not None) and
              (BATCH_HINT is None or B * ((T + 63) // 64) >= 8 * _H2_MIN_WGS))      # enough (sample, tile) steps to split
    if h2:
        _bww_form(L, a, 3, dev, f"conv_bwd_weight (split-fp16): unsupported shape Cig={Cig} Cog={Cog} K={K} T={T}")
        if not (x_scale and gy_scale):
            st = _amax_state(dev)
            key = None
            if AMAX_SCOPE is not None and site is not None:
                occ = st["occ"]
                base = (AMAX_SCOPE, (site, "w"), "conv_bwd_weight", B, T)
                k = occ[base] = occ.get(base, 0) + 1
                key = base + (k,)
            i = _amax_index(st, key if key is not None else (None, "bww"), 2)          # slots i (x) and i + 1 (gy); unscoped launches: a pair of their own
            nxt = st["nxt"].data_ptr() + 4 * i
            a.x_amax_next, a.gy_amax_next = nxt, nxt + 4
            if i not in st["ready"] or key is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("split-fp16 weight gradient: a call site's first launch cannot be captured")
                st["nxt"][i:i + 2] = 0.0
                _bww(L, a, live)      # (x_amax, gy_amax and clamped still NULL: it measures)
                st["cur"][i:i + 2] = st["nxt"][i:i + 2]
                if key is not None:
                    flag = _note_tail(st, i, [(xv, in_scale, pro), (gyv, None, None)])
                    if _tail_mode() == "fp32" and int(flag.item()):      # (the measuring launch is eager: one host read per site lifetime)
                        st["fp32"].add(i)
                        st["fallback"] += 1
                st["ready"].add(i)
            routed = i in st["fp32"]
            if not routed:
                st["used"] = True
                cur = st["cur"].data_ptr() + 4 * i
                a.x_amax, a.gy_amax, a.clamped = cur, cur + 4, st["clamped"].data_ptr()
        if not routed:
            tag = ("conv_bwd_weight", K, G, Cig, Cog, B, T) + (("up",) if pm0 & 2 else (("pw",) if pm0 & 4 else ()))
            frac = 1.0      # executed work: the producer / consumer kernel without a prologue leaves the dead 64-column items out
            if PROFILE is not None and live is not None and LIVE and LIVE_WGRAD and not pm0 and Cog % 128 == 0:
                frac = _live_frac(live, 0, T, 64)
            ev = _timed(tag)
            if ev is not None:
                EXEC_FRAC[tag] = 0.0
                EXEC_FP16[tag] = 3.0
                if LIVE:
                    _live_note(tag, frac)
            _bww(L, a, live)
            _done(ev)
            return gw
    # fp32 kernels.  A routed split-fp16 site (H2_TAIL_MODE) takes the DIRECT form: the transposed-Winograd transforms add and
    # subtract neighbouring products before the reduction, which on two heavy-tailed operands costs the small half of the gradient
    # what the split format does (log-normal K = 3: 2.3e-4 small-half rel-L2 through form 4, 7.8e-7 for torch's
    # fp32); bench.py sees its launches under their own tag ("f32" in the extra element).  pro_mode bit 2 (the polyphase weight
    # gradient's window continued with x'[0] / x'[T-1]): the zero-padded fp32 gradient + the row-end products of `xedge`
    # (nef_bwd_weight_clamp_ends).  The struct is the split-fp16 call's: these forms ignore its scale and magnitude fields.
    extra = ("up" if pm0 & 2 else "") + (("pw" if pm0 & 4 else "") + "f32" if routed else "")
    if routed:
        wino = False
    clamp = bool(pm0 & 4)
    if clamp:
        if xedge is None:
            raise _lib.NefLibraryError("conv_bwd_weight: pro_mode bit 2 on the fp32 kernels needs `xedge`")
        pm0 = a.pro_mode = pm0 & 3
    if wino is None:
        wino = (WINOGRAD and ((K == 3 and WINO_BW4) or (K == 7 and WINO_BW7)) and T % 2 == 0 and T >= 64
                and not (K == 7 and pm0))
    wino = 4 if wino else False
    assert wino or not pm0 or in_scale is None      # (the direct kernel's prologue forms take no in_scale)
    _bww_form(L, a, wino or 0, dev, f"conv_bwd_weight: unsupported shape Cig={Cig} Cog={Cog} K={K}")
    tag = ("conv_bwd_weight", K, G, Cig, Cog, B, T) + ((extra,) if extra else ())
    ev = _timed(tag)
    if ev is not None:
        EXEC_FRAC[tag] = _exec_frac(K, 2) if wino else 1.0
        EXEC_FP16[tag] = 0.0
    _bww(L, a)
    if clamp:
        assert K == 3 and in_scale is None and tuple(xedge.shape) == (B, G * Cig, 2)
        _lib.check(L.nef_bwd_weight_clamp_ends(_p(xedge), gyv.ptr, gyv.bs, gyv.gs, _p(gw), B, T, G, Cig, Cog, _stream()),
                   "nef_bwd_weight_clamp_ends")
    if ev is not None:
        ev.record()
    return gw


def _bww_form(L, a, form, device, unsupported):
    """Points the BwwArgs `a` at kernel family `form` and at a workspace of the size the library asks for."""
    a.form = form
    a.ws_bytes = L.nef_conv_bwd_weight_ws_bytes(C.byref(a))
    if a.ws_bytes == 0:
        raise _lib.NefLibraryError(unsupported)
    a.ws = _p(workspace(a.ws_bytes, device))


def _bww(L, a, live=None):
    """`live` = (int32 table [B, G], addend): every product of a (sample, 64-column tile) item with t0 >= table[b, g] + addend is zero
    (form 3 only: nef_conv_bwd_weight_live, same bits); ops.LIVE or ops.LIVE_WGRAD off: the plain entry."""
    if live is not None and LIVE and LIVE_WGRAD and a.form == 3:
        _lib.check(L.nef_conv_bwd_weight_live(C.byref(a), _p(live[0]), int(live[1]), _stream()), "nef_conv_bwd_weight_live")
    else:
        _lib.check(L.nef_conv_bwd_weight(C.byref(a), _stream()), "nef_conv_bwd_weight")


def _tail_mode():
    if H2_TAIL_MODE not in H2_TAIL_MODES:
        raise ValueError(f"ops.H2_TAIL_MODE={H2_TAIL_MODE!r}: expected one of {H2_TAIL_MODES}")
    return H2_TAIL_MODE


def chan_sum(x):
    L = _lib.load()
    _chk(x)
    B, Ct, T = x.shape
    out = torch.empty(Ct, device=x.device, dtype=torch.float32)
    n = L.nef_chan_sum_ws_bytes(Ct)
    ws = workspace(n, x.device)
    _lib.check(L.nef_chan_sum(_p(x), _p(out), _p(ws), n, B, Ct, T, _stream()), "nef_chan_sum")
    return out


# ------------------------------------------------------------------ transposed conv (k2 s2)
def _convt2_fma_fwd(x, w, bias, G):
    L = _lib.load()
    _chk(x), _chk(w), _chk(bias)
    B, Ct, T = x.shape
    Cig, Cog = Ct // G, w.shape[1]
    y = torch.empty(B, G * Cog, 2 * T, device=x.device, dtype=torch.float32)
    _lib.check(L.nef_convt2_fwd(_p(x), _p(w), _p(bias), _p(y), B, G, Cig, Cog, T, _stream()), "nef_convt2_fwd")
    return y


def _convt2_fma_bwd_data(gy, w, G):
    L = _lib.load()
    _chk(gy), _chk(w)
    B, Ct, To = gy.shape
    Cog, Cig, T = Ct // G, w.shape[0] // G, To // 2
    gx = torch.empty(B, G * Cig, T, device=gy.device, dtype=torch.float32)
    _lib.check(L.nef_convt2_bwd_data(_p(gy), _p(w), _p(gx), B, G, Cig, Cog, T, _stream()), "nef_convt2_bwd_data")
    return gx


def _convt2_fma_bwd_weight(x, gy, G):
    L = _lib.load()
    _chk(x), _chk(gy)
    B, Ct, T = x.shape
    Cig, Cog = Ct // G, gy.shape[1] // G
    gw = torch.empty(G * Cig, Cog, 2, device=x.device, dtype=torch.float32)
    gb = torch.empty(G * Cog, device=x.device, dtype=torch.float32)
    n = L.nef_convt2_bwd_weight_ws_bytes(G, Cig, Cog)
    ws = workspace(n, x.device)
    _lib.check(L.nef_convt2_bwd_weight(_p(x), _p(gy), _p(gw), _p(gb), _p(ws), n, B, G, Cig, Cog, T, _stream()),
               "nef_convt2_bwd_weight")
    return gw, gb


def group_transpose(t, G, R, Cn):
    """out[g][c][r] = in[g][r][c] over a flat [G*R*Cn] fp32 buffer."""
    L = _lib.load()
    _chk(t)
    out = torch.empty_like(t)
    _lib.check(L.nef_group_transpose(_p(t), _p(out), G, R, Cn, _stream()), "nef_group_transpose")
    return out


def convt2_as_conv_weight(w, G):
    """ConvTranspose1d weight [G*Cig, Cog, 2] -> the 1x1 conv weight [G*2Cog, Cig, 1] onto channels m = co*2+j."""
    Cig, Cog = w.shape[0] // G, w.shape[1]
    return group_transpose(w, G, Cig, 2 * Cog).view(G * 2 * Cog, Cig, 1)


def convt2_deinterleave(gy):
    L = _lib.load()
    _chk(gy)
    B, Ct, To = gy.shape
    gyq = torch.empty(B, 2 * Ct, To // 2, device=gy.device, dtype=torch.float32)
    _lib.check(L.nef_convt2_deinterleave(_p(gy), _p(gyq), B, Ct, To // 2, _stream()), "nef_convt2_deinterleave")
    return gyq


def convt2_fwd(x, w, bias, G, fma=False):
    """ConvTranspose1d(k=2, s=2, groups=G, bias).  Default: grouped 1x1 conv on the matrix cores + interleave;
    `fma=True` selects the plain-FMA kernel (kept as a cross-check)."""
    if fma:
        return _convt2_fma_fwd(x, w, bias, G)
    L = _lib.load()
    _chk(x), _chk(w), _chk(bias)
    B, Ct, T = x.shape
    Cog = w.shape[1]
    yq = conv(GV.dense(x, G), pack_weight(convt2_as_conv_weight(w, G), G), 2 * Cog, 1)     # [B, G*2Cog, T]
    y = torch.empty(B, G * Cog, 2 * T, device=x.device, dtype=torch.float32)
    _lib.check(L.nef_convt2_interleave(_p(yq), _p(bias), _p(y), B, G * Cog, T, _stream()), "nef_convt2_interleave")
    return y


def convt2_bwd_data(gy, w, G, fma=False, gyq=None):
    if fma:
        return _convt2_fma_bwd_data(gy, w, G)
    Cig = w.shape[0] // G
    gyq = convt2_deinterleave(gy) if gyq is None else gyq
    return conv(GV.dense(gyq, G), pack_weight(convt2_as_conv_weight(w, G), G, flip=True), Cig, 1, role="conv_bwd_data")


def convt2_bwd_weight(x, gy, G, fma=False, gyq=None):
    if fma:
        return _convt2_fma_bwd_weight(x, gy, G)
    B, Ct, T = x.shape
    Cig, Cog = Ct // G, gy.shape[1] // G
    gyq = convt2_deinterleave(gy) if gyq is None else gyq
    gwc = conv_bwd_weight(GV.dense(x, G), GV.dense(gyq, G), 1)                              # [G*2Cog, Cig, 1]
    gw = group_transpose(gwc.contiguous(), G, 2 * Cog, Cig).view(G * Cig, Cog, 2)
    return gw, chan_sum(gy)


# ------------------------------------------------------------------ angular encoding + MLP
def theta_mlp_fwd(theta, W, bias):
    L = _lib.load()
    _chk(theta), _chk(W), _chk(bias)
    N, O = theta.numel() // 2, W.shape[0]
    y = torch.empty(*theta.shape[:-1], O, device=theta.device, dtype=torch.float32)
    _lib.check(L.nef_theta_mlp_fwd(_p(theta), _p(W), _p(bias), _p(y), N, O, _stream()), "nef_theta_mlp_fwd")
    return y


def theta_mlp_bwd(theta, gy, O):
    L = _lib.load()
    _chk(theta), _chk(gy)
    N = theta.numel() // 2
    gW = torch.empty(O, 12, device=theta.device, dtype=torch.float32)
    gb = torch.empty(O, device=theta.device, dtype=torch.float32)
    _lib.check(L.nef_theta_mlp_bwd(_p(theta), _p(gy), _p(gW), _p(gb), N, O, _stream()), "nef_theta_mlp_bwd")
    return gW, gb


def theta_encode(theta):
    L = _lib.load()
    _chk(theta)
    N = theta.numel() // 2
    enc = torch.empty(*theta.shape[:-1], 12, device=theta.device, dtype=torch.float32)
    _lib.check(L.nef_theta_encode(_p(theta), _p(enc), N, _stream()), "nef_theta_encode")
    return enc


# ------------------------------------------------------------------ elementwise
def chscale_fwd(x, s, s_bs=None):
    L = _lib.load()
    _chk(x)
    B, Ct, T = x.shape
    y = torch.empty_like(x)
    ev = _hbm("chscale_fwd", x, y)
    _lib.check(L.nef_chscale_fwd(_p(x), _p(s), Ct if s_bs is None else s_bs, _p(y), B, Ct, T, _stream()), "nef_chscale_fwd")
    _done(ev)
    return y


def slots_to_rows(slots, B):
    """[B, C] per-(sample, channel) sums of the word-0 slot values a conv epilogue left (conv(..., stats=..., stats_mode=1))."""
    sl, nslot = slots
    out = torch.empty(B, sl.shape[0], device=sl.device, dtype=torch.float32)
    _lib.check(_lib.load().nef_slots_to_rows(_p(sl), nslot, _p(out), B, sl.shape[0], _stream()), "nef_slots_to_rows")
    return out


def chscale_bwd(gy, x, s, s_bs=None, relu_x=False):
    """`relu_x`: x is a ReLU output -- gx also carries that ReLU's backward mask (x > 0)."""
    L = _lib.load()
    _chk(gy), _chk(x)
    B, Ct, T = x.shape
    gx = torch.empty_like(x)
    gs = torch.empty(B, Ct, device=x.device, dtype=torch.float32)
    ev = _hbm("chscale_bwd", gy, x, gx)
    _lib.check(L.nef_chscale_bwd(_p(gy), _p(x), _p(s), Ct if s_bs is None else s_bs, _p(gx), _p(gs), B, Ct, T,
                                 int(relu_x), _stream()),
               "nef_chscale_bwd")
    _done(ev)
    return gx, gs


def gate(g, ref, scale=1.0):
    L = _lib.load()
    _chk(g), _chk(ref)
    out = torch.empty_like(g)
    _lib.check(L.nef_gate(_p(g), _p(ref), _p(out), scale, g.numel(), _stream()), "nef_gate")
    return out


def add(a, b):
    L = _lib.load()
    _chk(a), _chk(b)
    out = torch.empty_like(a)
    _lib.check(L.nef_add(_p(a), _p(b), _p(out), a.numel(), _stream()), "nef_add")
    return out


# ------------------------------------------------------------------ ROI ops
def roi_align_fwd(z, rois, T=None, t_off=0):
    """z [B,C,T], or a time window of it [B,C,zT] that starts at `t_off` of a length-`T` axis."""
    L = _lib.load()
    _chk(z), _chk(rois, torch.int64)
    B, Ct, zT = z.shape
    T = zT if T is None else T
    out = torch.empty(B, Ct, N_SEG, ROI_BINS, device=z.device, dtype=torch.float32)
    _lib.check(L.nef_roi_align_fwd(_p(z), _p(rois), _p(out), B, Ct, T, zT, t_off, _stream()), "nef_roi_align_fwd")
    return out


def roi_align_bwd(gout, rois, T, zT=None, t_off=0):
    """Gradient wrt z; with (zT, t_off) only that time window is produced (everything outside it is zero)."""
    L = _lib.load()
    _chk(gout), _chk(rois, torch.int64)
    B, Ct = gout.shape[0], gout.shape[1]
    zT = T if zT is None else zT
    gz = torch.empty(B, Ct, zT, device=gout.device, dtype=torch.float32)
    _lib.check(L.nef_roi_align_bwd(_p(gout), _p(rois), _p(gz), B, Ct, T, zT, t_off, _stream()), "nef_roi_align_bwd")
    return gz


def window_crop(xv, t0, W):
    """Dense [B, G*Cg, W] copy of the time window [t0, t0+W) of a grouped view."""
    L = _lib.load()
    dst = torch.empty(xv.B, xv.G * xv.Cg, W, device=xv.t.device, dtype=torch.float32)
    _lib.check(L.nef_window_crop(xv.ptr, xv.bs, xv.gs, _p(dst), xv.B, xv.G, xv.Cg, xv.T, t0, W, _stream()), "nef_window_crop")
    return dst


def window_scatter(src, outv, t0):
    """Write `src` [B, G*Cg, W] into the window [t0, t0+W) of the grouped view `outv`, zero everywhere else."""
    L = _lib.load()
    _chk(src)
    _lib.check(L.nef_window_scatter(_p(src), outv.ptr, outv.bs, outv.gs, outv.B, outv.G, outv.Cg, outv.T, t0,
                                    src.shape[2], _stream()), "nef_window_scatter")


def roi_unpool_fwd(zseg, rois, T, status=None):
    L = _lib.load()
    _chk(zseg), _chk(rois, torch.int64)
    B, Ct = zseg.shape[0], zseg.shape[1]
    out = torch.empty(B, Ct, T, device=zseg.device, dtype=torch.float32)
    ev = _hbm("roi_unpool_fwd", zseg, out)
    _lib.check(L.nef_roi_unpool_fwd(_p(zseg), _p(rois), _p(out), _p(status), B, Ct, T, _stream()), "nef_roi_unpool_fwd")
    _done(ev)
    return out


def roi_unpool_bwd(gout, rois):
    L = _lib.load()
    _chk(gout), _chk(rois, torch.int64)
    B, Ct, T = gout.shape
    gz = torch.empty(B, Ct, N_SEG, 2 * ROI_BINS, device=gout.device, dtype=torch.float32)
    ev = _hbm("roi_unpool_bwd", gout, gz)
    _lib.check(L.nef_roi_unpool_bwd(_p(gout), _p(rois), _p(gz), B, Ct, T, _stream()), "nef_roi_unpool_bwd")
    _done(ev)
    return gz


def roi_segment_table(rois):
    L = _lib.load()
    _chk(rois, torch.int64)
    B = rois.shape[0]
    start = torch.empty(B, N_SEG, device=rois.device, dtype=torch.int64)
    length = torch.empty(B, N_SEG, device=rois.device, dtype=torch.int64)
    _lib.check(L.nef_roi_segment_table(_p(rois), _p(start), _p(length), B, _stream()), "nef_roi_segment_table")
    return start, length


# ------------------------------------------------------------------ latent mix
def lead_mean(z1, z2r, V):
    L = _lib.load()
    _chk(z1), _chk(z2r)
    B, _, T = z1.shape
    latent = torch.empty(B, 256, T, device=z1.device, dtype=torch.float32)
    ev = _hbm("lead_mean", z1, z2r, latent)
    _lib.check(L.nef_lead_mean(_p(z1), _p(z2r), _p(latent), B, V, T, _stream()), "nef_lead_mean")
    _done(ev)
    return latent


def _choice(c):
    """(c1, c2) as ints, or a device int32[2] tensor (graph replay) -> (c1, c2, device pointer)."""
    if torch.is_tensor(c):
        return 0, 0, c.data_ptr()
    return int(c[0]), int(c[1]), None


def mix_fwd(latent, z1, z2r, q, V, c1, c2=None):
    L = _lib.load()
    c1, c2, cdev = _choice(c1 if c2 is None else (c1, c2))
    _chk(latent), _chk(q)
    B, _, T = latent.shape
    D = torch.empty(3 * B, 256, T, device=latent.device, dtype=torch.float32)
    _lib.check(L.nef_mix_fwd(_p(latent), _p(z1), _p(z2r), _p(q), _p(D), B, V, T, c1, c2, cdev, _stream()),
               "nef_mix_fwd")
    return D


def mix_fwd_shared(latent, z1, z2r, q, V, c1, c2=None):
    """The two DISTINCT decoder inputs, [2B,256,T] = (q*cat(z1m|z2m) | q*cat(z1[c1]|z2r[c2]))."""
    L = _lib.load()
    c1, c2, cdev = _choice(c1 if c2 is None else (c1, c2))
    _chk(latent), _chk(q)
    B, _, T = latent.shape
    D2 = torch.empty(2 * B, 256, T, device=latent.device, dtype=torch.float32)
    ev = _hbm("mix_fwd_shared", latent, z1, z2r, D2)
    _lib.check(L.nef_mix_fwd_shared(_p(latent), _p(z1), _p(z2r), _p(q), _p(D2), B, V, T, c1, c2, cdev, _stream()),
               "nef_mix_fwd_shared")
    _done(ev)
    return D2


def lead_mean_mix_shared(z1, z2r, q, V, c1, c2=None):
    """lead_mean + mix_fwd_shared in one pass: (latent [B,256,T], D2 [2B,256,T]), bit-identical to the two calls."""
    L = _lib.load()
    c1, c2, cdev = _choice(c1 if c2 is None else (c1, c2))
    _chk(z1), _chk(z2r), _chk(q)
    B, _, T = z1.shape
    latent = torch.empty(B, 256, T, device=z1.device, dtype=torch.float32)
    D2 = torch.empty(2 * B, 256, T, device=z1.device, dtype=torch.float32)
    ev = _hbm("lead_mean_mix_shared", z1, z2r, latent, D2)
    _lib.check(L.nef_lead_mean_mix_shared(_p(z1), _p(z2r), _p(q), _p(latent), _p(D2), B, V, T, c1, c2, cdev, _stream()),
               "nef_lead_mean_mix_shared")
    _done(ev)
    return latent, D2


UNPOOL_MIX_MAX_V = 12        # NEF_UNPOOL_MIX_MAX_V: the leads' segment samples of a row in one wave's LDS strip
UNPOOL_MIX_MAX_T = 1936      # NEF_UNPOOL_MIX_MAX_T: two gradient rows per wave, four waves, in 64 KiB of LDS


def lead_mean_mix_unpool(z1, z2b, rois, q, V, choice, T, status=None):
    """roi_unpool_fwd + lead_mean_mix_shared without the un-pooled tensor between them: (latent [B,256,T], D2 [2B,256,T]) straight
    from the segment tensor z2b [B,128V,7,32], bit-identical to the two calls.  V <= UNPOOL_MIX_MAX_V."""
    L = _lib.load()
    c1, c2, cdev = _choice(choice)
    _chk(z1), _chk(z2b), _chk(q), _chk(rois, torch.int64)
    B = z1.shape[0]
    assert z1.shape == (B, 128 * V, T) and z2b.shape == (B, 128 * V, N_SEG, 2 * ROI_BINS) and V <= UNPOOL_MIX_MAX_V
    latent = torch.empty(B, 256, T, device=z1.device, dtype=torch.float32)
    D2 = torch.empty(2 * B, 256, T, device=z1.device, dtype=torch.float32)
    ev = _hbm("lead_mean_mix_unpool", z1, z2b, latent, D2)
    _lib.check(L.nef_lead_mean_mix_unpool(_p(z1), _p(z2b), _p(rois), _p(q), _p(latent), _p(D2), _p(status), B, V, T, c1, c2, cdev,
                                          _stream()), "nef_lead_mean_mix_unpool")
    _done(ev)
    return latent, D2


def mix_bwd_shared_unpool(gD, latent, z1, z2b, rois, q, V, choice, relu_z1=False, chan_sum=False):
    """mix_bwd_shared_up (on the gradient wrt D2 itself, [2B,256,T]) + roi_unpool_bwd without gz2r between them:
    (gz1 [B,128V,T], gz2b [B,128V,7,32], gq [B,256]), bit-identical to the two calls.  T <= UNPOOL_MIX_MAX_T.
    `chan_sum`: chan_sum(gz1) [128V] follows, formed by the kernel that stores gz1 where the shape allows."""
    L = _lib.load()
    c1, c2, cdev = _choice(choice)
    _chk(gD), _chk(latent), _chk(z1), _chk(z2b), _chk(q), _chk(rois, torch.int64)
    B, _, T = latent.shape
    assert gD.shape == (2 * B, 256, T) and z2b.shape == (B, 128 * V, N_SEG, 2 * ROI_BINS) and 2 <= T <= UNPOOL_MIX_MAX_T
    gz1, gz2b = torch.empty_like(z1), torch.empty_like(z2b)
    gq = torch.empty(B, 256, device=latent.device, dtype=torch.float32)
    ev = _hbm("mix_bwd_shared_unpool", gD, latent, z1, z2b, gz1, gz2b)
    if chan_sum:
        cs = torch.empty(128 * V, device=latent.device, dtype=torch.float32)
        n = L.nef_mix_bwd_unpool_rs_ws_bytes(B, V)
        ws = workspace(n, latent.device)
        _lib.check(L.nef_mix_bwd_unpool_rs(_p(gD), _p(latent), _p(z1), _p(z2b), _p(rois), _p(q), _p(gz1), _p(gz2b), _p(gq), _p(cs), _p(ws),
                                           n, None, B, V, T, c1, c2, cdev, int(relu_z1), _stream()), "nef_mix_bwd_unpool_rs")
        _done(ev)
        return gz1, gz2b, gq, cs
    _lib.check(L.nef_mix_bwd_unpool(_p(gD), _p(latent), _p(z1), _p(z2b), _p(rois), _p(q), _p(gz1), _p(gz2b), _p(gq), B, V, T, c1, c2,
                                    cdev, int(relu_z1), _stream()), "nef_mix_bwd_unpool")
    _done(ev)
    return gz1, gz2b, gq


def mix_bwd_shared_up(gU2, latent, z1, z2r, q, V, c1, c2=None, relu_z1=False):
    """mix_bwd for the two-pass gradient wrt the shared input: gU2 [2B,256,2T] wrt its x2-upsampled form (the adjoint is taken on
    the fly), or [2B,256,T] wrt the input itself (what the polyphase backward-data pass leaves)."""
    L = _lib.load()
    c1, c2, cdev = _choice(c1 if c2 is None else (c1, c2))
    _chk(gU2)
    B, _, T = latent.shape
    up = gU2.shape[2] == 2 * T
    assert gU2.shape == (2 * B, 256, 2 * T if up else T)
    gz1, gz2r = torch.empty_like(z1), torch.empty_like(z2r)
    gq = torch.empty(B, 256, device=latent.device, dtype=torch.float32)
    name = "mix_bwd_shared_up" if up else "mix_bwd_shared"
    ev = _hbm(name, gU2, z1, z2r, gz1, gz2r)
    _lib.check(L.nef_mix_bwd(_p(gU2), _p(latent), _p(z1), _p(z2r), _p(q), _p(gz1), _p(gz2r), _p(gq), B, V, T, c1, c2, cdev,
                             int(relu_z1), int(up), 1, _stream()), "nef_mix_bwd (shared)")
    _done(ev)
    return gz1, gz2r, gq


def pass_combine_fwd(P2, bias, B):
    """P2 [2B,2C,L] (A | B half-conv outputs of the mean / picked inputs) -> c1 [3B,C,L] of the three Standin passes."""
    L = _lib.load()
    _chk(P2), _chk(bias)
    C2, Ln = P2.shape[1], P2.shape[2]
    c1 = torch.empty(3 * B, C2 // 2, Ln, device=P2.device, dtype=torch.float32)
    ev = _hbm("pass_combine_fwd", P2, c1)
    _lib.check(L.nef_pass_combine_fwd(_p(P2), _p(bias), _p(c1), B, C2 // 2, Ln, _stream()), "nef_pass_combine_fwd")
    _done(ev)
    return c1


def pass_combine_fwd_stats(P2, bias, B, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, nbt=None):
    """pass_combine_fwd + the train-mode BatchNorm statistics of its output: returns (c1, mean, invstd, a, b)."""
    L = _lib.load()
    _chk(P2), _chk(bias)
    C2, Ln = P2.shape[1], P2.shape[2]
    Ct = C2 // 2
    c1 = torch.empty(3 * B, Ct, Ln, device=P2.device, dtype=torch.float32)
    mean, invstd, a, b = (torch.empty(3, Ct, device=P2.device, dtype=torch.float32) for _ in range(4))
    n = L.nef_pass_combine_stats_ws_bytes(B, Ct)
    ws = workspace(n, P2.device)
    ev = _hbm("pass_combine_fwd", P2, c1)
    _lib.check(L.nef_pass_combine_fwd_stats(_p(P2), _p(bias), _p(c1), _p(gamma), _p(beta), _p(running_mean),
                                            _p(running_var), _p(mean), _p(invstd), _p(a), _p(b), _p(ws), n, B, Ct, Ln, eps,
                                            momentum, _p(nbt), _stream()), "nef_pass_combine_fwd_stats")
    _done(ev)
    return c1, mean, invstd, a, b


def pass_combine_bwd(gc1):
    L = _lib.load()
    _chk(gc1)
    B3, Ct, Ln = gc1.shape
    gP2 = torch.empty(2 * (B3 // 3), 2 * Ct, Ln, device=gc1.device, dtype=torch.float32)
    _lib.check(L.nef_pass_combine_bwd(_p(gc1), _p(gP2), B3 // 3, Ct, Ln, _stream()), "nef_pass_combine_bwd")
    return gP2


def mix_bwd(gD, latent, z1, z2r, q, V, c1, c2=None, upsampled=False, relu_z1=False):
    """`upsampled`: gD is the gradient wrt the x2-upsampled decoder input [3B,256,2T]; its adjoint is taken on the fly."""
    L = _lib.load()
    c1, c2, cdev = _choice(c1 if c2 is None else (c1, c2))
    _chk(gD)
    B, _, T = latent.shape
    assert gD.shape[2] == (2 * T if upsampled else T)
    gz1, gz2r = torch.empty_like(z1), torch.empty_like(z2r)
    gq = torch.empty(B, 256, device=latent.device, dtype=torch.float32)
    # relu_z1: z1 is a ReLU output; gz1 also carries that ReLU's backward mask
    _lib.check(L.nef_mix_bwd(_p(gD), _p(latent), _p(z1), _p(z2r), _p(q), _p(gz1), _p(gz2r), _p(gq), B, V, T, c1, c2, cdev,
                             int(relu_z1), int(upsampled), 0, _stream()), "nef_mix_bwd")
    return gz1, gz2r, gq


# ------------------------------------------------------------------ decoder pieces
def upsample2_fwd(x):
    L = _lib.load()
    _chk(x)
    N, Ct, T = x.shape
    y = torch.empty(N, Ct, 2 * T, device=x.device, dtype=torch.float32)
    _lib.check(L.nef_upsample2_fwd(_p(x), _p(y), N * Ct, T, _stream()), "nef_upsample2_fwd")
    return y


def upsample2_bwd(gy):
    L = _lib.load()
    _chk(gy)
    N, Ct, To = gy.shape
    gx = torch.empty(N, Ct, To // 2, device=gy.device, dtype=torch.float32)
    _lib.check(L.nef_upsample2_bwd(_p(gy), _p(gx), N * Ct, To // 2, _stream()), "nef_upsample2_bwd")
    return gx


def bn_train_stats(x, gamma, beta, running_mean, running_var, P, eps=1e-5, momentum=0.1, nbt=None):
    """Returns (mean, invstd, a, b), each [P, C]; updates the running statistics in place, pass by pass."""
    L = _lib.load()
    _chk(x)
    N, Ct, Ln = x.shape
    Bp = N // P
    mean, invstd, a, b = (torch.empty(P, Ct, device=x.device, dtype=torch.float32) for _ in range(4))
    n = L.nef_bn_ws_bytes(P, Ct)
    ws = workspace(n, x.device)
    ev = _hbm("bn_train_stats", x)
    _lib.check(L.nef_bn_train_stats(_p(x), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(mean), _p(invstd),
                                    _p(a), _p(b), _p(ws), n, P, Bp, Ct, Ln, eps, momentum, _p(nbt), _stream()), "nef_bn_train_stats")
    _done(ev)
    return mean, invstd, a, b


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=1e-5):
    L = _lib.load()
    Ct = gamma.numel()
    a = torch.empty(1, Ct, device=gamma.device, dtype=torch.float32)
    b = torch.empty(1, Ct, device=gamma.device, dtype=torch.float32)
    _lib.check(L.nef_bn_eval_affine(_p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(a), _p(b), Ct, eps,
                                    _stream()), "nef_bn_eval_affine")
    return a, b


def fold_bn(w, bias, a, b):
    """(a[co]*w[co], a*bias+b): eval-mode BatchNorm folded into the conv that feeds it."""
    L = _lib.load()
    _chk(w), _chk(bias)
    wf, bf = torch.empty_like(w), torch.empty_like(bias)
    _lib.check(L.nef_fold_bn(_p(w), _p(bias), _p(a), _p(b), _p(wf), _p(bf), w.shape[0], w.numel() // w.shape[0], _stream()),
               "nef_fold_bn")
    return wf, bf


def affine_relu_fwd(x, a, b, P):
    L = _lib.load()
    _chk(x)
    N, Ct, Ln = x.shape
    y = torch.empty_like(x)
    _lib.check(L.nef_affine_relu_fwd(_p(x), _p(a), _p(b), _p(y), P, N // P, Ct, Ln, _stream()), "nef_affine_relu_fwd")
    return y


def _bn_bwd(form, tag, hbm, x, mean, invstd, a, b, P, gx, chan_sum=True, slots=None, phase_major=False, outconv_w=False, **grad):
    """One nef_bn_relu_bwd call of kernel family `form` (nef_bn_bwd_args) writing into `gx`.  `grad`: g=..., or gout= / out= / wout=
    for form 1; `hbm`: the tensors the `tag` launch is priced by.  Returns (gx, ggamma, gbeta, sum_{b,t} gx per channel or None);
    `outconv_w` (form 1): nef_bn_relu_bwd_outconv_w, and the last conv's (gw [1,C,3], gb [1]) follow."""
    L = _lib.load()
    N, Ct, Ln = x.shape
    gg = torch.empty(Ct, device=x.device, dtype=torch.float32)
    gb = torch.empty(Ct, device=x.device, dtype=torch.float32)
    gs = torch.empty(Ct, device=x.device, dtype=torch.float32) if chan_sum else None
    A = _lib.BnBwdArgs(x=_p(x), mean=_p(mean), invstd=_p(invstd), a=_p(a), b=_p(b), gx=_p(gx), ggamma=_p(gg), gbeta=_p(gb),
                       gx_chan_sum=_p(gs), slots=_p(slots[0]) if slots else None, nslot=slots[1] if slots else 0, P=P, Bp=N // P,
                       C=Ct, L=Ln, form=form, phase_major=int(phase_major), **{k: _p(t) for k, t in grad.items()})
    A.ws_bytes = L.nef_bn_bwd_ws_bytes(C.byref(A))
    if outconv_w:
        gw = torch.empty(1, Ct, 3, device=x.device, dtype=torch.float32)
        gbo = torch.empty(1, device=x.device, dtype=torch.float32)
        n2, off = L.nef_bn_relu_bwd_outconv_w_ws_bytes(C.byref(A)), (A.ws_bytes + 255) // 256 * 256
        ws = workspace(off + n2, x.device)      # one buffer per stream: the second workspace sits behind the first
        A.ws = _p(ws)
        ev = _hbm(tag, *hbm)
        _lib.check(L.nef_bn_relu_bwd_outconv_w(C.byref(A), _p(gw), _p(gbo), ws.data_ptr() + off, n2, _stream()),
                   "nef_bn_relu_bwd_outconv_w")
        _done(ev)
        return gx, gg, gb, gs, gw, gbo
    A.ws = _p(workspace(A.ws_bytes, x.device))
    ev = _hbm(tag, *hbm)
    _lib.check(L.nef_bn_relu_bwd(C.byref(A), _stream()), f"nef_bn_relu_bwd form {form}")
    _done(ev)
    return gx, gg, gb, gs


def bn_relu_bwd(gy, x, gamma, mean, invstd, a, b, P, with_chan_sum=False, slots=None, phase_major=False):
    """Returns (gx, ggamma, gbeta[, sum_{b,t} gx per channel]).  `slots`: the conv_stats_buffer() the conv that produced
    `gy` filled (conv(..., bnb=...)) -- the reduction pass over (gy, x) is then skipped.  `phase_major`: gx comes back as
    [N, 2C, L/2], row 2c + p = positions p, p + 2, ... of channel c (the operand of the polyphase backward passes).
    `gamma` is not used: a = gamma * invstd carries it."""
    _chk(gy), _chk(x)
    N, Ct, Ln = x.shape
    gx = torch.empty(N, 2 * Ct, Ln // 2, device=x.device, dtype=torch.float32) if phase_major else torch.empty_like(x)
    r = _bn_bwd(0, "bn_relu_bwd", (gy, x, gx), x, mean, invstd, a, b, P, gx, with_chan_sum, slots, phase_major, g=gy)
    return r if with_chan_sum else r[:3]


def bn_relu_bwd_combine3(gy, x, mean, invstd, a, b, slots=None, phase_major=False):
    """pass_combine_bwd(bn_relu_bwd(gy, x, ..., P=3)) in one pass: returns (gP2 [2B,2C,L], ggamma, gbeta, chan sum of gx);
    `phase_major`: gP2 as [2B, 4C, L/2] (see bn_relu_bwd)."""
    _chk(gy), _chk(x)
    N, Ct, Ln = x.shape
    Bp = N // 3
    gP2 = torch.empty((2 * Bp, 4 * Ct, Ln // 2) if phase_major else (2 * Bp, 2 * Ct, Ln), device=x.device, dtype=torch.float32)
    return _bn_bwd(3, "bn_relu_bwd_combine3", (gy, x, gP2), x, mean, invstd, a, b, 3, gP2, slots=slots, phase_major=phase_major,
                   g=gy)


def bn_relu_bwd_up(gu, x, mean, invstd, a, b, P, slots=None):
    """bn_relu_bwd(upsample2_bwd(gu), x, ...) with the upsampling adjoint taken on the fly; gu [N,C,2L].
    Returns (gx, ggamma, gbeta, sum_{b,t} gx per channel)."""
    _chk(gu), _chk(x)
    N, Ct, Ln = x.shape
    assert gu.shape == (N, Ct, 2 * Ln)
    gx = torch.empty_like(x)
    return _bn_bwd(2, "bn_relu_bwd_up", (gu, x, gx), x, mean, invstd, a, b, P, gx, slots=slots, g=gu)


def bn_relu_bwd_outconv(gout, out, wout, x, mean, invstd, a, b, P, outconv_w=False):
    """bn_relu_bwd(outconv_bwd_data(gout, out, wout), x, ...) without materialising the [N,C,L] gradient in between.
    Returns (gx, ggamma, gbeta, sum_{b,t} gx per channel); with `outconv_w` the reduction pass also forms what
    outconv_bwd_weight(gout, out, x, pro=(a, b, N // P)) returns, and (gw, gb) follow."""
    _chk(gout), _chk(out), _chk(x)
    gx = torch.empty_like(x)
    # a two-pass pair by construction (the reduction pass reads x, the apply pass reads it again and writes gx): priced by
    # what the pair has to move -- 2 reads + 1 write of the [N, C, L] tensor (+ the small gout / out rows twice)
    return _bn_bwd(1, "bn_relu_bwd_outconv", (gout, out, x, gout, out, x, gx), x, mean, invstd, a, b, P, gx, outconv_w=outconv_w,
                   gout=gout, out=out, wout=wout)


def outconv_fwd(x, w, bias, pro=None):
    """`pro` = (a, b, Bp): x is the pre-BatchNorm tensor, relu(x*a[p,c]+b[p,c]) is applied on the fly."""
    L = _lib.load()
    _chk(x), _chk(w), _chk(bias)
    N, Ct, Ln = x.shape
    out = torch.empty(N, 1, Ln, device=x.device, dtype=torch.float32)
    a, b, Bp = pro if pro is not None else (None, None, 1)
    ev = _hbm("outconv_fwd", x, out)
    _lib.check(L.nef_outconv_fwd(_p(x), _p(a), _p(b), Bp, _p(w), _p(bias), _p(out), N, Ct, Ln, _stream()), "nef_outconv_fwd")
    _done(ev)
    return out


def outconv_bwd_data(gout, out, w, Ct):
    L = _lib.load()
    _chk(gout), _chk(out)
    N, Ln = out.shape[0], out.shape[-1]
    gx = torch.empty(N, Ct, Ln, device=out.device, dtype=torch.float32)
    _lib.check(L.nef_outconv_bwd_data(_p(gout), _p(out), _p(w), _p(gx), N, Ct, Ln, _stream()), "nef_outconv_bwd_data")
    return gx


def outconv_bwd_weight(gout, out, x, pro=None):
    L = _lib.load()
    _chk(gout), _chk(out), _chk(x)
    N, Ct, Ln = x.shape
    gw = torch.empty(1, Ct, 3, device=x.device, dtype=torch.float32)
    gb = torch.empty(1, device=x.device, dtype=torch.float32)
    n = L.nef_outconv_bwd_weight_ws_bytes(Ct)
    ws = workspace(n, x.device)
    a, b, Bp = pro if pro is not None else (None, None, 1)
    ev = _hbm("outconv_bwd_weight", gout, out, x)
    _lib.check(L.nef_outconv_bwd_weight(_p(gout), _p(out), _p(x), _p(a), _p(b), Bp, _p(gw), _p(gb), _p(ws), n, N, Ct, Ln,
                                        _stream()), "nef_outconv_bwd_weight")
    _done(ev)
    return gw, gb


# ------------------------------------------------------------------ loss / optimiser
def loss_fwd(pred, pred_p, pred_l, target, factors, reg_l2, use_mask, out=None, noise=None):
    """`noise`: None, or cfg.DATA.noise's addend in pred's layout -- every term is taken at pred + noise (reference solver.py:185-186).
    None is nef_loss_fwd: the same launches with a null pointer."""
    L = _lib.load()
    for t in (pred, pred_p, pred_l, target):
        _chk(t)
    if noise is not None and _chk(noise).numel() != pred.numel():
        raise ValueError(f"noise {tuple(noise.shape)} does not have the prediction's {tuple(pred.shape)} elements")
    losses = torch.empty(4, device=pred.device, dtype=torch.float32) if out is None else out
    n = L.nef_loss_ws_bytes()
    ws = workspace(n, pred.device)
    _lib.check(L.nef_loss_noise_fwd(_p(pred), _p(pred_p), _p(pred_l), _p(target), _p(noise), _p(losses), _p(ws), n, pred.numel(),
                                    factors[0], factors[1], factors[2], int(reg_l2), use_mask, _stream()), "nef_loss_noise_fwd")
    return losses


def loss_bwd(pred, pred_p, pred_l, target, gscale, factors, reg_l2, use_mask, noise=None):
    L = _lib.load()
    if noise is not None and _chk(noise).numel() != pred.numel():
        raise ValueError(f"noise {tuple(noise.shape)} does not have the prediction's {tuple(pred.shape)} elements")
    # the three gradients as ONE [3B, 1, L] buffer (views): engine._head_bwd takes it as the stacked decoder-output gradient as is
    g3 = torch.empty((3 * pred.shape[0],) + tuple(pred.shape[1:]), device=pred.device, dtype=torch.float32)
    g_pred, g_p, g_l = g3[0:pred.shape[0]], g3[pred.shape[0]:2 * pred.shape[0]], g3[2 * pred.shape[0]:]
    _lib.check(L.nef_loss_noise_bwd(_p(pred), _p(pred_p), _p(pred_l), _p(target), _p(noise), _p(gscale), _p(g_pred), _p(g_p),
                                    _p(g_l), pred.numel(), factors[0], factors[1], factors[2], int(reg_l2), use_mask, _stream()),
               "nef_loss_noise_bwd")
    return g_pred, g_p, g_l


def _row_term_args(what, pred, target, factor, rois, noise, max_rows=None, eps=None, g_pred=None, gscale=None):
    """The checks and the shape (B, L) the entries of a row term ('ssim', 'slope', 'correlation') share: pred / target [B, 1, L] (or
    [Q, B, 1, L], [B, L]), rois None or int64 [B, 7, 2], noise None or pred's elements.  `max_rows`: the row cap of the slope and correlation
    kernels, which also reject an empty prediction; `eps`: the correlation term's; `g_pred`, `gscale`: a backward entry's."""
    _chk(pred), _chk(target)
    if pred.dim() < 2 or target.numel() != pred.numel() or (max_rows is not None and pred.numel() == 0):
        raise ValueError(f"prediction {tuple(pred.shape)} and target {tuple(target.shape)} must hold the same [B, 1, L] rows")
    Ln = pred.shape[-1]
    B = pred.numel() // Ln
    if max_rows is not None and B > max_rows:
        raise ValueError(f"prediction {tuple(pred.shape)}: {B} rows is more than the {max_rows} the {what} kernels take")
    if noise is not None and _chk(noise).numel() != pred.numel():
        raise ValueError(f"noise {tuple(noise.shape)} does not have the prediction's {tuple(pred.shape)} elements")
    if rois is not None and (_chk(rois, torch.int64).dim() != 3 or tuple(rois.shape) != (B, N_SEG, 2)):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, {N_SEG}, 2]")
    if not float(factor) >= 0.0:
        raise ValueError(f"Invalid {what} factor: {factor}")
    if eps is not None and not float(eps) >= 0.0:
        raise ValueError(f"Invalid {what} eps: {eps}")
    if g_pred is not None and _chk(g_pred).numel() != pred.numel():
        raise ValueError(f"g_pred {tuple(g_pred.shape)} does not have the prediction's {tuple(pred.shape)} elements")
    if gscale is not None:
        _chk(gscale)
    return B, Ln


def _row_term_call(tag, A, *hbm):
    """The entry nef_<tag> on the filled struct `A`, priced for bench.py by the tensors `hbm`."""
    ev = _hbm(tag, *hbm)
    _lib.check(getattr(_lib.load(), "nef_" + tag)(C.byref(A), _stream()), "nef_" + tag)
    _done(ev)


LOSS_SSIM_TILE = 512      # NEF_LOSS_SSIM_TILE (include/nefnet_hip.h): window starts / positions per block of the two SSIM kernels


def loss_ssim_fwd(pred, target, losses, factor, rois=None, noise=None):
    """The SSIM term of the training loss behind loss_fwd (nef_loss_ssim_fwd, include/nefnet_hip.h): losses[4] = factor * (1 - mean SSIM
    of pred (+ noise) against target over the rows with a 7-tap window on [0, rois[i, -1, 0]), whole rows with rois None) and
    losses[0] += losses[4].  `losses`: the FIVE-element row whose first four elements loss_fwd(out=) has written.  Two launches,
    capturable."""
    B, Ln = _row_term_args("ssim", pred, target, factor, rois, noise)
    _chk(losses)
    assert losses.numel() == 5, losses.shape
    n = _lib.load().nef_loss_ssim_ws_bytes(B, Ln)
    ws = workspace(n, pred.device)
    A = _lib.LossSsimArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=_p(losses), ws=_p(ws), ws_bytes=n,
                          gscale=None, g_pred=None, B=B, L=Ln, factor=float(factor))
    _row_term_call("loss_ssim_fwd", A, pred, target, noise)
    return losses


def loss_ssim_bwd(pred, target, g_pred, factor, rois=None, noise=None, gscale=None):
    """g_pred += gscale * d(SSIM term) / d pred behind loss_bwd (nef_loss_ssim_bwd): `g_pred` is loss_bwd's first gradient, the first
    third of its [3B, 1, L] buffer.  Positions at or behind a row's end and rows without a window keep their bits.  `gscale`: None (1) or
    loss_bwd's device word.  One launch, capturable, no state: the row count is re-derived from `rois` on the device."""
    B, Ln = _row_term_args("ssim", pred, target, factor, rois, noise, g_pred=g_pred, gscale=gscale)
    A = _lib.LossSsimArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=None, ws=None, ws_bytes=0,
                          gscale=_p(gscale), g_pred=_p(g_pred), B=B, L=Ln, factor=float(factor))
    _row_term_call("loss_ssim_bwd", A, pred, target, noise, g_pred, g_pred)
    return g_pred


AUGMENT_TILE = 1024      # NEF_AUGMENT_TILE (include/nefnet_hip.h): positions of a row per workgroup of nef_augment


def augment(x, rois, aug, seed=0, seed_dev=None, out=None):
    """The input leads `x` [B, V, L] corrupted as cfg.DATA.aug_* say (`aug`: augment.from_cfg's Augment; nef_augment, include/nefnet_hip.h,
    defines every draw): a new tensor, or `out`; `x` is never written.  `aug` None: `x` itself, no launch.  `rois`: the batch's integer
    [B, R, 2] rows on x's device (read with aug.crop only).  `seed`: the launch's 64-bit seed word (augment.train_seed / eval_seed);
    `seed_dev`: None, or a one-element int64 device tensor added to it when the launch runs (the replayed step's seed word, with
    seed = augment.site_word()).  One launch, capturable.  Every argument check sits in front of the library."""
    if aug is None:
        return x
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise TypeError(f"x must be a float32 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 3 or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous [B, V, L] tensor, got {tuple(x.shape)} with strides {tuple(x.stride())}")
    B, V, Ln = x.shape
    if min(B, V, Ln) < 1 or Ln % 4 != 0:
        raise ValueError(f"x {tuple(x.shape)}: B, V, L >= 1 and L a multiple of 4")
    if not torch.is_tensor(rois) or rois.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"rois must be an integer tensor [B, R, 2], got {getattr(rois, 'dtype', type(rois))}")
    if rois.dim() != 3 or rois.shape[0] != B or rois.shape[1] < 1 or rois.shape[2] != 2:
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, R, 2]")
    if rois.device != x.device:
        raise ValueError(f"rois is on {rois.device}, x on {x.device}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
            raise ValueError("out must be a contiguous float32 tensor of x's shape on x's device")
        if out.data_ptr() == x.data_ptr():
            raise ValueError("out is x: the corruption is out of place, the loader's tensor is never modified")
    if seed_dev is not None and (not torch.is_tensor(seed_dev) or seed_dev.dtype != torch.int64 or seed_dev.numel() != 1
                                 or seed_dev.device != x.device):
        raise ValueError("seed_dev must be a one-element int64 tensor on x's device")
    if not x.is_cuda:
        raise RuntimeError("ops.augment runs on a HIP device only (no CPU path)")
    if x.data_ptr() % 16 != 0:
        raise ValueError("x is not 16-byte aligned")
    L = _lib.load()
    rois = rois.to(torch.int64).contiguous()
    y = torch.empty_like(x) if out is None else out
    ev = _hbm("augment", x, y)
    A = _lib.AugmentArgs(x=_p(x), rois=_p(rois), y=_p(y), seed_dev=_p(seed_dev), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                         wander_amp=aug.wander_amp, wander_lo=aug.wander_lo, wander_hi=aug.wander_hi, hum_amp=aug.hum_amp,
                         hum_hz=aug.hum_hz, sample_rate=aug.sample_rate, noise_std=aug.noise_std, lead_drop=aug.lead_drop,
                         B=B, V=V, L=Ln, R=rois.shape[1], crop=int(bool(aug.crop)))
    _lib.check(L.nef_augment(C.byref(A), _stream()), "nef_augment")
    _done(ev)
    return y


def noise_row(target, rois, seed, seed_dev=None, out=None, sigma_out=None):
    """cfg.DATA.device_noise's addend of the loss (nef_noise_row, include/nefnet_hip.h, defines it): per target row a Gaussian draw whose
    sigma is the standard deviation of the quiet second half of the row's T-P segment, +0.0 at and behind the row's end.  `target`: the
    step's final float32 target rows, [B, 1, L], [Q, B, 1, L] or [Rw, L], contiguous; `rois`: int64 [Rw, 7, 2] on target's device, one per
    row (a multi-view step's are tiled per view by the caller).  Returns a new tensor of target's shape, or `out`; `target` is never
    written.  `seed`: the launch's 64-bit seed word (device_noise.train_seed); `seed_dev`: None, or a one-element int64 device tensor added
    to it when the launch runs (the replayed step's seed word, with seed = device_noise.site_word()).  `sigma_out`: None, or a float64
    [Rw] tensor that receives every row's sigma.  One launch, capturable.  Every argument check sits in front of the library."""
    if not torch.is_tensor(target) or target.dtype != torch.float32:
        raise TypeError(f"target must be a float32 tensor, got {getattr(target, 'dtype', type(target))}")
    if target.dim() < 2 or not target.is_contiguous() or target.numel() == 0:
        raise ValueError(f"target must be a contiguous tensor of [.., L] rows, got {tuple(target.shape)} with strides {tuple(target.stride())}")
    Ln = target.shape[-1]
    Rw = target.numel() // Ln
    if Ln % 4 != 0:
        raise ValueError(f"target {tuple(target.shape)}: L a multiple of 4")
    if not torch.is_tensor(rois) or rois.dtype != torch.int64:
        raise TypeError(f"rois must be an int64 tensor [{Rw}, {N_SEG}, 2], got {getattr(rois, 'dtype', type(rois))}")
    if tuple(rois.shape) != (Rw, N_SEG, 2) or not rois.is_contiguous():
        raise ValueError(f"rois {tuple(rois.shape)} is not a contiguous [{Rw}, {N_SEG}, 2]")
    if rois.device != target.device:
        raise ValueError(f"rois is on {rois.device}, target on {target.device}")
    if out is not None:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or out.numel() != target.numel() or not out.is_contiguous()
                or out.device != target.device):
            raise ValueError("out must be a contiguous float32 tensor of target's elements on target's device")
        if out.data_ptr() == target.data_ptr():
            raise ValueError("out is target: the row is made out of place, the target is never modified")
    if sigma_out is not None and (not torch.is_tensor(sigma_out) or sigma_out.dtype != torch.float64 or tuple(sigma_out.shape) != (Rw,)
                                  or not sigma_out.is_contiguous() or sigma_out.device != target.device):
        raise ValueError(f"sigma_out must be a contiguous float64 tensor [{Rw}] on target's device")
    if seed_dev is not None and (not torch.is_tensor(seed_dev) or seed_dev.dtype != torch.int64 or seed_dev.numel() != 1
                                 or seed_dev.device != target.device):
        raise ValueError("seed_dev must be a one-element int64 tensor on target's device")
    if not target.is_cuda:
        raise RuntimeError("ops.noise_row runs on a HIP device only (no CPU path)")
    if target.data_ptr() % 16 != 0 or (out is not None and out.data_ptr() % 16 != 0):
        raise ValueError("target / out is not 16-byte aligned")
    L = _lib.load()
    y = torch.empty_like(target) if out is None else out
    ev = _hbm("noise_row", y)
    A = _lib.NoiseRowArgs(target=_p(target), rois=_p(rois), out=_p(y), sigma=_p(sigma_out), seed_dev=_p(seed_dev),
                          seed=int(seed) & 0xFFFFFFFFFFFFFFFF, Rw=Rw, L=Ln)
    _lib.check(L.nef_noise_row(C.byref(A), _stream()), "nef_noise_row")
    _done(ev)
    return y


LEAD_MASK_MAX_V = 12      # NEF_LEAD_MASK_MAX_V (include/nefnet_hip.h)


def lead_mask_arg(mask, B, V, device, what="lead_mask"):
    """`mask` as the uint8 [B, V] tensor the lead-mask entries read (torch.bool through a view).  Shape, dtype and device are checked;
    the content is not -- nothing is read by the host."""
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{what} must be a bool or uint8 tensor [B, V], got {getattr(mask, 'dtype', type(mask))}")
    if tuple(mask.shape) != (B, V):
        raise ValueError(f"{what} {tuple(mask.shape)} is not [{B}, {V}]")
    if mask.device != device:
        raise ValueError(f"{what} is on {mask.device}, the leads on {device}")
    mask = mask if mask.is_contiguous() else mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _lead_mask_leads(z1, z2r):
    for name, t in (("z1", z1), ("z2r", z2r)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous [B, 128 V, T] tensor, got {tuple(t.shape)} with strides {tuple(t.stride())}")
    B, Ct, T = z1.shape
    if B < 1 or T < 1 or Ct % 128 != 0 or not 1 <= Ct // 128 <= LEAD_MASK_MAX_V:
        raise ValueError(f"z1 {tuple(z1.shape)}: [B, 128 V, T] with B, T >= 1 and V in 1..{LEAD_MASK_MAX_V}")
    if z2r.shape != z1.shape or z2r.device != z1.device:
        raise ValueError(f"z2r {tuple(z2r.shape)} on {z2r.device} does not match z1 {tuple(z1.shape)} on {z1.device}")
    return B, Ct // 128, T


def _lead_mask_choice(choice, device):
    """The Standin draws: two ints >= 0, or a device int32[2] tensor (graph replay) -> (c1, c2, device pointer)."""
    if torch.is_tensor(choice):
        if choice.dtype != torch.int32 or choice.numel() != 2 or not choice.is_contiguous() or choice.device != device:
            raise ValueError("choice must be two ints or a contiguous int32 tensor of two elements on the leads' device")
        return 0, 0, choice.data_ptr()
    try:
        c1, c2 = choice
        if isinstance(c1, bool) or isinstance(c2, bool):
            raise TypeError
        c1, c2 = int(c1), int(c2)
    except (TypeError, ValueError):
        raise TypeError(f"choice must be two ints or a device int32[2] tensor, got {choice!r}") from None
    if c1 < 0 or c2 < 0 or c1 > 0x7FFFFFFF or c2 > 0x7FFFFFFF:
        raise ValueError(f"choice {choice!r}: both draws must be in 0 .. 2^31 - 1")
    return c1, c2, None


def _lead_mask_f32(name, t, shape, device):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {list(shape)} tensor, got {tuple(t.shape)} with strides {tuple(t.stride())}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the leads on {device}")


def lead_mask_mix_fwd(z1, z2r, mask, q, choice=(0, 0), picks=False):
    """The lead mean and the Standin mixes over each sample's present leads (nef_lead_mask_mix_fwd, include/nefnet_hip.h, defines every
    element): z1, z2r [B, 128 V, T], mask bool / uint8 [B, V], q [B, 256] -> (latent [B, 256, T], D [3B, 256, T]); `q` None: (latent,
    None), the inference form.  `choice`: the two Standin draws, ints or a device int32[2] tensor; sample b picks its
    (draw mod n_b)-th present lead.  picks=True: a third result, int32 [B, 2], the picked leads (-1 without a present lead).  One launch,
    capturable.  Every argument check sits in front of the library."""
    B, V, T = _lead_mask_leads(z1, z2r)
    mask = lead_mask_arg(mask, B, V, z1.device, "mask")
    if q is not None:
        _lead_mask_f32("q", q, (B, 256), z1.device)
    c1, c2, cdev = _lead_mask_choice(choice, z1.device)
    if not z1.is_cuda:
        raise RuntimeError("ops.lead_mask_mix_fwd runs on a HIP device only (no CPU path)")
    L = _lib.load()
    latent = torch.empty(B, 256, T, device=z1.device, dtype=torch.float32)
    D = torch.empty(3 * B, 256, T, device=z1.device, dtype=torch.float32) if q is not None else None
    pk = torch.empty(B, 2, device=z1.device, dtype=torch.int32) if picks else None
    ev = _hbm("lead_mask_mix_fwd", z1, z2r, latent, D)
    A = _lib.LeadMaskMixFwdArgs(z1=_p(z1), z2r=_p(z2r), mask=_p(mask), q=_p(q), choice_dev=cdev, latent=_p(latent), D=_p(D), picks=_p(pk),
                                B=B, V=V, T=T, c1=c1, c2=c2)
    _lib.check(L.nef_lead_mask_mix_fwd(C.byref(A), _stream()), "nef_lead_mask_mix_fwd")
    _done(ev)
    return (latent, D, pk) if picks else (latent, D)


def lead_mask_mix_bwd(gD, latent, z1, z2r, q, mask, choice=(0, 0), up=False, relu_z1=False):
    """The adjoint of lead_mask_mix_fwd (nef_lead_mask_mix_bwd): gD [3B, 256, T] -- [3B, 256, 2T] with `up`, the gradient wrt the
    x2-upsampled D, whose adjoint is taken while reading -- and the forward's latent, leads, q, mask and draws -> (gz1, gz2r
    [B, 128 V, T], gq [B, 256]).  Rows of absent leads are zeros.  relu_z1: gz1 also carries the mask z1 > 0.  One launch, capturable,
    no atomics.  Every argument check sits in front of the library."""
    B, V, T = _lead_mask_leads(z1, z2r)
    mask = lead_mask_arg(mask, B, V, z1.device, "mask")
    _lead_mask_f32("gD", gD, (3 * B, 256, 2 * T if up else T), z1.device)
    _lead_mask_f32("latent", latent, (B, 256, T), z1.device)
    _lead_mask_f32("q", q, (B, 256), z1.device)
    c1, c2, cdev = _lead_mask_choice(choice, z1.device)
    if not z1.is_cuda:
        raise RuntimeError("ops.lead_mask_mix_bwd runs on a HIP device only (no CPU path)")
    L = _lib.load()
    gz1, gz2r = torch.empty_like(z1), torch.empty_like(z2r)
    gq = torch.empty(B, 256, device=z1.device, dtype=torch.float32)
    ev = _hbm("lead_mask_mix_bwd", gD, latent, z1, z2r, gz1, gz2r)
    A = _lib.LeadMaskMixBwdArgs(gD=_p(gD), latent=_p(latent), z1=_p(z1), z2r=_p(z2r), q=_p(q), mask=_p(mask), choice_dev=cdev,
                                gz1=_p(gz1), gz2r=_p(gz2r), gq=_p(gq), B=B, V=V, T=T, c1=c1, c2=c2, relu_z1=int(bool(relu_z1)),
                                up=int(bool(up)))
    _lib.check(L.nef_lead_mask_mix_bwd(C.byref(A), _stream()), "nef_lead_mask_mix_bwd")
    _done(ev)
    return gz1, gz2r, gq


def augment_mask(B, V, lead_drop, seed=0, seed_dev=None, device=None, out=None):
    """uint8 [B, V]: 0 where ops.augment with the same seed, seed_dev and lead_drop zeroes the lead, 1 elsewhere (nef_augment_mask: the
    decision is one device function shared with nef_augment).  `device`: where the mask lives (taken from `out` or `seed_dev` when None).
    `out`: a contiguous uint8 [B, V] tensor to fill (the replayed step's static buffer).  One launch, capturable.  Every argument check
    sits in front of the library."""
    for name, n in (("B", B), ("V", V)):
        if isinstance(n, bool) or not isinstance(n, int):
            raise TypeError(f"{name} must be an int, got {n!r}")
    if B < 1 or not 1 <= V <= LEAD_MASK_MAX_V or B * V > 0x7FFFFFFF:
        raise ValueError(f"B = {B}, V = {V}: B >= 1, V in 1..{LEAD_MASK_MAX_V}")
    if not 0.0 <= float(lead_drop) < 1.0:
        raise ValueError(f"lead_drop must be in [0, 1), got {lead_drop!r}")
    if device is None:
        device = out.device if torch.is_tensor(out) else (seed_dev.device if torch.is_tensor(seed_dev) else None)
    if device is None:
        raise ValueError("augment_mask needs a device (or `out` / `seed_dev` to take it from)")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None and torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (B, V) or not out.is_contiguous()
                            or out.device != device):
        raise ValueError(f"out must be a contiguous uint8 [{B}, {V}] tensor on {device}")
    if seed_dev is not None and (not torch.is_tensor(seed_dev) or seed_dev.dtype != torch.int64 or seed_dev.numel() != 1
                                 or seed_dev.device != device):
        raise ValueError(f"seed_dev must be a one-element int64 tensor on {device}")
    if device.type != "cuda":
        raise RuntimeError("ops.augment_mask runs on a HIP device only (no CPU path)")
    L = _lib.load()
    mask = torch.empty(B, V, device=device, dtype=torch.uint8) if out is None else out
    A = _lib.AugmentMaskArgs(mask=_p(mask), seed_dev=_p(seed_dev), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, lead_drop=float(lead_drop), B=B, V=V)
    _lib.check(L.nef_augment_mask(C.byref(A), _stream()), "nef_augment_mask")
    return mask


def warp(data, target, rest, rois, warp, seed, index0=0):
    """The batch warped in time as cfg.DATA.aug_warp / aug_roi_jitter say (`warp`: warp.from_cfg's Warp; nef_warp, include/nefnet_hip.h,
    defines every step) -> (data, target, rest, rois), all new tensors; no input is written.  `data` [B, V, L], `target` [B, L] or
    [B, 1, L] (returned in the shape given), `rest` [B, R, L] or None (None back), `rois` [B, 7, 2] integer (int64 back): float32,
    contiguous, on one HIP device.  `warp` None: the four inputs themselves, no launch.  `seed`: the launch's 64-bit seed word
    (warp.train_seed / eval_seed); sample i draws as sample `index0` + i.  One launch, capturable.  Every argument check sits in front of
    the library."""
    if warp is None:
        return data, target, rest, rois
    for name, t in (("data", data), ("target", target)) + ((("rest", rest),) if rest is not None else ()):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got {tuple(t.shape)} with strides {tuple(t.stride())}")
    if data.dim() != 3:
        raise ValueError(f"data must be [B, V, L], got {tuple(data.shape)}")
    B, V, Ln = data.shape
    if B < 1 or not 1 <= V <= 12 or not 4 <= Ln <= 1 << 24 or Ln % 4 != 0:
        raise ValueError(f"data {tuple(data.shape)}: B >= 1, V in 1..12, L a multiple of 4 in 4..2^24")
    if tuple(target.shape) not in ((B, Ln), (B, 1, Ln)):
        raise ValueError(f"target {tuple(target.shape)} is neither [{B}, {Ln}] nor [{B}, 1, {Ln}]")
    R = 0
    if rest is not None:
        if rest.dim() != 3 or rest.shape[0] != B or rest.shape[2] != Ln or not 1 <= rest.shape[1] <= BEAT_MAX_REST:
            raise ValueError(f"rest {tuple(rest.shape)} is not [{B}, R, {Ln}] with R in 1..{BEAT_MAX_REST}")
        R = rest.shape[1]
    if not torch.is_tensor(rois) or rois.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"rois must be an integer tensor [B, 7, 2], got {getattr(rois, 'dtype', type(rois))}")
    if tuple(rois.shape) != (B, 7, 2):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, 7, 2]")
    for name, t in (("target", target), ("rest", rest), ("rois", rois)):
        if t is not None and t.device != data.device:
            raise ValueError(f"{name} is on {t.device}, data on {data.device}")
    amp = tuple(float(a) for a in warp.amp)
    if len(amp) != 6 or not all(0.0 <= a <= 0.9 for a in amp):
        raise ValueError(f"warp.amp {warp.amp!r}: six amplitudes in [0, 0.9]")
    if isinstance(warp.jitter, bool) or not isinstance(warp.jitter, int) or not 0 <= warp.jitter <= 64:
        raise ValueError(f"warp.jitter {warp.jitter!r}: an integer in 0..64")
    if not -(1 << 60) <= int(index0) < 1 << 60:
        raise ValueError(f"index0 {index0!r} is outside +-2^60")
    if not data.is_cuda:
        raise RuntimeError("ops.warp runs on a HIP device only (no CPU path)")
    rois = rois.to(torch.int64).contiguous()
    for name, t in (("data", data), ("target", target), ("rest", rest), ("rois", rois)):
        if t is not None and t.data_ptr() % 16 != 0:
            raise ValueError(f"{name} is not 16-byte aligned")
    L = _lib.load()
    data_o, target_o, rois_o = torch.empty_like(data), torch.empty_like(target), torch.empty_like(rois)
    rest_o = torch.empty_like(rest) if rest is not None else None
    ev = _hbm("warp", data, target, rest, rois, data_o, target_o, rest_o, rois_o)
    A = _lib.WarpArgs(data=_p(data), target=_p(target), rest=_p(rest), rois=_p(rois), data_out=_p(data_o), target_out=_p(target_o),
                      rest_out=_p(rest_o), rois_out=_p(rois_o), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, index0=int(index0),
                      amp=(C.c_double * 6)(*amp), jitter=warp.jitter, B=B, V=V, R=R, L=Ln)
    _lib.check(L.nef_warp(C.byref(A), _stream()), "nef_warp")
    _done(ev)
    return data_o, target_o, rest_o, rois_o


BEAT_LEN = 512           # NEF_BEAT_LEN (include/nefnet_hip.h): samples of a row of nef_beat_batch
BEAT_MAX_REST = 64       # the largest R nef_beat_batch takes


def _check_beat_plan(signal, plan, V, R, who):
    """The argument checks ops.beat_batch and ops.beat_range share; returns (V, R) as ints."""
    if not torch.is_tensor(signal) or signal.dtype not in (torch.int16, torch.float32):
        raise TypeError(f"signal must be an int16 or float32 tensor, got {getattr(signal, 'dtype', type(signal))}")
    if signal.dim() != 1 or signal.numel() < 1 or not signal.is_contiguous():
        raise ValueError(f"signal must be a non-empty contiguous 1-D tensor, got {tuple(signal.shape)}")
    V, R = int(V), int(R)
    if not 1 <= V <= 12 or not 0 <= R <= BEAT_MAX_REST:
        raise ValueError(f"V = {V}, R = {R}: 1 <= V <= 12 input leads and 0 <= R <= {BEAT_MAX_REST} rest leads")
    if not torch.is_tensor(plan) or plan.dtype != torch.int64:
        raise TypeError(f"plan must be an int64 tensor, got {getattr(plan, 'dtype', type(plan))}")
    W = 3 + V + 1 + R
    if plan.dim() != 2 or plan.shape[0] < 1 or plan.shape[1] != W or not plan.is_contiguous():
        raise ValueError(f"plan {tuple(plan.shape)} is not a contiguous [B >= 1, {W}] table (3 + V + 1 + R words per sample)")
    if not plan.is_cuda:
        off, stride, n = plan[:, 0], plan[:, 1], plan[:, 2]
        bad = (off < 0) | (stride < 1) | (n < 1) | (n > stride) | (off + 7 * stride + n > signal.numel()) | \
              ((plan[:, 3:] < 0) | (plan[:, 3:] > 11)).any(dim=1)
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            raise ValueError(f"plan row {i} {plan[i].tolist()} leaves the signal of {signal.numel()} elements or names a lead outside 0..11")
    elif plan.device != signal.device:
        raise ValueError(f"plan is on {plan.device}, signal on {signal.device}")
    if not signal.is_cuda:
        raise RuntimeError(f"ops.{who} runs on a HIP device only (no CPU path)")
    if signal.data_ptr() % 16 != 0:
        raise ValueError("signal is not 16-byte aligned")
    return V, R


def beat_batch(signal, plan, V, R):
    """One batch of Tianchi beats built from device-resident recordings (nef_beat_batch, include/nefnet_hip.h; the batches of
    cfg.DATA.device_resident): `signal` is the store's flat int16 or float32 device tensor, `plan` the int64 [B, 3 + V + 1 + R] table of
    dataset/resident.py's draw_plan -- per sample [offset of lead 0 at p_on, lead stride, n, V input leads, target lead, R rest leads].  A plan
    on the host is checked against `signal` here, row by row, and copied; one that is on the device already is taken as it is (the kernel
    gives a row that leaves `signal` NaNs, and reads nothing).  Returns fresh float32 (data [B, V, 512], target_view [B, 512],
    rest_view [B, R, 512]); one launch on the current stream, capturable with a device plan.  Every argument check sits in front of the library."""
    V, R = _check_beat_plan(signal, plan, V, R, "beat_batch")
    L = _lib.load()
    if not plan.is_cuda:
        plan = plan.to(signal.device, non_blocking=True)
    B = plan.shape[0]
    data = torch.empty((B, V, BEAT_LEN), dtype=torch.float32, device=signal.device)
    target = torch.empty((B, BEAT_LEN), dtype=torch.float32, device=signal.device)
    rest = torch.empty((B, R, BEAT_LEN), dtype=torch.float32, device=signal.device)
    ev = _hbm("beat_batch", plan, data, target, rest)
    A = _lib.BeatBatchArgs(signal=_p(signal), plan=_p(plan), data=_p(data), target_view=_p(target), rest_view=_p(rest) if R else None,
                           signal_elems=signal.numel(), B=B, V=V, R=R, dtype=0 if signal.dtype == torch.int16 else 1)
    _lib.check(L.nef_beat_batch(C.byref(A), _stream()), "nef_beat_batch")
    _done(ev)
    return data, target, rest


def _check_signal(signal, who):
    if not torch.is_tensor(signal) or signal.dtype not in (torch.int16, torch.float32):
        raise TypeError(f"signal must be an int16 or float32 tensor, got {getattr(signal, 'dtype', type(signal))}")
    if signal.dim() != 1 or signal.numel() < 1 or not signal.is_contiguous():
        raise ValueError(f"signal must be a non-empty contiguous 1-D tensor, got {tuple(signal.shape)}")
    if not signal.is_cuda:
        raise RuntimeError(f"ops.{who} runs on a HIP device only (no CPU path)")
    if signal.data_ptr() % 16 != 0:
        raise ValueError("signal is not 16-byte aligned")


def _device_table(t, name, cols, dtype, dev, rows=None):
    """An integer / fp64 table [rows >= 1, cols] (cols None: 1-D) as a contiguous tensor on `dev`; one on the host is copied."""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError(f"{name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    shape_ok = (t.dim() == 1) if cols is None else (t.dim() == 2 and t.shape[1] == cols)
    if not shape_ok or t.shape[0] < 1 or (rows is not None and t.shape[0] != rows) or not t.is_contiguous():
        want = f"[{rows if rows is not None else 'rows >= 1'}{'' if cols is None else ', ' + str(cols)}]"
        raise ValueError(f"{name} {tuple(t.shape)} is not a contiguous {want} table")
    if t.is_cuda and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, not on {dev}")
    return t if t.is_cuda else t.to(dev, non_blocking=True)


def beat_range(signal, plan, V, R):
    """(lo, hi) of every row of a beat plan, fp64 [B, 2], exactly as nef_beat_batch forms them for its normalisation (nef_beat_range,
    include/nefnet_hip.h): what de-normalises a row of ops.beat_batch, or a view predicted in its place.  `signal` and `plan` as for
    ops.beat_batch, a host plan checked against `signal` here in the same way; a row of a device plan that leaves the signal gives
    (NaN, NaN).  One launch on the current stream, capturable with a device plan."""
    V, R = _check_beat_plan(signal, plan, V, R, "beat_range")
    L = _lib.load()
    if not plan.is_cuda:
        plan = plan.to(signal.device, non_blocking=True)
    B = plan.shape[0]
    rng = torch.empty((B, 2), dtype=torch.float64, device=signal.device)
    ev = _hbm("beat_range", plan, rng)
    A = _lib.BeatRangeArgs(signal=_p(signal), plan=_p(plan), range=_p(rng), signal_elems=signal.numel(), B=B, V=V, R=R,
                           dtype=0 if signal.dtype == torch.int16 else 1)
    _lib.check(L.nef_beat_range(C.byref(A), _stream()), "nef_beat_range")
    _done(ev)
    return rng


STITCH_FILLS = ("nan", "bridge")      # nef_beat_stitch_args.fill 0 / 1
STITCH_MAX_BEATS = 65535              # the beats are a grid's y extent
STITCH_MAX_ANGLES = 65536


def _fill_code(fill):
    if fill in (0, 1) and not isinstance(fill, bool):
        return int(fill)
    if fill not in STITCH_FILLS:
        raise ValueError(f"fill must be one of {STITCH_FILLS} (or 0 / 1), got {fill!r}")
    return STITCH_FILLS.index(fill)


def beat_stitch(views, rng, table, out, fill):
    """De-normalise per-beat views and write them at the beats' P onsets of whole-recording signals (nef_beat_stitch, include/nefnet_hip.h).
    views: fp32 [Bt, A, 512] on the device, last dimension contiguous, any beat / angle strides (a slice of a larger tensor is taken as it
    is); rng: fp64 [Bt, 2] of ops.beat_range; table: int64 [Bt, 4] = [index in `out` of angle 0 at p_on, angle stride = the recording's
    length, n, 1 where the next row continues the recording]; out: a flat contiguous fp32 device buffer, written in place at the beats'
    positions only and returned.  fill: 'nan' or 'bridge' for the positions of a beat behind its 512-sample row.  A host table is checked
    against `out` here and copied; a row of a device table that would leave `out` writes nothing.  One launch, capturable."""
    code = _fill_code(fill)
    if not torch.is_tensor(views) or views.dtype != torch.float32 or views.dim() != 3 or views.shape[2] != BEAT_LEN:
        raise TypeError(f"views must be a float32 [Bt, A, {BEAT_LEN}] tensor, got {getattr(views, 'dtype', type(views))} "
                        f"{tuple(getattr(views, 'shape', ()))}")
    if not views.is_cuda:
        raise RuntimeError("ops.beat_stitch runs on a HIP device only (no CPU path)")
    Bt, A = views.shape[0], views.shape[1]
    if not 1 <= Bt <= STITCH_MAX_BEATS or not 1 <= A <= STITCH_MAX_ANGLES:
        raise ValueError(f"views {tuple(views.shape)}: 1 <= Bt <= {STITCH_MAX_BEATS} beats and 1 <= A <= {STITCH_MAX_ANGLES} angles a launch")
    as_ = views.stride(1) if A > 1 else BEAT_LEN        # the stride of a dimension of one entry means nothing
    bs = views.stride(0) if Bt > 1 else A * as_
    if views.stride(2) != 1 or as_ < BEAT_LEN or bs < A * as_:
        raise ValueError(f"views strides {views.stride()}: rows must be contiguous, angle rows {BEAT_LEN} apart or more and beats behind them")
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.dim() != 1 or out.numel() < 1 or not out.is_contiguous():
        raise TypeError("out must be a non-empty contiguous 1-D float32 tensor")
    if out.device != views.device:
        raise ValueError(f"out is on {out.device}, views on {views.device}")
    if out.numel() >= 1 << 40:
        raise ValueError(f"out holds {out.numel()} elements; a launch addresses fewer than 2^40")
    if torch.is_tensor(table) and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 4 and not table.is_cuda:
        base, stride, n = table[:, 0], table[:, 1], table[:, 2]
        bad = (base < 0) | (stride < 1) | (n < 1) | (n > stride) | (base + (A - 1) * stride + n > out.numel())
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            raise ValueError(f"table row {i} {table[i].tolist()} leaves the output of {out.numel()} elements at {A} angles")
    table = _device_table(table, "table", 4, torch.int64, views.device, rows=Bt)
    rng = _device_table(rng, "rng", 2, torch.float64, views.device, rows=Bt)
    L = _lib.load()
    ev = _hbm("beat_stitch", views, rng, table)
    S = _lib.BeatStitchArgs(views=_p(views), range=_p(rng), table=_p(table), out=_p(out), view_bs=bs, view_as=as_, out_elems=out.numel(),
                            Bt=Bt, A=A, fill=code, reserved0=0)
    _lib.check(L.nef_beat_stitch(C.byref(S), _stream()), "nef_beat_stitch")
    _done(ev)
    return out


def recording_stats(out, signal, beat_table, rec_table, score_leads, fill, out_offsets):
    """Per (recording, angle) the count and the six fp64 sums of the stitched signals against stored or derived leads: fp64 [N, A, 7] =
    [count, sum d^2, sum u, sum w, sum u^2, sum w^2, sum u w] (nef_recording_stats, include/nefnet_hip.h; recording.metrics turns them into
    RMSE and correlation).  out: the flat fp32 buffer ops.beat_stitch wrote; signal: the store's flat tensor; beat_table: the int64
    [Bt, 4] table of ops.beat_stitch over all recordings; rec_table: int64 [N, 4] = [first row, rows, offset in `signal`, length];
    score_leads: A leads in -1..11 (a list, or an int32 tensor; -1: the angle is not scored and gets zeros); out_offsets: int64 [N], where
    recording i's [A, len_i] signals start in `out`.  fill as for ops.beat_stitch: 'bridge' counts the positions behind a beat's 512-sample
    row too.  A row of a launch depends on that recording's own tables alone.  One launch, capturable with device tables."""
    code = _fill_code(fill)
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.dim() != 1 or out.numel() < 1 or not out.is_contiguous():
        raise TypeError("out must be a non-empty contiguous 1-D float32 tensor")
    if out.numel() >= 1 << 40:
        raise ValueError(f"out holds {out.numel()} elements; a launch addresses fewer than 2^40")
    if not torch.is_tensor(score_leads):
        score_leads = torch.tensor([int(v) for v in score_leads], dtype=torch.int32)
    if score_leads.dtype != torch.int32 or score_leads.dim() != 1 or not 1 <= score_leads.numel() <= STITCH_MAX_ANGLES:
        raise ValueError(f"score_leads must be 1 to {STITCH_MAX_ANGLES} int32 leads, got {score_leads.dtype} {tuple(score_leads.shape)}")
    if not score_leads.is_cuda and bool(((score_leads < -1) | (score_leads > 11)).any()):
        raise ValueError(f"score_leads {score_leads.tolist()}: each is a lead 0..11, or -1 for an angle that is not scored")
    _check_signal(signal, "recording_stats")
    dev = signal.device
    if out.device != dev:
        raise ValueError(f"out is on {out.device}, signal on {dev}")
    A = score_leads.numel()
    host = [t for t in (beat_table, rec_table, out_offsets) if torch.is_tensor(t) and not t.is_cuda]
    beat_table = _device_table(beat_table, "beat_table", 4, torch.int64, dev)
    rec_table = _device_table(rec_table, "rec_table", 4, torch.int64, dev)
    N, Bt = rec_table.shape[0], beat_table.shape[0]
    out_offsets = _device_table(out_offsets, "out_offsets", None, torch.int64, dev, rows=N)
    if len(host) == 3:          # all on the host: checked here as the kernel checks device tables
        bt, rt, oo = host
        first, rows, soff, ln = rt[:, 0], rt[:, 1], rt[:, 2], rt[:, 3]
        bad = (first < 0) | (rows < 0) | (first + rows > Bt) | (soff < 0) | (ln < 1) | (soff + 8 * ln > signal.numel()) | (oo < 0) | \
              (oo + A * ln > out.numel())
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            raise ValueError(f"rec_table row {i} {rt[i].tolist()} (output offset {int(oo[i])}) leaves the signal, the output or the beat table")
        for i in range(N):
            b = bt[int(first[i]):int(first[i] + rows[i])]
            p = b[:, 0] - oo[i]
            if bool(((p < 0) | (b[:, 1] != ln[i]) | (b[:, 2] < 1) | (p + b[:, 2] > ln[i])).any()):
                raise ValueError(f"a beat of recording {i} lies outside its {int(ln[i])} positions")
    if N * A > 0x7FFFFFFF:
        raise ValueError(f"{N} recordings x {A} angles: a launch takes fewer than 2^31 pairs")
    if score_leads.is_cuda and score_leads.device != dev:
        raise ValueError(f"score_leads is on {score_leads.device}, signal on {dev}")
    score_leads = score_leads.contiguous() if score_leads.is_cuda else score_leads.contiguous().to(dev, non_blocking=True)
    L = _lib.load()
    stats = torch.empty((N, A, 7), dtype=torch.float64, device=dev)
    ev = _hbm("recording_stats", out, signal, beat_table, rec_table, stats)
    S = _lib.RecordingStatsArgs(out=_p(out), signal=_p(signal), beat_table=_p(beat_table), rec_table=_p(rec_table),
                                out_offsets=_p(out_offsets), score_leads=_p(score_leads), stats=_p(stats), out_elems=out.numel(),
                                signal_elems=signal.numel(), Bt=Bt, N=N, A=A, fill=code, dtype=0 if signal.dtype == torch.int16 else 1,
                                reserved0=0)
    _lib.check(L.nef_recording_stats(C.byref(S), _stream()), "nef_recording_stats")
    _done(ev)
    return stats


MARK_TILE = 1024          # NEF_MARK_TILE (include/nefnet_hip.h): positions per workgroup of nef_mark_envelope
MARK_MAX_D, MARK_MAX_H, MARK_MAX_R, MARK_MAX_SEGMENTS = 4096, 256, 512, 4096
MARK_MAX_ROWS = 65535     # the rows are a grid's y extent
MARK_MAX_LEN = 0x7FFF0000
MARK_MAX_PEAKS = 1 << 20


def _mark_int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{name} = {v!r}: an integer in {lo}..{hi}")
    return v


def _mark_table(table, dev, max_len, env_elems, signal_elems=None, max_rows=None):
    """The (offset, len, env_offset) table of the two mark entries on `dev`, and the launch's max_len.  A host table is checked row by row
    against the buffers here, and gives max_len; a device table is taken as it is (the kernels answer a bad row themselves) and needs
    max_len from the caller."""
    if not torch.is_tensor(table) or table.dtype != torch.int64:
        raise TypeError(f"table must be an int64 tensor, got {getattr(table, 'dtype', type(table))}")
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_contiguous():
        raise ValueError(f"table {tuple(table.shape)} is not a contiguous [rows >= 1, 3] table of (offset, len, env_offset)")
    if max_rows is not None and table.shape[0] > max_rows:
        raise ValueError(f"table has {table.shape[0]} rows; a launch takes at most {max_rows}")
    if table.is_cuda:
        if table.device != dev:
            raise ValueError(f"table is on {table.device}, not on {dev}")
        if max_len is None:
            raise ValueError("a device table needs max_len: the launch is sized on the host")
        return table, _mark_int("max_len", max_len, 1, MARK_MAX_LEN)
    off, ln, eoff = table[:, 0], table[:, 1], table[:, 2]
    bad = (ln < 1) | (ln > MARK_MAX_LEN) | (eoff < 0) | (eoff + ln > env_elems)
    if signal_elems is not None:
        bad = bad | (off < 0) | (off + 8 * ln > signal_elems)
    if max_len is not None:
        bad = bad | (ln > _mark_int("max_len", max_len, 1, MARK_MAX_LEN))
    if bool(bad.any()):
        i = int(bad.nonzero()[0, 0])
        raise ValueError(f"table row {i} {table[i].tolist()} leaves the signal ({signal_elems} elements), the envelope ({env_elems}) or max_len {max_len}")
    return table.to(dev, non_blocking=True), int(ln.max()) if max_len is None else max_len


def _check_env(env, dev):
    if not torch.is_tensor(env) or env.dtype != torch.float64 or env.dim() != 1 or env.numel() < 1 or not env.is_contiguous():
        raise TypeError("env must be a non-empty contiguous 1-D float64 tensor")
    if not env.is_cuda:
        raise RuntimeError("the mark entries run on a HIP device only (no CPU path)")
    if dev is not None and env.device != dev:
        raise ValueError(f"env is on {env.device}, not on {dev}")


def mark_envelope(signal, table, env, D=2, H=20, lead_bits=255, max_len=None):
    """The detector's envelope of recordings of a resident store (nef_mark_envelope, include/nefnet_hip.h): for every row (offset, len,
    env_offset) of the int64 [N, 3] `table`, env[env_offset + t] = the sum over the window [t - H, t + H] (cut at the recording's ends) of
    the squared differences x[t + D] - x[t - D] (indices clamped) of the leads in `lead_bits`, in fp64 from the stored int16 / float32 values.
    `env` is a flat float64 device buffer, written in place at the rows' positions only and returned.  A host table is checked against
    `signal` and `env` here and copied; a device table needs `max_len`, and a row of it that would leave a buffer writes nothing.  One
    launch on the current stream, capturable with a device table."""
    _check_signal(signal, "mark_envelope")
    _check_env(env, signal.device)
    D, H = _mark_int("D", D, 0, MARK_MAX_D), _mark_int("H", H, 0, MARK_MAX_H)
    lead_bits = _mark_int("lead_bits", lead_bits, 1, 255)
    table, max_len = _mark_table(table, signal.device, max_len, env.numel(), signal.numel(), max_rows=MARK_MAX_ROWS)
    L = _lib.load()
    ev = _hbm("mark_envelope", signal, table, env)
    A = _lib.MarkEnvelopeArgs(signal=_p(signal), table=_p(table), env=_p(env), signal_elems=signal.numel(), env_elems=env.numel(),
                              max_len=max_len, N=table.shape[0], D=D, H=H, lead_bits=lead_bits,
                              dtype=0 if signal.dtype == torch.int16 else 1, reserved0=0)
    _lib.check(L.nef_mark_envelope(C.byref(A), _stream()), "nef_mark_envelope")
    _done(ev)
    return env


def mark_peaks(env, table, r=100, seg=1000, frac=0.125, max_peaks=256, max_len=None):
    """The peaks of every row's envelope (nef_mark_peaks, include/nefnet_hip.h): level = the lower median of the maxima of the len // seg
    segments; t is a peak iff env[t] > 0, env[t] >= level * frac, nothing in the r positions before it is as high and nothing in the r
    behind it higher.  `env` and `table` as for ops.mark_envelope (a row's signal offset is not read).  Returns fresh (peaks int32
    [N, max_peaks] ascending with -1 behind them, count int32 [N] -- the true number, also above max_peaks -- and level float64 [N]); a row
    with a non-finite envelope gets count -1, a NaN level and -1s.  One launch on the current stream, capturable with a device table."""
    _check_env(env, None)
    r, seg = _mark_int("r", r, 0, MARK_MAX_R), _mark_int("seg", seg, 1, MARK_MAX_LEN)
    max_peaks = _mark_int("max_peaks", max_peaks, 1, MARK_MAX_PEAKS)
    if isinstance(frac, bool) or not isinstance(frac, (int, float)) or not 0.0 <= float(frac) < float('inf'):
        raise ValueError(f"frac = {frac!r}: a finite number >= 0")
    table, max_len = _mark_table(table, env.device, max_len, env.numel())
    if max_len // seg > MARK_MAX_SEGMENTS:
        raise ValueError(f"max_len {max_len} with seg {seg}: more than {MARK_MAX_SEGMENTS} segments a recording")
    N = table.shape[0]
    peaks = torch.empty((N, max_peaks), dtype=torch.int32, device=env.device)
    count = torch.empty((N,), dtype=torch.int32, device=env.device)
    level = torch.empty((N,), dtype=torch.float64, device=env.device)
    L = _lib.load()
    ev = _hbm("mark_peaks", table, peaks, count, level)
    A = _lib.MarkPeaksArgs(env=_p(env), table=_p(table), peaks=_p(peaks), count=_p(count), level=_p(level), env_elems=env.numel(),
                           max_len=max_len, frac=float(frac), N=N, seg=seg, r=r, max_peaks=max_peaks)
    _lib.check(L.nef_mark_peaks(C.byref(A), _stream()), "nef_mark_peaks")
    _done(ev)
    return peaks, count, level


RESAMPLE_TILE = 1024      # NEF_RESAMPLE_TILE (include/nefnet_hip.h): outputs per workgroup of nef_resample
RESAMPLE_MAX_UP, RESAMPLE_MAX_K, RESAMPLE_MAX_RATIO = 1024, 512, 8
RESAMPLE_MAX_ROWS = 65535  # table rows, and signals a table row: a grid's z and y extents


def resample(src, table, dst, taps, first, up, down, max_out_len=None, max_rows=None):
    """Resample lead-major rows of `src` in time by up / down into `dst` (nef_resample, include/nefnet_hip.h).  Every row (in_offset, len,
    out_offset, rows) of the int64 [N, 4] `table` names `rows` signals [rows, len] of the flat int16 / float32 device buffer `src`; they
    come out as [rows, out_len] float32 at out_offset of the flat float32 device buffer `dst`, out_len = (len * up + down - 1) // down:
    y[m] = float32(sum_k taps[p, k] * x[clamp(i0 + first[p] + k, 0, len - 1)]), i0 = m * down // up, p = m * down % up, in fp64 and
    ascending k.  `taps` (float64 [up, K]) and `first` (int32 [up]) are resample.design's table, numpy or torch, host or device.  `dst` is
    written in place at the rows' positions only and returned.  A host table is checked against both buffers here and copied; a device
    table needs `max_out_len` and `max_rows` (the launch is sized on the host), and a row of it that would leave a buffer writes nothing.
    One launch on the current stream, capturable with device tables."""
    _check_signal(src, "resample")
    if not torch.is_tensor(dst) or dst.dtype != torch.float32 or dst.dim() != 1 or dst.numel() < 1 or not dst.is_contiguous():
        raise TypeError("dst must be a non-empty contiguous 1-D float32 tensor")
    if not dst.is_cuda or dst.device != src.device:
        raise ValueError(f"dst is on {dst.device}, src on {src.device}")
    up, down = _mark_int("up", up, 1, RESAMPLE_MAX_UP), _mark_int("down", down, 1, 1 << 30)
    if down > RESAMPLE_MAX_RATIO * up:
        raise ValueError(f"down = {down} is above {RESAMPLE_MAX_RATIO} x up = {up}")
    dev = src.device
    taps = torch.from_numpy(np.ascontiguousarray(taps)) if isinstance(taps, np.ndarray) else taps
    first = torch.from_numpy(np.ascontiguousarray(first)) if isinstance(first, np.ndarray) else first
    if not torch.is_tensor(taps) or taps.dtype != torch.float64 or taps.dim() != 2 or taps.shape[0] != up or \
            not 1 <= taps.shape[1] <= RESAMPLE_MAX_K:
        raise ValueError(f"taps must be float64 [up = {up}, K in 1..{RESAMPLE_MAX_K}], got "
                         f"{getattr(taps, 'dtype', type(taps))} {tuple(getattr(taps, 'shape', ()))}")
    if not torch.is_tensor(first) or first.dtype != torch.int32 or tuple(first.shape) != (up,):
        raise ValueError(f"first must be int32 [up = {up}], got {getattr(first, 'dtype', type(first))} {tuple(getattr(first, 'shape', ()))}")
    for name, t in (("taps", taps), ("first", first)):
        if t.is_cuda and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, src on {dev}")
    K = int(taps.shape[1])
    taps, first = taps.contiguous().to(dev, non_blocking=True), first.contiguous().to(dev, non_blocking=True)
    if not torch.is_tensor(table) or table.dtype != torch.int64:
        raise TypeError(f"table must be an int64 tensor, got {getattr(table, 'dtype', type(table))}")
    if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1 or not table.is_contiguous():
        raise ValueError(f"table {tuple(table.shape)} is not a contiguous [rows >= 1, 4] table of (in_offset, len, out_offset, rows)")
    if table.shape[0] > RESAMPLE_MAX_ROWS:
        raise ValueError(f"table has {table.shape[0]} rows; a launch takes at most {RESAMPLE_MAX_ROWS}")
    if table.is_cuda:
        if table.device != dev:
            raise ValueError(f"table is on {table.device}, not on {dev}")
        if max_out_len is None or max_rows is None:
            raise ValueError("a device table needs max_out_len and max_rows: the launch is sized on the host")
        max_out_len, max_rows = _mark_int("max_out_len", max_out_len, 1, MARK_MAX_LEN), _mark_int("max_rows", max_rows, 1, RESAMPLE_MAX_ROWS)
    else:
        off, ln, ooff, rows = table[:, 0], table[:, 1], table[:, 2], table[:, 3]
        bad = (ln < 1) | (ln > MARK_MAX_LEN) | (rows < 1) | (rows > RESAMPLE_MAX_ROWS) | (off < 0) | (ooff < 0)
        oln = (ln.clamp(1, MARK_MAX_LEN) * up + down - 1) // down
        r = rows.clamp(1, RESAMPLE_MAX_ROWS)
        bad = bad | (oln > MARK_MAX_LEN) | (off + r * ln.clamp(1, MARK_MAX_LEN) > src.numel()) | (ooff + r * oln > dst.numel())
        if max_out_len is not None:
            bad = bad | (oln > _mark_int("max_out_len", max_out_len, 1, MARK_MAX_LEN))
        if max_rows is not None:
            bad = bad | (rows > _mark_int("max_rows", max_rows, 1, RESAMPLE_MAX_ROWS))
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            raise ValueError(f"table row {i} {table[i].tolist()} leaves src ({src.numel()} elements), dst ({dst.numel()}), "
                             f"max_out_len {max_out_len} or max_rows {max_rows}")
        max_out_len = int(oln.max()) if max_out_len is None else max_out_len
        max_rows = int(rows.max()) if max_rows is None else max_rows
        table = table.to(dev, non_blocking=True)
    L = _lib.load()
    ev = _hbm("resample", src, table, dst)
    A = _lib.ResampleArgs(src=_p(src), table=_p(table), dst=_p(dst), taps=_p(taps), first=_p(first), src_elems=src.numel(),
                          dst_elems=dst.numel(), max_out_len=max_out_len, N=table.shape[0], max_rows=max_rows, up=up, down=down, K=K,
                          dtype=0 if src.dtype == torch.int16 else 1)
    _lib.check(L.nef_resample(C.byref(A), _stream()), "nef_resample")
    _done(ev)
    return dst


MEDIAN_TILE = 1024        # NEF_MEDIAN_TILE (include/nefnet_hip.h): outputs per workgroup of nef_sliding_median
MEDIAN_MAX_H = 512        # NEF_MEDIAN_MAX_H
MEDIAN_MAX_ROWS = 65535   # table rows, and signals a table row: a grid's z and y extents


def _overlap(a, b):
    """Two tensors whose bytes share an address."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def sliding_median(src, table, dst, h, minuend=None, max_len=None, max_rows=None):
    """The sliding median of lead-major rows of `src` into `dst` (nef_sliding_median, include/nefnet_hip.h).  Every row (offset, len,
    rows) of the int64 [N, 3] `table` names `rows` signals [rows, len] at the same offset of the flat int16 / float32 device buffer `src`,
    of the flat float32 device buffer `dst` and of `minuend`: dst[t] = m(t), the (h + 1)-th smallest of the 2 h + 1 values
    x[clamp(t + j, 0, len - 1)], j = -h .. h, as float32 -- NaN when the window holds one -- or, with `minuend` (flat int16 / float32, same
    layout), float32(float64(minuend[t]) - float64(m(t))).  `dst` may be a float32 `minuend` itself; it may not overlap `src`.  `dst` is
    written in place at the rows' positions only and returned.  A host table is checked against every buffer here and copied; a device
    table needs `max_len` and `max_rows` (the launch is sized on the host), and a row of it that would leave a buffer writes nothing.
    One launch on the current stream, capturable with a device table."""
    _check_signal(src, "sliding_median")
    if not torch.is_tensor(dst) or dst.dtype != torch.float32 or dst.dim() != 1 or dst.numel() < 1 or not dst.is_contiguous():
        raise TypeError("dst must be a non-empty contiguous 1-D float32 tensor")
    if not dst.is_cuda or dst.device != src.device:
        raise ValueError(f"dst is on {dst.device}, src on {src.device}")
    if _overlap(dst, src):
        raise ValueError("dst overlaps src: a window reads positions that other threads write")
    h = _mark_int("h", h, 0, MEDIAN_MAX_H)
    dev = src.device
    elems = min(src.numel(), dst.numel())
    if minuend is not None:
        if not torch.is_tensor(minuend) or minuend.dtype not in (torch.int16, torch.float32):
            raise TypeError(f"minuend must be an int16 or float32 tensor, got {getattr(minuend, 'dtype', type(minuend))}")
        if minuend.dim() != 1 or minuend.numel() < 1 or not minuend.is_contiguous():
            raise ValueError(f"minuend must be a non-empty contiguous 1-D tensor, got {tuple(minuend.shape)}")
        if not minuend.is_cuda or minuend.device != dev:
            raise ValueError(f"minuend is on {minuend.device}, src on {dev}")
        if minuend.data_ptr() != dst.data_ptr() and _overlap(minuend, dst):
            raise ValueError("dst overlaps minuend without being it: an element would be written by another thread than reads it")
        elems = min(elems, minuend.numel())
    if not torch.is_tensor(table) or table.dtype != torch.int64:
        raise TypeError(f"table must be an int64 tensor, got {getattr(table, 'dtype', type(table))}")
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_contiguous():
        raise ValueError(f"table {tuple(table.shape)} is not a contiguous [rows >= 1, 3] table of (offset, len, rows)")
    if table.shape[0] > MEDIAN_MAX_ROWS:
        raise ValueError(f"table has {table.shape[0]} rows; a launch takes at most {MEDIAN_MAX_ROWS}")
    if table.is_cuda:
        if table.device != dev:
            raise ValueError(f"table is on {table.device}, not on {dev}")
        if max_len is None or max_rows is None:
            raise ValueError("a device table needs max_len and max_rows: the launch is sized on the host")
        max_len, max_rows = _mark_int("max_len", max_len, 1, MARK_MAX_LEN), _mark_int("max_rows", max_rows, 1, MEDIAN_MAX_ROWS)
    else:
        off, ln, rows = table[:, 0], table[:, 1], table[:, 2]
        bad = (ln < 1) | (ln > MARK_MAX_LEN) | (rows < 1) | (rows > MEDIAN_MAX_ROWS) | (off < 0)
        bad = bad | (off + rows.clamp(1, MEDIAN_MAX_ROWS) * ln.clamp(1, MARK_MAX_LEN) > elems)
        if max_len is not None:
            bad = bad | (ln > _mark_int("max_len", max_len, 1, MARK_MAX_LEN))
        if max_rows is not None:
            bad = bad | (rows > _mark_int("max_rows", max_rows, 1, MEDIAN_MAX_ROWS))
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            raise ValueError(f"table row {i} {table[i].tolist()} leaves src ({src.numel()} elements), dst ({dst.numel()}), minuend "
                             f"({None if minuend is None else minuend.numel()}), max_len {max_len} or max_rows {max_rows}")
        max_len = int(ln.max()) if max_len is None else max_len
        max_rows = int(rows.max()) if max_rows is None else max_rows
        table = table.to(dev, non_blocking=True)
    L = _lib.load()
    ev = _hbm("sliding_median", src, table, dst, minuend)
    A = _lib.SlidingMedianArgs(src=_p(src), table=_p(table), dst=_p(dst), minuend=_p(minuend), src_elems=src.numel(), dst_elems=dst.numel(),
                               minuend_elems=0 if minuend is None else minuend.numel(), max_len=max_len, N=table.shape[0],
                               max_rows=max_rows, h=h, dtype=0 if src.dtype == torch.int16 else 1,
                               minuend_dtype=1 if minuend is None or minuend.dtype == torch.float32 else 0, reserved0=0)
    _lib.check(L.nef_sliding_median(C.byref(A), _stream()), "nef_sliding_median")
    _done(ev)
    return dst


LOSS_SEG_TILE = 1024      # NEF_LOSS_SEG_TILE (include/nefnet_hip.h): positions per block of the two segment-weight kernels
LOSS_SEG_MAX_ROWS = 65535  # the rows are a grid's y extent


def _seg_weights(weights):
    """SOLVER.seg_weights as the seven floats of nef_loss_seg_args.w: [P, PR, QRS, ST, T, TP, pad], finite and >= 0."""
    w = tuple(float(x) for x in weights)
    if len(w) != N_SEG:
        raise ValueError(f"segment weights {w}: {N_SEG} numbers are needed [P, PR, QRS, ST, T, TP, pad]")
    if not all(0.0 <= x < float("inf") for x in w):
        raise ValueError(f"Invalid segment weights: {w} (finite numbers >= 0)")
    return (C.c_float * N_SEG)(*w)


def _seg_rows(t, rois, what):
    """(B, L) of a [B, 1, L] / [Q, B, 1, L] / [B, L] tensor whose rows `rois` int64 [B, 7, 2] describes."""
    _chk(t)
    if t.dim() < 2:
        raise ValueError(f"{what} {tuple(t.shape)} must hold [B, 1, L] rows")
    Ln = t.shape[-1]
    B = t.numel() // Ln
    if _chk(rois, torch.int64).dim() != 3 or tuple(rois.shape) != (B, N_SEG, 2):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, {N_SEG}, 2]")
    if Ln % 4:
        raise ValueError(f"{what} {tuple(t.shape)}: the row length must be a multiple of 4")
    if B > LOSS_SEG_MAX_ROWS:
        raise ValueError(f"{what} {tuple(t.shape)}: {B} rows is more than the {LOSS_SEG_MAX_ROWS} the segment kernels take")
    return B, Ln


def loss_seg_fwd(pred, target, losses, weights, f2, reg_l2, rois, noise=None):
    """The wave-segment weighted reconstruction term behind loss_fwd (nef_loss_seg_fwd, include/nefnet_hip.h): losses[3] =
    f2 * (1/n) * sum w[seg(i, t)] * e(i, t) over all n = B * L elements, e as loss_fwd forms it at pred (+ noise), and losses[0] =
    (losses[1] + losses[2]) + losses[3].  `losses`: the row loss_fwd(out=) has written (4 elements, or 5 with the SSIM term, whose
    launches come behind this one).  `weights`: [P, PR, QRS, ST, T, TP, pad].  Two launches, capturable."""
    L = _lib.load()
    B, Ln = _seg_rows(pred, rois, "prediction")
    if _chk(target).numel() != pred.numel():
        raise ValueError(f"prediction {tuple(pred.shape)} and target {tuple(target.shape)} must hold the same rows")
    if noise is not None and _chk(noise).numel() != pred.numel():
        raise ValueError(f"noise {tuple(noise.shape)} does not have the prediction's {tuple(pred.shape)} elements")
    _chk(losses)
    assert losses.numel() in (4, 5), losses.shape
    n = L.nef_loss_seg_ws_bytes(B, Ln)
    ws = workspace(n, pred.device)
    ev = _hbm("loss_seg_fwd", pred, target, noise)
    A = _lib.LossSegArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=_p(losses), g_pred=None, ws=_p(ws),
                         ws_bytes=n, B=B, L=Ln, reg_l2=int(bool(reg_l2)), f2=float(f2), w=_seg_weights(weights))
    _lib.check(L.nef_loss_seg_fwd(C.byref(A), _stream()), "nef_loss_seg_fwd")
    _done(ev)
    return losses


def loss_seg_bwd(g_pred, weights, rois):
    """g_pred[i, t] = w[seg(i, t)] * g_pred[i, t] in place behind loss_bwd and in front of loss_ssim_bwd (nef_loss_seg_bwd): `g_pred` is
    loss_bwd's first gradient, the first third of its [3B, 1, L] buffer.  One fp32 multiply per element; one launch, capturable, no
    state."""
    L = _lib.load()
    B, Ln = _seg_rows(g_pred, rois, "g_pred")
    ev = _hbm("loss_seg_bwd", g_pred, g_pred)
    A = _lib.LossSegArgs(pred=None, target=None, noise=None, rois=_p(rois), losses=None, g_pred=_p(g_pred), ws=None, ws_bytes=0,
                         B=B, L=Ln, reg_l2=0, f2=0.0, w=_seg_weights(weights))
    _lib.check(L.nef_loss_seg_bwd(C.byref(A), _stream()), "nef_loss_seg_bwd")
    _done(ev)
    return g_pred


LOSS_SLOPE_TILE = 1024     # NEF_LOSS_SLOPE_TILE (include/nefnet_hip.h): difference starts / positions per block of the slope kernels
LOSS_SLOPE_MAX_ROWS = 65535  # the rows are a grid's y extent


def loss_slope_fwd(pred, target, losses, factor, l2, rois=None, noise=None):
    """The slope term of the training loss behind loss_fwd, loss_seg_fwd and loss_ssim_fwd (nef_loss_slope_fwd, include/nefnet_hip.h):
    losses[-1] = factor * mean over the rows with a difference of the row's mean |d| (`l2` False) or d^2, d(i, t) = (x[t + 1] - x[t]) -
    (y[t + 1] - y[t]) at x = pred (+ noise), y = target, t in [0, rois[i, -1, 0] - 1) (whole rows with rois None), and losses[0] +=
    losses[-1].  `losses`: the row whose front loss_fwd(out=) has written -- 5 elements (the term is losses[4]), or 6 with the SSIM term in
    losses[4] (the term is losses[5]).  Two launches, capturable."""
    B, Ln = _row_term_args("slope", pred, target, factor, rois, noise, LOSS_SLOPE_MAX_ROWS)
    _chk(losses)
    if losses.numel() not in (5, 6):
        raise ValueError(f"losses {tuple(losses.shape)}: the slope term takes a 5-element row, or a 6-element one behind the SSIM term")
    n = _lib.load().nef_loss_slope_ws_bytes(B, Ln)
    ws = workspace(n, pred.device)
    A = _lib.LossSlopeArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=_p(losses), ws=_p(ws), ws_bytes=n,
                           gscale=None, g_pred=None, B=B, L=Ln, factor=float(factor), l2=int(bool(l2)), slot=losses.numel() - 1)
    _row_term_call("loss_slope_fwd", A, pred, target, noise)
    return losses


def loss_slope_bwd(pred, target, g_pred, factor, l2, rois=None, noise=None, gscale=None):
    """g_pred += gscale * d(slope term) / d pred behind loss_bwd, loss_seg_bwd and loss_ssim_bwd (nef_loss_slope_bwd): `g_pred` is
    loss_bwd's first gradient, the first third of its [3B, 1, L] buffer.  Positions at or behind a row's end and rows without a difference
    keep their bits.  `gscale`: None (1) or loss_bwd's device word.  One launch, capturable, no state: the row count is re-derived from
    `rois` on the device."""
    B, Ln = _row_term_args("slope", pred, target, factor, rois, noise, LOSS_SLOPE_MAX_ROWS, g_pred=g_pred, gscale=gscale)
    A = _lib.LossSlopeArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=None, ws=None, ws_bytes=0,
                           gscale=_p(gscale), g_pred=_p(g_pred), B=B, L=Ln, factor=float(factor), l2=int(bool(l2)), slot=4)
    _row_term_call("loss_slope_bwd", A, pred, target, noise, g_pred, g_pred)
    return g_pred


LOSS_CORR_TILE = 1024      # NEF_LOSS_CORR_TILE (include/nefnet_hip.h): positions per block of the correlation term's kernels
LOSS_CORR_MAX_ROWS = 65535  # the rows are a grid's y extent


def loss_corr_fwd(pred, target, losses, factor, eps, rois=None, noise=None):
    """The correlation term of the training loss behind loss_fwd, loss_seg_fwd, loss_ssim_fwd and loss_slope_fwd (nef_loss_corr_fwd,
    include/nefnet_hip.h): losses[-1] = factor * mean over the rows with at least two samples of 1 - r_i, r_i the Pearson correlation
    coefficient (with `eps` in numerator and both variances) of x = pred (+ noise) and y = target over [0, rois[i, -1, 0]) (whole rows with
    rois None), and losses[0] += losses[-1].  `losses`: the row whose front loss_fwd(out=) has written -- 5 elements (the term is
    losses[4]), 6 or 7 with the SSIM and / or slope terms in front of it.  Two launches, capturable."""
    B, Ln = _row_term_args("correlation", pred, target, factor, rois, noise, LOSS_CORR_MAX_ROWS, eps)
    _chk(losses)
    if losses.numel() not in (5, 6, 7):
        raise ValueError(f"losses {tuple(losses.shape)}: the correlation term takes a 5-element row, or a 6- / 7-element one behind the "
                         "SSIM and slope terms")
    n = _lib.load().nef_loss_corr_ws_bytes(B, Ln)
    ws = workspace(n, pred.device)
    A = _lib.LossCorrArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=_p(losses), ws=_p(ws), ws_bytes=n,
                          gscale=None, g_pred=None, eps=float(eps), B=B, L=Ln, factor=float(factor), slot=losses.numel() - 1)
    _row_term_call("loss_corr_fwd", A, pred, target, noise)
    return losses


def loss_corr_bwd(pred, target, g_pred, factor, eps, rois=None, noise=None, gscale=None):
    """g_pred += gscale * d(correlation term) / d pred behind loss_bwd, loss_seg_bwd, loss_ssim_bwd and loss_slope_bwd
    (nef_loss_corr_bwd): `g_pred` is loss_bwd's first gradient, the first third of its [3B, 1, L] buffer.  Positions at or behind a row's
    end and rows with fewer than two samples keep their bits.  `gscale`: None (1) or loss_bwd's device word.  Three launches (the row
    moments are reduced again, then applied), capturable, no state from the forward."""
    B, Ln = _row_term_args("correlation", pred, target, factor, rois, noise, LOSS_CORR_MAX_ROWS, eps, g_pred=g_pred, gscale=gscale)
    n = _lib.load().nef_loss_corr_ws_bytes(B, Ln)
    ws = workspace(n, pred.device)
    A = _lib.LossCorrArgs(pred=_p(pred), target=_p(target), noise=_p(noise), rois=_p(rois), losses=None, ws=_p(ws), ws_bytes=n,
                          gscale=_p(gscale), g_pred=_p(g_pred), eps=float(eps), B=B, L=Ln, factor=float(factor), slot=4)
    _row_term_call("loss_corr_bwd", A, pred, target, noise, pred, target, noise, g_pred, g_pred)
    return g_pred


def flatten_into(tensors, out, accumulate=False, accumulate_dev=None):
    """out[:] = concatenation of `tensors` (contiguous fp32, flattened), ONE launch per 64 tensors (nef_flatten; was torch.cat).
    `accumulate`: out[:] += the concatenation instead (gradient accumulation: one fp32 add per element, no atomics).  `accumulate_dev`: a
    one-element int32 device tensor that replaces `accumulate` when the launch runs (non-zero: add) -- a captured launch then serves the
    first and the later micro-batches of a window.  Either one sends the call to nef_flatten_acc (tag "flatten_acc"); the default call
    is nef_flatten as before."""
    n = len(tensors)
    if n == 0:
        return out
    tensors = [t.detach() if t.is_contiguous() else t.detach().contiguous() for t in tensors]
    if not out.is_cuda or any((not t.is_cuda) or t.dtype != torch.float32 for t in tensors) or out.dtype != torch.float32:
        if accumulate_dev is not None:
            accumulate = bool(int(accumulate_dev.reshape(-1)[0]))
        if accumulate:
            return out.add_(torch.cat([t.reshape(-1) for t in tensors]))
        return torch.cat([t.reshape(-1) for t in tensors], out=out)          # (CPU plumbing tests; never on the device path)
    assert out.is_contiguous() and out.numel() == sum(t.numel() for t in tensors), (out.numel(), sum(t.numel() for t in tensors))
    srcs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    sizes = (C.c_int64 * n)(*[t.numel() for t in tensors])
    if not accumulate and accumulate_dev is None:
        _lib.check(_lib.load().nef_flatten(srcs, sizes, n, _p(out), _stream()), "nef_flatten")
        return out
    if accumulate_dev is not None:
        _chk(accumulate_dev, torch.int32)
        assert accumulate_dev.numel() == 1
    ev = _hbm("flatten_acc", out, *tensors)
    _lib.check(_lib.load().nef_flatten_acc(srcs, sizes, n, _p(out), int(bool(accumulate)), _p(accumulate_dev), _stream()),
               "nef_flatten_acc")
    _done(ev)
    return out


def copy_many(srcs, dsts, accumulate=False):
    """dsts[k][:] = srcs[k] -- or, `accumulate`, dsts[k][:] += srcs[k] -- for every pair of contiguous fp32 device tensors of equal
    element counts, ONE launch per 64 pairs (nef_copy_many; the multi-view train step's glue: no torch kernel in the replayed step).
    The tensors may be slices (4-byte aligned); no destination may overlap another destination or a source.  One writer per element,
    no atomics: the same bits eagerly and under replay."""
    n = len(srcs)
    if len(dsts) != n:
        raise ValueError(f"copy_many: {n} sources for {len(dsts)} destinations")
    if n == 0:
        return
    for s, d in zip(srcs, dsts):
        if _chk(s).numel() != _chk(d).numel():
            raise ValueError(f"copy_many: source {tuple(s.shape)} and destination {tuple(d.shape)} differ in size")
    sp = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
    sizes = (C.c_int64 * n)(*[s.numel() for s in srcs])
    ev = _hbm("copy_many", *srcs, *dsts, *(dsts if accumulate else ()))
    _lib.check(_lib.load().nef_copy_many(sp, dp, sizes, n, int(bool(accumulate)), _stream()), "nef_copy_many")
    _done(ev)


def stacked3(parts):
    """The three [B, 1, L] tensors as one [3B, 1, L] tensor WITHOUT a copy when they are consecutive views of one buffer (what
    loss_bwd returns), else None."""
    a, b, c = parts
    if any(t is None or not t.is_contiguous() for t in parts) or not (a.shape == b.shape == c.shape):
        return None
    n = a.numel() * 4
    if b.data_ptr() != a.data_ptr() + n or c.data_ptr() != b.data_ptr() + n or a._base is None or a._base is not b._base or a._base is not c._base:
        return None
    base = a._base
    if base.is_contiguous() and base.data_ptr() == a.data_ptr() and base.numel() == 3 * a.numel():
        return base.view((3 * a.shape[0],) + tuple(a.shape[1:]))
    return None


def regroup_halves(w, inverse=False):
    """w [Co, 2 Cih, K] -> grouped [2 Co, Cih, K] (group = input-channel half); inverse: the other way.  One launch (nef_regroup_halves)."""
    _chk(w)
    if inverse:
        co2, cih, k = w.shape
        out = torch.empty(co2 // 2, 2 * cih, k, device=w.device, dtype=torch.float32)
        co = co2 // 2
    else:
        co, ci, k = w.shape
        cih = ci // 2
        out = torch.empty(2 * co, cih, k, device=w.device, dtype=torch.float32)
    _lib.check(_lib.load().nef_regroup_halves(_p(w), _p(out), co, cih, k, int(bool(inverse)), _stream()), "nef_regroup_halves")
    return out


def view_metrics(pred, gt, rois=None):
    """Per-row PSNR and SSIM tables (fp64 [B, Q]) of pred vs gt [B, Q, L] on [0, rois[i, -1, 0])."""
    L = _lib.load()
    _chk(pred), _chk(gt)
    if rois is not None:
        _chk(rois, torch.int64)
    B, Q, Ln = pred.shape
    psnr = torch.empty(B, Q, device=pred.device, dtype=torch.float64)
    ssim = torch.empty(B, Q, device=pred.device, dtype=torch.float64)
    _lib.check(L.nef_view_metrics(_p(pred), _p(gt), _p(rois), _p(psnr), _p(ssim), B, Q, Ln, _stream()), "nef_view_metrics")
    return psnr, ssim


def view_seg_metrics(pred, gt, rois):
    """Per-row, per-wave-segment squared error of pred vs gt [B, Q, L] (nef_view_seg_metrics): (se fp64 [B, Q, 7], cnt int32 [B, Q, 7]) --
    the sum of squared differences over the positions of segment k of sample b (P, PR, QRS, ST, T, TP, pad; the definition of
    nef_loss_seg_args) and their number.  rois: int64 [B, 7, 2]."""
    L = _lib.load()
    _chk(pred), _chk(gt)
    if pred.dim() != 3 or gt.shape != pred.shape:
        raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} must both be [B, Q, L]")
    B, Q, Ln = pred.shape
    if _chk(rois, torch.int64).dim() != 3 or tuple(rois.shape) != (B, N_SEG, 2):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, {N_SEG}, 2]")
    if Ln % 4:
        raise ValueError(f"prediction {tuple(pred.shape)}: the row length must be a multiple of 4")
    se = torch.empty(B, Q, N_SEG, device=pred.device, dtype=torch.float64)
    cnt = torch.empty(B, Q, N_SEG, device=pred.device, dtype=torch.int32)
    _lib.check(L.nef_view_seg_metrics(_p(pred), _p(gt), _p(rois), _p(se), _p(cnt), B, Q, Ln, _stream()), "nef_view_seg_metrics")
    return se, cnt


def view_slope_metrics(pred, gt, rois=None):
    """Per-row squared slope error of pred vs gt [B, Q, L] (nef_view_slope_metrics): (se fp64 [B, Q], cnt int32 [B, Q]) -- the sum of
    ((x[t + 1] - x[t]) - (y[t + 1] - y[t]))^2 over t in [0, rois[b, -1, 0] - 1) (whole rows with rois None) and the number of those
    differences.  rois: None or int64 [B, 7, 2].  Any L >= 1."""
    L = _lib.load()
    _chk(pred), _chk(gt)
    if pred.dim() != 3 or gt.shape != pred.shape or pred.numel() == 0:
        raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} must both be [B, Q, L]")
    B, Q, Ln = pred.shape
    if rois is not None and (_chk(rois, torch.int64).dim() != 3 or tuple(rois.shape) != (B, N_SEG, 2)):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, {N_SEG}, 2]")
    se = torch.empty(B, Q, device=pred.device, dtype=torch.float64)
    cnt = torch.empty(B, Q, device=pred.device, dtype=torch.int32)
    _lib.check(L.nef_view_slope_metrics(_p(pred), _p(gt), _p(rois), _p(se), _p(cnt), B, Q, Ln, _stream()), "nef_view_slope_metrics")
    return se, cnt


def view_corr_metrics(pred, gt, rois=None):
    """Per-row moments of pred vs gt [B, Q, L] for the correlation coefficient (nef_view_corr_metrics): (mom fp64 [B, Q, 3], cnt int32
    [B, Q]) -- (vx, vy, c), the variances and the covariance over t in [0, rois[b, -1, 0]) (whole rows with rois None), and the number of
    those samples.  r = (c + eps) / sqrt((vx + eps) (vy + eps)) is formed by the caller for the rows with cnt >= 2.  rois: None or int64
    [B, 7, 2].  Any L >= 1."""
    L = _lib.load()
    _chk(pred), _chk(gt)
    if pred.dim() != 3 or gt.shape != pred.shape or pred.numel() == 0:
        raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} must both be [B, Q, L]")
    B, Q, Ln = pred.shape
    if rois is not None and (_chk(rois, torch.int64).dim() != 3 or tuple(rois.shape) != (B, N_SEG, 2)):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, {N_SEG}, 2]")
    mom = torch.empty(B, Q, 3, device=pred.device, dtype=torch.float64)
    cnt = torch.empty(B, Q, device=pred.device, dtype=torch.int32)
    _lib.check(L.nef_view_corr_metrics(_p(pred), _p(gt), _p(rois), _p(mom), _p(cnt), B, Q, Ln, _stream()), "nef_view_corr_metrics")
    return mom, cnt


LOCATE_MODES = {"mse": 0, "corr": 1}     # nef_locate_score_args.mode


def _rows3(t, dtype, what):
    """A [B, N, L] device tensor whose rows are dense (a slice of a larger tensor is fine): (batch stride, row stride) in elements."""
    if not (t.is_cuda and t.dtype == dtype and t.dim() == 3 and t.numel() > 0 and (t.shape[2] == 1 or t.stride(2) == 1)):
        raise ValueError(f"{what} must be a non-empty {dtype} device tensor [B, N, L] with dense rows, got {tuple(t.shape)} {t.dtype} "
                         f"strides {t.stride()}")
    return t.stride(0), t.stride(1)


def locate_score(pred, obs, rois=None, mode="corr", eps=1e-8, group=0, out=None, col=0):
    """Score every candidate view against the observed rows (nef_locate_score; lower is better): pred fp32 [B, A, L] and obs fp32
    [B, R, L] (rows dense, batch and row strides free: chunks of larger tensors are taken as they are), rois None (whole rows) or int64
    [B, 7, 2].  mode 'mse': the mean squared difference over t in [0, n_b); 'corr': 1 - r with r of view_corr_metrics' moments and `eps`;
    +inf for a row that does not count (n_b < 1 / n_b < 2) and for a NaN.  group 0: every candidate against every observed row ->
    [B, R, A]; group G > 0: A == R * G and candidate a is scored against row a // G -> [B, R, G].  `out`: an fp64 [B, R, N] tensor (or a
    slice of one) whose columns [col, col + A or G) are written; None: a new tensor of exactly that width.  Returns `out`."""
    L = _lib.load()
    if mode not in LOCATE_MODES:
        raise ValueError(f"score must be one of {sorted(LOCATE_MODES)}, got {mode!r}")
    p_bs, p_as = _rows3(pred, torch.float32, "pred")
    o_bs, o_rs = _rows3(obs, torch.float32, "obs")
    B, A, Ln = pred.shape
    R = obs.shape[1]
    if obs.shape[0] != B or obs.shape[2] != Ln:
        raise ValueError(f"obs {tuple(obs.shape)} does not match pred {tuple(pred.shape)}: [B, R, L] with the same B and L")
    if rois is not None and (_chk(rois, torch.int64).dim() != 3 or tuple(rois.shape) != (B, N_SEG, 2)):
        raise ValueError(f"rois {tuple(rois.shape)} is not [{B}, {N_SEG}, 2]")
    group = int(group)
    if group < 0 or (group and R * group != A):
        raise ValueError(f"group {group}: pred has {A} candidates per sample, not {R} x {group}")
    width = group if group else A
    if out is None:
        out, col = torch.empty(B, R, width, device=pred.device, dtype=torch.float64), 0
    s_bs, s_rs = _rows3(out, torch.float64, "out")
    if out.shape[0] != B or out.shape[1] != R or col < 0 or col + width > out.shape[2]:
        raise ValueError(f"out {tuple(out.shape)} does not hold columns [{col}, {col + width}) of [{B}, {R}, .]")
    a = _lib.LocateScoreArgs(pred=_p(pred), obs=_p(obs), rois=_p(rois), scores=_p(out), pred_bs=p_bs, pred_as=p_as, obs_bs=o_bs, obs_rs=o_rs,
                             sc_bs=s_bs, sc_rs=s_rs, col_off=int(col), eps=float(eps), B=B, A=A, R=R, L=Ln, mode=LOCATE_MODES[mode],
                             group=group)
    _lib.check(L.nef_locate_score(C.byref(a), _stream()), "nef_locate_score")
    return out


def locate_best(scores, cands, best=None, index_base=0, keep_index=False):
    """The deterministic arg-best of scores fp64 [B, R, A] (rows dense; a column slice is fine) over the matching candidates
    (nef_locate_best): cands fp32 [A, 2], shared, or [B, R * A, 2], the pair's own.  A strictly lower score replaces the running best,
    ties go to the earliest candidate, NaN counts as +inf.  `best` None: returns a new (score fp64 [B, R], theta fp32 [B, R, 2], index
    int64 [B, R]) -- index -1, theta NaN, score +inf where no score is finite; otherwise the three are merged into in place and
    returned.  A winner's index is index_base + its column; keep_index (levels >= 1): the index is left alone and a pair at -1 stays."""
    L = _lib.load()
    s_bs, s_rs = _rows3(scores, torch.float64, "scores")
    B, R, A = scores.shape
    _chk(cands)
    per_pair = cands.dim() == 3
    if tuple(cands.shape) != ((B, R * A, 2) if per_pair else (A, 2)):
        raise ValueError(f"cands {tuple(cands.shape)} is neither [{A}, 2] nor [{B}, {R * A}, 2]")
    init = best is None
    if init:
        if keep_index:
            raise ValueError("keep_index needs a running best")
        best = (torch.empty(B, R, device=scores.device, dtype=torch.float64), torch.empty(B, R, 2, device=scores.device, dtype=torch.float32),
                torch.empty(B, R, device=scores.device, dtype=torch.int64))
    bs, bt, bi = best
    _chk(bs, torch.float64), _chk(bt), _chk(bi, torch.int64)
    if tuple(bs.shape) != (B, R) or tuple(bt.shape) != (B, R, 2) or tuple(bi.shape) != (B, R):
        raise ValueError(f"best {tuple(bs.shape)}, {tuple(bt.shape)}, {tuple(bi.shape)} is not [{B}, {R}], [{B}, {R}, 2], [{B}, {R}]")
    a = _lib.LocateBestArgs(scores=_p(scores), cands=_p(cands), best_score=_p(bs), best_theta=_p(bt), best_index=_p(bi), sc_bs=s_bs,
                            sc_rs=s_rs, index_base=int(index_base), B=B, R=R, A=A, per_pair=int(per_pair), init=int(init),
                            keep_index=int(bool(keep_index)))
    _lib.check(L.nef_locate_best(C.byref(a), _stream()), "nef_locate_best")
    return bs, bt, bi


def locate_cands(best_theta, best_index, s1, s2, radius, placeholder):
    """The next level's candidates around the running best (nef_locate_cands): fp32 [B, R * (2 radius + 1)^2, 2], candidate
    r * G + i * (2 radius + 1) + k = best_theta[b, r] + (float(i - radius) * s1, float(k - radius) * s2) in fp32 (one rounded multiply, one
    rounded add); a pair whose best_index is -1 is centred on `placeholder` (two finite floats) instead."""
    L = _lib.load()
    _chk(best_theta), _chk(best_index, torch.int64)
    if best_theta.dim() != 3 or best_theta.shape[2] != 2 or tuple(best_index.shape) != tuple(best_theta.shape[:2]) or best_index.numel() == 0:
        raise ValueError(f"best_theta {tuple(best_theta.shape)} / best_index {tuple(best_index.shape)} are not [B, R, 2] / [B, R]")
    B, R = best_index.shape
    W = 2 * int(radius) + 1
    out = torch.empty(B, R * W * W, 2, device=best_theta.device, dtype=torch.float32)
    a = _lib.LocateCandsArgs(best_theta=_p(best_theta), best_index=_p(best_index), cands=_p(out), s1=float(s1), s2=float(s2),
                             ph1=float(placeholder[0]), ph2=float(placeholder[1]), B=B, R=R, radius=int(radius), reserved0=0)
    _lib.check(L.nef_locate_cands(C.byref(a), _stream()), "nef_locate_cands")
    return out


def sgd_momentum(p, g, buf, lr, mu, gscale, first_step, skip=None, lr_dev=None):
    """`skip`: a one-element fp32 device view (h2_taint's output, summed over the ranks): > 0 leaves p and buf untouched and counts
    the step in h2_skipped().  `lr_dev`: a one-element fp32 device tensor that replaces `lr` at run time (captured steps)."""
    L = _lib.load()
    _chk(p), _chk(buf)
    assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
    ev = _hbm("sgd_momentum", p, p, g, buf, buf)
    sk = _p(_amax_state(p.device)["skipped"]) if skip is not None else None
    _lib.check(L.nef_sgd_momentum(_p(p), _p(g), _p(buf), p.numel(), lr, mu, gscale, int(first_step), _p(skip), sk, _p(lr_dev),
                                  _stream()), "nef_sgd_momentum")
    _done(ev)


def adam(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, gscale, skip=None, lr_dev=None):
    """torch.optim.Adam's update (amsgrad=False, L2 weight_decay) over flat fp32 buffers, in place on p / m / v.  `step`: a one-element
    fp32 device tensor holding the completed updates (torch's state["step"]); the launch reads it and advances it on the device, so a
    captured update stays right on every replay.  `skip` / `lr_dev`: as for sgd_momentum (a skipped step leaves `step` as it is)."""
    L = _lib.load()
    _chk(p), _chk(m), _chk(v), _chk(step)
    assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
    assert g.numel() == p.numel() == m.numel() == v.numel() and step.numel() == 1
    ev = _hbm("adam", p, p, g, m, m, v, v)
    sk = _p(_amax_state(p.device)["skipped"]) if skip is not None else None
    _lib.check(L.nef_adam(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, gscale, _p(step), _p(skip), sk,
                          _p(lr_dev), _stream()), "nef_adam")
    _done(ev)


def _update(tag, hbm, rule, p, g, lr, gscale, weight_decay, runs, skip, lr_dev, ema=None, **fields):
    """One nef_update call (include/nefnet_hip.h).  `runs`: None, or the decay run table (run_end int64 [R], run_mul fp32 [R]) on p's
    device -- exclusive ends in flat order, ascending, the last one = p.numel(); the library cannot check it.  `ema`: None, or
    (ema, n_averaged, decay, warmup) -- the call is then nef_update_ema, its tag `tag` + "_ema" and its bytes two streams more."""
    L = _lib.load()
    _chk(p)
    E = None
    if ema is not None:
        e_buf, e_n, decay, warmup = ema
        _chk(e_buf), _chk(e_n)
        assert e_buf.numel() == p.numel() and e_n.numel() == 1
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"Invalid ema decay: {decay}")
        E = _lib.EmaArgs(ema=_p(e_buf), n_averaged=_p(e_n), decay=float(decay), warmup=int(bool(warmup)))
        tag, hbm = tag + "_ema", tuple(hbm) + (e_buf, e_buf)
    assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == p.numel()
    run_end = run_mul = None
    if runs is not None:
        run_end, run_mul = runs
        _chk(run_end, torch.int64), _chk(run_mul)
        assert run_end.numel() == run_mul.numel() > 0
    ev = _hbm(tag, *hbm)
    sk = _p(_amax_state(p.device)["skipped"]) if skip is not None else None
    A = _lib.UpdateArgs(p=_p(p), g=_p(g), n=p.numel(), lr=lr, gscale=gscale, weight_decay=weight_decay, rule=rule,
                        skip_if_positive=_p(skip), skipped=sk, lr_dev=_p(lr_dev), run_end=_p(run_end), run_mul=_p(run_mul),
                        n_runs=0 if run_end is None else run_end.numel(), **fields)
    if E is None:
        _lib.check(L.nef_update(C.byref(A), _stream()), "nef_update")
    else:
        _lib.check(L.nef_update_ema(C.byref(A), C.byref(E), _stream()), "nef_update_ema")
    _done(ev)


def update_sgd(p, g, buf, lr, mu, gscale, weight_decay=0.0, nesterov=False, runs=None, skip=None, lr_dev=None, ema=None):
    """torch.optim.SGD's update (momentum mu, dampening 0, L2 weight_decay, Nesterov) over flat fp32 buffers, in place on p / buf; `buf`
    starts at zero.  `runs`: the decay run table (element i of run r decays with weight_decay * run_mul[r]); None = 1 everywhere.
    `skip` / `lr_dev`: as for sgd_momentum -- a skipped step does not decay either.  `ema`: None, or (ema, n_averaged, decay, warmup):
    the same launch also moves the flat fp32 average `ema` towards the new p by 1 - decay (warmup: 1 - min(decay, (1 + t) / (10 + t)))
    and the one-word device count `n_averaged` = t advances behind it; a skipped step leaves both."""
    _chk(buf)
    assert buf.numel() == p.numel()
    _update("update_sgd", (p, p, g, buf, buf), 0, p, g, lr, gscale, weight_decay, runs, skip, lr_dev, ema=ema, buf=_p(buf), mu=mu,
            nesterov=int(bool(nesterov)))


def update_adam(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, gscale, decoupled=False, runs=None, skip=None, lr_dev=None,
                ema=None):
    """torch.optim.Adam's update with L2 weight_decay, or (`decoupled`) torch.optim.AdamW's, over flat fp32 buffers; `step`, `skip`,
    `lr_dev`: as for adam.  `runs`: the decay run table, `ema`: the weight average, both as for update_sgd."""
    _chk(m), _chk(v), _chk(step)
    assert p.numel() == m.numel() == v.numel() and step.numel() == 1
    _update("update_adamw" if decoupled else "update_adam", (p, p, g, m, m, v, v), 2 if decoupled else 1, p, g, lr, gscale,
            weight_decay, runs, skip, lr_dev, ema=ema, m=_p(m), v=_p(v), step=_p(step), beta1=beta1, beta2=beta2, eps=eps)


def _update_trust(tag, hbm, rule, p, g, lr, gscale, weight_decay, segs, ratio, stats, trust_coef, trust_eps, skip, lr_dev, taint, ema,
                  **fields):
    """One nef_update_trust call (include/nefnet_hip.h).  `segs`: the segment table (seg_end int64 [S], seg_wd_mul fp32 [S], seg_adapt
    fp32 [S]) on p's device -- one segment per parameter tensor, exclusive ends in flat order, ascending, the last one = p.numel(); the
    library cannot check it.  `ratio` fp32 [S] and `stats` fp32 [4] are the caller's: the call writes them.  `ema`: as for _update (the
    tag gets "_ema", the bytes two streams more)."""
    L = _lib.load()
    _chk(p), _chk(ratio), _chk(stats)
    seg_end, seg_wd_mul, seg_adapt = segs
    _chk(seg_end, torch.int64), _chk(seg_wd_mul), _chk(seg_adapt)
    S = seg_end.numel()
    assert 0 < S == seg_wd_mul.numel() == seg_adapt.numel() == ratio.numel() and stats.numel() == 4
    assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == p.numel()
    if taint is not None:
        _chk(taint)
    E = None
    if ema is not None:
        e_buf, e_n, decay, warmup = ema
        _chk(e_buf), _chk(e_n)
        assert e_buf.numel() == p.numel() and e_n.numel() == 1
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"Invalid ema decay: {decay}")
        E = _lib.EmaArgs(ema=_p(e_buf), n_averaged=_p(e_n), decay=float(decay), warmup=int(bool(warmup)))
        tag, hbm = tag + "_ema", tuple(hbm) + (e_buf, e_buf)
    nws = L.nef_update_trust_ws_bytes(p.numel(), S)
    ws = workspace(nws, p.device)
    ev = _hbm(tag, *hbm)
    sk = _p(_amax_state(p.device)["skipped"]) if skip is not None else None
    A = _lib.UpdateArgs(p=_p(p), g=_p(g), n=p.numel(), lr=lr, gscale=gscale, weight_decay=weight_decay, rule=rule,
                        skip_if_positive=_p(skip), skipped=sk, lr_dev=_p(lr_dev), n_runs=0, **fields)
    T = _lib.TrustArgs(seg_end=_p(seg_end), seg_wd_mul=_p(seg_wd_mul), seg_adapt=_p(seg_adapt), ratio=_p(ratio), stats=_p(stats),
                       taint=_p(taint), ws=_p(ws), ws_bytes=nws, trust_coef=float(trust_coef), trust_eps=float(trust_eps), n_segs=S)
    _lib.check(L.nef_update_trust(C.byref(A), C.byref(T), None if E is None else C.byref(E), _stream()), "nef_update_trust")
    _done(ev)
    # the call's trust flag (> 0: norms not finite or a positive skip word -- nothing was applied): the fp32 word at the start of the
    # workspace's last 16 bytes, valid in stream order until the next call that takes the workspace (lr_sched(flag=) reads it)
    return ws[nws - 16:nws - 12].view(torch.float32)


def update_lars(p, g, buf, lr, mu, gscale, segs, ratio, stats, trust_coef=1e-3, trust_eps=1e-8, weight_decay=0.0, nesterov=False,
                skip=None, lr_dev=None, taint=None, ema=None):
    """LARS over flat fp32 buffers, in place on p / buf (`buf` starts at zero): momentum SGD (dampening 0, optional Nesterov) whose
    decayed gradient of segment s is multiplied by q_s = trust_coef * ||p_s|| / (||g'_s|| + wd_s * ||p_s|| + trust_eps), g' = g * gscale,
    wd_s = weight_decay * seg_wd_mul[s]; q_s = 1 where seg_adapt[s] is 0 or a norm is 0.  `segs`: (seg_end int64, seg_wd_mul, seg_adapt)
    device tensors, one entry per parameter tensor.  `ratio` [S] receives the q_s of this call; `stats` (4 words): [0] / [1] the smallest
    / largest q_s over the adapted segments, [2] += 1 when the call updated, [3] += 1 when a norm was not finite -- such a call changes
    nothing else but `taint` (+= 1 when given) and counts in h2_skipped().  `skip`, `lr_dev`, `ema`: as for update_sgd.  The norms are
    deterministic fp64 sums: the same buffers give the same bits eagerly, under graph replay and on every rank.  Capturable.  Returns the
    call's trust flag, a one-element fp32 device view (> 0: nothing was applied) for lr_sched(flag=)."""
    _chk(buf)
    assert buf.numel() == p.numel()
    return _update_trust("update_lars", (p, g, p, p, g, buf, buf), 0, p, g, lr, gscale, weight_decay, segs, ratio, stats, trust_coef, trust_eps,
                  skip, lr_dev, taint, ema, buf=_p(buf), mu=mu, nesterov=int(bool(nesterov)))


def update_lamb(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, gscale, segs, ratio, stats, skip=None, lr_dev=None, taint=None,
                ema=None):
    """LAMB over flat fp32 buffers, in place on p / m / v: Adam's moments and bias corrections (`step` as for adam), the direction
    u = (m / bc1) / (sqrt(v / bc2) + eps) + wd_s * p, and p -= lr * q_s * u with q_s = ||p_s|| / ||u_s|| per segment (1 where seg_adapt[s]
    is 0 or a norm is 0).  `segs`, `ratio`, `stats`, `taint`, `skip`, `lr_dev`, `ema`: as for update_lars."""
    _chk(m), _chk(v), _chk(step)
    assert p.numel() == m.numel() == v.numel() and step.numel() == 1
    return _update_trust("update_lamb", (p, g, m, v, p, p, g, m, m, v, v), 1, p, g, lr, gscale, weight_decay, segs, ratio, stats, 0.0, 0.0,
                  skip, lr_dev, taint, ema, m=_p(m), v=_p(v), step=_p(step), beta1=beta1, beta2=beta2, eps=eps)


LR_SHAPES = {"const": 0, "cosine": 1, "poly": 2}


def lr_sched(t, lr_out, base, shape, warmup_updates=0, warmup_start=0.01, total_updates=0, lr_floor=0.0, poly_power=1.0, advance=True,
             skip=None, flag=None):
    """The per-update learning-rate schedule, one single-wave launch (nef_lr_sched, include/nefnet_hip.h).  `t`: a one-element int64
    device tensor, the updates applied so far; `lr_out`: a one-element fp32 device tensor, the rate the next update reads as `lr_dev`;
    `base`: a one-element fp64 device tensor or a Python float; `shape`: 'const', 'cosine' or 'poly'.  advance: behind an update --
    t += 1 and lr_out = (float)(base * m(t)) unless `skip` (the update's skip word) or `flag` (update_lars' / update_lamb's return) is
    positive, which leaves both words alone.  advance False: lr_out = (float)(base * m(t)) and nothing else.  Capturable."""
    L = _lib.load()
    _chk(t, torch.int64), _chk(lr_out)
    assert t.numel() == 1 and lr_out.numel() == 1
    base_dev = None
    if torch.is_tensor(base):
        base_dev, base = _chk(base, torch.float64), 0.0
        assert base_dev.numel() == 1
    if skip is not None:
        _chk(skip)
    if flag is not None:
        _chk(flag)
    if shape not in LR_SHAPES:
        raise ValueError(f"Invalid lr shape: {shape!r}")
    ev = _timed(("lr_sched", "advance" if advance else "evaluate"))
    A = _lib.LrSchedArgs(t=_p(t), base_dev=_p(base_dev), lr_out=_p(lr_out), skip_if_positive=_p(skip), flag=_p(flag),
                         warmup_updates=int(warmup_updates), total_updates=int(total_updates), base=float(base),
                         warmup_start=float(warmup_start), lr_floor=float(lr_floor), poly_power=float(poly_power),
                         shape=LR_SHAPES[shape], advance=int(bool(advance)))
    _lib.check(L.nef_lr_sched(C.byref(A), _stream()), "nef_lr_sched")
    _done(ev)


def grad_clip(g, max_norm, gscale, stats, taint=None):
    """torch.nn.utils.clip_grad_norm_(max_norm, norm_type=2) on the averaged flat gradient gscale * g, in place on `g` (which stays the
    un-averaged sum: the update behind it applies gscale).  `stats`: 4 fp32 device words -- [0] the norm and [1] the coefficient of this
    call, [2] += 1 when it clipped, [3] += 1 when the norm was not finite.  A non-finite norm leaves g alone and adds 1 to `taint` (the
    word h2_taint wrote: sgd_momentum / adam(skip=taint) then skip the step, h2_skipped() counts it).  Three stream-ordered launches,
    capturable, nothing read by the host."""
    L = _lib.load()
    _chk(stats)
    assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and stats.numel() == 4
    if taint is not None:
        _chk(taint)
    n = L.nef_grad_clip_ws_bytes()
    ws = workspace(n, g.device)
    ev = _hbm("grad_clip", g, g, g)
    _lib.check(L.nef_grad_clip(_p(g), g.numel(), float(max_norm), float(gscale), _p(taint), _p(stats), _p(ws), n, _stream()),
               "nef_grad_clip")
    _done(ev)


# ------------------------------------------------------------------ half-precision panorama decoder (pano_h.hip)
def pano_h_from_f32(x):
    """fp32 [B,C,T] -> fp16 [B,T,C] (time-major)."""
    L = _lib.load()
    _chk(x)
    B, Ct, T = x.shape
    y = torch.empty(B, T, Ct, device=x.device, dtype=torch.float16)
    _lib.check(L.nef_pano_h_from_f32(_p(x), _p(y), B, Ct, T, _stream()), "nef_pano_h_from_f32")
    return y


def pano_h_pack_weight(w):
    """fp32 [Cout,Cin,3] -> fp16 MFMA A-fragment order (flat)."""
    L = _lib.load()
    _chk(w)
    Co, Ci, K = w.shape
    assert K == 3
    wp = torch.empty(Co * Ci * 3, device=w.device, dtype=torch.float16)
    _lib.check(L.nef_pano_h_pack_weight(_p(w), _p(wp), Co, Ci, _stream()), "nef_pano_h_pack_weight")
    return wp


def pano_h_conv(x, wp, bias, Cout, N=None, upsample=False, scale=None, x_div=1, nq=1, out=None):
    """ReLU(conv_k3(pro(x)) + bias) on fp16 [.,Tin,Cin] -> fp16 [N,T,Cout].  `scale` = (tensor, sc_bs, sc_is)."""
    L = _lib.load()
    _chk(x, torch.float16), _chk(bias)
    Tin, Ci = x.shape[1], x.shape[2]
    N = x.shape[0] * x_div if N is None else N
    T = 2 * Tin if upsample else Tin
    y = torch.empty(N, T, Cout, device=x.device, dtype=torch.float16) if out is None else out
    mode = (1 if scale is not None else 0) | (2 if upsample else 0)
    sc, sc_bs, sc_is = scale if scale is not None else (None, 0, 0)
    e = _timed(("pano_h_conv", Ci, Cout, N, T))
    _lib.check(L.nef_pano_h_conv(_p(x), _p(wp), _p(bias), _p(sc), _p(y), N, T, Ci, Cout, mode, x_div, nq, sc_bs, sc_is,
                                 _stream()), "nef_pano_h_conv")
    if e is not None:
        e.record()
    return y


PANO_PAIR_MAX_T = 256     # nef_pano_h_conv_pair: up to here one 256-row tile per (sample, angle); longer sequences in tiles of 252 output rows


def pano_h_conv_pair(x, wp1, bias1, scale, wp2, bias2, N, x_div, nq, out=None):
    """Decoder layers 1 + 2 in one pass (c1 stays on chip): x fp16 [.,Tin,256] -> fp16 [N,2*Tin,128].  Up to 256 output rows one tile per
    pair; longer sequences (round 6) in tiles of 252 output rows with two recomputed slots + one halo row per side.
    `scale` = (tensor, sc_bs, sc_is) as in pano_h_conv."""
    L = _lib.load()
    _chk(x, torch.float16), _chk(bias1), _chk(bias2)
    Tin, Ci = x.shape[1], x.shape[2]
    T = 2 * Tin
    assert Ci == 256
    y = torch.empty(N, T, 128, device=x.device, dtype=torch.float16) if out is None else out
    sc, sc_bs, sc_is = scale
    e = _timed(("pano_h_conv_pair", N, T))
    _lib.check(L.nef_pano_h_conv_pair(_p(x), _p(wp1), _p(bias1), _p(sc), _p(wp2), _p(bias2), _p(y), N, T, x_div, nq,
                                      sc_bs, sc_is, _stream()), "nef_pano_h_conv_pair")
    if e is not None:
        e.record()
    return y


PANO_TAIL_MAX_T = 512     # nef_pano_h_conv_tail: up to here one tile per (sample, angle); longer sequences in tiles of 508 output rows


def pano_h_conv_tail(x, wp3, bias3, wp4, bias4, wout, bout, out, nq, out_bs, out_is):
    """Layers 3 + 4 + last conv + sigmoid(x/3) in one pass (c3, c4 stay on chip): x fp16 [N, Tin, 128] (layer 2's output) -> the fp32
    views at `out` (view base, addressed as in pano_h_conv_outconv).  Sequences of up to 512 rows are one tile per pair; longer ones run
    in tiles of 508 output rows with three recomputed halo rows per side."""
    L = _lib.load()
    _chk(x, torch.float16), _chk(bias3), _chk(bias4), _chk(wout)
    N, Tin, Ci = x.shape
    assert Ci == 128
    e = _timed(("pano_h_conv_tail", N, 2 * Tin))
    _lib.check(L.nef_pano_h_conv_tail(_p(x), _p(wp3), _p(bias3), _p(wp4), _p(bias4), _p(wout), _p(bout), _p(out), N, 2 * Tin, nq,
                                      out_bs, out_is, _stream()), "nef_pano_h_conv_tail")
    if e is not None:
        e.record()
    return out


def pano_h_outconv(x, w, bias, out, nq, out_bs, out_is):
    """out[(n/nq)*out_bs + (n%nq)*out_is + t] = sigmoid((conv_k3(x[n]) + bias)/3); x fp16 [N,T,64], out fp32 view base."""
    L = _lib.load()
    _chk(x, torch.float16), _chk(w)
    N, T, Ci = x.shape
    assert Ci == 64
    _lib.check(L.nef_pano_h_outconv(_p(x), _p(w), _p(bias), _p(out), N, T, nq, out_bs, out_is, _stream()),
               "nef_pano_h_outconv")
    return out


def pano_h_conv_outconv(x, wp, bias, wout, bout, out, nq, out_bs, out_is):
    """Layer 4 (64->64) + last conv + sigmoid(x/3) in one pass; x fp16 [N,T,64], out fp32 view base."""
    L = _lib.load()
    _chk(x, torch.float16), _chk(bias), _chk(wout)
    N, T, Ci = x.shape
    assert Ci == 64
    e = _timed(("pano_h_conv_outconv", N, T))
    _lib.check(L.nef_pano_h_conv_outconv(_p(x), _p(wp), _p(bias), _p(wout), _p(bout), _p(out), N, T, nq, out_bs, out_is,
                                         _stream()), "nef_pano_h_conv_outconv")
    if e is not None:
        e.record()
    return out
