"""Whole recordings on their own time axis and in their own units, synthesised beat by beat.

The model sees one beat at a time, min-max normalised and padded to 512 positions.  `synthesize` walks every beat of every recording of a
device-resident store (dataset/resident.py) in order -- no draw: `recording_plan` -- and per chunk of whole recordings builds the beats'
input leads (ops.beat_batch), keeps each beat's (lo, hi) (ops.beat_range), decodes its views at the query angles in one encoder pass and
one eval-mode sweep (Model_nefnet.panorama), and writes them, de-normalised, at the beat's P onset of the recording's [A, len] signals
(ops.beat_stitch).  One ops.recording_stats launch then scores every (recording, angle) against a stored or derived lead in fp64.
Everything is stream-ordered; the host reads nothing until the caller asks a `Synthesis` for numbers.

Not done here: smoothing of the seams between independently normalised beats; the positions before a recording's first and after its last
P onset (no beat: NaN); PTB; more than one rank."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops, resample
from .dataset import marks
from .dataset.resident import RecordingPlan, check_leads, recording_plan, stage_to_device
from .synth import LEAD_THETA

STAT_NAMES = ("count", "se", "su", "sw", "suu", "sww", "suw")


def metrics(stats):
    """(rmse, corr), fp64 [..., A], from the [..., A, 7] sums of ops.recording_stats on the host: rmse = sqrt(se / count) in signal units,
    corr = c / sqrt(vx * vy) from the shifted moments; NaN for count < 2, for vx * vy <= 0 and for an angle that was not scored (count 0)."""
    s = np.asarray(stats, dtype=np.float64)
    cnt, se, su, sw, suu, sww, suw = (s[..., k] for k in range(7))
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.sqrt(se / cnt)
        c, vx, vy = suw - su * sw / cnt, suu - su * su / cnt, sww - sw * sw / cnt
        corr = c / np.sqrt(vx * vy)
        corr = np.where(vx * vy > 0, corr, np.nan)
    few = ~(cnt >= 2)
    return np.where(few, np.nan, rmse), np.where(few, np.nan, corr)


class Synthesis(NamedTuple):
    """What synthesize returns.  Tensors are on the store's device; `rmse` / `corr` read `stats` (they synchronise)."""
    out: torch.Tensor                   # the flat fp32 buffer: recording j at [plan.out_offsets[j], plan.out_offsets[j + 1]) as [A, len_j]
    range: torch.Tensor                 # fp64 [Bt, 2]: every beat's (lo, hi)
    stats: torch.Tensor                 # fp64 [N, A, 7]: ops.recording_stats
    plan: RecordingPlan
    score_leads: tuple
    views: Optional[torch.Tensor]       # fp32 [Bt, A, 512] with return_views, else None
    native: Optional[torch.Tensor] = None       # native_rate on a resampled store: the flat fp32 buffer of the [A, raw_len_j] strips
    native_offsets: Optional[np.ndarray] = None # int64 [N + 1]: recording j at [native_offsets[j], native_offsets[j + 1]) of `native`

    @property
    def native_signals(self):
        """Per recording the [A, raw_len] strip at the store's source rate; `signals` when nothing was resampled."""
        if self.native is None:
            return self.signals
        o, A = self.native_offsets, self.plan.A
        return [self.native[int(o[j]):int(o[j + 1])].view(A, -1) for j in range(len(o) - 1)]

    @property
    def signals(self):
        """Per recording the [A, len] view of `out`: NaN before the first and from the last P onset on."""
        o, A = self.plan.out_offsets, self.plan.A
        return [self.out[int(o[j]):int(o[j + 1])].view(A, -1) for j in range(len(o) - 1)]

    @property
    def rmse(self):
        return metrics(self.stats.cpu().numpy())[0]

    @property
    def corr(self):
        return metrics(self.stats.cpu().numpy())[1]


def chunks(plan, beats_per_pass):
    """[(first row, end row)] of whole recordings with at most beats_per_pass beats each; a recording with more forms a chunk alone."""
    out, r0, rows = [], 0, 0
    for first, cnt in plan.recordings[:, :2].tolist():
        if rows and rows + cnt > beats_per_pass:
            out.append((r0, r0 + rows))
            r0, rows = first, 0
        rows += cnt
    out.append((r0, r0 + rows))
    return out


def to_native_rate(store, out, out_offsets, lengths, raw_lengths, A, budget=1 << 25):
    """The [A, len'] strips of `out` (recording j at out_offsets[j]) back at the store's source rate: resampled with the swapped ratio
    (resample.design(down, up); one ops.resample per chunk of whole recordings, rows = A, fp32 in) and cut to raw_len columns -- the way
    back gives ceil(len' down / up) >= raw_len of them, so nothing has to be held at the edge; a recording for which that is raw_len
    itself is written in place, the others pass through a scratch buffer.  NaNs spread as the formula says: by at most
    K samples.  Returns (flat fp32 buffer, int64 offsets [N + 1])."""
    src = store.source
    resample.check_ratio(src.down, src.up, src.zeros, f"DATA.sample_rate {src.sample_rate}", f"DATA.source_rate {src.source_rate}")
    taps, first = resample.design(src.down, src.up, src.zeros, src.beta)
    dev = out.device
    taps_d, first_d = torch.from_numpy(taps).to(dev), torch.from_numpy(first).to(dev)
    back = resample.out_len(lengths, src.down, src.up)
    noff = np.concatenate([[0], np.cumsum(A * raw_lengths)]).astype(np.int64)
    native = torch.empty(int(noff[-1]), dtype=torch.float32, device=dev)
    exact = back == raw_lengths                          # these land in `native` as they are; the others go through `tmp` and are cut
    tmp = None
    for a, b in marks._chunks((A * back).tolist(), int(budget)):
        toff = np.concatenate([[0], np.cumsum(np.where(exact[a:b], 0, A * back[a:b]))]).astype(np.int64)
        for direct in (True, False):
            rows = np.flatnonzero(exact[a:b] == direct)
            if not rows.size:
                continue
            if not direct and (tmp is None or tmp.numel() < int(toff[-1])):
                tmp = torch.empty(int(toff[-1]), dtype=torch.float32, device=dev)
            table = np.stack([out_offsets[a:b][rows], lengths[a:b][rows], (noff[a:b] if direct else toff[:-1])[rows],
                              np.full(rows.size, A, dtype=np.int64)], axis=1)
            ops.resample(out, torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)), native if direct else tmp, taps_d, first_d,
                         src.down, src.up)
            if not direct:
                for r in rows.tolist():
                    n, raw, j = int(back[a + r]), int(raw_lengths[a + r]), a + r
                    native[int(noff[j]):int(noff[j + 1])].view(A, raw).copy_(tmp[int(toff[r]):int(toff[r + 1])].view(A, n)[:, :raw])
    return native, noff


def synthesize(model, store, indices, input_leads, query_thetas=None, score_leads=None, fill="nan", beats_per_pass=256, return_views=False,
               native_rate=False):
    """The recordings `indices` of `store` (a ResidentTianchi on the model's device) at the angles query_thetas ([A, 2]; None: the 12 rows
    of LEAD_THETA), predicted from their `input_leads`.  score_leads: per angle the lead 0..11 that is its truth, or -1 (None: 0..11 with
    the default angles, else none).  fill: 'nan' or 'bridge' for the positions of a beat behind its 512-sample row (ops.beat_stitch).
    A beat whose range is not finite or is flat (hi == lo) has no normalised form: its input rows go to the model as zeros -- its NaNs
    would spoil the chunk's shared activation scales -- and its output is what the stitch makes of that range (NaN, or the constant lo).
    native_rate: on a store that was resampled (DATA.source_rate) the strips are also handed back at the source rate, [A, raw_len] each
    (Synthesis.native, .native_signals: to_native_rate); the statistics are still taken at the model's rate.  On any other store it
    changes nothing.  On a store that was cleaned (DATA.baseline_ms / DATA.mains_hz) the strips and the scores are in the cleaned signal's
    units: the baseline and the hum the store removed are not put back."""
    if fill not in ops.STITCH_FILLS:
        raise ValueError(f"fill must be one of {ops.STITCH_FILLS}, got {fill!r}")
    leads = check_leads(input_leads)
    if isinstance(beats_per_pass, bool) or not isinstance(beats_per_pass, int) or beats_per_pass < 1:
        raise ValueError(f"beats_per_pass must be an integer >= 1, got {beats_per_pass!r}")
    theta = np.asarray(LEAD_THETA if query_thetas is None else (query_thetas.detach().cpu().numpy() if torch.is_tensor(query_thetas)
                                                                else query_thetas), dtype=np.float32)
    if theta.ndim != 2 or theta.shape[0] < 1 or theta.shape[1] != 2:
        raise ValueError(f"query_thetas {theta.shape} is not [A >= 1, 2]")
    A = theta.shape[0]
    if score_leads is None:
        score_leads = list(range(12)) if query_thetas is None else [-1] * A
    score = [int(v) for v in score_leads]
    if len(score) != A or any(not -1 <= v <= 11 for v in score):
        raise ValueError(f"score_leads {score}: one lead in -1..11 per angle ({A})")
    dev = store.signal.device
    if dev.type != "cuda":
        raise ValueError("synthesize: the store is on the CPU; build it on the model's device (ResidentTianchi(cfg, phase, device))")
    mdev = next(model.parameters()).device
    if mdev != dev:
        raise ValueError(f"synthesize: the model is on {mdev}, the store on {dev}")
    plan = recording_plan(store, indices, leads, angles=A)
    V, Bt = plan.plan.V, plan.rec.size
    out = torch.full((int(plan.out_offsets[-1]),), float("nan"), dtype=torch.float32, device=dev)
    rng = torch.empty((Bt, 2), dtype=torch.float64, device=dev)
    views_all = torch.empty((Bt, A, ops.BEAT_LEN), dtype=torch.float32, device=dev) if return_views else None
    q = torch.from_numpy(theta).to(dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    for r0, r1 in chunks(plan, beats_per_pass):
        table, rois, in_th, stitch = stage_to_device((plan.plan.table[r0:r1], plan.plan.rois[r0:r1], plan.plan.input_theta[r0:r1],
                                                      plan.stitch[r0:r1]), dev)
        data = ops.beat_batch(store.signal, table, V, 0)[0]
        r = ops.beat_range(store.signal, table, V, 0)
        usable = torch.isfinite(r).all(dim=1) & (r[:, 1] > r[:, 0])
        data = torch.where(usable[:, None, None], data, zero)
        views = model.panorama(data, in_th, rois, q)
        ops.beat_stitch(views, r, stitch, out, fill)
        rng[r0:r1] = r
        if views_all is not None:
            views_all[r0:r1] = views
    beat_table, rec_table, offs = stage_to_device((plan.stitch, plan.recordings, plan.out_offsets[:-1]), dev)
    stats = ops.recording_stats(out, store.signal, beat_table, rec_table, score, fill, offs)
    native, noff = None, None
    if native_rate and getattr(store, 'source', None) is not None:
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        native, noff = to_native_rate(store, out, plan.out_offsets[:-1], store.lengths[idx], store.raw_lengths[idx], A)
    return Synthesis(out=out, range=rng, stats=stats, plan=plan, score_leads=tuple(score), views=views_all, native=native, native_offsets=noff)
