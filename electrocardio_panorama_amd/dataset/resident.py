"""Tianchi batches built on the device from recordings kept in device memory (cfg.DATA.device_resident).

The host path (dataset/tianchi.py behind a 16-worker DataLoader) builds every beat in numpy.  Here the phase's recordings are read once
and packed into one device tensor (`ResidentTianchi`); per batch the host only makes the draws of `EcgTianChiInterval.__getitem__` -- the
beat, the input leads, the target lead -- into a small integer table (`draw_plan`), and one launch of nef_beat_batch (ops.beat_batch) crops,
derives the four limb leads, normalises and pads.  The bits are the host path's: the kernel works in fp64 from a lossless copy of the
stored values.  `ResidentLoader` is the iterable of `meta` dicts the Solver consumes in place of the DataLoader.

Left out on this path, and rejected where the key is read: DATA.noise (it needs the quiet segment's sigma and a device draw, a different
random stream from the host's), DATA.weighted_sample, DATA.synthetic and every dataset but tianchi (PTB).  DATA.device_noise is that device
draw, made by the train step from the batch this path builds (device_noise.py): it goes with the key."""
import os
import random
import warnings
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch

from .. import clean, resample
from ..synth import LEAD_THETA
from . import marks
from .tianchi import BEAT_LEN, EcgTianChiInterval, _lead_plan

LABEL_KEYS = ('P on', 'P off', 'R on', 'R off', 'T on', 'T off')
READERS = 16          # files read at a time; a constant, never the host's core count (a job's CPU allotment is smaller than the machine)


def check_cfg(cfg):
    """DATA.device_resident goes with the tianchi dataset and without DATA.noise / weighted_sample / synthetic: ValueError otherwise."""
    if cfg.DATA.get('dataset', 'tianchi') != 'tianchi':
        raise ValueError(f"DATA.device_resident keeps Tianchi recordings on the device; DATA.dataset {cfg.DATA.dataset!r} is not built there")
    if cfg.DATA.get('noise', False):
        raise ValueError("DATA.device_resident with DATA.noise: the noise row needs the quiet segment's sigma and a host draw; "
                         "it is not built on the device (DATA.device_noise: the train step draws the row itself)")
    if cfg.DATA.get('weighted_sample', False):
        raise ValueError("DATA.device_resident with DATA.weighted_sample: the weighted draw is not planned on this path")
    if cfg.DATA.get('synthetic', False):
        raise ValueError("DATA.device_resident with DATA.synthetic: synthetic batches have no recordings to keep on the device")
    marks.check_cfg(cfg)                                   # DATA.auto_marks needs DATA.mark_table
    source_plan(cfg)                                       # DATA.source_rate: whole rates, a ratio nef_resample takes
    clean.clean_plan(cfg)                                  # DATA.baseline_ms / DATA.mains_hz: windows and a band the kernels take


class SourcePlan(NamedTuple):
    """DATA.source_rate read: the two rates, their ratio and the filter's two parameters."""
    source_rate: int
    sample_rate: int
    up: int
    down: int
    zeros: int
    beta: float


def source_plan(cfg, need_resident=True):
    """None with DATA.source_rate off (0, or DATA.sample_rate itself), else the SourcePlan.  ValueError: the key without
    DATA.device_resident (the loaders; the store itself does not ask), a rate that is not a whole positive number of Hz, a ratio or a
    filter outside nef_resample's limits."""
    src = cfg.DATA.get('source_rate', 0)
    if isinstance(src, bool) or not isinstance(src, (int, float)) or src != src or src != int(src) or src < 0:
        raise ValueError(f"DATA.source_rate = {src!r}: a whole number of Hz, or 0 for off; non-integer and negative rates are not resampled")
    src = int(src)
    if src == 0:
        return None
    if need_resident and not cfg.DATA.get('device_resident', False):
        raise ValueError("DATA.source_rate resamples the recordings of the device-resident store: set DATA.device_resident (the host "
                         "loader stays file based; `python -m electrocardio_panorama_amd.mark_net --resample DIR` writes files for it)")
    try:
        dst = resample.check_rate("DATA.sample_rate", cfg.DATA.get('sample_rate', 500.0))
    except ValueError as e:
        raise ValueError(f"{e}; DATA.source_rate = {src} needs an integer DATA.sample_rate") from None
    if src == dst:
        return None
    zeros, beta = cfg.DATA.get('resample_zeros', 16), cfg.DATA.get('resample_beta', 8.6)
    if isinstance(zeros, bool) or not isinstance(zeros, int) or zeros < 1:
        raise ValueError(f"DATA.resample_zeros = {zeros!r}: an integer >= 1")
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 <= float(beta) < float('inf'):
        raise ValueError(f"DATA.resample_beta = {beta!r}: a finite number >= 0")
    up, down = resample.ratio(src, dst)
    resample.check_ratio(up, down, zeros, f"DATA.source_rate {src}", f"DATA.sample_rate {dst}")
    return SourcePlan(src, dst, up, down, zeros, float(beta))


def _pack(name, sig):
    """One recording's [8, len] float64 signal as int16 when that is lossless, else as float32 when that is, else ValueError."""
    sig = np.asarray(sig)
    if sig.ndim != 2 or sig.shape[0] != 8 or sig.shape[1] < 1:
        raise ValueError(f"recording {name}: signal {sig.shape} is not [8, len]")
    with np.errstate(invalid='ignore'):
        as16 = sig.astype(np.int16)
    if np.array_equal(as16.astype(np.float64), sig):
        return as16
    with np.errstate(over='ignore'):
        as32 = sig.astype(np.float32)
    if np.array_equal(as32.astype(np.float64), sig):
        return as32
    raise ValueError(f"recording {name}: its values survive neither int16 nor float32 storage exactly; the device path "
                     "cannot promise the host path's bits from a lossy copy")


class ResidentTianchi:
    """Every recording of the phase's label list, read once through `EcgTianChiInterval._load` (.npy + .json, or .npz bundles).

    signal        flat int16 tensor on `device` -- float32 when some value of some recording is not an int16 -- recording i at
                  [offsets[i], offsets[i + 1]) as [8, lengths[i]], lead-major
    offsets       int64 numpy [N + 1], in elements; lengths int64 numpy [N]
    labels[k]     the six 'P on' .. 'T off' index lists, each concatenated over the recordings (host numpy int64, never on the device),
                  recording i at [label_offsets[k][i], label_offsets[k][i + 1])
    names         the label list's lines (the `id` of a sample)
    `device` None or 'cpu' keeps `signal` on the host (packing only: ops.beat_batch has no CPU path).

    `marks` (or cfg.DATA.auto_marks, which reads cfg.DATA.mark_table): the signals alone are read -- no label file is opened -- and the
    six lists are made on the device from a timing table (dataset/marks.py: detect, labels_from_peaks).  `marks` is a [6, 2] table, a
    (table, MarkParams) pair or the path of a table file; it needs a HIP `device`.  A recording that gets no labels raises a ValueError
    naming it; with cfg.DATA.auto_marks_skip it is dropped from `names` and counted in one warning.  `auto_report` holds the counts
    (None on an annotated store).

    cfg.DATA.source_rate (not 0, not DATA.sample_rate): the files hold recordings at that rate.  They are packed and uploaded as above,
    resampled on the device to DATA.sample_rate (resample.design; ops.resample, one launch per chunk) into a float32 `signal` with new
    `lengths` and `offsets`, and the raw buffer is released; annotated label lists are rescaled on the host (resample.rescale_all) and
    checked again, auto marks are detected on the resampled signal.  It needs a HIP `device`.  `source_rate` (0: the files were at the
    model's rate), `raw_lengths` (the files' lengths), `source` (the SourcePlan, or None) and `resample_report` (None when off) stay.

    cfg.DATA.baseline_ms / cfg.DATA.mains_hz (clean.py): behind the resampling and in front of the marks the recordings are cleaned on the
    device, per chunk of whole recordings -- the mains band-stop first (ops.resample at 1/1 with clean.notch_taps' row), then the signal
    minus the h2 sliding median of its h1 sliding median (ops.sliding_median, twice) -- into a float32 `signal`; `lengths`, `offsets`
    and annotated labels stay, auto marks are detected on the cleaned signal.  It needs a HIP `device`.  `clean` holds the CleanPlan (None
    with both keys off) and `clean_report` the recordings, h1, h2, the taps and the launch count (None when off)."""

    def __init__(self, cfg, phase, device=None, marks=None):
        ds = EcgTianChiInterval(cfg, phase)
        self.cfg, self.phase, self.names = cfg, phase, list(ds.dataset)
        self.auto_report = None
        self.source = source_plan(cfg, need_resident=False)
        self.source_rate, self.resample_report = 0 if self.source is None else self.source.source_rate, None
        self.clean, self.clean_report = clean.clean_plan(cfg, need_resident=False), None
        if not self.names:
            raise ValueError(f"DATA.device_resident: the {phase} label list is empty")
        spec = marks
        if spec is None and cfg.DATA.get('auto_marks', False):
            spec = cfg.DATA.get('mark_table', '')
            if not spec:
                raise ValueError("DATA.auto_marks needs DATA.mark_table: the JSON timing table `mark_net --fit` writes")

        def read(name):
            if spec is not None:
                return _pack(name, ds._load_signal(name)), None
            sig, label = ds._load(name)
            lab = [np.asarray(label[k], dtype=np.int64).reshape(-1) for k in LABEL_KEYS]
            self._check_labels(name, lab, sig.shape[-1])
            return _pack(name, sig), lab

        with ThreadPoolExecutor(max_workers=min(READERS, len(self.names))) as pool:
            items = list(pool.map(read, self.names))          # results (and the first error) in list order
        sigs = [s for s, _ in items]
        if any(s.dtype != np.int16 for s in sigs):
            sigs = [s.astype(np.float32) for s in sigs]        # int16 -> float32 is exact
        self.lengths = np.array([s.shape[1] for s in sigs], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(8 * self.lengths)]).astype(np.int64)
        flat = torch.from_numpy(np.concatenate([s.reshape(-1) for s in sigs]))
        dev = torch.device('cpu' if device is None else device)
        self.signal = flat if dev.type == 'cpu' else flat.to(dev)
        self.raw_lengths = self.lengths
        if self.source is not None:
            self._resample()
        if self.clean is not None:
            self._clean()
        if spec is not None:
            self._auto_mark(spec, bool(cfg.DATA.get('auto_marks_skip', False)))
            return
        if self.source is not None:
            self._rescale_labels([lab for _, lab in items])
        else:
            self.labels = [np.concatenate([lab[k] for _, lab in items]) for k in range(6)]
            self.label_offsets = [np.concatenate([[0], np.cumsum([lab[k].size for _, lab in items])]).astype(np.int64) for k in range(6)]
        self.n_p_on = np.diff(self.label_offsets[0])

    def _resample(self, budget=1 << 25):
        """`signal` from source.source_rate to source.sample_rate on the device: chunks of whole recordings of at most `budget` output
        samples, one ops.resample launch each, all into one float32 buffer that replaces the raw one."""
        from .. import ops
        src = self.source
        if not self.signal.is_cuda:
            raise RuntimeError("DATA.source_rate resamples on a HIP device only: build the store on one (no CPU path)")
        taps, first = resample.design(src.up, src.down, src.zeros, src.beta)
        lengths = resample.out_len(self.raw_lengths, src.up, src.down)
        offsets = np.concatenate([[0], np.cumsum(8 * lengths)]).astype(np.int64)
        out = torch.empty(int(offsets[-1]), dtype=torch.float32, device=self.signal.device)
        taps_d, first_d = torch.from_numpy(taps).to(out.device), torch.from_numpy(first).to(out.device)
        chunks = marks._chunks((8 * lengths).tolist(), int(budget))
        for a, b in chunks:
            table = np.stack([self.offsets[a:b], self.raw_lengths[a:b], offsets[a:b], np.full(b - a, 8, dtype=np.int64)], axis=1)
            ops.resample(self.signal, torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)), out, taps_d, first_d, src.up, src.down)
        self.signal, self.lengths, self.offsets = out, lengths, offsets
        self.resample_report = {'recordings': len(self.names), 'source_rate': src.source_rate, 'sample_rate': src.sample_rate, 'up': src.up,
                                'down': src.down, 'taps': int(taps.shape[1]), 'launches': len(chunks), 'adjusted': 0}

    def _clean(self, budget=1 << 25):
        """`signal` cleaned on the device (clean.py), in chunks of whole recordings of at most `budget` samples: the band-stop at
        clean.mains_hz by one ops.resample at 1/1 per chunk into a fresh float32 buffer that replaces the one before; then per chunk
        tmp = median_h1(signal) and out = signal - median_h2(tmp) by two ops.sliding_median launches, one `tmp` of at most a chunk,
        `out` a fresh float32 store."""
        from .. import ops
        plan = self.clean
        if not self.signal.is_cuda:
            raise RuntimeError("DATA.baseline_ms / DATA.mains_hz clean on a HIP device only: build the store on one (no CPU path)")
        dev = self.signal.device
        chunks = marks._chunks((8 * self.lengths).tolist(), int(budget))
        eight = np.full(len(self.names), 8, dtype=np.int64)
        launches, K = 0, 0
        if plan.mains_hz > 0:
            taps, first = clean.notch_taps(plan.rate, plan.mains_hz, plan.width, plan.taps, plan.beta)
            taps_d, first_d = torch.from_numpy(taps).to(dev), torch.from_numpy(first).to(dev)
            out = torch.empty(int(self.offsets[-1]), dtype=torch.float32, device=dev)
            for a, b in chunks:
                table = np.stack([self.offsets[a:b], self.lengths[a:b], self.offsets[a:b], eight[a:b]], axis=1)
                ops.resample(self.signal, torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)), out, taps_d, first_d, 1, 1)
            self.signal, launches, K = out, launches + len(chunks), int(taps.shape[1])
        if plan.h1 > 0:
            out = torch.empty(int(self.offsets[-1]), dtype=torch.float32, device=dev)
            tmp = torch.empty(int(max(self.offsets[b] - self.offsets[a] for a, b in chunks)), dtype=torch.float32, device=dev)
            for a, b in chunks:
                lo, hi = int(self.offsets[a]), int(self.offsets[b])
                table = np.stack([self.offsets[a:b] - lo, self.lengths[a:b], eight[a:b]], axis=1)
                table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64))
                part = self.signal[lo:hi]                                   # a chunk starts at a multiple of 8 elements: 16-byte aligned
                ops.sliding_median(part, table, tmp[:hi - lo], plan.h1)
                ops.sliding_median(tmp[:hi - lo], table, out[lo:hi], plan.h2, minuend=part)
            self.signal, launches = out, launches + 2 * len(chunks)
        self.clean_report = {'recordings': len(self.names), 'h1': plan.h1, 'h2': plan.h2, 'taps': K, 'launches': launches}

    def _rescale_labels(self, labs):
        """`labels` / `label_offsets` from the annotated lists on the resampled time axis (resample.rescale_all: every recording in one
        pass), checked against the new lengths."""
        self.labels, self.label_offsets, moved = resample.rescale_all(labs, self.source.up, self.source.down)
        self.resample_report['adjusted'] = moved
        for i, name in enumerate(self.names):
            self._check_labels(name, [self.labels[k][self.label_offsets[k][i]:self.label_offsets[k][i + 1]] for k in range(6)],
                               int(self.lengths[i]))

    def _auto_mark(self, spec, skip):
        """Fill labels, label_offsets and n_p_on from the signals (dataset/marks.py); recordings without labels raise, or leave with `skip`."""
        if isinstance(spec, (str, os.PathLike)):
            table, _, params = marks.load_table(spec)
        elif isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[1], marks.MarkParams):
            table, params = spec
        else:
            table, params = spec, marks.MarkParams()
        table = marks._check_table(table)
        found = marks.detect(self, params=params)
        lab = marks.labels_from_peaks(found.peaks, found.count, self.lengths, table)
        beats = np.diff(lab.label_offsets[0])
        bare = np.flatnonzero(beats < 2)
        report = {'recordings': len(self.names), 'marked': len(self.names) - bare.size, 'skipped': [self.names[i] for i in bare.tolist()],
                  'peaks': int(np.maximum(found.count, 0).sum()), 'dropped': int(lab.dropped.sum()), 'adjusted': int(lab.adjusted.sum())}
        labels, offsets = lab.labels, lab.label_offsets
        if bare.size:
            if not skip:
                i = int(bare[0])
                raise ValueError(f"recording {self.names[i]}: no labels from its {int(found.count[i])} detected peaks ({bare.size} of "
                                 f"{len(self.names)} recordings have none; DATA.auto_marks_skip drops them)")
            keep = np.flatnonzero(beats >= 2)
            if not keep.size:
                raise ValueError(f"DATA.auto_marks: none of the {len(self.names)} recordings of the {self.phase} list got labels")
            warnings.warn(f"DATA.auto_marks_skip: {bare.size} of {len(self.names)} recordings of the {self.phase} list got no labels and "
                          f"were dropped (first: {self.names[int(bare[0])]})")
            self.signal = torch.cat([self.signal[self.offsets[i]:self.offsets[i + 1]] for i in keep.tolist()])
            self.names = [self.names[i] for i in keep.tolist()]
            self.lengths, self.raw_lengths = self.lengths[keep], self.raw_lengths[keep]
            self.offsets = np.concatenate([[0], np.cumsum(8 * self.lengths)]).astype(np.int64)
            offsets = [np.concatenate([[0], np.cumsum(beats[keep])]).astype(np.int64) for _ in range(6)]      # bare recordings hold no marks
        self.labels, self.label_offsets = labels, offsets
        self.n_p_on = np.diff(self.label_offsets[0])
        for i, name in enumerate(self.names):
            self._check_labels(name, [self.labels[k][offsets[k][i]:offsets[k][i + 1]] for k in range(6)], int(self.lengths[i]))
        self.auto_report = report

    @staticmethod
    def _check_labels(name, lab, length):
        """Every beat a draw can pick is usable: at least two P onsets, each with its five other marks, 0 <= p_on < the next p_on <= len."""
        p_on = lab[0]
        if p_on.size < 2:
            raise ValueError(f"recording {name}: {p_on.size} 'P on' entries, no drawable beat (two are needed)")
        if any(v.size < p_on.size - 1 for v in lab[1:]):
            raise ValueError(f"recording {name}: a label list is shorter than its {p_on.size - 1} drawable beats")
        if p_on[0] < 0 or np.any(np.diff(p_on) < 1) or p_on[-1] > length:
            raise ValueError(f"recording {name}: 'P on' must rise strictly within [0, {length}]")

    def __len__(self):
        return len(self.names)

    @property
    def device_bytes(self):
        return self.signal.numel() * self.signal.element_size()


class Plan(NamedTuple):
    """What draw_plan returns: `table` goes to the kernel, the rest is the batch's small host part."""
    table: np.ndarray           # int64 [B, 3 + V + 1 + R]: offset of lead 0 at p_on, lead stride, n, V input leads, target lead, R rest leads
    rois: np.ndarray            # int64 [B, 7, 2]
    input_theta: np.ndarray     # float32 [B, V, 2]
    target_theta: np.ndarray    # float32 [B, 2]
    rest_theta: np.ndarray      # float32 [B, R, 2]
    id: list
    unsupervision_lead_name: list
    V: int
    R: int
    beats: np.ndarray           # int64 [B]: the beat drawn of every sample's recording


def draw_plan(store, indices, cfg, phase, rng, jitter_rng=None):
    """The draws of `EcgTianChiInterval.__getitem__` for the recordings `indices`, item after item and in its order -- the beat, the input-lead
    scheme's draws, the target lead -- from `rng` (a `random.Random`, or the `random` module).  MODEL.jitter_factor > 0 in the train phase
    draws the angles' jitter from `jitter_rng`, a numpy Generator (required then); numpy's global state is never used."""
    jitter = float(cfg.MODEL.jitter_factor) if phase == 'train' else 0.0
    if jitter > 0 and jitter_rng is None:
        raise ValueError("MODEL.jitter_factor > 0: draw_plan needs a numpy Generator for the jitter (jitter_rng)")
    lead_num, super_mode, data_mode = cfg.DATA.lead_num, cfg.DATA.super_mode, cfg.DATA.train_data_mode
    idx = np.asarray(list(indices), dtype=np.int64)
    B = idx.size
    n_p_on = store.n_p_on[idx].tolist()
    beats, rows, unsups, thetas = [], [], [], []
    for j in range(B):
        beats.append(rng.sample(range(n_p_on[j] - 1), 1)[0])
        if jitter > 0:
            thetas.append(LEAD_THETA + jitter_rng.normal(scale=jitter / 180 * np.pi, size=LEAD_THETA.shape))
        sel, sup, unsup, keep = _lead_plan(lead_num, super_mode, data_mode, rng=rng)
        rest = list(sup) if keep else [x for x in sup if x not in sel]
        target = rng.sample(rest, 1)[0]
        rows.append(list(sel) + [target] + rest + list(unsup))           # unsupervised leads last
        unsups.append(list(unsup))
    V = len(sel)
    leads = np.array(rows, dtype=np.int64)
    R = leads.shape[1] - V - 1
    beats = np.array(beats, dtype=np.int64)
    marks = [store.labels[k][store.label_offsets[k][idx] + beats] for k in range(6)]
    p_on, p_off, r_on, r_off, t_on, t_off = marks
    end = store.labels[0][store.label_offsets[0][idx] + beats + 1]      # always the next P onset: the beat comes from range(n_P_on - 1)
    edges = np.stack([p_on, p_off, r_on, r_off, t_on, t_off, end, BEAT_LEN + p_on], axis=1) - p_on[:, None]
    rois = np.stack([edges[:, :-1], edges[:, 1:]], axis=2)
    table = np.concatenate([np.stack([store.offsets[idx] + p_on, store.lengths[idx], end - p_on], axis=1), leads], axis=1)
    theta = np.stack(thetas) if jitter > 0 else np.broadcast_to(LEAD_THETA, (B,) + LEAD_THETA.shape)
    take = np.arange(B)[:, None]
    return Plan(table=np.ascontiguousarray(table, dtype=np.int64), rois=np.ascontiguousarray(rois, dtype=np.int64),
                input_theta=theta[take, leads[:, :V]].astype(np.float32), target_theta=theta[np.arange(B), leads[:, V]].astype(np.float32),
                rest_theta=theta[take, leads[:, V + 1:]].astype(np.float32), id=[store.names[i] for i in idx.tolist()],
                unsupervision_lead_name=unsups, V=V, R=R, beats=beats)


class RecordingPlan(NamedTuple):
    """What recording_plan returns: `plan` is a Plan of every beat, the tables place its rows in [A, len_i] signals."""
    plan: Plan
    rec: np.ndarray             # int64 [Bt]: the position in `indices` of each row's recording
    stitch: np.ndarray          # int64 [Bt, 4]: index in the output of angle 0 at p_on, the recording's length, n, 1 where row b + 1 continues
    recordings: np.ndarray      # int64 [N, 4]: first row, rows, store.offsets[i], len_i
    out_offsets: np.ndarray     # int64 [N + 1]: recording j owns [out_offsets[j], out_offsets[j + 1]) of the flat output as [A, len]
    A: int


def check_leads(input_leads):
    """1 to 12 distinct integers in 0..11, as a list: ValueError otherwise."""
    leads = list(input_leads)
    if not 1 <= len(leads) <= 12 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 11 for v in leads) \
            or len(set(int(v) for v in leads)) != len(leads):
        raise ValueError(f"input_leads {leads}: 1 to 12 distinct integers in 0..11")
    return [int(v) for v in leads]


def recording_plan(store, indices, input_leads, angles=12):
    """Every beat of the recordings `indices`, in their order and in beat order: no draw, no RNG state touched.  The Plan's rows carry
    `input_leads` as the V input leads, input_leads[0] as the (unused) target, R = 0, LEAD_THETA without jitter and the rois of
    `EcgTianChiInterval.__getitem__` for that beat; the tables lay the beats out in one flat output of [angles, len_i] signals per
    recording (recording.synthesize; ops.beat_stitch, ops.recording_stats)."""
    leads = check_leads(input_leads)
    if isinstance(angles, bool) or not isinstance(angles, (int, np.integer)) or angles < 1:
        raise ValueError(f"angles must be an integer >= 1, got {angles!r}")
    idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
    if idx.size < 1 or np.any(idx < 0) or np.any(idx >= len(store)):
        raise ValueError(f"indices {idx.tolist()[:8]}...: at least one recording, each in 0..{len(store) - 1}")
    A, V = int(angles), len(leads)
    counts = store.n_p_on[idx] - 1
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rec = np.repeat(np.arange(idx.size, dtype=np.int64), counts)
    beats = np.arange(first[-1], dtype=np.int64) - first[rec]
    of = idx[rec]
    marks = [store.labels[k][store.label_offsets[k][of] + beats] for k in range(6)]
    p_on = marks[0]
    end = store.labels[0][store.label_offsets[0][of] + beats + 1]
    edges = np.stack(marks + [end, BEAT_LEN + p_on], axis=1) - p_on[:, None]
    rois = np.stack([edges[:, :-1], edges[:, 1:]], axis=2)
    Bt = rec.size
    row = np.array(leads + [leads[0]], dtype=np.int64)
    table = np.concatenate([np.stack([store.offsets[of] + p_on, store.lengths[of], end - p_on], axis=1), np.broadcast_to(row, (Bt, V + 1))], axis=1)
    out_offsets = np.concatenate([[0], np.cumsum(A * store.lengths[idx])]).astype(np.int64)
    link = np.zeros(Bt, dtype=np.int64)
    link[:-1] = rec[1:] == rec[:-1]
    stitch = np.stack([out_offsets[rec] + p_on, store.lengths[of], end - p_on, link], axis=1)
    recordings = np.stack([first[:-1], counts, store.offsets[idx], store.lengths[idx]], axis=1)
    plan = Plan(table=np.ascontiguousarray(table, dtype=np.int64), rois=np.ascontiguousarray(rois, dtype=np.int64),
                input_theta=np.ascontiguousarray(np.broadcast_to(LEAD_THETA[leads], (Bt, V, 2)), dtype=np.float32),
                target_theta=np.ascontiguousarray(np.broadcast_to(LEAD_THETA[leads[0]], (Bt, 2)), dtype=np.float32),
                rest_theta=np.zeros((Bt, 0, 2), dtype=np.float32), id=[store.names[i] for i in of.tolist()],
                unsupervision_lead_name=[[] for _ in range(Bt)], V=V, R=0, beats=beats)
    return RecordingPlan(plan=plan, rec=rec, stitch=np.ascontiguousarray(stitch, dtype=np.int64),
                         recordings=np.ascontiguousarray(recordings, dtype=np.int64), out_offsets=out_offsets, A=A)


class _EpochSampler:
    """The `.sampler` the Solver pokes once per epoch."""

    def __init__(self):
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)


def _align16(n):
    return (n + 15) // 16 * 16


def stage_to_device(parts, dev):
    """int64 / float32 / float64 numpy arrays -> device tensors of their shapes through one pinned staging buffer and one copy on the current
    stream; every part starts 16-byte aligned."""
    kinds = {np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
    starts, total = [], 0
    for a in parts:
        starts.append(total)
        total = _align16(total + a.nbytes)
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    host = stage.numpy()
    for a, s in zip(parts, starts):
        host[s:s + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = stage.to(dev, non_blocking=True)
    return [buf[s:s + a.nbytes].view(kinds[a.dtype]).view(a.shape) for a, s in zip(parts, starts)]


class ResidentLoader:
    """Iterable of `meta` dicts on `store`'s device: data, rois, input_theta, target_view, target_theta, rest_theta in the dtypes of the
    collated host batch, rest_view float32 (always carried), noise zeros [B, 512], id and unsupervision_lead_name as host lists.

    Train phase: the epoch's order is a permutation of the list drawn from (seed, epoch); of its first (N // world) * world entries rank r
    takes every world-th from r (the shards are disjoint).  Test phase: the list in order, whole, on every rank.  `batch_size` is this
    rank's; a short last batch is dropped, as the DataLoaders do.  Batch i's draws come from a private random.Random seeded by
    (seed, epoch, rank, i) -- and a numpy Generator of the same four for MODEL.jitter_factor -- so neither Python's nor numpy's global state
    is touched and an epoch entered after a resume repeats the uninterrupted one.  Every batch gets fresh tensors; the one launch and the
    one copy of the plan go on the current stream."""

    def __init__(self, store, cfg, phase, batch_size, seed=0, rank=0, world=1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"batch_size {batch_size}, rank {rank}, world {world}")
        self.store, self.cfg, self.phase, self.batch_size = store, cfg, phase, int(batch_size)
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.sampler = _EpochSampler()

    def __len__(self):
        return (len(self.store) // self.world) // self.batch_size

    def order(self, epoch=None):
        """This rank's recording indices of the epoch, before they are cut into batches."""
        epoch = self.sampler.epoch if epoch is None else int(epoch)
        idx = list(range(len(self.store)))
        if self.phase == 'train':
            random.Random(f"nef-resident-order:{self.seed}:{epoch}").shuffle(idx)
        return idx[:(len(idx) // self.world) * self.world][self.rank::self.world]

    def plans(self, epoch=None):
        """(batch index, recording indices, Plan) of every batch of the epoch: the host half of the loader, no device needed."""
        epoch = self.sampler.epoch if epoch is None else int(epoch)
        idx, B = self.order(epoch), self.batch_size
        jitter = self.phase == 'train' and float(self.cfg.MODEL.jitter_factor) > 0
        for i in range(len(idx) // B):
            rng = random.Random(f"nef-resident-batch:{self.seed}:{epoch}:{self.rank}:{i}")
            jrng = np.random.default_rng([abs(self.seed), epoch, self.rank, i]) if jitter else None
            batch = idx[i * B:(i + 1) * B]
            yield i, batch, draw_plan(self.store, batch, self.cfg, self.phase, rng, jrng)

    def __iter__(self):
        from .. import ops
        dev = self.store.signal.device
        for _, _, plan in self.plans():
            yield self._build(ops, dev, plan)

    def _build(self, ops, dev, plan):
        B, V, R = plan.table.shape[0], plan.V, plan.R
        table, rois, in_th, tg_th, rs_th = stage_to_device((plan.table, plan.rois, plan.input_theta, plan.target_theta, plan.rest_theta), dev)
        data, target, rest = ops.beat_batch(self.store.signal, table, V, R)
        return {'data': data, 'rois': rois, 'input_theta': in_th, 'target_view': target, 'target_theta': tg_th, 'rest_view': rest,
                'rest_theta': rs_th, 'noise': torch.zeros((B, BEAT_LEN), dtype=torch.float32, device=dev), 'id': plan.id,
                'unsupervision_lead_name': plan.unsupervision_lead_name}


def build_loader(cfg, phase, batch_size, device, rank=0, world=1):
    """The ResidentLoader of `phase` as train_net.build_loaders hands it out: `batch_size` is this rank's share; only the train phase is
    sharded and shuffled.  DATA.auto_marks: the store marks its recordings itself (ResidentTianchi)."""
    check_cfg(cfg)
    store = ResidentTianchi(cfg, phase, device)
    if phase == 'train':
        return ResidentLoader(store, cfg, phase, batch_size, seed=cfg.seed, rank=rank, world=world)
    return ResidentLoader(store, cfg, phase, batch_size, seed=cfg.seed)
