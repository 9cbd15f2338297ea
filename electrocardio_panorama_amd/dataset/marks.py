"""Marks for unannotated recordings: the six label lists of a resident store made from its signals alone (cfg.DATA.auto_marks).

Every path of the project reads six hand-made index lists per recording -- 'P on' .. 'T off'.  Here they are made in two steps.  `detect`
finds the QRS complexes on the device, over the store's own copy of the recordings: nef_mark_envelope (ops.mark_envelope) sums the squared
central differences of the leads over a short window, nef_mark_peaks (ops.mark_peaks) keeps the positions that are the highest within r
samples and reach a fraction of the recording's level -- non-maximum suppression, no running threshold, so a recording's peaks are a
function of that recording alone.  `labels_from_peaks` then places the six marks of every beat at fixed fractions of the RR interval around
its peak, from a [6, 2] timing table that `fit_table` fits on an annotated store; it is host numpy, a few milliseconds.  The lists come out
in `ResidentTianchi`'s own format, so draw_plan, recording_plan, ResidentLoader and recording.synthesize run on them unchanged.

What a timing table cannot do: mark a rhythm whose waves do not keep their place in the RR interval.  `compare` is the read-out."""
import json
from typing import NamedTuple

import numpy as np
import torch

from ..resample import increasing

LABEL_KEYS = ('P on', 'P off', 'R on', 'R off', 'T on', 'T off')
FORMS = ('ratio', 'affine')
MAX_ROWS = 65535          # recordings a launch (ops.MARK_MAX_ROWS)


class MarkParams(NamedTuple):
    """The detector's parameters, in samples (the defaults are `from_rate(500)`)."""
    D: int = 2                  # half step of the central difference
    H: int = 20                 # half window of the envelope
    r: int = 100                # suppression radius: a peak is the highest within r samples
    seg: int = 1000             # segment whose maxima give the level
    frac: float = 0.125         # a peak reaches level * frac
    lead_bits: int = 255        # bit c: stored lead c takes part
    max_peaks: int = 256        # peaks kept per recording; one with more has no labels

    @classmethod
    def from_rate(cls, sample_rate, **kw):
        """4 ms, 40 ms, 200 ms and 2 s at `sample_rate` Hz, each at least one sample."""
        rate = float(sample_rate)
        if not rate > 0 or rate != rate or rate == float('inf'):
            raise ValueError(f"sample_rate {sample_rate!r}: a positive finite number of Hz")
        n = lambda sec: max(1, int(round(sec * rate)))
        return cls(D=n(0.004), H=n(0.04), r=n(0.2), seg=n(2.0), **kw)


class Peaks(NamedTuple):
    """What detect returns, host numpy, one row per recording of `indices`."""
    peaks: np.ndarray           # int32 [N, max_peaks]: ascending, -1 behind the count
    count: np.ndarray           # int32 [N]: the true number, also above max_peaks; -1: the envelope was not finite
    level: np.ndarray           # float64 [N]


class Labels(NamedTuple):
    """What labels_from_peaks returns: `labels` / `label_offsets` as ResidentTianchi keeps them."""
    labels: list                # six int64 arrays, each concatenated over the recordings
    label_offsets: list         # six int64 [N + 1]
    dropped: np.ndarray         # int64 [N]: peaks that did not become a labelled beat
    adjusted: np.ndarray        # int64 [N]: marks the strictly-increasing fix-up moved


class Fit(NamedTuple):
    table: np.ndarray           # float64 [6, 2]: (a_k, b_k)
    form: str
    matched: int                # annotated beats with exactly one peak in [R on, R off]
    left_out: int               # the others


def _chunks(lengths, budget):
    """Consecutive runs of recordings of at most `budget` samples and MAX_ROWS rows each (a longer recording stands alone)."""
    out, start, total = [], 0, 0
    for i, n in enumerate(lengths):
        if i > start and (total + n > budget or i - start >= MAX_ROWS):
            out.append((start, i))
            start, total = i, 0
        total += n
    out.append((start, len(lengths)))
    return out


def detect(store, indices=None, params=MarkParams(), budget=1 << 25):
    """The peaks of the recordings `indices` (all, in order, by default) of a resident store on a HIP device.  The recordings are cut into
    chunks of at most `budget` samples that share one fp64 envelope buffer; both launches run per chunk on the current stream, and one copy
    of peaks, count and level goes to the host at the end."""
    from .. import ops
    if not isinstance(params, MarkParams):
        raise TypeError(f"params must be a MarkParams, got {type(params)}")
    if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)) or budget < 1:
        raise ValueError(f"budget {budget!r}: a positive number of samples")
    idx = np.arange(len(store), dtype=np.int64) if indices is None else np.asarray(list(indices), dtype=np.int64).reshape(-1)
    if idx.size < 1 or np.any(idx < 0) or np.any(idx >= len(store)):
        raise ValueError(f"indices {idx.tolist()[:8]}...: at least one recording, each in 0..{len(store) - 1}")
    if not store.signal.is_cuda:
        raise RuntimeError("marks.detect runs on a HIP device only: build the store on one (no CPU path)")
    lengths, offsets = store.lengths[idx], store.offsets[idx]
    chunks = _chunks(lengths.tolist(), int(budget))
    env = torch.empty(max(int(lengths[a:b].sum()) for a, b in chunks), dtype=torch.float64, device=store.signal.device)
    parts = []
    for a, b in chunks:
        ln = lengths[a:b]
        eoff = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
        table = torch.from_numpy(np.ascontiguousarray(np.stack([offsets[a:b], ln, eoff], axis=1), dtype=np.int64))
        ops.mark_envelope(store.signal, table, env, D=params.D, H=params.H, lead_bits=params.lead_bits)
        parts.append(ops.mark_peaks(env, table, r=params.r, seg=params.seg, frac=params.frac, max_peaks=params.max_peaks))
    peaks, count, level = (torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in range(3))
    return Peaks(peaks.cpu().numpy(), count.cpu().numpy(), level.cpu().numpy())


def _check_table(table):
    t = np.asarray(table, dtype=np.float64)
    if t.shape != (6, 2) or not np.all(np.isfinite(t)):
        raise ValueError(f"table {t.shape}: six finite (a_k, b_k) rows, one per mark")
    return t


def _beat_rr(p, first, last):
    """RR_prev and RR_next of flat peaks `p`; `first` / `last` flag a recording's first / last peak (each recording holds two or more)."""
    d = np.diff(p)
    nxt, prv = np.empty_like(p), np.empty_like(p)
    nxt[:-1], prv[1:] = d, d
    nxt[last] = p[last] - p[np.flatnonzero(last) - 1]
    prv[first] = p[np.flatnonzero(first) + 1] - p[first]
    return prv, nxt


def labels_from_peaks(peaks, count, lengths, table):
    """The six label lists of every recording from its peaks, vectorised over all beats.  For the peaks p_0 .. p_{P-1} of a recording,
    mark[j, k] = p[j] + floor(a_k + b_k * RR + 0.5), RR the interval to the previous peak for 'P on' / 'P off' and to the next one for the
    other four (the first peak has no previous and takes its next, the last the reverse).  Dropped: every beat up to the last one whose
    'P on' is negative and from the first one whose 'T off' lies behind len - 1.  The marks of the beats left, in time order, are then made
    strictly increasing by m_i = max(m_i, m_{i-1} + 1) -- a changed mark counts as adjusted -- and trailing beats are dropped until the end
    fits.  The last beat left is not drawable: as in the annotated lists, its 'P on' closes the beat before it.  A recording with fewer
    than two peaks, a count of -1 or above max_peaks, or fewer than two beats left has no labels."""
    table = _check_table(table)
    peaks, count, lengths = np.asarray(peaks), np.asarray(count).astype(np.int64), np.asarray(lengths).astype(np.int64)
    if peaks.ndim != 2 or count.shape != (peaks.shape[0],) or lengths.shape != count.shape:
        raise ValueError(f"peaks {peaks.shape}, count {count.shape}, lengths {lengths.shape}: [N, max_peaks], [N], [N]")
    N, max_peaks = peaks.shape
    P = np.where((count >= 2) & (count <= max_peaks), count, 0)
    nb = np.zeros(N, dtype=np.int64)
    adjusted = np.zeros(N, dtype=np.int64)
    marks = np.zeros((0, 6), dtype=np.int64)
    keep_rec = np.zeros(0, dtype=np.int64)
    M = int(P.sum())
    if M:
        rec = np.repeat(np.arange(N, dtype=np.int64), P)
        start = np.concatenate([[0], np.cumsum(P)[:-1]])
        j = np.arange(M, dtype=np.int64) - start[rec]
        p = peaks[rec, j].astype(np.int64)
        prv, nxt = _beat_rr(p, j == 0, j == P[rec] - 1)
        rr = np.stack([prv, prv, nxt, nxt, nxt, nxt], axis=1).astype(np.float64)
        m = p[:, None] + np.floor(table[None, :, 0] + table[None, :, 1] * rr + 0.5).astype(np.int64)
        # beats up to the last negative 'P on', and from the first 'T off' behind the end
        lo = np.zeros(N, dtype=np.int64)
        np.maximum.at(lo, rec, np.where(m[:, 0] < 0, j + 1, 0))
        hi = P.copy()
        np.minimum.at(hi, rec, np.where(m[:, 5] > lengths[rec] - 1, j, max_peaks))
        keep = (j >= lo[rec]) & (j < hi[rec])
        m, rec = m[keep], rec[keep]
        # strictly increasing within a recording (resample.increasing: the fix-up rescaled label lists get too)
        fixed, changed = increasing(m.reshape(-1), np.repeat(rec, 6))
        changed = changed.reshape(-1, 6)
        m = fixed.reshape(-1, 6)
        keep = m[:, 5] <= lengths[rec] - 1                      # increasing: what does not fit is a recording's tail
        m, rec, changed = m[keep], rec[keep], changed[keep]
        nb = np.bincount(rec, minlength=N).astype(np.int64)
        keep = nb[rec] >= 2
        m, rec, changed = m[keep], rec[keep], changed[keep]
        nb[nb < 2] = 0
        adjusted = np.bincount(rec, weights=changed.sum(axis=1), minlength=N).astype(np.int64)
        marks, keep_rec = m, rec
    offsets = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    return Labels(labels=[np.ascontiguousarray(marks[:, k]) for k in range(6)], label_offsets=[offsets.copy() for _ in range(6)],
                  dropped=np.maximum(count, 0) - nb, adjusted=adjusted)


def _matched(store, peaks):
    """(mark - p [M, 6], RR_prev [M], RR_next [M], annotated beats, matched) over the annotated beats of `store` with exactly one peak in
    [R on, R off]; a recording whose count is not in 2..max_peaks matches nothing."""
    ys, prvs, nxts, beats = [], [], [], 0
    for i in range(len(store)):
        lab = [store.labels[k][store.label_offsets[k][i]:store.label_offsets[k][i + 1]] for k in range(6)]
        n = min(v.size for v in lab)
        beats += n
        c = int(peaks.count[i])
        if n < 1 or not 2 <= c <= peaks.peaks.shape[1]:
            continue
        p = peaks.peaks[i, :c].astype(np.int64)
        prv, nxt = _beat_rr(p, np.arange(c) == 0, np.arange(c) == c - 1)
        a, b = np.searchsorted(p, lab[2][:n], side='left'), np.searchsorted(p, lab[3][:n], side='right')
        one = np.flatnonzero(b - a == 1)
        jj = a[one]
        ys.append(np.stack([lab[k][one] for k in range(6)], axis=1) - p[jj][:, None])
        prvs.append(prv[jj])
        nxts.append(nxt[jj])
    if not ys:
        return np.zeros((0, 6), dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), beats, 0
    y = np.concatenate(ys)
    return y, np.concatenate(prvs), np.concatenate(nxts), beats, y.shape[0]


def fit_table(store, peaks, form='ratio'):
    """The timing table of an annotated store: for each mark, y = mark - p is fitted against its RR by least squares in fp64 over the
    annotated beats with exactly one peak in [R on, R off].  'ratio': a = 0, b = sum(RR y) / sum(RR^2); 'affine': both coefficients
    (ValueError when the matched RR values are all equal)."""
    if form not in FORMS:
        raise ValueError(f"form {form!r}: one of {FORMS}")
    y, prv, nxt, beats, matched = _matched(store, peaks)
    if matched < 1:
        raise ValueError(f"no annotated beat of the {len(store)} recordings has exactly one peak in [R on, R off]: nothing to fit")
    table = np.zeros((6, 2), dtype=np.float64)
    for k in range(6):
        rr = (prv if k < 2 else nxt).astype(np.float64)
        yk = y[:, k].astype(np.float64)
        if form == 'ratio':
            table[k, 1] = np.sum(rr * yk) / np.sum(rr * rr)
        else:
            if np.all(rr == rr[0]):
                raise ValueError("form 'affine': the matched RR intervals are all equal, the two coefficients are not determined")
            mr, my = rr.mean(), yk.mean()
            table[k, 1] = np.sum((rr - mr) * (yk - my)) / np.sum((rr - mr) ** 2)
            table[k, 0] = my - table[k, 1] * mr
    return Fit(table=table, form=form, matched=matched, left_out=beats - matched)


def compare(store_annotated, auto_labels):
    """Auto labels against an annotated store of the same recordings: an annotated beat is matched to an auto beat iff exactly one auto
    beat's [R on, R off] meets its own.  Per mark the mean, median and largest absolute difference over the matched beats, and the
    matched share of the annotated beats."""
    diffs, beats = [], 0
    for i in range(len(store_annotated)):
        s = store_annotated
        lab = [s.labels[k][s.label_offsets[k][i]:s.label_offsets[k][i + 1]] for k in range(6)]
        aut = [auto_labels.labels[k][auto_labels.label_offsets[k][i]:auto_labels.label_offsets[k][i + 1]] for k in range(6)]
        n, na = min(v.size for v in lab), min(v.size for v in aut)
        beats += n
        if n < 1 or na < 1:
            continue
        a = np.searchsorted(aut[3][:na], lab[2][:n], side='left')          # auto beats whose R off lies in front are out
        b = np.searchsorted(aut[2][:na], lab[3][:n], side='right')         # ... and those whose R on lies behind
        one = np.flatnonzero(b - a == 1)
        diffs.append(np.abs(np.stack([lab[k][one] - aut[k][a[one]] for k in range(6)], axis=1)))
    d = np.concatenate(diffs) if diffs else np.zeros((0, 6), dtype=np.int64)
    out = {'matched': d.shape[0], 'beats': beats, 'share': d.shape[0] / beats if beats else 0.0}
    for k, key in enumerate(LABEL_KEYS):
        out[key] = {'mean': float(d[:, k].mean()), 'median': float(np.median(d[:, k])), 'max': int(d[:, k].max())} if d.shape[0] else None
    return out


def save_table(path, table, form='ratio', params=MarkParams()):
    """Write the [6, 2] numbers, the form and the detector's parameters as JSON."""
    table = _check_table(table)
    if form not in FORMS:
        raise ValueError(f"form {form!r}: one of {FORMS}")
    with open(path, 'w') as f:
        json.dump({'marks': list(LABEL_KEYS), 'table': table.tolist(), 'form': form, 'params': dict(params._asdict())}, f, indent=1)


def load_table(path):
    """(table float64 [6, 2], form, MarkParams) of a file save_table wrote; ValueError for anything else."""
    with open(path) as f:
        doc = json.load(f)
    try:
        table, form, params = _check_table(doc['table']), doc['form'], MarkParams(**doc['params'])
    except (KeyError, TypeError) as e:
        raise ValueError(f"{path}: not a mark table file ({e})") from None
    if form not in FORMS:
        raise ValueError(f"{path}: form {form!r} is not one of {FORMS}")
    return table, form, params


def check_cfg(cfg):
    """DATA.auto_marks goes with DATA.device_resident and a DATA.mark_table file: ValueError otherwise.  Returns whether the key is on."""
    if not cfg.DATA.get('auto_marks', False):
        return False
    if not cfg.DATA.get('device_resident', False):
        raise ValueError("DATA.auto_marks marks the recordings of the device-resident store: set DATA.device_resident, or write label "
                         "files for the host loader with `python -m electrocardio_panorama_amd.mark_net --write`")
    if not cfg.DATA.get('mark_table', ''):
        raise ValueError("DATA.auto_marks needs DATA.mark_table: the JSON timing table `mark_net --fit` writes")
    return True
