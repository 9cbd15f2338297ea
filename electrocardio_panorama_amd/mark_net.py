"""`python -m electrocardio_panorama_amd.mark_net --config-file F (--fit TABLE.json [--form ratio|affine] | --compare TABLE.json |
--write DIR TABLE.json | --resample DIR | --clean DIR [--phase test])` -- no counterpart in the reference, whose label lists come from an annotation tool: make the six
'P on' .. 'T off' lists of recordings from their signals (dataset/marks.py).

--fit      detect the QRS complexes of the annotated train list on the device (the detector's windows follow DATA.sample_rate) and fit the
           timing table on its annotated beats; writes TABLE.json.
--compare  mark the annotated test list with TABLE.json and print, per mark, the mean, median and largest absolute difference to the
           annotator in samples, and the share of annotated beats that were matched.
--write    mark the phase's recordings from their signals alone and write `<id>.json` in the reference's six-key format into DIR, so the
           host loader -- and the reference itself -- can train on them (DATA.train_label_root = DIR).
--resample with DATA.source_rate: resample the phase's recordings to DATA.sample_rate on the device (resample.py) and write
           each as `<id>.npy`, float32 [8, len'], into DIR; for an annotated list also `<id>.json` with the rescaled marks in the
           six-key format, so the host loader -- and the reference itself -- train on what the device path sees (DATA.train_data_root =
           DATA.train_label_root = DIR, DATA.source_rate 0).  With DATA.auto_marks the marks written are the detector's.
--clean    with DATA.baseline_ms / DATA.mains_hz: clean the phase's recordings on the device (clean.py) -- behind the
           resampling when DATA.source_rate is on -- and write them and their marks in the format of --resample, for the host loader and
           the reference (DATA.baseline_ms [], DATA.mains_hz 0 and DATA.source_rate 0 there).  An error with both cleaning keys off.

One rank only."""
import argparse
import json
import os

import numpy as np
import torch

from .clean import clean_plan
from .config import cfg, resolve_config_path
from .dataset import marks
from .dataset.resident import ResidentTianchi


def _one_rank(cfg):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                                      and torch.distributed.get_world_size() > 1):
        raise NotImplementedError("mark_net runs on one rank: the recordings are not sharded")
    if cfg.DATA.get('dataset', 'tianchi') != 'tianchi':
        raise ValueError(f"mark_net marks Tianchi recordings; DATA.dataset {cfg.DATA.dataset!r} is not kept on the device")


def fit(cfg, table_path, form='ratio', device='cuda:0'):
    """Fit the timing table on the annotated train list and write it; returns the marks.Fit."""
    _one_rank(cfg)
    params = marks.MarkParams.from_rate(cfg.DATA.get('sample_rate', 500.0))
    store = ResidentTianchi(cfg, 'train', torch.device(device))
    got = marks.fit_table(store, marks.detect(store, params=params), form=form)
    marks.save_table(table_path, got.table, form=form, params=params)
    print('fit {}: {} of {} annotated beats matched, table {}'.format(form, got.matched, got.matched + got.left_out,
                                                                      np.round(got.table, 4).tolist()))
    return got


def compare(cfg, table_path, device='cuda:0'):
    """Mark the annotated test list with the table and print marks.compare's rows; returns its dict."""
    _one_rank(cfg)
    table, _, params = marks.load_table(table_path)
    store = ResidentTianchi(cfg, 'test', torch.device(device))
    found = marks.detect(store, params=params)
    rows = marks.compare(store, marks.labels_from_peaks(found.peaks, found.count, store.lengths, table))
    print('matched {} of {} annotated beats ({:.4f})'.format(rows['matched'], rows['beats'], rows['share']))
    for key in marks.LABEL_KEYS:
        if rows[key] is not None:
            print('{:6s} mean {:.3f} median {:.1f} max {}'.format(key, rows[key]['mean'], rows[key]['median'], rows[key]['max']))
    return rows


def write(cfg, out_dir, table_path, phase='test', device='cuda:0'):
    """Write `<id>.json` with the six lists of every marked recording of the phase's list; returns the store's auto_report."""
    _one_rank(cfg)
    store = ResidentTianchi(cfg, phase, torch.device(device), marks=table_path)
    os.makedirs(out_dir, exist_ok=True)
    for i, name in enumerate(store.names):
        doc = {key: store.labels[k][store.label_offsets[k][i]:store.label_offsets[k][i + 1]].tolist() for k, key in enumerate(marks.LABEL_KEYS)}
        stem = name[:-len('.json')] if name.endswith('.json') else name
        with open(os.path.join(out_dir, stem + '.json'), 'w') as f:
            json.dump(doc, f)
    print('wrote {marked} of {recordings} recordings: {dropped} of {peaks} peaks dropped, {adjusted} marks adjusted'.format(**store.auto_report))
    return store.auto_report


def _write_store(store, out_dir):
    """Every recording of the store as `<id>.npy`, float32 [8, len], and `<id>.json` with its six lists."""
    os.makedirs(out_dir, exist_ok=True)
    signal = store.signal.cpu().numpy()
    for i, name in enumerate(store.names):
        stem = name[:-len('.json')] if name.endswith('.json') else name
        np.save(os.path.join(out_dir, stem + '.npy'), signal[store.offsets[i]:store.offsets[i + 1]].reshape(8, -1))
        doc = {key: store.labels[k][store.label_offsets[k][i]:store.label_offsets[k][i + 1]].tolist() for k, key in enumerate(marks.LABEL_KEYS)}
        with open(os.path.join(out_dir, stem + '.json'), 'w') as f:
            json.dump(doc, f)


def resample_to(cfg, out_dir, phase='test', device='cuda:0'):
    """Write the phase's recordings at DATA.sample_rate, and their marks, into out_dir; returns the store's resample_report."""
    _one_rank(cfg)
    store = ResidentTianchi(cfg, phase, torch.device(device))
    if store.source is None:
        raise ValueError("mark_net --resample: DATA.source_rate is off (0, or DATA.sample_rate itself); there is nothing to resample")
    _write_store(store, out_dir)
    print('resampled {recordings} recordings from {source_rate} Hz to {sample_rate} Hz ({up}/{down}, {taps} taps a phase), {adjusted} marks '
          'adjusted'.format(**store.resample_report))
    return store.resample_report


def clean_to(cfg, out_dir, phase='test', device='cuda:0'):
    """Write the phase's cleaned recordings (resampled first with DATA.source_rate), and their marks, into out_dir; returns the store's
    clean_report."""
    _one_rank(cfg)
    if clean_plan(cfg, need_resident=False) is None:
        raise ValueError("mark_net --clean: DATA.baseline_ms is [] and DATA.mains_hz is 0; there is nothing to clean")
    store = ResidentTianchi(cfg, phase, torch.device(device))
    _write_store(store, out_dir)
    print('cleaned {recordings} recordings: median half widths {h1} and {h2}, {taps} notch taps, {launches} launches'.format(**store.clean_report))
    return store.clean_report


def run(argv=None):
    parser = argparse.ArgumentParser(description='marks for unannotated ecg recordings')
    parser.add_argument('--config-file', default="", metavar="FILE", help="path to config file", type=str)
    what = parser.add_mutually_exclusive_group(required=True)
    what.add_argument('--fit', metavar="TABLE.json", help="fit the timing table on the annotated train list")
    what.add_argument('--compare', metavar="TABLE.json", help="compare the table's marks with the annotated test list")
    what.add_argument('--write', nargs=2, metavar=("DIR", "TABLE.json"), help="write <id>.json label files for the phase's recordings")
    what.add_argument('--resample', metavar="DIR", help="with DATA.source_rate: write the recordings at DATA.sample_rate, and their marks")
    what.add_argument('--clean', metavar="DIR", help="with DATA.baseline_ms / DATA.mains_hz: write the cleaned recordings, and their marks")
    parser.add_argument('--form', default='ratio', choices=marks.FORMS)
    parser.add_argument('--phase', default='test', choices=('train', 'test'))
    parser.add_argument('opts', nargs=argparse.REMAINDER, help="KEY VALUE overrides")
    args = parser.parse_args(argv)
    if args.config_file != '':
        cfg.merge_from_file(resolve_config_path(args.config_file))
    if args.opts:
        cfg.merge_from_list(args.opts)
    if args.fit:
        return fit(cfg, args.fit, form=args.form)
    if args.compare:
        return compare(cfg, args.compare)
    if args.resample:
        return resample_to(cfg, args.resample, phase=args.phase)
    if args.clean:
        return clean_to(cfg, args.clean, phase=args.phase)
    return write(cfg, args.write[0], args.write[1], phase=args.phase)


if __name__ == '__main__':
    run()
