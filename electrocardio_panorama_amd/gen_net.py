"""`python -m electrocardio_panorama_amd.gen_net --config-file config/nef_net.yml [--epoch N] [--leads I ...] [--fill bridge] [--out DIR]
[--phase test] [--auto-marks TABLE.json] [--native-rate]` -- no counterpart in the reference: synthesise every recording of the phase's label list as a
whole 12-lead strip on its own time axis and in its own units (recording.synthesize) from the leads the model takes as inputs, and print RMSE and correlation per
recording and lead, averaged: rec_rmse_reg / rec_corr_reg over the input leads, rec_rmse_gen / rec_corr_gen over the others.  The
checkpoint is `best_valid.pkl` (or `epoch_N.pkl`), with the averaged weights under SOLVER.ema_eval as Solver.val takes them.  `--out`
writes `<id>.npy` ([12, len] float32) per recording and one `metrics.json`.  Without `--leads` the input leads are those of the
configured lead scheme; the random 3-lead mode has no fixed ones and asks for `--leads`.  `--auto-marks TABLE.json` builds the store from
the signals alone: the beats are marked on the device with that timing table (dataset/marks.py), no label file is read.
`--native-rate`: with DATA.source_rate the store holds the recordings resampled to DATA.sample_rate; `--out` then writes each strip back on
the time axis its recording came with, [12, raw_len] (recording.to_native_rate).  The metrics stay those of the model's rate."""
import argparse
import json
import os
import random

import numpy as np
import torch

from . import recording
from .config import cfg, resolve_config_path
from .dataset.resident import ResidentTianchi
from .dataset.tianchi import _lead_plan
from .solver import Solver
from .utils import CheckPointer, seed_torch

RECORDINGS_PER_CALL = 256       # recordings synthesised (and, with --out, held on the host) at a time


def scheme_leads(cfg):
    """The input leads of the configured scheme when it draws none of them: ValueError for the random 3-lead mode."""
    if cfg.DATA.lead_num == 3 and cfg.DATA.train_data_mode != 'input_fix':
        raise ValueError("DATA.lead_num 3 without train_data_mode 'input_fix' draws its input leads per sample: name them with --leads")
    return list(_lead_plan(cfg.DATA.lead_num, cfg.DATA.super_mode, cfg.DATA.train_data_mode, rng=random.Random(0))[0])


def _mean(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.mean(a)) if a.size else float('nan')


def main(cfg, epoch=-1, leads=None, fill='nan', out_dir=None, phase='test', beats_per_pass=256, auto_marks=None, native_rate=False):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                                      and torch.distributed.get_world_size() > 1):
        raise NotImplementedError("gen_net runs on one rank: the recordings are not sharded")
    if cfg.DATA.get('dataset', 'tianchi') != 'tianchi':
        raise ValueError(f"gen_net synthesises Tianchi recordings; DATA.dataset {cfg.DATA.dataset!r} is not kept on the device")
    leads = scheme_leads(cfg) if not leads else [int(v) for v in leads]
    seed_torch(seed=cfg.seed)
    solver = Solver(cfg, use_tensorboardx=False)
    if len(leads) != solver.model.lead_num:
        raise ValueError(f"{len(leads)} input leads {leads} for a model of DATA.lead_num {solver.model.lead_num}")
    ema = solver._ema_eval()
    ckpt = CheckPointer(solver.model, save_dir=solver.output_dir)
    extra = ckpt.load(best_valid=True, ema=ema) if epoch == -1 else \
        ckpt.load(os.path.join(solver.output_dir, 'epoch_{}.pkl'.format(epoch)), ema=ema)
    print('the latest best_test_psnr_gen is {:06f} of epoch {}'.format(extra.get('best_test_psnr_gen', 0.), extra.get('epoch', 0)))
    store = ResidentTianchi(cfg, phase, solver.device, marks=auto_marks)       # None: annotated, or marked as DATA.auto_marks says
    if store.auto_report is not None:
        print('auto marks: {marked} of {recordings} recordings marked, {dropped} of {peaks} peaks dropped, {adjusted} marks adjusted'.format(
            **store.auto_report))
    if store.resample_report is not None:
        print('resampled {recordings} recordings from {source_rate} Hz to {sample_rate} Hz ({up}/{down}, {taps} taps a phase), {adjusted} marks '
              'adjusted'.format(**store.resample_report))
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    rmse, corr = [], []
    for i0 in range(0, len(store), RECORDINGS_PER_CALL):
        idx = range(i0, min(i0 + RECORDINGS_PER_CALL, len(store)))
        syn = recording.synthesize(solver.model, store, idx, leads, fill=fill, beats_per_pass=beats_per_pass,
                                   native_rate=bool(native_rate and out_dir))
        rmse.append(syn.rmse)
        corr.append(syn.corr)
        if out_dir:
            for i, sig in zip(idx, syn.native_signals if native_rate else syn.signals):
                np.save(os.path.join(out_dir, os.path.splitext(os.path.basename(store.names[i]))[0] + '.npy'), sig.cpu().numpy())
    rmse, corr = np.concatenate(rmse), np.concatenate(corr)            # [N, 12]
    rest = [k for k in range(12) if k not in leads]
    result = {'rec_rmse_reg': _mean(rmse[:, leads]), 'rec_corr_reg': _mean(corr[:, leads]),
              'rec_rmse_gen': _mean(rmse[:, rest]), 'rec_corr_gen': _mean(corr[:, rest])}
    print('rec_rmse_reg:{}, rec_corr_reg:{}, rec_rmse_gen:{}, rec_corr_gen:{}'.format(
        result['rec_rmse_reg'], result['rec_corr_reg'], result['rec_rmse_gen'], result['rec_corr_gen']))
    if out_dir:
        doc = dict(result, phase=phase, fill=fill, input_leads=leads, native_rate=bool(native_rate), source_rate=store.source_rate, ids=list(store.names), rmse=rmse.tolist(), corr=corr.tolist())
        with open(os.path.join(out_dir, 'metrics.json'), 'w') as f:
            json.dump(doc, f)
    return result


def run(argv=None):
    parser = argparse.ArgumentParser(description='whole-recording ecg synthesis')
    parser.add_argument('--config-file', default="", metavar="FILE", help="path to config file", type=str)
    parser.add_argument('--epoch', default=-1, type=int)
    parser.add_argument('--leads', nargs='+', type=int, default=None, help="the input leads (0..11), in the order the model takes them")
    parser.add_argument('--fill', default='nan', choices=('nan', 'bridge'), help="positions of a beat behind its 512-sample row")
    parser.add_argument('--out', default=None, metavar="DIR", help="write <id>.npy per recording and metrics.json here")
    parser.add_argument('--phase', default='test', choices=('train', 'test'))
    parser.add_argument('--auto-marks', default=None, metavar="TABLE.json", help="mark the recordings on the device with this timing table")
    parser.add_argument('--native-rate', action='store_true', help="with DATA.source_rate: write the strips at the recordings' own rate")
    parser.add_argument('opts', nargs=argparse.REMAINDER, help="KEY VALUE overrides")
    args = parser.parse_args(argv)
    if args.config_file != '':
        cfg.merge_from_file(resolve_config_path(args.config_file))
    if args.opts:
        cfg.merge_from_list(args.opts)
    cfg.desc = args.config_file.split('/')[-1].replace('.yml', '') or cfg.desc
    cfg.output_dir = os.path.join(cfg.output_dir, cfg.desc)
    return main(cfg, epoch=args.epoch, leads=args.leads, fill=args.fill, out_dir=args.out, phase=args.phase, auto_marks=args.auto_marks,
                native_rate=args.native_rate)


if __name__ == '__main__':
    run()
