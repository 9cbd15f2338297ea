"""Throughput of whole-recording synthesis (recording.synthesize) on the synthetic tree of tools/bench_loader.py.

Per panorama dtype (fp32, fp16) and per beats_per_pass (256, 1024), in `--rounds` alternating rounds of fresh processes: recordings/s and
beats/s of `synthesize` over all recordings (3 input leads, the 12 angles of LEAD_THETA, scored against the 12 leads); the time of
ops.beat_batch + Model_nefnet.panorama alone on the same chunks in the same process, the two alternating; and the three new launches
alone, each behind a 512 MiB fill (cold), with their algorithmic bytes.  Prints one JSON line of [min, median, max] per figure; the one
condition it judges is `synthesize`'s median time at most 10 % above the median of beat_batch + panorama alone on the same beats.

    python tools/bench_recording.py [--rounds 3] [--n 2048] [--out profiles/r24_recording_bench_line.json]

`--source-rate R` writes the tree at R Hz and builds the store with DATA.source_rate = R (resampled to 500 Hz on the device): every figure
is then taken on the resampled store, and `synthesize(native_rate=True)` -- the strips handed back at R Hz -- is timed beside the plain one.

    python tools/bench_recording.py --source-rate 1000 [--rounds 3] [--n 2048] [--out FILE]

Not measured: real Tianchi at full size, more than one GPU, gen_net's file writing."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np   # noqa: E402
import torch         # noqa: E402

PASSES = (256, 1024)
LEADS = [1, 3, 6]
MARGIN = 1.10


def leg(a):
    from bench_loader import tree_cfg
    from electrocardio_panorama_amd import ops, recording
    from electrocardio_panorama_amd.dataset import resident
    from electrocardio_panorama_amd.network import build_model
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    cfg = tree_cfg(a.tree, len(LEADS))
    cfg.DATA.source_rate = a.source_rate
    torch.manual_seed(1234)
    model = build_model(cfg).float().to(dev).eval()
    model.panorama_dtype = a.leg
    store = resident.ResidentTianchi(cfg, "test", dev)
    idx = range(len(store))
    plan = resident.recording_plan(store, idx, LEADS)
    q = torch.from_numpy(np.asarray(recording.LEAD_THETA, dtype=np.float32)).to(dev)
    out = {"leg": a.leg, "beats": int(plan.rec.size), "beats_longer_than_512": int((plan.stitch[:, 2] > 512).sum())}

    def alone(bpp):
        for r0, r1 in recording.chunks(plan, bpp):
            table, rois, in_th = resident.stage_to_device((plan.plan.table[r0:r1], plan.plan.rois[r0:r1], plan.plan.input_theta[r0:r1]), dev)
            model.panorama(ops.beat_batch(store.signal, table, 3, 0)[0], in_th, rois, q)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with torch.no_grad():
        for bpp in PASSES:
            synth = lambda: recording.synthesize(model, store, idx, LEADS, beats_per_pass=bpp)      # noqa: E731
            timed(lambda: alone(bpp))                    # first launches of this batch shape, untimed
            timed(synth)
            ts, ta = [], []
            for _ in range(a.repeats):
                ta.append(timed(lambda: alone(bpp)))
                ts.append(timed(synth))
            s, al = float(np.median(ts)), float(np.median(ta))
            out[f"synthesize_s_p{bpp}"], out[f"batch_and_panorama_s_p{bpp}"] = round(s, 4), round(al, 4)
            out[f"recordings_per_s_p{bpp}"], out[f"beats_per_s_p{bpp}"] = round(len(store) / s, 1), round(plan.rec.size / s, 1)
            out[f"synthesize_over_alone_p{bpp}"] = round(s / al, 4)
            if store.source is not None:                 # the strips also handed back at the source rate
                native = lambda: recording.synthesize(model, store, idx, LEADS, beats_per_pass=bpp, native_rate=True)      # noqa: E731
                timed(native)
                tn = float(np.median([timed(native) for _ in range(a.repeats)]))
                out[f"synthesize_native_rate_s_p{bpp}"], out[f"native_rate_over_plain_p{bpp}"] = round(tn, 4), round(tn / s, 4)
        # the three new launches alone on the first 1024 beats' worth of whole recordings, each behind a fill larger than every cache
        r0, r1 = recording.chunks(plan, 1024)[0]
        nrec = int(plan.rec[r1 - 1]) + 1
        table, stitch, recs, offs = resident.stage_to_device((plan.plan.table[r0:r1], plan.stitch[r0:r1], plan.recordings[:nrec],
                                                              plan.out_offsets[:nrec]), dev)
        views = torch.rand((r1 - r0, 12, 512), dtype=torch.float32, device=dev)
        buf = torch.full((int(plan.out_offsets[nrec]),), float("nan"), dtype=torch.float32, device=dev)
        flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        rng = ops.beat_range(store.signal, table, 3, 0)
        n_sum, cover = int(plan.stitch[r0:r1, 2].sum()), int(np.minimum(plan.stitch[r0:r1, 2], 512).sum())
        esz = store.signal.element_size()
        calls = {"beat_range": (lambda: ops.beat_range(store.signal, table, 3, 0), n_sum * 8 * esz + table.numel() * 8 + rng.numel() * 8),
                 "beat_stitch": (lambda: ops.beat_stitch(views, rng, stitch, buf, "nan"), views.numel() * 4 + 12 * n_sum * 4 + stitch.numel() * 8),
                 "recording_stats": (lambda: ops.recording_stats(buf, store.signal, stitch, recs, list(range(12)), "nan", offs),
                                     12 * cover * 4 + 10 * cover * esz + nrec * 12 * 7 * 8)}
        for name, (fn, nbytes) in calls.items():
            us = []
            for _ in range(6):
                flush.zero_()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                us.append(s.elapsed_time(e) * 1e3)
            out[f"{name}_cold_us"], out[f"{name}_bytes"] = round(float(np.median(us[2:])), 2), int(nbytes)
        out["cold_launch_beats"] = r1 - r0
    return out


def drive(a):
    from bench_loader import make_tree
    root = tempfile.mkdtemp(prefix="nef_recording_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    runs = []
    try:
        make_tree(root, a.n, rate=a.source_rate or 500)
        for _ in range(a.rounds):
            for dtype in ("fp32", "fp16"):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", dtype, "--tree", root, "--repeats", str(a.repeats),
                       "--source-rate", str(a.source_rate)]
                res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.leg_timeout)
                if res.returncode != 0:
                    raise RuntimeError(f"leg {dtype} ended with exit code {res.returncode}")
                runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
                print(json.dumps(runs[-1]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = {"recordings": a.n, "rounds": a.rounds, "input_leads": LEADS, "angles": 12}
    if a.source_rate:
        line["source_rate"] = a.source_rate
    for dtype in ("fp32", "fp16"):
        mine = [r for r in runs if r["leg"] == dtype]
        for key in sorted(mine[0]):
            vals = [r[key] for r in mine]
            if key != "leg":
                line[f"{dtype}_{key}"] = [min(vals), float(np.median(vals)), max(vals)] if len(set(vals)) > 1 else vals[0]
    med = lambda v: v[1] if isinstance(v, list) else v      # noqa: E731
    line["synthesize_within_10_percent_of_batch_and_panorama"] = {
        f"{d}_p{p}": bool(med(line[f"{d}_synthesize_s_p{p}"]) <= MARGIN * med(line[f"{d}_batch_and_panorama_s_p{p}"]))
        for d in ("fp32", "fp16") for p in PASSES}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="timed (alone, synthesize) pairs per beats_per_pass in a process")
    ap.add_argument("--leg-timeout", type=float, default=400.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--source-rate", type=int, default=0, metavar="R", help="write the tree at R Hz and resample it on the device")
    ap.add_argument("--leg", choices=("fp32", "fp16"), help="(internal) one panorama dtype in this process")
    ap.add_argument("--tree", default="", help="(internal) the tree --leg reads")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recording needs a HIP device")
    if a.leg:
        print(json.dumps(leg(a)))
        return
    drive(a)


if __name__ == "__main__":
    main()
