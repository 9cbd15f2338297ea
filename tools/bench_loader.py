"""Throughput of the host `meta` pipeline (reference codes/train_net.py:27-28 + dataset/tianchi.py:84-225).

Builds a synthetic Tianchi-format tree (N recordings of 8 x 5000 samples with P/R/T on/off index lists, the on-disk layout of
reference codes/README.md:13), then drives it exactly as the packaged trainer does -- train_net.build_loaders (batch 32,
16 workers, pinned memory, the per-item restatement of EcgTianChiInterval.__getitem__) behind prefetch.DevicePrefetcher when
a HIP device is present -- and prints samples/s next to the rate one GPU consumes at that shape.

    python tools/bench_loader.py [--n 2048] [--epochs 3] [--workers 16] [--batch 32]

`--resident` compares that loader with DATA.device_resident (dataset/resident.py) on the same tree: `--rounds` alternating rounds of fresh
processes, each leg at batch 32 and batch 256 -- the worker loader through DevicePrefetcher as above; the resident loader alone with one
host thread; nef_beat_batch alone on cold recordings; the resident loader feeding a graphed FusedSGD step at batch 32 beside the same step
on preloaded synthetic batches.  Prints one JSON line of [min, median, max] per figure (`--out FILE` also writes it).

    python tools/bench_loader.py --resident [--rounds 3] [--n 2048] [--out profiles/r23_resident_bench_line.json]

`--resident --auto-marks` times DATA.auto_marks (dataset/marks.py) instead: the timing table is fitted on the tree once, then `--rounds`
alternating rounds of fresh processes build the annotated store and the auto-marked one (signals only, no label file read), and the second
also times marks.detect alone and the two kernels on cold data with their algorithmic bytes.  The line says how many recordings got labels.

    python tools/bench_loader.py --resident --auto-marks [--rounds 3] [--n 2048] [--out profiles/r29_marks_bench_line.json]

`--resident --source-rate R [R ...]` times DATA.source_rate (resample.py; nef_resample): per rate the tree is written at R Hz -- the same
beats, 5000 R / 500 samples a recording -- and `--rounds` alternating rounds of fresh processes build the store of those files with the key
off and with DATA.source_rate = R; the second also times nef_resample alone on cold data, with its algorithmic bytes, at the store's own
ratio (taps in LDS) and at 500 / 257 on the same buffer (taps in global memory).  The line says whether the key-on build stays within 10 %.

    python tools/bench_loader.py --resident --source-rate 1000 360 [--rounds 3] [--n 2048] [--out profiles/r31_resample_bench_line.json]

`--resident --clean` times DATA.baseline_ms / DATA.mains_hz (clean.py; nef_sliding_median): the tree is written with a 0.3 Hz wander and a
50 Hz hum added to every lead, and `--rounds` alternating rounds of fresh processes build the store of those files with the keys off and
with [200, 600] ms + 50 Hz on; the second also times, on one chunk of at most 2^25 samples behind a cache flush and with their algorithmic
bytes, nef_sliding_median at h = 50 and h = 150 and the 1/1 511-tap nef_resample.  The line says whether the key-on build stays within 10 %.

    python tools/bench_loader.py --resident --clean [--rounds 3] [--n 2048] [--out profiles/r32_clean_bench_line.json]
"""
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
import numpy as np   # noqa: E402
import torch         # noqa: E402

BATCHES = (32, 256)


def make_tree(root, n, seed=0, rate=500, dirty=False):
    """n recordings: smooth 8-lead signals with a beat every 600..900 samples and plausible wave boundaries -- at 500 Hz; `rate` writes the
    same ten seconds at another rate (every count of samples times rate / 500); `dirty` adds a 0.3 Hz wander of half a beat's height and a
    50 Hz hum of a tenth to every lead."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "npy"), exist_ok=True)
    os.makedirs(os.path.join(root, "json"), exist_ok=True)
    names = []
    k = rate / 500.0
    q = lambda v: np.round(np.asarray(v) * k).astype(np.int64)      # noqa: E731
    length = int(q(5000))
    t = np.arange(length)
    for i in range(n):
        period = int(q(rng.integers(600, 900)))
        p_on = np.arange(int(q(rng.integers(20, 100))), length - period, period)
        lab = {"P on": p_on, "P off": p_on + q(60), "R on": p_on + q(110), "R off": p_on + q(170), "T on": p_on + q(260), "T off": p_on + q(400)}
        sig = np.zeros((8, length))
        for c, w in ((85 * k, 18 * k), (140 * k, 9 * k), (330 * k, 40 * k)):
            for p in p_on:
                sig += rng.normal(1.0, 0.3, size=(8, 1)) * np.exp(-0.5 * ((t - p - c) / w) ** 2)
        sig += rng.normal(0, 0.01, size=sig.shape)
        if dirty:
            sig += 0.5 * np.sin(2 * np.pi * 0.3 * t / rate + 0.7) + 0.1 * np.sin(2 * np.pi * 50.0 * t / rate + 0.3)
        np.save(os.path.join(root, "npy", f"{i}.npy"), sig.astype(np.float32))
        with open(os.path.join(root, "json", f"{i}.json"), "w") as f:
            json.dump({k: v.tolist() for k, v in lab.items()}, f)
        names.append(f"{i}.json")
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("\n".join(names))
    return os.path.join(root, "list.txt")


def tree_cfg(root, leads):
    from electrocardio_panorama_amd.config import get_defaults, resolve_config_path
    cfg = get_defaults()
    cfg.merge_from_file(resolve_config_path("config/nef_net.yml"))
    cfg.DATA.lead_num = leads
    cfg.DATA.dataset = "tianchi"
    cfg.DATA.train_label_path = cfg.DATA.test_label_path = os.path.join(root, "list.txt")
    cfg.DATA.train_data_root = os.path.join(root, "npy")
    cfg.DATA.train_label_root = os.path.join(root, "json")
    return cfg


def worker_loader_rates(cfg, batch, workers, epochs, modes):
    """samples/s of the packaged worker loader: 'host' = batches arriving in the trainer, 'device' = behind DevicePrefetcher."""
    from electrocardio_panorama_amd import train_net
    from electrocardio_panorama_amd.prefetch import DevicePrefetcher
    import torch.utils.data as tud
    orig = tud.DataLoader

    def patched(*args, **kw):           # the packaged loader, with the worker count under test
        if kw.get("num_workers", 0) == 16:
            kw["num_workers"] = workers
        return orig(*args, **kw)
    tud.DataLoader = patched
    try:
        dl = train_net.build_loaders(cfg, batch_size=batch, phases=("train",))[0]
    finally:
        tud.DataLoader = orig
    dev = torch.device("cuda", 0)
    res = {}
    for mode in modes:
        it_src = dl if mode == "host" else DevicePrefetcher(dl, dev)
        n, t0 = 0, None
        for ep in range(epochs + 1):            # epoch 0: worker start-up, untimed
            if ep == 1:
                t0, n = time.perf_counter(), 0
            for meta in it_src:
                n += int(meta["data"].shape[0])
        if mode == "device":
            torch.cuda.synchronize()
        res[mode] = n / (time.perf_counter() - t0)
    del dl
    return res


def leg_workers(a):
    cfg = tree_cfg(a.tree, a.leads)
    cfg.MODEL.jitter_factor = 0.0       # both legs of --resident without the angle jitter
    out = {"leg": "workers", "workers": a.workers}
    for b in BATCHES:
        out[f"workers_on_device_b{b}"] = round(worker_loader_rates(cfg, b, a.workers, a.epochs, ["device"])["device"], 1)
    return out


def leg_resident(a):
    """The resident loader alone (one host thread), the kernel alone on cold recordings, and the loader feeding a graphed step."""
    import random
    from electrocardio_panorama_amd import ops, synth
    from electrocardio_panorama_amd.dataset import resident
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    cfg = tree_cfg(a.tree, a.leads)
    cfg.DATA.device_resident = True
    cfg.MODEL.jitter_factor = 0.0
    torch.zeros(1, device=dev)
    t0 = time.perf_counter()
    store = resident.ResidentTianchi(cfg, "train", dev)
    torch.cuda.synchronize()
    out = {"leg": "resident", "store_build_s": round(time.perf_counter() - t0, 3), "store_device_bytes": store.device_bytes,
           "store_dtype": str(store.signal.dtype).replace("torch.", "")}
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)        # larger than L2 and the Infinity Cache together
    for b in BATCHES:
        ld = resident.ResidentLoader(store, cfg, "train", b, seed=cfg.seed)
        n, t0 = 0, None
        for ep in range(a.resident_epochs + 1):                          # epoch 0: first launches, untimed
            if ep == 1:
                torch.cuda.synchronize()
                t0, n = time.perf_counter(), 0
            ld.sampler.set_epoch(ep)
            for meta in ld:
                n += int(meta["data"].shape[0])
        torch.cuda.synchronize()
        out[f"resident_on_device_b{b}"] = round(n / (time.perf_counter() - t0), 1)
        # the kernel alone: every launch behind a 512 MiB fill, so its recordings come from HBM
        us, nbytes = [], 0
        for _, _, plan in list(ld.plans(0))[:12]:
            table = torch.from_numpy(plan.table).to(dev)
            flush.zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ops.beat_batch(store.signal, table, plan.V, plan.R)
            e.record()
            e.synchronize()
            us.append(s.elapsed_time(e) * 1e3)
            # algorithmic bytes: the beat's eight stored leads once, the plan, the rows written
            nbytes = int(plan.table[:, 2].sum()) * 8 * store.signal.element_size() + plan.table.nbytes + b * (plan.V + 1 + plan.R) * 512 * 4
        out[f"beat_batch_cold_us_b{b}"] = round(float(np.median(us[2:] or us)), 2)      # the first two: code load, allocator
        out[f"beat_batch_bytes_b{b}"] = nbytes
    del flush
    # the graphed FusedSGD step at batch 32: fed by the resident loader, and on preloaded synthetic batches of the same shape
    cfg.SOLVER.graph = True
    ld = resident.ResidentLoader(store, cfg, "train", 32, seed=cfg.seed)
    pre = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.make_batch(32, a.leads, 512, seed=i, Q=9).items()}
           for i in range(len(ld))]
    for name, feed in (("resident", ld), ("preloaded_synthetic", pre)):
        torch.manual_seed(1234)
        sol = Solver(cfg, use_tensorboardx=False)
        opt = get_optimizer(cfg, sol.model.parameters())
        random.seed(1)
        sol.run_one_epoch(feed, "train", opt, collect_views=False)       # capture and warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.step_epochs):
            sol.run_one_epoch(feed, "train", opt, collect_views=False)
        torch.cuda.synchronize()
        out[f"graphed_step_ms_b32_{name}"] = round((time.perf_counter() - t0) * 1e3 / (a.step_epochs * len(feed)), 4)
        assert getattr(sol, "_graph_stepper", None) is not None
    return out


def _timed_store(cfg, dev, **kw):
    from electrocardio_panorama_amd.dataset import resident
    torch.zeros(1, device=dev)
    t0 = time.perf_counter()
    store = resident.ResidentTianchi(cfg, "train", dev, **kw)
    torch.cuda.synchronize()
    return store, round(time.perf_counter() - t0, 3)


def leg_fit(a):
    """Fit the ratio table on the tree's own annotations and leave it in the tree."""
    from electrocardio_panorama_amd.dataset import marks, resident
    cfg = tree_cfg(a.tree, a.leads)
    store = resident.ResidentTianchi(cfg, "train", torch.device("cuda", 0))
    params = marks.MarkParams.from_rate(cfg.DATA.sample_rate)
    fit = marks.fit_table(store, marks.detect(store, params=params))
    marks.save_table(os.path.join(a.tree, "table.json"), fit.table, params=params)
    return {"leg": "fit", "fit_matched_beats": fit.matched, "fit_left_out_beats": fit.left_out, "fit_table_b": np.round(fit.table[:, 1], 4).tolist()}


def leg_store(a):
    """The annotated store build alone: what the auto-marked build is held against."""
    cfg = tree_cfg(a.tree, a.leads)
    cfg.DATA.device_resident = True
    torch.set_num_threads(1)
    _, sec = _timed_store(cfg, torch.device("cuda", 0))
    return {"leg": "store", "annotated_store_build_s": sec}


def leg_auto(a):
    """The auto-marked store build (signals only), marks.detect alone on the built store, and the two kernels behind a cache flush."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.dataset import marks
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    cfg = tree_cfg(a.tree, a.leads)
    cfg.DATA.train_label_root = os.path.join(a.tree, "no_labels")        # nothing there: the build opens no label file
    cfg.DATA.device_resident, cfg.DATA.auto_marks, cfg.DATA.auto_marks_skip = True, True, True
    cfg.DATA.mark_table = os.path.join(a.tree, "table.json")
    store, sec = _timed_store(cfg, dev)
    rep = store.auto_report
    out = {"leg": "auto", "auto_store_build_s": sec, "auto_recordings_marked": rep["marked"], "auto_recordings": rep["recordings"],
           "auto_peaks": rep["peaks"], "auto_peaks_dropped": rep["dropped"], "auto_marks_adjusted": rep["adjusted"],
           "store_dtype": str(store.signal.dtype).replace("torch.", "")}
    _, _, params = marks.load_table(cfg.DATA.mark_table)
    ms = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        marks.detect(store, params=params)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["detect_ms"] = round(float(np.median(ms[1:])), 3)
    # the kernels alone, every launch behind a 512 MiB fill: one chunk of at most 2^25 samples, as detect cuts them
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    a0, b0 = marks._chunks(store.lengths.tolist(), 1 << 25)[0]
    ln = store.lengths[a0:b0]
    eoff = np.concatenate([[0], np.cumsum(ln)[:-1]])
    table = torch.from_numpy(np.ascontiguousarray(np.stack([store.offsets[a0:b0], ln, eoff], axis=1), dtype=np.int64)).to(dev)
    env = torch.empty(int(ln.sum()), dtype=torch.float64, device=dev)
    us = {"mark_envelope": [], "mark_peaks": []}
    for _ in range(5):
        for name, call in (("mark_envelope", lambda: ops.mark_envelope(store.signal, table, env, D=params.D, H=params.H,
                                                                       lead_bits=params.lead_bits, max_len=int(ln.max()))),
                           ("mark_peaks", lambda: ops.mark_peaks(env, table, r=params.r, seg=params.seg, frac=params.frac,
                                                                 max_peaks=params.max_peaks, max_len=int(ln.max())))):
            flush.zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            call()
            e.record()
            e.synchronize()
            us[name].append(s.elapsed_time(e) * 1e3)
    samples, rows = int(ln.sum()), int(ln.size)
    nbytes = {"mark_envelope": samples * 8 * store.signal.element_size() + samples * 8 + rows * 24,
              "mark_peaks": samples * 8 + rows * (24 + 4 * params.max_peaks + 12)}
    for name in us:
        t = float(np.median(us[name][1:]))                              # the first: code load, allocator
        out[f"{name}_cold_us"], out[f"{name}_bytes"], out[f"{name}_tb_s"] = round(t, 2), nbytes[name], round(nbytes[name] / t * 1e-6, 4)
    return out


def leg_rate(a):
    """The store build with DATA.source_rate on, and nef_resample alone behind a cache flush: at the store's ratio (taps in LDS) and at
    500 / 257 on the same raw buffer (taps in global memory)."""
    from electrocardio_panorama_amd import ops, resample
    from electrocardio_panorama_amd.dataset import marks, resident
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    cfg = tree_cfg(a.tree, a.leads)
    cfg.DATA.device_resident, cfg.DATA.source_rate = True, a.rate
    store, sec = _timed_store(cfg, dev)
    rep = store.resample_report
    out = {"leg": "rate", "resampled_store_build_s": sec, "store_dtype": str(store.signal.dtype).replace("torch.", ""), "up": rep["up"],
           "down": rep["down"], "taps_per_phase": rep["taps"], "launches": rep["launches"], "marks_adjusted": rep["adjusted"],
           "store_device_bytes": store.device_bytes}
    cfg.DATA.source_rate = 0
    raw = resident.ResidentTianchi(cfg, "train", dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for tag, (up, down) in (("lds_taps", (rep["up"], rep["down"])), ("global_taps", (500, 257))):
        taps, first = resample.design(up, down)
        assert (taps.size <= 4096) == (tag == "lds_taps")
        new = resample.out_len(raw.lengths, up, down)
        a0, b0 = marks._chunks((8 * new).tolist(), 1 << 25)[0]
        ooff = np.concatenate([[0], np.cumsum(8 * new[a0:b0])])
        table = torch.from_numpy(np.ascontiguousarray(np.stack([raw.offsets[a0:b0], raw.lengths[a0:b0], ooff[:-1], np.full(b0 - a0, 8)], axis=1),
                                                      dtype=np.int64)).to(dev)
        dst = torch.empty(int(ooff[-1]), dtype=torch.float32, device=dev)
        taps_d, first_d = torch.from_numpy(taps).to(dev), torch.from_numpy(first).to(dev)
        us = []
        for _ in range(6):
            flush.zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ops.resample(raw.signal, table, dst, taps_d, first_d, up, down, max_out_len=int(new[a0:b0].max()), max_rows=8)
            e.record()
            e.synchronize()
            us.append(s.elapsed_time(e) * 1e3)
        # algorithmic bytes: the rows read once, the results written once, the two tables
        nbytes = int(8 * raw.lengths[a0:b0].sum()) * raw.signal.element_size() + int(ooff[-1]) * 4 + table.numel() * 8 + taps.nbytes + first.nbytes
        t = float(np.median(us[1:]))                                    # the first: code load, allocator
        out[f"resample_{tag}_cold_us"], out[f"resample_{tag}_bytes"] = round(t, 2), nbytes
        out[f"resample_{tag}_tb_s"], out[f"resample_{tag}_ratio"] = round(nbytes / t * 1e-6, 4), f"{up}/{down}"
    return out


def leg_clean(a):
    """The store build with DATA.baseline_ms and DATA.mains_hz on, and the three launches alone behind a cache flush on one chunk."""
    from electrocardio_panorama_amd import clean, ops
    from electrocardio_panorama_amd.dataset import marks, resident
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    cfg = tree_cfg(a.tree, a.leads)
    cfg.DATA.device_resident, cfg.DATA.baseline_ms, cfg.DATA.mains_hz = True, [200, 600], 50.0
    store, sec = _timed_store(cfg, dev)
    rep = store.clean_report
    out = {"leg": "clean", "cleaned_store_build_s": sec, "store_dtype": str(store.signal.dtype).replace("torch.", ""), "h1": rep["h1"],
           "h2": rep["h2"], "notch_taps": rep["taps"], "launches": rep["launches"], "store_device_bytes": store.device_bytes}
    cfg.DATA.baseline_ms, cfg.DATA.mains_hz = [], 0.0
    raw = resident.ResidentTianchi(cfg, "train", dev)
    a0, b0 = marks._chunks((8 * raw.lengths).tolist(), 1 << 25)[0]
    lo, hi = int(raw.offsets[a0]), int(raw.offsets[b0])
    src = raw.signal[lo:hi]
    table = torch.from_numpy(np.ascontiguousarray(np.stack([raw.offsets[a0:b0] - lo, raw.lengths[a0:b0], np.full(b0 - a0, 8)], axis=1),
                                                  dtype=np.int64)).to(dev)
    table4 = torch.from_numpy(np.ascontiguousarray(np.stack([raw.offsets[a0:b0] - lo, raw.lengths[a0:b0], raw.offsets[a0:b0] - lo,
                                                             np.full(b0 - a0, 8)], axis=1), dtype=np.int64)).to(dev)
    dst, tmp = torch.empty(hi - lo, dtype=torch.float32, device=dev), torch.empty(hi - lo, dtype=torch.float32, device=dev)
    taps, first = clean.notch_taps(500.0, 50.0)
    taps_d, first_d = torch.from_numpy(taps).to(dev), torch.from_numpy(first).to(dev)
    max_len = int(raw.lengths[a0:b0].max())
    ops.sliding_median(src, table, tmp, 50, max_len=max_len, max_rows=8)
    calls = (("median_h50", lambda: ops.sliding_median(src, table, dst, 50, max_len=max_len, max_rows=8), src.element_size() + 4),
             ("median_h150_minus", lambda: ops.sliding_median(tmp, table, dst, 150, minuend=src, max_len=max_len, max_rows=8), 4 + src.element_size() + 4),
             ("notch_511", lambda: ops.resample(src, table4, dst, taps_d, first_d, 1, 1, max_out_len=max_len, max_rows=8), src.element_size() + 4))
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)        # larger than L2 and the Infinity Cache together
    out["chunk_samples"] = hi - lo
    for name, call, per_sample in calls:
        us = []
        for _ in range(5):
            flush.zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            call()
            e.record()
            e.synchronize()
            us.append(s.elapsed_time(e) * 1e3)
        # algorithmic bytes: every input read once, the result written once, the table
        nbytes = (hi - lo) * per_sample + table.numel() * 8 + (taps.nbytes + first.nbytes if name == "notch_511" else 0)
        t = float(np.median(us[1:]))                                    # the first: code load, allocator
        out[f"{name}_cold_us"], out[f"{name}_bytes"], out[f"{name}_tb_s"] = round(t, 2), nbytes, round(nbytes / t * 1e-6, 4)
    return out


def drive_clean(a):
    """The dirty tree once, then `--rounds` alternating rounds of fresh processes: the key-off build, the key-on build."""
    root = tempfile.mkdtemp(prefix="nef_clean_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    runs = []
    try:
        make_tree(root, a.n, dirty=True)
        for leg in ["store", "clean"] * a.rounds:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", root, "--leads", str(a.leads)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.leg_timeout)
            if res.returncode != 0:
                raise RuntimeError(f"leg {leg} ended with exit code {res.returncode}")
            runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = {"recordings": a.n, "rounds": a.rounds}
    for key in sorted({k for r in runs for k in r}):
        vals = [r[key] for r in runs if key in r]
        if isinstance(vals[0], (int, float)) and len(set(vals)) > 1:
            line[key] = [min(vals), float(np.median(vals)), max(vals)]
        elif key != "leg":
            line[key] = vals[0]
    med = lambda v: v[1] if isinstance(v, list) else v      # noqa: E731
    line["key_off_store_build_s"] = line.pop("annotated_store_build_s")
    line["cleaned_build_over_key_off"] = round(med(line["cleaned_store_build_s"]) / med(line["key_off_store_build_s"]), 4)
    line["cleaned_build_within_10_percent"] = bool(line["cleaned_build_over_key_off"] <= 1.10)
    launches_ms = (med(line["median_h50_cold_us"]) + med(line["median_h150_minus_cold_us"]) + med(line["notch_511_cold_us"])) * 1e-3
    line["launches_ms_one_chunk"] = round(launches_ms, 3)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


def drive_rate(a):
    """Per rate: the tree at that rate, then `--rounds` alternating rounds of fresh processes -- the key-off build, the key-on build."""
    line = {"recordings": a.n, "rounds": a.rounds, "rates": {}}
    med = lambda v: v[1] if isinstance(v, list) else v      # noqa: E731
    for rate in a.source_rate:
        root = tempfile.mkdtemp(prefix="nef_rate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        runs = []
        try:
            make_tree(root, a.n, rate=rate)
            for leg in ["store", "rate"] * a.rounds:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", root, "--leads", str(a.leads), "--rate", str(rate)]
                res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.leg_timeout)
                if res.returncode != 0:
                    raise RuntimeError(f"leg {leg} ended with exit code {res.returncode}")
                runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
                print(json.dumps(runs[-1]), flush=True)
        finally:
            shutil.rmtree(root, ignore_errors=True)
        one = {}
        for key in sorted({k for r in runs for k in r}):
            vals = [r[key] for r in runs if key in r]
            if isinstance(vals[0], (int, float)) and len(set(vals)) > 1:
                one[key] = [min(vals), float(np.median(vals)), max(vals)]
            elif key != "leg":
                one[key] = vals[0]
        one["key_off_store_build_s"] = one.pop("annotated_store_build_s")
        one["resampled_build_over_key_off"] = round(med(one["resampled_store_build_s"]) / med(one["key_off_store_build_s"]), 4)
        one["resampled_build_within_10_percent"] = bool(one["resampled_build_over_key_off"] <= 1.10)
        line["rates"][str(rate)] = one
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


def drive_auto(a):
    """The table once, then `--rounds` alternating rounds of fresh processes: the annotated build, the auto-marked build."""
    root = tempfile.mkdtemp(prefix="nef_marks_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    runs = []
    try:
        make_tree(root, a.n)
        for leg in ["fit"] + ["store", "auto"] * a.rounds:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", root, "--leads", str(a.leads)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.leg_timeout)
            if res.returncode != 0:
                raise RuntimeError(f"leg {leg} ended with exit code {res.returncode}")
            runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = {"recordings": a.n, "rounds": a.rounds}
    for key in sorted({k for r in runs for k in r}):
        vals = [r[key] for r in runs if key in r]
        if isinstance(vals[0], (int, float)) and len(set(vals)) > 1:
            line[key] = [min(vals), float(np.median(vals)), max(vals)]
        elif key != "leg":
            line[key] = vals[0]
    med = lambda v: v[1] if isinstance(v, list) else v      # noqa: E731
    line["auto_build_over_annotated"] = round(med(line["auto_store_build_s"]) / med(line["annotated_store_build_s"]), 4)
    line["auto_build_within_10_percent"] = bool(line["auto_build_over_annotated"] <= 1.10)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


def drive_resident(a):
    """`--rounds` alternating rounds of fresh processes on one tree; [min, median, max] of every figure."""
    root = tempfile.mkdtemp(prefix="nef_loader_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    runs = []
    try:
        make_tree(root, a.n)
        for _ in range(a.rounds):
            for leg in ("workers", "resident"):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", root, "--epochs", str(a.epochs), "--workers",
                       str(a.workers), "--leads", str(a.leads), "--resident-epochs", str(a.resident_epochs), "--step-epochs", str(a.step_epochs)]
                res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.leg_timeout)
                if res.returncode != 0:
                    raise RuntimeError(f"leg {leg} ended with exit code {res.returncode}")
                runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
                print(json.dumps(runs[-1]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = {"recordings": a.n, "rounds": a.rounds, "leads": a.leads, "workers": a.workers, "host_cores": os.cpu_count()}
    for key in sorted({k for r in runs for k in r}):
        vals = [r[key] for r in runs if key in r]
        if isinstance(vals[0], (int, float)) and key != "workers":
            line[key] = [min(vals), float(np.median(vals)), max(vals)] if len(set(vals)) > 1 else vals[0]
        elif key not in ("leg", "workers"):
            line[key] = vals[0]
    w, r = line.get("workers_on_device_b32"), line.get("resident_on_device_b32")
    med = lambda v: v[1] if isinstance(v, list) else v      # noqa: E731
    line["resident_one_thread_matches_workers_b32"] = bool(med(r) >= med(w))
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--leads", type=int, default=3)
    ap.add_argument("--resident", action="store_true", help="compare the worker loader with DATA.device_resident (needs a HIP device)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--resident-epochs", type=int, default=10)
    ap.add_argument("--step-epochs", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=400.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--auto-marks", action="store_true", help="with --resident: time DATA.auto_marks against the annotated store build")
    ap.add_argument("--source-rate", type=int, nargs="+", default=[], metavar="R",
                    help="with --resident: time DATA.source_rate = R against the key-off build of the same files, per rate")
    ap.add_argument("--clean", action="store_true", help="with --resident: time DATA.baseline_ms / DATA.mains_hz against the key-off build")
    ap.add_argument("--leg", choices=("workers", "resident", "fit", "store", "auto", "rate", "clean"), help="(internal) one leg of --resident in this process")
    ap.add_argument("--rate", type=int, default=500, help="(internal) the rate the tree of --leg rate was written at")
    ap.add_argument("--tree", default="", help="(internal) the tree --leg reads")
    a = ap.parse_args()
    if a.leg:
        if not torch.cuda.is_available():
            raise SystemExit("--resident needs a HIP device")
        legs = {"workers": leg_workers, "resident": leg_resident, "fit": leg_fit, "store": leg_store, "auto": leg_auto, "rate": leg_rate,
                "clean": leg_clean}
        print(json.dumps(legs[a.leg](a)))
        return
    if a.auto_marks and not a.resident:
        raise SystemExit("--auto-marks goes with --resident: the marks are made on the device-resident store")
    if a.source_rate and (not a.resident or a.auto_marks):
        raise SystemExit("--source-rate goes with --resident alone: the recordings are resampled on the device-resident store")
    if a.clean and (not a.resident or a.auto_marks or a.source_rate):
        raise SystemExit("--clean goes with --resident alone: the recordings are cleaned on the device-resident store")
    if a.resident and a.clean:
        return drive_clean(a)
    if a.resident and a.source_rate:
        return drive_rate(a)
    if a.resident:
        return drive_auto(a) if a.auto_marks else drive_resident(a)
    root = tempfile.mkdtemp(prefix="nef_loader_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        make_tree(root, a.n)
        cfg = tree_cfg(root, a.leads)
        dev = torch.device("cuda", 0) if torch.cuda.is_available() else None
        res = worker_loader_rates(cfg, a.batch, a.workers, a.epochs, ["host"] + (["device"] if dev is not None else []))
        out = {"recordings": a.n, "batch": a.batch, "workers": a.workers, "host_cores": os.cpu_count(), "leads": a.leads,
               "samples_per_s_host_batches": round(res["host"], 1),
               "samples_per_s_on_device": round(res.get("device", float("nan")), 1)}
        print(json.dumps(out))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
