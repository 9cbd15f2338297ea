"""Cost of Model_nefnet.locate at BASELINE configs[3]'s shape (1024 samples, 1 lead in, 360 level-0 angles, L = 512, fp16 panorama) against
the sweep it is built on.  `python tools/bench_locate.py [--rounds 3] [--out FILE]` prints one JSON line.

Legs, each in a fresh process per round, the rounds alternating them (gen, loc0, loc3, kernels, gen, ...), reported as [min, median, max]
over the rounds of each process's median call time (host clock around calls that end in a device synchronise, one warm-up call):
  gen      gen_ecg alone on the 18 x 20 grid, from latents -- existing code, the yardstick
  enc_gen  forward(phase='gen') + gen_ecg: the yardstick plus the encoder pass that locate() also makes (same process as gen)
  loc0     locate(levels=0): encoder pass, level-0 sweep, nef_locate_score, nef_locate_best
  loc3     locate(levels=3)
  kernels  nef_locate_score and nef_locate_best alone on a [1024, 360, 512] view tensor (755 MB: three times the Infinity Cache, so
           every call reads the views from HBM), device events; GB/s = view bytes / score time
The speed condition: loc0's median is no more than 5 % above gen's median in the same session."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, L, GRID = 1024, 1, 512, (18, 20)
LEGS = ("gen", "loc0", "loc3", "kernels")


def _cfg(V):
    class Cfg(dict):
        __getattr__ = dict.__getitem__
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=V, noise=False))


def child(leg, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from electrocardio_panorama_amd import locate, ops, synth
    from electrocardio_panorama_amd.network import build_model
    dev = torch.device("cuda", 0)
    torch.manual_seed(123)
    m = build_model(_cfg(V)).float().to(dev).eval()
    m.panorama_dtype = "fp16"
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.make_batch(B, V, L, seed=123, Q=1).items()
         if k in ("data", "input_theta", "target_theta", "rois", "rest_view")}
    grid = locate.Grid(*GRID)
    thetas = torch.from_numpy(grid.thetas()).to(dev).unsqueeze(0).expand(B, -1, -1).contiguous()
    observed = t["rest_view"][:, 0].contiguous()

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    res = {}
    if leg == "gen":
        z1, z2 = m(t["data"], t["input_theta"], t["target_theta"], t["rois"], phase="gen")
        res["gen"] = timed(lambda: m.gen_ecg(z1, z2, thetas, t["rois"]))
        res["enc_gen"] = timed(lambda: m.gen_ecg(*m(t["data"], t["input_theta"], t["target_theta"], t["rois"], phase="gen"), thetas, t["rois"]))
    elif leg in ("loc0", "loc3"):
        levels = 0 if leg == "loc0" else 3
        res[leg] = timed(lambda: m.locate(t["data"], t["input_theta"], t["rois"], observed, grid=grid, levels=levels))
    else:
        z1, z2 = m(t["data"], t["input_theta"], t["target_theta"], t["rois"], phase="gen")
        views = m.gen_ecg(z1, z2, thetas, t["rois"])
        obs3, cands = observed.unsqueeze(1).contiguous(), torch.from_numpy(grid.thetas()).to(dev)
        scores = torch.empty(B, 1, grid.size, device=dev, dtype=torch.float64)
        for mode in ("corr", "mse"):
            ops.locate_score(views, obs3, t["rois"], mode, out=scores)
            ops.locate_best(scores, cands)
            torch.cuda.synchronize(dev)
            ts, tb = [], []
            for _ in range(calls):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                ops.locate_score(views, obs3, t["rois"], mode, out=scores)
                e[1].record()
                ops.locate_best(scores, cands)
                e[2].record()
                torch.cuda.synchronize(dev)
                ts.append(e[0].elapsed_time(e[1]))
                tb.append(e[1].elapsed_time(e[2]))
            res["score_" + mode] = statistics.median(ts)
            res["best_" + mode] = statistics.median(tb)
        res["view_bytes"] = views.numel() * 4
    print("BENCH_LOCATE " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return child(a.leg, a.calls)
    got = {}
    for _ in range(a.rounds):
        for leg in LEGS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(a.calls)], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("BENCH_LOCATE ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"leg {leg} failed (exit {p.returncode})")
            for k, v in json.loads(line[-1][len("BENCH_LOCATE "):]).items():
                got.setdefault(k, []).append(v)
    view_bytes = got.pop("view_bytes")[0]
    out = {k + "_ms": [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in got.items()}
    for mode in ("corr", "mse"):
        out[f"score_{mode}_GBps"] = round(view_bytes / (statistics.median(got["score_" + mode]) * 1e-3) / 1e9, 1)
    ratio = statistics.median(got["loc0"]) / statistics.median(got["gen"])
    out.update(workload=f"batch={B}, {V} lead in, {GRID[0]} x {GRID[1]} = {GRID[0] * GRID[1]} level-0 angles, len={L}, fp16 panorama, 'corr' score",
               rounds=a.rounds, calls_per_process=a.calls, loc0_over_gen=round(ratio, 4),
               loc0_over_enc_gen=round(statistics.median(got["loc0"]) / statistics.median(got["enc_gen"]), 4), bar=1.05, within_bar=bool(ratio <= 1.05))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
