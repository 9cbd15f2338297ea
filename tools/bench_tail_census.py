"""Time nef_h2_tail_census (ops.tail_census: the partial launch + the one-workgroup combine) on full-size activations of the
configs[1] step, by HIP events around the pair, median of 20 after one warm call.

    python tools/bench_tail_census.py          -> profiles/r07_h2_tail_census.md (table on stdout)

The census runs once per call-site lifetime (at the site's measuring launch), never in a replayed step."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from electrocardio_panorama_amd import ops  # noqa: E402
from electrocardio_panorama_amd.ops import GV  # noqa: E402

SHAPES = [((256, 384, 1250), 3, "encoder activation [256, 3 x 128, 1250]"),
          ((256, 128, 2500), 1, "decoder activation [256, 128, 2500]"),
          ((256, 64, 5000), 1, "decoder activation [256, 64, 5000]")]
print("| operand | MB | median µs | GB/s |")
print("|---|---:|---:|---:|")
for shape, G, name in SHAPES:
    x = torch.exp(4.0 * torch.randn(*shape, device="cuda"))
    amax = x.abs().max().reshape(1)
    xv = GV.dense(x, G)
    ops.tail_census(xv, amax)
    ts = []
    for _ in range(20):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.tail_census(xv, amax)
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    mb = x.numel() * 4 / 1e6
    print(f"| {name} | {mb:.0f} | {ts[10] * 1e3:.1f} | {mb / ts[10]:.0f} |")
