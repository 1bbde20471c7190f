"""Time of the launches of a wave-spectra push (waves_kernels.hip) on one MI355X -> profiles/waves_kernel_summary.md.

    python scripts/waves_time.py [--out FILE] [--pushes 30] [--warmup 5] [--sizes 512x512,1920x1080] [--bins 4,16] [--window 64]

Rows at 512x512 and 1080p with 4 and 16 bins, spacing 2, a grid of 16 x 9 cells, random frames (every pixel changes at every
push, so no lane of waves@0 finds its four pixels unchanged).  Per launch: the library's own HIP events (rcflow_profile_read,
"waves@0".."waves@2"), one reading per push, the median over `pushes` pushes after `warmup`, in two passes.  Beside waves@0
stand what its (2 + 16 K) bytes per pixel would take at the data sheet's 8 TB/s, which is the roof and no measurement of this
kernel, and the ring-slot launch of the flow map ("ftle@0", 16 bytes per pixel) at the same size, timed in the same run by the
same events.  Per push as a caller sees it: a host clock over the window ending in one synchronise, profiling off, once with
every output NULL and once with every output asked for.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ripcurrents_amd.api import Context           # noqa: E402

ROOF = 8e12                                       # bytes per second: the data sheet's HBM figure


def measure(ctx, w, h, K, window, pushes, warmup):
    gx, gy = 16, 9
    rng = np.random.default_rng(1)
    frames = [torch.as_tensor(rng.integers(0, 256, (h, w), dtype=np.uint8)).cuda() for _ in range(5)]      # 5 does not divide the window: the slot a push replaces holds another frame
    flow = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    ctx.waves_open(w, h, window=window, bin_lo=2, bin_hi=1 + K, spacing=2, grid_x=gx, grid_y=gy, fps=2.0, metres_per_pixel_x=0.5,
                   metres_per_pixel_y=0.5)
    ctx.ftle_open(w, h, window=2)
    kw = dict(cells=torch.empty(gy * gx * 32, dtype=torch.uint8, device="cuda"), sums=torch.empty((gy, gx, K, 6), dtype=torch.int64, device="cuda"),
              bin_map=torch.empty((h, w), dtype=torch.uint8, device="cuda"), vis=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"),
              summary=torch.empty(8, dtype=torch.int64, device="cuda"))
    passes = []
    for _ in range(2):
        per = {"waves@%d" % k: [] for k in range(3)}
        per["ftle@0"] = []
        ctx.profile_enable(True)
        for t in range(warmup + pushes):
            ctx.profile_reset()
            ctx.waves_push(frames[t % 5], **kw)
            ctx.ftle_push(flow)
            torch.cuda.synchronize()
            if t >= warmup:
                for r in ctx.profile_read():
                    if r["kernel"] in per and r["launches"]:
                        per[r["kernel"]].append(r["total_ms"] * 1e3)
        ctx.profile_enable(False)
        wall = []
        for out in ({}, kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(pushes):
                ctx.waves_push(frames[t % 5], **out)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / pushes * 1e6)
        passes.append(({k: float(np.median(v)) for k, v in per.items()}, wall))
    got = ctx.waves_read()[2]
    assert got["participating"] == (w - 4) * (h - 4) and got["held"] == min(got["pushes"], window)
    ctx.ftle_close()
    ctx.waves_close()
    return passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="512x512,1920x1080")
    ap.add_argument("--bins", default="4,16")
    ap.add_argument("--window", type=int, default=64)
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    lines = ["| size | bins | pass | waves@0 us | (2 + 16 K) B/px at 8 TB/s, us | waves@0 / roof | waves@0 TB/s | ftle@0 us | waves@1 us | waves@2 us | "
             "push, no output, host us | push, every output, host us |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    with Context(3840, 2160) as ctx:
        for w, h in sizes:
            for K in (int(v) for v in a.bins.split(",")):
                for i, (per, wall) in enumerate(measure(ctx, w, h, K, a.window, a.pushes, a.warmup)):
                    byts = (2. + 16. * K) * w * h
                    roof = byts / ROOF * 1e6
                    lines.append("| %dx%d | %d | %d | %.1f | %.1f | %.2f | %.2f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
                        w, h, K, i + 1, per["waves@0"], roof, per["waves@0"] / roof, byts / per["waves@0"] / 1e6, per["ftle@0"], per["waves@1"],
                        per["waves@2"], wall[0], wall[1]))
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
