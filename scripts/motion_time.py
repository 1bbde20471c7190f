"""Time of the three launches of a motion-templates push (motion_kernels.hip) on one MI355X -> profiles/motion_kernel_summary.md.

    python scripts/motion_time.py [--out FILE] [--pushes 50] [--warmup 10]

Rows at 640x480, 1080p and 4K, grid 30 x 30, the texture clip of tests/_motion_ref.py moving 1 px per frame (threshold 12,
duration 6, deltas 0.5 and 2.5), with every output requested and with none.  Per launch: the library's own HIP events
(rcflow_profile_read, "motion@0".."motion@2"), one reading per push, the median over `pushes` pushes after `warmup`; beside it
the launch's compulsory bytes and what they come to per second.  Per push as a caller sees it: a host clock over the window
ending in one synchronise, profiling off.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ripcurrents_amd.api import Context           # noqa: E402
import _motion_ref as M                           # noqa: E402

PRM = dict(diff_threshold=12, duration=6, delta1=0.5, delta2=2.5)
GRID = (30, 30)


def measure(ctx, w, h, outputs, pushes, warmup):
    frames = [torch.as_tensor(f).cuda() for f in M.texture_clip(w, h, 40)]
    ctx.motion_open(w, h, grid=GRID, **PRM)
    kw = {}
    if outputs:
        kw = dict(mhi=torch.empty((h, w), dtype=torch.float32, device="cuda"), orient=torch.empty((h, w), dtype=torch.float32, device="cuda"),
                  mask=torch.empty((h, w), dtype=torch.uint8, device="cuda"), vis=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"),
                  cells=torch.empty(GRID[0] * GRID[1] * 40, dtype=torch.uint8, device="cuda"), frame=torch.empty(40, dtype=torch.uint8, device="cuda"))
    per = {"motion@%d" % k: [] for k in range(3)}
    nbytes = {}
    ctx.profile_enable(True)
    for t in range(warmup + pushes):
        ctx.profile_reset()
        ctx.motion_push(frames[t % len(frames)], **kw)
        torch.cuda.synchronize()
        if t >= warmup:
            for r in ctx.profile_read():
                if r["kernel"] in per and r["launches"]:
                    per[r["kernel"]].append(r["total_ms"] * 1e3)
                    nbytes[r["kernel"]] = r["alg_bytes"]
    ctx.profile_enable(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(pushes):
        ctx.motion_push(frames[t % len(frames)], **kw)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / pushes * 1e6
    got = ctx.motion_read()
    ctx.motion_close()
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v)), nbytes[k]) for k, v in per.items()}, wall, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    lines = ["| size | outputs | launch | median us | min..max us | compulsory MB | GB/s at the median |", "|---|---|---|---|---|---|---|"]
    with Context(3840, 2160) as ctx:
        for w, h in ((640, 480), (1920, 1080), (3840, 2160)):
            for outputs in (True, False):
                per, wall, got = measure(ctx, w, h, outputs, a.pushes, a.warmup)
                for k in sorted(per):
                    med, lo, hi, nb = per[k]
                    lines.append("| %dx%d | %s | %s | %.1f | %.1f..%.1f | %.2f | %.0f |" % (w, h, "all" if outputs else "none", k, med, lo, hi,
                                                                                       nb / 1e6, nb / med / 1e3))
                lines.append("| %dx%d | %s | push, host clock | %.1f | | | | angle %.2f, %d of %d masked pixels used |" % (
                    w, h, "all" if outputs else "none", wall, got["angle"], got["frame"]["n_used"], got["frame"]["n_masked"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
