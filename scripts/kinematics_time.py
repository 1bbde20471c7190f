"""Time of the launches of a kinematics push (kinematics_kernels.hip) on one MI355X -> profiles/kinematics_kernel_summary.md.

    python scripts/kinematics_time.py [--out FILE] [--pushes 30] [--warmup 5] [--size 1920x1080] [--radius 3] [--spacing 2]
                                      [--grid 32x18]

A smooth random field (two of them, alternating).  Per launch: the library's own HIP events (rcflow_profile_read,
"kinematics@0" and "kinematics@1"), one reading per push, the median over `pushes` pushes after `warmup`, in two passes, once
with every output and once with mask and records only.  Beside each launch stand the bytes it cannot avoid and the rate they
amount to:
  @0  the field 8 B/px in, the two state planes 8 B/px out, and 4 B/px for each of omega, div and ow that is asked for;
  @1  the two state planes 8 B/px in, the mask 1 B/px and the picture 3 B/px out where asked for.
Per push as a caller sees it: a host clock over the window ending in one synchronise, profiling off.  Needs a GPU: there is no
fallback.
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


def measure(ctx, w, h, R, s, gx, gy, pushes, warmup):
    rng = np.random.default_rng(1)
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    flow = []
    for k in range(2):
        u = np.sin(2 * np.pi * y / 97 + k) + 0.05 * rng.standard_normal((h, w), dtype=np.float32)
        v = np.cos(2 * np.pi * x / 131 - k) + 0.05 * rng.standard_normal((h, w), dtype=np.float32)
        flow.append(torch.as_tensor(np.stack([u, v], -1).astype(np.float32)).cuda())
    ctx.kinematics_open(w, h, radius=R, sigma=1.5, spacing=s, grid_x=gx, grid_y=gy, scale=25.0, pixel_area=0.01, ow_k=0.2, min_core=8, vis_max=5.0)
    nc = gx * gy
    every = dict(omega=torch.empty((h, w), dtype=torch.float32, device="cuda"), div=torch.empty((h, w), dtype=torch.float32, device="cuda"),
                 ow=torch.empty((h, w), dtype=torch.float32, device="cuda"), mask=torch.empty((h, w), dtype=torch.uint8, device="cuda"),
                 vis=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"), cells=torch.empty(nc * 48, dtype=torch.uint8, device="cuda"),
                 sums=torch.empty(nc * 11, dtype=torch.int64, device="cuda"), summary=torch.empty(8, dtype=torch.int64, device="cuda"))
    few = {k: every[k] for k in ("mask", "cells")}
    px = float(w * h)
    rows = []
    for name, kw, b0, b1 in (("every output", every, 28 * px, 12 * px), ("mask and records", few, 16 * px, 9 * px)):
        for p in range(2):
            per = {"kinematics@0": [], "kinematics@1": []}
            ctx.profile_enable(True)
            for t in range(warmup + pushes):
                ctx.profile_reset()
                ctx.kinematics_push(flow[t % 2], **kw)
                torch.cuda.synchronize()
                if t >= warmup:
                    for r in ctx.profile_read():
                        if r["kernel"] in per and r["launches"]:
                            per[r["kernel"]].append(r["total_ms"] * 1e3)
            ctx.profile_enable(False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(pushes):
                ctx.kinematics_push(flow[t % 2], **kw)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / pushes * 1e6
            t0us, t1us = float(np.median(per["kinematics@0"])), float(np.median(per["kinematics@1"]))
            rows.append((name, p + 1, t0us, b0 / 1e6, b0 / t0us / 1e6, t1us, b1 / 1e6, b1 / t1us / 1e6, wall))
    summ = ctx.kinematics_read()[2]
    assert summ["valid"] == (w - 2 * (R + s)) * (h - 2 * (R + s)) and summ["bad"] == 0 and summ["cores_cw"] > 0 and summ["cores_ccw"] > 0
    state = ctx.kinematics_info()["device_bytes"]
    ctx.kinematics_close()
    return state, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--spacing", type=int, default=2)
    ap.add_argument("--grid", default="32x18")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    gx, gy = (int(v) for v in a.grid.split("x"))
    lines = ["| size | R / s | grid | state MB | outputs | pass | @0 us | @0 MB | @0 TB/s | @1 us | @1 MB | @1 TB/s | push, host us |", "|" + "---|" * 13]
    with Context(3840, 2160) as ctx:
        state, rows = measure(ctx, w, h, a.radius, a.spacing, gx, gy, a.pushes, a.warmup)
        for r in rows:
            lines.append("| %dx%d | %d / %d | %dx%d | %.1f | %s | %d | %.1f | %.1f | %.2f | %.1f | %.1f | %.2f | %.1f |" % (
                (w, h, a.radius, a.spacing, gx, gy, state / 1e6) + r))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
