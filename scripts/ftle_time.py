"""Time of the launches of a flow-map / FTLE push (ftle_kernels.hip) on one MI355X -> profiles/ftle_kernel_summary.md.

    python scripts/ftle_time.py [--out FILE] [--pushes 30] [--warmup 5] [--sizes 640x480,1920x1080,3840x2160] [--windows 8,30]

Rows at 640x480, 1080p and 4K, windows 8 and 30, backward, spacing 1, every output requested, on two inputs: the surf field
of ripcurrents_amd/synth.py (steady; most particles stay in the frame) and the same field five times as fast (most particles
leave it).  Per launch: the library's own HIP events (rcflow_profile_read, "ftle@0".."ftle@2"), one reading per push with a
full ring, the median over `pushes` pushes after `warmup`, in two passes.  The yardstick of ftle@1 is the existing code doing
the same arithmetic the slow way: `window` launches of advect_field (rcflow_advect_field_dev, iterations 1, UPPER +inf) at the
same size, timed in the same run by the same events ("advect_field@0", the sum of a push's worth).  Per push as a caller sees
it: a host clock over the window ending in one synchronise, profiling off.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ripcurrents_amd import synth                 # noqa: E402
from ripcurrents_amd.api import Context           # noqa: E402


def field(w, h, speed):
    U, V = synth.surf_field(w, h)
    return torch.as_tensor(np.ascontiguousarray(np.stack([U, V], -1) * speed, dtype=np.float32)).cuda()


def measure(ctx, w, h, window, speed, pushes, warmup):
    f = field(w, h, speed)
    ctx.ftle_open(w, h, window=window, direction="backward", dt=1.0, spacing=1, threshold=0.02, vis_max=0.1)
    kw = dict(map=torch.empty((h, w, 2), dtype=torch.float32, device="cuda"), steps=torch.empty((h, w), dtype=torch.int32, device="cuda"),
              lam=torch.empty((h, w), dtype=torch.float32, device="cuda"), ftle=torch.empty((h, w), dtype=torch.float32, device="cuda"),
              mask=torch.empty((h, w), dtype=torch.uint8, device="cuda"), vis=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"),
              summary=torch.empty(8, dtype=torch.int64, device="cuda"))
    for _ in range(window):                       # fill the ring: every timed push walks `window` fields
        ctx.ftle_push(f)
    ctx.analysis_reset(w, h)
    passes = []
    for _ in range(2):
        per = {"ftle@%d" % k: [] for k in range(3)}
        per["advect_field@0"] = []
        ctx.profile_enable(True)
        for t in range(warmup + pushes):
            ctx.profile_reset()
            ctx.ftle_push(f, **kw)
            ctx.analysis_reset(w, h)              # the yardstick's particles start at their pixels, as the flow map's do
            for _k in range(window):
                ctx.streamline_field(f, 1.0, 1, UPPER=float("inf"))
            torch.cuda.synchronize()
            if t >= warmup:
                for r in ctx.profile_read():
                    if r["kernel"] in per and r["launches"]:
                        per[r["kernel"]].append(r["total_ms"] * 1e3)
        ctx.profile_enable(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(pushes):
            ctx.ftle_push(f, **kw)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / pushes * 1e6
        passes.append(({k: float(np.median(v)) for k, v in per.items()}, wall))
    got = ctx.ftle_read()
    ctx.ftle_close()
    return passes, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640x480,1920x1080,3840x2160")
    ap.add_argument("--windows", default="8,30")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    lines = ["| size | window | input | pass | ftle@0 us | ftle@1 us | ftle@2 us | window x advect_field us | advect / ftle@1 | push, host us | "
             "stopped share | valid share |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    with Context(3840, 2160) as ctx:
        for w, h in sizes:
            for window in (int(v) for v in a.windows.split(",")):
                for name, speed in (("surf", 1.0), ("surf x 5", 5.0)):
                    passes, got = measure(ctx, w, h, window, speed, a.pushes, a.warmup)
                    for i, (per, wall) in enumerate(passes):
                        lines.append("| %dx%d | %d | %s | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f | %.3f | %.3f |" % (
                            w, h, window, name, i + 1, per["ftle@0"], per["ftle@1"], per["ftle@2"], per["advect_field@0"],
                            per["advect_field@0"] / per["ftle@1"], wall, got["stopped"] / (w * h), got["valid"] / (w * h)))
                    print(lines[-2], flush=True)
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
