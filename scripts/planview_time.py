"""Time of the plan view's launches (planview_kernels.hip) on one MI355X -> profiles/planview_kernel_summary.md.

    python scripts/planview_time.py [--out FILE] [--pushes 30] [--warmup 5] [--sizes 640x480:512x512,...]

Rows at 640x480 -> 512x512, 1080p -> 1024x1024, 1080p -> 2048x2048 and 4K -> 2048x2048, each through two cameras: the tilted
shore camera of the tests scaled to the size (10 m up, 20 degrees down, the plan the same 61 x 55.5 m of water, no max_gsd
cut: a scattered gather over the part of the plan the camera sees) and the identity (plan cell = pixel: the coherent gather),
and in two forms: the field alone (plan field and mask out) and field + frame with every output.  Per launch: the library's
own HIP events (rcflow_profile_read, "planview@1"), one reading per push, the median over `pushes` pushes after `warmup`, in
two passes that must agree.  Yardsticks, timed in the same run by the same events: one advect_field launch at the plan's size
(rcflow_advect_field_dev, iterations 1, UPPER +inf: the same sampler, one gather per cell) and, for the picture,
rcflow_warp_perspective_bgr_dev from the frame to the plan's size through the same map without the distortion
("framestab@9").  The bytes of a push are counted from the shapes and the seen cells: 32 (record) per cell, 32 (gather) per
seen cell, 8 + 1 out per cell; with the picture 12 in per seen cell and 3 out per cell.  planview@0 is paid once, by open; its
one reading is reported and nothing else.  Needs a GPU: there is no fallback.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ripcurrents_amd import synth                 # noqa: E402
from ripcurrents_amd.api import Context           # noqa: E402


def tilted(w, h, nx, ny):
    """the tests' camera (tests/_planview_ref.py, tilted_camera) with the focal length scaled to the image"""
    f, t = 90.0 * w / 97.0, math.radians(20.0)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    R = np.array([[1.0, 0.0, 0.0], [0.0, -math.sin(t), -math.cos(t)], [0.0, math.cos(t), -math.sin(t)]])
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    Hm = K @ np.column_stack([R[:, 0], R[:, 1], -R @ np.array([0.0, 0.0, 10.0])])
    return dict(H=Hm, fx=f, fy=f, cx=cx, cy=cy, k1=-0.12, k2=0.02, x0=-30.0, y0=-6.0, dx=61.0 / nx, dy=55.5 / ny, nx=nx, ny=ny, fps=10.0,
                max_gsd=float("inf"))


def identity(nx, ny):
    return dict(H=np.eye(3), fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, x0=0.0, y0=0.0, dx=1.0, dy=1.0, nx=nx, ny=ny, fps=1.0,
                max_gsd=float("inf"))


def median_us(ctx, kernel, call, pushes, warmup):
    per = []
    for t in range(warmup + pushes):
        ctx.profile_reset()
        call()
        torch.cuda.synchronize()
        if t >= warmup:
            per += [r["total_ms"] * 1e3 for r in ctx.profile_read() if r["kernel"] == kernel and r["launches"]]
    return float(np.median(per))


def measure(ctx, w, h, prm, pushes, warmup):
    nx, ny = prm["nx"], prm["ny"]
    U, V = synth.surf_field(w, h)
    flow = torch.as_tensor(np.ascontiguousarray(np.stack([U, V], -1), dtype=np.float32)).cuda()
    frame = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
    pf = torch.as_tensor(np.ascontiguousarray(np.stack(synth.surf_field(nx, ny), -1), dtype=np.float32)).cuda()   # the yardstick's field
    plan = torch.empty((ny, nx, 2), dtype=torch.float32, device="cuda")
    mask = torch.empty((ny, nx), dtype=torch.uint8, device="cuda")
    pic = torch.empty((ny, nx, 3), dtype=torch.uint8, device="cuda")
    summ = torch.empty(8, dtype=torch.int64, device="cuda")
    M = np.asarray(prm["H"], np.float64).reshape(3, 3) @ np.array([[prm["dx"], 0.0, prm["x0"]], [0.0, prm["dy"], prm["y0"]], [0.0, 0.0, 1.0]])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.planview_open(w, h, **prm)
    torch.cuda.synchronize()
    t0 = [r["total_ms"] * 1e3 for r in ctx.profile_read() if r["kernel"] == "planview@0" and r["launches"]][0]

    def advect():
        ctx.analysis_reset(nx, ny)                # the yardstick's particles start at their pixels
        ctx.streamline_field(pf, 1.0, 1, UPPER=float("inf"))

    passes = []
    for _ in range(2):
        passes.append(dict(
            field=median_us(ctx, "planview@1", lambda: ctx.planview_push(flow, None, plan=plan, mask=mask), pushes, warmup),
            full=median_us(ctx, "planview@1", lambda: ctx.planview_push(flow, frame, plan=plan, mask=mask, plan_bgr=pic, summary=summ), pushes, warmup),
            advect=median_us(ctx, "advect_field@0", advect, pushes, warmup),
            warp=median_us(ctx, "framestab@9", lambda: ctx.warp_perspective(frame, M, inverse_map=True, dsize=(nx, ny), out=pic), pushes, warmup)))
    ctx.profile_enable(False)
    got = ctx.planview_read()
    ctx.planview_close()
    return t0, passes, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640x480:512x512,1920x1080:1024x1024,1920x1080:2048x2048,3840x2160:2048x2048")
    a = ap.parse_args()
    sizes = [tuple(tuple(int(v) for v in s.split("x")) for s in pair.split(":")) for pair in a.sizes.split(",")]
    lines = ["| image | plan | camera | pass | planview@0 us | field alone us | all outputs us | advect_field us | field / advect | warp us | "
             "(all - field) / warp | seen share | field alone GB/s | all outputs GB/s | of 8 TB/s |", "|" + "---|" * 15]
    with Context(3840, 2160) as ctx:
        for (w, h), (nx, ny) in sizes:
            for name, prm in (("tilted", tilted(w, h, nx, ny)), ("identity", identity(nx, ny))):
                t0, passes, got = measure(ctx, w, h, prm, a.pushes, a.warmup)
                cells, seen = nx * ny, got["seen"]
                b_field = cells * 41.0 + seen * 32.0
                b_full = b_field + cells * 3.0 + seen * 12.0
                for i, p in enumerate(passes):
                    gf, ga = b_field / p["field"] * 1e-3, b_full / p["full"] * 1e-3
                    lines.append("| %dx%d | %dx%d | %s | %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f | %.2f | %.3f | %.0f | %.0f | %.1f %% |" % (
                        w, h, nx, ny, name, i + 1, t0, p["field"], p["full"], p["advect"], p["field"] / p["advect"], p["warp"],
                        (p["full"] - p["field"]) / p["warp"], seen / cells, gf, ga, ga / 80.0))
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
