"""Time of one tracer-session push (tracer_kernels.hip, draw_kernels.hip) on one MI355X, beside the host classes it
replaces, and of the drawing stage alone -> profiles/tracers_kernel_summary.md.

    python scripts/tracers_time.py [--out FILE] [--pushes 100] [--warmup 10] [--quick]

Session: the reference's scene (five streaklines, two timelines, a cloud of 12) at 640x480 and 1080p, LK mover on a surf
clip of 8 frames cycled, FLOW mover on a smooth field; streakline rings of 64, filled before anything is timed (64 +
warmup pushes).  Per launch: the library's own HIP events (rcflow_profile_read: "trackstab@1..3" pyramid, Scharr, track;
"advect_points@0"; "tracers@0" book-keeping and primitives; "tracers@1" draw).  Per push as a caller sees it: a host clock
over `pushes` pushes ending in one synchronise, profiling off, for the session and for the host classes (Streakline.runLK
/ Timeline.runLK / PopulationMap.runLK, or Streakline.run), which synchronise once per object and push and draw nothing.
Stage: rcflow_draw_dev at 1080p, 8UC3, over n = 256 .. 65 536 random short primitives (discs of radius 2-10, thin and
thick lines up to 40 px): the unit is microseconds per launch; work is tiles x n box tests, not bytes.  The whole
thing runs twice and both passes are printed, as the spread.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripcurrents_amd import synth                                                             # noqa: E402
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, Context, PopulationMap, Streakline, Timeline  # noqa: E402

RING = 64


def scene(ctx, w, h, only_streaks):
    host = []
    for i in range(5):
        p = (w * (i + 1) / 6.0, h / 2.0 + 9 * i)
        ctx.tracers_add_streakline(p)
        host.append(Streakline(p))
    if only_streaks:
        return host
    for a, b, n in [((w * 0.2, h * 0.25), (w * 0.8, h * 0.3), 9), ((w * 0.3, h * 0.8), (w * 0.35, h * 0.2), 6)]:
        ctx.tracers_add_timeline(a, b, n)
        host.append(Timeline(a, b, n))
    rect = ((w * 0.15, h * 0.15), (w * 0.45, h * 0.4))
    ctx.tracers_add_cloud(rect[0], rect[1], 12, rng=np.random.RandomState(5))
    host.append(PopulationMap(rect[0], rect[1], 12, rng=np.random.RandomState(5)))
    return host


def session(ctx, w, h, mover, frames, pushes, warmup):
    ctx.tracers_open(w, h, mover, max_lines=8, max_vertices=RING, dt=1.0)
    host = scene(ctx, w, h, mover == "flow")
    canvas = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    kw = (lambda t: dict(gray=frames[t % len(frames)])) if mover == "lk" else (lambda t: dict(flow=frames[t % len(frames)]))
    for t in range(RING + warmup):
        ctx.tracers_push(canvas=canvas, **kw(t))
    ctx.sync()
    t0 = time.perf_counter()
    for t in range(pushes):
        ctx.tracers_push(canvas=canvas, **kw(t))
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e6 / pushes
    ctx.profile_reset()
    ctx.profile_enable(True)
    for t in range(pushes):
        ctx.tracers_push(canvas=canvas, **kw(t))
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r["total_ms"] * 1e3 / pushes for r in ctx.profile_read() if r["launches"]}
    ctx.profile_reset()
    info = ctx.tracers_info()
    ctx.tracers_close()
    # the host classes, their streaklines cut to the ring's length so that both sides move the same number of vertices
    for o in host:
        if isinstance(o, Streakline):
            o.vertices = [o.generationPoint] * RING
    t0 = time.perf_counter()
    n = max(pushes // 10, 3)
    for t in range(n):
        for o in host:
            if mover == "lk":
                o.runLK(ctx, frames[t % len(frames)], frames[(t + 1) % len(frames)])
            else:
                o.run(ctx, frames[t % len(frames)], w, h)
            if isinstance(o, Streakline):
                o.vertices = o.vertices[:RING]
    ctx.sync()
    host_wall = (time.perf_counter() - t0) * 1e6 / n
    return wall, rec, info, host_wall


def stage(ctx, w, h, n, reps):
    rng = np.random.RandomState(n)
    p = np.zeros(n, DRAW_PRIM_DTYPE)
    p["kind"] = rng.choice([1, 2], n)
    p["x0"], p["y0"] = rng.randint(0, w, n), rng.randint(0, h, n)
    p["x1"], p["y1"] = p["x0"] + rng.randint(-40, 41, n), p["y0"] + rng.randint(-40, 41, n)
    p["size"] = np.where(p["kind"] == 1, rng.randint(2, 11, n), rng.choice([1, 1, 2, 4], n))
    p["color"] = rng.randint(0, 2 ** 24, n)
    p["flags"] = rng.rand(n) < 0.2
    d = torch.from_numpy(p.view(np.uint8).reshape(-1)).cuda()
    img = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        ctx.draw(img, d)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(reps):
        ctx.draw(img, d)
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r["total_ms"] * 1e3 / reps for r in ctx.profile_read() if r["launches"]}
    ctx.profile_reset()
    return rec["tracers@1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--pushes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes = [(640, 480)] if a.quick else [(640, 480), (1920, 1080)]
    lines = ["| size | mover | vertices | primitives | push: host µs | host classes: host µs | launches: µs per push |", "|---|---|---|---|---|---|---|"]
    stage_lines = ["| primitives | tracers@1 µs (pass 1 / 2) |", "|---|---|"]
    with Context(1920, 1080) as ctx:
        rows, srows = {}, {}
        for _ in range(2):
            for (w, h) in sizes:
                clip = [torch.as_tensor(f).cuda() for f in synth.surf_clip(w, h, 8, seed=5)]
                y, x = torch.meshgrid(torch.arange(h, device="cuda").float(), torch.arange(w, device="cuda").float(), indexing="ij")
                field = [torch.stack([2.5 * torch.sin(x / 31 + 0.4 * t) + 1.5, 2 * torch.cos(y / 27 - 0.3 * t) - 0.5], -1).contiguous()
                         for t in range(4)]
                for mover, frames in (("lk", clip), ("flow", field)):
                    wall, rec, info, host_wall = session(ctx, w, h, mover, frames, a.pushes, a.warmup)
                    rows.setdefault((w, h, mover), []).append((wall, rec, info, host_wall))
            for n in ([256, 4096] if a.quick else [256, 4096, 16384, 65536]):
                srows.setdefault(n, []).append(stage(ctx, 1920, 1080, n, 20))
        for (w, h, mover), r in rows.items():
            k = ", ".join("%s %s" % (name, " / ".join("%.1f" % p[1].get(name, 0.0) for p in r)) for name in sorted(r[0][1]))
            lines.append("| %dx%d | %s | %d | %d | %s | %s | %s |" % (w, h, mover, r[0][2]["points"], r[0][2]["prims"],
                         " / ".join("%.1f" % p[0] for p in r), " / ".join("%.1f" % p[3] for p in r), k))
        for n, r in srows.items():
            stage_lines.append("| %d | %s |" % (n, " / ".join("%.1f" % v for v in r)))
    text = "\n".join(lines) + "\n\n" + "\n".join(stage_lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
