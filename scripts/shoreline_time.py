"""Time of the launches of a shoreline push (shoreline_kernels.hip) on one MI355X -> profiles/shoreline_kernel_summary.md.

    python scripts/shoreline_time.py [--out FILE] [--pushes 30] [--warmup 5] [--size 1920x1080] [--radius 2] [--lines 128]
                                     [--samples 512] [--window 512]

The synthetic beach of tests/_shoreline_ref.py (four pictures, alternating), RMB.  Per launch: the library's own HIP events
(rcflow_profile_read, "shoreline@0".."shoreline@3"), one reading per push, the median over `pushes` pushes after `warmup`, in two
passes, once with every output and once without the pictures (no mask, plane or histogram: no shoreline@3).  Beside shoreline@0
stand the bytes it cannot avoid (the picture 3 B/px in, the plane 2 B/px out), the time those bytes take at the rate a
device-to-device copy of the same size reaches here, and kinematics@0 at the same size (R 3, s 2, 32 x 18 cells, mask and records):
the nearest kernel of the same shape, a two-pass LDS stencil that ends in a ticket.  Before anything is timed the first push is
held to the numpy statement, bit for bit: at 1080p a block walks two tiles, which no test of the suite reaches (none is larger
than 640 x 360).  Per push as a caller sees it: a host clock over the window ending in one synchronise, profiling off.  Needs a
GPU: there is no fallback.
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
import _shoreline_ref as S                                           # noqa: E402
from ripcurrents_amd.api import SHORELINE_DTYPE, Context             # noqa: E402

NAMES = ["shoreline@%d" % k for k in range(4)]


def events(ctx, push, pushes, warmup, names):
    per = {k: [] for k in names}
    ctx.profile_enable(True)
    for t in range(warmup + pushes):
        ctx.profile_reset()
        push(t)
        torch.cuda.synchronize()
        if t >= warmup:
            for r in ctx.profile_read():
                if r["kernel"] in per and r["launches"]:
                    per[r["kernel"]].append(r["total_ms"] * 1e3)
    ctx.profile_enable(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(pushes):
        push(t)
    torch.cuda.synchronize()
    return {k: float(np.median(v)) if v else 0.0 for k, v in per.items()}, (time.perf_counter() - t0) / pushes * 1e6


def copy_rate(nbytes, reps=30):
    """bytes read plus bytes written per second of a device-to-device copy of nbytes"""
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps + 5):
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 2.0 * nbytes / (float(np.median(ms[5:])) * 1e-3)


def measure(ctx, w, h, r, L, n, T, pushes, warmup):
    lines = [(0.05 * w, (i + 0.5) * h / L, 0.95 * w, (i + 0.5) * h / L, n) for i in range(L)]
    p = S.Params(radius=r, window=T, permille=20, max_jump=max(8.0, 2.0 * h / L))
    host = [S.beach(w, h, t, amp=0.02 * w) for t in range(4)]
    imgs = [torch.as_tensor(a).cuda() for a in host]
    ctx.shoreline_open(w, h, lines, **p.kw())
    every = dict(records=torch.empty(L * 64, dtype=torch.uint8, device="cuda"), summary=torch.empty(8, dtype=torch.int64, device="cuda"),
                 mask=torch.empty((h, w), dtype=torch.uint8, device="cuda"), plane=torch.empty((h, w), dtype=torch.int16, device="cuda"),
                 hist=torch.empty(512, dtype=torch.int32, device="cuda"))
    few = {k: every[k] for k in ("records", "summary")}
    # the statement first
    ref = S.ShorelineRef(w, h, lines, p)
    want = ref.push(host[0])
    ctx.shoreline_push(imgs[0], **every)
    got = {k: v.cpu().numpy() for k, v in every.items()}
    assert got["records"].view(SHORELINE_DTYPE).tobytes() == want["records"].tobytes() and np.array_equal(got["summary"], want["summary"])
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["plane"].view(np.uint16), want["plane"])
    assert np.array_equal(got["hist"].view(np.uint32), want["hist"])
    ctx.shoreline_reset()
    px = float(w * h)
    rows = []
    for name, kw in (("every output", every), ("records and summary", few)):
        for k in range(2):
            us, wall = events(ctx, lambda t: ctx.shoreline_push(imgs[t % 4], **kw), pushes, warmup, NAMES)
            rows.append((name, k + 1) + tuple(us[q] for q in NAMES) + (wall,))
    rec, summ = ctx.shoreline_read()
    assert summ["positions"] == L and 240 <= summ["thr"] <= 270
    state = ctx.shoreline_info()["device_bytes"]
    ctx.shoreline_close()
    # the yardsticks: the copy rate at the size of shoreline@0's bytes, and kinematics@0
    rate = copy_rate(int(2.5 * px))
    flow = torch.as_tensor(np.random.default_rng(1).standard_normal((h, w, 2)).astype(np.float32) * 0.1).cuda()
    ctx.kinematics_open(w, h, radius=3, sigma=1.5, spacing=2, grid_x=32, grid_y=18, scale=25.0, pixel_area=0.01, ow_k=0.2, min_core=8, vis_max=5.0)
    kk = dict(mask=torch.empty((h, w), dtype=torch.uint8, device="cuda"), cells=torch.empty(32 * 18 * 48, dtype=torch.uint8, device="cuda"))
    kus, _ = events(ctx, lambda t: ctx.kinematics_push(flow, **kk), pushes, warmup, ["kinematics@0"])
    ctx.kinematics_close()
    return state, rows, 5.0 * px, rate, kus["kinematics@0"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--lines", type=int, default=128)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--window", type=int, default=512)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    out = ["| size | r | lines x n | T | state MB | outputs | pass | @0 us | @1 us | @2 us | @3 us | push, host us |", "|" + "---|" * 12]
    with Context(3840, 2160) as ctx:
        state, rows, b0, rate, kn0 = measure(ctx, w, h, a.radius, a.lines, a.samples, a.window, a.pushes, a.warmup)
        for r in rows:
            out.append("| %dx%d | %d | %d x %d | %d | %.1f | %s | %d | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
                (w, h, a.radius, a.lines, a.samples, a.window, state / 1e6) + r))
    out.append("")
    out.append("shoreline@0: %.1f MB it cannot avoid; a device-to-device copy moves bytes at %.2f TB/s here (read plus written), which is %.1f us "
               "for them; kinematics@0 at the same size (R 3, s 2, 32 x 18 cells, mask and records): %.1f us." % (b0 / 1e6, rate / 1e12, b0 / rate * 1e6, kn0))
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
