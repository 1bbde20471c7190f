"""Time of the launches of a transects push (transects_kernels.hip) on one MI355X -> profiles/transects_kernel_summary.md.

    python scripts/transects_time.py [--out FILE] [--pushes 30] [--warmup 5] [--size 1920x1080] [--lines 64] [--samples 1024]
                                     [--window 256] [--range 16] [--lag 1]

Random frames and fields, both sources, horizontal lines spread over the picture.  The ring is filled first (`window` pushes
with no output), so that every timed push takes a pair off the accumulators as well as adding one, and every computing push
averages a full window.  Per launch: the library's own HIP events (rcflow_profile_read, "transects@0".."transects@2"), one
reading per push, the median over `pushes` pushes after `warmup`, in two passes, every output requested.  Beside each launch
stand the bytes it cannot avoid at the 5.9 TB/s a streaming read reaches on this card (profiles/planview_kernel_summary.md):
  @0  per sample the four pixels of the frame (4 bytes) and of the field (32), the ring entries out (1 + 8), and with a
      correlation range the three older grey rows in (3); the accumulators in and out;
  @1  the flow ring once (8 bytes per sample and held row), the profile out;
  @2  both rings once, both pictures out (1 + 3 bytes per sample and row of the window).
Per push as a caller sees it: a host clock over the window ending in one synchronise, profiling off, once with every output
NULL and once with every output asked for.  Needs a GPU: there is no fallback.
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

HBM = 5.9e12                                      # bytes per second of a streaming read on this card


def floors(S, L, T, D):
    nw = 3 * (2 * D + 1) + 2
    b0 = S * (4 + 32 + 9 + (3 if D else 0)) + (16 * L * nw if D else 0)
    b1 = S * 8 * T + S * 8
    b2 = S * T * (1 + 8 + 1 + 3)
    return [b / HBM * 1e6 for b in (b0, b1, b2)]


def measure(ctx, w, h, L, n, T, D, lag, pushes, warmup):
    rng = np.random.default_rng(1)
    gray = [torch.as_tensor(rng.integers(0, 256, (h, w), dtype=np.uint8)).cuda() for _ in range(5)]
    flow = [torch.as_tensor(rng.normal(0, 1, (h, w, 2)).astype(np.float32)).cuda() for _ in range(5)]
    lines = [(8.0, 4.0 + k * (h - 9.0) / max(L - 1, 1), w - 9.0, 4.0 + k * (h - 9.0) / max(L - 1, 1), n) for k in range(L)]
    ctx.transects_open(w, h, lines, window=T, lag=lag, range=D, fps=25.0, metres_per_pixel=0.1, jet_min=0.5, vis_max=5.0)
    info = ctx.transects_info()
    S = info["samples"]
    kw = dict(records=torch.empty(L * 64, dtype=torch.uint8, device="cuda"), sums=torch.empty(L * 16, dtype=torch.int64, device="cuda"),
              profile=torch.empty(S * 2, dtype=torch.float32, device="cuda"), stack=torch.empty((T, S), dtype=torch.uint8, device="cuda"),
              hov=torch.empty((T, S, 3), dtype=torch.uint8, device="cuda"), summary=torch.empty(8, dtype=torch.int64, device="cuda"))
    for t in range(T):
        ctx.transects_push(gray[t % 5], flow[t % 5])
    passes = []
    for _ in range(2):
        per = {"transects@%d" % k: [] for k in range(3)}
        ctx.profile_enable(True)
        for t in range(warmup + pushes):
            ctx.profile_reset()
            ctx.transects_push(gray[t % 5], flow[t % 5], **kw)
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
                ctx.transects_push(gray[t % 5], flow[t % 5], **out)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / pushes * 1e6)
        passes.append(({k: float(np.median(v)) for k, v in per.items()}, wall))
    got = ctx.transects_read()[1]
    assert got["held"] == T and got["pairs"] == (T - lag if D else 0) and got["bad"] == 0
    ctx.transects_close()
    return S, info["device_bytes"], passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--range", type=int, default=16)
    ap.add_argument("--lag", type=int, default=1)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    lines = ["| size | lines x samples | T / D / lag | state MB | pass | @0 us | @0 bytes floor us | @1 us | @1 bytes floor us | @2 us | @2 bytes floor us | "
             "push, no output, host us | push, every output, host us |", "|" + "---|" * 13]
    with Context(3840, 2160) as ctx:
        S, state, passes = measure(ctx, w, h, a.lines, a.samples, a.window, a.range, a.lag, a.pushes, a.warmup)
        f = floors(S, a.lines, a.window, a.range)
        for i, (per, wall) in enumerate(passes):
            lines.append("| %dx%d | %d x %d | %d / %d / %d | %.0f | %d | %.1f | %.2f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
                w, h, a.lines, a.samples, a.window, a.range, a.lag, state / 1e6, i + 1, per["transects@0"], f[0], per["transects@1"], f[1],
                per["transects@2"], f[2], wall[0], wall[1]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
