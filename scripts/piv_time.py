"""Time of the launches of an ensemble-PIV push (piv_kernels.hip) on one MI355X -> profiles/piv_kernel_summary.md.

    python scripts/piv_time.py [--out FILE] [--pushes 30] [--warmup 5] [--size 1920x1080] [--window 32] [--range 8] [--step 16]
                               [--ensembles 1,16]

Random frames, every output requested.  Per launch: the library's own HIP events (rcflow_profile_read, "piv@0".."piv@2"), one
reading per push, the median over `pushes` pushes after `warmup`, in two passes.  Beside piv@0 stand the two floors it is held
against, neither a measurement of this kernel:
  issue   cells * D^2 * M^2 / 4 v_dot4_u32_u8 per lane plus three v_alignbyte_b32 per four of them, at a wave64 vector
          instruction per two cycles and SIMD, four SIMDs in each of 256 CUs, 2.4 GHz;
  bytes   the accumulator update: per word of a cell 8 bytes written (ensemble 1), or 8 read and 8 written plus the ring
          slot's 4 read and 4 written, at the 5.9 TB/s a streaming read reaches on this card (profiles/planview_kernel_summary.md).
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

LANES_PER_SECOND = 256 * 4 * 32 * 2.4e9           # vector lane-operations: 256 CUs, 4 SIMDs, a wave64 instruction per 2 cycles
HBM = 5.9e12                                      # bytes per second of a streaming read on this card


def floors(cells, M, R, E):
    D = 2 * R + 1
    dot4 = cells * D * D * M * M / 4.0
    issue = (dot4 + 0.75 * dot4) / LANES_PER_SECOND * 1e6
    words = cells * (3 * D * D + 2)
    byts = words * (24.0 if E > 1 else 8.0) / HBM * 1e6
    return issue, byts


def measure(ctx, w, h, M, R, step, E, pushes, warmup):
    rng = np.random.default_rng(1)
    frames = [torch.as_tensor(rng.integers(0, 256, (h, w), dtype=np.uint8)).cuda() for _ in range(5)]
    ctx.piv_open(w, h, window=M, range=R, step=step, ensemble=E)
    info = ctx.piv_info()
    gx, gy = info["grid_x"], info["grid_y"]
    kw = dict(cells=torch.empty(gy * gx * 32, dtype=torch.uint8, device="cuda"), field=torch.empty((gy, gx, 2), dtype=torch.float32, device="cuda"),
              vis=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"), summary=torch.empty(8, dtype=torch.int64, device="cuda"))
    passes = []
    for _ in range(2):
        per = {"piv@%d" % k: [] for k in range(3)}
        ctx.profile_enable(True)
        for t in range(warmup + pushes):
            ctx.profile_reset()
            ctx.piv_push(frames[t % 5], **kw)
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
                ctx.piv_push(frames[t % 5], **out)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / pushes * 1e6)
        passes.append(({k: float(np.median(v)) for k, v in per.items()}, wall))
    got = ctx.piv_read()[1]
    assert got["cells"] == gx * gy and got["pairs"] == E and got["lowpeak"] == gx * gy      # noise: no cell passes
    ctx.piv_close()
    return gx, gy, info["device_bytes"], passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--range", type=int, default=8)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--ensembles", default="1,16")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    lines = ["| size | M / R / step | cells | E | state MB | pass | piv@0 us | issue floor us | piv@0 / issue | bytes floor us | piv@0 / (issue + bytes) | "
             "piv@1 us | piv@2 us | push, no output, host us | push, every output, host us |", "|" + "---|" * 15]
    with Context(3840, 2160) as ctx:
        for E in (int(v) for v in a.ensembles.split(",")):
            gx, gy, state, passes = measure(ctx, w, h, a.window, a.range, a.step, E, a.pushes, a.warmup)
            issue, byts = floors(gx * gy, a.window, a.range, E)
            for i, (per, wall) in enumerate(passes):
                lines.append("| %dx%d | %d / %d / %d | %d x %d | %d | %.0f | %d | %.1f | %.1f | %.2f | %.1f | %.2f | %.1f | %.1f | %.1f | %.1f |" % (
                    w, h, a.window, a.range, a.step, gx, gy, E, state / 1e6, i + 1, per["piv@0"], issue, per["piv@0"] / issue, byts,
                    per["piv@0"] / (issue + byts), per["piv@1"], per["piv@2"], wall[0], wall[1]))
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
