"""Per-launch time of the general warps and of the multi-patch stabiliser (warp_kernels.hip, stab_kernels.hip) on one
MI355X -> profiles/framewarp_kernel_summary.md.

    python scripts/framewarp_time.py [--out FILE] [--pushes 200] [--warmup 20]

Three tables, every figure from the library's own profile records (a HIP event pair around each launch), `warmup` calls
and then `pushes` timed ones, the whole thing twice with both passes printed as the spread:
  * the multi-patch correlate + fit ("framestab@7") for n = 1, 4, 8, 16 patches of 50 x 50 on a 640 x 480 frame, beside
    the single-patch correlate ("framestab@0");
  * the affine ("framestab@8") and perspective ("framestab@9") warp at 640 x 480 and 1080p beside the translate warp
    ("framestab@1"), for a small roll + zoom (what a shaking camera gives) and a mild keystone;
  * a whole push of a four-patch similarity slot at both sizes.
These are small launches, bound by latency; a bandwidth figure is derived for the 1080p warps only.
Needs a GPU: there is no fallback.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripcurrents_amd import synth                    # noqa: E402
from ripcurrents_amd.api import Context              # noqa: E402


def _records(ctx):
    rec = {r["kernel"]: r for r in ctx.profile_read() if r["kernel"].startswith("framestab@")}
    ctx.profile_reset()
    return {k: r["total_ms"] * 1e3 / r["launches"] for k, r in rec.items()}


def _timed(ctx, call, pushes, warmup):
    for t in range(warmup):
        call(t)
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for t in range(pushes):
        call(t + 3)
    ctx.sync()
    ctx.profile_enable(False)
    return _records(ctx)


def rois_for(w, h, n, size=50):
    """n patches of size x size along the frame's border, clockwise from the top left."""
    per = (n + 3) // 4
    out = []
    for k in range(n):
        side, i = k % 4, k // 4
        f = (i + 0.5) / per if per > 1 else 0.0
        x = int(8 + f * (w - size - 16)) if side in (0, 2) else (w - size - 8 if side == 1 else 8)
        y = (8 if side == 0 else h - size - 8) if side in (0, 2) else int(8 + f * (h - size - 16))
        out.append((x, y, size, size))
    return out


def measure_push(ctx, frames, rois, model, pushes, warmup):
    n, h, w = frames.shape[:3]
    if rois is None:
        ctx.framestab_open(w, h, (8, 8, 50, 50))
    else:
        ctx.framestab_open(w, h, rois=rois, model=model)
    out = torch.empty_like(frames[0])
    res = torch.empty(3, dtype=torch.float64, device="cuda")
    per = _timed(ctx, lambda t: ctx.framestab_push(frames[t % n], out=out, result=res), pushes, warmup)
    ctx.framestab_close()
    return per


def measure_warps(ctx, frame, pushes, warmup):
    h, w = frame.shape[:2]
    out = torch.empty_like(frame)
    ang, s = math.radians(0.2), 1.003
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    A = s * np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])
    A = np.hstack([A, (c - A @ c + [1.3, -0.7])[:, None]])
    H = np.vstack([A, [2e-5, -1e-5, 1.0]])
    per = {}
    per.update(_timed(ctx, lambda t: ctx.warp_translate(frame, 1.3, -0.7, out=out), pushes, warmup))
    per.update(_timed(ctx, lambda t: ctx.warp_affine(frame, A, inverse_map=True, out=out), pushes, warmup))
    per.update(_timed(ctx, lambda t: ctx.warp_perspective(frame, H, inverse_map=True, out=out), pushes, warmup))
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("framewarp_time.py needs a GPU")
    corr, warps, push = [], [], []
    with Context(1920, 1080) as ctx:
        for w, h in ((640, 480), (1920, 1080)):
            g = synth.surf_clip(w, h, 16, device="cuda")
            frames = torch.stack([g, g, g], -1).contiguous()
            if w == 640:
                corr.append(("single-patch slot", [measure_push(ctx, frames, None, None, a.pushes, a.warmup) for _ in range(2)]))
                for n in (1, 4, 8, 16):
                    corr.append(("n = %d" % n, [measure_push(ctx, frames, rois_for(w, h, n), "similarity", a.pushes, a.warmup) for _ in range(2)]))
            warps.append((w, h, [measure_warps(ctx, frames[0], a.pushes, a.warmup) for _ in range(2)]))
            push.append((w, h, [measure_push(ctx, frames, rois_for(w, h, 4), "similarity", a.pushes, a.warmup) for _ in range(2)]))
            del g, frames
            torch.cuda.empty_cache()
    lines = ["| slot (640x480, 50x50 patches) | correlate launch | correlate µs (pass 1 / pass 2) | warp launch | warp µs (pass 1 / pass 2) |",
             "|---|---|---|---|---|"]
    for name, p in corr:
        ck, wk = ("framestab@0", "framestab@1") if "framestab@0" in p[0] else ("framestab@7", "framestab@8")
        lines.append("| %s | %s | %.1f / %.1f | %s | %.1f / %.1f |" % (name, ck, p[0][ck], p[1][ck], wk, p[0][wk], p[1][wk]))
    lines += ["", "| frame | translate µs (framestab@1) | affine µs (framestab@8) | perspective µs (framestab@9) | bytes read + written | "
              "affine GB/s | perspective GB/s |", "|---|---|---|---|---|---|---|"]
    for w, h, p in warps:
        mb = 6e-6 * w * h
        rate = (lambda us: "%.0f" % (mb * 1e6 / (us * 1e-6) / 1e9)) if w == 1920 else (lambda us: "-")
        lines.append("| %dx%d | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.2f MB | %s | %s |" % (
            w, h, p[0]["framestab@1"], p[1]["framestab@1"], p[0]["framestab@8"], p[1]["framestab@8"], p[0]["framestab@9"],
            p[1]["framestab@9"], mb, rate(p[0]["framestab@8"]), rate(p[0]["framestab@9"])))
    lines += ["", "| frame | whole push, 4 patches + similarity: correlate + fit µs | warp µs | sum µs (pass 1 / pass 2) |", "|---|---|---|---|"]
    for w, h, p in push:
        lines.append("| %dx%d | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f |" % (
            w, h, p[0]["framestab@7"], p[1]["framestab@7"], p[0]["framestab@8"], p[1]["framestab@8"],
            p[0]["framestab@7"] + p[0]["framestab@8"], p[1]["framestab@7"] + p[1]["framestab@8"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
