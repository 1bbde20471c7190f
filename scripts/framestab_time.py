"""Per-launch time of the frame-stabilisation kernels (stab_kernels.hip) on one MI355X -> profiles/framestab_kernel_summary.md.

    python scripts/framestab_time.py [--out FILE] [--pushes 200] [--warmup 20]

640x480 and 1080p frames, patches of 50x50 (the reference's), 64x64, 96x96 (the largest square the one-workgroup
correlation holds in LDS), 128x128 and 256x256 (a launch per pass).  After `warmup` pushes, `pushes` pushes are timed per
launch with the library's own HIP events (rcflow_profile_read: "framestab@0" the correlation as one workgroup,
"framestab@1" the warp, "framestab@2..6" the passes of the large form).  The whole thing runs twice and both passes are
printed, as the spread.  These are times of small launches, bound by latency: no rate is derived from them.
Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripcurrents_amd import synth                    # noqa: E402
from ripcurrents_amd.api import Context              # noqa: E402


def measure(ctx, frames, patch, pushes, warmup):
    n, h, w = frames.shape[:3]
    ctx.framestab_open(w, h, (w - patch - 8, 8, patch, patch))
    out = torch.empty_like(frames[0])
    res = torch.empty(3, dtype=torch.float64, device="cuda")
    for t in range(warmup):
        ctx.framestab_push(frames[t % n], out=out, result=res)
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for t in range(pushes):
        ctx.framestab_push(frames[(t + 3) % n], out=out, result=res)
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r for r in ctx.profile_read() if r["kernel"].startswith("framestab@")}
    ctx.profile_reset()
    info = ctx.framestab_info()
    ctx.framestab_close()
    per = {k: r["total_ms"] * 1e3 / r["launches"] for k, r in rec.items()}
    warp = per.pop("framestab@1")
    return sum(per.values()), warp, len(per), info["dft_size"], sum(r["alg_bytes"] for k, r in rec.items() if k != "framestab@1") / pushes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("framestab_time.py needs a GPU")
    rows = []
    with Context(1920, 1080) as ctx:
        for w, h in ((640, 480), (1920, 1080)):
            g = synth.surf_clip(w, h, 16, device="cuda")
            frames = torch.stack([g, g, g], -1).contiguous()
            for patch in (50, 64, 96, 128, 256):
                passes = [measure(ctx, frames, patch, a.pushes, a.warmup) for _ in range(2)]
                rows.append((w, h, patch, passes))
            del g, frames
            torch.cuda.empty_cache()
    lines = ["| frame | patch | DFT size | correlate launches | correlate bytes as built | correlate µs per push (pass 1 / pass 2) "
             "| warp bytes | warp µs (pass 1 / pass 2) |", "|---|---|---|---|---|---|---|---|"]
    for w, h, patch, passes in rows:
        lines.append("| %dx%d | %dx%d | %dx%d | %d | %.1f KB | %.1f / %.1f | %.2f MB | %.1f / %.1f |" % (
            w, h, patch, patch, passes[0][3][0], passes[0][3][1], passes[0][2], passes[0][4] / 1e3, passes[0][0], passes[1][0],
            6e-6 * w * h, passes[0][1], passes[1][1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
