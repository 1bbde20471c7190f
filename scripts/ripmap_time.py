"""Time of one opposing-flow-map push (ripmap_kernels.hip) on one MI355X, beside the two existing calls it replaces
-> profiles/ripmap_kernel_summary.md.

    python scripts/ripmap_time.py [--out FILE] [--pushes 200] [--warmup 20] [--quick]

640x480 and 1080p, 30 x 30 cells, windows 10 and 300.  The ring is filled and wrapped before anything is timed (window +
warmup pushes over 16 distinct flow fields).  Per launch: the library's own HIP events (rcflow_profile_read: "ripmap@0" =
ring, mean, cell sums, colour and the finish; "ripmap@1" = the mask).  Per push as a caller sees it: host clock over
`pushes` pushes ending in one synchronise, for the session (colour only, and colour + mask + cells) and for the separate
calls: rcflow_window_mean_dev on a caller-owned ring followed by rcflow_vector_to_color_dev, which synchronises in every
call to hand its maximum back.  The separate calls produce no cell grid at all.  The whole thing runs twice and both
passes are printed, as the spread.
Bytes per pixel as built: flow 8 + slot 8 in, slot 8 out, mean 8 in / 8 out, colour 3 = 43.  What a push touches again
and again is the mean, the 16 fields and the images; of the ring it touches one slot, each slot once per `window`
pushes.  At 640x480 mean and slot are 2.5 MB each and at window 10 the whole ring is 25 MB: all of it sits in the 256 MiB
Infinity Cache, so those rates are cache rates and no fraction of the HBM copy rate is printed for them.
Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripcurrents_amd.api import Context              # noqa: E402

COPY_TBS = 5.2            # scripts/diag/membw copy rate on these devices
CACHE_BYTES = 256 << 20   # Infinity Cache
NFIELDS = 16


def flow_fields(w, h):
    g = torch.Generator(device="cuda").manual_seed(1)
    y, x = torch.meshgrid(torch.arange(h, device="cuda").float(), torch.arange(w, device="cuda").float(), indexing="ij")
    out = []
    for t in range(NFIELDS):
        f = torch.stack([torch.sin(x / 37 + 0.3 * t) + 0.8, torch.cos(y / 29 - 0.2 * t)], -1) * 2
        out.append((f + 0.3 * torch.randn((h, w, 2), device="cuda", generator=g)).contiguous())
    return out


def session(ctx, fields, window, pushes, warmup, full):
    h, w = fields[0].shape[:2]
    ctx.ripmap_open(w, h, window, (30, 30))
    hsv = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    kw = dict(hsv=hsv)
    if full:
        kw.update(mask=torch.empty((h, w), dtype=torch.uint8, device="cuda"),
                  cells=torch.empty((30, 30, 4), dtype=torch.float32, device="cuda"),
                  summary=torch.empty(8, dtype=torch.float64, device="cuda"))
    for t in range(window + warmup):
        ctx.ripmap_push(fields[t % NFIELDS], **kw)
    ctx.sync()
    t0 = time.perf_counter()
    for t in range(pushes):
        ctx.ripmap_push(fields[(t + 7) % NFIELDS], **kw)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e6 / pushes
    ctx.profile_reset()
    ctx.profile_enable(True)
    for t in range(pushes):
        ctx.ripmap_push(fields[(t + 7) % NFIELDS], **kw)
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r for r in ctx.profile_read()}
    ctx.profile_reset()
    ctx.ripmap_close()
    k0 = rec["ripmap@0"]["total_ms"] * 1e3 / pushes
    k1 = rec["ripmap@1"]["total_ms"] * 1e3 / pushes if "ripmap@1" in rec else 0.0
    return wall, k0, k1, rec["ripmap@0"]["alg_bytes"] / pushes


def separate(ctx, fields, window, pushes, warmup):
    """rcflow_window_mean_dev + rcflow_vector_to_color_dev, the caller owning the ring."""
    h, w = fields[0].shape[:2]
    ring = torch.zeros((window, h, w, 2), dtype=torch.float32, device="cuda")
    avg = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    md = 1e-6
    for t in range(window + warmup):
        ctx.window_mean(avg, ring[t % window], fields[t % NFIELDS], window)
        _, md = ctx.vectorToColor(avg, md)
    ctx.sync()
    t0 = time.perf_counter()
    for t in range(pushes):
        ctx.window_mean(avg, ring[(t + warmup) % window], fields[(t + 7) % NFIELDS], window)
        _, md = ctx.vectorToColor(avg, md)           # allocates its image and synchronises, as the entry point does
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e6 / pushes
    # the two device parts on their own, by events
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for t in range(pushes):
        ctx.window_mean(avg, ring[(t + warmup) % window], fields[(t + 7) % NFIELDS], window)
    e[1].record()
    ctx.sync()
    wm = e[0].elapsed_time(e[1]) * 1e3 / pushes
    del ring
    return wall, wm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="640x480, window 10 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ripmap_time.py needs a GPU")
    sizes = [(640, 480)] if a.quick else [(640, 480), (1920, 1080)]
    windows = [10] if a.quick else [10, 300]
    lines = ["| size | window | ring | ripmap@0 µs (pass 1 / 2) | bytes / time | of %.1f TB/s | ripmap@1 µs | push, colour only: host µs "
             "| push, colour + mask + cells: host µs | window_mean + vector_to_color: host µs (pass 1 / 2) | window_mean alone: device µs |" % COPY_TBS,
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    with Context(1920, 1080) as ctx:
        for w, h in sizes:
            fields = flow_fields(w, h)
            for window in windows:
                p = []
                for _ in range(2):
                    s0 = session(ctx, fields, window, a.pushes, a.warmup, full=False)
                    s1 = session(ctx, fields, window, a.pushes, a.warmup, full=True)
                    sep = separate(ctx, fields, window, a.pushes, a.warmup)
                    torch.cuda.empty_cache()
                    p.append((s0, s1, sep))
                ring = window * ((w + 1) & ~1) * h * 8
                k0 = min(x[0][1] for x in p)
                by = p[0][0][3]
                cached = ring + 2 * w * h * 8 + NFIELDS * w * h * 8 <= CACHE_BYTES
                lines.append("| %dx%d | %d | %.0f MB%s | %.1f / %.1f | %.2f TB/s | %s | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f | %.1f / %.1f |" % (
                    w, h, window, ring / 1e6, " (cache)" if cached else "", p[0][0][1], p[1][0][1], by / k0 / 1e6,
                    "-" if cached else "%.0f %%" % (100 * by / k0 / 1e6 / COPY_TBS), p[0][1][2], p[1][1][2],
                    p[0][0][0], p[1][0][0], p[0][1][0], p[1][1][0], p[0][2][0], p[1][2][0], p[0][2][1], p[1][2][1]))
            del fields
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
