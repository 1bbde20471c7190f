"""Time of one rip-tracks push (track_kernels.hip) on one MI355X, beside the regions push that feeds it and the only route
there was before it: the label image, the records and the summary copied to the host, the association there, the confirmed
mask copied back -> profiles/tracks_kernel_summary.md.

    python scripts/tracks_time.py [--out FILE] [--pushes 50] [--warmup 5] [--quick]

Rows at 640x480, 1080p and 4K for: a natural mask (thresholded smooth noise, 45 % foreground, 8-connectivity, min_area 16),
the full mask (one region over the whole frame on one track: every pixel meets on one word of the overlap table) and a
checkerboard at 4-connectivity (every pixel its own component, almost every label above R; the first 1024 labels are as many
distinct pairs per row as there are pixels).  Every row alternates two inputs, the mask and the mask moved by two pixels (the
checkerboard: by one, its inverse), so that regions move, overlap, split and merge; both are labelled once by
rcflow_regions_push_dev and the tracks read those device outputs.  Per launch: the library's own HIP events
(rcflow_profile_read, "tracks@0".."tracks@5") summed over a window of `pushes` pushes.  Per push as a caller sees it: a host
clock over the window ending in one synchronise, profiling off; the regions push at the same size the same way, in the same
run.  Host route: labels, records and summary .cpu(), the numpy statement of tests/_tracks_ref.py, .cuda() of the mask, timed
per push with a synchronise.  The whole thing runs twice and both passes are printed, as the spread.  Needs a GPU: there is
no fallback.
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
from ripcurrents_amd.api import REGION_DTYPE, Context      # noqa: E402
import _tracks_ref as T                                   # noqa: E402

MAX_REGIONS, MAX_TRACKS = 1024, 64
PRM = dict(max_regions=MAX_REGIONS, max_tracks=MAX_TRACKS, min_overlap=4, max_misses=2, min_hits=3)


def smooth_noise(h, w, seed, thresh=0.55):
    rng = np.random.RandomState(seed)
    f = np.fft.rfft2(rng.rand(h, w).astype(np.float32))
    ky, kx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    g = np.fft.irfft2(f * np.exp(-(kx * kx + ky * ky) * (2 * np.pi * 6.0) ** 2 / 2), (h, w))
    return np.where(g > np.quantile(g, thresh), 255, 0).astype(np.uint8)


def window(push, sync, pushes, warmup):
    for i in range(warmup):
        push(i)
    sync()
    t0 = time.perf_counter()
    for i in range(pushes):
        push(i)
    sync()
    return (time.perf_counter() - t0) * 1e6 / pushes


def host_route(ctx, inputs, reps, prm):
    """what a host had to do per frame without rcflow_tracks_*"""
    h, w = inputs[0][0].shape
    ref = T.Tracks(w, h, **prm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        labels, regions, summary = inputs[i % 2]
        out = ref.push(labels.cpu().numpy(), regions.cpu().numpy().view(REGION_DTYPE), int(summary.cpu()[2]))
        torch.as_tensor(out["mask_out"]).cuda()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def one(ctx, masks, conn, min_area, pushes, warmup, prm):
    h, w = masks[0].shape
    ctx.regions_open(w, h, conn, min_area, MAX_REGIONS)
    dmasks = [torch.as_tensor(m).cuda() for m in masks]
    inputs = [(torch.empty((h, w), dtype=torch.int32, device="cuda"), torch.empty(MAX_REGIONS * 144, dtype=torch.uint8, device="cuda"),
               torch.empty(8, dtype=torch.int64, device="cuda")) for _ in masks]

    def regions_push(i):
        ctx.regions_push(dmasks[i % 2], labels=inputs[i % 2][0], regions=inputs[i % 2][1], summary=inputs[i % 2][2])

    regions_wall = window(regions_push, ctx.sync, pushes, warmup)
    ctx.regions_close()
    ctx.tracks_open(w, h, **prm)
    conf = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    tab = torch.empty(prm["max_tracks"] * 128, dtype=torch.uint8, device="cuda")

    def tracks_push(i):
        ctx.tracks_push(*inputs[i % 2], tracks=tab, mask_out=conf)

    wall = window(tracks_push, ctx.sync, pushes, warmup)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for i in range(pushes):
        tracks_push(i)
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r["total_ms"] * 1e3 / pushes for r in ctx.profile_read() if r["launches"]}
    ctx.profile_reset()
    _, _, summ = ctx.tracks_read()
    ctx.tracks_close()
    return wall, rec, summ, regions_wall, int(inputs[0][2].cpu()[2]), host_route(ctx, inputs, 3, prm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--pushes", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes = [(640, 480)] if a.quick else [(640, 480), (1920, 1080), (3840, 2160)]
    head = ["max_regions %d, max_tracks %d, min_overlap %d, max_misses %d, min_hits %d; host route: the numpy statement; µs, pass 1 / pass 2" % (
        MAX_REGIONS, MAX_TRACKS, PRM["min_overlap"], PRM["max_misses"], PRM["min_hits"]), "",
            "| size | mask | records / tracks alive | tracks push: host µs | launches: sum µs | @0 | @1 | @2 | @3 | @4 | @5 | regions push: host µs | host route µs |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rows = {}
    with Context(3840, 2160) as ctx:
        for _ in range(2):
            for (w, h) in sizes:
                natural = smooth_noise(h, w, 7)
                board = ((np.indices((h, w)).sum(0) % 2) == 0).astype(np.uint8) * 255
                full = np.full((h, w), 255, np.uint8)
                cases = [("natural", [natural, np.roll(natural, (2, 2), (0, 1))], 8, 16, PRM), ("full", [full, full], 8, 16, dict(PRM, max_tracks=1)),
                         ("full", [full, full], 8, 16, PRM), ("checkerboard", [board, 255 - board], 4, 1, dict(PRM, min_overlap=1)),
                         ("checkerboard, still", [board, board], 4, 1, dict(PRM, min_overlap=1))]
                for name, masks, conn, min_area, prm in cases:
                    r = one(ctx, masks, conn, min_area, a.pushes, a.warmup, prm)
                    rows.setdefault((w, h, name, prm["max_tracks"]), []).append(r)
    lines = list(head)
    k = ["tracks@%d" % i for i in range(6)]
    for (w, h, name, nt), r in rows.items():
        lines.append("| %dx%d | %s%s | %d / %d | %s | %s | %s | %s | %s |" % (
            w, h, name, "" if nt == MAX_TRACKS else ", max_tracks %d" % nt, r[0][4], r[0][2]["alive"], " / ".join("%.1f" % p[0] for p in r),
            " / ".join("%.1f" % sum(p[1].get(i, 0.0) for i in k) for p in r),
            " | ".join(" / ".join("%.1f" % p[1].get(i, 0.0) for p in r) for i in k),
            " / ".join("%.1f" % p[3] for p in r), " / ".join("%.0f" % p[5] for p in r)))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
