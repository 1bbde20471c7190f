"""Per-launch time of the time-exposure kernels (timex_kernels.hip) on one MI355X -> profiles/timex_kernel_summary.md.

    python scripts/timex_time.py [--out FILE] [--pushes 200] [--warmup 20] [--quick]

1080p and 640x480; each product alone and all four; window 50 and 300; a natural clip (synth.surf_clip made
three-channel, 64 distinct frames cycled) and a static scene.  The ring is filled and wrapped before anything is timed
(window + warmup pushes), then `pushes` pushes are timed per launch with the library's own HIP events
(rcflow_profile_read: "timex@0" = mean launch, "timex@1" = ring launch).  The whole thing runs twice and both passes are
printed, as the spread.  Bytes are the compulsory bytes of the launches as built (what rcflow_profile_read books), so the
rate excludes the data-dependent walks of expired BRIGHT / DARK winners: their cost shows as a lower rate.
"touched every push" is what the timed pushes read and write again and again (the state outside the ring, the distinct
frames, the images); where that fits the 256 MiB Infinity Cache ("cache") most of the traffic never reaches HBM, the rate
is a cache rate and no fraction of the HBM copy rate is printed.  Of the ring a push touches one slot.
Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripcurrents_amd import synth                    # noqa: E402
from ripcurrents_amd.api import Context              # noqa: E402

ALL = ("mean", "average", "bright", "dark")
COPY_TBS = 5.2      # scripts/diag/membw copy rate on these devices
CACHE_BYTES = 256 << 20   # Infinity Cache: a working set below it is re-read from cache, its rate is no HBM figure


def colour_frames(w, h, n):
    g = synth.surf_clip(w, h, n, device="cuda").float()
    noise = torch.randint(0, 64, g.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).float()
    c = torch.stack([(g * 0.9 + 10), (g * 1.2 - 20), (255 - g * 0.8 + noise - 32)], -1)
    return c.clamp(0, 255).round().to(torch.uint8)


def measure(ctx, frames, window, products, pushes, warmup):
    h, w = frames.shape[1:3]
    ctx.timex_open(w, h, window, products)
    outs = {p: torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for p in products}
    n = frames.shape[0]
    ring = any(p != "mean" for p in products)
    for t in range((window if ring else 0) + warmup):
        ctx.timex_push(frames[t % n], out=outs)
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for t in range(pushes):
        ctx.timex_push(frames[(t + 7) % n], out=outs)
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r for r in ctx.profile_read()}
    ctx.profile_reset()
    us = sum(r["total_ms"] for r in rec.values()) * 1e3 / pushes
    by = sum(r["alg_bytes"] for r in rec.values()) / pushes
    launches = sum(r["launches"] for r in rec.values()) / pushes
    nbytes = ctx.timex_info()["device_bytes"]
    ctx.timex_close()
    # what every push touches again: the state outside the ring, the distinct frames, the images; of the ring a push
    # touches one slot (and what the walks read), each slot once per `window` pushes
    ring_bytes = 3 * window * ((w + 3) & ~3) * h if ring else 0
    hot = nbytes - ring_bytes + frames.numel() + sum(o.numel() for o in outs.values())
    return us, by, launches, ring_bytes, hot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="640x480, window 50 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("timex_time.py needs a GPU")
    sizes = [(640, 480)] if a.quick else [(1920, 1080), (640, 480)]
    windows = [50] if a.quick else [50, 300]
    sets = [(p,) for p in ALL] + [ALL]
    rows = []
    with Context(1920, 1080) as ctx:
        for w, h in sizes:
            natural = colour_frames(w, h, 64)
            static = natural[:1]
            for window in windows:
                for products in sets:
                    if products == ("mean",) and window != windows[0]:
                        continue                     # no ring: the window does not matter
                    for scene, frames in (("natural", natural), ("static", static)):
                        passes = [measure(ctx, frames, window, products, a.pushes, a.warmup) for _ in range(2)]
                        rows.append((w, h, window, products, scene, passes))
            del natural, static
            torch.cuda.empty_cache()
    lines = ["| size | window | products | scene | launches | touched every push | ring | bytes per frame as built "
             "| µs per frame (pass 1 / pass 2) | bytes / time | of %.1f TB/s |" % COPY_TBS, "|---|---|---|---|---|---|---|---|---|---|---|"]
    for w, h, window, products, scene, passes in rows:
        us = min(p[0] for p in passes)
        by, launches, ring_bytes, hot = passes[0][1:]
        cached = hot <= CACHE_BYTES
        lines.append("| %dx%d | %s | %s | %s | %d | %.0f MB%s | %.0f MB | %.2f MB (%.0f B/px) | %.2f / %.2f | %.2f TB/s | %s |" % (
            w, h, "-" if products == ("mean",) else window, "+".join(products), scene, launches, hot / 1e6,
            " (cache)" if cached else "", ring_bytes / 1e6, by / 1e6, by / (w * h), passes[0][0], passes[1][0], by / us / 1e6,
            "-" if cached else "%.0f %%" % (100 * by / us / 1e6 / COPY_TBS)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
