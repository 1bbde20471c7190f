"""Time of one rip-regions push (region_kernels.hip) on one MI355X, beside the only route there was before it: a synchronous
copy of the mask to the host, the labelling there, and the copy of the cleaned mask back -> profiles/regions_kernel_summary.md.

    python scripts/regions_time.py [--out FILE] [--pushes 50] [--warmup 5] [--quick]

Rows at 640x480, 1080p and 4K for: the empty mask, the full mask (every partial sum meets on one record: the contention
case), a natural mask (thresholded smooth noise, 45 % foreground), random pixels at density 0.593 at 8-connectivity (the
tortuous case), a checkerboard at 4-connectivity (every pixel its own component: 32 distinct numbers per wave and row in
the statistics launch for the first max_regions of them), a one-pixel spiral at 640x480 (the longest merge chains); the natural mask also with the flow sums and
without the label image.  Per launch: the library's own HIP events (rcflow_profile_read, "regions@0".."regions@6") summed
over a window of `pushes` pushes.  Per push as a caller sees it: a host clock over the window ending in one synchronise,
profiling off.  Host route: mask.cpu(), scipy.ndimage.label + an area filter (the numpy statement of tests/_regions_ref.py
when scipy is missing; the table says which), .cuda() of the cleaned mask, timed per push with a synchronise.  The whole
thing runs twice and both passes are printed, as the spread.  Needs a GPU: there is no fallback.
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
from ripcurrents_amd.api import Context           # noqa: E402
import _regions_ref as R                          # noqa: E402

try:
    import scipy.ndimage as ndi
except ImportError:
    ndi = None

MIN_AREA, MAX_REGIONS = 16, 1024      # the checkerboard row runs with min_area 1


def smooth_noise(h, w, seed, thresh=0.55):
    rng = np.random.RandomState(seed)
    f = np.fft.rfft2(rng.rand(h, w).astype(np.float32))
    ky, kx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    g = np.fft.irfft2(f * np.exp(-(kx * kx + ky * ky) * (2 * np.pi * 6.0) ** 2 / 2), (h, w))
    return np.where(g > np.quantile(g, thresh), 255, 0).astype(np.uint8)


def spiral(h, w):
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 255

    def free(y, x, dy, dx):
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < h and 0 <= nx < w) or m[ny, nx]:
            return False
        return not (0 <= ay < h and 0 <= ax < w and m[ay, ax])

    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy
            if not free(y, x, dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = 255


def host_route(dmask, conn, reps):
    st = None if ndi is None else (np.ones((3, 3), int) if conn == 8 else ndi.generate_binary_structure(2, 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        m = dmask.cpu().numpy()
        if ndi is not None:
            lab, n = ndi.label(m, st)
            keep = np.concatenate([[False], np.bincount(lab.reshape(-1), minlength=n + 1)[1:] >= MIN_AREA])
            out = np.where(keep[lab], 255, 0).astype(np.uint8)
        else:
            out = R.regions(m, conn, MIN_AREA, MAX_REGIONS)["mask_out"]
        torch.as_tensor(out).cuda()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def one(ctx, mask, conn, flow, labels, pushes, warmup, min_area=MIN_AREA):
    h, w = mask.shape
    ctx.regions_open(w, h, conn, min_area, MAX_REGIONS)
    dm = torch.as_tensor(mask).cuda()
    out = torch.empty_like(dm)
    dl = torch.empty((h, w), dtype=torch.int32, device="cuda") if labels else None
    kw = dict(flow=flow, labels=dl, mask_out=out)
    for _ in range(warmup):
        ctx.regions_push(dm, **kw)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(pushes):
        ctx.regions_push(dm, **kw)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e6 / pushes
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(pushes):
        ctx.regions_push(dm, **kw)
    ctx.sync()
    ctx.profile_enable(False)
    rec = {r["kernel"]: r["total_ms"] * 1e3 / pushes for r in ctx.profile_read() if r["launches"]}
    ctx.profile_reset()
    _, summ = ctx.regions_read()
    ctx.regions_close()
    return wall, rec, summ, dm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--pushes", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    sizes = [(640, 480)] if a.quick else [(640, 480), (1920, 1080), (3840, 2160)]
    head = ["host labelling: %s; min_area %d, max_regions %d; µs, pass 1 / pass 2" % ("scipy.ndimage.label" if ndi is not None else "the numpy statement",
                                                                                     MIN_AREA, MAX_REGIONS), "",
            "| size | mask | conn | flow | labels | components / kept | push: host µs | launches: sum µs | @0 | @1 | @2 | @3 | @4 | @5 | @6 | host route µs |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    rows = {}
    with Context(3840, 2160) as ctx:
        for _ in range(2):
            for (w, h) in sizes:
                rng = np.random.RandomState(w)
                y, x = torch.meshgrid(torch.arange(h, device="cuda").float(), torch.arange(w, device="cuda").float(), indexing="ij")
                flow = torch.stack([2.5 * torch.sin(x / 31) + 1.5, 2 * torch.cos(y / 27) - 0.5], -1).contiguous()
                natural = smooth_noise(h, w, 7)
                cases = [("empty", np.zeros((h, w), np.uint8), 8, None, True), ("full", np.full((h, w), 255, np.uint8), 8, None, True),
                         ("full", np.full((h, w), 255, np.uint8), 8, flow, True),
                         ("natural", natural, 8, None, True), ("natural", natural, 4, None, True), ("natural", natural, 8, flow, True),
                         ("natural", natural, 8, None, False), ("natural", natural, 8, flow, False),
                         ("random 0.593", (rng.rand(h, w) < 0.593).astype(np.uint8) * 255, 8, None, True)]
                cases.append(("checkerboard", ((np.indices((h, w)).sum(0) % 2) == 0).astype(np.uint8) * 255, 4, flow, True))
                if (w, h) == (640, 480):
                    cases.append(("spiral", spiral(h, w), 8, None, True))
                for name, m, conn, fl, lab in cases:
                    wall, rec, summ, dm = one(ctx, m, conn, fl, lab, a.pushes, a.warmup, 1 if name == "checkerboard" else MIN_AREA)
                    key = (w, h, name, conn, fl is not None, lab)
                    host = host_route(dm, conn, 3) if fl is None and lab else None
                    rows.setdefault(key, []).append((wall, rec, summ, host))
    lines = list(head)
    for (w, h, name, conn, fl, lab), r in rows.items():
        k = ["regions@%d" % i for i in range(7)]
        lines.append("| %dx%d | %s | %d | %s | %s | %d / %d | %s | %s | %s | %s |" % (
            w, h, name, conn, "yes" if fl else "no", "yes" if lab else "no", r[0][2]["components"], r[0][2]["kept"],
            " / ".join("%.1f" % p[0] for p in r), " / ".join("%.1f" % sum(p[1].get(i, 0.0) for i in k) for p in r),
            " | ".join(" / ".join("%.1f" % p[1].get(i, 0.0) for p in r) for i in k),
            "-" if r[0][3] is None else " / ".join("%.0f" % p[3] for p in r)))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
