"""Time of the launches of a surf push (surf_kernels.hip) on one MI355X -> profiles/surf_kernel_summary.md.

    python scripts/surf_time.py [--out FILE] [--pushes 30] [--warmup 5] [--size 1920x1080] [--window 256] [--lines 128] [--samples 512]

A surf zone drawn at the size asked for (a breaker band with moving fronts and two gaps, four frames alternating).  Per launch:
the library's own HIP events (rcflow_profile_read, "surf@0".."surf@2"), one reading per push, the median over `pushes` pushes after
`warmup`, in two passes, once with every output and once with none.  Beside surf@0 stand the bytes it cannot avoid (the frame 1 B/px
in; the ring slot 1 + 1, S1 and S2 4 + 4 each, Q 2 + 2, the flags 1/8 + 1/8: 23.25 B/px), the time those bytes take at the rate a
device-to-device copy of the same size reaches here, and two neighbours at the same size: timex@1 (the time exposure's ring
products, window 50, "average", "bright" and "dark") and shoreline@0 (r 2).  Before anything is timed the first pushes are held to
the numpy statement, bit for bit, at the size that is timed.  Per push as a caller sees it: a host clock over the window ending in
one synchronise, profiling off.  Needs a GPU: there is no fallback.
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
import _shoreline_ref as SH                                          # noqa: E402
import _surf_ref as S                                                # noqa: E402
from ripcurrents_amd.api import SURF_CHANNEL_DTYPE, SURF_LINE_DTYPE, Context      # noqa: E402

NAMES = ["surf@%d" % k for k in range(3)]
STATE_BYTES_PER_PIXEL = 1 + 2 + 8 + 8 + 4 + 0.25


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


def scene(w, h, t, seed=3):
    """the CPU tier's scene at the size asked for: sand, water, a band of fronts in the middle fifth with two gaps, noise"""
    rng = np.random.default_rng(1000 * seed + t)
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    img = np.where(x < w // 5, 170, 70)
    band = (x >= 2 * w // 5) & (x < 3 * w // 5)
    gap = ((y >= h // 4) & (y < h // 4 + h // 12)) | ((y >= 2 * h // 3) & (y < 2 * h // 3 + h // 16))
    front = ((x + 8 * t) % 64 < 16) & ~gap
    img = np.where(band & front, 230, img) + rng.integers(-10, 11, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def measure(ctx, w, h, W, L, n, pushes, warmup):
    lines = [(0.05 * w, (i + 0.5) * h / L, 0.95 * w, (i + 0.5) * h / L, n) for i in range(L)]
    p = S.Params(window=W, bright=180, delta=40, q_min=100, min_run=3, span=6, ratio=500, min_lines=2, vis_permille=500)
    host = [scene(w, h, t) for t in range(8)]
    imgs = [torch.as_tensor(a).cuda() for a in host]
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
    every = dict(now=u8(h, w), surf=u8(h, w), q=torch.empty((h, w), dtype=torch.int16, device="cuda"), mean=u8(h, w), sd=u8(h, w), picture=u8(h, w, 3),
                 lines=u8(L * 64), channels=u8(32 * 32), summary=torch.empty(8, dtype=torch.int64, device="cuda"))
    # the statement first: a window of 4 at this size, so that the ring wraps in 6 pushes
    p4 = S.Params(**dict(S.asdict(p), window=4))
    ref = S.SurfRef(w, h, lines, p4, ctx.jet_lut())
    ctx.surf_open(w, h, lines, **p4.kw())
    for t in range(6):
        want = ref.push(host[t])
        ctx.surf_push(imgs[t], **every)
        got = {k: v.cpu().numpy() for k, v in every.items()}
        for k in S.PICTURES:
            assert np.array_equal(got[k].view(np.uint16) if k == "q" else got[k], want[k]), "%s differs from the statement at push %d" % (k, t + 1)
        assert got["lines"].view(SURF_LINE_DTYPE).tobytes() == want["lines"].tobytes() and np.array_equal(got["summary"], want["summary"])
        assert got["channels"].view(SURF_CHANNEL_DTYPE).tobytes() == want["channels"].tobytes()
    ctx.surf_open(w, h, lines, **p.kw())
    rows = []
    for name, kw in (("every output", every), ("none", {})):
        for k in range(2):
            us, wall = events(ctx, lambda t: ctx.surf_push(imgs[t % 8], **kw), pushes, warmup, NAMES)
            rows.append((name, k + 1) + tuple(us[q] for q in NAMES) + (wall,))
    rl, rc, summ = ctx.surf_read()
    found = (summ["bands"], summ["channel_lines"], summ["channels"])
    state = ctx.surf_info()["device_bytes"]
    ctx.surf_close()
    # the yardsticks: the copy rate at the size of surf@0's bytes, and the neighbours
    P = (w + 3) & ~3
    b0 = STATE_BYTES_PER_PIXEL * P * h
    rate = copy_rate(int(b0 / 2))
    bgr = torch.as_tensor(np.repeat(host[0][..., None], 3, axis=2)).cuda()
    prod = ("average", "bright", "dark")
    ctx.timex_open(w, h, window=50, products=prod)
    outs = {k: u8(h, w, 3) for k in prod}
    tus, _ = events(ctx, lambda t: ctx.timex_push(bgr, out=outs), pushes, warmup, ["timex@1"])
    ctx.timex_close()
    beach = torch.as_tensor(SH.beach(w, h, 0, amp=0.02 * w)).cuda()
    ctx.shoreline_open(w, h, lines, **SH.Params(radius=2, window=16).kw())
    sus, _ = events(ctx, lambda t: ctx.shoreline_push(beach), pushes, warmup, ["shoreline@0"])
    ctx.shoreline_close()
    return state, rows, b0, rate, tus["timex@1"], sus["shoreline@0"], found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--lines", type=int, default=128)
    ap.add_argument("--samples", type=int, default=512)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    out = ["| size | W | lines x n | state MB | outputs | pass | @0 us | @1 us | @2 us | push, host us |", "|" + "---|" * 10]
    with Context(3840, 2160) as ctx:
        state, rows, b0, rate, tx1, sh0, found = measure(ctx, w, h, a.window, a.lines, a.samples, a.pushes, a.warmup)
        for r in rows:
            out.append("| %dx%d | %d | %d x %d | %.1f | %s | %d | %.1f | %.1f | %.1f | %.1f |" % ((w, h, a.window, a.lines, a.samples, state / 1e6) + r))
    out.append("")
    out.append("surf@0: %.1f MB it cannot avoid (%.2f B/px); a device-to-device copy moves bytes at %.2f TB/s here (read plus written), which is "
               "%.1f us for them; timex@1 at the same size (window 50, average, bright and dark): %.1f us; shoreline@0 (r 2): %.1f us.  The last "
               "push found %d lines with a band, %d channel lines, %d channels." % ((b0 / 1e6, STATE_BYTES_PER_PIXEL, rate / 1e12, b0 / rate * 1e6, tx1, sh0) + found))
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
