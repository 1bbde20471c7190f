"""Time of the two launches of a mean-flow push (meanflow_kernels.hip) on one MI355X -> profiles/meanflow_kernel_summary.md.

    python scripts/meanflow_time.py [--out FILE] [--pushes 30] [--warmup 5] [--sizes 640x480,1920x1080] [--windows 16,300]

Waves, a jet and noise drawn at the size asked for, eight fields in turn.  Per launch: the library's own HIP events
(rcflow_profile_read, "meanflow@0" and "meanflow@1"), one reading per push, the median over `pushes` pushes after `warmup`, in two
passes, once with every output and once with none, after the ring has wrapped (so that a push also reads the slot it replaces).
Beside meanflow@0 stand the bytes it cannot avoid as built (the field 8 B/px in; the ring slot 4 + 4; n 2 + 2, Su, Sv and Sm 4 + 4
each, Suu, Svv and Suv 8 + 8 each: 92 B/px), the time a device-to-device copy of that many bytes takes here, and two neighbours at
the same size and window: ripmap@0 (the opposing-flow map, 30 x 30 cells) and surf@0 (the surf zone without lines).  Where the whole
state fits the 256 MiB Infinity Cache the row says so and gives no fraction of the copy's rate.  Before anything is timed six pushes
into a window of 4 are held to the numpy statement, bit for bit, every output, at the size that is timed.  Per push as a caller sees
it: a host clock over the window ending in one synchronise, profiling off.  Needs a GPU: there is no fallback.
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
import _meanflow_ref as M                                            # noqa: E402
from _dev import same_bits                                           # noqa: E402
from ripcurrents_amd.api import MEANFLOW_CELL_DTYPE, Context         # noqa: E402

NAMES = ["meanflow@0", "meanflow@1"]
BYTES_PER_PIXEL = 8 + 4 + 4 + 2 * 38
INFINITY_CACHE = 256 << 20


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


def copy_us(nbytes, reps=30):
    """microseconds of a device-to-device copy that reads and writes nbytes in all"""
    a, b = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps + 5):
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[5:])) * 1e3


def scene(w, h, t, seed=3):
    """the naming scene's waves at the size asked for, the jet on the middle tenth of the columns, noise of sigma 0.2"""
    rng = np.random.default_rng(1000 * seed + t)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    v = 0.5 + 3.0 * np.sin(2 * np.pi * t / 4 + 0.03 * x)
    u = 0.7 * np.cos(2 * np.pi * t / 4 + 0.02 * y)
    v[:, 9 * w // 20:11 * w // 20] -= 2.5
    return np.ascontiguousarray(np.stack([u, v], -1) + rng.normal(0., 0.2, (h, w, 2)), np.float32)


def verify(ctx, w, h, host, dev, every):
    """six pushes into a window of 4 against the statement, every output"""
    p = M.Params(window=4, grid_x=30, grid_y=30, min_fill=3, steady_min=600, speed_min=0.5, min_cos2=0.5)
    ref = M.MeanFlowRef(w, h, p, ctx.jet_lut())
    ctx.meanflow_open(w, h, **p.kw())
    for t in range(6):
        want = ref.push(host[t])
        ctx.meanflow_push(dev[t], **every)
        got = {k: v.cpu().numpy() for k, v in every.items()}
        for k in ("mean", "std"):
            assert same_bits(got[k], want[k]), "%s differs from the statement at push %d" % (k, t + 1)
        assert np.array_equal(got["steady"].view(np.uint16), want["steady"]) and np.array_equal(got["mask"], want["mask"])
        assert np.array_equal(got["picture"], want["picture"]) and np.array_equal(got["sums"].reshape(-1, 8), want["sums"])
        assert got["cells"].view(MEANFLOW_CELL_DTYPE).tobytes() == want["cells"].tobytes() and np.array_equal(got["summary"], want["summary"])
    ctx.meanflow_close()
    return int(want["summary"][1])


def measure(ctx, w, h, W, pushes, warmup, host, dev, every):
    ctx.meanflow_open(w, h, window=W, grid_x=30, grid_y=30, min_fill=W, steady_min=600, speed_min=0.5, min_cos2=0.5)
    state = ctx.meanflow_info()["device_bytes"]
    for t in range(W):                                         # the ring wraps: from here on a push reads the slot it replaces
        ctx.meanflow_push(dev[t % 8])
    rows = []
    for name, kw in (("every output", every), ("none", {})):
        for k in range(2):
            us, wall = events(ctx, lambda t: ctx.meanflow_push(dev[t % 8], **kw), pushes, warmup, NAMES)
            rows.append((name, k + 1, us[NAMES[0]], us[NAMES[1]], wall))
    ctx.meanflow_close()
    # the yardsticks: a copy of meanflow@0's bytes, and the neighbours at the same size and window
    P = (w + 3) & ~3
    b0 = BYTES_PER_PIXEL * P * h
    cp = copy_us(b0)
    ctx.ripmap_open(w, h, W, (30, 30))
    for t in range(min(W, 16)):
        ctx.ripmap_push(dev[t % 8])
    rus, _ = events(ctx, lambda t: ctx.ripmap_push(dev[t % 8]), pushes, warmup, ["ripmap@0"])
    ctx.ripmap_close()
    gray = torch.as_tensor(np.clip(host[0][..., 1] * 30 + 128, 0, 255).astype(np.uint8)).cuda()
    ctx.surf_open(w, h, (), window=W)
    for t in range(min(W, 16)):
        ctx.surf_push(gray)
    sus, _ = events(ctx, lambda t: ctx.surf_push(gray), pushes, warmup, ["surf@0"])
    ctx.surf_close()
    return state, rows, b0, cp, rus["ripmap@0"], sus["surf@0"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640x480,1920x1080")
    ap.add_argument("--windows", default="16,300")
    a = ap.parse_args()
    out = ["| size | W | state MB | outputs | pass | @0 us | @1 us | push, host us |", "|" + "---|" * 8]
    notes = []
    with Context(3840, 2160) as ctx:
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            host = [scene(w, h, t) for t in range(8)]
            dev = [torch.as_tensor(f).cuda() for f in host]
            f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
            u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
            every = dict(mean=f32(h, w, 2), steady=torch.empty((h, w), dtype=torch.int16, device="cuda"), std=f32(h, w, 2), mask=u8(h, w), picture=u8(h, w, 3),
                         cells=u8(900 * 32), sums=torch.empty(900 * 8, dtype=torch.int64, device="cuda"), summary=torch.empty(8, dtype=torch.int64, device="cuda"))
            named = verify(ctx, w, h, host, dev, every)
            for W in (int(v) for v in a.windows.split(",")):
                state, rows, b0, cp, rm0, sf0 = measure(ctx, w, h, W, a.pushes, a.warmup, host, dev, every)
                for r in rows:
                    out.append("| %dx%d | %d | %.1f | %s | %d | %.1f | %.1f | %.1f |" % ((w, h, W, state / 1e6) + r))
                best = min(r[2] for r in rows if r[0] == "none")
                note = ("%dx%d, W = %d: meanflow@0 moves %.1f MB it cannot avoid (%d B/px); a device-to-device copy that reads and writes that many "
                        "bytes in all takes %.1f us here; ripmap@0 %.1f us, surf@0 %.1f us at the same size and window." % (w, h, W, b0 / 1e6, BYTES_PER_PIXEL, cp, rm0, sf0))
                if state <= INFINITY_CACHE:
                    note += "  The whole state (%.1f MB) fits the 256 MiB Infinity Cache: no fraction of the copy's rate is given." % (state / 1e6)
                else:
                    note += "  Without outputs meanflow@0 runs at %.0f %% of the copy's rate." % (100. * cp / best)
                notes.append(note)
            notes.append("%dx%d: the statement's mask held %d pixels at the sixth verified push." % (w, h, named))
    text = "\n".join(out) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
