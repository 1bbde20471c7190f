"""Time of the two launches of a flow-check push (flowcheck_kernels.hip) on one MI355X -> profiles/flowcheck_kernel_summary.md.

    python scripts/flowcheck_time.py [--out FILE] [--pushes 30] [--warmup 5] [--sizes 640x480,1920x1080] [--radii 2,7]

The translating texture drawn at the size asked for, its true field with +-3 px of noise on the middle ninth of the picture and no
backward field, every test on.  Per launch: the library's own HIP events (rcflow_profile_read, "flowcheck@0" and "flowcheck@1"), one reading per push,
the median over `pushes` pushes after `warmup`, in two passes, once with every output and once with the mask and the checked field
only; both frames are named, so the copy that holds the frame is part of the host's time and not of the launch's.  Beside each stand
the bytes the launch cannot avoid (the two frames 1 + 1 B/px and the field 8 B/px in, the outputs asked for out: 25 B/px for all six,
9 for the mask and the checked field) and the time a device-to-device copy of that many bytes takes here.  Before anything is timed
one push is held to the numpy statement, bit for bit, every output, at the size and radius that are timed.  Per push as a caller
sees it: a host clock over the window ending in one synchronise, profiling off.  Needs a GPU: there is no fallback.
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
import _flowcheck_ref as F                                           # noqa: E402
from _dev import same_bits                                           # noqa: E402
from ripcurrents_amd import synth                                    # noqa: E402
from ripcurrents_amd.api import FLOWCHECK_CELL_DTYPE, Context        # noqa: E402

NAMES = ("flowcheck@0", "flowcheck@1")
IN_BYTES = 1 + 1 + 8
OUT_BYTES = dict(flags=1, mask=1, checked=8, resid=8, texture=4, picture=3)


def events(ctx, push, pushes, warmup):
    per = {k: [] for k in NAMES}
    ctx.profile_enable(True)
    for t in range(warmup + pushes):
        ctx.profile_reset()
        push()
        torch.cuda.synchronize()
        if t >= warmup:
            for r in ctx.profile_read():
                if r["kernel"] in per and r["launches"]:
                    per[r["kernel"]].append(r["total_ms"] * 1e3)
    ctx.profile_enable(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(pushes):
        push()
    torch.cuda.synchronize()
    a, b = per[NAMES[0]], per[NAMES[1]]
    return float(np.median(a)), float(min(a)), float(max(a)), float(np.median(b)), (time.perf_counter() - t0) / pushes * 1e6


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


def verify(ctx, w, h, p, clip, fld, dev, every):
    ctx.flowcheck_push(dev[1], dev[0], dev[2], **every)
    want = F.check(clip[0], clip[1], fld, None, p)
    got = {k: v.cpu().numpy() for k, v in every.items()}
    for k in ("checked", "resid", "texture"):
        assert same_bits(got[k], want[k]), "%s differs from the statement" % k
    for k in ("flags", "mask", "picture", "summary"):
        assert np.array_equal(got[k], want[k]), "%s differs from the statement" % k
    assert np.array_equal(got["sums"].reshape(-1, F.SUMS), want["sums"]) and got["cells"].view(FLOWCHECK_CELL_DTYPE).tobytes() == want["cells"].tobytes()
    return int(want["summary"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640x480,1920x1080")
    ap.add_argument("--radii", default="2,7")
    a = ap.parse_args()
    out = ["| size | radius | outputs | pass | @0 median us | min | max | @1 median us | bytes MB | copy of them us | push, host us |", "|" + "---|" * 11]
    notes = []
    with Context(3840, 2160) as ctx:
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            clip = synth.translating_clip(w, h, 2)
            fld = F.noisy_patch(F.constant_field(w, h, 1.25, -0.75), patch=(slice(h // 3, 2 * h // 3), slice(w // 3, 2 * w // 3)))
            dev = [torch.as_tensor(clip[0]).cuda(), torch.as_tensor(clip[1]).cuda(), torch.as_tensor(fld).cuda()]
            f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
            u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
            every = dict(flags=u8(h, w), mask=u8(h, w), checked=f32(h, w, 2), resid=f32(h, w, 2), texture=f32(h, w), picture=u8(h, w, 3),
                         cells=u8(900 * 32), sums=torch.empty(900 * F.SUMS, dtype=torch.int64, device="cuda"),
                         summary=torch.empty(F.SUMMARY_WORDS, dtype=torch.int64, device="cuda"))
            lean = {k: every[k] for k in ("mask", "checked")}
            for r in (int(v) for v in a.radii.split(",")):
                p = F.Params(radius=r, grid_x=30, grid_y=30, tests=F.TESTS, tex_min=1, gain_pm=900, res_max=1.5, speed_max=8.0)
                ctx.flowcheck_open(w, h, **p.kw())
                valid = verify(ctx, w, h, p, clip, fld, dev, every)
                for name, kw in (("all six", every), ("mask, checked", lean)):
                    nbytes = w * h * (IN_BYTES + sum(OUT_BYTES[k] for k in kw if k in OUT_BYTES))
                    cp = copy_us(nbytes)
                    for k in range(2):
                        med, lo, hi, med1, wall = events(ctx, lambda: ctx.flowcheck_push(dev[1], dev[0], dev[2], **kw), a.pushes, a.warmup)
                        out.append("| %dx%d | %d | %s | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (w, h, r, name, k + 1, med, lo, hi, med1, nbytes / 1e6, cp, wall))
                ctx.flowcheck_close()
                notes.append("%dx%d, radius %d: the statement names %d of %d pixels VALID; device and statement agree on every output." % (w, h, r, valid, w * h))
    text = "\n".join(out) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
