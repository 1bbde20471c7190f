"""Time of the launches of a flow-infill push (infill_kernels.hip) on one MI355X -> profiles/infill_kernel_summary.md.

    python scripts/infill_time.py [--out FILE] [--pushes 30] [--warmup 5] [--sizes 1920x1080,3840x2160] [--holds 0,4] [--patterns p300,p900,block40]

The statement's shear with its jet, repeated to the size asked for, and its hole patterns (block40 scaled to the picture), 7 levels,
min_known 1, a grid of 30 x 30 cells, the filled field and the source byte asked for.  Per launch: the library's own HIP events
(rcflow_profile_read, "infill@0" .. "infill@3"), one reading per push, the median over `pushes` pushes after `warmup`, in two passes.
Beside them stand the bytes the push cannot avoid (the field 8 B/px read once, d_filled 8 B/px and d_source 1 B/px written once: the
valid mask, the value and class planes and the pyramid are the method's own traffic and count against it) and the time a
device-to-device copy of that many bytes takes here.  With hold > 0 the valid mask moves three pixels a push, so pixels are held.
Before anything is timed one push is held to the numpy statement, bit for bit, every output, at the size that is timed.  Per push
as a caller sees it: a host clock over the window ending in one synchronise, profiling off.  Needs a GPU: there is no fallback.
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
import _infill_ref as R                                              # noqa: E402
from _dev import same_bits                                           # noqa: E402
from ripcurrents_amd.api import INFILL_CELL_DTYPE, Context           # noqa: E402

NAMES = ("infill@0", "infill@1", "infill@2", "infill@3")
BYTES = 8 + 8 + 1


def events(ctx, push, pushes, warmup):
    per = {k: [] for k in NAMES}
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
    wall = (time.perf_counter() - t0) / pushes * 1e6
    return [float(np.median(per[k])) if per[k] else 0.0 for k in NAMES], wall


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


def verify(ctx, w, h, p, fld, valid, every):
    ctx.infill_push(torch.as_tensor(fld).cuda(), torch.as_tensor(valid).cuda(), **every)
    want = R.fill(fld, valid, p, ctx.jet_lut())
    got = {k: v.cpu().numpy() for k, v in every.items()}
    assert same_bits(got["filled"], want["filled"]), "filled differs from the statement"
    for k in ("source", "mask", "picture", "summary"):
        assert np.array_equal(got[k], want[k]), "%s differs from the statement" % k
    assert np.array_equal(got["sums"].reshape(-1, R.SUMS), want["sums"]) and got["cells"].view(INFILL_CELL_DTYPE).tobytes() == want["cells"].tobytes()
    ctx.infill_reset()
    return want["summary"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--holds", default="0,4")
    ap.add_argument("--patterns", default="p300,p900,block40")
    a = ap.parse_args()
    out = ["| size | pattern | hold | pass | @0 us | @1 us | @2 us | @3 us | sum us | bytes MB | copy of them us | multiple | push, host us |", "|" + "---|" * 13]
    notes = []
    with Context(3840, 2160) as ctx:
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            fld = np.ascontiguousarray(np.tile(R.shear_field(), ((h + 119) // 120, (w + 159) // 160, 1))[:h, :w])
            dfld = torch.as_tensor(fld).cuda()
            u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
            every = dict(filled=torch.empty((h, w, 2), dtype=torch.float32, device="cuda"), source=u8(h, w), mask=u8(h, w), picture=u8(h, w, 3),
                         cells=u8(900 * 32), sums=torch.empty(900 * R.SUMS, dtype=torch.int64, device="cuda"),
                         summary=torch.empty(R.SUMMARY_WORDS, dtype=torch.int64, device="cuda"))
            lean = {k: every[k] for k in ("filled", "source")}
            cp = copy_us(w * h * BYTES)
            for pat in a.patterns.split(","):
                valids = [torch.as_tensor(R.pattern(pat, w, h, shift=3 * t)).cuda() for t in range(8)]
                for hold in (int(v) for v in a.holds.split(",")):
                    p = R.Params(levels=7, min_known=1, hold=hold, grid_x=30, grid_y=30)
                    ctx.infill_open(w, h, **p.kw())
                    sm = verify(ctx, w, h, p, fld, R.pattern(pat, w, h), every)
                    for k in range(2):
                        per, wall = events(ctx, lambda t: ctx.infill_push(dfld, valids[t % 8 if hold else 0], **lean), a.pushes, a.warmup)
                        out.append("| %dx%d | %s | %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f |" % (
                            w, h, pat, hold, k + 1, per[0], per[1], per[2], per[3], sum(per), w * h * BYTES / 1e6, cp, sum(per) / cp, wall))
                    ctx.infill_close()
                    notes.append("%dx%d, %s, hold %d: %d KNOWN, %d FILLED, %d UNFILLED, by lev %s; device and statement agree on every output." % (
                        w, h, pat, hold, sm[0], sm[2], sm[3], [int(v) for v in sm[9:]]))
    text = "\n".join(out) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
