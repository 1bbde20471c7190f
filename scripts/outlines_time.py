"""Time of the launches of the region outlines (outline_kernels.hip) on one MI355X -> profiles/outlines_kernel_summary.md.

    python scripts/outlines_time.py [--out FILE] [--calls 20] [--warmup 3] [--size 1920x1080]

Three pictures: a straight shoreline mask (wet below a third of the height: one long loop), the label plane the regions make of some
fifty blobs (made on the device by rcflow_regions_push_dev, as a user's would be), and 50 % speckle, the worst case for the number
of cracks.  Each is traced with a slot opened for the worst case (max_cracks 2^22, 22 rounds) and, where the picture is small, with
one opened to fit (the next power of two above its cracks), with and without the early return of the pointer rounds (option
"outlines_early").  Per launch group: the library's own HIP events (rcflow_profile_read), summed over the group's launches, one
reading per push, the median over `calls` pushes after `warmup`:
    flag and scan      outlines@0 .. @2   sides, block counts and their scan, the cracks in key order, the successor's place
    leader rounds      outlines@3         `rounds` launches
    rank rounds        outlines@4, @5     the cut and `rounds` launches
    order and measure  outlines@6 .. @10  loop numbers, loop order, area and box, vertices, records
Beside them: the whole push between two events on the stream with the profile off (what a caller waits for, the gaps between the
launches included), and the time of copying the label plane to the host (pinned memory, 4 bytes a pixel), which is what the host
route costs before it has traced anything.  Before anything is timed the result is held to what must be true of it: the cracks of
every loop add up to the picture's, the areas add up to twice the foreground's pixels (one-label pictures), every stored polygon's
shoelace sum is its record's area2.  The sequential statement itself is held bit for bit by tests/test_gpu_outlines.py at sizes a
Python walk can afford.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _outlines_ref as R                                            # noqa: E402
from ripcurrents_amd.api import Context                              # noqa: E402

MARKER = "## Beside the table"
HEADER = """# Region outlines: what the launches cost

Written by `python scripts/outlines_time.py --out profiles/outlines_kernel_summary.md` on one MI355X; everything below the heading
"Beside the table" is kept by the script as it finds it.  Microseconds, the median over the pushes timed.  Per launch group the
library's own events summed over the group's launches (flag and scan `outlines@0..2`, leader rounds `@3`, rank rounds `@4, @5`, order
and measure `@6..10`); "push on the stream" is the whole push between two events with the profile off, the gaps between its launches
included.  max_cracks is what the slot was opened for: 2^22 for the worst case at this size, or the next power of two above the
picture's own cracks.

"""
GROUPS = (("flag and scan", (0, 1, 2)), ("leader rounds", (3,)), ("rank rounds", (4, 5)), ("order and measure", (6, 7, 8, 9, 10)))
WORST = 1 << 22


def events(ctx, call, calls, warmup):
    per = {g: [] for g, _ in GROUPS}
    ctx.profile_enable(True)
    for t in range(warmup + calls):
        ctx.profile_reset()
        call()
        torch.cuda.synchronize()
        if t >= warmup:
            got = {r["kernel"]: r["total_ms"] * 1e3 for r in ctx.profile_read() if r["launches"]}
            for g, ids in GROUPS:
                per[g].append(sum(got.get("outlines@%d" % k, 0.0) for k in ids))
    ctx.profile_enable(False)
    return {g: float(np.median(v)) for g, v in per.items()}


def stream_us(call, calls, warmup):
    """microseconds between two events around the call, the profile off"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for t in range(warmup + calls):
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if t >= warmup:
            us.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(us))


def host_copy_us(plane, calls, warmup):
    """microseconds of the label plane's copy into pinned host memory, by the host's clock around a synchronised copy"""
    import time
    host = torch.empty(plane.shape, dtype=plane.dtype).pin_memory()
    us = []
    for t in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(plane, non_blocking=True)
        torch.cuda.synchronize()
        if t >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us))


def holds(rec, verts, summ, pixels, one_label):
    assert not summ["overflow"] and summ["records"] == len(rec)
    if summ["records"] == summ["kept"] == summ["loops"]:
        assert int(rec["cracks"].sum()) == summ["cracks"], "the loops' cracks do not add up to the picture's"
        if one_label:
            assert int(rec["area2"].sum()) == 2 * pixels, "the areas do not add up to the foreground"
    for r in rec[:200]:
        if r["offset"] < 0:
            continue
        v = verts[r["offset"]:r["offset"] + r["verts"]].astype(np.int64)
        n = np.roll(v, -1, axis=0)
        assert int((v[:, 0] * n[:, 1] - n[:, 0] * v[:, 1]).sum()) == int(r["area2"]), "a polygon's shoelace sum is not its area2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    out = ["| picture | max_cracks | rounds | early return | flag and scan us | leader rounds us | rank rounds us | order and measure us | sum us | push on the stream us |",
           "|" + "---|" * 10]
    notes = []
    with Context(3840, 2160) as ctx:
        y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
        shore = np.where(y >= h // 3, 255, 0).astype(np.uint8)
        speckle = np.where(np.random.RandomState(5).rand(h, w) < 0.5, 255, 0).astype(np.uint8)
        blobs = torch.as_tensor(R.blobs(w, h, 50, 3)).cuda()
        labels = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        ctx.regions_open(w, h, connectivity=8, min_area=1, max_regions=1024)
        ctx.regions_push(blobs, labels=labels)
        ctx.regions_close()
        copy = host_copy_us(labels, a.calls, a.warmup)
        cases = (("shoreline mask", dict(mask=torch.as_tensor(shore).cuda()), int((shore != 0).sum()), True),
                 ("labels of 50 blobs", dict(labels=labels), int((labels != 0).sum().item()), False),
                 ("50 % speckle", dict(mask=torch.as_tensor(speckle).cuda()), int((speckle != 0).sum()), True))
        for name, kw, pixels, one_label in cases:
            ctx.outlines_open(w, h, connectivity=8, min_cracks=4, max_cracks=WORST, max_loops=1 << 20, max_vertices=1 << 23)
            ctx.outlines_push(**kw)
            rec, verts, summ = ctx.outlines_read()
            holds(rec, verts, summ, pixels, one_label)
            notes.append("%s: %d cracks, %d loops, %d vertices, longest loop %d cracks, %d holes." % (
                name, summ["cracks"], summ["loops"], summ["vertices"], int(rec["cracks"].max()), int((rec["area2"] < 0).sum())))
            fit = max(4096, 1 << int(summ["cracks"] - 1).bit_length())
            for cap in sorted({WORST, fit}, reverse=True):
                ctx.outlines_open(w, h, connectivity=8, min_cracks=4, max_cracks=cap, max_loops=1 << 20, max_vertices=1 << 23)
                rounds = ctx.outlines_info()["rounds"]
                for early in (1, 0):
                    ctx.set_option("outlines_early", early)
                    t = events(ctx, lambda: ctx.outlines_push(**kw), a.calls, a.warmup)
                    whole = stream_us(lambda: ctx.outlines_push(**kw), a.calls, a.warmup)
                    out.append("| %s | %d | %d | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
                        name, cap, rounds, "yes" if early else "no", *(t[g] for g, _ in GROUPS), sum(t.values()), whole))
                ctx.set_option("outlines_early", 1)
            ctx.outlines_close()
        notes.append("%d x %d; the label plane (%.1f MB) to pinned host memory: %.1f us." % (w, h, w * h * 4 / 1e6, copy))
    text = HEADER + "\n".join(out) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        kept = ""
        if os.path.exists(a.out):                                    # what was written by hand below the marker stays
            old = open(a.out).read()
            kept = old[old.index(MARKER):] if MARKER in old else ""
        with open(a.out, "w") as f:
            f.write(text + ("\n" + kept if kept else ""))


if __name__ == "__main__":
    main()
