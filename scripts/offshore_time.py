"""Time of the launches of the offshore frame (offshore_kernels.hip) on one MI355X -> profiles/offshore_kernel_summary.md.

    python scripts/offshore_time.py [--out FILE] [--calls 20] [--warmup 3] [--sizes 1920x1080,640x480] [--shores straight,cuspate,speckle]

Three shores: a straight one at a third of the height (the walk of the row pass is as long as the pixel is far from the shore), a
cuspate one (4 pixels of amplitude, a period of 48), and 99 % wet speckle (short walks, many ties).  The map with dist2 and near
asked for, the push with the cross / along field and the mask, the band.  Per launch: the library's own HIP events
(rcflow_profile_read, "offshore@0" .. "offshore@5"), one reading per call, the median over `calls` calls after `warmup`.  Beside
them stand the bytes the call cannot avoid (map: the mask 1 B/px in, dist2 and near 4 B/px each out; push: the field 8 B/px in, the
cross / along field 8 B/px and the mask 1 B/px out; band: d2 4 B/px in, the band 1 B/px out; the column planes and the state's own
planes are the method's traffic and count against it) and the time a device-to-device copy of that many bytes takes here.
Before anything is timed, d2 and near of 512 pixels drawn at random are held to the brute force over every candidate of the
picture, at the size that is timed; the whole map is held to the statement by tests/test_gpu_offshore.py at sizes the brute force
can afford.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _offshore_ref as R                                            # noqa: E402
from ripcurrents_amd.api import Context                              # noqa: E402

NAMES = tuple("offshore@%d" % k for k in range(6))
MAP_BYTES, PUSH_BYTES, BAND_BYTES = 1 + 4 + 4, 8 + 8 + 1, 4 + 1


def shore(name, w, h):
    if name == "straight":
        return R.beach(w, h, h / 3.0, 0.0)
    if name == "cuspate":
        return R.beach(w, h, h / 3.0, 4.0, 48.0)
    return R.speckle(w, h, 0.99, 5)


def events(ctx, call, calls, warmup):
    per = {k: [] for k in NAMES}
    ctx.profile_enable(True)
    for t in range(warmup + calls):
        ctx.profile_reset()
        call()
        torch.cuda.synchronize()
        if t >= warmup:
            for r in ctx.profile_read():
                if r["kernel"] in per and r["launches"]:
                    per[r["kernel"]].append(r["total_ms"] * 1e3)
    ctx.profile_enable(False)
    return {k: float(np.median(v)) for k, v in per.items() if v}


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


def spot_check(wet, dist2, near, n=512, seed=1):
    """d2 and near of n pixels against every candidate of the picture"""
    h, w = wet.shape
    c = (wet != 0).ravel()
    idx = np.arange(h * w)
    ys, xs = idx // w, idx % w
    for i in np.random.default_rng(seed).integers(0, h * w, n):
        other = idx[c != c[i]]
        dd = (ys[other] - ys[i]) ** 2 + (xs[other] - xs[i]) ** 2
        j = int(dd.argmin())
        assert abs(int(dist2.flat[i])) == int(dd[j]) and int(near.flat[i]) == int(other[j]), "pixel %d differs from the brute force" % i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,640x480")
    ap.add_argument("--shores", default="straight,cuspate,speckle")
    a = ap.parse_args()
    out = ["| size | shore | map @0 us | @1 us | @2 us | map us | copy of its bytes us | multiple | push @3 us | @4 us | push us | copy us | multiple | band @5 us | copy us | multiple |",
           "|" + "---|" * 16]
    notes = []
    with Context(3840, 2160) as ctx:
        for size in a.sizes.split(","):
            w, h = (int(v) for v in size.split("x"))
            cps = [copy_us(w * h * b) for b in (MAP_BYTES, PUSH_BYTES, BAND_BYTES)]
            fld = torch.as_tensor(R.jet_field(w, h, w // 2, w // 2 + w // 16, (0.5, -0.25), (0.25, 3.0))).cuda()
            i32 = lambda: torch.empty((h, w), dtype=torch.int32, device="cuda")
            dist2, near = i32(), i32()
            ca, mask = torch.empty((h, w, 2), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.uint8, device="cuda")
            band = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            for name in a.shores.split(","):
                wet = shore(name, w, h)
                dwet = torch.as_tensor(wet).cuda()
                ctx.offshore_open(w, h, min_dist=2, max_dist=min(h, 1000), stations=16, bins=20, bin_width=max(1, h // 40), min_count=16, rip_bins=3,
                                  cross_min=0.25, station="x")
                ctx.offshore_map(dwet, dist2=dist2, near=near)
                spot_check(wet, dist2.cpu().numpy(), near.cpu().numpy())
                t = events(ctx, lambda: ctx.offshore_map(dwet, dist2=dist2, near=near), a.calls, a.warmup)
                t.update(events(ctx, lambda: ctx.offshore_push(fld, cross_along=ca, mask=mask), a.calls, a.warmup))
                t.update(events(ctx, lambda: ctx.offshore_band(10, 50, band), a.calls, a.warmup))
                recs, table, ps, ms = ctx.offshore_read()
                ctx.offshore_close()
                m, p, b = sum(t[k] for k in NAMES[:3]), t[NAMES[3]] + t[NAMES[4]], t[NAMES[5]]
                out.append("| %dx%d | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
                    w, h, name, t[NAMES[0]], t[NAMES[1]], t[NAMES[2]], m, cps[0], m / cps[0], t[NAMES[3]], t[NAMES[4]], p, cps[1], p / cps[1], b, cps[2], b / cps[2]))
                notes.append("%dx%d, %s: %d wet, largest distance %.1f px; OK %d, mask %d, stations flagged %d; 512 pixels agree with the brute force." % (
                    w, h, name, ms["wet"], np.sqrt(float(ms["max_d2"])), ps["ok"], ps["mask"], ps["rips"]))
    text = "\n".join(out) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
