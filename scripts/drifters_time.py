"""Time of the two launches of a drifters push (drifters_kernels.hip) on one MI355X -> profiles/drifters_kernel_summary.md.

    python scripts/drifters_time.py [--out FILE] [--pushes 30] [--warmup 5] [--size 1920x1080] [--counts 65536,262144,1048576]

The synthetic rip (synth.surf_field) at the size asked for, rows 0..7 % of the height zone OFFSHORE and the last 7 % zone SHORE, the
drifters on a lattice over the rest.  Per launch: the library's own HIP events (rcflow_profile_read, "drifters@0" and "drifters@1"),
one reading per push, the median over `pushes` pushes after `warmup`, in two passes.  Each count is timed twice: FRESH, right after
the release, where neighbours in memory share pixels' neighbourhoods and cells; and after 200 pushes with RESPAWN, where the
drifters are scattered along their paths and crowded at the jet, because the cost of the scattered adds changes with the crowding.
Beside a push stand the bytes it cannot avoid (24 B a drifter in, 16 out, the four gathered vectors 32, the occupancy word and three
cell words in and out; the occupancy plane in, and out where a drifter is), the time a device-to-device copy of that many bytes
takes here, and the nearest thing the project had before: rcflow_tracers_push_dev with the FLOW mover over the same points as one
cloud (advect_points@0 and tracers@0; counts above its 2^20 points are left out).  Before anything is timed eight pushes of 4096
drifters are held to the numpy statement, bit for bit, every output, at the size that is timed.  Needs a GPU: there is no fallback.
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
import _drifters_ref as D                                            # noqa: E402
from _dev import same_bits                                           # noqa: E402
from ripcurrents_amd import synth                                    # noqa: E402
from ripcurrents_amd.api import DRIFTERS_CELL_DTYPE, Context         # noqa: E402

NAMES = ["drifters@0", "drifters@1"]
TRACER_NAMES = ["advect_points@0", "tracers@0"]


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


def lattice(w, h, n):
    """n homes on a lattice over the picture between the zones, x fastest"""
    ny = max(1, int(round(np.sqrt(n * h / w))))
    nx = n // ny
    xy = D.lattice(np.linspace(4, w - 5, nx), np.linspace(0.15 * h, 0.85 * h, ny))
    return np.concatenate([xy, xy[:n - len(xy)]]) if len(xy) < n else xy[:n]


def zones(w, h):
    z = np.zeros((h, w), np.uint8)
    z[:int(0.07 * h)], z[h - int(0.07 * h):] = 2, 1
    return z


def verify(ctx, w, h, field, zone, dfield, dzone):
    """eight pushes of 4096 drifters against the statement, every output"""
    n = 4096
    p = D.Params(max_drifters=n, grid_x=30, grid_y=30, max_age=5, flags=D.RESPAWN)
    ref = D.DriftersRef(w, h, p, ctx.jet_lut())
    homes = lattice(w, h, n)
    ref.seed(homes)
    ctx.drifters_open(w, h, **p.kw())
    ctx.drifters_seed(homes)
    t = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    every = dict(now=t((h, w), torch.int16), density=t((h, w), torch.int32), live=t((h, w), torch.uint8), picture=t((h, w, 3), torch.uint8),
                 xy=t((2 * n,), torch.float32), age=t((n,), torch.int32), state=t((n,), torch.uint8), cells=t((900 * 32,), torch.uint8),
                 place=t((900 * 8,), torch.int64), origin=t((900 * 8,), torch.int64), hist=t((128,), torch.int64), summary=t((24,), torch.int64))
    for k in range(8):
        want = ref.push(field, zone)
        ctx.drifters_push(dfield, dzone, **every)
        got = {k2: v.cpu().numpy() for k2, v in every.items()}
        assert same_bits(got["xy"].reshape(-1, 2), want["xy"]), "xy differs from the statement at push %d" % (k + 1)
        assert np.array_equal(got["now"].view(np.uint16), want["now"]) and np.array_equal(got["density"].view(np.uint32), want["density"])
        assert np.array_equal(got["live"], want["live"]) and np.array_equal(got["picture"], want["picture"])
        assert np.array_equal(got["age"], want["age"]) and np.array_equal(got["state"], want["state"])
        assert np.array_equal(got["place"].reshape(-1, 8), want["place"]) and np.array_equal(got["origin"].reshape(-1, 8), want["origin"])
        assert np.array_equal(got["hist"].view(np.uint64).reshape(4, 32), want["hist"]) and np.array_equal(got["summary"], want["summary"])
        assert got["cells"].view(DRIFTERS_CELL_DTYPE).tobytes() == want["cells"].tobytes()
    ctx.drifters_close()
    return int(want["summary"][8:].sum())


def measure(ctx, w, h, n, pushes, warmup, dfield, dzone):
    homes = lattice(w, h, n)
    ctx.drifters_open(w, h, max_drifters=n, grid_x=30, grid_y=30, max_age=0, respawn=True)
    ctx.drifters_seed(homes)
    push = lambda t: ctx.drifters_push(dfield, dzone)
    rows = []
    push(0)                                                       # the release
    for k in range(2):
        us, wall = events(ctx, push, pushes, warmup, NAMES)
        rows.append(("fresh", k + 1, us[NAMES[0]], us[NAMES[1]], wall))
        if k == 0:
            ctx.drifters_reset()
            push(0)
    for t in range(200):
        push(t)
    for k in range(2):
        us, wall = events(ctx, push, pushes, warmup, NAMES)
        rows.append(("after 200 pushes", k + 1, us[NAMES[0]], us[NAMES[1]], wall))
    _, _, _, _, summ = ctx.drifters_read()
    ctx.drifters_close()
    P = (w + 3) & ~3
    b = n * (24 + 16 + 32 + 8 + 48) + P * h * 4 + min(n, P * h) * 12
    cp = copy_us(b)
    tr = None
    if n <= 1 << 20:
        ctx.tracers_open(w, h, mover="flow", max_lines=1, max_vertices=2, max_points=n)
        ctx.tracers_add("cloud", homes)
        tus, _ = events(ctx, lambda t: ctx.tracers_push(flow=dfield), pushes, warmup, TRACER_NAMES)
        ctx.tracers_close()
        tr = (tus[TRACER_NAMES[0]], tus[TRACER_NAMES[1]])
    return rows, b, cp, tr, summ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--counts", default="65536,262144,1048576")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    out = ["| size | drifters | state | pass | @0 us | @1 us | push, host us |", "|" + "---|" * 7]
    notes = []
    with Context(3840, 2160) as ctx:
        field, zone = D.field(*synth.surf_field(w, h)), zones(w, h)
        dfield, dzone = torch.as_tensor(field).cuda(), torch.as_tensor(zone).cuda()
        deaths = verify(ctx, w, h, field, zone, dfield, dzone)
        notes.append("%dx%d: eight pushes of 4096 drifters equal the statement on every output (%d deaths among them)." % (w, h, deaths))
        for n in (int(v) for v in a.counts.split(",")):
            rows, b, cp, tr, summ = measure(ctx, w, h, n, a.pushes, a.warmup, dfield, dzone)
            for r in rows:
                out.append("| %dx%d | %d | %s | %d | %.1f | %.1f | %.1f |" % ((w, h, n) + r))
            note = ("%d drifters: a push moves %.1f MB it cannot avoid; a device-to-device copy that reads and writes that many bytes in all takes "
                    "%.1f us here." % (n, b / 1e6, cp))
            if tr:
                note += "  rcflow_tracers_push_dev with the FLOW mover over the same points: advect_points@0 %.1f us, tracers@0 %.1f us." % tr
            note += "  After the timed pushes: %d alive, %d released, %d SHORE and %d OFFSHORE deaths." % (
                summ["alive"], summ["released"], summ["fate%d" % D.SHORE], summ["fate%d" % D.OFFSHORE])
            notes.append(note)
    text = "\n".join(out) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
