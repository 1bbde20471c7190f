"""The surf zone (include/rcflow.h, "surf") stated in numpy: the ring of grey frames, S1, S2, the flags and their count Q, the six
pictures, the counts, the samples of the Q plane along the lines, the runs, the band and its edge points, the load, the alongshore
reference, the channel lines, the channels, the records, the summary and the primitives.  Integers are Python / int64 and exact;
the float conversions are float64 operation by operation, in the order the header gives.  Also the synthetic surf zone the tests
look at."""
import math
from dataclasses import asdict, dataclass

import numpy as np

import _shoreline_ref as shref

NOBAND, NOREF, CHANNEL, IN_CHANNEL = 1, 2, 4, 8
MAX_LINES, MIN_SAMPLES, MAX_SAMPLES, MAX_TOTAL, MAX_WINDOW, MAX_SPAN, MAX_CHANNELS, MAX_SHARE = 1024, 8, 1024, 262144, 4096, 32, 32, 1000000
MAX_PIXELS, MAX_STATE_BYTES = 1 << 25, 4 << 30
DISC, LINE_PRIM = 1, 2
f32, f64 = np.float32, np.float64

LINE = np.dtype([("flags", "<i4"), ("k0", "<i4"), ("k1", "<i4"), ("load", "<i4"), ("peak", "<i4"), ("kpeak", "<i4"), ("ix", "<i4"), ("iy", "<i4"),
                 ("ox", "<i4"), ("oy", "<i4"), ("ref", "<i4"), ("share", "<i4"), ("width_m", "<f4"), ("pad", "<i4", (3,))])
CHAN = np.dtype([("first", "<i4"), ("count", "<i4"), ("centre", "<i4"), ("share", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("width_m", "<f4"),
                 ("pad", "<i4")])
PRIM = shref.PRIM
SAMPLE, GEOM = shref.SAMPLE, shref.GEOM
SUMMARY = ("n", "now", "surf", "sum_q", "bands", "channel_lines", "channels", "pushes")
PICTURES = ("now", "surf", "q", "mean", "sd", "picture")


@dataclass
class Params:
    window: int = 32
    bright: int = 180
    delta: int = 40
    q_min: int = 100
    min_run: int = 3
    span: int = 6
    ratio: int = 500
    min_load: int = 0
    min_lines: int = 2
    vis_permille: int = 500
    metres_per_pixel: float = 1.0

    def kw(self):
        """the keywords of Context.surf_open"""
        return asdict(self)


def plan(w, h, lines, metres_per_pixel=1.0):
    """-> (table SAMPLE[S], geom GEOM[L]): the shoreline's rule per line; no lines at all are allowed; ValueError where
    rcflow_surf_plan answers RC_EINVAL"""
    if not (w > 0 and h > 0 and len(lines) <= MAX_LINES and 0 < metres_per_pixel < math.inf):
        raise ValueError("picture, line count or metres_per_pixel")
    if not lines:
        return np.zeros(0, SAMPLE), np.zeros(0, GEOM)
    if any(not MIN_SAMPLES <= int(l[4]) <= MAX_SAMPLES for l in lines) or sum(int(l[4]) for l in lines) > MAX_TOTAL:
        raise ValueError("samples")
    return shref.plan(w, h, lines, metres_per_pixel)


def settable_error(bright, delta, q_min, ratio, min_load, vis_permille):
    if not (0 <= bright <= 255 and 0 <= delta <= 255 and 1 <= q_min <= 1000 and 1 <= ratio <= 999 and min_load >= 0 and 1 <= vis_permille <= 1000):
        return "bright, delta, q_min, ratio, min_load or vis_permille"
    return None


def state_bytes(w, h, window):
    """ring, flag ring, S1, S2 and Q as the header lays them out"""
    P = (w + 3) & ~3
    return P * h * (window + 10) + 32 * window * ((P * h + 255) // 256)


def open_error(w, h, lines, p):
    """what rcflow_surf_open refuses before it looks at the context: None, or the reason"""
    if not (2 <= p.window <= MAX_WINDOW and 1 <= p.min_run <= 64 and 0 <= p.span <= MAX_SPAN and 1 <= p.min_lines <= 64 and
            0 < p.metres_per_pixel < math.inf) or settable_error(p.bright, p.delta, p.q_min, p.ratio, p.min_load, p.vis_permille):
        return "parameters"
    try:
        plan(w, h, lines, p.metres_per_pixel)
    except ValueError as e:
        return str(e)
    if w * h > MAX_PIXELS or state_bytes(w, h, p.window) > MAX_STATE_BYTES:
        return "size"
    return None


def isqrt(v):
    """the exact floor square root of an int64 array"""
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def runs(inside, min_run):
    """-> [(first, last)] of the maximal runs of True at least min_run long"""
    out, j, n = [], 0, len(inside)
    while j < n:
        if not inside[j]:
            j += 1
            continue
        e = j
        while e < n and inside[e]:
            e += 1
        if e - j >= min_run:
            out.append((j, e - 1))
        j = e
    return out


def point(Xa, Xb, pos, n):
    """the shoreline's formula: 1/16 pixel ends, pos in 1/256 sample -> 1/256 pixel"""
    return 16 * Xa + (16 * (Xb - Xa) * pos + 128 * (n - 1)) // (256 * (n - 1))


def reference(B, span):
    """the lower median of the loads within span lines, the line itself included -> int64 [L]"""
    L = len(B)
    out = np.zeros(L, np.int64)
    for i in range(L):
        lo, hi = max(0, i - span), min(L - 1, i + span)
        out[i] = np.sort(B[lo:hi + 1])[(hi - lo) // 2]
    return out


class SurfRef:
    def __init__(self, w, h, lines, p, lut):
        assert open_error(w, h, lines, p) is None
        self.w, self.h, self.p, self.lut = w, h, Params(**asdict(p)), np.asarray(lut, np.uint8).reshape(256, 3)
        self.table, self.geom = plan(w, h, lines, p.metres_per_pixel)
        self.L = len(lines)
        self.reset()

    def reset(self):
        W, h, w = self.p.window, self.h, self.w
        self.ring = np.zeros((W, h, w), np.uint8)
        self.bits = np.zeros((W, h, w), bool)
        self.S1, self.S2, self.Q = (np.zeros((h, w), np.int64) for _ in range(3))
        self.lines = np.zeros(self.L, LINE)
        self.channels = np.zeros(MAX_CHANNELS, CHAN)
        self.summary = np.zeros(8, np.int64)
        self.pushes = 0

    def set(self, bright, delta, q_min, ratio, min_load, vis_permille):
        assert settable_error(bright, delta, q_min, ratio, min_load, vis_permille) is None
        p = self.p
        p.bright, p.delta, p.q_min, p.ratio, p.min_load, p.vis_permille = bright, delta, q_min, ratio, min_load, vis_permille

    def push(self, frame):
        """one HxW uint8 frame -> dict of every output of the push, and V and B for the tests"""
        p, w, h, L, W = self.p, self.w, self.h, self.L, self.p.window
        g = frame.astype(np.int64)
        c = self.pushes % W
        old = self.ring[c].astype(np.int64)
        self.S1 += g - old
        self.S2 += g * g - old * old
        assert self.S2.max() < 2 ** 32 and self.S1.min() >= 0
        self.ring[c] = frame
        n = min(self.pushes + 1, W)
        S1, S2 = self.S1, self.S2
        b = (g >= p.bright) & (g * n >= S1 + p.delta * n)
        self.Q += b.astype(np.int64) - self.bits[c]
        self.bits[c] = b
        Q = self.Q
        assert Q.min() >= 0 and Q.max() <= n
        surf = Q * 1000 >= p.q_min * n
        out = dict(now=np.where(b, 255, 0).astype(np.uint8), surf=np.where(surf, 255, 0).astype(np.uint8), q=Q.astype(np.uint16),
                   mean=((2 * S1 + n) // (2 * n)).astype(np.uint8),
                   sd=np.minimum(255, isqrt((4 * (n * S2 - S1 * S1)) // (n * n))).astype(np.uint8),
                   picture=self.lut[np.minimum(255, (Q * 255000) // (p.vis_permille * n))])
        self.pushes += 1
        lines, chans = np.zeros(L, LINE), np.zeros(MAX_CHANNELS, CHAN)
        nchan, V, B = 0, np.zeros(0, np.int64), np.zeros(L, np.int64)
        if L:
            V = shref.sample(Q, self.table, w, h)
            X, Y = self.table["X"].astype(np.int64), self.table["Y"].astype(np.int64)
            for i, gm in enumerate(self.geom):
                nn, first = int(gm["n"]), int(gm["first"])
                v, r = V[first:first + nn], lines[i]
                rr = runs(v * 1000 >= p.q_min * n, p.min_run)
                B[i] = int(v.sum())
                r["load"], r["peak"], r["kpeak"] = B[i], int(v.max()), int(np.argmax(v))
                if not rr:
                    r["flags"], r["k0"], r["k1"] = NOBAND, -1, -1
                    continue
                k0, k1 = rr[0][0], rr[-1][1]
                Xa, Xb, Ya, Yb = int(X[first]), int(X[first + nn - 1]), int(Y[first]), int(Y[first + nn - 1])
                r["k0"], r["k1"] = k0, k1
                r["ix"], r["iy"] = point(Xa, Xb, 256 * k0, nn), point(Ya, Yb, 256 * k0, nn)
                r["ox"], r["oy"] = point(Xa, Xb, 256 * k1, nn), point(Ya, Yb, 256 * k1, nn)
                r["width_m"] = f32(f64(k1 - k0 + 1) * f64(gm["ds"]))
            ref = reference(B, p.span)
            noref = ref < max(p.min_load, 1)
            chan = ~noref & (B * 1000 < p.ratio * ref)
            share = np.where(ref > 0, np.minimum((B * 1000) // np.maximum(ref, 1), MAX_SHARE), 1000)
            lines["ref"], lines["share"] = ref, share
            lines["flags"] |= np.where(noref, NOREF, 0) | np.where(chan, CHANNEL, 0)
            for first, last in runs(chan, p.min_lines):
                count = last - first + 1
                lines["flags"][first:last + 1] |= IN_CHANNEL
                if nchan < MAX_CHANNELS:
                    centre = first + int(np.argmin(share[first:last + 1]))
                    E = [j for j in (first - 1, last + 1) if 0 <= j < L and not lines["flags"][j] & NOBAND]
                    gc = self.geom[centre]
                    nc, fc = int(gc["n"]), int(gc["first"])
                    pos = sum(128 * (int(lines["k0"][j]) + int(lines["k1"][j])) for j in E) // len(E) if E else 128 * (nc - 1)
                    pos = min(pos, 256 * (nc - 1))
                    fa, fz = int(self.geom[max(first - 1, 0)]["first"]), int(self.geom[min(last + 1, L - 1)]["first"])
                    dx, dy = int(X[fa] - X[fz]), int(Y[fa] - Y[fz])
                    k = chans[nchan]
                    k["first"], k["count"], k["centre"], k["share"] = first, count, centre, share[centre]
                    k["cx"], k["cy"] = point(int(X[fc]), int(X[fc + nc - 1]), pos, nc), point(int(Y[fc]), int(Y[fc + nc - 1]), pos, nc)
                    k["width_m"] = f32((np.sqrt(f64(dx * dx + dy * dy)) / f64(16.0)) * f64(p.metres_per_pixel))
                nchan += 1
        summ = np.array([n, int(b.sum()), int(surf.sum()), int(Q.sum()), int(((lines["flags"] & NOBAND) == 0).sum()),
                         int(((lines["flags"] & CHANNEL) != 0).sum()), nchan, self.pushes], np.int64)
        self.lines, self.channels, self.summary = lines, chans, summ
        out.update(lines=lines, channels=chans, summary=summ, V=V, B=B)
        return out

    def rescan(self):
        """S1, S2 and Q from scratch, from the rings"""
        r = self.ring.astype(np.int64)
        return r.sum(axis=0), (r * r).sum(axis=0), self.bits.sum(axis=0).astype(np.int64)

    def prims(self, color, thickness, disc_radius):
        """the L - 1 + MAX_CHANNELS primitives of the last push"""
        rec, L = self.lines, self.L
        out = np.zeros(L - 1 + MAX_CHANNELS, PRIM)
        if self.pushes == 0:
            return out
        ok = (rec["flags"] & NOBAND) == 0
        px, py = (rec["ox"].astype(np.int64) + 128) >> 8, (rec["oy"].astype(np.int64) + 128) >> 8
        for i in range(L - 1):
            nxt = [j for j in range(i + 1, L) if ok[j]]
            if ok[i] and nxt:
                j = nxt[0]
                out[i] = (LINE_PRIM, px[i], py[i], px[j], py[j], thickness, color, 0)
        for k, ch in enumerate(self.channels):
            if ch["count"] > 0:
                x, y = (int(ch["cx"]) + 128) >> 8, (int(ch["cy"]) + 128) >> 8
                out[L - 1 + k] = (DISC, x, y, x, y, disc_radius, color, 0)
        return out


# ---------------------------------------------------------------------------- the scene
SCENE_W, SCENE_H = 96, 64
BAND = (40, 60)                    # x of the breaker band
CHANNEL_ROWS = ((18, 24), (44, 48))
CHANNEL_LINES = (9, 10, 11, 22, 23)
SCENE = Params(window=32, bright=180, delta=40, q_min=100, min_run=3, span=6, ratio=500, min_lines=2)


def surf_scene(t, foam=False, seed=7, w=SCENE_W, h=SCENE_H):
    """The synthetic surf zone at push t -> HxW uint8: sand of grey 170 where x < 20, water of grey 70; a breaker band in x 40..59
    with fronts of grey 230 where (x + 2 t) mod 16 < 4; two channels, rows 18..23 and 44..47, where only (x + 2 t) mod 16 < 1 on
    every second wave breaks; glitter of grey 240 with probability 0.01 at x >= 62; uniform noise of +-10; optionally a
    persistent foam strip of grey 215 at x 20..23."""
    rng = np.random.default_rng(1000 * seed + t)
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    y = np.arange(h)[:, None] + np.zeros((1, w), np.int64)
    img = np.where(x < 20, 170, 70)
    if foam:
        img = np.where((x >= 20) & (x < 24), 215, img)
    ph = x + 2 * t
    band = (x >= BAND[0]) & (x < BAND[1])
    chan = np.zeros((h, w), bool)
    for a, b in CHANNEL_ROWS:
        chan |= (y >= a) & (y < b)
    front = np.where(chan, (ph % 16 < 1) & ((ph // 16) % 2 == 0), ph % 16 < 4)
    img = np.where(band & front, 230, img)
    img = np.where((rng.random((h, w)) < 0.01) & (x >= 62), 240, img)
    img = img + rng.integers(-10, 11, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def scene_lines(w=SCENE_W, h=SCENE_H):
    """32 horizontal lines y = 1 + 2 i from x = 4 (land) to x = 91 (sea), 88 samples: a sample a pixel"""
    return [(4.0, float(1 + 2 * i), float(w - 5), float(1 + 2 * i), w - 8) for i in range(h // 2)]


def fake_lut():
    """a colour table for the CPU tier, where the library's is not needed: every entry distinct"""
    i = np.arange(256)
    return np.stack([i, 255 - i, (i * 7) % 256], axis=1).astype(np.uint8)
