"""The shoreline (include/rcflow.h, "shoreline") stated in numpy: the indicator, the box with a replicated border, the plane J, its
histogram, Otsu's threshold and separability, the samples along the lines, the best split, the sub-sample position, the waterline
point, the outlier test along the shore, the ring, the window statistics, the records, the summary, the mask and the primitives.
Integers are Python / int64 and exact; the two places in double are float64 operation by operation, in the order the header
gives.  Also the synthetic beach the tests look at."""
import math
from dataclasses import asdict, dataclass

import numpy as np

import _transects_ref as tsref

RMB, GRAY, PLANE = 0, 1, 2
EMPTY, DRY, WET, UNSURE, OUTLIER, NO_WINDOW = 1, 2, 4, 8, 16, 32
MAX_LINES, MIN_SAMPLES, MAX_SAMPLES, MAX_TOTAL, MAX_RADIUS, MAX_WINDOW = 1024, 8, 1024, 262144, 7, 4096
MAX_PIXELS, MAX_STATE_BYTES, HIST = 1 << 25, 64 << 20, 512
DISC, LINE = 1, 2
f32, f64 = np.float32, np.float64

RECORD = np.dtype([("flags", "<i4"), ("k", "<i4"), ("pos", "<i4"), ("agree", "<i4"), ("wx", "<i4"), ("wy", "<i4"), ("x", "<f4"), ("y", "<f4"),
                   ("dist_m", "<f4"), ("nv", "<i4"), ("pos_min", "<i4"), ("pos_max", "<i4"), ("pos_q", "<i4"), ("pos_mean", "<f4"),
                   ("excursion_m", "<f4"), ("pad", "<i4")])
PRIM = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"), ("color", "<u4"), ("flags", "<u4")])
SAMPLE, GEOM = tsref.SAMPLE, tsref.GEOM
SUMMARY = ("thr", "N", "eta_q32", "positions", "dry", "wet", "outliers", "pushes")


@dataclass
class Params:
    source: int = RMB
    radius: int = 2
    wet_is_high: int = 0
    threshold: int = -1
    window: int = 16
    permille: int = 20
    min_sep: float = 0.0
    max_jump: float = 8.0
    metres_per_pixel: float = 1.0

    def kw(self):
        """the keywords of Context.shoreline_open"""
        d = asdict(self)
        d["source"] = ("rmb", "gray", "plane")[d["source"]]
        return d


def plan(w, h, lines, metres_per_pixel=1.0):
    """-> (table SAMPLE[S], geom GEOM[L]): the transects' rule per line with fps = 1; ValueError where rcflow_shoreline_plan
    answers RC_EINVAL"""
    if not (w > 0 and h > 0 and 1 <= len(lines) <= MAX_LINES and 0 < metres_per_pixel < math.inf):
        raise ValueError("picture, line count or metres_per_pixel")
    if any(not MIN_SAMPLES <= int(l[4]) <= MAX_SAMPLES for l in lines) or sum(int(l[4]) for l in lines) > MAX_TOTAL:
        raise ValueError("samples")
    tabs, geom, first = [], np.zeros(len(lines), GEOM), 0
    for i, l in enumerate(lines):
        t, g = tsref.plan(w, h, [l], metres_per_pixel, 1.0)
        t["line"] = i
        g["first"] = first
        tabs.append(t)
        geom[i] = g[0]
        first += int(l[4])
    return np.concatenate(tabs), geom


def settable_error(threshold, min_sep, max_jump):
    if not (-1 <= threshold <= 509 and 0 <= min_sep <= 1 and 0 < max_jump <= 16384):
        return "threshold, min_sep or max_jump"
    return None


def open_error(w, h, lines, p):
    """what rcflow_shoreline_open refuses before it looks at the context: None, or the reason"""
    if not (p.source in (RMB, GRAY, PLANE) and 0 <= p.radius <= MAX_RADIUS and p.wet_is_high in (0, 1) and 2 <= p.window <= MAX_WINDOW and
            1 <= p.permille <= 999 and 0 < p.metres_per_pixel < math.inf) or settable_error(p.threshold, p.min_sep, p.max_jump):
        return "parameters"
    try:
        plan(w, h, lines, p.metres_per_pixel)
    except ValueError as e:
        return str(e)
    if w * h > MAX_PIXELS or 4 * p.window * len(lines) > MAX_STATE_BYTES:
        return "size"
    return None


def indicator(img, source):
    """the picture (HxWx3 uint8 as it lies in memory, or HxW for PLANE) -> int64 HxW"""
    a = img.astype(np.int64)
    if source == PLANE:
        return a
    if source == RMB:
        return a[..., 2] - a[..., 0] + 255
    return (a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14


def smooth(ind, r):
    """the box over (2 r + 1)^2 with a replicated border -> J, int64 in 0..510"""
    h, w = ind.shape
    p = np.pad(ind, r, mode="edge")
    s = np.zeros((h, w), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            s += p[dy:dy + h, dx:dx + w]
    A = (2 * r + 1) ** 2
    return (2 * s + A) // (2 * A)


def histogram(J, roi=None):
    v = J if roi is None else J[roi != 0]
    return np.bincount(v.ravel(), minlength=HIST)[:HIST].astype(np.int64)


def otsu(hist, fixed=-1):
    """hist: at least 511 counts -> (thr, eta float64, N)"""
    hh = [int(v) for v in hist[:511]]
    N = sum(hh)
    S1 = sum(i * v for i, v in enumerate(hh))
    S2 = sum(i * i * v for i, v in enumerate(hh))
    best, thr, w0, m0 = f64(-1.0), -1, 0, 0
    sfix = f64(0.0)
    for t in range(510):
        w0 += hh[t]
        m0 += t * hh[t]
        w1 = N - w0
        if w0 == 0 or w1 == 0:
            continue
        a = S1 * w0 - m0 * N
        s = (f64(a) * f64(a)) / (f64(w0) * f64(w1))
        if t == fixed:
            sfix = s
        if s > best:
            best, thr = s, t
    tot = f64(N) * f64(S2) - f64(S1) * f64(S1)
    if fixed >= 0:
        if N == 0:
            return -1, f64(0.0), 0
        return fixed, (sfix / tot if tot > 0 else f64(0.0)), N
    if thr < 0:
        return -1, f64(0.0), N
    return thr, (best / tot if tot > 0 else f64(0.0)), N


def sample(J, table, w, h):
    """the integer bilinear sample of J at the table's positions -> int64 [S]"""
    X, Y = table["X"].astype(np.int64), table["Y"].astype(np.int64)
    ix, fx, iy, fy = X >> 4, X & 15, Y >> 4, Y & 15
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    return ((16 - fx) * (16 - fy) * J[iy, ix] + fx * (16 - fy) * J[iy, ix1] + (16 - fx) * fy * J[iy1, ix] + fx * fy * J[iy1, ix1] + 128) >> 8


def is_wet(v, thr, wet_is_high):
    return (v > thr) if wet_is_high else (v <= thr)


def split(wet):
    """-> (k*, score(k*)): score(k) = #dry in [0, k) + #wet in [k, n), the smallest k of the largest"""
    n = wet.size
    dry_before = np.concatenate(([0], np.cumsum(~wet)))
    wet_from = np.concatenate((np.cumsum(wet[::-1])[::-1], [0]))
    score = dry_before + wet_from
    k = int(np.argmax(score))
    assert score.size == n + 1
    return k, int(score[k])


def frac_of(a, b, thr):
    d, e = abs(b - a), abs(2 * thr + 1 - 2 * a)
    return (e * 256 + d) // (2 * d)


def first_crossing(wet):
    """the first wet sample, or n: what the best split is measured against"""
    i = np.flatnonzero(wet)
    return int(i[0]) if i.size else wet.size


def rank_of(nv, p):
    return (nv * p + 999) // 1000 - 1


def outliers(has, wx, wy, max_jump):
    """-> bool [L]: the outlier test along the shore"""
    L, lim = len(has), int(np.rint(f64(max_jump) * 256.0))
    out = np.zeros(L, bool)
    for i in range(L):
        if not has[i]:
            continue
        nb = []
        for side in (-1, 1):
            for step in (1, 2):
                j = i + side * step
                if 0 <= j < L and has[j]:
                    nb.append(j)
                    break
        if nb and all(max(abs(int(wx[j]) - int(wx[i])), abs(int(wy[j]) - int(wy[i]))) > lim for j in nb):
            out[i] = True
    return out


class ShorelineRef:
    def __init__(self, w, h, lines, p):
        assert open_error(w, h, lines, p) is None
        self.w, self.h, self.p = w, h, Params(**asdict(p))
        self.table, self.geom = plan(w, h, lines, p.metres_per_pixel)
        self.L = len(lines)
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.L, self.p.window), np.int32)
        self.records = np.zeros(self.L, RECORD)
        self.summary = np.zeros(8, np.int64)
        self.pushes = 0

    def set(self, threshold, min_sep, max_jump):
        assert settable_error(threshold, min_sep, max_jump) is None
        self.p.threshold, self.p.min_sep, self.p.max_jump = threshold, min_sep, max_jump

    def push(self, img, roi=None):
        """-> dict(records, summary, mask, plane, hist, V): every output of the push, and the samples for the tests"""
        p, w, h, L, T = self.p, self.w, self.h, self.L, self.p.window
        J = smooth(indicator(img, p.source), p.radius)
        hist = histogram(J, roi)
        thr, eta, N = otsu(hist, p.threshold)
        V = sample(J, self.table, w, h)
        rec = np.zeros(L, RECORD)
        for i, g in enumerate(self.geom):
            n, first = int(g["n"]), int(g["first"])
            r = rec[i]
            r["pos"] = -1
            if thr < 0:
                r["flags"] = EMPTY
                continue
            v = V[first:first + n]
            wet = is_wet(v, thr, p.wet_is_high)
            k, score = split(wet)
            r["k"], r["agree"] = k, score
            if eta < p.min_sep:
                r["flags"] |= UNSURE
            if k == n:
                r["flags"] |= DRY
            elif k == 0:
                r["flags"] |= WET
            else:
                assert not wet[k - 1] and wet[k]
                a, b = int(v[k - 1]), int(v[k])
                fr = frac_of(a, b, thr)
                assert 0 <= fr <= 256
                pos = (k - 1) * 256 + fr
                Xa, Xb = int(self.table["X"][first]), int(self.table["X"][first + n - 1])
                Ya, Yb = int(self.table["Y"][first]), int(self.table["Y"][first + n - 1])
                r["pos"] = pos
                r["wx"] = 16 * Xa + (16 * (Xb - Xa) * pos + 128 * (n - 1)) // (256 * (n - 1))
                r["wy"] = 16 * Ya + (16 * (Yb - Ya) * pos + 128 * (n - 1)) // (256 * (n - 1))
        has = rec["pos"] >= 0
        out = outliers(has, rec["wx"], rec["wy"], p.max_jump)
        rec["flags"][out] |= OUTLIER
        c = self.pushes % T
        self.ring[:, c] = np.where(has & ~out, rec["pos"], -1)
        held = min(self.pushes + 1, T)
        for i, g in enumerate(self.geom):
            r, ds = rec[i], f64(g["ds"])
            vals = np.sort(self.ring[i, :held][self.ring[i, :held] >= 0].astype(np.int64))
            nv = vals.size
            if nv == 0:
                r["flags"] |= NO_WINDOW
            else:
                r["nv"], r["pos_min"], r["pos_max"], r["pos_q"] = nv, vals[0], vals[-1], vals[rank_of(nv, p.permille)]
                r["pos_mean"] = f32(f64(int(vals.sum())) / f64(nv))
                r["excursion_m"] = f32((f64(int(vals[-1] - vals[0])) / f64(256.0)) * ds)
            r["x"], r["y"] = f32(f64(int(r["wx"])) / f64(256.0)), f32(f64(int(r["wy"])) / f64(256.0))
            r["dist_m"] = f32((f64(int(r["pos"])) / f64(256.0)) * ds) if r["pos"] >= 0 else f32(0)
        self.pushes += 1
        fl = rec["flags"]
        summ = np.array([thr, N, int(np.rint(eta * f64(4294967296.0))), int((has & ~out).sum()), int(((fl & DRY) != 0).sum()),
                         int(((fl & WET) != 0).sum()), int(out.sum()), self.pushes], np.int64)
        mask = np.where(is_wet(J, thr, p.wet_is_high) & (thr >= 0), 255, 0).astype(np.uint8)
        h32 = hist.astype(np.uint32)
        h32[511:] = 0
        self.records, self.summary = rec, summ
        return dict(records=rec, summary=summ, mask=mask, plane=J.astype(np.uint16), hist=h32, V=V, thr=thr, eta=float(eta))

    def ring_read(self):
        """lines x T: per line the held slots oldest first, then -1"""
        T, held = self.p.window, min(self.pushes, self.p.window)
        out = np.full((self.L, T), -1, np.int32)
        oldest = self.pushes % T if self.pushes >= T else 0
        for r in range(held):
            out[:, r] = self.ring[:, (oldest + r) % T]
        return out

    def prims(self, color, thickness, disc_radius):
        """the 2 L - 1 primitives of the last push"""
        rec, L = self.records, self.L
        out = np.zeros(2 * L - 1, PRIM)
        ok = (rec["pos"] >= 0) & ((rec["flags"] & OUTLIER) == 0) & (self.pushes > 0)
        px, py = (rec["wx"].astype(np.int64) + 128) >> 8, (rec["wy"].astype(np.int64) + 128) >> 8
        for i in range(L):
            if not ok[i]:
                continue
            out[2 * i] = (DISC, px[i], py[i], px[i], py[i], disc_radius, color, 0)
            nxt = [j for j in range(i + 1, L) if ok[j]]
            if nxt:
                j = nxt[0]
                out[2 * i + 1] = (LINE, px[i], py[i], px[j], py[j], thickness, color, 0)
        return out


# ---------------------------------------------------------------------------- the scene
SAND, WATER, FOAM = (120.0, 170.0, 200.0), (170.0, 140.0, 90.0), (225.0, 228.0, 230.0)      # BGR


def beach_waterline(w, h, t, period=16, amp=5):
    """x_s(y, t) for y = 0..h-1"""
    y = np.arange(h, dtype=np.float64)
    return 0.45 * w + 0.08 * w * np.sin(2 * np.pi * y / h) + amp * np.sin(2 * np.pi * t / period)


def beach(w, h, t, seed=7, period=16, amp=5, foam=False, noise=6):
    """The synthetic beach at push t -> HxWx3 uint8 (BGR): sand to the left, water to the right of a waterline that swings with
    `period`, an optional foam band just seaward of it, normal noise and 1 % speckle pixels."""
    rng = np.random.default_rng(1000 * seed + t)
    d = np.arange(w, dtype=np.float64)[None, :] - beach_waterline(w, h, t, period, amp)[:, None]
    with np.errstate(over="ignore"):                          # far up the beach exp overflows to infinity and the blend is 0
        a = (1.0 / (1.0 + np.exp(-d / 0.7)))[..., None]
    img = np.array(SAND)[None, None, :] * (1.0 - a) + np.array(WATER)[None, None, :] * a
    if foam:
        f = (0.8 * np.exp(-((d - 4.0) / 3.0) ** 2))[..., None]
        img = img * (1.0 - f) + np.array(FOAM)[None, None, :] * f
    img = img + rng.normal(0.0, noise, img.shape)
    m = rng.random((h, w)) < 0.01
    img[m] = rng.integers(0, 256, (int(m.sum()), 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def beach_lines(w, h):
    """the issue's lines: horizontal, rows 4, 9, ..., from x = 4 (land) to x = w - 5 (sea), a sample a pixel"""
    return [(4.0, float(y), float(w - 5), float(y), w - 8) for y in range(4, h, 5)]


def ragged_lines(w, h):
    """diagonals with fractional ends, the last row, the last column (the ix1 and iy1 clamps), n = 8 and n = 1024"""
    return [(1.3, 2.7, w - 1.6, h - 2.2, 33), (0.0, float(h - 1), float(w - 1), float(h - 1), 40), (float(w - 1), 0.0, float(w - 1), float(h - 1), 19),
            (2.5, h - 1.25, w - 1.0, 0.0, 8), (0.0, 0.0, float(w - 1), float(h - 1), 1024), (0.4, 17.5, w - 1.4, 17.5, 129)]
