"""The motion templates (include/rcflow.h, "motion templates") in numpy: what ripcurrents_amd/csrc/motion_kernels.hip must equal
bit for bit.  float32 operation by operation, the integer sums in int64 (exact), fastAtan2 from the caller (the oracle's
orc.fast_atan2_deg, so nothing here comes from the device code).  Test infrastructure: the product never imports it."""
import numpy as np

f32, f64 = np.float32, np.float64

CELL_DTYPE = np.dtype([("angle", "<f8"), ("S", "<i8"), ("W", "<i8"), ("tsmax", "<f4"), ("n_masked", "<i4"), ("n_used", "<i4"),
                       ("peak_bin", "<i4")])
EPS = f32(1e-4) * f32(9)
TWO32 = 4294967296.0


def update(mhi, prev, cur, ts, delbound, threshold):
    """-> (history, silhouette).  prev None: no previous frame, an empty silhouette."""
    if prev is None:
        s = np.zeros(cur.shape, bool)
    else:
        s = np.abs(cur.astype(np.int32) - prev.astype(np.int32)) > int(threshold)
    kept = np.where(mhi < f32(delbound), f32(0), mhi)
    return np.where(s, f32(ts), kept).astype(f32), s


def gradient(mhi, delta1, delta2, atan2):
    """-> (orient float32, mask bool).  3 x 3, replicate border; the stated order of operations."""
    h, w = mhi.shape
    p = np.pad(mhi, 1, mode="edge")
    n = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    two = f32(2)
    dx = ((n(-1, 1) - n(-1, -1)) + two * (n(0, 1) - n(0, -1))) + (n(1, 1) - n(1, -1))
    dy = ((n(1, -1) - n(-1, -1)) + two * (n(1, 0) - n(-1, 0))) + (n(1, 1) - n(-1, 1))
    assert dx.dtype == f32 and dy.dtype == f32
    mask = ~((np.abs(dx) < EPS) & (np.abs(dy) < EPS))
    nb = np.stack([n(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)])
    d0 = nb.max(0) - nb.min(0)
    mask &= ~((d0 < f32(delta1)) | (f32(delta2) < d0))
    orient = atan2(dy, dx).reshape(h, w).astype(f32)
    return np.where(mask, orient, f32(0)).astype(f32), mask


def picture(mhi, delbound, duration):
    db, du = f32(delbound), f32(duration)
    with np.errstate(invalid="ignore"):
        v = np.where(mhi > db, (mhi - db) / du, f32(0)).astype(f32)
    g = np.clip(np.rint(v * f32(255)), 0, 255).astype(np.uint8)
    return np.repeat(g[..., None], 3, axis=2)


def cell_index(w, h, gx, gy):
    y, x = np.mgrid[0:h, 0:w]
    return np.minimum(y // (h // gy), gy - 1) * gx + np.minimum(x // (w // gx), gx - 1)


def terms(mhi, orient, base, b, dele, a):
    """Per pixel (flat arrays; base, b, dele per pixel or scalars): (used, t, wgt) in float32."""
    wgt = mhi * f32(a) + b
    rel = orient - base
    rel = rel + np.where(rel < f32(-180), f32(360), f32(0))
    rel = rel + np.where(rel > f32(180), f32(-360), f32(0))
    used = (mhi > dele) & (np.abs(rel) < f32(45))
    t = wgt * rel
    assert wgt.dtype == f32 and rel.dtype == f32 and t.dtype == f32
    return used, t, wgt


def orientations(mhi, orient, mask, idx, nsets, duration):
    """The orientation of `nsets` sets of pixels; idx: the set of every pixel.  -> records of CELL_DTYPE."""
    m = mask.ravel()
    hm, om, im = mhi.ravel()[m], orient.ravel()[m], idx.ravel()[m]
    rec = np.zeros(nsets, CELL_DTYPE)
    rec["n_masked"] = np.bincount(im, minlength=nsets)
    b12 = np.floor(om.astype(f64) * (12.0 / 360.0)).astype(np.int64)
    inb = (b12 >= 0) & (b12 < 12)
    hist = np.bincount(im[inb] * 12 + b12[inb], minlength=nsets * 12).reshape(nsets, 12)
    rec["peak_bin"] = hist.argmax(1)                     # the first maximum: the lowest bin wins a tie
    tsmax = np.zeros(nsets, f32)
    np.maximum.at(tsmax, im, hm)
    rec["tsmax"] = tsmax
    a = f32(254. / 255. / duration)
    base = (rec["peak_bin"] * 30).astype(f32)
    b = (1. - tsmax.astype(f64) * f64(a)).astype(f32)
    dele = (tsmax.astype(f64) - duration).astype(f32)
    used, t, wgt = terms(hm, om, base[im], b[im], dele[im], a)
    S, W = np.zeros(nsets, np.int64), np.zeros(nsets, np.int64)
    np.add.at(S, im[used], np.rint(t[used].astype(f64) * TWO32).astype(np.int64))
    np.add.at(W, im[used], np.rint(wgt[used].astype(f64) * TWO32).astype(np.int64))
    rec["S"], rec["W"] = S, W
    rec["n_used"] = np.bincount(im[used], minlength=nsets)
    with np.errstate(invalid="ignore", divide="ignore"):
        ang = base.astype(f64) + np.where(W != 0, S.astype(f64) / W.astype(f64), 0.)
    ang = np.where(ang >= 360., ang - 360., ang)
    rec["angle"] = np.where(ang < 0., ang + 360., ang)
    return rec


def upstream_float_sum(mhi, orient, mask, duration):
    """calcGlobalOrientation's own accumulation over the whole frame: two floats added in raster order.  -> degrees."""
    fr = orientations(mhi, orient, mask, np.zeros(mhi.shape, np.int64), 1, duration)[0]
    a = f32(254. / 255. / duration)
    base = f32(fr["peak_bin"] * 30)
    b = f32(1. - f64(fr["tsmax"]) * f64(a))
    dele = f32(f64(fr["tsmax"]) - duration)
    m = mask.ravel()
    used, t, wgt = terms(mhi.ravel()[m], orient.ravel()[m], base, b, dele, a)
    so, sw = f32(0), f32(0)
    for tv, wv in zip(t[used], wgt[used]):
        so = f32(so + tv)
        sw = f32(sw + wv)
    ang = f64(base) + (f64(so / sw) if sw != 0 else 0.)      # upstream: shiftOrient /= shiftWeight in float
    ang -= 360. if ang >= 360. else 0.
    ang += 360. if ang < 0. else 0.
    return ang


def prims(cells, frame, w, h, color, thickness, radius, length):
    """The records as 2 * (cells + 1) primitives (kind, x0, y0, x1, y1, size, color, flags), int64 rows."""
    gy, gx = cells.shape
    out = np.zeros((2 * (gx * gy + 1), 8), np.int64)
    cw, ch = w // gx, h // gy
    sets = [(cells[cy, cx], (cx * cw + (w if cx == gx - 1 else (cx + 1) * cw) - 1) // 2,
             (cy * ch + (h if cy == gy - 1 else (cy + 1) * ch) - 1) // 2) for cy in range(gy) for cx in range(gx)]
    sets.append((frame, (w - 1) // 2, (h - 1) // 2))
    for i, (r, px, py) in enumerate(sets):
        if not r["W"]:
            continue
        rad = float(r["angle"]) * (np.pi / 180.0)
        out[2 * i] = (1, px, py, px, py, radius, color, 0)
        out[2 * i + 1] = (2, px, py, px + int(np.rint(length * np.cos(rad))), py + int(np.rint(length * np.sin(rad))), thickness, color, 0)
    return out


class MotionRef:
    def __init__(self, w, h, atan2, diff_threshold=30, duration=1.0, delta1=0.25, delta2=1.0, grid=(1, 1), fresh=False):
        self.w, self.h, self.atan2, self.thr, self.grid, self.fresh = w, h, atan2, diff_threshold, grid, fresh
        self.duration = 1.0 if fresh else float(duration)
        self.d1, self.d2 = min(delta1, delta2), max(delta1, delta2)      # swapped, as upstream does
        self.idx = cell_index(w, h, *grid)
        self.reset()

    def reset(self):
        self.mhi, self.prev, self.pushes = np.zeros((self.h, self.w), f32), None, 0

    def push(self, gray, timestamp=None):
        ts = float(self.pushes + 1) if timestamp is None else float(timestamp)
        if self.fresh:
            ts, self.mhi = 1.0, np.zeros((self.h, self.w), f32)
        delbound = f32(ts - self.duration)
        self.mhi, s = update(self.mhi, self.prev, gray, f32(ts), delbound, self.thr)
        self.prev, self.pushes = gray.copy(), self.pushes + 1
        orient, mask = gradient(self.mhi, self.d1, self.d2, self.atan2)
        gx, gy = self.grid
        cells = orientations(self.mhi, orient, mask, self.idx, gx * gy, self.duration).reshape(gy, gx)
        frame = orientations(self.mhi, orient, mask, np.zeros_like(self.idx), 1, self.duration)[0]
        return dict(mhi=self.mhi.copy(), orient=orient, mask=np.where(mask, 255, 0).astype(np.uint8),
                    vis=picture(self.mhi, delbound, self.duration), cells=cells, frame=frame, angle=float(frame["angle"]),
                    silhouette=int(s.sum()))


# ---------------------------------------------------------------------------- clips
def bar_clip(direction, w=67, h=45, n=30, width=9):
    """A full-height (or full-width) bar, 200 on 50, moving 1 px per frame along +x, -x, +y or -y."""
    out = []
    for t in range(n):
        f = np.full((h, w), 50, np.uint8)
        if direction in ("+x", "-x"):
            x0 = 5 + t if direction == "+x" else w - 5 - width - t
            f[:, max(x0, 0):max(x0 + width, 0)] = 200
        else:
            y0 = 3 + t if direction == "+y" else h - 3 - width - t
            f[max(y0, 0):max(y0 + width, 0), :] = 200
        out.append(f)
    return out


def diagonal_clip(sx, sy, w=67, h=45, n=30, width=18):
    """A bar 18 wide in u = sx * x + sy * y, moving 2 per frame in u."""
    y, x = np.mgrid[0:h, 0:w]
    u = sx * x + sy * y
    lo = int(u.min())
    return [np.where((u >= lo + 4 + 2 * t) & (u < lo + 4 + 2 * t + width), 200, 50).astype(np.uint8) for t in range(n)]


def texture(w, h, seed=2, sigma=2.0):
    """Gaussian-smoothed noise scaled to 0..255, with a margin of 40 columns to slide a window over.  The direction the
    templates read off a moving texture is biased by what the texture holds: seeds 1..11 at 97 x 61 land between 357.6 and 4.3
    degrees for a motion along +x; seed 2 stays within 1 degree on both sides of the seam."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((h, w + 40))
    r = int(4 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="wrap"), k, mode="valid"), 1, a)
    a = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode="wrap"), k, mode="valid"), 0, a)
    a = (a - a.min()) / (a.max() - a.min())
    return np.rint(a * 255).astype(np.uint8)


def texture_clip(w, h, n, step=1, seed=2):
    """The texture moving +x by `step` px per frame."""
    t = texture(w, h, seed)
    return [np.ascontiguousarray(t[:, 40 - step * k:40 - step * k + w]) for k in range(n)]
