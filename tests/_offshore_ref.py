"""The offshore frame (include/rcflow.h, "offshore frame") stated in numpy: the exact distance map by brute force over all pairs of
pixels, the classes, the cross and along components, every output, the table, the records, the summaries and the band.  Integers are
int64 and exact; the only floats are v / 64 in float32, which is exact, and the records' means in float64 operation by operation.
Also the prototype of the issue and the shores the tests look at."""
from dataclasses import asdict, dataclass

import numpy as np

from _meanflow_ref import quantize                   # the mean current's sample rule, word for word

FAR = 0x7fffffff
STATION_X, STATION_Y = 1, 2
OK, NEAR, C_FAR, DRY, BAD = 0, 1, 2, 3, 4
EMPTY, RIP = 1, 2
MAX_DIST, MAX_STATIONS, MAX_BINS, MAX_BIN_WIDTH, MAX_SIDE, SUMS, SUMMARY_WORDS = 4095, 256, 256, 256, 32767, 4, 8
NAN_BITS = 0x7fc00000
f32, f64, i64 = np.float32, np.float64, np.int64

STATION = np.dtype([("flags", "<i4"), ("first", "<i4"), ("reach_end", "<i4"), ("peak_bin", "<i4"), ("peak_cross", "<i4"), ("count", "<i4"),
                    ("beyond", "<i4"), ("pad0", "<i4"), ("mean_cross", "<f4"), ("mean_along", "<f4"), ("pad1", "<i4", (2,))])
MAP_SUMMARY = ("wet", "dry", "wet_near_shore", "max_d2", "sum_d2_wet", "sum_d2_dry", "zero", "maps")
PUSH_SUMMARY = ("ok", "near", "far", "dry", "bad", "mask", "rips", "pushes")
MAP_PLANES = ("dist2", "near", "sdist", "picture")
PUSH_PLANES = ("cross_along", "cls", "mask", "picture")
DRY_BGR, FAR_BGR, NEAR_BGR, BAD_BGR = (64, 64, 64), (0, 0, 0), (128, 128, 128), (255, 0, 255)


@dataclass
class Params:
    min_dist: int = 0
    max_dist: int = 4095
    stations: int = 1
    bins: int = 1
    bin_width: int = 1
    min_count: int = 1
    rip_bins: int = 1
    cross_min: float = 0.0
    station: str = "x"

    def kw(self):
        """the keywords of Context.offshore_open"""
        return asdict(self)


def params_error(p):
    """what rcflow_offshore_open and rcflow_offshore_set refuse in the parameters: None, or the reason"""
    ok = (1 <= p.max_dist <= MAX_DIST and 0 <= p.min_dist <= p.max_dist and 1 <= p.stations <= MAX_STATIONS and 1 <= p.bins <= MAX_BINS and
          1 <= p.bin_width <= MAX_BIN_WIDTH and p.min_count >= 1 and 1 <= p.rip_bins <= p.bins and np.isfinite(p.cross_min) and
          0 <= p.cross_min <= 400 and p.station in ("x", "y"))
    return None if ok else "parameters"


def ceil64(v):
    """(int)ceil((double)(float)v * 64.0)"""
    return int(np.ceil(f64(f32(v)) * 64.0))


def rdiv(a, b):
    """floor((2 a + b) / (2 b)), the floor towards minus infinity; b > 0 (numpy's // floors)"""
    return (2 * a + b) // (2 * b)


def isqrt64(v):
    """floor(sqrt(v)) of int64 values below 2^52, exactly"""
    v = np.asarray(v, i64)
    r = np.floor(np.sqrt(v.astype(f64))).astype(i64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def distance_map(wet, chunk=None, count_ties=False):
    """wet [h][w], non-zero is water -> (d2 [h][w] int64, near [h][w] int64[, pixels at which several candidates attain d2]): over
    all pixels of the other class the least squared distance and the smallest raster index that attains it; FAR and -1 without one.
    Brute force, a chunk of pixels against every candidate at a time"""
    c = np.asarray(wet) != 0
    h, w = c.shape
    idx = np.arange(h * w)
    ys, xs = idx // w, idx % w
    d2 = np.full(h * w, FAR, i64)
    near = np.full(h * w, -1, i64)
    tied = 0
    flat = c.ravel()
    for cls in (False, True):
        mine, other = idx[flat == cls], idx[flat != cls]      # both in raster order
        if not mine.size or not other.size:
            continue
        oy, ox = ys[other].astype(np.int32), xs[other].astype(np.int32)
        step = chunk or max(1, (1 << 24) // other.size)
        for k in range(0, mine.size, step):
            m = mine[k:k + step]
            dy, dx = ys[m].astype(np.int32)[:, None] - oy[None, :], xs[m].astype(np.int32)[:, None] - ox[None, :]
            dd = dy * dy + dx * dx                            # int32: below 2^31 by MAX_SIDE
            j = dd.argmin(axis=1)                             # the first of several: the smallest raster index
            d2[m] = dd[np.arange(m.size), j]
            near[m] = other[j]
            if count_ties:
                tied += int(((dd == dd.min(axis=1)[:, None]).sum(axis=1) > 1).sum())
    out = (d2.reshape(h, w), near.reshape(h, w))
    return out + (tied,) if count_ties else out


_MAPS = {}


class OffshoreRef:
    def __init__(self, w, h, p, lut):
        assert params_error(p) is None and 0 < w <= MAX_SIDE and 0 < h <= MAX_SIDE
        self.w, self.h, self.p, self.lut = w, h, Params(**asdict(p)), np.asarray(lut, np.uint8).reshape(256, 3)
        self.reset()

    def reset(self):
        self.maps = self.pushes = 0
        self.wet = self.d2 = self.near_ = self.r = None

    def set(self, p):
        assert params_error(p) is None and (p.stations, p.bins) == (self.p.stations, self.p.bins)
        self.p = Params(**asdict(p))

    # ------------------------------------------------------------------ the map
    def map(self, wet):
        wet = np.asarray(wet) != 0
        assert wet.shape == (self.h, self.w)
        key = (wet.shape, wet.tobytes())
        if key not in _MAPS:                                  # the brute force once per shore, shared by the tests and never changed
            _MAPS[key] = distance_map(wet)
        d2, near = _MAPS[key]
        far = d2 == FAR
        r = np.where(far, FAR, isqrt64(4096 * np.where(far, 0, d2)))
        self.wet, self.d2, self.near_, self.r, self.far = wet, d2, near, r, far
        self.maps += 1
        sign = np.where(wet, 1, -1)
        pic = np.zeros((self.h, self.w, 3), np.uint8)
        pic[~wet] = DRY_BGR
        pic[wet] = self.lut[np.minimum(r[wet] // 64, self.p.max_dist) * 255 // self.p.max_dist]
        pic[far] = FAR_BGR
        shore = wet & ~far
        summary = np.array([wet.sum(), (~wet).sum(), shore.sum(), d2[shore].max(initial=0), d2[shore].sum(), d2[~wet & ~far].sum(), 0, self.maps], i64)
        return dict(dist2=(sign * d2).astype(np.int32), near=near.astype(np.int32), sdist=(sign * r).astype(np.int32), picture=pic, summary=summary,
                    sides=dict(d2=d2, r=r, wet=wet, far=far))

    # ------------------------------------------------------------------ the push
    def push(self, flow):
        assert self.d2 is not None, "a push before any map is RC_ESTATE"
        p, w, h = self.p, self.w, self.h
        d2, r = self.d2, self.r
        bad, qx, qy = quantize(flow)
        cls = np.full((h, w), OK, i64)
        cls[bad] = BAD
        cls[d2 < p.min_dist ** 2] = NEAR
        cls[self.far | (d2 > p.max_dist ** 2)] = C_FAR
        cls[~self.wet] = DRY
        ok = cls == OK
        y, x = np.mgrid[0:h, 0:w]
        nx, ny = np.where(ok, x - self.near_ % w, 0), np.where(ok, y - self.near_ // w, 0)
        C, A = qx * nx + qy * ny, -qx * ny + qy * nx
        assert np.abs(C[ok]).max(initial=0) < 2 ** 31 and np.abs(A[ok]).max(initial=0) < 2 ** 31
        r1 = np.where(ok, r, 1)
        cross, along = np.where(ok, rdiv(64 * C, r1), 0), np.where(ok, rdiv(64 * A, r1), 0)
        assert np.abs(cross).max(initial=0) < 2 ** 24 and np.abs(along).max(initial=0) < 2 ** 24
        cmin_q = ceil64(p.cross_min)
        in_mask = ok & (cross >= cmin_q)
        ca = np.full((h, w, 2), NAN_BITS, np.uint32).view(f32)
        ca[ok] = np.stack([cross[ok].astype(f32) / f32(64.0), along[ok].astype(f32) / f32(64.0)], -1)
        S = max(4 * cmin_q, 1)
        c = np.clip(cross, -S, S)
        m = (255 - np.abs(c) * 255 // S).astype(np.uint8)
        full = np.full((h, w), 255, np.uint8)
        pic = np.where((c >= 0)[..., None], np.stack([m, m, full], -1), np.stack([full, m, m], -1))
        for k, bgr in ((DRY, DRY_BGR), (C_FAR, FAR_BGR), (NEAR, NEAR_BGR), (BAD, BAD_BGR)):
            pic[cls == k] = bgr
        # the table
        bin_ = r1 // (64 * p.bin_width)
        st = x * p.stations // w if p.station == "x" else y * p.stations // h
        inside = ok & (bin_ < p.bins)
        table = np.zeros((p.stations, p.bins, SUMS), i64)
        for k, v in enumerate((np.ones((h, w), i64), cross, along, in_mask.astype(i64))):
            np.add.at(table[..., k], (st[inside], bin_[inside]), v[inside])
        beyond = np.bincount(st[ok & (bin_ >= p.bins)], minlength=p.stations)
        # the records
        recs = np.zeros(p.stations, STATION)
        recs["beyond"] = beyond
        for s in range(p.stations):
            n, sc, sa = (table[s, :, k] for k in range(3))
            enough = n >= p.min_count
            if not enough.any():
                recs[s]["flags"] = EMPTY
                continue
            first = int(np.argmax(enough))
            passes = enough & (sc >= cmin_q * n)
            passes[:first] = False
            b = first
            while b < p.bins and passes[b]:
                b += 1
            end = 0 if b == first else b
            peak, peak_cross = -1, 0
            for k in range(first, p.bins):
                if passes[k]:
                    mean = int(rdiv(int(sc[k]), int(n[k])))
                    if peak < 0 or mean > peak_cross:
                        peak, peak_cross = k, mean
            cnt, scr, sar = int(n[first:end].sum()), int(sc[first:end].sum()), int(sa[first:end].sum())
            rec = recs[s]
            rec["first"], rec["reach_end"], rec["peak_bin"], rec["peak_cross"], rec["count"] = first, end, peak, peak_cross, cnt
            if cnt:
                rec["mean_cross"] = f32((f64(scr) / f64(64.0)) / f64(cnt))
                rec["mean_along"] = f32((f64(sar) / f64(64.0)) / f64(cnt))
            if end - first >= p.rip_bins:
                rec["flags"] |= RIP
        self.pushes += 1
        summary = np.array([(cls == k).sum() for k in range(5)] + [in_mask.sum(), ((recs["flags"] & RIP) != 0).sum(), self.pushes], i64)
        return dict(cross_along=ca, cls=cls.astype(np.uint8), mask=np.where(in_mask, 255, 0).astype(np.uint8), picture=pic, stations=recs,
                    table=table.reshape(-1, SUMS), summary=summary, sides=dict(cross=cross, along=along, ok=ok, bin=bin_, station=st, beyond=beyond))

    # ------------------------------------------------------------------ the band
    def band(self, lo, hi):
        assert self.d2 is not None and 0 <= lo <= hi <= 65536
        return np.where(self.wet & ~self.far & (self.r >= ceil64(lo)) & (self.r < ceil64(hi)), 255, 0).astype(np.uint8)


# ---------------------------------------------------------------------------- shores and fields of the tests
def beach(w, h, base=20.0, amp=4.0, period=48.0):
    """land at the top: wet where y >= rint(base + amp sin(2 pi x / period))"""
    x = np.arange(w)
    line = np.rint(base + amp * np.sin(2 * np.pi * x / period)).astype(i64)
    return np.where(np.arange(h)[:, None] >= line[None, :], 255, 0).astype(np.uint8)


def speckle(w, h, wet_share, seed):
    return np.where(np.random.default_rng(seed).random((h, w)) < wet_share, 255, 0).astype(np.uint8)


def jet_field(w, h, x0, x1, base=(1.0, -0.25), jet=(1.0, 2.0)):
    """`base` everywhere, `jet` in the columns x0..x1-1"""
    f = np.empty((h, w, 2), f32)
    f[...] = np.asarray(base, f32)
    f[:, x0:x1] = np.asarray(jet, f32)
    return f


def wavy_field(w, h, seed=0):
    """a smooth field with both signs of cross and along on any shore, of 1/16 pixel steps"""
    y, x = np.mgrid[0:h, 0:w]
    u = ((x * 7 + y * 13 + seed) % 97 - 48).astype(f32) / f32(16.0)
    v = ((x * 5 + y * 11 + x * y + 3 * seed) % 89 - 30).astype(f32) / f32(16.0)
    return np.stack([u, v], -1)


def hostile(flow, seed):
    """NaN, the infinities, +-500.0, +-499.99 and -0.0 scattered over a copy of the field"""
    f = np.array(flow, f32)
    rng = np.random.default_rng(seed)
    vals = np.array([np.nan, np.inf, -np.inf, 500.0, -500.0, 499.99, -499.99, -0.0], f32)
    n = max(8, f.shape[0] * f.shape[1] // 12)
    ys, xs, cs = rng.integers(0, f.shape[0], n), rng.integers(0, f.shape[1], n), rng.integers(0, 2, n)
    f[ys, xs, cs] = vals[np.arange(n) % vals.size]
    return f


PROTOTYPE = Params(min_dist=3, max_dist=40, stations=8, bins=8, bin_width=5, min_count=8, rip_bins=3, cross_min=1.0, station="x")


def prototype():
    """the issue's case -> (w, h, wet, flow, Params)"""
    w, h = 96, 64
    flow = jet_field(w, h, 48, 60)
    flow[30, 10] = np.nan
    return w, h, beach(w, h), flow, PROTOTYPE
