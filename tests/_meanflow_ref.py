"""The mean current (include/rcflow.h, "mean flow") stated in numpy: the fixed-point sample, the ring, the seven sums per pixel, the
mean, the steadiness, the spread, the picture, the cell sums, the global vector, the mask, the records and the summary.  Integers
are int64 and exact; the float results are float64 operation by operation, in the order the header gives, then rounded to float32.
No angle is computed anywhere.  Also the scenes the tests look at."""
import math
from dataclasses import asdict, dataclass

import numpy as np

DIR_FIXED, DIR_OPPOSED = 1, 2
EMPTY = 1
MAX_WINDOW, MAX_CELLS, MAX_STATE_BYTES, SUMS = 4096, 16384, 4 << 30, 8
BAD_U = -32768                  # the ring's u of a bad sample
LIMIT = 500.0                   # |component| at and above this is bad
f32, f64, i64 = np.float32, np.float64, np.int64

CELL = np.dtype([("flags", "<i4"), ("filled", "<i4"), ("mask", "<i4"), ("bad", "<i4"), ("mean_x", "<f4"), ("mean_y", "<f4"), ("steadiness", "<f4"),
                 ("pad", "<i4")])
SUMMARY = ("filled", "mask", "bad", "gx", "gy", "sum_m", "held", "pushes")
PICTURES = ("mean", "steady", "std", "mask", "picture")


@dataclass
class Params:
    window: int = 8
    grid_x: int = 1
    grid_y: int = 1
    min_fill: int = 8
    steady_min: int = 600
    flags: int = DIR_FIXED
    speed_min: float = 0.5
    min_cos2: float = 0.5
    dir_x: float = 0.0
    dir_y: float = -1.0

    def kw(self):
        """the keywords of Context.meanflow_open"""
        d = asdict(self)
        d["opposed"] = d.pop("flags") == DIR_OPPOSED
        return d


def settable_error(p):
    if not (0 <= p.steady_min <= 1000 and 1 <= p.min_fill <= p.window and math.isfinite(p.speed_min) and 0. <= p.speed_min <= 400. and
            0. <= p.min_cos2 < 1.):
        return "steady_min, min_fill, speed_min or min_cos2"
    if p.flags == DIR_FIXED and not (math.isfinite(p.dir_x) and math.isfinite(p.dir_y) and (p.dir_x != 0. or p.dir_y != 0.)):
        return "direction"
    return None


def state_bytes(w, h, window):
    """the ring and the seven sum planes as the header lays them out"""
    P = (w + 3) & ~3
    return P * h * (4 * window + 38)


def open_error(w, h, p):
    """what rcflow_meanflow_open refuses before it looks at the context: None, or the reason"""
    if not (w > 0 and h > 0 and 2 <= p.window <= MAX_WINDOW and p.flags in (DIR_FIXED, DIR_OPPOSED)) or settable_error(p):
        return "parameters"
    if not (1 <= p.grid_x <= w and 1 <= p.grid_y <= h and p.grid_x * p.grid_y <= MAX_CELLS):
        return "grid"
    if state_bytes(w, h, p.window) > MAX_STATE_BYTES:
        return "size"
    return None


def isqrt(v):
    """the exact floor square root of an int64 array"""
    v = np.asarray(v, i64)
    r = np.floor(np.sqrt(v.astype(f64))).astype(i64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def quantize(flow):
    """flow [h][w][2] float32 -> (bad [h][w] bool, qu, qv int64): a component that is not finite or fabsf(component) >= 500 makes
    the sample bad; otherwise q = rint(component * 64) in float32, |q| <= 32000"""
    f = np.asarray(flow, f32)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(f) < f32(LIMIT)).all(axis=2)          # NaN and inf fail the comparison
        q = np.rint(np.where(bad[..., None], f32(0), f) * f32(64.0)).astype(i64)
    return bad, q[..., 0], q[..., 1]


def cell_index(w, h, gx, gy):
    """the opposing-flow map's cell rule: cells of w // gx by h // gy pixels, the remainder columns and rows to the last cell"""
    cw, ch = w // gx, h // gy
    cx = np.minimum(np.arange(w) // cw, gx - 1)
    cy = np.minimum(np.arange(h) // ch, gy - 1)
    return (cy[:, None] * gx + cx[None, :]).ravel()


class MeanFlowRef:
    def __init__(self, w, h, p, lut):
        assert open_error(w, h, p) is None
        self.w, self.h, self.p, self.lut = w, h, Params(**asdict(p)), np.asarray(lut, np.uint8).reshape(256, 3)
        self.cell = cell_index(w, h, p.grid_x, p.grid_y)
        self.reset()

    def reset(self):
        W, h, w = self.p.window, self.h, self.w
        self.ru = np.full((W, h, w), BAD_U, i64)              # bad / never written
        self.rv = np.zeros((W, h, w), i64)
        self.n, self.Su, self.Sv, self.Suu, self.Svv, self.Suv, self.Sm = (np.zeros((h, w), i64) for _ in range(7))
        self.pushes = 0
        nc = self.p.grid_x * self.p.grid_y
        self.cells, self.sums, self.summary = np.zeros(nc, CELL), np.zeros((nc, SUMS), i64), np.zeros(8, i64)

    def set(self, **kw):
        q = Params(**{**asdict(self.p), **kw})
        if settable_error(q):
            raise ValueError(settable_error(q))
        self.p = q

    def update(self, flow):
        """the ring and the sums of one push -> bad [h][w]"""
        c = self.pushes % self.p.window
        bad, u, v = quantize(flow)
        ou, ov = self.ru[c], self.rv[c]
        old = (ou != BAD_U).astype(i64)
        ou, ov = ou * old, ov * old
        new = (~bad).astype(i64)
        self.n += new - old
        self.Su += u - ou
        self.Sv += v - ov
        self.Suu += u * u - ou * ou
        self.Svv += v * v - ov * ov
        self.Suv += u * v - ou * ov
        self.Sm += isqrt(u * u + v * v) - isqrt(ou * ou + ov * ov)
        self.ru[c] = np.where(bad, BAD_U, u)
        self.rv[c] = np.where(bad, 0, v)
        self.pushes += 1
        return bad

    def bounds(self):
        """the largest magnitudes of what the device narrows or multiplies, as Python integers"""
        n = self.n.astype(object)
        Su, Sv = self.Su.astype(object), self.Sv.astype(object)
        out = dict(S=max(abs(Su).max(), abs(Sv).max()), Sm=self.Sm.astype(object).max(),
                   nS2=max((n * self.Suu.astype(object)).max(), (n * self.Svv.astype(object)).max(), abs(n * self.Suv.astype(object)).max()),
                   SS=(Su * Su + Sv * Sv).max())
        return {k: int(v) for k, v in out.items()}

    def steadiness(self):
        """-> (R, st): R = isqrt(Su^2 + Sv^2), st = min(1000, R 1000 / Sm), 0 where Sm = 0"""
        R = isqrt(self.Su * self.Su + self.Sv * self.Sv)
        st = np.where(self.Sm > 0, np.minimum(1000, R * 1000 // np.maximum(self.Sm, 1)), 0)
        return R, st

    def push(self, flow, pictures=True):
        """-> dict of every output of the push (the pictures only when asked for; what the state becomes does not depend on it)"""
        p, w, h = self.p, self.w, self.h
        bad = self.update(flow)
        n, Su, Sv, Sm = self.n, self.Su, self.Sv, self.Sm
        filled = n >= p.min_fill
        R, st = self.steadiness()
        nc = p.grid_x * p.grid_y
        fi = filled.ravel()

        sums = np.zeros((nc, SUMS), i64)
        sums[:, 0] = np.bincount(self.cell[fi], minlength=nc)
        sums[:, 1] = _isum(self.cell[fi], n.ravel()[fi], nc)
        sums[:, 2] = _isum(self.cell[fi], Su.ravel()[fi], nc)
        sums[:, 3] = _isum(self.cell[fi], Sv.ravel()[fi], nc)
        sums[:, 4] = _isum(self.cell[fi], Sm.ravel()[fi], nc)
        sums[:, 6] = np.bincount(self.cell[bad.ravel()], minlength=nc)
        Gx, Gy = int(sums[:, 2].sum()), int(sums[:, 3].sum())
        # the mask: exact integers, then the direction in double as the opposing-flow map decides its cells
        smin_q = math.ceil(p.speed_min * 64.0)
        Sx, Sy = Su.astype(f64), Sv.astype(f64)
        Dx, Dy = (f64(p.dir_x), f64(p.dir_y)) if p.flags == DIR_FIXED else (-f64(Gx), -f64(Gy))
        dot = Sx * Dx + Sy * Dy
        cc = Sx * Sx + Sy * Sy
        dd = Dx * Dx + Dy * Dy
        mask = filled & (st >= p.steady_min) & (R >= smin_q * n) & (dot > 0) & (dot * dot >= f64(p.min_cos2) * (cc * dd))
        sums[:, 5] = np.bincount(self.cell[mask.ravel()], minlength=nc)
        cells = np.zeros(nc, CELL)
        for c in range(nc):
            nf, sn, sx, sy, sm = (int(x) for x in sums[c, :5])
            cells[c]["filled"], cells[c]["mask"], cells[c]["bad"] = nf, sums[c, 5], sums[c, 6]
            if nf == 0:
                cells[c]["flags"] = EMPTY
                continue
            cells[c]["mean_x"] = f32((f64(sx) / f64(64.0)) / f64(sn))
            cells[c]["mean_y"] = f32((f64(sy) / f64(64.0)) / f64(sn))
            if sm > 0:
                dx, dy = f64(sx), f64(sy)
                cells[c]["steadiness"] = f32((np.sqrt(dx * dx + dy * dy) / f64(sm)) * f64(1000.0))
        summary = np.array([sums[:, 0].sum(), sums[:, 5].sum(), sums[:, 6].sum(), Gx, Gy, sums[:, 4].sum(), min(self.pushes, p.window), self.pushes], i64)
        self.cells, self.sums, self.summary = cells, sums, summary
        out = dict(cells=cells, sums=sums, summary=summary, mask=np.where(mask, 255, 0).astype(np.uint8))
        if not pictures:
            return out
        nd = np.maximum(n, 1).astype(f64)
        mean = np.zeros((h, w, 2), f32)
        mean[..., 0] = np.where(filled, (Sx / 64.0) / nd, 0.).astype(f32)
        mean[..., 1] = np.where(filled, (Sy / 64.0) / nd, 0.).astype(f32)
        a, c, b = n * self.Suu - Su * Su, n * self.Svv - Sv * Sv, n * self.Suv - Su * Sv
        assert (a >= 0).all() and (c >= 0).all()
        A, B, C = a.astype(f64), b.astype(f64), c.astype(f64)
        r = np.sqrt((A - C) * (A - C) + 4.0 * (B * B))
        l1 = ((A + C) + r) * 0.5
        l2 = np.maximum(((A + C) - r) * 0.5, 0.)
        std = np.zeros((h, w, 2), f32)
        std[..., 0] = np.where(filled, np.sqrt(l1) / (64.0 * nd), 0.).astype(f32)
        std[..., 1] = np.where(filled, np.sqrt(l2) / (64.0 * nd), 0.).astype(f32)
        picture = np.where(filled[..., None], self.lut[st * 255 // 1000], 0).astype(np.uint8)
        out.update(mean=mean, steady=np.where(filled, st, 0).astype(np.uint16), std=std, picture=picture)
        return out


def _isum(idx, val, nc):
    """exact int64 sums of val per index"""
    out = np.zeros(nc, i64)
    np.add.at(out, idx, val.astype(i64))
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def naming_scene(t, w=20, h=12, drift=0.5, jet=(8, 12), jet_v=-2.5, amp=3.0, seed=7):
    """Field t of the scene the product is named for: waves v = drift + amp sin(2 pi t / 4 + 0.3 x), u = 0.7 cos(2 pi t / 4 + 0.2 y),
    a jet of jet_v px in v on columns jet[0]..jet[1] - 1, seeded noise of sigma 0.2 -> [h][w][2] float32"""
    rng = np.random.default_rng(seed * 1000 + t)
    x, y = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    v = drift + amp * np.sin(2 * np.pi * t / 4 + 0.3 * x)
    u = 0.7 * np.cos(2 * np.pi * t / 4 + 0.2 * y)
    v[:, jet[0]:jet[1]] += jet_v
    f = np.stack([u, v], -1) + rng.normal(0., 0.2, (h, w, 2))
    return np.ascontiguousarray(f, f32)


def jet_mask(w=20, h=12, jet=(8, 12)):
    m = np.zeros((h, w), np.uint8)
    m[:, jet[0]:jet[1]] = 255
    return m


NAMING = Params(window=8, grid_x=4, grid_y=3, min_fill=8, steady_min=600, flags=DIR_FIXED, speed_min=0.5, min_cos2=0.5, dir_x=0., dir_y=-1.)
# the same waves on a drift of +1 px in v with a jet of -4 px on 2 of 20 columns: G points down the picture, the jet against it
OPPOSED = Params(window=8, grid_x=4, grid_y=3, min_fill=8, steady_min=750, flags=DIR_OPPOSED, speed_min=0.5, min_cos2=0.5)
OPPOSED_SCENE = dict(drift=1.0, jet=(9, 11), jet_v=-4.0)


def hostile_field(w, h, t, seed=3):
    """a field with every kind of bad sample in places that move with t, and good values up to the limit"""
    rng = np.random.default_rng(seed * 7919 + t)
    f = rng.uniform(-6., 6., (h, w, 2)).astype(f32)
    specials = [np.nan, np.inf, -np.inf, 500.0, -500.0, 499.99997, -499.99997, 0.0]
    k = rng.integers(0, len(specials), (h, w))
    hit = rng.random((h, w)) < 0.3
    comp = rng.integers(0, 3, (h, w))                         # 0: u, 1: v, 2: both
    sp = np.array(specials, f32)[k]
    f[..., 0] = np.where(hit & (comp != 1), sp, f[..., 0])
    f[..., 1] = np.where(hit & (comp != 0), sp, f[..., 1])
    return f
