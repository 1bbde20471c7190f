"""The virtual drifters (include/rcflow.h, "drifters") stated in numpy: the fixed-point sample, the state of a drifter, the release,
the move through the four-vector gather, the fates in their order, the occupancy and the density, the two cell tables, the
histograms, the summary and the records.  Integers are int64 here and exact (the device's int32 and uint32 words hold them); the
few floats are float64 operation by operation, then rounded to float32.  Also the zones helper's three lines and the scenes the
tests look at."""
from dataclasses import asdict, dataclass

import numpy as np

WAITING, ALIVE = -1, 0
EDGE_LEFT, EDGE_TOP, EDGE_RIGHT, EDGE_BOTTOM, BAD, AGED = 1, 2, 3, 4, 5, 6
ZONE0 = 8                       # fate 8 + z of zone z = 1..7
SHORE, OFFSHORE = 9, 10
RESPAWN = 1                     # Params.flags
EMPTY = 1                       # a record's flag
MAX_DRIFTERS, MAX_CELLS, SUMS, HIST_BINS, SUMMARY_WORDS = 1 << 22, 16384, 8, 32, 24
LIMIT = 500.0
f32, f64, i64 = np.float32, np.float64, np.int64

CELL = np.dtype([("flags", "<i4"), ("pad0", "<i4"), ("mean_u", "<f4"), ("mean_v", "<f4"), ("escape", "<f4"), ("beached", "<f4"),
                 ("mean_exit_age", "<f4"), ("pad1", "<i4")])
SUMMARY = ("drifters", "alive", "released", "pushes", "age_shore", "age_offshore", "zero6", "zero7") + tuple("fate%d" % f for f in range(16))
PLACE = ("visits", "su", "sv", "shore", "offshore", "edge", "other", "age_offshore")
ORIGIN = ("released", "shore", "offshore", "edge", "other", "age_shore", "age_offshore", "zero")
PIXEL_OUTPUTS = ("now", "density", "live", "picture")
DRIFTER_OUTPUTS = ("xy", "age", "state")


@dataclass
class Params:
    max_drifters: int = 4096
    grid_x: int = 1
    grid_y: int = 1
    dt: float = 1.0
    max_age: int = 0
    age_bin: int = 8
    density_full: int = 16
    live_min: int = 1
    flags: int = 0

    def kw(self):
        """the keywords of Context.drifters_open"""
        d = asdict(self)
        d["respawn"] = bool(d.pop("flags") & RESPAWN)
        return d


def dt_q(dt):
    """rint(dt * 256), which must lie in 1..65536; None otherwise"""
    if not np.isfinite(dt):
        return None
    q = int(np.rint(f64(dt) * 256.0))
    return q if 1 <= q <= 65536 else None


def settable_error(p):
    if dt_q(p.dt) is None or p.max_age < 0 or p.density_full < 1 or p.live_min < 1 or p.flags & ~RESPAWN:
        return "dt, max_age, density_full, live_min or flags"
    return None


def open_error(w, h, p):
    """what rcflow_drifters_open refuses before it looks at the context: None, or the reason"""
    if not (w > 0 and h > 0 and 1 <= p.max_drifters <= MAX_DRIFTERS and p.age_bin >= 1) or settable_error(p):
        return "parameters"
    if not (1 <= p.grid_x <= w and 1 <= p.grid_y <= h and p.grid_x * p.grid_y <= MAX_CELLS):
        return "grid"
    return None


def quantize(flow):
    """flow [h][w][2] float32 -> (bad [h][w] bool, qu, qv int64): the mean current's sample, word for word"""
    f = np.asarray(flow, f32)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(f) < f32(LIMIT)).all(axis=2)
        q = np.rint(np.where(bad[..., None], f32(0), f) * f32(64.0)).astype(i64)
    return bad, q[..., 0], q[..., 1]


def cell_of(x, y, w, h, gx, gy):
    """the opposing-flow map's cell of pixel (x, y)"""
    return np.minimum(y // (h // gy), gy - 1) * gx + np.minimum(x // (w // gx), gx - 1)


def fate_class(f):
    """0 SHORE, 1 OFFSHORE, 2 EDGE, 3 other"""
    f = np.asarray(f)
    return np.where(f == SHORE, 0, np.where(f == OFFSHORE, 1, np.where((f >= 1) & (f <= 4), 2, 3)))


def seed_points(xy, w, h):
    """host points [n][2] -> (X, Y) in 1/64 pixel, or None when one is not finite or lies outside the picture"""
    xy = np.asarray(xy, f64).reshape(-1, 2)
    ok = np.isfinite(xy).all() and (xy[:, 0] >= 0).all() and (xy[:, 0] <= w - 1).all() and (xy[:, 1] >= 0).all() and (xy[:, 1] <= h - 1).all()
    if not ok:
        return None
    q = np.rint(xy * 64.0).astype(i64)
    return q[:, 0], q[:, 1]


def zones(wet, inside):
    """the zones helper: 1 where the wet byte is zero, else 2 where the inside byte is zero, else 0; either input may be None"""
    shape = (wet if wet is not None else inside).shape
    z = np.zeros(shape, np.uint8)
    if inside is not None:
        z[np.asarray(inside) == 0] = 2
    if wet is not None:
        z[np.asarray(wet) == 0] = 1
    return z


def _isum(out, idx, val):
    np.add.at(out, idx, np.asarray(val, i64))


class DriftersRef:
    def __init__(self, w, h, p, lut):
        assert open_error(w, h, p) is None
        self.w, self.h, self.p, self.lut = w, h, Params(**asdict(p)), np.asarray(lut, np.uint8).reshape(256, 3)
        self.HX, self.HY, self.X, self.Y, self.age, self.st = (np.zeros(0, i64) for _ in range(6))
        self._zero()

    @property
    def n(self):
        return self.st.size

    def _zero(self):
        nc = self.p.grid_x * self.p.grid_y
        self.density = np.zeros((self.h, self.w), i64)
        self.place, self.origin = np.zeros((nc, SUMS), i64), np.zeros((nc, SUMS), i64)
        self.hist = np.zeros((4, HIST_BINS), i64)
        self.deaths = np.zeros(16, i64)
        self.released = self.age_shore = self.age_offshore = self.pushes = 0
        self.cells, self.summary = np.zeros(nc, CELL), np.zeros(SUMMARY_WORDS, i64)

    def seed(self, xy):
        """appends the points as WAITING -> True; False (nothing added) for a refused point or too many"""
        q = seed_points(xy, self.w, self.h)
        if q is None or self.n + q[0].size > self.p.max_drifters:
            return False
        k = q[0].size
        self.HX, self.HY = np.concatenate([self.HX, q[0]]), np.concatenate([self.HY, q[1]])
        self.X, self.Y = np.concatenate([self.X, q[0]]), np.concatenate([self.Y, q[1]])
        self.age, self.st = np.concatenate([self.age, np.zeros(k, i64)]), np.concatenate([self.st, np.full(k, WAITING, i64)])
        return True

    def set(self, **kw):
        q = Params(**{**asdict(self.p), **kw})
        if settable_error(q):
            raise ValueError(settable_error(q))
        self.p = q

    def reset(self):
        self.X, self.Y = self.HX.copy(), self.HY.copy()
        self.age[:] = 0
        self.st[:] = WAITING
        self._zero()

    def pixel(self, X, Y):
        return (X + 32) >> 6, (Y + 32) >> 6

    def push(self, flow, zone=None):
        """-> dict of every output of the push; `step` and `fate` (this push's, 0 where none) besides, for the tests"""
        p, w, h, n = self.p, self.w, self.h, self.n
        assert n > 0
        gx, gy = p.grid_x, p.grid_y
        bad, qu, qv = quantize(flow)
        dq = dt_q(p.dt)
        X, Y, age, st = self.X, self.Y, self.age, self.st
        rel = (st == WAITING) | ((st > 0) & bool(p.flags & RESPAWN))
        mov = st == ALIVE
        act = rel | mov
        fate = np.zeros(n, i64)
        # 1. release
        X[rel], Y[rel], age[rel] = self.HX[rel], self.HY[rel], 0
        # 2. move
        ix, fx, iy, fy = X >> 6, X & 63, Y >> 6, Y & 63
        x1, y1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
        Du, Dv, anybad = np.zeros(n, i64), np.zeros(n, i64), np.zeros(n, bool)
        for wt, cx, cy in (((64 - fx) * (64 - fy), ix, iy), (fx * (64 - fy), x1, iy), ((64 - fx) * fy, ix, y1), (fx * fy, x1, y1)):
            anybad |= (wt > 0) & bad[cy, cx]
            Du += wt * qu[cy, cx]
            Dv += wt * qv[cy, cx]
        anybad &= mov
        fate[anybad] = BAD
        go = mov & ~anybad
        su = np.where(go, (Du * dq + (1 << 19)) >> 20, 0)
        sv = np.where(go, (Dv * dq + (1 << 19)) >> 20, 0)
        Tx, Ty = X + su, Y + sv
        # 3. edge, the first that holds
        for cond, f in ((Tx < 0, EDGE_LEFT), (Tx > 64 * (w - 1), EDGE_RIGHT), (Ty < 0, EDGE_TOP), (Ty > 64 * (h - 1), EDGE_BOTTOM)):
            fate[go & (fate == 0) & cond] = f
        # 4. zone
        free = act & (fate == 0)
        tpx, tpy = self.pixel(np.where(free, Tx, 0), np.where(free, Ty, 0))
        if zone is not None:
            z = np.minimum(np.asarray(zone)[tpy, tpx].astype(i64), 7)
            inz = free & (z > 0)
            fate[inz] = ZONE0 + z[inz]
        else:
            inz = np.zeros(n, bool)
        # 5. age
        age[mov] += 1
        old = mov & (fate == 0) & (p.max_age > 0) & (age >= p.max_age)
        fate[old] = AGED
        # 6. alive or dead
        alive = act & (fate == 0)
        takeT = alive | inz | old
        X[takeT], Y[takeT] = Tx[takeT], Ty[takeT]
        dead = act & (fate > 0)
        st[alive] = ALIVE
        st[dead] = fate[dead]
        px, py = self.pixel(X, Y)
        pc = cell_of(px, py, w, h, gx, gy)
        hx, hy = self.pixel(self.HX, self.HY)
        oc = cell_of(hx, hy, w, h, gx, gy)
        occ = np.zeros((h, w), i64)
        np.add.at(occ, (py[alive], px[alive]), 1)
        _isum(self.place[:, 0], pc[alive], 1)
        _isum(self.place[:, 1], pc[alive], su[alive])
        _isum(self.place[:, 2], pc[alive], sv[alive])
        _isum(self.origin[:, 0], oc[rel], 1)
        cls = fate_class(fate)
        for k in range(4):
            m = dead & (cls == k)
            _isum(self.place[:, 3 + k], pc[m], 1)
            _isum(self.origin[:, 1 + k], oc[m], 1)
            _isum(self.hist[k], np.minimum(HIST_BINS - 1, age[m] // p.age_bin), 1)
        m = dead & (cls == 1)
        _isum(self.place[:, 7], pc[m], age[m])
        _isum(self.origin[:, 6], oc[m], age[m])
        self.age_offshore += int(age[m].sum())
        m = dead & (cls == 0)
        _isum(self.origin[:, 5], oc[m], age[m])
        self.age_shore += int(age[m].sum())
        _isum(self.deaths, fate[dead], 1)
        self.released += int(rel.sum())
        self.pushes += 1
        self.density = (self.density + occ) & 0xFFFFFFFF
        self.summary = np.array([n, int(alive.sum()), self.released, self.pushes, self.age_shore, self.age_offshore, 0, 0] + list(self.deaths), i64)
        self.cells = self.records()
        d = self.density
        out = dict(now=np.minimum(occ, 65535).astype(np.uint16), density=d.astype(np.uint32),
                   live=np.where(occ >= p.live_min, 255, 0).astype(np.uint8),
                   picture=np.where((d > 0)[..., None], self.lut[np.minimum(255, d * 255 // p.density_full)], 0).astype(np.uint8),
                   xy=(np.stack([X, Y], 1).astype(f32) / f32(64.0)), age=age.astype(np.int32),
                   state=np.where(st == WAITING, 255, st).astype(np.uint8),
                   cells=self.cells, place=self.place.copy(), origin=self.origin.copy(), hist=self.hist.astype(np.uint64), summary=self.summary,
                   occupancy=occ, step=np.stack([su, sv], 1), fate=fate)
        return out

    def records(self):
        nc = self.p.grid_x * self.p.grid_y
        cells = np.zeros(nc, CELL)
        for c in range(nc):
            pl, og = (int(v) for v in self.place[c]), (int(v) for v in self.origin[c])
            pl, og = list(pl), list(og)
            if pl[0] == 0 and og[0] == 0:
                cells[c]["flags"] = EMPTY
            if pl[0] > 0:
                cells[c]["mean_u"] = f32((f64(pl[1]) / f64(64.0)) / f64(pl[0]))
                cells[c]["mean_v"] = f32((f64(pl[2]) / f64(64.0)) / f64(pl[0]))
            deaths = og[1] + og[2] + og[3] + og[4]
            if deaths > 0:
                cells[c]["escape"] = f32(f64(og[2]) / f64(deaths))
                cells[c]["beached"] = f32(f64(og[1]) / f64(deaths))
            if og[2] > 0:
                cells[c]["mean_exit_age"] = f32(f64(og[6]) / f64(og[2]))
        return cells


# ---------------------------------------------------------------------------------------------------------------- scenes
def field(U, V):
    return np.ascontiguousarray(np.stack([U, V], -1), f32)


def uniform_field(w, h, u, v):
    return field(np.full((h, w), u), np.full((h, w), v))


def lattice(xs, ys):
    """homes on a lattice, x fastest: neighbouring drifters are neighbours"""
    gx, gy = np.meshgrid(np.asarray(xs, f64), np.asarray(ys, f64))
    return np.stack([gx.ravel(), gy.ravel()], 1)


def prototype_zone(w=160, h=120):
    z = np.zeros((h, w), np.uint8)
    z[:8] = OFFSHORE - ZONE0
    z[h - 8:] = SHORE - ZONE0
    return z


def prototype_lattice():
    return lattice(np.linspace(4, 155, 76), np.linspace(20, 99, 20))


def converging_field(w, h, cx, cy):
    """every vector points at pixel (cx, cy) and reaches it in one step where it is nearer than 8 pixels"""
    y, x = np.mgrid[0:h, 0:w].astype(f64)
    dx, dy = cx - x, cy - y
    r = np.maximum(np.hypot(dx, dy), 1e-9)
    s = np.minimum(r, 8.0) / r
    return field(dx * s, dy * s)


def hostile_field(w, h, seed=3):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-3., 3., (h, w, 2)).astype(f32)
    specials = np.array([np.nan, np.inf, -np.inf, 500.0, -500.0, 499.99997, -0.0, 0.0], f32)
    hit = rng.random((h, w)) < 0.08
    sp = specials[rng.integers(0, specials.size, (h, w))]
    comp = rng.integers(0, 2, (h, w))
    f[..., 0] = np.where(hit & (comp == 0), sp, f[..., 0])
    f[..., 1] = np.where(hit & (comp == 1), sp, f[..., 1])
    return f
