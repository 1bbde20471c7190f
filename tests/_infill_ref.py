"""The flow infill (include/rcflow.h, "flow infill") stated in numpy: the sample rule and the classes, the held state, the pull
over a pyramid of block sums, the push from the coarsest level down, every output, the cell sums, the records and the summary.
Integers are int64 and exact (the kernels work in int32: the bounds are asserted here); the only floats are F / 64 in float32,
which is exact, and the records' means in float64 operation by operation.  Also the fields and hole patterns the tests look at."""
from dataclasses import asdict, dataclass

import numpy as np

from _meanflow_ref import cell_index, quantize      # the mean current's sample rule and the opposing-flow map's cells, word for word

LEAVE_NAN, LEAVE_ZERO = 1, 2
HELD, OUTSIDE, UNFILLED = 64, 254, 255
NONE = 1
MAX_LEVELS, MAX_MIN_KNOWN, MAX_HOLD, MAX_CELLS, SUMS, SUMMARY_WORDS = 7, 16384, 254, 16384, 8, 16
NAN_BITS = 0x7fc00000
f32, f64, i64 = np.float32, np.float64, np.int64

CELL = np.dtype([("flags", "<i4"), ("pixels", "<i4"), ("known_pm", "<i4"), ("valued_pm", "<i4"), ("mean_x", "<f4"), ("mean_y", "<f4"),
                 ("mean_level", "<f4"), ("pad", "<i4")])
SUMMARY = ("known", "held", "filled", "unfilled", "outside", "pushes", "zero0", "zero1") + tuple("lev%d" % k for k in range(8))
PICTURES = ("filled", "source", "mask", "picture")
KNOWN_BGR, HELD_BGR, UNFILLED_BGR, OUTSIDE_BGR = (64, 64, 64), (255, 255, 255), (255, 0, 255), (0, 0, 0)


@dataclass
class Params:
    levels: int = 7
    min_known: int = 1
    hold: int = 0
    grid_x: int = 1
    grid_y: int = 1
    leave: str = "nan"

    def kw(self):
        """the keywords of Context.infill_open"""
        return asdict(self)


def settable_error(p):
    ok = 1 <= p.levels <= MAX_LEVELS and 1 <= p.min_known <= MAX_MIN_KNOWN and p.leave in ("nan", "zero")
    return None if ok else "levels, min_known or leave"


def open_error(w, h, p):
    """what rcflow_infill_open refuses before it looks at the context: None, or the reason"""
    if not (w > 0 and h > 0 and 0 <= p.hold <= MAX_HOLD) or settable_error(p):
        return "parameters"
    if not (1 <= p.grid_x <= w and 1 <= p.grid_y <= h and p.grid_x * p.grid_y <= MAX_CELLS):
        return "grid"
    return None


def sizes(w, h, L):
    """[(w_l, h_l)] for l = 0..L: halved and rounded up, 1 x 1 stays"""
    s = [(w, h)]
    for _ in range(L):
        s.append(((s[-1][0] + 1) >> 1, (s[-1][1] + 1) >> 1))
    return s


def rdiv(a, b):
    """floor((2 a + b) / (2 b)), the floor towards minus infinity; b > 0 (numpy's // floors)"""
    return (2 * a + b) // (2 * b)


def pull_once(S):
    """the sums of S [h][w][3] over 2 x 2 blocks; rows and columns past the edge count as nothing"""
    h, w = S.shape[:2]
    P = np.zeros((h + (h & 1), w + (w & 1), 3), i64)
    P[:h, :w] = S
    return P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2]


def parents(n, n_up):
    """for the cells 0..n-1 of an axis: (X0, X1) on the axis of n_up cells above"""
    x = np.arange(n)
    x0 = x >> 1
    return x0, np.clip(x0 + np.where(x & 1, 1, -1), 0, n_up - 1)


def pull_push(qx, qy, have, L, min_known):
    """qx, qy [h][w] int64, have [h][w] bool (KNOWN or HELD) -> (Fx, Fy, lev, val) of level 0: val where the pixel has a value,
    lev the coarsest level that contributed (0 where have)"""
    h, w = have.shape
    sz = sizes(w, h, L)
    S = [np.stack([np.where(have, qx, 0), np.where(have, qy, 0), have.astype(i64)], -1).astype(i64)]
    for l in range(L):
        S.append(pull_once(S[-1]))
        assert S[-1].shape[:2] == (sz[l + 1][1], sz[l + 1][0]) and np.abs(S[-1][..., :2]).max(initial=0) < 2 ** 30
    # level L
    N = S[L][..., 2]
    val = N >= min_known
    n1 = np.maximum(N, 1)
    Fx, Fy = np.where(val, rdiv(S[L][..., 0], n1), 0), np.where(val, rdiv(S[L][..., 1], n1), 0)
    lev = np.where(val, L, 0)
    for l in range(L - 1, -1, -1):
        wl, hl = sz[l]
        N = S[l][..., 2]
        own = (N >= min_known) if l >= 1 else have
        n1 = np.maximum(N, 1)
        ox, oy = rdiv(S[l][..., 0], n1), rdiv(S[l][..., 1], n1)         # at level 0, N = 1: its q
        X0, X1 = parents(wl, sz[l + 1][0])
        Y0, Y1 = parents(hl, sz[l + 1][1])
        A, nx, ny, lv = (np.zeros((hl, wl), i64) for _ in range(4))
        for ys, xs, wt in ((Y0, X0, 9), (Y0, X1, 3), (Y1, X0, 3), (Y1, X1, 1)):
            v = val[ys][:, xs]
            A += wt * v
            nx += wt * np.where(v, Fx[ys][:, xs], 0)
            ny += wt * np.where(v, Fy[ys][:, xs], 0)
            lv = np.maximum(lv, np.where(v, lev[ys][:, xs], 0))
        a1 = np.maximum(A, 1)
        got = A > 0
        assert max(np.abs(nx).max(initial=0), np.abs(ny).max(initial=0)) <= 16 * 32000
        Fx = np.where(own, ox, np.where(got, rdiv(nx, a1), 0))
        Fy = np.where(own, oy, np.where(got, rdiv(ny, a1), 0))
        lev = np.where(own, l, np.where(got, lv, 0))
        val = own | got
    return Fx, Fy, lev, val


class InfillRef:
    """the session: the held state, the push count, set and reset"""

    def __init__(self, w, h, p, lut):
        assert open_error(w, h, p) is None
        self.w, self.h, self.p, self.lut = w, h, Params(**asdict(p)), np.asarray(lut, np.uint8).reshape(256, 3)
        self.cell = cell_index(w, h, p.grid_x, p.grid_y)
        self.reset()

    def reset(self):
        h, w, nc = self.h, self.w, self.p.grid_x * self.p.grid_y
        self.hq = np.zeros((h, w, 2), i64)
        self.age = np.full((h, w), 255, i64)
        self.pushes = 0
        self.cells, self.sums, self.summary = np.zeros(nc, CELL), np.zeros((nc, SUMS), i64), np.zeros(SUMMARY_WORDS, i64)

    def set(self, levels, min_known, leave):
        q = Params(**{**asdict(self.p), "levels": levels, "min_known": min_known, "leave": leave})
        if settable_error(q):
            raise ValueError(settable_error(q))
        self.p = q

    def push(self, flow, valid=None, domain=None):
        """-> every output of the push, and `sides`: what the tests look at"""
        p, w, h = self.p, self.w, self.h
        flow = np.asarray(flow, f32)
        assert flow.shape == (h, w, 2)
        bad, qx, qy = quantize(flow)
        known = ~bad if valid is None else ~bad & (np.asarray(valid) != 0)
        if p.hold > 0:
            held = ~known & (self.age < p.hold)
            self.hq[known, 0], self.hq[known, 1] = qx[known], qy[known]
            self.age = np.where(known, 0, np.where(held, self.age + 1, 255))
            vx, vy = np.where(known, qx, self.hq[..., 0]), np.where(known, qy, self.hq[..., 1])
        else:
            held = np.zeros((h, w), bool)
            vx, vy = qx, qy
        have = known | held
        Fx, Fy, lev, val = pull_push(vx, vy, have, p.levels, p.min_known)
        wanted = np.ones((h, w), bool) if domain is None else np.asarray(domain) != 0
        source = np.where(known, 0, np.where(~wanted, OUTSIDE, np.where(held, HELD, np.where(val, lev, UNFILLED)))).astype(i64)
        assert not (val & ~have & (lev < 1)).any()
        valued = source <= HELD
        is_filled = (source >= 1) & (source <= MAX_LEVELS)
        pattern = NAN_BITS if p.leave == "nan" else 0
        out = np.full((h, w, 2), pattern, np.uint32)
        F = np.stack([Fx, Fy], -1)
        assert np.abs(F[valued]).max(initial=0) <= 32000
        comp = (F.astype(f32) / f32(64.0)).view(np.uint32)
        out = np.where((valued & ~known)[..., None], comp, out)
        out = np.where(known[..., None], flow.view(np.uint32), out)
        picture = np.zeros((h, w, 3), np.uint8)
        picture[source == 0] = KNOWN_BGR
        picture[source == HELD] = HELD_BGR
        picture[source == UNFILLED] = UNFILLED_BGR
        picture[source == OUTSIDE] = OUTSIDE_BGR
        picture[is_filled] = self.lut[source[is_filled] * 255 // 7]
        # cells, records, summary
        nc = p.grid_x * p.grid_y
        cell, src = self.cell, source.ravel()
        sums = np.zeros((nc, SUMS), i64)
        for k, m in enumerate((src == 0, src == HELD, is_filled.ravel(), src == UNFILLED, src == OUTSIDE)):
            sums[:, k] = np.bincount(cell[m], minlength=nc)
        v = valued.ravel()
        np.add.at(sums[:, 5], cell[v], Fx.ravel()[v])
        np.add.at(sums[:, 6], cell[v], Fy.ravel()[v])
        np.add.at(sums[:, 7], cell[is_filled.ravel()], src[is_filled.ravel()])
        cells = np.zeros(nc, CELL)
        cells["pixels"] = np.bincount(cell, minlength=nc)
        nv = sums[:, 0] + sums[:, 1] + sums[:, 2]
        cells["known_pm"] = sums[:, 0] * 1000 // cells["pixels"]
        cells["valued_pm"] = nv * 1000 // cells["pixels"]
        for k in range(nc):
            if nv[k] == 0:
                cells[k]["flags"] = NONE
            else:
                cells[k]["mean_x"] = f32((f64(sums[k, 5]) / f64(64.0)) / f64(nv[k]))
                cells[k]["mean_y"] = f32((f64(sums[k, 6]) / f64(64.0)) / f64(nv[k]))
            if sums[k, 2]:
                cells[k]["mean_level"] = f32(f64(sums[k, 7]) / f64(sums[k, 2]))
        self.pushes += 1
        by_lev = np.bincount(src[is_filled.ravel()], minlength=8)[:8]
        summary = np.concatenate([sums[:, :5].sum(0), [self.pushes, 0, 0], by_lev]).astype(i64)
        self.cells, self.sums, self.summary = cells, sums, summary
        return dict(filled=out.view(f32), source=source.astype(np.uint8), mask=np.where(valued, 255, 0).astype(np.uint8), picture=picture,
                    cells=cells, sums=sums, summary=summary,
                    sides=dict(known=known, held=held, Fx=Fx, Fy=Fy, lev=lev, val=val, qx=qx, qy=qy, bad=bad))


def fill(flow, valid, p, lut, domain=None):
    """one push through a fresh session"""
    h, w = np.asarray(flow).shape[:2]
    return InfillRef(w, h, p, lut).push(flow, valid, domain)


# ---------------------------------------------------------------------------------------------------------------- fields
def plain_lut():
    """a stand-in for COLORMAP_JET where no library is at hand: the tests of the statement do not look at the colours' values"""
    i = np.arange(256, dtype=np.uint8)
    return np.stack([255 - i, i, i // 2], -1)


def shear_field(w=160, h=120):
    """a shear with a Gaussian jet in the middle: what the prototype's figures were taken on"""
    y, x = np.mgrid[0:h, 0:w].astype(f64)
    g = np.exp(-(x - 80.0) ** 2 / (2.0 * 16.0 ** 2))
    f = np.empty((h, w, 2), f32)
    f[..., 0] = (0.03 * (y - 60.0) + 1.5 * g).astype(f32)
    f[..., 1] = (-0.03 * (x - 80.0) - 2.0 * g).astype(f32)
    return f


def pattern(name, w, h, shift=0):
    """the valid bytes of a hole pattern: pN, block40 (scaled to the picture from 160 x 120), all, none, corners; shift moves the
    pattern to the right by so many pixels, cyclically"""
    y, x = np.mgrid[0:h, 0:w].astype(i64)
    x = (x - shift) % w
    if name.startswith("p"):
        known = (7919 * x + 104729 * y + 31 * x * y + 17 * (x * x + y)) % 1000 >= int(name[1:])
    elif name == "block40":
        known = ~((y >= h // 3) & (y < 2 * h // 3) & (x >= 3 * w // 8) & (x < 5 * w // 8))
    elif name == "all":
        known = np.ones((h, w), bool)
    elif name == "none":
        known = np.zeros((h, w), bool)
    else:
        assert name == "corners"
        known = np.zeros((h, w), bool)
        known[0, 0] = known[0, w - 1] = known[h - 1, 0] = known[h - 1, w - 1] = True
    return np.where(known, 255, 0).astype(np.uint8)


def hostile(field, seed=3, share=0.2):
    """NaN, +-inf, +-500.0, +-499.99, -0.0 and denormals sprinkled into a field, next to good pixels"""
    f = np.array(field, f32)
    rng = np.random.RandomState(seed)
    h, w = f.shape[:2]
    sp = np.array([np.nan, np.inf, -np.inf, 500.0, -500.0, 499.99, -499.99, -0.0, 1e-42, -1e-42], f32)
    hit = rng.uniform(size=(h, w)) < share
    k = rng.randint(0, len(sp), (h, w))
    comp = rng.randint(0, 3, (h, w))                          # 0: u, 1: v, 2: both
    f[..., 0] = np.where(hit & (comp != 1), sp[k], f[..., 0])
    f[..., 1] = np.where(hit & (comp != 0), sp[k], f[..., 1])
    return f


def saturated(w, h):
    """every vector (+-499.99, +-499.99), the signs in blocks of 128 x 128: whole blocks of the coarsest level add up with one sign"""
    y, x = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 2), f32)
    f[..., 0] = np.where((x // 128) & 1, -499.99, 499.99)
    f[..., 1] = np.where((y // 128) & 1, 499.99, -499.99)
    return f


def errors(out, hole):
    """e^2 = (Fx - qx)^2 + (Fy - qy)^2 over the holes that got a value -> the int64 array"""
    s = out["sides"]
    m = hole & s["val"]
    return ((s["Fx"] - s["qx"]) ** 2 + (s["Fy"] - s["qy"]) ** 2)[m]
