"""The flow check (include/rcflow.h, "flow check") stated in numpy: the fixed-point sample, the target, the bilinear gather in
integer weights, the residuals, the clipped box sums, the structure tensor, the seven tests, every output, the cell sums, the
records and the summary.  Integers are int64 and exact; the float results are float64 operation by operation, in the order the
header gives, then rounded to float32.  Also the fields the tests look at."""
import math
from dataclasses import asdict, dataclass

import numpy as np

from _meanflow_ref import cell_index, quantize      # the mean current's sample rule and the opposing-flow map's cells, word for word

BAD, OUT, FLAT, RESID, NOGAIN, FB, FAST = 1, 2, 4, 8, 16, 32, 64
NAMES = ("bad", "out", "flat", "resid", "nogain", "fb", "fast")
TESTS = FLAT | RESID | NOGAIN | FB | FAST
NONE_VALID = 1
MAX_RADIUS, MAX_CELLS, SUMS, SUMMARY_WORDS = 7, 16384, 10, 10
NAN_BITS = 0x7fc00000
f32, f64, i64 = np.float32, np.float64, np.int64

CELL = np.dtype([("flags", "<i4"), ("pixels", "<i4"), ("valid", "<i4"), ("valid_pm", "<i4"), ("mean_x", "<f4"), ("mean_y", "<f4"), ("pad", "<i4", (2,))])
SUMMARY = ("valid", "bad", "out", "flat", "resid", "nogain", "fb", "fast", "computing", "pushes")
PICTURES = ("flags", "mask", "checked", "resid", "texture", "picture")
# the colour of the lowest set bit, B G R, in the order of the bits
COLOURS = np.array([(255, 0, 255), (128, 128, 128), (255, 0, 0), (0, 0, 255), (0, 165, 255), (0, 255, 255), (0, 255, 0)], np.uint8)


class StateError(Exception):
    """RC_ESTATE: d_prev is None and no frame is held"""


@dataclass
class Params:
    radius: int = 4
    grid_x: int = 1
    grid_y: int = 1
    tests: int = TESTS
    fill: str = "nan"
    tex_min: int = 1
    gain_pm: int = 0
    res_max: float = 1.5
    fb_rel: float = 0.01
    fb_abs: float = math.sqrt(0.5)
    speed_max: float = 1000.0

    def kw(self):
        """the keywords of Context.flowcheck_open"""
        return asdict(self)


def settable_error(p):
    ok = (not (p.tests & ~TESTS) and 0 <= p.tex_min <= 65025 and 0 <= p.gain_pm <= 1000 and 0. <= p.res_max <= 255. and 0. <= p.fb_rel <= 1. and
          0. <= p.fb_abs <= 500. and 0. <= p.speed_max <= 1000.)       # NaN fails every comparison
    return None if ok else "tests, tex_min, gain_pm, res_max, fb_rel, fb_abs or speed_max"


def open_error(w, h, p):
    """what rcflow_flowcheck_open refuses before it looks at the context: None, or the reason"""
    if not (w > 0 and h > 0 and 0 <= p.radius <= MAX_RADIUS and p.fill in ("nan", "zero")) or settable_error(p):
        return "parameters"
    if not (1 <= p.grid_x <= w and 1 <= p.grid_y <= h and p.grid_x * p.grid_y <= MAX_CELLS):
        return "grid"
    return None


def host_constants(p):
    """what the host takes from the doubles -> (res_q, fb_rel_q, fb_abs_q, smax_q)"""
    return (math.floor(p.res_max * 4096.0), int(np.rint(f64(p.fb_rel) * 1024.0)), math.floor(p.fb_abs * p.fb_abs * 4194304.0),
            math.floor(p.speed_max * 64.0))


def box_sum(p, r):
    """the sums of the int64 plane p over the (2 r + 1)^2 box clipped to the plane, from its integral image"""
    p = np.asarray(p, i64)
    h, w = p.shape
    c = np.zeros((h + 1, w + 1), i64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def target(q, n):
    """a coordinate in 1/64 pixel on an axis of n pixels -> (i0, frac, i1)"""
    i0 = q >> 6
    return i0, q & 63, np.minimum(i0 + 1, n - 1)


def gradients(prev):
    """central differences with a replicated border -> (gx, gy) int64"""
    P = np.asarray(prev).astype(i64)
    h, w = P.shape
    x, y = np.arange(w), np.arange(h)
    return P[:, np.minimum(x + 1, w - 1)] - P[:, np.maximum(x - 1, 0)], P[np.minimum(y + 1, h - 1)] - P[np.maximum(y - 1, 0)]


def tensor(prev, r):
    """-> (a, c, b, N): the window sums of gx^2, gy^2, gx gy and the window's pixels"""
    gx, gy = gradients(prev)
    return box_sum(gx * gx, r), box_sum(gy * gy, r), box_sum(gx * gy, r), box_sum(np.ones(gx.shape, i64), r)


def flat_test(a, c, b, t):
    """True where the pixel is FLAT: the smaller eigenvalue of [[a, b], [b, c]] is below t, in integers"""
    return ~((a + c >= 2 * t) & ((a - t) * (c - t) >= b * b))


def texture(a, c, b, N):
    A, B, C = a.astype(f64), b.astype(f64), c.astype(f64)
    lam = np.maximum(((A + C) - np.sqrt((A - C) * (A - C) + 4.0 * (B * B))) * 0.5, 0.)
    return (lam / N.astype(f64)).astype(f32)


def residuals(prev, nxt, flow):
    """-> dict(bad, out, ok, qx, qy, X, Y, res, res0): res and res0 are zero where the pixel is not OK"""
    P, Q = np.asarray(prev).astype(i64), np.asarray(nxt).astype(i64)
    h, w = P.shape
    bad, qx, qy = quantize(flow)
    ys, xs = np.mgrid[0:h, 0:w]
    X, Y = 64 * xs + qx, 64 * ys + qy
    out = ~bad & ((X < 0) | (Y < 0) | (X > 64 * (w - 1)) | (Y > 64 * (h - 1)))
    ok = ~bad & ~out
    x0, fx, x1 = target(np.where(ok, X, 0), w)
    y0, fy, y1 = target(np.where(ok, Y, 0), h)
    Wn = (64 - fx) * (64 - fy) * Q[y0, x0] + fx * (64 - fy) * Q[y0, x1] + (64 - fx) * fy * Q[y1, x0] + fx * fy * Q[y1, x1]
    assert Wn.max() <= 255 * 4096
    return dict(bad=bad, out=out, ok=ok, qx=qx, qy=qy, X=X, Y=Y, res=np.where(ok, np.abs(Wn - 4096 * P), 0), res0=np.where(ok, 4096 * np.abs(Q - P), 0))


def round_trip(s, back, w, h, fb_rel_q, fb_abs_q):
    """True where FB is set, over the OK pixels of s = residuals(...)"""
    ok, qx, qy = s["ok"], s["qx"], s["qy"]
    bbad, bqx, bqy = quantize(back)
    x0, fx, x1 = target(np.where(ok, s["X"], 0), w)
    y0, fy, y1 = target(np.where(ok, s["Y"], 0), h)
    anybad = bbad[y0, x0] | bbad[y0, x1] | bbad[y1, x0] | bbad[y1, x1]
    k00, k10, k01, k11 = (64 - fx) * (64 - fy), fx * (64 - fy), (64 - fx) * fy, fx * fy
    bx = k00 * bqx[y0, x0] + k10 * bqx[y0, x1] + k01 * bqx[y1, x0] + k11 * bqx[y1, x1]
    by = k00 * bqy[y0, x0] + k10 * bqy[y0, x1] + k01 * bqy[y1, x0] + k11 * bqy[y1, x1]
    assert np.abs(bx).max() < 2 ** 31 and np.abs(by).max() < 2 ** 31
    bxr, byr = (bx + 2048) // 4096, (by + 2048) // 4096         # floor
    ex, ey = qx + bxr, qy + byr
    e2, m2 = ex * ex + ey * ey, qx * qx + qy * qy + bxr * bxr + byr * byr
    return ok & (anybad | (1024 * e2 > fb_rel_q * m2 + fb_abs_q))


def check(prev, nxt, flow, back, p, computing=1, pushes=1):
    """every output of one computing push -> dict"""
    assert open_error(prev.shape[1], prev.shape[0], p) is None
    h, w = prev.shape
    r = p.radius
    res_q, fb_rel_q, fb_abs_q, smax_q = host_constants(p)
    flow = np.asarray(flow, f32)
    s = residuals(prev, nxt, flow)
    bad, out, ok, qx, qy = s["bad"], s["out"], s["ok"], s["qx"], s["qy"]
    a, c, b, N = tensor(prev, r)
    Nr, R, R0 = box_sum(ok, r), box_sum(s["res"], r), box_sum(s["res0"], r)
    assert max(R.max(), R0.max(), a.max(), c.max(), np.abs(b).max()) < 2 ** 31
    fl = np.where(bad, BAD, 0) | np.where(out, OUT, 0)
    if p.tests & FLAT:
        fl |= np.where(~bad & flat_test(a, c, b, p.tex_min * N), FLAT, 0)
    if p.tests & FAST:
        fl |= np.where(~bad & (qx * qx + qy * qy > smax_q * smax_q), FAST, 0)
    if p.tests & RESID:
        fl |= np.where(ok & (R > res_q * Nr), RESID, 0)
    if p.tests & NOGAIN and p.gain_pm > 0:
        fl |= np.where(ok & ((qx != 0) | (qy != 0)) & (1000 * R > p.gain_pm * R0), NOGAIN, 0)
    if p.tests & FB and back is not None:
        fl |= np.where(round_trip(s, back, w, h, fb_rel_q, fb_abs_q), FB, 0)
    valid = fl == 0
    checked = flow.view(np.uint32).copy()
    checked[~valid] = NAN_BITS if p.fill == "nan" else 0
    nr = np.maximum(Nr, 1).astype(f64)
    resid = np.zeros((h, w, 2), f32)
    resid[..., 0] = np.where(ok, R.astype(f64) / (4096.0 * nr), 0.).astype(f32)
    resid[..., 1] = np.where(ok, R0.astype(f64) / (4096.0 * nr), 0.).astype(f32)
    low = np.zeros((h, w), i64)
    for k in range(7):
        low = np.where((fl & ((1 << (k + 1)) - 1)) == (1 << k), k, low)       # the index of the lowest set bit
    g = np.asarray(prev, np.uint8)
    picture = np.where(valid[..., None], g[..., None].repeat(3, 2), COLOURS[low]).astype(np.uint8)
    # cells, records, summary
    nc = p.grid_x * p.grid_y
    cell = cell_index(w, h, p.grid_x, p.grid_y)
    sums = np.zeros((nc, SUMS), i64)
    sums[:, 0] = np.bincount(cell[valid.ravel()], minlength=nc)
    for k in range(7):
        sums[:, 1 + k] = np.bincount(cell[(fl.ravel() >> k & 1) == 1], minlength=nc)
    np.add.at(sums[:, 8], cell[valid.ravel()], qx.ravel()[valid.ravel()])
    np.add.at(sums[:, 9], cell[valid.ravel()], qy.ravel()[valid.ravel()])
    cells = np.zeros(nc, CELL)
    cells["pixels"] = np.bincount(cell, minlength=nc)
    cells["valid"] = sums[:, 0]
    cells["valid_pm"] = sums[:, 0] * 1000 // cells["pixels"]
    for k in range(nc):
        nv = int(sums[k, 0])
        if nv == 0:
            cells[k]["flags"] = NONE_VALID
            continue
        cells[k]["mean_x"] = f32((f64(sums[k, 8]) / f64(64.0)) / f64(nv))
        cells[k]["mean_y"] = f32((f64(sums[k, 9]) / f64(64.0)) / f64(nv))
    summary = np.concatenate([sums[:, :8].sum(0), [computing, pushes]]).astype(i64)
    return dict(flags=fl.astype(np.uint8), mask=np.where(valid, 255, 0).astype(np.uint8), checked=checked.view(f32), resid=resid,
                texture=texture(a, c, b, N), picture=picture, cells=cells, sums=sums, summary=summary,
                sides=dict(ok=ok, N=N, Nr=Nr, R=R, R0=R0, a=a, b=b, c=c, qx=qx, qy=qy))


class FlowCheckRef:
    """the session: the held frame, the counts, set and reset"""

    def __init__(self, w, h, p):
        assert open_error(w, h, p) is None
        self.w, self.h, self.p = w, h, Params(**asdict(p))
        self.held, self.pushes, self.computing = None, 0, 0
        self._clear()

    def _clear(self):
        nc = self.p.grid_x * self.p.grid_y
        self.cells, self.sums, self.counts = np.zeros(nc, CELL), np.zeros((nc, SUMS), i64), np.zeros(8, i64)

    @property
    def summary(self):
        return np.concatenate([self.counts, [self.computing, self.pushes]]).astype(i64)

    def set(self, **kw):
        q = Params(**{**asdict(self.p), **kw})
        if settable_error(q):
            raise ValueError(settable_error(q))
        self.p = q

    def reset(self):
        """forgets the held frame and the last push's records; the counts are since open"""
        self.held = None
        self._clear()

    def push(self, nxt, prev=None, flow=None, back=None):
        """-> every output of the push, or None where the push only stored its frame"""
        if prev is None:
            prev = self.held
        if prev is None and self.pushes > 0:
            raise StateError()
        out = None
        if prev is not None:
            out = check(prev, nxt, flow, back, self.p, self.computing + 1, self.pushes + 1)
            self.computing += 1
            self.cells, self.sums, self.counts = out["cells"], out["sums"], out["summary"][:8].copy()
        self.held = np.array(nxt, np.uint8)
        self.pushes += 1
        return out


# ---------------------------------------------------------------------------------------------------------------- fields
def constant_field(w, h, u, v):
    f = np.empty((h, w, 2), f32)
    f[..., 0], f[..., 1] = u, v
    return f


PATCH = (slice(40, 80), slice(60, 110))       # rows, columns of the noisy patch on the 160 x 120 clip


def noisy_patch(field, amp=3.0, seed=7, patch=PATCH):
    """uniform noise of +-amp pixels added to the field inside the patch"""
    f = np.array(field, f32)
    rng = np.random.RandomState(seed)
    shape = f[patch].shape
    f[patch] += rng.uniform(-amp, amp, shape).astype(f32)
    return f


def hostile(field, seed=3, share=0.06):
    """NaN, +-inf, 500.0 and -0.0 sprinkled into a field, next to good pixels"""
    f = np.array(field, f32)
    rng = np.random.RandomState(seed)
    h, w = f.shape[:2]
    sp = np.array([np.nan, np.inf, -np.inf, 500.0, -0.0], f32)
    hit = rng.uniform(size=(h, w)) < share
    k = rng.randint(0, len(sp), (h, w))
    comp = rng.randint(0, 3, (h, w))                          # 0: u, 1: v, 2: both
    f[..., 0] = np.where(hit & (comp != 1), sp[k], f[..., 0])
    f[..., 1] = np.where(hit & (comp != 0), sp[k], f[..., 1])
    return f


def edge_field(w, h):
    """vectors that leave the picture over each of its four edges, that land exactly on the last column and row, and fractional parts
    of 0, 1/64 and 63/64"""
    f = np.zeros((h, w, 2), f32)
    f[:, 0, 0] = -1 / 64.                                     # out on the left by a 64th
    f[:, w - 1, 0] = 1 / 64.                                  # out on the right
    f[0, 1:w - 1, 1] = -0.5                                   # out at the top
    f[h - 1, 1:w - 1, 1] = 63 / 64.                           # out at the bottom
    f[1:h - 1, w - 2, 0] = 1.0                                # exactly the last column: x1 is clamped, its weight 0
    f[h - 2, 1:w - 2, 1] = 1.0                                # exactly the last row
    f[2:h - 2:3, 2:w - 3, 0] = 1 / 64.
    f[3:h - 2:3, 2:w - 3, 0] = 63 / 64.
    f[2:h - 2, 2:w - 3:2, 1] = -63 / 64.
    return f
