"""The flow map and FTLE of include/rcflow.h ("flow map and FTLE") in numpy: the statement ftle_kernels.hip is held to.

All fp32, every operation rounded on its own, in the header's order; the logarithm and the mask's bound in double.  Arrays
are [row][column]; a field is h x w x 2 float32 (x, y)."""
import math

import numpy as np

f32 = np.float32
FORWARD, BACKWARD = 0, 1
INT_MIN = -2 ** 31
QNAN = np.uint32(0x7FC00000)


def cvt_i32_x86(v):
    """(int)float as x86 converts: NaN and values outside the int range give INT_MIN"""
    ok = (v >= f32(-2147483648.0)) & (v < f32(2147483648.0))
    return np.where(ok, np.where(ok, v, 0).astype(np.int64), INT_MIN)


def sample(field, x, y):
    """the streamline sampler at float32 positions -> (accepted, dx, dy); dx, dy are 0 where rejected"""
    h, w = field.shape[:2]
    if w < 3 or h < 3:                                        # no index passes 1 <= ind and ind + 2 <= size
        z = np.zeros(np.shape(x), f32)
        return np.zeros(np.shape(x), bool), z, z.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        xind, yind = cvt_i32_x86(np.floor(x)), cvt_i32_x86(np.floor(y))
        ok = ~((xind < 1) | (yind < 1) | (xind + 2 > w) | (yind + 2 > h))
        xi, yi = np.where(ok, xind, 1), np.where(ok, yind, 1)
        xrem, yrem = (x - xi.astype(f32)).astype(f32), (y - yi.astype(f32)).astype(f32)
        p00, p01, p10, p11 = field[yi, xi], field[yi, xi + 1], field[yi + 1, xi], field[yi + 1, xi + 1]
        wa, wb = f32(1) - xrem, f32(1) - yrem
        out = []
        for c in (0, 1):
            v = p00[..., c] * wa * wb + p01[..., c] * xrem * wb + p10[..., c] * wa * yrem + p11[..., c] * xrem * yrem
            out.append(np.where(ok, v, f32(0)).astype(f32))
    return ok, out[0], out[1]


def flow_map(fields, direction, dt):
    """fields: the held ones, oldest first -> (D h x w x 2 float32, steps h x w int32)"""
    h, w = fields[0].shape[:2]
    xo, yo = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    D = np.zeros((h, w, 2), f32)
    steps = np.zeros((h, w), np.int32)
    alive = np.ones((h, w), bool)
    order = fields if direction == FORWARD else fields[::-1]
    sdt = f32(dt) if direction == FORWARD else -f32(dt)
    for f in order:
        f = np.asarray(f, f32)
        x, y = D[..., 0] + xo, D[..., 1] + yo
        ok, dx, dy = sample(f, x, y)
        go = alive & ok & np.isfinite(dx) & np.isfinite(dy)
        with np.errstate(invalid="ignore", over="ignore"):
            nx, ny = D[..., 0] + dx * sdt, D[..., 1] + dy * sdt
        D[..., 0] = np.where(go, nx, D[..., 0])
        D[..., 1] = np.where(go, ny, D[..., 1])
        steps += go
        alive = go
    return D, steps


def jet_index(ftle, vis_max):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.rint(ftle / f32(vis_max) * f32(255))
    return np.clip(np.nan_to_num(r, nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.int64)


def deformation(D, steps, n, spacing, threshold, vis_max, lut, pushes):
    """-> dict(lam, ftle float32, valid bool, mask uint8, index int64, vis uint8 h x w x 3, summary 8 int64)"""
    h, w = steps.shape
    s = spacing
    full = steps == n
    valid = np.zeros((h, w), bool)
    lam = np.zeros((h, w), f32)
    ftle = np.zeros((h, w), f32)
    if w > 2 * s and h > 2 * s:
        c = (slice(s, h - s), slice(s, w - s))
        E, W = (slice(s, h - s), slice(2 * s, w)), (slice(s, h - s), slice(0, w - 2 * s))
        S, N = (slice(2 * s, h), slice(s, w - s)), (slice(0, h - 2 * s), slice(s, w - s))
        valid[c] = full[c] & full[E] & full[W] & full[S] & full[N]
        inv = f32(1.0) / f32(2 * s)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            a = f32(1) + (D[E][..., 0] - D[W][..., 0]) * inv
            b = (D[S][..., 0] - D[N][..., 0]) * inv
            cc = (D[E][..., 1] - D[W][..., 1]) * inv
            d = f32(1) + (D[S][..., 1] - D[N][..., 1]) * inv
            c11, c12, c22 = a * a + cc * cc, a * b + cc * d, b * b + d * d
            m, q = (c11 + c22) * f32(0.5), (c11 - c22) * f32(0.5)
            l = (m + np.sqrt(q * q + c12 * c12)).astype(f32)
            ft = (np.log(l.astype(np.float64)) / float(2 * n)).astype(f32)
        nan = np.isnan(l)
        l = np.where(nan, QNAN.view(f32), l)
        ft = np.where(nan, QNAN.view(f32), ft)
        lam[c] = np.where(valid[c], l, f32(0))
        ftle[c] = np.where(valid[c], ft, f32(0))
    lam_thr = f32(math.exp(2.0 * n * threshold))
    with np.errstate(invalid="ignore"):
        mask = valid & (lam >= lam_thr)
    index = jet_index(ftle, vis_max)
    vis = np.where(valid[..., None], np.asarray(lut, np.uint8)[index], np.uint8(0)).astype(np.uint8)
    ok = valid & ~np.isnan(lam)
    maxbits = int(lam[ok].view(np.uint32).max()) if ok.any() else 0
    summary = np.array([n, valid.sum(), mask.sum(), (steps < n).sum(), maxbits, pushes, 0, 0], np.int64)
    return dict(lam=lam, ftle=ftle, valid=valid, mask=(mask * 255).astype(np.uint8), index=index, vis=vis, summary=summary)


class FtleRef:
    """a session: the ring of the last `window` fields, pushes counted from open / reset"""

    def __init__(self, w, h, lut, window, direction=BACKWARD, dt=1.0, spacing=1, threshold=0.1, vis_max=0.5):
        self.w, self.h, self.lut = w, h, lut
        self.window, self.direction, self.dt, self.spacing = window, direction, dt, spacing
        self.threshold, self.vis_max = threshold, vis_max
        self.fields, self.pushes = [], 0

    def reset(self):
        self.fields, self.pushes = [], 0

    def push(self, field, compute=True):
        field = np.asarray(field, f32)
        assert field.shape == (self.h, self.w, 2)
        self.fields = (self.fields + [field])[-self.window:]
        self.pushes += 1
        if not compute:
            return None
        n = len(self.fields)
        D, steps = flow_map(self.fields, self.direction, self.dt)
        out = deformation(D, steps, n, self.spacing, self.threshold, self.vis_max, self.lut, self.pushes)
        out.update(map=D, steps=steps, n=n)
        return out


# ---------------------------------------------------------------------------- inputs
def mixed_fields(w=131, h=70, count=6, seed=7):
    """the time-varying input of both tiers: shear waves, a weak saddle, a drift that takes particles out of the frame, noise"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    out = []
    for k in range(count):
        u = 0.9 * np.sin(2 * np.pi * y / 23 + 0.3 * k) + 0.004 * (x - cx) + 1.1
        v = 0.9 * np.cos(2 * np.pi * x / 31 - 0.3 * k) - 0.004 * (y - cy) - 0.6
        f = np.stack([u, v], -1) + 0.05 * rng.standard_normal((h, w, 2))
        out.append(f.astype(f32))
    return out


def uniform_field(w, h, u, v):
    f = np.empty((h, w, 2), f32)
    f[..., 0], f[..., 1] = u, v
    return f


def saddle_field(w, h, a):
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return np.stack([a * (x - cx), -a * (y - cy)], -1).astype(f32)


def rotation_field(w, h, om):
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return np.stack([-om * (y - cy), om * (x - cx)], -1).astype(f32)
