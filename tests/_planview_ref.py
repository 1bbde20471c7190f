"""The plan view of include/rcflow.h ("plan view") in numpy: the statement planview_kernels.hip is held to, bit for bit.

The table is float64, every operation rounded on its own and in the header's order (only + - * /, fabs and sqrt, so numpy
gives the device's bits); the push is float32 in the same way.  Arrays are [row][column]: a plan array is ny x nx, a field
h x w x 2 float32 (x, y), a frame h x w x 3 uint8."""
import math

import numpy as np

from _ftle_ref import sample

f32, f64 = np.float32, np.float64
SUMMARY = ("usable", "seen", "valid", "max_speed2_bits", "pushes", "reserved0", "reserved1", "reserved2")


class Params:
    """rc_planview_params.  H: 9 numbers, row-major, ground (X, Y, 1) in metres -> homogeneous ideal pixel."""

    def __init__(self, H, fx, fy, cx, cy, k1=0.0, k2=0.0, x0=0.0, y0=0.0, dx=1.0, dy=1.0, nx=1, ny=1, fps=1.0, max_gsd=math.inf):
        self.H = [float(v) for v in np.asarray(H, f64).reshape(9)]
        self.fx, self.fy, self.cx, self.cy, self.k1, self.k2 = float(fx), float(fy), float(cx), float(cy), float(k1), float(k2)
        self.x0, self.y0, self.dx, self.dy, self.nx, self.ny = float(x0), float(y0), float(dx), float(dy), int(nx), int(ny)
        self.fps, self.max_gsd = float(fps), float(max_gsd)

    def kw(self):
        return dict(self.__dict__)


def project(p, X, Y):
    """ground points (float64 arrays) -> (U, V, pz, g), the header's project() operation by operation"""
    H = [f64(v) for v in p.H]
    fx, fy, cx, cy, k1, k2 = f64(p.fx), f64(p.fy), f64(p.cx), f64(p.cy), f64(p.k1), f64(p.k2)
    with np.errstate(all="ignore"):
        px = H[0] * X + H[1] * Y + H[2]
        py = H[3] * X + H[4] * Y + H[5]
        pz = H[6] * X + H[7] * Y + H[8]
        u, v = px / pz, py / pz
        xn, yn = (u - cx) / fx, (v - cy) / fy
        r2 = xn * xn + yn * yn
        r4 = r2 * r2
        s = f64(1) + k1 * r2 + k2 * r4
        g = f64(1) + f64(3) * k1 * r2 + f64(5) * k2 * r4
        U, V = cx + fx * (xn * s), cy + fy * (yn * s)
    return U, V, pz, g


def table_parts(p):
    """-> dict of the float64 intermediates per cell and `usable`, for the tests that count the classes"""
    i, j = np.meshgrid(np.arange(p.nx, dtype=f64), np.arange(p.ny, dtype=f64))
    dx, dy, fps = f64(p.dx), f64(p.dy), f64(p.fps)
    with np.errstate(all="ignore"):
        X, Y = f64(p.x0) + i * dx, f64(p.y0) + j * dy
        hx, hy = f64(0.5) * dx, f64(0.5) * dy
        U, V, pz, g = project(p, X, Y)
        UE, VE, pzE, gE = project(p, X + hx, Y)
        UW, VW, pzW, gW = project(p, X - hx, Y)
        US, VS, pzS, gS = project(p, X, Y + hy)
        UN, VN, pzN, gN = project(p, X, Y - hy)
        a, b, c, d = (UE - UW) / dx, (US - UN) / dy, (VE - VW) / dx, (VS - VN) / dy
        det = a * d - b * c
        m00, m01, m10, m11 = d / det * fps, -b / det * fps, -c / det * fps, a / det * fps
        gsd = np.sqrt(np.fabs(f64(1) / det))
        front = (pz > 0) & (pzE > 0) & (pzW > 0) & (pzS > 0) & (pzN > 0)
        unfolded = (g > 0) & (gE > 0) & (gW > 0) & (gS > 0) & (gN > 0)
        finite = np.ones(U.shape, bool)
        for q in (U, V, det, m00, m01, m10, m11, gsd):
            finite &= np.isfinite(q)
        usable = front & unfolded & finite & (det != 0) & (gsd <= f64(p.max_gsd))
    return dict(X=X, Y=Y, U=U, V=V, m00=m00, m01=m01, m10=m10, m11=m11, gsd=gsd, det=det, front=front, unfolded=unfolded,
                finite=finite, usable=usable)


def table(p):
    """-> ny x nx x 8 float32: U, V, m00, m01, m10, m11, gsd, 1.0; eight zeros where the cell is not usable"""
    t = table_parts(p)
    out = np.zeros((p.ny, p.nx, 8), f32)
    with np.errstate(over="ignore"):
        for k, name in enumerate(("U", "V", "m00", "m01", "m10", "m11", "gsd")):
            out[..., k] = t[name].astype(f32)
    out[..., 7] = f32(1)
    out[~t["usable"]] = f32(0)
    return out


def seen_cells(tab, w, h):
    """the sampler's test at the table's (U, V) for a w x h image; a zero record fails it (U = 0)"""
    z = np.zeros((h, w, 2), f32)
    ok, _, _ = sample(z, tab[..., 0], tab[..., 1])
    return ok


def picture(tab, seen, bgr):
    """the warps' sample: fractions of 1/32 pixel, weights of 2^15, rounded per channel; a tap outside counts 0"""
    h, w = bgr.shape[:2]
    U, V = np.where(seen, tab[..., 0], f32(0)), np.where(seen, tab[..., 1], f32(0))
    ix, iy = np.rint(U * f32(32)).astype(np.int64), np.rint(V * f32(32)).astype(np.int64)
    sx, sy, fx, fy = ix >> 5, iy >> 5, ix & 31, iy & 31
    pad = np.zeros((h + 2, w + 2, 3), np.int64)
    pad[:h, :w] = bgr
    tap = lambda x, y: pad[np.where((x >= 0) & (x < w) & (y >= 0) & (y < h), y, h), np.where((x >= 0) & (x < w), x, w)]
    w00, w01 = ((32 - fy) * (32 - fx) * 32)[..., None], ((32 - fy) * fx * 32)[..., None]
    w10, w11 = (fy * (32 - fx) * 32)[..., None], (fy * fx * 32)[..., None]
    v = tap(sx, sy) * w00 + tap(sx + 1, sy) * w01 + tap(sx, sy + 1) * w10 + tap(sx + 1, sy + 1) * w11
    out = ((v + (1 << 14)) >> 15).astype(np.uint8)
    return np.where(seen[..., None], out, np.uint8(0)).astype(np.uint8)


def push(tab, w, h, flow, bgr, pushes):
    """one push -> dict(plan ny x nx x 2 float32, mask uint8, bgr (or None), usable, seen, valid bool, summary 8 int64).
    flow or bgr may be None; without the field nothing is valid and the plan and the mask are zero."""
    usable = tab[..., 7] != 0
    seen = seen_cells(tab, w, h)
    plan = np.zeros(tab.shape[:2] + (2,), f32)
    valid = np.zeros(tab.shape[:2], bool)
    maxbits = 0
    if flow is not None:
        flow = np.asarray(flow, f32)
        assert flow.shape == (h, w, 2)
        _, sx, sy = sample(flow, tab[..., 0], tab[..., 1])
        valid = seen & np.isfinite(sx) & np.isfinite(sy)
        with np.errstate(invalid="ignore", over="ignore"):
            vx = tab[..., 2] * sx + tab[..., 3] * sy
            vy = tab[..., 4] * sx + tab[..., 5] * sy
            plan[..., 0] = np.where(valid, vx, f32(0))
            plan[..., 1] = np.where(valid, vy, f32(0))
            m2 = (vx * vx + vy * vy).astype(f32)
        ok = valid & ~np.isnan(m2)
        maxbits = int(m2[ok].view(np.uint32).max()) if ok.any() else 0
    summary = np.array([usable.sum(), seen.sum(), valid.sum(), maxbits, pushes, 0, 0, 0], np.int64)
    return dict(plan=plan, mask=(valid * 255).astype(np.uint8), bgr=None if bgr is None else picture(tab, seen, np.asarray(bgr, np.uint8)),
                usable=usable, seen=seen, valid=valid, summary=summary)


class PlanViewRef:
    """a session: the table of open, pushes counted from open / reset"""

    def __init__(self, w, h, p):
        self.w, self.h, self.p = w, h, p
        self.table = table(p)
        self.pushes = 0

    def reset(self):
        self.pushes = 0

    def push(self, flow=None, bgr=None):
        self.pushes += 1
        return push(self.table, self.w, self.h, flow, bgr, self.pushes)


# ---------------------------------------------------------------------------- cameras and inputs
def tilted_camera(w, h, f, height=10.0, tilt_deg=20.0):
    """a pinhole `height` metres above the plane Z = 0 at X = Y = 0, looking along +Y and tilted down by tilt_deg, the
    principal point at the image centre -> (H 3 x 3, f, f, cx, cy)"""
    t = math.radians(tilt_deg)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    R = np.array([[1.0, 0.0, 0.0], [0.0, -math.sin(t), -math.cos(t)], [0.0, math.cos(t), -math.sin(t)]])   # rows: right, down, forward
    C = np.array([0.0, 0.0, height])
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    P = K @ np.column_stack([R[:, 0], R[:, 1], -R @ C])
    return P, float(f), float(f), cx, cy


def shore_camera(w=97, h=53, f=90.0, nx=61, ny=37, dx=1.0, dy=1.5, max_gsd=0.6, k1=0.0, k2=0.0, fps=10.0):
    """the camera of both tiers (the issue's): 97 x 53 -> 61 x 37 from (-30, -6) in cells of 1 x 1.5 m"""
    H, fx, fy, cx, cy = tilted_camera(w, h, f)
    return Params(H, fx, fy, cx, cy, k1, k2, -30.0, -6.0, dx, dy, nx, ny, fps, max_gsd)


def identity(w, h):
    return Params(np.eye(3), 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, w, h, 1.0, math.inf)


def jacobian(p, X, Y):
    """the analytic derivative of project() at ground points -> (U, V, a, b, c, d) with [[a, b], [c, d]] = d(U, V) / d(X, Y)"""
    H = p.H
    px, py, pz = H[0] * X + H[1] * Y + H[2], H[3] * X + H[4] * Y + H[5], H[6] * X + H[7] * Y + H[8]
    u, v = px / pz, py / pz
    ux, uy, vx, vy = (H[0] - u * H[6]) / pz, (H[1] - u * H[7]) / pz, (H[3] - v * H[6]) / pz, (H[4] - v * H[7]) / pz
    xn, yn = (u - p.cx) / p.fx, (v - p.cy) / p.fy
    xnx, xny, ynx, yny = ux / p.fx, uy / p.fx, vx / p.fy, vy / p.fy
    r2 = xn * xn + yn * yn
    s = 1 + p.k1 * r2 + p.k2 * r2 * r2
    sr = p.k1 + 2 * p.k2 * r2
    sx, sy = sr * 2 * (xn * xnx + yn * ynx), sr * 2 * (xn * xny + yn * yny)
    U, V = p.cx + p.fx * xn * s, p.cy + p.fy * yn * s
    return U, V, p.fx * (xnx * s + xn * sx), p.fx * (xny * s + xn * sy), p.fy * (ynx * s + yn * sx), p.fy * (yny * s + yn * sy)


def ground_flow_field(p, w, h, vel, iters=30, tol=1e-10):
    """the image flow (pixels per field, h x w x 2 float32) of a uniform ground velocity vel (m/s) seen through the camera:
    every pixel's ground point by Newton on project(), then the analytic Jacobian times vel / fps.  NaN where the pixel
    sees no ground (above the horizon) or Newton does not reach tol pixels."""
    y, x = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing="ij")
    Hi = np.linalg.inv(np.asarray(p.H, f64).reshape(3, 3))
    with np.errstate(all="ignore"):
        gz = Hi[2, 0] * x + Hi[2, 1] * y + Hi[2, 2]
        X, Y = (Hi[0, 0] * x + Hi[0, 1] * y + Hi[0, 2]) / gz, (Hi[1, 0] * x + Hi[1, 1] * y + Hi[1, 2]) / gz
        for _ in range(iters):
            U, V, a, b, c, d = jacobian(p, X, Y)
            ru, rv, det = U - x, V - y, a * d - b * c
            X, Y = X - (d * ru - b * rv) / det, Y - (a * rv - c * ru) / det
        U, V, a, b, c, d = jacobian(p, X, Y)
        pz = p.H[6] * X + p.H[7] * Y + p.H[8]
        good = (np.hypot(U - x, V - y) < tol) & (pz > 0)
        fx_, fy_ = (a * vel[0] + b * vel[1]) / p.fps, (c * vel[0] + d * vel[1]) / p.fps
    f = np.stack([fx_, fy_], -1)
    f[~good] = np.nan
    return f.astype(f32)


def wavy_field(w, h, seed=3, k=0):
    """a finite field with no zero component: shear waves, a drift, noise"""
    rng = np.random.default_rng(seed + k)
    y, x = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing="ij")
    u = 0.9 * np.sin(2 * np.pi * y / 23 + 0.3 * k) + 0.004 * (x - w / 2) + 1.1
    v = 0.9 * np.cos(2 * np.pi * x / 31 - 0.3 * k) - 0.004 * (y - h / 2) - 0.6
    f = (np.stack([u, v], -1) + 0.05 * rng.standard_normal((h, w, 2))).astype(f32)
    f[f == 0] = f32(0.5)
    return f


def frame(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
