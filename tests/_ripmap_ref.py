"""The opposing-flow map (ripcurrents_amd/csrc/ripmap_kernels.hip) stated in numpy, the slow obvious way.

averageVector (ripcurrents_module.cpp:386-484 of the reference) finished: a ring of the last `window` flow fields and
their mean in rcflow_window_mean_dev's operation order, the mean in 16.16 fixed point summed per cell of a grid, a global
vector, and a decision per cell in float64 with every operation rounded on its own, in one fixed order.  Integer sums do
not depend on the order of addition, so sums, counts and flags are compared bit for bit with the device; angles are
atan2 and compared within a tolerance.
"""
import numpy as np

f32 = np.float32
K_DEFAULT = 0.3454915028125263          # cos^2(0.7 pi), ripcurrents_module.cpp:471
QMAX = float(2 ** 40)


def cell_index(n, g):
    """Cell of every coordinate 0..n-1: the reference's integer cell size n // g, the remainder going to the last cell."""
    return np.minimum(np.arange(n) // (n // g), g - 1)


def window_mean_push(avg, slot, v, window):
    """k_window_mean (main.cpp:1142-1153) in place, float32, operation by operation."""
    inv = f32(1.0 / float(f32(window)))
    t = slot * inv
    a = avg - t
    slot[...] = v
    t = v * inv
    avg[...] = a + t


def get_delta_zero(flow, UPPER, dt=2.0):
    """get_delta (ripcurrents_module.cpp:650-679) from a zero point: the bilinear sample at an integer position keeps
    its four taps (a NaN neighbour still poisons the sum), the border and vectors longer than UPPER stay zero."""
    f = np.asarray(flow, f32)
    h, w = f.shape[:2]
    out = np.zeros_like(f)
    if w < 3 or h < 3:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        p00, p01, p10, p11 = f[1:h - 1, 1:w - 1], f[1:h - 1, 2:w], f[2:h, 1:w - 1], f[2:h, 2:w]
        one, zero = f32(1), f32(0)
        d = p00 * one * one + p01 * zero * one + p10 * one * zero + p11 * zero * zero
        r = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        keep = ~(r > f32(UPPER))
        moved = f32(0) + d * f32(dt)
        out[1:h - 1, 1:w - 1] = np.where(keep[..., None], moved, f32(0))
    return out


def cell_sums(avg, gx, gy, order=None):
    """-> (sums [gy][gx][Sx, Sy, n] int64, bad pixels).  order: a permutation of the h * w pixels to add in."""
    a = np.asarray(avg, f32)
    h, w = a.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        q = a * f32(65536.0)
        good = (np.abs(q[..., 0]) <= f32(QMAX)) & (np.abs(q[..., 1]) <= f32(QMAX))     # NaN fails
        qi = np.where(good[..., None], np.rint(q), 0).astype(np.int64)
    cy, cx = np.meshgrid(cell_index(h, gy), cell_index(w, gx), indexing="ij")
    idx = (cy * gx + cx).ravel()
    vals = np.stack([qi[..., 0].ravel(), qi[..., 1].ravel(), good.ravel().astype(np.int64)], -1)
    if order is not None:
        idx, vals = idx[order], vals[order]
    sums = np.zeros((gy * gx, 3), np.int64)
    np.add.at(sums, idx, vals)
    return sums.reshape(gy, gx, 3), int((~good).sum())


def decide(sums, K=K_DEFAULT, M=0.0, gate=False):
    """-> dict(opposed bool grid, cells grid x 4 float32, direction, mean_magnitude, opposed_cells, live_cells)."""
    S = np.asarray(sums, np.int64)
    G = S.reshape(-1, 3).sum(0)                              # int64: exact
    Sx, Sy, n = S[..., 0].astype(np.float64), S[..., 1].astype(np.float64), S[..., 2].astype(np.float64)
    Gx, Gy = np.float64(G[0]), np.float64(G[1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dot = Sx * Gx + Sy * Gy
        cc = Sx * Sx + Sy * Sy
        gg = Gx * Gx + Gy * Gy
        need = (np.float64(M) * 65536.0) * n
        opposed = (S[..., 2] > 0) & (dot < 0) & (dot * dot > np.float64(K) * (cc * gg)) & (cc >= need * need)
        if gate:
            opposed = np.zeros_like(opposed)
        live = S[..., 2] > 0
        cells = np.zeros(S.shape[:2] + (4,), f32)
        cells[..., 0] = np.where(live, Sx / 65536.0 / n, 0).astype(f32)
        cells[..., 1] = np.where(live, Sy / 65536.0 / n, 0).astype(f32)
        cross = Sx * Gy - Sy * Gx
        cells[..., 2] = np.where(live, np.degrees(np.arctan2(np.abs(cross), dot)), 0).astype(f32)
        cells[..., 3] = opposed
        direction = float(np.degrees(np.arctan2(Gy, Gx)))
        if direction < 0:
            direction += 360.0
        if direction >= 360.0:
            direction = 0.0
        mag = 0.0
        if G[2] > 0:
            mx, my = Gx / 65536.0 / np.float64(G[2]), Gy / 65536.0 / np.float64(G[2])
            mag = float(np.sqrt(mx * mx + my * my))
    return dict(opposed=opposed, cells=cells, direction=direction, mean_magnitude=mag, opposed_cells=int(opposed.sum()),
                live_cells=int(live.sum()))


def max_magnitude(avg):
    """max |avg| as the device keeps it: float32 per pixel, NaN ignored (fmaxf), 0 for an empty maximum."""
    a = np.asarray(avg, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        mag = np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1])
    mag = mag[~np.isnan(mag)]
    return f32(mag.max()) if mag.size else f32(0)


def mask_of(opposed, w, h):
    gy, gx = opposed.shape
    return (opposed[cell_index(h, gy)][:, cell_index(w, gx)] * 255).astype(np.uint8)


class RipMapRef:
    """The session: push(flow) -> the result of that push."""

    def __init__(self, w, h, window, grid=(30, 30), source=0, wait_full=False, K=K_DEFAULT, M=0.0, UPPER=100.0, color=None):
        self.w, self.h, self.window, self.grid, self.source, self.wait_full = w, h, window, grid, source, wait_full
        self.K, self.M, self.UPPER, self.color = K, M, UPPER, color
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.window, self.h, self.w, 2), f32)
        self.avg = np.zeros((self.h, self.w, 2), f32)
        self.frames, self.cur = 0, 0
        self.scale = f32(1e-6)              # max_displacement before the first frame (main.cpp:1069)

    def push(self, flow):
        v = np.asarray(flow, f32)
        if self.source == 1:
            v = get_delta_zero(v, self.UPPER)
        with np.errstate(invalid="ignore", over="ignore"):
            window_mean_push(self.avg, self.ring[self.cur], v, self.window)
        self.cur = (self.cur + 1) % self.window
        self.frames += 1
        gx, gy = self.grid
        sums, bad = cell_sums(self.avg, gx, gy)
        r = decide(sums, self.K, self.M, gate=self.wait_full and self.frames < self.window)
        r.update(sums=sums, bad_pixels=bad, frames_pushed=self.frames, mean=self.avg.copy(), scale_in=self.scale,
                 mask=mask_of(r["opposed"], self.w, self.h))
        if self.color is not None:          # vectorToColor of the mean with the previous push's maximum
            r["hsv"] = self.color(self.avg, float(self.scale))[0]
        self.scale = r["max_magnitude"] = max_magnitude(self.avg)
        return r
