"""The wave spectra of include/rcflow.h ("wave spectra") in numpy: the statement waves_kernels.hip is held to.

Everything up to the cell sums is integer and exact; the closing is double, every operation rounded on its own, in the
header's order, with math.atan2 and math.atanh where the device has its own (a stored float may differ from the device's by
one unit in the last place).  Arrays are [row][column]; a frame is h x w uint8."""
import math

import numpy as np

f32 = np.float32
EMPTY, NOWAVE, DEEP = 1, 2, 4
MAX_WINDOW, MAX_BINS, MAX_SPACING = 4096, 16, 16
TWO_PI = 6.283185307179586
RECORD_DTYPE = np.dtype([("bin", "<i4"), ("flags", "<i4"), ("freq_hz", "<f4"), ("kx", "<f4"), ("ky", "<f4"), ("celerity", "<f4"),
                         ("depth", "<f4"), ("quality", "<f4")])
assert RECORD_DTYPE.itemsize == 32


def table(window):
    """-> (Tc, Ts) int32 [window]: lrint(2048 cos(2 pi j / W)), lrint(2048 sin(2 pi j / W)), in double"""
    j = np.arange(window, dtype=np.float64)
    a = (TWO_PI * j) / float(window)
    return np.rint(2048.0 * np.cos(a)).astype(np.int32), np.rint(2048.0 * np.sin(a)).astype(np.int32)


def shift_of(window):
    return max(0, (255 * 2048 * window).bit_length() - 15)


def rescan(ring, bins, tc, ts):
    """the quantised-table DFT of a whole ring [W][h][w] uint8 -> K x h x w x 2 int64"""
    W = ring.shape[0]
    r = ring.astype(np.int64)
    out = np.zeros((len(bins),) + ring.shape[1:] + (2,), np.int64)
    c = np.arange(W)
    for k, b in enumerate(bins):
        j = (b * c) % W
        out[k, ..., 0] = np.tensordot(tc[j].astype(np.int64), r, 1)
        out[k, ..., 1] = -np.tensordot(ts[j].astype(np.int64), r, 1)
    return out


def participating(w, h, s, mask=None):
    """pixel (x, y) takes part: s <= x < w - s, s <= y < h - s, and the mask non-zero at it and at its four neighbours at +-s"""
    part = np.zeros((h, w), bool)
    if w > 2 * s and h > 2 * s:
        part[s:h - s, s:w - s] = True
        if mask is not None:
            m = np.asarray(mask) != 0
            part[s:h - s, s:w - s] &= m[s:h - s, s:w - s] & m[s:h - s, 2 * s:] & m[s:h - s, :w - 2 * s] & m[2 * s:, s:w - s] & m[:h - 2 * s, s:w - s]
    return part


def cell_index(w, h, gx, gy):
    """ripmap's cell of a pixel: min(x / (w / gx), gx - 1), the remainder columns and rows in the last cell -> (cx [w], cy [h])"""
    return np.minimum(np.arange(w) // (w // gx), gx - 1), np.minimum(np.arange(h) // (h // gy), gy - 1)


def cell_sums(acc, sh, s, gx, gy, mask=None):
    """acc K x h x w x 2 int64 -> gy x gx x K x 6 int64: n, P, Re Cx, Im Cx, Re Cy, Im Cy"""
    K, h, w = acc.shape[:3]
    X = acc >> sh                                             # arithmetic, per component
    assert np.abs(X).max(initial=0) < 2 ** 15
    part = participating(w, h, s, mask)
    cx, cy = cell_index(w, h, gx, gy)
    cell = (cy[:, None] * gx + cx[None, :])[part]
    sums = np.zeros((gy * gx, K, 6), np.int64)
    ys, xs = np.nonzero(part)
    for k in range(K):
        C, E, Wn, S, N = X[k, ys, xs], X[k, ys, xs + s], X[k, ys, xs - s], X[k, ys + s, xs], X[k, ys - s, xs]
        vals = (np.ones(len(ys), np.int64), C[:, 0] * C[:, 0] + C[:, 1] * C[:, 1],
                E[:, 0] * Wn[:, 0] + E[:, 1] * Wn[:, 1], E[:, 1] * Wn[:, 0] - E[:, 0] * Wn[:, 1],
                S[:, 0] * N[:, 0] + S[:, 1] * N[:, 1], S[:, 1] * N[:, 0] - S[:, 0] * N[:, 1])
        for q, v in enumerate(vals):
            np.add.at(sums[:, k, q], cell, v)
    return sums.reshape(gy, gx, K, 6)


def close_cell(sums, bins, window, s, fps, mx, my, gravity, tanh_max, min_pixels):
    """one cell's K x 6 sums -> (record tuple in RECORD_DTYPE's order with the floats still double, t or None)"""
    n = int(sums[0, 0])
    P = [int(v) for v in sums[:, 1]]
    if n < min_pixels or not any(P):
        return (0, EMPTY, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), None
    k = 0
    for q in range(1, len(bins)):
        if P[q] > P[k]:                                       # the lowest bin wins ties
            k = q
    b = bins[k]
    cxr, cxi, cyr, cyi = (int(v) for v in sums[k, 2:6])
    kx = math.atan2(float(-cxi), float(cxr)) / float(2 * s) / mx
    ky = math.atan2(float(-cyi), float(cyr)) / float(2 * s) / my
    kmag = math.sqrt(kx * kx + ky * ky)
    freq = float(b) * fps / float(window)
    omega = TWO_PI * float(b) * fps / float(window)
    ax, ay = float(cxr), float(cxi)
    bx, by = float(cyr), float(cyi)
    quality = (math.sqrt(ax * ax + ay * ay) + math.sqrt(bx * bx + by * by)) / (2.0 * float(P[k]))
    if kmag == 0.0:
        return (b, NOWAVE, freq, kx, ky, 0.0, 0.0, quality), None
    celerity = omega / kmag
    t = omega * omega / (gravity * kmag)
    if t < tanh_max:
        return (b, 0, freq, kx, ky, celerity, math.atanh(t) / kmag, quality), t
    return (b, DEEP, freq, kx, ky, celerity, 0.0, quality), t


def jet_index(depth, vis_max_depth):
    """FTLE's picture index: rint(depth / (float)vis_max_depth * 255) saturated to 0..255, in float32"""
    with np.errstate(over="ignore"):
        r = np.rint(np.asarray(depth, f32) / f32(vis_max_depth) * f32(255))
    return np.clip(np.nan_to_num(r, nan=0.0, posinf=255.0), 0, 255).astype(np.int64)


class Params:
    def __init__(self, window, bin_lo, bin_hi, spacing=1, grid_x=1, grid_y=1, min_pixels=1, fps=2.0, metres_per_pixel_x=1.0,
                 metres_per_pixel_y=1.0, gravity=9.81, tanh_max=0.95, vis_max_depth=10.0):
        self.window, self.bin_lo, self.bin_hi, self.spacing, self.grid_x, self.grid_y = window, bin_lo, bin_hi, spacing, grid_x, grid_y
        self.min_pixels, self.fps, self.metres_per_pixel_x, self.metres_per_pixel_y = min_pixels, fps, metres_per_pixel_x, metres_per_pixel_y
        self.gravity, self.tanh_max, self.vis_max_depth = gravity, tanh_max, vis_max_depth

    def kw(self):
        return dict(self.__dict__)

    @property
    def bins(self):
        return list(range(self.bin_lo, self.bin_hi + 1))


class WavesRef:
    """a session: the ring of the last `window` frames (zeros at open), the accumulators, pushes counted from open / reset"""

    def __init__(self, w, h, p, lut=None):
        self.w, self.h, self.p, self.lut = w, h, p, lut
        self.tc, self.ts = table(p.window)
        self.sh = shift_of(p.window)
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.p.window, self.h, self.w), np.uint8)
        self.acc = np.zeros((len(self.p.bins), self.h, self.w, 2), np.int64)
        self.pushes = 0

    def push(self, gray, mask=None, compute=True):
        p = self.p
        gray = np.asarray(gray, np.uint8)
        assert gray.shape == (self.h, self.w)
        c = self.pushes % p.window
        d = gray.astype(np.int64) - self.ring[c].astype(np.int64)
        self.ring[c] = gray
        for k, b in enumerate(p.bins):
            j = (b * c) % p.window
            self.acc[k, ..., 0] += d * int(self.tc[j])
            self.acc[k, ..., 1] -= d * int(self.ts[j])
        assert np.abs(self.acc).max() < 2 ** 31
        self.pushes += 1
        return self.outputs(mask) if compute else None

    def outputs(self, mask=None):
        """-> dict(sums, records, t (double, NaN where there is none), depth64, bin_map, index, vis, summary)"""
        p = self.p
        gx, gy = p.grid_x, p.grid_y
        sums = cell_sums(self.acc, self.sh, p.spacing, gx, gy, mask)
        rec = np.zeros((gy, gx), RECORD_DTYPE)
        t = np.full((gy, gx), np.nan)
        depth64 = np.zeros((gy, gx))
        for j in range(gy):
            for i in range(gx):
                r, tt = close_cell(sums[j, i], p.bins, p.window, p.spacing, p.fps, p.metres_per_pixel_x, p.metres_per_pixel_y, p.gravity,
                                   p.tanh_max, p.min_pixels)
                rec[j, i] = r
                depth64[j, i] = r[6]
                if tt is not None:
                    t[j, i] = tt
        cx, cy = cell_index(self.w, self.h, gx, gy)
        bin_map = rec["bin"][cy[:, None], cx[None, :]].astype(np.uint8)
        index = jet_index(rec["depth"], p.vis_max_depth)
        out = dict(sums=sums, records=rec, t=t, depth64=depth64, bin_map=bin_map, index=index)
        if self.lut is not None:
            colour = np.where((rec["flags"] == 0)[..., None], np.asarray(self.lut, np.uint8)[index], np.uint8(0)).astype(np.uint8)
            out["vis"] = colour[cy[:, None], cx[None, :]]
        nonempty = (rec["flags"] & EMPTY) == 0
        out["summary"] = np.array([min(self.pushes, p.window), sums[:, :, 0, 0].sum(), nonempty.sum(), (rec["flags"] == 0).sum(), self.pushes,
                                   0, 0, 0], np.int64)
        return out


# ---------------------------------------------------------------------------- inputs
def dispersion_k(omega, depth, gravity=9.81):
    """the wavenumber of omega^2 = g k tanh(k depth), by bisection"""
    lo, hi = omega * omega / gravity, omega * omega / gravity + omega / math.sqrt(gravity * depth) + 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if gravity * mid * math.tanh(mid * depth) < omega * omega:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def plane_wave(w, h, count, window, cycles, kx_px, ky_px, amp=60.0, sigma=10.0, seed=3, t0=0):
    """frames of 128 + amp cos(kx x + ky y - omega t) + noise, omega = 2 pi cycles / window per frame (cycles may be a fraction)"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    om = 2.0 * math.pi * cycles / window
    out = []
    for t in range(t0, t0 + count):
        v = 128.0 + amp * np.cos(kx_px * x + ky_px * y - om * t) + sigma * rng.standard_normal((h, w))
        out.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
    return out


def square_wave(w, h, count, window, b):
    """0 / 255 in step with bin b's cosine: every term of the real part has the table's own sign, the largest sum there is"""
    tc, _ = table(window)
    return [np.full((h, w), 255 if tc[(b * (t % window)) % window] > 0 else 0, np.uint8) for t in range(count)]


def noise_frames(w, h, count, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(count)]


def wave_params(window, bin_lo, bin_hi, b, depth, theta, spacing=2, grid_x=1, grid_y=1, fps=2.0, mpp=2.0, gravity=9.81, **kw):
    """Params and the per-pixel wavenumber (kx, ky) of a bin-centred wave of bin b over water `depth` metres deep, travelling
    towards theta"""
    k = dispersion_k(TWO_PI * b * fps / window, depth, gravity)
    p = Params(window, bin_lo, bin_hi, spacing, grid_x, grid_y, fps=fps, metres_per_pixel_x=mpp, metres_per_pixel_y=mpp, gravity=gravity, **kw)
    return p, k * math.cos(theta) * mpp, k * math.sin(theta) * mpp


def three_kinds(w, h, count, window, b, kx_px, ky_px):
    """columns 0..19 black, 20..41 one series for every pixel (no phase gradient), from 42 on a plane wave over noise"""
    frames = plane_wave(w, h, count, window, b, kx_px, ky_px)
    om = 2.0 * math.pi * b / window
    for t, f in enumerate(frames):
        f[:, :20] = 0
        f[:, 20:42] = int(round(128 + 100 * math.cos(om * t)))
    return frames


def blob_mask(w, h, seed=5):
    """most pixels set, holes of every size, one corner cleared entirely"""
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) > 0.08).astype(np.uint8) * 255
    m[:h // 3, :w // 4] = 0
    m[m != 0] = rng.integers(1, 256, int((m != 0).sum()), dtype=np.uint8)      # non-zero, not only 255
    return m


class Case:
    """one input of both tiers: the frames, the pushes that compute (1-based), the mask of those pushes"""

    def __init__(self, w, h, p, frames, compute, mask=None, pad=0, sets=None):
        self.w, self.h, self.p, self.frames, self.compute, self.mask, self.pad = w, h, p, frames, set(compute), mask, pad
        self.sets = sets or {}                                # push -> (tanh_max, min_pixels, vis_max_depth) set before it


def cpp_case(count=40):
    """the input tests/cpp/test_waves.cpp makes for itself from integers: every fifth push computes, under a mask with a hole"""
    w, h = 61, 37
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    mask = np.where((x >= 30) & (x < 34) & (y >= 10) & (y < 14), 0, 1 + (x + y) % 255).astype(np.uint8)
    frames = [((x * 37 + y * 11 + t * 48 + (x * y * (t + 1)) % 23) % 256).astype(np.uint8) for t in range(count)]
    p = Params(16, 2, 5, 2, 3, 2, 1, 1.0, 1.0, 0.5, 9.8125, 0.9375, 2.0)
    return Case(w, h, p, frames, {t + 1 for t in range(count) if t % 5 == 3}, mask=mask)


def cases():
    """name -> Case.  61 x 37 and 130 x 9 are ragged against groups of 4 pixels and waves of 64 columns; windows 3, 7, 12 and 128
    (a window of 2 has no bin: 2 bin_hi < W); 1 and 16 bins; spacing 1, 2 and 16; grids that do not divide the frame and 1 x 1;
    every case but the two large ones, whose cells launches have waves that walk three and five rows, crosses its ring twice"""
    c = {}
    c["w3"] = Case(61, 37, Params(3, 1, 1, 1, 5, 4, min_pixels=3), noise_frames(61, 37, 8, 1), {1, 2, 3, 4, 8}, pad=3)
    c["w7"] = Case(61, 37, Params(7, 3, 3, 1, 4, 3, vis_max_depth=3.0), noise_frames(61, 37, 16, 2), {1, 3, 7, 8, 15, 16}, pad=3)
    c["w12-mask"] = Case(130, 9, Params(12, 1, 5, 1, 1, 1, fps=4.0, metres_per_pixel_x=0.5, metres_per_pixel_y=0.7),
                         noise_frames(130, 9, 26, 3), {2, 12, 13, 26}, mask=blob_mask(130, 9), pad=5)
    p, kx, ky = wave_params(128, 4, 19, 8, 3.0, math.radians(200), grid_x=3, grid_y=2, vis_max_depth=6.0)
    c["w128-k16"] = Case(61, 37, p, plane_wave(61, 37, 260, 128, 8, kx, ky), {5, 128, 200, 260})
    p, kx, ky = wave_params(128, 8, 8, 8, 3.0, math.radians(-35), grid_x=2, grid_y=2, vis_max_depth=6.0, min_pixels=50)
    c["w128-k1-mask"] = Case(130, 9, p, plane_wave(130, 9, 258, 128, 8, kx, ky, seed=4), {128, 258}, mask=blob_mask(130, 9, 6), pad=2)
    p, kx, ky = wave_params(12, 2, 4, 3, 1.0, math.radians(80), spacing=16, grid_x=2, grid_y=1, fps=1.0, mpp=0.25, vis_max_depth=2.0, min_pixels=72)
    c["s16"] = Case(61, 37, p, plane_wave(61, 37, 25, 12, 3, kx, ky, seed=5), {12, 25}, pad=1)
    c["s16-nobody"] = Case(130, 9, Params(12, 2, 4, 16, 3, 2), noise_frames(130, 9, 25, 6), {1, 25})
    p, kx, ky = wave_params(16, 2, 5, 3, 1.5, math.radians(20), grid_x=3, grid_y=1, fps=1.0, mpp=1.0, vis_max_depth=2.0)
    c["three-kinds"] = Case(61, 37, p, three_kinds(61, 37, 34, 16, 3, kx, ky), {16, 33, 34}, sets={34: (0.3, 1, 2.0)})
    # the cells launch keeps to WV_MAX_BLOCKS blocks (waves_kernels.hip), a wave walking several rows above that: 9 x 128 groups of
    # four rows times 4 and 8 bins are 3 and 5 rows a wave (tests/test_waves_ref.py computes it from the source).  Neither is a
    # multiple of the four rows a wave keeps in flight, 509 is no multiple of 12 or 20, and the cell rows of 101 pixels begin
    # inside a wave's walk
    c["three-rows"] = Case(520, 509, Params(12, 2, 5, 1, 7, 5, min_pixels=3000, fps=30.0, metres_per_pixel_x=0.1, metres_per_pixel_y=0.1,
                                            vis_max_depth=1.0),
                           noise_frames(520, 509, 4, 7), {2, 4}, mask=blob_mask(520, 509, 8), pad=7)
    c["five-rows"] = Case(520, 509, Params(24, 2, 9, 2, 6, 4, fps=30.0, metres_per_pixel_x=0.1, metres_per_pixel_y=0.1, vis_max_depth=1.0),
                          noise_frames(520, 509, 3, 9), {3}, mask=blob_mask(520, 509, 10), pad=3)
    c["cpp"] = cpp_case()
    c["w4096"] = Case(16, 8, Params(4096, 5, 5, 1, 2, 1), square_wave(16, 8, 4100, 4096, 5), {4096, 4100})
    return c


def run_case(case, lut=None):
    """the statement's outputs of every computing push of a case, in order: [(push, outputs)]"""
    ref = WavesRef(case.w, case.h, Params(**case.p.kw()), lut)
    out = []
    for t, f in enumerate(case.frames, 1):
        if t in case.sets:
            ref.p.tanh_max, ref.p.min_pixels, ref.p.vis_max_depth = case.sets[t]
        r = ref.push(f, case.mask, compute=t in case.compute)
        if r is not None:
            r["tanh_max"], r["min_pixels"] = ref.p.tanh_max, ref.p.min_pixels
            out.append((t, r))
    return ref, out
