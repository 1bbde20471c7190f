"""The ensemble PIV of include/rcflow.h ("ensemble PIV") stated in numpy: block cross-correlation of interrogation windows between
consecutive grey frames, the correlation sums added over the last `ensemble` pairs before the peak is taken, a three-point
parabolic sub-pixel step and the normalised median test.  Every sum is an integer and exact; the score, the peak and the
sub-pixel step are double, the median test is float32, each operation rounded on its own.  The device (piv_kernels.hip) is held
to this bit for bit in every integer and within one unit in the last place in the records' floats."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

f32 = np.float32
EMPTY, FLAT, EDGE, LOWPEAK, OUTLIER = 1, 2, 4, 8, 16
INVALID = EMPTY | FLAT | LOWPEAK
REPLACE = 1
MAX_CELLS = 16384
MAX_STATE_BYTES = 4 << 30
LAUNCHES = 3
CELL_DTYPE = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("peak", "<f4"), ("resid", "<f4"), ("ix", "<i4"), ("iy", "<i4"), ("flags", "<i4"),
                       ("pairs", "<i4")])


class Params:
    def __init__(self, window, range, step, ensemble=1, flags=0, min_peak=0.25, median_eps=0.1, median_thr=2.0, vis_max=4.0):
        self.window, self.range, self.step, self.ensemble, self.flags = window, range, step, ensemble, flags
        self.min_peak, self.median_eps, self.median_thr, self.vis_max = min_peak, median_eps, median_thr, vis_max

    def kw(self):
        return dict(self.__dict__)


def params_ok(p):
    M, R, E = p.window, p.range, p.ensemble
    return (M % 4 == 0 and 8 <= M <= 64 and 1 <= R <= 16 and 1 <= p.step <= M and 1 <= E <= 256 and E * M * M <= 2 ** 18 and
            0.0 <= p.min_peak <= 1.0 and 0.0 < p.median_eps < math.inf and 0.0 < p.median_thr < math.inf and 0.0 < p.vis_max < math.inf and
            p.flags in (0, REPLACE))


def grid(w, h, p):
    """(grid_x, grid_y), or None where the frame is smaller than one search area"""
    need = p.window + 2 * p.range
    if w < need or h < need:
        return None
    return (w - need) // p.step + 1, (h - need) // p.step + 1


def window_sums(img, M, step, gx, gy):
    """sums over the M x M windows whose corners are (cx step, cy step) -> [gy, gx] int64"""
    return sliding_window_view(img, (M, M))[::step, ::step][:gy, :gx].sum((-1, -2), dtype=np.int64)


def pair_sums(A, B, p, gx, gy):
    """One pair's planes -> (S [gy, gx, D, D, 3] int64: Sab, Sb, Sbb per displacement (j outer, i inner); Sa, Saa [gy, gx])"""
    M, R, step = p.window, p.range, p.step
    D = 2 * R + 1
    ww, hh = (gx - 1) * step + M, (gy - 1) * step + M
    a = A[R:R + hh, R:R + ww].astype(np.int64)
    B = B.astype(np.int64)
    S = np.zeros((gy, gx, D, D, 3), np.int64)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            b = B[R + j:R + j + hh, R + i:R + i + ww]
            S[:, :, j + R, i + R, 0] = window_sums(a * b, M, step, gx, gy)
            S[:, :, j + R, i + R, 1] = window_sums(b, M, step, gx, gy)
            S[:, :, j + R, i + R, 2] = window_sums(b * b, M, step, gx, gy)
    return S, window_sums(a, M, step, gx, gy), window_sums(a * a, M, step, gx, gy)


def scores(T, Ta, Taa, n, M):
    """the signed square of the zero-normalised cross-correlation -> (s [gy, gx, D, D] float64, va [gy, gx] int64)"""
    N = n * M * M
    num = N * T[..., 0] - Ta[..., None, None] * T[..., 1]
    va = N * Taa - Ta * Ta
    vb = N * T[..., 2] - T[..., 1] * T[..., 1]
    assert max(np.abs(num).max(), va.max(), vb.max(), (N * T[..., 0]).max(), (Ta * Ta).max()) < 2 ** 53
    ok = (va[..., None, None] > 0) & (vb > 0)
    numd = num.astype(np.float64)
    den = np.where(ok, va[..., None, None].astype(np.float64) * vb.astype(np.float64), 1.0)
    return np.where(ok, (numd * np.abs(numd)) / den, 0.0), va


def _root(s):
    return math.copysign(math.sqrt(abs(s)), s)


def _offset(l, c, r):
    l, c, r = _root(l), _root(c), _root(r)
    e = (l - c) + (r - c)
    return (l - r) / (2.0 * e) if e < 0 else 0.0


def peaks(s, va, n, p):
    """the records before the median test"""
    gy, gx, D, _ = s.shape
    R = p.range
    rec = np.zeros((gy, gx), CELL_DTYPE)
    for cy in range(gy):
        for cx in range(gx):
            r = rec[cy, cx]
            if n == 0:
                r["flags"] = EMPTY
                continue
            r["pairs"] = n
            k = int(np.argmax(s[cy, cx]))                     # the first occurrence of the largest, j outer and i inner
            j, i = k // D, k % D
            top = float(s[cy, cx, j, i])
            r["peak"] = f32(top)
            if va[cy, cx] == 0 or top <= 0.0:
                r["flags"] = FLAT
                continue
            r["ix"], r["iy"] = i - R, j - R
            flags, ox, oy = 0, 0.0, 0.0
            if i == 0 or i == D - 1 or j == 0 or j == D - 1:
                flags |= EDGE
            else:
                ox = _offset(s[cy, cx, j, i - 1], top, s[cy, cx, j, i + 1])
                oy = _offset(s[cy, cx, j - 1, i], top, s[cy, cx, j + 1, i])
            if top < p.min_peak:
                flags |= LOWPEAK
            r["dx"], r["dy"], r["flags"] = f32(float(i - R) + ox), f32(float(j - R) + oy), flags
    return rec


def _median(v):
    v = sorted(v)
    k = len(v)
    return v[k // 2] if k % 2 else (v[k // 2 - 1] + v[k // 2]) * f32(0.5)


def median_test(rec, p):
    """The normalised median test in float32 -> (records with resid and OUTLIER, field [gy, gx, 2] float32)"""
    gy, gx = rec.shape
    out = rec.copy()
    field = np.zeros((gy, gx, 2), f32)
    eps, thr = f32(p.median_eps), f32(p.median_thr)
    valid = (rec["flags"] & INVALID) == 0
    for cy in range(gy):
        for cx in range(gx):
            nb = [(y, x) for y in (cy - 1, cy, cy + 1) for x in (cx - 1, cx, cx + 1)
                  if (y, x) != (cy, cx) and 0 <= y < gy and 0 <= x < gx and valid[y, x]]
            if not valid[cy, cx]:
                continue
            field[cy, cx] = rec["dx"][cy, cx], rec["dy"][cy, cx]
            if len(nb) < 3:
                continue
            res, um = [], []
            for name in ("dx", "dy"):
                v = [f32(rec[name][y, x]) for y, x in nb]
                m = _median(v)
                rm = _median([abs(a - m) for a in v])
                res.append(abs(f32(rec[name][cy, cx]) - m) / (rm + eps))
                um.append(m)
            out["resid"][cy, cx] = max(res)
            if max(res) > thr:
                out["flags"][cy, cx] |= OUTLIER
                if p.flags & REPLACE:
                    field[cy, cx] = um
    return out, field


def jet_index(mag, vis_max):
    """the FTLE picture's index: rint(mag / (float)vis_max * 255) saturated to 0..255, in float32"""
    with np.errstate(over="ignore"):
        r = np.rint(np.asarray(mag, f32) / f32(vis_max) * f32(255))
    return np.clip(np.nan_to_num(r, nan=0.0, posinf=255.0), 0, 255).astype(np.int64)


def pixel_cells(w, h, p, gx, gy):
    """a pixel's cell: min((x - R) / step, gx - 1); -1 left of and above R -> (cx [w], cy [h])"""
    cx = np.minimum((np.arange(w) - p.range) // p.step, gx - 1)
    cy = np.minimum((np.arange(h) - p.range) // p.step, gy - 1)
    return np.where(np.arange(w) < p.range, -1, cx), np.where(np.arange(h) < p.range, -1, cy)


def picture(rec, field, w, h, p, lut):
    gy, gx = rec.shape
    valid = (rec["flags"] & INVALID) == 0
    index = jet_index(np.hypot(field[..., 0], field[..., 1]), p.vis_max)
    colour = np.where(valid[..., None], np.asarray(lut, np.uint8)[index], np.uint8(0)).astype(np.uint8)
    cx, cy = pixel_cells(w, h, p, gx, gy)
    vis = colour[np.maximum(cy, 0)[:, None], np.maximum(cx, 0)[None, :]]
    vis[cy < 0, :] = 0
    vis[:, cx < 0] = 0
    return vis, index


class PivRef:
    """One slot's session.  push() -> None for a push that only stores, else the outputs as a dict."""

    def __init__(self, w, h, p, lut=None):
        assert params_ok(p)
        self.w, self.h, self.p, self.lut = w, h, p, lut
        self.gx, self.gy = grid(w, h, p)
        assert self.gx * self.gy <= MAX_CELLS
        self.D = 2 * p.range + 1
        self.reset()

    def reset(self):
        gy, gx, D, E = self.gy, self.gx, self.D, self.p.ensemble
        self.prev, self.pushes = None, 0
        self.T = np.zeros((gy, gx, D, D, 3), np.int64)
        self.Ta, self.Taa = np.zeros((gy, gx), np.int64), np.zeros((gy, gx), np.int64)
        self.ring = [(np.zeros_like(self.T), np.zeros_like(self.Ta), np.zeros_like(self.Taa)) for _ in range(E)] if E > 1 else None
        self.history = []                                     # the last `ensemble` pairs, for rescan()

    @property
    def pairs(self):
        return max(self.pushes - 1, 0)

    @property
    def n(self):
        return min(self.pairs, self.p.ensemble)

    def push(self, frame, compute=True):
        frame = np.ascontiguousarray(frame, np.uint8)
        assert frame.shape == (self.h, self.w)
        if self.prev is not None:
            new = pair_sums(self.prev, frame, self.p, self.gx, self.gy)
            assert max(int(a.max()) for a in new) < 2 ** 31
            if self.ring is None:
                self.T, self.Ta, self.Taa = new
            else:
                slot = (self.pairs) % self.p.ensemble
                old = self.ring[slot]
                self.T, self.Ta, self.Taa = self.T + (new[0] - old[0]), self.Ta + (new[1] - old[1]), self.Taa + (new[2] - old[2])
                self.ring[slot] = new
            self.history = (self.history + [(self.prev, frame)])[-self.p.ensemble:]
        self.prev = frame
        self.pushes += 1
        return self.outputs() if compute else None

    def rescan(self):
        """the accumulators from the last n pairs themselves"""
        T, Ta, Taa = np.zeros_like(self.T), np.zeros_like(self.Ta), np.zeros_like(self.Taa)
        for a, b in self.history:
            s = pair_sums(a, b, self.p, self.gx, self.gy)
            T, Ta, Taa = T + s[0], Ta + s[1], Taa + s[2]
        return T, Ta, Taa

    def outputs(self):
        p, n = self.p, self.n
        if n:
            s, va = scores(self.T, self.Ta, self.Taa, n, p.window)
        else:
            s, va = np.zeros(self.T.shape[:4]), np.zeros_like(self.Ta)
        raw = peaks(s, va, n, p)
        rec, field = median_test(raw, p)
        out = dict(records=rec, field=field, scores=s, raw=raw)
        if self.lut is not None:
            out["vis"], out["index"] = picture(rec, field, self.w, self.h, p, self.lut)
        fl = rec["flags"]
        out["summary"] = np.array([n, fl.size, ((fl & INVALID) == 0).sum(), ((fl & FLAT) != 0).sum(), ((fl & LOWPEAK) != 0).sum(),
                                   ((fl & EDGE) != 0).sum(), ((fl & OUTLIER) != 0).sum(), self.pushes], np.int64)
        return out


# ---------------------------------------------------------------------------- decisions the device's last place could turn
def near(a, b):
    """a float32 within one unit in the last place of the float32 b"""
    a, b = np.asarray(a, f32), f32(b)
    return (a >= np.nextafter(b, f32(-np.inf))) & (a <= np.nextafter(b, f32(np.inf)))


def flag_exceptions(out, p):
    """cells whose peak lies within one unit in the last place of min_peak, or whose resid lies that near median_thr, or who have
    such a cell among their neighbours (its validity decides their medians)"""
    rec = out["records"]
    live = (rec["flags"] & (EMPTY | FLAT)) == 0
    a = live & near(rec["peak"], p.min_peak)
    grown = a.copy()
    gy, gx = a.shape
    for cy, cx in zip(*np.nonzero(a)):
        grown[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = True
    return grown | (live & (rec["resid"] > 0) & near(rec["resid"], p.median_thr))


def doubtful_cells(out, p):
    """cells whose colour index changes under one unit in the last place of a field component or of the magnitude"""
    f, idx = out["field"], out["index"]
    valid = (out["records"]["flags"] & INVALID) == 0
    doubt = np.zeros(idx.shape, bool)
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            fx = np.nextafter(f[..., 0], f32(sx * np.inf)) if sx else f[..., 0]
            fy = np.nextafter(f[..., 1], f32(sy * np.inf)) if sy else f[..., 1]
            m = np.hypot(fx, fy)
            for sm in (-1, 0, 1):
                mm = np.nextafter(m, f32(sm * np.inf)) if sm else m
                doubt |= jet_index(mm, p.vis_max) != idx
    return doubt & valid


def doubtful_share(out, w, h, p):
    gy, gx = out["index"].shape
    cx, cy = pixel_cells(w, h, p, gx, gy)
    d = doubtful_cells(out, p)[np.maximum(cy, 0)[:, None], np.maximum(cx, 0)[None, :]]
    d[cy < 0, :] = False
    d[:, cx < 0] = False
    return d


# ---------------------------------------------------------------------------- inputs
def noise_frames(w, h, count, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(count)]


def binary_frames(w, h, count, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 2, (h, w)) * 255).astype(np.uint8) for _ in range(count)]


def drifting_frames(w, h, count, seed, shifts, sigma=6.0, patch=None):
    """a random texture moved by whole pixels (shifts[t] = (u, v) of frame t against frame 0) under fresh noise: a field with
    a clear peak in every cell, and different from pair to pair.  patch (y0, y1, x0, x1) moves the other way: the outliers"""
    rng = np.random.default_rng(seed)
    m = 24
    base = rng.integers(30, 226, (h + 2 * m, w + 2 * m)).astype(np.float64)
    base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4.0
    out = []
    for t in range(count):
        u, v = shifts[t % len(shifts)]
        f = base[m - v:m - v + h, m - u:m - u + w].copy()
        if patch:
            y0, y1, x0, x1 = patch
            f[y0:y1, x0:x1] = base[m + v + y0:m + v + y1, m + u + x0:m + u + x1]
        f = f + sigma * rng.standard_normal((h, w))
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return out


class Case:
    """one input of both tiers: the frames, the pushes that compute (1-based), the row padding of the device tier"""

    def __init__(self, w, h, p, frames, compute, pad=0, sets=None):
        self.w, self.h, self.p, self.frames, self.compute, self.pad = w, h, p, frames, set(compute), pad
        self.sets = sets or {}                                # push -> (min_peak, median_eps, median_thr, vis_max) set before it


def translating(u, v, p, swap=False):
    from ripcurrents_amd import synth
    clip = synth.translating_clip(160, 120, 2, u, v)
    frames = [clip[1], clip[0]] if swap else [clip[0], clip[1]]
    return Case(160, 120, p, frames, {2})


# the translating clips: the shift, and the bounds on the largest error in x and y: 1.5 times what this statement measures
# (0.2214 / 0.2089 px and 0.0715 / 0.1182 px), the margin for the rounding of the stored floats and nothing else
RECOVERY = {"translating": ((1.25, -0.75), (1.5 * 0.2214, 1.5 * 0.2089)), "translating-far": ((5.25, -3.75), (1.5 * 0.0715, 1.5 * 0.1182))}


def cpp_case(count=12):
    """the input tests/cpp/test_piv.cpp makes for itself from integers: a pattern that moves two pixels right and one down per
    frame, every third push computes"""
    w, h = 70, 50
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    frames = []
    for t in range(count):
        xs, ys = x - 2 * t + 64, y - t + 64
        frames.append((((xs * xs * 7 + ys * ys * 13 + xs * ys * 3) % 251 + (x * y + t) % 5) % 256).astype(np.uint8))
    p = Params(16, 4, 10, ensemble=3, flags=REPLACE, min_peak=0.25, median_eps=0.125, median_thr=2.0, vis_max=4.0)
    return Case(w, h, p, frames, {t + 1 for t in range(count) if t % 3 == 2})


def cases():
    """name -> Case.  75 x 61 is ragged against dwords and has cells that overlap (step 5 under a window of 8); 100 x 84 with an
    ensemble of 3 over 7 pushes wraps its ring twice; 96 x 96 is one cell of the largest window and range, the frame exactly
    one search area, first all 255 (the largest sums there are, and FLAT), then 0 / 255 at random; the translating clips are
    the recovery cases of tests/test_piv_ref.py"""
    c = {}
    sh = [(0, 0), (2, 0), (2, 1), (1, -1)]                    # pairs that moved by (2, 0): the edge of the range; (0, 1); (-1, -2)
    c["ragged"] = Case(75, 61, Params(8, 2, 5, 1, REPLACE, 0.25, 0.1, 2.0, 2.0), drifting_frames(75, 61, 4, 21, sh, patch=(20, 42, 30, 52)),
                       {1, 2, 3, 4}, pad=5)
    sh = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 1), (6, 1)]
    c["ring"] = Case(100, 84, Params(16, 4, 16, 3, 0, 0.25, 0.1, 2.0, 3.0), drifting_frames(100, 84, 7, 22, sh, patch=(30, 60, 40, 70)),
                     {1, 2, 4, 7}, pad=3, sets={7: (0.5, 0.2, 1.0, 2.0)})
    c["extreme"] = Case(96, 96, Params(64, 16, 64, 4, 0, 0.25, 0.1, 2.0, 4.0),
                        [np.full((96, 96), 255, np.uint8)] * 3 + binary_frames(96, 96, 5, 23), {2, 3, 4, 8})
    c["noise"] = Case(75, 61, Params(12, 3, 7, 2, 0, 0.25, 0.1, 2.0, 4.0), noise_frames(75, 61, 4, 24), {3, 4}, pad=1)
    c["translating"] = translating(1.25, -0.75, Params(16, 4, 16, 1, 0, 0.25, 0.1, 2.0, 4.0))
    c["translating-far"] = translating(5.25, -3.75, Params(32, 8, 32, 1, 0, 0.25, 0.1, 2.0, 8.0))
    c["cpp"] = cpp_case()
    return c


def run_case(case, lut=None):
    """the statement's outputs of every computing push of a case, in order: (the session, [(push, outputs, parameters then)])"""
    ref = PivRef(case.w, case.h, Params(**case.p.kw()), lut)
    out = []
    for t, f in enumerate(case.frames, 1):
        if t in case.sets:
            ref.p.min_peak, ref.p.median_eps, ref.p.median_thr, ref.p.vis_max = case.sets[t]
        r = ref.push(f, compute=t in case.compute)
        if r is not None:
            out.append((t, r, Params(**ref.p.kw())))
    return ref, out
