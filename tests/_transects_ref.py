"""The transects (include/rcflow.h, "transects") stated in numpy: the geometry, the sampling of the grey frame and of the field
on 1/16-pixel positions, the rings, the correlation sums of every grey row with the one `lag` pushes later (kept in step by
adding the pair that comes in and taking off the one that goes out, and also by a rescan), the velocity along the line, the
window means, the exact Q sums, the jets, the records, the summary and the two pictures.  Integers are Python / int64 and exact;
floats are float32 operation by operation, doubles float64 operation by operation, in the order the header gives."""
import math
from dataclasses import asdict, dataclass

import numpy as np

GRAY, FLOW = 1, 2
EMPTY, FLAT, EDGE = 1, 2, 4
MAX_LINES, MAX_SAMPLES, MAX_TOTAL, MAX_WINDOW, MAX_LAG, MAX_RANGE, NSUMS = 64, 1024, 65536, 4096, 8, 16, 16
BADQ = -(1 << 63)
f32 = np.float32

RECORD = np.dtype([("flags", "<i4"), ("pairs", "<i4"), ("peak_shift", "<i4"), ("v_along", "<f4"), ("corr_peak", "<f4"), ("mean_along", "<f4"),
                   ("mean_cross", "<f4"), ("flux_out", "<f4"), ("flux_in", "<f4"), ("jets", "<i4"), ("jet_start", "<i4"), ("jet_len", "<i4"),
                   ("jet_flux", "<f4"), ("jet_peak", "<f4"), ("jet_peak_at", "<i4"), ("bad", "<i4")])
SAMPLE = np.dtype([("X", "<i4"), ("Y", "<i4"), ("line", "<i4"), ("offset", "<i4")])
GEOM = np.dtype([("first", "<i4"), ("n", "<i4"), ("ex", "<f4"), ("ey", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("scale", "<f4"), ("pad", "<i4"),
                 ("len", "<f8"), ("ds", "<f8")])
FLOATS = ("v_along", "corr_peak", "mean_along", "mean_cross", "flux_out", "flux_in", "jet_flux", "jet_peak")
INTS = ("flags", "pairs", "peak_shift", "jets", "jet_start", "jet_len", "jet_peak_at", "bad")


@dataclass
class Params:
    window: int = 32
    sources: int = GRAY | FLOW
    lag: int = 1
    range: int = 0
    fps: float = 1.0
    metres_per_pixel: float = 1.0
    jet_min: float = 0.25
    vis_max: float = 2.0

    def kw(self):
        """the keywords of Context.transects_open"""
        d = asdict(self)
        src = d.pop("sources")
        d["gray"], d["flow"] = bool(src & GRAY), bool(src & FLOW)
        return d


def plan(w, h, lines, metres_per_pixel=1.0, fps=1.0):
    """-> (table SAMPLE[S], geom GEOM[L]); ValueError where rcflow_transects_plan answers RC_EINVAL"""
    if not (w > 0 and h > 0 and 1 <= len(lines) <= MAX_LINES and 0 < metres_per_pixel < math.inf and 0 < fps < math.inf):
        raise ValueError("picture, line count, fps or metres_per_pixel")
    if any(not 2 <= int(l[4]) <= MAX_SAMPLES for l in lines) or sum(int(l[4]) for l in lines) > MAX_TOTAL:
        raise ValueError("samples")
    S = sum(int(l[4]) for l in lines)
    table, geom = np.zeros(S, SAMPLE), np.zeros(len(lines), GEOM)
    first = 0
    for i, l in enumerate(lines):
        x0, y0, x1, y1 = (float(f32(v)) for v in l[:4])
        n = int(l[4])
        if not all(math.isfinite(v) for v in (x0, y0, x1, y1)):
            raise ValueError("endpoint")
        dx, dy = x1 - x0, y1 - y0
        ln = math.hypot(dx, dy)
        if not (ln > 0 and math.isfinite(ln)):
            raise ValueError("length")
        t = np.arange(n, dtype=np.float64) / np.float64(n - 1)
        X, Y = np.rint(16.0 * (x0 + dx * t)), np.rint(16.0 * (y0 + dy * t))
        if not ((X >= 0) & (X <= 16 * (w - 1)) & (Y >= 0) & (Y <= 16 * (h - 1))).all():
            raise ValueError("sample outside the picture")
        rows = table[first:first + n]
        rows["X"], rows["Y"], rows["line"], rows["offset"] = X.astype(np.int32), Y.astype(np.int32), i, np.arange(n)
        geom[i] = (first, n, f32(dx / ln), f32(dy / ln), f32(dy / ln), f32(-dx / ln), f32(metres_per_pixel * fps), 0, ln,
                   (ln * metres_per_pixel) / float(n - 1))
        first += n
    return table, geom


def open_error(w, h, lines, p):
    """what rcflow_transects_open refuses before it looks at the context: None, or the reason"""
    pos = lambda v: 0 < v < math.inf
    if not (2 <= p.window <= MAX_WINDOW and 1 <= p.sources <= 3 and 1 <= p.lag <= MAX_LAG and 0 <= p.range <= MAX_RANGE and pos(p.fps) and
            pos(p.metres_per_pixel) and 0 < p.jet_min < 2.0 ** 20 and pos(p.vis_max)):
        return "parameters"
    if p.range >= 1 and (not p.sources & GRAY or p.window <= p.lag):
        return "range"
    try:
        plan(w, h, lines, p.metres_per_pixel, p.fps)
    except ValueError as e:
        return str(e)
    if p.range >= 1 and any(int(l[4]) < 2 * p.range + 8 for l in lines):
        return "short line"
    return None


def Q(x):
    return int(np.rint(np.float64(x) * 65536.0))


def pair_sums(A, B, D):
    """one pair's sums of one line -> ((2 D + 1) x 3 int64: Tab, Tb, Tbb; (Ta, Taa))"""
    n = A.size
    a = A[D:n - D].astype(np.int64)
    out = np.zeros((2 * D + 1, 3), np.int64)
    for k, d in enumerate(range(-D, D + 1)):
        b = B[D + d:n - D + d].astype(np.int64)
        out[k] = (int((a * b).sum()), int(b.sum()), int((b * b).sum()))
    return out, np.array([a.sum(), (a * a).sum()], np.int64)


class TransectsRef:
    def __init__(self, w, h, lines, p, jet_lut=None):
        assert open_error(w, h, lines, p) is None
        self.w, self.h, self.p, self.lut = w, h, p, jet_lut
        self.table, self.geom = plan(w, h, lines, p.metres_per_pixel, p.fps)
        self.L, self.S = len(lines), len(self.table)
        self.reset()

    def reset(self):
        D = self.p.range
        self.rows_g, self.rows_f = [], []          # the held rows, oldest first
        self.pushes = 0
        self.T = np.zeros((self.L, 2 * D + 1, 3), np.int64)
        self.Ta = np.zeros((self.L, 2), np.int64)

    # ---- sampling
    def _corners(self):
        X, Y = self.table["X"].astype(np.int64), self.table["Y"].astype(np.int64)
        ix, fx, iy, fy = X >> 4, X & 15, Y >> 4, Y & 15
        return ix, fx, np.minimum(ix + 1, self.w - 1), iy, fy, np.minimum(iy + 1, self.h - 1)

    def sample_gray(self, gray):
        ix, fx, ix1, iy, fy, iy1 = self._corners()
        g = gray.astype(np.int64)
        v = (16 - fx) * (16 - fy) * g[iy, ix] + fx * (16 - fy) * g[iy, ix1] + (16 - fx) * fy * g[iy1, ix] + fx * fy * g[iy1, ix1] + 128
        return (v >> 8).astype(np.uint8)

    def sample_flow(self, flow):
        ix, fx, ix1, iy, fy, iy1 = self._corners()
        a, b = fx.astype(f32) / f32(16), fy.astype(f32) / f32(16)
        line = self.table["line"]
        out = np.zeros((self.S, 2), f32)
        with np.errstate(all="ignore"):
            val = []
            for c in range(2):
                f = flow[..., c].astype(f32)
                p00, p10, p01, p11 = f[iy, ix], f[iy, ix1], f[iy1, ix], f[iy1, ix1]
                top = p00 + a * (p10 - p00)
                bot = p01 + a * (p11 - p01)
                val.append(top + b * (bot - top))
            u, v = val
            gm = self.geom[line]
            out[:, 0] = (u * gm["ex"] + v * gm["ey"]) * gm["scale"]
            out[:, 1] = (u * gm["nx"] + v * gm["ny"]) * gm["scale"]
        return out

    # ---- the accumulators
    def pairs(self):
        return max(0, min(self.pushes, self.p.window) - self.p.lag) if self.p.range >= 1 else 0

    def rescan(self):
        """the accumulators from the held rows alone"""
        D, lag = self.p.range, self.p.lag
        T, Ta = np.zeros_like(self.T), np.zeros_like(self.Ta)
        if D >= 1:
            for r in range(len(self.rows_g) - lag):
                for i, gm in enumerate(self.geom):
                    sl = slice(gm["first"], gm["first"] + gm["n"])
                    t, ta = pair_sums(self.rows_g[r][sl], self.rows_g[r + lag][sl], D)
                    T[i] += t
                    Ta[i] += ta
        return T, Ta

    def _pair(self, A, B, sign):
        for i, gm in enumerate(self.geom):
            sl = slice(gm["first"], gm["first"] + gm["n"])
            t, ta = pair_sums(A[sl], B[sl], self.p.range)
            self.T[i] += sign * t
            self.Ta[i] += sign * ta

    def push(self, gray=None, flow=None, compute=True):
        p = self.p
        assert (gray is not None) == bool(p.sources & GRAY) and (flow is not None) == bool(p.sources & FLOW)
        if gray is not None:
            row = self.sample_gray(gray)
            if p.range >= 1:
                if len(self.rows_g) == p.window:                   # the pair whose older row goes
                    self._pair(self.rows_g[0], self.rows_g[p.lag], -1)
                if len(self.rows_g) >= p.lag:
                    self._pair(self.rows_g[-p.lag], row, 1)
            self.rows_g = (self.rows_g + [row])[-p.window:]
        if flow is not None:
            self.rows_f = (self.rows_f + [self.sample_flow(flow)])[-p.window:]
        self.pushes += 1
        return self.outputs() if compute else None

    # ---- the outputs of a computing push
    def velocity(self, i):
        """-> (flags, peak_shift, v_along, corr_peak, (N, num, va, vb, q))"""
        p, D, pairs = self.p, self.p.range, self.pairs()
        n = int(self.geom[i]["n"])
        N = pairs * (n - 2 * D)
        if pairs == 0:
            return EMPTY, 0, f32(0), f32(0), (N, 0, 0, 0, 0)
        Ta, Taa = int(self.Ta[i, 0]), int(self.Ta[i, 1])
        va = N * Taa - Ta * Ta
        s, nums, vbs = [], [], []
        for k in range(2 * D + 1):
            Tab, Tb, Tbb = (int(v) for v in self.T[i, k])
            num, vb = N * Tab - Ta * Tb, N * Tbb - Tb * Tb
            nums.append(num)
            vbs.append(vb)
            nd = float(num)
            s.append((nd * abs(nd)) / (float(va) * float(vb)) if va > 0 and vb > 0 else 0.0)
        if not any(s):
            return FLAT, 0, f32(0), f32(0), (N, 0, 0, 0, 0)
        q = int(np.argmax(s))                                     # the first largest
        root = lambda v: math.copysign(math.sqrt(abs(v)), v)
        rq, delta, flags = root(s[q]), 0.0, 0
        if 0 < q < 2 * D:
            rl, rr = root(s[q - 1]), root(s[q + 1])
            den = (rl - 2.0 * rq) + rr
            if den < 0:
                delta = (0.5 * (rl - rr)) / den
        else:
            flags = EDGE
        v = ((((q - D) + delta) * float(self.geom[i]["ds"])) * p.fps) / float(p.lag)
        return flags, q - D, f32(v), f32(rq), (N, nums[q], va, vbs[q], q)

    def outputs(self):
        p = self.p
        held = min(self.pushes, p.window)
        rec, sums, profile = np.zeros(self.L, RECORD), np.zeros((self.L, NSUMS), np.int64), np.zeros((self.S, 2), f32)
        qmin = int(np.rint(np.float64(p.jet_min) * 65536.0))
        if self.rows_f:
            with np.errstate(all="ignore"):
                acc = np.zeros((self.S, 2), f32)
                for r in self.rows_f:
                    acc = acc + r
                profile = acc / f32(held)
        with_v = with_jet = jets_all = bad_all = 0
        for i, gm in enumerate(self.geom):
            first, n, ds = int(gm["first"]), int(gm["n"]), float(gm["ds"])
            flags, shift, v, peak, (N, num, va, vb, q) = self.velocity(i)
            Fpos = Fneg = Ft = nv = bad = 0
            qs = [BADQ] * n
            if self.rows_f:
                for j in range(n):
                    mt, mn = profile[first + j]
                    if abs(mt) < 1048576.0 and abs(mn) < 1048576.0:
                        qs[j] = Q(mn)
                        Fpos, Fneg, Ft, nv = Fpos + max(qs[j], 0), Fneg + min(qs[j], 0), Ft + Q(mt), nv + 1
                    else:
                        bad += 1
            jets, best = 0, (0, 0, 0, 0, 0)                       # start, length, sum, peak, peak_at
            j = 0
            while j < n:
                if qs[j] != BADQ and qs[j] >= qmin:
                    k = j
                    while k < n and qs[k] != BADQ and qs[k] >= qmin:
                        k += 1
                    run = qs[j:k]
                    if jets == 0 or sum(run) > best[2]:
                        best = (j, k - j, sum(run), max(run), j + run.index(max(run)))
                    jets += 1
                    j = k
                else:
                    j += 1
            sums[i] = (Fpos, Fneg, Ft, nv, bad, jets) + best + (N, num, va, vb, q)
            r = rec[i]
            r["flags"], r["pairs"], r["peak_shift"], r["v_along"], r["corr_peak"] = flags, self.pairs(), shift, v, peak
            if nv:
                r["mean_along"], r["mean_cross"] = f32((Ft / 65536.0) / nv), f32(((Fpos + Fneg) / 65536.0) / nv)
            r["flux_out"], r["flux_in"], r["jet_flux"] = f32((Fpos / 65536.0) * ds), f32((Fneg / 65536.0) * ds), f32((best[2] / 65536.0) * ds)
            r["jets"], r["jet_start"], r["jet_len"], r["jet_peak"], r["jet_peak_at"], r["bad"] = jets, best[0], best[1], f32(best[3] / 65536.0), best[4], bad
            with_v += not flags & (EMPTY | FLAT)
            with_jet += jets > 0
            jets_all += jets
            bad_all += bad
        out = dict(records=rec, sums=sums, profile=profile,
                   summary=np.array([held, self.pairs(), with_v, with_jet, jets_all, bad_all, self.pushes, 0], np.int64))
        if self.rows_g:
            stack = np.zeros((p.window, self.S), np.uint8)
            stack[:held] = np.stack(self.rows_g)
            out["stack"] = stack
        if self.rows_f and self.lut is not None:
            hov = np.zeros((p.window, self.S, 3), np.uint8)
            with np.errstate(all="ignore"):
                un = np.stack(self.rows_f)[..., 1]
                f = np.rint(un / f32(p.vis_max) * f32(127.5) + f32(127.5))
                idx = np.where(f > 0, np.minimum(f, 255), 0).astype(np.int64)
                lut = np.asarray(self.lut, np.uint8).reshape(256, 3)
                hov[:held] = np.where(np.isfinite(un)[..., None], lut[idx], 0)
            out["hov"] = hov
        return out


# ---------------------------------------------------------------------------- cases for the device tests
@dataclass
class Case:
    w: int
    h: int
    lines: list
    p: Params
    gray: list          # frames or None
    flow: list          # fields or None
    pad: int = 0
    compute: tuple = ()  # the pushes (from 1) at which the sparse session asks for outputs


def _texture(rng, w, h, frames, u, v):
    """a smooth random texture moved by (u, v) whole pixels per frame, with a little noise"""
    big = rng.integers(0, 256, (h + 64, w + 64)).astype(np.float64)
    for _ in range(2):
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) / 4
    big = (big - big.min()) / (big.max() - big.min()) * 255
    out = []
    for t in range(frames):
        f = np.roll(big, (v * t, u * t), (0, 1))[32:32 + h, 32:32 + w] + rng.integers(-3, 4, (h, w))
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return out


def _fields(rng, w, h, frames, spoil=True):
    """random fields; spoil: NaN under the middle of the line from (3, 60.25) to (40.5, 8.125), 1e30 in the last pixel, infinities
    that wander along the last row"""
    out = []
    for t in range(frames):
        f = rng.normal(0, 1, (h, w, 2)).astype(f32) + f32(0.5)
        if spoil:
            f[32, 23, 0] = np.nan
            f[h - 1, w - 1, 1] = 1e30
            f[h - 1, 40 + t % 3] = (np.inf, -np.inf)
        out.append(f)
    return out


def cases():
    rng = np.random.default_rng(20260131)
    c = {}
    # three lines of unequal length, S odd (16 + 37 + 50 = 103): n = 2 D + 8, an n that is no multiple of 4, fractional positions,
    # samples on the last column and the last row; T = 5, lag 2; 13 pushes > 2 T; rows padded; NaN, infinities and 1e30 in the field
    w, h = 96, 64
    lines = [(3.0, 60.25, 40.5, 8.125, 16), (95.0, 2.0, 95.0, 63.0, 37), (2.5, 63.0, 93.0, 63.0, 50)]
    c["three"] = Case(w, h, lines, Params(window=5, lag=2, range=4, fps=25.0, metres_per_pixel=0.5, jet_min=3.0, vis_max=20.0),
                      _texture(rng, w, h, 13, 2, 0), _fields(rng, w, h, 13), pad=5, compute=(1, 2, 3, 6, 11, 13))
    # one line of 1024 samples at fractional positions, D = 16, T = lag + 1 (one pair), GRAY alone
    w, h = 1100, 12
    c["long"] = Case(w, h, [(1.0, 3.3, 1098.7, 8.6, 1024)], Params(window=2, sources=GRAY, lag=1, range=16), _texture(rng, w, h, 5, 3, 0), None,
                     compute=(2, 5))
    # FLOW alone, no correlation; the window wraps
    w, h = 64, 48
    c["flow"] = Case(w, h, [(1.0, 1.0, 62.0, 46.0, 33), (60.0, 5.0, 4.0, 5.0, 29)], Params(window=4, sources=FLOW, jet_min=0.5, vis_max=1.5), None,
                     _fields(rng, w, h, 9, spoil=False), pad=3, compute=(1, 4, 9))
    # GRAY and a correlation on a flat frame
    flat = [np.full((h, w), 77, np.uint8)] * 4
    c["flat"] = Case(w, h, [(2.0, 20.0, 61.0, 20.0, 60)], Params(window=3, sources=GRAY, lag=1, range=3), flat, None, compute=(1, 2, 4))
    # lag 8 and the largest window a few pushes can fill; both sources, D = 0 on a GRAY session
    c["nocorr"] = Case(w, h, [(0.0, 0.0, 63.0, 47.0, 41)], Params(window=3, lag=8, range=0, vis_max=1.0), _texture(rng, w, h, 4, 1, 1),
                       _fields(rng, w, h, 4, spoil=False), compute=(2, 4))
    return c


def run_case(case, jet_lut):
    """-> (the session after the last push, [outputs of every push])"""
    ref = TransectsRef(case.w, case.h, case.lines, case.p, jet_lut)
    n = len(case.gray or case.flow)
    outs = [ref.push(case.gray[t] if case.gray else None, case.flow[t] if case.flow else None) for t in range(n)]
    return ref, outs
