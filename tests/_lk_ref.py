"""Sparse pyramidal Lucas-Kanade restated in numpy, the slow obvious way, with order-free window sums.

cv::calcOpticalFlowPyrLK on 8UC1 images as OpenCV 4.1.0 computes it (video/src/lkpyramid.cpp: buildOpticalFlowPyramid,
calcSharrDeriv, LKTrackerInvoker, SparsePyrLKOpticalFlowImpl::calc; imgproc pyrDown), written out from the published
algorithm as remembered: there is no OpenCV build here to pin it against.  One thing differs from upstream on purpose:
the window sums (the three covariance sums, the two mismatch sums, the residual) are exact integers converted to float
once, where upstream's scalar path adds floats in raster order.  That is the form the device kernel computes and the
form oracle.pyrlk(exact_sums=True) computes, so all three can be compared bit for bit.

Everything up to the sums is integer arithmetic in int64 numpy (pyramid, Scharr derivatives, the 14-bit bilinear
weights applied to the patch and its derivatives); the 2 x 2 solve and the termination tests are np.float32 / float64
scalars exactly where the algorithm has float / double.  One point at a time, the window vectorised.

Also here, because no conftest may be added: the point classes and scenes the CPU tier (tests/test_lk_ref.py) and the
device tier (tests/test_gpu_lk.py) share.
"""
import math

import numpy as np

f32 = np.float32
INT_MIN = -2147483648
W_BITS = 14
USE_INITIAL_FLOW, GET_MIN_EIGENVALS = 4, 8
COUNT, EPS = 1, 2
FLT_EPSILON = f32(1.1920928955078125e-07)
FLT_SCALE = f32(1.0 / (1 << 20))


# ---------------------------------------------------------------------------- integer stages
def reflect101(p, n):
    """BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) for any distance: the triangle wave of period 2 (n - 1)."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p >= n, period - p, p)


def pyr_down(img):
    """imgproc pyrDown on 8U: (1 4 6 4 1) x (1 4 6 4 1) / 256 rounded, every second pixel, REFLECT_101."""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    k = (1, 4, 6, 4, 1)
    xs, ys = 2 * np.arange((w + 1) // 2), 2 * np.arange((h + 1) // 2)
    t = sum(k[j] * a[:, reflect101(xs - 2 + j, w)] for j in range(5))
    t = sum(k[j] * t[reflect101(ys - 2 + j, h), :] for j in range(5))
    return (t + 128) >> 8


def scharr(img):
    """calcSharrDeriv: (dx, dy) with the 3-10-3 smoothing across and the central difference along, REFLECT_101."""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    up, dn = a[reflect101(np.arange(h) - 1, h)], a[reflect101(np.arange(h) + 1, h)]
    smooth, diff = (up + dn) * 3 + a * 10, dn - up
    lf, rt = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    dx = smooth[:, rt] - smooth[:, lf]
    dy = (diff[:, rt] + diff[:, lf]) * 3 + diff * 10
    return np.stack([dx, dy], axis=-1)


def levels(w, h, win, max_level):
    """buildOpticalFlowPyramid's early return: the last level whose successor would still exceed the window."""
    for level in range(max_level + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win[0] or h <= win[1]:
            return level
    return max_level


def pyramid(img, win, max_level):
    out = [np.asarray(img).astype(np.int64)]
    for _ in range(levels(out[0].shape[1], out[0].shape[0], win, max_level)):
        out.append(pyr_down(out[-1]))
    return out


# ---------------------------------------------------------------------------- the tracker
def cv_floor(v):
    """cvFloor of a float on x86: NaN, infinities and anything beyond int32 convert to INT_MIN."""
    v = float(v)
    if not math.isfinite(v) or v >= 2147483648.0 or v < -2147483648.0:
        return INT_MIN
    return int(math.floor(v))


def _weights(a, b):
    """The four 14-bit bilinear weights of the fractional position (a, b); cvRound is half to even."""
    one = f32(1)
    scale = f32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * scale))
    w01 = int(np.rint(a * (one - b) * scale))
    w10 = int(np.rint((one - a) * b * scale))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _bilinear(g, wts, shift):
    """g is (win_h + 1, win_w + 1[, c]) of integers; the weighted 2 x 2 sum, rounded and shifted."""
    w00, w01, w10, w11 = wts
    return (g[:-1, :-1] * w00 + g[:-1, 1:] * w01 + g[1:, :-1] * w10 + g[1:, 1:] * w11 + (1 << (shift - 1))) >> shift


def _image_patch(img, ix, iy, win, wts):
    """Patch of the 8-bit level with its corner at (ix, iy), in 1/32 grey levels; outside reads reflect."""
    h, w = img.shape
    ys, xs = reflect101(iy + np.arange(win[1] + 1), h), reflect101(ix + np.arange(win[0] + 1), w)
    return _bilinear(img[ys[:, None], xs[None, :]], wts, W_BITS - 5)


def _deriv_patch(der, ix, iy, win, wts):
    """Patch of the derivative image; outside reads are zero (the pyramid pads it with BORDER_CONSTANT)."""
    h, w = der.shape[:2]
    ys, xs = iy + np.arange(win[1] + 1), ix + np.arange(win[0] + 1)
    g = np.zeros((win[1] + 1, win[0] + 1, 2), np.int64)
    yv, xv = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    if yv.any() and xv.any():
        g[np.ix_(yv, xv)] = der[np.ix_(ys[yv], xs[xv])]
    return _bilinear(g, wts, W_BITS)


def _outside(ix, iy, win, w, h):
    return ix < -win[0] or ix >= w or iy < -win[1] or iy >= h


def clamp_criteria(crit_type, max_count, epsilon):
    """SparsePyrLKOpticalFlowImpl::calc: an absent criterion gets its default, a present one is clamped."""
    max_count = 30 if (crit_type & COUNT) == 0 else min(max(int(max_count), 0), 100)
    epsilon = 0.01 if (crit_type & EPS) == 0 else min(max(float(epsilon), 0.0), 10.0)
    return max_count, epsilon * epsilon


def track_point(P, D, N, p, guess, win, max_count, eps2, flags, min_eig_threshold, with_err):
    """One point through every level.  P, N: pyramids of the two images, D: derivatives of P's levels."""
    halfx, halfy = f32(win[0] - 1) * f32(0.5), f32(win[1] - 1) * f32(0.5)
    n_win = win[0] * win[1]
    top = len(P) - 1
    status, err = 1, f32(0)
    qx, qy = f32(guess[0]), f32(guess[1])
    for level in range(top, -1, -1):
        I, J, dI = P[level], N[level], D[level]
        h, w = I.shape
        sc = f32(1.0 / (1 << level))
        px, py = f32(p[0]) * sc, f32(p[1]) * sc
        if level == top:
            nx, ny = (qx * sc, qy * sc) if flags & USE_INITIAL_FLOW else (px, py)
        else:
            nx, ny = qx * f32(2), qy * f32(2)
        qx, qy = nx, ny
        px, py = px - halfx, py - halfy
        ipx, ipy = cv_floor(px), cv_floor(py)
        if _outside(ipx, ipy, win, w, h):
            if level == 0:
                status, err = 0, f32(0)
            continue
        wts = _weights(px - f32(ipx), py - f32(ipy))
        Ip = _image_patch(I, ipx, ipy, win, wts)
        dIp = _deriv_patch(dI, ipx, ipy, win, wts)
        ix, iy = dIp[..., 0], dIp[..., 1]
        A11 = f32(int((ix * ix).sum())) * FLT_SCALE
        A12 = f32(int((ix * iy).sum())) * FLT_SCALE
        A22 = f32(int((iy * iy).sum())) * FLT_SCALE
        det = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + f32(4) * A12 * A12)) / f32(2 * n_win)
        if with_err and flags & GET_MIN_EIGENVALS:
            err = min_eig
        if float(min_eig) < min_eig_threshold or det < FLT_EPSILON:
            if level == 0:
                status = 0
            continue
        det = f32(1) / det
        nx, ny = nx - halfx, ny - halfy
        pdx, pdy = f32(0), f32(0)
        for j in range(max_count):
            inx, iny = cv_floor(nx), cv_floor(ny)
            if _outside(inx, iny, win, w, h):
                if level == 0:
                    status = 0
                break
            diff = _image_patch(J, inx, iny, win, _weights(nx - f32(inx), ny - f32(iny))) - Ip
            b1 = f32(int((diff * ix).sum())) * FLT_SCALE
            b2 = f32(int((diff * iy).sum())) * FLT_SCALE
            dx, dy = (A12 * b2 - A22 * b1) * det, (A12 * b1 - A11 * b2) * det
            nx, ny = nx + dx, ny + dy
            qx, qy = nx + halfx, ny + halfy
            if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                break
            if j > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                qx, qy = qx - dx * f32(0.5), qy - dy * f32(0.5)
                break
            pdx, pdy = dx, dy
        if status and with_err and level == 0 and not flags & GET_MIN_EIGENVALS:
            fx, fy = qx - halfx, qy - halfy
            inx, iny = cv_floor(fx), cv_floor(fy)
            if _outside(inx, iny, win, w, h):
                status = 0
                continue
            diff = _image_patch(J, inx, iny, win, _weights(fx - f32(inx), fy - f32(iny))) - Ip
            err = f32(int(np.abs(diff).sum())) * f32(1) / f32(32 * n_win)
    return (qx, qy), status, err


def pyrlk(prev, nxt, prev_pts, next_pts=None, win=(21, 21), max_level=3, crit_type=COUNT | EPS, max_count=30,
          epsilon=0.01, flags=0, min_eig_threshold=1e-4, with_err=True):
    """Returns (next_pts float32 n x 2, status uint8 n, err float32 n or None), like oracle.pyrlk."""
    pts = np.asarray(prev_pts, np.float32).reshape(-1, 2)
    n = len(pts)
    guess = np.zeros((n, 2), np.float32) if next_pts is None else np.asarray(next_pts, np.float32).reshape(-1, 2)
    max_count, eps2 = clamp_criteria(crit_type, max_count, epsilon)
    P, N = pyramid(prev, win, max_level), pyramid(nxt, win, max_level)
    D = [scharr(a) for a in P]
    q, st, er = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            q[i], st[i], er[i] = track_point(P, D, N, pts[i], guess[i], win, max_count, eps2, flags,
                                             min_eig_threshold, with_err)
    return q, st, (er if with_err else None)


# ---------------------------------------------------------------------------- shared inputs of both tiers
# tests/golden/pyrlk_exact_160x120.npz: (tag, window, epsilon, flags); three window shapes, two criteria
GOLDEN_CASES = tuple(("%dx%d_%s" % (win[0], win[1], name), win, eps, flags)
                     for win in ((5, 9), (21, 21), (31, 15)) for name, eps, flags in (("fine", 0.01, 4), ("coarse", 0.1, 8)))


def transpose_case(prev, nxt, pts, guess, win):
    """The same problem with x and y exchanged."""
    sw = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32)[:, ::-1])
    return np.ascontiguousarray(prev.T), np.ascontiguousarray(nxt.T), sw(pts), sw(guess), (win[1], win[0])


def half_texture_pair(w, h, seed=5, shift=(1.25, -0.75)):
    """Left half smooth texture moving by `shift`, right half one grey level, with a ramp of fading contrast
    between them: the minimum eigenvalue runs from large to exactly zero across the frame."""
    rng = np.random.RandomState(seed)
    ph = rng.uniform(0, 2 * np.pi, 6)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def tex(x, y):
        return (40 * np.sin(x / 5.0 + ph[0]) * np.cos(y / 7.0 + ph[1]) + 30 * np.sin((x + y) / 11.0 + ph[2])
                + 25 * np.cos(x / 3.1 - y / 4.3 + ph[3]) + 15 * np.sin(x / 2.3 + ph[4]) * np.sin(y / 2.9 + ph[5]))
    fade = np.clip((0.62 * w - x) / (0.25 * w), 0.0, 1.0) ** 2
    out = [np.clip(np.rint(120 + fade * tex(x - dx, y - dy)), 0, 255).astype(np.uint8) for dx, dy in ((0, 0), shift)]
    return out[0], out[1]


def analytic_pair(w, h, shift):
    """A smooth analytic image and the same image translated by a sub-pixel shift (sampled, not interpolated)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def f(x, y):
        return 128 + 45 * np.sin(x / 6.0) * np.cos(y / 8.0) + 35 * np.sin((x + 2 * y) / 17.0) + 25 * np.cos(x / 3.3 - y / 4.1)
    return (np.rint(f(x, y)).astype(np.uint8), np.rint(f(x - shift[0], y - shift[1])).astype(np.uint8))


def leaving_pair(w, h, seed=9, shift=(-9.0, -7.0)):
    """A textured scene moving towards the top-left corner fast enough that points near those borders are
    carried past the bounds test during the iteration."""
    rng = np.random.RandomState(seed)
    big = rng.randint(0, 256, size=(h // 4 + 8, w // 4 + 8)).astype(np.float64)
    big = np.kron(big, np.ones((4, 4)))
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for ax in (0, 1):
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), ax, big)
    sx, sy = int(-shift[0]), int(-shift[1])
    a = big[16:16 + h, 16:16 + w]
    b = big[16 + sy:16 + sy + h, 16 + sx:16 + sx + w]
    return np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8)


def bounds_points(w, h, win, max_level):
    """The first and the last position that pass each of the four bounds tests (floor(p * 2^-l - half) in
    [-win, size_l)), and their neighbours that fail it, at level 0 and at the top level."""
    out = []
    top = levels(w, h, win, max_level)
    for level in sorted({0, top}):
        lw, lh = w, h
        for _ in range(level):
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
        s = float(1 << level)
        for axis, (size, wn, mid) in enumerate(((lw, win[0], h / 2.0), (lh, win[1], w / 2.0))):
            half = (wn - 1) * 0.5
            lo, hi = f32((half - wn) * s), f32((size + half) * s)      # first passing / first failing
            for v in (lo, np.nextafter(lo, f32(-np.inf)), np.nextafter(lo, f32(np.inf)), hi,
                      np.nextafter(hi, f32(-np.inf)), np.nextafter(hi, f32(np.inf))):
                out.append((v, mid + 0.25) if axis == 0 else (mid + 0.25, v))
    return np.array(out, np.float32)


def point_classes(w, h, win, max_level, n_random=24, seed=1):
    """Integer and half-integer coordinates, fractions of 1/16384 either side of 0 and 1, the bounds cases,
    windows over every edge and corner, and the unusable coordinates (NaN, infinite, beyond int32)."""
    rng = np.random.RandomState(seed)
    pts = [(x, y) for x in (0.0, 3.0, w // 2, w - 1.0) for y in (0.0, 2.0, h // 2, h - 1.0)]
    pts += [(x + 0.5, y + 0.5) for x in (1.0, w // 3, w - 2.0) for y in (1.0, h // 3, h - 2.0)]
    pts += [(w // 2 + 0.5, h // 3), (w // 3, h // 2 + 0.5), (w // 2 + 1.5, h // 2 + 2.5)]
    u = 1.0 / 16384
    for base in (0.0, 0.5):                    # win - 1 even: fraction = point's; odd: shifted by a half
        for k in (-2, -1, -0.5, -0.25, 0.25, 0.5, 1, 1.5, 2, 3):
            pts += [(w // 2 + base + k * u, h // 2 + base), (w // 3 + base, h // 3 + base + k * u),
                    (w // 4 + base + k * u, h // 4 + base - k * u)]
    pts = np.array(pts, np.float64)
    rnd = np.stack([rng.uniform(-2, w + 2, n_random), rng.uniform(-2, h + 2, n_random)], axis=1)
    bad = [(np.nan, 5.0), (6.0, np.nan), (np.inf, 1.0), (-np.inf, -np.inf), (3e38, 3e38), (-3e38, 10.0),
           (2147483648.0, 5.0), (5.0, -2147483904.0), (-300.0, 10.0), (w / 2.0, h + 400.0)]
    return np.concatenate([pts, rnd, bounds_points(w, h, win, max_level), np.array(bad)]).astype(np.float32)


def guesses(pts, w, h, seed=2):
    """Initial estimates for OPTFLOW_USE_INITIAL_FLOW: near the point, far from it, outside the image, unusable."""
    rng = np.random.RandomState(seed)
    with np.errstate(all="ignore"):
        g = (pts.astype(np.float64) + rng.uniform(-2, 2, pts.shape)).astype(np.float32)
    g[0] = (-1000.0, 10.0)
    g[1] = (w + 500.0, h + 500.0)
    g[2] = (np.nan, 3.0)
    g[3] = (w / 2.0, -np.inf)
    g[4] = (-12.0, -12.0)
    g[5] = (w + 9.5, h / 2.0)
    return g


def mismatch(got, ref, flags):
    """Compares (next_pts, status, err) triples bit for bit; err only where upstream defines it (status 1, or
    GET_MIN_EIGENVALS).  Returns '' when they agree, otherwise a description with the counts."""
    q, st, er = got
    rq, rst, rer = ref
    bad_st = st != rst
    bad_q = ~((q == rq) | (np.isnan(q) & np.isnan(rq))).all(axis=1)
    bad_er = np.zeros(len(st), bool)
    if er is not None and rer is not None:
        defined = np.ones(len(st), bool) if flags & GET_MIN_EIGENVALS else rst == 1
        bad_er = defined & ~((er == rer) | (np.isnan(er) & np.isnan(rer)))
    if not (bad_st.any() or bad_q.any() or bad_er.any()):
        return ""
    both = bad_q & ~bad_st & np.isfinite(q).all(axis=1) & np.isfinite(rq).all(axis=1)
    worst = float(np.abs(q[both].astype(np.float64) - rq[both]).max()) if both.any() else 0.0
    first = int(np.flatnonzero(bad_st | bad_q | bad_er)[0])
    return ("%d of %d points differ: status %d, position %d (max %.3g px), err %d; first at index %d: got %r %r, "
            "expected %r %r" % (int((bad_st | bad_q | bad_er).sum()), len(st), int(bad_st.sum()), int(bad_q.sum()), worst,
                                int(bad_er.sum()), first, q[first].tolist(), int(st[first]), rq[first].tolist(),
                                int(rst[first])))
