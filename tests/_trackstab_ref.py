"""numpy statement of the corner cells and the robust motion fit, written from the contract in include/rcflow.h
(corner_kernels.hip, fit_kernels.hip are held to it).  Integers are exact; every fp64 operation is written in the order
the header gives, one rounding each."""
import math

import numpy as np

M32 = 0xffffffff
MODELS = {"translation": 1, "similarity": 2, "affine": 3, "homography": 4}
NEED = {1: 3, 2: 4, 3: 6, 4: 8}          # max(2 k, k + 2)
f64 = np.float64


# ---------------------------------------------------------------------------- gray and corner cells
def bgr_to_gray(img):
    """COLOR_BGR2GRAY in 14-bit fixed point (rc_pix3.h)."""
    i = img.astype(np.int64)
    return ((i[..., 0] * 1868 + i[..., 1] * 9617 + i[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def corner_response(gray):
    """R for every pixel at least 2 from the border (0 elsewhere), int64."""
    g = gray.astype(np.int64)
    h, w = g.shape
    dx = np.zeros((h, w), np.int64)
    dy = np.zeros((h, w), np.int64)
    dx[1:-1, 1:-1] = (g[:-2, 2:] + 2 * g[1:-1, 2:] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[1:-1, :-2] + g[2:, :-2])
    dy[1:-1, 1:-1] = (g[2:, :-2] + 2 * g[2:, 1:-1] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[:-2, 1:-1] + g[:-2, 2:])

    def box(a):
        o = np.zeros_like(a)
        for v in (-1, 0, 1):
            for u in (-1, 0, 1):
                o[2:-2, 2:-2] += a[2 + v:h - 2 + v, 2 + u:w - 2 + u]
        return o
    a, b, c = box(dx * dx), box(dx * dy), box(dy * dy)
    D = (a - c) ** 2 + 4 * b * b
    s = np.floor(np.sqrt(D.astype(f64))).astype(np.int64)
    for _ in range(3):                       # the exact ceiling, by comparison
        s = np.where(s * s < D, s + 1, s)
    for _ in range(3):
        s = np.where((s > 0) & ((s - 1) * (s - 1) >= D), s - 1, s)
    assert np.all(s * s >= D) and np.all((s == 0) | ((s - 1) * (s - 1) < D))
    R = a + c - s
    R[:2] = 0; R[-2:] = 0; R[:, :2] = 0; R[:, -2:] = 0
    return R


def isqrt_ceil(D):
    s = math.isqrt(D)
    return s if s * s == D else s + 1


def corner_cells(gray, cells_x, cells_y, margin, min_score):
    """-> (pts [cells, 2] float32, scores [cells] int32) in cell order."""
    h, w = gray.shape
    R = corner_response(gray)
    cw, ch = (w - 2 * margin) // cells_x, (h - 2 * margin) // cells_y
    assert margin >= 2 and cw >= 8 and ch >= 8
    pts = np.zeros((cells_x * cells_y, 2), np.float32)
    scores = np.zeros(cells_x * cells_y, np.int32)
    for cy in range(cells_y):
        y0 = margin + cy * ch
        y1 = h - margin if cy == cells_y - 1 else y0 + ch
        for cx in range(cells_x):
            x0 = margin + cx * cw
            x1 = w - margin if cx == cells_x - 1 else x0 + cw
            blk = R[y0:y1, x0:x1]
            k = int(np.argmax(blk))              # first maximum in row-major order: the lowest (y, x)
            by, bx = divmod(k, x1 - x0)
            best = int(blk[by, bx])
            i = cy * cells_x + cx
            if best == 0 or best < min_score:
                pts[i] = (np.float32(x0 + x1 - 1) * np.float32(0.5), np.float32(y0 + y1 - 1) * np.float32(0.5))
            else:
                pts[i] = (x0 + bx, y0 + by)
                scores[i] = best
    return pts, scores


def default_cells(w, h):
    side = 40
    while True:
        cx, cy = max(1, (w + side // 2) // side), max(1, (h + side // 2) // side)
        if cx * cy <= 4096:
            return cx, cy
        side += 8


# ---------------------------------------------------------------------------- sampler
def mix32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw(seed, j, d):
    return mix32(mix32((seed + 0x9E3779B9 * (j + 1)) & M32) + 0x85EBCA6B * (d + 1))


def sample(seed, j, k, nv):
    """Indices into the valid list, or None for a void hypothesis."""
    if nv < k:
        return None
    got = []
    for d in range(16):
        if len(got) == k:
            break
        idx = (draw(seed, j, d) * nv) >> 32
        if idx not in got:
            got.append(idx)
    return got if len(got) == k else None


# ---------------------------------------------------------------------------- the fit
class Frame:
    def __init__(self, w, h):
        self.S = f64(max(w, h)); self.cx = f64(w) * f64(0.5); self.cy = f64(h) * f64(0.5)
        self.fcx = (f64(w) - 1.0) / 2.0; self.fcy = (f64(h) - 1.0) / 2.0

    def norm(self, v):
        """v [n, 4] float32 -> Px, Py, Qx, Qy, Dx, Dy (float64 arrays)."""
        x, y, z, t = (v[:, i].astype(f64) for i in range(4))
        return ((x - self.cx) / self.S, (y - self.cy) / self.S, (z - self.cx) / self.S, (t - self.cy) / self.S,
                (z - x) / self.S, (t - y) / self.S)


def to_pixels(fr, E, persp):
    E = np.asarray(E, f64).reshape(3, 3)
    F = np.zeros((3, 3), f64)
    for i in range(3):
        F[i, 0] = E[i, 0] / fr.S; F[i, 1] = E[i, 1] / fr.S
        F[i, 2] = E[i, 2] - (E[i, 0] * fr.cx + E[i, 1] * fr.cy) / fr.S
    G = np.zeros((3, 3), f64)
    for j in range(3):
        G[0, j] = fr.S * F[0, j] + fr.cx * F[2, j]
        G[1, j] = fr.S * F[1, j] + fr.cy * F[2, j]
        G[2, j] = F[2, j]
    T = np.eye(3) + G
    ok = bool(np.all(np.isfinite(T)))
    if persp:
        d = T[2, 2]
        ok = ok and bool(d > 0.1)
        with np.errstate(all="ignore"):
            T = T / d
    return T if ok else None


def finish_lin(model, n, mpx, mpy, mdx, mdy, sxx, sxy, syy, xdx, ydx, xdy, ydy):
    b00 = b01 = b10 = b11 = f64(0.)
    if model == 3:
        det = sxx * syy - sxy * sxy
        if not (n >= 3.) or not (det > 1e-12 * (sxx * syy)):
            return None
        b00 = (xdx * syy - ydx * sxy) / det; b01 = (ydx * sxx - xdx * sxy) / det
        b10 = (xdy * syy - ydy * sxy) / det; b11 = (ydy * sxx - xdy * sxy) / det
    elif model == 2:
        if not (n >= 2.) or not (sxx + syy > 0.):
            return None
        sa = (xdx + ydy) / (sxx + syy); sb = (xdy - ydx) / (sxx + syy)
        b00, b01, b10, b11 = sa, -sb, sb, sa
    elif not (n >= 1.):
        return None
    return np.array([b00, b01, mdx - (b00 * mpx + b01 * mpy), b10, b11, mdy - (b10 * mpx + b11 * mpy), 0., 0., 0.], f64)


def ge8(M, tol):
    M = np.array(M, f64)
    for c in range(8):
        col = np.abs(M[c:, c])
        pr = c + int(np.argmax(col))             # first largest
        if not (col[pr - c] >= tol):
            return None
        if pr != c:
            M[[c, pr]] = M[[pr, c]]
        for r in range(c + 1, 8):
            f = M[r, c] / M[c, c]
            M[r, c:] = M[r, c:] - f * M[c, c:]
    z = np.zeros(8, f64)
    for c in range(7, -1, -1):
        s = M[c, 8]
        for k in range(c + 1, 8):
            s = s - M[c, k] * z[k]
        z[c] = s / M[c, c]
    return z


def homography_rows(Px, Py, Qx, Qy, Dx, Dy):
    n = len(Px)
    one, zero = np.ones(n), np.zeros(n)
    r1 = np.stack([Px, Py, one, zero, zero, zero, -Qx * Px, -Qx * Py, Dx], 1)
    r2 = np.stack([zero, zero, zero, Px, Py, one, -Qy * Px, -Qy * Py, Dy], 1)
    return r1, r2


def hypothesis(fr, model, pts, smp):
    """Minimal solve of the sample (indices into pts) -> T or None."""
    Px, Py, Qx, Qy, Dx, Dy = fr.norm(pts[smp])
    if model == 4:
        r1, r2 = homography_rows(Px, Py, Qx, Qy, Dx, Dy)
        M = np.zeros((8, 9), f64)
        M[0::2] = r1; M[1::2] = r2
        z = ge8(M, 1e-9)
        return None if z is None else to_pixels(fr, np.append(z, 0.), True)
    k = len(smp)
    seq = lambda a: np.add.accumulate(np.concatenate([[0.], a]))[-1]      # 0 + a0 + a1 + ... in order
    n = f64(k)
    mpx, mpy, mdx, mdy = seq(Px) / n, seq(Py) / n, seq(Dx) / n, seq(Dy) / n
    ux, uy, ex, ey = Px - mpx, Py - mpy, Dx - mdx, Dy - mdy
    E = finish_lin(model, n, mpx, mpy, mdx, mdy, seq(ux * ux), seq(ux * uy), seq(uy * uy), seq(ux * ex), seq(uy * ex), seq(ux * ey),
                   seq(uy * ey))
    return None if E is None else to_pixels(fr, E, False)


def errors2(T, pts):
    """Squared reprojection error of every pair and the sign test of W."""
    px, py, qx, qy = (pts[:, i].astype(f64) for i in range(4))
    X = (T[0, 0] * px + T[0, 1] * py) + T[0, 2]
    Y = (T[1, 0] * px + T[1, 1] * py) + T[1, 2]
    W = (T[2, 0] * px + T[2, 1] * py) + T[2, 2]
    with np.errstate(all="ignore"):
        ex, ey = X / W - qx, Y / W - qy
        return ex * ex + ey * ey, W > 0.


def inliers(T, pts, thr2):
    e2, pos = errors2(T, pts)
    with np.errstate(invalid="ignore"):
        return pos & (e2 <= thr2)


def blk_sum(terms):
    """The fixed summation order of the refits (256 partial sums, halves of 64, four results)."""
    t = np.asarray(terms, f64)
    pad = (-len(t)) % 256
    t = np.concatenate([t, np.zeros(pad)]).reshape(-1, 256) if len(t) + pad else np.zeros((0, 256))
    acc = np.zeros(256, f64)
    for row in t:
        acc = acc + row
    v = acc.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :o] + v[:, o:2 * o]
    v = v[:, 0]
    return ((v[0] + v[1]) + v[2]) + v[3]


def block_fit(fr, model, pts, inl):
    Px, Py, Qx, Qy, Dx, Dy = fr.norm(pts)
    m = lambda a: np.where(inl, a, 0.)
    n = blk_sum(m(np.ones(len(pts))))
    if model == 4:
        r1, r2 = homography_rows(Px, Py, Qx, Qy, Dx, Dy)
        M = np.zeros((8, 9), f64)
        for r in range(8):
            for k in range(r, 9):
                s = blk_sum(m(r1[:, r] * r1[:, k] + r2[:, r] * r2[:, k]))
                M[r, k] = s
                if k < 8:
                    M[k, r] = s
        if not n >= 4.:
            return None
        z = ge8(M, 1e-12)
        return None if z is None else to_pixels(fr, np.append(z, 0.), True)
    spx, spy, sdx, sdy = blk_sum(m(Px)), blk_sum(m(Py)), blk_sum(m(Dx)), blk_sum(m(Dy))
    nn = n if n > 0. else f64(1.)
    mpx, mpy, mdx, mdy = spx / nn, spy / nn, sdx / nn, sdy / nn
    s7 = [f64(0.)] * 7
    if model >= 2:
        ux, uy, ex, ey = Px - mpx, Py - mpy, Dx - mdx, Dy - mdy
        s7 = [blk_sum(m(a)) for a in (ux * ux, ux * uy, uy * uy, ux * ex, uy * ex, ux * ey, uy * ey)]
    E = finish_lin(model, n, mpx, mpy, mdx, mdy, *s7)
    return None if E is None else to_pixels(fr, E, False)


def fit_motion(p, q, status, size, scores=None, model=2, hypotheses=0, seed=0, min_score=0, quality=0.0, max_shift=0.0, inlier_px=0.0):
    """-> dict(T, model_used, n_valid, n_inliers, winner, inlier [n] uint8, samples [hypotheses, 4] int32 (input indices),
    counts [hypotheses], edge: the smallest | error - threshold | in px over every decision the final answer rests on)."""
    w, h = size
    fr = Frame(w, h)
    p = np.asarray(p, np.float32).reshape(-1, 2); q = np.asarray(q, np.float32).reshape(-1, 2)
    status = np.asarray(status, np.uint8).reshape(-1)
    n = len(p)
    H = hypotheses or 512
    ms = max_shift if max_shift > 0 else 0.1 * float(max(w, h))
    thr = inlier_px if inlier_px > 0 else 1.0
    thr2 = f64(thr) * f64(thr)
    dx, dy = q[:, 0].astype(f64) - p[:, 0].astype(f64), q[:, 1].astype(f64) - p[:, 1].astype(f64)
    with np.errstate(invalid="ignore"):
        valid = (status == 1) & (dx * dx + dy * dy <= f64(ms) * f64(ms))
    if scores is not None:
        sc = np.asarray(scores, np.int32).reshape(-1)
        gate = f64(quality) * f64(int(sc.max()) if n else 0)
        valid &= (sc > 0) & (sc >= min_score) & (sc.astype(f64) >= gate)
    vidx = np.flatnonzero(valid)
    pts = np.concatenate([p[vidx], q[vidx]], 1).astype(np.float32)
    nv = len(vidx)
    k = model
    samples = np.full((H, 4), -1, np.int32)
    counts = np.zeros(H, np.int64)
    edge = [np.inf]

    def note(T):
        if nv:
            e2, _ = errors2(T, pts)
            with np.errstate(invalid="ignore"):
                d = np.abs(np.sqrt(e2) - thr)
            if np.any(np.isfinite(d)):
                edge[0] = min(edge[0], float(np.nanmin(d)))

    best, winner, Tw = -1, 0, None
    for j in range(H):
        smp = sample(seed, j, k, nv)
        T = hypothesis(fr, model, pts, smp) if smp is not None else None
        if T is not None:
            samples[j, :k] = vidx[smp]
            counts[j] = int(inliers(T, pts, thr2).sum())
        if counts[j] > best:
            best, winner, Tw = int(counts[j]), j, T
    if Tw is not None:
        note(Tw)
    inl = inliers(Tw, pts, thr2) if Tw is not None else np.zeros(nv, bool)
    m = model
    T = np.eye(3)
    while True:
        if m == 0:
            T = np.eye(3)
            note(T)
            inl = inliers(T, pts, thr2)
            break
        ok = True
        for _ in range(2 if m == model else 1):
            Tn = block_fit(fr, m, pts, inl)
            if Tn is None:
                ok = False
                break
            T = Tn
            note(T)
            inl = inliers(T, pts, thr2)
        if ok and int(inl.sum()) >= NEED[m]:
            break
        m -= 1
    out = np.zeros(n, np.uint8)
    out[vidx] = inl
    X = (T[0, 0] * fr.fcx + T[0, 1] * fr.fcy) + T[0, 2]
    Y = (T[1, 0] * fr.fcx + T[1, 1] * fr.fcy) + T[1, 2]
    W = (T[2, 0] * fr.fcx + T[2, 1] * fr.fcy) + T[2, 2]
    ninl = int(inl.sum())
    return dict(T=T, model_used=m, n_valid=nv, n_inliers=ninl, winner=winner, inlier=out, samples=samples, counts=counts,
                edge=edge[0], result=(X / W - fr.fcx, Y / W - fr.fcy, ninl / nv if nv else 0.0))
