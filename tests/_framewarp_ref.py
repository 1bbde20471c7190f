"""General warps and the multi-patch stabiliser restated in numpy, the slow obvious way.

warpAffine / warpPerspective on 8UC3 (INTER_LINEAR, BORDER_CONSTANT 0) as OpenCV 4.1.0's CPU path computes them
(imgwarp.cpp), written out from upstream's sources as remembered: there is no OpenCV build here to pin them against.
The coordinates are upstream's (fixed point for the affine form, double per pixel in 64-wide blocks for the
perspective form), the sample is remap's 8-bit table form, exactly as tests/_framestab_ref.py has it for a translation.
The multi-patch stabiliser (several static patches, gated by their response, a translation / similarity / affine
motion fitted to their shifts) is this project's own; its arithmetic is restated from include/rcflow.h.
"""
import numpy as np

import _framestab_ref as S

INT_MIN, INT_MAX = -2147483648, 2147483647
TRANSLATION, SIMILARITY, AFFINE = 1, 2, 3
MODELS = {"translation": TRANSLATION, "similarity": SIMILARITY, "affine": AFFINE}


# ---------------------------------------------------------------------------- matrices
def invert_affine(M):
    """warpAffine's inversion of a forward 2 x 3 matrix (double, upstream's order of operations)."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, np.float64).reshape(2, 3)


def invert_perspective(M):
    """The closed-form 3 x 3 inverse: every entry a 2 x 2 minor times 1 / det, in double."""
    a = np.asarray(M, np.float64).reshape(3, 3)
    det = a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) - a[0, 1] * (a[1, 0] * a[2, 2] - a[1, 2] * a[2, 0]) \
        + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0])
    d = 1.0 / det
    o = np.empty((3, 3), np.float64)
    o[0, 0] = (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) * d
    o[0, 1] = (a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]) * d
    o[0, 2] = (a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]) * d
    o[1, 0] = (a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]) * d
    o[1, 1] = (a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]) * d
    o[1, 2] = (a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]) * d
    o[2, 0] = (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]) * d
    o[2, 1] = (a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]) * d
    o[2, 2] = (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]) * d
    return o


# ---------------------------------------------------------------------------- coordinates
def _sat_short(v):
    return np.clip(v, -32768, 32767)


def affine_coords(M, dw, dh):
    """Destination-to-source matrix M (2 x 3) -> (sx, sy, fx, fy), each (dh, dw) int64: the source pixel (saturated to
    short) and the 1/32 px fractions.  AB_BITS = 10, INTER_BITS = 5; every product and sum rounds on its own."""
    m = np.asarray(M, np.float64).reshape(6)
    x = np.arange(dw, dtype=np.float64)
    y = np.arange(dh, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024.0).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024.0).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    return _sat_short(X >> 5), _sat_short(Y >> 5), X & 31, Y & 31


def perspective_block(dw, dh):
    """Width of the blocks upstream walks the destination in: bh0 = min(16, dh), bw0 = min(1024 / bh0, dw)."""
    bh0 = min(16, dh)
    return min(1024 // bh0, dw)


def perspective_coords(M, dw, dh):
    """Destination-to-source matrix M (3 x 3) -> (sx, sy, fx, fy).  Double per pixel; the bits depend on the block's
    first column xb: X0 = M0 xb + M1 y + M2 and the pixel adds M0 (x - xb)."""
    m = np.asarray(M, np.float64).reshape(9)
    bw0 = perspective_block(dw, dh)
    x = np.arange(dw, dtype=np.int64)
    xb = ((x // bw0) * bw0).astype(np.float64)[None, :]
    x1 = (x % bw0).astype(np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    X0 = m[0] * xb + m[1] * y + m[2]
    Y0 = m[3] * xb + m[4] * y + m[5]
    W0 = m[6] * xb + m[7] * y + m[8]
    W = W0 + m[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = np.where(W != 0, 32.0 / W, 0.0)
        fX = (X0 + m[0] * x1) * W
        fY = (Y0 + m[3] * x1) * W

    def clamp(v):
        # std::max((double)INT_MIN, std::min((double)INT_MAX, v)): min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a
        v = np.where(v < float(INT_MAX), v, float(INT_MAX))
        return np.where(float(INT_MIN) < v, v, float(INT_MIN))

    X = np.rint(clamp(fX)).astype(np.int64)
    Y = np.rint(clamp(fY)).astype(np.int64)
    return _sat_short(X >> 5), _sat_short(Y >> 5), X & 31, Y & 31


# ---------------------------------------------------------------------------- sample
def sample(img, sx, sy, fx, fy):
    """remap's bilinear sample in 8-bit fixed point: weights of 2^15, (sum + 2^14) >> 15, a tap outside counts 0."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    src = img.reshape(h, w, -1).astype(np.int64)
    Wt = S.warp_weights()[fy, fx]                            # (dh, dw, 4)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]

    acc = tap(sy, sx) * Wt[..., 0:1] + tap(sy, sx + 1) * Wt[..., 1:2] + tap(sy + 1, sx) * Wt[..., 2:3] \
        + tap(sy + 1, sx + 1) * Wt[..., 3:4]
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    return out if img.ndim == 3 else out[..., 0]


def warp_affine(img, M, dsize=None, inverse_map=False):
    """cv::warpAffine(img, M, dsize, INTER_LINEAR [| WARP_INVERSE_MAP]); dsize = (dw, dh), default the source's."""
    h, w = np.asarray(img).shape[:2]
    dw, dh = (w, h) if dsize is None else dsize
    M = np.asarray(M, np.float64).reshape(2, 3)
    if not inverse_map:
        M = invert_affine(M)
    return sample(img, *affine_coords(M, dw, dh))


def warp_perspective(img, M, dsize=None, inverse_map=False):
    """cv::warpPerspective(img, M, dsize, INTER_LINEAR [| WARP_INVERSE_MAP])."""
    h, w = np.asarray(img).shape[:2]
    dw, dh = (w, h) if dsize is None else dsize
    M = np.asarray(M, np.float64).reshape(3, 3)
    if not inverse_map:
        M = invert_perspective(M)
    return sample(img, *perspective_coords(M, dw, dh))


# ---------------------------------------------------------------------------- the fit
def patch_centres(rois):
    r = np.asarray(rois, np.float64).reshape(-1, 4)
    return np.stack([r[:, 0] + (r[:, 2] - 1.0) / 2.0, r[:, 1] + (r[:, 3] - 1.0) / 2.0], -1)


def fit_motion(rois, shifts, model, min_response, frame_size):
    """Least-squares motion over the patches whose response passes the gate.

    rois: n x (x, y, w, h); shifts: n x (dx, dy, response); frame_size = (w, h).
    -> (motion (2, 3): T p = A p + b maps the corrected frame to the incoming one, model_used, patches_used,
        result = (dx, dy of the frame centre under T, smallest response used)).
    The DISPLACEMENT d = B (p - pbar) + t is fitted on centred coordinates (B = A - I), so zero shifts give the
    identity exactly.  Ladder: affine needs 3 patches and det > 1e-12 Sxx Syy; similarity 2 patches and a spread
    S > 0; translation 1; none: the identity, model_used 0."""
    c = patch_centres(rois)
    s = np.asarray(shifts, np.float64).reshape(-1, 3)
    use = [k for k in range(len(c)) if s[k, 2] >= min_response]       # NaN fails the comparison
    m = len(use)
    if m == 0:
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), 0, 0, (0.0, 0.0, 0.0)
    px = py = tx = ty = 0.0
    rmin = np.inf
    for k in use:
        px += c[k, 0]
        py += c[k, 1]
        tx += s[k, 0]
        ty += s[k, 1]
        rmin = min(rmin, s[k, 2])
    px, py, tx, ty = px / m, py / m, tx / m, ty / m
    sxx = sxy = syy = xdx = ydx = xdy = ydy = 0.0
    for k in use:
        ux, uy = c[k, 0] - px, c[k, 1] - py
        ex, ey = s[k, 0] - tx, s[k, 1] - ty
        sxx += ux * ux
        sxy += ux * uy
        syy += uy * uy
        xdx += ux * ex
        ydx += uy * ex
        xdy += ux * ey
        ydy += uy * ey
    b00 = b01 = b10 = b11 = 0.0
    used = TRANSLATION
    det = sxx * syy - sxy * sxy
    if model >= AFFINE and m >= 3 and det > 1e-12 * (sxx * syy):
        used = AFFINE
        b00, b01 = (xdx * syy - ydx * sxy) / det, (ydx * sxx - xdx * sxy) / det
        b10, b11 = (xdy * syy - ydy * sxy) / det, (ydy * sxx - xdy * sxy) / det
    elif model >= SIMILARITY and m >= 2 and sxx + syy > 0.0:
        used = SIMILARITY
        a, b = (xdx + ydy) / (sxx + syy), (xdy - ydx) / (sxx + syy)
        b00, b01, b10, b11 = a, -b, b, a
    motion = np.array([[1.0 + b00, b01, tx - (b00 * px + b01 * py)], [b10, 1.0 + b11, ty - (b10 * px + b11 * py)]])
    fw, fh = frame_size
    cx, cy = (fw - 1.0) / 2.0 - px, (fh - 1.0) / 2.0 - py
    return motion, used, m, ((b00 * cx + b01 * cy) + tx, (b10 * cx + b11 * cy) + ty, float(rmin))


# ---------------------------------------------------------------------------- the chain
class MultiStabRef:
    """The multi-patch stabiliser: push() returns the corrected frame, the n x 3 shifts and the fit.  anchor =
    "previous": every frame is registered to the last CORRECTED frame (the reference's chain); "first": to the first
    frame after open / reset."""

    def __init__(self, w, h, rois, model="similarity", min_response=0.0, anchor="previous"):
        self.w, self.h = w, h
        self.rois = [tuple(int(v) for v in r) for r in rois]
        self.model = MODELS[model] if isinstance(model, str) else model
        self.min_response, self.anchor = min_response, anchor
        self.window = S.hanning_window(self.rois[0][3], self.rois[0][2])
        self.prev = None                                     # the n gray float patches to register against

    def patches(self, frame):
        return [S.bgr_to_gray(frame[y:y + rh, x:x + rw]).astype(S.f32) for (x, y, rw, rh) in self.rois]

    def shifts(self, frame):
        return np.array([S.phase_correlate(a, b, self.window) for a, b in zip(self.prev, self.patches(frame))])

    def push(self, frame, shifts=None, motion=None):
        """shifts / motion: use these instead of the chain's own (to follow another implementation bit for bit)."""
        if self.prev is None:
            self.prev = self.patches(frame)
            return frame.copy(), np.zeros((len(self.rois), 3)), (np.array([[1.0, 0, 0], [0, 1.0, 0]]), 0, 0, (0.0, 0.0, 0.0))
        own = self.shifts(frame)
        fit = fit_motion(self.rois, own if shifts is None else shifts, self.model, self.min_response, (self.w, self.h))
        out = warp_affine(frame, fit[0] if motion is None else motion, inverse_map=True)
        if self.anchor != "first":
            self.prev = self.patches(out)
        return out, own, fit


# ---------------------------------------------------------------------------- a rolling, breathing, shaking clip
def rolling_clip(w=640, h=480, frames=40, seed=7, max_roll_deg=0.3, max_zoom=0.005, max_shake=4.0, margin=48,
                 water=None):
    """A colour clip of a static textured scene seen by a camera that rolls, zooms and shakes, with moving water in
    the middle third -> (clip (frames, h, w, 3) uint8, motions (frames, 2, 3): frame_t(p) = scene(T_t p), T_0 = I).

    The static scene is a DenseTexture tile larger than the frame by `margin` on every side, rendered per frame by
    warp_affine (inverse map) so that the clip is exactly reproducible from numpy alone.  water: (frames, h', w') uint8
    painted (unwarped) over the middle of every frame, or None."""
    rng = np.random.RandomState(seed)
    tex = S.DenseTexture(1024, 311 + seed).u8()
    assert w + 2 * margin <= 1024 and h + 2 * margin <= 1024
    scene = tex[:h + 2 * margin, :w + 2 * margin]
    scene = np.stack([np.clip(np.rint(scene * 0.9 + 10), 0, 255), scene, np.clip(np.rint(255 - scene * 0.8), 0, 255)], -1).astype(np.uint8)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    clip = np.zeros((frames, h, w, 3), np.uint8)
    motions = np.zeros((frames, 2, 3))
    for t in range(frames):
        ang = np.deg2rad(rng.uniform(-max_roll_deg, max_roll_deg)) if t else 0.0
        s = 1.0 + (rng.uniform(-max_zoom, max_zoom) if t else 0.0)
        sh = rng.randint(-int(max_shake * 4), int(max_shake * 4) + 1, 2) / 4.0 if t else np.zeros(2)
        a, b = s * np.cos(ang), s * np.sin(ang)
        T = np.array([[a, -b, cx - (a * cx - b * cy) + sh[0]], [b, a, cy - (b * cx + a * cy) + sh[1]]])
        motions[t] = T
        Ts = T.copy()
        Ts[:, 2] += margin                                   # frame pixel -> scene pixel
        clip[t] = warp_affine(scene, Ts, dsize=(w, h), inverse_map=True)
        if water is not None:
            wh, ww = water.shape[1:3]
            y0, x0 = (h - wh) // 2, (w - ww) // 2
            g = water[t].astype(np.float64)
            clip[t, y0:y0 + wh, x0:x0 + ww, 0] = np.clip(np.rint(g * 0.9 + 10), 0, 255)
            clip[t, y0:y0 + wh, x0:x0 + ww, 1] = g
            clip[t, y0:y0 + wh, x0:x0 + ww, 2] = np.clip(np.rint(255 - g * 0.8), 0, 255)
    return clip, motions


def corner_rois(w, h, size=50, inset=20):
    return [(inset, inset, size, size), (w - inset - size, inset, size, size),
            (inset, h - inset - size, size, size), (w - inset - size, h - inset - size, size, size)]


def patch_drift(roi, frame0, frame):
    """Displacement of `frame`'s patch against `frame0`'s by the numpy phase correlation -> max(|dx|, |dy|)."""
    x, y, rw, rh = roi
    win = S.hanning_window(rh, rw)
    a = S.bgr_to_gray(frame0[y:y + rh, x:x + rw]).astype(S.f32)
    b = S.bgr_to_gray(frame[y:y + rh, x:x + rw]).astype(S.f32)
    d = S.phase_correlate(a, b, win)
    return max(abs(d[0]), abs(d[1]))
