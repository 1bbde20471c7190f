"""The reference's frame stabilisation restated in numpy, the slow obvious way.

compute_phaseCorrelate (main.cpp:1684-1775): per frame cvtColor(BGR2GRAY) -> float, crop the static patch of the last
CORRECTED frame and of the new one, phaseCorrelate with a Hann window, warpAffine the new frame back by the shift, and
the corrected frame becomes `prev`.  The OpenCV 4.1.0 calls (getOptimalDFTSize, createHanningWindow, phaseCorrelate:
phasecorr.cpp; warpAffine + remap INTER_LINEAR on 8UC3: imgwarp.cpp) are written out from upstream's sources as
remembered; there is no OpenCV build here to pin them against.  The DFTs go through np.fft in double (upstream's are
float): the device kernels are held to this by tolerance, the warp bit for bit.
"""
import numpy as np

f32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)


def optimal_dft_size(n):
    """getOptimalDFTSize: the smallest 2^a 3^b 5^c >= n."""
    m = int(n)
    while True:
        k = m
        for p in (2, 3, 5):
            while k % p == 0:
                k //= p
        if k == 1:
            return m
        m += 1


def hanning_window(rows, cols):
    """createHanningWindow(Size(cols, rows), CV_32F): the raised-cosine factors in double, their product rounded to
    float, then a float square root of the whole image."""
    c0, c1 = 2.0 * np.pi / (cols - 1), 2.0 * np.pi / (rows - 1)
    wc = 0.5 * (1.0 - np.cos(c0 * np.arange(cols, dtype=np.float64)))
    wr = 0.5 * (1.0 - np.cos(c1 * np.arange(rows, dtype=np.float64)))
    return np.sqrt((wr[:, None] * wc[None, :]).astype(f32))


def bgr_to_gray(bgr):
    """cvtColor(COLOR_BGR2GRAY) on 8UC3: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    p = bgr.astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def fft_shift(a):
    """phasecorr.cpp fftShift: index i goes to (i + floor(n / 2)) mod n on both axes (odd sizes too)."""
    return np.roll(a, (a.shape[0] // 2, a.shape[1] // 2), (0, 1))


def correlation_surface(a, b, window=None):
    """The shifted correlation surface phaseCorrelate takes its peak from (float32, M x N)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    h, w = a.shape
    M, N = optimal_dft_size(h), optimal_dft_size(w)
    if window is not None:
        a, b = a * window, b * window                      # float products
    pa, pb = np.zeros((M, N), np.float64), np.zeros((M, N), np.float64)
    pa[:h, :w], pb[:h, :w] = a, b                          # padded at the bottom / right
    P = (np.fft.fft2(pa) * np.conj(np.fft.fft2(pb))).astype(np.complex64)      # mulSpectrums(F1, F2, conjB = true)
    m = np.sqrt(P.real.astype(np.float64) ** 2 + P.imag.astype(np.float64) ** 2).astype(f32)   # magSpectrums
    den = (m * m + f32(FLT_EPSILON)).astype(np.float64)                        # divSpectrums by (m, 0)
    C = ((P.real * m).astype(np.float64) / den).astype(f32) + 1j * ((P.imag * m).astype(np.float64) / den).astype(f32)
    r = (np.fft.ifft2(C.astype(np.complex128)).real * (M * N)).astype(f32)     # idft without DFT_SCALE
    return fft_shift(r)


def phase_correlate(a, b, window=None, return_surface=False):
    """cv::phaseCorrelate(a, b, window, &response) -> (shift_x, shift_y, response).  b(x) = a(x - d) gives +d."""
    s = correlation_surface(a, b, window)
    M, N = s.shape
    py, px = np.unravel_index(int(np.argmax(s)), s.shape)          # minMaxLoc: the first maximum in row-major order
    minr, maxr, minc, maxc = max(py - 2, 0), min(py + 2, M - 1), max(px - 2, 0), min(px + 2, N - 1)
    cx = cy = total = 0.0
    for y in range(minr, maxr + 1):                                # weightedCentroid, 5 x 5, double
        for x in range(minc, maxc + 1):
            v = float(s[y, x])
            cx += x * v
            cy += y * v
            total += v
    response = total / (M * N)
    total += DBL_EPSILON
    out = (N / 2.0 - cx / total, M / 2.0 - cy / total, response)
    return out + (s,) if return_surface else out


def peak_is_ambiguous(surface, rel=1e-3):
    """True when the two highest values of the surface are within `rel` of each other: such a frame may resolve its
    peak differently in fp32 and is excluded from device comparisons."""
    v = np.sort(surface.ravel().astype(np.float64))
    return bool(v[-1] - v[-2] <= rel * abs(v[-1]))


def warp_weights():
    """The 32 x 32 bilinear weight quadruples of remap's fixed-point table: (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx in
    1/1024 scaled to 2^15, as integers -> (32, 32, 4) int64 indexed [fy, fx]."""
    f = np.arange(32, dtype=np.int64)
    fy, fx = f[:, None], f[None, :]
    return np.stack([(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32], -1)


def warp_translate(img, shift_x, shift_y):
    """warpAffine(img, [1 0 -shift_x; 0 1 -shift_y], img.size()) on 8UC3 / 8UC1: INTER_LINEAR, BORDER_CONSTANT 0.
    The matrix is inverted first, so dst(x, y) = src(x + shift_x, y + shift_y), in 8-bit fixed point."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    src = img.reshape(h, w, -1).astype(np.int64)
    X0 = int(np.rint(float(shift_x) * 1024.0)) + 16
    X = (X0 + np.arange(w, dtype=np.int64) * 1024) >> 5
    sx, fx = X >> 5, X & 31
    Y0 = np.rint((np.arange(h, dtype=np.float64) + float(shift_y)) * 1024.0).astype(np.int64) + 16   # y inside the rounding
    Y = Y0 >> 5
    sy, fy = Y >> 5, Y & 31
    W = warp_weights()[fy[:, None], fx[None, :]]                   # (h, w, 4)

    def tap(yy, xx):
        ok = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
        v = src[np.clip(yy, 0, h - 1)[:, None], np.clip(xx, 0, w - 1)[None, :]]
        return v * ok[..., None]                                   # a tap outside the image contributes 0

    acc = tap(sy, sx) * W[..., 0:1] + tap(sy, sx + 1) * W[..., 1:2] + tap(sy + 1, sx) * W[..., 2:3] + tap(sy + 1, sx + 1) * W[..., 3:4]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8).reshape(img.shape)


class FrameStabRef:
    """The loop of main.cpp:1707-1759 with its loop-carried `prev` (the last CORRECTED frame).  push() returns the
    corrected frame and (shift_x, shift_y, response); the first frame is returned as it is with (0, 0, 0)."""

    def __init__(self, w, h, roi=None):
        self.w, self.h = w, h
        self.roi = (w - 50, 50, 50, 50) if roi is None else tuple(roi)
        self.window = hanning_window(self.roi[3], self.roi[2])
        self.prev = None

    def patch(self, frame):
        x, y, rw, rh = self.roi
        return bgr_to_gray(frame[y:y + rh, x:x + rw]).astype(f32)

    def shift(self, frame):
        return phase_correlate(self.patch(self.prev), self.patch(frame), self.window)

    def push(self, frame, shift=None):
        """shift: use this (shift_x, shift_y) for the warp instead of the loop's own (to follow another
        implementation's track bit for bit)."""
        if self.prev is None:
            self.prev = frame.copy()
            return self.prev, (0.0, 0.0, 0.0)
        res = self.shift(frame)
        use = res if shift is None else shift
        self.prev = warp_translate(frame, use[0], use[1])
        return self.prev, res


# ---------------------------------------------------------------------------- a shaken clip to stabilise
class DenseTexture:
    """A periodic n x n texture with a dense 1/f spectrum up to 0.45 cycles / px (filtered seeded white noise), which
    can be evaluated displaced by any sub-pixel amount exactly (a phase ramp on its spectrum).  Phase correlation
    whitens the spectrum, so a texture needs signal in every bin to be registered well: a sum of a few dozen sinusoids
    (synth._eval_texture) leaves most bins to the 8-bit rounding noise."""

    def __init__(self, n=256, seed=3):
        rng = np.random.RandomState(seed)
        f = np.fft.fft2(rng.standard_normal((n, n)))
        self.ky, self.kx = np.meshgrid(np.fft.fftfreq(n), np.fft.fftfreq(n), indexing="ij")
        k = np.hypot(self.kx, self.ky)
        f = f * np.where(k > 0, 1.0 / np.maximum(k, 1.0 / n), 0.0) * (k <= 0.45)
        self.f = f / np.fft.ifft2(f).real.std()

    def at(self, sx, sy):
        """The texture displaced by (sx, sy): at(sx, sy)[y, x] = T(x - sx, y - sy); unit variance."""
        return np.fft.ifft2(self.f * np.exp(-2j * np.pi * (self.kx * sx + self.ky * sy))).real

    def u8(self, sx=0.0, sy=0.0):
        return np.clip(np.rint(128.0 + 40.0 * self.at(sx, sy)), 0, 255).astype(np.uint8)


def shaken_clip(w=640, h=480, frames=40, seed=5, roi=None, block=120, max_shake=6.0, device=None):
    """A colour clip seen by a shaking camera -> (clip (frames, h, w, 3) uint8, shake (frames, 2) float64 = (sx, sy)).

    The scene is synth.surf_clip (moving water) with a static block x block patch of DenseTexture painted around the
    ROI (default: the reference's (w - 50, 50, 50, 50)).  Frame t shows the scene displaced by shake[t]:
    frame_t(x) = scene_t(x - shake[t]), the water by whole pixels, the static block at the exact sub-pixel position.
    shake[0] = 0; the others are seeded multiples of 1/4 px, every other frame a whole number, within +-max_shake.
    device: torch device for the synthesis of the water (None: numpy)."""
    from ripcurrents_amd import synth
    x, y, rw, rh = (w - 50, 50, 50, 50) if roi is None else roi
    rng = np.random.RandomState(seed)
    shake = np.zeros((frames, 2))
    q = rng.randint(-int(max_shake * 4), int(max_shake * 4) + 1, (frames, 2)) / 4.0
    q[::2] = np.rint(q[::2])
    shake[1:] = q[1:]
    water = synth.surf_clip(w, h, frames, seed=1234 + seed, device=device)
    if device is not None:
        water = water.cpu().numpy()
    mg = int(np.ceil(max_shake)) + 2
    tex = DenseTexture(256, 977 + seed)
    assert block + 2 * mg <= 256
    bx0, by0 = x + rw // 2 - block // 2, y + rh // 2 - block // 2
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    clip = np.zeros((frames, h, w, 3), np.uint8)
    for t in range(frames):
        sx, sy = shake[t]
        g = np.roll(water[t], (int(np.rint(sy)), int(np.rint(sx))), (0, 1)).astype(np.float64)
        px, py = xs - sx, ys - sy                                  # the scene point a pixel shows
        inside = (px >= bx0) & (px < bx0 + block) & (py >= by0) & (py < by0 + block)
        img = tex.u8(sx, sy)                                       # canvas index = frame index - block origin + mg
        g[inside] = img[ys[inside] - by0 + mg, xs[inside] - bx0 + mg]
        clip[t, ..., 0] = np.clip(np.rint(g * 0.9 + 10), 0, 255)
        clip[t, ..., 1] = g
        clip[t, ..., 2] = np.clip(np.rint(255 - g * 0.8), 0, 255)
    return clip, shake


def drift(ref, frame0, frame):
    """Displacement of `frame`'s ROI against `frame0`'s, measured by the numpy phase correlation -> max(|dx|, |dy|)."""
    d = phase_correlate(ref.patch(frame0), ref.patch(frame), ref.window)
    return max(abs(d[0]), abs(d[1]))
