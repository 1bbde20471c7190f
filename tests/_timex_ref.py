"""The reference's time-exposure pipelines restated in numpy, the slow obvious way.

compute_timex (main.cpp:1195-1263) and compute_brightColor (main.cpp:1265-1383) of /root/reference/RipCurrents_main, with
the OpenCV 4.1.0 calls they make (cvtColor COLOR_RGB2HSV / COLOR_HSV2RGB on 8UC3: color_hsv.cpp RGB2HSV_b / HSV2RGB_b;
Mat / scalar and convertTo: convert_scale) written out.  Every product is recomputed from the whole ring on every frame,
slot by slot, as the reference's loops do: no running sums, no winner bookkeeping.  The colour conversions are restated
from upstream's sources as remembered; there is no OpenCV build here to pin them against.
"""
import numpy as np

PRODUCTS = ("mean", "average", "bright", "dark")
f32 = np.float32


def cv_round(x):
    """cvRound: to nearest, ties to even."""
    return np.rint(x)


def saturate_u8(x):
    return np.clip(x, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------- color_hsv.cpp, 8-bit forms, hue range 180
HSV_SHIFT = 12
SDIV = np.zeros(256, np.int64)
HDIV = np.zeros(256, np.int64)
for _i in range(1, 256):                                   # RGB2HSV_b::operator(): the tables, filled once
    SDIV[_i] = int(cv_round((255 << HSV_SHIFT) / (1.0 * _i)))
    HDIV[_i] = int(cv_round((180 << HSV_SHIFT) / (6.0 * _i)))


def rgb_to_hsv_u8(img):
    """cvtColor(img, COLOR_RGB2HSV), 8UC3: bytes 0, 1, 2 are r, g, b."""
    a = np.asarray(img).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = (diff * SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.empty_like(v)
    is_r = v == r                                          # vr = v == r ? -1 : 0
    is_g = ~is_r & (v == g)                                # vg, only looked at where vr is 0
    rest = ~is_r & ~is_g
    h[is_r] = (g - b)[is_r]
    h[is_g] = (b - r + 2 * diff)[is_g]
    h[rest] = (r - g + 4 * diff)[rest]
    h = (h * HDIV[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT      # arithmetic shift of a possibly negative product
    h[h < 0] += 180
    return np.stack([saturate_u8(h), s.astype(np.uint8), v.astype(np.uint8)], -1)


def hsv_to_rgb_u8(img):
    """cvtColor(img, COLOR_HSV2RGB), 8UC3: HSV2RGB_b = scale to float, HSV2RGB_f with hscale 6 / 180, scale back."""
    a = np.asarray(img)
    h = a[..., 0].astype(f32)
    s = a[..., 1].astype(f32) * (f32(1) / f32(255))
    v = a[..., 2].astype(f32) * (f32(1) / f32(255))
    h = h * (f32(6) / f32(180))
    while (h >= 6).any():                                  # do h -= 6; while (h >= 6)
        h = np.where(h >= 6, h - f32(6), h).astype(f32)
    sector = np.floor(h).astype(np.int64)
    h = (h - sector.astype(f32)).astype(f32)
    one = f32(1)
    tab = [v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))]
    sector_data = [(1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0)]     # (b, g, r)
    b, g, r = v.copy(), v.copy(), v.copy()                 # s == 0: b = g = r = v
    for k, (ib, ig, ir) in enumerate(sector_data):
        m = (sector == k) & (s != 0)
        b[m], g[m], r[m] = tab[ib][m], tab[ig][m], tab[ir][m]
    to8 = lambda x: saturate_u8(cv_round(x * f32(255)))
    return np.stack([to8(r), to8(g), to8(b)], -1)          # COLOR_HSV2RGB: blue index 2


# ---------------------------------------------------------------------------- Mat / scalar
def divide_u8(m, w):
    """`Mat(8U) / w`: convertTo with alpha = 1 / w, scaled in float, rounded by cvRound, saturated."""
    return saturate_u8(cv_round(m.astype(f32) * f32(1.0 / w)))


def add_u8(a, b):
    """Mat(8U) += Mat(8U): saturating."""
    return saturate_u8(a.astype(np.int32) + b.astype(np.int32))


def resize_bgr(img, dw, dh):
    """resize(img, Size(dw, dh), 0, 0, INTER_LINEAR) on 8UC3: resize.cpp's 11-bit fixed-point bilinear."""
    img = np.asarray(img)
    sh, sw = img.shape[:2]

    def taps(dn, sn, clamp_alpha):
        scale = 1.0 / (dn / sn)
        f = ((np.arange(dn) + 0.5) * scale - 0.5).astype(f32)
        i = np.floor(f).astype(np.int64)
        f = (f - i.astype(f32)).astype(f32)
        if clamp_alpha:                                    # columns: the coefficient is zeroed at the borders
            lo, hi = i < 0, i >= sn - 1
            f[lo | hi] = 0
            i[lo] = 0
            i[hi] = sn - 1
        c0 = cv_round((f32(1) - f) * f32(2048)).astype(np.int64)
        c1 = cv_round(f * f32(2048)).astype(np.int64)
        return i, c0, c1

    sx, a0, a1 = taps(dw, sw, True)
    sy, b0, b1 = taps(dh, sh, False)
    sx1 = np.minimum(sx + 1, sw - 1)
    sy0, sy1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    src = img.astype(np.int64)
    rows0 = src[sy0][:, sx] * a0[None, :, None] + src[sy0][:, sx1] * a1[None, :, None]
    rows1 = src[sy1][:, sx] * a0[None, :, None] + src[sy1][:, sx1] * a1[None, :, None]
    v = (((b0[:, None, None] * (rows0 >> 4)) >> 16) + ((b1[:, None, None] * (rows1 >> 4)) >> 16) + 2) >> 2
    return saturate_u8(v)


def bgr_to_gray(img):
    """cvtColor(COLOR_BGR2GRAY) on 8UC3: 14-bit coefficients."""
    a = np.asarray(img).astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


# ---------------------------------------------------------------------------- the two pipelines
class TimexRef:
    """State of compute_timex (sum_rgb, framecount) and compute_brightColor (buffer_hsv, currentBuffer) for one clip."""

    def __init__(self, w, h, window=50):
        self.window = window
        self.sum_rgb = np.zeros((h, w, 3), f32)                                  # main.cpp:1216
        self.framecount = 0
        self.buffer_hsv = [np.zeros((h, w, 3), np.uint8) for _ in range(window)]   # main.cpp:1292-1295
        self.current = 0

    def push_mean(self, frame):
        """main.cpp:1229-1241"""
        self.framecount += 1
        self.sum_rgb = self.sum_rgb + np.asarray(frame).astype(f32)
        average_rgb = self.sum_rgb * f32(1.0 / self.framecount)                  # Mat(32F) / int
        return saturate_u8(cv_round(average_rgb))

    def push_ring(self, frame, options=(0, 1, 2)):
        """main.cpp:1305-1361 for each `option` asked for: {option: outImg}."""
        W, buf = self.window, self.buffer_hsv
        buf[self.current] = rgb_to_hsv_u8(frame)
        out = {}
        for option in options:
            average_hsv = divide_u8(buf[0], W)
            for i in range(1, W):
                if option == 0:
                    average_hsv = add_u8(average_hsv, divide_u8(buf[i], W))
                else:
                    val, val_o = buf[i][..., 2], average_hsv[..., 2]
                    m = (val_o < val) if option == 1 else (val_o > val)
                    average_hsv[m] = buf[i][m]
            out[option] = hsv_to_rgb_u8(average_hsv)
        self.current += 1
        if self.current >= W:
            self.current = 0
        return out

    def push(self, frame, products=PRODUCTS):
        """One frame through both pipelines -> {product name: image}."""
        res = {}
        if "mean" in products:
            res["mean"] = self.push_mean(frame)
        options = [k for k, name in enumerate(PRODUCTS[1:]) if name in products]
        if options:
            ring = self.push_ring(frame, options)
            for k in options:
                res[PRODUCTS[1 + k]] = ring[k]
        return res
