"""Float64 reference of ONE flow-iteration launch (flow_iter_kernels.hip):

    flow_out = solve( window( FarnebackUpdateMatrices( R0, R1 sampled at p + flow_in, flow_in ) ) )

= oracle/np_oracle.update_matrices followed by blur_solve, on given R0, R1 and flow_in.  Everything is float64 except the
coordinates p + flow_in, which np_oracle forms in float32 as the C++ and the kernels do, so every floor and every `inside`
branch is decided as they decide it.  Shared by tests/test_flow_forms_ref.py (CPU tier: the reference against the C++ float
oracle, the yardstick) and tests/test_gpu_flow_forms.py (every kernel form against the reference).

The bars of the GPU tests are set from the reference side alone (the issue's rule):

    e = |field - ref64|_inf per pixel,        q = e (det + 1e-3),   det = g11 g22 - g12^2 of the float64 window sums

    max q(kernel) <= 4 max q(C++ float oracle)                over every pixel
    max e(kernel) <= 4 max e(C++ float oracle)                over the pixels with det > 1e-2

and a pixel whose error is within ULP_FLOOR = 8 float32 ulps of the LARGEST |flow| of the reference field passes either way
(the issue's "floor of a few float32 ulps of the largest flow").  Where the 8 comes from, per pixel: the result is stored as
float32 (0.5 ulp of the pixel's flow), the winsize-3 forms solve in float32 -- two differences of products by Kahan's scheme
(1.5 ulp each), a reciprocal (1 ulp), a product (0.5 ulp): 4 ulp -- and the oracle's field is itself float32 (0.5 ulp); 8 is the
next power of two.  That derivation is in ulps of the pixel's own flow; the floor is applied in ulps of the field's maximum,
which is its upper bound over the field and is what the issue words.  The floor is NOT negligible: the largest flow of these
fields is 8 to 340 px (the whole-pixel and outlier fields), so the floor is 7.6e-6 to 2.4e-4 px, often above 4x the oracle's own
e on small or well-conditioned fields (27 x 29 zeros: 7.6e-6 against 5.4e-6).  It decides every committed row whose ratio is
above its factor with nothing missed; every "[flow-forms]" line and the table count those pixels ("under floor").

A winsize-2 / 3 box launch beyond 4x may also pass on the form's own float32 order restated in numpy on the same inputs
(restate_w3_box_f32, the issue's "numpy float32 restatement of that form's summation order, measured on the CPU"): within
RESTATED_FACTOR = 1.25 of the restatement's two maxima AND within RESTATED_CAP = 5 of the oracle's.  tests/test_flow_forms_ref.py
runs the restatement over every committed stage case and over two-launch chains on the driver cases' own frames and pins
that it never misses the 4x bars there: an excess the restatement can justify is a small one, and 1.25 x 4 = 5 bounds it, the
ceiling the pointwise forms have too.  1.25, not 1: the kernel's reciprocal is the hardware's (1 ulp) where the restatement divides, and numpy's fused
multiply-add is rounded twice; both are a fraction of an ulp of the flow against the ten or so ulps of the form's window
sums and solve that the restatement carries in full.
"""
import numpy as np
from scipy.ndimage import correlate1d

from oracle import np_oracle

ULP_FLOOR = 8
FACTOR = 4.0
RESTATED_FACTOR = 1.25
RESTATED_CAP = 5.0
EXCLUDE_PX = 1e-4          # launches fed from the coarser scale: |p + flow_in - border line| below this is excluded
EXCLUDE_CAP = 0.005        # at most this share of a field


def window_sums(M, winsize, gaussian):
    """The window of np_oracle.blur_solve on the five planes (same taps, same border): h x w x 5 float64."""
    m = winsize // 2
    if gaussian:
        sigma = m * 0.3
        i = np.arange(-m, m + 1, dtype=np.float64)
        k = np.exp(-i * i / (2 * sigma * sigma)) if m > 0 else np.ones(1)
        k /= k.sum()
    else:
        k = np.ones(2 * m + 1) / (winsize * winsize) ** 0.5
    return correlate1d(correlate1d(M, k, axis=0, mode="nearest"), k, axis=1, mode="nearest")


def launch(R0, R1, flow_in, winsize, gaussian):
    """(flow_out, det) of one launch in float64.  flow_in None = zeros (the coarsest scale)."""
    R0 = np.asarray(R0, np.float64)
    R1 = np.asarray(R1, np.float64)
    h, w = R0.shape[:2]
    fin = np.zeros((h, w, 2), np.float32) if flow_in is None else np.ascontiguousarray(flow_in, np.float32)
    M = np_oracle.update_matrices(R0, R1, fin.astype(np.float64))
    flow = np_oracle.blur_solve(M, winsize, bool(gaussian))
    B = window_sums(M, winsize, bool(gaussian))
    det = B[..., 0] * B[..., 2] - B[..., 1] ** 2
    return flow, det


def oracle_launch(orc, R0, R1, flow_in, winsize, gaussian):
    """The same launch by the C++ float oracle: update_matrices + update_flow (FarnebackUpdateFlow_Blur / _GaussianBlur)."""
    R0 = np.ascontiguousarray(R0, np.float32)
    R1 = np.ascontiguousarray(R1, np.float32)
    h, w = R0.shape[:2]
    fin = np.zeros((h, w, 2), np.float32) if flow_in is None else np.ascontiguousarray(flow_in, np.float32)
    M = orc.update_matrices(R0, R1, fin)
    out = fin.copy()
    orc.update_flow(R0, R1, out, M, winsize, False, bool(gaussian))
    return out


def border_excluded(flow_in):
    """Pixels whose displaced position p + flow_in (float32, as the kernels form it) lies within EXCLUDE_PX of the lines
    x = 0, x = w - 1, y = 0 or y = h - 1: an ulp of the kernel's float32 up-sampling can flip their `inside` branch."""
    h, w = flow_in.shape[:2]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fx = (xs.astype(np.float32) + flow_in[..., 0].astype(np.float32)).astype(np.float64)
    fy = (ys.astype(np.float32) + flow_in[..., 1].astype(np.float32)).astype(np.float64)
    near = lambda v, line: np.abs(v - line) < EXCLUDE_PX
    return near(fx, 0) | near(fx, w - 1) | near(fy, 0) | near(fy, h - 1)


def upsampled(orc, coarse, w, h, pyr_scale):
    """flow_in of a launch fed from the coarser scale: resize(prevFlow, INTER_LINEAR) * (1 / pyr_scale), float32 like
    optflow.cpp calc() (oracle.resize_linear, then the product rounded once)."""
    return (orc.resize_linear(np.ascontiguousarray(coarse, np.float32), w, h) * np.float32(1.0 / pyr_scale)).astype(np.float32)


def figures(field, ref, det, exclude=None):
    """(max q, max e on det > 1e-2, max e) of a float32 field against the float64 reference, over the non-excluded pixels."""
    e = np.abs(np.asarray(field, np.float64) - ref).max(-1)
    if exclude is not None:
        e = np.where(exclude, 0.0, e)
    q = e * (det + 1e-3)
    well = det > 1e-2
    return float(q.max()), float(e[well].max()) if well.any() else 0.0, float(e.max())


def ulp_floor(ref):
    return ULP_FLOOR * float(np.spacing(np.float32(max(float(np.abs(ref).max()), 1e-30))))


def violations(field, ref, det, oracle_field, exclude=None, factor=FACTOR, restated=None):
    """Pixels of `field` that miss the bars set by `oracle_field` (see the module text), and the figures of both:
    returns (number of violating pixels, dict of figures; under_floor = the pixels beyond the factor that the ulp floor passes).
    `restated` (optional): the same launch by restate_w3_box_f32; a pixel then also passes within RESTATED_FACTOR x the
    restatement's two maxima, as long as it is within RESTATED_CAP x the oracle's."""
    e = np.abs(np.asarray(field, np.float64) - ref).max(-1)
    if not np.isfinite(e).all():
        return int((~np.isfinite(e)).sum()), dict(nonfinite=True)
    keep = np.ones(e.shape, bool) if exclude is None else ~exclude
    qo, eo, eo_all = figures(oracle_field, ref, det, exclude)
    qk, ek, ek_all = figures(field, ref, det, exclude)
    floor = ulp_floor(ref)
    q = e * (det + 1e-3)
    well = det > 1e-2
    beyond = keep & ((q > factor * qo) | (well & (e > factor * eo)))
    bad = beyond & (e > floor)
    g = dict(q_oracle=qo, q_kernel=qk, e_oracle=eo, e_kernel=ek, e_oracle_all=eo_all, e_kernel_all=ek_all, floor=floor,
             under_floor=int((beyond & (e <= floor)).sum()), excluded=0.0 if exclude is None else float(exclude.mean()))
    if restated is not None:
        qr, er, _ = figures(restated, ref, det, exclude)
        g.update(q_restated=qr, e_restated=er)
        bad &= (q > RESTATED_FACTOR * qr) | (well & (e > RESTATED_FACTOR * er)) | (q > RESTATED_CAP * qo) | (well & (e > RESTATED_CAP * eo))
    return int(bad.sum()), g


# ---------------------------------------------------------------------------- inputs shared by the two test files
def smooth_field(w, h, seed=0, amp=1.5):
    """A smooth field of +-amp px."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ph = 0.7 * seed
    f = np.stack([np.sin(xs / 7.0 + ph) * np.cos(ys / 11.0), np.cos(xs / 9.0 + ys / 5.0 + ph)], -1)
    return (amp * f).astype(np.float32)


def outlier_field(w, h, seed=0):
    """smooth_field with 2 % of the pixels at +-3 .. +-40 px (finite): beyond the fused kernel's LDS window (|flow| >= D), some
    of them out of the image, from border tiles and from interior ones."""
    rng = np.random.RandomState(100 + seed)
    f = smooth_field(w, h, seed).copy()
    n = max(1, (w * h) // 50)
    idx = rng.choice(w * h, n, replace=False)
    mag = rng.uniform(3.0, 40.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    f.reshape(-1, 2)[idx] = mag.astype(np.float32)
    return f


def whole_pixel_field(w, h, seed=0):
    """p + flow on whole pixels everywhere (fractions exactly 0), with the last column and the last row as targets: columns
    x >= w/2 point at x = w - 1, rows y >= h/2 at y = h - 1 (floor = w - 1: outside the bilinear footprint), the rest at
    whole displacements of -2 .. 2."""
    rng = np.random.RandomState(200 + seed)
    f = rng.randint(-2, 3, (h, w, 2)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    right = (xs >= w // 2) & ((xs + ys) % 3 == 0)
    low = (ys >= h // 2) & ((xs + ys) % 3 == 1)
    f[..., 0] = np.where(right, (w - 1 - xs), f[..., 0])
    f[..., 1] = np.where(low, (h - 1 - ys), f[..., 1])
    return f.astype(np.float32)


FIELDS = {"zeros": lambda w, h, seed=0: None, "smooth": smooth_field, "outliers": outlier_field, "whole": whole_pixel_field}


def surf_R(orc, w, h, seed=21, n=15, sigma=1.2):
    """(R0, R1) of two surf-clip frames at w x h by the C++ oracle (float32), for the stage entry."""
    from ripcurrents_amd import synth
    clip = synth.surf_clip(max(w, 8), max(h, 8), 2, seed=seed)[:, :h, :w]
    I0 = orc.pyr_level(np.ascontiguousarray(clip[0]), 0.0, 3, w, h)
    I1 = orc.pyr_level(np.ascontiguousarray(clip[1]), 0.0, 3, w, h)
    return orc.polyexp(I0, n, sigma), orc.polyexp(I1, n, sigma)


# ---------------------------------------------------------------------------- the committed cases
# 1x1 .. 9x1000: lower or narrower than a window radius; 27x29 .. 57x41: one 28-wide tile of the fused kernel plus or minus
# one, one 32-wide tile plus one; 65x33: one 64 x 32 tile plus one each way; 97x70, 130x67, 131x71, 333x251: several tiles,
# ragged both ways (64-, 32- and 28-wide tiles, 12- / 16- / 20- / 28- / 32-row tiles)
SIZES = [(1, 1), (2, 200), (200, 2), (9, 1000), (27, 29), (28, 28), (29, 13), (33, 47), (57, 41), (65, 33), (97, 70), (130, 67), (131, 71),
         (333, 251)]
SIZES_FUSED = [s for s in SIZES if s[0] >= 27 and s[1] >= 13]

# name -> (winsize, flags, option ablate, the kernel rcflow_debug_flow_form must report)
STAGE_FORMS = {
    "w3 box": (3, 0, 0, "w3"), "w3 gauss": (3, 256, 0, "w3"), "w3 box winsize 2": (2, 0, 0, "w3"), "w3 gauss winsize 2": (2, 256, 0, "w3"),
    "big m2 box": (5, 0, 0, "big"), "big m2 gauss": (4, 256, 0, "big"),
    "big m5 box": (10, 0, 0, "big"), "big m5 gauss": (11, 256, 0, "big"),
    "big m10 box": (21, 0, 0, "big"), "big m10 gauss": (20, 256, 0, "big"),
    "sweep m5": (10, 256, 8388608, "sweep"), "sweep m10": (20, 256, 8388608, "sweep"),
}
for _ws in (1, 7, 9, 15, 31, 49):
    STAGE_FORMS["runtime box %d" % _ws] = (_ws, 0, 0, "runtime")
    STAGE_FORMS["runtime gauss %d" % _ws] = (_ws, 256, 0, "runtime")


def yardstick_window(winsize, flags):
    """The window the C++ oracle is run with to set a case's bars: the case's own, except for the box window of winsize 1.
    There m = 0 and both windows are the identity, which is what the kernels and the reference compute; upstream's running
    sums (FarnebackUpdateFlow_Blur) start from (m + 2) x row 0 and come out as a two-row, two-column sum at m = 0, another
    operation (tests/test_flow_forms_ref.py pins that).  The Gaussian statement of the same identity window is the yardstick."""
    return (winsize, 256) if winsize == 1 else (winsize, flags)


# Forms whose correct float32 arithmetic needs more than FACTOR, shown from the reference side: restate_pointwise_f32 (numpy
# float32 in the kernels' operation order, CPU) against the same oracle yardstick.  At winsize 1 the solve is pointwise, the
# population with det > 1e-2 of a 29 x 13 field is a few dozen pixels, and the maximum of so few errors of either float32
# statement is a coarse statistic: the restatement is 4.55x the oracle's on the whole-pixel field there (1.13x the ulp floor)
# and at most 3.1x on every other committed case.  5 is the next integer; tests/test_flow_forms_ref.py asserts that the
# restatement passes at 5 and misses at 4.
FORM_FACTOR = {"runtime box 1": 5.0, "runtime gauss 1": 5.0}


def factor_of(form):
    return FORM_FACTOR.get(form, FACTOR)


# launches fed from the coarser scale (two-image calls, levels = 1): (w, h, pyr_scale).  0.5 on even sizes is the exact 2:1
# form (up_exact2), 0.5 on odd sizes and the other ratios the general one.
UP_CASES = [(98, 70, 0.5), (130, 68, 0.5), (332, 252, 0.5), (97, 70, 0.5), (131, 71, 0.5), (333, 251, 0.5),
            (97, 70, 0.6), (131, 71, 0.75), (333, 251, 0.8), (130, 67, 0.75), (333, 251, 0.6)]


# ---------------------------------------------------------------------------- float32 restatement of the kernels' matrix step
def _fma(a, b, c):
    """fused multiply-add in float32: the product of two float32 is exact in float64, the sum is rounded once there and once to
    float32 (a double rounding differs from a true fma in about one case in 2^29)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def restate_matrices_f32(R0, R1, flow_in):
    """FarnebackUpdateMatrices in the fast kernels' own float32 operation order (rc_matrices_reg of flow_iter_kernels.hip: the R
    planes at their stored half / quarter scale, four fused multiply-adds per bilinear coefficient starting from the stored R0,
    fused sums of products): h x w x 5 float32.  Reference-side evidence only -- nothing here reads a kernel's output."""
    R0 = np.ascontiguousarray(R0, np.float32)
    R1 = np.ascontiguousarray(R1, np.float32)
    h, w = R0.shape[:2]
    f32 = np.float32
    fin = np.zeros((h, w, 2), f32) if flow_in is None else np.ascontiguousarray(flow_in, f32)
    st = np.array([0.5, 0.5, 0.5, 0.5, 0.25], f32)
    S0, S1 = R0 * st, R1 * st
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dx, dy = fin[..., 0], fin[..., 1]
    fx, fy = xs.astype(f32) + dx, ys.astype(f32) + dy
    x1, y1 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    ax, ay = fx - x1.astype(f32), fy - y1.astype(f32)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xc, yc = np.clip(x1, 0, max(w - 2, 0)), np.clip(y1, 0, max(h - 2, 0))
    xd, yd = np.minimum(xc + 1, w - 1), np.minimum(yc + 1, h - 1)
    hx0, fy0 = f32(1) - ax, f32(1) - ay
    h00, h01, h10, h11 = hx0 * fy0, ax * fy0, hx0 * ay, ax * ay
    r = []
    for c in range(5):
        sg = f32(-1) if c < 2 else f32(1)
        v = _fma(sg * h00, S1[yc, xc, c], S0[..., c])
        v = _fma(sg * h01, S1[yc, xd, c], v)
        v = _fma(sg * h10, S1[yd, xc, c], v)
        v = _fma(sg * h11, S1[yd, xd, c], v)
        r.append(np.where(inside, v, S0[..., c] * (f32(1) if c < 2 else f32(2))).astype(f32))
    r2, r3, r4, r5, r6 = r
    r2 = _fma(r6, dx, _fma(r4, dy, r2))
    r3 = _fma(r5, dx, _fma(r6, dy, r3))
    X, Y = xs, ys
    one = np.ones((h, w), f32)
    bl = np.where(X < 5, np.where(X < 2, f32(0.14), f32(0.4472)), one)
    br = np.where(X >= w - 5, np.where(w - X - 1 < 2, f32(0.14), f32(0.4472)), one)
    bt = np.where(Y < 5, np.where(Y < 2, f32(0.14), f32(0.4472)), one)
    bb = np.where(Y >= h - 5, np.where(h - Y - 1 < 2, f32(0.14), f32(0.4472)), one)
    u32 = lambda v: np.asarray(v, np.int64) % (1 << 32)
    scale = np.where((u32(X - 5) >= u32(w - 10)) | (u32(Y - 5) >= u32(h - 10)), ((bl * br).astype(f32) * bt).astype(f32) * bb, one).astype(f32)
    r2, r3, r4, r5, r6 = [(v * scale).astype(f32) for v in (r2, r3, r4, r5, r6)]
    M = np.empty((h, w, 5), f32)
    M[..., 0] = _fma(r4, r4, r6 * r6)
    M[..., 1] = (r4 + r5) * r6
    M[..., 2] = _fma(r5, r5, r6 * r6)
    M[..., 3] = _fma(r4, r2, r6 * r3)
    M[..., 4] = _fma(r6, r2, r5 * r3)
    return M


def restate_pointwise_f32(R0, R1, flow_in):
    """One launch at winsize 1 (m = 0: the window is the pixel itself, weight 1, box or Gaussian) in the kernels' order: the
    float32 matrices above, then rc_solve in double, stored as float32."""
    g = restate_matrices_f32(R0, R1, flow_in).astype(np.float64)
    idet = 1.0 / (g[..., 0] * g[..., 2] - g[..., 1] * g[..., 1] + 1e-3)
    out = np.empty(g.shape[:2] + (2,), np.float32)
    out[..., 0] = ((g[..., 0] * g[..., 4] - g[..., 1] * g[..., 3]) * idet).astype(np.float32)
    out[..., 1] = ((g[..., 2] * g[..., 3] - g[..., 1] * g[..., 4]) * idet).astype(np.float32)
    return out


def _dop(a, b, c, d):
    """a b - c d by Kahan's scheme in float32 (rc_diff_of_products)."""
    w = (c * d).astype(np.float32)
    e = _fma(-c, d, w)
    f = _fma(a, b, -w)
    return (f + e).astype(np.float32)


def restate_w3_box_f32(R0, R1, flow_in, winsize=3):
    """One launch of the winsize-3 (or 2) box form in the kernels' order (k_flow_iter_w3, k_flow_iter2_rrc): the float32 matrices
    above, the 3 x 3 window as float32 sums -- centre + (below + above) per column, then (centre + left) + right -- on the
    replicated border, and rc_solve3: differences of products by Kahan's scheme, eps = 1e-3 winsize^4 on the unscaled sums, a
    float32 reciprocal."""
    f32 = np.float32
    M = restate_matrices_f32(R0, R1, flow_in)
    P = np.pad(M, ((1, 1), (1, 1), (0, 0)), mode="edge")
    V = (P[1:-1] + (P[2:] + P[:-2]).astype(f32)).astype(f32)                  # h x (w + 2) x 5
    g = ((V[:, 1:-1] + V[:, :-2]).astype(f32) + V[:, 2:]).astype(f32)
    eps = f32(1e-3 / (1.0 / (float(winsize) * winsize)) ** 2)
    det = (_dop(g[..., 0], g[..., 2], g[..., 1], g[..., 1]) + eps).astype(f32)
    nx = _dop(g[..., 0], g[..., 4], g[..., 1], g[..., 3])
    ny = _dop(g[..., 2], g[..., 3], g[..., 1], g[..., 4])
    idet = (f32(1) / det).astype(f32)
    return np.stack([(nx * idet).astype(f32), (ny * idet).astype(f32)], -1)
