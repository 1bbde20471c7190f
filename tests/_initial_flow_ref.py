"""Reference for OPTFLOW_USE_INITIAL_FLOW (tests/test_initial_flow.py, tests/test_gpu_initial_flow.py).

Two pieces, both test infrastructure:

  area_reduce   a numpy fp32 restatement of resize(flow0, Size(wk, hk), INTER_AREA) on CV_32FC2 followed by
                `*= (float)pyr_scale^k`, in the operation order include/rcflow.h and DESIGN.md section 2 state
                (imgproc/resize.cpp, scalar code path: resizeAreaFast_ for integer ratios, resizeArea_ with the
                computeResizeAreaTab tables otherwise);
  farneback     FarnebackOpticalFlowImpl::calc composed from the oracle's stage functions, following
                orc_farneback_u8_ex's level loop, with the coarsest scale started from the reduced field.

PARITY UNPINNED like the oracle itself: no OpenCV exists here to run the flag against.
"""
import math

import numpy as np

USE_INITIAL_FLOW = 4
GAUSSIAN = 256
DBL_EPSILON = 2.220446049250313e-16


def area_tab(ssize, dsize, scale):
    """computeResizeAreaTab grouped by destination index: (start[dsize + 1], si[], alpha[] float32)."""
    start, si, alpha = [], [], []
    for dx in range(dsize):
        start.append(len(si))
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(math.ceil(fsx1)), int(math.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            si.append(sx1 - 1)
            alpha.append((sx1 - fsx1) / cell)
        for sx in range(sx1, sx2):
            si.append(sx)
            alpha.append(1.0 / cell)
        if fsx2 - sx2 > 1e-3:
            si.append(sx2)
            alpha.append(min(min(fsx2 - sx2, 1.0), cell) / cell)
    start.append(len(si))
    return np.array(start), np.array(si), np.array(alpha, np.float64).astype(np.float32)


def area_resize(src, dw, dh):
    """resize(src, Size(dw, dh), INTER_AREA) of an H x W x C float32 image, shrinking only, fp32 in upstream's order."""
    src = np.asarray(src, np.float32)
    H, W = src.shape[:2]
    assert dw <= W and dh <= H
    scale_x, scale_y = W / dw, H / dh
    ix, iy = int(round(scale_x)), int(round(scale_y))
    if abs(scale_x - ix) < DBL_EPSILON and abs(scale_y - iy) < DBL_EPSILON:
        # resizeAreaFast_: sum over the iy x ix block in row-major order, then * (1.f / area)
        s = None
        for ky in range(iy):
            for kx in range(ix):
                v = src[ky::iy, kx::ix][:dh, :dw]
                s = v.copy() if s is None else s + v
        return s * np.float32(np.float32(1.0) / np.float32(ix * iy))
    xs, xi, xa = area_tab(W, dw, scale_x)
    ys, yi, ya = area_tab(H, dh, scale_y)
    # per source row: buf = sum_k S[xsi[k]] * xalpha[k] in table order
    buf = np.zeros((H, dw) + src.shape[2:], np.float32)
    ntap = np.diff(xs)
    for t in range(int(ntap.max())):
        m = ntap > t
        k = xs[:-1][m] + t
        al = xa[k].reshape((1, -1) + (1,) * (src.ndim - 2))
        buf[:, m] = buf[:, m] + src[:, xi[k]] * al
    # per output row: sum = beta * buf for its first source row, sum += beta * buf after it
    out = np.zeros((dh, dw) + src.shape[2:], np.float32)
    ntap = np.diff(ys)
    for t in range(int(ntap.max())):
        m = ntap > t
        j = ys[:-1][m] + t
        beta = ya[j].reshape((-1, 1) + (1,) * (src.ndim - 2))
        term = beta * buf[yi[j]]
        out[m] = term if t == 0 else out[m] + term
    return out


def seed_scale(pyr_scale, k):
    scale = 1.0
    for _ in range(k):
        scale *= pyr_scale
    return np.float32(scale)


def area_reduce(flow0, wk, hk, pyr_scale, k):
    """The initial field at the coarsest scale k: INTER_AREA reduction, then one fp32 multiply by pyr_scale^k."""
    return area_resize(flow0, wk, hk) * seed_scale(pyr_scale, k)


def farneback(orc, prev, nxt, pyr_scale=0.5, levels=2, winsize=3, iterations=2, poly_n=15, poly_sigma=1.2, flags=0,
              flow0=None):
    """calc() composed from the oracle's stages; flow0 (H x W x 2) is used when flags has USE_INITIAL_FLOW."""
    prev = np.ascontiguousarray(prev, np.uint8)
    nxt = np.ascontiguousarray(nxt, np.uint8)
    h, w = prev.shape
    L = orc.level_geometry(w, h, pyr_scale, levels, 0)["levels"]
    gaussian = bool(flags & GAUSSIAN)
    prev_flow = None
    for k in range(L, -1, -1):
        g = orc.level_geometry(w, h, pyr_scale, levels, k)
        gw, gh = g["w"], g["h"]
        if prev_flow is not None:
            flow = orc.resize_linear(prev_flow, gw, gh) * np.float32(1.0 / pyr_scale)
        elif flags & USE_INITIAL_FLOW:
            flow = area_reduce(flow0, gw, gh, pyr_scale, k)
        else:
            flow = np.zeros((gh, gw, 2), np.float32)
        flow = np.ascontiguousarray(flow, np.float32)
        R = [orc.polyexp(orc.pyr_level(img, g["sigma"], g["ksize"], gw, gh), poly_n, poly_sigma) for img in (prev, nxt)]
        M = orc.update_matrices(R[0], R[1], flow)
        for i in range(iterations):
            orc.update_flow(R[0], R[1], flow, M, winsize, i < iterations - 1, gaussian)
        prev_flow = flow
    return prev_flow


def smooth_field(w, h, seed, amplitude=3.0):
    """A smooth random flow field of a few pixels (sum of a few long sinusoids), H x W x 2 float32."""
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.zeros((h, w, 2), np.float64)
    for c in range(2):
        for _ in range(4):
            lam = rng.uniform(0.3, 1.5) * max(w, h)
            th = rng.uniform(0, 2 * math.pi)
            out[..., c] += rng.uniform(-1, 1) * np.sin(2 * math.pi * (xs * math.cos(th) + ys * math.sin(th)) / lam + rng.uniform(0, 6.28))
    return (out * (amplitude / 2.0)).astype(np.float32)


def endpoint_error(flow, u, v):
    return np.hypot(flow[..., 0].astype(np.float64) - u, flow[..., 1].astype(np.float64) - v)
