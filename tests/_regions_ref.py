"""numpy statement of the rip regions (rcflow_regions_*), written from the contract in include/rcflow.h, not from the
kernels: runs per row, a union-find over the runs of adjacent rows, numbering by first pixel, the area filter, the
records, the summary, the derived values and the primitives.  Integers are int64 throughout."""
import numpy as np

REGION = np.dtype([("label", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                   ("first_x", "<i4"), ("first_y", "<i4"), ("edges", "<i4"), ("bad", "<i4"),
                   ("sx", "<i8"), ("sy", "<i8"), ("sxx", "<i8"), ("syy", "<i8"), ("sxy", "<i8"), ("fx", "<i8"), ("fy", "<i8"),
                   ("cx", "<f8"), ("cy", "<f8"), ("var_major", "<f8"), ("var_minor", "<f8"), ("angle", "<f8"),
                   ("mean_fx", "<f4"), ("mean_fy", "<f4")])
INT_FIELDS = ("label", "area", "x0", "y0", "x1", "y1", "first_x", "first_y", "edges", "bad", "sx", "sy", "sxx", "syy", "sxy", "fx", "fy")
FLOAT_FIELDS = ("cx", "cy", "var_major", "var_minor", "angle", "mean_fx", "mean_fy")
PRIM = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"),
                 ("color", "<u4"), ("flags", "<u4")])
DISC, LINE = 1, 2
QMAX = 2.0 ** 40


def runs_of(fg):
    """the runs of a bool h x w array in raster order -> (row, start, end exclusive) int64 arrays"""
    h, w = fg.shape
    p = np.zeros((h, w + 2), np.int8)
    p[:, 1:-1] = fg
    d = np.diff(p, axis=1)
    ys, xs = np.nonzero(d == 1)
    ye, xe = np.nonzero(d == -1)
    assert np.array_equal(ys, ye)
    return ys.astype(np.int64), xs.astype(np.int64), xe.astype(np.int64)


def label_runs(ry, xs, xe, w, connectivity):
    """union-find over the runs: runs of adjacent rows that touch (4: share a column; 8: also diagonally) are one set.
    Returns for every run the index of the first run (raster order) of its set."""
    n = len(ry)
    lab = np.arange(n, dtype=np.int64)
    if n == 0:
        return lab
    c = 1 if connectivity == 8 else 0
    W = w + 4
    kend, kstart = ry * W + xe + 1, ry * W + xs + 1
    # run b touches the runs a of the row above with xe_a > xs_b - c and xs_a < xe_b + c: a contiguous range
    lo = np.searchsorted(kend, (ry - 1) * W + xs - c + 1, side="right")
    hi = np.searchsorted(kstart, (ry - 1) * W + xe + c + 1, side="left")
    cnt = np.maximum(hi - lo, 0)
    b = np.repeat(np.arange(n, dtype=np.int64), cnt)
    a = np.repeat(lo, cnt) + (np.arange(cnt.sum(), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    assert (ry[a] == ry[b] - 1).all()
    while True:
        ra, rb = lab[a], lab[b]
        d = ra != rb
        if not d.any():
            return lab
        np.minimum.at(lab, np.maximum(ra, rb)[d], np.minimum(ra, rb)[d])     # hook the later root under the earlier one
        while True:                                                           # every run points at its root again
            nl = lab[lab]
            if np.array_equal(nl, lab):
                break
            lab = nl


def _s1(n):
    return n * (n + 1) // 2


def _s2(n):
    return n * (n + 1) * (2 * n + 1) // 6


def flow_q(flow):
    """the fixed point of rcflow_ripmap_*: (qx, qy int64, bad bool) per pixel"""
    f = np.asarray(flow, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = f * np.float32(65536.0)
        ok = (np.abs(s) <= np.float32(QMAX)).all(-1)                          # NaN and Inf fail the comparison
        q = np.rint(np.where(ok[..., None], s, np.float32(0))).astype(np.int64)
    return q[..., 0], q[..., 1], ~ok


def derive(rec):
    """the derived part of the records, in double, each operation rounded on its own, in the header's order"""
    n = rec["area"].astype(np.float64)
    m = (rec["area"] - rec["bad"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cx, cy = rec["sx"].astype(np.float64) / n, rec["sy"].astype(np.float64) / n
        rec["cx"], rec["cy"] = cx, cy
        rec["mean_fx"] = np.where(m > 0, (rec["fx"].astype(np.float64) / 65536.0 / m), 0.0).astype(np.float32)
        rec["mean_fy"] = np.where(m > 0, (rec["fy"].astype(np.float64) / 65536.0 / m), 0.0).astype(np.float32)
        mxx = rec["sxx"].astype(np.float64) / n - cx * cx
        myy = rec["syy"].astype(np.float64) / n - cy * cy
        mxy = rec["sxy"].astype(np.float64) / n - cx * cy
    t, d = (mxx + myy) * 0.5, (mxx - myy) * 0.5
    r = np.sqrt(d * d + mxy * mxy)
    rec["var_major"], rec["var_minor"] = t + r, t - r
    ang = np.arctan2(mxy, d) * 0.5 * (180.0 / np.pi)
    ang = np.where(ang < 0, ang + 180.0, ang)
    rec["angle"] = np.where(ang >= 180.0, 0.0, ang)
    return rec


def regions(mask, connectivity=8, min_area=1, max_regions=1024, flow=None, pushes=1):
    """-> dict(labels int32 h x w, mask_out uint8, records (max_regions REGION, zero beyond the written ones), summary 8 int64,
    K, all_records (every kept component, also beyond max_regions))"""
    mask = np.asarray(mask)
    h, w = mask.shape
    fg = mask != 0
    ry, xs, xe = runs_of(fg)
    root = label_runs(ry, xs, xe, w, connectivity)
    roots, comp = np.unique(root, return_inverse=True)                        # ascending run index = raster order of first pixels
    ncomp = len(roots)
    ln = xe - xs
    area = np.zeros(ncomp, np.int64)
    np.add.at(area, comp, ln)
    keep = area >= min_area
    K = int(keep.sum())
    number = np.where(keep, np.cumsum(keep), 0).astype(np.int64)              # kept number of a component, 0 when dropped
    labels = np.zeros(h * w, np.int32)
    labels[np.flatnonzero(fg.reshape(-1))] = np.repeat(number[comp], ln)      # the runs cover the foreground in raster order
    labels = labels.reshape(h, w)
    rec = np.zeros(K, REGION)
    kr = keep[comp]                                                           # runs of kept components
    k = number[comp][kr] - 1
    y_, a_, b_, n_ = ry[kr], xs[kr], xe[kr], ln[kr]
    rec["label"] = np.arange(1, K + 1)
    rec["area"] = area[keep]
    fr = roots[keep]
    rec["first_x"], rec["first_y"] = xs[fr], ry[fr]
    for name, val, fn, init in (("x0", a_, np.minimum, w), ("y0", y_, np.minimum, h), ("x1", b_ - 1, np.maximum, -1), ("y1", y_, np.maximum, -1)):
        v = np.full(K, init, np.int64)
        fn.at(v, k, val)
        rec[name] = v
    rec["edges"] = (rec["x0"] == 0) * 1 + (rec["y0"] == 0) * 2 + (rec["x1"] == w - 1) * 4 + (rec["y1"] == h - 1) * 8
    sumx = _s1(b_ - 1) - _s1(a_ - 1)
    for name, val in (("sx", sumx), ("sy", y_ * n_), ("sxx", _s2(b_ - 1) - _s2(a_ - 1)), ("syy", y_ * y_ * n_), ("sxy", y_ * sumx)):
        v = np.zeros(K, np.int64)
        np.add.at(v, k, val)
        rec[name] = v
    bad_total = 0
    if flow is not None:
        qx, qy, bad = flow_q(flow)
        sel = labels > 0
        kk = labels[sel].astype(np.int64) - 1
        good = ~bad[sel]
        for name, q in (("fx", qx), ("fy", qy)):
            v = np.zeros(K, np.int64)
            np.add.at(v, kk[good], q[sel][good])
            rec[name] = v
        v = np.zeros(K, np.int64)
        np.add.at(v, kk[~good], 1)
        rec["bad"] = v
        bad_total = int(v.sum())
    derive(rec)
    nrec = min(K, max_regions)
    out = np.zeros(max_regions, REGION)
    out[:nrec] = rec[:nrec]
    summary = np.array([ncomp, K, nrec, int(fg.sum()), int(area[keep].sum()), bad_total, pushes, int(area[keep].max()) if K else 0], np.int64)
    return dict(labels=labels, mask_out=np.where(labels > 0, 255, 0).astype(np.uint8), records=out, summary=summary, K=K, all_records=rec)


def _step(mean, scale):
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(mean * scale)
    ok = np.abs(v) <= 2.0 ** 30
    return np.where(ok, np.where(ok, v, 0).astype(np.int64), -2 ** 31), ok


def prims(records, color=0x00ffff, thickness=1, disc_radius=3, flow_scale=0.0):
    """the 6 primitives per record slot of rcflow_regions_prims_dev"""
    q = np.asarray(records)
    out = np.zeros((len(q), 6), PRIM)
    live = q["label"] != 0
    x0, y0, x1, y1 = (q[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1"))
    for j, (a, b, c, d) in enumerate(((x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0))):
        out["kind"][:, j], out["size"][:, j], out["color"][:, j] = LINE, thickness, color
        out["x0"][:, j], out["y0"][:, j], out["x1"][:, j], out["y1"][:, j] = a, b, c, d
    n = np.maximum(q["area"].astype(np.int64), 1)
    px, py = (2 * q["sx"] + n) // (2 * n), (2 * q["sy"] + n) // (2 * n)
    out["kind"][:, 4], out["size"][:, 4], out["color"][:, 4] = DISC, disc_radius, color
    out["x0"][:, 4] = out["x1"][:, 4] = px
    out["y0"][:, 4] = out["y1"][:, 4] = py
    m = (q["area"] - q["bad"]).astype(np.int64)
    if flow_scale != 0.0:
        md = np.maximum(m, 1).astype(np.float64)
        (dx, okx), (dy, oky) = _step(q["fx"].astype(np.float64) / 65536.0 / md, flow_scale), _step(q["fy"].astype(np.float64) / 65536.0 / md, flow_scale)
        out["kind"][:, 5], out["size"][:, 5], out["color"][:, 5] = LINE, thickness, color
        out["x0"][:, 5], out["y0"][:, 5] = px, py
        out["x1"][:, 5], out["y1"][:, 5] = np.where(okx, px + dx, -2 ** 31), np.where(oky, py + dy, -2 ** 31)
        out[~(m > 0), 5] = np.zeros((), PRIM)
    out[~live] = np.zeros((), PRIM)
    return out.reshape(-1)


def flood(mask, connectivity):
    """brute force: labels by raster-order flood fill (small masks only)"""
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    lab = np.zeros((h, w), np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    n = 0
    for y in range(h):
        for x in range(w):
            if fg[y, x] and not lab[y, x]:
                n += 1
                lab[y, x] = n
                stack = [(y, x)]
                while stack:
                    cy, cx = stack.pop()
                    for dy, dx in nb:
                        yy, xx = cy + dy, cx + dx
                        if 0 <= yy < h and 0 <= xx < w and fg[yy, xx] and not lab[yy, xx]:
                            lab[yy, xx] = n
                            stack.append((yy, xx))
    return lab
