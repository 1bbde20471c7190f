"""Sequential statement of the region outlines (rcflow_outlines_*), written from the contract in include/rcflow.h ("region outlines"),
not from the kernels: the cracks of a label plane, their successor, the loops by a plain walk from every leader, the filter, the caps,
the records, the vertices, the summary and the primitives.  No pointer jumping, no scan: one loop after the other, crack by crack.
Every value is an integer."""
import numpy as np

LOOP = np.dtype([("label", "<i4"), ("flags", "<i4"), ("x", "<i4"), ("y", "<i4"), ("cracks", "<i4"), ("verts", "<i4"), ("offset", "<i4"),
                 ("pad", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area2", "<i8")])
PRIM = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"), ("color", "<u4"), ("flags", "<u4")])
assert LOOP.itemsize == 56 and PRIM.itemsize == 32
HOLE, NOVERTS = 1, 2
LINE = 2
SUMMARY_WORDS = 8
MAX_SIDE = 16383
N, E, S, W = 0, 1, 2, 3
D = ((1, 0), (0, 1), (-1, 0), (0, -1))            # a crack's direction, by side
A = ((0, -1), (1, 0), (0, 1), (-1, 0))            # the step across it
FROM = ((0, 0), (1, 0), (1, 1), (0, 1))           # its first corner, from the pixel's (x, y)
TO = ((1, 0), (1, 1), (0, 1), (0, 0))             # its second corner


def plane_of(labels=None, mask=None):
    """exactly one of the two inputs -> the int64 label plane"""
    assert (labels is None) != (mask is None)
    return np.asarray(labels).astype(np.int64) if mask is None else (np.asarray(mask) != 0).astype(np.int64)


def cracks_of(lab):
    """-> the keys (y * w + x) * 4 + s of the cracks, ascending"""
    h, w = lab.shape
    keys = []
    for y in range(h):
        for x in range(w):
            L = lab[y, x]
            if not L:
                continue
            for s in range(4):
                xx, yy = x + A[s][0], y + A[s][1]
                if not (0 <= xx < w and 0 <= yy < h) or lab[yy, xx] != L:
                    keys.append((y * w + x) * 4 + s)
    return keys


def successor(lab, key, connectivity):
    h, w = lab.shape
    s, p = key & 3, key >> 2
    x, y = p % w, p // w
    L = lab[y, x]

    def same(xx, yy):
        return 0 <= xx < w and 0 <= yy < h and lab[yy, xx] == L

    rx, ry = x + D[s][0], y + D[s][1]
    lx, ly = rx + A[s][0], ry + A[s][1]
    left, straight, right = (ly * w + lx) * 4 + (s + 3) % 4, (ry * w + rx) * 4 + s, (y * w + x) * 4 + (s + 1) % 4
    if connectivity == 8:
        return left if same(lx, ly) else straight if same(rx, ry) else right
    return right if not same(rx, ry) else left if same(lx, ly) else straight


def corners(key, w):
    s, p = key & 3, key >> 2
    x, y = p % w, p // w
    return (x + FROM[s][0], y + FROM[s][1]), (x + TO[s][0], y + TO[s][1])


def loops_of(lab, connectivity):
    """every loop in the order of its leader's key: dict(leader, label, cracks, area2, verts (list of corners), box, keys (in rank order))"""
    h, w = lab.shape
    keys = cracks_of(lab)
    seen = set()
    out = []
    for k in keys:                                    # ascending: the first crack of a loop not yet walked is its leader
        if k in seen:
            continue
        walk, c = [], k
        while True:
            seen.add(c)
            walk.append(c)
            c = successor(lab, c, connectivity)
            if c == k:
                break
        assert min(walk) == k
        area2, verts = 0, []
        x0 = y0 = 1 << 30
        x1 = y1 = -1
        for i, c in enumerate(walk):
            (ax, ay), (bx, by) = corners(c, w)
            area2 += ax * by - bx * ay
            x0, y0, x1, y1 = min(x0, ax, bx), min(y0, ay, by), max(x1, ax, bx), max(y1, ay, by)
            if (walk[(i + 1) % len(walk)] & 3) != (c & 3):
                verts.append((bx, by))
        p = k >> 2
        out.append(dict(leader=k, label=int(lab[p // w, p % w]), cracks=len(walk), area2=area2, verts=verts, box=(x0, y0, x1, y1), keys=walk))
    return out, len(keys)


def outlines(labels=None, mask=None, connectivity=8, min_cracks=4, max_cracks=1 << 20, max_loops=1024, max_vertices=1 << 14, pushes=1):
    """-> dict(loops (max_loops LOOP, zero beyond the written ones), verts (max_vertices x 2 int32, zero beyond the written ones),
    summary 8 int64, next (per written vertex the index of its loop's next one), all (every loop before the filter))"""
    lab = plane_of(labels, mask)
    h, w = lab.shape
    recs, verts, nxt = np.zeros(max_loops, LOOP), np.zeros((max_vertices, 2), np.int32), []
    everything, ncracks = loops_of(lab, connectivity)
    summary = np.zeros(SUMMARY_WORDS, np.int64)
    summary[0], summary[7] = ncracks, pushes
    if ncracks > max_cracks:
        summary[6] = 1
        return dict(loops=recs, verts=verts, summary=summary, next=nxt, all=everything)
    kept = [q for q in everything if q["cracks"] >= min_cracks]
    offset = written = 0
    for i, q in enumerate(kept):
        nv = len(q["verts"])
        if i < max_loops:
            r = recs[i]
            p = q["leader"] >> 2
            r["label"], r["x"], r["y"], r["cracks"], r["verts"], r["area2"] = q["label"], p % w, p // w, q["cracks"], nv, q["area2"]
            r["x0"], r["y0"], r["x1"], r["y1"] = q["box"]
            r["flags"] = HOLE if q["area2"] < 0 else 0
            if offset + nv <= max_vertices:
                r["offset"] = offset
                verts[offset:offset + nv] = q["verts"]
                nxt += [offset + (j + 1) % nv for j in range(nv)]
                written = offset + nv
            else:
                r["offset"] = -1
                r["flags"] |= NOVERTS
        offset += nv
    summary[1:6] = len(everything), len(kept), min(len(kept), max_loops), offset, written
    return dict(loops=recs, verts=verts, summary=summary, next=nxt, all=everything)


def prims(out, w, h, color=0x00ffff, thickness=1):
    """the max_vertices primitives of rcflow_outlines_prims_dev from the result of outlines()"""
    v = out["verts"].astype(np.int64)
    p = np.zeros(len(v), PRIM)
    for i, j in enumerate(out["next"]):
        p[i] = (LINE, min(v[i, 0], w - 1), min(v[i, 1], h - 1), min(v[j, 0], w - 1), min(v[j, 1], h - 1), thickness, color, 0)
    return p


# ---------------------------------------------------------------------------- shapes for the tests
def random_labels(w, h, labels, seed, share=0.5):
    r = np.random.RandomState(seed)
    return np.where(r.rand(h, w) < share, r.randint(1, labels + 1, (h, w)), 0).astype(np.int32)


def checkerboard(w, h):
    y, x = np.mgrid[:h, :w]
    return ((x + y) % 2 == 0).astype(np.int32)


def rings(w, h):
    """nested square rings two pixels apart around the centre, labels 1"""
    y, x = np.mgrid[:h, :w]
    d = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y))
    return (d % 2 == 0).astype(np.int32)


def serpentine(w, h):
    """one 4-connected path of label 1 that fills every other row and turns at alternating ends: one loop, no hole"""
    lab = np.zeros((h, w), np.int32)
    lab[0::2, :] = 1
    for i, y in enumerate(range(1, h - 1, 2)):
        lab[y, w - 1 if i % 2 == 0 else 0] = 1
    return lab


def blobs(w, h, n, seed):
    """n discs of random place and size as a mask"""
    r = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        cx, cy, rad = r.randint(0, w), r.randint(0, h), r.randint(2, max(3, min(w, h) // 6))
        m |= (x - cx) ** 2 + (y - cy) ** 2 <= rad * rad
    return np.where(m, 255, 0).astype(np.uint8)
