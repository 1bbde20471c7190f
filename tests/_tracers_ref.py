"""numpy statement of the tracer sessions (rcflow_tracers_*) and of the painting rules of rcflow_draw_dev, written from
the contract in include/rcflow.h and from the reference's drawing calls (Streakline.cpp:35-66,
ripcurrents_module.cpp:794-805, :1175-1194), not from the kernels.  Everything is integer arithmetic in Python / int64."""
import numpy as np

DISC, LINE, BLEND = 1, 2, 1
COORD_MAX, MAX_THICKNESS = 16383, 8
PRIM = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"),
                 ("color", "<u4"), ("flags", "<u4")])
GREEN, BLUE, RED = 100 << 8, 100, 100 << 16      # CV_RGB(0,100,0), CV_RGB(0,0,100), CV_RGB(100,0,0) as b | g << 8 | r << 16
STREAK, TIMELINE, CLOUD = 0, 1, 2


def prim(kind, x0, y0, x1=0, y1=0, size=1, color=0xffffff, flags=0):
    p = np.zeros(1, PRIM)
    p[0] = (kind, x0, y0, x1, y1, size, color, flags)
    return p


def disc(x, y, r, color=0xffffff, flags=0):
    return prim(DISC, x, y, x, y, r, color, flags)


def line(x0, y0, x1, y1, t=1, color=0xffffff):
    return prim(LINE, x0, y0, x1, y1, t, color, 0)


def valid(p):
    """False: the primitive is skipped and counted."""
    ok = abs(int(p["x0"])) <= COORD_MAX and abs(int(p["y0"])) <= COORD_MAX
    if p["kind"] == DISC:
        return ok and 0 <= p["size"] <= COORD_MAX
    if p["kind"] != LINE:
        return False
    return ok and abs(int(p["x1"])) <= COORD_MAX and abs(int(p["y1"])) <= COORD_MAX and 1 <= p["size"] <= MAX_THICKNESS


def mask(p, w, h):
    """bool h x w: the pixels a valid primitive lights."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    x0, y0, x1, y1, s = (int(p[k]) for k in ("x0", "y0", "x1", "y1", "size"))
    px, py = xs - x0, ys - y0
    if p["kind"] == DISC:
        return px * px + py * py <= s * s + s
    bx, by = x1 - x0, y1 - y0
    if s == 1:
        adx, ady = abs(bx), abs(by)
        if adx == 0 and ady == 0:
            return (px == 0) & (py == 0)
        if adx >= ady:
            t = np.abs(px)
            inside = (np.sign(px) * np.sign(bx) >= 0) & (t <= adx)
            y = y0 + int(np.sign(by)) * ((2 * ady * t + adx) // (2 * adx))
            return inside & (ys == y)
        t = np.abs(py)
        inside = (np.sign(py) * np.sign(by) >= 0) & (t <= ady)
        x = x0 + int(np.sign(bx)) * ((2 * adx * t + ady) // (2 * ady))
        return inside & (xs == x)
    # thick: exact squared distance to the segment against (t / 2)^2; Python integers where int64 could overflow
    tt, bb = s * s, bx * bx + by * by
    dot = px * bx + py * by
    cross = px * by - py * bx
    near = 4 * (px * px + py * py) <= tt
    far = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= tt
    if np.abs(cross).max() < 2 ** 30:                             # 4 c^2 stays inside int64
        mid = 4 * cross * cross <= tt * bb
    else:
        mid = np.frompyfunc(lambda c: 4 * c * c <= tt * bb, 1, 1)(cross.astype(object)).astype(bool)
    return np.where(dot <= 0, near, np.where(dot >= bb, far, mid))


def blend(c, p):
    """cvRound(0.5 c + 0.5 p), half to even, on uint8 arrays"""
    s = c.astype(np.int32) + p.astype(np.int32)
    hs = s >> 1
    return np.where(s & 1, hs + (hs & 1), hs).astype(np.uint8)


def draw(img, prims):
    """Paints in place into a h x w or h x w x 3 uint8 array; returns the number of skipped primitives."""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    skipped = 0
    for p in prims:
        if not valid(p):
            skipped += 1
            continue
        # the box first: a primitive off the image costs nothing
        g = int(p["size"]) if p["kind"] == DISC else int(p["size"]) // 2
        xa, xb = min(p["x0"], p["x1"]) - g, max(p["x0"], p["x1"]) + g
        ya, yb = min(p["y0"], p["y1"]) - g, max(p["y0"], p["y1"]) + g
        if xb < 0 or yb < 0 or xa >= w or ya >= h:
            continue
        xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, w - 1), min(yb, h - 1)
        q = p.copy()
        for k in ("x0", "x1"):
            q[k] = int(p[k]) - xa
        for k in ("y0", "y1"):
            q[k] = int(p[k]) - ya
        m = mask(q, xb - xa + 1, yb - ya + 1)
        view = img[ya:yb + 1, xa:xb + 1]
        col = np.array([(int(p["color"]) >> (8 * k)) & 255 for k in range(ch)], np.uint8)
        if ch == 1:
            view[m] = blend(col[0], view[m]) if p["flags"] & BLEND else col[0]
        else:
            view[m] = blend(col[None, :], view[m]) if p["flags"] & BLEND else col[None, :]
    return skipped


def trunc_i32(v):
    """Point(float, float): truncation toward zero; INT32_MIN for what int32 cannot hold (cvtt on x86)"""
    v = np.asarray(v, np.float32)
    ok = np.isfinite(v) & (v >= -2147483648.0) & (v < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64), -2147483648).astype(np.int32)


def round_i32(v):
    """cvRound: half to even; INT32_MIN for what int32 cannot hold"""
    v = np.asarray(v, np.float32)
    r = np.rint(v)
    ok = np.isfinite(r) & (r >= -2147483648.0) & (r < 2147483648.0)
    return np.where(ok, np.where(ok, r, 0).astype(np.int64), -2147483648).astype(np.int32)


def trace_prims(trace, start=None, color=0xffffff):
    """the pathline overlay's cv::line(overlay, *pt, newpt, color, 1) per step, ends rounded"""
    trace = np.asarray(trace, np.float32)
    n, iters = trace.shape[:2]
    pts = trace if start is None else np.concatenate([np.asarray(start, np.float32).reshape(n, 1, 2), trace], 1)
    a, b = round_i32(pts[:, :-1]), round_i32(pts[:, 1:])
    out = np.zeros(a.shape[:2], PRIM)
    out["kind"], out["size"], out["color"] = LINE, 1, color
    out["x0"], out["y0"], out["x1"], out["y1"] = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    return out.reshape(-1)


class Line:
    def __init__(self, kind, xy, max_vertices):
        self.kind = kind
        self.first = np.asarray(xy, np.float32).reshape(-1, 2).copy()
        self.max_vertices = max_vertices
        self.reset()

    def reset(self):
        self.v = self.first.copy()       # the reference's order: a streakline newest first
        self.dropped = 0

    def step(self, moved, w, h):
        """moved: where the mover put self.v (same order)"""
        moved = np.asarray(moved, np.float32).reshape(-1, 2)
        if self.kind != STREAK:
            self.v = moved.copy()
            return
        d = np.abs(self.v - moved)                                   # float32 differences
        big = (d[:, 0].astype(np.float64) > w * 0.1) | (d[:, 1].astype(np.float64) > h * 0.1)
        nxt = np.where(big[:, None], self.v, moved)
        self.v = np.concatenate([self.first[:1], nxt], 0)            # vertices.insert(begin(), generationPoint)
        if len(self.v) > self.max_vertices:                          # the ring: the oldest vertex goes
            self.v = self.v[:self.max_vertices]
            self.dropped += 1

    def prims(self):
        v = trunc_i32(self.v)
        out = []
        if self.kind == STREAK:
            g = trunc_i32(self.first[0])
            out.append(disc(g[0], g[1], 3, GREEN))
            out.append(line(g[0], g[1], v[0, 0], v[0, 1], 1, RED))
            out.append(disc(v[0, 0], v[0, 1], 2, BLUE))
            for i in range(len(v) - 1):
                out.append(disc(v[i + 1, 0], v[i + 1, 1], 2, BLUE))
                out.append(line(v[i, 0], v[i, 1], v[i + 1, 0], v[i + 1, 1], 1, RED))
        elif self.kind == TIMELINE:
            out.append(disc(v[0, 0], v[0, 1], 4, BLUE))
            for i in range(len(v) - 1):
                out.append(line(v[i, 0], v[i, 1], v[i + 1, 0], v[i + 1, 1], 2, RED))
                out.append(disc(v[i + 1, 0], v[i + 1, 1], 4, BLUE))
        else:
            for p in v:
                out.append(disc(p[0], p[1], 10, RED, BLEND))
        return np.concatenate(out)


class Session:
    """The book-keeping of a tracer session; the mover is the caller's (a function from all vertices to moved ones)."""

    def __init__(self, w, h, max_vertices):
        self.w, self.h, self.max_vertices = w, h, max_vertices
        self.lines = []

    def add(self, kind, xy):
        self.lines.append(Line(kind, xy, self.max_vertices))
        return len(self.lines) - 1

    def reset(self):
        for ln in self.lines:
            ln.reset()

    def all_vertices(self):
        return np.concatenate([ln.v for ln in self.lines], 0)

    def push(self, moved_all):
        """moved_all: the moved positions of all_vertices(), in its order"""
        o = 0
        for ln in self.lines:
            n = len(ln.v)
            ln.step(moved_all[o:o + n], self.w, self.h)
            o += n

    def prims(self):
        return np.concatenate([ln.prims() for ln in self.lines])

    def draw(self, canvas):
        return draw(canvas, self.prims())
