"""The numpy statement of the plan view (tests/_planview_ref.py) against what it must mean: every class of cell occurs, a
uniform ground velocity comes back in metres per second, the exact cases are exact; and the library exports the entry points."""
import math

import numpy as np
import pytest

import _planview_ref as P
from _dev import bits

f32 = np.float32
W, H = 97, 53
DISTORTED = dict(k1=-0.12, k2=0.02)


# ---------------------------------------------------------------------------- the classes of cells
@pytest.mark.parametrize("dist", [{}, DISTORTED])
def test_every_class_of_cell_occurs(dist):
    """97 x 53, f = 90, 10 m up, 20 degrees down -> 61 x 37 cells of 1 x 1.5 m from (-30, -6), max_gsd 0.6.  This statement
    counts, of 2257 cells: behind the camera 183 | in front but outside the image 1272 (1238 distorted) | inside but over
    max_gsd 549 (582) | valid 253 (254)."""
    p = P.shore_camera(**dist)
    parts, tab = P.table_parts(p), P.table(p)
    inside = P.seen_cells(P.table(P.Params(**dict(p.kw(), max_gsd=math.inf))), W, H)      # the sampler's test without the cut
    behind = ~parts["front"]
    outside = parts["front"] & ~inside
    over = parts["front"] & inside & ~parts["usable"]
    r = P.push(tab, W, H, P.wavy_field(W, H), P.frame(W, H), 1)
    counts = [int(v.sum()) for v in (behind, outside, over, r["valid"])]
    print("behind %d, outside %d, over max_gsd %d, valid %d" % tuple(counts))
    assert all(c > 0 for c in counts) and sum(counts) == 61 * 37
    assert counts[0] == 183                                       # three rows of cells with a point at Y <= -3.64 m
    assert parts["unfolded"].all()                                # this distortion has no fold inside the plan
    # what the table holds for each class
    assert not tab[behind | over].any() and (tab[r["valid"]][:, 7] == 1).all()
    assert np.array_equal(r["seen"], r["valid"]) and np.array_equal(r["mask"] != 0, r["valid"])
    assert list(r["summary"]) == [int(parts["usable"].sum()), counts[3], counts[3], int(r["summary"][3]), 1, 0, 0, 0]
    assert (tab[r["valid"]][:, 6] <= f32(0.6)).all() and not r["bgr"][~r["seen"]].any() and r["bgr"][r["seen"]].any()
    assert not r["plan"][~r["valid"]].any()


def test_a_fold_of_the_distortion_is_cut():
    """a strong barrel distortion folds the image back on itself at r2 = 1 / (3 |k1|): cells past it are not usable"""
    p = P.shore_camera(k1=-1.5, max_gsd=math.inf)
    parts = P.table_parts(p)
    folded = parts["front"] & ~parts["unfolded"]
    assert folded.any() and parts["usable"].any() and not P.table(p)[folded].any()


# ---------------------------------------------------------------------------- a uniform ground velocity comes back
# what this statement measures (the bound is twice that: the margin covers another legitimate Newton tolerance only)
MEASURED = {(97, 53, False): 3.191e-4, (97, 53, True): 2.807e-4, (640, 480, False): 3.151e-5}


@pytest.mark.parametrize("w,h,f,nx,ny,dx,dy,gsd,dist", [
    (97, 53, 90.0, 61, 37, 1.0, 1.5, 0.6, False), (97, 53, 90.0, 61, 37, 1.0, 1.5, 0.6, True), (640, 480, 600.0, 244, 148, 0.25, 0.375, 0.09, False)])
def test_uniform_ground_velocity_is_recovered(w, h, f, nx, ny, dx, dy, gsd, dist):
    """(0.5, 0.2) m/s on the ground, projected into an image flow field through the camera (every pixel's ground point by
    Newton, the analytic Jacobian), comes back from the plan view; the errors left are the linearisation over one cell and
    the bilinear sample.  Largest error over the cells whose four taps are defined, against the analytic velocity, as
    measured with this statement: 97 x 53 3.191e-4 m/s, distorted 2.807e-4 m/s, 640 x 480 (f = 600, plan 244 x 148 in cells
    of 0.25 x 0.375 m, max_gsd 0.09) 3.151e-5 m/s.  The bound is twice that."""
    p = P.shore_camera(w, h, f, nx, ny, dx, dy, gsd, **(DISTORTED if dist else {}))
    flow = P.ground_flow_field(p, w, h, (0.5, 0.2))
    r = P.push(P.table(p), w, h, flow, None, 1)
    assert r["valid"].sum() >= 250
    err = np.hypot(r["plan"][..., 0].astype(np.float64) - 0.5, r["plan"][..., 1].astype(np.float64) - 0.2)[r["valid"]]
    print("%d x %d%s: %d valid cells, largest error %.4g m/s" % (w, h, " distorted" if dist else "", int(r["valid"].sum()), err.max()))
    assert err.max() <= 2 * MEASURED[(w, h, dist)]
    speed = float(np.array([r["summary"][3]], np.uint32).view(f32)[0]) ** 0.5
    assert abs(speed - math.hypot(0.5, 0.2)) <= 2 * MEASURED[(w, h, dist)]


# ---------------------------------------------------------------------------- exact cases
def test_half_scale_is_exact():
    """H = diag(2, 2, 1), unit cells, fps 1: cell (i, j) looks at pixel (2 i, 2 j), an integer, and its velocity is exactly
    half the field there"""
    w, h, nx, ny = 40, 30, 19, 14
    p = P.Params(np.diag([2.0, 2.0, 1.0]), 1.0, 1.0, 0.0, 0.0, nx=nx, ny=ny)
    tab = P.table(p)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    usable = tab[..., 7] == 1
    assert usable.all()
    assert np.array_equal(tab[..., 0], (2 * i).astype(f32)) and np.array_equal(tab[..., 1], (2 * j).astype(f32))
    assert (tab[..., 2] == 0.5).all() and (tab[..., 5] == 0.5).all() and (tab[..., 3] == 0).all() and (tab[..., 4] == 0).all()
    assert (tab[..., 6] == 0.5).all()                             # half a metre per pixel
    f = P.wavy_field(w, h)
    r = P.push(tab, w, h, f, None, 1)
    want = (2 * i >= 1) & (2 * j >= 1) & (2 * i + 2 <= w) & (2 * j + 2 <= h)
    assert np.array_equal(r["valid"], want) and want.sum() > 200
    half = f[::2, ::2][:ny, :nx] * f32(0.5)
    assert np.array_equal(bits(r["plan"][want]), bits(half[want]))


def test_identity_returns_the_field_and_the_frame():
    """H = I, unit cells from (0, 0), fps 1, no distortion, the plan the image's size: the field and the frame come back on
    [1, w - 2] x [1, h - 2].  The field has no zero component: m01 is -0.0 here, so a -0.0 would come back as +0.0."""
    w, h = 37, 23
    tab = P.table(P.identity(w, h))
    f, img = P.wavy_field(w, h), P.frame(w, h)
    assert (f != 0).all()
    r = P.push(tab, w, h, f, img, 1)
    inner = np.zeros((h, w), bool)
    inner[1:h - 1, 1:w - 1] = True
    assert np.array_equal(r["valid"], inner) and np.array_equal(r["seen"], inner)
    assert np.array_equal(bits(r["plan"][inner]), bits(f[inner])) and not r["plan"][~inner].any()
    assert np.array_equal(r["bgr"][inner], img[inner]) and not r["bgr"][~inner].any()
    assert list(r["summary"][:3]) == [w * h, inner.sum(), inner.sum()]


def test_bad_values_and_a_push_without_the_field():
    p = P.shore_camera()
    ref = P.PlanViewRef(W, H, p)
    f = P.wavy_field(W, H)
    clean = ref.push(f, P.frame(W, H))
    f2 = f.copy()
    f2[20:30, 40:50, 0] = [np.nan, np.inf, -np.inf, 1e30, 1.0] * 2
    r = ref.push(f2, P.frame(W, H))
    assert r["summary"][4] == 2 and 0 < r["valid"].sum() < clean["valid"].sum() and np.array_equal(r["bgr"], clean["bgr"])
    assert np.isinf(r["plan"]).any() or (np.abs(r["plan"]) > 1e29).any()      # 1e30 is a finite sample; its product may overflow
    only = ref.push(None, P.frame(W, H))
    assert list(only["summary"]) == [clean["summary"][0], clean["summary"][1], 0, 0, 3, 0, 0, 0] and np.array_equal(only["bgr"], clean["bgr"])
    ref.reset()
    assert ref.push(f)["summary"][4] == 1


# ---------------------------------------------------------------------------- the library
def test_entry_points_are_exported_and_declared():
    from ripcurrents_amd import _lib
    import ripcurrents_amd.api as api
    lib = _lib.load()
    for n in ("rcflow_planview_open", "rcflow_planview_push_dev", "rcflow_planview_read", "rcflow_planview_table_read",
              "rcflow_planview_reset", "rcflow_planview_close", "rcflow_planview_info"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert len(_lib.SIGNATURES["rcflow_planview_push_dev"]) == 13
    for m in ("open", "push", "read", "table", "reset", "close", "info"):
        assert callable(getattr(api.Context, "planview_" + m))
    assert api.PLANVIEW_SUMMARY == P.SUMMARY and _lib.RC_PLANVIEW_LAUNCHES == 1
    assert [k for k, _ in _lib.PlanViewParams._fields_] == ["H", "fx", "fy", "cx", "cy", "k1", "k2", "x0", "y0", "dx", "dy", "nx", "ny", "fps",
                                                            "max_gsd", "flags"]
