"""The numpy statement of the motion templates (tests/_motion_ref.py) held to known answers: bars whose direction is known
exactly, diagonal bars, a texture across the 0 / 360 seam, the reference's literal call, and the gates one by one.  CPU
only; the device kernels are held to the same statement in tests/test_gpu_motion.py."""
import numpy as np
import pytest

import _motion_ref as M

f32 = np.float32


def seam_distance(a):
    return min(a % 360.0, 360.0 - a % 360.0)


# ---------------------------------------------------------------------------- bars
@pytest.mark.parametrize("direction,angle,n,rows", [("+x", 0.0, 630, 45), ("-x", 180.0, 630, 45), ("+y", 90.0, 938, 67), ("-y", 270.0, 938, 67)])
def test_bar_direction_is_exact(orc, direction, angle, n, rows):
    """From the tenth push on the angle is exact and n_used is 14 pixels per row of the bar: the two ramps the bar's edges
    leave (stamps ts - 8 .. ts, nine pixels each, abutting) less their four ends.  n_masked equals n_used from the eleventh
    push on.  At the tenth push alone it is one pixel per row more (675 and 1005): the oldest living stamp, 2, equals
    delbound, the pixel behind it holds 0, and d0 = 2 - 0 lies inside (0.5, 2.5), so that zero pixel passes the gradient's
    gates; its history is not above tsmax - duration, so it is masked but not used.  One push later the oldest stamp is 3
    and d0 = 3 fails delta2."""
    ref = M.MotionRef(67, 45, orc.fast_atan2_deg, diff_threshold=30, duration=8, delta1=0.5, delta2=2.5)
    for t, f in enumerate(M.bar_clip(direction)):
        r = ref.push(f)
        if t + 1 >= 10:
            assert r["angle"] == angle, (t + 1, r["angle"])
            assert r["frame"]["n_used"] == n, (t + 1, r["frame"])
            assert r["frame"]["n_masked"] == (n + rows if t + 1 == 10 else n), (t + 1, r["frame"])


@pytest.mark.parametrize("sx,sy,angle", [(1, 1, 45.0), (-1, 1, 135.0), (-1, -1, 225.0), (1, -1, 315.0)])
def test_diagonal_bar_direction(orc, sx, sy, angle):
    ref = M.MotionRef(67, 45, orc.fast_atan2_deg, diff_threshold=30, duration=8, delta1=0.5, delta2=4.5)
    worst = 0.0
    for t, f in enumerate(M.diagonal_clip(sx, sy)):
        r = ref.push(f)
        if t + 1 >= 10 and r["frame"]["n_used"]:
            worst = max(worst, abs(r["angle"] - angle))
    print("diagonal %+d%+d: worst error %.3f degrees" % (sx, sy, worst))
    assert worst < 1.0


# ---------------------------------------------------------------------------- the seam
def test_texture_across_the_seam(orc):
    ref = M.MotionRef(97, 61, orc.fast_atan2_deg, diff_threshold=12, duration=6, delta1=0.5, delta2=2.5)
    seen = []
    for t, f in enumerate(M.texture_clip(97, 61, 12)):
        r = ref.push(f)
        if t == 0:
            continue                                     # no previous frame yet
        b12 = np.floor(r["orient"][r["mask"] != 0].astype(np.float64) * (12.0 / 360.0)).astype(int)
        assert (b12 == 0).any() and (b12 == 11).any(), "the clip does not straddle the seam"
        assert seam_distance(r["angle"]) < 1.0, r["angle"]
        # upstream's two floats added in raster order against the integer sums
        up = M.upstream_float_sum(r["mhi"], r["orient"], r["mask"] != 0, 6.0)
        d = abs(up - r["angle"])
        d = min(d, 360.0 - d)
        seen.append((r["angle"], d, int(r["frame"]["n_used"])))
        assert d < 1e-3, (up, r["angle"])
    print("seam: angles %s" % ", ".join("%.2f" % a for a, _, _ in seen))
    print("seam: float-sequential sum against integer sums, worst %.2e degrees over %d..%d pixels"
          % (max(d for _, d, _ in seen), min(n for _, _, n in seen), max(n for _, _, n in seen)))
    # measured on this clip: the two sums agree to 2.1e-6 degrees at worst (771 to 1 600 pixels per push)
    assert max(d for _, d, _ in seen) < 1e-3


# ---------------------------------------------------------------------------- the reference's literal call
def test_fresh_on_two_frames(orc):
    a, b = M.texture_clip(97, 61, 2, step=2)
    ref = M.MotionRef(97, 61, orc.fast_atan2_deg, diff_threshold=12, fresh=True, duration=5, delta1=0.25, delta2=1.0)
    r0 = ref.push(a)
    assert not r0["mhi"].any() and not r0["mask"].any() and r0["angle"] == 0.0 and r0["frame"]["W"] == 0 and r0["silhouette"] == 0
    r = ref.push(b)
    assert set(np.unique(r["mhi"])) == {f32(0), f32(1)}
    assert set(np.unique(r["vis"])) == {0, 255} and np.array_equal(r["vis"][..., 0] == 255, r["mhi"] == 1)
    assert r["silhouette"] == int((r["mhi"] == 1).sum())
    print("fresh: %d silhouette pixels, %d masked, angle %.3f" % (r["silhouette"], r["frame"]["n_masked"], r["angle"]))
    assert r["frame"]["n_masked"] > 1000
    # the same as a session with a history, opened anew, stamps 0 and 1, duration 1
    ref2 = M.MotionRef(97, 61, orc.fast_atan2_deg, diff_threshold=12, duration=1, delta1=0.25, delta2=1.0)
    ref2.push(a, 0.0)
    r2 = ref2.push(b, 1.0)
    for k in ("mhi", "orient", "mask", "vis"):
        assert np.array_equal(r[k], r2[k]), k
    assert r["frame"] == r2["frame"]
    # an empty silhouette: all zero, angle 0 (the reference divides 0 by 0)
    r3 = ref.push(b)
    assert not r3["mhi"].any() and not r3["mask"].any() and not r3["vis"].any() and r3["angle"] == 0.0


# ---------------------------------------------------------------------------- the gates
def sets_5x5(orient, mhi=None, mask=None, duration=4.0):
    orient = np.asarray(orient, f32).reshape(5, 5)
    mhi = np.full((5, 5), 3, f32) if mhi is None else np.asarray(mhi, f32).reshape(5, 5)
    mask = np.ones((5, 5), bool) if mask is None else np.asarray(mask, bool).reshape(5, 5)
    return M.orientations(mhi, orient, mask, np.zeros((5, 5), np.int64), 1, duration)[0]


def test_gate_orient_360_is_masked_but_not_counted(orc):
    assert orc.fast_atan2_deg(f32(-1e-12), f32(1))[0] == f32(360)       # it occurs
    o = np.full(25, 100, f32)
    o[:13] = 360                                                     # the majority, yet in no bin
    r = sets_5x5(o)
    assert r["n_masked"] == 25 and r["peak_bin"] == 3
    assert r["n_used"] == 12                                         # 360 - 90 = 270 -> -90: outside the 45 degree gate


def test_gate_histogram_tie_goes_to_the_lower_bin():
    o = np.zeros(25, f32)
    o[:12], o[12:24], o[24] = 200, 100, 310                          # bins 6 and 3, twelve each
    r = sets_5x5(o)
    assert r["peak_bin"] == 3 and r["n_used"] == 12 and r["angle"] == 100.0


def test_gate_no_weight_gives_the_base():
    r = sets_5x5(np.full(25, 100, f32), mask=np.zeros(25, bool))
    assert r["W"] == 0 and r["S"] == 0 and r["n_masked"] == 0 and r["tsmax"] == 0 and r["angle"] == 0.0 == r["peak_bin"] * 30
    # pixels older than tsmax - duration carry no weight
    mhi = np.full(25, 1, f32)
    mhi[0] = 9
    r = sets_5x5(np.full(25, 100, f32), mhi=mhi)
    assert r["n_used"] == 1 and r["tsmax"] == 9 and r["W"] == int(np.rint(float(f32(9) * f32(254. / 255. / 4.) + f32(1. - 9. * float(f32(254. / 255. / 4.)))) * 2.0 ** 32))


def test_gate_deltas_are_swapped(orc):
    mhi = (np.arange(5, dtype=f32)[None, :] + np.zeros((5, 1), f32)) * f32(1.0)       # a ramp along +x
    o1, m1 = M.gradient(mhi, 1.5, 2.5, orc.fast_atan2_deg)
    a = M.MotionRef(5, 5, orc.fast_atan2_deg, delta1=2.5, delta2=1.5)
    assert (a.d1, a.d2) == (1.5, 2.5)
    o2, m2 = M.gradient(mhi, a.d1, a.d2, orc.fast_atan2_deg)
    assert np.array_equal(m1, m2) and np.array_equal(o1, o2)
    assert m1[:, 1:4].all() and not m1[:, 0].any() and not m1[:, 4].any()       # d0 = 2 inside, 1 at the replicated ends
    assert (o1[:, 1:4] == 0).all()
    _, m3 = M.gradient(mhi, 2.5, 1.5, orc.fast_atan2_deg)                       # unswapped: nothing passes
    assert not m3.any()
