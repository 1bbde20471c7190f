"""The numpy statement of the flow check (tests/_flowcheck_ref.py) against properties, not against itself: a true field passes and a
noisy one is named, flat and one-dimensional pictures are FLAT, a round trip closes, and every decision's edge is hit exactly by
constructed integers.  No GPU.  The figures in the docstrings were measured with this statement."""
import numpy as np
import pytest

import _flowcheck_ref as F
from ripcurrents_amd import synth

W, H = 160, 120
_CLIPS = {}


def clip(shift):
    if shift not in _CLIPS:
        _CLIPS[shift] = synth.translating_clip(W, H, 2, *shift)
    return _CLIPS[shift]


def inner(r):
    m = np.zeros((H, W), bool)
    m[F.PATCH[0].start + r:F.PATCH[0].stop - r, F.PATCH[1].start + r:F.PATCH[1].stop - r] = True
    return m


# ---------------------------------------------------------------------------- separation
@pytest.mark.parametrize("shift", [(1.25, -0.75), (5.25, -3.75)])
@pytest.mark.parametrize("radius", [4, 2])
def test_true_field_passes_and_noisy_patch_is_named(shift, radius):
    """res_max = 1.5 lies between what a true field leaves and what +-3 px of noise leaves.  Measured with this statement, both
    shifts alike: the largest window-mean residual of the true field over full, wholly OK windows is 0.5849 grey levels at radius 4
    and 0.7750 at radius 2; the smallest inside the noisy patch, r inside it, is 4.367 and 2.567"""
    prev, nxt = clip(shift)
    p = F.Params(radius=radius, res_max=1.5, tex_min=1, tests=F.RESID)
    true = F.constant_field(W, H, *shift)
    o = F.check(prev, nxt, true, None, p)
    s = o["sides"]
    full = (s["N"] == (2 * radius + 1) ** 2) & (s["Nr"] == s["N"])
    assert full.sum() > 15000 and not (o["flags"][full] & F.RESID).any()
    top = o["resid"][..., 0][full].max()
    n = F.check(prev, nxt, F.noisy_patch(true), None, p)
    m = inner(radius)
    assert n["sides"]["ok"][m].all() and ((n["flags"][m] & F.RESID) != 0).all()
    low = n["resid"][..., 0][m].min()
    print("shift %s radius %d: true field at most %.4f, noisy patch at least %.4f grey levels" % (shift, radius, top, low))
    assert top < 1.5 < low
    # a field that is ignored cannot do both: with no motion claimed the true clip's own change is far above the bound
    assert o["resid"][..., 1][full].min() > o["resid"][..., 0][full].max()


def test_a_constant_error_of_one_pixel_is_recorded_not_asserted():
    """a constant error of 1 px inside the patch is not cleanly separable at res_max = 1.5.  Measured with this statement at radius
    4 (radius 2): (+1, 0) window means from 1.396 (0.468), median 3.030 (2.885), RESID on 99.85 % (95.2 %) of the inner patch;
    (0, +1) from 1.573 (0.750), median 3.842 (3.500); the diagonal from 1.512 (0.740), median 2.869 (2.896)"""
    prev, nxt = clip((1.25, -0.75))
    for radius in (4, 2):
        for err in ((1.0, 0.0), (0.0, 1.0), (0.70710678, 0.70710678)):
            f = F.constant_field(W, H, 1.25, -0.75)
            f[F.PATCH] += np.array(err, np.float32)
            o = F.check(prev, nxt, f, None, F.Params(radius=radius, res_max=1.5, tests=F.RESID))
            v = o["resid"][..., 0][inner(radius)]
            print("radius %d error %s: window means from %.3f, median %.3f, RESID on %.4f of the patch" % (
                radius, err, v.min(), np.median(v), ((o["flags"][inner(radius)] & F.RESID) != 0).mean()))


# ---------------------------------------------------------------------------- texture
@pytest.mark.parametrize("tex_min", [1, 65025])
def test_constant_and_one_dimensional_frames_are_flat(tex_min):
    p = F.Params(radius=3, tex_min=tex_min, tests=F.FLAT)
    zero = np.zeros((24, 31, 2), np.float32)
    const = np.full((24, 31), 93, np.uint8)
    o = F.check(const, const, zero, None, p)
    assert (o["flags"] == F.FLAT).all() and not o["texture"].any()
    ramp = np.tile(((np.arange(31) * 37) % 256).astype(np.uint8), (24, 1))       # varies along x only: the smaller eigenvalue is 0
    o = F.check(ramp, ramp, zero, None, p)
    assert (o["flags"] == F.FLAT).all() and not o["texture"].any() and o["sides"]["a"].min() > 0 and not o["sides"]["c"].any()


def test_synthetic_texture_is_not_flat():
    """the smallest smaller eigenvalue of the mean structure tensor of the 160 x 120 clip's first frame at radius 4: 2.290 (measured
    with this statement); 0.259 at radius 2, where tex_min = 1 names some pixels"""
    prev, nxt = clip((1.25, -0.75))
    o = F.check(prev, nxt, F.constant_field(W, H, 1.25, -0.75), None, F.Params(radius=4, tex_min=1, tests=F.FLAT))
    print("smallest texture at radius 4: %.4f" % o["texture"].min())
    assert not (o["flags"] & F.FLAT).any() and o["texture"].min() > 1.0
    o = F.check(prev, nxt, F.constant_field(W, H, 1.25, -0.75), None, F.Params(radius=4, tex_min=3, tests=F.FLAT))
    assert np.array_equal((o["flags"] & F.FLAT) != 0, o["texture"] < 3.0)         # far from the edge of the decision the float agrees


# ---------------------------------------------------------------------------- round trip
def test_round_trip_closes_and_an_error_of_a_pixel_does_not():
    prev, nxt = synth.translating_clip(W, H, 2, 3.0, -2.0)
    fwd, back = F.constant_field(W, H, 3.0, -2.0), F.constant_field(W, H, -3.0, 2.0)
    p = F.Params(radius=1, tests=F.FB, fb_rel=0.0, fb_abs=0.0)
    o = F.check(prev, nxt, fwd, back, p)
    ok = o["sides"]["ok"]
    assert ok.sum() == (W - 3) * (H - 2) and not (o["flags"] & F.FB).any() and (o["flags"][~ok] == F.OUT).all()
    off = F.constant_field(W, H, -2.0, 2.0)
    o = F.check(prev, nxt, fwd, off, F.Params(radius=1, tests=F.FB, fb_rel=0.0, fb_abs=0.5))
    assert np.array_equal((o["flags"] & F.FB) != 0, ok)
    assert not (F.check(prev, nxt, fwd, None, p)["flags"] & F.FB).any()             # no back field, no test


# ---------------------------------------------------------------------------- the edges of the decisions
def frames(w=9, h=7, g=100):
    return np.full((h, w), g, np.uint8), np.full((h, w), g, np.uint8)


def test_edge_resid():
    """radius 0: N = Nr = 1 and R = res.  The vector (1/64, 1/64) weighs next[y+1, x+1] with 1: res = its difference from prev"""
    prev, nxt = frames()
    f = np.zeros((7, 9, 2), np.float32)
    f[3, 4] = (1 / 64., 1 / 64.)
    p = F.Params(radius=0, tests=F.RESID, res_max=1 / 4096.)
    assert F.host_constants(p)[0] == 1
    nxt[4, 5] = 101
    o = F.check(prev, nxt, f, None, p)
    assert o["sides"]["R"][3, 4] == 1 and o["sides"]["Nr"][3, 4] == 1 and not o["flags"][3, 4] & F.RESID      # R == res_q Nr
    nxt[4, 5] = 102
    o = F.check(prev, nxt, f, None, p)
    assert o["sides"]["R"][3, 4] == 2 and o["flags"][3, 4] & F.RESID                                          # one more
    # a window of nine with one pixel not OK: Nr = 8
    f[2, 3] = (np.nan, 0.0)
    nxt[4, 5] = 100
    nxt[3, 3] = 108                                               # res = 8 * 4096 at (3, 3), zero flow
    q = F.Params(radius=1, tests=F.RESID, res_max=1.0)
    o = F.check(prev, nxt, f, None, q)
    assert o["sides"]["Nr"][3, 3] == 8 and o["sides"]["N"][3, 3] == 9 and o["sides"]["R"][3, 3] == 8 * 4096 and not o["flags"][3, 3] & F.RESID
    nxt[4, 5] = 101                                               # res = 1 at (3, 4), inside the window of (3, 3)
    o = F.check(prev, nxt, f, None, q)
    assert o["sides"]["R"][3, 3] == 8 * 4096 + 1 and o["flags"][3, 3] & F.RESID


def test_edge_flat():
    assert not F.flat_test(np.array([5]), np.array([10]), np.array([6]), np.array([1]))[0]       # (5 - 1)(10 - 1) == 6 * 6: passes
    assert F.flat_test(np.array([5]), np.array([10]), np.array([6]), np.array([2]))[0]
    assert F.flat_test(np.array([5]), np.array([10]), np.array([-7]), np.array([1]))[0]
    assert F.flat_test(np.array([1]), np.array([9]), np.array([0]), np.array([5]))[0] is np.True_    # a + c == 2 t, but a < t
    # through a picture at radius 0: gx = gy = 2, so a = c = b = 4 and the smaller eigenvalue is 0: passes at tex_min 0 only
    prev = (2 * (np.arange(7)[:, None] + np.arange(9)[None, :])).astype(np.uint8)
    zero = np.zeros((7, 9, 2), np.float32)
    o = F.check(prev, prev, zero, None, F.Params(radius=0, tests=F.FLAT, tex_min=0))
    s = o["sides"]
    assert (s["a"][3, 4], s["c"][3, 4], s["b"][3, 4]) == (16, 16, 16) and not o["flags"].any()
    assert (F.check(prev, prev, zero, None, F.Params(radius=0, tests=F.FLAT, tex_min=1))["flags"] == F.FLAT).all()


def test_edge_round_trip():
    """q = (64, 0), the back vector -(64, 0) + (8, 0): e2 = 64 and 1024 e2 = 65536 = fb_abs_q with fb_abs = 1/8"""
    prev, nxt = frames()
    fwd = F.constant_field(9, 7, 1.0, 0.0)
    p = F.Params(radius=0, tests=F.FB, fb_rel=0.0, fb_abs=0.125)
    assert F.host_constants(p)[2] == 65536
    o = F.check(prev, nxt, fwd, F.constant_field(9, 7, -1.0 + 8 / 64., 0.0), p)
    assert o["sides"]["ok"][:, :8].all() and not (o["flags"][:, :8] & F.FB).any()
    o = F.check(prev, nxt, fwd, F.constant_field(9, 7, -1.0 + 9 / 64., 0.0), p)
    assert (o["flags"][:, :8] & F.FB).all()
    # the relative term: m2 = 64^2 + 56^2 = 7232, fb_rel_q = 1024 * 0.5 = 512: 512 * 7232 > 65536, so e2 = 64 passes without fb_abs
    o = F.check(prev, nxt, fwd, F.constant_field(9, 7, -1.0 + 8 / 64., 0.0), F.Params(radius=0, tests=F.FB, fb_rel=0.5, fb_abs=0.0))
    assert not (o["flags"][:, :8] & F.FB).any()
    # a BAD back sample under a corner of weight 0 still sets the bit: the vector (1, 0) lands on (x + 1, y) with fx = 0
    back = F.constant_field(9, 7, -1.0, 0.0)
    back[3, 6] = (np.inf, 0.0)
    o = F.check(prev, nxt, fwd, back, p)
    named = np.zeros((7, 9), bool)
    named[2:4, 4:6] = True                                        # the pixels whose x0 or x1 is 6 and whose y0 or y1 is 3
    assert np.array_equal((o["flags"][:, :8] & F.FB) != 0, named[:, :8])


def test_edge_target_and_sample():
    prev, nxt = frames()
    w, h = 9, 7
    f = np.zeros((h, w, 2), np.float32)
    f[2, w - 2] = (1.0, 0.0)                                      # X == 64 (w - 1): in, x1 clamped with weight 0
    f[3, w - 2] = (1.0 + 1 / 64., 0.0)                            # one more: OUT
    f[h - 2, 3] = (0.0, 1.0)
    f[h - 2, 4] = (0.0, 1.0 + 1 / 64.)
    f[1, 1] = (500.0, 0.0)                                        # BAD
    f[1, 2] = (np.nextafter(np.float32(500.0), np.float32(0.0)), 0.0)      # the float below: a sample, and OUT
    f[1, 3] = (0.0, -500.0)
    f[0, 0] = (-0.0, -0.0)
    o = F.check(prev, nxt, f, None, F.Params(radius=0, tests=0))
    fl = o["flags"]
    assert fl[2, w - 2] == 0 and fl[3, w - 2] == F.OUT and fl[h - 2, 3] == 0 and fl[h - 2, 4] == F.OUT
    assert fl[1, 1] == F.BAD and fl[1, 2] == F.OUT and fl[1, 3] == F.BAD and fl[0, 0] == 0
    assert o["sides"]["qx"][1, 2] == 32000 and o["summary"][0] == w * h - 5
    ck = o["checked"].view(np.uint32)
    assert ck[0, 0, 0] == 0x80000000 and (ck[1, 1] == F.NAN_BITS).all() and (ck[1, 2] == F.NAN_BITS).all()     # the input's bits, -0.0 kept
    z = F.check(prev, nxt, f, None, F.Params(radius=0, tests=0, fill="zero"))["checked"].view(np.uint32)
    assert not z[1, 1].any() and z[2, w - 2, 0] == np.float32(1.0).view(np.uint32)


def test_edge_speed():
    prev, nxt = frames()
    f = np.zeros((7, 9, 2), np.float32)
    f[3, 2] = (2.0, 0.0)                                          # |q| = 128 = smax_q exactly
    f[3, 3] = (2.0 + 1 / 64., 0.0)
    f[3, 6] = (0.0, -2.0 - 1 / 64.)
    f[0, 0] = (-3.0, 0.0)                                         # OUT, and FAST all the same
    o = F.check(prev, nxt, f, None, F.Params(radius=0, tests=F.FAST, speed_max=2.0))
    assert o["flags"][3, 2] == 0 and o["flags"][3, 3] == F.FAST and o["flags"][3, 6] == F.FAST and o["flags"][0, 0] == F.OUT | F.FAST


def test_no_gain():
    """a vector that explains nothing is named; with gain_pm = 1000 a vector may do as badly as no motion, not worse"""
    prev, nxt = clip((1.25, -0.75))
    true = F.constant_field(W, H, 1.25, -0.75)
    p = F.Params(radius=2, tests=F.NOGAIN, gain_pm=500)
    o = F.check(prev, nxt, true, None, p)
    s = o["sides"]
    full = s["Nr"] == 25
    assert not (o["flags"][full] & F.NOGAIN).any()
    wrong = F.check(prev, nxt, F.constant_field(W, H, -1.25, 0.75), None, p)
    assert ((wrong["flags"][wrong["sides"]["Nr"] == 25] & F.NOGAIN) != 0).mean() > 0.9
    assert not (F.check(prev, nxt, F.constant_field(W, H, 0.0, 0.0), None, p)["flags"]).any()        # q = (0, 0) is not asked
    assert not (F.check(prev, nxt, F.constant_field(W, H, -1.25, 0.75), None, F.Params(radius=2, tests=F.NOGAIN, gain_pm=0))["flags"] & F.NOGAIN).any()


# ---------------------------------------------------------------------------- the helper and the session
def test_box_sums_against_a_double_loop():
    rng = np.random.RandomState(5)
    p = rng.randint(-1000, 1000, (7, 11)).astype(np.int64)
    for r in (0, 1, 3, 7):
        want = np.zeros_like(p)
        for y in range(7):
            for x in range(11):
                want[y, x] = p[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].sum()
        assert np.array_equal(F.box_sum(p, r), want)


def test_picture_cells_and_summary():
    prev, nxt = clip((1.25, -0.75))
    f = F.hostile(F.noisy_patch(F.constant_field(W, H, 1.25, -0.75)))
    p = F.Params(radius=2, grid_x=7, grid_y=5, tests=F.TESTS, gain_pm=900, speed_max=3.0, tex_min=1)
    o = F.check(prev, nxt, f, None, p, computing=4, pushes=6)
    fl = o["flags"]
    assert (fl[np.isnan(f).any(-1)] == F.BAD).all() and set(np.unique(fl)) >= {0, F.BAD, F.RESID, F.RESID | F.FAST}
    valid = fl == 0
    assert np.array_equal(o["mask"] == 255, valid) and np.array_equal(o["picture"][valid], np.repeat(prev[valid][:, None], 3, 1))
    assert (o["picture"][fl == F.BAD] == F.COLOURS[0]).all() and (o["picture"][(fl & 15) == F.RESID] == F.COLOURS[3]).all()
    assert np.isnan(o["checked"][~valid]).all() and np.array_equal(o["checked"][valid], f[valid])
    assert o["sums"][:, 0].sum() == valid.sum() == o["summary"][0] and list(o["summary"][8:]) == [4, 6]
    assert o["cells"]["pixels"].sum() == W * H and o["cells"]["pixels"][-1] == (W - 6 * (W // 7)) * (H - 4 * (H // 5))
    assert [int(o["summary"][1 + k]) for k in range(7)] == [int(((fl >> k) & 1).sum()) for k in range(7)]
    sx = o["sides"]["qx"][valid].sum()
    assert o["sums"][:, 8].sum() == sx and abs(o["cells"]["mean_x"][0] - 1.25) < 0.01


def test_session_holds_the_frame_and_counts():
    c = synth.translating_clip(40, 30, 4, 1.0, 0.0)
    f = F.constant_field(40, 30, 1.0, 0.0)
    ref = F.FlowCheckRef(40, 30, F.Params(radius=1))
    assert ref.push(c[0], None, f) is None and list(ref.summary) == [0] * 8 + [0, 1]       # the first push only stores its frame
    a = ref.push(c[1], None, f)
    b = F.check(c[0], c[1], f, None, F.Params(radius=1), 1, 2)
    assert np.array_equal(a["flags"], b["flags"]) and list(a["summary"]) == list(b["summary"]) and list(ref.summary[8:]) == [1, 2]
    ref.reset()
    assert list(ref.summary) == [0] * 8 + [1, 2]
    with pytest.raises(F.StateError):
        ref.push(c[2], None, f)
    assert ref.push(c[3], c[2], f)["summary"][9] == 3
    with pytest.raises(ValueError):
        ref.set(tests=128)


def test_library_exports_the_entry_points():
    import ctypes as C
    import os
    from ripcurrents_amd import _lib
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ripcurrents_amd", "librcflow.so")
    lib = C.CDLL(so)
    for name in ("open", "push_dev", "read", "set", "reset", "close", "info"):
        assert hasattr(lib, "rcflow_flowcheck_" + name) and "rcflow_flowcheck_" + name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rcflow_flowcheck_push_dev"]) == 25
    assert C.sizeof(_lib.FlowcheckParams) == 64 and C.sizeof(_lib.FlowcheckCell) == 32 and C.sizeof(_lib.FlowcheckInfo) == 104
    from ripcurrents_amd.api import FLOWCHECK_CELL_DTYPE, FLOWCHECK_FLAGS, FLOWCHECK_SUMMARY, FLOWCHECK_SUMS, FlowCheck
    assert FLOWCHECK_CELL_DTYPE == F.CELL and FLOWCHECK_SUMMARY == F.SUMMARY and len(FLOWCHECK_SUMS) == F.SUMS == _lib.RC_FLOWCHECK_SUMS and FlowCheck
    assert tuple(FLOWCHECK_FLAGS) == F.NAMES and tuple(FLOWCHECK_FLAGS.values()) == (F.BAD, F.OUT, F.FLAT, F.RESID, F.NOGAIN, F.FB, F.FAST)
    assert (_lib.RC_FLOWCHECK_TESTS, _lib.RC_FLOWCHECK_MAX_RADIUS, _lib.RC_FLOWCHECK_LAUNCHES) == (F.TESTS, F.MAX_RADIUS, 2)
