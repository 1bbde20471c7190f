"""GPU parity of sparse pyramidal Lucas-Kanade (rcflow_pyrlk_dev / rcflow_pyrlk_u8 and its clients) vs the CPU oracle.

Two figures, because the oracle has two modes:

* Bit-equal to the exact-sum oracle.  The kernel sums its window products as exact integers; oracle.pyrlk(
  exact_sums=True) does the same and is otherwise upstream's scalar path operation for operation, so next points,
  status and err (where upstream defines err: status 1, or GET_MIN_EIGENVALS) are np.array_equal.  Asserted over the
  reference's call shapes (every pixel of a 640x480 frame), point counts, window shapes up to 128x128, levels 0..7,
  frame sizes from 5 pixels wide to 4K, the criteria, the point classes of tests/_lk_ref.py, the C ABI plumbing and
  the host classes; a subset also against the numpy restatement tests/_lk_ref.py directly.
* A statistical bar against upstream's raster-order float sums (the oracle's default): the two differ by summation
  noise, ~1e-4 px, except where a termination test sits on its threshold and one side takes a Newton step more.
  Status identical, >= 97 % of points within 2e-3 px, all within 0.15 px (one Newton step at the eps = 0.1
  criterion).  The first tests below assert that; tests/test_lk_ref.py asserts the same between the oracle's modes.
"""
import os

import numpy as np
import pytest

import _lk_ref as R
from ripcurrents_amd import synth
from ripcurrents_amd.api import PopulationMap, Streakline, Timeline

pytestmark = pytest.mark.gpu


def _points(w, h, n, seed):
    rng = np.random.RandomState(seed)
    p = np.stack([rng.uniform(5, w - 5, n), rng.uniform(5, h - 5, n)], axis=1).astype(np.float32)
    p[0] = (2.0, 3.0)                 # windows hanging over the corner
    p[1] = (w - 1.5, h - 2.5)
    p[2] = (-300.0, 10.0)             # outside: status 0
    p[3] = (w / 2, h + 400.0)
    return p


@pytest.mark.parametrize("clip,size", [("translating", (320, 240)), ("surf", (640, 480))])
@pytest.mark.parametrize("win,eps,flags", [((21, 21), 0.01, 0), ((21, 21), 0.1, 0), ((50, 50), 0.1, 10)])
def test_pyrlk_matches_oracle(ctx, orc, clip, size, win, eps, flags):
    w, h = size
    fr = synth.translating_clip(w, h, 2) if clip == "translating" else synth.surf_clip(w, h, 2)
    pts = _points(w, h, 200, 11)
    ref_q, ref_st, ref_er = orc.pyrlk(fr[0], fr[1], pts, win=win, max_level=3, epsilon=eps, flags=flags)
    q, st, er = ctx.calcOpticalFlowPyrLK(fr[0], fr[1], pts, win=win, max_level=3, epsilon=eps, flags=flags)
    q, st, er = q.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()
    assert ctx.pyrlk_levels(w, h, win, 3) == orc.pyrlk_levels(w, h, win, 3)
    assert np.array_equal(st, ref_st)
    good = ref_st == 1
    d = np.abs(q[good] - ref_q[good]).max(axis=1)
    print("[parity] pyrlk %s win %s eps %g flags %d: max %.3g  frac<2e-3 %.4f" % (clip, win, eps, flags, d.max(), (d < 2e-3).mean()))
    assert (d < 2e-3).mean() >= 0.97 and d.max() < 0.15
    # failed points keep the position the last level left them at (same arithmetic, no iteration)
    assert np.abs(q[~good] - ref_q[~good]).max() < 1e-3
    if flags & 8:      # min eigenvalue of the (exactly summed vs float-summed) covariance matrix
        assert np.allclose(er[good], ref_er[good], rtol=1e-4, atol=1e-7)
    else:              # mean |I - J| in 1/32 grey levels at the final position: a few fixed-point LSBs
        assert np.abs(er[good] - ref_er[good]).max() <= 16.0 / (32 * win[0] * win[1])


def test_pyrlk_unusable_points(ctx, orc):
    """NaN, infinite and huge point coordinates: status 0 like the oracle (x86 conversions give INT_MIN,
    which fails the window bounds check), never an out-of-bounds read; the other points are unaffected."""
    w, h = 320, 240
    fr = synth.surf_clip(w, h, 2)
    pts = _points(w, h, 40, 3)
    pts[5] = (np.nan, 50.0)
    pts[6] = (60.0, np.nan)
    pts[7] = (np.inf, 10.0)
    pts[8] = (-np.inf, -np.inf)
    pts[9] = (3e38, 3e38)
    pts[10] = (-3e38, 100.0)
    pts[11] = (2147483648.0, 5.0)
    with np.errstate(all="ignore"):
        ref_q, ref_st, _ = orc.pyrlk(fr[0], fr[1], pts, win=(21, 21), max_level=3)
        q, st, _ = ctx.calcOpticalFlowPyrLK(fr[0], fr[1], pts, win=(21, 21), max_level=3)
    q, st = q.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, ref_st) and not st[5:12].any() and st[12:].all()
    good = ref_st == 1
    assert np.abs(q[good] - ref_q[good]).max() < 0.15


def test_pyrlk_initial_flow_and_strided_input(ctx, orc):
    import torch
    w, h = 320, 240
    fr = synth.translating_clip(w, h, 2)
    pts = _points(w, h, 32, 5)[4:]
    guess = pts + np.array([[1.0, -0.5]], np.float32)
    ref_q, ref_st, _ = orc.pyrlk(fr[0], fr[1], pts, next_pts=guess, win=(21, 21), flags=4)
    big = torch.zeros((2, h, w + 37), dtype=torch.uint8, device="cuda")      # row pitch != width
    big[:, :, :w] = torch.from_numpy(fr).cuda()
    q, st, _ = ctx.calcOpticalFlowPyrLK(big[0, :, :w], big[1, :, :w], pts, next_pts=guess, win=(21, 21), flags=4)
    assert np.array_equal(st.cpu().numpy(), ref_st)
    assert np.abs(q.cpu().numpy() - ref_q).max() < 2e-3


def test_pyrlk_host_pointer_form(ctx):
    w, h = 320, 240
    fr = synth.translating_clip(w, h, 2)
    pts = _points(w, h, 40, 9)
    q, st, er = ctx.calcOpticalFlowPyrLK(fr[0], fr[1], pts, win=(21, 21), flags=8)
    qh, sth, erh = ctx.calcOpticalFlowPyrLK_host(fr[0], fr[1], pts, win=(21, 21), flags=8)
    assert np.array_equal(qh, q.cpu().numpy()) and np.array_equal(sth, st.cpu().numpy())
    assert np.array_equal(erh, er.cpu().numpy())


def test_pyrlk_rejects_bad_arguments(ctx):
    fr = synth.translating_clip(64, 64, 2)
    with pytest.raises(Exception):
        ctx.calcOpticalFlowPyrLK(fr[0], fr[1], np.zeros((1, 2), np.float32), win=(2, 2))
    with pytest.raises(Exception):
        ctx.calcOpticalFlowPyrLK(fr[0], fr[1][:32], np.zeros((1, 2), np.float32))
    q, st, er = ctx.calcOpticalFlowPyrLK(fr[0], fr[1], np.zeros((0, 2), np.float32))     # empty point list
    assert q.shape == (0, 2) and st.shape == (0,)


def test_streakline_runlk_matches_oracle(ctx, orc):
    """Streakline::runLK as the reference runs it (PyrLK-driven vertices, Streakline.cpp:22-71)."""
    w, h = 640, 480
    fr = synth.surf_clip(w, h, 6)
    gen = (300.0, 200.0)
    sl = Streakline(gen)
    verts = np.zeros((16, 2), np.float32)
    verts[0] = gen
    n, fc = 1, 1
    for t in range(5):
        sl.runLK(ctx, fr[t], fr[t + 1])
        n, fc = orc.streakline_step_lk(verts, n, gen, fr[t], fr[t + 1], fc)
        assert sl.numberOfVertices == n and sl.frameCount == fc
        got = np.asarray(sl.vertices, np.float32)
        assert np.abs(got - verts[:n]).max() < 5e-3


def test_timeline_and_population_map(ctx, orc):
    """Timeline / PopulationMap (ripcurrents_module.cpp:751-807, :1140-1196): constructors as written
    in the reference, vertices moved by the PyrLK call of :775 / :1162 without jump rejection."""
    w, h = 640, 480
    fr = synth.surf_clip(w, h, 4)
    tl = Timeline((100.0, 100.0), (500.0, 300.0), 8)
    assert len(tl.vertices) == 9 and tl.vertices[0] == (100.0, 100.0) and tl.vertices[8] == (500.0, 300.0)
    pm = PopulationMap((50.0, 60.0), (150.0, 160.0), 12, rng=np.random.RandomState(3))
    assert all(150.0 <= x <= 250.0 and 160.0 <= y <= 260.0 for x, y in pm.vertices)   # the (u + 1) factor
    for obj in (tl, pm):
        ref = np.asarray(obj.vertices, np.float32)
        for t in range(3):
            obj.runLK(ctx, fr[t], fr[t + 1])
            ref, _, _ = orc.pyrlk(fr[t], fr[t + 1], ref, win=(50, 50), max_level=3, epsilon=0.1, flags=10)
            assert np.abs(np.asarray(obj.vertices, np.float32) - ref).max() < 5e-3


def test_pyrlk_against_committed_golden_fixture(ctx):
    """tests/golden/pyrlk_160x120.npz: inputs + oracle outputs (tests/golden/make_golden.py)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyrlk_160x120.npz"))
    for tag, win, eps, flags in (("50", (50, 50), 0.1, 10), ("21", (21, 21), 0.01, 0)):
        q, st, er = ctx.calcOpticalFlowPyrLK(g["prev"], g["next"], g["pts"], win=win, max_level=3, epsilon=eps, flags=flags)
        assert np.array_equal(st.cpu().numpy(), g["status" + tag])
        ok = g["status" + tag] == 1
        assert np.abs(q.cpu().numpy()[ok] - g["next" + tag][ok]).max() < 2e-3


# ---------------------------------------------------------------------------------------------------------------
# Bit-equality with the exact-sum oracle (orc.pyrlk(exact_sums=True)) over the tracker's whole accepted range.
# ---------------------------------------------------------------------------------------------------------------
ORC_THREADS = 16


def _gpu(ctx, prev, nxt, pts, guess=None, **kw):
    q, st, er = ctx.calcOpticalFlowPyrLK(prev, nxt, pts, next_pts=guess, **kw)
    return q.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()


def _exact(orc, prev, nxt, pts, guess=None, **kw):
    with np.errstate(all="ignore"):
        return orc.pyrlk(prev, nxt, pts, next_pts=guess, exact_sums=True, nthreads=ORC_THREADS, **kw)


def _check(ctx, orc, prev, nxt, pts, guess=None, what="", **kw):
    got, ref = _gpu(ctx, prev, nxt, pts, guess, **kw), _exact(orc, prev, nxt, pts, guess, **kw)
    diff = R.mismatch(got, ref, kw.get("flags", 0))
    assert not diff, "%s %r: %s" % (what, kw, diff)
    return got


def _c_pyrlk_dev(ctx, prev, nxt, pts, q, st, er, win, max_level=3, crit_type=3, max_count=30, epsilon=0.01, flags=0,
                 min_eig=1e-4, stream=0):
    """rcflow_pyrlk_dev through the C ABI on tensors the caller owns (er may be None: d_err = NULL).  Returns rc."""
    h, w = prev.shape
    ctx._bind(stream)
    return ctx._lib.rcflow_pyrlk_dev(ctx._h, stream, ctx._ptr(prev), prev.stride(0), ctx._ptr(nxt), nxt.stride(0), w, h,
                                     ctx._ptr(pts), ctx._ptr(q), pts.shape[0], ctx._ptr(st),
                                     None if er is None else ctx._ptr(er), int(win[0]), int(win[1]), int(max_level),
                                     int(crit_type), int(max_count), float(epsilon), int(flags), float(min_eig))


def _last_error():
    from ripcurrents_amd import _lib
    return (_lib.load().rcflow_last_error() or b"").decode()


@pytest.fixture(scope="module")
def surf640():
    return synth.surf_clip(640, 480, 2)


@pytest.fixture(scope="module")
def surf320():
    return synth.surf_clip(320, 240, 2)


@pytest.mark.parametrize("eps", [0.01, 0.1])
def test_every_pixel_of_a_640x480_frame(ctx, orc, surf640, eps):
    """ripcurrents_module.cpp:716 (eps 0.01) and :738 (eps 0.1): every pixel a point, 307 200 blocks."""
    ys, xs = np.mgrid[0:480, 0:640]
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)
    q, st, er = _check(ctx, orc, surf640[0], surf640[1], pts, what="every pixel", win=(21, 21), max_level=3,
                       max_count=30, epsilon=eps, flags=0)
    assert len(st) == 307200 and st.mean() > 0.9


def test_streakline_form_on_a_lattice(ctx, orc, surf640):
    """Streakline.cpp:32 / ripcurrents_module.cpp:775 / :1162: win 50, eps 0.1, flags 10, a 40 x 30 lattice."""
    ys, xs = np.mgrid[0:30, 0:40]
    pts = np.stack([xs.ravel() * 16 + 8, ys.ravel() * 16 + 8], axis=1).astype(np.float32)
    guess = pts + np.float32(0.5)
    _check(ctx, orc, surf640[0], surf640[1], pts, guess, what="lattice", win=(50, 50), max_level=3, max_count=30,
           epsilon=0.1, flags=10)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65535, 65536, 70000])
def test_point_counts(ctx, orc, surf320, n):
    rng = np.random.RandomState(n)
    pts = np.stack([rng.uniform(-3, 323, n), rng.uniform(-3, 243, n)], axis=1).astype(np.float32)
    _check(ctx, orc, surf320[0], surf320[1], pts, what="npts %d" % n, win=(21, 21), max_level=3)


@pytest.mark.parametrize("win", [(3, 3), (5, 9), (9, 5), (31, 15), (15, 31), (21, 21), (50, 50)])
@pytest.mark.parametrize("flags", [0, 4, 8, 12])
def test_window_shapes_and_point_classes(ctx, orc, win, flags):
    """Rectangular windows and an odd number of window pixels, on the point classes of tests/_lk_ref.py."""
    for (w, h) in ((320, 240), (333, 251)):
        fr = synth.surf_clip(w, h, 2)
        pts = R.point_classes(w, h, win, 3)
        _check(ctx, orc, fr[0], fr[1], pts, R.guesses(pts, w, h), what="%dx%d" % (w, h), win=win, max_level=3,
               flags=flags)


@pytest.mark.parametrize("win", [(127, 128), (128, 128), (128, 127)])
def test_largest_windows(ctx, orc, win):
    """The accepted limit: 128 x 128 (about 102 KB of dynamic LDS per block) on a 1080p frame."""
    fr = synth.surf_clip(1920, 1080, 2)
    pts = R.point_classes(1920, 1080, win, 3, n_random=40)
    _check(ctx, orc, fr[0], fr[1], pts, what="1080p", win=win, max_level=3, epsilon=0.1, flags=0)
    _check(ctx, orc, fr[0], fr[1], pts, what="1080p", win=win, max_level=3, epsilon=0.1, flags=8)


@pytest.mark.parametrize("win,max_level", [((129, 128), 3), ((128, 129), 3), ((2, 5), 3), ((5, 2), 3), ((21, 21), 8),
                                           ((21, 21), -1)])
def test_refusals_just_beyond_the_range(ctx, surf320, win, max_level):
    """RC_EINVAL, rcflow_last_error set, no output touched."""
    import torch
    a, b = torch.from_numpy(surf320[0]).cuda(), torch.from_numpy(surf320[1]).cuda()
    pts = torch.full((8, 2), 100.0, device="cuda")
    q = torch.full((8, 2), -7.0, device="cuda")
    st = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    er = torch.full((8,), -3.0, device="cuda")
    rc = _c_pyrlk_dev(ctx, a, b, pts, q, st, er, win, max_level=max_level)
    torch.cuda.synchronize()
    assert rc == -1 and "PyrLK" in _last_error()                      # RC_EINVAL
    assert (q == -7.0).all() and (st == 9).all() and (er == -3.0).all()
    with pytest.raises(Exception):
        ctx.calcOpticalFlowPyrLK(surf320[0], surf320[1], np.full((8, 2), 100, np.float32), win=win, max_level=max_level)
    # the host-pointer form refuses the same call and writes nothing
    p = np.full((8, 2), 100, np.float32)
    qh, sth, erh = np.full((8, 2), -7, np.float32), np.full(8, 9, np.uint8), np.full(8, -3, np.float32)
    rc = ctx._lib.rcflow_pyrlk_u8(ctx._h, 0, surf320[0].ctypes.data, 320, surf320[1].ctypes.data, 320, 320, 240,
                                  p.ctypes.data, qh.ctypes.data, 8, sth.ctypes.data, erh.ctypes.data, win[0], win[1],
                                  max_level, 3, 30, 0.01, 0, 1e-4)
    assert rc == -1 and (qh == -7).all() and (sth == 9).all() and (erh == -3).all()


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("max_level", [0, 1, 3, 7])
def test_levels_on_large_frames(ctx, orc, size, max_level):
    w, h = size
    fr = synth.surf_clip(w, h, 2)
    rng = np.random.RandomState(max_level)
    pts = np.stack([rng.uniform(-8, w + 8, 500), rng.uniform(-8, h + 8, 500)], axis=1).astype(np.float32)
    edge = R.bounds_points(w, h, (21, 21), max_level)
    pts[:len(edge)] = edge
    assert ctx.pyrlk_levels(w, h, (21, 21), max_level) == orc.pyrlk_levels(w, h, (21, 21), max_level)
    _check(ctx, orc, fr[0], fr[1], pts, what="%dx%d" % size, win=(21, 21), max_level=max_level)


@pytest.mark.parametrize("size,win", [((333, 251), (21, 21)), ((64, 48), (21, 21)), ((21, 17), (21, 21)),
                                      ((16, 16), (21, 21)), ((5, 400), (21, 21)), ((400, 5), (21, 21)),
                                      ((5, 400), (3, 3)), ((400, 5), (3, 3)), ((64, 48), (5, 9)), ((97, 33), (9, 5))])
def test_small_and_odd_frames(ctx, orc, size, win):
    """Odd sizes, frames smaller than the window (reads reflect more than once), the level capping rule."""
    w, h = size
    fr = synth.surf_clip(w, h, 2)
    for max_level in (0, 1, 2, 4, 7):
        assert ctx.pyrlk_levels(w, h, win, max_level) == orc.pyrlk_levels(w, h, win, max_level)
        pts = R.point_classes(w, h, win, max_level, n_random=16)
        for flags in (0, 12):
            _check(ctx, orc, fr[0], fr[1], pts, R.guesses(pts, w, h), what="%dx%d" % size, win=win,
                   max_level=max_level, flags=flags)


@pytest.mark.parametrize("crit_type", [0, 1, 2, 3])
def test_criteria(ctx, orc, surf320, crit_type):
    pts = R.point_classes(320, 240, (21, 21), 3)
    for max_count in (0, 1, 5, 100, 1000):
        for epsilon in (-1.0, 0.0, 0.01, 0.1, 50.0):
            _check(ctx, orc, surf320[0], surf320[1], pts, what="criteria", win=(21, 21), max_level=3,
                   crit_type=crit_type, max_count=max_count, epsilon=epsilon, flags=0)


def test_min_eig_threshold_on_half_textured_frame(ctx, orc):
    """Half texture, half one grey level, fading contrast between: each threshold splits the points differently,
    and a point can fail at level 0 after coarser levels have moved it."""
    w, h = 320, 240
    a, b = R.half_texture_pair(w, h)
    ys, xs = np.mgrid[0:12, 0:32]
    pts = np.stack([xs.ravel() * 10 + 4.25, ys.ravel() * 20 + 6.5], axis=1).astype(np.float32)
    counts = []
    for thr in (0.0, 1e-4, 1e-2, 1.0):
        for flags in (0, 8):
            q, st, er = _check(ctx, orc, a, b, pts, what="half texture", win=(15, 15), max_level=3, flags=flags,
                               min_eig_threshold=thr)
        counts.append(int(st.sum()))
        if thr in (1e-4, 1e-2):
            assert ((st == 0) & (np.abs(q - pts).max(axis=1) > 0)).any()      # moved by a coarser level, then failed
    print("[parity] pyrlk tracked of %d by min_eig threshold: %s" % (len(pts), counts))
    assert len(pts) > counts[0] > counts[1] > counts[2] > counts[3] == 0


def test_points_carried_out_of_the_frame(ctx, orc):
    a, b = R.leaving_pair(320, 240)
    ys, xs = np.mgrid[0:20, 0:20]
    pts = np.stack([xs.ravel() * 1.5 - 2, ys.ravel() * 1.5 - 2], axis=1).astype(np.float32)
    for win in ((5, 5), (9, 5), (21, 21)):
        for flags in (0, 8):
            for max_level, max_count in ((2, 30), (0, 1), (0, 2), (1, 3)):
                _check(ctx, orc, a, b, pts, what="leaving", win=win, max_level=max_level, max_count=max_count, flags=flags)


def test_strided_inputs_with_an_odd_base_offset(ctx, orc, surf320):
    import torch
    w, h, pitch = 320, 240, 357
    views = []
    for k, off in enumerate((1, 3)):
        flat = torch.zeros(h * pitch + 8, dtype=torch.uint8, device="cuda")
        v = flat[off:off + h * pitch].view(h, pitch)[:, :w]
        v.copy_(torch.from_numpy(surf320[k]).cuda())
        assert v.data_ptr() % 2 == 1 and v.stride(0) == pitch
        views.append(v)
    pts = R.point_classes(w, h, (21, 21), 3)
    ref = _exact(orc, surf320[0], surf320[1], pts, win=(21, 21), max_level=3)
    q, st, er = ctx.calcOpticalFlowPyrLK(views[0], views[1], pts, win=(21, 21), max_level=3)
    assert not R.mismatch((q.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()), ref, 0)


def test_slot_one_and_scratch_regrown(ctx, orc, surf320):
    pts = R.point_classes(320, 240, (21, 21), 3)
    kw = dict(win=(21, 21), max_level=3, flags=0)
    for stream in (0, 1):
        small = _gpu(ctx, surf320[0], surf320[1], pts, stream=stream, **kw)
        big = synth.surf_clip(3840, 2160, 2)
        bp = R.point_classes(3840, 2160, (50, 50), 5)
        assert not R.mismatch(_gpu(ctx, big[0], big[1], bp, win=(50, 50), max_level=5, stream=stream),
                              _exact(orc, big[0], big[1], bp, win=(50, 50), max_level=5), 0)
        again = _gpu(ctx, surf320[0], surf320[1], pts, stream=stream, **kw)
        for x, y in zip(small, again):
            assert np.array_equal(x, y, equal_nan=True)
        assert not R.mismatch(small, _exact(orc, surf320[0], surf320[1], pts, **kw), 0)


@pytest.mark.parametrize("flags", [0, 8])
def test_err_absent(ctx, orc, flags):
    """d_err = NULL in rcflow_pyrlk_dev and err = NULL in rcflow_pyrlk_u8: upstream then skips the residual pass and
    the bounds test of the final position in it, so a point whose last step left the frame keeps status 1."""
    import torch
    a, b = R.leaving_pair(320, 240)
    ys, xs = np.mgrid[0:20, 0:20]
    pts = np.stack([xs.ravel() * 1.5 - 2, ys.ravel() * 1.5 - 2], axis=1).astype(np.float32)
    for win in ((5, 5), (9, 5)):
        kw = dict(win=win, max_level=0, max_count=2, flags=flags)
        with np.errstate(all="ignore"):
            ref = orc.pyrlk(a, b, pts, exact_sums=True, with_err=False, **kw)
        with_err = _exact(orc, a, b, pts, **kw)
        assert flags == 8 or (ref[1] != with_err[1]).sum() >= 5        # the case is in the data
        ta, tb, tp = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(pts).cuda()
        q = torch.zeros((len(pts), 2), device="cuda")
        st = torch.zeros(len(pts), dtype=torch.uint8, device="cuda")
        assert _c_pyrlk_dev(ctx, ta, tb, tp, q, st, None, win, max_level=0, max_count=2, flags=flags) == 0
        diff = R.mismatch((q.cpu().numpy(), st.cpu().numpy(), None), ref, flags)
        assert not diff, diff
        # host-pointer form, pitches above the width: err = NULL, then err given
        pa, pb = np.zeros((240, 333), np.uint8), np.zeros((240, 349), np.uint8)
        pa[:, :320], pb[:, :320] = a, b
        for erh, want in ((None, ref), (np.zeros(len(pts), np.float32), with_err)):
            qh, sth = np.zeros((len(pts), 2), np.float32), np.zeros(len(pts), np.uint8)
            rc = ctx._lib.rcflow_pyrlk_u8(ctx._h, 0, pa.ctypes.data, 333, pb.ctypes.data, 349, 320, 240, pts.ctypes.data,
                                          qh.ctypes.data, len(pts), sth.ctypes.data,
                                          None if erh is None else erh.ctypes.data, win[0], win[1], 0, 3, 2, 0.01,
                                          flags, 1e-4)
            diff = R.mismatch((qh, sth, erh), want, flags)
            assert rc == 0 and not diff, diff


@pytest.mark.parametrize("win", [(5, 9), (31, 15)])
def test_transposition_on_the_device(ctx, win):
    """Images transposed, x and y of points and guesses exchanged, window (win_h, win_w): the transposed answer, bit
    for bit.  Needs no second implementation; a width taken for a height anywhere breaks it."""
    w, h = 333, 251
    fr = synth.surf_clip(w, h, 2)
    pts = R.point_classes(w, h, win, 3)
    g = R.guesses(pts, w, h)
    for flags in (0, 4, 8):
        a = _gpu(ctx, fr[0], fr[1], pts, g, win=win, max_level=3, flags=flags)
        tp, tn, tpts, tg, twin = R.transpose_case(fr[0], fr[1], pts, g, win)
        b = _gpu(ctx, tp, tn, tpts, tg, win=twin, max_level=3, flags=flags)
        diff = R.mismatch((np.ascontiguousarray(b[0][:, ::-1]), b[1], b[2]), a, flags)
        assert not diff, diff


@pytest.mark.parametrize("win,eps,flags", [((5, 9), 0.01, 0), ((21, 21), 0.01, 4), ((31, 15), 0.1, 8)])
def test_against_the_numpy_restatement(ctx, win, eps, flags):
    """The device tied to tests/_lk_ref.py directly, not only through the oracle."""
    w, h = 333, 251
    fr = synth.surf_clip(w, h, 2)
    pts = R.point_classes(w, h, win, 3)
    g = R.guesses(pts, w, h)
    got = _gpu(ctx, fr[0], fr[1], pts, g, win=win, max_level=3, epsilon=eps, flags=flags)
    diff = R.mismatch(got, R.pyrlk(fr[0], fr[1], pts, g, win=win, max_level=3, epsilon=eps, flags=flags), flags)
    assert not diff, diff


def _cut_clip(n):
    """n frames of the 640x480 surf clip; the second half is cut to a smoothly shaded, low-contrast rendering of it,
    and its last quarter is 25 grey levels brighter: on shading that faint LK reads the brightness step as a motion of
    many pixels along the shading gradient."""
    a = synth.surf_clip(640, 480, n)
    y, x = np.mgrid[0:480, 0:640]
    out = a.copy()
    for t in range(n // 2, n):
        shaded = 50 + 0.2 * x + 0.1 * y + 0.25 * (a[t].astype(np.float64) - 128) + (25 if t >= 3 * n // 4 else 0)
        out[t] = np.clip(np.rint(shaded), 0, 255).astype(np.uint8)
    return out


def test_streakline_over_a_scene_cut(ctx, orc):
    """Streakline.runLK over 40 frames; at the cut and at the brightness step the tracker's jumps exceed a tenth of
    the frame and are reverted (Streakline.cpp:35-40).  Vertices equal to the exact-sum oracle chain after every frame."""
    fr = _cut_clip(41)
    gen = (300.0, 200.0)
    sl = Streakline(gen)
    verts = np.zeros((64, 2), np.float32)
    verts[0] = gen
    n, fc, reverted = 1, 1, 0
    for t in range(40):
        before = verts[:n].copy()
        with np.errstate(all="ignore"):
            q, _, _ = orc.pyrlk(fr[t], fr[t + 1], before, win=(50, 50), max_level=3, epsilon=0.1, flags=10,
                                exact_sums=True)
        reverted += int(((np.abs(before[:, 0] - q[:, 0]) > 64) | (np.abs(before[:, 1] - q[:, 1]) > 48)).sum())
        sl.runLK(ctx, fr[t], fr[t + 1])
        n, fc = orc.streakline_step_lk(verts, n, gen, fr[t], fr[t + 1], fc, exact_sums=True)
        assert sl.numberOfVertices == n and sl.frameCount == fc
        assert np.array_equal(np.asarray(sl.vertices, np.float32), verts[:n]), "frame %d" % t
    print("[parity] streakline over a cut: %d jumps reverted" % reverted)
    assert reverted >= 1


def test_timeline_and_population_map_exact(ctx, orc):
    fr = _cut_clip(11)
    tl = Timeline((100.0, 100.0), (500.0, 300.0), 24)
    pm = PopulationMap((50.0, 60.0), (150.0, 160.0), 40, rng=np.random.RandomState(3))
    for obj in (tl, pm):
        ref = np.asarray(obj.vertices, np.float32)
        for t in range(10):
            obj.runLK(ctx, fr[t], fr[t + 1])
            ref, _, _ = _exact(orc, fr[t], fr[t + 1], ref, ref, win=(50, 50), max_level=3, epsilon=0.1, flags=10)
            assert np.array_equal(np.asarray(obj.vertices, np.float32), ref), "frame %d" % t


def test_exact_golden_fixture(ctx):
    """tests/golden/pyrlk_exact_160x120.npz: inputs and exact-sum oracle outputs (tests/golden/make_golden.py), so a
    change that moves the oracle and the kernel together is still seen."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyrlk_exact_160x120.npz"))
    for tag, win, eps, flags in R.GOLDEN_CASES:
        got = _gpu(ctx, g["prev"], g["next"], g["pts"], g["guess"], win=win, max_level=3, epsilon=eps, flags=flags)
        diff = R.mismatch(got, (g["next_" + tag], g["status_" + tag], g["err_" + tag]), flags)
        assert not diff, "%s: %s" % (tag, diff)
