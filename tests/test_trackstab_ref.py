"""CPU tier of the tracking stabiliser: known answers of the numpy statement (tests/_trackstab_ref.py) the device is held
to, and the whole chain (reference corners -> the exact-sum PyrLK oracle -> reference fit -> the numpy warp) on a clip."""
import math

import numpy as np

import _framewarp_ref as W
import _trackstab_ref as R
from ripcurrents_amd import synth


def _response_by_hand(g, x, y):
    """R of one pixel in plain Python integers with math.isqrt."""
    g = g.astype(int)
    a = b = c = 0
    for v in (-1, 0, 1):
        for u in (-1, 0, 1):
            yy, xx = y + v, x + u
            dx = (g[yy - 1, xx + 1] + 2 * g[yy, xx + 1] + g[yy + 1, xx + 1]) - (g[yy - 1, xx - 1] + 2 * g[yy, xx - 1] + g[yy + 1, xx - 1])
            dy = (g[yy + 1, xx - 1] + 2 * g[yy + 1, xx] + g[yy + 1, xx + 1]) - (g[yy - 1, xx - 1] + 2 * g[yy - 1, xx] + g[yy - 1, xx + 1])
            a += dx * dx; b += dx * dy; c += dy * dy
    return int(a + c - R.isqrt_ceil(int((a - c) ** 2 + 4 * b * b)))


def test_corner_response_known_answers():
    flat = np.full((40, 60), 91, np.uint8)
    pts, sc = R.corner_cells(flat, 3, 2, 4, 1)
    assert not sc.any()
    # candidates 52 x 32 from (4, 4): cells of 17 x 16, the last column 18 wide
    assert np.array_equal(pts[0], [4 + 8.0, 4 + 7.5]) and np.array_equal(pts[2], [38 + 8.5, 4 + 7.5]) and np.array_equal(pts[5], [46.5, 27.5])
    # a step edge has one zero eigenvalue everywhere: R = 0 along it
    edge = np.zeros((40, 60), np.uint8); edge[:, 30:] = 200
    assert not R.corner_response(edge).any() and not R.corner_cells(edge, 3, 2, 4, 1)[1].any()
    # a bright square: its four corners, one per cell, equal by symmetry; the value worked by hand.  At the corner pixel
    # the block holds dx = dy = 255 k for k in (1, 3; 3, 3 ...): a = c, so R = 2 a - 2 |b|
    sq = np.zeros((60, 80), np.uint8); sq[20:40, 30:50] = 255
    pts, sc = R.corner_cells(sq, 2, 2, 4, 1)
    assert len(set(sc.tolist())) == 1 and sc[0] > 0
    assert sc[0] == _response_by_hand(sq, int(pts[0, 0]), int(pts[0, 1]))
    assert [tuple(p) for p in pts] == [(30.0, 20.0), (49.0, 20.0), (30.0, 39.0), (49.0, 39.0)]
    # every response equals the plain-integer statement, on noise
    img = np.random.RandomState(1).randint(0, 256, (30, 41)).astype(np.uint8)
    Rm = R.corner_response(img)
    for (x, y) in ((2, 2), (38, 27), (17, 9), (20, 20)):
        assert Rm[y, x] == _response_by_hand(img, x, y)
    assert R.isqrt_ceil(16) == 4 and R.isqrt_ceil(17) == 5 and R.isqrt_ceil(0) == 0 and R.isqrt_ceil((1 << 48) + 1) == (1 << 24) + 1


def test_corner_ties_remainders_margins_and_gate():
    # two identical squares in one cell: the upper-left corner of the upper one wins
    img = np.zeros((64, 64), np.uint8); img[10:20, 10:20] = 255; img[40:50, 10:20] = 255
    pts, sc = R.corner_cells(img, 1, 1, 2, 1)
    assert tuple(pts[0]) == (10.0, 10.0)
    # the margin excludes it
    pts, _ = R.corner_cells(img, 1, 1, 12, 1)
    assert pts[0, 0] >= 12 and pts[0, 1] >= 12
    # remainder pixels go to the last cell: a corner at x = 61 of a 64-wide image with margin 2 and 7 cells of 8
    img = np.zeros((64, 64), np.uint8); img[30:34, 58:62] = 255
    pts, sc = R.corner_cells(img, 7, 1, 2, 1)
    assert sc[6] > 0 and pts[6, 0] >= 58 and not sc[:6].any()
    # the gate
    assert not R.corner_cells(img, 7, 1, 2, int(sc[6]) + 1)[1].any() and R.corner_cells(img, 7, 1, 2, int(sc[6]))[1][6] == sc[6]
    assert R.default_cells(640, 480) == (16, 12) and R.default_cells(1920, 1080) == (48, 27) and R.default_cells(3840, 2160) == (80, 45)


def test_sampler_fixed_vectors():
    assert [R.draw(0, 0, 0), R.draw(0, 0, 1), R.draw(1, 0, 0), R.draw(12345, 7, 3), R.draw(0xffffffff, 4095, 15)] == \
        [3713553442, 4112612813, 3469932832, 4192828979, 4140769267]
    assert R.sample(0, 0, 4, 100) == [86, 95, 59, 87] and R.sample(5, 17, 3, 192) == [144, 29, 42] and R.sample(5, 17, 2, 2) == [1, 0]
    assert R.sample(1, 0, 4, 3) is None and R.sample(9, 2, 1, 1) == [0]
    got = [R.sample(1, j, 4, 4) for j in range(12)]
    assert got[8] is None                                   # 16 draws did not bring four distinct indices out of four
    assert all(g is None or sorted(g) == [0, 1, 2, 3] for g in got) and got[3] == [1, 3, 0, 2]


def _pairs(T, n, seed, outliers, w=640, h=480):
    rng = np.random.RandomState(seed)
    p = np.stack([rng.randint(10, w - 10, n), rng.randint(10, h - 10, n)], 1).astype(np.float64)
    ph = np.concatenate([p, np.ones((n, 1))], 1) @ T.T
    q = ph[:, :2] / ph[:, 2:]
    bad = rng.rand(n) < outliers
    q[bad] += rng.choice([-1, 1], (int(bad.sum()), 2)) * rng.uniform(5, 60, (int(bad.sum()), 2))
    return p.astype(np.float32), q.astype(np.float32), bad


def test_fit_recovers_planted_motions_and_inliers():
    c, s = math.cos(0.02), math.sin(0.02)
    mats = {1: np.array([[1, 0, 3.25], [0, 1, -2.5], [0, 0, 1.0]]),
            2: np.array([[1.01 * c, -1.01 * s, 3.25], [1.01 * s, 1.01 * c, -2.5], [0, 0, 1.0]]),
            3: np.array([[1.02, 0.015, 3.25], [-0.01, 0.99, -2.5], [0, 0, 1.0]]),
            4: np.array([[1.02, 0.015, 3.25], [-0.01, 0.99, -2.5], [2e-5, -3e-5, 1.0]])}
    for model, T in mats.items():
        p, q, bad = _pairs(T, 300, model, 0.6)
        r = R.fit_motion(p, q, np.ones(300, np.uint8), (640, 480), model=model, seed=3)
        assert r["model_used"] == model and np.array_equal(r["inlier"] == 1, ~bad), model
        # integer p and a translation by quarters are exact in float32: 1e-9; elsewhere q carries float32 rounding (3e-5 px)
        assert np.abs(r["T"] - T).max() < (1e-9 if model == 1 else 2e-4), (model, np.abs(r["T"] - T).max())
        assert r["edge"] > 1e-6
    p, q, _ = _pairs(mats[4], 200, 9, 0.5)
    r = R.fit_motion(p, p.copy(), np.ones(200, np.uint8), (640, 480), model=4)
    assert np.array_equal(r["T"], np.eye(3)) and r["n_inliers"] == 200 and r["result"] == (0.0, 0.0, 1.0)


def test_fit_ladder_gates_and_degenerate_input():
    T = np.array([[1.0, -0.01, 2.0], [0.01, 1.0, -1.0], [0, 0, 1.0]])
    p, q, _ = _pairs(T, 40, 2, 0.0)
    st = np.zeros(40, np.uint8)
    for keep, model, want in ((8, 4, 4), (7, 4, 3), (5, 3, 2), (3, 2, 0), (2, 1, 0)):
        st[:] = 0; st[:keep] = 1
        r = R.fit_motion(p, q, st, (640, 480), model=model, hypotheses=64)
        assert r["model_used"] == want and r["n_valid"] == keep, (keep, model, r["model_used"])
    tr = np.array([[1.0, 0, 2.0], [0, 1.0, -1.0], [0, 0, 1.0]])
    p1, q1, _ = _pairs(tr, 3, 3, 0.0)
    assert R.fit_motion(p1, q1, np.ones(3, np.uint8), (640, 480), model=3, hypotheses=64)["model_used"] == 1
    # gates: status, score floor, quality against the largest score, the jump rule
    sc = np.arange(40, dtype=np.int32) * 10
    st[:] = 1; st[35] = 0
    r = R.fit_motion(p, q, st, (640, 480), scores=sc, model=2, min_score=100, quality=0.5)
    assert r["n_valid"] == 19 and not r["inlier"][:20].any() and not r["inlier"][35]        # scores 200 .. 390 without index 35
    qq = q.copy(); qq[0] += 100.0
    assert R.fit_motion(p, qq, np.ones(40, np.uint8), (640, 480), model=2)["n_valid"] == 39
    assert R.fit_motion(p, qq, np.ones(40, np.uint8), (640, 480), model=2, max_shift=1.0)["n_valid"] == 0
    r = R.fit_motion(p[:0], q[:0], st[:0], (640, 480), model=3)
    assert r["model_used"] == 0 and np.array_equal(r["T"], np.eye(3)) and r["result"] == (0.0, 0.0, 0.0)
    # collinear pairs: every affine sample is void (the identity); a similarity fits them
    pc = np.stack([np.linspace(50, 600, 30), np.linspace(40, 440, 30)], 1).astype(np.float32)
    qc = pc + np.float32([2.0, -1.0])
    assert R.fit_motion(pc, qc, np.ones(30, np.uint8), (640, 480), model=3, hypotheses=64)["model_used"] == 0
    assert R.fit_motion(pc, qc, np.ones(30, np.uint8), (640, 480), model=2, hypotheses=64)["model_used"] == 2
    # the summation order is the stated one
    v = np.random.RandomState(4).rand(1000)
    acc = np.zeros(256)
    for i in range(1000):
        acc[i % 256] += v[i]
    w4 = []
    for k in range(4):
        x = acc[64 * k:64 * k + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            x = x[:o] + x[o:2 * o]
        w4.append(x[0])
    assert R.blk_sum(v) == ((w4[0] + w4[1]) + w4[2]) + w4[3]


def test_homography_beats_affine_on_a_keystone():
    """A tilting pole: the affine model leaves the far corners out, the homography does not.  Measured here: affine 9.8 px at
    the worst frame corner against 4e-6 px; asserted with margin as > 1.0 and < 1e-3."""
    H = np.array([[1.0, 0.004, 1.5], [-0.003, 1.0, -2.0], [6e-5, -4e-5, 1.0]])
    ys, xs = np.mgrid[20:480:40, 20:640:40]
    p = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    ph = np.concatenate([p, np.ones((len(p), 1))], 1) @ H.T
    q = (ph[:, :2] / ph[:, 2:]).astype(np.float32)
    corners = np.array([[0, 0, 1.0], [639, 0, 1], [0, 479, 1], [639, 479, 1]])
    want = corners @ H.T
    want = want[:, :2] / want[:, 2:]
    err = {}
    for model in (3, 4):
        r = R.fit_motion(p.astype(np.float32), q, np.ones(len(p), np.uint8), (640, 480), model=model, inlier_px=3.0)
        assert r["model_used"] == model
        got = corners @ r["T"].T
        err[model] = float(np.abs(got[:, :2] / got[:, 2:] - want).max())
    assert err[3] > 1.0 and err[4] < 1e-3, err


def test_whole_chain_holds_the_shore_where_surf_polluted_patches_do_not(orc):
    """Static textured shore, moving surf over the middle, roll + zoom + shake (W.rolling_clip).  The tracks chain
    (corners -> exact-sum PyrLK -> robust similarity -> warp, chained) against the 4-patch similarity reference with two of
    its four patches on the surf.  Measured here over 8 frames: tracks hold the four shore patches within 0.15 px of frame 0,
    the polluted patches drift 1.9 px; asserted as < 0.3 and > 0.6."""
    n, w, h = 8, 640, 480
    water = synth.surf_clip(240, 160, n, seed=99)
    frames, _ = W.rolling_clip(w, h, n, seed=7, water=water)
    cells = R.default_cells(w, h)
    shore = W.corner_rois(w, h)
    kept, worst = frames[0], 0.0
    for k in range(1, n):
        gray = R.bgr_to_gray(kept)
        pts, scores = R.corner_cells(gray, cells[0], cells[1], 12, 1)
        q, st, _ = orc.pyrlk(gray, R.bgr_to_gray(frames[k]), pts, win=(21, 21), max_level=3, exact_sums=True, with_err=False)
        fit = R.fit_motion(pts, q, st, (w, h), scores=scores, model=2, min_score=1, seed=5)
        assert fit["model_used"] == 2 and fit["n_inliers"] >= 60
        # the water is thrown out by consensus: few inliers inside the painted rectangle
        inside = (np.abs(pts[:, 0] - 319.5) < 110) & (np.abs(pts[:, 1] - 239.5) < 70)
        assert fit["inlier"][inside].mean() < 0.2 and fit["inlier"][~inside].mean() > 0.6
        kept = W.warp_affine(frames[k], fit["T"][:2], inverse_map=True)
        worst = max(worst, max(W.patch_drift(r, frames[0], kept) for r in shore))
    rois = [shore[0], shore[3], (260, 200, 50, 50), (330, 240, 50, 50)]             # two on the shore, two on the surf
    stab = W.MultiStabRef(w, h, rois, "similarity", 0.0)
    polluted = 0.0
    for k in range(n):
        out = stab.push(frames[k])[0]
        if k:
            polluted = max(polluted, max(W.patch_drift(r, frames[0], out) for r in shore))
    assert worst < 0.3 and polluted > 0.6, (worst, polluted)
