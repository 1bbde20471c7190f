"""Corner cells, the robust fit and the tracking stabiliser on the device (corner_kernels.hip, fit_kernels.hip,
stab_kernels.hip) against their numpy statement (tests/_trackstab_ref.py): integers bit for bit, T within 1e-9."""
import numpy as np
import pytest
import torch

import _framewarp_ref as W
import _trackstab_ref as R
from _dev import EINVAL, ESIZE, ESTATE
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RcflowError

pytestmark = pytest.mark.gpu

NAMES = {v: k for k, v in R.MODELS.items()}


def _textured(h, w, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (h // 4 + 2, w // 4 + 2)).astype(np.float64)
    img = np.kron(img, np.ones((4, 4)))[:h, :w]
    return np.clip(img + rng.randint(-20, 21, (h, w)), 0, 255).astype(np.uint8)


def _check_corners(ctx, img, cells, margin, min_score, dev=None):
    dev = torch.as_tensor(img).cuda() if dev is None else dev
    pts, sc = ctx.corners(dev, cells, margin, min_score)
    ctx.sync()
    rp, rs = R.corner_cells(img, cells[0], cells[1], margin, min_score)
    assert np.array_equal(sc.cpu().numpy(), rs), (img.shape, cells, margin)
    assert np.array_equal(pts.cpu().numpy(), rp), (img.shape, cells, margin)
    return rs


@pytest.mark.parametrize("w,h,cells,margin", [(640, 480, (16, 12), 12), (1920, 1080, (48, 27), 12), (3840, 2160, (80, 45), 12),
                                              (333, 251, (7, 5), 2), (101, 67, (1, 1), 5), (640, 480, (1, 1), 2), (640, 480, (77, 53), 12),
                                              (1031, 517, (64, 64), 2)])
def test_corner_cells_equal_the_reference(ctx, w, h, cells, margin):
    img = _textured(h, w, w + h) if w < 3000 else np.random.RandomState(5).randint(0, 256, (h, w)).astype(np.uint8)
    rs = _check_corners(ctx, img, cells, margin, 1)
    assert (rs > 0).mean() > 0.9


def test_corner_cells_structured_images_and_padded_rows(ctx):
    flat = np.full((120, 160), 77, np.uint8)
    assert not _check_corners(ctx, flat, (4, 3), 4, 1).any()
    sq = np.zeros((120, 160), np.uint8); sq[40:80, 50:110] = 255
    assert (_check_corners(ctx, sq, (2, 2), 4, 1) > 0).all()
    edge = np.zeros((120, 160), np.uint8); edge[:, 80:] = 200
    assert not _check_corners(ctx, edge, (4, 3), 4, 1).any()
    ramp = (np.add.outer(np.arange(120), np.arange(160)) % 256).astype(np.uint8)          # many ties
    _check_corners(ctx, ramp, (5, 4), 3, 1)
    img = _textured(200, 300, 3)
    _check_corners(ctx, img, (6, 4), 6, 10 ** 6)                                            # a gate most cells fail
    buf = torch.full((210, 340), 9, dtype=torch.uint8, device="cuda")
    buf[5:205, 17:317] = torch.as_tensor(img).cuda()
    _check_corners(ctx, img, (6, 4), 6, 1, dev=buf[5:205, 17:317])
    for bad in (dict(cells=(0, 1)), dict(cells=(65, 64)), dict(margin=1), dict(cells=(40, 4)), dict(min_score=-1)):
        kw = dict(cells=(4, 4), margin=4, min_score=1); kw.update(bad)
        with pytest.raises(RcflowError) as e:
            ctx.corners(torch.as_tensor(img).cuda(), **kw)
        assert e.value.code == EINVAL


def _scene(model, n, seed, w=640, h=480, outliers=0.6):
    """n pairs under a known motion of `model`, a fraction of gross outliers, float32 pairs (so not exact)."""
    rng = np.random.RandomState(seed)
    p = np.stack([rng.uniform(10, w - 10, n), rng.uniform(10, h - 10, n)], 1)
    ang, s = np.deg2rad(1.5), 1.01
    T = np.eye(3)
    if model >= 2:
        T[:2, :2] = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    if model >= 3:
        T[:2, :2] = T[:2, :2] @ np.array([[1.0, 0.02], [0.0, 0.99]])
    if model == 4:
        T[2, :2] = (2e-5, -3e-5)
    T[:2, 2] = (3.25, -2.5)
    ph = np.concatenate([p, np.ones((n, 1))], 1) @ T.T
    q = ph[:, :2] / ph[:, 2:]
    bad = rng.rand(n) < outliers
    q[bad] += rng.uniform(-40, 40, (int(bad.sum()), 2))
    status = (rng.rand(n) > 0.05).astype(np.uint8)
    return p.astype(np.float32), q.astype(np.float32), status, T


def _check_fit(ctx, p, q, status, size, scores=None, **kw):
    m = kw.pop("model", "similarity")
    got = ctx.fit_motion(p, q, status, size, scores=scores, model=m, want_samples=True, **kw)
    ref = R.fit_motion(p, q, status, size, scores=scores, model=R.MODELS[m], **kw)
    assert ref["edge"] > 1e-9, "a point sits on the inlier threshold: choose another scene"
    assert np.array_equal(got["samples"], ref["samples"])
    assert got["winner"] == ref["winner"] and got["n_valid"] == ref["n_valid"] and got["n_inliers"] == ref["n_inliers"]
    assert got["model_used"] == NAMES.get(ref["model_used"])
    assert np.array_equal(got["inlier"], ref["inlier"])
    assert np.allclose(got["T"], ref["T"], rtol=1e-9, atol=1e-12)
    return got, ref


@pytest.mark.parametrize("model", ["translation", "similarity", "affine", "homography"])
def test_fit_motion_equals_the_reference(ctx, model):
    for n, seed, hyp in ((200, 1, 0), (4096, 2, 256), (37, 3, 64)):
        p, q, st, T = _scene(R.MODELS[model], n, seed)
        got, ref = _check_fit(ctx, p, q, st, (640, 480), model=model, hypotheses=hyp, seed=seed)
        assert got["model_used"] == model and got["n_inliers"] > 0.25 * n
        assert np.abs(got["T"] - T).max() < (2e-2 if model != "homography" else 5e-2), (model, n)
    sc = np.random.RandomState(9).randint(0, 5000, 200).astype(np.int32)
    p, q, st, _ = _scene(R.MODELS[model], 200, 4, outliers=0.3)
    _check_fit(ctx, p, q, st, (640, 480), scores=sc, model=model, min_score=500, quality=0.2, seed=11)


def test_fit_motion_ladder_and_edges(ctx):
    p, q, st, _ = _scene(2, 200, 5)
    # identity in: T = I bit for bit, every valid pair an inlier
    got, _ = _check_fit(ctx, p, p.copy(), st, (640, 480), model="homography")
    assert np.array_equal(got["T"], np.eye(3)) and got["n_inliers"] == got["n_valid"] == int(st.sum())
    # nothing to fit
    for kw in (dict(p=p[:0], q=q[:0], status=st[:0]), dict(p=p, q=q, status=np.zeros_like(st))):
        got = ctx.fit_motion(kw["p"], kw["q"], kw["status"], (640, 480), model="affine")
        assert got["model_used"] is None and np.array_equal(got["T"], np.eye(3)) and got["n_valid"] == 0 and got["n_inliers"] == 0
    # the ladder: 5 consistent pairs cannot carry an affine model (6) but carry a similarity (4); 3 carry a translation only
    # when they agree with one; 2 carry nothing
    for keep, model, want in ((5, "affine", "similarity"), (7, "homography", "affine"), (3, "similarity", None), (2, "translation", None)):
        pp, qq, ss, _ = _scene(2, 40, 6, outliers=0.0)
        ss[:] = 0; ss[:keep] = 1
        got, ref = _check_fit(ctx, pp, qq, ss, (640, 480), model=model, hypotheses=64)
        assert got["model_used"] == want, (keep, model, got["model_used"])
    pp, qq, ss, _ = _scene(1, 40, 7, outliers=0.0)
    ss[:] = 0; ss[:3] = 1
    assert _check_fit(ctx, pp, qq, ss, (640, 480), model="affine", hypotheses=64)[0]["model_used"] == "translation"
    # collinear points: every affine sample is void, so there is no winner and no inlier to step down with (the identity);
    # asked for a similarity, the same pairs give one
    pc = np.stack([np.linspace(50, 600, 30), np.linspace(40, 440, 30)], 1).astype(np.float32)
    qc = (pc * np.float32(1.0) + np.float32([2.0, -1.0])).astype(np.float32)
    assert _check_fit(ctx, pc, qc, np.ones(30, np.uint8), (640, 480), model="affine", hypotheses=64)[0]["model_used"] is None
    assert _check_fit(ctx, pc, qc, np.ones(30, np.uint8), (640, 480), model="similarity", hypotheses=64)[0]["model_used"] == "similarity"
    # hypotheses 1 and 4096; two seeds draw different samples, as the reference says
    _check_fit(ctx, p, q, st, (640, 480), model="similarity", hypotheses=1, seed=3)
    a, _ = _check_fit(ctx, p, q, st, (640, 480), model="affine", hypotheses=4096, seed=3)
    b, _ = _check_fit(ctx, p, q, st, (640, 480), model="affine", hypotheses=4096, seed=4)
    assert not np.array_equal(a["samples"], b["samples"])
    for bad in (dict(hypotheses=4097), dict(quality=1.5), dict(inlier_px=-1.0), dict(max_shift=float("nan"))):
        with pytest.raises(RcflowError) as e:
            ctx.fit_motion(p, q, st, (640, 480), **bad)
        assert e.value.code == EINVAL


@pytest.fixture(scope="module")
def clip():
    water = synth.surf_clip(240, 160, 14, seed=99)
    return W.rolling_clip(640, 480, 14, seed=7, water=water)


def _ref_push(orc, ref_gray, pts, scores, frame, prm):
    """What one push must compute from the kept gray image and corners: tracks, fit, corrected frame."""
    w, h = frame.shape[1], frame.shape[0]
    q, st, _ = orc.pyrlk(ref_gray, R.bgr_to_gray(frame), pts, win=(21, 21), max_level=3, exact_sums=True, with_err=False)
    fit = R.fit_motion(pts, q, st, (w, h), scores=scores, model=R.MODELS[prm["model"]], min_score=1, seed=prm.get("seed", 0))
    return q, st, fit


@pytest.mark.parametrize("anchor,model", [("previous", "similarity"), ("first", "similarity"), ("previous", "homography"), ("first", "affine")])
def test_session_push_by_push(ctx, orc, clip, anchor, model):
    frames, motions = clip
    w, h = 640, 480
    prm = dict(model=model, seed=5)
    ctx.framestab_open_tracks(w, h, model=model, seed=5, anchor=anchor)
    cells = R.default_cells(w, h)
    assert cells == (16, 12) and ctx.framestab_motion()["rois"] == []
    out = ctx.framestab_push(frames[0])
    assert torch.equal(out, torch.as_tensor(frames[0]).cuda())
    t = ctx.framestab_read_tracks()
    assert np.array_equal(t["T"], np.eye(3)) and t["model_used"] is None and t["n_valid"] == 0 and t["frames_pushed"] == 1
    assert ctx.framestab_read() == ((0.0, 0.0, 0.0), 1)
    kept = frames[0]
    resid = []
    for k in range(1, len(frames)):
        gray = R.bgr_to_gray(kept)
        pts, scores = R.corner_cells(gray, cells[0], cells[1], 12, 1)
        res3 = torch.zeros(3, dtype=torch.float64, device="cuda")
        out = ctx.framestab_push(frames[k], result=res3).cpu().numpy()
        t = ctx.framestab_read_tracks()
        assert np.array_equal(t["pts"][:, :2], pts) and np.array_equal(t["scores"], scores), "kept corners differ at push %d" % k
        q, st, fit = _ref_push(orc, gray, pts, scores, frames[k], prm)
        ok = st == 1
        assert np.array_equal(t["pts"][ok, 2:], q[ok]), "tracks differ at push %d" % k
        assert fit["edge"] > 1e-9
        assert t["n_valid"] == fit["n_valid"] and t["n_inliers"] == fit["n_inliers"] and t["model_used"] == NAMES.get(fit["model_used"])
        assert np.array_equal(t["inlier"], fit["inlier"]), "inlier bytes differ at push %d" % k
        assert np.allclose(t["T"], fit["T"], rtol=1e-9, atol=1e-12)
        warp = W.warp_perspective if model == "homography" else W.warp_affine
        M = t["T"] if model == "homography" else t["T"][:2]
        assert np.array_equal(out, warp(frames[k], M, inverse_map=True)), "corrected frame differs at push %d" % k
        r3, n = ctx.framestab_read()
        assert n == k + 1 and np.allclose(r3, fit["result"], rtol=1e-9, atol=1e-12) and np.array_equal(res3.cpu().numpy(), np.array(r3))
        if model != "homography":
            assert np.array_equal(ctx.framestab_motion()["motion"], t["T"][:2])
        if anchor == "previous":
            kept = out
        # the shore (outside the water in the middle) stays where frame 0 has it
        resid.append(max(W.patch_drift(roi, frames[0], out) for roi in W.corner_rois(w, h)))
        assert t["n_inliers"] >= 60
    assert max(resid) < 0.5, resid
    ctx.framestab_close()


def test_session_still_clip_lifecycle_and_refusals(ctx, clip):
    frames, _ = clip
    f0 = torch.as_tensor(frames[0]).cuda()
    ctx.framestab_open_tracks(640, 480, model="homography")
    for k in range(3):
        assert torch.equal(ctx.framestab_push(f0), f0)
        t = ctx.framestab_read_tracks()
        assert np.array_equal(t["T"], np.eye(3)) and t["frames_pushed"] == k + 1
        if k:
            assert t["model_used"] == "homography" and t["n_inliers"] == t["n_valid"] > 100
            with pytest.raises(RcflowError) as e:
                ctx.framestab_motion()
            assert e.value.code == EINVAL
    info = ctx.framestab_info()
    assert info["roi"] == (12, 12, 616, 456) and info["launches_per_push"] == 4 + 3 + 3 + 6
    ctx.framestab_reset()
    assert ctx.framestab_read_tracks()["frames_pushed"] == 0
    assert torch.equal(ctx.framestab_push(f0), f0) and ctx.framestab_read_tracks()["model_used"] is None
    # refused re-opens leave the state as it was
    for bad, code in ((dict(win=20), EINVAL), (dict(cells=(200, 2)), EINVAL), (dict(hypotheses=5000), EINVAL), (dict(w=5000), ESIZE),
                      (dict(quality=2.0), EINVAL), (dict(max_level=9), EINVAL)):
        kw = dict(w=640, h=480, model="homography"); kw.update(bad)
        with pytest.raises(RcflowError) as e:
            ctx.framestab_open_tracks(**kw)
        assert e.value.code == code, bad
        assert ctx.framestab_read_tracks()["frames_pushed"] == 1
    # an accepted re-open, on two streams, independent of each other
    ctx.framestab_open_tracks(640, 480, model="similarity", stream=0)
    ctx.framestab_open_tracks(640, 480, model="affine", anchor="first", stream=1)
    a = [ctx.framestab_push(frames[k], stream=0).cpu().numpy() for k in range(3)]
    b = [ctx.framestab_push(frames[k], stream=1).cpu().numpy() for k in range(3)]
    assert ctx.framestab_read_tracks(stream=0)["model_used"] == "similarity" and ctx.framestab_read_tracks(stream=1)["model_used"] == "affine"
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])
    ctx.framestab_close(stream=1)
    ctx.framestab_close(stream=0)
    with pytest.raises(RcflowError) as e:
        ctx.framestab_read_tracks()
    assert e.value.code == ESTATE
    # the two older forms still answer as they did, and have no tracks
    ctx.framestab_open(640, 480, roi=(20, 20, 50, 50))
    with pytest.raises(RcflowError) as e:
        ctx.framestab_read_tracks()
    assert e.value.code == ESTATE
    one = [ctx.framestab_push(frames[k]).cpu().numpy() for k in range(3)]
    ctx.framestab_open(640, 480, rois=[(20, 20, 50, 50)], model="translation")
    multi = [ctx.framestab_push(frames[k]).cpu().numpy() for k in range(3)]
    assert all(np.array_equal(x, y) for x, y in zip(one, multi))
    ctx.framestab_close()
