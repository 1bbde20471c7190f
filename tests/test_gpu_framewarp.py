"""General warps and the multi-patch stabiliser on the device (warp_kernels.hip, stab_kernels.hip) against the numpy
restatement (tests/_framewarp_ref.py): the warps bit for bit on the destination-to-source matrix, the per-patch shifts
within 1e-3 px (fp32 direct DFT sums against np.fft in double), the fitted motion within 1e-9 of the numpy fit of the
device's own shifts, the corrected frame bit for bit against the numpy warp fed the device's own motion."""
import ctypes as C

import numpy as np
import pytest
import torch

import _framestab_ref as S
import _framewarp_ref as W
from _dev import EINVAL, ESIZE, ESTATE
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RcflowError
from ripcurrents_amd.api import Context

pytestmark = pytest.mark.gpu

SIZES = ((640, 480), (333, 251), (1920, 1080), (5, 3), (4, 1))


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _random_affine(rng, w, h):
    """Destination-to-source: rotation within 5 degrees, scale 0.9..1.1, a little shear, a shift with a fraction."""
    ang, s, sh = np.deg2rad(rng.uniform(-5, 5)), rng.uniform(0.9, 1.1), rng.uniform(-0.03, 0.03)
    A = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) @ np.array([[1, sh], [0, 1]])
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    return np.hstack([A, (c - A @ c + rng.uniform(-6, 6, 2))[:, None]])


def _random_keystone(rng, w, h):
    M = np.vstack([_random_affine(rng, w, h), [0, 0, 1]])
    M[2, :2] = rng.uniform(-1, 1, 2) * 0.1 / max(w, h)
    return M


def test_warp_affine_bit_exact(ctx):
    rng = np.random.RandomState(21)
    for (w, h) in SIZES:
        img = _img(h, w, w)
        dev = torch.as_tensor(img).cuda()
        mats = [_random_affine(rng, w, h) for _ in range(3)]
        mats += [np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[1.0, 0, w], [0, 1.0, 0.3]]),            # all outside
                 np.array([[1.0, 0, w - 1.5], [0, 1.0, h - 1.5]]), np.array([[0.5, 0, -w / 3.0], [0.1, 2.0, -h / 2.0]]),
                 np.array([[-1.0, 0, w - 1.0], [0, -1.0, h - 1.0]])]
        for M in mats:
            got = ctx.warp_affine(dev, M, inverse_map=True).cpu().numpy()
            assert np.array_equal(got, W.warp_affine(img, M, inverse_map=True)), (w, h, M)
    assert np.array_equal(ctx.warp_affine(dev, [[1, 0, 0], [0, 1, 0]]).cpu().numpy(), img)


def test_warp_perspective_bit_exact(ctx):
    rng = np.random.RandomState(22)
    for (w, h) in SIZES:
        img = _img(h, w, w + 1)
        dev = torch.as_tensor(img).cuda()
        mats = [_random_keystone(rng, w, h) for _ in range(3)]
        mats += [np.eye(3), np.diag([1.0, 1.0, 2.0]), np.array([[1.0, 0, 0], [0, 1.0, 0], [2.0 / w, 0, -1.0]]),      # W changes sign inside
                 np.array([[1.0, 0, 0], [0, 1.0, 0], [0.1, 0, -1.0]]),                                               # W = 0 on column 10
                 np.array([[1e300, 0, 1e300], [0, 1.0, 0], [0, 0, 1e-300]]), np.array([[0.1, 0, 0], [0, 0.1, 0], [0, 0, 1.0]])]
        for M in mats:
            got = ctx.warp_perspective(dev, M, inverse_map=True).cpu().numpy()
            assert np.array_equal(got, W.warp_perspective(img, M, inverse_map=True)), (w, h, M)


def test_warp_destination_size_steps_and_guards(ctx):
    rng = np.random.RandomState(23)
    buf = torch.as_tensor(_img(70, 120, 5)).cuda()
    src = buf[4:64, 9:102]                                 # 93 x 60, row step 360
    img = src.cpu().numpy()
    for (dw, dh) in ((41, 77), (200, 30), (93, 60), (258, 17), (1, 1)):
        outbuf = torch.full((dh + 2, dw + 11, 3), 201, dtype=torch.uint8, device="cuda")
        view = outbuf[1:dh + 1, 6:dw + 6]
        A, H = _random_affine(rng, 93, 60), _random_keystone(rng, 93, 60)
        ctx.warp_affine(src, A, inverse_map=True, dsize=(dw, dh), out=view)
        assert np.array_equal(view.cpu().numpy(), W.warp_affine(img, A, (dw, dh), True)), (dw, dh)
        ctx.warp_perspective(src, H, inverse_map=True, dsize=(dw, dh), out=view)
        assert np.array_equal(view.cpu().numpy(), W.warp_perspective(img, H, (dw, dh), True)), (dw, dh)
        guard = outbuf.clone()
        guard[1:dh + 1, 6:dw + 6] = 201
        assert (guard == 201).all(), "guard columns and rows were written"
    assert ctx.warp_affine(src, A, inverse_map=True, dsize=(41, 77)).shape == (77, 41, 3)


def test_warp_affine_of_a_translation_is_the_translate_warp(ctx):
    img = torch.as_tensor(_img(251, 333, 9)).cuda()
    for (sx, sy) in ((0.0, 0.0), (-3.7, 2.2), (5.75, 3.5), (1 / 64.0, -1 / 128.0), (100.3, -77.9), (0.4, 15.5 / 1024), (12345.678, 0.1)):
        a = ctx.warp_affine(img, [[1, 0, sx], [0, 1, sy]], inverse_map=True)
        assert torch.equal(a, ctx.warp_translate(img, sx, sy)), (sx, sy)
    # the reference's call: the forward matrix [1 0 -sx; 0 1 -sy]
    assert torch.equal(ctx.warp_affine(img, [[1, 0, -3.5], [0, 1, 2.25]]), ctx.warp_translate(img, 3.5, -2.25))


def test_forward_form_agrees_with_the_inverse_form(ctx):
    rng = np.random.RandomState(24)
    img = torch.as_tensor(_img(240, 320, 10)).cuda()
    for _ in range(4):
        A, H = _random_affine(rng, 320, 240), _random_keystone(rng, 320, 240)
        assert torch.equal(ctx.warp_affine(img, A), ctx.warp_affine(img, W.invert_affine(A), inverse_map=True))
        assert torch.equal(ctx.warp_perspective(img, H), ctx.warp_perspective(img, W.invert_perspective(H), inverse_map=True))


def test_warp_refusals_write_nothing(ctx):
    img = torch.as_tensor(_img(20, 30, 11)).cuda()
    out = torch.full((20, 30, 3), 77, dtype=torch.uint8, device="cuda")
    I2, I3 = [[1, 0, 0], [0, 1, 0]], np.eye(3)
    bad_affine = ([[np.nan, 0, 0], [0, 1, 0]], [[1, 0, np.inf], [0, 1, 0]], [[1, 0, 2e6], [0, 1, 0]], [[1e5, 0, 0], [0, 1, 0]])
    for M in bad_affine:
        with pytest.raises(RcflowError) as e:
            ctx.warp_affine(img, M, inverse_map=True, out=out)
        assert e.value.code == EINVAL, M
    for M in ([[1, 2, 0], [2, 4, 0]], [[0, 0, 1], [0, 0, 1]]):          # singular in the forward form
        with pytest.raises(RcflowError) as e:
            ctx.warp_affine(img, M, out=out)
        assert e.value.code == EINVAL
    for M in (np.diag([1.0, 1.0, np.nan]),):
        with pytest.raises(RcflowError) as e:
            ctx.warp_perspective(img, M, inverse_map=True, out=out)
        assert e.value.code == EINVAL
    with pytest.raises(RcflowError) as e:
        ctx.warp_perspective(img, [[1, 2, 3], [2, 4, 6], [0, 0, 1]], out=out)
    assert e.value.code == EINVAL
    for fn, M in ((ctx.warp_affine, I2), (ctx.warp_perspective, I3)):
        with pytest.raises(RcflowError) as e:
            fn(img, M, out=img)                             # in place
        assert e.value.code == EINVAL
        with pytest.raises(RcflowError) as e:
            fn(img, M, dsize=(4000, 20))
        assert e.value.code == ESIZE
    lib, h = ctx._lib, ctx._h
    m6, m9 = (C.c_double * 6)(1, 0, 0, 0, 1, 0), (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    src, dst = C.c_void_p(img.data_ptr()), C.c_void_p(out.data_ptr())
    for fn, m in ((lib.rcflow_warp_affine_bgr_dev, m6), (lib.rcflow_warp_perspective_bgr_dev, m9)):
        assert fn(h, 0, src, 89, 30, 20, dst, 90, 30, 20, m, 16) == EINVAL          # steps below 3 * w
        assert fn(h, 0, src, 90, 30, 20, dst, 89, 30, 20, m, 16) == EINVAL
        assert fn(h, 0, None, 90, 30, 20, dst, 90, 30, 20, m, 16) == EINVAL
        assert fn(h, 0, src, 90, 30, 20, dst, 90, 30, 20, None, 16) == EINVAL
        assert fn(h, 0, src, 90, 30, 20, dst, 90, 30, 20, m, 16 | 1) == EINVAL      # unknown flag bits
    ctx.sync()
    assert (out == 77).all()                                # no refused call wrote
    for fn, m in ((lib.rcflow_warp_affine_bgr_dev, m6), (lib.rcflow_warp_perspective_bgr_dev, m9)):
        out.fill_(77)
        assert fn(h, 0, src, 90, 30, 20, dst, 90, 30, 20, m, 16) == 0
        ctx.sync()
        assert torch.equal(out, img)


# ---------------------------------------------------------------------------- the stabiliser
def _push_all(ctx, clip, stream=0, want_motion=True):
    """Queues the whole clip; reads the motion after every push only when asked (that synchronises)."""
    n = len(clip)
    frames = torch.as_tensor(clip).cuda()
    outs = torch.empty_like(frames)
    res = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    motions = []
    for t in range(n):
        ctx.framestab_push(frames[t], out=outs[t], result=res[t], stream=stream)
        if want_motion:
            motions.append(ctx.framestab_motion(stream=stream))
    last, pushed = ctx.framestab_read(stream=stream)
    res = res.cpu().numpy()
    assert tuple(res[-1]) == last
    return outs.cpu().numpy(), res, motions


def _check_against_numpy(clip, outs, res, motions, rois, model, min_response=0.0, anchor="previous"):
    """The numpy chain fed the device's own shifts and motion: shifts within 1e-3 px, motion within 1e-9 of the numpy fit
    of the device's shifts, frames bit for bit."""
    n, h, w = clip.shape[:3]
    ref = W.MultiStabRef(w, h, rois, model, min_response, anchor)
    for t in range(n):
        m = motions[t]
        out, own, _ = ref.push(clip[t], motion=m["motion"])
        assert np.array_equal(outs[t], out), "corrected frame %d" % t
        if t == 0:
            assert m["model_used"] is None and m["patches_used"] == 0 and np.array_equal(m["motion"], [[1, 0, 0], [0, 1, 0]])
            assert not m["shifts"].any() and tuple(res[0]) == (0.0, 0.0, 0.0)
            continue
        assert np.abs(m["shifts"] - own).max() < 1e-3, (t, m["shifts"], own)
        fit = W.fit_motion(rois, m["shifts"], ref.model, min_response, (w, h))
        assert np.abs(m["motion"] - fit[0]).max() < 1e-9, (t, m["motion"], fit[0])
        assert W.MODELS.get(m["model_used"], 0) == fit[1] and m["patches_used"] == fit[2]
        assert np.abs(res[t] - np.array(fit[3])).max() < 1e-9 and m["frames_pushed"] == t + 1


@pytest.fixture(scope="module")
def shaken():
    return S.shaken_clip(640, 480, 40, device="cuda")


@pytest.fixture(scope="module")
def rolling():
    """40 frames of a static texture under a rolling (0.3 deg), breathing (0.5 %), shaking (4 px) camera, moving water
    in the middle."""
    water = synth.surf_clip(240, 160, 40, seed=99)
    return W.rolling_clip(640, 480, 40, seed=7, water=water)


def test_one_patch_translation_is_the_existing_stabiliser(ctx, shaken):
    clip, _ = shaken
    roi = (590, 50, 50, 50)
    ctx.framestab_open(640, 480, roi)
    a_out, a_res, a_mo = _push_all(ctx, clip)
    assert a_mo[5]["model_used"] == "translation" and a_mo[5]["patches_used"] == 1       # read_motion serves either slot
    assert np.array_equal(a_mo[5]["motion"], [[1, 0, a_res[5, 0]], [0, 1, a_res[5, 1]]]) and a_mo[5]["rois"] == [roi]
    ctx.framestab_open(640, 480, rois=[roi], model="translation", min_response=-1.0)
    b_out, b_res, b_mo = _push_all(ctx, clip)
    assert np.array_equal(a_out, b_out) and np.array_equal(a_res, b_res)
    for t in range(1, 40):
        assert np.array_equal(b_mo[t]["motion"], [[1, 0, a_res[t, 0]], [0, 1, a_res[t, 1]]]) and tuple(b_mo[t]["shifts"][0]) == tuple(a_res[t])
    info = ctx.framestab_info()
    assert info["roi"] == roi and info["launches_per_push"] == 2 and info["frames_pushed"] == 40
    ctx.framestab_close()


def _median_flow(ctx, frames, roi):
    x, y, rw, rh = roi
    mags = []
    for t in range(1, len(frames)):
        flow = ctx.calcOpticalFlowFarneback(S.bgr_to_gray(frames[t - 1]), S.bgr_to_gray(frames[t]), None, 0.5, 2, 3, 2, 15, 1.2, 0)
        flow = flow.cpu().numpy() if torch.is_tensor(flow) else flow
        mags.append(np.hypot(flow[y:y + rh, x:x + rw, 0], flow[y:y + rh, x:x + rw, 1]))
    return float(np.median(np.stack(mags)))


def test_rotation_and_zoom_are_corrected(ctx, rolling):
    """What the feature is for.  Bounds from the numpy chain on this clip, with margin: unstabilised corners up to
    5.9 px from frame 0; four corner patches + similarity, chained: every corner within 1.9 px (the estimator's walk);
    one patch + translation: its own corner within 1.9 px, the opposite corner up to 4.0 px."""
    clip, _ = rolling
    rois = W.corner_rois(640, 480)
    ctx.framestab_open(640, 480, rois=rois, model="similarity")
    outs, res, motions = _push_all(ctx, clip)
    m = motions[-1]
    assert m["rois"] == rois and m["model"] == "similarity" and m["anchor"] == "previous" and m["min_response"] == 0.0
    _check_against_numpy(clip, outs, res, motions, rois, "similarity")
    multi = max(W.patch_drift(r, clip[0], outs[t]) for r in rois for t in range(1, 40))
    ctx.framestab_open(640, 480, rois[0])
    single, _, _ = _push_all(ctx, clip, want_motion=False)
    ctx.framestab_close()
    far = max(W.patch_drift(rois[3], clip[0], single[t]) for t in range(1, 40))
    print("worst corner drift: four patches + similarity %.2f px, one patch + translation (opposite corner) %.2f px" % (multi, far))
    assert multi < 2.5 and far > 3.2 and far > 1.6 * multi, (multi, far)
    # Farneback flow (ripcurrents.cpp:215 parameters) over the corners: of the order of the camera motion before, a
    # fraction of it after
    for r in (rois[0], rois[3]):
        raw, stab = _median_flow(ctx, clip[:12], r), _median_flow(ctx, outs[:12], r)
        print("median |flow| over %s: unstabilised %.3f px, stabilised %.3f px" % (r, raw, stab))
        assert raw > 2.5 and stab < 1.0 and stab < raw / 4, (r, raw, stab)      # numpy chain + CPU oracle: 5.0 / 6.1 px before, 0.51 / 0.46 px after


def test_anchor_first_does_not_walk(ctx, rolling):
    """Numpy chain on this clip: anchored, every corner within 0.83 px of frame 0 at all 40 frames (0.18 at frame 5, 0.11
    at frame 39); chained, up to 1.9 px."""
    clip, _ = rolling
    rois = W.corner_rois(640, 480)
    ctx.framestab_open(640, 480, rois=rois, model="similarity", anchor="first")
    outs, res, motions = _push_all(ctx, clip)
    assert motions[-1]["anchor"] == "first"
    _check_against_numpy(clip, outs, res, motions, rois, "similarity", anchor="first")
    drift = [max(W.patch_drift(r, clip[0], outs[t]) for r in rois) for t in range(40)]
    ctx.framestab_open(640, 480, rois=rois, model="similarity")
    chained, _, _ = _push_all(ctx, clip, want_motion=False)
    ctx.framestab_close()
    worst_chained = max(W.patch_drift(r, clip[0], chained[t]) for r in rois for t in range(1, 40))
    print("anchored: frame 5 %.2f, frame 39 %.2f, worst %.2f px; chained worst %.2f px" % (drift[5], drift[39], max(drift), worst_chained))
    assert drift[39] <= drift[5] + 0.5 and max(drift) < 1.2 and max(drift) < worst_chained


def test_gate_and_ladder(ctx, rolling):
    """A fifth patch on the static texture that something black covers in frames 3, 4 and 7: a patch of zeros has no
    spectrum, so its response is 0.  (Neither the synthetic water nor seeded noise decorrelates a patch reliably: the
    numpy chain gives them responses of 0.2 to 0.8 beside 0.4 to 0.9 for the static corners.)  Anchored, so the shifts
    do not depend on the corrections and the gated run sees the responses of the ungated one."""
    clip = rolling[0][:10].copy()
    crossed = (3, 4, 7)
    fifth = (295, 20, 50, 50)
    for t in crossed:
        clip[t, 12:78, 287:353] = 0
    rois = W.corner_rois(640, 480) + [fifth]
    ctx.framestab_open(640, 480, rois=rois, model="affine", min_response=0.0, anchor="first")
    _, _, free = _push_all(ctx, clip)
    resp = np.array([m["shifts"][:, 2] for m in free[1:]])                     # (9, 5)
    hit = np.array([t in crossed for t in range(1, 10)])
    low, high = resp[hit, 4].max(), min(resp[:, :4].min(), resp[~hit, 4].min())
    print("response of the crossed patch at most %.3f, of every other at least %.3f" % (low, high))
    assert low < 0.5 * high, (low, high)
    gate = 0.5 * (low + high)
    ctx.framestab_open(640, 480, rois=rois, model="affine", min_response=gate, anchor="first")
    outs, res, gated = _push_all(ctx, clip)
    _check_against_numpy(clip, outs, res, gated, rois, "affine", gate, "first")
    for t in range(1, 10):
        assert gated[t]["patches_used"] == (4 if t in crossed else 5) and gated[t]["model_used"] == "affine"
        assert np.array_equal(gated[t]["shifts"], free[t]["shifts"])
        want = W.fit_motion(rois[:4] if t in crossed else rois, gated[t]["shifts"][:4 if t in crossed else 5], W.AFFINE, gate, (640, 480))
        assert np.abs(gated[t]["motion"] - want[0]).max() < 1e-9
    # the ladder on the device: collinear patches fall from affine to similarity, two patches likewise, one to translation
    line = [(20, 20, 50, 50), (300, 20, 50, 50), (570, 20, 50, 50)]
    for rr, model, used in ((line, "affine", "similarity"), (rois[:2], "affine", "similarity"), (rois[:1], "similarity", "translation"),
                            (rois[:3], "affine", "affine")):
        ctx.framestab_open(640, 480, rois=rr, model=model)
        outs, res, mo = _push_all(ctx, clip[:3])
        assert mo[2]["model_used"] == used, (model, used, mo[2])
        _check_against_numpy(clip[:3], outs, res, mo, rr, model)
    # every patch gated out: the identity, the frame is copied
    ctx.framestab_open(640, 480, rois=rois, model="similarity", min_response=10.0)
    outs, res, mo = _push_all(ctx, clip[:4])
    assert np.array_equal(outs, clip[:4]) and not res.any()
    assert all(m["model_used"] is None and m["patches_used"] == 0 and np.array_equal(m["motion"], [[1, 0, 0], [0, 1, 0]]) for m in mo)
    assert mo[2]["shifts"][:, 2].min() > 0.1                                   # measured all the same
    ctx.framestab_close()


def test_slots_reset_reopen_and_refusals(ctx, rolling):
    clip = rolling[0][:6]
    small = W.rolling_clip(333, 251, 6, seed=11, margin=40)[0]
    ra, rb = W.corner_rois(640, 480), W.corner_rois(333, 251, 40, 10)[:3]
    ctx.framestab_open(640, 480, rois=ra, model="similarity", stream=0)
    ctx.framestab_open(333, 251, rois=rb, model="affine", anchor="first", stream=1)
    fa, fb = torch.as_tensor(clip).cuda(), torch.as_tensor(small).cuda()
    oa, ob = torch.empty_like(fa), torch.empty_like(fb)
    resa, resb = torch.zeros((6, 3), dtype=torch.float64, device="cuda"), torch.zeros((6, 3), dtype=torch.float64, device="cuda")
    ma, mb = [], []
    for t in range(6):                                      # interleaved
        ctx.framestab_push(fa[t], out=oa[t], result=resa[t], stream=0)
        ctx.framestab_push(fb[t], out=ob[t], result=resb[t], stream=1)
        ma.append(ctx.framestab_motion(stream=0))
        mb.append(ctx.framestab_motion(stream=1))
    _check_against_numpy(clip, oa.cpu().numpy(), resa.cpu().numpy(), ma, ra, "similarity")
    _check_against_numpy(small, ob.cpu().numpy(), resb.cpu().numpy(), mb, rb, "affine", anchor="first")
    assert ctx.framestab_info(stream=1)["roi"] == rb[0] and ctx.framestab_info(stream=1)["dft_size"] == (40, 40)
    # reset: the next push is a first push again, also for the anchored slot
    ctx.framestab_reset(stream=1)
    assert ctx.framestab_read(stream=1) == ((0.0, 0.0, 0.0), 0) and ctx.framestab_motion(stream=1)["model_used"] is None
    outs, res, mo = _push_all(ctx, small[2:], stream=1)
    _check_against_numpy(small[2:], outs, res, mo, rb, "affine", anchor="first")
    # refusals leave the state as it was
    before = ctx.framestab_motion(stream=0)
    bad = (([(600, 20, 50, 50)], EINVAL), ([(20, 20, 50, 50), (90, 20, 48, 50)], EINVAL), ([(0, 0, 7, 50)], EINVAL),
           ([(0, 0, 128, 128)], ESIZE), ([(0, 0, 50, 300)], ESIZE), ([(20, 20, 50, 50)] * 17, EINVAL))
    for rr, code in bad:
        with pytest.raises(RcflowError) as e:
            ctx.framestab_open(640, 480, rois=rr)
        assert e.value.code == code, rr
    lib, h = ctx._lib, ctx._h
    r4 = (C.c_int * 4)(20, 20, 50, 50)
    assert lib.rcflow_framestab_open_multi(h, 0, 640, 480, r4, 1, 4, 0.0, 0) == EINVAL            # unknown model
    assert lib.rcflow_framestab_open_multi(h, 0, 640, 480, r4, 1, 2, 0.0, 2) == EINVAL            # unknown flag
    assert lib.rcflow_framestab_open_multi(h, 0, 640, 480, r4, 1, 2, float("nan"), 0) == EINVAL
    assert lib.rcflow_framestab_open_multi(h, 0, 640, 480, None, 1, 2, 0.0, 0) == EINVAL
    assert lib.rcflow_framestab_open_multi(h, 0, 4000, 480, r4, 1, 2, 0.0, 0) == ESIZE
    with pytest.raises(RcflowError) as e:
        ctx.framestab_push(fa[1], out=fa[1], stream=0)      # overlapping output
    assert e.value.code == EINVAL
    src, dst = C.c_void_p(fa[1].data_ptr()), C.c_void_p(oa[1].data_ptr())
    assert lib.rcflow_framestab_push_dev(h, 0, src, 640 * 3 - 1, dst, 640 * 3, None) == EINVAL
    after = ctx.framestab_motion(stream=0)
    assert after["frames_pushed"] == 6 and np.array_equal(after["motion"], before["motion"]) and np.array_equal(after["shifts"], before["shifts"])
    assert after["rois"] == ra
    # the chain goes on as if nothing had been refused: push the same six frames again as frames 6..11
    outs, res, mo = _push_all(ctx, clip[1:3], stream=0)
    ref = W.MultiStabRef(640, 480, ra, "similarity")
    for t in range(6):
        ref.push(clip[t], motion=ma[t]["motion"])
    for t in range(2):
        assert np.array_equal(outs[t], ref.push(clip[1 + t], motion=mo[t]["motion"])[0])
    # re-open with another n, then back to a single patch, then close
    ctx.framestab_open(640, 480, rois=ra[:2], model="translation", stream=0)
    outs, res, mo = _push_all(ctx, clip[:3], stream=0)
    _check_against_numpy(clip[:3], outs, res, mo, ra[:2], "translation")
    ctx.framestab_close(stream=0)
    ctx.framestab_close(stream=1)
    for fn in (ctx.framestab_motion, ctx.framestab_info):
        with pytest.raises(RcflowError) as e:
            fn(stream=1)
        assert e.value.code == ESTATE


def test_fresh_context_on_a_torch_stream_and_profile_records(rolling):
    clip = rolling[0][:5]
    rois = W.corner_rois(640, 480)
    ts = torch.cuda.Stream()
    with Context(640, 480) as c, torch.cuda.stream(ts):
        c.framestab_open(640, 480, rois=rois, model="similarity")
        c.profile_reset()
        c.profile_enable(True)
        try:
            outs, res, mo = _push_all(c, clip)
            img = torch.as_tensor(clip[0]).cuda()
            c.warp_affine(img, [[1, 0, 0.5], [0, 1, 0]])
            c.warp_perspective(img, np.eye(3))
            c.sync()
        finally:
            c.profile_enable(False)
        _check_against_numpy(clip, outs, res, mo, rois, "similarity")
        rec = {r["kernel"]: r for r in c.profile_read()}
        assert rec["framestab@7"]["launches"] == 4 and rec["framestab@8"]["launches"] == 5 + 1 and rec["framestab@9"]["launches"] == 1
        assert not any(k.startswith("framestab@") and k not in ("framestab@7", "framestab@8", "framestab@9") for k in rec)
        assert rec["framestab@7"]["alg_bytes"] == 4 * (4 * (7 * 2500 + 4 * 2500 + 8 * 100 + 24) + 72 + 24)
        assert c.profile_read_buckets()["farneback"] > 0
        c.framestab_close()
    ts.synchronize()
