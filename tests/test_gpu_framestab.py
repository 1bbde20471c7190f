"""Frame stabilisation on the device (stab_kernels.hip) against the numpy restatement of the reference's loop
(tests/_framestab_ref.py): the warp bit for bit, the phase correlation within 1e-3 px (its DFTs are fp32 direct sums,
the restatement's go through np.fft in double)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _framestab_ref as R
from _dev import EINVAL, ESIZE, ESTATE
from ripcurrents_amd._lib import RcflowError
from ripcurrents_amd.api import Context

pytestmark = pytest.mark.gpu


def _patches(w, h, d, seed=3):
    tex = R.DenseTexture(512, seed)
    a = tex.u8()[60:60 + h, 70:70 + w].astype(np.float32)
    b = tex.u8(*d)[60:60 + h, 70:70 + w].astype(np.float32)
    return a, b


@pytest.mark.parametrize("w,h", [(50, 50), (64, 64), (48, 80), (51, 37), (25, 25), (96, 96), (128, 128), (200, 256), (8, 8)])
def test_phase_correlate_matches_numpy(ctx, w, h):
    """One-workgroup form (up to 96 x 96: 151 KB of LDS), padded (51 x 37 -> 54 x 40), odd (25 x 25: the +0.5 px
    quirk) and the launch-per-pass form (128 x 128, 200 x 256)."""
    for k, d in enumerate(((0.0, 0.0), (1.5, -2.25), (-3.0, 2.0))):
        d = tuple(v * min(w, h) / 50.0 for v in d) if min(w, h) < 50 else d
        a, b = _patches(w, h, d, seed=3 + k)
        for window in (True, False):
            win = R.hanning_window(h, w) if window else None
            want = R.phase_correlate(a, b, win, return_surface=True)
            assert not R.peak_is_ambiguous(want[3]), (w, h, d, window)
            got = ctx.phase_correlate(a, b, window=window).cpu().numpy()
            assert abs(got[0] - want[0]) < 1e-3 and abs(got[1] - want[1]) < 1e-3, (w, h, d, window, got, want[:3])
            assert abs(got[2] - want[2]) < 1e-4 * abs(want[2]) + 1e-6, (w, h, d, window, got, want[:3])


def test_phase_correlate_steps_and_refusals(ctx):
    a, b = _patches(50, 50, (2.0, 1.0))
    big = torch.zeros((60, 80), dtype=torch.float32, device="cuda")
    big2 = torch.full((60, 80), 7.0, dtype=torch.float32, device="cuda")
    big[3:53, 5:55] = torch.as_tensor(a).cuda()
    big2[3:53, 5:55] = torch.as_tensor(b).cuda()
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    got = ctx.phase_correlate(big[3:53, 5:55], big2[3:53, 5:55], out=out).cpu().numpy()
    want = R.phase_correlate(a, b, R.hanning_window(50, 50))
    assert np.abs(got - np.array(want)).max() < 1e-3
    for (w, h, code) in ((7, 50, EINVAL), (50, 4, EINVAL), (257, 50, ESIZE), (50, 300, ESIZE)):
        with pytest.raises(RcflowError) as e:
            ctx.phase_correlate(np.zeros((h, w), np.float32), np.zeros((h, w), np.float32))
        assert e.value.code == code


def _warp_check(ctx, img, sx, sy, out=None):
    got = ctx.warp_translate(img, sx, sy, out=out).cpu().numpy()
    want = R.warp_translate(img.cpu().numpy() if torch.is_tensor(img) else img, sx, sy)
    assert np.array_equal(got, want), (tuple(got.shape), sx, sy)


def test_warp_translate_every_fraction_bit_exact(ctx):
    """All 32 x 32 fractional phases, on a width with w % 4 != 0 and a padded step."""
    rng = np.random.RandomState(11)
    buf = torch.as_tensor(rng.randint(0, 256, (29, 64, 3)).astype(np.uint8)).cuda()
    img = buf[:, 3:40]                                      # 37 wide, row step 192
    outbuf = torch.zeros((29, 50, 3), dtype=torch.uint8, device="cuda")
    for fy in range(32):
        for fx in range(32):
            _warp_check(ctx, img, 2 + fx / 32.0, -1 + fy / 32.0, out=outbuf[:, 5:42])
    assert not outbuf[:, :5].any() and not outbuf[:, 42:].any()


def test_warp_translate_sizes_and_shifts_bit_exact(ctx):
    rng = np.random.RandomState(12)
    shifts = ((0.0, 0.0), (-3.7, 2.2), (5.75, 3.5), (1 / 64.0, -1 / 128.0), (-0.25, -0.5), (100.3, -77.9), (12345.678, 0.1))
    for (w, h) in ((640, 480), (333, 251), (1920, 1080), (5, 3), (4, 1)):
        img = torch.as_tensor(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
        for (sx, sy) in shifts:
            _warp_check(ctx, img, sx, sy)
        _warp_check(ctx, img, float(w), 0.0)               # past the frame: all zero
        _warp_check(ctx, img, -float(w) - 1, 0.3)
        _warp_check(ctx, img, 0.0, float(h))
        _warp_check(ctx, img, w - 1.5, h - 1.5)
    # rows where the double sum y + shift.y lands on a rounding tie of 1/1024
    img = torch.as_tensor(rng.randint(0, 256, (300, 41, 3)).astype(np.uint8)).cuda()
    for sy in (0.5 / 1024, 1.5 / 1024, -0.5 / 1024, 7 + 0.5 / 1024, 1 / 3.0, 15.5 / 1024):
        _warp_check(ctx, img, 0.4, sy)


def test_warp_translate_refusals(ctx):
    img = torch.zeros((20, 30, 3), dtype=torch.uint8, device="cuda")
    for (sx, sy) in ((float("nan"), 0.0), (0.0, float("inf")), (2e6, 0.0)):
        with pytest.raises(RcflowError) as e:
            ctx.warp_translate(img, sx, sy)
        assert e.value.code == EINVAL
    with pytest.raises(RcflowError) as e:
        ctx.warp_translate(img, 1.0, 1.0, out=img)          # in place
    assert e.value.code == EINVAL


def test_resize_bgr_area_matches_the_gray_path(ctx, orc):
    """gray(v, v, v) = v: on a frame of three equal channels every channel of the colour result is the oracle's
    resize + gray; on three different planes each channel is the result for that plane alone."""
    rng = np.random.RandomState(8)
    for (sw, sh, dw, dh) in ((1280, 960, 640, 480), (1920, 1440, 640, 480), (1920, 960, 640, 480), (1920, 1080, 640, 480),
                             (1000, 700, 640, 480), (641, 481, 640, 480), (640, 480, 640, 480), (97, 65, 31, 17)):
        planes = rng.randint(0, 256, (3, sh, sw)).astype(np.uint8)
        got = ctx.resize_bgr(np.ascontiguousarray(planes.transpose(1, 2, 0)), dw, dh, interpolation="area").cpu().numpy()
        assert got.shape == (dh, dw, 3)
        for c in range(3):
            want = orc.resize_area_bgr_to_gray(np.repeat(planes[c][..., None], 3, 2), dw, dh)
            assert np.array_equal(got[..., c], want), (sw, sh, dw, dh, c)
    with pytest.raises(Exception):
        ctx.resize_bgr(np.zeros((240, 320, 3), np.uint8), 640, 480, interpolation="area")    # enlarging


@pytest.fixture(scope="module")
def shaken():
    clip, shake = R.shaken_clip(640, 480, 40, device="cuda")
    return clip, shake


def _run_pipeline(ctx, clip, roi=None, stream=0, reopen=True):
    """Queues the whole clip without a synchronisation in between -> (corrected frames, (n, 3) results), host arrays."""
    n, h, w = clip.shape[:3]
    if reopen:
        ctx.framestab_open(w, h, roi, stream=stream)
    frames = torch.as_tensor(clip).cuda()
    outs = torch.empty_like(frames)
    res = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    for t in range(n):
        ctx.framestab_push(frames[t], out=outs[t], result=res[t], stream=stream)
    last, pushed = ctx.framestab_read(stream=stream)                # the one blocking call
    assert pushed == n
    res = res.cpu().numpy()
    assert tuple(res[-1]) == last
    return outs.cpu().numpy(), res


def _check_against_chain(clip, outs, res, roi=None, drift_bound=None):
    """The numpy chain fed the device's own shifts: frames bit for bit, its shifts within 1e-3 px of the device's."""
    n, h, w = clip.shape[:3]
    ref = R.FrameStabRef(w, h, roi)
    worst = 0.0
    for t in range(n):
        if t:
            s = R.correlation_surface(ref.patch(ref.prev), ref.patch(clip[t]), ref.window)
            assert not R.peak_is_ambiguous(s), t
        out, want = ref.push(clip[t], shift=None if t == 0 else (res[t, 0], res[t, 1]))
        assert np.array_equal(outs[t], out), "corrected frame %d" % t
        assert np.abs(res[t] - np.array(want)).max() < 1e-3, (t, res[t], want)
        assert abs(res[t, 2] - want[2]) < 1e-4 * abs(want[2]) + 1e-6
        if drift_bound is not None:
            worst = max(worst, R.drift(ref, clip[0], out))
    if drift_bound is not None:
        assert worst < drift_bound, worst
    return worst


def test_pipeline_follows_the_reference_chain(ctx, shaken):
    """40 pushes queued with their results going to the rows of one device array, one read at the end.  The ROI of
    every corrected frame stays within 3 px of frame 0 (the bound the numpy chain is held to in
    tests/test_framestab_ref.py: the estimator's own walk; the shaken frames are up to 6 px away)."""
    clip, shake = shaken
    outs, res = _run_pipeline(ctx, clip)
    assert tuple(res[0]) == (0.0, 0.0, 0.0) and np.array_equal(outs[0], clip[0])
    info = ctx.framestab_info()
    assert info["roi"] == (590, 50, 50, 50) and info["dft_size"] == (50, 50) and info["launches_per_push"] == 2
    assert info["frames_pushed"] == 40 and (info["w"], info["h"]) == (640, 480)
    _check_against_chain(clip, outs, res, drift_bound=3.0)
    ctx.framestab_close()


def _median_flow(ctx, frames, roi):
    x, y, rw, rh = roi
    mags = []
    for t in range(1, len(frames)):
        g0, g1 = R.bgr_to_gray(frames[t - 1]), R.bgr_to_gray(frames[t])
        flow = ctx.calcOpticalFlowFarneback(g0, g1, None, 0.5, 2, 3, 2, 15, 1.2, 0)
        flow = flow.cpu().numpy() if torch.is_tensor(flow) else flow
        mags.append(np.hypot(flow[y:y + rh, x:x + rw, 0], flow[y:y + rh, x:x + rw, 1]))
    return float(np.median(np.stack(mags)))


def test_stabilised_clip_has_a_still_roi_in_the_flow(ctx, shaken):
    """The point of the feature: Farneback flow (the parameters of ripcurrents.cpp:215) over the static patch of the
    shaken clip is of the order of the shake; of the stabilised clip at least five times smaller.  The bounds are set
    from what the run showed, with margin."""
    clip, shake = shaken
    roi = (590, 50, 50, 50)
    outs, _ = _run_pipeline(ctx, clip)
    ctx.framestab_close()
    shaken_med, stab_med = _median_flow(ctx, clip[:16], roi), _median_flow(ctx, outs[:16], roi)
    print("median |flow| over the ROI: shaken %.3f px, stabilised %.3f px" % (shaken_med, stab_med))
    # measured: shaken 7.2 px, stabilised 0.69 px (the estimator's residual of up to half a pixel per step)
    assert shaken_med > 3.0, shaken_med
    assert stab_med < 1.2 and stab_med < shaken_med / 5, (shaken_med, stab_med)


def test_two_slots_reset_reopen_and_large_roi(ctx, shaken):
    clip, _ = shaken
    a = clip[:6]
    b, _ = R.shaken_clip(333, 251, 6, seed=9, roi=(200, 60, 64, 48), block=100)
    fa, fb = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()
    ctx.framestab_open(640, 480, None, stream=0)
    ctx.framestab_open(333, 251, (200, 60, 64, 48), stream=1)
    oa, ob = torch.empty_like(fa), torch.empty_like(fb)
    ra = torch.zeros((6, 3), dtype=torch.float64, device="cuda")
    rb = torch.zeros((6, 3), dtype=torch.float64, device="cuda")
    for t in range(6):                                      # interleaved
        ctx.framestab_push(fa[t], out=oa[t], result=ra[t], stream=0)
        ctx.framestab_push(fb[t], out=ob[t], result=rb[t], stream=1)
    ctx.framestab_read(stream=0)
    ctx.framestab_read(stream=1)
    _check_against_chain(a, oa.cpu().numpy(), ra.cpu().numpy())
    _check_against_chain(b, ob.cpu().numpy(), rb.cpu().numpy(), roi=(200, 60, 64, 48))
    assert ctx.framestab_info(stream=1)["dft_size"] == (64, 48)
    # reset: the next push is a first push again
    ctx.framestab_reset(stream=0)
    assert ctx.framestab_info(stream=0)["frames_pushed"] == 0 and ctx.framestab_read(stream=0) == ((0.0, 0.0, 0.0), 0)
    outs, res = _run_pipeline(ctx, a[2:], reopen=False)
    _check_against_chain(a[2:], outs, res)
    # re-open with a patch beyond the LDS limit: the correlation runs as a launch per pass
    roi = (500, 20, 128, 128)
    outs, res = _run_pipeline(ctx, a, roi=roi)
    assert ctx.framestab_info()["launches_per_push"] == 6
    _check_against_chain(a, outs, res, roi=roi)
    ctx.framestab_close(stream=0)
    ctx.framestab_close(stream=1)
    ctx.framestab_close(stream=1)                           # nothing open: RC_OK
    with pytest.raises(RcflowError) as e:
        ctx.framestab_info(stream=1)
    assert e.value.code == ESTATE


def test_fresh_context_and_padded_steps(shaken):
    clip, _ = shaken
    with Context(640, 480) as c:
        c.framestab_open(640, 480)
        buf = torch.zeros((4, 480, 700, 3), dtype=torch.uint8, device="cuda")
        buf[:, :, 7:647] = torch.as_tensor(clip[:4]).cuda()
        outbuf = torch.zeros((4, 480, 650, 3), dtype=torch.uint8, device="cuda")
        res = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
        for t in range(4):
            c.framestab_push(buf[t, :, 7:647], out=outbuf[t, :, 10:650], result=res[t])
        c.framestab_read()
        _check_against_chain(clip[:4], outbuf[:, :, 10:650].cpu().numpy(), res.cpu().numpy())
        assert not outbuf[:, :, :10].any()


def test_refusals_leave_the_state_untouched(ctx, shaken):
    clip, _ = shaken
    with pytest.raises(RcflowError) as e:
        ctx.framestab_push(torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda"))      # before open
    assert e.value.code == ESTATE
    ctx.framestab_open(640, 480)
    f = torch.as_tensor(clip[:3]).cuda()
    outs = torch.empty_like(f)
    res = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
    ctx.framestab_push(f[0], out=outs[0], result=res[0])
    for roi, code in (((600, 50, 50, 50), EINVAL), ((-1, 0, 50, 50), EINVAL), ((0, 0, 7, 50), EINVAL), ((0, 0, 50, 6), EINVAL),
                      ((0, 0, 257, 50), ESIZE), ((0, 0, 50, 300), ESIZE), ((0, 440, 50, 50), EINVAL)):
        with pytest.raises(RcflowError) as e:
            ctx.framestab_open(640, 480, roi)
        assert e.value.code == code, roi
    with pytest.raises(RcflowError) as e:
        ctx.framestab_open(4000, 480)
    assert e.value.code == ESIZE
    with pytest.raises(RcflowError) as e:
        ctx.framestab_push(f[1], out=f[1])                  # overlapping output
    assert e.value.code == EINVAL
    lib, h = ctx._lib, ctx._h
    out = torch.empty_like(f[1])
    src, dst = C.c_void_p(f[1].data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.rcflow_framestab_push_dev(h, 0, src, 640 * 3 - 1, dst, 640 * 3, None) == EINVAL      # wrong steps
    assert lib.rcflow_framestab_push_dev(h, 0, src, 640 * 3, dst, 100, None) == EINVAL
    assert lib.rcflow_framestab_push_dev(h, 0, src, 640 * 3, None, 640 * 3, None) == EINVAL
    info = ctx.framestab_info()
    assert info["frames_pushed"] == 1 and info["roi"] == (590, 50, 50, 50)
    ctx.framestab_push(f[1], out=outs[1], result=res[1])
    ctx.framestab_push(f[2], out=outs[2], result=res[2])
    last, n = ctx.framestab_read()
    assert n == 3
    _check_against_chain(clip[:3], outs.cpu().numpy(), res.cpu().numpy())      # the chain went on as if nothing had been refused
    ctx.framestab_close()


def test_profile_records_two_launches_per_push(ctx, shaken):
    clip, _ = shaken
    f = torch.as_tensor(clip[:4]).cuda()
    ctx.framestab_open(640, 480)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        for t in range(4):
            ctx.framestab_push(f[t])
        ctx.resize_bgr(f[0], 320, 240, interpolation="area")
        ctx.sync()
    finally:
        ctx.profile_enable(False)
    rec = {r["kernel"]: r for r in ctx.profile_read()}
    assert rec["framestab@0"]["launches"] == 3 and rec["framestab@1"]["launches"] == 4      # the first push only copies
    assert rec["frame_color@3"]["launches"] == 1
    assert not any(k.startswith("framestab@") and k not in ("framestab@0", "framestab@1") for k in rec)
    assert rec["framestab@1"]["alg_bytes"] == 4 * (6 * 640 * 480 + 4 * 50 * 50) + 3 * 16
    assert rec["framestab@0"]["alg_bytes"] == 3 * (7 * 2500 + 4 * 2500 + 8 * 100 + 24)
    buckets = ctx.profile_read_buckets()
    assert buckets["farneback"] > 0 and buckets["overlay"] > 0 and buckets["threshold"] == 0
    ctx.profile_reset()
    ctx.framestab_close()
