"""The numpy restatement of the reference's frame stabilisation (tests/_framestab_ref.py) against known answers: the
checker itself has to be right before the device is held to it."""
import numpy as np

import _framestab_ref as R


def test_optimal_dft_size_known_answers():
    for n, want in ((1, 1), (8, 8), (50, 50), (51, 54), (97, 100), (241, 243), (256, 256), (257, 270), (7, 8), (11, 12)):
        assert R.optimal_dft_size(n) == want, n


def test_hanning_window_is_the_square_root_form():
    w = R.hanning_window(50, 50)
    assert w.dtype == np.float32 and w.shape == (50, 50)
    assert w[0, 0] == 0 and w[49, 49] < 1e-7 and w[0, 25] == 0
    # the square root: sin(pi i / (n - 1)) sin(pi j / (n - 1)), not its square
    i = np.arange(50)
    want = np.sin(np.pi * i / 49)[:, None] * np.sin(np.pi * i / 49)[None, :]
    assert np.abs(w - want).max() < 1e-6
    assert R.hanning_window(37, 51).shape == (37, 51)


def test_circular_integer_shift_is_recovered_exactly():
    rng = np.random.RandomState(1)
    for (h, w, dy, dx) in ((50, 50, 3, -7), (64, 64, -20, 11), (48, 80, 0, 1), (50, 50, 0, 0)):
        a = rng.rand(h, w).astype(np.float32)
        sx, sy, resp = R.phase_correlate(a, np.roll(a, (dy, dx), (0, 1)))
        assert abs(sx - dx) < 1e-6 and abs(sy - dy) < 1e-6, (h, w, sx, sy)
        assert abs(resp - 1.0) < 1e-5


def test_odd_optimal_size_reports_half_a_pixel():
    """fftShift sends index 0 to floor(n / 2) while the centre is n / 2.0: 25 x 25 reports +0.5 for no shift."""
    a = np.random.RandomState(2).rand(25, 25).astype(np.float32)
    sx, sy, _ = R.phase_correlate(a, a)
    assert abs(sx - 0.5) < 1e-6 and abs(sy - 0.5) < 1e-6
    sx, sy, _ = R.phase_correlate(a, np.roll(a, (2, -3), (0, 1)))
    assert abs(sx - (-3 + 0.5)) < 1e-6 and abs(sy - (2 + 0.5)) < 1e-6


def test_padded_patch_and_first_maximum():
    a = np.random.RandomState(3).rand(37, 51).astype(np.float32)
    s = R.correlation_surface(a, a)
    assert s.shape == (40, 54) and s.dtype == np.float32
    assert np.unravel_index(int(np.argmax(s)), s.shape) == (20, 27)
    flat = np.zeros((16, 16), np.float32)                  # an all-zero spectrum: C = 0 everywhere, the first index wins
    sx, sy, resp = R.phase_correlate(flat, flat)
    assert (sx, sy, resp) == (8.0, 8.0, 0.0)


def test_subpixel_shift_with_the_window():
    """A dense texture displaced by a fraction of a pixel: the 5 x 5 centroid of upstream's estimator pulls towards
    the nearest whole pixel (a true 0.5 reads about 0.2-0.3), so the bound is what that estimator gives: 0.6 px."""
    tex = R.DenseTexture(256, 3)
    win = R.hanning_window(50, 50)
    a = tex.u8()[100:150, 100:150].astype(np.float32)
    for d in ((0.25, 0.0), (1.5, -2.25), (3.0, 0.0), (-2.0, 1.0), (5.75, 3.5), (-6.0, 6.0)):
        b = tex.u8(*d)[100:150, 100:150].astype(np.float32)
        sx, sy, resp, s = R.phase_correlate(a, b, win, return_surface=True)
        assert abs(sx - d[0]) < 0.6 and abs(sy - d[1]) < 0.6, (d, sx, sy)
        assert resp > 0.3 and not R.peak_is_ambiguous(s)


def test_sign_convention_warp_restores_prev():
    tex = R.DenseTexture(256, 4)
    prev = np.repeat(tex.u8()[:96, :128, None], 3, 2)
    for d in ((3, -2), (-5, 4)):
        curr = np.repeat(tex.u8(*d)[:96, :128, None], 3, 2)          # curr(x) = prev(x - d)
        sx, sy, _ = R.phase_correlate(R.bgr_to_gray(prev[20:70, 40:90]).astype(np.float32),
                                      R.bgr_to_gray(curr[20:70, 40:90]).astype(np.float32), R.hanning_window(50, 50))
        assert round(sx) == d[0] and round(sy) == d[1]
        back = R.warp_translate(curr, float(d[0]), float(d[1]))
        inner = (slice(8, 88), slice(8, 120))
        assert np.abs(back[inner].astype(int) - prev[inner].astype(int)).max() <= 1      # two roundings to 8 bits


def test_bgr_to_gray():
    assert R.bgr_to_gray(np.array([[[255, 255, 255], [0, 0, 0], [7, 7, 7], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)).tolist() \
        == [[255, 0, 7, 29, 150, 76]]


def test_integer_warps_are_zero_filled_rolls():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (23, 31, 3)).astype(np.uint8)
    for (dx, dy) in ((0, 0), (3, 0), (0, -4), (-5, 7), (30, 22), (-30, -22)):
        want = np.zeros_like(img)
        ys, xs = np.arange(23) + dy, np.arange(31) + dx
        oky, okx = (ys >= 0) & (ys < 23), (xs >= 0) & (xs < 31)
        want[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
        assert np.array_equal(R.warp_translate(img, dx, dy), want), (dx, dy)
    assert np.array_equal(R.warp_translate(img[..., 0], 2, 1)[:-1, :-2], img[1:, 2:, 0])     # 8UC1 too


def test_half_pixel_warp_is_the_rounded_mean():
    rng = np.random.RandomState(6)
    img = rng.randint(0, 256, (9, 40, 3)).astype(np.int64)
    got = R.warp_translate(img.astype(np.uint8), 0.5, 0.0)
    assert np.array_equal(got[:, :-1], (img[:, :-1] + img[:, 1:] + 1) >> 1)
    got = R.warp_translate(img.astype(np.uint8), 0.0, 0.5)
    assert np.array_equal(got[:-1], (img[:-1] + img[1:] + 1) >> 1)
    assert np.array_equal(got[-1], (img[-1] + 1) >> 1)                 # the tap below the frame counts 0


def test_warp_weights_sum_to_one():
    W = R.warp_weights()
    assert W.shape == (32, 32, 4) and (W.sum(-1) == 1 << 15).all() and (W >= 0).all()
    assert W[0, 0].tolist() == [1 << 15, 0, 0, 0]


def test_warp_fraction_grid_and_rounding():
    img = np.zeros((4, 8, 3), np.uint8)
    img[:, 4] = 200
    # 1/32 px, to nearest through the + 16: 1/128 -> 0, 1/64 -> 1/32, 3/64 -> 2/32 (cvRound(48) + 16 = 64 -> X = 2)
    assert np.array_equal(R.warp_translate(img, 1 / 128.0, 0), img)
    assert R.warp_translate(img, 1 / 64.0, 0)[0, 3, 0] == (200 * 1 * 32 * 32 + (1 << 14)) >> 15
    assert R.warp_translate(img, 3 / 64.0, 0)[0, 3, 0] == (200 * 2 * 32 * 32 + (1 << 14)) >> 15
    # negative shifts use the arithmetic shift: -0.25 -> integer part -1, fraction 24/32
    assert R.warp_translate(img, -0.25, 0)[0, 5, 0] == (200 * 8 * 32 * 32 + (1 << 14)) >> 15
    assert R.warp_translate(img, -0.25, 0)[0, 4, 0] == (200 * 24 * 32 * 32 + (1 << 14)) >> 15


def test_shift_past_the_frame_is_all_zero():
    img = np.full((12, 17, 3), 255, np.uint8)
    for d in ((17, 0), (-18, 0), (0, 12), (0, -13), (1000.25, -3000.5)):
        assert not R.warp_translate(img, *d).any(), d
    assert R.warp_translate(img, 16, 0)[:, 0].all() and not R.warp_translate(img, 16, 0)[:, 1:].any()


def test_chain_keeps_the_roi_in_place():
    """The loop with its loop-carried prev on a shaken clip: every frame is registered to the last corrected one, so
    the estimator's error (up to half a pixel per step: see test_subpixel_shift_with_the_window) walks; measured here,
    the ROI of the corrected frames stays within 2.3 px of frame 0 where the shaken frames are up to 6 px away.
    tests/test_gpu_framestab.py holds the device to the same bound on the same clip."""
    clip, shake = R.shaken_clip(320, 240, 24)
    ref = R.FrameStabRef(320, 240)
    assert ref.roi == (270, 50, 50, 50)
    worst = shaken = 0.0
    for t in range(len(clip)):
        out, res = ref.push(clip[t])
        if t == 0:
            assert res == (0.0, 0.0, 0.0) and np.array_equal(out, clip[0])
        else:
            assert np.array_equal(out, R.warp_translate(clip[t], res[0], res[1]))
        worst = max(worst, R.drift(ref, clip[0], out))
        shaken = max(shaken, R.drift(ref, clip[0], clip[t]))
    assert shaken > 5.0
    assert worst < 3.0, worst
