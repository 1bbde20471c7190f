"""The numpy restatement of the general warps and of the multi-patch fit (tests/_framewarp_ref.py) against known
answers: the checker itself has to be right before the device is held to it."""
import numpy as np

import _framestab_ref as S
import _framewarp_ref as W


def _img(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_translations_over_every_phase_equal_the_translate_warp():
    img = _img(13, 19, 1)
    for fy in range(32):
        for fx in range(32):
            sx, sy = 2 + fx / 32.0, -1 + fy / 32.0
            got = W.warp_affine(img, [[1, 0, sx], [0, 1, sy]], inverse_map=True)
            assert np.array_equal(got, S.warp_translate(img, sx, sy)), (fx, fy)
    # the forward form: warpAffine(img, [1 0 -sx; 0 1 -sy]) as the reference calls it
    assert np.array_equal(W.warp_affine(img, [[1, 0, -3.7], [0, 1, 2.2]]), S.warp_translate(img, 3.7, -2.2))
    for sy in (0.5 / 1024, 1.5 / 1024, 7 + 0.5 / 1024, 1 / 3.0):      # rounding ties of y + shift
        assert np.array_equal(W.warp_affine(_img(300, 9, 2), [[1, 0, 0.4], [0, 1, sy]], inverse_map=True),
                              S.warp_translate(_img(300, 9, 2), 0.4, sy))


def test_identity_is_a_copy_rotation_and_flip_are_exact():
    img = _img(24, 24, 3)
    assert np.array_equal(W.warp_affine(img, [[1, 0, 0], [0, 1, 0]]), img)
    assert np.array_equal(W.warp_perspective(img, np.eye(3)), img)
    # dst(x, y) = src(23 - y, x): a quarter turn about the centre
    assert np.array_equal(W.warp_affine(img, [[0, -1, 23], [1, 0, 0]], inverse_map=True), np.rot90(img, 1))
    assert np.array_equal(W.warp_affine(img, [[0, 1, 0], [-1, 0, 23]], inverse_map=True), np.rot90(img, -1))
    # a flip with an integer shift: dst(x, y) = src(20 - x, y + 2), zero where the source ends
    got = W.warp_affine(img, [[-1, 0, 20], [0, 1, 2]], inverse_map=True)
    want = np.zeros_like(img)
    want[:22, :21] = img[2:, 20::-1]
    assert np.array_equal(got, want)
    # a destination size of its own
    got = W.warp_affine(img, [[1, 0, 4], [0, 1, 6]], dsize=(7, 5), inverse_map=True)
    assert got.shape == (5, 7, 3) and np.array_equal(got, img[6:11, 4:11])


def test_affine_inversion_matches_the_matrix_inverse():
    rng = np.random.RandomState(4)
    for _ in range(20):
        M = np.hstack([np.eye(2) + rng.uniform(-0.3, 0.3, (2, 2)), rng.uniform(-50, 50, (2, 1))])
        inv = np.linalg.inv(np.vstack([M, [0, 0, 1]]))[:2]
        assert np.abs(W.invert_affine(M) - inv).max() < 1e-12
    assert np.array_equal(W.invert_affine([[1, 0, -3.5], [0, 1, 2.25]]), [[1, 0, 3.5], [0, 1, -2.25]])
    H = np.array([[1.02, 0.01, 3.0], [-0.02, 0.98, -4.0], [1e-5, -2e-5, 1.0]])
    assert np.abs(W.invert_perspective(H) - np.linalg.inv(H)).max() < 1e-12


def test_perspective_special_cases():
    img = _img(40, 90, 5)
    # no projective part, whole-pixel translation: the affine result
    for (tx, ty) in ((3, -2), (0, 0), (-70, 11)):
        A = [[1, 0, tx], [0, 1, ty]]
        assert np.array_equal(W.warp_perspective(img, A + [[0, 0, 1]], inverse_map=True), W.warp_affine(img, A, inverse_map=True))
    # a smooth affine map agrees wherever the double path and the fixed-point path round the same way: nearly everywhere
    A = np.array([[0.998, -0.01, 1.3], [0.012, 1.003, -0.7]])
    a, b = W.warp_perspective(img, np.vstack([A, [0, 0, 1]]), inverse_map=True), W.warp_affine(img, A, inverse_map=True)
    assert (np.abs(a.astype(int) - b.astype(int)) > 8).mean() < 0.02
    # M8 = 2 halves the coordinates: dst(x, y) = src(x / 2, y / 2)
    got = W.warp_perspective(img, np.diag([1.0, 1.0, 2.0]), inverse_map=True)
    assert np.array_equal(got[::2, ::2], img[:20, :45])
    sx, sy, fx, fy = W.perspective_coords(np.diag([1.0, 1.0, 2.0]), 90, 40)
    assert np.array_equal(sx[0], np.arange(90) // 2) and np.array_equal(fx[0], (np.arange(90) % 2) * 16) and not fy[0].any()


def test_perspective_tiling_and_clamps():
    assert W.perspective_block(1920, 1080) == 64 and W.perspective_block(640, 480) == 64
    assert W.perspective_block(5, 3) == 5 and W.perspective_block(500, 3) == 341 and W.perspective_block(40, 100) == 40
    # the bits depend on xb: M0 = 0.1 has no exact double, so 0.1 * 64 + 0.1 * 1 and 0.1 * 65 differ in the last place
    M = np.array([[0.1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    sx, _, fx, _ = W.perspective_coords(M, 200, 16)
    X = (sx[0] << 5) | fx[0]
    xb, x1 = (np.arange(200) // 64) * 64.0, (np.arange(200) % 64).astype(np.float64)
    assert np.array_equal(X, np.rint((0.1 * xb + 0.1 * x1) * 32.0).astype(np.int64))
    # W = 0 on the column x = 10: the pixel reads source (0, 0); W changes sign across it: the other sheet of the map
    M = np.array([[1.0, 0, 0], [0, 1.0, 0], [0.1, 0, -1.0]])
    sx, sy, fx, fy = W.perspective_coords(M, 32, 4)
    assert sx[0, 10] == 0 and sy[2, 10] == 0 and fx[0, 10] == 0
    assert (sx[0, 1:10] < 0).all() and (sx[0, 11:] > 0).all()          # x / (0.1 x - 1): negative before, positive after
    assert sx[0, 11] == 110 and sx[0, 9] == -90                        # 11 / 0.1 and 9 / -0.1
    img = _img(4, 32, 6)
    out = W.warp_perspective(img, M, inverse_map=True)
    assert np.array_equal(out[0, 10], img[0, 0]) and not out[:, 1:10].any()
    # a huge quotient clamps to INT_MAX before cvRound and to SHRT_MAX after: outside any frame, zero
    M = np.array([[1e300, 0, 1e300], [0, 1.0, 0], [0, 0, 1e-300]])
    sx, sy, fx, fy = W.perspective_coords(M, 8, 2)
    assert (sx == 32767).all() and (fx == 31).all()
    assert not W.warp_perspective(_img(2, 8), M, inverse_map=True).any()


ROIS = [(20, 20, 50, 50), (570, 20, 50, 50), (20, 410, 50, 50), (570, 410, 50, 50), (300, 30, 50, 50)]


def _shifts_of(T, rois, resp=0.5):
    c = W.patch_centres(rois)
    d = c @ np.asarray(T)[:, :2].T + np.asarray(T)[:, 2] - c
    return np.hstack([d, np.full((len(c), 1), resp)])


def test_fit_recovers_similarity_and_affine():
    ang, s = np.deg2rad(0.27), 1.004
    T = np.array([[s * np.cos(ang), -s * np.sin(ang), 3.25], [s * np.sin(ang), s * np.cos(ang), -1.5]])
    for model in (W.SIMILARITY, W.AFFINE):
        m, used, n, res = W.fit_motion(ROIS, _shifts_of(T, ROIS), model, 0.1, (640, 480))
        assert used == model and n == 5 and np.abs(m - T).max() < 1e-12
        centre = T[:, :2] @ [319.5, 239.5] + T[:, 2] - [319.5, 239.5]
        assert abs(res[0] - centre[0]) < 1e-11 and abs(res[1] - centre[1]) < 1e-11 and res[2] == 0.5
    T = np.array([[1.003, 0.004, -2.0], [-0.002, 0.997, 0.75]])
    m, used, n, _ = W.fit_motion(ROIS, _shifts_of(T, ROIS), W.AFFINE, 0.1, (640, 480))
    assert used == W.AFFINE and np.abs(m - T).max() < 1e-12
    m, used, _, _ = W.fit_motion(ROIS, _shifts_of(T, ROIS), W.TRANSLATION, 0.1, (640, 480))
    assert used == W.TRANSLATION and np.array_equal(m[:, :2], np.eye(2))


def test_fit_of_a_still_scene_is_the_identity_exactly():
    z = np.zeros((5, 3))
    z[:, 2] = 0.9
    for model in (W.TRANSLATION, W.SIMILARITY, W.AFFINE):
        m, used, n, res = W.fit_motion(ROIS, z, model, 0.1, (640, 480))
        assert used == model and np.array_equal(m, [[1, 0, 0], [0, 1, 0]]) and res[:2] == (0.0, 0.0)


def test_fit_ladder():
    T = np.array([[1.002, -0.003, 1.5], [0.003, 1.002, -2.0]])
    sh = _shifts_of(T, ROIS)
    # one patch and the translation model: its shift as it is
    m, used, n, res = W.fit_motion(ROIS[:1], [[1.25, -0.5, 0.7]], W.TRANSLATION, 0.0, (640, 480))
    assert used == W.TRANSLATION and n == 1 and np.array_equal(m, [[1, 0, 1.25], [0, 1, -0.5]]) and res == (1.25, -0.5, 0.7)
    # gated out: the weak patch takes no part, a NaN response fails the comparison
    g = sh.copy()
    g[4, :2] += 30.0
    g[4, 2] = 0.05
    m, used, n, res = W.fit_motion(ROIS, g, W.SIMILARITY, 0.1, (640, 480))
    assert n == 4 and np.abs(m - T).max() < 1e-12 and res[2] == 0.5
    g[3, 2] = np.nan
    assert W.fit_motion(ROIS, g, W.SIMILARITY, 0.1, (640, 480))[2] == 3
    # two patches for affine: similarity; one: translation; none: the identity and model 0
    g = sh.copy()
    g[2:, 2] = 0.0
    m, used, n, _ = W.fit_motion(ROIS, g, W.AFFINE, 0.1, (640, 480))
    assert used == W.SIMILARITY and n == 2 and np.abs(m - T).max() < 1e-12
    g[1, 2] = 0.0
    m, used, n, _ = W.fit_motion(ROIS, g, W.AFFINE, 0.1, (640, 480))
    assert used == W.TRANSLATION and n == 1 and np.array_equal(m[:, 2], sh[0, :2])
    g[0, 2] = 0.0
    m, used, n, res = W.fit_motion(ROIS, g, W.AFFINE, 0.1, (640, 480))
    assert used == 0 and n == 0 and np.array_equal(m, [[1, 0, 0], [0, 1, 0]]) and res == (0.0, 0.0, 0.0)
    # collinear centres: the affine normal matrix is singular, similarity is not
    line = [(20, 100, 50, 50), (220, 100, 50, 50), (520, 100, 50, 50)]
    m, used, n, _ = W.fit_motion(line, _shifts_of(T, line), W.AFFINE, 0.1, (640, 480))
    assert used == W.SIMILARITY and n == 3 and np.abs(m - T).max() < 1e-12
    # coincident centres: translation
    same = [(20, 100, 50, 50), (20, 100, 50, 50)]
    assert W.fit_motion(same, _shifts_of(T, same), W.AFFINE, 0.1, (640, 480))[1] == W.TRANSLATION


def test_multi_chain_with_one_patch_is_the_single_patch_chain():
    clip, _ = S.shaken_clip(160, 120, 5, roi=(100, 30, 40, 40), block=60, max_shake=3.0)
    one, multi = S.FrameStabRef(160, 120, (100, 30, 40, 40)), W.MultiStabRef(160, 120, [(100, 30, 40, 40)], "translation")
    for t in range(5):
        a, ra = one.push(clip[t])
        b, sh, fit = multi.push(clip[t])
        assert np.array_equal(a, b), t
        if t:
            assert tuple(sh[0]) == ra and fit[3] == ra and fit[1] == W.TRANSLATION


def test_multi_chain_holds_the_corners_of_a_rolling_clip():
    """The numpy chain on a small rolling, breathing, shaking clip: four corner patches and the similarity model hold
    every corner; one patch and a translation leave the opposite corner several times farther out."""
    w, h = 320, 240
    clip, motions = W.rolling_clip(w, h, 8, seed=3, max_roll_deg=0.6, max_zoom=0.01, max_shake=3.0)
    rois = W.corner_rois(w, h, 48, 12)
    multi = W.MultiStabRef(w, h, rois, "similarity", anchor="first")
    single = S.FrameStabRef(w, h, rois[0])
    worst_m = worst_s = 0.0
    for t in range(8):
        out, sh, fit = multi.push(clip[t])
        outs, _ = single.push(clip[t])
        if t:
            assert fit[1] == W.SIMILARITY and fit[2] == 4
            inv = W.invert_affine(motions[t])           # frame_t(p) = scene(T_t p): the correction undoes T_t
            assert np.abs(fit[0][:, :2] - inv[:, :2]).max() < 4e-3 and np.abs(fit[0][:, 2] - inv[:, 2]).max() < 1.0, (t, fit[0], inv)
            worst_m = max(worst_m, max(W.patch_drift(r, clip[0], out) for r in rois))
            worst_s = max(worst_s, W.patch_drift(rois[3], clip[0], outs))
    assert worst_m < 1.0 and worst_s > 2.0 * worst_m, (worst_m, worst_s)
