"""Known answers on the numpy statement of the opposing-flow map (tests/_ripmap_ref.py): what the device is held to."""
import numpy as np

import _ripmap_ref as R

f32 = np.float32


def field(w, h, v=(1.0, 0.0)):
    f = np.zeros((h, w, 2), f32)
    f[...] = v
    return f


def vec(deg, mag=1.0):
    return (mag * np.cos(np.radians(deg)), mag * np.sin(np.radians(deg)))


def opposed_of(f, grid=(30, 30), **kw):
    sums, bad = R.cell_sums(f, *grid)
    assert bad == 0
    return R.decide(sums, **kw)


def test_uniform_field_opposes_nowhere():
    r = opposed_of(field(300, 240, (0.7, -0.2)))
    assert r["opposed_cells"] == 0 and r["live_cells"] == 900
    x, y = np.rint(0.7 * 65536), np.rint(-0.2 * 65536)   # 16.16 fixed point: a direction is good to about 1e-3 degrees
    assert abs(r["direction"] - (360 + np.degrees(np.arctan2(y, x)))) < 1e-9
    assert abs(r["mean_magnitude"] - np.hypot(x, y) / 65536) < 1e-12
    assert np.all(r["cells"][..., 2] < 1e-3)


def test_block_against_the_field_flags_exactly_its_cells():
    w, h = 300, 240                      # cells of 10 x 8 pixels
    f = field(w, h)
    f[4 * 8:5 * 8, 2 * 10:4 * 10] = (-1.0, 0.0)       # cells (cx 2..3, cy 4)
    r = opposed_of(f)
    want = np.zeros((30, 30), bool)
    want[4, 2:4] = True
    assert np.array_equal(r["opposed"], want)
    assert np.allclose(r["cells"][4, 2:4, :3], [-1, 0, 180]) and np.allclose(r["cells"][0, 0, :3], [1, 0, 0])
    m = R.mask_of(r["opposed"], w, h)
    assert m.sum() == 255 * 160 and np.all(m[32:40, 20:40] == 255)


def test_the_threshold_is_0_7_pi():
    w, h = 300, 240
    for deg, flagged in ((100, False), (125, False), (127, True), (130, True), (-130, True), (180, True)):
        f = field(w, h)
        f[32:40, 20:40] = vec(deg)
        r = opposed_of(f)
        # G is tilted by the block itself by less than 0.2 degrees
        assert r["opposed_cells"] == (2 if flagged else 0), deg
        assert abs(r["cells"][4, 2, 2] - abs(deg)) < 0.3


def test_a_straddling_cell_follows_its_sum():
    w, h = 300, 240
    f = field(w, h)
    f[32:40, 20:26] = (-1.0, 0.0)        # 6 of cell (2, 4)'s 10 columns: the sum points back
    assert opposed_of(f)["opposed"][4, 2]
    f = field(w, h)
    f[32:40, 20:24] = (-1.0, 0.0)        # 4 of 10: it points forward
    assert opposed_of(f)["opposed_cells"] == 0


def test_sums_do_not_depend_on_the_order_of_addition():
    rng = np.random.RandomState(5)
    f = (rng.standard_normal((61, 97, 2)) * 3).astype(f32)
    base, _ = R.cell_sums(f, 7, 5)
    for seed in range(3):
        order = np.random.RandomState(seed).permutation(61 * 97)
        s, _ = R.cell_sums(f, 7, 5, order=order)
        assert np.array_equal(s, base)
    assert R.decide(base)["opposed"].dtype == bool


def test_the_seam_case_flags_where_a_linear_angle_mean_would_not():
    # a cell whose pixels point to 350 and 10 degrees (towards +x) against G at 180: the reference's linear mean of the
    # angles is (350 + 10) / 2 = 180, "with the flow"; the summed vector points to 0
    w, h = 300, 240
    f = field(w, h, vec(180))
    f[32:40, 20:25] = vec(350)
    f[32:40, 25:30] = vec(10)
    r = opposed_of(f)
    want = np.zeros((30, 30), bool)
    want[4, 2] = True
    assert np.array_equal(r["opposed"], want)
    assert abs(r["cells"][4, 2, 2] - 180) < 0.1


def test_remainder_goes_to_the_last_cell():
    w, h = 97, 61                        # 97 // 7 = 13, 61 // 5 = 12: 6 columns and 1 row over
    assert R.cell_index(97, 7)[-7:].tolist() == [6] * 7 and R.cell_index(97, 7)[77] == 5
    sums, _ = R.cell_sums(field(w, h), 7, 5)
    assert sums[0, 0, 2] == 13 * 12 and sums[0, 6, 2] == 19 * 12 and sums[4, 6, 2] == 19 * 13
    assert sums[..., 2].sum() == w * h and np.all(sums[..., 0] == sums[..., 2] * 65536)


def test_bad_pixels_are_left_out():
    f = field(64, 48)
    f[3, 5] = (np.nan, 0)
    f[4, 6] = (0, np.inf)
    f[5, 7] = (1e9, 0)                   # beyond 2^40 in fixed point
    f[6, 8] = (1e6, 0)                   # inside
    sums, bad = R.cell_sums(f, 1, 1)
    assert bad == 3 and sums[0, 0, 2] == 64 * 48 - 3
    assert sums[0, 0, 0] == (64 * 48 - 4) * 65536 + 1000000 * 65536 and sums[0, 0, 1] == 0
    assert R.max_magnitude(f) == np.inf


def test_min_cell_mag_and_the_fill_gate():
    w, h = 300, 240
    f = field(w, h)
    f[32:40, 20:40] = (-0.25, 0.0)
    assert opposed_of(f)["opposed_cells"] == 2
    assert opposed_of(f, M=0.25)["opposed_cells"] == 2 and opposed_of(f, M=0.26)["opposed_cells"] == 0
    assert opposed_of(f, gate=True)["opposed_cells"] == 0
    ref = R.RipMapRef(w, h, 3, wait_full=True)
    got = [ref.push(f)["opposed_cells"] for _ in range(4)]
    assert got == [0, 0, 2, 2]


def test_the_ring_expires():
    # the bug of the original (the ring passed by value, never expiring): after `window` pushes of a new field the old
    # one has left the mean but for the rounding of the running sum
    w, h = 60, 40
    ref = R.RipMapRef(w, h, 4, grid=(6, 4))
    for _ in range(4):
        ref.push(field(w, h, (2.0, 0.0)))
    for _ in range(4):
        r = ref.push(field(w, h, (0.0, -1.0)))
    assert np.allclose(r["mean"], (0.0, -1.0), atol=1e-6) and abs(r["direction"] - 270) < 1e-3
    assert r["frames_pushed"] == 8 and r["scale_in"] > 0


def test_get_delta_from_a_zero_point():
    rng = np.random.RandomState(2)
    f = rng.standard_normal((9, 11, 2)).astype(f32)
    f[4, 4] = (30, 40)                   # |v| = 50 > UPPER
    d = R.get_delta_zero(f, UPPER=10.0)
    assert np.all(d[0] == 0) and np.all(d[-1] == 0) and np.all(d[:, 0] == 0) and np.all(d[:, -1] == 0)
    assert np.all(d[4, 4] == 0) and np.array_equal(d[3, 3], f[3, 3] * f32(2))
