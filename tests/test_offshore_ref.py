"""The numpy statement of the offshore frame (tests/_offshore_ref.py) against a separable distance transform written on its own,
against cases worked by hand, and against the figures of the prototype the product was specified with."""
import numpy as np
import pytest

import _offshore_ref as R

LUT = np.stack([np.arange(256)] * 3, -1).astype(np.uint8)         # entry k is (k, k, k): the entry can be read off a picture


def separable(wet):
    """the two-pass form: per class and pixel the row of the nearest pixel of the class in its own column, the upper on a tie; then
    per pixel the least key (dx^2 + dy^2, raster index) over every column's entry for the other class.  Plain loops, no numpy"""
    c = (np.asarray(wet) != 0).tolist()
    h, w = len(c), len(c[0])
    g = [[[-1] * w for _ in range(h)] for _ in range(2)]
    for x in range(w):
        for t in (0, 1):
            rows = [y for y in range(h) if c[y][x] == bool(t)]
            for y in range(h):
                if rows:
                    g[t][y][x] = min(rows, key=lambda r: (abs(r - y), r))
    d2 = [[R.FAR] * w for _ in range(h)]
    near = [[-1] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            other = g[0 if c[y][x] else 1][y]
            keys = [((x - xc) ** 2 + (y - other[xc]) ** 2, other[xc] * w + xc) for xc in range(w) if other[xc] >= 0]
            if keys:
                d2[y][x], near[y][x] = min(keys)
    return np.array(d2, np.int64), np.array(near, np.int64)


@pytest.mark.parametrize("name", ["random 37 x 23", "beach 40 x 30", "speckle 99 %", "column", "row"])
def test_the_statement_equals_a_separable_form_ties_included(name):
    wet = {"random 37 x 23": lambda: R.speckle(37, 23, 0.5, 1), "beach 40 x 30": lambda: R.beach(40, 30, 12.0, 4.0, 16.0),
           "speckle 99 %": lambda: R.speckle(31, 29, 0.99, 2), "column": lambda: R.speckle(1, 40, 0.7, 3), "row": lambda: R.speckle(40, 1, 0.7, 4)}[name]()
    d2, near, tied = R.distance_map(wet, count_ties=True)
    sd2, snear = separable(wet)
    assert np.array_equal(d2, sd2) and np.array_equal(near, snear)
    if name == "random 37 x 23":
        assert tied > 100
    if name == "beach 40 x 30":
        assert tied > 40
    # a chunk of one pixel at a time gives the same
    d2c, nearc = R.distance_map(wet, chunk=1)
    assert np.array_equal(d2, d2c) and np.array_equal(near, nearc)


def test_one_dry_pixel():
    w, h = 7, 5
    wet = np.full((h, w), 255, np.uint8)
    wet[1, 2] = 0
    ref = R.OffshoreRef(w, h, R.Params(max_dist=10), LUT)
    m = ref.map(wet)
    y, x = np.mgrid[0:h, 0:w]
    want = (x - 2) ** 2 + (y - 1) ** 2
    assert np.array_equal(np.abs(m["dist2"]), np.where(want == 0, 1, want)) and m["dist2"][1, 2] == -1
    assert (m["near"][wet != 0] == 1 * w + 2).all() and m["near"][1, 2] == 0 * w + 2          # of four at distance 1 the smallest index
    assert m["sdist"][1, 6] == 256 and m["sdist"][4, 2] == 192 and m["sdist"][2, 3] == 90 and m["sdist"][1, 2] == -64       # floor(64 sqrt 2) = 90
    assert list(m["summary"]) == [34, 1, 34, 25, int(want.sum()), 1, 0, 1]
    assert tuple(m["picture"][1, 2]) == R.DRY_BGR and tuple(m["picture"][1, 6]) == (4 * 255 // 10,) * 3
    # the flow (1, 0): away from the shore on the right of the pixel, towards it on the left
    f = np.zeros((h, w, 2), np.float32)
    f[..., 0] = 1.0
    p = ref.push(f)
    assert p["cls"][1, 2] == R.DRY and (p["cls"][wet != 0] == R.OK).all()
    ca = p["cross_along"]
    assert ca[1, 5, 0] == 1.0 and ca[1, 0, 0] == -1.0 and ca[4, 2, 0] == 0.0 and ca[4, 2, 1] == -1.0 and ca[0, 2, 1] == 1.0
    assert np.isnan(ca[1, 2]).all() and ca.view(np.uint32)[1, 2, 0] == R.NAN_BITS
    assert p["sides"]["cross"][2, 3] == R.rdiv(64 * 64, 90)       # n = (1, 1), q = (64, 0): C = 64, r = 90


def test_two_dry_pixels_equidistant_from_a_wet_one():
    wet = np.full((3, 5), 255, np.uint8)
    wet[1, 1] = wet[1, 3] = 0
    d2, near, tied = R.distance_map(wet, count_ties=True)
    assert d2[1, 2] == 1 and near[1, 2] == 1 * 5 + 1              # the left one: the smaller raster index
    assert d2[0, 2] == 2 and near[0, 2] == 6 and d2[2, 2] == 2 and near[2, 2] == 6 and tied >= 3
    wet = np.full((5, 3), 255, np.uint8)
    wet[1, 1] = wet[3, 1] = 0
    d2, near = R.distance_map(wet)
    assert d2[2, 1] == 1 and near[2, 1] == 1 * 3 + 1              # the upper one
    assert near[2, 0] == 4 and near[2, 2] == 4


def test_a_checkerboard():
    w, h = 6, 5
    y, x = np.mgrid[0:h, 0:w]
    wet = np.where((x + y) % 2 == 0, 255, 0).astype(np.uint8)
    m = R.OffshoreRef(w, h, R.Params(), LUT).map(wet)
    assert (np.abs(m["dist2"]) == 1).all() and (np.abs(m["sdist"]) == 64).all()
    up = (y - 1) * w + x
    assert np.array_equal(m["near"], np.where(y > 0, up, np.where(x > 0, x - 1, 1)))           # above; in the top row to the left; (0, 0) to the right


def test_all_wet_and_all_dry():
    w, h = 4, 3
    for value, sign in ((255, 1), (0, -1)):
        ref = R.OffshoreRef(w, h, R.Params(stations=2, bins=2), LUT)
        m = ref.map(np.full((h, w), value, np.uint8))
        assert (m["dist2"] == sign * R.FAR).all() and (m["sdist"] == sign * R.FAR).all() and (m["near"] == -1).all() and not m["picture"].any()
        assert list(m["summary"]) == ([12, 0] if value else [0, 12]) + [0, 0, 0, 0, 0, 1]
        p = ref.push(np.ones((h, w, 2), np.float32))
        assert (p["cls"] == (R.C_FAR if value else R.DRY)).all() and not p["table"].any() and (p["stations"]["flags"] == R.EMPTY).all()
        assert not ref.band(0, 100).any()


def test_the_prototype():
    w, h, wet, flow, p = R.prototype()
    assert (w, h) == (96, 64) and (p.min_dist, p.max_dist, p.stations, p.bins, p.bin_width, p.min_count, p.cross_min, p.station) == (3, 40, 8, 8, 5, 8, 1.0, "x")
    ref = R.OffshoreRef(w, h, p, LUT)
    d2, near, tied = R.distance_map(wet, count_ties=True)
    m = ref.map(wet)
    assert np.array_equal(np.abs(m["dist2"]), d2) and np.array_equal(m["near"], near)
    assert list(m["summary"]) == [4224, 1920, 4224, 2074, 2517482, 245999, 0, 1] and tied == 364
    assert int(near.sum()) == 12299798 and int(np.abs(m["sdist"]).astype(np.int64).sum()) == 6927040
    q = ref.push(flow)
    s = q["sides"]
    assert q["summary"][0] == 3745 and q["summary"][4] == 1 and s["beyond"].sum() == 16
    assert s["cross"].sum() == 15240 and s["along"].sum() == -241909 and np.abs(s["cross"]).max() == 128 and np.abs(s["along"]).max() == 128
    assert q["summary"][5] == 458 and (q["mask"] != 0).sum() == 458
    assert (ref.band(10, 25) != 0).sum() == 1507
    t = q["table"].reshape(8, 8, R.SUMS)
    assert list(t[4, :, 0]) == [24, 65, 62, 62, 60, 61, 61, 60]
    assert [int(R.rdiv(int(a), int(b))) for a, b in zip(t[4, :, 1], t[4, :, 0])] == [108, 108, 112, 113, 116, 117, 119, 120]
    assert list(q["stations"]["reach_end"]) == [0, 0, 0, 0, 8, 0, 0, 0]
    r4 = q["stations"][4]
    assert (r4["flags"], r4["first"], r4["peak_bin"], r4["peak_cross"], r4["count"]) == (R.RIP, 0, 7, 120, 455) and q["summary"][6] == 1
    assert t[..., 0].sum() + s["beyond"].sum() == 3745 and t[..., 1].sum() + s["cross"][s["ok"] & (s["bin"] >= 8)].sum() == 15240


def test_records_on_a_table_made_by_hand():
    """one station by y over a shore on the left edge: the flow away from it in the rings 1 and 2 only"""
    w, h = 30, 8
    wet = np.full((h, w), 255, np.uint8)
    wet[:, 0] = 0
    f = np.zeros((h, w, 2), np.float32)
    f[:, 5:15, 0] = 2.0                                            # distances 5..14: the rings 1 and 2 of width 5
    f[:, 20:25, 0] = 3.0                                           # ring 4, beyond a break
    ref = R.OffshoreRef(w, h, R.Params(min_dist=0, max_dist=26, stations=1, bins=5, bin_width=5, min_count=8, rip_bins=2, cross_min=1.0, station="y"), LUT)
    ref.map(wet)
    q = ref.push(f)
    rec = q["stations"][0]
    assert list(q["table"][:, 0]) == [32, 40, 40, 40, 40] and rec["beyond"] == 2 * 8              # the distances 25 and 26; 27 on is FAR
    assert (rec["first"], rec["reach_end"], rec["flags"]) == (0, 0, 0)            # ring 0 has the pixels but not the flow: the run is empty
    assert (rec["peak_bin"], rec["peak_cross"], rec["count"], rec["mean_cross"]) == (4, 192, 0, 0.0)
    ref.set(R.Params(min_dist=5, max_dist=26, stations=1, bins=5, bin_width=5, min_count=8, rip_bins=2, cross_min=1.0, station="y"))
    rec = ref.push(f)["stations"][0]                               # without ring 0 the run is the rings 1 and 2
    assert (rec["first"], rec["reach_end"], rec["flags"], rec["peak_bin"], rec["count"], rec["mean_cross"], rec["mean_along"]) == (1, 3, R.RIP, 4, 80, 2.0, 0.0)
