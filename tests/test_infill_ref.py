"""The numpy statement of the flow infill (tests/_infill_ref.py) against properties, not against itself, and against the figures of
the prototype the product was specified from (a shear with a Gaussian jet on 160 x 120, hole patterns p300, p900 and block40).
No GPU."""
import numpy as np
import pytest

import _infill_ref as R

W, H = 160, 120
LUT = R.plain_lut()
FIELD = R.shear_field(W, H)
_OUT = {}


def filled(pat, levels, min_known=1):
    key = (pat, levels, min_known)
    if key not in _OUT:
        v = R.pattern(pat, W, H)
        _OUT[key] = (v == 0, R.fill(FIELD, v, R.Params(levels=levels, min_known=min_known), LUT))
    return _OUT[key]


# ---------------------------------------------------------------------------- properties
@pytest.mark.parametrize("leave", ["nan", "zero"])
def test_known_pixels_keep_their_bits(leave):
    """-0.0, denormals and +-499.99 are KNOWN and come out as they went in; NaN with a valid byte of 255 is a hole"""
    f = R.hostile(FIELD, seed=1)
    v = R.pattern("p300", W, H)
    o = R.fill(f, v, R.Params(levels=7, leave=leave), LUT)
    known = o["sides"]["known"]
    assert known.any() and (o["source"][known] == 0).all() and (o["source"][~known] != 0).all()
    assert np.array_equal(o["filled"].view(np.uint32)[known], f.view(np.uint32)[known])
    assert (np.signbit(f[..., 0]) & (f[..., 0] == 0) & known).any()                # a -0.0 among them
    assert not known[np.isnan(f).any(-1)].any() and (v[np.isnan(f).any(-1)] != 0).any()
    assert (np.abs(f) >= 500).any(-1)[~known].any() and ((np.abs(f) == np.float32(499.99)).any(-1) & known).any()


def test_single_known_pixel_reaches_every_pixel_with_seven_levels():
    w, h = 37, 29
    f = np.full((h, w, 2), np.nan, np.float32)
    f[11, 23] = (1.25, -3.5)
    o = R.fill(f, None, R.Params(levels=7), LUT)
    assert (o["filled"] == np.float32([1.25, -3.5])).all() and o["summary"][0] == 1 and o["summary"][2] == w * h - 1 and o["summary"][3] == 0
    assert set(np.unique(o["source"])) <= set(range(8)) and o["source"].max() == 6     # 37 x 29 is one cell from level 6 on
    few = R.fill(f, None, R.Params(levels=2), LUT)
    assert 0 < few["summary"][2] < w * h - 1 and few["summary"][3] > 0


@pytest.mark.parametrize("leave,bits", [("nan", R.NAN_BITS), ("zero", 0)])
def test_all_holes_nothing_has_a_value(leave, bits):
    f = np.full((H, W, 2), np.inf, np.float32)
    o = R.fill(f, None, R.Params(levels=7, grid_x=4, grid_y=3, leave=leave), LUT)
    assert (o["source"] == R.UNFILLED).all() and (o["filled"].view(np.uint32) == bits).all() and not o["mask"].any()
    assert (o["cells"]["flags"] == R.NONE).all() and (o["cells"]["valued_pm"] == 0).all() and o["summary"][3] == W * H
    assert (o["picture"] == R.UNFILLED_BGR).all()


@pytest.mark.parametrize("pat,levels", [("p300", 7), ("p900", 2), ("block40", 2), ("block40", 7)])
def test_source_bytes_partition_the_picture_and_the_sums_add_up(pat, levels):
    v = R.pattern(pat, W, H)
    dom = np.zeros((H, W), np.uint8)
    dom[:, : W // 2 + 3] = 255
    o = R.fill(FIELD, v, R.Params(levels=levels, grid_x=7, grid_y=5), LUT, dom)
    src, s = o["source"], o["sums"]
    classes = [src == 0, src == R.HELD, (src >= 1) & (src <= 7), src == R.UNFILLED, src == R.OUTSIDE]
    assert sum(c.astype(int) for c in classes).min() == 1 and sum(c.astype(int) for c in classes).max() == 1
    assert [int(c.sum()) for c in classes] == [int(x) for x in o["summary"][:5]] == [int(x) for x in s[:, :5].sum(0)]
    assert s[:, :5].sum(1).tolist() == o["cells"]["pixels"].tolist() and o["cells"]["pixels"].sum() == W * H
    assert o["summary"][8:].sum() == o["summary"][2] and o["summary"][8] == 0 and (o["summary"][6:8] == 0).all()
    assert s[:, 7].sum() == sum(k * int(o["summary"][8 + k]) for k in range(8))
    assert ((o["mask"] == 255) == (src <= R.HELD)).all() and (src[(v != 0)] == 0).all()       # KNOWN outside the domain passes through
    assert (src[(v == 0) & (dom == 0)] == R.OUTSIDE).all() and (o["filled"].view(np.uint32)[src == R.OUTSIDE] == R.NAN_BITS).all()
    val = src <= R.HELD
    assert s[:, 5].sum() == o["sides"]["Fx"][val].sum() and s[:, 6].sum() == o["sides"]["Fy"][val].sum()


@pytest.mark.parametrize("hold", [1, 3, 254])
def test_a_pixel_known_once_is_held_for_exactly_hold_pushes(hold):
    w, h = 9, 7
    ref = R.InfillRef(w, h, R.Params(levels=1, hold=hold), LUT)
    f = np.full((h, w, 2), np.nan, np.float32)
    g = f.copy()
    g[3, 4] = (2.5, -1.0)
    o = ref.push(g)
    assert o["source"][3, 4] == 0
    for t in range(min(hold, 5)):
        o = ref.push(f)
        assert o["source"][3, 4] == R.HELD and (o["filled"][3, 4] == np.float32([2.5, -1.0])).all() and o["summary"][1] == 1
    if hold <= 5:
        o = ref.push(f)
        assert o["source"][3, 4] == R.UNFILLED and o["summary"][1] == 0 and ref.age[3, 4] == 255
    ref.reset()
    assert (ref.age == 255).all() and ref.pushes == 0 and not ref.summary.any()
    assert ref.push(f)["summary"][[1, 5]].tolist() == [0, 1]


def test_hold_zero_holds_nothing_and_held_pixels_feed_the_pyramid():
    w, h = 9, 7
    f = np.full((h, w, 2), np.nan, np.float32)
    g = f.copy()
    g[3, 4] = (2.5, -1.0)
    none = R.InfillRef(w, h, R.Params(levels=7, hold=0), LUT)
    none.push(g)
    assert (none.push(f)["source"] == R.UNFILLED).all()
    some = R.InfillRef(w, h, R.Params(levels=7, hold=2), LUT)
    some.push(g)
    o = some.push(f)
    assert o["summary"][1] == 1 and o["summary"][2] == w * h - 1 and (o["filled"] == np.float32([2.5, -1.0])).all()


def test_rdiv_rounds_halves_up_and_floors_negative_numerators():
    a = np.array([-7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7])
    assert R.rdiv(a, 4).tolist() == [-2, -1, -1, -1, -1, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2]        # -6 / 4 = -1.5 -> -1, 6 / 4 -> 2
    assert R.rdiv(a, 1).tolist() == a.tolist() and R.rdiv(np.array([-3, 3]), 2).tolist() == [-1, 2]


def test_sizes_shrink_to_one_and_stay():
    assert R.sizes(129, 65, 7) == [(129, 65), (65, 33), (33, 17), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1)]
    assert R.sizes(5, 3, 7)[3:] == [(1, 1)] * 5 and R.sizes(1, 1, 7) == [(1, 1)] * 8


def test_results_do_not_depend_on_min_known_where_everything_is_known():
    for mk in (1, 4, 16384):
        o = R.fill(FIELD, None, R.Params(levels=7, min_known=mk), LUT)
        assert np.array_equal(o["filled"].view(np.uint32), FIELD.view(np.uint32)) and o["summary"][0] == W * H


# ---------------------------------------------------------------------------- the prototype's figures
@pytest.mark.parametrize("pat,levels,holes,unfilled,se2,me2,by_lev", [
    ("p300", 7, 5796, 0, 6137, 29, [5169, 537, 90]),
    ("p900", 2, 17265, 4, 173761, 1413, [190, 17071]),
    ("p900", 7, 17265, 0, 90814, 117, [190, 6039, 11036]),
    ("block40", 2, 1600, 1156, 106030, 1066, [0, 444]),
    ("block40", 7, 1600, 0, 1580144, 2896, [0, 0, 0, 0, 1600]),
])
def test_prototype_figures(pat, levels, holes, unfilled, se2, me2, by_lev):
    hole, o = filled(pat, levels)
    e = R.errors(o, hole)
    assert (int(hole.sum()), int(o["summary"][3]), int(e.sum()), int(e.max())) == (holes, unfilled, se2, me2)
    assert o["summary"][9:].tolist() == by_lev + [0] * (7 - len(by_lev))


def test_prototype_figures_by_min_known():
    got = [int(R.errors(filled("p900", 7, mk)[1], filled("p900", 7, mk)[0]).sum()) for mk in (1, 2, 4, 8)]
    assert got == [90814, 132659, 311618, 951150]


def test_prototype_rms_against_zero_fill():
    """zero fill, what RC_FLOWCHECK_FILL_ZERO amounts to, against the infill over the holes of p300, and a big hole: a mean of the
    surroundings, not an extrapolation"""
    hole, o = filled("p300", 7)
    s = o["sides"]
    zero = np.sqrt(((s["qx"] ** 2 + s["qy"] ** 2)[hole]).mean()) / 64
    rms = np.sqrt(R.errors(o, hole).mean()) / 64
    assert round(zero, 2) == 2.02 and round(rms, 3) == 0.016
    hole, o = filled("block40", 7)
    assert round(np.sqrt(R.errors(o, hole).mean()) / 64, 2) == 0.49 and (o["source"][hole] == 5).all()
