"""The numpy statement of the flow kinematics (tests/_kinematics_ref.py) against what is known without it: the taps of the C side,
the record layouts, analytic fields, and the conditions that make the GPU tier's inputs worth testing on."""
import ctypes as C
import math

import numpy as np
import pytest

import _kinematics_ref as K
import _regions_ref as R
from ripcurrents_amd import _lib, synth
from ripcurrents_amd.api import KINEMATICS_CELL_DTYPE, KINEMATICS_SUMS, kinematics_taps

f32 = np.float32
LUT = np.zeros((256, 3), np.uint8)          # the colours are not this tier's subject


@pytest.mark.parametrize("sigma", [0.5, 1.5, 4.0])
@pytest.mark.parametrize("radius", [0, 1, 3, 8])
def test_taps_of_the_library_are_the_statements(radius, sigma):
    got, want = kinematics_taps(radius, sigma), K.taps(radius, sigma)
    assert got.dtype == f32 and got.shape == (radius + 1,)
    assert got.tobytes() == want.tobytes()
    assert abs(float(want[0]) + 2 * float(want[1:].sum()) - 1.0) < 1e-6 and (np.diff(want) <= 0).all()


def test_taps_refusals():
    lib = _lib.load()
    buf = (C.c_float * 16)()
    for radius, sigma in ((-1, 1.0), (K.MAX_RADIUS + 1, 1.0), (1, 0.0), (1, -1.0), (3, float("nan")), (3, float("inf")), (8, float("-inf"))):
        assert lib.rcflow_kinematics_taps(radius, sigma, buf) == -1, (radius, sigma)
    assert lib.rcflow_kinematics_taps(2, 1.0, None) == -1
    assert lib.rcflow_kinematics_taps(0, float("nan"), buf) == 0 and buf[0] == 1.0       # sigma is ignored without smoothing


def test_record_layouts():
    assert C.sizeof(_lib.KinematicsCell) == K.CELL.itemsize == KINEMATICS_CELL_DTYPE.itemsize == 48
    assert K.CELL == KINEMATICS_CELL_DTYPE
    for name, _ in _lib.KinematicsCell._fields_:
        assert getattr(_lib.KinematicsCell, name).offset == K.CELL.fields[name][1], name
    assert C.sizeof(_lib.KinematicsParams) == 88 and _lib.KinematicsParams.sigma.offset == 32
    assert C.sizeof(_lib.KinematicsInfo) == 120 and _lib.KinematicsInfo.prm.offset == 8
    assert len(KINEMATICS_SUMS) == K.SUMS == _lib.RC_KINEMATICS_SUMS and KINEMATICS_SUMS == K.SUM_NAMES


@pytest.mark.parametrize("radius,sigma,spacing", [(0, 1.0, 1), (2, 1.5, 1), (3, 2.0, 2), (8, 3.0, 8)])
def test_rotation_field(radius, sigma, spacing):
    """the field is linear, so smoothing changes nothing: omega = 100 / w + 100 / h and ow = -4 (100 / w)(100 / h) everywhere.  The
    error is a few ulp of values up to 50, divided by 2 s"""
    w, h = 64, 48
    out = K.kinematics(synth.rotation_field(w, h), LUT, K.params(radius, sigma, spacing, 2, 2))
    v = out["valid"]
    m = radius + spacing
    assert v.sum() == (w - 2 * m) * (h - 2 * m) and not out["bad"].any()
    print("omega off by %.3g, ow by %.3g, |div| up to %.3g" % (np.abs(out["omega"][v] - (100 / w + 100 / h)).max(),
                                                              np.abs(out["ow"][v] + 4 * (100 / w) * (100 / h)).max(), np.abs(out["div"][v]).max()))
    assert np.abs(out["omega"][v] - (100 / w + 100 / h)).max() <= 2e-5
    assert np.abs(out["ow"][v] + 4 * (100 / w) * (100 / h)).max() <= 2e-4
    assert np.abs(out["div"][v]).max() <= 1e-5
    assert not out["omega"][~v].any() and not out["ow"][~v].any() and not out["div"][~v].any()
    # every valid pixel turns clockwise and is a core; the cells' sums are the pixels'
    assert out["summary"][0] == v.sum() and out["summary"][2] == v.sum() and out["summary"][3] == 0
    assert out["sums"][:, 0].sum() == v.sum() and (out["cells"]["flags"] == K.CW).all()
    assert np.allclose(out["cells"]["mean_vorticity"], 100 / w + 100 / h, atol=2e-5)
    assert np.allclose(out["cells"]["circulation"], out["cells"]["n"] * (100 / w + 100 / h), rtol=1e-5)


def test_surf_field_has_shear_layers_of_both_signs():
    """the jet runs up the picture along x = 0.55 w: the vorticity of its flanks has opposite signs"""
    w, h = 96, 64
    out = K.kinematics(K.surf(w, h), LUT, K.params(2, 1.5, 1, 4, 3, ow_k=0.2))
    cw, ccw = out["core"] & (out["omega"] > 0), out["core"] & (out["omega"] < 0)
    print("cores: %d clockwise, %d counter-clockwise" % (cw.sum(), ccw.sum()))
    assert cw.sum() >= 100 and ccw.sum() >= 100
    xs_cw, xs_ccw = np.nonzero(cw)[1], np.nonzero(ccw)[1]
    axis = 0.55 * w
    assert (xs_cw > axis).all() != (xs_ccw > axis).all() and ((xs_cw > axis).all() or (xs_cw < axis).all())
    assert (xs_ccw > axis).all() or (xs_ccw < axis).all()
    assert out["summary"][2] == cw.sum() and out["summary"][3] == ccw.sum()


@pytest.mark.parametrize("prm", [K.params(2, 1.0, 1, 4, 2, ow_k=0.2), K.pair_params()], ids=["relative", "absolute"])
def test_lamb_oseen_pair_gives_two_cores(prm):
    w, h = 96, 64
    f = K.lamb_oseen_pair(w, h)
    assert np.array_equal(f[:, ::-1, 0], -f[..., 0]) and np.array_equal(f[:, ::-1, 1], f[..., 1]), "the pair is mirror symmetric"
    out = K.kinematics(f, LUT, prm)
    cw, ccw = out["core"] & (out["omega"] > 0), out["core"] & (out["omega"] < 0)
    print("cores: %d clockwise, %d counter-clockwise" % (cw.sum(), ccw.sum()))
    assert cw.sum() == ccw.sum() > 50 and np.array_equal(cw[:, ::-1], ccw)
    assert cw[:, :w // 2].sum() == cw.sum(), "the positive vortex is the left one"
    reg = R.regions(out["mask"], connectivity=8)
    assert reg["K"] == 2
    both = (out["cells"]["flags"] & (K.CW | K.CCW)) == (K.CW | K.CCW)
    assert out["summary"][5] == both.sum()
    # the circulation of the left half is close to +Gamma (times scale and pixel area), of the right half to -Gamma
    circ = out["cells"]["circulation"].reshape(prm["grid_y"], prm["grid_x"])
    unit = K.PAIR_GAMMA * prm["scale"] * prm["pixel_area"]
    left, right = circ[:, :prm["grid_x"] // 2].sum(), circ[:, prm["grid_x"] // 2:].sum()
    print("circulation: %.3f left, %.3f right, of %.3f" % (left, right, unit))
    assert 0.5 * unit < left < 1.05 * unit and abs(left + right) < 1e-3 * unit


def test_poisoned_field_is_counted_and_part_of_nothing():
    f = K.poisoned(96, 64)
    out = K.kinematics(f, LUT, K.params(2, 1.5, 1, 4, 3, ow_k=0.2))
    assert out["bad"].sum() > 50 and out["summary"][1] == out["bad"].sum()
    for k in ("omega", "div", "ow"):
        assert np.isfinite(out[k]).all() and not out[k][out["bad"]].any()
    assert not out["mask"][out["bad"]].any() and not out["vis"][out["bad"]].any()
    assert math.isfinite(out["T2"]) and np.isfinite(out["cells"]["mean_ow"]).all()
    assert out["summary"][2] > 0 and out["summary"][3] > 0


def test_cases_cover_the_paths():
    """the conditions the GPU tier's cases are chosen for"""
    c = K.cases()
    f, p = c["one_interior_pixel"]
    assert f.shape[0] == f.shape[1] == 2 * (p["radius"] + p["spacing"]) + 1
    f, p = c["no_smoothing"]
    out = K.kinematics(f, LUT, p)
    assert (out["cells"]["flags"].reshape(29, 37)[0] == K.EMPTY).all() and (out["cells"]["n"].reshape(29, 37)[1:-1, 1:-1] == 1).all()
    for name in ("sliver_column", "sliver_row"):
        f, p = c[name]
        assert min(f.shape[:2]) == 2 * (p["radius"] + p["spacing"]) + 1
    for name, (f, p) in c.items():
        out = K.kinematics(f, LUT, p)
        assert out["summary"][0] > 0, name
        if name not in ("one_interior_pixel",):
            assert out["summary"][2] + out["summary"][3] > 0, name
