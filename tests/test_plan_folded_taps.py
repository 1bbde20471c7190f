"""CPU test of the derived taps of the fast expansion (RcPolyK::qh, xga, xgb, kdch in ripcurrents_amd/csrc/rc_plan.cpp,
DESIGN.md section 4): each equals its double formula over the plan's own g, xg, xxg and ig to 1 ulp of float, the taps
beyond n_eff are zero, and the constants the exact expansion and tests/test_plan_host.py read are untouched by them."""
import ctypes as C

import numpy as np
import pytest

CASES = [(15, 1.2), (5, 1.1), (7, 1.5)]


def _lib():
    import ripcurrents_amd
    lib = ripcurrents_amd.load()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    lib.rcflow_debug_plan_poly.argtypes = [C.c_int, C.c_double, C.c_int, fp, fp, fp, dp, C.POINTER(C.c_int), dp]
    lib.rcflow_debug_plan_poly.restype = C.c_int
    lib.rcflow_debug_plan_poly_folded.argtypes = [C.c_int, C.c_double, C.c_int, fp, fp, fp, dp]
    lib.rcflow_debug_plan_poly_folded.restype = C.c_int
    return lib


def _plan(lib, n, sigma, exact_taps):
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    g, xg, xxg, qh, xga, xgb = (np.full(n + 1, np.nan, np.float32) for _ in range(6))
    ig = np.full(4, np.nan, np.float64)
    n_eff, kdc, kdch = C.c_int(-1), C.c_double(np.nan), C.c_double(np.nan)
    assert lib.rcflow_debug_plan_poly(n, sigma, exact_taps, g.ctypes.data_as(fp), xg.ctypes.data_as(fp), xxg.ctypes.data_as(fp),
                                      ig.ctypes.data_as(dp), C.byref(n_eff), C.byref(kdc)) == 0
    assert lib.rcflow_debug_plan_poly_folded(n, sigma, exact_taps, qh.ctypes.data_as(fp), xga.ctypes.data_as(fp),
                                             xgb.ctypes.data_as(fp), C.byref(kdch)) == 0
    return g, xg, xxg, ig, n_eff.value, kdc.value, qh, xga, xgb, kdch.value


def _within_one_ulp(got, want64):
    """got (float32) against the double value: at most one float32 step from the nearest float32"""
    near = want64.astype(np.float32)
    step = np.maximum(np.abs(np.spacing(near)), np.float32(2.0) ** -149)
    return np.all(np.abs(got.astype(np.float64) - near.astype(np.float64)) <= step.astype(np.float64))


@pytest.mark.parametrize("n,sigma", CASES)
@pytest.mark.parametrize("exact_taps", [0, 1])
def test_derived_taps_match_their_double_formulas(n, sigma, exact_taps):
    lib = _lib()
    g, xg, xxg, ig, n_eff, kdc, qh, xga, xgb, kdch = _plan(lib, n, sigma, exact_taps)
    ig11, ig03, ig33, ig55 = ig
    k = n_eff + 1
    assert n_eff == (n if exact_taps else {(15, 1.2): 7, (5, 1.1): 5, (7, 1.5): 7}[(n, sigma)])
    g64, xg64, xxg64 = g[:k].astype(np.float64), xg[:k].astype(np.float64), xxg[:k].astype(np.float64)
    assert _within_one_ulp(qh[:k], 0.5 * (ig03 * g64 + ig33 * xxg64))
    assert _within_one_ulp(xga[:k], xg64 * (ig11 * 0.5))
    assert _within_one_ulp(xgb[:k], xg64 * ((ig55 * 0.25) / (ig11 * 0.5)))
    assert kdch == 0.5 * kdc
    assert not qh[k:].any() and not xga[k:].any() and not xgb[k:].any()
    # the odd taps have no centre; the even one does (ig03 g[0] / 2: xxg[0] is zero)
    assert xga[0] == 0 and xgb[0] == 0 and qh[0] != 0
    # the products the kernels used to form per pixel, now inside the taps: xgb applied to an xga-filtered plane is
    # xg (x) xg ig55 / 4 to two float roundings
    assert np.allclose(np.outer(xgb[:k].astype(np.float64), xga[:k].astype(np.float64)), np.outer(xg64, xg64) * ig55 * 0.25,
                       rtol=3e-7, atol=0)


def test_folded_entry_point_checks_its_arguments():
    lib = _lib()
    fp = C.POINTER(C.c_float)
    a = np.zeros(34, np.float32)
    kd = C.c_double()
    p = a.ctypes.data_as(fp)
    assert lib.rcflow_debug_plan_poly_folded(0, 1.2, 0, p, p, p, C.byref(kd)) == -1
    assert lib.rcflow_debug_plan_poly_folded(33, 1.2, 0, p, p, p, C.byref(kd)) == -1
    assert lib.rcflow_debug_plan_poly_folded(15, 1.2, 0, None, p, p, C.byref(kd)) == -1
