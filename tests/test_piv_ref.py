"""The numpy statement of the ensemble PIV (tests/_piv_ref.py) against what it must mean: the ring update is a rescan of the
last pairs, the integer sums do not depend on the order they are taken in, no sum leaves its word at the extremes, a known
shift comes back, noise and constant frames are refused, ties go to the first in scan order, the median test finds the one
spike, and no input of either tier sits on a decision the device's last-place allowance could turn; and the library exports
the entry points."""
import math

import numpy as np

import _piv_ref as R
# the statement's flags and bounds are the library's: without the product this file does not import
from ripcurrents_amd._lib import (RC_PIV_EDGE, RC_PIV_EMPTY, RC_PIV_FLAT, RC_PIV_LAUNCHES, RC_PIV_LOWPEAK, RC_PIV_MAX_ENSEMBLE,
                                  RC_PIV_MAX_PIXEL_PAIRS, RC_PIV_MAX_RANGE, RC_PIV_MAX_STATE_BYTES, RC_PIV_MAX_WINDOW, RC_PIV_OUTLIER,
                                  RC_PIV_REPLACE)

_CACHE = {}


def results():
    """every case's computing pushes, computed once for the whole file"""
    if not _CACHE:
        lut = np.stack([np.arange(256)] * 3, 1).astype(np.uint8)  # any table of 256 distinct colours: the doubtful share is about indices
        for name, case in R.cases().items():
            _CACHE[name] = (case,) + R.run_case(case, lut)
    return _CACHE


# ---------------------------------------------------------------------------- the sums
def test_ring_update_equals_a_rescan_at_every_push():
    """an ensemble of 3 over 7 pushes: fewer pairs than the ensemble, exactly as many, and the ring wrapped twice"""
    w, h = 40, 36
    p = R.Params(8, 2, 6, ensemble=3)
    ref = R.PivRef(w, h, p)
    for t, f in enumerate(R.noise_frames(w, h, 7, 31), 1):
        ref.push(f, compute=False)
        T, Ta, Taa = ref.rescan()
        assert ref.n == min(t - 1, 3) == len(ref.history)
        assert np.array_equal(ref.T, T) and np.array_equal(ref.Ta, Ta) and np.array_equal(ref.Taa, Taa), t
    assert ref.pairs == 6 and ref.n == 3
    for name, (case, ref, _) in results().items():               # and at the end of every case of both tiers
        T, Ta, Taa = ref.rescan()
        assert np.array_equal(ref.T, T) and np.array_equal(ref.Ta, Ta) and np.array_equal(ref.Taa, Taa), name


def test_sums_do_not_depend_on_summation_order():
    """the statement's window sums against a plain loop over the pixels of each window, taken last pixel first, and against the
    same sums with both frames mirrored"""
    w, h = 31, 27
    p = R.Params(8, 2, 5)
    gx, gy = R.grid(w, h, p)
    a, b = R.noise_frames(w, h, 2, 32)
    S, Sa, Saa = R.pair_sums(a, b, p, gx, gy)
    M, Rr = p.window, p.range
    for cy in range(gy):
        for cx in range(gx):
            x0, y0 = Rr + cx * p.step, Rr + cy * p.step
            sa = sum(int(a[y, x]) for y in reversed(range(y0, y0 + M)) for x in reversed(range(x0, x0 + M)))
            assert sa == Sa[cy, cx] and sum(int(a[y, x]) ** 2 for y in range(y0, y0 + M) for x in range(x0, x0 + M)) == Saa[cy, cx]
            for j, i in ((-2, -2), (0, 1), (2, -1), (2, 2)):
                t = [0, 0, 0]
                for y in reversed(range(M)):
                    for x in reversed(range(M)):
                        va, vb = int(a[y0 + y, x0 + x]), int(b[y0 + j + y, x0 + i + x])
                        t[0] += va * vb; t[1] += vb; t[2] += vb * vb
                assert t == [int(v) for v in S[cy, cx, j + Rr, i + Rr]], (cx, cy, j, i)
    # both frames mirrored, cut to the width the cells cover so that the grid mirrors onto itself: displacements and cells mirror
    w2 = Rr * 2 + M + (gx - 1) * p.step
    S2, Sa2, _ = R.pair_sums(a[:, :w2][:, ::-1], b[:, :w2][:, ::-1], p, gx, gy)
    assert np.array_equal(S2, S[:, ::-1, :, ::-1]) and np.array_equal(Sa2, Sa[:, ::-1])


def test_no_sum_leaves_its_word_at_the_extremes():
    """M = 64 and E = 64 (E M^2 = 2^18): all-255 frames give the largest sums there are, random 0 / 255 frames the largest
    variances; a per-pair sum stays below 2^31 and every term of the score below 2^53"""
    p = R.Params(64, 1, 64, ensemble=64)
    assert R.params_ok(p) and not R.params_ok(R.Params(64, 1, 64, ensemble=65))
    w = h = 66
    full = np.full((h, w), 255, np.uint8)
    S, Sa, Saa = R.pair_sums(full, full, p, 1, 1)
    assert S.max() == Saa.max() == 255 * 255 * 4096 < 2 ** 31 and Sa.max() == 255 * 4096
    n, N = 64, 64 * 4096
    T, Ta, Taa = n * S, n * Sa, n * Saa
    assert (N * T[..., 0]).max() == (Ta * Ta).max() == (255 * 2 ** 18) ** 2 < 2 ** 53
    s, va = R.scores(T, Ta, Taa, n, 64)                           # asserts every term below 2^53 itself
    assert not s.any() and not va.any()
    a, b = R.binary_frames(w, h, 2, 33)
    S, Sa, Saa = R.pair_sums(a, b, p, 1, 1)
    assert max(S.max(), Saa.max()) < 2 ** 31
    s, va = R.scores(n * S, n * Sa, n * Saa, n, 64)
    assert 0 < va.max() < 2 ** 53 and np.abs(s).max() < 0.01
    # and through a session: 65 pushes of one 0 / 255 pair alternating
    ref = R.PivRef(w, h, R.Params(64, 1, 64, ensemble=64))
    for t in range(66):
        ref.push(a if t % 2 else b, compute=False)
    assert ref.n == 64 and ref.T.max() < 2 ** 31 * 64
    R.scores(ref.T, ref.Ta, ref.Taa, ref.n, 64)


# ---------------------------------------------------------------------------- what comes back
def test_translation_recovery():
    """synth.translating_clip(160, 120).  Measured with this statement: shift (1.25, -0.75), M 16, R 4, step 16, 63 cells: largest
    error 0.2214 / 0.2089 px in x / y, mean (1.2430, -0.7739), no EDGE cell; shift (5.25, -3.75), M 32, R 8, step 32, 12 cells:
    0.0715 / 0.1182 px, mean (5.2562, -3.7529).  The bounds are 1.5 times those: 0.3321 / 0.3134 and 0.1073 / 0.1773 px."""
    for name, cells in (("translating", 63), ("translating-far", 12)):
        case, ref, outs = results()[name]
        (u, v), (bx, by) = R.RECOVERY[name]
        rec = outs[-1][1]["records"]
        ex, ey = np.abs(rec["dx"] - u).max(), np.abs(rec["dy"] - v).max()
        print("%s: max abs error %.4f / %.4f px, mean (%.4f, %.4f)" % (name, ex, ey, rec["dx"].mean(), rec["dy"].mean()))
        assert rec.size == cells and not rec["flags"].any()
        assert ex <= bx and ey <= by
        assert abs(rec["dx"].mean() - u) <= 0.05 and abs(rec["dy"].mean() - v) <= 0.05
        assert (rec["ix"] == round(u)).all() or name == "translating"
        # swapping the two frames negates the result
        back = R.run_case(R.translating(u, v, case.p, swap=True))[1][-1][1]["records"]
        assert np.abs(back["dx"] + u).max() <= bx and np.abs(back["dy"] + v).max() <= by
        assert abs(back["dx"].mean() + u) <= 0.05 and abs(back["dy"].mean() + v) <= 0.05


def test_noise_is_lowpeak_everywhere():
    """two independent uniform-noise frames: the largest peak is some 0.05, far below min_peak = 0.25"""
    w, h = 160, 120
    p = R.Params(16, 4, 16, min_peak=0.25)
    ref = R.PivRef(w, h, p)
    a, b = R.noise_frames(w, h, 2, 34)
    ref.push(a)
    out = ref.push(b)
    rec = out["records"]
    print("largest peak over noise: %.4f" % rec["peak"].max())
    assert (rec["flags"] & R.LOWPEAK).all() and rec["peak"].max() < 0.1 and out["summary"][2] == 0 and not out["field"].any()
    for _, o, _ in results()["noise"][2]:
        assert (o["records"]["flags"] & R.LOWPEAK).all()


def test_constant_frames_are_flat():
    p = R.Params(8, 2, 4)
    ref = R.PivRef(30, 26, p)
    ref.push(np.full((26, 30), 77, np.uint8))
    out = ref.push(np.full((26, 30), 200, np.uint8))
    rec = out["records"]
    assert (rec["flags"] == R.FLAT).all() and not rec["dx"].any() and not rec["ix"].any() and out["summary"][3] == rec.size
    # a constant template over a textured frame is FLAT too (va = 0); a textured template over a constant frame has every s = 0
    ref.reset()
    ref.push(np.full((26, 30), 77, np.uint8))
    assert (ref.push(R.noise_frames(30, 26, 1, 35)[0])["records"]["flags"] == R.FLAT).all()
    assert (ref.push(np.full((26, 30), 9, np.uint8))["records"]["flags"] == R.FLAT).all()
    for t, o, _ in results()["extreme"][2][:3]:
        assert (o["records"]["flags"] == R.FLAT).all()


def test_first_push_is_empty():
    ref = R.PivRef(30, 26, R.Params(8, 2, 4, ensemble=2))
    out = ref.push(R.noise_frames(30, 26, 1, 36)[0])
    assert (out["records"]["flags"] == R.EMPTY).all() and list(out["summary"]) == [0, out["records"].size, 0, 0, 0, 0, 0, 1]


def test_ties_go_to_the_first_in_scan_order():
    """a pattern of period 4 px in x under R = 4: the displacements -4, 0 and +4 score the same, bit for bit, and the first wins"""
    w, h = 40, 30
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = (np.array([10, 200, 90, 30])[x % 4] + 7 * (y % 5)).astype(np.uint8)
    ref = R.PivRef(w, h, R.Params(8, 4, 8))
    ref.push(f)
    out = ref.push(f)
    s, rec = out["scores"], out["records"]
    assert (s[:, :, 4, 0] == s[:, :, 4, 4]).all() and (s[:, :, 4, 4] == s[:, :, 4, 8]).all() and (s[:, :, 4, 4] == s.max((2, 3))).all()
    assert (rec["ix"] == -4).all() and (rec["flags"] & R.EDGE).all()
    # the rows repeat after 5, beyond the range: iy is the only 0
    assert (rec["iy"] == 0).all()


def test_median_test_finds_the_one_spike():
    rec = np.zeros((5, 5), R.CELL_DTYPE)
    rng = np.random.default_rng(37)
    rec["dx"] = (1.0 + 0.05 * rng.standard_normal((5, 5))).astype(np.float32)
    rec["dy"] = (-0.5 + 0.05 * rng.standard_normal((5, 5))).astype(np.float32)
    rec["pairs"] = 1
    rec["dx"][2, 2] = 3.0
    # two corners with fewer than three valid neighbours
    rec["flags"][0, 1] = rec["flags"][1, 0] = R.LOWPEAK
    rec["flags"][4, 3] = R.FLAT
    rec["flags"][3, 4] = R.LOWPEAK | R.EDGE
    rec["dx"][0, 0] = -9.0
    p = R.Params(8, 2, 4, median_eps=0.1, median_thr=2.0)
    out, field = R.median_test(rec, p)
    spike = np.zeros((5, 5), bool)
    spike[2, 2] = True
    assert np.array_equal((out["flags"] & R.OUTLIER) != 0, spike) and out["resid"][2, 2] > 10
    assert out["resid"][0, 0] == 0 and out["resid"][4, 4] == 0 and out["flags"][0, 0] == 0      # untested: one and two candidates
    assert out["resid"][0, 1] == 0 and not field[0, 1].any() and not field[4, 3].any()            # invalid cells: no residual, no field
    assert field[2, 2, 0] == np.float32(3.0) and field[0, 0, 0] == np.float32(-9.0)
    p.flags = R.REPLACE
    out2, field2 = R.median_test(rec, p)
    nb = sorted(float(rec["dx"][y, x]) for y in (1, 2, 3) for x in (1, 2, 3) if (y, x) != (2, 2))
    assert field2[2, 2, 0] == (np.float32(nb[3]) + np.float32(nb[4])) * np.float32(0.5) and np.array_equal(out2, out)
    keep = ~spike
    assert np.array_equal(field2[keep], field[keep])
    # an odd count takes the middle one
    assert R._median([np.float32(v) for v in (3, 1, 2)]) == 2 and R._median([np.float32(v) for v in (4, 1, 2, 3)]) == np.float32(2.5)


def test_sub_pixel_step():
    assert R._offset(0.25, 1.0, 0.25) == 0.0 and R._offset(1.0, 1.0, 1.0) == 0.0
    assert R._offset(0.81, 1.0, 0.49) == (0.9 - 0.7) / (2.0 * ((0.9 - 1.0) + (0.7 - 1.0)))
    assert -0.5 <= R._offset(1.0, 1.0, 0.0) <= 0.5 and R._offset(-0.04, 0.0, -0.04) == 0.0
    assert R._root(-0.25) == -0.5 and math.copysign(1.0, R._root(-0.0)) == -1.0


# ---------------------------------------------------------------------------- conditions on the inputs of the device tier
def test_no_case_sits_on_a_decision():
    """no cell of any case has its peak within one unit in the last place of min_peak or its residual that near median_thr, and
    less than 1 % of any picture changes its colour index under one unit in the last place of dx, dy or the magnitude"""
    kinds = 0
    for name, (case, ref, outs) in results().items():
        for t, o, p in outs:
            assert not R.flag_exceptions(o, p).any(), (name, t)
            share = R.doubtful_share(o, case.w, case.h, p).mean()
            assert share < 0.01, (name, t, share)
            kinds |= int(np.bitwise_or.reduce(o["records"]["flags"].ravel()))
    assert kinds == R.EMPTY | R.FLAT | R.EDGE | R.LOWPEAK | R.OUTLIER          # every flag occurs in the device tier


def test_cases_cover_what_they_claim():
    c = R.cases()
    assert c["ragged"].w % 4 and c["ragged"].p.step < c["ragged"].p.window and c["ragged"].pad == 5
    assert (len(c["ring"].frames) - 1) // c["ring"].p.ensemble == 2
    e = c["extreme"]
    assert e.w == e.p.window + 2 * e.p.range and R.grid(e.w, e.h, e.p) == (1, 1) and (e.frames[0] == 255).all()
    assert R.grid(160, 120, c["translating"].p) == (9, 7)
    assert R.grid(1920, 1080, R.Params(32, 8, 16)) == (118, 65)
    assert R.grid(23, 40, R.Params(16, 4, 16)) is None


def test_library_exports_the_entry_points():
    import ctypes as C
    import os
    from ripcurrents_amd import _lib
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ripcurrents_amd", "librcflow.so")
    lib = C.CDLL(so)
    for name in ("open", "push_dev", "read", "sums_read", "set", "reset", "close", "info"):
        assert hasattr(lib, "rcflow_piv_" + name) and "rcflow_piv_" + name in _lib.SIGNATURES
    assert C.sizeof(_lib.PivParams) == 56 and C.sizeof(_lib.PivInfo) == 96
    from ripcurrents_amd.api import PIV_CELL_DTYPE, PIV_SUMMARY, Piv
    assert PIV_CELL_DTYPE == R.CELL_DTYPE and PIV_CELL_DTYPE.itemsize == 32 and len(PIV_SUMMARY) == 8 and Piv
    assert (RC_PIV_EMPTY, RC_PIV_FLAT, RC_PIV_EDGE, RC_PIV_LOWPEAK, RC_PIV_OUTLIER, RC_PIV_REPLACE) == (R.EMPTY, R.FLAT, R.EDGE, R.LOWPEAK, R.OUTLIER,
                                                                                                        R.REPLACE)
    assert RC_PIV_MAX_STATE_BYTES == R.MAX_STATE_BYTES and RC_PIV_LAUNCHES == R.LAUNCHES
    # the statement's parameter check ends where the library's bounds are
    ok = lambda **kw: R.params_ok(R.Params(**dict(dict(window=16, range=4, step=16), **kw)))
    assert ok(window=RC_PIV_MAX_WINDOW, ensemble=RC_PIV_MAX_PIXEL_PAIRS // RC_PIV_MAX_WINDOW ** 2) and not ok(window=RC_PIV_MAX_WINDOW + 4)
    assert not ok(window=RC_PIV_MAX_WINDOW, ensemble=RC_PIV_MAX_PIXEL_PAIRS // RC_PIV_MAX_WINDOW ** 2 + 1)
    assert ok(range=RC_PIV_MAX_RANGE) and not ok(range=RC_PIV_MAX_RANGE + 1)
    assert ok(window=8, step=8, ensemble=RC_PIV_MAX_ENSEMBLE) and not ok(window=8, step=8, ensemble=RC_PIV_MAX_ENSEMBLE + 1)
