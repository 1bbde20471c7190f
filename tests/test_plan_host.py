"""CPU tests of the Farneback plan (ripcurrents_amd/csrc/rc_plan.cpp) and of the profile-kind table (csrc/rc_host.h), through
diagnostic entry points of librcflow.so that need no context and no GPU: the constants the kernels are handed are upstream's
bit for bit, so a flow that departs from the oracle departs in a kernel."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY_N = (1, 2, 3, 5, 7, 15, 20, 32)
POLY_SIGMA = (0, 0.5, 1.1, 1.2, 1.5, 4.0, 7.3)
PYR_KSIZE = (1, 3, 5, 7, 9, 11, 21, 41)
PYR_SIGMA = (0, 0.5, 1.5, 3.5)

# kKindNames, kBucketOfKind and kBucketNames of the commit before the three lists became one table, by id
KINDS = [("pyr_level", "farneback"), ("polyexp", "farneback"), ("flow_iter", "farneback"), ("polar_hist", "threshold"),
         ("thresholds", "threshold"), ("classify_accumulate", "threshold"), ("advect_field", "stream"), ("advect_points", "stream"),
         ("flow_postop", "farneback"), ("flow_color", "threshold"), ("flow_iter_x2", "farneback"), ("frame_preproc", "farneback"),
         ("create_edges", "erosion"), ("streamline_display", "stream"), ("hsv_to_bgr", "threshold"), ("create_output", "overlay"),
         ("flow_area_init", "farneback"), ("timex", "overlay"), ("frame_color", "overlay"), ("framestab", "farneback"),
         ("ripmap", "farneback"), ("trackstab", "farneback"), ("tracers", "stream"), ("regions", "threshold"), ("tracks", "threshold")]


def _lib():
    import ripcurrents_amd
    lib = ripcurrents_amd.load()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    lib.rcflow_debug_plan_poly.argtypes = [C.c_int, C.c_double, C.c_int, fp, fp, fp, dp, C.POINTER(C.c_int), dp]
    lib.rcflow_debug_plan_poly.restype = C.c_int
    lib.rcflow_debug_plan_pyr_kernel.argtypes = [C.c_int, C.c_double, fp]
    lib.rcflow_debug_plan_pyr_kernel.restype = C.c_int
    lib.rcflow_debug_kind.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    lib.rcflow_debug_kind.restype = C.c_int
    return lib


def _poly(lib, n, sigma, exact_taps):
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    g, xg, xxg = (np.full(n + 1, np.nan, np.float32) for _ in range(3))
    ig = np.full(4, np.nan, np.float64)
    n_eff, kdc = C.c_int(-1), C.c_double(np.nan)
    rc = lib.rcflow_debug_plan_poly(n, sigma, exact_taps, g.ctypes.data_as(fp), xg.ctypes.data_as(fp), xxg.ctypes.data_as(fp),
                                    ig.ctypes.data_as(dp), C.byref(n_eff), C.byref(kdc))
    return rc, g, xg, xxg, ig, n_eff.value, kdc.value


def test_poly_constants_are_upstreams_bits(orc):
    """FarnebackPrepareGaussian with every tap kept: g, xg, xxg and the four entries of the Cholesky-inverted moment matrix
    equal the oracle's byte for byte, and no combination is refused as not positive definite."""
    lib = _lib()
    for n in POLY_N:
        for sigma in POLY_SIGMA:
            rc, g, xg, xxg, ig, n_eff, kdc = _poly(lib, n, sigma, 1)
            assert rc == 0, (n, sigma, rc)
            og, oxg, oxxg, oig = orc.prepare_gaussian(n, sigma)
            assert n_eff == n and np.isfinite(kdc), (n, sigma, n_eff, kdc)
            for name, mine, ref in (("g", g, og[n:]), ("xg", xg, oxg[n:]), ("xxg", xxg, oxxg[n:]), ("ig", ig, oig)):
                assert mine.dtype == ref.dtype and mine.tobytes() == ref.tobytes(), (n, sigma, name, mine, ref)
    assert _poly(lib, 33, 1.2, 1)[0] == -1 and _poly(lib, 0, 1.2, 1)[0] == -1


def test_poly_tap_truncation():
    """poly_n = 15, sigma = 1.2 without exact_taps: the taps whose weight cannot move a sum are dropped.  n_eff = 7 (15 of
    the 31 taps) is what the commit before rc_plan.cpp existed computes: its host_prepare_poly, compiled on its own with
    g++ -O2 -ffp-contract=off, gives 7 (the comment that stood beside it said 19 taps, i.e. 9; it was wrong).  The taps kept
    are the exact ones."""
    lib = _lib()
    rc, g, xg, xxg, ig, n_eff, kdc = _poly(lib, 15, 1.2, 0)
    rce, ge, xge, xxge, ige, n_effe, kdce = _poly(lib, 15, 1.2, 1)
    assert rc == 0 and rce == 0
    assert n_eff == 7 and n_effe == 15
    k = n_eff + 1
    assert g[:k].tobytes() == ge[:k].tobytes() and xg[:k].tobytes() == xge[:k].tobytes() and xxg[:k].tobytes() == xxge[:k].tobytes()
    assert not g[k:].any() and not xg[k:].any() and not xxg[k:].any()
    assert ig.tobytes() == ige.tobytes()


def test_pyramid_kernel_is_upstreams_bits(orc):
    """getGaussianKernel(ksize, sigma, CV_32F), the fixed small kernels of sigma <= 0 included."""
    lib = _lib()
    fp = C.POINTER(C.c_float)
    for ksize in PYR_KSIZE:
        for sigma in PYR_SIGMA:
            k = np.full(ksize, np.nan, np.float32)
            assert lib.rcflow_debug_plan_pyr_kernel(ksize, sigma, k.ctypes.data_as(fp)) == 0
            assert k.tobytes() == orc.gaussian_kernel(ksize, sigma).tobytes(), (ksize, sigma)
    assert lib.rcflow_debug_plan_pyr_kernel(0, 1.0, np.zeros(1, np.float32).ctypes.data_as(fp)) == -1


def test_profile_kinds_keep_their_ids_names_and_buckets():
    """rcflow_profile_read's name@level strings and rcflow_profile_read_buckets' sums are read by bench.py and kept under
    profiles/: the table's rows are the three parallel lists it replaced."""
    lib = _lib()
    got = []
    for i in range(len(KINDS)):
        name, bucket = C.c_char_p(), C.c_char_p()
        assert lib.rcflow_debug_kind(i, C.byref(name), C.byref(bucket)) == 0
        got.append((name.value.decode(), bucket.value.decode()))
    assert len(KINDS) == 25 and got == KINDS
    name, bucket = C.c_char_p(), C.c_char_p()
    assert lib.rcflow_debug_kind(25, C.byref(name), C.byref(bucket)) == -1 and name.value is None
    assert lib.rcflow_debug_kind(-1, C.byref(name), C.byref(bucket)) == -1


def test_plan_sweep_runs_clean_under_asan_and_ubsan():
    """tests/cpp/plan_check.cpp: rc_plan.cpp alone, over everything the parameter check admits, as a child process."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "plan_check"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "plan_check")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("plan_check: ok")
