"""CPU tier of the transects: rcflow_transects_plan (no context, no GPU) against the numpy statement, the sizes of the structs,
the statement's own invariant (accumulators kept in step = a rescan of the ring), and what the statement recovers: the drift
along a line on the translating clip, flux and jets on the surf field."""
import ctypes as C

import numpy as np
import pytest

import _transects_ref as R
from ripcurrents_amd import _lib, synth


def _c_plan(w, h, lines, mpp=1.0, fps=1.0):
    """rcflow_transects_plan through ctypes alone -> (code, table, geom)"""
    lib = _lib.load()
    arr = (_lib.TransectLine * len(lines))(*[_lib.TransectLine(*[float(v) for v in l[:4]], int(l[4])) for l in lines])
    total = C.c_int(-1)
    rc = lib.rcflow_transects_plan(w, h, arr, len(lines), mpp, fps, None, None, C.byref(total))
    if rc:
        return rc, None, None
    table, geom = np.zeros(total.value, R.SAMPLE), np.zeros(len(lines), R.GEOM)
    assert lib.rcflow_transects_plan(w, h, arr, len(lines), mpp, fps, table.ctypes.data, geom.ctypes.data, None) == 0
    return 0, table, geom


LINE_SETS = [
    (160, 120, [(8.0, 60.0, 151.0, 60.0, 144)], 1.0, 1.0),
    (96, 64, [(3.0, 60.25, 40.5, 8.125, 16), (95.0, 2.0, 95.0, 63.0, 37), (2.5, 63.0, 93.0, 63.0, 50)], 0.5, 25.0),
    (1100, 12, [(1.0, 3.3, 1098.7, 8.6, 1024)], 0.037, 29.97),
    (640, 480, [(0.0, 0.0, 639.0, 479.0, 2), (639.0, 479.0, 0.0, 0.0, 1024), (17.3, 400.9, 17.3, 2.2, 7)], 2.5, 2.0),
    (64, 48, [(float(k), 0.0, 63.0 - k, 47.0, 1024) for k in range(64)], 1.0, 1.0),        # 64 lines of 1024 samples: every bound
]


@pytest.mark.parametrize("k", range(len(LINE_SETS)))
def test_plan_equals_the_statement(k):
    w, h, lines, mpp, fps = LINE_SETS[k]
    rc, table, geom = _c_plan(w, h, lines, mpp, fps)
    assert rc == 0
    t, g = R.plan(w, h, lines, mpp, fps)
    assert table.tobytes() == t.tobytes() and geom.tobytes() == g.tobytes()
    assert int(g["n"].sum()) == len(t) and (np.diff(g["first"]) == g["n"][:-1]).all()
    # the normal is the tangent turned to the left as the picture shows it (y down): a line drawn left to right looks up
    assert np.allclose(g["nx"], g["ey"]) and np.allclose(g["ny"], -g["ex"])


def test_plan_left_to_right_has_its_positive_side_up():
    _, _, g = _c_plan(160, 120, [(8.0, 60.0, 151.0, 60.0, 144)])
    assert (g["ex"][0], g["ey"][0], g["nx"][0], g["ny"][0]) == (1.0, 0.0, 0.0, -1.0) and g["ds"][0] == 1.0 and g["len"][0] == 143.0


def test_plan_refusals():
    ok = (8.0, 60.0, 151.0, 60.0, 144)
    nan, inf = float("nan"), float("inf")
    bad = [
        (160, 120, [], 1.0, 1.0), (160, 120, [ok] * 65, 1.0, 1.0), (0, 120, [ok], 1.0, 1.0), (160, 120, [ok], 0.0, 1.0), (160, 120, [ok], 1.0, nan),
        (160, 120, [ok], inf, 1.0), (160, 120, [ok[:4] + (1,)], 1.0, 1.0), (160, 120, [ok[:4] + (1025,)], 1.0, 1.0),
        (160, 120, [(8.0, 60.0, 8.0, 60.0, 10)], 1.0, 1.0),                                   # no length
        (160, 120, [(8.0, 60.0, 159.04, 60.0, 10)], 1.0, 1.0), (160, 120, [(-0.04, 60.0, 100.0, 60.0, 10)], 1.0, 1.0),
        (160, 120, [(8.0, 60.0, 100.0, 119.04, 10)], 1.0, 1.0), (160, 120, [(nan, 60.0, 100.0, 60.0, 10)], 1.0, 1.0),
        (160, 120, [(8.0, inf, 100.0, 60.0, 10)], 1.0, 1.0),
    ]
    for w, h, lines, mpp, fps in bad:
        if lines:
            assert _c_plan(w, h, lines, mpp, fps)[0] == -1, lines
            with pytest.raises(ValueError):
                R.plan(w, h, lines, mpp, fps)
    lib = _lib.load()
    assert lib.rcflow_transects_plan(160, 120, None, 1, 1.0, 1.0, None, None, None) == -1 and lib.rcflow_last_error()
    # the rim itself is inside: 159.03 rounds to 16 * 159
    assert _c_plan(160, 120, [(8.0, 60.0, 159.03, 119.03, 10)])[0] == 0


def test_struct_sizes_and_exports():
    assert C.sizeof(_lib.TransectLine) == 20 and C.sizeof(_lib.TransectsParams) == 56 and C.sizeof(_lib.TransectsInfo) == 104
    assert R.RECORD.itemsize == 64 and R.SAMPLE.itemsize == 16 and R.GEOM.itemsize == 48
    import ripcurrents_amd.api as api
    assert api.TRANSECT_DTYPE == R.RECORD and api.TRANSECT_SAMPLE_DTYPE == R.SAMPLE and api.TRANSECT_GEOM_DTYPE == R.GEOM
    assert len(api.TRANSECTS_SUMS) == _lib.RC_TRANSECTS_SUMS == R.NSUMS and len(api.TRANSECTS_SUMMARY) == 8
    lib = _lib.load()
    for n in ("plan", "open", "push_dev", "read", "sums_read", "table_read", "set", "reset", "close", "info"):
        assert hasattr(lib, "rcflow_transects_" + n) and "rcflow_transects_" + n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rcflow_transects_push_dev"]) == 14
    assert (_lib.RC_TRANSECTS_MAX_LINES, _lib.RC_TRANSECTS_MAX_SAMPLES, _lib.RC_TRANSECTS_MAX_TOTAL, _lib.RC_TRANSECTS_LAUNCHES) == (64, 1024, 65536, 3)
    t, g = api.transects_plan(160, 120, [(8.0, 60.0, 151.0, 60.0, 144)])
    assert len(t) == 144 and g["n"][0] == 144


def test_accumulators_equal_a_rescan_through_two_wraps():
    case = R.cases()["three"]
    ref = R.TransectsRef(case.w, case.h, case.lines, case.p)
    T = case.p.window
    assert len(case.gray) > 2 * T
    for t in range(len(case.gray)):
        ref.push(case.gray[t], case.flow[t], compute=False)
        Ts, Ta = ref.rescan()
        assert np.array_equal(ref.T, Ts) and np.array_equal(ref.Ta, Ta), "push %d" % (t + 1)
        assert ref.pairs() == max(0, min(t + 1, T) - case.p.lag) and (ref.pairs() > 0) == bool(ref.T.any())
    assert ref.pairs() == T - case.p.lag


# ---------------------------------------------------------------------------- what the statement recovers
# motion purely along the line, in pixels per frame; fps = metres_per_pixel = 1 and samples a pixel apart, so v_along is in those
# units.  name -> (motion, line, {lag: |v_along - truth| of the statement in that run, as measured: DESIGN 7o})
RECOVERY = {
    "right": ((1.25, 0.0), (16.0, 60.0, 143.0, 60.0, 128), {1: 0.00191, 2: 0.00056}),
    "left": ((-2.5, 0.0), (16.0, 60.0, 143.0, 60.0, 128), {1: 0.00096, 2: 0.00842}),
    "down": ((0.0, 1.0), (80.0, 12.0, 80.0, 107.0, 96), {1: 0.00210, 2: 0.00110}),
    "half": ((0.4, 0.0), (16.5, 60.5, 143.5, 60.5, 128), {1: 0.00727, 2: 0.01014}),
}
RECOVERY_FRAMES = 12


def recovered(name, lag):
    (u, v), line, _ = RECOVERY[name]
    clip = synth.translating_clip(160, 120, frames=RECOVERY_FRAMES, u=u, v=v)
    ref = R.TransectsRef(160, 120, [line], R.Params(window=32, sources=R.GRAY, lag=lag, range=8))
    for f in clip:
        out = ref.push(np.asarray(f))
    along = u if line[1] == line[3] else v
    return out["records"][0], along


@pytest.mark.parametrize("lag", (1, 2))
@pytest.mark.parametrize("name", list(RECOVERY))
def test_recovers_the_drift_along_the_line(name, lag):
    rec, truth = recovered(name, lag)
    err = abs(float(rec["v_along"]) - truth)
    print("%s lag %d: v_along %.5f, truth %.2f, error %.5f, peak %.4f" % (name, lag, rec["v_along"], truth, err, rec["corr_peak"]))
    assert rec["flags"] == 0 and rec["pairs"] == RECOVERY_FRAMES - lag
    assert err <= 1.5 * RECOVERY[name][2][lag]                    # each run against its own figure


def test_flux_and_jets_on_the_surf_field():
    w, h = 160, 120
    U, V = synth.surf_field(w, h)
    flow = np.stack([U, V], -1).astype(np.float32)
    ref = R.TransectsRef(w, h, [(8.0, 60.0, 151.0, 60.0, 144)], R.Params(window=4, sources=R.FLOW, jet_min=0.25))
    for _ in range(6):
        out = ref.push(flow=flow)
    rec, sums = out["records"][0], out["sums"][0]
    # the line looks offshore (up the picture): un = -V = 3.5 jet - 1.5, at least 0.25 where |x - 88| <= 11.3
    assert rec["jets"] == 1 and rec["jet_start"] == 69 and rec["jet_len"] == 23 and rec["jet_peak_at"] == 80 and rec["bad"] == 0
    assert rec["jet_peak"] == 2.0 and sums[9] == 2 << 16
    assert abs(float(rec["flux_out"]) - 30.494) < 1e-3 and abs(float(rec["flux_in"]) + 162.271) < 1e-3
    assert sums[0] + sums[1] == sum(R.Q(v) for v in out["profile"][:, 1]) and sums[3] == 144
    assert rec["flags"] == R.EMPTY and list(out["summary"]) == [4, 0, 0, 1, 1, 0, 6, 0]
    # a constant field: the window mean is the field, whatever the window holds
    assert np.array_equal(out["profile"], ref.rows_f[-1])


def test_open_rules_of_the_statement():
    line = [(2.0, 20.0, 61.0, 20.0, 60)]
    ok = R.Params(window=3, sources=R.GRAY, lag=1, range=3)
    assert R.open_error(64, 48, line, ok) is None
    for bad in (dict(window=1), dict(window=4097), dict(sources=0), dict(sources=4), dict(lag=0), dict(lag=9), dict(range=17), dict(range=-1),
                dict(sources=R.FLOW), dict(window=2, lag=2), dict(fps=0.0), dict(jet_min=float("nan")), dict(jet_min=2.0 ** 20), dict(jet_min=1e20),
                dict(vis_max=float("inf")), dict(metres_per_pixel=-1.0)):
        assert R.open_error(64, 48, line, R.Params(**dict(R.asdict(ok), **bad))) is not None, bad
    assert R.open_error(64, 48, [(2.0, 20.0, 61.0, 20.0, 14)], ok) is None and R.open_error(64, 48, [(2.0, 20.0, 61.0, 20.0, 13)], ok) is not None
