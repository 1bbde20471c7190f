"""CPU tier of the shoreline: rcflow_shoreline_plan (no context, no GPU) against the numpy statement and against the transects'
plan, the sizes of the structs, Otsu on hand-made histograms, the sub-sample fraction, the rank rule, the outlier test, and what
the statement finds on the synthetic beach: threshold, separability, waterline error, runup excursion, and why the split is
taken instead of the first crossing."""
import ctypes as C
import functools

import numpy as np
import pytest

import _shoreline_ref as S
import _transects_ref as T
from ripcurrents_amd import _lib

W, H, PUSHES, WINDOW = 96, 64, 32, 16


@functools.lru_cache(maxsize=None)
def beach_run(foam):
    """32 pushes of the beach through the statement, once per kind -> per push: records, summary, thr, eta"""
    ref = S.ShorelineRef(W, H, S.beach_lines(W, H), S.Params(source=S.RMB, radius=2, window=WINDOW, permille=20))
    out = []
    for t in range(PUSHES):
        o = ref.push(S.beach(W, H, t, foam=foam))
        out.append((o["records"].copy(), o["summary"].copy(), o["thr"], o["eta"]))
    return ref, out


def truth(t):
    """the waterline's x on the lines' rows at push t"""
    rows = np.array([int(l[1]) for l in S.beach_lines(W, H)])
    return S.beach_waterline(W, H, t)[rows]


@pytest.mark.parametrize("foam", [False, True])
def test_beach_threshold_and_separability(foam):
    _, out = beach_run(foam)
    thr = [o[2] for o in out]
    eta = [o[3] for o in out]
    print("foam %d: thr %d..%d, eta %.4f..%.4f" % (foam, min(thr), max(thr), min(eta), max(eta)))
    assert all(245 <= t <= 265 for t in thr)
    assert min(eta) >= 0.9


@pytest.mark.parametrize("foam,bar", [(False, 1.0), (True, 2.0)])
def test_beach_waterline_error(foam, bar):
    _, out = beach_run(foam)
    n = W - 8
    worst, mean, agree = 0.0, [], n
    for t, (rec, _, _, _) in enumerate(out):
        assert not (rec["flags"] & (S.DRY | S.WET | S.EMPTY)).any()
        err = rec["x"].astype(np.float64) - truth(t)
        worst = max(worst, float(np.abs(err).max()))
        mean.append(float(err.mean()))
        agree = min(agree, int(rec["agree"].min()))
    print("foam %d: largest waterline error %.3f px, mean %+.3f px, least agree %d of %d" % (foam, worst, float(np.mean(mean)), agree, n))
    assert worst <= bar


@pytest.mark.parametrize("foam", [False, True])
def test_beach_runup_excursion(foam):
    """a window of 16 pushes holds one period: the excursion is 2 amp = 10 px (a sample a pixel, a metre a pixel)"""
    _, out = beach_run(foam)
    lo, hi, merr = 1e9, 0.0, 0.0
    for t in range(WINDOW - 1, PUSHES):
        rec = out[t][0]
        assert (rec["nv"] == WINDOW).all()
        lo, hi = min(lo, float(rec["excursion_m"].min())), max(hi, float(rec["excursion_m"].max()))
        want = np.mean([truth(u) for u in range(t - WINDOW + 1, t + 1)], axis=0) - 4.0       # the lines begin at x = 4
        merr = max(merr, float(np.abs(rec["pos_mean"] / 256.0 - want).max()))
        assert ((rec["pos_min"] <= rec["pos_q"]) & (rec["pos_q"] <= rec["pos_max"])).all()
    print("foam %d: excursion %.2f..%.2f px, window mean error %.2f px" % (foam, lo, hi, merr))
    assert 9.0 <= lo and hi <= 11.0


def test_why_the_split_and_not_the_first_crossing():
    """on the unsmoothed indicator the first sample at or below thr lies more than 2 samples from the split on well over 5 % of
    lines and pushes: the speckles"""
    lines = S.beach_lines(W, H)
    table, geom = S.plan(W, H, lines)
    far = total = worst = 0
    for t in range(PUSHES):
        J = S.smooth(S.indicator(S.beach(W, H, t), S.RMB), 0)
        thr, _, _ = S.otsu(S.histogram(J))
        V = S.sample(J, table, W, H)
        for g in geom:
            wet = S.is_wet(V[g["first"]:g["first"] + g["n"]], thr, 0)
            d = abs(S.first_crossing(wet) - S.split(wet)[0])
            far, total, worst = far + (d > 2), total + 1, max(worst, d)
    print("first crossing more than 2 samples from the split on %.1f %% of %d lines, up to %d samples" % (100.0 * far / total, total, worst))
    assert far / total > 0.05


def test_otsu_on_hand_made_histograms():
    h = np.zeros(512, np.int64)
    h[100], h[300] = 7, 7
    thr, eta, N = S.otsu(h)
    assert (thr, N) == (100, 14) and eta == 1.0            # every t in 100..299 ties: the first wins
    assert S.otsu(h, fixed=200)[0] == 200 and S.otsu(h, fixed=200)[1] == 1.0
    assert S.otsu(h, fixed=50) == (50, 0.0, 14)             # a skipped t: no score
    h[:] = 0
    h[123] = 9
    assert S.otsu(h) == (-1, 0.0, 9)                        # one bin
    assert S.otsu(h, fixed=10) == (10, 0.0, 9)
    h[:] = 0
    assert S.otsu(h) == (-1, 0.0, 0) and S.otsu(h, fixed=10) == (-1, 0.0, 0)
    h[0], h[510] = 1, 3                                     # the ends of the range
    thr, eta, N = S.otsu(h)
    assert (thr, N) == (0, 4) and eta == 1.0
    h[:] = 0
    h[10], h[20], h[30] = 5, 1, 5                           # symmetric: t = 10 and t = 20 tie, the first wins
    assert S.otsu(h)[0] == 10 and 0 < S.otsu(h)[1] < 1


def test_frac_at_the_ends():
    thr = 255
    assert S.frac_of(thr + 40, thr, thr) == (79 * 256 + 40) // 80 == 253      # b = thr: the crossing lies just before sample k*
    assert S.frac_of(thr + 1, thr - 39, thr) == (256 + 40) // 80 == 3         # a = thr + 1: just after sample k* - 1
    assert S.frac_of(thr + 1, thr, thr) == 128                                # neighbours: the middle
    for a, b in ((256, 255), (510, 0), (256, 0), (510, 255), (300, 200)):
        assert 0 <= S.frac_of(a, b, thr) <= 256
    assert S.frac_of(0, 510, 200) <= 256 and S.frac_of(200, 201, 200) == 128  # wet_is_high: a <= thr < b


@pytest.mark.parametrize("nv", [1, 16, 4096])
def test_rank_rule(nv):
    want = {1: (0, 0, 0, 0), 16: (0, 0, 7, 15), 4096: (4, 81, 2047, 4091)}[nv]
    assert tuple(S.rank_of(nv, p) for p in (1, 20, 500, 999)) == want
    assert all(0 <= S.rank_of(nv, p) < nv for p in range(1, 1000))


def test_planted_outlier():
    wx = np.array([1000, 1010, 9000, 1030, 1040, 1050]) * 1
    wy = np.arange(6) * 1280
    has = np.ones(6, bool)
    assert S.outliers(has, wx, wy, 8.0).tolist() == [False, False, True, False, False, False]      # the good lines have a good neighbour
    assert not S.outliers(has, wx, wy, 40.0).any()           # |dwy| = 1280 * 2 is the nearest good one's: 10 px
    has[2] = False
    assert not S.outliers(has, wx, wy, 8.0 + 2.0).any()      # line 2 has no position: its neighbours look past it, 2 places
    lone = np.array([False, False, False, True, False, False])
    assert not S.outliers(lone, wx, wy, 0.01).any()          # no neighbour within 2 places: not tested


def test_struct_sizes_and_exports():
    assert C.sizeof(_lib.ShorelineParams) == 56 and C.sizeof(_lib.ShorelineRecord) == 64 and C.sizeof(_lib.ShorelineInfo) == 96
    import ripcurrents_amd.api as api
    assert api.SHORELINE_DTYPE == S.RECORD and S.RECORD.itemsize == 64
    for name, _ in _lib.ShorelineRecord._fields_:
        assert getattr(_lib.ShorelineRecord, name).offset == S.RECORD.fields[name][1], name
    assert api.SHORELINE_SUMMARY == S.SUMMARY and _lib.RC_SHORE_HIST == S.HIST
    assert (_lib.RC_SHORE_MAX_LINES, _lib.RC_SHORE_MIN_SAMPLES, _lib.RC_SHORE_MAX_SAMPLES, _lib.RC_SHORE_MAX_TOTAL, _lib.RC_SHORE_MAX_RADIUS,
            _lib.RC_SHORE_MAX_WINDOW) == (S.MAX_LINES, S.MIN_SAMPLES, S.MAX_SAMPLES, S.MAX_TOTAL, S.MAX_RADIUS, S.MAX_WINDOW)
    lib = _lib.load()
    for n in ("plan", "open", "push_dev", "prims_dev", "read", "ring_read", "table_read", "set", "reset", "close", "info"):
        assert hasattr(lib, "rcflow_shoreline_" + n)


def test_plan_is_the_statements_and_the_transects():
    import ripcurrents_amd.api as api
    lines = [(4.0, 4.0, 91.0, 4.0, 88), (3.3, 60.7, 90.2, 2.1, 8), (95.0, 0.0, 95.0, 63.0, 1024), (0.0, 63.0, 95.0, 63.0, 17)]
    table, geom = api.shoreline_plan(W, H, lines, 0.25)
    rt, rg = S.plan(W, H, lines, 0.25)
    assert table.tobytes() == rt.tobytes() and geom.tobytes() == rg.tobytes()
    tt, tg = api.transects_plan(W, H, lines, 0.25, 1.0)      # the shared per-line rule
    assert table.tobytes() == tt.tobytes() and geom.tobytes() == tg.tobytes()
    t0, g0 = T.plan(W, H, lines, 0.25, 1.0)                   # and the transects' own plan is what it was
    assert tt.tobytes() == t0.tobytes() and tg.tobytes() == g0.tobytes()


def test_plan_refusals():
    lib = _lib.load()
    def plan(lines, w=W, h=H, mpp=1.0):
        arr = (_lib.TransectLine * len(lines))(*[_lib.TransectLine(*l) for l in lines])
        rc = lib.rcflow_shoreline_plan(w, h, arr, len(lines), mpp, None, None, None)
        return rc, (lib.rcflow_last_error() or b"").decode()
    good = (4.0, 4.0, 91.0, 4.0, 88)
    assert plan([good])[0] == 0
    for bad in ([(4.0, 4.0, 91.0, 4.0, 7)], [(4.0, 4.0, 91.0, 4.0, 1025)], [(4.0, 4.0, 96.0, 4.0, 88)], [(4.0, 4.0, 4.0, 4.0, 8)],
                [(float("nan"), 4.0, 91.0, 4.0, 8)], [good] * 1025, [(4.0, 4.0, 91.0, 4.0, 1024)] * 257):
        rc, text = plan(bad)
        assert rc == -1 and text.startswith("rcflow_shoreline_plan"), text
    assert plan([good], mpp=0.0)[0] == -1 and plan([good], w=0)[0] == -1
    assert plan([(4.0, 4.0, 91.0, 4.0, 1024)] * 256)[0] == 0  # S = 262144 is the bound itself
