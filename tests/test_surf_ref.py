"""CPU tier of the surf zone: what the numpy statement finds on the synthetic surf zone (the channel lines and nothing else, the
band's edges, no breaking on sand or persistent foam), the variance image against numpy.std, the running sums against a rescan of
the rings, rcflow_surf_plan (no context, no GPU) against the statement and against the shoreline's and the transects' plans, the
sizes of the structs."""
import ctypes as C
import functools

import numpy as np
import pytest

import _shoreline_ref as SH
import _surf_ref as S
import _transects_ref as T
from ripcurrents_amd import _lib

W, H, PUSHES = S.SCENE_W, S.SCENE_H, 64


@functools.lru_cache(maxsize=None)
def scene_run(foam):
    """64 pushes of the scene through the statement, once per kind -> per push: lines, channels, summary, Q, surf mask"""
    ref = S.SurfRef(W, H, S.scene_lines(), S.SCENE, S.fake_lut())
    out = []
    for t in range(PUSHES):
        o = ref.push(S.surf_scene(t, foam=foam))
        out.append((o["lines"].copy(), o["channels"].copy(), o["summary"].copy(), o["q"].astype(np.int64), o["surf"].copy()))
    return ref, out


@pytest.mark.parametrize("foam", [False, True])
def test_scene_channels_are_the_five_lines(foam):
    """from push 8 on: exactly lines 9, 10, 11, 22 and 23, two channels [9, 3] and [22, 2]; their share at most 300 per mille,
    every other line's at least 900.  (The statement: the set is exact from push 3 on, 154..214 against >= 982 at push 64.)"""
    _, out = scene_run(foam)
    ch = np.isin(np.arange(H // 2), S.CHANNEL_LINES)
    exact = [tuple(np.flatnonzero(o[0]["flags"] & S.CHANNEL)) == S.CHANNEL_LINES for o in out]
    lo_c, hi_c, lo_o = 10 ** 9, 0, 10 ** 9
    for t, (lines, chans, summ, _, _) in enumerate(out):
        if t + 1 < 8:
            continue
        assert exact[t], "push %d: channel lines %s" % (t + 1, np.flatnonzero(lines["flags"] & S.CHANNEL))
        assert int(summ[5]) == 5 and int(summ[6]) == 2 and not chans[2:].view(np.uint8).any()
        assert [(int(c["first"]), int(c["count"])) for c in chans[:2]] == [(9, 3), (22, 2)]
        assert tuple(np.flatnonzero(lines["flags"] & S.IN_CHANNEL)) == S.CHANNEL_LINES and not (lines["flags"] & S.NOREF).any()
        lo_c, hi_c, lo_o = min(lo_c, int(lines["share"][ch].min())), max(hi_c, int(lines["share"][ch].max())), min(lo_o, int(lines["share"][~ch].min()))
        for c in chans[:2]:
            assert c["first"] <= c["centre"] < c["first"] + c["count"] and c["share"] == lines["share"][c["centre"]]
            assert c["share"] == lines["share"][c["first"]:c["first"] + c["count"]].min()
            assert c["cy"] == 256 * (1 + 2 * c["centre"])
        assert [float(c["width_m"]) for c in chans[:2]] == [8.0, 6.0]     # between the land ends of lines 8 and 12, 21 and 24
    print("foam %d: the channel set is exact from push %d on; from push 8 on share on channel lines %d..%d, elsewhere >= %d" % (
        foam, len(exact) - exact[::-1].index(False) + 1, lo_c, hi_c, lo_o))
    assert hi_c <= 300 and lo_o >= 900


@pytest.mark.parametrize("foam", [False, True])
def test_scene_band_edges_and_quiet_sand(foam):
    """Q is 0 on the sand and on the persistent foam strip, however bright, on every push.  Once the window is full (push 32 on)
    k0 and k1 are within one sample of 36 and 55 (x 40..59) on every line outside the channels, and those inside have no band;
    a channel's centre point lies in the middle of the band.  The edges are read at the full window because q_min is a share of
    the n frames held: while n <= 10 a single glitter hit is a tenth of a pixel's time, and three glitter pixels in a row make a
    run (the statement: k1 = 79 on one line at push 9, 79 and 65 on two lines at push 10, 36 and 55 on every line of every other
    push from 8 on; at the full window Q among the glitter is at most 4 and needs 4 in 3 pixels in a row)."""
    _, out = scene_run(foam)
    ch = np.isin(np.arange(H // 2), S.CHANNEL_LINES)
    rows = np.ones(H, bool)
    for a, b in S.CHANNEL_ROWS:
        rows[a:b] = False
    qb, qc, qg, surf_px, early = set(), 0, 0, set(), []
    for t, (lines, chans, summ, Q, surf) in enumerate(out):
        assert not Q[:, :24].any(), "push %d: breaking on the sand or the foam strip" % (t + 1)
        off = (np.abs(lines["k0"][~ch] - 36) > 1) | (np.abs(lines["k1"][~ch] - 55) > 1)
        if 8 <= t + 1 < S.SCENE.window and off.any():
            early.append((t + 1, int(off.sum())))
        if t + 1 < S.SCENE.window:
            continue
        assert not off.any(), "push %d: k0 %s k1 %s" % (t + 1, lines["k0"][~ch], lines["k1"][~ch])
        assert (lines["flags"][ch] & S.NOBAND).all() and (lines["k0"][ch] == -1).all() and (lines["k1"][ch] == -1).all()
        assert all(abs(c["cx"] / 256.0 - 49.5) <= 1.0 for c in chans[:2])
        if t + 1 < 48:                                       # flags of the first pushes, taken against a mean of a few frames, are still held
            continue
        qb |= set(np.unique(Q[rows][:, S.BAND[0]:S.BAND[1]]).tolist())
        qc, qg = max(qc, int(Q[~rows][:, S.BAND[0]:S.BAND[1]].max())), max(qg, int(Q[:, 62:].max()))
        surf_px.add(int(summ[2]))
    print("foam %d: Q in the band %s of 32, in a channel <= %d, among the glitter <= %d; surf pixels %d..%d (the band has %d); "
          "pushes 8..31 with an edge off by more than a sample (push, lines): %s" % (foam, sorted(qb), qc, qg, min(surf_px), max(surf_px), 20 * (H - 10), early))
    assert qb == {8} and qc <= 2


def test_bright_but_not_above_its_mean_never_breaks():
    """a saturated sky: bright in every frame, so never above its own mean by delta; and nothing breaks on the first push"""
    ref = S.SurfRef(5, 4, [], S.Params(window=4, bright=180, delta=1), S.fake_lut())
    for t in range(9):
        o = ref.push(np.full((4, 5), 255, np.uint8))
        assert not o["now"].any() and not o["q"].any() and int(o["summary"][0]) == min(t + 1, 4)
    o = ref.push(np.full((4, 5), 100, np.uint8))
    assert not o["now"].any()
    o = ref.push(np.full((4, 5), 255, np.uint8))       # the mean is now below 255 - 1
    assert o["now"].all() and (o["q"] == 1).all()


@pytest.mark.parametrize("W_", [2, 5, 32])
def test_sd_is_twice_numpy_std_within_one_level(W_):
    rng = np.random.default_rng(3)
    ref = S.SurfRef(23, 11, [], S.Params(window=W_), S.fake_lut())
    worst = 0.0
    for t in range(3 * W_):
        f = rng.integers(0, 256, (11, 23), dtype=np.uint8) if t % 7 else np.where(rng.random((11, 23)) < 0.5, 255, 0).astype(np.uint8)
        o = ref.push(f)
        held = ref.ring[:min(t + 1, W_)].astype(np.float64)
        two_sigma = np.minimum(255.0, 2.0 * held.std(axis=0))
        worst = max(worst, float(np.abs(o["sd"].astype(np.float64) - two_sigma).max()))
        assert np.abs(o["mean"].astype(np.float64) - held.mean(axis=0)).max() <= 0.5 + 1e-9
    print("W %d: largest |sd - 2 sigma| %.3f grey levels" % (W_, worst))
    assert worst <= 1.0


def test_running_sums_equal_a_rescan_after_every_push():
    rng = np.random.default_rng(11)
    W_ = 7
    ref = S.SurfRef(19, 6, [], S.Params(window=W_, bright=128, delta=10), S.fake_lut())
    for t in range(3 * W_):
        o = ref.push(rng.integers(0, 256, (6, 19), dtype=np.uint8))
        s1, s2, q = ref.rescan()
        assert np.array_equal(ref.S1, s1) and np.array_equal(ref.S2, s2) and np.array_equal(ref.Q, q) and np.array_equal(o["q"], q)
    assert ref.Q.max() > 0


def test_isqrt_and_reference_and_runs():
    v = np.array([0, 1, 2, 3, 4, 8, 9, 15, 16, 2 ** 40 - 1, 2 ** 40, 2 ** 46 - 1], np.int64)
    assert S.isqrt(v).tolist() == [0, 1, 1, 1, 2, 2, 3, 3, 4, 2 ** 20 - 1, 2 ** 20, 8388607]
    assert S.reference(np.array([5, 1, 9, 3]), 0).tolist() == [5, 1, 9, 3]                 # the line itself
    assert S.reference(np.array([5, 1, 9, 3]), 1).tolist() == [1, 5, 3, 3]                 # m = 2: the lower of two; m = 3: the median
    assert S.reference(np.array([5, 1, 9, 3]), 32).tolist() == [3, 3, 3, 3]                # m = 4: rank 1
    assert S.runs(np.array([1, 1, 0, 1, 1, 1, 0, 1], bool), 2) == [(0, 1), (3, 5)] and S.runs(np.zeros(4, bool), 1) == []
    assert S.point(64, 1456, 256 * 87, 88) == 16 * 1456 and S.point(64, 1456, 0, 88) == 16 * 64


def test_struct_sizes_and_exports():
    assert C.sizeof(_lib.SurfParams) == 56 and C.sizeof(_lib.SurfLine) == 64 and C.sizeof(_lib.SurfChannel) == 32 and C.sizeof(_lib.SurfInfo) == 96
    import ripcurrents_amd.api as api
    assert api.SURF_LINE_DTYPE == S.LINE and S.LINE.itemsize == 64 and api.SURF_CHANNEL_DTYPE == S.CHAN and S.CHAN.itemsize == 32
    for rec, dt in ((_lib.SurfLine, S.LINE), (_lib.SurfChannel, S.CHAN)):
        for name, _ in rec._fields_:
            assert getattr(rec, name).offset == dt.fields[name][1], name
    assert api.SURF_SUMMARY == S.SUMMARY
    assert (_lib.RC_SURF_MAX_LINES, _lib.RC_SURF_MIN_SAMPLES, _lib.RC_SURF_MAX_SAMPLES, _lib.RC_SURF_MAX_TOTAL, _lib.RC_SURF_MAX_WINDOW,
            _lib.RC_SURF_MAX_SPAN, _lib.RC_SURF_MAX_CHANNELS, _lib.RC_SURF_MAX_SHARE, _lib.RC_SURF_MAX_PIXELS, _lib.RC_SURF_MAX_STATE_BYTES) == (
        S.MAX_LINES, S.MIN_SAMPLES, S.MAX_SAMPLES, S.MAX_TOTAL, S.MAX_WINDOW, S.MAX_SPAN, S.MAX_CHANNELS, S.MAX_SHARE, S.MAX_PIXELS, S.MAX_STATE_BYTES)
    assert (_lib.RC_SURF_NOBAND, _lib.RC_SURF_NOREF, _lib.RC_SURF_CHANNEL, _lib.RC_SURF_IN_CHANNEL) == (S.NOBAND, S.NOREF, S.CHANNEL, S.IN_CHANNEL)
    lib = _lib.load()
    for n in ("plan", "open", "push_dev", "prims_dev", "read", "table_read", "set", "reset", "close", "info"):
        assert hasattr(lib, "rcflow_surf_" + n)


def test_plan_is_the_statements_and_leaves_the_others_as_they_were():
    import ripcurrents_amd.api as api
    lines = [(4.0, 4.0, 91.0, 4.0, 88), (3.3, 60.7, 90.2, 2.1, 8), (95.0, 0.0, 95.0, 63.0, 1024), (0.0, 63.0, 95.0, 63.0, 17)]
    table, geom = api.surf_plan(W, H, lines, 0.25)
    rt, rg = S.plan(W, H, lines, 0.25)
    assert table.tobytes() == rt.tobytes() and geom.tobytes() == rg.tobytes()
    st, sg = api.shoreline_plan(W, H, lines, 0.25)             # the shared per-line rule: the shoreline's table is what it was
    assert st.tobytes() == table.tobytes() and sg.tobytes() == geom.tobytes()
    s0, g0 = SH.plan(W, H, lines, 0.25)
    assert st.tobytes() == s0.tobytes() and sg.tobytes() == g0.tobytes()
    tt, tg = api.transects_plan(W, H, lines, 0.25, 1.0)        # and so is the transects'
    t0, g0 = T.plan(W, H, lines, 0.25, 1.0)
    assert tt.tobytes() == t0.tobytes() and tg.tobytes() == g0.tobytes() and tt.tobytes() == table.tobytes()
    table, geom = api.surf_plan(W, H, [])                      # no lines: allowed
    assert table.size == 0 and geom.size == 0


def test_plan_refusals():
    lib = _lib.load()

    def plan(lines, w=W, h=H, mpp=1.0):
        arr = (_lib.TransectLine * len(lines))(*[_lib.TransectLine(*l) for l in lines]) if lines else None
        rc = lib.rcflow_surf_plan(w, h, arr, len(lines), mpp, None, None, None)
        return rc, (lib.rcflow_last_error() or b"").decode()
    good = (4.0, 4.0, 91.0, 4.0, 88)
    assert plan([good])[0] == 0 and plan([])[0] == 0
    for bad in ([(4.0, 4.0, 91.0, 4.0, 7)], [(4.0, 4.0, 91.0, 4.0, 1025)], [(4.0, 4.0, 96.0, 4.0, 88)], [(4.0, 4.0, 4.0, 4.0, 8)],
                [(float("nan"), 4.0, 91.0, 4.0, 8)], [good] * 1025, [(4.0, 4.0, 91.0, 4.0, 1024)] * 257):
        rc, text = plan(bad)
        assert rc == -1 and text.startswith("rcflow_surf_plan"), text
    assert plan([good], mpp=0.0)[0] == -1 and plan([good], w=0)[0] == -1
    assert lib.rcflow_surf_plan(W, H, None, 1, 1.0, None, None, None) == -1
    assert plan([(4.0, 4.0, 91.0, 4.0, 1024)] * 256)[0] == 0  # S = 262144 is the bound itself


def test_state_bytes_rule():
    assert S.state_bytes(1920, 1080, 256) == 1920 * 1080 * 266 + 32 * 256 * 8100
    assert S.open_error(1920, 1080, [], S.Params(window=4096)) == "size" and S.open_error(640, 360, [], S.Params(window=4096)) is None
    assert S.open_error(5, 4, [], S.Params(window=1)) == "parameters" and S.open_error(5, 4, [], S.Params(span=33)) == "parameters"
