"""The offshore frame on the device (offshore_kernels.hip) against its numpy statement (tests/_offshore_ref.py): every plane of the map,
of the push and of the band, the table, the records and both summaries, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _drifters_ref as D
import _meanflow_ref as M
import _offshore_ref as R
import _regions_ref as RG
import _shoreline_ref as S
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, Outputs, Padded, ptr, raw, same_bits
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RC_OFFSHORE_MAP_LAUNCHES, RC_OFFSHORE_PUSH_LAUNCHES, OffshoreInfo, OffshoreParams, RcflowError
from ripcurrents_amd.api import OFFSHORE_MAP_SUMMARY, OFFSHORE_PUSH_SUMMARY, OFFSHORE_STATION_DTYPE, Offshore

pytestmark = pytest.mark.gpu

OF_TILE = 256                                                     # offshore_kernels.hip: the pixels of a row one block of the row pass owns
dev = Padded.of
GENERAL = R.Params(min_dist=2, max_dist=30, stations=5, bins=6, bin_width=4, min_count=3, rip_bins=2, cross_min=0.5, station="x")


def with_(p, **kw):
    return R.Params(**{**R.asdict(p), **kw})


def views(d):
    if "stations" in d:
        d["stations"] = d["stations"].view(OFFSHORE_STATION_DTYPE)
    if "table" in d:
        d["table"] = d["table"].reshape(-1, R.SUMS)


def map_outputs(w, h, pad=0):
    planes = dict(dist2=((h, w), torch.int32), near=((h, w), torch.int32), sdist=((h, w), torch.int32), picture=((h, w, 3), torch.uint8))
    return Outputs(planes, dict(summary=((R.SUMMARY_WORDS,), torch.int64, -1)), pad)


def push_outputs(p, w, h, pad=0):
    planes = dict(cross_along=((h, w, 2), torch.float32), cls=((h, w), torch.uint8), mask=((h, w), torch.uint8), picture=((h, w, 3), torch.uint8))
    flat = dict(stations=((p.stations * 48,), torch.uint8, None), table=((p.stations * p.bins * R.SUMS,), torch.int64, -1),
                summary=((R.SUMMARY_WORDS,), torch.int64, -1))
    return Outputs(planes, flat, pad, views)


def same(k, a, b):
    if k == "cross_along":
        return same_bits(a, b)
    if k == "stations":
        return all(a[f].tobytes() == b[f].tobytes() for f in b.dtype.names)
    return np.array_equal(a, b)


def compare(got, want, what):
    for k in got:
        assert same(k, got[k], want[k]), "%s differs %s: %s, wanted %s" % (k, what, got[k], want[k])


class Session:
    """the device session and the statement side by side"""

    def __init__(self, ctx, w, h, p, pad=0, stream=0):
        self.ctx, self.w, self.h, self.pad, self.stream = ctx, w, h, pad, stream
        self.ref = R.OffshoreRef(w, h, p, ctx.jet_lut())
        ctx.offshore_open(w, h, stream=stream, **p.kw())
        info = ctx.offshore_info(stream=stream)
        assert (info["launches_per_map"], info["launches_per_push"]) == (RC_OFFSHORE_MAP_LAUNCHES, RC_OFFSHORE_PUSH_LAUNCHES) == (3, 2)
        assert (info["have_map"], info["maps"], info["pushes"]) == (0, 0, 0) and info["device_bytes"] >= 12 * w * h
        self.mout, self.pout = map_outputs(w, h, pad), push_outputs(p, w, h, pad)
        self.last_map = self.last_push = None

    def read_is(self, what):
        recs, table, ps, ms = self.ctx.offshore_read(stream=self.stream)
        if self.last_map is not None:
            assert [ms[k] for k in OFFSHORE_MAP_SUMMARY] == [int(v) for v in self.last_map["summary"]], "the slot's map summary differs " + what
        if self.last_push is not None:
            assert same("stations", recs, self.last_push["stations"]), "the slot's records differ " + what
            assert np.array_equal(table.reshape(-1, R.SUMS), self.last_push["table"]), "the slot's table differs " + what
            assert [ps[k] for k in OFFSHORE_PUSH_SUMMARY] == [int(v) for v in self.last_push["summary"]], "the slot's push summary differs " + what

    def map(self, wet, what="", only=None):
        want = self.last_map = self.ref.map(wet)
        d = dev(wet, self.pad)
        self.ctx.offshore_map(d.view, stream=self.stream, **self.mout.kw(only))
        got = self.mout.host()
        what = "after map %d %s" % (self.ref.maps, what)
        compare(got if only is None else {k: got[k] for k in only}, want, what)
        self.read_is(what)
        assert np.array_equal(d.view.cpu().numpy(), wet), "the wet mask was written"
        d.check("the wet mask")
        info = self.ctx.offshore_info(stream=self.stream)
        assert (info["have_map"], info["maps"]) == (1, self.ref.maps)
        return want

    def push(self, flow, what="", only=None):
        want = self.last_push = self.ref.push(flow)
        d = dev(flow, self.pad)
        self.ctx.offshore_push(d.view, stream=self.stream, **self.pout.kw(only))
        got = self.pout.host()
        what = "after push %d %s" % (self.ref.pushes, what)
        compare(got if only is None else {k: got[k] for k in only}, want, what)
        self.read_is(what)
        assert np.ascontiguousarray(d.view.cpu().numpy()).tobytes() == np.ascontiguousarray(flow).tobytes(), "the field was written"
        d.check("the field")
        assert self.ctx.offshore_info(stream=self.stream)["pushes"] == self.ref.pushes
        return want

    def band(self, lo, hi):
        out = Padded.empty((self.h, self.w), torch.uint8, self.pad)
        self.ctx.offshore_band(lo, hi, out.view, stream=self.stream)
        want = self.ref.band(lo, hi)
        assert np.array_equal(out.view.cpu().numpy(), want), "the band %s..%s differs" % (lo, hi)
        out.check("the band")
        return want

    def close(self):
        self.ctx.offshore_close(stream=self.stream)


def once(ctx, w, h, p, wet, flow, pad=0, bands=((0, 3), (2.5, 11.25))):
    s = Session(ctx, w, h, p, pad)
    m = s.map(wet, "(%d x %d)" % (w, h))
    q = s.push(flow, "(%d x %d, %s)" % (w, h, p))
    b = [s.band(lo, hi) for lo, hi in bands]
    s.close()
    return m, q, b


def long_shore(w, h):
    """all water but two dry pixels far apart along the long side: the walk along a row passes several tiles, the nearest rows of a
    column lie hundreds of rows away"""
    wet = np.full((h, w), 255, np.uint8)
    if w >= h:
        wet[2 % h, 3] = wet[h - 1, 900] = 0
    else:
        wet[3, 2 % w] = wet[900, w - 1] = 0
    return wet


# ---------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("w,h", [(67, 45), (96, 64), (1, 40), (40, 1), (1100, 5), (5, 1100), (OF_TILE + 1, 9)])
def test_sizes_with_padded_steps(ctx, w, h):
    """67 x 45: odd, smaller than a tile; 96 x 64: the prototype's; a column and a row; 1100 x 5 and 5 x 1100: a row and a column
    longer than any one tile, with walks of hundreds of pixels; 257 x 9: one pixel into the second tile"""
    if max(w, h) >= 1000:
        wet, p = long_shore(w, h), with_(GENERAL, min_dist=0, max_dist=1000, bin_width=100, stations=min(5, w, h) if w < h else 5, station="x")
    elif min(w, h) == 1:
        wet, p = R.speckle(w, h, 0.7, 5), with_(GENERAL, min_dist=1, stations=1, min_count=1)
    else:
        wet, p = R.beach(w, h, h / 3.0, 4.0, 48.0), GENERAL
    m, q, b = once(ctx, w, h, p, wet, R.wavy_field(w, h), pad=3)
    assert m["summary"][2] > 0 and q["summary"][R.OK] > 0 and q["table"][:, 0].sum() > 0
    if max(w, h) >= 1000:
        assert m["summary"][3] > 400 ** 2                         # a nearest pixel more than a tile away


def test_the_prototype(ctx):
    w, h, wet, flow, p = R.prototype()
    m, q, b = once(ctx, w, h, p, wet, flow, pad=1, bands=((10, 25),))
    assert list(m["summary"][:6]) == [4224, 1920, 4224, 2074, 2517482, 245999]
    assert list(q["summary"]) == [3745, 253, 225, 1920, 1, 458, 1, 1] and list(q["stations"]["reach_end"]) == [0, 0, 0, 0, 8, 0, 0, 0]
    assert (b[0] != 0).sum() == 1507


# ---------------------------------------------------------------------------- shores
@pytest.mark.parametrize("share", [0.5, 0.99])
def test_random_shores_for_ties_and_long_searches(ctx, share):
    w, h = 130, 131
    wet = R.speckle(w, h, share, 11)
    m, q, b = once(ctx, w, h, with_(GENERAL, min_dist=0, stations=7, min_count=1), wet, R.wavy_field(w, h, 1), pad=2)
    if share == 0.99:
        assert m["summary"][3] >= 100                             # somewhere the nearest land is ten pixels away


@pytest.mark.parametrize("corner", [(0, 0), (44, 66)])
def test_a_single_dry_pixel_in_a_corner(ctx, corner):
    w, h = 67, 45
    wet = np.full((h, w), 255, np.uint8)
    wet[corner] = 0
    m, q, b = once(ctx, w, h, with_(GENERAL, max_dist=100, bins=20), wet, R.wavy_field(w, h), pad=1)
    assert m["summary"][3] == 66 ** 2 + 44 ** 2 and (m["near"][wet != 0] == corner[0] * w + corner[1]).all()


@pytest.mark.parametrize("value", [255, 0])
def test_all_wet_and_all_dry_are_far(ctx, value):
    w, h = 67, 45
    m, q, b = once(ctx, w, h, GENERAL, np.full((h, w), value, np.uint8), R.wavy_field(w, h), pad=1)
    assert (np.abs(m["dist2"]) == R.FAR).all() and (m["near"] == -1).all() and q["summary"][R.C_FAR if value else R.DRY] == w * h
    assert (q["stations"]["flags"] == R.EMPTY).all() and not b[0].any()


@pytest.mark.parametrize("edge", ["top row", "right column", "bottom right pixel wet"])
def test_a_shore_on_the_pictures_edge(ctx, edge):
    w, h = 67, 45
    wet = np.full((h, w), 255, np.uint8)
    if edge == "top row":
        wet[0, :] = 0
    elif edge == "right column":
        wet[:, w - 1] = 0
    else:
        wet[:] = 0
        wet[h - 1, w - 1] = 255
    once(ctx, w, h, with_(GENERAL, min_dist=1, station="y" if edge == "right column" else "x"), wet, R.wavy_field(w, h), pad=1)


# ---------------------------------------------------------------------------- fields and parameters
def test_hostile_field(ctx):
    """NaN, +-inf, +-500.0, +-499.99 and -0.0"""
    w, h = 67, 45
    f = R.hostile(R.wavy_field(w, h), seed=4)
    f[20, 5], f[21, 6], f[22, 7], f[23, 8] = (np.nan, 1), (1, np.inf), (500.0, 0), (0, -499.99)
    m, q, b = once(ctx, w, h, with_(GENERAL, cross_min=100.0), R.beach(w, h, 15.0), f, pad=2)
    assert q["summary"][R.BAD] >= 3 and q["cls"][23, 8] == R.OK and q["cls"][22, 7] == R.BAD and np.abs(q["sides"]["cross"]).max() > 30000


@pytest.mark.parametrize("kw", [dict(min_dist=0), dict(min_dist=30), dict(max_dist=7), dict(max_dist=4095, bins=256, bin_width=1), dict(station="y"),
                                dict(station="y", stations=45), dict(stations=256), dict(cross_min=0.0), dict(cross_min=400.0), dict(bin_width=256),
                                dict(min_count=1000), dict(rip_bins=6)])
def test_parameters(ctx, kw):
    """min_dist 0 and max_dist; max_dist below the largest distance; a station per row and more stations than columns; bins a pixel
    wide; the ends of cross_min"""
    w, h = 67, 45
    p = with_(GENERAL, **kw)
    m, q, b = once(ctx, w, h, p, R.beach(w, h, 15.0), R.jet_field(w, h, 30, 40, (0.5, -0.25), (0.25, 3.0)), pad=1)
    if kw == dict(max_dist=7):
        assert m["summary"][3] > 49 and q["summary"][R.C_FAR] > 0
    if kw == dict(min_dist=0):
        assert q["summary"][R.NEAR] == 0
    if kw == dict(cross_min=0.0):
        assert (q["picture"][q["cls"] == R.OK] != 255).any()


def test_each_output_alone_and_none(ctx):
    """what a call asks for changes nothing of what it gives"""
    w, h = 67, 45
    s = Session(ctx, w, h, GENERAL, pad=2)
    wet, f = R.beach(w, h, 15.0), R.wavy_field(w, h)
    for only in [()] + [(k,) for k in R.MAP_PLANES + ("summary",)] + [None]:
        s.map(np.roll(wet, s.ref.maps, axis=1), "asking %s" % (only,), only=only)
    for only in [()] + [(k,) for k in R.PUSH_PLANES + ("stations", "table", "summary")] + [None]:
        s.push(f + np.float32(0.25 * s.ref.pushes), "asking %s" % (only,), only=only)
    s.close()


def test_a_second_map_after_pushes_set_reset_and_reopen(ctx):
    w, h = 67, 45
    s = Session(ctx, w, h, GENERAL, pad=1)
    f = R.jet_field(w, h, 30, 40, (0.5, -0.25), (0.25, 3.0))
    s.map(R.beach(w, h, 15.0))
    first = s.push(f)
    s.push(R.wavy_field(w, h))
    s.map(R.beach(w, h, 25.0, 6.0, 30.0), "(the shore has moved)")
    second = s.push(f)
    assert not np.array_equal(first["table"], second["table"]) and second["summary"][7] == 3
    p2 = with_(GENERAL, min_dist=0, max_dist=20, bin_width=3, min_count=1, rip_bins=1, cross_min=2.0, station="y")
    ctx.offshore_set(**{k: v for k, v in p2.kw().items() if k not in ("stations", "bins")})
    s.ref.set(p2)
    info = ctx.offshore_info()
    assert [info[k] for k in ("min_dist", "max_dist", "stations", "bins", "bin_width", "min_count", "rip_bins", "cross_min", "station")] == \
        [0, 20, 5, 6, 3, 1, 1, 2.0, "y"] and info["pushes"] == 3
    third = s.push(f, "(after set)")
    assert third["summary"][R.NEAR] == 0
    s.map(R.beach(w, h, 25.0, 6.0, 30.0), "(the picture by the new max_dist)")
    ctx.offshore_reset()
    s.ref.reset()
    recs, table, ps, ms = ctx.offshore_read()
    assert not recs.view(np.uint8).any() and not table.any() and not any(ps.values()) and not any(ms.values())
    info = ctx.offshore_info()
    assert (info["have_map"], info["maps"], info["pushes"], info["max_dist"], info["station"]) == (0, 0, 0, 20, "y")
    with pytest.raises(RcflowError) as e:
        ctx.offshore_push(dev(f).view)
    assert e.value.code == ESTATE                                 # the map was forgotten
    with pytest.raises(RcflowError) as e:
        ctx.offshore_band(0, 5)
    assert e.value.code == ESTATE
    s.last_map = s.last_push = None
    s.map(R.beach(w, h, 15.0), "(after the reset)")
    s.push(f, "(after the reset)")
    s.close()
    s = Session(ctx, w + 3, h + 2, with_(GENERAL, stations=3, bins=4))          # a re-open with other sizes
    s.map(R.beach(w + 3, h + 2, 15.0))
    s.push(R.wavy_field(w + 3, h + 2))
    s2 = Session(ctx, w, h, GENERAL)                              # over the open one
    s2.map(R.beach(w, h, 15.0))
    s2.push(f)
    s2.close()


def test_two_slots_interleaved(ctx):
    (wa, ha), (wb, hb) = (67, 45), (40, 33)
    a, b = Session(ctx, wa, ha, GENERAL, stream=0), Session(ctx, wb, hb, with_(GENERAL, station="y", stations=3), pad=1, stream=1)
    a.map(R.beach(wa, ha, 15.0))
    b.map(R.speckle(wb, hb, 0.9, 3))
    for t in range(2):
        a.push(R.wavy_field(wa, ha, t), "slot 0")
        b.push(R.wavy_field(wb, hb, t), "slot 1")
    b.close()
    assert ctx.offshore_info(stream=0)["pushes"] == 2
    a.close()


def test_launch_counts_against_the_profile(ctx):
    w, h = 67, 45
    s = Session(ctx, w, h, GENERAL)
    wet, f = dev(R.beach(w, h, 15.0)).view, dev(R.wavy_field(w, h)).view
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(2):
        ctx.offshore_map(wet)
    for _ in range(3):
        ctx.offshore_push(f)
    ctx.offshore_band(1, 9)
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    ctx.profile_enable(False)
    info = ctx.offshore_info()
    assert prof == {"offshore@0": 2, "offshore@1": 2, "offshore@2": 2, "offshore@3": 3, "offshore@4": 3, "offshore@5": 1}, prof
    assert sum(v for k, v in prof.items() if k in ("offshore@0", "offshore@1", "offshore@2")) == info["launches_per_map"] * info["maps"]
    assert prof["offshore@3"] + prof["offshore@4"] == info["launches_per_push"] * info["pushes"]
    s.close()


def test_product_object(ctx):
    w, h = 67, 45
    ref = R.OffshoreRef(w, h, GENERAL, ctx.jet_lut())
    wet, f = R.beach(w, h, 15.0), R.wavy_field(w, h)
    with Offshore(ctx, w, h, **GENERAL.kw()) as o:
        ca = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
        sd = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        o.map(dev(wet).view, sdist=sd)
        o.push(dev(f).view, cross_along=ca)
        wm, wp = ref.map(wet), ref.push(f)
        recs, table, ps, ms = o.read()
        assert same("stations", recs, wp["stations"]) and ps["pushes"] == 1 and ms["wet"] == int(wm["summary"][0])
        assert same_bits(ca.cpu().numpy(), wp["cross_along"]) and np.array_equal(sd.cpu().numpy(), wm["sdist"])
        assert np.array_equal(o.band(2, 9).cpu().numpy(), ref.band(2, 9))
        with pytest.raises(ValueError):
            o.push(dev(f[:, :-1]).view)                           # a field of another size
        o.set(0, 12, 2, 1, 1, 0.25, "y")
        o.reset()
        info = o.info()
        assert (info["have_map"], info["max_dist"], info["station"], info["stations"]) == (0, 12, "y", 5)
    with pytest.raises(RcflowError):
        ctx.offshore_info()


# ---------------------------------------------------------------------------- the chain
def test_chain_shoreline_map_meanflow_push_regions_and_band_zones(ctx):
    """End to end on synth.surf_clip(160, 120): the shoreline's wet mask of a frame goes into the map as it is; the frame loop's
    Farneback fields go through the mean current, whose mean field goes into the push, and the resident field itself too (d_flow_xy
    NULL); the push's mask goes into the regions, the band into the drifters' zones helper.  Each hand-over equals the statements.
    What it finds is printed, not asserted"""
    w, h = 160, 120
    clip = synth.surf_clip(w, h, 4)
    lut = ctx.jet_lut()
    # the shoreline's wet mask
    sp, lines = S.Params(source=S.GRAY, radius=2, window=2), S.beach_lines(w, h)
    bgr = np.ascontiguousarray(np.stack([clip[0]] * 3, -1))
    ctx.shoreline_open(w, h, lines, **sp.kw())
    wet = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    ctx.shoreline_push(dev(bgr).view, mask=wet)
    want_wet = S.ShorelineRef(w, h, lines, sp).push(bgr)["mask"]
    assert np.array_equal(wet.cpu().numpy(), want_wet) and 0 < (want_wet != 0).sum() < w * h
    ctx.shoreline_close()
    # the map
    p = R.Params(min_dist=1, max_dist=30, stations=8, bins=6, bin_width=3, min_count=8, rip_bins=2, cross_min=0.125, station="x")
    ref = R.OffshoreRef(w, h, p, lut)
    ctx.offshore_open(w, h, **p.kw())
    mout, pout = map_outputs(w, h), push_outputs(p, w, h)
    ctx.offshore_map(wet, **mout.kw())
    wm = ref.map(want_wet)
    compare(mout.host(), wm, "(the shoreline's mask)")
    # the mean current of the frame loop's fields, and the resident field itself
    mp = M.Params(window=2, grid_x=4, grid_y=3, min_fill=1, steady_min=300, flags=M.DIR_OPPOSED, speed_min=0.1, min_cos2=0.25)
    mref = M.MeanFlowRef(w, h, mp, lut)
    ctx.meanflow_open(w, h, **mp.kw())
    mean = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    ctx.stream_reset()
    assert ctx.push_frame_host(clip[0]) is None
    for t in range(1, 4):
        flow = ctx.push_frame_host(clip[t]).cpu().numpy()
        ctx.meanflow_push(None, mean=mean)
        wmean = mref.push(flow)["mean"]
    assert same_bits(mean.cpu().numpy(), wmean)
    ctx.offshore_push(None, **pout.kw())
    compare(pout.host(), ref.push(flow), "(the resident Farneback field)")
    ctx.offshore_push(mean, **pout.kw())
    wp = ref.push(wmean)
    got = pout.host()
    compare(got, wp, "(the mean current's field)")
    # the mask into the regions
    ctx.regions_open(w, h, connectivity=8, min_area=6, max_regions=64)
    ctx.regions_push(pout.t["mask"])
    rec, summ = ctx.regions_read()
    wr = RG.regions(wp["mask"], 8, 6, 64, None, 1)
    assert summ["kept"] == int(wr["summary"][1]) and np.array_equal(rec["area"], wr["records"]["area"][:len(rec)])
    ctx.regions_close()
    # the band into the drifters' zones
    band = ctx.offshore_band(2, 12)
    wband = ref.band(2, 12)
    assert np.array_equal(band.cpu().numpy(), wband)
    zone = ctx.drifters_zones(wet, band)
    assert np.array_equal(zone.cpu().numpy(), D.zones(want_wet, wband))
    st = wp["stations"]
    print("wet %d of %d pixels, largest distance %.1f px; OK %d, mask %d, regions %d; stations flagged %s, reach_end %s; band 2..12 px: %d pixels"
          % (wm["summary"][0], w * h, np.sqrt(float(wm["summary"][3])), wp["summary"][0], wp["summary"][5], summ["kept"],
             [int(v) for v in np.nonzero(st["flags"] & R.RIP)[0]], [int(v) for v in st["reach_end"]], (wband != 0).sum()))
    ctx.offshore_open(128, 96, **p.kw())
    ctx.offshore_map(dev(R.beach(128, 96)).view)
    with pytest.raises(RcflowError) as e:
        ctx.offshore_push(None)
    assert e.value.code == ESIZE                                  # the resident field has another size
    ctx.stream_reset()
    with pytest.raises(RcflowError) as e:
        ctx.offshore_push(None)
    assert e.value.code == ESTATE and ctx.offshore_info()["pushes"] == 0
    ctx.offshore_close()
    ctx.meanflow_close()


# ---------------------------------------------------------------------------- arguments and refusals
def test_refusals_leave_state_and_outputs_untouched(ctx):
    w, h = 40, 24
    good = with_(GENERAL, stations=4, bins=5)
    ns, nb = good.stations, good.bins
    ctx.offshore_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.offshore_info, ctx.offshore_read, ctx.offshore_reset, lambda: ctx.offshore_band(0, 1)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 1024)()
    okp = OffshoreParams(min_dist=2, max_dist=30, stations=4, bins=5, bin_width=4, min_count=3, rip_bins=2, cross_min=0.5, flags=1)
    for name, args in (("info", (C.byref(OffshoreInfo()),)), ("read", (buf, buf, buf, buf)), ("reset", ()), ("set", (C.byref(okp),)),
                       ("map_dev", (null, 0) * 5 + (null,)), ("push_dev", (null, 0) * 5 + (null, null, null)), ("band_dev", (0.0, 1.0, null, 0))):
        assert getattr(lib, "rcflow_offshore_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_offshore_%s:" % name), text()
    kw = good.kw()
    bads = (dict(min_dist=-1), dict(min_dist=31), dict(max_dist=0), dict(max_dist=4096), dict(stations=0), dict(stations=257), dict(bins=0),
            dict(bins=257), dict(bin_width=0), dict(bin_width=257), dict(min_count=0), dict(rip_bins=0), dict(rip_bins=6), dict(cross_min=-0.5),
            dict(cross_min=400.5), dict(cross_min=float("nan")), dict(cross_min=float("inf")))
    for bad in bads:
        assert R.params_error(with_(good, **bad)) == "parameters"
        with pytest.raises(RcflowError) as e:
            ctx.offshore_open(w, h, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_offshore_open"), bad
    p = OffshoreParams(min_dist=2, max_dist=30, stations=4, bins=5, bin_width=4, min_count=3, rip_bins=2, cross_min=0.5, flags=0)
    for flags in (0, 3, 4):                                       # neither station rule, both, an unknown one
        p.flags = flags
        assert lib.rcflow_offshore_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "exactly one" in text()
    p.flags = 1
    p.pad[2] = 1
    assert lib.rcflow_offshore_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "pad" in text()
    p.pad[2] = 0
    assert lib.rcflow_offshore_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_offshore_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_offshore_open(hdl, 2, w, h, C.byref(p)) == EINVAL            # no such slot
    with pytest.raises(RcflowError) as e:
        ctx.offshore_open(4000, 2161, **kw)                       # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_offshore_open")
    with pytest.raises(RcflowError):
        ctx.offshore_info()                                       # nothing was left open by any of them

    s = Session(ctx, w, h, good, pad=2)
    wets = [R.beach(w, h, 8.0 + 3 * t, 3.0, 20.0) for t in range(3)]
    f = R.wavy_field(w, h)
    dw, df = [dev(x) for x in wets], dev(f)
    with pytest.raises(RcflowError) as e:
        ctx.offshore_push(df.view)                                # before any map
    assert e.value.code == ESTATE and text().startswith("rcflow_offshore_push_dev")
    first_map = s.map(wets[0], "(before the refusals)")
    first = s.push(f, "(before the refusals)")
    assert lib.rcflow_offshore_info(hdl, 0, None) == EINVAL
    before = ctx.offshore_info()
    for bad in (dict(max_dist=5000), dict(rip_bins=9)):           # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.offshore_open(w, h, **dict(kw, **bad))
    assert ctx.offshore_info() == before
    big = torch.zeros(64 * h * w + 4096, dtype=torch.uint8, device="cuda")
    N = (null, 0)
    mo, po = s.mout.t, s.pout.t

    def im(t, off=0, step=None):
        return (ptr(t, off), t.stride(0) * t.element_size() if step is None else step)

    def map_(wet=None, dist2=N, near=N, sdist=N, pic=N, summ=null, slot=0):
        return lib.rcflow_offshore_map_dev(hdl, slot, *(wet or im(dw[1].view)), *dist2, *near, *sdist, *pic, summ)

    def push(flow=None, ca=N, cls=N, mask=N, pic=N, recs=null, table=null, summ=null, slot=0):
        return lib.rcflow_offshore_push_dev(hdl, slot, *(flow or im(df.view)), *ca, *cls, *mask, *pic, recs, table, summ)

    def band(lo=1.0, hi=5.0, out=None):
        return lib.rcflow_offshore_band_dev(hdl, 0, lo, hi, *(out or (ptr(big), w)))

    refused = [
        map_(wet=N), map_(wet=im(dw[1].view, step=w - 1)),
        map_(dist2=im(mo["dist2"], 2)), map_(dist2=im(mo["dist2"], step=4 * w + 2)), map_(near=im(mo["near"], step=4 * w - 4)),
        map_(sdist=im(mo["sdist"], 1)), map_(pic=im(mo["picture"], step=3 * w - 1)), map_(summ=ptr(big, 4)),
        map_(dist2=im(mo["dist2"]), near=im(mo["dist2"])),        # two outputs in one place
        map_(wet=(ptr(big), w), sdist=(ptr(big, 4 * w), 4 * w)),  # an output over the mask's last rows
        map_(near=(ptr(big), 4 * w), summ=ptr(big, 4 * w * h - 8)), map_(pic=(ptr(big), 3 * w), dist2=(ptr(big, 3 * w * h - 4), 4 * w)),
        push(flow=im(df.view, step=8 * w - 8)), push(flow=im(df.view, step=8 * w + 4)), push(flow=im(df.view, 4)),
        push(ca=im(po["cross_along"], 4)), push(ca=im(po["cross_along"], step=8 * w + 4)), push(ca=im(po["cross_along"], step=8 * w - 8)),
        push(cls=im(po["cls"], step=w - 1)), push(mask=im(po["mask"], step=w - 1)), push(pic=im(po["picture"], step=3 * w - 1)),
        push(recs=ptr(big, 2)), push(table=ptr(big, 4)), push(summ=ptr(big, 4)),
        push(ca=im(df.view)),                                     # d_cross_along over the field
        push(cls=(ptr(big), w), mask=(ptr(big, w * (h - 1)), w)), # two outputs meeting in one row
        push(ca=(ptr(big), 8 * w), pic=(ptr(big, 8), 3 * w)), push(recs=ptr(big), table=ptr(big, 48 * ns - 8)),
        push(table=ptr(big), summ=ptr(big, 32 * ns * nb - 8)), push(pic=(ptr(big), 3 * w), summ=ptr(big)),
        band(out=N), band(out=(ptr(big), w - 1)), band(lo=-1.0), band(lo=6.0, hi=5.0), band(hi=70000.0), band(lo=float("nan")), band(hi=float("inf")),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert map_(slot=2) == EINVAL and push(slot=2) == EINVAL
    sets = [dict(p=None), dict(stations=5), dict(bins=4), dict(max_dist=0), dict(min_dist=31), dict(rip_bins=6), dict(cross_min=401.0), dict(flags=3), dict(flags=0)]
    for bad in sets:
        q = OffshoreParams(min_dist=2, max_dist=30, stations=4, bins=5, bin_width=4, min_count=3, rip_bins=2, cross_min=0.5, flags=1)
        for k, v in bad.items():
            if k != "p":
                setattr(q, k, v)
        assert lib.rcflow_offshore_set(hdl, 0, None if "p" in bad else C.byref(q)) == EINVAL and text().startswith("rcflow_offshore_set"), bad
    assert ctx.offshore_info() == before and not big.any()
    # the outputs of the calls before stand as they were, with their fences; the slot's copies too
    compare(s.mout.host(), first_map, "(after the refusals)")
    compare(s.pout.host(), first, "(after the refusals)")
    s.read_is("(after the refusals)")
    # nothing was queued and nothing changed: the map is still the first one
    s.push(f + np.float32(0.5), "(the push after the refusals)")
    s.map(wets[1], "(the map after the refusals)")
    # a slot moved to another stream between calls
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s.map(wets[2], "(on another stream)")
        s.push(f, "(on another stream)")
        s.band(1, 6)
    torch.cuda.synchronize()
    ctx.offshore_close()                                          # closing twice is fine
    ctx.offshore_close()
