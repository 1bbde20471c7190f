"""The virtual drifters on the device (drifters_kernels.hip) against their numpy statement (tests/_drifters_ref.py): the pictures, the
per-drifter arrays, the records, both tables, the histograms and the summary of every push, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _drifters_ref as D
import _flowcheck_ref as F
import _regions_ref as RG
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, Outputs, Padded, ptr, raw, same_bits
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RC_DRIFTERS_LAUNCHES, DriftersInfo, DriftersParams, RcflowError
from ripcurrents_amd.api import DRIFTERS_CELL_DTYPE, DRIFTERS_SUMMARY, Drifters

pytestmark = pytest.mark.gpu

IMAGES = D.PIXEL_OUTPUTS
PER_DRIFTER = D.DRIFTER_OUTPUTS
ARRAYS = ("cells", "place", "origin", "hist", "summary")
dev = Padded.of


def outputs(p, w, h, n, pad=0, only=None):
    nc = p.grid_x * p.grid_y
    planes = dict(now=((h, w), torch.int16), density=((h, w), torch.int32), live=((h, w), torch.uint8), picture=((h, w, 3), torch.uint8))
    flat = dict(xy=((2 * n,), torch.float32, None), age=((n,), torch.int32, None), state=((n,), torch.uint8, None),
                cells=((nc * 32,), torch.uint8, None), place=((nc * D.SUMS,), torch.int64, -1), origin=((nc * D.SUMS,), torch.int64, -1),
                hist=((4 * D.HIST_BINS,), torch.int64, -1), summary=((D.SUMMARY_WORDS,), torch.int64, -1))
    if only is not None:
        planes = {k: v for k, v in planes.items() if k in only}
        flat = {k: v for k, v in flat.items() if k in only}

    def views(d):
        for k, f in (("now", lambda a: a.view(np.uint16)), ("density", lambda a: a.view(np.uint32)), ("xy", lambda a: a.reshape(-1, 2)),
                     ("cells", lambda a: a.view(DRIFTERS_CELL_DTYPE)), ("place", lambda a: a.reshape(-1, D.SUMS)),
                     ("origin", lambda a: a.reshape(-1, D.SUMS)), ("hist", lambda a: a.view(np.uint64).reshape(4, D.HIST_BINS))):
            if k in d:
                d[k] = f(d[k])
    return Outputs(planes, flat, pad, views)


def same(k, a, b):
    if k == "xy":
        return same_bits(a, b)
    if k == "cells":
        return all(a[f].tobytes() == b[f].tobytes() for f in b.dtype.names)
    return np.array_equal(a, b)


def compare(got, read, want, what):
    for k in got:
        assert same(k, got[k], want[k]), "%s differs %s: %s, wanted %s" % (k, what, got[k], want[k])
    if read is not None:
        rc, rp, ro, rh, rsum = read
        assert same("cells", rc.ravel(), want["cells"]), "the slot's records differ " + what
        assert np.array_equal(rp.reshape(-1, D.SUMS), want["place"]) and np.array_equal(ro.reshape(-1, D.SUMS), want["origin"]), "the slot's tables differ " + what
        assert np.array_equal(rh, want["hist"]), "the slot's histograms differ " + what
        assert [rsum[k] for k in DRIFTERS_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


class Session:
    """the device session and the statement side by side"""

    def __init__(self, ctx, w, h, p, pad=0, stream=0):
        self.ctx, self.w, self.h, self.p, self.pad, self.stream = ctx, w, h, p, pad, stream
        self.ref = D.DriftersRef(w, h, p, ctx.jet_lut())
        ctx.drifters_open(w, h, stream=stream, **p.kw())
        info = ctx.drifters_info(stream=stream)
        assert info["launches_per_push"] == RC_DRIFTERS_LAUNCHES == 2 and info["drifters"] == 0 and info["device_bytes"] >= 24 * p.max_drifters + 8 * w * h
        self.cache, self.out, self.wants = {}, None, []

    def seed(self, homes):
        assert self.ref.seed(homes)
        self.ctx.drifters_seed(homes, stream=self.stream)
        self.out = outputs(self.ref.p, self.w, self.h, self.ref.n, self.pad)

    def up(self, a):
        if a is None:
            return None
        if id(a) not in self.cache:
            self.cache[id(a)] = (dev(a, self.pad), a)
        return self.cache[id(a)][0].view

    def push(self, flow, zone=None, what=""):
        want = self.ref.push(flow, zone)
        self.ctx.drifters_push(self.up(flow), self.up(zone), stream=self.stream, **self.out.kw())
        compare(self.out.host(), self.ctx.drifters_read(stream=self.stream), want, "after push %d %s" % (self.ref.pushes, what))
        info = self.ctx.drifters_info(stream=self.stream)
        assert (info["drifters"], info["pushes"]) == (self.ref.n, self.ref.pushes)
        self.wants.append(want)
        return want

    def close(self):
        for d, a in self.cache.values():
            assert d.view.cpu().numpy().tobytes() == a.tobytes(), "an input was written"
            d.check("an input")
        self.ctx.drifters_close(stream=self.stream)


def homes_in(w, h, n, seed=1):
    """n homes in raster order of a random draw: neighbours in memory are near each other on the picture"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1)
    return xy[np.lexsort((xy[:, 0], np.floor(xy[:, 1] / 4)))]


def rotation(w, h, scale=0.04):
    return np.ascontiguousarray(synth.rotation_field(w, h) * np.float32(scale))


def surf(w, h):
    return D.field(*synth.surf_field(w, h))


def bands(w, h, top=2, bottom=3):
    z = np.zeros((h, w), np.uint8)
    z[:top], z[h - bottom:] = 2, 1
    return z


# ---------------------------------------------------------------------------- counts, pictures, fields
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_drifter_counts(ctx, n):
    """a wave less one, a wave, a wave and one, a block and one, four blocks less some: the rotation carries them across cells and
    over the edges, RESPAWN brings them back"""
    w, h = 37, 29
    s = Session(ctx, w, h, D.Params(max_drifters=n, grid_x=5, grid_y=4, max_age=9, age_bin=2, flags=D.RESPAWN), pad=3)
    s.seed(homes_in(w, h, n, seed=n))
    f, z = rotation(w, h, 0.12), bands(w, h)
    for _ in range(14):
        s.push(f, z)
    last = s.wants[-1]["summary"]
    assert last[8 + D.AGED] + last[8 + D.SHORE] + last[8 + D.OFFSHORE] + last[9:13].sum() > 0 and last[2] > n
    s.close()


@pytest.mark.parametrize("w,h", [(37, 29), (131, 67)])
@pytest.mark.parametrize("name", ["uniform", "rotation", "surf", "hostile"])
def test_pictures_and_fields(ctx, w, h, name):
    """widths that are no multiple of 4 with padded steps; a uniform field (1.25, -0.75), the rotation, the synthetic rip, and a field
    with NaN, infinities, +-500.0, the float below it and -0.0"""
    f = dict(uniform=lambda: D.uniform_field(w, h, 1.25, -0.75), rotation=lambda: rotation(w, h), surf=lambda: surf(w, h),
             hostile=lambda: D.hostile_field(w, h, seed=w))[name]()
    s = Session(ctx, w, h, D.Params(max_drifters=600, grid_x=4, grid_y=3, max_age=25, age_bin=3, density_full=5, live_min=2, flags=D.RESPAWN), pad=5)
    s.seed(homes_in(w, h, 600, seed=h))
    z = bands(w, h)
    for _ in range(12):
        s.push(f, z, name)
    want = s.wants[-1]
    assert want["picture"].any() and want["live"].any() and (want["density"] > 1).any()
    if name == "hostile":
        assert want["summary"][8 + D.BAD] > 0
    if name == "uniform":
        assert want["summary"][8 + D.EDGE_RIGHT] + want["summary"][8 + D.EDGE_TOP] + want["summary"][8 + D.OFFSHORE] > 0
    s.close()


def test_converging_field_4096_on_one_pixel(ctx):
    """every vector points at pixel (60, 30): after some pushes whole waves sit on one pixel and in one cell, the form in which a
    wave issues one atomic"""
    w, h, n = 131, 67, 4096
    s = Session(ctx, w, h, D.Params(max_drifters=n, grid_x=6, grid_y=5, density_full=40000), pad=1)
    s.seed(D.lattice(np.linspace(0, w - 1, 64), np.linspace(0, h - 1, 64)))
    f = D.converging_field(w, h, 60, 30)
    for _ in range(18):
        want = s.push(f)
    assert want["now"][30, 60] == n and want["summary"][1] == n and want["density"][30, 60] > 4 * n
    s.close()


def test_499_pixels_at_dt_256_needs_the_int64_product(ctx):
    w, h = 64, 9
    f = np.zeros((h, w, 2), np.float32)
    f[:, :32, 0], f[:, 32:, 0] = 499.0, -499.0
    f[4:, :, 1] = 0.01                                            # q = 1, D dt_q below 2^19: a step of 0 at dt 1/256
    s = Session(ctx, w, h, D.Params(max_drifters=128, dt=256.0), pad=2)
    s.seed(homes_in(w, h, 128))
    s.push(f)
    want = s.push(f)
    left, right = s.ref.HX <= 31 * 64, s.ref.HX >= 32 * 64        # between columns 31 and 32 the two mix
    assert left.any() and right.any() and (want["step"][left, 0] == 31936 * 256).all() and (want["step"][right, 0] == -31936 * 256).all()
    assert (s.ref.st[left] == D.EDGE_RIGHT).all() and (s.ref.st[right] == D.EDGE_LEFT).all()
    s.close()
    s = Session(ctx, w, h, D.Params(max_drifters=128, dt=1 / 256), pad=2)
    s.seed(homes_in(w, h, 128))
    for _ in range(3):
        want = s.push(f)
    assert want["summary"][1] == 128 and np.abs(want["step"][:, 0]).max() == 125 and not want["step"][:, 1].any()      # (4096 * 31936 + 2^19) >> 20
    s.close()


def test_occupancy_saturates_at_65535(ctx):
    """70 000 drifters on one home in a zero field: d_now saturates, the density takes 70 000 a push"""
    w, h, n = 16, 8, 70000
    s = Session(ctx, w, h, D.Params(max_drifters=n, grid_x=2, grid_y=2, density_full=1 << 20, live_min=65536))
    s.seed(np.tile([[5.25, 3.5]], (n, 1)))
    f = np.zeros((h, w, 2), np.float32)
    for k in range(3):
        want = s.push(f)
        assert want["now"][4, 5] == 65535 and want["density"][4, 5] == n * (k + 1) and want["live"][4, 5] == 255 and want["place"][:, 0].sum() == n * (k + 1)
    s.close()


# ---------------------------------------------------------------------------- zones
def test_zones_none_constructed_and_bytes_above_7(ctx):
    w, h = 37, 29
    f = rotation(w, h, 0.08)
    z = np.zeros((h, w), np.uint8)
    z[:3], z[-3:], z[10:14, 5:9], z[10:14, 20:24], z[20:23, 30:] = 2, 1, 7, 8, 255
    z[15, 15:18] = (3, 4, 6)
    s = Session(ctx, w, h, D.Params(max_drifters=500, grid_x=3, grid_y=3, flags=D.RESPAWN), pad=2)
    s.seed(homes_in(w, h, 500))
    for k in range(16):
        want = s.push(f, None if k < 4 else z)
    sm = want["summary"]
    assert s.wants[3]["summary"][16:].sum() == 0 and sm[8 + 15] > 0 and sm[8 + D.SHORE] > 0 and sm[8 + D.OFFSHORE] > 0 and sm[8 + 7] == 0 and sm[8] == 0
    s.close()


@pytest.mark.parametrize("which", ["both", "wet", "inside"])
def test_zones_helper(ctx, which):
    w, h = 131, 67
    rng = np.random.default_rng(4)
    wet = np.where(rng.random((h, w)) < 0.6, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    inside = np.where(rng.random((h, w)) < 0.5, 255, 0).astype(np.uint8)
    a, b = (wet if which != "inside" else None), (inside if which != "wet" else None)
    da, db = (None if a is None else dev(a, 3)), (None if b is None else dev(b, 1))
    out = Padded.empty((h, w), torch.uint8, 7)
    ctx.drifters_zones(None if da is None else da.view, None if db is None else db.view, out=out.view)
    out.check("the zones")
    assert np.array_equal(out.view.cpu().numpy(), D.zones(a, b))
    fresh = ctx.drifters_zones(None if da is None else da.view, None if db is None else db.view)
    assert np.array_equal(fresh.cpu().numpy(), D.zones(a, b))


def test_zones_helper_refusals(ctx):
    lib, hdl = raw(ctx)
    w, h = 20, 12
    t = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda")
    z = (ptr(t, 2 * w * h), w)
    refused = [lib.rcflow_drifters_zones_dev(hdl, 0, null, 0, null, 0, w, h, *z), lib.rcflow_drifters_zones_dev(hdl, 0, ptr(t), w, null, 0, w, h, null, w),
               lib.rcflow_drifters_zones_dev(hdl, 0, ptr(t), w - 1, null, 0, w, h, *z), lib.rcflow_drifters_zones_dev(hdl, 0, ptr(t), w, null, 0, 0, h, *z),
               lib.rcflow_drifters_zones_dev(hdl, 0, ptr(t), w, null, 0, w, h, ptr(t, w), w),       # the output over an input
               lib.rcflow_drifters_zones_dev(hdl, 2, ptr(t), w, null, 0, w, h, *z)]
    assert refused == [EINVAL] * len(refused) and not t.any()


# ---------------------------------------------------------------------------- grids
@pytest.mark.parametrize("w,h,gx,gy", [(37, 29, 1, 1), (37, 29, 5, 4), (131, 130, 128, 128)])
def test_grids(ctx, w, h, gx, gy):
    """one cell; remainder columns and rows in the last cells; 16384 cells of a pixel, the last of 4 x 3"""
    s = Session(ctx, w, h, D.Params(max_drifters=700, grid_x=gx, grid_y=gy, max_age=6, flags=D.RESPAWN), pad=1)
    s.seed(homes_in(w, h, 700, seed=gx))
    f, z = surf(w, h), bands(w, h, 4, 4)
    for _ in range(4 if gx == 128 else 10):
        want = s.push(f, z)
    assert (want["cells"]["flags"] == 0).sum() > (0 if gx == 1 else 5)
    s.close()


# ---------------------------------------------------------------------------- outputs, set, seed, reset, slots
def test_each_output_alone(ctx):
    """what a push does to the state does not depend on the outputs it asked for"""
    w, h, n = 37, 29, 300
    p = D.Params(max_drifters=n, grid_x=3, grid_y=2, max_age=7, flags=D.RESPAWN)
    ref = D.DriftersRef(w, h, p, ctx.jet_lut())
    ctx.drifters_open(w, h, **p.kw())
    homes = homes_in(w, h, n)
    ref.seed(homes)
    ctx.drifters_seed(homes)
    f, z = rotation(w, h, 0.1), bands(w, h)
    df, dz = dev(f, 1), dev(z, 2)
    for k in IMAGES + PER_DRIFTER + ARRAYS + (None,):
        out = outputs(p, w, h, n, pad=3, only=() if k is None else (k,))
        want = ref.push(f, z)
        ctx.drifters_push(df.view, dz.view, **out.kw())
        compare(out.host(), ctx.drifters_read(), want, "with %s alone" % k)
    ctx.drifters_close()


def test_respawn_switched_by_set_seed_after_pushes_and_reset(ctx):
    w, h = 37, 29
    s = Session(ctx, w, h, D.Params(max_drifters=400, grid_x=4, grid_y=4, max_age=5, age_bin=1), pad=2)
    homes = homes_in(w, h, 400)
    s.seed(homes[:150])
    f, z = rotation(w, h, 0.1), bands(w, h)
    for _ in range(8):
        want = s.push(f, z)
    assert want["summary"][1] == 0 and want["summary"][2] == 150          # all dead, nobody released again
    s.ref.set(flags=D.RESPAWN, dt=0.5, max_age=9, density_full=3, live_min=2)
    ctx.drifters_set(0.5, 9, 3, 2, True)
    assert ctx.drifters_info()["respawn"] is True and ctx.drifters_info()["dt"] == 0.5
    for _ in range(3):
        want = s.push(f, z)
    assert want["summary"][2] >= 300
    s.seed(homes[150:])                                           # after pushes: waiting beside the living
    assert s.out.t["state"].numel() == 400
    for _ in range(3):
        want = s.push(f, z)
    assert want["summary"][0] == 400
    s.ref.set(flags=0)
    ctx.drifters_set(0.5, 9, 3, 2, False)
    for _ in range(12):
        want = s.push(f, z)
    assert want["summary"][1] == 0
    s.ref.reset()
    ctx.drifters_reset()
    rc, rp, ro, rh, rsum = ctx.drifters_read()
    assert not rp.any() and not ro.any() and not rh.any() and not any(rsum.values()) and ctx.drifters_info()["pushes"] == 0 and ctx.drifters_info()["drifters"] == 400
    for _ in range(3):
        want = s.push(f, z)
    assert want["summary"][2] == 400 and want["density"].sum() == want["place"][:, 0].sum()
    s.close()


def test_two_slots(ctx):
    w, h = 37, 29
    a = Session(ctx, w, h, D.Params(max_drifters=100, grid_x=2, grid_y=2, flags=D.RESPAWN), stream=0)
    b = Session(ctx, 20, 12, D.Params(max_drifters=77, grid_x=3, grid_y=1, max_age=4), stream=1)
    a.seed(homes_in(w, h, 100))
    b.seed(homes_in(20, 12, 77))
    fa, fb = rotation(w, h, 0.1), D.uniform_field(20, 12, -0.5, 0.25)
    for _ in range(6):
        a.push(fa, bands(w, h))
        b.push(fb)
    a.close()
    b.close()


def test_resident_flow_field_and_the_checked_farneback_field(ctx):
    """End to end on synth.surf_clip(160, 120): the project's own Farneback field (the frame-at-a-time entry), through the flow
    check's d_checked (NaN at the rejected pixels), into the drifters with the prototype's zones and lattice, max_age 300, 301 pushes;
    the device equals the statement on that field on every output (compared at pushes 50, 100, 200 and 301).  Measured on an MI355X
    with this test: checked for BAD, OUT, FLAT and FAST, 420 of the 19200 vectors are rejected (0.021875) and the census is 1514
    SHORE, 0 OFFSHORE, 6 BAD, 0 AGED of 1520: the field Farneback gives for this clip at this size carries nobody out (supposed, not
    examined: the clip's wave fronts travel shoreward at 2.5 px a frame over a jet about 10 px wide).  With the residual test at the translating clip's 1.5 grey
    levels 0.991406 of the field is rejected (brightness is not constant along this clip's flow, by construction) and all 1520 end
    BAD.  The bound on the share that ends BAD is 1.5 times the measured one, the margin convention of the PIV test's recovery
    bounds; nothing else of the census is asserted"""
    w, h = 160, 120
    clip = synth.surf_clip(w, h, 2)
    ctx.stream_reset()
    assert ctx.push_frame_host(clip[0]) is None
    flow = ctx.push_frame_host(clip[1])
    checked = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    # the clip is a texture that follows surf_field under wave fronts that travel at their own 2.5 px a frame: brightness is not
    # constant along the flow by construction, and the residual test at the translating clip's 1.5 grey levels rejects nearly all of it
    fp = F.Params(radius=4, grid_x=4, grid_y=3, tests=F.FLAT | F.RESID, res_max=1.5, tex_min=1)
    ctx.flowcheck_open(w, h, **fp.kw())
    ctx.flowcheck_push(dev(clip[1]).view, dev(clip[0]).view, None, checked=checked)
    rejected_resid = float(np.isnan(checked.cpu().numpy()[..., 0]).mean())
    # so the field is checked for what does not rest on brightness constancy: BAD, OUT, FLAT and FAST
    fp = F.Params(radius=4, grid_x=4, grid_y=3, tests=F.FLAT | F.FAST, tex_min=1, speed_max=20.0)
    ctx.flowcheck_open(w, h, **fp.kw())
    ctx.flowcheck_push(dev(clip[1]).view, dev(clip[0]).view, None, checked=checked)
    p = D.Params(max_drifters=2000, grid_x=8, grid_y=6, max_age=300)
    homes, z = D.prototype_lattice(), D.prototype_zone()
    dz = dev(z)
    # the resident field first: one push, against the statement on the field the slot holds
    ref = D.DriftersRef(w, h, p, ctx.jet_lut())
    ctx.drifters_open(w, h, **p.kw())
    with pytest.raises(RcflowError) as e:
        ctx.drifters_push(None)
    assert e.value.code == ESTATE                                 # no drifter seeded
    ref.seed(homes)
    ctx.drifters_seed(homes)
    out = outputs(p, w, h, ref.n)
    for _ in range(2):
        ctx.drifters_push(None, dz.view, **out.kw())
        compare(out.host(), ctx.drifters_read(), ref.push(flow.cpu().numpy(), z), "(the resident field)")
    # the checked field
    ref.reset()
    ctx.drifters_reset()
    host = checked.cpu().numpy()
    rejected = float(np.isnan(host[..., 0]).mean())
    for k in range(301):
        want = ref.push(host, z)
        ctx.drifters_push(checked, dz.view, **(out.kw() if k in (49, 99, 199, 300) else {}))
        if k in (49, 99, 199, 300):
            compare(out.host(), ctx.drifters_read(), want, "(the checked field, push %d)" % (k + 1))
    sm = want["summary"]
    census = dict(shore=int(sm[8 + D.SHORE]), offshore=int(sm[8 + D.OFFSHORE]), bad=int(sm[8 + D.BAD]), aged=int(sm[8 + D.AGED]), alive=int(sm[1]))
    print("census on the checked Farneback field: %s; rejected share of the field %.6f (with RESID at 1.5: %.6f)" % (census, rejected, rejected_resid))
    assert sum(census.values()) + int(sm[9:13].sum()) == 1520
    assert census["bad"] / 1520 <= 1.5 * MEASURED_BAD_SHARE
    ctx.flowcheck_close()
    ctx.drifters_open(128, 96, **p.kw())
    ctx.drifters_seed([[1.0, 1.0]])
    with pytest.raises(RcflowError) as e:
        ctx.drifters_push(None)
    assert e.value.code == ESIZE                                  # the resident field has another size
    ctx.stream_reset()
    with pytest.raises(RcflowError) as e:
        ctx.drifters_push(None)
    assert e.value.code == ESTATE and ctx.drifters_info()["pushes"] == 0
    ctx.drifters_close()


MEASURED_BAD_SHARE = 6 / 1520                                     # of the 1520 drifters; see the test above


def test_live_mask_into_the_regions(ctx):
    """d_live goes into rcflow_regions_push_dev as it is: the regions equal _regions_ref on the statement's mask"""
    w, h = 131, 67
    s = Session(ctx, w, h, D.Params(max_drifters=4096, grid_x=4, grid_y=4, live_min=3))
    s.seed(D.lattice(np.linspace(0, w - 1, 64), np.linspace(0, h - 1, 64)))
    f = D.converging_field(w, h, 60, 30)
    for _ in range(5):
        want = s.push(f)
    ctx.regions_open(w, h, connectivity=8, min_area=1, max_regions=64)
    ctx.regions_push(s.out.t["live"])
    rec, summ = ctx.regions_read()
    wr = RG.regions(want["live"], 8, 1, 64, None, 1)
    assert summ["kept"] == int(wr["summary"][1]) >= 1 and np.array_equal(rec["area"], wr["records"]["area"][:len(rec)]) and want["live"].any()
    ctx.regions_close()
    s.close()


def test_product_object(ctx):
    w, h = 37, 29
    p = D.Params(max_drifters=64, grid_x=2, grid_y=2, max_age=5)
    ref = D.DriftersRef(w, h, p, ctx.jet_lut())
    homes = homes_in(w, h, 64)
    ref.seed(homes)
    f = rotation(w, h, 0.1)
    with Drifters(ctx, w, h, **p.kw()) as dr:
        dr.seed(homes)
        state = torch.zeros(64, dtype=torch.uint8, device="cuda")
        for _ in range(7):
            dr.push(dev(f).view, state=state)
            want = ref.push(f)
        rc, rp, ro, rh, rsum = dr.read()
        assert same("cells", rc.ravel(), want["cells"]) and rsum["pushes"] == 7 and np.array_equal(state.cpu().numpy(), want["state"])
        assert dr.info()["drifters"] == 64 and dr.info()["respawn"] is False
        with pytest.raises(ValueError):
            dr.push(dev(f[..., 0]).view)                          # one component is no field
        dr.set(2.0, 11, 4, 2, True)
        dr.reset()
        assert dr.info()["pushes"] == 0 and dr.info()["max_age"] == 11 and dr.info()["respawn"] is True
    with pytest.raises(RcflowError):
        ctx.drifters_info()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    w, h, n = 20, 12, 40
    good = D.Params(max_drifters=64, grid_x=4, grid_y=3, max_age=6, flags=D.RESPAWN)
    nc = good.grid_x * good.grid_y
    ctx.drifters_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.drifters_info, ctx.drifters_read, ctx.drifters_reset, lambda: ctx.drifters_set(1.0, 0, 1, 1, False), lambda: ctx.drifters_seed([[1.0, 1.0]])):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 1024)()
    for name, args in (("info", (C.byref(DriftersInfo()),)), ("read", (buf, buf, buf, buf, buf)), ("reset", ()), ("set", (1.0, 0, 1, 1, 0)),
                       ("push_dev", (null, 0) * 6 + (null,) * 8)):
        assert getattr(lib, "rcflow_drifters_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_drifters_%s:" % name), text()
    nan = float("nan")
    kw = good.kw()
    for bad in (dict(max_drifters=0), dict(max_drifters=D.MAX_DRIFTERS + 1), dict(age_bin=0), dict(dt=0.0), dict(dt=0.001), dict(dt=256.01), dict(dt=nan),
                dict(dt=float("inf")), dict(max_age=-1), dict(density_full=0), dict(live_min=0), dict(grid_x=0), dict(grid_x=21), dict(grid_y=13)):
        assert D.open_error(w, h, D.Params(**{**D.asdict(good), **bad})) in ("parameters", "grid")
        with pytest.raises(RcflowError) as e:
            ctx.drifters_open(w, h, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_drifters_open"), bad
    p = DriftersParams(max_drifters=64, grid_x=4, grid_y=3, max_age=6, age_bin=8, density_full=16, live_min=1, flags=2, dt=1.0)
    assert lib.rcflow_drifters_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "RC_DRIFTERS_RESPAWN" in text()
    p.flags = 1
    assert lib.rcflow_drifters_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_drifters_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_drifters_open(hdl, 2, w, h, C.byref(p)) == EINVAL           # no such slot
    with pytest.raises(RcflowError) as e:
        ctx.drifters_open(4000, 2161, **kw)                       # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_drifters_open")
    with pytest.raises(RcflowError):
        ctx.drifters_info()                                       # nothing was left open by any of them

    s = Session(ctx, w, h, good)
    fld, z = D.uniform_field(w, h, 0.5, -0.25), bands(w, h)
    dfld = s.up(fld)
    assert lib.rcflow_drifters_push_dev(hdl, 0, ptr(dfld), 8 * w, *((null, 0) * 5), *((null,) * 8)) == ESTATE and "seeded" in text()
    homes = homes_in(w, h, n)
    pts = np.ascontiguousarray(homes, np.float64)
    seed = lambda a, k: lib.rcflow_drifters_seed(hdl, 0, a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None, k)
    assert seed(None, 1) == EINVAL and seed(pts, 0) == EINVAL and seed(pts, 65) == ESIZE
    for x, y in ((nan, 1.0), (1.0, float("inf")), (-0.001, 1.0), (w - 1 + 0.001, 1.0), (1.0, -1.0), (1.0, h - 1 + 0.5)):
        worse = pts.copy()
        worse[n - 1] = (x, y)                                     # the last point: nothing of the call is added
        assert seed(worse, n) == EINVAL and text().startswith("rcflow_drifters_seed") and ctx.drifters_info()["drifters"] == 0
    edge = np.array([[0.0, 0.0], [w - 1.0, h - 1.0]])
    s.seed(np.concatenate([homes, edge]))                         # the corners of the picture are inside it
    s.push(fld, z)
    assert seed(pts, 64 - n - 2 + 1) == ESIZE and ctx.drifters_info()["drifters"] == n + 2
    assert lib.rcflow_drifters_info(hdl, 0, None) == EINVAL
    before = ctx.drifters_info()
    for bad in (dict(age_bin=0), dict(grid_x=21)):                # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.drifters_open(w, h, **dict(kw, **bad))
    assert ctx.drifters_info() == before
    m = n + 2
    big = torch.zeros(64 * h * w + 8192, dtype=torch.uint8, device="cuda")
    dzone = s.up(z)
    N = (null, 0)

    def push(field=None, step=8 * w, zone=N, now=N, dens=N, live=N, pic=N, xy=null, age=null, state=null, cells=null, place=null, origin=null, hist=null,
             summ=null, slot=0):
        return lib.rcflow_drifters_push_dev(hdl, slot, ptr(dfld) if field is None else field, step, *zone, *now, *dens, *live, *pic, xy, age, state, cells,
                                            place, origin, hist, summ)

    refused = [
        push(step=8 * w - 8), push(step=8 * w + 4), push(field=ptr(dfld, 4)), push(zone=(ptr(dzone), w - 1)),
        push(now=(ptr(big), 2 * w - 2)), push(now=(ptr(big, 1), 2 * w)), push(now=(ptr(big), 2 * w + 1)), push(dens=(ptr(big), 4 * w - 4)),
        push(dens=(ptr(big, 2), 4 * w)), push(dens=(ptr(big), 4 * w + 2)), push(live=(ptr(big), w - 1)), push(pic=(ptr(big), 3 * w - 1)),
        push(xy=ptr(big, 4)), push(age=ptr(big, 2)), push(cells=ptr(big, 2)), push(place=ptr(big, 4)), push(origin=ptr(big, 4)), push(hist=ptr(big, 4)),
        push(summ=ptr(big, 4)),
        push(dens=(ptr(dfld), 4 * w)),                            # an output over the field
        push(zone=(ptr(dzone), w), live=(ptr(dzone), w)),         # an output over the zones
        push(now=(ptr(big), 2 * w), dens=(ptr(big, 2 * w * (h - 1)), 4 * w)),     # two outputs meeting in one row
        push(xy=ptr(big), age=ptr(big, 8 * m - 4)), push(age=ptr(big), state=ptr(big, 4 * m - 1)), push(place=ptr(big), origin=ptr(big, 64 * nc - 8)),
        push(cells=ptr(big), hist=ptr(big, 32 * nc - 8)), push(hist=ptr(big), summ=ptr(big, 8 * 128 - 8)), push(live=(ptr(big), w), summ=ptr(big)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert text().startswith("rcflow_drifters_push_dev")
    assert push(slot=2) == EINVAL
    for bad in ((0.0, 6, 16, 1, True), (nan, 6, 16, 1, True), (300.0, 6, 16, 1, True), (1.0, -1, 16, 1, True), (1.0, 6, 0, 1, True), (1.0, 6, 16, 0, True)):
        with pytest.raises(RcflowError) as e:
            ctx.drifters_set(*bad)
        assert e.value.code == EINVAL and text().startswith("rcflow_drifters_set")
    assert lib.rcflow_drifters_set(hdl, 0, 1.0, 6, 16, 1, 2) == EINVAL
    assert ctx.drifters_info() == before and not big.any()
    # nothing was queued and nothing changed: the next pushes give what the statement gives
    for _ in range(3):
        s.push(fld, z, "(after the refusals)")
    # an accepted boundary: age begins at the first byte after xy's range, in one allocation
    one = torch.zeros(12 * m + 64, dtype=torch.uint8, device="cuda")
    txy, tage = one[:8 * m].view(torch.float32), one[8 * m:12 * m].view(torch.int32)
    want = s.ref.push(fld, z)
    ctx.drifters_push(dfld, dzone, xy=txy, age=tage)
    assert same_bits(txy.cpu().numpy().reshape(-1, 2), want["xy"]) and np.array_equal(tage.cpu().numpy(), want["age"]) and not one[12 * m:].any()
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        want = s.push(fld, z, "(on another stream)")
    torch.cuda.synchronize()
    s.close()
    ctx.drifters_close()                                          # closing twice is fine
