"""The plan view on the device (planview_kernels.hip) against its numpy statement (tests/_planview_ref.py): the table, the plan
field, the mask, the picture and both copies of the summary, all bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _cpp
import _ftle_ref as F
import _planview_ref as P
import _regions_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, bits, ptr, raw
from ripcurrents_amd._lib import RC_PLANVIEW_LAUNCHES, PlanViewParams, RcflowError
from ripcurrents_amd.api import FTLE_SUMMARY, PLANVIEW_SUMMARY

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 97, 53


def outputs(nx, ny, pad=0):
    return Outputs(dict(plan=((ny, nx, 2), torch.float32), mask=((ny, nx), torch.uint8), plan_bgr=((ny, nx, 3), torch.uint8)),
                   dict(summary=((8,), torch.int64, -1)), pad)


def dev(a, pad=0):
    return Padded.of(a, pad).view


def compare(got, read, want, what):
    assert np.array_equal(bits(got["plan"]), bits(want["plan"])), "plan field differs " + what
    assert np.array_equal(got["mask"], want["mask"]), "mask differs " + what
    assert np.array_equal(got["plan_bgr"], want["bgr"]), "picture differs " + what
    assert np.array_equal(got["summary"], want["summary"]), "summary %s, wanted %s %s" % (got["summary"], want["summary"], what)
    assert [read[k] for k in PLANVIEW_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


def run(ctx, w, h, p, fields, frames, pad=0, stream=0):
    """Pushes fields and frames into the device session and the numpy one; compares after every push."""
    ctx.planview_open(w, h, stream=stream, **p.kw())
    ref = P.PlanViewRef(w, h, p)
    assert np.array_equal(bits(ctx.planview_table(stream=stream)), bits(ref.table)), "table differs"
    out = outputs(p.nx, p.ny, pad)
    want = None
    for t, (f, g) in enumerate(zip(fields, frames)):
        ctx.planview_push(dev(f, pad), dev(g, pad), stream=stream, **out.kw())
        want = ref.push(f, g)
        compare(out.host(), ctx.planview_read(stream=stream), want, "after push %d of %dx%d -> %dx%d" % (t + 1, w, h, p.nx, p.ny))
    return ref, want


def inputs(w, h, count):
    return [P.wavy_field(w, h, k=k) for k in range(count)], [P.frame(w, h, seed=k + 1) for k in range(count)]


def horizon_camera():
    """two degrees of tilt and a plan that reaches 60 m behind the camera: pz changes sign inside the plan, and inside a cell"""
    Hm, fx, fy, cx, cy = P.tilted_camera(W, H, 90.0, tilt_deg=2.0)
    return P.Params(Hm, fx, fy, cx, cy, 0.0, 0.0, -30.0, -60.0, 1.0, 3.3, 61, 37, 10.0, math.inf)


CAMERAS = {
    "pinhole": lambda: P.shore_camera(),
    "distorted": lambda: P.shore_camera(k1=-0.12, k2=0.02),
    "identity": lambda: P.identity(W, H),
    "dx<0": lambda: P.Params(**dict(P.shore_camera(k1=-0.12, k2=0.02).kw(), x0=30.0, dx=-1.0)),
    "horizon": horizon_camera,
}


# ---------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name", list(CAMERAS))
def test_table_bit_for_bit(ctx, name):
    p = CAMERAS[name]()
    want = P.table(p)
    usable = want[..., 7] != 0
    assert usable.any() and (name == "identity" or not usable.all())
    if name == "horizon":
        parts = P.table_parts(p)
        assert (~parts["front"]).sum() > 61 * 10 and parts["front"].sum() > 61 * 10
    ctx.planview_open(W, H, **p.kw())
    got = ctx.planview_table()
    assert got.shape == (p.ny, p.nx, 8) and np.array_equal(bits(got), bits(want))
    if name == "dx<0":                                            # the mirrored grid sees the same water: the same cells, mirrored
        fwd = P.table(P.shore_camera(k1=-0.12, k2=0.02))
        assert np.array_equal(got[:, ::-1, 7], fwd[..., 7]) and np.array_equal(got[:, ::-1, 0], fwd[..., 0])
    ctx.planview_close()


# ---------------------------------------------------------------------------- the push
def test_pushes_of_the_small_camera_with_padded_rows(ctx):
    fields, frames = inputs(W, H, 3)
    _, want = run(ctx, W, H, P.shore_camera(k1=-0.12, k2=0.02), fields, frames, pad=5)
    assert want["summary"][2] > 200 and want["summary"][0] > want["summary"][1] and want["summary"][4] == 3
    ctx.planview_close()


def test_many_blocks_reach_the_ticket(ctx):
    """320 x 240 -> 300 x 200: 5 x 50 blocks"""
    w, h = 320, 240
    fields, frames = inputs(w, h, 2)
    p = P.shore_camera(w, h, 300.0, 300, 200, 0.2, 0.3, 0.2, k1=-0.12, k2=0.02)
    _, want = run(ctx, w, h, p, fields, frames)
    assert want["summary"][2] > 5000 and want["summary"][0] > want["summary"][1]
    ctx.planview_close()


def test_waves_that_walk_two_rows(ctx):
    """plan 1030 x 1026: 17 x 257 groups of four rows are more than the launch's 4096 blocks, so a wave walks two rows, four
    apart, and the last block has one; the last wave across is 6 cells wide"""
    w, h = 320, 240
    fields, frames = inputs(w, h, 1)
    p = P.shore_camera(w, h, 300.0, 1030, 1026, 61.0 / 1030, 55.5 / 1026, math.inf, k1=-0.12, k2=0.02)
    p.x0 = -58.0
    _, want = run(ctx, w, h, p, fields, frames, pad=2)
    assert want["valid"][1025].any() and want["valid"][:, 1024:].any() and want["summary"][0] > want["summary"][2] > 100000
    ctx.planview_close()


def test_a_ragged_last_wave(ctx):
    """plan 261 x 5: five waves across, the last 5 cells wide; two blocks down, the second one row"""
    fields, frames = inputs(W, H, 2)
    p = P.shore_camera(nx=261, ny=5, dx=0.25, dy=3.0, max_gsd=math.inf, k1=-0.12, k2=0.02)
    p.x0, p.y0 = -60.0, 2.0
    _, want = run(ctx, W, H, p, fields, frames, pad=3)
    assert want["valid"][:, 256:].any() and want["valid"][4].any()
    ctx.planview_close()


@pytest.mark.parametrize("nx,ny", [(5, 3), (70, 9), (130, 29)])
def test_fewer_blocks_than_shards_and_a_few_more(ctx, nx, ny):
    """1, 6 and 24 blocks: the closing's eight shards with no block in most, with one block at most, and with three each"""
    fields, frames = inputs(W, H, 2)
    p = P.shore_camera(nx=nx, ny=ny, dx=20.0 / nx, dy=30.0 / ny, max_gsd=math.inf, k1=-0.12, k2=0.02)
    p.x0, p.y0 = -10.0, 2.0
    _, want = run(ctx, W, H, p, fields, frames)
    assert want["summary"][2] > 0
    ctx.planview_close()


def test_bad_values_in_the_field(ctx):
    """NaN, +-inf and 1e30 in the field: the finite test, an overflowing Vx and the one NaN rule of the maximum"""
    p = P.shore_camera(k1=-0.12, k2=0.02, fps=3000.0)           # m of 10 and more: a sample of 3e38 overflows the products
    fields, frames = inputs(W, H, 4)
    clean = P.push(P.table(p), W, H, fields[0], None, 1)
    fields[0][33:37, 68:72] = (3e38, 3e38)                        # inf - inf in Vx or Vy, in one of the two: a NaN plan value
    fields[1][33:37, 68:72] = (3e38, -3e38)
    rng = np.random.default_rng(5)
    vals = [np.nan, np.inf, -np.inf, 1e30, -3e38]
    for k in range(200):
        y, x, c = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1)), int(rng.integers(0, 2))
        fields[k % 4][y, x, c] = vals[k % 5]
    _, want = run(ctx, W, H, p, fields, frames)
    assert 0 < want["valid"].sum() < clean["valid"].sum()
    assert np.isinf(want["plan"]).any()                           # a valid cell whose product overflowed
    nans = [P.push(P.table(p), W, H, f, None, 1) for f in fields[:2]]
    assert any(np.isnan(r["plan"][r["valid"]]).any() for r in nans)           # and a valid cell whose sum is NaN: the maximum passes it by
    assert all(0 < r["summary"][3] <= 0x7F800000 for r in nans)
    ctx.planview_close()


def test_each_output_and_each_input_alone(ctx):
    p = P.shore_camera(k1=-0.12, k2=0.02)
    (f,), (g,) = inputs(W, H, 1)
    ctx.planview_open(W, H, **p.kw())
    ref = P.PlanViewRef(W, H, p)
    assert ctx.planview_read() == dict(dict.fromkeys(PLANVIEW_SUMMARY, 0), max_speed=0.0)
    df, dg = dev(f), dev(g)
    for name in ("plan", "mask", "plan_bgr", "summary"):
        o = outputs(p.nx, p.ny)
        ctx.planview_push(df, dg, **{name: o.kw()[name]})
        want = ref.push(f, g)
        got = o.host()
        key = "bgr" if name == "plan_bgr" else name
        assert np.array_equal(got[name].view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), name
        for other in ("plan", "mask", "plan_bgr"):
            if other != name:
                assert (got[other].view(np.uint8) == SENTINEL).all(), "%s was written" % other
        assert [ctx.planview_read()[k] for k in PLANVIEW_SUMMARY] == [int(v) for v in want["summary"]]
    # the field alone, the frame alone
    o = outputs(p.nx, p.ny)
    ctx.planview_push(df, None, plan=o.t["plan"], mask=o.t["mask"], summary=o.t["summary"])
    want = ref.push(f, None)
    got = o.host()
    assert np.array_equal(bits(got["plan"]), bits(want["plan"])) and np.array_equal(got["mask"], want["mask"])
    assert np.array_equal(got["summary"], want["summary"]) and (got["plan_bgr"] == SENTINEL).all()
    o = outputs(p.nx, p.ny)
    ctx.planview_push(None, dg, plan_bgr=o.t["plan_bgr"])
    want = ref.push(None, g)
    assert np.array_equal(o.host()["plan_bgr"], want["bgr"])
    r = ctx.planview_read()
    assert [r[k] for k in PLANVIEW_SUMMARY] == [int(v) for v in want["summary"]] and r["valid"] == 0 and r["pushes"] == 6
    ctx.planview_push(df, dg)                                     # no output at all is a push too
    assert ctx.planview_read()["pushes"] == 7 and ctx.planview_info()["pushes"] == 7
    ctx.planview_close()


# ---------------------------------------------------------------------------- identity
def test_identity_returns_the_field_and_the_frame(ctx):
    """H = I, unit cells from (0, 0), fps 1, no distortion, the plan the image's size, a finite field with no zero component:
    the plan field equals the field bit for bit on [1, w - 2] x [1, h - 2] and is 0 outside; the picture equals the frame
    there.  Zeros are excluded because m01 is -0.0 here: a -0.0 component would come back as +0.0."""
    w, h = 131, 70
    f, g = P.wavy_field(w, h), P.frame(w, h)
    assert np.isfinite(f).all() and (f != 0).all()
    ctx.planview_open(w, h, **P.identity(w, h).kw())
    o = outputs(w, h)
    ctx.planview_push(dev(f), dev(g), **o.kw())
    got = o.host()
    inner = np.zeros((h, w), bool)
    inner[1:h - 1, 1:w - 1] = True
    assert np.array_equal(bits(got["plan"][inner]), bits(f[inner])) and not got["plan"][~inner].any()
    assert np.array_equal(got["plan_bgr"][inner], g[inner]) and not got["plan_bgr"][~inner].any()
    assert np.array_equal(got["mask"] != 0, inner)
    assert list(got["summary"][:3]) == [w * h, inner.sum(), inner.sum()]
    ctx.planview_close()


# ---------------------------------------------------------------------------- the chain
def test_plan_field_goes_straight_into_ftle_and_regions(ctx):
    """planview -> ftle on the same slot and stream, nothing in between; the plan-view mask into regions without a copy"""
    w, h = 320, 240
    p = P.shore_camera(w, h, 300.0, 150, 100, 0.4, 0.6, 0.2, fps=4.0)
    nx, ny = p.nx, p.ny
    fields, _ = inputs(w, h, 3)
    lut = ctx.jet_lut()
    ctx.planview_open(w, h, **p.kw())
    ctx.ftle_open(nx, ny, window=3, direction="backward", threshold=0.02, vis_max=0.4)
    ctx.regions_open(nx, ny, connectivity=8, min_area=4, max_regions=256)
    pref, fref = P.PlanViewRef(w, h, p), F.FtleRef(nx, ny, lut, 3, F.BACKWARD, 1.0, 1, 0.02, 0.4)
    plan = torch.zeros((ny, nx, 2), dtype=torch.float32, device="cuda")
    pmask = torch.zeros((ny, nx), dtype=torch.uint8, device="cuda")
    m = torch.zeros((ny, nx, 2), dtype=torch.float32, device="cuda")
    steps = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
    lam = torch.zeros((ny, nx), dtype=torch.float32, device="cuda")
    fmask = torch.zeros((ny, nx), dtype=torch.uint8, device="cuda")
    summ = torch.zeros(8, dtype=torch.int64, device="cuda")
    for f in fields:
        ctx.planview_push(dev(f), plan=plan, mask=pmask)
        ctx.ftle_push(plan, map=m, steps=steps, lam=lam, mask=fmask, summary=summ)
        ctx.regions_push(pmask, flow=plan)
        wp = pref.push(f)
        wf = fref.push(wp["plan"])
    assert np.isfinite(wp["plan"]).all() and wp["valid"].sum() > 2000
    assert np.array_equal(bits(plan.cpu().numpy()), bits(wp["plan"]))
    assert np.array_equal(bits(m.cpu().numpy()), bits(wf["map"])) and np.array_equal(steps.cpu().numpy(), wf["steps"])
    assert np.array_equal(bits(lam.cpu().numpy()), bits(wf["lam"])) and np.array_equal(fmask.cpu().numpy(), wf["mask"])
    assert np.array_equal(summ.cpu().numpy(), wf["summary"]) and wf["summary"][1] > 0
    assert [ctx.ftle_read()[k] for k in FTLE_SUMMARY] == [int(v) for v in wf["summary"]]
    rec, rs = ctx.regions_read()
    wr = R.regions(wp["mask"], 8, 4, 256, wp["plan"], len(fields))
    assert rs["kept"] == int(wr["summary"][1]) > 0
    assert np.array_equal(rec["area"], wr["records"]["area"][:len(rec)]) and np.array_equal(rec["label"], wr["records"]["label"][:len(rec)])
    ctx.regions_close()
    ctx.ftle_close()
    ctx.planview_close()


# ---------------------------------------------------------------------------- the profile
def test_profile_books_one_table_and_one_push_launch(ctx):
    p = P.shore_camera()
    (f,), (g,) = inputs(W, H, 1)
    df, dg = dev(f), dev(g)
    o = outputs(p.nx, p.ny)
    ctx.planview_close()
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.planview_open(W, H, **p.kw())
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    assert prof == {"planview@0": 1}, prof
    assert ctx.planview_info()["launches_per_push"] == RC_PLANVIEW_LAUNCHES == 1
    ctx.profile_reset()
    for k in range(3):
        ctx.planview_push(df, dg, **o.kw())
    ctx.planview_push(df, None, mask=o.t["mask"])
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    assert prof == {"planview@1": 4}, prof
    assert ctx.profile_read_buckets()["farneback"] > 0
    ctx.profile_enable(False)
    ctx.planview_close()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    p = P.shore_camera(k1=-0.12, k2=0.02)
    good = p.kw()
    nx, ny = p.nx, p.ny
    (f, f2), (g, g2) = inputs(W, H, 2)
    ctx.planview_close()
    for call in (ctx.planview_info, ctx.planview_read, ctx.planview_reset, ctx.planview_table):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    lib, hdl = raw(ctx)
    assert lib.rcflow_planview_push_dev(hdl, 0, null, 0, null, 0, null, 0, null, 0, null, 0, null) == ESTATE
    nan, inf = float("nan"), float("inf")
    Hbad = list(p.H)
    Hbad[4] = nan
    Hinf = list(p.H)
    Hinf[8] = inf
    for bad in (dict(H=Hbad), dict(H=Hinf), dict(fx=0.0), dict(fx=-90.0), dict(fy=0.0), dict(fy=nan), dict(fx=inf), dict(cx=nan), dict(cy=inf),
                dict(k1=nan), dict(k2=-inf), dict(x0=nan), dict(y0=inf), dict(dx=0.0), dict(dy=0.0), dict(dx=nan), dict(dy=inf), dict(nx=0),
                dict(ny=0), dict(ny=-3), dict(fps=0.0), dict(fps=-1.0), dict(fps=inf), dict(fps=nan), dict(max_gsd=0.0), dict(max_gsd=-1.0),
                dict(max_gsd=nan)):
        with pytest.raises(RcflowError) as e:
            ctx.planview_open(W, H, **dict(good, **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    for bad in (dict(nx=3841), dict(ny=2161)):
        with pytest.raises(RcflowError) as e:
            ctx.planview_open(W, H, **dict(good, **bad))
        assert e.value.code == ESIZE, bad
    cp = PlanViewParams(fx=90.0, fy=90.0, cx=48.0, cy=26.0, dx=1.0, dy=1.0, nx=8, ny=8, fps=1.0, max_gsd=inf, flags=1)
    cp.H[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    assert lib.rcflow_planview_open(hdl, 0, W, H, C.byref(cp)) == EINVAL       # unknown flag bits
    cp.flags = 0
    assert lib.rcflow_planview_open(hdl, 0, W, H, None) == EINVAL
    assert lib.rcflow_planview_open(hdl, 0, 0, H, C.byref(cp)) == EINVAL
    assert lib.rcflow_planview_open(hdl, 0, 8192, 4096, C.byref(cp)) == ESIZE  # an image beyond the context
    assert lib.rcflow_planview_open(hdl, 2, W, H, C.byref(cp)) == EINVAL       # no such slot
    with pytest.raises(RcflowError):
        ctx.planview_info()                                       # nothing was opened by any of them

    ref, _ = run(ctx, W, H, p, [f], [g])
    info = ctx.planview_info()
    assert (info["w"], info["h"], info["nx"], info["ny"], info["pushes"], info["launches_per_push"]) == (W, H, nx, ny, 1, 1)
    assert info["H"] == tuple(p.H) and (info["k1"], info["k2"], info["fps"], info["max_gsd"]) == (-0.12, 0.02, 10.0, 0.6)
    assert info["device_bytes"] >= nx * ny * 32
    before, tab = info, ctx.planview_table()
    for bad in (dict(dx=0.0), dict(max_gsd=nan), dict(nx=3841)):  # a refused re-open keeps the state and the table
        with pytest.raises(RcflowError):
            ctx.planview_open(W, H, **dict(good, **bad))
    with pytest.raises(RcflowError) as e:
        ctx.planview_open(4000, 2160, **good)
    assert e.value.code == ESIZE and ctx.planview_info() == before and np.array_equal(bits(ctx.planview_table()), bits(tab))

    df, dg = dev(f2), dev(g2)
    big = torch.zeros(ny * nx * 8 + 512, dtype=torch.uint8, device="cuda")

    def push(flow=None, fstep=8 * W, bgr=None, bstep=3 * W, plan=(null, 0), mask=(null, 0), pic=(null, 0), summ=null, slot=0):
        fp = ptr(df) if flow is None else flow
        bp = ptr(dg) if bgr is None else bgr
        return lib.rcflow_planview_push_dev(hdl, slot, fp, fstep, bp, bstep, plan[0], plan[1], mask[0], mask[1], pic[0], pic[1], summ)

    refused = [
        push(flow=null, bgr=null),                                # neither input
        push(flow=null, plan=(ptr(big), 8 * nx)), push(flow=null, mask=(ptr(big), nx)), push(flow=null, summ=ptr(big)),   # need the field
        push(bgr=null, pic=(ptr(big), 3 * nx)),                   # needs the frame
        push(fstep=8 * W - 8), push(fstep=8 * W + 4), push(flow=ptr(df, 4)), push(bstep=3 * W - 1),
        push(plan=(ptr(big), 8 * nx - 8)), push(plan=(ptr(big), 8 * nx + 4)), push(plan=(ptr(big, 4), 8 * nx)),
        push(mask=(ptr(big), nx - 1)), push(pic=(ptr(big), 3 * nx - 1)), push(summ=ptr(big, 4)),
        push(mask=(ptr(df), nx)),                                 # an output over the field
        push(pic=(ptr(dg, 7), 3 * nx)),                           # an output over the frame
        push(plan=(ptr(df), 8 * nx)),
        push(flow=ptr(big, 16), plan=(ptr(big), 8 * nx)),         # the field inside an output (W > nx: it reaches past it too)
        push(plan=(ptr(big), 8 * nx), mask=(ptr(big, 8 * nx * ny - 1), nx)),       # two outputs meeting in one row
        push(plan=(ptr(big), 8 * nx), pic=(ptr(big, 64), 3 * nx)),
        push(mask=(ptr(big), nx), pic=(ptr(big, nx * (ny - 1)), 3 * nx)),
        push(pic=(ptr(big), 3 * nx), summ=ptr(big, 8)), push(mask=(ptr(big), nx), summ=ptr(big, 0)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert push(slot=2) == EINVAL                                 # no such slot
    assert ctx.planview_info() == before
    # nothing was queued and nothing changed: the second push gives what the statement gives
    o = outputs(nx, ny)
    ctx.planview_push(df, dg, **o.kw())
    compare(o.host(), ctx.planview_read(), ref.push(f2, g2), "(after the refusals)")
    # an accepted boundary: the mask begins at the first byte after the plan field's range, in one allocation
    one = torch.full((9 * nx * ny + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tp, tm = one[:8 * nx * ny].view(torch.float32).view(ny, nx, 2), one[8 * nx * ny:9 * nx * ny].view(ny, nx)
    ctx.planview_push(df, None, plan=tp, mask=tm)
    w3 = ref.push(f2, None)
    assert np.array_equal(bits(tp.cpu().numpy()), bits(w3["plan"])) and np.array_equal(tm.cpu().numpy(), w3["mask"])
    assert (one[9 * nx * ny:] == SENTINEL).all()
    # reset clears the pushes and the summary and keeps the table
    ctx.planview_reset()
    ref.reset()
    assert ctx.planview_info()["pushes"] == 0 and ctx.planview_read() == dict(dict.fromkeys(PLANVIEW_SUMMARY, 0), max_speed=0.0)
    assert np.array_equal(bits(ctx.planview_table()), bits(tab))
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    for k, (ff, gg) in enumerate(((f, g), (f2, g2), (f, g2))):
        torch.cuda.synchronize()
        if k % 2:
            with torch.cuda.stream(side):
                ctx.planview_push(dev(ff), dev(gg), **o.kw())
                got = ctx.planview_read()
        else:
            ctx.planview_push(dev(ff), dev(gg), **o.kw())
            got = ctx.planview_read()
        torch.cuda.synchronize()
        compare(o.host(), got, ref.push(ff, gg), "(streams alternating, push %d)" % (k + 1))
    # re-open with other parameters replaces it; the second slot has a state of its own
    run(ctx, W, H, P.identity(W, H), [f], [g])
    assert ctx.planview_info()["nx"] == W
    run(ctx, W, H, p, [f2], [g2], stream=1)
    assert ctx.planview_info(stream=1)["nx"] == nx and ctx.planview_info()["nx"] == W
    ctx.planview_close(stream=1)
    ctx.planview_close()
    ctx.planview_close()                                          # closing twice is fine


# ---------------------------------------------------------------------------- the C++ mirror
def test_cpp_planview_against_the_statement(ctx, tmp_path):
    """rc::PlanView (include/rcflow_module.hpp) compiled with the flags of tests/cpp's test_module and run on fields and frames
    it makes itself from integers (exact in float, so this file makes the same ones) through a camera whose numbers are exact
    in double; the summaries and counts it prints equal the statement's."""
    n = 3
    stdout = _cpp.run("test_planview", tmp_path, n)
    p = P.Params([90.0, 45.0, 165.0, 0.0, -6.5625, 933.125, 0.0, 0.9375, 3.4375], 90.0, 90.0, 48.0, 26.0, -0.125, 0.03125, -30.0, -6.0, 1.0, 1.5,
                 61, 37, 10.0, 0.6)
    ref = P.PlanViewRef(W, H, p)
    tl = [l.split() for l in stdout.splitlines() if l.startswith("table ")]
    assert len(tl) == 1 and int(tl[0][1]) == int((ref.table[..., 7] != 0).sum()) > 0
    lines = [l.split() for l in stdout.splitlines() if l.startswith("push ")]
    assert len(lines) == n
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for t, l in enumerate(lines):
        u = ((x * 7 + y * 3 + t * 5) % 32 - 12).astype(f32) / f32(16)
        v = ((x * 5 + y * 11 + t * 3) % 32 - 18).astype(f32) / f32(16)
        img = np.stack([(x * 7 + y * 13 + c * 5 + t) % 256 for c in range(3)], -1).astype(np.uint8)
        want = ref.push(np.stack([u, v], -1), img)
        assert [int(s) for s in l[1:9]] == [int(s) for s in want["summary"]] and want["summary"][2] > 100, "push %d" % (t + 1)
        assert int(l[9]) == int((want["mask"] != 0).sum()) and int(l[10]) == int(want["bgr"].any(-1).sum()), "push %d" % (t + 1)
        assert int(l[11]) == int(bits(want["plan"]).astype(np.uint64).sum()), "push %d" % (t + 1)
