"""The flow kinematics on the device (kinematics_kernels.hip) against their numpy statement (tests/_kinematics_ref.py): every
plane, the mask, the picture, the sums, the summary and the records bit for bit.  Nothing on the device is transcendental and
no square root is taken, so nothing weaker is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _kinematics_ref as K
import _regions_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, bits, ptr, raw
from ripcurrents_amd._lib import RC_KINEMATICS_LAUNCHES, KinematicsParams, RcflowError
from ripcurrents_amd.api import KINEMATICS_CELL_DTYPE, KINEMATICS_SUMMARY, Kinematics

pytestmark = pytest.mark.gpu

FLOATS = ("mean_vorticity", "circulation", "mean_divergence", "enstrophy", "mean_ow", "circulation_cw", "circulation_ccw")


def views(d):
    d["cells"], d["sums"] = d["cells"].view(KINEMATICS_CELL_DTYPE), d["sums"].reshape(-1, K.SUMS)


def outputs(w, h, gx, gy, pad=0):
    f, b, i64 = torch.float32, torch.uint8, torch.int64
    return Outputs(dict(omega=((h, w), f), div=((h, w), f), ow=((h, w), f), mask=((h, w), b), vis=((h, w, 3), b)),
                   dict(cells=((gy * gx * 48,), b, None), sums=((gy * gx * K.SUMS,), i64, -1), summary=((8,), i64, -1)), pad, views)


def dev_field(f, pad=0):
    return Padded.of(f, pad).view


def compare_one(name, got, want, what):
    if name in ("omega", "div", "ow"):
        assert np.array_equal(bits(got), bits(want[name])), "%s differs %s: %d pixels" % (name, what, int((bits(got) != bits(want[name])).sum()))
    elif name == "cells":
        for k in KINEMATICS_CELL_DTYPE.names:
            g, w_ = got[k].reshape(-1), want["cells"][k]
            same = np.array_equal(bits(g), bits(w_)) if k in FLOATS else np.array_equal(g, w_)
            assert same, "records differ in %s %s: %s, wanted %s" % (k, what, g, w_)
    else:
        assert np.array_equal(got, want[name]), "%s differs %s: %s, wanted %s" % (name, what, got, want[name])


def compare(got, read, want, what):
    for name in ("omega", "div", "ow", "mask", "vis", "sums", "summary", "cells"):
        compare_one(name, got[name], want, what)
    cells, sums, summ = read
    compare_one("cells", cells, want, "(the slot's) " + what)
    assert np.array_equal(sums.reshape(-1, K.SUMS), want["sums"]), "the slot's sums differ " + what
    assert [summ[k] for k in KINEMATICS_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what
    assert summ["t2"] == want["T2"]
    for k in ("omega", "div", "ow"):
        assert np.isfinite(got[k]).all()


@pytest.fixture(scope="module")
def cases():
    return K.cases()


@pytest.fixture(scope="module")
def wanted(ctx, cases):
    """the statement of every case, computed once and left unchanged"""
    lut = ctx.jet_lut()
    return {name: K.kinematics(f, lut, p) for name, (f, p) in cases.items()}


def open_case(ctx, f, p, stream=0):
    ctx.kinematics_open(f.shape[1], f.shape[0], stream=stream, **p)


CASES = ("surf", "ragged", "one_interior_pixel", "no_smoothing", "tiles_and_full_halo", "sliver_column", "sliver_row", "many_tiles", "pair", "poisoned")


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name,pad", [(n, 0) for n in CASES] + [("ragged", 5), ("poisoned", 3)],
                         ids=list(CASES) + ["strided", "strided_poisoned"])
def test_case_against_the_statement(ctx, cases, wanted, name, pad):
    """field and output steps larger than the rows in the strided forms, with sentinel padding that must stay"""
    f, p = cases[name]
    h, w = f.shape[:2]
    open_case(ctx, f, p)
    out = outputs(w, h, p["grid_x"], p["grid_y"], pad)
    ctx.kinematics_push(dev_field(f, pad), **out.kw())
    compare(out.host(), ctx.kinematics_read(), wanted[name], "in case %s" % name)
    # a second push of the same field gives the same: every counter was left zero
    out2 = outputs(w, h, p["grid_x"], p["grid_y"], pad)
    ctx.kinematics_push(dev_field(f, pad), **out2.kw())
    want2 = dict(wanted[name], summary=wanted[name]["summary"].copy())
    want2["summary"][6] = 2
    compare(out2.host(), ctx.kinematics_read(), want2, "in case %s, pushed again" % name)
    ctx.kinematics_close()


# ---------------------------------------------------------------------------- outputs optional
def test_each_output_alone_and_a_push_with_none(ctx, cases, wanted):
    f, p = cases["ragged"]
    h, w = f.shape[:2]
    want = wanted["ragged"]
    open_case(ctx, f, p)
    assert ctx.kinematics_info()["launches_per_push"] == RC_KINEMATICS_LAUNCHES == 2
    cells, sums, summ = ctx.kinematics_read()
    assert not sums.any() and not cells["flags"].any() and all(summ[k] == 0 for k in KINEMATICS_SUMMARY)
    d = dev_field(f)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(3):
        ctx.kinematics_push(d)                                    # every output NULL: only counted
    torch.cuda.synchronize()
    assert not [r for r in ctx.profile_read() if r["launches"]]
    assert ctx.kinematics_info()["pushes"] == 3 and ctx.kinematics_read()[2]["pushes"] == 0
    ctx.profile_reset()
    n = 3
    for name in ("omega", "div", "ow", "mask", "vis", "cells", "sums", "summary"):
        out = outputs(w, h, p["grid_x"], p["grid_y"])
        ctx.kinematics_push(d, **out.kw(only=(name,)))
        n += 1
        got = out.host()
        w1 = dict(want, summary=want["summary"].copy())
        w1["summary"][6] = n
        compare_one(name, got[name], w1, "asked for alone")
        assert ctx.kinematics_read()[2]["pushes"] == n            # the slot's copy is written whatever was asked for
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    assert prof == {"kinematics@0": 8, "kinematics@1": 8}, prof
    buckets = ctx.profile_read_buckets()
    assert buckets["farneback"] > 0 and not any(v for k, v in buckets.items() if k != "farneback"), buckets
    ctx.profile_enable(False)
    ctx.kinematics_close()


# ---------------------------------------------------------------------------- the chain
def test_mask_goes_straight_into_regions(ctx, cases, wanted):
    f, p = cases["pair"]
    h, w = f.shape[:2]
    open_case(ctx, f, p)
    ctx.regions_open(w, h, connectivity=8, min_area=4, max_regions=64)
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    d = dev_field(f)
    ctx.kinematics_push(d, mask=mask)
    ctx.regions_push(mask, flow=d)                                # the same stream: no host round trip in between
    rec, summ = ctx.regions_read()
    wr = R.regions(wanted["pair"]["mask"], 8, 4, 64, f, 1)
    assert summ["kept"] == int(wr["summary"][1]) == 2 and len(rec) == 2
    assert np.array_equal(rec["area"], wr["records"]["area"][:2]) and rec["area"][0] == rec["area"][1]
    ctx.regions_close()
    ctx.kinematics_close()


# ---------------------------------------------------------------------------- set and reset
def test_set_acts_from_the_next_push_and_reset_keeps_it(ctx, cases, wanted):
    f, p = cases["surf"]
    h, w = f.shape[:2]
    lut = ctx.jet_lut()
    open_case(ctx, f, p)
    out = outputs(w, h, p["grid_x"], p["grid_y"])
    d = dev_field(f)
    ctx.kinematics_push(d, **out.kw())
    compare(out.host(), ctx.kinematics_read(), wanted["surf"], "before set")
    ctx.kinematics_set(0.6, 0.0, 0.02, 0.25)
    p2 = dict(p, ow_k=0.6, omega_min=0.02, vis_max=0.25)
    info = ctx.kinematics_info()
    assert (info["ow_k"], info["ow_min"], info["omega_min"], info["vis_max"], info["pushes"]) == (0.6, 0.0, 0.02, 0.25, 1)
    ctx.kinematics_push(d, **out.kw())
    want = K.kinematics(f, lut, p2, pushes=2)
    assert want["summary"][2] < wanted["surf"]["summary"][2] and not np.array_equal(want["vis"], wanted["surf"]["vis"])
    compare(out.host(), ctx.kinematics_read(), want, "after set")
    ctx.kinematics_reset()
    info = ctx.kinematics_info()
    assert (info["ow_k"], info["omega_min"], info["vis_max"], info["pushes"]) == (0.6, 0.02, 0.25, 0)
    cells, sums, summ = ctx.kinematics_read()
    assert not sums.any() and all(summ[k] == 0 for k in KINEMATICS_SUMMARY)
    ctx.kinematics_push(d, **out.kw())
    compare(out.host(), ctx.kinematics_read(), K.kinematics(f, lut, p2, pushes=1), "after reset")
    ctx.kinematics_close()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx, cases, wanted):
    f, good = cases["ragged"]
    h, w = f.shape[:2]
    nc = good["grid_x"] * good["grid_y"]
    ctx.kinematics_close()
    for call in (ctx.kinematics_info, ctx.kinematics_read, ctx.kinematics_reset, lambda: ctx.kinematics_set(0.2, 0.0, 0.0, 0.5)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    lib, hdl = raw(ctx)
    assert lib.rcflow_kinematics_push_dev(hdl, 0, null, 0, null, 0, null, 0, null, 0, null, 0, null, 0, null, null, null) == ESTATE
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=-1), dict(radius=9), dict(sigma=0.0), dict(sigma=nan), dict(sigma=inf), dict(spacing=0), dict(spacing=9),
                dict(grid_x=0), dict(grid_y=0), dict(grid_x=w + 1), dict(grid_y=h + 1), dict(scale=0.0), dict(scale=nan), dict(scale=inf),
                dict(pixel_area=0.0), dict(pixel_area=-1.0), dict(pixel_area=nan), dict(ow_k=-0.1), dict(ow_k=nan), dict(ow_k=inf),
                dict(ow_min=-1.0), dict(ow_min=nan), dict(omega_min=-1.0), dict(omega_min=inf), dict(min_core=0), dict(vis_max=0.0),
                dict(vis_max=nan), dict(vis_max=inf)):
        with pytest.raises(RcflowError) as e:
            ctx.kinematics_open(w, h, **dict(good, **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    for bw, bh in ((2 * 5, h), (w, 2 * 5)):                       # m = 5: one pixel short of an interior
        with pytest.raises(RcflowError) as e:
            ctx.kinematics_open(bw, bh, **dict(good, grid_x=1, grid_y=1))
        assert e.value.code == EINVAL
    with pytest.raises(RcflowError) as e:
        ctx.kinematics_open(512, 512, **dict(good, grid_x=129, grid_y=128))                 # more than RC_RIPMAP_MAX_CELLS cells
    assert e.value.code == EINVAL
    p = KinematicsParams(radius=3, spacing=2, grid_x=5, grid_y=3, min_core=1, flags=2, sigma=1.2, scale=1.0, pixel_area=1.0, ow_k=0.5,
                         ow_min=0.0, omega_min=0.01, vis_max=0.5)
    assert lib.rcflow_kinematics_open(hdl, 0, w, h, C.byref(p)) == EINVAL     # unknown flag bits
    p.flags = 1
    assert lib.rcflow_kinematics_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_kinematics_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_kinematics_open(hdl, 0, 8192, 4100, C.byref(p)) == ESIZE            # beyond the context, which refuses first
    assert lib.rcflow_kinematics_open(hdl, 2, w, h, C.byref(p)) == EINVAL     # no such slot
    with pytest.raises(RcflowError):
        ctx.kinematics_info()                                     # nothing was opened by any of them

    open_case(ctx, f, good)
    assert lib.rcflow_kinematics_info(hdl, 0, None) == EINVAL     # no buffer
    d = dev_field(f)
    o = outputs(w, h, good["grid_x"], good["grid_y"])
    ctx.kinematics_push(d, **o.kw())
    before = ctx.kinematics_info()
    assert (before["w"], before["h"], before["radius"], before["spacing"], before["margin"], before["relative"], before["pushes"]) == (w, h, 3, 2, 5, True, 1)
    assert before["device_bytes"] >= w * h * 8 + nc * (K.SUMS * 16 + 48)
    for bad in (dict(radius=9), dict(vis_max=0.0)):               # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.kinematics_open(w, h, **dict(good, **bad))
    with pytest.raises(RcflowError) as e:
        ctx.kinematics_open(4000, 2160, **good)
    assert e.value.code == ESIZE and ctx.kinematics_info() == before

    big = torch.zeros(h * w * 8 + 256, dtype=torch.uint8, device="cuda")

    def push(flow=None, step=8 * w, omega=(null, 0), div=(null, 0), ow=(null, 0), mask=(null, 0), vis=(null, 0), cells=null, sums=null,
             summ=null, slot=0):
        fp = ptr(d) if flow is None else flow
        return lib.rcflow_kinematics_push_dev(hdl, slot, fp, step, omega[0], omega[1], div[0], div[1], ow[0], ow[1], mask[0], mask[1], vis[0],
                                              vis[1], cells, sums, summ)

    refused = [
        push(flow=null), push(step=8 * w - 8), push(step=8 * w + 4), push(flow=ptr(d, 4)),
        push(omega=(ptr(big), 4 * w - 4)), push(omega=(ptr(big), 4 * w + 2)), push(omega=(ptr(big, 2), 4 * w)),
        push(div=(ptr(big), 4 * w - 4)), push(div=(ptr(big, 1), 4 * w)), push(ow=(ptr(big), 4 * w + 2)), push(ow=(ptr(big, 2), 4 * w)),
        push(mask=(ptr(big), w - 1)), push(vis=(ptr(big), 3 * w - 1)), push(cells=ptr(big, 2)), push(sums=ptr(big, 4)), push(summ=ptr(big, 4)),
        push(mask=(ptr(d), w)),                                   # an output over the field
        push(flow=ptr(big, 16), omega=(ptr(big), 4 * w)),         # the field inside an output
        push(omega=(ptr(big), 4 * w), ow=(ptr(big, 4 * w * (h - 1)), 4 * w)),      # two outputs meeting in one row
        push(div=(ptr(big), 4 * w), mask=(ptr(big, 4 * w * h - 1), w)),
        push(vis=(ptr(big), 3 * w), cells=ptr(big, 3 * w * h // 4 * 4 - 4)),
        push(cells=ptr(big), sums=ptr(big, 8 * (nc * 6 - 1))),
        push(sums=ptr(big), summ=ptr(big, 8 * (nc * K.SUMS - 1))),
        push(mask=(ptr(big), w), summ=ptr(big, 0)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert push(slot=2) == EINVAL                                 # no such slot
    for bad in ((nan, 0.0, 0.0, 0.5), (-1.0, 0.0, 0.0, 0.5), (0.2, inf, 0.0, 0.5), (0.2, 0.0, -1.0, 0.5), (0.2, 0.0, 0.0, 0.0), (0.2, 0.0, 0.0, inf)):
        with pytest.raises(RcflowError) as e:
            ctx.kinematics_set(*bad)
        assert e.value.code == EINVAL
    assert ctx.kinematics_info() == before
    # nothing was queued and nothing changed: the second push gives what the statement gives
    ctx.kinematics_push(d, **o.kw())
    w2 = dict(wanted["ragged"], summary=wanted["ragged"]["summary"].copy())
    w2["summary"][6] = 2
    compare(o.host(), ctx.kinematics_read(), w2, "(after the refusals)")
    # an accepted boundary: the mask begins at the first byte after omega's range, in one allocation
    one = torch.full((5 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tl, tm = one[:4 * h * w].view(torch.float32).view(h, w), one[4 * h * w:5 * h * w].view(h, w)
    ctx.kinematics_push(d, omega=tl, mask=tm)
    assert np.array_equal(bits(tl.cpu().numpy()), bits(w2["omega"])) and np.array_equal(tm.cpu().numpy(), w2["mask"]) and (one[5 * h * w:] == SENTINEL).all()
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.kinematics_push(d, **o.kw())
        got = ctx.kinematics_read()
    torch.cuda.synchronize()
    w2["summary"][6] = 4
    compare(o.host(), got, w2, "(on another stream)")
    # re-open with another size replaces it
    f3, p3 = cases["no_smoothing"]
    open_case(ctx, f3, p3)
    assert ctx.kinematics_info()["w"] == 37 and ctx.kinematics_info()["pushes"] == 0
    o3 = outputs(37, 29, 37, 29)
    ctx.kinematics_push(dev_field(f3), **o3.kw())
    compare(o3.host(), ctx.kinematics_read(), wanted["no_smoothing"], "(after a re-open)")
    ctx.kinematics_close()
    ctx.kinematics_close()                                        # closing twice is fine


def test_two_slots(ctx, cases, wanted):
    (fa, pa), (fb, pb) = cases["surf"], cases["sliver_row"]
    open_case(ctx, fa, pa, stream=0)
    open_case(ctx, fb, pb, stream=1)
    oa = outputs(fa.shape[1], fa.shape[0], pa["grid_x"], pa["grid_y"])
    ob = outputs(fb.shape[1], fb.shape[0], pb["grid_x"], pb["grid_y"])
    ctx.kinematics_push(dev_field(fa), stream=0, **oa.kw())
    ctx.kinematics_push(dev_field(fb), stream=1, **ob.kw())
    compare(oa.host(), ctx.kinematics_read(stream=0), wanted["surf"], "(slot 0)")
    compare(ob.host(), ctx.kinematics_read(stream=1), wanted["sliver_row"], "(slot 1)")
    ctx.kinematics_close(stream=0)
    ctx.kinematics_close(stream=1)


# ---------------------------------------------------------------------------- the object
def test_product_object_holds_its_arguments_to_the_session(ctx, cases, wanted):
    f, p = cases["pair"]
    h, w = f.shape[:2]
    with Kinematics(ctx, w, h, **p) as kn:
        assert kn.info()["margin"] == 3 and kn.info()["relative"] is False
        out = outputs(w, h, p["grid_x"], p["grid_y"])
        kn.push(dev_field(f), **out.kw())
        compare(out.host(), kn.read(), wanted["pair"], "(through api.Kinematics)")
        for bad in (dict(omega=torch.zeros((h, w + 1), dtype=torch.float32, device="cuda")),
                    dict(mask=torch.zeros((h, w), dtype=torch.float32, device="cuda")),
                    dict(vis=torch.zeros((h, w), dtype=torch.uint8, device="cuda")),
                    dict(cells=torch.zeros(p["grid_x"] * p["grid_y"] * 48 - 1, dtype=torch.uint8, device="cuda")),
                    dict(sums=torch.zeros(p["grid_x"] * p["grid_y"] * K.SUMS, dtype=torch.int32, device="cuda")),
                    dict(summary=torch.zeros(8, dtype=torch.int64))):
            with pytest.raises(ValueError):
                kn.push(dev_field(f), **bad)
        with pytest.raises(ValueError):
            kn.push(dev_field(f[:, :-1]))
        with pytest.raises(ValueError):
            kn.push(f)
        assert kn.info()["pushes"] == 1
        kn.set(0.2, 6.0, 2.0, 20.0)
        assert kn.info()["ow_min"] == 6.0
        kn.reset()
        assert kn.info()["pushes"] == 0
    with pytest.raises(RcflowError) as e:
        ctx.kinematics_info()
    assert e.value.code == ESTATE
