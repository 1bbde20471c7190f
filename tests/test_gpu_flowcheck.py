"""The flow check on the device (flowcheck_kernels.hip) against its numpy statement (tests/_flowcheck_ref.py): the flags, the mask,
the checked field, the residuals, the texture, the picture, the cell sums, the records and the summary of every push, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _flowcheck_ref as F
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, Outputs, Padded, ptr, raw, same_bits
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RC_FLOWCHECK_LAUNCHES, FlowcheckInfo, FlowcheckParams, RcflowError
from ripcurrents_amd.api import FLOWCHECK_CELL_DTYPE, FLOWCHECK_SUMMARY, FlowCheck

pytestmark = pytest.mark.gpu

IMAGES = F.PICTURES
ARRAYS = ("cells", "sums", "summary")
FLOATS = ("checked", "resid", "texture")
FC_TW, FC_TH = 64, 16                                             # flowcheck_kernels.hip: a block's tile
SHIFT = (1.25, -0.75)
dev = Padded.of
_CLIPS = {}


def clip(w, h, frames=2, shift=SHIFT):
    key = (w, h, frames, shift)
    if key not in _CLIPS:
        _CLIPS[key] = synth.translating_clip(w, h, frames, *shift)
    return _CLIPS[key]


def views(d):
    if "cells" in d:
        d["cells"] = d["cells"].view(FLOWCHECK_CELL_DTYPE)
    if "sums" in d:
        d["sums"] = d["sums"].reshape(-1, F.SUMS)


def outputs(p, w, h, pad=0):
    nc = p.grid_x * p.grid_y
    planes = dict(flags=((h, w), torch.uint8), mask=((h, w), torch.uint8), checked=((h, w, 2), torch.float32), resid=((h, w, 2), torch.float32),
                  texture=((h, w), torch.float32), picture=((h, w, 3), torch.uint8))
    flat = dict(cells=((nc * 32,), torch.uint8, None), sums=((nc * F.SUMS,), torch.int64, -1), summary=((F.SUMMARY_WORDS,), torch.int64, -1))
    return Outputs(planes, flat, pad, views)


def same(k, a, b):
    if k in FLOATS:
        return same_bits(a, b)
    if k == "cells":
        return all(a[f].tobytes() == b[f].tobytes() for f in b.dtype.names)
    return np.array_equal(a, b)


def compare(got, read, want, what):
    for k in got:
        assert same(k, got[k], want[k]), "%s differs %s: %s, wanted %s" % (k, what, got[k], want[k])
    if read is not None:
        rc, rs, rsum = read
        assert same("cells", rc.ravel(), want["cells"]), "the slot's records differ " + what
        assert np.array_equal(rs.reshape(-1, F.SUMS), want["sums"]), "the slot's sums differ " + what
        assert [rsum[k] for k in FLOWCHECK_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


def with_(p, **kw):
    return F.Params(**{**F.asdict(p), **kw})


def patch(w, h):
    return (slice(h // 3, 2 * h // 3), slice(w // 3, 2 * w // 3))


def field(kind, w, h):
    true = F.constant_field(w, h, *SHIFT)
    if kind == "true":
        return true
    if kind == "noisy":
        return F.noisy_patch(true, patch=patch(w, h))
    if kind == "hostile":
        return F.hostile(F.noisy_patch(true, patch=patch(w, h)), seed=w)
    assert kind == "edges"
    return F.edge_field(w, h)


def back_field(kind, w, h):
    if kind is None:
        return None
    b = F.noisy_patch(F.constant_field(w, h, -SHIFT[0], -SHIFT[1]), amp=1.5, seed=11, patch=patch(w, h))
    return F.hostile(b, seed=5) if kind == "bad" else b


def once(ctx, w, h, p, fld, back=None, pad=0, stream=0, close=True):
    """one explicit pair through a fresh session and the statement -> the statement's outputs"""
    prev, nxt = clip(w, h)
    ctx.flowcheck_open(w, h, stream=stream, **p.kw())
    info = ctx.flowcheck_info(stream=stream)
    assert info["launches_per_push"] == RC_FLOWCHECK_LAUNCHES == 2 and info["held"] == 0
    out = outputs(p, w, h, pad)
    d = [dev(prev, pad), dev(nxt, pad), dev(fld, pad)] + ([dev(back, pad)] if back is not None else [])
    ctx.flowcheck_push(d[1].view, d[0].view, d[2].view, d[3].view if back is not None else None, stream=stream, **out.kw())
    want = F.check(prev, nxt, fld, back, p)
    compare(out.host(), ctx.flowcheck_read(stream=stream), want, "(%d x %d, radius %d)" % (w, h, p.radius))
    for x, a in zip(d, [prev, nxt, fld, back]):
        assert np.ascontiguousarray(x.view.cpu().numpy()).tobytes() == np.ascontiguousarray(a).tobytes(), "an input was written"
        x.check("an input")
    if close:
        ctx.flowcheck_close(stream=stream)
    return want


BUSY = F.Params(radius=4, grid_x=5, grid_y=4, tests=F.TESTS, tex_min=3, gain_pm=700, res_max=1.5, fb_rel=0.01, speed_max=3.5)


# ---------------------------------------------------------------------------- sizes, radii
@pytest.mark.parametrize("radius", [0, 1, 4, 7])
@pytest.mark.parametrize("w,h", [(37, 29), (131, 67), (FC_TW + 7 + 2, FC_TH + 7 + 2)])
def test_sizes_and_radii_with_padded_steps(ctx, w, h, radius):
    """37 x 29: smaller than a tile, the window clipped on all sides at radius 7; 131 x 67: three tiles by five, ragged last tiles;
    73 x 25: just above one tile of 64 x 16 plus the halo of 7 plus the gradient's pixel.  Every test on, a back field with BAD
    samples, a grid with remainder cells.  At radius 0 the tensor of one pixel has no smaller eigenvalue: every sample is FLAT"""
    want = once(ctx, w, h, with_(BUSY, radius=radius), field("hostile", w, h), back_field("bad", w, h), pad=3)
    s = want["sides"]
    assert (s["Nr"] < s["N"]).any() and (want["summary"][0] > 0 or radius == 0) and all(want["summary"][k] > 0 for k in (1, 4, 6))
    assert s["N"].min() == (radius + 1) ** 2 and s["N"].max() == (2 * radius + 1) ** 2


# ---------------------------------------------------------------------------- fields
@pytest.mark.parametrize("back", [None, "good", "bad"])
@pytest.mark.parametrize("kind", ["true", "noisy", "hostile", "edges"])
def test_fields_and_back_fields(ctx, kind, back):
    w, h = 131, 67
    want = once(ctx, w, h, with_(BUSY, speed_max=3.0), field(kind, w, h), back_field(back, w, h), pad=1)
    fl = want["flags"]
    if kind == "true":
        assert want["summary"][0] > 0.6 * w * h and not (fl & F.BAD).any()
    if kind == "noisy":
        assert (fl[patch(w, h)] & F.RESID).any() and (fl & F.FAST).any()
    if kind == "hostile":
        assert (fl == F.BAD).any() and (want["sides"]["Nr"] < want["sides"]["N"])[8:-8, 8:-8].any()
    if kind == "edges":
        assert (fl[:, 0] & F.OUT).all() and (fl[:, w - 1] & F.OUT).all() and (fl[0, 1:w - 1] & F.OUT).all() and (fl[h - 1, 1:w - 1] & F.OUT).all()
        assert not (fl[1:h - 1, w - 2] & F.OUT).any() and not (fl[h - 2, 1:w - 2] & F.OUT).any()
    assert bool(want["summary"][6]) == (back is not None)


# ---------------------------------------------------------------------------- grids
@pytest.mark.parametrize("w,h,gx,gy", [(131, 67, 1, 1), (131, 67, 7, 5), (131, 67, 2, 67), (160, 128, 128, 128)])
def test_grids(ctx, w, h, gx, gy):
    """one cell: every lane of every block adds to one cell; 7 x 5 with remainder columns and rows, a wave's pixels in several
    cells; 2 x 67: a cell row a pixel row; 128 x 128 = RC_RIPMAP_MAX_CELLS cells of a pixel (the last a remainder):
    1024 cells under a block, more than its table in LDS holds, so its sums go straight to memory"""
    assert gx * gy <= F.MAX_CELLS
    want = once(ctx, w, h, with_(BUSY, radius=2, grid_x=gx, grid_y=gy), field("hostile", w, h), pad=2)
    assert want["cells"]["pixels"].sum() == w * h and want["sums"][:, 0].sum() == want["summary"][0] and want["cells"].size == gx * gy


# ---------------------------------------------------------------------------- lifecycle
def test_each_output_alone_and_none(ctx):
    """what a push asks for changes nothing of what it gives"""
    w, h, p = 73, 25, with_(BUSY, radius=2)
    prev, nxt = clip(w, h)
    fld, back = field("hostile", w, h), back_field("good", w, h)
    want = F.check(prev, nxt, fld, back, p)
    ctx.flowcheck_open(w, h, **p.kw())
    d = [dev(a, 1) for a in (prev, nxt, fld, back)]
    out = outputs(p, w, h, 2)
    for n, only in enumerate([()] + [(k,) for k in IMAGES + ARRAYS] + [IMAGES + ARRAYS]):
        ctx.flowcheck_push(d[1].view, d[0].view, d[2].view, d[3].view, **out.kw(only))
        got = out.host()
        w2 = dict(want, summary=np.concatenate([want["summary"][:8], [n + 1, n + 1]]))
        compare({k: got[k] for k in only}, ctx.flowcheck_read(), w2, "asking %s" % (only,))
    ctx.flowcheck_close()


def test_held_frame_against_the_explicit_call(ctx):
    """the first push with no previous frame only stores its frame; the second uses it, the third the second's; each equals the call
    that names both frames"""
    w, h, p = 131, 67, with_(BUSY, radius=1)
    c = clip(w, h, 4)
    fld = field("noisy", w, h)
    ref = F.FlowCheckRef(w, h, p)
    ctx.flowcheck_open(w, h, **p.kw())
    out = outputs(p, w, h, 1)
    d = [dev(x, 1) for x in c]
    df = dev(fld, 1)
    ctx.flowcheck_push(d[0].view, None, df.view, **out.kw())
    assert ref.push(c[0], None, fld) is None
    info = ctx.flowcheck_info()
    assert (info["pushes"], info["computing"], info["held"]) == (1, 0, 1)
    host = out.host()                                             # nothing was written: the sentinel bytes stand
    assert (host["flags"] == 0xA5).all() and (host["summary"] == -1).all() and (host["picture"] == 0xA5).all()
    rc, rs, rsum = ctx.flowcheck_read()
    assert not rs.any() and [rsum[k] for k in FLOWCHECK_SUMMARY] == [0] * 8 + [0, 1]
    for t in (1, 2):
        ctx.flowcheck_push(d[t].view, None, df.view, **out.kw())
        want = ref.push(c[t], None, fld)
        compare(out.host(), ctx.flowcheck_read(), want, "push %d on the held frame" % t)
        explicit = F.check(c[t - 1], c[t], fld, None, p, t, t + 1)
        assert np.array_equal(want["flags"], explicit["flags"]) and same_bits(want["resid"], explicit["resid"])
    ctx.flowcheck_push(d[3].view, d[2].view, df.view, **out.kw())     # and a named previous frame while one is held
    compare(out.host(), ctx.flowcheck_read(), ref.push(c[3], c[2], fld), "the explicit call")
    ctx.flowcheck_close()


def test_set_between_pushes_and_reset(ctx):
    w, h, p = 73, 25, with_(BUSY, radius=2, grid_x=3, grid_y=2)
    c = clip(w, h, 4)
    fld, back = field("hostile", w, h), back_field("good", w, h)
    ref = F.FlowCheckRef(w, h, p)
    ctx.flowcheck_open(w, h, **p.kw())
    out = outputs(p, w, h)
    d, df, db = [dev(x) for x in c], dev(fld), dev(back)

    def push(t, named=False):
        ctx.flowcheck_push(d[t].view, d[t - 1].view if named else None, df.view, db.view, **out.kw())
        compare(out.host(), ctx.flowcheck_read(), ref.push(c[t], c[t - 1] if named else None, fld, back), "push of frame %d" % t)
    push(1, named=True)
    new = dict(tests=F.RESID | F.FB, tex_min=0, res_max=0.75, gain_pm=0, fb_rel=0.0, fb_abs=0.25, speed_max=0.0)
    ctx.flowcheck_set(**new)
    ref.set(**new)
    info = ctx.flowcheck_info()
    assert {k: info[k] for k in new} == new and info["pushes"] == 1
    push(2)
    ctx.flowcheck_reset()
    ref.reset()
    info = ctx.flowcheck_info()
    assert {k: info[k] for k in new} == new and (info["pushes"], info["computing"], info["held"]) == (2, 2, 0)
    rc, rs, rsum = ctx.flowcheck_read()
    assert not rc.view(np.uint8).any() and not rs.any() and [rsum[k] for k in FLOWCHECK_SUMMARY] == [0] * 8 + [2, 2]
    with pytest.raises(RcflowError) as e:
        ctx.flowcheck_push(d[3].view, None, df.view, **out.kw())  # no frame is held and this is not the first push
    assert e.value.code == ESTATE and ctx.flowcheck_info()["pushes"] == 2
    push(3, named=True)
    push(0)                                                       # the frame of the push before is held again
    ctx.flowcheck_close()


def test_two_slots_interleaved(ctx):
    (wa, ha, pa), (wb, hb, pb) = (73, 25, with_(BUSY, radius=1)), (37, 29, with_(BUSY, radius=7, grid_x=2, grid_y=3, fill="zero"))
    ca, cb = clip(wa, ha, 3), clip(wb, hb, 3)
    fa, fb = field("noisy", wa, ha), field("hostile", wb, hb)
    ra, rb = F.FlowCheckRef(wa, ha, pa), F.FlowCheckRef(wb, hb, pb)
    ctx.flowcheck_open(wa, ha, stream=0, **pa.kw())
    ctx.flowcheck_open(wb, hb, stream=1, **pb.kw())
    oa, ob = outputs(pa, wa, ha), outputs(pb, wb, hb, 1)
    for t in range(3):
        ctx.flowcheck_push(dev(ca[t]).view, None, dev(fa).view, stream=0, **oa.kw())
        ctx.flowcheck_push(dev(cb[t], 1).view, None, dev(fb, 1).view, stream=1, **ob.kw())
        wa_, wb_ = ra.push(ca[t], None, fa), rb.push(cb[t], None, fb)
        if t:
            compare(oa.host(), ctx.flowcheck_read(stream=0), wa_, "slot 0, push %d" % t)
            compare(ob.host(), ctx.flowcheck_read(stream=1), wb_, "slot 1, push %d" % t)
    assert not np.isnan(ob.host()["checked"]).any() and (wb_["flags"] != 0).any()       # the fill is zero
    ctx.flowcheck_close(stream=1)
    assert ctx.flowcheck_info(stream=0)["pushes"] == 3
    ctx.flowcheck_close(stream=0)


def test_resident_field_into_the_check_and_checked_field_into_the_mean_current(ctx):
    """End to end on the 160 x 120 translating clip: the project's own Farneback field (the frame-at-a-time entry, the parameters
    of the reference's ripcurrents.cpp:215) is checked at radius 4, res_max 1.5, tex_min 1 with no back field; d_checked with NaN at
    the rejected pixels goes into the mean current, whose newest-bad count is w h minus the VALID count, exactly; and the device's
    flags equal the numpy statement's on the same field.  The share of VALID pixels at least 8 px inside the frame was measured on
    an MI355X with this test (device and statement agree exactly): 52 of those 14976 pixels are rejected, 0.9965 are VALID (16836 of
    the picture's 19200); the bound is 1.5 times the rejected share measured, the margin convention of the PIV test's recovery bounds"""
    w, h = 160, 120
    prev, nxt = clip(w, h)
    ctx.stream_reset()
    assert ctx.push_frame_host(prev) is None
    flow = ctx.push_frame_host(nxt)
    p = F.Params(radius=4, grid_x=4, grid_y=3, tests=F.FLAT | F.RESID, res_max=1.5, tex_min=1)
    ctx.flowcheck_open(w, h, **p.kw())
    out = outputs(p, w, h)
    ctx.flowcheck_push(dev(nxt).view, dev(prev).view, None, **out.kw())
    got = out.host()
    want = F.check(prev, nxt, flow.cpu().numpy(), None, p)
    compare(got, ctx.flowcheck_read(), want, "(the resident Farneback field)")
    ctx.meanflow_open(w, h, window=2, grid_x=4, grid_y=3, min_fill=1)
    ctx.meanflow_push(out.t["checked"])
    _, _, ms = ctx.meanflow_read()
    assert ms["bad"] == w * h - int(got["summary"][0]) and ms["bad"] > 0
    inside = np.zeros((h, w), bool)
    inside[8:-8, 8:-8] = True
    rejected = float((got["flags"][inside] != 0).mean())
    print("rejected share 8 px inside the frame: %.6f (device) %.6f (statement); VALID over the picture %d of %d" % (
        rejected, float((want["flags"][inside] != 0).mean()), int(got["summary"][0]), w * h))
    assert rejected <= 1.5 * MEASURED_REJECTED_SHARE
    ctx.meanflow_close()
    ctx.flowcheck_open(128, 96, **p.kw())
    with pytest.raises(RcflowError) as e:
        ctx.flowcheck_push(dev(clip(128, 96)[1]).view, dev(clip(128, 96)[0]).view, None)
    assert e.value.code == ESIZE                                  # the resident field has another size
    ctx.stream_reset()
    with pytest.raises(RcflowError) as e:
        ctx.flowcheck_push(dev(clip(128, 96)[1]).view, dev(clip(128, 96)[0]).view, None)
    assert e.value.code == ESTATE and ctx.flowcheck_info()["pushes"] == 0
    ctx.flowcheck_close()


MEASURED_REJECTED_SHARE = 52 / 14976                                  # of the pixels 8 px inside the frame; see the test above


def test_product_object(ctx):
    w, h, p = 73, 25, with_(BUSY, radius=1)
    c = clip(w, h, 3)
    fld = field("noisy", w, h)
    ref = F.FlowCheckRef(w, h, p)
    with FlowCheck(ctx, w, h, **p.kw()) as fc:
        mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        for t in range(3):
            fc.push(dev(c[t]).view, flow=dev(fld).view, mask=mask)
            want = ref.push(c[t], None, fld)
        rc, rs, rsum = fc.read()
        assert same("cells", rc.ravel(), want["cells"]) and rsum["pushes"] == 3 and rsum["computing"] == 2 and np.array_equal(mask.cpu().numpy(), want["mask"])
        assert fc.info()["fill"] == "nan" and fc.info()["held"] == 1
        with pytest.raises(ValueError):
            fc.push(dev(c[0][:, :-1]).view, flow=dev(fld).view)   # a frame of another size
        fc.set(F.RESID, 0, 2.0, 0, 0.0, 0.0, 0.0)
        fc.reset()
        assert fc.info()["held"] == 0 and fc.info()["tests"] == F.RESID and fc.info()["res_max"] == 2.0
    with pytest.raises(RcflowError):
        ctx.flowcheck_info()


# ---------------------------------------------------------------------------- arguments and refusals
def test_refusals_leave_state_and_outputs_untouched(ctx):
    w, h = 40, 24
    good = with_(BUSY, radius=2, grid_x=4, grid_y=3)
    nc = good.grid_x * good.grid_y
    ctx.flowcheck_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.flowcheck_info, ctx.flowcheck_read, ctx.flowcheck_reset, lambda: ctx.flowcheck_set(F.TESTS, 1, 1.5, 0, 0.01, 0.5, 10.0)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 1024)()
    for name, args in (("info", (C.byref(FlowcheckInfo()),)), ("read", (buf, buf, buf)), ("reset", ()), ("set", (F.TESTS, 1, 1.5, 0, 0.01, 0.5, 10.0)),
                       ("push_dev", (null, 0) * 10 + (null, null, null))):
        assert getattr(lib, "rcflow_flowcheck_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_flowcheck_%s:" % name), text()
    nan, inf = float("nan"), float("inf")
    kw = good.kw()
    for bad in (dict(radius=-1), dict(radius=8), dict(tests=128), dict(tests=1), dict(tests=F.TESTS | 2), dict(tex_min=-1), dict(tex_min=65026),
                dict(gain_pm=-1), dict(gain_pm=1001), dict(res_max=-0.5), dict(res_max=255.5), dict(res_max=nan), dict(fb_rel=-0.1), dict(fb_rel=1.5),
                dict(fb_rel=nan), dict(fb_abs=-1.0), dict(fb_abs=500.5), dict(fb_abs=inf), dict(speed_max=-1.0), dict(speed_max=1000.5),
                dict(speed_max=nan), dict(grid_x=0), dict(grid_x=41), dict(grid_y=25)):
        assert bad.get("tests") in (1, F.TESTS | 2) or F.open_error(w, h, with_(good, **bad)) in ("parameters", "grid")
        with pytest.raises(RcflowError) as e:
            ctx.flowcheck_open(w, h, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_flowcheck_open"), bad
    p = FlowcheckParams(radius=2, grid_x=4, grid_y=3, tests=F.TESTS, flags=0, tex_min=1, gain_pm=0, res_max=1.5, fb_rel=0.01, fb_abs=0.5, speed_max=10.0)
    for flags in (0, 3, 4):                                       # neither fill, both, an unknown one
        p.flags = flags
        assert lib.rcflow_flowcheck_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "exactly one" in text()
    p.flags = 1
    assert lib.rcflow_flowcheck_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_flowcheck_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_flowcheck_open(hdl, 2, w, h, C.byref(p)) == EINVAL              # no such slot
    with pytest.raises(RcflowError) as e:
        ctx.flowcheck_open(4000, 2161, **kw)                          # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_flowcheck_open")
    with pytest.raises(RcflowError):
        ctx.flowcheck_info()                                          # nothing was left open by any of them

    c = clip(w, h, 3)
    fld, back = field("hostile", w, h), back_field("good", w, h)
    ref = F.FlowCheckRef(w, h, good)
    ctx.flowcheck_open(w, h, **kw)
    out = outputs(good, w, h, 2)
    d, df, db = [dev(x) for x in c], dev(fld), dev(back)
    ctx.flowcheck_push(d[1].view, d[0].view, df.view, db.view, **out.kw())
    first = ref.push(c[1], c[0], fld, back)
    kept = out.host()
    compare(kept, ctx.flowcheck_read(), first, "(before the refusals)")
    assert lib.rcflow_flowcheck_info(hdl, 0, None) == EINVAL
    before = ctx.flowcheck_info()
    for bad in (dict(radius=9), dict(tests=256)):                     # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.flowcheck_open(w, h, **dict(kw, **bad))
    assert ctx.flowcheck_info() == before
    big = torch.zeros(64 * h * w + 4096, dtype=torch.uint8, device="cuda")
    N = (null, 0)
    o = out.t

    def im(t, off=0, step=None):
        return (ptr(t, off), t.stride(0) * t.element_size() if step is None else step)

    def push(nxt=None, prev=None, flow=None, back=N, flags=N, mask=N, checked=N, resid=N, texture=N, pic=N, cells=null, sums=null, summ=null, slot=0):
        return lib.rcflow_flowcheck_push_dev(hdl, slot, *(nxt or im(d[2].view)), *(prev or im(d[1].view)), *(flow or im(df.view)), *back, *flags, *mask,
                                             *checked, *resid, *texture, *pic, cells, sums, summ)

    refused = [
        push(nxt=(null, w)), push(nxt=im(d[2].view, step=w - 1)), push(prev=im(d[1].view, step=w - 1)),
        push(flow=im(df.view, step=8 * w - 8)), push(flow=im(df.view, step=8 * w + 4)), push(flow=im(df.view, 4)),
        push(back=im(db.view, step=8 * w - 8)), push(back=im(db.view, 4)),
        push(flags=im(o["flags"], step=w - 1)), push(mask=im(o["mask"], step=w - 1)), push(pic=im(o["picture"], step=3 * w - 1)),
        push(checked=im(o["checked"], 4)), push(checked=im(o["checked"], step=8 * w + 4)), push(resid=im(o["resid"], 4)),
        push(resid=im(o["resid"], step=8 * w - 8)), push(texture=im(o["texture"], 2)), push(texture=im(o["texture"], step=4 * w + 2)),
        push(cells=ptr(big, 2)), push(sums=ptr(big, 4)), push(summ=ptr(big, 4)),
        push(checked=im(df.view)),                                    # d_checked over the field: a block reads its neighbours' vectors
        push(checked=im(db.view), back=im(db.view)),                  # over the backward field
        push(mask=im(d[2].view)), push(flags=im(d[1].view)),          # an output over a frame
        push(flags=(ptr(big), w), mask=(ptr(big, w * (h - 1)), w)),   # two outputs meeting in one row
        push(resid=(ptr(big), 8 * w), texture=(ptr(big, 8), 4 * w)), push(cells=ptr(big), sums=ptr(big, 32 * nc - 8)),
        push(sums=ptr(big), summ=ptr(big, 80 * nc - 8)), push(pic=(ptr(big), 3 * w), summ=ptr(big)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert text().startswith("rcflow_flowcheck_push_dev")
    assert push(slot=2) == EINVAL
    for bad in ((128, 1, 1.5, 0, 0.01, 0.5, 10.0), (F.TESTS, -1, 1.5, 0, 0.01, 0.5, 10.0), (F.TESTS, 1, 256.0, 0, 0.01, 0.5, 10.0),
                (F.TESTS, 1, 1.5, 1001, 0.01, 0.5, 10.0), (F.TESTS, 1, 1.5, 0, nan, 0.5, 10.0), (F.TESTS, 1, 1.5, 0, 0.01, -0.5, 10.0),
                (F.TESTS, 1, 1.5, 0, 0.01, 0.5, inf)):
        with pytest.raises(RcflowError) as e:
            ctx.flowcheck_set(*bad)
        assert e.value.code == EINVAL and text().startswith("rcflow_flowcheck_set")
    assert ctx.flowcheck_info() == before
    # the outputs of the push before stand as they were, with their fences; the slot's records too
    compare(out.host(), ctx.flowcheck_read(), first, "(after the refusals)")
    # nothing was queued and nothing changed: the held frame is still the first push's d_next
    ctx.flowcheck_push(d[2].view, None, df.view, db.view, **out.kw())
    compare(out.host(), ctx.flowcheck_read(), ref.push(c[2], None, fld, back), "(the push after the refusals)")
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.flowcheck_push(d[0].view, None, df.view, db.view, **out.kw())
        got = ctx.flowcheck_read()
    torch.cuda.synchronize()
    compare(out.host(), got, ref.push(c[0], None, fld, back), "(on another stream)")
    ctx.flowcheck_close()                                             # closing twice is fine
    ctx.flowcheck_close()
