"""The flow infill on the device (infill_kernels.hip) against its numpy statement (tests/_infill_ref.py): the filled field, the source
byte, the mask, the picture, the cell sums, the records and the summary of every push, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _drifters_ref as D
import _flowcheck_ref as F
import _ftle_ref as T
import _infill_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, Outputs, Padded, ptr, raw, same_bits
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RC_INFILL_LAUNCHES, InfillInfo, InfillParams, RcflowError
from ripcurrents_amd.api import INFILL_CELL_DTYPE, INFILL_SUMMARY, Infill

pytestmark = pytest.mark.gpu

IMAGES = R.PICTURES
ARRAYS = ("cells", "sums", "summary")
IF_TW, IF_TH = 64, 16                                             # infill_kernels.hip: a block's tile
dev = Padded.of
_FIELDS = {}


def shear(w, h):
    """the statement's shear with its jet, cut or repeated to w x h"""
    if (w, h) not in _FIELDS:
        f = R.shear_field()
        _FIELDS[(w, h)] = np.ascontiguousarray(np.tile(f, ((h + 119) // 120, (w + 159) // 160, 1))[:h, :w])
    return _FIELDS[(w, h)]


def views(d):
    if "cells" in d:
        d["cells"] = d["cells"].view(INFILL_CELL_DTYPE)
    if "sums" in d:
        d["sums"] = d["sums"].reshape(-1, R.SUMS)


def outputs(p, w, h, pad=0):
    nc = p.grid_x * p.grid_y
    planes = dict(filled=((h, w, 2), torch.float32), source=((h, w), torch.uint8), mask=((h, w), torch.uint8), picture=((h, w, 3), torch.uint8))
    flat = dict(cells=((nc * 32,), torch.uint8, None), sums=((nc * R.SUMS,), torch.int64, -1), summary=((R.SUMMARY_WORDS,), torch.int64, -1))
    return Outputs(planes, flat, pad, views)


def same(k, a, b):
    if k == "filled":
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
        assert np.array_equal(rs.reshape(-1, R.SUMS), want["sums"]), "the slot's sums differ " + what
        assert [rsum[k] for k in INFILL_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


def with_(p, **kw):
    return R.Params(**{**R.asdict(p), **kw})


class Session:
    """the device session and the statement side by side"""

    def __init__(self, ctx, w, h, p, pad=0, stream=0):
        self.ctx, self.w, self.h, self.pad, self.stream = ctx, w, h, pad, stream
        self.ref = R.InfillRef(w, h, p, ctx.jet_lut())
        ctx.infill_open(w, h, stream=stream, **p.kw())
        info = ctx.infill_info(stream=stream)
        assert info["launches_per_push"] == (RC_INFILL_LAUNCHES if p.levels >= 5 else RC_INFILL_LAUNCHES - 1) and RC_INFILL_LAUNCHES == 4
        assert info["pushes"] == 0 and info["device_bytes"] >= 5 * w * h
        self.out = outputs(p, w, h, pad)

    def push(self, flow, valid=None, domain=None, what="", only=None):
        want = self.ref.push(flow, valid, domain)
        d = [None if a is None else dev(a, self.pad) for a in (flow, valid, domain)]
        self.ctx.infill_push(*[None if x is None else x.view for x in d], stream=self.stream, **self.out.kw(only))
        got = self.out.host()
        compare(got if only is None else {k: got[k] for k in only}, self.ctx.infill_read(stream=self.stream), want,
                "after push %d %s" % (self.ref.pushes, what))
        for x, a in zip(d, (flow, valid, domain)):
            if a is not None:
                assert np.ascontiguousarray(x.view.cpu().numpy()).tobytes() == np.ascontiguousarray(a).tobytes(), "an input was written"
                x.check("an input")
        assert self.ctx.infill_info(stream=self.stream)["pushes"] == self.ref.pushes
        return want

    def close(self):
        self.ctx.infill_close(stream=self.stream)


def once(ctx, w, h, p, flow, valid=None, domain=None, pad=0):
    s = Session(ctx, w, h, p, pad)
    want = s.push(flow, valid, domain, "(%d x %d, %s)" % (w, h, p))
    s.close()
    return want


# ---------------------------------------------------------------------------- sizes, levels
@pytest.mark.parametrize("levels", [1, 3, 4, 5, 7])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (37, 29), (129, 65), (IF_TW + 9, IF_TH + 9), (301, 263)])
def test_sizes_and_levels_with_padded_steps(ctx, w, h, levels):
    """1 x 1 and 5 x 3: levels that are one cell; 37 x 29: smaller than a tile; 129 x 65: odd at every level; 73 x 25: just
    above one tile; 301 x 263: 38 x 33 = 1254 cells at level 3, 19 x 17 at level 4.  Levels 4 and 5: either side of the level at which
    the one workgroup of infill@1 takes over from the tiles.  p900 leaves holes that reach the coarse levels, a grid with remainder
    cells where it fits"""
    g = (min(3, w), min(2, h))
    want = once(ctx, w, h, R.Params(levels=levels, grid_x=g[0], grid_y=g[1]), shear(w, h), R.pattern("p900", w, h), pad=3)
    if w * h > 100:
        assert want["summary"][0] > 0 and want["summary"][2] > 0 and want["source"].max() >= min(levels, 2)
    if (w, h) == (301, 263) and levels == 1:
        assert want["summary"][3] > 0


def test_more_cells_than_threads_in_the_one_workgroup(ctx):
    """1100 x 1000: 35 x 32 = 1120 cells at level 5, more than the 1024 threads of infill@1, so its loop over a level's cells runs
    twice; holes in blocks so that the values come from the levels that launch pushes"""
    w, h = 1100, 1000
    y, x = np.mgrid[0:h, 0:w]
    valid = np.where(((x // 48 + y // 48) % 3 == 0) & ((x + 7 * y) % 11 == 0), 255, 0).astype(np.uint8)
    want = once(ctx, w, h, R.Params(levels=7, min_known=3, grid_x=5, grid_y=4), shear(w, h), valid, pad=1)
    assert want["summary"][3] == 0 and want["summary"][8 + 6] > 0 and want["summary"][8 + 7] > 0


# ---------------------------------------------------------------------------- patterns
@pytest.mark.parametrize("name", ["all", "none", "corners", "p300", "p900", "block40"])
def test_patterns(ctx, name):
    w, h = 131, 67
    f = shear(w, h)
    want = once(ctx, w, h, R.Params(levels=7, grid_x=5, grid_y=4), f, R.pattern(name, w, h), pad=1)
    sm = want["summary"]
    if name == "all":
        assert sm[0] == w * h and same_bits(want["filled"], f)
    if name == "none":
        assert sm[3] == w * h and np.isnan(want["filled"]).all()
    if name == "corners":
        assert sm[0] == 4 and sm[2] == w * h - 4
    if name == "block40":
        assert sm[3] == 0 and want["source"].max() >= 4


@pytest.mark.parametrize("levels", [2, 7])
def test_hostile_field(ctx, levels):
    """NaN, +-inf, +-500.0, +-499.99, -0.0 and denormals; finite vectors with a valid byte of 0 and NaN with a byte of 255"""
    w, h = 131, 67
    f = R.hostile(shear(w, h), seed=4)
    v = R.pattern("p300", w, h)
    want = once(ctx, w, h, R.Params(levels=levels, grid_x=4, grid_y=3), f, v, pad=2)
    s = want["sides"]
    assert (s["bad"] & (v != 0)).any() and (~s["bad"] & (v == 0)).any() and (s["known"] & (f[..., 0] == 0) & np.signbit(f[..., 0])).any()
    assert same_bits(want["filled"][s["known"]], f[s["known"]])
    once(ctx, w, h, R.Params(levels=levels), f, None)             # and with no valid mask


def test_saturated_field_at_the_int32_bound(ctx):
    """every vector +-499.99 (q = 31999), 256 x 256 with the signs in blocks of 128: cells of level 7 hold 16384 known pixels of one
    sign, |SX| = 524271616, the bound of the statement; holes so that the means are used"""
    w, h = 256, 256
    f = R.saturated(w, h)
    want = once(ctx, w, h, R.Params(levels=7, min_known=16384 - 4000, grid_x=2, grid_y=2), f, R.pattern("p100", w, h))
    assert (want["source"] == 7).any() and np.abs(want["sides"]["Fx"]).max() == 31999
    want = once(ctx, w, h, R.Params(levels=7, min_known=16384), f, None)
    assert want["summary"][0] == w * h


# ---------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("leave", ["nan", "zero"])
@pytest.mark.parametrize("min_known", [1, 2, 4, 16, 64, 16384])
def test_min_known_and_both_patterns(ctx, min_known, leave):
    w, h = 131, 67
    want = once(ctx, w, h, R.Params(levels=7, min_known=min_known, grid_x=3, grid_y=3, leave=leave), shear(w, h), R.pattern("p900", w, h), pad=1)
    if min_known == 16384:
        assert want["summary"][2] == 0 and want["summary"][3] > 0
        assert (want["filled"].view(np.uint32)[want["source"] == R.UNFILLED] == (R.NAN_BITS if leave == "nan" else 0)).all()
    else:
        assert want["summary"][2] > 0


@pytest.mark.parametrize("kind", ["half", "stripes"])
def test_domain(ctx, kind):
    """a half plane and stripes one pixel wide; KNOWN pixels outside the domain pass through"""
    w, h = 131, 67
    dom = np.zeros((h, w), np.uint8)
    if kind == "half":
        dom[:, : w // 2] = 1
    else:
        dom[:, ::2] = 255
    want = once(ctx, w, h, R.Params(levels=7, grid_x=4, grid_y=2), shear(w, h), R.pattern("p300", w, h), dom, pad=2)
    src = want["source"]
    assert (src[dom == 0] == 0).any() and (src[dom == 0] == R.OUTSIDE).any() and not (src[dom != 0] == R.OUTSIDE).any()


# ---------------------------------------------------------------------------- hold
@pytest.mark.parametrize("hold", [0, 1, 3, 254])
def test_hold_over_six_pushes_with_a_reset(ctx, hold):
    """a pattern that moves three pixels a push; the state is seen through the outputs of each push"""
    w, h = 131, 67
    s = Session(ctx, w, h, R.Params(levels=5, hold=hold, grid_x=3, grid_y=2), pad=1)
    f = shear(w, h)
    held = []
    for t in range(6):
        if t == 3:
            ctx.infill_reset()
            s.ref.reset()
            rc, rs, rsum = ctx.infill_read()
            assert not rc.view(np.uint8).any() and not rs.any() and not any(rsum.values()) and ctx.infill_info()["pushes"] == 0
        held.append(int(s.push(f + np.float32(0.25 * t), R.pattern("p900", w, h, shift=3 * t), what="(hold %d)" % hold)["summary"][1]))
    assert held[0] == 0 and held[3] == 0 and (held[1] > 0) == (hold > 0) and (hold < 3 or held[2] > held[1])
    s.close()


# ---------------------------------------------------------------------------- grids
@pytest.mark.parametrize("w,h,gx,gy", [(131, 67, 1, 1), (131, 67, 7, 5), (131, 67, 2, 67), (160, 128, 128, 128)])
def test_grids(ctx, w, h, gx, gy):
    """one cell; 7 x 5 with remainder columns and rows; 2 x 67: a cell row a pixel row; 128 x 128 = RC_RIPMAP_MAX_CELLS cells: more
    under a block than its table in LDS holds, so its sums go straight to memory"""
    want = once(ctx, w, h, R.Params(levels=7, grid_x=gx, grid_y=gy), shear(w, h), R.pattern("p900", w, h), pad=2)
    assert want["cells"]["pixels"].sum() == w * h and want["sums"][:, 2].sum() == want["summary"][2] and want["cells"].size == gx * gy


# ---------------------------------------------------------------------------- calling patterns
def test_each_output_alone_and_none(ctx):
    """what a push asks for changes nothing of what it gives, nor of what it does to the held state"""
    w, h = 73, 25
    s = Session(ctx, w, h, R.Params(levels=5, hold=2, grid_x=3, grid_y=2), pad=2)
    f = shear(w, h)
    for n, only in enumerate([()] + [(k,) for k in IMAGES + ARRAYS] + [IMAGES + ARRAYS]):
        s.push(f, R.pattern("p900", w, h, shift=n), what="asking %s" % (only,), only=only)
    s.close()


def test_two_slots_interleaved(ctx):
    (wa, ha, pa), (wb, hb, pb) = (73, 25, R.Params(levels=7, hold=1)), (37, 29, R.Params(levels=2, grid_x=2, grid_y=3, leave="zero"))
    a, b = Session(ctx, wa, ha, pa, stream=0), Session(ctx, wb, hb, pb, pad=1, stream=1)
    for t in range(3):
        a.push(shear(wa, ha), R.pattern("p900", wa, ha, shift=t), what="slot 0")
        wb_ = b.push(shear(wb, hb), R.pattern("corners", wb, hb, shift=t), what="slot 1")
    assert not np.isnan(wb_["filled"]).any() and wb_["summary"][3] > 0
    b.close()
    assert ctx.infill_info(stream=0)["pushes"] == 3
    a.close()


def test_set_between_pushes(ctx):
    w, h = 131, 67
    s = Session(ctx, w, h, R.Params(levels=2, grid_x=3, grid_y=2))
    f, v = shear(w, h), R.pattern("block40", w, h)
    first = s.push(f, v)
    ctx.infill_set(7, 4, "zero")
    s.ref.set(7, 4, "zero")
    info = ctx.infill_info()
    assert (info["levels"], info["min_known"], info["leave"], info["launches_per_push"], info["pushes"]) == (7, 4, "zero", 4, 1)
    second = s.push(f, v)
    assert first["summary"][3] > 0 and second["summary"][3] == 0
    ctx.infill_set(1, 16384, "nan")
    s.ref.set(1, 16384, "nan")
    assert ctx.infill_info()["launches_per_push"] == 3
    s.push(f, v)
    s.close()


def test_chain_flowcheck_infill_drifters_ftle(ctx):
    """End to end on synth.surf_clip(160, 120): the project's own Farneback field left resident by the frame loop goes into the
    infill as it is (d_flow_xy NULL), then through the flow check (NaN fill, FLAT and FAST), whose d_checked and d_mask go into the
    infill, and the filled field into the drifters and the flow map.  Each stage equals its own statement; with nothing UNFILLED no
    drifter dies BAD, and the particles the flow map stops are those the statement stops on the filled field: the picture's border
    alone, fewer than on the checked field"""
    w, h = 160, 120
    clip = synth.surf_clip(w, h, 2)
    ctx.stream_reset()
    assert ctx.push_frame_host(clip[0]) is None
    flow = ctx.push_frame_host(clip[1]).cpu().numpy()
    lut = ctx.jet_lut()
    p = R.Params(levels=7, grid_x=4, grid_y=3)
    ref = R.InfillRef(w, h, p, lut)
    ctx.infill_open(w, h, **p.kw())
    out = outputs(p, w, h)
    ctx.infill_push(None, **out.kw())
    compare(out.host(), ctx.infill_read(), ref.push(flow), "(the resident Farneback field)")
    fp = F.Params(radius=4, grid_x=4, grid_y=3, tests=F.FLAT | F.FAST, tex_min=1, speed_max=20.0)
    ctx.flowcheck_open(w, h, **fp.kw())
    checked = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    valid = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    ctx.flowcheck_push(dev(clip[1]).view, dev(clip[0]).view, None, checked=checked, mask=valid)
    fc = F.check(clip[0], clip[1], flow, None, fp)
    assert same_bits(checked.cpu().numpy(), fc["checked"]) and np.array_equal(valid.cpu().numpy(), fc["mask"])
    ctx.infill_push(checked, valid, **out.kw())
    want = ref.push(fc["checked"], fc["mask"])
    got = out.host()
    compare(got, ctx.infill_read(), want, "(the checked field)")
    holes = int((fc["mask"] == 0).sum())
    assert holes > 0 and want["summary"][3] == 0 and want["summary"][2] == holes and not np.isnan(got["filled"]).any()
    filled = out.t["filled"]
    # drifters on the filled field: nobody dies BAD
    dp = D.Params(max_drifters=2000, grid_x=8, grid_y=6, max_age=60)
    dref = D.DriftersRef(w, h, dp, lut)
    ctx.drifters_open(w, h, **dp.kw())
    homes = D.prototype_lattice()
    dref.seed(homes)
    ctx.drifters_seed(homes)
    summ = torch.zeros(24, dtype=torch.int64, device="cuda")
    for k in range(61):
        dw = dref.push(want["filled"], None)
        ctx.drifters_push(filled, None, summary=summ)
    assert np.array_equal(summ.cpu().numpy(), dw["summary"]) and dw["summary"][8 + D.BAD] == 0
    ctx.drifters_close()
    # the flow map: the stopped particles are the border's alone
    stopped = {}
    for name, fld in (("filled", want["filled"]), ("checked", fc["checked"])):
        tref = T.FtleRef(w, h, lut, window=3)
        ctx.ftle_open(w, h, window=3)
        steps = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        for k in range(3):
            tw = tref.push(fld)
            ctx.ftle_push(dev(fld).view, steps=steps)
        assert np.array_equal(steps.cpu().numpy(), tw["steps"]) and ctx.ftle_read()["stopped"] == int(tw["summary"][3])
        stopped[name] = int(tw["summary"][3])
        ctx.ftle_close()
    print("holes %d; particles the flow map stops on the filled field %d, on the checked field %d" % (holes, stopped["filled"], stopped["checked"]))
    assert stopped["filled"] < stopped["checked"]
    ctx.flowcheck_close()
    ctx.infill_open(128, 96, **p.kw())
    with pytest.raises(RcflowError) as e:
        ctx.infill_push(None)
    assert e.value.code == ESIZE                                  # the resident field has another size
    ctx.stream_reset()
    with pytest.raises(RcflowError) as e:
        ctx.infill_push(None)
    assert e.value.code == ESTATE and ctx.infill_info()["pushes"] == 0
    ctx.infill_close()


def test_product_object(ctx):
    w, h, p = 73, 25, R.Params(levels=4, hold=1, grid_x=2, grid_y=2)
    ref = R.InfillRef(w, h, p, ctx.jet_lut())
    f = shear(w, h)
    with Infill(ctx, w, h, **p.kw()) as fi:
        filled = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
        for t in range(3):
            fi.push(dev(f).view, dev(R.pattern("p900", w, h, shift=t)).view, filled=filled)
            want = ref.push(f, R.pattern("p900", w, h, shift=t))
        rc, rs, rsum = fi.read()
        assert same("cells", rc.ravel(), want["cells"]) and rsum["pushes"] == 3 and rsum["held"] > 0 and same_bits(filled.cpu().numpy(), want["filled"])
        assert fi.info()["leave"] == "nan" and fi.info()["hold"] == 1
        with pytest.raises(ValueError):
            fi.push(dev(f[:, :-1]).view)                          # a field of another size
        fi.set(2, 3, "zero")
        fi.reset()
        assert fi.info()["pushes"] == 0 and fi.info()["levels"] == 2 and fi.info()["min_known"] == 3 and fi.info()["leave"] == "zero"
    with pytest.raises(RcflowError):
        ctx.infill_info()


# ---------------------------------------------------------------------------- arguments and refusals
def test_refusals_leave_state_and_outputs_untouched(ctx):
    w, h = 40, 24
    good = R.Params(levels=5, min_known=2, hold=2, grid_x=4, grid_y=3)
    nc = good.grid_x * good.grid_y
    ctx.infill_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.infill_info, ctx.infill_read, ctx.infill_reset, lambda: ctx.infill_set(7, 1, "nan")):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 1024)()
    for name, args in (("info", (C.byref(InfillInfo()),)), ("read", (buf, buf, buf)), ("reset", ()), ("set", (7, 1, 1)),
                       ("push_dev", (null, 0) * 7 + (null, null, null))):
        assert getattr(lib, "rcflow_infill_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_infill_%s:" % name), text()
    kw = good.kw()
    for bad in (dict(levels=0), dict(levels=8), dict(min_known=0), dict(min_known=16385), dict(hold=-1), dict(hold=255), dict(grid_x=0),
                dict(grid_x=41), dict(grid_y=25)):
        assert R.open_error(w, h, with_(good, **bad)) in ("parameters", "grid")
        with pytest.raises(RcflowError) as e:
            ctx.infill_open(w, h, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_infill_open"), bad
    p = InfillParams(levels=5, min_known=2, hold=2, grid_x=4, grid_y=3, flags=0)
    for flags in (0, 3, 4):                                       # neither pattern, both, an unknown one
        p.flags = flags
        assert lib.rcflow_infill_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "exactly one" in text()
    p.flags = 1
    p.pad[5] = 1
    assert lib.rcflow_infill_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "pad" in text()
    p.pad[5] = 0
    assert lib.rcflow_infill_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_infill_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_infill_open(hdl, 2, w, h, C.byref(p)) == EINVAL              # no such slot
    with pytest.raises(RcflowError) as e:
        ctx.infill_open(4000, 2161, **kw)                         # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_infill_open")
    with pytest.raises(RcflowError):
        ctx.infill_info()                                         # nothing was left open by any of them

    f = shear(w, h)
    v = [R.pattern("p900", w, h, shift=t) for t in range(3)]
    dom = np.ones((h, w), np.uint8)
    ref = R.InfillRef(w, h, good, ctx.jet_lut())
    ctx.infill_open(w, h, **kw)
    out = outputs(good, w, h, 2)
    df, dv, dd = dev(f), [dev(x) for x in v], dev(dom)
    ctx.infill_push(df.view, dv[0].view, dd.view, **out.kw())
    first = ref.push(f, v[0], dom)
    compare(out.host(), ctx.infill_read(), first, "(before the refusals)")
    assert lib.rcflow_infill_info(hdl, 0, None) == EINVAL
    before = ctx.infill_info()
    for bad in (dict(levels=9), dict(hold=300)):                  # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.infill_open(w, h, **dict(kw, **bad))
    assert ctx.infill_info() == before
    big = torch.zeros(64 * h * w + 4096, dtype=torch.uint8, device="cuda")
    N = (null, 0)
    o = out.t

    def im(t, off=0, step=None):
        return (ptr(t, off), t.stride(0) * t.element_size() if step is None else step)

    def push(flow=None, valid=N, domain=N, filled=N, source=N, mask=N, pic=N, cells=null, sums=null, summ=null, slot=0):
        return lib.rcflow_infill_push_dev(hdl, slot, *(flow or im(df.view)), *valid, *domain, *filled, *source, *mask, *pic, cells, sums, summ)

    refused = [
        push(flow=im(df.view, step=8 * w - 8)), push(flow=im(df.view, step=8 * w + 4)), push(flow=im(df.view, 4)),
        push(valid=im(dv[1].view, step=w - 1)), push(domain=im(dd.view, step=w - 1)),
        push(filled=im(o["filled"], 4)), push(filled=im(o["filled"], step=8 * w + 4)), push(filled=im(o["filled"], step=8 * w - 8)),
        push(source=im(o["source"], step=w - 1)), push(mask=im(o["mask"], step=w - 1)), push(pic=im(o["picture"], step=3 * w - 1)),
        push(cells=ptr(big, 2)), push(sums=ptr(big, 4)), push(summ=ptr(big, 4)),
        push(filled=im(df.view)),                                     # d_filled over the field: filling in place is not this product
        push(valid=im(dv[1].view), source=im(dv[1].view)), push(domain=im(dd.view), mask=im(dd.view)),       # an output over a mask
        push(source=(ptr(big), w), mask=(ptr(big, w * (h - 1)), w)),  # two outputs meeting in one row
        push(filled=(ptr(big), 8 * w), pic=(ptr(big, 8), 3 * w)), push(cells=ptr(big), sums=ptr(big, 32 * nc - 8)),
        push(sums=ptr(big), summ=ptr(big, 64 * nc - 8)), push(pic=(ptr(big), 3 * w), summ=ptr(big)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert text().startswith("rcflow_infill_push_dev")
    assert push(slot=2) == EINVAL
    for bad in ((0, 1, "nan"), (8, 1, "nan"), (7, 0, "zero"), (7, 16385, "nan")):
        with pytest.raises(RcflowError) as e:
            ctx.infill_set(*bad)
        assert e.value.code == EINVAL and text().startswith("rcflow_infill_set")
    assert lib.rcflow_infill_set(hdl, 0, 7, 1, 3) == EINVAL and lib.rcflow_infill_set(hdl, 0, 7, 1, 0) == EINVAL
    assert ctx.infill_info() == before
    # the outputs of the push before stand as they were, with their fences; the slot's records too
    compare(out.host(), ctx.infill_read(), first, "(after the refusals)")
    # nothing was queued and nothing changed: the held state is the first push's
    ctx.infill_push(df.view, dv[1].view, dd.view, **out.kw())
    second = ref.push(f, v[1], dom)
    compare(out.host(), ctx.infill_read(), second, "(the push after the refusals)")
    assert second["summary"][1] > 0
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.infill_push(df.view, dv[2].view, dd.view, **out.kw())
        got = ctx.infill_read()
    torch.cuda.synchronize()
    compare(out.host(), got, ref.push(f, v[2], dom), "(on another stream)")
    ctx.infill_close()                                            # closing twice is fine
    ctx.infill_close()
