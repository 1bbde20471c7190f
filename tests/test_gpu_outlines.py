"""The region outlines on the device (outline_kernels.hip) against their sequential statement (tests/_outlines_ref.py): every record,
every vertex, the summary, the slot's read and the primitives, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _outlines_ref as R
import _regions_ref as RG
import _tracers_ref as TR
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, Outputs, Padded, ptr, raw
from ripcurrents_amd._lib import RC_OUTLINES_FIXED_LAUNCHES, OutlinesInfo, OutlinesParams, RcflowError
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, OUTLINE_LOOP_DTYPE, OUTLINES_SUMMARY, Outlines

pytestmark = pytest.mark.gpu

OL_SEG = 256                                                      # outline_kernels.hip: the pixels of a row one block owns
dev = Padded.of
assert OUTLINE_LOOP_DTYPE == R.LOOP and DRAW_PRIM_DTYPE == R.PRIM


def rounds_of(max_cracks):
    return int(max_cracks - 1).bit_length()


def views(d):
    d["loops"] = d["loops"].view(OUTLINE_LOOP_DTYPE)
    d["verts"] = d["verts"].reshape(-1, 2)


class Session:
    """the device session and the statement side by side"""

    def __init__(self, ctx, w, h, connectivity=8, min_cracks=4, max_cracks=1 << 14, max_loops=64, max_vertices=512, pad=0, stream=0):
        self.ctx, self.w, self.h, self.pad, self.stream = ctx, w, h, pad, stream
        self.kw = dict(connectivity=connectivity, min_cracks=min_cracks, max_cracks=max_cracks, max_loops=max_loops, max_vertices=max_vertices)
        ctx.outlines_open(w, h, stream=stream, **self.kw)
        info = ctx.outlines_info(stream=stream)
        assert info["rounds"] == rounds_of(max_cracks) and info["launches_per_push"] == RC_OUTLINES_FIXED_LAUNCHES + 2 * info["rounds"]
        assert info["pushes"] == 0 and info["device_bytes"] >= 5 * w * h + 36 * max_cracks
        self.pushes = 0
        self.out = Outputs({}, dict(loops=((max_loops * 56,), torch.uint8, None), verts=((max_vertices * 2,), torch.int32, -7),
                                    summary=((8,), torch.int64, -1)), 0, views)
        self.last = None

    def want(self, labels=None, mask=None):
        return R.outlines(labels, mask, pushes=self.pushes, **self.kw)

    def holds(self, got, what, only=None):
        want = self.last
        asked = lambda k: only is None or k in only
        assert not asked("summary") or list(got["summary"]) == list(want["summary"]), "summary %s: %s, wanted %s" % (what, got["summary"], want["summary"])
        n = int(want["summary"][3])
        assert not asked("loops") or got["loops"].tobytes() == want["loops"].tobytes(), \
            "records differ %s: %s, wanted %s" % (what, got["loops"][:n + 1], want["loops"][:n + 1])
        assert not asked("verts") or np.array_equal(got["verts"], want["verts"]), "vertices differ %s" % what

    def read_is(self, what):
        rec, verts, summ = self.ctx.outlines_read(stream=self.stream)
        want = self.last
        n, nv = int(want["summary"][3]), int(want["summary"][5])
        assert [summ[k] for k in OUTLINES_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what
        assert rec.tobytes() == want["loops"][:n].tobytes() and np.array_equal(verts, want["verts"][:nv]), "the slot's records or vertices differ " + what

    def prims_are(self, what, color=0x20c0ff, thickness=1):
        got = self.ctx.outlines_prims(color, thickness, stream=self.stream).cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE)
        want = R.prims(self.last, self.w, self.h, color, thickness)
        assert got.tobytes() == want.tobytes(), "primitives differ " + what
        return got

    def push(self, labels=None, mask=None, what="", only=None):
        self.pushes += 1
        self.last = want = self.want(labels, mask)
        d = dev(labels if mask is None else mask, self.pad)
        self.ctx.outlines_push(labels=d.view if mask is None else None, mask=d.view if labels is None else None, stream=self.stream, **self.out.kw(only))
        what = "after push %d %s" % (self.pushes, what)
        self.holds(self.out.host(), what, only)
        self.read_is(what)
        self.prims_are(what)
        assert np.array_equal(d.view.cpu().numpy(), labels if mask is None else mask), "the input was written"
        d.check("the input")
        assert self.ctx.outlines_info(stream=self.stream)["pushes"] == self.pushes
        return want

    def close(self):
        self.ctx.outlines_close(stream=self.stream)


def once(ctx, lab, what="", **kw):
    h, w = lab.shape
    s = Session(ctx, w, h, **kw)
    want = s.push(labels=lab, what=what)
    s.close()
    return want


# ---------------------------------------------------------------------------- sizes and shapes
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (13, 11), (67, 19), (130, 33), (OL_SEG + 3, 5), (3, 300)])
def test_random_labels_with_padded_steps(ctx, w, h, connectivity):
    """a pixel, a column, a row; 13 x 11; 67 x 19 and 130 x 33, ragged against a wave; 259 x 5: three pixels into a row's second block;
    3 x 300: 300 pixel blocks, so the one-block scan of the block counts carries into a second pass of 256"""
    lab = R.random_labels(w, h, 3, 100 * w + h, 0.6)
    want = once(ctx, lab, "(%d x %d)" % (w, h), connectivity=connectivity, pad=3, max_loops=2048, max_vertices=8192)
    assert want["summary"][0] > 0 and want["summary"][5] == want["summary"][4] and not want["summary"][6]


def test_all_zero_and_all_one(ctx):
    w, h = 67, 19
    z = once(ctx, np.zeros((h, w), np.int32), "(all zero)", pad=1)
    assert list(z["summary"]) == [0, 0, 0, 0, 0, 0, 0, 1]
    o = once(ctx, np.full((h, w), 5, np.int32), "(all one label)", pad=1)
    r = o["loops"][0]
    assert list(o["summary"][:6]) == [2 * (w + h), 1, 1, 1, 4, 4] and (r["label"], r["cracks"], r["area2"], r["x1"], r["y1"]) == (5, 2 * (w + h), 2 * w * h, w, h)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_checkerboard(ctx, connectivity):
    """under 4 every pixel is a loop; under 8 one large loop with a hole per background pixel inside"""
    w, h = 21, 13
    lab = R.checkerboard(w, h)
    o = once(ctx, lab, "(checkerboard)", connectivity=connectivity, pad=2, max_loops=256, max_vertices=4096)
    n = int(lab.sum())
    if connectivity == 4:
        assert o["summary"][1] == n and (o["loops"]["cracks"][:n] == 4).all()
    else:
        inner = int((lab[1:-1, 1:-1] == 0).sum())
        assert o["summary"][1] == 1 + inner and (o["loops"]["flags"][1:1 + inner] == R.HOLE).all() and o["loops"][0]["cracks"] == 4 * n - 4 * inner


def test_nested_rings_and_two_labels_sharing_an_edge(ctx):
    o = once(ctx, R.rings(23, 17), "(rings)", pad=1)
    k = int(o["summary"][3])
    assert k == 9 and list(np.sign(o["loops"]["area2"][:k])) == [1] + [-1, 1] * 4
    lab = np.zeros((9, 14), np.int32)
    lab[2:7, 2:7], lab[2:7, 7:12] = 1, 2
    o = once(ctx, lab, "(two labels)")
    assert list(o["loops"]["label"][:2]) == [1, 2] and list(o["loops"]["cracks"][:2]) == [20, 20] and o["summary"][1] == 2


# ---------------------------------------------------------------------------- the rounds and the caps
def test_serpentine_needs_the_last_round_and_one_crack_less_overflows(ctx):
    w, h = 96, 64
    lab = R.serpentine(w, h)
    n = len(R.cracks_of(lab.astype(np.int64)))
    assert n > 6000 and rounds_of(n) > rounds_of(n // 2)
    kw = dict(connectivity=4, max_loops=4, max_vertices=1024, pad=1)
    s = Session(ctx, w, h, max_cracks=n, **kw)
    o = s.push(labels=lab, what="(the serpentine, max_cracks its own count)")
    assert list(o["summary"][:4]) == [n, 1, 1, 1] and o["loops"][0]["cracks"] == n
    ctx.set_option("outlines_early", 0)
    try:
        s.push(labels=lab, what="(every round does its work)")
    finally:
        ctx.set_option("outlines_early", 1)
    s = Session(ctx, w, h, max_cracks=n - 1, **kw)                # over the open one
    o = s.push(labels=lab, what="(one crack too many)")
    assert list(o["summary"]) == [n, 0, 0, 0, 0, 0, 1, 1] and not o["loops"].view(np.uint8).any() and not o["verts"].any()
    small = np.zeros((h, w), np.int32)
    small[3:9, 4:30] = 2
    o = s.push(labels=small, what="(the slot after an overflow)")
    assert list(o["summary"]) == [64, 1, 1, 1, 4, 4, 0, 2]
    s.close()


def test_max_loops_and_max_vertices_one_short(ctx):
    lab = R.rings(23, 17)
    full = R.outlines(labels=lab)
    kept, nv = int(full["summary"][2]), int(full["summary"][4])
    few = once(ctx, lab, "(max_loops one short)", max_loops=kept - 1, pad=2)
    assert few["summary"][3] == kept - 1 and few["summary"][4] == nv and few["summary"][5] == nv - 4
    short = once(ctx, lab, "(max_vertices one short)", max_vertices=nv - 1, pad=2)
    last = short["loops"][kept - 1]
    assert last["offset"] == -1 and last["flags"] == R.NOVERTS and short["summary"][5] == nv - 4 and not short["verts"][nv - 4:].any()
    one = once(ctx, lab, "(room for one loop's vertices)", max_vertices=4, max_loops=3)
    assert list(one["loops"]["flags"][:3]) == [0, R.HOLE | R.NOVERTS, R.NOVERTS] and list(one["summary"][3:6]) == [3, nv, 4]


def test_min_cracks_through_set_between_pushes_and_reset(ctx):
    w, h = 67, 19
    lab = R.random_labels(w, h, 2, 5, 0.5)
    s = Session(ctx, w, h, pad=1, max_loops=512, max_vertices=4096)
    a = s.push(labels=lab)
    for m in (5, 13, 1):
        ctx.outlines_set(m)
        s.kw["min_cracks"] = m
        assert ctx.outlines_info()["min_cracks"] == m and ctx.outlines_info()["pushes"] == s.pushes
        b = s.push(labels=lab, what="(min_cracks %d)" % m)
        assert b["summary"][1] == a["summary"][1] and (b["summary"][2] < a["summary"][2]) == (m > 4)
    ctx.outlines_reset()
    rec, verts, summ = ctx.outlines_read()
    assert len(rec) == 0 and len(verts) == 0 and not any(summ.values())
    assert not ctx.outlines_prims().cpu().numpy().any()
    info = ctx.outlines_info()
    assert (info["pushes"], info["min_cracks"]) == (0, 1)
    s.pushes = 0
    s.push(labels=lab, what="(after the reset)")
    s.close()


def test_each_output_alone_and_none(ctx):
    """what a call asks for changes nothing of what it gives or keeps"""
    w, h = 40, 24
    s = Session(ctx, w, h, pad=2)
    for i, only in enumerate([(), ("loops",), ("verts",), ("summary",), None]):
        s.push(labels=R.random_labels(w, h, 2, 30 + i), what="asking %s" % (only,), only=only)
    s.close()


def test_mask_path_equals_labels_all_one(ctx):
    w, h = 130, 33
    mask = R.blobs(w, h, 9, 2)
    s = Session(ctx, w, h, pad=5, max_loops=128, max_vertices=2048)
    a = s.push(mask=mask, what="(the mask)")
    b = s.push(labels=(mask != 0).astype(np.int32), what="(labels all 1)")
    assert a["loops"].tobytes() == b["loops"].tobytes() and np.array_equal(a["verts"], b["verts"]) and a["summary"][1] > 3
    s.close()


# ---------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("connectivity", [4, 8])
def test_labels_straight_from_the_regions_and_the_drawing(ctx, connectivity):
    """the regions' label plane never leaves the device; every region's first pixel is its outer loop's leader pixel; the primitives
    painted by rcflow_draw_dev equal the statement's primitives painted by the tracer tests' drawing statement"""
    w, h = 130, 33
    mask = R.blobs(w, h, 9, 4)
    mask[::7, ::5] = 255
    ctx.regions_open(w, h, connectivity=connectivity, min_area=3, max_regions=64)
    labels = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ctx.regions_push(dev(mask).view, labels=labels)
    kw = dict(connectivity=connectivity, min_cracks=4, max_cracks=1 << 13, max_loops=128, max_vertices=2048)
    ctx.outlines_open(w, h, **kw)
    ctx.outlines_push(labels=labels)
    prims = ctx.outlines_prims(0x20c0ff, 2)
    canvas_in = (np.arange(h * w * 3, dtype=np.int64) * 7).astype(np.uint8).reshape(h, w, 3)
    canvas = torch.as_tensor(canvas_in).cuda()
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.draw(canvas, prims, skipped=skipped)
    # only now the host looks
    regs, rsum = ctx.regions_read()
    wl = RG.regions(mask, connectivity, 3, 64)["labels"]
    assert np.array_equal(labels.cpu().numpy(), wl) and len(regs) > 3
    want = R.outlines(labels=wl, **kw)
    rec, verts, summ = ctx.outlines_read()
    n, nv = int(want["summary"][3]), int(want["summary"][5])
    assert rec.tobytes() == want["loops"][:n].tobytes() and np.array_equal(verts, want["verts"][:nv])
    assert [summ[k] for k in OUTLINES_SUMMARY] == [int(v) for v in want["summary"]]
    outer = rec[rec["area2"] > 0]
    assert len(outer) == len(regs) and list(outer["label"]) == list(regs["label"])
    assert list(outer["x"]) == list(regs["first_x"]) and list(outer["y"]) == list(regs["first_y"])
    wp = R.prims(want, w, h, 0x20c0ff, 2)
    assert prims.cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE).tobytes() == wp.tobytes()
    ref = canvas_in.copy()
    nskip = TR.draw(ref, wp.astype(TR.PRIM))
    assert np.array_equal(canvas.cpu().numpy(), ref) and int(skipped.item()) == nskip == kw["max_vertices"] - nv and (ref != canvas_in).any()
    ctx.outlines_close()
    ctx.regions_close()


def test_two_slots_and_the_product_object(ctx):
    (wa, ha), (wb, hb) = (67, 19), (40, 33)
    a, b = Session(ctx, wa, ha, stream=0, max_loops=512, max_vertices=4096), Session(ctx, wb, hb, connectivity=4, pad=1, stream=1, max_loops=512, max_vertices=4096)
    for t in range(2):
        a.push(labels=R.random_labels(wa, ha, 3, t), what="slot 0")
        b.push(mask=R.blobs(wb, hb, 5, t), what="slot 1")
    b.close()
    assert ctx.outlines_info(stream=0)["pushes"] == 2
    a.close()
    lab = R.rings(23, 17)
    with Outlines(ctx, 23, 17, connectivity=4, max_loops=32, max_vertices=256) as o:
        o.push(dev(lab, 1).view)
        want = R.outlines(labels=lab, connectivity=4, max_loops=32, max_vertices=256)
        rec, verts, summ = o.read()
        assert rec.tobytes() == want["loops"][:len(rec)].tobytes() and np.array_equal(verts, want["verts"][:len(verts)]) and summ["pushes"] == 1
        assert o.prims(0xff, 3).cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE).tobytes() == R.prims(want, 23, 17, 0xff, 3).tobytes()
        with pytest.raises(ValueError):
            o.push(dev(lab[:, :-1]).view)                         # a plane of another size
        with pytest.raises(ValueError):
            o.push()                                              # neither input
        o.set(6)
        o.reset()
        assert (o.info()["min_cracks"], o.info()["pushes"]) == (6, 0)
    with pytest.raises(RcflowError):
        ctx.outlines_info()


def test_launch_counts_against_the_profile(ctx):
    w, h = 67, 19
    s = Session(ctx, w, h, max_cracks=1000)
    lab = dev(R.random_labels(w, h, 2, 1)).view
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(2):
        ctx.outlines_push(labels=lab)
    ctx.outlines_prims()
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    ctx.profile_enable(False)
    info = ctx.outlines_info()
    assert info["rounds"] == 10
    want = {"outlines@0": 4, "outlines@1": 2, "outlines@2": 2, "outlines@3": 20, "outlines@4": 2, "outlines@5": 20, "outlines@6": 6, "outlines@7": 2,
            "outlines@8": 2, "outlines@9": 4, "outlines@10": 2, "outlines@11": 1}
    assert prof == want, prof
    assert sum(v for k, v in prof.items() if k != "outlines@11") == info["launches_per_push"] * info["pushes"]
    s.close()


# ---------------------------------------------------------------------------- arguments and refusals
def test_refusals_leave_state_and_outputs_untouched(ctx):
    w, h = 40, 24
    ctx.outlines_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.outlines_info, ctx.outlines_read, ctx.outlines_reset, ctx.outlines_prims, lambda: ctx.outlines_set(4)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 64)()
    n = C.c_int(0)
    for name, args in (("info", (C.byref(OutlinesInfo()),)), ("read", (buf, 0, C.byref(n), buf, 0, C.byref(n), buf)), ("reset", ()), ("set", (4,)),
                       ("push_dev", (null, 0) * 2 + (null, null, null)), ("prims_dev", (0, 1, null))):
        assert getattr(lib, "rcflow_outlines_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_outlines_%s:" % name), text()
    good = dict(connectivity=8, min_cracks=4, max_cracks=4096, max_loops=16, max_vertices=128)
    bads = (dict(connectivity=6), dict(connectivity=0), dict(min_cracks=0), dict(max_cracks=3), dict(max_cracks=(1 << 25) + 1), dict(max_loops=0),
            dict(max_loops=(1 << 20) + 1), dict(max_vertices=3), dict(max_vertices=(1 << 24) + 1))
    for bad in bads:
        with pytest.raises(RcflowError) as e:
            ctx.outlines_open(w, h, **dict(good, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_outlines_open"), bad
    p = OutlinesParams(flags=1, **good)
    assert lib.rcflow_outlines_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "flags" in text()
    p.flags = 0
    p.pad[1] = 1
    assert lib.rcflow_outlines_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "pad" in text()
    p.pad[1] = 0
    assert lib.rcflow_outlines_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_outlines_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_outlines_open(hdl, 2, w, h, C.byref(p)) == EINVAL            # no such slot
    # RC_ESIZE beyond RC_OUTLINES_MAX_SIDE is not reached here: the session's context is 3840 x 2160, and rc_fits_context refuses first
    with pytest.raises(RcflowError) as e:
        ctx.outlines_open(4000, 2161, **good)                     # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_outlines_open")
    with pytest.raises(RcflowError):
        ctx.outlines_info()                                       # nothing was left open by any of them

    s = Session(ctx, w, h, pad=2, **good)
    labs = [R.random_labels(w, h, 2, 40 + t) for t in range(3)]
    first = s.push(labels=labs[0], what="(before the refusals)")
    assert lib.rcflow_outlines_info(hdl, 0, None) == EINVAL
    before = ctx.outlines_info()
    for bad in (dict(connectivity=5), dict(max_cracks=2)):        # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.outlines_open(w, h, **dict(good, **bad))
    assert ctx.outlines_info() == before
    dl, dm = dev(labs[1], 2), dev(np.where(labs[1], 255, 0).astype(np.uint8), 2)
    big = torch.zeros(64 * h * w + 4096, dtype=torch.uint8, device="cuda")
    N = (null, 0)
    o = s.out.t
    nl, nvb = good["max_loops"] * 56, good["max_vertices"] * 8

    def im(t, off=0, step=None):
        return (ptr(t, off), t.stride(0) * t.element_size() if step is None else step)

    def push(lab=None, mask=N, loops=null, verts=null, summ=null, slot=0):
        return lib.rcflow_outlines_push_dev(hdl, slot, *(im(dl.view) if lab is None else lab), *mask, loops, verts, summ)

    refused = [
        push(lab=N), push(mask=im(dm.view)),                      # neither input, both
        push(lab=im(dl.view, 2)), push(lab=im(dl.view, step=4 * w + 2)), push(lab=im(dl.view, step=4 * w - 4)),
        push(lab=N, mask=im(dm.view, step=w - 1)),
        push(loops=ptr(big, 4)), push(verts=ptr(big, 2)), push(summ=ptr(big, 4)),
        push(loops=ptr(big), verts=ptr(big, nl - 4)), push(verts=ptr(big), summ=ptr(big, nvb - 8)), push(loops=ptr(big), summ=ptr(big)),
        push(lab=(ptr(big), 4 * w), loops=ptr(big, 4 * w * h - 8)),          # an output over the labels' last row
        push(lab=N, mask=(ptr(big), w), verts=ptr(big, w * (h - 1))),        # an output over the mask's last row
        lib.rcflow_outlines_prims_dev(hdl, 0, 0, 1, null), lib.rcflow_outlines_prims_dev(hdl, 0, 0, 1, ptr(big, 2)),
        lib.rcflow_outlines_prims_dev(hdl, 0, 0, 0, ptr(big)), lib.rcflow_outlines_prims_dev(hdl, 0, 0, 9, ptr(big)),
        lib.rcflow_outlines_set(hdl, 0, 0), lib.rcflow_outlines_set(hdl, 0, -3),
        lib.rcflow_outlines_read(hdl, 0, None, 4, C.byref(n), None, 0, C.byref(n), buf), lib.rcflow_outlines_read(hdl, 0, None, 0, None, buf, -1, None, None),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert push(slot=2) == EINVAL
    assert ctx.outlines_info() == before and not big.any()
    # the outputs of the push before stand as they were; the slot's copies too
    s.holds(s.out.host(), "(after the refusals)")
    s.read_is("(after the refusals)")
    s.push(labels=labs[1], what="(the push after the refusals)")
    # a slot moved to another stream between calls
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s.push(labels=labs[2], what="(on another stream)")
    torch.cuda.synchronize()
    ctx.outlines_close()                                          # closing twice is fine
    ctx.outlines_close()
