"""The shoreline on the device (shoreline_kernels.hip) against its numpy statement (tests/_shoreline_ref.py): the table, the
records, the summary, the mask, the plane, the histogram, the ring and the primitives of every push, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _regions_ref as RG
import _shoreline_ref as S
import _tracers_ref as TR
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ptr, raw
from _shoreline_ref import ragged_lines
from ripcurrents_amd._lib import RC_SHORE_LAUNCHES, RcflowError, ShorelineInfo, ShorelineParams, TransectLine
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, SHORELINE_DTYPE, SHORELINE_SUMMARY, Shoreline

pytestmark = pytest.mark.gpu

dev_image = Padded.of                                             # a picture on the device, rows `pad` pixels longer and the sentinel there


def views(d):
    d["records"], d["plane"], d["hist"] = d["records"].view(SHORELINE_DTYPE), d["plane"].view(np.uint16), d["hist"].view(np.uint32)


def outputs(L, w, h, pad=0):
    return Outputs(dict(mask=((h, w), torch.uint8), plane=((h, w), torch.int16)),
                   dict(records=((L * 64,), torch.uint8, None), summary=((8,), torch.int64, -1), hist=((512,), torch.int32, -1)), pad, views)


def compare(got, read, want, what):
    for k in ("summary", "hist", "plane", "mask"):
        assert np.array_equal(got[k], want[k]), "%s differs %s: %s, wanted %s" % (k, what, got[k], want[k])
    for f in S.RECORD.names:
        assert got["records"][f].tobytes() == want["records"][f].tobytes(), "%s differs %s: %s, wanted %s" % (f, what, got["records"][f], want["records"][f])
    if read is not None:
        rrec, rsumm = read
        assert rrec.tobytes() == got["records"].tobytes(), "the slot's copy differs " + what
        assert [rsumm[k] for k in SHORELINE_SUMMARY] == [int(v) for v in got["summary"]], "the slot's summary differs " + what


def run(ctx, w, h, lines, p, images, rois=None, pad=0, stream=0, keep_open=False):
    """a sequence of pictures through the device session and the statement, every output compared after every push
    -> (the statement, its outputs of every push)"""
    ref = S.ShorelineRef(w, h, lines, p)
    ctx.shoreline_open(w, h, lines, stream=stream, **p.kw())
    info = ctx.shoreline_info(stream=stream)
    assert (info["lines"], info["samples"], info["launches_per_push"], info["source"]) == (ref.L, len(ref.table), RC_SHORE_LAUNCHES, p.kw()["source"])
    table, geom = ctx.shoreline_table(stream=stream)
    assert table.tobytes() == ref.table.tobytes() and geom.tobytes() == ref.geom.tobytes()
    out, wants = outputs(ref.L, w, h, pad), []
    for t, img in enumerate(images):
        roi = None if rois is None else rois[t]
        d = dev_image(img, pad)
        droi = None if roi is None else dev_image(roi, pad).view
        ctx.shoreline_push(d.view, droi, stream=stream, **out.kw())
        want = ref.push(img, roi)
        what = "after push %d" % (t + 1)
        compare(out.host(), ctx.shoreline_read(stream=stream), want, what)
        assert np.array_equal(ctx.shoreline_ring(stream=stream), ref.ring_read()), "the ring differs " + what
        assert np.array_equal(d.view.cpu().numpy(), img), "the picture was written"
        d.check("the picture")
        info = ctx.shoreline_info(stream=stream)
        assert (info["held"], info["pushes"]) == (min(t + 1, p.window), t + 1)
        wants.append(want)
    if not keep_open:
        ctx.shoreline_close(stream=stream)
    return ref, wants


def flags_seen(wants):
    return int(np.bitwise_or.reduce(np.concatenate([x["records"]["flags"] for x in wants])))


def polygon_roi(w, h):
    yy, xx = np.mgrid[:h, :w]
    inside = (yy > 0.1 * h) & (yy < 0.93 * h) & (xx > 0.15 * w + 0.2 * yy) & (xx < 0.9 * w - 0.1 * yy)
    return np.where(inside, 200, 0).astype(np.uint8)


# ---------------------------------------------------------------------------- the beach
@pytest.mark.parametrize("foam,pushes", [(False, 32), (True, 32), (False, 40)])
def test_beach_every_output_after_every_push(ctx, foam, pushes):
    """the scene of the CPU tier; 32 and 40 pushes into a window of 16 wrap the ring"""
    w, h = 96, 64
    ref, wants = run(ctx, w, h, S.beach_lines(w, h), S.Params(radius=2, window=16, permille=20), [S.beach(w, h, t, foam=foam) for t in range(pushes)])
    assert all(245 <= x["thr"] <= 265 for x in wants) and not flags_seen(wants) & (S.DRY | S.WET | S.EMPTY)
    assert (wants[-1]["records"]["nv"] == 16).all()


@pytest.mark.parametrize("r", [0, 1, 7])
def test_ragged_with_padded_steps(ctx, r):
    w, h = 67, 35
    run(ctx, w, h, ragged_lines(w, h), S.Params(radius=r, window=3, permille=500), [S.beach(w, h, t, amp=3) for t in range(4)], pad=5)


def test_one_line_alone(ctx):
    w, h = 67, 35
    ref, wants = run(ctx, w, h, [(3.0, 20.0, 63.0, 11.5, 61)], S.Params(radius=1, window=4), [S.beach(w, h, t) for t in range(3)], pad=3)
    assert wants[-1]["records"]["pos"][0] > 0 and not flags_seen(wants) & S.OUTLIER    # no neighbour: not tested


def test_more_lines_than_a_launchs_blocks(ctx):
    """300 lines of n = 8: shoreline@1 packs four to a block, shoreline@2 is a block a line"""
    w, h = 67, 35
    lines = [(25.0 + (i % 7), (i % 35) * 1.0, 37.0 + (i % 5), (i * 3 % 35) * 1.0, 8) for i in range(300)]
    ref, wants = run(ctx, w, h, lines, S.Params(radius=1, window=2, max_jump=3.0), [S.beach(w, h, t) for t in range(3)])
    assert int(wants[-1]["summary"][3]) > 0


def test_radius_larger_than_the_picture(ctx):
    w, h = 5, 4
    img = np.zeros((h, w, 3), np.uint8)
    img[:, :2] = S.SAND
    img[:, 2:] = S.WATER
    img[3, 4] = (7, 9, 250)
    run(ctx, w, h, [(0.0, 0.5, 4.0, 3.0, 8), (0.0, 3.0, 4.0, 0.0, 9)], S.Params(radius=7, window=2), [img, img[::-1].copy()])
    run(ctx, w, h, [(0.0, 0.5, 4.0, 3.0, 8), (0.0, 3.0, 4.0, 0.0, 9)], S.Params(radius=0, window=2), [img, img[::-1].copy()], pad=2)


def test_many_blocks_with_a_polygon_roi(ctx):
    """640 x 360: the only case with many blocks, several tiles and the histogram flush and ticket of a full launch"""
    w, h = 640, 360
    lines = [(40.0, 3.0 + 5.5 * i, 600.0, 6.0 + 5.5 * i, 280) for i in range(64)]
    roi = polygon_roi(w, h)
    ref, wants = run(ctx, w, h, lines, S.Params(radius=3, window=4), [S.beach(w, h, t, amp=20) for t in range(3)], rois=[roi, roi, None], pad=8)
    assert int(wants[0]["summary"][1]) == int((roi != 0).sum()) and int(wants[2]["summary"][1]) == w * h


# ---------------------------------------------------------------------------- sources, thresholds, degenerate pictures
def test_gray_and_plane_sources_and_wet_is_high(ctx):
    w, h = 96, 64
    imgs = [S.beach(w, h, t) for t in range(3)]
    lines = S.beach_lines(w, h)
    ref, wants = run(ctx, w, h, lines, S.Params(source=S.GRAY, radius=1, window=4, wet_is_high=0), imgs)
    assert all(0 <= x["thr"] <= 255 for x in wants)
    planes = [np.ascontiguousarray(255 - i[..., 2]) for i in imgs]          # the water is bright in the inverted red plane
    ref, wants = run(ctx, w, h, lines, S.Params(source=S.PLANE, radius=2, window=4, wet_is_high=1), planes, pad=7)
    assert not flags_seen(wants) & (S.DRY | S.WET | S.EMPTY) and (wants[-1]["mask"][:, -4:] == 255).all()
    run(ctx, 67, 35, ragged_lines(67, 35), S.Params(source=S.PLANE, radius=1, window=4), [np.ascontiguousarray(S.beach(67, 35, t)[..., 2]) for t in range(2)])


def test_fixed_threshold_empty_roi_and_constant_picture(ctx):
    w, h = 96, 64
    lines, imgs = S.beach_lines(w, h), [S.beach(w, h, t) for t in range(2)]
    ref, wants = run(ctx, w, h, lines, S.Params(radius=2, window=4, threshold=230, min_sep=0.99), imgs)
    assert all(x["thr"] == 230 and 0 < x["eta"] < 0.99 for x in wants) and flags_seen(wants) & S.UNSURE
    run(ctx, w, h, lines, S.Params(radius=2, window=4, threshold=0), imgs)      # a skipped t: eta 0, every line DRY
    run(ctx, w, h, lines, S.Params(radius=2, window=4, threshold=509), imgs)
    empty = np.zeros((h, w), np.uint8)
    for p in (S.Params(radius=2, window=4), S.Params(radius=2, window=4, threshold=250)):
        ref, wants = run(ctx, w, h, lines, p, imgs, rois=[empty, None])
        first, second = wants
        assert first["thr"] == -1 and (first["records"]["flags"] == S.EMPTY | S.NO_WINDOW).all() and not first["mask"].any()
        assert (first["records"]["pos"] == -1).all() and second["thr"] >= 0 and (second["records"]["nv"] == 1).all()
    flat = np.full((h, w, 3), 90, np.uint8)
    ref, wants = run(ctx, w, h, lines, S.Params(radius=1, window=4), [flat, imgs[0], flat])
    assert wants[0]["thr"] == -1 and wants[2]["thr"] == -1 and not wants[2]["mask"].any() and (wants[2]["records"]["nv"] == 1).all()


def test_pure_noise(ctx):
    """ties in the split, DRY, WET and OUTLIER lines and NO_WINDOW"""
    w, h = 67, 35
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(6)]
    lines = [(2.0 + (i % 3), 1.0 + i * 0.5, 30.0 + i * 0.5, 2.0 + i * 0.5, 8) for i in range(60)] + [(1.0, 30.0, 65.0, 33.5, 200)]
    ref, wants = run(ctx, w, h, lines, S.Params(radius=0, window=2, max_jump=1.5), imgs, pad=1)
    seen = flags_seen(wants)
    assert seen & S.DRY and seen & S.WET and seen & S.OUTLIER and seen & S.NO_WINDOW
    ties = 0
    for x in wants:
        for g in ref.geom:
            wet = S.is_wet(x["V"][g["first"]:g["first"] + g["n"]], x["thr"], 0)
            sc = np.concatenate(([0], np.cumsum(~wet))) + np.concatenate((np.cumsum(wet[::-1])[::-1], [0]))
            ties += int((sc == sc.max()).sum() > 1)
    assert ties > 10


@pytest.mark.parametrize("T,pushes,p", [(2, 5, 1), (2, 5, 999), (64, 70, 20), (64, 70, 999), (16, 20, 1)])
def test_windows_and_ranks(ctx, T, pushes, p):
    w, h = 48, 32
    ref, wants = run(ctx, w, h, S.beach_lines(w, h), S.Params(radius=1, window=T, permille=p), [S.beach(w, h, t, amp=3) for t in range(pushes)])
    last = wants[-1]["records"]
    assert (last["nv"] == T).all() and (last["pos_q"] == (last["pos_min"] if p == 1 else last["pos_max"] if p == 999 else last["pos_q"])).all()


# ---------------------------------------------------------------------------- outputs
def test_each_output_alone_and_a_push_with_none(ctx):
    """what a push gives does not depend on which outputs it or earlier pushes asked for"""
    w, h = 67, 35
    lines, p = ragged_lines(w, h), S.Params(radius=2, window=3)
    imgs = [S.beach(w, h, t) for t in range(7)]
    ref = S.ShorelineRef(w, h, lines, p)
    ctx.shoreline_open(w, h, lines, **p.kw())
    out = outputs(ref.L, w, h)
    for t, key in enumerate(("records", "summary", "hist", "mask", "plane", None, "all")):
        d = dev_image(imgs[t]).view
        want = ref.push(imgs[t])
        fresh = outputs(ref.L, w, h)
        if key == "all":
            ctx.shoreline_push(d, **out.kw())
            compare(out.host(), ctx.shoreline_read(), want, "after the single outputs")
            continue
        ctx.shoreline_push(d, **({} if key is None else {key: fresh.kw()[key]}))
        got = fresh.host()
        if key is not None:
            a, b = (got[key], want[key]) if key != "records" else (got[key].tobytes(), want[key].tobytes())
            assert np.array_equal(a, b), "%s alone differs" % key
        for other in ("summary", "hist", "mask", "plane"):
            if other != key:
                assert np.array_equal(fresh.kw()[other].cpu().numpy(), outputs(ref.L, w, h).kw()[other].cpu().numpy()), "%s was written" % other
        rec, summ = ctx.shoreline_read()
        assert rec.tobytes() == want["records"].tobytes() and [summ[k] for k in SHORELINE_SUMMARY] == [int(v) for v in want["summary"]]
        assert np.array_equal(ctx.shoreline_ring(), ref.ring_read())
    ctx.shoreline_close()


def test_mask_goes_straight_into_regions(ctx):
    w, h = 96, 64
    img = S.beach(w, h, 3)
    p = S.Params(radius=2, window=2)
    ref = S.ShorelineRef(w, h, S.beach_lines(w, h), p)
    want = ref.push(img)
    ctx.shoreline_open(w, h, S.beach_lines(w, h), **p.kw())
    ctx.regions_open(w, h, connectivity=8, min_area=16, max_regions=16)
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    ctx.shoreline_push(dev_image(img).view, mask=mask)
    ctx.regions_push(mask)                                        # the same stream: no host round trip in between
    rec, summ = ctx.regions_read()
    wr = RG.regions(want["mask"], 8, 16, 16, None, 1)
    assert summ["kept"] == int(wr["summary"][1]) >= 1 and np.array_equal(rec["area"], wr["records"]["area"][:len(rec)])
    assert rec["area"].max() > w * h // 3                         # the sea
    ctx.regions_close()
    ctx.shoreline_close()


def test_primitives_painted_by_draw(ctx):
    w, h = 67, 35
    rng = np.random.default_rng(11)
    lines = [(2.0, 1.0 + i, 64.0, 2.0 + i, 30) for i in range(30)]
    noisy = S.beach(w, h, 0)
    noisy[8:14] = rng.integers(0, 256, (6, w, 3), dtype=np.uint8)          # lines without a position and outliers among good ones
    noisy[20:23, :, 0], noisy[20:23, :, 2] = 250, 5                         # three WET lines
    p = S.Params(radius=0, window=2, max_jump=2.0)
    ref = S.ShorelineRef(w, h, lines, p)
    ctx.shoreline_open(w, h, lines, **p.kw())
    empty = ctx.shoreline_prims(color=0x3060f0, thickness=2, disc_radius=2).cpu().numpy().view(DRAW_PRIM_DTYPE).ravel()
    assert empty.size == 2 * len(lines) - 1 and not empty.view(np.uint8).any()                 # before the first push
    ctx.shoreline_push(dev_image(noisy).view)
    want = ref.push(noisy)
    fl = want["records"]["flags"]
    assert (fl & S.OUTLIER).any() and (fl & S.WET).any() and ((fl & S.OUTLIER) == 0).sum() > 10
    prims = ctx.shoreline_prims(color=0x3060f0, thickness=2, disc_radius=2)
    got, wp = prims.cpu().numpy().view(DRAW_PRIM_DTYPE).ravel(), ref.prims(0x3060f0, 2, 2)
    assert got.tobytes() == wp.tobytes()
    assert (wp["kind"] == S.LINE).sum() == (wp["kind"] == S.DISC).sum() - 1 and (wp["kind"] == 0).any()
    canvas = dev_image(noisy, 4)
    ctx.draw(canvas.view, prims)
    painted = noisy.copy()
    TR.draw(painted, wp)
    assert np.array_equal(canvas.view.cpu().numpy(), painted) and not np.array_equal(painted, noisy)
    canvas.check("the canvas")
    ctx.shoreline_close()


# ---------------------------------------------------------------------------- set, reset, slots
def test_set_acts_from_the_next_push_and_reset_keeps_it(ctx):
    w, h = 96, 64
    lines, p = S.beach_lines(w, h), S.Params(radius=2, window=4, max_jump=8.0)
    imgs = [S.beach(w, h, t) for t in range(4)]
    ref = S.ShorelineRef(w, h, lines, p)
    ctx.shoreline_open(w, h, lines, **p.kw())
    out = outputs(ref.L, w, h)
    push = lambda t: (ctx.shoreline_push(dev_image(imgs[t]).view, **out.kw()), compare(out.host(), ctx.shoreline_read(), ref.push(imgs[t]), "push %d" % t))
    push(0)
    ctx.shoreline_set(240, 0.995, 0.05)
    ref.set(240, 0.995, 0.05)
    info = ctx.shoreline_info()
    assert (info["threshold"], info["min_sep"], info["max_jump"], info["pushes"]) == (240, 0.995, 0.05, 1)
    push(1)
    assert int(ref.summary[0]) == 240 and (ref.records["flags"] & S.UNSURE).all() and (ref.records["flags"] & S.OUTLIER).any()
    ctx.shoreline_reset()
    ref.reset()
    info = ctx.shoreline_info()
    assert (info["threshold"], info["min_sep"], info["max_jump"], info["pushes"], info["held"]) == (240, 0.995, 0.05, 0, 0)
    rec, summ = ctx.shoreline_read()
    assert not rec.view(np.uint8).any() and all(summ[k] == 0 for k in SHORELINE_SUMMARY) and (ctx.shoreline_ring() == -1).all()
    push(2)
    push(3)
    assert np.array_equal(ctx.shoreline_ring(), ref.ring_read())
    ctx.shoreline_close()


def test_two_slots(ctx):
    wa, ha, wb, hb = 96, 64, 67, 35
    pa, pb = S.Params(radius=2, window=3), S.Params(radius=1, window=2, source=S.GRAY)
    la, lb = S.beach_lines(wa, ha), ragged_lines(wb, hb)
    ra, rb = S.ShorelineRef(wa, ha, la, pa), S.ShorelineRef(wb, hb, lb, pb)
    ctx.shoreline_open(wa, ha, la, stream=0, **pa.kw())
    ctx.shoreline_open(wb, hb, lb, stream=1, **pb.kw())
    oa, ob = outputs(ra.L, wa, ha), outputs(rb.L, wb, hb)
    for t in range(4):
        ia, ib = S.beach(wa, ha, t), S.beach(wb, hb, t, seed=9)
        ctx.shoreline_push(dev_image(ia).view, stream=0, **oa.kw())
        ctx.shoreline_push(dev_image(ib).view, stream=1, **ob.kw())
        compare(oa.host(), ctx.shoreline_read(stream=0), ra.push(ia), "slot 0, push %d" % t)
        compare(ob.host(), ctx.shoreline_read(stream=1), rb.push(ib), "slot 1, push %d" % t)
    ctx.shoreline_close(stream=1)
    assert ctx.shoreline_info(stream=0)["pushes"] == 4
    ctx.shoreline_close(stream=0)


def test_product_object(ctx):
    w, h = 96, 64
    p = S.Params(radius=2, window=4)
    ref = S.ShorelineRef(w, h, S.beach_lines(w, h), p)
    with Shoreline(ctx, w, h, lines=S.beach_lines(w, h), **p.kw()) as sh:
        img = S.beach(w, h, 0)
        sh.push(dev_image(img).view)
        rec, summ = sh.read()
        want = ref.push(img)
        assert rec.tobytes() == want["records"].tobytes() and abs(summ["eta"] - want["eta"]) < 2.0 ** -32
        assert sh.info()["pushes"] == 1 and sh.ring().shape == (ref.L, 4) and sh.table()[0].size == len(ref.table)
        assert sh.prims().shape == (2 * ref.L - 1, 32)
        with pytest.raises(ValueError):
            sh.push(dev_image(img[..., 0].copy()).view)               # a plane into an 8UC3 session
        sh.set(-1, 0.5, 4.0)
        sh.reset()
        assert sh.info()["pushes"] == 0
    with pytest.raises(RcflowError):
        ctx.shoreline_info()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    w, h = 96, 64
    lines, good = S.beach_lines(w, h), S.Params(radius=2, window=4)
    L = len(lines)
    ctx.shoreline_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.shoreline_info, ctx.shoreline_read, ctx.shoreline_reset, ctx.shoreline_ring, ctx.shoreline_table,
                 lambda: ctx.shoreline_set(-1, 0.0, 8.0), ctx.shoreline_prims):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 64)()
    for name, args in (("info", (C.byref(ShorelineInfo()),)), ("read", (buf, buf)), ("reset", ()), ("ring_read", (buf,)), ("table_read", (buf, buf)),
                       ("set", (-1, 0.0, 8.0)), ("prims_dev", (1, 1, 2, buf)), ("push_dev", (null, 0, 3, null, 0, null, null, 0, null, 0, null, null))):
        assert getattr(lib, "rcflow_shoreline_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_shoreline_%s:" % name), text()
    nan, inf = float("nan"), float("inf")
    kw = good.kw()
    for bad in (dict(radius=-1), dict(radius=8), dict(wet_is_high=2), dict(wet_is_high=-1), dict(threshold=-2), dict(threshold=510), dict(window=1),
                dict(window=4097), dict(permille=0), dict(permille=1000), dict(min_sep=-0.1), dict(min_sep=1.1), dict(min_sep=nan), dict(max_jump=0.0),
                dict(max_jump=16385.0), dict(max_jump=nan), dict(max_jump=inf), dict(metres_per_pixel=0.0), dict(metres_per_pixel=nan),
                dict(metres_per_pixel=inf)):
        with pytest.raises(RcflowError) as e:
            ctx.shoreline_open(w, h, lines, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_shoreline_open"), bad
    for bad_lines in ([(4.0, 4.0, 96.5, 4.0, 88)], [(4.0, 4.0, 91.0, 64.0, 88)], [(4.0, 4.0, 91.0, 4.0, 7)], [(4.0, 4.0, 91.0, 4.0, 1025)],
                      [(4.0, 4.0, 4.0, 4.0, 8)], lines * 100, [(4.0, 4.0, 91.0, 4.0, 1024)] * 257):
        with pytest.raises(RcflowError) as e:
            ctx.shoreline_open(w, h, bad_lines, **kw)                 # a line leaving the picture, n, no length, too many, S above the bound
        assert e.value.code == EINVAL and text().startswith("rcflow_shoreline_open"), bad_lines[0]
    arr = (TransectLine * L)(*[TransectLine(*l) for l in lines])
    p = ShorelineParams(source=3, radius=2, wet_is_high=0, threshold=-1, window=4, permille=20, flags=0, pad=0, min_sep=0.0, max_jump=8.0, metres_per_pixel=1.0)
    assert lib.rcflow_shoreline_open(hdl, 0, w, h, arr, L, C.byref(p)) == EINVAL          # no such source
    p.source, p.flags = 0, 1
    assert lib.rcflow_shoreline_open(hdl, 0, w, h, arr, L, C.byref(p)) == EINVAL          # unknown flag bits
    p.flags = 0
    assert lib.rcflow_shoreline_open(hdl, 0, w, h, arr, L, None) == EINVAL
    assert lib.rcflow_shoreline_open(hdl, 0, w, h, None, L, C.byref(p)) == EINVAL
    assert lib.rcflow_shoreline_open(hdl, 0, 0, h, arr, L, C.byref(p)) == EINVAL
    assert lib.rcflow_shoreline_open(hdl, 2, w, h, arr, L, C.byref(p)) == EINVAL          # no such slot
    big_lines = [(4.0, 4.0 + i, 91.0, 4.0 + i, 8) for i in range(1024)]
    with pytest.raises(RcflowError) as e:
        ctx.shoreline_open(4000, 2161, lines, **kw)                   # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_shoreline_open")
    ctx.shoreline_open(1200, 1100, big_lines, **dict(kw, window=4096))                    # 16 MiB of ring: inside the bound
    assert ctx.shoreline_info()["device_bytes"] >= 4 * 4096 * 1024 + 2 * 1200 * 1100
    ctx.shoreline_close()
    with pytest.raises(RcflowError):
        ctx.shoreline_info()                                          # nothing was left open by any of them

    ref, _ = run(ctx, w, h, lines, good, [S.beach(w, h, 0)], keep_open=True)
    assert lib.rcflow_shoreline_info(hdl, 0, None) == EINVAL and lib.rcflow_shoreline_ring_read(hdl, 0, None) == EINVAL
    before = ctx.shoreline_info()
    for bad in (dict(radius=8), dict(window=1)):                      # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.shoreline_open(w, h, lines, **dict(kw, **bad))
    assert ctx.shoreline_info() == before
    img = dev_image(S.beach(w, h, 1)).view
    big = torch.zeros(8 * h * w + 256, dtype=torch.uint8, device="cuda")

    def push(image=None, step=3 * w, ch=3, roi=(null, 0), rec=null, mask=(null, 0), plane=(null, 0), hist=null, summ=null, slot=0):
        return lib.rcflow_shoreline_push_dev(hdl, slot, ptr(img) if image is None else image, step, ch, roi[0], roi[1], rec, mask[0], mask[1],
                                             plane[0], plane[1], hist, summ)

    refused = [
        push(image=null), push(step=3 * w - 1), push(ch=1), push(ch=4), push(ch=0),                  # the wrong channel count for the source
        push(roi=(ptr(big), w - 1)), push(rec=ptr(big, 2)), push(mask=(ptr(big), w - 1)), push(plane=(ptr(big), 2 * w - 2)),
        push(plane=(ptr(big, 1), 2 * w)), push(plane=(ptr(big), 2 * w + 1)), push(hist=ptr(big, 2)), push(summ=ptr(big, 4)),
        push(mask=(ptr(img), w)),                                     # an output over the picture
        push(roi=(ptr(big, 64), w), plane=(ptr(big), 2 * w)),         # the region of interest inside an output
        push(mask=(ptr(big), w), plane=(ptr(big, w * (h - 1)), 2 * w)),                             # two outputs meeting in one row
        push(rec=ptr(big), hist=ptr(big, 64 * L - 4)), push(hist=ptr(big), summ=ptr(big, 2040)), push(mask=(ptr(big), w), summ=ptr(big)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert text().startswith("rcflow_shoreline_push_dev")
    assert push(slot=2) == EINVAL
    for bad in ((-2, 0.0, 8.0), (510, 0.0, 8.0), (-1, nan, 8.0), (-1, 1.5, 8.0), (-1, 0.0, 0.0), (-1, 0.0, inf)):
        with pytest.raises(RcflowError) as e:
            ctx.shoreline_set(*bad)
        assert e.value.code == EINVAL and text().startswith("rcflow_shoreline_set")
    assert lib.rcflow_shoreline_prims_dev(hdl, 0, 1, 0, 2, ptr(big)) == EINVAL and lib.rcflow_shoreline_prims_dev(hdl, 0, 1, 1, 2, null) == EINVAL
    assert text().startswith("rcflow_shoreline_prims_dev")
    assert ctx.shoreline_info() == before
    # nothing was queued and nothing changed: the second push gives what the statement gives
    out = outputs(L, w, h)
    ctx.shoreline_push(img, **out.kw())
    compare(out.host(), ctx.shoreline_read(), ref.push(S.beach(w, h, 1)), "(after the refusals)")
    # an accepted boundary: the plane begins at the first byte after the mask's range, in one allocation
    one = torch.full((3 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tm, tp = one[:h * w].view(h, w), one[h * w:3 * h * w].view(torch.int16).view(h, w)
    ctx.shoreline_push(img, mask=tm, plane=tp)
    want = ref.push(S.beach(w, h, 1))
    assert np.array_equal(tm.cpu().numpy(), want["mask"]) and np.array_equal(tp.cpu().numpy().view(np.uint16), want["plane"]) and (one[3 * h * w:] == SENTINEL).all()
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.shoreline_push(img, **out.kw())
        got = ctx.shoreline_read()
    torch.cuda.synchronize()
    compare(out.host(), got, ref.push(S.beach(w, h, 1)), "(on another stream)")
    # re-open with another size replaces it
    run(ctx, 67, 35, ragged_lines(67, 35), S.Params(radius=1, window=2), [S.beach(67, 35, 0)])
    ctx.shoreline_close()                                             # closing twice is fine
