"""The mean current on the device (meanflow_kernels.hip) against its numpy statement (tests/_meanflow_ref.py): the mean, the
steadiness, the spread, the mask, the picture, the records, the cell sums and the summary of every push, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _kinematics_ref as KN
import _meanflow_ref as M
import _regions_ref as RG
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ptr, raw, same_bits
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RC_MEANFLOW_LAUNCHES, MeanflowInfo, MeanflowParams, RcflowError
from ripcurrents_amd.api import MEANFLOW_CELL_DTYPE, MEANFLOW_SUMMARY, MeanFlow

pytestmark = pytest.mark.gpu

IMAGES = M.PICTURES
ARRAYS = ("cells", "sums", "summary")
FLOATS = ("mean", "std")
MF_MAX_BLOCKS0, MF_MAX_BLOCKS1, MF_WAVES, MF_TW = 256, 1024, 4, 256      # meanflow_kernels.hip: the caps on the launches' blocks, a block's waves, a wave's columns
dev_field = Padded.of                                             # a field on the device, rows `pad` pixels longer and the sentinel there


def views(d):
    if "steady" in d:
        d["steady"] = d["steady"].view(np.uint16)
    if "cells" in d:
        d["cells"] = d["cells"].view(MEANFLOW_CELL_DTYPE)
    if "sums" in d:
        d["sums"] = d["sums"].reshape(-1, M.SUMS)


def outputs(p, w, h, pad=0, pictures=True):
    nc = p.grid_x * p.grid_y
    planes = {}
    if pictures:
        planes = dict(mean=((h, w, 2), torch.float32), steady=((h, w), torch.int16), std=((h, w, 2), torch.float32), mask=((h, w), torch.uint8),
                      picture=((h, w, 3), torch.uint8))
    flat = dict(cells=((nc * 32,), torch.uint8, None), sums=((nc * M.SUMS,), torch.int64, -1), summary=((8,), torch.int64, -1))
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
        assert np.array_equal(rs.reshape(-1, M.SUMS), want["sums"]), "the slot's sums differ " + what
        assert [rsum[k] for k in MEANFLOW_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


def run(ctx, w, h, p, fields, pad=0, stream=0, keep_open=False, pictures_from=0):
    """a sequence of fields through the device session and the statement; records, sums and summary compared after every push, the
    five pictures too from push `pictures_from` on -> (the statement, its outputs of every push)"""
    ref = M.MeanFlowRef(w, h, p, ctx.jet_lut())
    ctx.meanflow_open(w, h, stream=stream, **p.kw())
    info = ctx.meanflow_info(stream=stream)
    assert info["launches_per_push"] == RC_MEANFLOW_LAUNCHES == 2 and info["device_bytes"] >= M.state_bytes(w, h, p.window)
    full, lean, wants = outputs(p, w, h, pad), outputs(p, w, h, pad, pictures=False), []
    cache = {}
    for t, f in enumerate(fields):
        if id(f) not in cache:
            cache[id(f)] = (dev_field(f, pad), f)
        d = cache[id(f)][0]
        out = full if t >= pictures_from else lean
        want = ref.push(f, pictures=out is full)
        ctx.meanflow_push(d.view, stream=stream, **out.kw())
        compare(out.host(), ctx.meanflow_read(stream=stream), want, "after push %d" % (t + 1))
        info = ctx.meanflow_info(stream=stream)
        assert (info["held"], info["pushes"]) == (min(t + 1, p.window), t + 1)
        wants.append(want)
    for d, f in cache.values():
        assert same_bits(d.view.cpu().numpy(), f), "the field was written"
        d.check("the field")
    if not keep_open:
        ctx.meanflow_close(stream=stream)
    return ref, wants


def with_(p, **kw):
    return M.Params(**{**M.asdict(p), **kw})


# ---------------------------------------------------------------------------- the scene
@pytest.mark.parametrize("name", ["fixed", "opposed"])
def test_naming_scene_every_output_after_every_push(ctx, name):
    """the scene of the CPU tier, 20 pushes into a window of 8: the mask is the jet"""
    p, kw = (M.NAMING, {}) if name == "fixed" else (M.OPPOSED, M.OPPOSED_SCENE)
    ref, wants = run(ctx, 20, 12, p, [M.naming_scene(t, **kw) for t in range(20)], pad=3)
    assert np.array_equal(wants[-1]["mask"], M.jet_mask(jet=kw.get("jet", (8, 12)))) and not wants[p.window - 2]["mask"].any()
    assert (name == "fixed") or wants[-1]["summary"][4] > 0


def test_resident_flow_field(ctx):
    """d_flow_xy = NULL: the field the frame loop left on the slot"""
    w, h = 256, 192
    clip = synth.surf_clip(w, h, 5)
    p = M.Params(window=2, grid_x=8, grid_y=6, min_fill=1, steady_min=300, flags=M.DIR_OPPOSED, speed_min=0.1, min_cos2=0.25)
    ctx.stream_reset()
    ctx.meanflow_open(w, h, **p.kw())
    ref, out = M.MeanFlowRef(w, h, p, ctx.jet_lut()), outputs(p, w, h, 1)
    with pytest.raises(RcflowError) as e:
        ctx.meanflow_push(None)
    assert e.value.code == ESTATE and ctx.meanflow_info()["pushes"] == 0
    pushed = 0
    for t in range(5):
        flow = ctx.push_frame_host(clip[t])
        if flow is None:
            continue
        ctx.meanflow_push(None, **out.kw())
        compare(out.host(), ctx.meanflow_read(), ref.push(flow.cpu().numpy()), "after frame %d" % t)
        pushed += 1
    assert pushed >= 3 and ref.summary[0] == w * h
    ctx.meanflow_open(128, 96, **p.kw())
    with pytest.raises(RcflowError) as e:
        ctx.meanflow_push(None)
    assert e.value.code == ESIZE
    ctx.meanflow_close()


# ---------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("w,h,gx,gy", [(5, 3, 2, 1), (37, 19, 5, 4), (130, 7, 3, 2), (257, 9, 4, 4), (260, 12, 260, 12)])
def test_ragged_with_padded_steps(ctx, w, h, gx, gy):
    """5 x 3: narrower than the 4 pixels of two lanes; 37 x 19 and 130 x 7: widths that are no multiple of 4, a last lane of 1 and
    of 2 pixels; 257 x 9: one pixel into a second block column; these grids have remainder columns and rows.  260 x 12 with a cell a
    pixel: 1024 cells under the first block, more than the 256 its table in LDS holds, so its sums go straight to memory.  The ring
    wraps"""
    p = M.Params(window=3, grid_x=gx, grid_y=gy, min_fill=2, steady_min=200, speed_min=0.5, min_cos2=0.1, dir_x=1.0, dir_y=-1.0)
    ref, wants = run(ctx, w, h, p, [M.hostile_field(w, h, t, seed=w) for t in range(8)], pad=5)
    assert any(x["mask"].any() for x in wants) and wants[-1]["std"].max() > 0 and wants[-1]["summary"][2] > 0


def test_more_rows_than_one_pass_of_the_capped_grids(ctx):
    """meanflow@0 is launched with at most MF_MAX_BLOCKS0 = 256 blocks and meanflow@1 with at most MF_MAX_BLOCKS1 = 1024, of 4 waves,
    a wave a row of 256 columns at a time: 260 columns are two block columns, so a pass is 512 rows of meanflow@0 and 2048 of
    meanflow@1.  At 2052 rows a wave of meanflow@0 walks five rows and one of meanflow@1 two, and with cell rows of 3 pixels both change
    their cell row on the way"""
    w, h = 260, 2052
    tx = (w + MF_TW - 1) // MF_TW
    assert tx == 2 and (MF_MAX_BLOCKS0 // tx) * MF_WAVES == 512 < (MF_MAX_BLOCKS1 // tx) * MF_WAVES == 2048 < h
    p = M.Params(window=2, grid_x=4, grid_y=684, min_fill=1, steady_min=300, flags=M.DIR_OPPOSED, speed_min=0.5, min_cos2=0.1)
    run(ctx, w, h, p, [M.hostile_field(w, h, t, seed=5) for t in range(3)], pad=3)


# ---------------------------------------------------------------------------- window
def test_window_2_three_wraps(ctx):
    p = M.Params(window=2, grid_x=3, grid_y=2, min_fill=2, steady_min=100, speed_min=0.0, min_cos2=0.0, dir_x=-1.0, dir_y=0.5)
    run(ctx, 37, 19, p, [M.hostile_field(37, 19, t, seed=2) for t in range(7)], pad=2)


def test_window_4096_the_bounds_of_the_sums_and_the_wrap(ctx):
    """4100 pushes of +-499.999 (q = +-32000) into W = 4096 on 16 x 8: the left half holds its signs and reaches the bounds of Su, Sv,
    Sm and n Suu, the right half flips with every push.  Records, sums and summary after every push; the pictures for the last 8"""
    w, h, W, v = 16, 8, 4096, np.float32(499.999)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    a = np.stack([np.where(x % 2 == 0, v, -v), np.where(y % 2 == 0, v, -v)], -1).astype(np.float32)
    b = a.copy()
    b[:, 8:] = -b[:, 8:]
    p = M.Params(window=W, grid_x=2, grid_y=2, min_fill=W, steady_min=900, speed_min=400.0, min_cos2=0.25, dir_x=1.0, dir_y=1.0)
    ref, wants = run(ctx, w, h, p, [a if t % 2 == 0 else b for t in range(4100)], pictures_from=4092)
    bd = ref.bounds()
    assert bd["S"] == 4096 * 32000 and bd["nS2"] == 4096 * 4096 * 32000 ** 2 and bd["SS"] == 2 * (4096 * 32000) ** 2
    last = wants[-1]
    assert (last["steady"][:, :8] >= 999).all() and not last["steady"][:, 8:].any() and not last["std"][:, :8].any()
    assert (last["std"][:, 8:, 0] > 499.9).all() and not last["std"][:, 8:, 1].any() and last["summary"][0] == w * h and wants[4094]["summary"][0] == 0
    assert last["mask"][0, 0] == 255 and last["mask"][1, 1] == 0 and last["mask"][:, :8].any() and not last["mask"][:, 8:].any()


# ---------------------------------------------------------------------------- samples
@pytest.mark.parametrize("min_fill", [1, 4])
def test_bad_samples_enter_and_leave(ctx, min_fill):
    """NaN, +-inf, +-500.0 and +-499.99997 in one or both components come and go; pixel (0, 0) is bad throughout, pixel (1, 1) for a
    whole window; min_fill below and at W while the ring fills"""
    w, h, W = 9, 6, 4
    fields = [M.hostile_field(w, h, t, seed=9) for t in range(14)]
    for t, f in enumerate(fields):
        f[0, 0] = (np.nan, 1.0)
        f[2, 3] = (499.99997, -499.99997)                     # the largest good sample, both components
        f[3, 3] = (500.0, 0.0) if t % 2 else (0.0, -np.inf)
        f[1, 1] = (np.inf, np.nan) if 4 <= t < 8 else (1.0, -2.0)
    p = M.Params(window=W, grid_x=3, grid_y=2, min_fill=min_fill, steady_min=100, speed_min=0.25, min_cos2=0.0, dir_x=0.3, dir_y=-1.0)
    ref, wants = run(ctx, w, h, p, fields, pad=1)
    filled = [x["summary"][0] for x in wants]
    assert filled[0] == (0 if min_fill == W else filled[0]) and filled[0] < max(filled) and min(filled[W:]) < max(filled)     # n falls and recovers
    assert ref.n[0, 0] == 0 and ref.n[3, 3] == 0 and ref.n[2, 3] == W and ref.Su[2, 3] == W * 32000
    assert wants[7]["steady"][1, 1] == 0 and not wants[7]["mean"][1, 1].any() and wants[-1]["steady"][1, 1] > 0      # its whole window was bad
    assert all(x["sums"][0, 6] >= 1 for x in wants)


def test_all_zero_field(ctx):
    w, h = 20, 12
    ref, wants = run(ctx, w, h, with_(M.NAMING, window=3, min_fill=2, steady_min=0, speed_min=0.0), [np.zeros((h, w, 2), np.float32)] * 5)
    last = wants[-1]
    assert last["summary"][0] == w * h and last["summary"][5] == 0 and not last["steady"].any() and not last["mask"].any()
    assert not last["std"].any() and not last["mean"].any() and (last["picture"] == np.asarray(ctx.jet_lut()).reshape(256, 3)[0]).all()


# ---------------------------------------------------------------------------- decisions
def test_decision_edges(ctx):
    """a pixel with R = smin_q n exactly is in, one a 64th of a pixel slower is out; K = 0 lets every pixel with dot > 0 in;
    steady_min 0 and 1000"""
    w, h, W = 8, 4, 3
    f = np.zeros((h, w, 2), np.float32)
    f[..., 1] = -0.5                                          # q = -32: R = 32 n
    f[:, 4:, 1] = -0.484375                                   # q = -31
    f[2:, :, 0] = 0.25
    base = M.Params(window=W, grid_x=2, grid_y=2, min_fill=W, steady_min=1000, speed_min=0.5, min_cos2=0.9, dir_x=0.0, dir_y=-1.0)
    ref, wants = run(ctx, w, h, base, [f] * 4)
    m = wants[-1]["mask"]
    assert m[:2, :4].all() and not m[:2, 4:].any()            # R = 32 n = smin_q n: in; 31 n: out
    assert ref.steadiness()[1][0, 0] == 1000 and (ref.steadiness()[0][0, :4] == 32 * W).all()
    assert not m[2:].any()                                    # (16, -32): isqrt floors m to 35, R = 107 = 3 * 35 + 2; cos^2 = 0.8 < 0.9
    ref, wants = run(ctx, w, h, with_(base, min_cos2=0.0, speed_min=0.0, dir_x=1.0, dir_y=0.0), [f] * 4)
    assert wants[-1]["mask"][2:].all() and not wants[-1]["mask"][:2].any()      # K = 0: dot > 0 alone; rows 0 and 1 have dot = 0
    noisy = [M.naming_scene(t) for t in range(10)]
    ref, wants = run(ctx, 20, 12, with_(M.NAMING, steady_min=0, speed_min=0.0, min_cos2=0.0), noisy)
    assert np.array_equal(wants[-1]["mask"] > 0, ref.Sv < 0)
    ref, wants = run(ctx, 20, 12, with_(M.NAMING, steady_min=1000, speed_min=0.0, min_cos2=0.0), noisy)
    assert not wants[-1]["mask"].any() and wants[-1]["steady"].max() < 1000


def test_opposed_with_g_zero_names_nothing(ctx):
    w, h = 8, 4
    f = np.zeros((h, w, 2), np.float32)
    f[:, :4, 1], f[:, 4:, 1] = 1.0, -1.0
    p = M.Params(window=2, grid_x=2, grid_y=1, min_fill=1, steady_min=0, flags=M.DIR_OPPOSED, speed_min=0.0, min_cos2=0.0)
    ref, wants = run(ctx, w, h, p, [f] * 3)
    assert all(x["summary"][3] == 0 and x["summary"][4] == 0 and not x["mask"].any() for x in wants)
    assert wants[-1]["sums"][0, 3] == 16 * 2 * 64 and wants[-1]["sums"][1, 3] == -16 * 2 * 64


# ---------------------------------------------------------------------------- grids
@pytest.mark.parametrize("gx,gy", [(1, 1), (20, 12), (3, 5), (7, 2)])
def test_grids(ctx, gx, gy):
    """one cell; a cell a pixel (240 cells, every lane's four pixels in four cells); remainder columns and rows (20 = 3 * 6 + 2,
    12 = 5 * 2 + 2; 20 = 7 * 2 + 6)"""
    ref, wants = run(ctx, 20, 12, with_(M.NAMING, grid_x=gx, grid_y=gy, window=4, min_fill=3), [M.naming_scene(t) for t in range(7)], pad=1)
    assert wants[-1]["sums"][:, 0].sum() == 240 and wants[-1]["cells"].size == gx * gy


# ---------------------------------------------------------------------------- outputs and plumbing
def test_each_output_alone_and_none(ctx):
    """what a push asks for changes nothing of what this or a later push gives"""
    w, h, p = 37, 19, with_(M.NAMING, window=3, min_fill=2, grid_x=5, grid_y=4)
    ref, out = M.MeanFlowRef(w, h, p, ctx.jet_lut()), outputs(p, w, h, 2)
    ctx.meanflow_open(w, h, **p.kw())
    asks = [()] + [(k,) for k in IMAGES + ARRAYS] + [()]
    for t, only in enumerate(asks * 2):
        f = M.naming_scene(t, w, h)
        want = ref.push(f)
        ctx.meanflow_push(dev_field(f, 1).view, **out.kw(only))
        got = out.host()
        compare({k: got[k] for k in only}, ctx.meanflow_read(), want, "push %d asking %s" % (t, only))
    f = M.naming_scene(99, w, h)
    ctx.meanflow_push(dev_field(f).view, **out.kw())
    compare(out.host(), ctx.meanflow_read(), ref.push(f), "(every output, after the lone ones)")
    ctx.meanflow_close()


def test_two_slots(ctx):
    pa, pb = M.NAMING, M.Params(window=3, grid_x=5, grid_y=4, min_fill=2, steady_min=200, flags=M.DIR_OPPOSED, speed_min=0.25, min_cos2=0.1)
    (wa, ha), (wb, hb) = (20, 12), (37, 19)
    ra, rb = M.MeanFlowRef(wa, ha, pa, ctx.jet_lut()), M.MeanFlowRef(wb, hb, pb, ctx.jet_lut())
    ctx.meanflow_open(wa, ha, stream=0, **pa.kw())
    ctx.meanflow_open(wb, hb, stream=1, **pb.kw())
    oa, ob = outputs(pa, wa, ha), outputs(pb, wb, hb, 1)
    for t in range(10):
        fa, fb = M.naming_scene(t), M.hostile_field(wb, hb, t)
        ctx.meanflow_push(dev_field(fa).view, stream=0, **oa.kw())
        ctx.meanflow_push(dev_field(fb, 1).view, stream=1, **ob.kw())
        compare(oa.host(), ctx.meanflow_read(stream=0), ra.push(fa), "slot 0, push %d" % t)
        compare(ob.host(), ctx.meanflow_read(stream=1), rb.push(fb), "slot 1, push %d" % t)
    ctx.meanflow_close(stream=1)
    assert ctx.meanflow_info(stream=0)["pushes"] == 10
    ctx.meanflow_close(stream=0)


def test_set_acts_from_the_next_push_and_reset_keeps_it(ctx):
    w, h, p = 20, 12, with_(M.NAMING, window=4, min_fill=4)
    ref, out = M.MeanFlowRef(w, h, p, ctx.jet_lut()), outputs(p, w, h)
    ctx.meanflow_open(w, h, **p.kw())

    def push(t):
        f = M.naming_scene(t)
        ctx.meanflow_push(dev_field(f).view, **out.kw())
        compare(out.host(), ctx.meanflow_read(), ref.push(f), "push %d" % t)
    for t in range(5):
        push(t)
    new = dict(steady_min=350, speed_min=0.125, min_cos2=0.25, dir_x=1.0, dir_y=-3.0, min_fill=2)
    ctx.meanflow_set(**new)
    ref.set(**new)
    info = ctx.meanflow_info()
    assert {k: info[k] for k in new} == new and info["pushes"] == 5
    push(5)
    push(6)
    ctx.meanflow_reset()
    ref.reset()
    info = ctx.meanflow_info()
    assert {k: info[k] for k in new} == new and (info["pushes"], info["held"]) == (0, 0)
    rc, rs, rsum = ctx.meanflow_read()
    assert not rc.view(np.uint8).any() and not rs.any() and all(rsum[k] == 0 for k in MEANFLOW_SUMMARY)
    for t in range(7, 14):                                    # from nothing again: what the ring held before the reset is not seen
        push(t)
    ctx.meanflow_close()


def test_mask_into_regions_and_mean_into_kinematics(ctx):
    """the mask is what rcflow_regions_push_dev takes and d_mean what rcflow_kinematics_push_dev takes, unchanged, on one stream"""
    w, h = 20, 12
    ref = M.MeanFlowRef(w, h, M.NAMING, ctx.jet_lut())
    ctx.meanflow_open(w, h, **M.NAMING.kw())
    ctx.regions_open(w, h, connectivity=8, min_area=4, max_regions=8)
    kp = KN.params(radius=1, sigma=1.0, spacing=1, grid_x=2, grid_y=2)
    ctx.kinematics_open(w, h, **kp)
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    mean = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    omega = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    for t in range(12):
        f = M.naming_scene(t)
        want = ref.push(f)
        ctx.meanflow_push(dev_field(f).view, mask=mask, mean=mean)
    ctx.regions_push(mask)
    ctx.kinematics_push(mean, omega=omega)
    rec, summ = ctx.regions_read()
    wr = RG.regions(want["mask"], 8, 4, 8, None, 1)
    assert summ["kept"] == int(wr["summary"][1]) == 1 and rec["area"][0] == 48 == wr["records"]["area"][0]       # the jet, one region
    wk = KN.kinematics(want["mean"], ctx.jet_lut(), kp)
    assert same_bits(omega.cpu().numpy(), wk["omega"]) and np.abs(wk["omega"]).max() > 0
    ctx.kinematics_close()
    ctx.regions_close()
    ctx.meanflow_close()


def test_product_object(ctx):
    w, h = 20, 12
    ref = M.MeanFlowRef(w, h, M.NAMING, ctx.jet_lut())
    with MeanFlow(ctx, w, h, **M.NAMING.kw()) as mf:
        steady = torch.zeros((h, w), dtype=torch.int16, device="cuda")
        for t in range(9):
            f = M.naming_scene(t)
            mf.push(dev_field(f).view, steady=steady)
            want = ref.push(f)
        rc, rs, rsum = mf.read()
        assert same("cells", rc.ravel(), want["cells"]) and rsum["pushes"] == 9 and np.array_equal(steady.cpu().numpy().view(np.uint16), want["steady"])
        assert mf.info()["pushes"] == 9 and mf.info()["opposed"] is False
        with pytest.raises(ValueError):
            mf.push(dev_field(f[..., 0]).view)                # one component is no field
        mf.set(350, 0.125, 0.25, 1.0, -3.0, 2)
        mf.reset()
        assert mf.info()["pushes"] == 0 and mf.info()["steady_min"] == 350
    with pytest.raises(RcflowError):
        ctx.meanflow_info()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    w, h = 20, 12
    good = with_(M.NAMING, window=4, min_fill=3)
    nc = good.grid_x * good.grid_y
    ctx.meanflow_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.meanflow_info, ctx.meanflow_read, ctx.meanflow_reset, lambda: ctx.meanflow_set(600, 0.5, 0.5, 0., -1., 1)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 1024)()
    for name, args in (("info", (C.byref(MeanflowInfo()),)), ("read", (buf, buf, buf)), ("reset", ()), ("set", (600, 0.5, 0.5, 0., -1., 1)),
                       ("push_dev", (null, 0) + (null, 0) * 5 + (null, null, null))):
        assert getattr(lib, "rcflow_meanflow_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_meanflow_%s:" % name), text()
    nan, inf = float("nan"), float("inf")
    kw = good.kw()
    for bad in (dict(window=1), dict(window=4097), dict(min_fill=0), dict(min_fill=5), dict(steady_min=-1), dict(steady_min=1001), dict(speed_min=-0.5),
                dict(speed_min=400.5), dict(speed_min=nan), dict(speed_min=inf), dict(min_cos2=-0.1), dict(min_cos2=1.0), dict(min_cos2=nan),
                dict(dir_x=0.0, dir_y=0.0), dict(dir_x=nan), dict(dir_y=inf), dict(grid_x=0), dict(grid_x=21), dict(grid_y=13)):
        assert M.open_error(w, h, with_(good, **bad)) in ("parameters", "grid")
        with pytest.raises(RcflowError) as e:
            ctx.meanflow_open(w, h, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_meanflow_open"), bad
    ctx.meanflow_open(w, h, **dict(kw, opposed=True, dir_x=0.0, dir_y=0.0))      # the direction is not looked at
    ctx.meanflow_close()
    p = MeanflowParams(window=4, grid_x=4, grid_y=3, min_fill=3, steady_min=600, flags=0, speed_min=0.5, min_cos2=0.5, dir_x=0.0, dir_y=-1.0)
    for flags in (0, 3, 4):
        p.flags = flags
        assert lib.rcflow_meanflow_open(hdl, 0, w, h, C.byref(p)) == EINVAL and "exactly one" in text()
    p.flags = 1
    assert lib.rcflow_meanflow_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_meanflow_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_meanflow_open(hdl, 2, w, h, C.byref(p)) == EINVAL               # no such slot
    with pytest.raises(RcflowError) as e:
        ctx.meanflow_open(4000, 2161, **kw)                           # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_meanflow_open")
    with pytest.raises(RcflowError) as e:
        ctx.meanflow_open(1920, 1080, **dict(kw, window=4096, min_fill=1))      # 34 GB of ring
    assert e.value.code == ESIZE and text().startswith("rcflow_meanflow_open") and str(M.state_bytes(1920, 1080, 4096)) in text()
    with pytest.raises(RcflowError):
        ctx.meanflow_info()                                           # nothing was left open by any of them

    ref, _ = run(ctx, w, h, good, [M.naming_scene(0)], keep_open=True)
    assert lib.rcflow_meanflow_info(hdl, 0, None) == EINVAL
    before = ctx.meanflow_info()
    for bad in (dict(window=1), dict(min_fill=9)):                    # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.meanflow_open(w, h, **dict(kw, **bad))
    assert ctx.meanflow_info() == before
    fld = dev_field(M.naming_scene(1)).view
    big = torch.zeros(32 * h * w + 4096, dtype=torch.uint8, device="cuda")
    N = (null, 0)

    def push(field=None, step=8 * w, mean=N, steady=N, std=N, mask=N, pic=N, cells=null, sums=null, summ=null, slot=0):
        return lib.rcflow_meanflow_push_dev(hdl, slot, ptr(fld) if field is None else field, step, *mean, *steady, *std, *mask, *pic, cells, sums, summ)

    refused = [
        push(step=8 * w - 8), push(step=8 * w + 4), push(field=ptr(fld, 4)),
        push(mean=(ptr(big), 8 * w - 8)), push(mean=(ptr(big, 4), 8 * w)), push(mean=(ptr(big), 8 * w + 4)), push(std=(ptr(big), 8 * w - 8)),
        push(std=(ptr(big, 4), 8 * w)), push(steady=(ptr(big), 2 * w - 2)), push(steady=(ptr(big, 1), 2 * w)), push(steady=(ptr(big), 2 * w + 1)),
        push(mask=(ptr(big), w - 1)), push(pic=(ptr(big), 3 * w - 1)), push(cells=ptr(big, 2)), push(sums=ptr(big, 4)), push(summ=ptr(big, 4)),
        push(mean=(ptr(fld), 8 * w)),                                 # an output over the field
        push(mask=(ptr(fld, 8), w)),
        push(mean=(ptr(big), 8 * w), std=(ptr(big, 8 * w * (h - 1)), 8 * w)),     # two outputs meeting in one row
        push(mask=(ptr(big), w), pic=(ptr(big, 16), 3 * w)), push(cells=ptr(big), sums=ptr(big, 32 * nc - 8)), push(sums=ptr(big), summ=ptr(big, 64 * nc - 8)),
        push(steady=(ptr(big), 2 * w), summ=ptr(big)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert text().startswith("rcflow_meanflow_push_dev")
    assert push(slot=2) == EINVAL
    for bad in ((1001, 0.5, 0.5, 0., -1., 3), (600, -1.0, 0.5, 0., -1., 3), (600, 0.5, 1.0, 0., -1., 3), (600, 0.5, 0.5, 0., 0., 3),
                (600, 0.5, 0.5, nan, -1., 3), (600, 0.5, 0.5, 0., -1., 0), (600, 0.5, 0.5, 0., -1., 5)):
        with pytest.raises(RcflowError) as e:
            ctx.meanflow_set(*bad)
        assert e.value.code == EINVAL and text().startswith("rcflow_meanflow_set")
    assert ctx.meanflow_info() == before
    # nothing was queued and nothing changed: the second push gives what the statement gives
    out = outputs(good, w, h)
    ctx.meanflow_push(fld, **out.kw())
    compare(out.host(), ctx.meanflow_read(), ref.push(M.naming_scene(1)), "(after the refusals)")
    # an accepted boundary: steady begins at the first byte after the mask's range, in one allocation
    one = torch.full((3 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tm, ts = one[:h * w].view(h, w), one[h * w:3 * h * w].view(torch.int16).view(h, w)
    ctx.meanflow_push(fld, mask=tm, steady=ts)
    want = ref.push(M.naming_scene(1))
    assert np.array_equal(tm.cpu().numpy(), want["mask"]) and np.array_equal(ts.cpu().numpy().view(np.uint16), want["steady"]) and (one[3 * h * w:] == SENTINEL).all()
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.meanflow_push(fld, **out.kw())
        got = ctx.meanflow_read()
    torch.cuda.synchronize()
    compare(out.host(), got, ref.push(M.naming_scene(1)), "(on another stream)")
    # re-open with another size replaces it
    run(ctx, 37, 19, M.Params(window=2, grid_x=2, grid_y=2, min_fill=1), [M.hostile_field(37, 19, t) for t in range(3)])
    ctx.meanflow_close()                                              # closing twice is fine
    ctx.meanflow_close()
