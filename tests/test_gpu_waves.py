"""The wave spectra on the device (waves_kernels.hip) against their numpy statement (tests/_waves_ref.py): the table, the
accumulators, the cell sums, the bin map, the summary and every integer of the records bit for bit; the records' floats within
one unit in the last place; the picture wherever the statement's depth is not within that of a colour's boundary."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cpp
import _waves_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ordered, ptr, raw, reference
from ripcurrents_amd._lib import RC_WAVES_LAUNCHES, RC_WAVES_MAX_STATE_BYTES, RcflowError, WavesParams
from ripcurrents_amd.api import WAVE_CELL_DTYPE, WAVES_SUMMARY, Waves

pytestmark = pytest.mark.gpu

FLOATS = ("freq_hz", "kx", "ky", "celerity", "depth", "quality")


dev_frames = Padded.stack


def dev_image(a, pad):
    return dev_frames([a], pad)[0]


def outputs(w, h, gx, gy, K, pad=0):
    def views(d):
        d["cells"] = d["cells"].view(WAVE_CELL_DTYPE).reshape(gy, gx)
    return Outputs(dict(bin_map=((h, w), torch.uint8), vis=((h, w, 3), torch.uint8)),
                   dict(cells=((gy * gx * 32,), torch.uint8, None), sums=((gy, gx, K, 6), torch.int64, -1), summary=((8,), torch.int64, -1)), pad, views)


def doubtful_cells(want, vis_max_depth):
    """cells whose statement depth is within one unit in the last place of a colour's rounding boundary"""
    d = want["records"]["depth"]
    lo, hi = np.nextafter(d, np.float32(-np.inf)), np.nextafter(d, np.float32(np.inf))
    return (want["records"]["flags"] == 0) & ((R.jet_index(lo, vis_max_depth) != want["index"]) | (R.jet_index(hi, vis_max_depth) != want["index"]))


def compare(got, read, want, case, vis_max_depth, what):
    assert np.array_equal(got["sums"], want["sums"]), "sums differ " + what
    assert np.array_equal(got["summary"], want["summary"]), "summary %s, wanted %s %s" % (got["summary"], want["summary"], what)
    assert np.array_equal(got["bin_map"], want["bin_map"]), "bin map differs " + what
    rec, ref = got["cells"], want["records"]
    assert np.array_equal(rec["bin"], ref["bin"]) and np.array_equal(rec["flags"], ref["flags"]), "bins or flags differ " + what
    for f in FLOATS:
        ulps = np.abs(ordered(rec[f]) - ordered(ref[f]))
        assert ulps.max() <= 1, "%s is %d units in the last place off %s" % (f, ulps.max(), what)
    cx, cy = R.cell_index(case.w, case.h, case.p.grid_x, case.p.grid_y)
    doubt = doubtful_cells(want, vis_max_depth)[cy[:, None], cx[None, :]]
    assert doubt.mean() < 0.01, "the inputs put %.3f of the picture on a boundary %s" % (doubt.mean(), what)
    assert np.array_equal(got["vis"][~doubt], want["vis"][~doubt]), "picture differs " + what
    rcells, rsums, rsumm = read
    assert np.array_equal(rcells.view(np.uint8), rec.view(np.uint8)) and np.array_equal(rsums, want["sums"]), "the slot's copy differs " + what
    assert [rsumm[k] for k in WAVES_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


def run(ctx, name, stream=0, compute_all=False):
    """a case through the device session; compares at every computing push.  -> the device outputs of the last one"""
    case, ref, outs = reference(R, ctx, name)
    p = case.p
    ctx.waves_open(case.w, case.h, stream=stream, **p.kw())
    tc, ts = ctx.waves_table(stream=stream)
    assert np.array_equal(tc, ref.tc) and np.array_equal(ts, ref.ts), "table differs"
    info = ctx.waves_info(stream=stream)
    assert info["shift"] == ref.sh and info["bins"] == len(p.bins)
    frames = dev_frames(case.frames, case.pad)
    mask = None if case.mask is None else dev_image(case.mask, case.pad)
    want = dict(outs)
    vis_max = p.vis_max_depth
    out = outputs(case.w, case.h, p.grid_x, p.grid_y, len(p.bins), case.pad)
    got = None
    check = R.WavesRef(case.w, case.h, p) if len(case.frames) <= 300 else None      # the accumulators after every computing push
    for t, f in enumerate(frames, 1):
        if t in case.sets:
            ctx.waves_set(*case.sets[t], stream=stream)
            vis_max = case.sets[t][2]
        if check is not None:
            check.push(case.frames[t - 1], compute=False)
        if t not in want:
            if compute_all:
                ctx.waves_push(f, mask=mask, stream=stream, **out.kw())
            else:
                ctx.waves_push(f, stream=stream)
            continue
        ctx.waves_push(f, mask=mask, stream=stream, **out.kw())
        got = out.host()
        compare(got, ctx.waves_read(stream=stream), want[t], case, vis_max, "after push %d of %s" % (t, name))
        if check is not None:
            assert np.array_equal(ctx.waves_spectrum(stream=stream), check.acc), "accumulators differ after push %d of %s" % (t, name)
    assert np.array_equal(ctx.waves_spectrum(stream=stream), ref.acc), "accumulators differ at the end of " + name
    assert (frames[0].cpu().numpy() == case.frames[0]).all()
    return got


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(R.cases()))
def test_case_against_the_statement(ctx, name):
    run(ctx, name)
    ctx.waves_close()


def test_result_does_not_depend_on_which_pushes_computed(ctx):
    """one session computes at every push, one at the marked ones only, on two slots: the same bytes at the end"""
    a = run(ctx, "w7", stream=0, compute_all=True)
    b = run(ctx, "w7", stream=1)
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    assert np.array_equal(ctx.waves_spectrum(stream=0), ctx.waves_spectrum(stream=1))
    ctx.waves_close(stream=1)
    ctx.waves_close()


def test_each_output_alone(ctx):
    case, ref, outs = reference(R, ctx, "three-kinds")
    p = case.p
    with Waves(ctx, case.w, case.h, **p.kw()) as wv:
        frames = dev_frames(case.frames[:16], 0)
        for f in frames[:15]:
            wv.push(f)
        assert wv.read()[2] == dict.fromkeys(WAVES_SUMMARY, 0) and wv.info()["held"] == 15
        want = outs[0][1]
        wv.push(frames[15])
        for name in ("cells", "sums", "bin_map", "vis", "summary"):
            o = outputs(case.w, case.h, p.grid_x, p.grid_y, len(p.bins))
            ctx.waves_reset()
            for f in frames[:15]:
                wv.push(f)
            wv.push(frames[15], **{name: o.kw()[name]})
            got = o.host()
            if name == "cells":
                assert np.array_equal(got["cells"]["flags"], want["records"]["flags"]) and np.array_equal(got["cells"]["bin"], want["records"]["bin"])
            elif name == "vis":
                assert np.array_equal(got["vis"], want["vis"])
            else:
                assert np.array_equal(got[name], want[name]), name
            for other in ("bin_map", "vis"):
                if other != name:
                    assert (got[other] == SENTINEL).all(), "%s was written" % other
            if name != "cells":
                assert (o.t["cells"] == SENTINEL).all()
            if name != "summary":
                assert (got["summary"] == -1).all()
            assert [wv.read()[2][k] for k in WAVES_SUMMARY] == [int(v) for v in want["summary"]]


# ---------------------------------------------------------------------------- the profile
def test_profile_books_the_launches(ctx):
    case, ref, outs = reference(R, ctx, "w7")
    p = case.p
    frames = dev_frames(case.frames[:4], 0)
    o = outputs(case.w, case.h, p.grid_x, p.grid_y, len(p.bins))
    ctx.waves_open(case.w, case.h, **p.kw())
    ctx.profile_enable(True)
    ctx.profile_reset()
    read = lambda: {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    ctx.waves_push(frames[0])
    ctx.waves_push(frames[1])
    torch.cuda.synchronize()
    assert read() == {"waves@0": 2}
    ctx.profile_reset()
    ctx.waves_push(frames[2], summary=o.t["summary"])
    torch.cuda.synchronize()
    assert read() == {"waves@0": 1, "waves@1": 1}
    ctx.profile_reset()
    ctx.waves_push(frames[3], **o.kw())
    torch.cuda.synchronize()
    prof = read()
    assert prof == {"waves@0": 1, "waves@1": 1, "waves@2": 1} and sum(prof.values()) == ctx.waves_info()["launches_per_push"] == RC_WAVES_LAUNCHES <= 3
    assert ctx.profile_read_buckets()["overlay"] > 0
    ctx.profile_enable(False)
    ctx.waves_close()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    case, ref0, outs = reference(R, ctx, "w7")
    p, w, h = case.p, case.w, case.h
    good = p.kw()
    gx, gy, K = p.grid_x, p.grid_y, len(p.bins)
    ctx.waves_close()
    for call in (ctx.waves_info, ctx.waves_read, ctx.waves_reset, ctx.waves_spectrum, ctx.waves_table, lambda: ctx.waves_set(0.9, 1, 5.0)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    lib, hdl = raw(ctx)
    assert lib.rcflow_waves_push_dev(hdl, 0, null, 0, null, 0, null, null, null, 0, null, 0, null) == ESTATE
    nan, inf = float("nan"), float("inf")
    for bad in (dict(window=1), dict(window=2, bin_lo=1, bin_hi=1), dict(window=4097), dict(bin_lo=0), dict(bin_lo=4), dict(bin_hi=4),
                dict(window=128, bin_lo=1, bin_hi=17), dict(window=128, bin_lo=60, bin_hi=64), dict(spacing=0), dict(spacing=17),
                dict(grid_x=0), dict(grid_y=0), dict(grid_x=w + 1), dict(grid_y=h + 1), dict(min_pixels=0), dict(fps=0.0), dict(fps=nan),
                dict(fps=inf), dict(metres_per_pixel_x=0.0), dict(metres_per_pixel_y=-1.0), dict(metres_per_pixel_x=nan), dict(gravity=0.0),
                dict(gravity=inf), dict(tanh_max=0.0), dict(tanh_max=1.0), dict(tanh_max=nan), dict(vis_max_depth=0.0), dict(vis_max_depth=inf)):
        with pytest.raises(RcflowError) as e:
            ctx.waves_open(w, h, **dict(good, **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    cp = WavesParams(**dict(good, flags=1))
    assert lib.rcflow_waves_open(hdl, 0, w, h, C.byref(cp)) == EINVAL         # unknown flag bits
    cp.flags = 0
    assert lib.rcflow_waves_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_waves_open(hdl, 0, 0, h, C.byref(cp)) == EINVAL
    assert lib.rcflow_waves_open(hdl, 2, w, h, C.byref(cp)) == EINVAL         # no such slot
    assert lib.rcflow_waves_open(hdl, 0, 8192, 4096, C.byref(cp)) == ESIZE    # a frame beyond the context
    big = dict(good, window=4096, bin_lo=1, bin_hi=16)                        # 3840 x 2160: 34 GB of ring
    assert 3840 * 2160 * (4096 + 128) > RC_WAVES_MAX_STATE_BYTES
    with pytest.raises(RcflowError) as e:
        ctx.waves_open(3840, 2160, **big)
    assert e.value.code == ESIZE
    with pytest.raises(RcflowError):
        ctx.waves_info()                                          # nothing was opened by any of them

    ctx.waves_open(w, h, **good)
    ref = R.WavesRef(w, h, R.Params(**good), ctx.jet_lut())
    frames = dev_frames(case.frames, 0)
    o = outputs(w, h, gx, gy, K)
    for t in range(9):
        ctx.waves_push(frames[t])
        ref.push(case.frames[t], compute=False)
    before, spec = ctx.waves_info(), ctx.waves_spectrum()
    assert before["pushes"] == 9 and before["held"] == 7 and before["device_bytes"] >= 64 * h * (7 + 8) and np.array_equal(spec, ref.acc)
    for bad in (dict(window=1), dict(tanh_max=1.5), dict(grid_x=w + 1)):       # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.waves_open(w, h, **dict(good, **bad))
    with pytest.raises(RcflowError) as e:
        ctx.waves_open(4000, 2160, **good)
    assert e.value.code == ESIZE
    for bad in ((0.0, 1, 5.0), (1.0, 1, 5.0), (0.9, 0, 5.0), (0.9, 1, 0.0), (nan, 1, 5.0), (0.9, 1, nan)):
        with pytest.raises(RcflowError) as e:
            ctx.waves_set(*bad)
        assert e.value.code == EINVAL
    assert ctx.waves_info() == before and np.array_equal(ctx.waves_spectrum(), spec)

    g = frames[9]
    mask = torch.ones((h, w), dtype=torch.uint8, device="cuda")
    buf = torch.zeros(max(3 * w * h, gy * gx * K * 48) + 1024, dtype=torch.uint8, device="cuda")

    def push(gray=None, step=w, msk=(null, 0), cells=null, sums=null, bm=(null, 0), vis=(null, 0), summ=null, slot=0):
        return lib.rcflow_waves_push_dev(hdl, slot, ptr(g) if gray is None else gray, step, msk[0], msk[1], cells, sums, bm[0], bm[1],
                                         vis[0], vis[1], summ)

    refused = [
        push(gray=null), push(step=w - 1), push(msk=(ptr(mask), w - 1)),
        push(cells=ptr(buf, 2)), push(sums=ptr(buf, 4)), push(summ=ptr(buf, 4)), push(bm=(ptr(buf), w - 1)), push(vis=(ptr(buf), 3 * w - 1)),
        push(bm=(ptr(g), w)),                                     # an output over the frame
        push(msk=(ptr(mask), w), vis=(ptr(mask), 3 * w)),         # an output over the mask
        push(cells=ptr(g, 4)), push(msk=(ptr(mask), w), sums=ptr(mask, 8)), push(summ=ptr(g, 8)),
        push(bm=(ptr(buf), w), vis=(ptr(buf, w * (h - 1)), 3 * w)),            # two outputs meeting in one row
        push(cells=ptr(buf), sums=ptr(buf, 8)), push(cells=ptr(buf), summ=ptr(buf, gy * gx * 32 - 8)),
        push(sums=ptr(buf), bm=(ptr(buf, 16), w)), push(vis=(ptr(buf), 3 * w), summ=ptr(buf, 64)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert push(slot=2) == EINVAL                                 # no such slot
    assert ctx.waves_info() == before and np.array_equal(ctx.waves_spectrum(), spec)
    # nothing was queued and nothing changed: the tenth push gives what the statement gives
    ctx.waves_push(g, **o.kw())
    compare(o.host(), ctx.waves_read(), ref.push(case.frames[9]), case, p.vis_max_depth, "(after the refusals)")
    # an accepted boundary: the summary begins at the first byte after the records, in one allocation
    one = torch.full((gy * gx * 32 + 64 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert push(gray=ptr(frames[10]), cells=ptr(one), summ=ptr(one, gy * gx * 32)) == 0
    want = ref.push(case.frames[10])
    assert np.array_equal(one[gy * gx * 32:gy * gx * 32 + 64].cpu().numpy().view(np.int64), want["summary"]) and (one[-8:] == SENTINEL).all()
    # reset empties the ring and the spectrum and keeps the table
    ctx.waves_reset()
    ref.reset()
    assert ctx.waves_info()["pushes"] == 0 and not ctx.waves_spectrum().any() and ctx.waves_read()[2] == dict.fromkeys(WAVES_SUMMARY, 0)
    assert np.array_equal(ctx.waves_table()[0], ref.tc)
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    for k in range(3):
        torch.cuda.synchronize()
        if k % 2:
            with torch.cuda.stream(side):
                ctx.waves_push(frames[k], **o.kw())
                got = ctx.waves_read()
        else:
            ctx.waves_push(frames[k], **o.kw())
            got = ctx.waves_read()
        torch.cuda.synchronize()
        compare(o.host(), got, ref.push(case.frames[k]), case, p.vis_max_depth, "(streams alternating, push %d)" % (k + 1))
    # re-open with other parameters replaces it; the second slot has a state of its own
    run(ctx, "w3")
    assert ctx.waves_info()["window"] == 3
    run(ctx, "s16", stream=1)
    assert ctx.waves_info(stream=1)["spacing"] == 16 and ctx.waves_info()["window"] == 3
    assert lib.rcflow_waves_info(hdl, 0, None) == EINVAL and lib.rcflow_last_error()       # no buffer
    ctx.waves_close(stream=1)
    # a bin above 255 does not fit the bin map's byte: the map is refused, the other outputs are not
    ctx.waves_open(w, h, **dict(good, window=600, bin_lo=255, bin_hi=256))
    o2 = outputs(w, h, gx, gy, 2)
    with pytest.raises(RcflowError) as e:
        ctx.waves_push(frames[0], bin_map=o2.t["bin_map"])
    assert e.value.code == EINVAL and ctx.waves_info()["pushes"] == 0 and not ctx.waves_spectrum().any()
    ctx.waves_push(frames[0], **o2.kw(only=("cells", "sums", "vis", "summary")))
    assert ctx.waves_info()["pushes"] == 1 and o2.host()["summary"][4] == 1 and (o2.host()["bin_map"] == SENTINEL).all()
    ctx.waves_close()
    ctx.waves_close()                                             # closing twice is fine


# ---------------------------------------------------------------------------- the C++ mirror
def test_cpp_waves_against_the_statement(ctx, tmp_path):
    """rc::Waves (include/rcflow_module.hpp) compiled with the flags of tests/cpp's test_module and run on frames it makes itself
    from integers; the summaries, bins, flags and checksums it prints equal the statement's."""
    n = 40
    lines = [l.split() for l in _cpp.run("test_waves", tmp_path, n).splitlines() if l.startswith("push ")]
    case = R.cpp_case(n)
    ref = R.WavesRef(case.w, case.h, case.p, ctx.jet_lut())
    assert len(lines) == n // 5
    k = 0
    for t in range(n):
        want = ref.push(case.frames[t], case.mask, compute=t + 1 in case.compute)
        if want is None:
            continue
        l = [int(s) for s in lines[k][1:]]
        k += 1
        assert l[:8] == [int(s) for s in want["summary"]] and want["summary"][2] > 0, "push %d" % (t + 1)
        assert l[8] == int(ref.acc.sum()) and l[9] == int(want["sums"].sum()) and l[10] == int(want["bin_map"].sum()), "push %d" % (t + 1)
        rec = want["records"].ravel()
        assert l[12::2] == [int(v) for v in rec["bin"]] and l[13::2] == [int(v) for v in rec["flags"]], "push %d" % (t + 1)
        if not doubtful_cells(want, 2.0).any():
            assert l[11] == int(want["vis"].sum()), "push %d" % (t + 1)
