"""The ensemble PIV on the device (piv_kernels.hip) against its numpy statement (tests/_piv_ref.py): the accumulators, the
summary and every integer of the records bit for bit; the records' floats and the field within one unit in the last place; the
picture wherever the statement's magnitude is not within that of a colour's boundary.

On the MI355X every float came out equal to the statement's: no cell of any case differed at all (the count is printed by
compare() and asserted to stay within the one unit the device's double division and square root are allowed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cpp
import _piv_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ordered, ptr, raw, reference
from ripcurrents_amd._lib import RC_PIV_LAUNCHES, RC_PIV_MAX_STATE_BYTES, PivParams, RcflowError
from ripcurrents_amd.api import PIV_CELL_DTYPE, PIV_SUMMARY, Piv

pytestmark = pytest.mark.gpu

FLOATS = ("dx", "dy", "peak", "resid")
dev_frames = Padded.stack


def open_kw(p):
    kw = p.kw()
    kw["replace"] = bool(kw.pop("flags") & R.REPLACE)
    return kw


def outputs(w, h, gx, gy, pad=0):
    def views(d):
        d["cells"] = d["cells"].view(PIV_CELL_DTYPE).reshape(gy, gx)
    return Outputs(dict(vis=((h, w, 3), torch.uint8), field=((gy, gx, 2), torch.float32, -7.0)),
                   dict(cells=((gy * gx * 32,), torch.uint8, None), summary=((8,), torch.int64, -1)), pad, views)


def compare(got, read, want, case, p, what):
    rec, ref = got["cells"], want["records"]
    exc = R.flag_exceptions(want, p)
    assert exc.mean() <= 0.01, "the inputs put %.3f of the cells on a threshold %s" % (exc.mean(), what)
    for f in ("ix", "iy", "pairs"):
        assert np.array_equal(rec[f], ref[f]), "%s differs %s" % (f, what)
    assert np.array_equal(rec["flags"][~exc], ref["flags"][~exc]), "flags differ %s: %s, wanted %s" % (what, rec["flags"], ref["flags"])
    if not exc.any():
        assert np.array_equal(got["summary"], want["summary"]), "summary %s, wanted %s %s" % (got["summary"], want["summary"], what)
    differ = np.zeros(rec.shape, bool)
    for f in FLOATS:
        ulps = np.abs(ordered(rec[f]) - ordered(ref[f]))[~exc]
        differ[~exc] |= ulps > 0
        assert ulps.max(initial=0) <= 1, "%s is %d units in the last place off %s" % (f, ulps.max(), what)
    ulps = np.abs(ordered(got["field"]) - ordered(want["field"]))[~exc]
    assert ulps.max(initial=0) <= 1, "the field is %d units in the last place off %s" % (ulps.max(), what)
    print("%s: %d of %d cells differ in a float" % (what, int(differ.sum()), differ.size))
    doubt = R.doubtful_share(want, case.w, case.h, p)
    assert doubt.mean() < 0.01, "the inputs put %.3f of the picture on a boundary %s" % (doubt.mean(), what)
    if not exc.any():
        assert np.array_equal(got["vis"][~doubt], want["vis"][~doubt]), "picture differs " + what
    rcells, rsumm = read
    assert np.array_equal(rcells.view(np.uint8), rec.view(np.uint8)), "the slot's copy differs " + what
    assert [rsumm[k] for k in PIV_SUMMARY] == [int(v) for v in got["summary"]], "the slot's summary differs " + what


def check_sums(ctx, ref, stream, what):
    sums, cell = ctx.piv_sums(stream=stream)
    assert np.array_equal(sums, ref.T), "accumulators differ " + what
    assert np.array_equal(cell[..., 0], ref.Ta) and np.array_equal(cell[..., 1], ref.Taa), "the cells' own sums differ " + what


def run(ctx, name, stream=0, compute_all=False):
    """a case through the device session; compares at every computing push.  -> the device outputs of the last one"""
    case, ref, outs = reference(R, ctx, name)
    p = case.p
    ctx.piv_open(case.w, case.h, stream=stream, **open_kw(p))
    info = ctx.piv_info(stream=stream)
    assert (info["grid_x"], info["grid_y"]) == (ref.gx, ref.gy) and info["launches_per_push"] == RC_PIV_LAUNCHES
    frames = dev_frames(case.frames, case.pad)
    want = {t: (o, q) for t, o, q in outs}
    out = outputs(case.w, case.h, ref.gx, ref.gy, case.pad)
    check = R.PivRef(case.w, case.h, R.Params(**p.kw()))         # the accumulators after every computing push
    got = None
    for t, f in enumerate(frames, 1):
        if t in case.sets:
            ctx.piv_set(*case.sets[t], stream=stream)
        check.push(case.frames[t - 1], compute=False)
        if t not in want:
            if compute_all:
                ctx.piv_push(f, stream=stream, **out.kw())
            else:
                ctx.piv_push(f, stream=stream)
            continue
        ctx.piv_push(f, stream=stream, **out.kw())
        got = out.host()
        compare(got, ctx.piv_read(stream=stream), want[t][0], case, want[t][1], "after push %d of %s" % (t, name))
        check_sums(ctx, check, stream, "after push %d of %s" % (t, name))
        assert ctx.piv_info(stream=stream)["pairs"] == check.n
    assert (frames[0].cpu().numpy() == case.frames[0]).all()
    return got


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(R.cases()))
def test_case_against_the_statement(ctx, name):
    got = run(ctx, name)
    ctx.piv_close()
    if name in R.RECOVERY:                                         # the bounds of tests/test_piv_ref.py, on the device's records
        (u, v), (bx, by) = R.RECOVERY[name]
        rec = got["cells"]
        assert np.abs(rec["dx"] - u).max() <= bx and np.abs(rec["dy"] - v).max() <= by
        assert abs(rec["dx"].mean() - u) <= 0.05 and abs(rec["dy"].mean() - v) <= 0.05 and not (rec["flags"] & R.EDGE).any()


def test_more_cells_than_one_validating_block(ctx):
    """piv@2 gives a validating block 256 cells, and the launch's last such block adds the blocks' counts up behind the ticket.
    No case of the statement's has more than 256 cells; 46 x 44 under a window of 8, a range of 2 and a step of 2 has 18 x 17 = 306:
    two blocks, 256 and 50 valid cells.  Pushes 2 and 3 compute, and the third finds the ticket and the counters zero"""
    name = "two validating blocks"
    case = R.Case(46, 44, R.Params(8, 2, 2, 1, 0, 0.25, 0.1, 2.0, 2.0), R.drifting_frames(46, 44, 3, 26, [(0, 0), (1, 0), (1, 1)]), {2, 3}, pad=3)
    case, ref, outs = reference(R, ctx, name, case)
    assert ref.gx * ref.gy == 306 and [int(o["summary"][2]) for _, o, _ in outs] == [306, 306]
    run(ctx, name)
    ctx.piv_close()


def test_result_does_not_depend_on_which_pushes_computed(ctx):
    """one session computes at every push, one at the marked ones only (pushes with no output between them), on two slots open
    at once: the same bytes at the end"""
    a = run(ctx, "ring", stream=0, compute_all=True)
    b = run(ctx, "ring", stream=1)
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    for x, y in zip(ctx.piv_sums(stream=0), ctx.piv_sums(stream=1)):
        assert np.array_equal(x, y)
    # the slots do not disturb each other: another case on slot 1 while slot 0 stays as it is
    before = ctx.piv_sums(stream=0)
    run(ctx, "ragged", stream=1)
    assert np.array_equal(ctx.piv_sums(stream=0)[0], before[0]) and ctx.piv_info(stream=0)["window"] == 16
    ctx.piv_close(stream=1)
    ctx.piv_close()


def test_each_output_alone(ctx):
    case, ref, outs = reference(R, ctx, "ragged")
    p = case.p
    want = outs[2][1]                                             # push 3
    with Piv(ctx, case.w, case.h, **open_kw(p)) as pv:
        frames = dev_frames(case.frames[:3], 0)
        for name in ("cells", "field", "vis", "summary"):
            o = outputs(case.w, case.h, ref.gx, ref.gy)
            pv.reset()
            pv.push(frames[0])
            pv.push(frames[1])
            assert pv.read()[1] == dict.fromkeys(PIV_SUMMARY, 0) and pv.info()["pairs"] == 1
            pv.push(frames[2], **{name: o.kw()[name]})
            got = o.host()
            if name == "cells":
                assert np.array_equal(got["cells"]["flags"], want["records"]["flags"]) and np.array_equal(got["cells"]["ix"], want["records"]["ix"])
            elif name == "field":
                assert np.abs(ordered(got["field"]) - ordered(want["field"])).max() <= 1
            else:
                assert np.array_equal(got[name], want[name]), name
            if name != "vis":
                assert (got["vis"] == SENTINEL).all(), "vis was written"
            if name != "field":
                assert (got["field"] == -7.0).all(), "field was written"
            if name != "cells":
                assert (o.t["cells"] == SENTINEL).all()
            if name != "summary":
                assert (got["summary"] == -1).all()
            assert [pv.read()[1][k] for k in PIV_SUMMARY] == [int(v) for v in want["summary"]]


# ---------------------------------------------------------------------------- the profile
def test_profile_books_the_launches(ctx):
    case, ref, outs = reference(R, ctx, "ring")
    frames = dev_frames(case.frames[:4], 0)
    o = outputs(case.w, case.h, ref.gx, ref.gy)
    ctx.piv_open(case.w, case.h, **open_kw(case.p))
    ctx.profile_enable(True)
    ctx.profile_reset()
    read = lambda: {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    ctx.piv_push(frames[0])                                       # the first push only stores its frame: a copy, no launch
    torch.cuda.synchronize()
    assert read() == {}
    ctx.piv_push(frames[1])
    ctx.piv_push(frames[2])
    torch.cuda.synchronize()
    assert read() == {"piv@0": 2}
    ctx.profile_reset()
    ctx.piv_push(frames[3], **o.kw())
    torch.cuda.synchronize()
    prof = read()
    assert prof == {"piv@0": 1, "piv@1": 1, "piv@2": 1} and sum(prof.values()) == ctx.piv_info()["launches_per_push"] == RC_PIV_LAUNCHES == 3
    assert ctx.profile_read_buckets()["farneback"] > 0
    ctx.profile_enable(False)
    ctx.piv_close()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    case, ref0, outs = reference(R, ctx, "ring")
    p, w, h = case.p, case.w, case.h
    good = open_kw(p)
    gx, gy = ref0.gx, ref0.gy
    ctx.piv_close()
    for call in (ctx.piv_info, ctx.piv_read, ctx.piv_reset, ctx.piv_sums, lambda: ctx.piv_set(0.25, 0.1, 2.0, 4.0)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    lib, hdl = raw(ctx)
    assert lib.rcflow_piv_push_dev(hdl, 0, null, 0, null, null, 0, null, 0, null) == ESTATE       # a push before open
    nan, inf = float("nan"), float("inf")
    for bad in (dict(window=6), dict(window=68), dict(window=10), dict(window=4), dict(range=0), dict(range=17), dict(step=0), dict(step=17),
                dict(ensemble=0), dict(ensemble=257), dict(window=64, range=4, step=8, ensemble=65), dict(window=32, ensemble=257),
                dict(min_peak=-0.1), dict(min_peak=1.1), dict(min_peak=nan), dict(median_eps=0.0), dict(median_eps=nan), dict(median_thr=0.0),
                dict(median_thr=inf), dict(vis_max=0.0), dict(vis_max=inf)):
        with pytest.raises(RcflowError) as e:
            ctx.piv_open(w, h, **dict(good, **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    assert 65 * 64 * 64 > 2 ** 18 >= 64 * 64 * 64
    for size in ((23, h), (w, 23), (16, 16)):                     # smaller than one search area of 16 + 2 * 4
        with pytest.raises(RcflowError) as e:
            ctx.piv_open(*size, **good)
        assert e.value.code == EINVAL
    with pytest.raises(RcflowError) as e:                         # 631 x 471 cells
        ctx.piv_open(640, 480, **dict(good, window=8, range=1, step=1))
    assert e.value.code == EINVAL and "cells" in str(e.value)
    cp = PivParams(**dict(p.kw(), flags=2))
    assert lib.rcflow_piv_open(hdl, 0, w, h, C.byref(cp)) == EINVAL           # unknown flag bits
    cp.flags = 0
    assert lib.rcflow_piv_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_piv_open(hdl, 0, 0, h, C.byref(cp)) == EINVAL
    assert lib.rcflow_piv_open(hdl, 2, w, h, C.byref(cp)) == EINVAL           # no such slot
    assert lib.rcflow_piv_open(hdl, 0, 8192, 4096, C.byref(cp)) == ESIZE      # a frame beyond the context
    big = dict(good, window=8, range=16, step=8, ensemble=256)                # 76 x 56 cells of 3269 words: 14 GB of ring
    assert 76 * 56 * (3 * 33 * 33 + 2) * (8 + 4 * 256) > RC_PIV_MAX_STATE_BYTES and 76 * 56 <= R.MAX_CELLS
    with pytest.raises(RcflowError) as e:
        ctx.piv_open(640, 480, **big)
    assert e.value.code == ESIZE
    with pytest.raises(RcflowError):
        ctx.piv_info()                                            # nothing was opened by any of them

    ctx.piv_open(w, h, **good)
    ref = R.PivRef(w, h, R.Params(**p.kw()), ctx.jet_lut())
    frames = dev_frames(case.frames, 0)
    o = outputs(w, h, gx, gy)
    for t in range(5):
        ctx.piv_push(frames[t])
        ref.push(case.frames[t], compute=False)
    before, sums = ctx.piv_info(), ctx.piv_sums()
    assert before["pushes"] == 5 and before["pairs"] == 3 and before["device_bytes"] >= gx * gy * 243 * (8 + 12)
    check_sums(ctx, ref, 0, "(before the refusals)")
    for bad in (dict(window=6), dict(min_peak=2.0), dict(range=17)):           # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.piv_open(w, h, **dict(good, **bad))
    with pytest.raises(RcflowError) as e:
        ctx.piv_open(4000, 2160, **good)
    assert e.value.code == ESIZE
    for bad in ((-0.1, 0.1, 2.0, 4.0), (0.25, 0.0, 2.0, 4.0), (0.25, 0.1, nan, 4.0), (0.25, 0.1, 2.0, 0.0)):
        with pytest.raises(RcflowError) as e:
            ctx.piv_set(*bad)
        assert e.value.code == EINVAL
    assert ctx.piv_info() == before

    g = frames[5]
    buf = torch.zeros(3 * w * h + 1024, dtype=torch.uint8, device="cuda")

    def push(gray=None, step=w, cells=null, field=(null, 0), vis=(null, 0), summ=null, slot=0):
        return lib.rcflow_piv_push_dev(hdl, slot, ptr(g) if gray is None else gray, step, cells, field[0], field[1], vis[0], vis[1], summ)

    refused = [
        push(gray=null), push(step=w - 1),
        push(cells=ptr(buf, 2)), push(field=(ptr(buf, 4), gx * 8)), push(summ=ptr(buf, 4)),        # misaligned
        push(field=(ptr(buf), gx * 8 - 8)), push(field=(ptr(buf), gx * 8 + 4)), push(vis=(ptr(buf), 3 * w - 1)),
        push(vis=(ptr(g), 3 * w)), push(cells=ptr(g, 4)), push(field=(ptr(g, 8), gx * 8)), push(summ=ptr(g, 8)),      # an output over the frame
        push(cells=ptr(buf), field=(ptr(buf, 8), gx * 8)), push(cells=ptr(buf), summ=ptr(buf, gy * gx * 32 - 8)),      # outputs over each other
        push(field=(ptr(buf), gx * 8), vis=(ptr(buf, 16), 3 * w)), push(vis=(ptr(buf), 3 * w), summ=ptr(buf, 64)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert push(slot=2) == EINVAL                                 # no such slot
    assert ctx.piv_info() == before
    check_sums(ctx, ref, 0, "(after the refusals)")
    # nothing was queued and nothing changed: the sixth push gives what the statement gives
    ctx.piv_push(g, **o.kw())
    compare(o.host(), ctx.piv_read(), ref.push(case.frames[5]), case, ref.p, "(after the refusals)")
    # an accepted boundary: the summary begins at the first byte after the records, in one allocation
    one = torch.full((gy * gx * 32 + 64 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert push(gray=ptr(frames[6]), cells=ptr(one), summ=ptr(one, gy * gx * 32)) == 0
    want = ref.push(case.frames[6])
    assert np.array_equal(one[gy * gx * 32:gy * gx * 32 + 64].cpu().numpy().view(np.int64), want["summary"]) and (one[-8:] == SENTINEL).all()
    # set takes effect at the next push, and only there
    ctx.piv_set(0.9, 0.1, 0.5, 1.0)
    ref.p.min_peak, ref.p.median_eps, ref.p.median_thr, ref.p.vis_max = 0.9, 0.1, 0.5, 1.0
    assert np.array_equal(ctx.piv_read()[0]["flags"], want["records"]["flags"])
    ctx.piv_push(frames[0], **o.kw())
    want2 = ref.push(case.frames[0])
    compare(o.host(), ctx.piv_read(), want2, case, ref.p, "(after set)")
    assert not np.array_equal(want2["records"]["flags"] & R.LOWPEAK, want["records"]["flags"] & R.LOWPEAK)
    # after reset the next push is EMPTY, and the ring starts again
    ctx.piv_reset()
    ref.reset()
    assert ctx.piv_info()["pushes"] == 0 and ctx.piv_read()[1] == dict.fromkeys(PIV_SUMMARY, 0) and not ctx.piv_sums()[0].any()
    ctx.piv_push(frames[3], **o.kw())
    got = o.host()
    compare(got, ctx.piv_read(), ref.push(case.frames[3]), case, ref.p, "(after reset)")
    assert (got["cells"]["flags"] == R.EMPTY).all() and got["summary"][0] == 0 and got["summary"][7] == 1 and not got["field"].any()
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    for k in range(4, 7):
        torch.cuda.synchronize()
        if k % 2:
            with torch.cuda.stream(side):
                ctx.piv_push(frames[k], **o.kw())
                got = ctx.piv_read()
        else:
            ctx.piv_push(frames[k], **o.kw())
            got = ctx.piv_read()
        torch.cuda.synchronize()
        compare(o.host(), got, ref.push(case.frames[k]), case, ref.p, "(streams alternating, push %d)" % (k + 1))
    # re-open with other parameters replaces it
    run(ctx, "noise")
    assert ctx.piv_info()["window"] == 12
    assert lib.rcflow_piv_info(hdl, 0, None) == EINVAL and lib.rcflow_last_error()       # no buffer
    ctx.piv_close()
    ctx.piv_close()                                               # closing twice is fine


# ---------------------------------------------------------------------------- the C++ mirror
def test_cpp_piv_against_the_statement(ctx, tmp_path):
    """rc::Piv (include/rcflow_module.hpp) compiled with the flags of tests/cpp's test_module and run on frames it makes itself
    from integers; the summaries, peaks, flags and checksums it prints equal the statement's."""
    n = 12
    lines = [l.split() for l in _cpp.run("test_piv", tmp_path, n).splitlines() if l.startswith("push ")]
    case = R.cpp_case(n)
    ref = R.PivRef(case.w, case.h, case.p, ctx.jet_lut())
    assert len(lines) == n // 3
    k = 0
    for t in range(n):
        want = ref.push(case.frames[t], compute=t + 1 in case.compute)
        if want is None:
            continue
        l = [int(s) for s in lines[k][1:]]
        k += 1
        assert l[:8] == [int(s) for s in want["summary"]] and want["summary"][2] > 0, "push %d" % (t + 1)
        assert l[8] == int(ref.T.sum()) and l[9] == int(ref.Ta.sum() + ref.Taa.sum()), "push %d" % (t + 1)
        rec = want["records"].ravel()
        assert l[11::3] == [int(v) for v in rec["ix"]] and l[12::3] == [int(v) for v in rec["iy"]] and l[13::3] == [int(v) for v in rec["flags"]]
        if not R.doubtful_cells(want, ref.p).any():
            assert l[10] == int(want["vis"].sum()), "push %d" % (t + 1)
