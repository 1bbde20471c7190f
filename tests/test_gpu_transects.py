"""The transects on the device (transects_kernels.hip) against their numpy statement (tests/_transects_ref.py): the table, the
grey ring (through the time stack), the accumulators, the Q sums, the jets, the pictures, the summary and every integer of the
records bit for bit; the records' floats and the profile equal or within one unit in the last place, the count printed by
compare() (the waves convention)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _transects_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ptr, raw, reference, ulps
from ripcurrents_amd._lib import RC_TRANSECTS_LAUNCHES, RC_TRANSECTS_MAX_STATE_BYTES, RcflowError, TransectLine, TransectsParams
from ripcurrents_amd.api import TRANSECT_DTYPE, TRANSECTS_SUMMARY, Transects

pytestmark = pytest.mark.gpu

def dev_frames(frames, pad, fill):
    """all frames of a case in one upload, rows `pad` pixels longer than the frame and `fill` there"""
    return None if frames is None else Padded.stack(frames, pad, fill)


def views(d):
    d["records"], d["sums"], d["profile"] = d["records"].view(TRANSECT_DTYPE), d["sums"].reshape(-1, 16), d["profile"].reshape(-1, 2)


def outputs(L, S, T, gray, flow, pad=0):
    """the time stack only where there are grey frames, the Hovmoeller picture only where there is flow"""
    planes = dict(stack=((T, S), torch.uint8)) if gray else {}
    if flow:
        planes["hov"] = ((T, S, 3), torch.uint8)
    return Outputs(planes, dict(records=((L * 64,), torch.uint8, None), sums=((L * 16,), torch.int64, -1), profile=((S * 2,), torch.float32, -7.0),
                                summary=((8,), torch.int64, -1)), pad, views)


def compare(got, read, want, what):
    rec, ref = got["records"], want["records"]
    for f in R.INTS:
        assert np.array_equal(rec[f], ref[f]), "%s differs %s: %s, wanted %s" % (f, what, rec[f], ref[f])
    assert np.array_equal(got["sums"], want["sums"]), "sums differ " + what
    assert np.array_equal(got["summary"], want["summary"]), "summary %s, wanted %s %s" % (got["summary"], want["summary"], what)
    differ = 0
    for f in R.FLOATS:
        u = ulps(rec[f], ref[f])
        differ += int((u > 0).sum())
        assert u.max() <= 1, "%s is %d units in the last place off %s" % (f, u.max(), what)
    u = ulps(got["profile"], want["profile"])
    assert u.max() <= 1, "the profile is %d units in the last place off %s" % (u.max(), what)
    print("%s: %d record floats and %d of %d profile floats differ" % (what, differ, int((u > 0).sum()), u.size))
    for k in ("stack", "hov"):
        assert (k in got) == (k in want)
        if k in got:
            assert np.array_equal(got[k], want[k]), "%s differs %s" % (k, what)
    rrec, rsumm = read
    assert rrec.tobytes() == rec.tobytes(), "the slot's copy differs " + what
    assert [rsumm[k] for k in TRANSECTS_SUMMARY] == [int(v) for v in got["summary"]], "the slot's summary differs " + what


def check_sums(ctx, ref, stream, what):
    sums, line = ctx.transects_sums(stream=stream)
    assert np.array_equal(sums, ref.T), "accumulators differ " + what
    assert np.array_equal(line, ref.Ta), "the lines' own sums differ " + what


def run(ctx, name, stream=0, compute_all=True):
    """a case through the device session; compares at every computing push.  -> the device outputs of the last one"""
    case, _, outs = reference(R, ctx, name)
    p = case.p
    ctx.transects_open(case.w, case.h, case.lines, stream=stream, **p.kw())
    info = ctx.transects_info(stream=stream)
    check = R.TransectsRef(case.w, case.h, case.lines, p)         # the accumulators after every push
    assert (info["lines"], info["samples"], info["launches_per_push"]) == (check.L, check.S, RC_TRANSECTS_LAUNCHES)
    table, geom = ctx.transects_table(stream=stream)
    assert table.tobytes() == check.table.tobytes() and geom.tobytes() == check.geom.tobytes()
    gray, flow = dev_frames(case.gray, case.pad, SENTINEL), dev_frames(case.flow, case.pad, 3.0)
    out = outputs(check.L, check.S, p.window, gray is not None, flow is not None, case.pad)
    got = None
    for t in range(len(outs)):
        g, f = gray[t] if gray else None, flow[t] if flow else None
        check.push(case.gray[t] if gray else None, case.flow[t] if flow else None, compute=False)
        if not compute_all and t + 1 not in case.compute:
            ctx.transects_push(g, f, stream=stream)
            continue
        ctx.transects_push(g, f, stream=stream, **out.kw())
        got = out.host()
        what = "after push %d of %s" % (t + 1, name)
        compare(got, ctx.transects_read(stream=stream), outs[t], what)
        check_sums(ctx, check, stream, what)
        info = ctx.transects_info(stream=stream)
        assert (info["pairs"], info["held"], info["pushes"]) == (check.pairs(), min(t + 1, p.window), t + 1)
    return got


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(R.cases()))
def test_case_against_the_statement(ctx, name):
    got = run(ctx, name)
    ctx.transects_close()
    case, ref, outs = reference(R, ctx, name)
    flags = [o["records"]["flags"] for o in outs]
    if name == "three":                                           # the first lag pushes are EMPTY; bad samples and jets occur
        assert all((f == R.EMPTY).all() for f in flags[:case.p.lag]) and not (flags[-1] & R.EMPTY).any()
        assert outs[-1]["summary"][5] > 0 and outs[-1]["summary"][4] > 0 and len(outs) > 2 * case.p.window
        assert ref.S % 2 == 1 and sorted(ref.geom["n"]) == [2 * case.p.range + 8, 37, 50]
    if name == "long":
        assert (flags[-1] == 0).all() and outs[-1]["records"]["peak_shift"][0] == 3 and outs[-1]["records"]["pairs"][0] == 1
    if name == "flat":
        assert (flags[0] == R.EMPTY).all() and all((f == R.FLAT).all() for f in flags[1:])
    if name in ("flow", "nocorr"):
        assert all((f == R.EMPTY).all() for f in flags)


def test_the_flow_ring_holds_the_statements_samples(ctx):
    """the first push's window mean is its row of the ring: (ut, un) of every sample, NaN and infinities included"""
    case, ref, outs = reference(R, ctx, "three")
    with Transects(ctx, case.w, case.h, lines=case.lines, **case.p.kw()) as ts:
        o = outputs(ref.L, ref.S, case.p.window, True, True)
        ts.push(dev_frames(case.gray[:1], 0, 0)[0], dev_frames(case.flow[:1], 0, 0.0)[0], profile=o.t["profile"])
        row = R.TransectsRef(case.w, case.h, case.lines, case.p).sample_flow(case.flow[0])
        u = ulps(o.host()["profile"], row)
        print("%d of %d ring floats differ" % (int((u > 0).sum()), u.size))
        # an infinity times a zero component of the tangent is NaN; 1e30 stays finite and huge
        assert u.max() <= 1 and np.isnan(row).sum() >= 4 and (np.nan_to_num(np.abs(row), nan=0.0) > 2.0 ** 20).any()


def test_result_does_not_depend_on_which_pushes_computed(ctx):
    """one session computes at every push, one at every k-th (pushes with no output between them), on two slots open at once:
    the same bytes at the end"""
    a = run(ctx, "three", stream=0, compute_all=True)
    b = run(ctx, "three", stream=1, compute_all=False)
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
    for x, y in zip(ctx.transects_sums(stream=0), ctx.transects_sums(stream=1)):
        assert np.array_equal(x, y)
    before = ctx.transects_sums(stream=0)
    run(ctx, "flat", stream=1)                                    # the slots do not disturb each other
    assert np.array_equal(ctx.transects_sums(stream=0)[0], before[0]) and ctx.transects_info(stream=0)["window"] == 5
    ctx.transects_close(stream=1)
    ctx.transects_close()


def test_each_output_alone(ctx):
    case, ref, outs = reference(R, ctx, "three")
    want = outs[2]
    gray, flow = dev_frames(case.gray[:3], 0, 0), dev_frames(case.flow[:3], 0, 0.0)
    with Transects(ctx, case.w, case.h, lines=case.lines, **case.p.kw()) as ts:
        for name in ("records", "sums", "profile", "stack", "hov", "summary"):
            o = outputs(ref.L, ref.S, case.p.window, True, True)
            ts.reset()
            ts.push(gray[0], flow[0])
            ts.push(gray[1], flow[1])
            assert ts.read()[1] == dict.fromkeys(TRANSECTS_SUMMARY, 0) and ts.info()["held"] == 2
            ts.push(gray[2], flow[2], **{name: o.kw()[name]})
            got = o.host()
            if name == "records":
                assert all(np.array_equal(got[name][f], want[name][f]) for f in R.INTS)
            elif name == "profile":
                assert ulps(got[name], want[name]).max() <= 1
            else:
                assert np.array_equal(got[name], want[name]), name
            for other in ("stack", "hov"):
                if other != name:
                    assert (got[other] == SENTINEL).all(), other + " was written"
            if name != "records":
                assert (o.t["records"] == SENTINEL).all()
            if name != "sums":
                assert (o.t["sums"] == -1).all()
            if name != "profile":
                assert (o.t["profile"] == -7.0).all()
            if name != "summary":
                assert (o.t["summary"] == -1).all()
            if name in ("stack", "hov"):
                assert ts.read()[1] == dict.fromkeys(TRANSECTS_SUMMARY, 0)       # a picture alone computes no records
            else:
                assert [ts.read()[1][k] for k in TRANSECTS_SUMMARY] == [int(v) for v in want["summary"]]


def test_python_class_holds_its_arguments_to_the_session(ctx):
    """Transects.push refuses tensors that are not what was opened before the library sees them, and changes nothing"""
    w, h, lines = 64, 48, [(2.0, 20.0, 61.0, 20.0, 60)]
    with Transects(ctx, w, h, lines=lines, window=3, range=3) as ts:
        g, f = torch.zeros((h, w), dtype=torch.uint8, device="cuda"), torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
        stack = torch.zeros((3, 60), dtype=torch.uint8, device="cuda")
        for kw in (dict(gray=g.cpu(), flow=f), dict(gray=g.float(), flow=f), dict(gray=g[:, :-1], flow=f), dict(gray=g, flow=f[..., :1]),
                   dict(gray=g, flow=f.double()), dict(gray=g, flow=f, stack=stack[:2]), dict(gray=g, flow=f, stack=stack.t().contiguous().t()),
                   dict(gray=g, flow=f, records=torch.zeros(63, dtype=torch.uint8, device="cuda")),
                   dict(gray=g, flow=f, summary=torch.zeros(8, dtype=torch.int32, device="cuda")),
                   dict(gray=g, flow=f, profile=torch.zeros(120, dtype=torch.float32))):
            with pytest.raises(ValueError):
                ts.push(**kw)
        assert ts.info()["pushes"] == 0
        ts.push(g, f, stack=stack)
        assert ts.info()["pushes"] == 1 and ts.table()[1]["n"][0] == 60 and ts.sums()[0].shape == (1, 7, 3)
        with pytest.raises(ValueError):
            ctx.transects_open(w, h, [(2.0, 20.0, 61.0, 20.0)])
        with pytest.raises(ValueError):
            ctx.transects_open(w, h, [])
        assert ts.info()["pushes"] == 1


# ---------------------------------------------------------------------------- the profile
def test_profile_books_the_launches(ctx):
    case, ref, outs = reference(R, ctx, "three")
    gray, flow = dev_frames(case.gray[:4], 0, 0), dev_frames(case.flow[:4], 0, 0.0)
    o = outputs(ref.L, ref.S, case.p.window, True, True)
    ctx.transects_open(case.w, case.h, case.lines, **case.p.kw())
    ctx.profile_enable(True)
    ctx.profile_reset()
    read = lambda: {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    for t in range(3):
        ctx.transects_push(gray[t], flow[t])                      # no output: one launch, nothing else
    torch.cuda.synchronize()
    assert read() == {"transects@0": 3}
    ctx.profile_reset()
    ctx.transects_push(gray[3], flow[3], summary=o.t["summary"])
    torch.cuda.synchronize()
    assert read() == {"transects@0": 1, "transects@1": 1}
    ctx.profile_reset()
    ctx.transects_push(gray[0], flow[0], **o.kw())
    torch.cuda.synchronize()
    prof = read()
    assert prof == {"transects@0": 1, "transects@1": 1, "transects@2": 1}
    assert sum(prof.values()) == ctx.transects_info()["launches_per_push"] == RC_TRANSECTS_LAUNCHES == 3
    assert ctx.profile_read_buckets()["stream"] > 0
    ctx.profile_enable(False)
    ctx.transects_close()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    case, ref0, outs = reference(R, ctx, "three")
    p, w, h, lines = case.p, case.w, case.h, case.lines
    good = p.kw()
    L, S, T = ref0.L, ref0.S, p.window
    ctx.transects_close()
    for call in (ctx.transects_info, ctx.transects_read, ctx.transects_reset, ctx.transects_sums, ctx.transects_table,
                 lambda: ctx.transects_set(0.25, 2.0)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    lib, hdl = raw(ctx)
    assert lib.rcflow_transects_push_dev(hdl, 0, null, 0, null, 0, null, null, null, null, 0, null, 0, null) == ESTATE       # a push before open
    nan, inf = float("nan"), float("inf")
    for bad in (dict(window=1), dict(window=4097), dict(gray=False, flow=False), dict(lag=0), dict(lag=9), dict(range=-1), dict(range=17),
                dict(range=5), dict(gray=False), dict(window=2, lag=2), dict(fps=0.0), dict(fps=nan), dict(metres_per_pixel=inf),
                dict(jet_min=0.0), dict(jet_min=nan), dict(jet_min=2.0 ** 20), dict(jet_min=1e20), dict(vis_max=0.0), dict(vis_max=inf)):
        with pytest.raises(RcflowError) as e:
            ctx.transects_open(w, h, lines, **dict(good, **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    for bad_lines in ([(3.0, 60.0, 96.0, 60.0, 20)], [(3.0, 60.0, 3.0, 60.0, 20)], lines + [(0.0, 0.0, 9.0, 9.0, 1)], [lines[0]] * 65):
        with pytest.raises(RcflowError) as e:
            ctx.transects_open(w, h, bad_lines, **good)
        assert e.value.code == EINVAL
    cp = TransectsParams(window=5, sources=3, lag=2, range=4, flags=1, pad=0, fps=25.0, metres_per_pixel=0.5, jet_min=3.0, vis_max=20.0)
    arr = (TransectLine * L)(*[TransectLine(*l) for l in lines])
    assert lib.rcflow_transects_open(hdl, 0, w, h, arr, L, C.byref(cp)) == EINVAL          # unknown flag bits
    cp.flags = 0
    assert lib.rcflow_transects_open(hdl, 0, w, h, arr, L, None) == EINVAL
    assert lib.rcflow_transects_open(hdl, 0, w, h, None, L, C.byref(cp)) == EINVAL
    assert lib.rcflow_transects_open(hdl, 0, 0, h, arr, L, C.byref(cp)) == EINVAL
    assert lib.rcflow_transects_open(hdl, 2, w, h, arr, L, C.byref(cp)) == EINVAL          # no such slot
    assert lib.rcflow_transects_open(hdl, 0, 8192, 4096, arr, L, C.byref(cp)) == ESIZE     # a frame beyond the context
    big = [(0.0, float(k), 1023.0, float(k), 1024) for k in range(64)]                     # 65536 samples, 2048 rows of 9 bytes
    assert 65536 * 2048 * 8 <= RC_TRANSECTS_MAX_STATE_BYTES < 65536 * 2048 * 9
    with pytest.raises(RcflowError) as e:
        ctx.transects_open(1024, 64, big, **dict(good, window=2048, range=0))
    assert e.value.code == ESIZE
    with pytest.raises(RcflowError):
        ctx.transects_info()                                      # nothing was opened by any of them

    ctx.transects_open(w, h, lines, **good)
    ref = R.TransectsRef(w, h, lines, R.Params(**R.asdict(p)), ctx.jet_lut())
    gray, flow = dev_frames(case.gray, 0, 0), dev_frames(case.flow, 0, 0.0)
    o = outputs(L, S, T, True, True)
    for t in range(7):
        ctx.transects_push(gray[t], flow[t])
        ref.push(case.gray[t], case.flow[t], compute=False)
    before = ctx.transects_info()
    assert before["pushes"] == 7 and before["pairs"] == 3 and before["held"] == 5 and before["device_bytes"] >= T * S * 9
    check_sums(ctx, ref, 0, "(before the refusals)")
    for bad in (dict(window=1), dict(range=17), dict(jet_min=-1.0)):                       # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.transects_open(w, h, lines, **dict(good, **bad))
    with pytest.raises(RcflowError) as e:
        ctx.transects_open(4000, 2161, lines, **good)
    assert e.value.code == ESIZE
    for bad in ((0.0, 2.0), (nan, 2.0), (2.0 ** 20, 2.0), (1e20, 2.0), (0.25, inf), (0.25, -1.0)):
        with pytest.raises(RcflowError) as e:
            ctx.transects_set(*bad)
        assert e.value.code == EINVAL
    assert ctx.transects_info() == before

    g, f = gray[7], flow[7]
    buf = torch.zeros(4 * T * S + 4096, dtype=torch.uint8, device="cuda")

    def push(gr=(ptr(g), w), fl=(ptr(f), 8 * w), rec=null, sums=null, prof=null, stack=(null, 0), hov=(null, 0), summ=null, slot=0):
        return lib.rcflow_transects_push_dev(hdl, slot, gr[0], gr[1], fl[0], fl[1], rec, sums, prof, stack[0], stack[1], hov[0], hov[1], summ)

    refused = [
        push(gr=(null, 0)), push(fl=(null, 0)), push(gr=(ptr(g), w - 1)), push(fl=(ptr(f), 8 * w - 8)), push(fl=(ptr(f), 8 * w + 4)),
        push(fl=(ptr(f, 4), 8 * w)),
        push(rec=ptr(buf, 2)), push(sums=ptr(buf, 4)), push(prof=ptr(buf, 4)), push(summ=ptr(buf, 4)),                # misaligned
        push(stack=(ptr(buf), S - 1)), push(hov=(ptr(buf), 3 * S - 1)),
        push(rec=ptr(g, 4)), push(stack=(ptr(f, 8), S)), push(hov=(ptr(g), 3 * S)), push(summ=ptr(f, 8)),            # an output over an input
        push(rec=ptr(buf), sums=ptr(buf, 64 * L - 8)), push(rec=ptr(buf), summ=ptr(buf, 8)),                          # outputs over each other
        push(stack=(ptr(buf), S), hov=(ptr(buf, 16), 3 * S)), push(prof=ptr(buf), stack=(ptr(buf, 8 * S - 1), S)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert push(slot=2) == EINVAL                                 # no such slot
    assert ctx.transects_info() == before
    check_sums(ctx, ref, 0, "(after the refusals)")
    # nothing was queued and nothing changed: the eighth push gives what the statement gives
    ctx.transects_push(g, f, **o.kw())
    compare(o.host(), ctx.transects_read(), ref.push(case.gray[7], case.flow[7]), "(after the refusals)")
    # an accepted boundary: the summary begins at the first byte after the records, in one allocation
    one = torch.full((L * 64 + 64 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert push(gr=(ptr(gray[8]), w), fl=(ptr(flow[8]), 8 * w), rec=ptr(one), summ=ptr(one, L * 64)) == 0
    want = ref.push(case.gray[8], case.flow[8])
    assert np.array_equal(one[L * 64:L * 64 + 64].cpu().numpy().view(np.int64), want["summary"]) and (one[-8:] == SENTINEL).all()
    # set takes effect at the next push, and only there
    ctx.transects_set(1.0, 5.0)
    ref.p.jet_min, ref.p.vis_max = 1.0, 5.0
    assert np.array_equal(ctx.transects_read()[0]["jets"], want["records"]["jets"])
    ctx.transects_push(gray[9], flow[9], **o.kw())
    want2 = ref.push(case.gray[9], case.flow[9])
    compare(o.host(), ctx.transects_read(), want2, "(after set)")
    assert want2["summary"][4] != want["summary"][4] and ctx.transects_info()["jet_min"] == 1.0
    # after reset the next push is the first again
    ctx.transects_reset()
    ref.reset()
    assert ctx.transects_info()["pushes"] == 0 and ctx.transects_read()[1] == dict.fromkeys(TRANSECTS_SUMMARY, 0) and not ctx.transects_sums()[0].any()
    # a slot moved to another stream between reset and push, and between pushes
    side = torch.cuda.Stream()
    for k in range(4):
        torch.cuda.synchronize()
        if k % 2 == 0:
            with torch.cuda.stream(side):
                ctx.transects_push(gray[k], flow[k], **o.kw())
                got = ctx.transects_read()
        else:
            ctx.transects_push(gray[k], flow[k], **o.kw())
            got = ctx.transects_read()
        torch.cuda.synchronize()
        want = ref.push(case.gray[k], case.flow[k])
        compare(o.host(), got, want, "(streams alternating, push %d)" % (k + 1))
        if k == 0:
            assert (want["records"]["flags"] == R.EMPTY).all() and want["summary"][0] == 1 and not want["stack"][1:].any()
    # a session opened for one source refuses the other and the picture made from it
    run(ctx, "long")                                              # re-open with other parameters replaces it
    assert ctx.transects_info()["window"] == 2 and not ctx.transects_info()["flow"]
    big_g, big_f = torch.zeros((12, 1100), dtype=torch.uint8, device="cuda"), torch.zeros((12, 1100, 2), dtype=torch.float32, device="cuda")
    hov = torch.zeros((2, 1024, 3), dtype=torch.uint8, device="cuda")
    for kw in (dict(gray=big_g, flow=big_f), dict(flow=big_f), dict(), dict(gray=big_g, hov=hov)):
        with pytest.raises(RcflowError) as e:
            ctx.transects_push(**kw)
        assert e.value.code == EINVAL
    assert lib.rcflow_transects_info(hdl, 0, None) == EINVAL and lib.rcflow_last_error()   # no buffer
    ctx.transects_close()
    ctx.transects_close()                                         # closing twice is fine
