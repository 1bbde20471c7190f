"""The motion templates on the device (motion_kernels.hip) against their numpy statement (tests/_motion_ref.py), after every
push: history, orientation, mask and picture bit for bit; every cell's and the frame's record field for field (the angle is
a double computed from equal integers by the stated operations, so it is equal too); the silhouette's pixel count."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cpp
import _motion_ref as M
import _tracers_ref as TR
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ptr, raw, same_bits
from ripcurrents_amd._lib import RC_MOTION_LAUNCHES, MotionParams, RcflowError
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, MOTION_CELL_DTYPE

pytestmark = pytest.mark.gpu

f32 = np.float32
BAR = dict(diff_threshold=30, duration=8, delta1=0.5, delta2=2.5)
TEX = dict(diff_threshold=12, duration=6, delta1=0.5, delta2=2.5)


def views(d):
    d["cells"], d["frame"] = d["cells"].view(MOTION_CELL_DTYPE), d["frame"].view(MOTION_CELL_DTYPE)[0]


def outputs(w, h, grid, pad=0):
    return Outputs(dict(mhi=((h, w), torch.float32), orient=((h, w), torch.float32), mask=((h, w), torch.uint8), vis=((h, w, 3), torch.uint8)),
                   dict(cells=((grid[0] * grid[1] * 40,), torch.uint8, 0), frame=((40,), torch.uint8, 0)), pad, views)


def records_equal(got, want, what):
    got, want = np.atleast_1d(got).ravel(), np.atleast_1d(want).ravel()
    assert got.shape == want.shape, what
    for k in ("S", "W", "n_masked", "n_used", "peak_bin"):
        assert np.array_equal(got[k], want[k]), "%s differs %s" % (k, what)
    assert same_bits(got["tsmax"], want["tsmax"]), "tsmax differs " + what
    assert np.array_equal(got["angle"].view(np.uint64), want["angle"].view(np.uint64)), "angle differs " + what


def compare(read, out, want, what):
    if out is not None:
        assert same_bits(out["mhi"], want["mhi"]), "history differs " + what
        assert np.array_equal(out["mask"], want["mask"]), "mask differs " + what
        assert same_bits(out["orient"], want["orient"]), "orientation differs " + what
        assert np.array_equal(out["vis"], want["vis"]), "picture differs " + what
        records_equal(out["cells"], read["cells"], "(caller's cells against the slot's) " + what)
        records_equal(out["frame"], read["frame"], "(caller's frame against the slot's) " + what)
    records_equal(read["cells"], want["cells"], "in the cells " + what)
    records_equal(read["frame"], want["frame"], "in the frame " + what)
    assert read["silhouette"] == want["silhouette"], "silhouette count differs " + what


def dev_frame(f, pad=0):
    return Padded.of(f, pad).view


def run(ctx, orc, frames, prm, grid=(1, 1), stamps=None, pad=0, stream=0, reopen=True, fresh=False):
    """Pushes the frames into the device session and the numpy one; compares after every push."""
    h, w = frames[0].shape
    if reopen:
        ctx.motion_open(w, h, grid=grid, fresh=fresh, stream=stream, **prm)
    ref = M.MotionRef(w, h, orc.fast_atan2_deg, grid=grid, fresh=fresh, **prm)
    out = outputs(w, h, grid, pad)
    want = None
    for t, f in enumerate(frames):
        ts = None if stamps is None else stamps[t]
        ctx.motion_push(dev_frame(f, pad), timestamp=ts, stream=stream, **out.kw())
        want = ref.push(f, ts)
        compare(ctx.motion_read(stream=stream), out.host(), want, "after push %d of %dx%d" % (t + 1, w, h))
    return ref, want


# ---------------------------------------------------------------------------- the clips of the CPU tier
@pytest.mark.parametrize("direction,angle", [("+x", 0.0), ("-x", 180.0), ("+y", 90.0), ("-y", 270.0)])
def test_bars(ctx, orc, direction, angle):
    _, want = run(ctx, orc, M.bar_clip(direction, n=12), BAR, grid=(3, 2))
    assert want["angle"] == angle and ctx.motion_read()["angle"] == angle
    ctx.motion_close()


def test_texture(ctx, orc):
    _, want = run(ctx, orc, M.texture_clip(97, 61, 12), TEX, grid=(7, 5))
    assert want["frame"]["n_used"] > 500
    ctx.motion_close()


# ---------------------------------------------------------------------------- sizes at which the tiling can go wrong
@pytest.mark.parametrize("w,h,grid,pad", [(5, 3, (1, 1), 0), (33, 31, (30, 30), 0), (130, 9, (4, 2), 0), (97, 61, (7, 5), 3),
                                          (640, 480, (21, 16), 0)])
def test_sizes(ctx, orc, w, h, grid, pad):
    _, want = run(ctx, orc, M.texture_clip(w, h, 4), TEX, grid=grid, pad=pad)
    assert want["silhouette"] > 0 and (w * h < 1000 or want["frame"]["n_used"] > 0)
    ctx.motion_close()


def test_1080p(ctx, orc):
    _, want = run(ctx, orc, M.texture_clip(1920, 1080, 2), TEX, grid=(30, 30))
    assert want["frame"]["n_used"] > 100000
    ctx.motion_close()


def test_float_stamps_exercise_the_sobel_order(ctx, orc):
    frames = M.texture_clip(97, 61, 10)
    _, want = run(ctx, orc, frames, dict(diff_threshold=12, duration=2.0, delta1=0.1, delta2=1.0), grid=(7, 5),
                  stamps=[0.37 * (k + 1) for k in range(len(frames))])
    assert want["frame"]["n_used"] > 100
    ctx.motion_close()


def test_duration_expiry_returns_to_zero(ctx, orc):
    frames = M.bar_clip("+x", n=5)
    frames += [frames[-1]] * 5                                  # the bar stands still from push 5
    _, want = run(ctx, orc, frames, dict(BAR, duration=3), grid=(3, 2))
    got = ctx.motion_read()
    assert not want["mhi"].any() and not want["mask"].any()
    assert got["angle"] == 0.0 and got["frame"]["W"] == 0 and not got["cells"]["W"].any() and got["silhouette"] == 0
    ctx.motion_close()


# ---------------------------------------------------------------------------- the reference's literal call
def test_fresh_equals_global_orientation_and_a_reopened_session(ctx, orc):
    w, h = 97, 61
    frames = M.texture_clip(w, h, 4, step=2)
    prm = dict(diff_threshold=30, duration=1.0, delta1=0.25, delta2=1.0)        # the reference's numbers
    ctx.motion_open(w, h, grid=(1, 1), fresh=True, **prm)
    out = outputs(w, h, (1, 1))
    ctx.motion_push(dev_frame(frames[0]))
    for a, b in zip(frames, frames[1:]):
        ctx.motion_push(dev_frame(b), **out.kw())
        fresh, fread = out.host(), ctx.motion_read()
        ref = M.MotionRef(w, h, orc.fast_atan2_deg, fresh=True, **prm)
        ref.push(a)
        compare(fread, fresh, ref.push(b), "(fresh)")
        assert set(np.unique(fresh["vis"])) <= {0, 255} and set(np.unique(fresh["mhi"])) <= {f32(0), f32(1)}
        # a session with a history, re-opened before the pair, stamps 0 and 1
        ctx.motion_open(w, h, grid=(1, 1), stream=1, **prm)
        out2 = outputs(w, h, (1, 1))
        ctx.motion_push(dev_frame(a), timestamp=0.0, stream=1)
        ctx.motion_push(dev_frame(b), timestamp=1.0, stream=1, **out2.kw())
        again, aread = out2.host(), ctx.motion_read(stream=1)
        for k in ("mhi", "orient", "mask", "vis"):
            assert np.array_equal(fresh[k], again[k]), k
        records_equal(fread["frame"], aread["frame"], "(fresh against re-opened)")
    ctx.motion_close(stream=1)
    # the one-line call: stream 1 has nothing open, stream 0 holds the fresh session of this size
    for stream in (1, 0):
        angle, vis = ctx.globalOrientation(frames[-2], frames[-1], stream=stream)
        assert angle == fread["angle"] and np.array_equal(vis.cpu().numpy(), fresh["vis"])
        assert ctx.motion_info(stream=stream)["fresh"]
        ctx.motion_close(stream=stream)


# ---------------------------------------------------------------------------- the state and its lifecycle
def test_null_outputs_still_advance_the_state(ctx, orc):
    frames = M.texture_clip(97, 61, 6)
    ctx.motion_open(97, 61, grid=(7, 5), **TEX)
    ref = M.MotionRef(97, 61, orc.fast_atan2_deg, grid=(7, 5), **TEX)
    for f in frames[:5]:
        ctx.motion_push(dev_frame(f))                           # every output pointer NULL
        want = ref.push(f)
        compare(ctx.motion_read(), None, want, "(no outputs)")
    out = outputs(97, 61, (7, 5))
    ctx.motion_push(dev_frame(frames[5]), **out.kw())
    compare(ctx.motion_read(), out.host(), ref.push(frames[5]), "(outputs after five pushes without)")
    ctx.motion_close()


def test_reset_equals_a_fresh_open(ctx, orc):
    frames = M.texture_clip(97, 61, 8)
    run(ctx, orc, frames[:4], TEX, grid=(7, 5))
    ctx.motion_reset()
    info = ctx.motion_info()
    assert info["pushes"] == 0 and info["last_timestamp"] == 0.0
    z = ctx.motion_read()
    assert z["silhouette"] == 0 and not z["cells"]["W"].any() and not z["cells"]["n_masked"].any() and z["frame"]["tsmax"] == 0
    run(ctx, orc, frames[4:], TEX, grid=(7, 5), reopen=False)   # stamps start at 1 again, no previous frame is held
    ctx.motion_close()


def test_reopen_replaces_and_a_refused_reopen_keeps_the_state(ctx, orc):
    frames = M.texture_clip(97, 61, 6)
    ref, _ = run(ctx, orc, frames[:3], TEX, grid=(7, 5))
    before = ctx.motion_info()
    for bad in (dict(diff_threshold=256), dict(duration=0.0), dict(grid=(98, 5)), dict(delta1=float("nan"))):
        with pytest.raises(RcflowError) as e:
            ctx.motion_open(97, 61, **dict(dict(TEX, grid=(7, 5)), **bad))
        assert e.value.code == EINVAL
    with pytest.raises(RcflowError) as e:
        ctx.motion_open(4000, 2160, **TEX)
    assert e.value.code == ESIZE
    assert ctx.motion_info() == before
    out = outputs(97, 61, (7, 5))
    ctx.motion_push(dev_frame(frames[3]), **out.kw())           # the old state still works, and continues
    compare(ctx.motion_read(), out.host(), ref.push(frames[3]), "(after refused re-opens)")
    run(ctx, orc, M.texture_clip(64, 48, 3), TEX, grid=(2, 2))  # another size replaces it
    assert ctx.motion_info()["w"] == 64
    ctx.motion_close()
    ctx.motion_close()                                          # closing twice is fine


def test_two_slots_on_two_streams(ctx, orc):
    fa, fb = M.texture_clip(97, 61, 5), M.bar_clip("+y", n=5)
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.motion_open(97, 61, grid=(7, 5), stream=0, **TEX)
    ctx.motion_open(67, 45, grid=(3, 2), stream=1, **BAR)
    ra = M.MotionRef(97, 61, orc.fast_atan2_deg, grid=(7, 5), **TEX)
    rb = M.MotionRef(67, 45, orc.fast_atan2_deg, grid=(3, 2), **BAR)
    oa, ob = outputs(97, 61, (7, 5)), outputs(67, 45, (3, 2))
    torch.cuda.synchronize()                                    # the outputs were filled on the default stream
    for a, b in zip(fa, fb):
        with torch.cuda.stream(s0):
            ctx.motion_push(dev_frame(a), stream=0, **oa.kw())
        with torch.cuda.stream(s1):
            ctx.motion_push(dev_frame(b), stream=1, **ob.kw())
        with torch.cuda.stream(s0):
            r0 = ctx.motion_read(stream=0)
        with torch.cuda.stream(s1):
            r1 = ctx.motion_read(stream=1)
        torch.cuda.synchronize()
        compare(r0, oa.host(), ra.push(a), "(slot 0)")
        compare(r1, ob.host(), rb.push(b), "(slot 1)")
    ctx.motion_close(stream=0)
    ctx.motion_close(stream=1)


# ---------------------------------------------------------------------------- refusals
def test_every_refusal_returns_its_code_and_queues_nothing(ctx, orc):
    w, h = 97, 61
    for call in (ctx.motion_info, ctx.motion_read, ctx.motion_reset, ctx.motion_prims, lambda: ctx.motion_push(dev_frame(np.zeros((h, w), np.uint8)))):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    for bad in (dict(diff_threshold=-1), dict(duration=float("inf")), dict(delta2=-1.0), dict(grid=(0, 1)), dict(grid=(7, 62)), dict(w=640, h=480, grid=(200, 100))):      # the last: beyond RC_RIPMAP_MAX_CELLS cells
        with pytest.raises(RcflowError) as e:
            ctx.motion_open(**dict(dict(TEX, w=w, h=h), **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    lib, hdl = raw(ctx)
    p = MotionParams(diff_threshold=12, duration=6.0, delta1=0.5, delta2=2.5, grid_x=1, grid_y=1, flags=2)
    assert lib.rcflow_motion_open(hdl, 0, w, h, C.byref(p)) == EINVAL             # unknown flag bits
    assert lib.rcflow_motion_open(hdl, 0, w, h, None) == EINVAL
    p.flags = 0
    assert lib.rcflow_motion_open(hdl, 0, 8192, 4096, C.byref(p)) == ESIZE
    with pytest.raises(RcflowError):
        ctx.motion_info()                                       # nothing was opened by any of them

    frames = M.texture_clip(w, h, 4)
    ref, _ = run(ctx, orc, frames[:2], TEX, grid=(7, 5), stamps=[1.0, 2.0])
    g = dev_frame(frames[2])
    out = outputs(w, h, (7, 5))

    def push(gray=None, step=w, ts=3.0, mhi=(null, 0), orient=(null, 0), mask=(null, 0), vis=(null, 0), cells=null, frame=null):
        gp = ptr(g) if gray is None else gray
        return lib.rcflow_motion_push_dev(hdl, 0, gp, step, ts, mhi[0], mhi[1], orient[0], orient[1], mask[0], mask[1], vis[0], vis[1], cells, frame)

    big = torch.zeros(h * w * 4 + 64, dtype=torch.uint8, device="cuda")
    refused = [
        push(ts=2.0), push(ts=1.5), push(ts=float("nan")), push(ts=float("inf")), push(ts=-2.0), push(ts=2.0 ** 24 + 2),   # the timestamp rules
        push(gray=null), push(step=w - 1),
        push(mhi=(ptr(big), 4 * w - 4)), push(mhi=(ptr(big), 4 * w + 2)), push(mhi=(ptr(big, 2), 4 * w)),
        push(orient=(ptr(big), 4 * w - 4)), push(orient=(ptr(big, 1), 4 * w)),
        push(mask=(ptr(big), w - 1)), push(vis=(ptr(big), 3 * w - 1)),
        push(cells=ptr(big, 4)), push(frame=ptr(big, 4)),
        push(mask=(ptr(g), w)),                                   # an output over the frame
        push(gray=ptr(big, 16), mhi=(ptr(big), 4 * w)),           # the frame inside an output
        push(mhi=(ptr(big), 4 * w), orient=(ptr(big, 4 * w * (h - 1)), 4 * w)),      # two outputs meeting in one row
        push(mhi=(ptr(big), 4 * w), cells=ptr(big, 8)), push(cells=ptr(big), frame=ptr(big, 32)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert lib.rcflow_motion_push_dev(hdl, 2, ptr(g), w, 3.0, null, 0, null, 0, null, 0, null, 0, null, null) == EINVAL   # no such slot
    for bad in (dict(thickness=0), dict(thickness=9), dict(disc_radius=-1), dict(length=float("nan")), dict(length=1e6)):
        with pytest.raises(RcflowError) as e:
            ctx.motion_prims(**bad)
        assert e.value.code == EINVAL
    info = ctx.motion_info()
    assert info["pushes"] == 2 and info["last_timestamp"] == 2.0
    # nothing was queued and nothing changed: the third push gives what the statement gives
    ctx.motion_push(g, timestamp=3.0, **out.kw())
    compare(ctx.motion_read(), out.host(), ref.push(frames[2], 3.0), "(after the refusals)")
    # an accepted boundary: the mask begins at the first byte after the frame's range, in one allocation
    one = torch.full((2 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tg, tm = one[:h * w].view(h, w), one[h * w:2 * h * w].view(h, w)
    assert tm.data_ptr() == tg.data_ptr() + (h - 1) * tg.stride(0) + w
    tg.copy_(dev_frame(frames[3]))
    ctx.motion_push(tg, timestamp=4.0, mask=tm)
    touching, want4 = ctx.motion_read(), ref.push(frames[3], 4.0)
    compare(touching, None, want4, "(the mask right after the frame)")
    assert np.array_equal(tm.cpu().numpy(), want4["mask"]) and np.array_equal(tg.cpu().numpy(), frames[3]) and (one[2 * h * w:] == SENTINEL).all()
    ctx.motion_open(w, h, grid=(7, 5), stream=1, **TEX)         # the same four pushes with separate allocations, on the other slot
    sep = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    for t in range(4):
        ctx.motion_push(dev_frame(frames[t]), timestamp=t + 1.0, mask=sep, stream=1)
    apart = ctx.motion_read(stream=1)
    ctx.motion_close(stream=1)
    assert np.array_equal(tm.cpu().numpy(), sep.cpu().numpy()) and touching["silhouette"] == apart["silhouette"]
    records_equal(touching["cells"], apart["cells"], "(touching against separate allocations)")
    records_equal(touching["frame"], apart["frame"], "(touching against separate allocations)")
    ctx.motion_push(dev_frame(frames[3]), timestamp=2.0 ** 24)      # the largest stamp
    with pytest.raises(RcflowError) as e:
        ctx.motion_push(g)                                      # automatic: pushes + 1 = 6 is not greater
    assert e.value.code == EINVAL
    ctx.motion_close()


def test_deltas_are_swapped(ctx, orc):
    frames = M.texture_clip(97, 61, 4)
    ctx.motion_open(97, 61, grid=(7, 5), **dict(TEX, delta1=2.5, delta2=0.5))
    info = ctx.motion_info()
    assert (info["delta1"], info["delta2"]) == (0.5, 2.5)
    run(ctx, orc, frames, TEX, grid=(7, 5), reopen=False)
    ctx.motion_close()


# ---------------------------------------------------------------------------- profile, launches, drawing
def test_profile_and_launch_count(ctx):
    frames = [dev_frame(f) for f in M.texture_clip(320, 240, 4)]
    ctx.motion_open(320, 240, grid=(10, 8), **TEX)
    assert ctx.motion_info()["launches_per_push"] == RC_MOTION_LAUNCHES <= 3
    out = outputs(320, 240, (10, 8))
    ctx.profile_enable(True)
    ctx.profile_reset()
    for k, f in enumerate(frames):
        ctx.motion_push(f, **(out.kw() if k % 2 else {}))
    ctx.motion_prims()
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    assert prof == {"motion@0": 4, "motion@1": 4, "motion@2": 4, "motion@3": 1}, prof
    assert ctx.profile_read_buckets()["farneback"] > 0
    ctx.profile_enable(False)
    ctx.motion_close()


def test_primitives_and_drawing(ctx, orc):
    w, h, grid = 97, 61, (3, 2)
    _, want = run(ctx, orc, M.texture_clip(w, h, 5), TEX, grid=grid)
    got = ctx.motion_read()
    prims = ctx.motion_prims(color=0x20c0ff, thickness=2, disc_radius=3, length=12.0)
    p = prims.cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE)
    wp = M.prims(want["cells"], want["frame"], w, h, 0x20c0ff, 2, 3, 12.0)
    assert len(p) == 2 * (grid[0] * grid[1] + 1) == len(wp)
    names = DRAW_PRIM_DTYPE.names
    for i, (a, b) in enumerate(zip(p, wp)):
        for k, name in enumerate(names):
            tol = 1 if name in ("x1", "y1") and a["kind"] == 2 else 0        # cos and sin are the device's: a line's far end is good to one pixel
            assert abs(int(a[name]) - int(b[k])) <= tol, (i, name, a, b)
    assert got["cells"]["W"].all() and got["frame"]["W"]         # every set has a direction: nothing to skip
    vis = torch.as_tensor(want["vis"]).cuda()
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.draw(vis, prims, skipped=skipped)
    canvas = want["vis"].copy()
    nskip = TR.draw(canvas, p.astype(TR.PRIM))
    assert nskip == 0 and int(skipped.item()) == 0
    assert np.array_equal(vis.cpu().numpy(), canvas) and (canvas != want["vis"]).any()
    # a set without a direction gives two records of kind 0
    ctx.motion_reset()
    z = ctx.motion_prims().cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE)
    assert not z["kind"].any()
    ctx.motion_close()


# ---------------------------------------------------------------------------- the C++ mirror
def test_cpp_motion_against_the_statement(ctx, orc, tmp_path):
    """rc::MotionTemplates (include/rcflow_module.hpp) compiled with the flags of tests/cpp's test_module and run on the +x bar;
    the records it prints equal the numpy statement's, and the angle is 0."""
    n = 12
    stdout = _cpp.run("test_motion", tmp_path, n)
    lines = [l.split() for l in stdout.splitlines() if l.startswith("push ")]
    assert len(lines) == n
    ref = M.MotionRef(67, 45, orc.fast_atan2_deg, grid=(3, 2), **BAR)
    for t, (l, f) in enumerate(zip(lines, M.bar_clip("+x", n=n))):
        want = ref.push(f)
        fr = want["frame"]
        assert int(l[1]) == t + 1 and float(l[2]) == fr["angle"]
        assert [int(v) for v in l[3:]] == [fr["S"], fr["W"], fr["n_masked"], fr["n_used"], fr["peak_bin"], want["silhouette"],
                                           int((want["vis"][..., 0] != 0).sum())], "push %d" % (t + 1)
    assert [l for l in stdout.splitlines() if l.startswith("angle ")] == ["angle 0"]
