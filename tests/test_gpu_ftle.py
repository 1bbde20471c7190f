"""The flow map and FTLE on the device (ftle_kernels.hip) against their numpy statement (tests/_ftle_ref.py): map, steps, lam
and mask bit for bit, the summary field for field, ftle within one unit in the last place (its logarithm is the device's, in
double, rounded to float once), the picture equal where ftle is and one JET entry off at most elsewhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cpp
import _ftle_ref as F
import _regions_ref as R
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, bits, ordered, ptr, raw
from ripcurrents_amd._lib import RC_FTLE_LAUNCHES, FtleParams, RcflowError
from ripcurrents_amd.api import FTLE_SUMMARY

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = {F.FORWARD: "forward", F.BACKWARD: "backward"}


def outputs(w, h, pad=0):
    f, b = torch.float32, torch.uint8
    return Outputs({"map": ((h, w, 2), f), "steps": ((h, w), torch.int32), "lam": ((h, w), f), "ftle": ((h, w), f), "mask": ((h, w), b),
                    "vis": ((h, w, 3), b)}, dict(summary=((8,), torch.int64, -1)), pad)


def dev_field(f, pad=0):
    return Padded.of(f, pad).view


def compare(got, read, want, lut, what):
    assert np.array_equal(bits(got["map"]), bits(want["map"])), "map differs " + what
    assert np.array_equal(got["steps"], want["steps"]), "steps differ " + what
    assert np.array_equal(bits(got["lam"]), bits(want["lam"])), "lam differs " + what
    assert np.array_equal(got["mask"], want["mask"]), "mask differs " + what
    assert np.array_equal(got["summary"], want["summary"]), "summary %s, wanted %s %s" % (got["summary"], want["summary"], what)
    assert [read[k] for k in FTLE_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what
    same = bits(got["ftle"]) == bits(want["ftle"])
    nan = np.isnan(want["ftle"])
    assert same[nan].all(), "ftle: a NaN of another pattern " + what
    ulp = np.abs(ordered(got["ftle"]) - ordered(want["ftle"]))[~nan]
    print("ftle %s: %d of %d pixels not bit-equal, largest distance %d ulp" % (what, int((~same).sum()), same.size, int(ulp.max()) if ulp.size else 0))
    assert (ulp <= 1).all(), "ftle is %d ulp off %s" % (int(ulp.max()), what)
    assert np.array_equal(got["vis"][same], want["vis"][same]), "picture differs where ftle is equal " + what
    for y, x in zip(*np.nonzero(~same)):
        i = int(want["index"][y, x])
        assert any(np.array_equal(got["vis"][y, x], lut[k]) for k in (max(i - 1, 0), i, min(i + 1, 255))), "picture at (%d, %d) %s" % (x, y, what)


def run(ctx, fields, window, direction, spacing=1, threshold=0.15, vis_max=0.4, dt=1.0, pad=0, stream=0, every=True, reopen=True):
    """Pushes the fields into the device session and the numpy one; compares after every push (or after the last)."""
    h, w = fields[0].shape[:2]
    lut = ctx.jet_lut()
    if reopen:
        ctx.ftle_open(w, h, window=window, direction=NAMES[direction], dt=dt, spacing=spacing, threshold=threshold, vis_max=vis_max, stream=stream)
    ref = F.FtleRef(w, h, lut, window, direction, dt, spacing, threshold, vis_max)
    out = outputs(w, h, pad)
    want = None
    for t, f in enumerate(fields):
        last = t == len(fields) - 1
        if every or last:
            ctx.ftle_push(dev_field(f, pad), stream=stream, **out.kw())
            want = ref.push(f)
            compare(out.host(), ctx.ftle_read(stream=stream), want, lut, "after push %d of %dx%d, window %d, %s, spacing %d" % (
                t + 1, w, h, window, NAMES[direction], spacing))
        else:
            ctx.ftle_push(dev_field(f, pad), stream=stream)
            ref.push(f, compute=False)
    return ref, want


@pytest.fixture(scope="module")
def mixed():
    return F.mixed_fields(131, 70, 6)


def small_fields(w, h, count, seed=3, speed=1.0):
    """the mixed input's recipe at another size"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = []
    for k in range(count):
        u = speed * (0.9 * np.sin(2 * np.pi * y / 23 + 0.3 * k) + 0.004 * (x - w / 2) + 1.1)
        v = speed * (0.9 * np.cos(2 * np.pi * x / 31 - 0.3 * k) - 0.004 * (y - h / 2) - 0.6)
        out.append((np.stack([u, v], -1) + 0.05 * rng.standard_normal((h, w, 2))).astype(f32))
    return out


# ---------------------------------------------------------------------------- warm-up, a full ring, a wrapped ring
@pytest.mark.parametrize("direction", [F.FORWARD, F.BACKWARD])
@pytest.mark.parametrize("window", [1, 2, 5])
def test_every_push_of_a_ragged_size(ctx, window, direction):
    fields = small_fields(67, 45, 2 * window + 3)
    _, want = run(ctx, fields, window, direction, pad=5)
    assert want["n"] == window and want["summary"][1] > 0 and want["summary"][3] > 0
    ctx.ftle_close()


@pytest.mark.parametrize("direction", [F.FORWARD, F.BACKWARD])
@pytest.mark.parametrize("spacing", [1, 3])
def test_the_mixed_input(ctx, mixed, spacing, direction):
    _, want = run(ctx, mixed, 6, direction, spacing=spacing)
    n, valid, nmask, stopped = (int(v) for v in want["summary"][:4])
    assert n == 6 and valid >= 0.6 * 131 * 70 and stopped >= 0.05 * 131 * 70 and 0 < nmask < 0.5 * valid
    ctx.ftle_close()


@pytest.mark.parametrize("w,h,spacing", [(5, 5, 1), (4, 4, 1), (7, 7, 3), (1, 9, 1), (3, 3, 1), (2, 6, 1)])
def test_degenerate_sizes(ctx, w, h, spacing):
    fields = [F.uniform_field(w, h, 0.25, 0.125), F.saddle_field(w, h, 0.05), F.uniform_field(w, h, -0.25, 0.0)]
    for direction in (F.FORWARD, F.BACKWARD):
        _, want = run(ctx, fields, 2, direction, spacing=spacing, pad=1)
        if min(w, h) < 5 or (w, h, spacing) == (7, 7, 3):
            # the sampler needs a 3 x 3 interior to move at all, the stencil a moved particle at every arm
            assert want["summary"][1] == 0 and not want["lam"].any() and not want["mask"].any() and not want["vis"].any()
    ctx.ftle_close()


def test_5x5_has_one_valid_pixel(ctx):
    # slow fields: the particles of (1..3, 1..3) stay inside; only the centre has all four neighbours
    fields = [F.uniform_field(5, 5, 0.25, 0.125)] * 2
    _, want = run(ctx, fields, 2, F.FORWARD)
    assert want["summary"][1] == 1 and want["valid"][2, 2]
    ctx.ftle_close()


@pytest.mark.parametrize("w,h,window", [(640, 480, 8), (1001, 731, 2)])
def test_many_blocks_and_whole_grid_counters(ctx, w, h, window):
    """640 x 480: many blocks, every wave of ftle@2 walking two rows; 1001 x 731: three rows a wave, the last block's ragged."""
    fields = small_fields(w, h, window, seed=11)
    _, want = run(ctx, fields, window, F.BACKWARD, every=False)
    assert want["n"] == window and want["summary"][1] > 0.6 * w * h and want["summary"][3] > 0 and 0 < want["summary"][2]
    ctx.ftle_close()


# ---------------------------------------------------------------------------- bad values
def test_bad_values_in_the_field(ctx, mixed):
    fields = [f.copy() for f in mixed]
    rng = np.random.default_rng(5)
    vals = [np.nan, np.inf, -np.inf, 1e30]
    for k in range(24):
        y, x, c = int(rng.integers(2, 68)), int(rng.integers(2, 129)), int(rng.integers(0, 2))
        fields[k % 6][y, x, c] = vals[k % 4]
    for direction in (F.FORWARD, F.BACKWARD):
        clean = F.FtleRef(131, 70, ctx.jet_lut(), 6, direction)
        for f in mixed:
            cw = clean.push(f)
        _, want = run(ctx, fields, 6, direction, every=False)
        assert np.isfinite(want["map"]).all()                     # and the device's map equals it bit for bit
        assert (want["steps"] < cw["steps"]).any() and (want["steps"] <= cw["steps"]).all()
        untouched = want["steps"] == cw["steps"]
        assert untouched.mean() > 0.9
    ctx.ftle_close()


# ---------------------------------------------------------------------------- the independent pin
def test_forward_map_equals_advect_field(ctx, mixed):
    h, w = 70, 131
    ctx.ftle_open(w, h, window=8, direction="forward", dt=1.0)
    ctx.analysis_reset(w, h)
    m = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    for f in mixed:
        d = dev_field(f)
        ctx.ftle_push(d, map=m)
        ctx.streamline_field(d, 1.0, 1, UPPER=float("inf"))
    pt, _ = ctx.streamline_field_state(w, h)
    assert np.array_equal(bits(m.cpu().numpy()), bits(pt))
    assert ctx.ftle_info()["held"] == 6
    ctx.ftle_close()


# ---------------------------------------------------------------------------- outputs optional
def test_outputs_are_optional_and_launches_counted(ctx, mixed):
    h, w = 70, 131
    lut = ctx.jet_lut()
    ctx.ftle_open(w, h, window=4, direction="backward", threshold=0.15, vis_max=0.4)
    assert ctx.ftle_info()["launches_per_push"] == RC_FTLE_LAUNCHES == 3
    ref = F.FtleRef(w, h, lut, 4, F.BACKWARD, 1.0, 1, 0.15, 0.4)
    assert ctx.ftle_read() == dict(dict.fromkeys(FTLE_SUMMARY, 0), max_lam=0.0)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for f in mixed[:3]:
        ctx.ftle_push(dev_field(f))                               # every output NULL
        ref.push(f, compute=False)
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    assert prof == {"ftle@0": 3}, prof
    assert ctx.ftle_read()["pushes"] == 0                         # no push has computed a summary yet
    ctx.profile_reset()
    only = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    ctx.ftle_push(dev_field(mixed[3]), mask=only)                 # one output is enough
    want = ref.push(mixed[3])
    torch.cuda.synchronize()
    prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
    assert prof == {"ftle@0": 1, "ftle@1": 1, "ftle@2": 1}, prof
    assert ctx.profile_read_buckets()["stream"] > 0
    ctx.profile_enable(False)
    assert np.array_equal(only.cpu().numpy(), want["mask"])
    assert [ctx.ftle_read()[k] for k in FTLE_SUMMARY] == [int(v) for v in want["summary"]]
    out = outputs(w, h)
    ctx.ftle_push(dev_field(mixed[4]), **out.kw())                # does not depend on which earlier pushes computed
    compare(out.host(), ctx.ftle_read(), ref.push(mixed[4]), lut, "(after pushes without outputs)")
    summ = torch.zeros(8, dtype=torch.int64, device="cuda")
    ctx.ftle_push(dev_field(mixed[5]), summary=summ)              # the summary alone
    assert np.array_equal(summ.cpu().numpy(), ref.push(mixed[5])["summary"])
    ctx.ftle_close()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx, mixed):
    h, w = 70, 131
    lut = ctx.jet_lut()
    good = dict(window=3, direction="backward", dt=1.0, spacing=1, threshold=0.15, vis_max=0.4)
    ctx.ftle_close()
    for call in (ctx.ftle_info, ctx.ftle_read, ctx.ftle_reset, lambda: ctx.ftle_set(0.1, 0.5)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE and str(e.value).split(": ", 1)[1]
    lib, hdl = raw(ctx)
    assert lib.rcflow_ftle_push_dev(hdl, 0, null, 0, null, 0, null, 0, null, 0, null, 0, null, 0, null, 0, null) == ESTATE
    for bad in (dict(window=0), dict(window=257), dict(direction=2), dict(direction=-1), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")),
                dict(dt=float("nan")), dict(spacing=0), dict(spacing=17), dict(threshold=float("nan")), dict(threshold=float("inf")),
                dict(vis_max=0.0), dict(vis_max=-1.0), dict(vis_max=float("nan")), dict(vis_max=float("inf"))):
        with pytest.raises(RcflowError) as e:
            ctx.ftle_open(w, h, **dict(good, **bad))
        assert e.value.code == EINVAL and str(e.value).split(": ", 1)[1], bad
    p = FtleParams(window=3, direction=1, dt=1.0, spacing=1, threshold=0.15, vis_max=0.4, flags=1)
    assert lib.rcflow_ftle_open(hdl, 0, w, h, C.byref(p)) == EINVAL           # unknown flag bits
    p.flags = 0
    assert lib.rcflow_ftle_open(hdl, 0, w, h, None) == EINVAL
    assert lib.rcflow_ftle_open(hdl, 0, 0, h, C.byref(p)) == EINVAL
    assert lib.rcflow_ftle_open(hdl, 0, 8192, 4096, C.byref(p)) == ESIZE      # beyond the context
    p.window = 256
    assert lib.rcflow_ftle_open(hdl, 0, 3840, 2160, C.byref(p)) == ESIZE      # a ring of 17 GB
    assert lib.rcflow_ftle_open(hdl, 2, w, h, C.byref(p)) == EINVAL           # no such slot
    with pytest.raises(RcflowError):
        ctx.ftle_info()                                           # nothing was opened by any of them

    ref, _ = run(ctx, mixed[:2], **dict(good, direction=F.BACKWARD))
    info = ctx.ftle_info()
    assert (info["w"], info["h"], info["window"], info["direction"], info["spacing"], info["held"], info["pushes"]) == (w, h, 3, "backward", 1, 2, 2)
    assert info["device_bytes"] >= 3 * 132 * 70 * 8 + w * h * 16 and info["launches_per_push"] == 3
    before = info
    for bad in (dict(window=0), dict(vis_max=0.0)):               # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.ftle_open(w, h, **dict(good, **bad))
    with pytest.raises(RcflowError) as e:
        ctx.ftle_open(4000, 2160, **good)
    assert e.value.code == ESIZE and ctx.ftle_info() == before

    d = dev_field(mixed[2])
    o = outputs(w, h)
    big = torch.zeros(h * w * 8 + 256, dtype=torch.uint8, device="cuda")

    def push(flow=None, step=8 * w, map=(null, 0), steps=(null, 0), lam=(null, 0), ftle=(null, 0), mask=(null, 0), vis=(null, 0), summ=null, slot=0):
        fp = ptr(d) if flow is None else flow
        return lib.rcflow_ftle_push_dev(hdl, slot, fp, step, map[0], map[1], steps[0], steps[1], lam[0], lam[1], ftle[0], ftle[1], mask[0], mask[1],
                                        vis[0], vis[1], summ)

    refused = [
        push(flow=null), push(step=8 * w - 8), push(step=8 * w + 4), push(flow=ptr(d, 4)),
        push(map=(ptr(big), 8 * w - 8)), push(map=(ptr(big), 8 * w + 4)), push(map=(ptr(big, 4), 8 * w)),
        push(steps=(ptr(big), 4 * w - 4)), push(steps=(ptr(big), 4 * w + 2)), push(steps=(ptr(big, 2), 4 * w)),
        push(lam=(ptr(big), 4 * w - 4)), push(lam=(ptr(big, 1), 4 * w)), push(ftle=(ptr(big), 4 * w + 2)), push(ftle=(ptr(big, 2), 4 * w)),
        push(mask=(ptr(big), w - 1)), push(vis=(ptr(big), 3 * w - 1)), push(summ=ptr(big, 4)),
        push(mask=(ptr(d), w)),                                   # an output over the field
        push(flow=ptr(big, 16), lam=(ptr(big), 4 * w)),           # the field inside an output
        push(lam=(ptr(big), 4 * w), ftle=(ptr(big, 4 * w * (h - 1)), 4 * w)),      # two outputs meeting in one row
        push(map=(ptr(big), 8 * w), mask=(ptr(big, 8 * w * h - 1), w)),
        push(steps=(ptr(big), 4 * w), vis=(ptr(big, 64), 3 * w)),
        push(vis=(ptr(big), 3 * w), summ=ptr(big, 8)), push(mask=(ptr(big), w), summ=ptr(big, 0)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert lib.rcflow_last_error()
    assert push(slot=2) == EINVAL                                 # no such slot
    for bad in ((float("nan"), 0.4), (0.1, 0.0), (0.1, float("inf"))):
        with pytest.raises(RcflowError) as e:
            ctx.ftle_set(*bad)
        assert e.value.code == EINVAL
    assert ctx.ftle_info() == before
    # nothing was queued and nothing changed: the third push gives what the statement gives
    ctx.ftle_push(d, **o.kw())
    compare(o.host(), ctx.ftle_read(), ref.push(mixed[2]), lut, "(after the refusals)")
    # set takes effect on the next push
    ctx.ftle_set(0.05, 0.2)
    ref.threshold, ref.vis_max = 0.05, 0.2
    i2 = ctx.ftle_info()
    assert (i2["threshold"], i2["vis_max"]) == (0.05, 0.2)
    ctx.ftle_push(dev_field(mixed[3]), **o.kw())
    w4 = ref.push(mixed[3])
    compare(o.host(), ctx.ftle_read(), w4, lut, "(after set)")
    # an accepted boundary: the mask begins at the first byte after lam's range, in one allocation
    one = torch.full((5 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tl, tm = one[:4 * h * w].view(torch.float32).view(h, w), one[4 * h * w:5 * h * w].view(h, w)
    ctx.ftle_push(dev_field(mixed[4]), lam=tl, mask=tm)
    w5 = ref.push(mixed[4])
    assert np.array_equal(bits(tl.cpu().numpy()), bits(w5["lam"])) and np.array_equal(tm.cpu().numpy(), w5["mask"]) and (one[5 * h * w:] == SENTINEL).all()
    # reset equals a fresh open
    ctx.ftle_reset()
    assert ctx.ftle_info()["pushes"] == 0 and ctx.ftle_info()["held"] == 0 and ctx.ftle_read()["pushes"] == 0
    run(ctx, mixed[3:], reopen=False, **dict(good, direction=F.BACKWARD, threshold=0.05, vis_max=0.2))
    # a slot moved to another stream after open, and between pushes
    ctx.ftle_reset()
    ref.reset()
    side = torch.cuda.Stream()
    for k, f in enumerate(mixed[:4]):
        torch.cuda.synchronize()
        if k % 2:
            with torch.cuda.stream(side):
                ctx.ftle_push(dev_field(f), **o.kw())
                got = ctx.ftle_read()
        else:
            ctx.ftle_push(dev_field(f), **o.kw())
            got = ctx.ftle_read()
        torch.cuda.synchronize()
        compare(o.host(), got, ref.push(f), lut, "(streams alternating, push %d)" % (k + 1))
    # re-open with another size replaces it
    run(ctx, small_fields(64, 48, 3), 2, F.FORWARD)
    assert ctx.ftle_info()["w"] == 64
    ctx.ftle_close()
    ctx.ftle_close()                                              # closing twice is fine


def test_two_slots_on_two_streams(ctx, mixed):
    lut = ctx.jet_lut()
    fb = small_fields(67, 45, 4)
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.ftle_open(131, 70, window=3, direction="backward", threshold=0.15, vis_max=0.4, stream=0)
    ctx.ftle_open(67, 45, window=2, direction="forward", spacing=2, threshold=0.1, vis_max=0.3, stream=1)
    ra, rb = F.FtleRef(131, 70, lut, 3, F.BACKWARD, 1.0, 1, 0.15, 0.4), F.FtleRef(67, 45, lut, 2, F.FORWARD, 1.0, 2, 0.1, 0.3)
    oa, ob = outputs(131, 70), outputs(67, 45)
    torch.cuda.synchronize()                                      # the outputs were filled on the default stream
    for a, b in zip(mixed, fb):
        da, db = dev_field(a), dev_field(b)
        torch.cuda.synchronize()
        with torch.cuda.stream(s0):
            ctx.ftle_push(da, stream=0, **oa.kw())
        with torch.cuda.stream(s1):
            ctx.ftle_push(db, stream=1, **ob.kw())
        with torch.cuda.stream(s0):
            r0 = ctx.ftle_read(stream=0)
        with torch.cuda.stream(s1):
            r1 = ctx.ftle_read(stream=1)
        torch.cuda.synchronize()
        compare(oa.host(), r0, ra.push(a), lut, "(slot 0)")
        compare(ob.host(), r1, rb.push(b), lut, "(slot 1)")
    ctx.ftle_close(stream=0)
    ctx.ftle_close(stream=1)


# ---------------------------------------------------------------------------- the chain
def test_mask_goes_straight_into_regions(ctx, mixed):
    h, w = 70, 131
    ctx.ftle_open(w, h, window=6, direction="backward", threshold=0.15, vis_max=0.4)
    ctx.regions_open(w, h, connectivity=8, min_area=4, max_regions=256)
    ref = F.FtleRef(w, h, ctx.jet_lut(), 6, F.BACKWARD, 1.0, 1, 0.15, 0.4)
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    for k, f in enumerate(mixed):
        d = dev_field(f)
        ctx.ftle_push(d, mask=mask)
        ctx.regions_push(mask, flow=d)                            # the same stream: no host round trip in between
        want = ref.push(f)
    rec, summ = ctx.regions_read()
    wr = R.regions(want["mask"], 8, 4, 256, mixed[-1], len(mixed))
    assert summ["kept"] == int(wr["summary"][1]) > 0
    assert np.array_equal(rec["area"], wr["records"]["area"][:len(rec)]) and np.array_equal(rec["label"], wr["records"]["label"][:len(rec)])
    ctx.regions_close()
    ctx.ftle_close()


# ---------------------------------------------------------------------------- the C++ mirror
def test_cpp_ftle_against_the_statement(ctx, tmp_path):
    """rc::Ftle (include/rcflow_module.hpp) compiled with the flags of tests/cpp's test_module and run on fields it makes
    itself from integers (exact in float, so this file makes the same ones); the summaries it prints equal the statement's."""
    n = 7
    lines = [l.split() for l in _cpp.run("test_ftle", tmp_path, n).splitlines() if l.startswith("push ")]
    assert len(lines) == n
    w, h = 67, 45
    ref = F.FtleRef(w, h, ctx.jet_lut(), 4, F.BACKWARD, 1.0, 2, 0.05, 0.25)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for t, l in enumerate(lines):
        u = ((x * 7 + y * 3 + t * 5) % 32 - 12).astype(f32) / f32(16)
        v = ((x * 5 + y * 11 + t * 3) % 32 - 18).astype(f32) / f32(16)
        want = ref.push(np.stack([u, v], -1))
        assert [int(s) for s in l[1:9]] == [int(s) for s in want["summary"]], "push %d" % (t + 1)
        assert int(l[9]) == int((want["mask"] != 0).sum()) and int(l[10]) == int(want["vis"].any(-1).sum()), "push %d" % (t + 1)
