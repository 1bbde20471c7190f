"""Rip regions on the device (region_kernels.hip) against the numpy statement (tests/_regions_ref.py): every output byte of
every case -- labels, the opened mask, the integer fields of every record, the summary, the primitives -- is compared with
np.array_equal; the derived doubles within 1e-6 * max(1, |b|), the angle only where the two variances differ by more than
1e-3 of the larger.  Outputs sit between fence bytes in rows with poisoned padding; nothing is sampled."""
import numpy as np
import pytest
import torch

import _cpp
import _regions_ref as R
import _tracers_ref as TR
from _dev import EINVAL, ESIZE, ESTATE, SENTINEL, Fenced
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RC_REGIONS_LAUNCHES, RcflowError
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, REGION_DTYPE

pytestmark = pytest.mark.gpu


def compare_records(got, want, what):
    assert got.dtype == REGION_DTYPE and len(got) == len(want), what
    for k in R.INT_FIELDS:
        assert np.array_equal(got[k], want[k]), "%s: field %s differs" % (what, k)
    live = want["label"] > 0
    for k in R.FLOAT_FIELDS:
        a, b = got[k].astype(np.float64), want[k].astype(np.float64)
        sel = live & (want["var_major"] - want["var_minor"] > 1e-3 * want["var_major"]) if k == "angle" else live
        assert (np.abs(a[sel] - b[sel]) <= 1e-6 * np.maximum(1.0, np.abs(b[sel]))).all(), "%s: derived field %s" % (what, k)
        assert (a[~live] == 0).all(), what
    assert not got.view(np.uint8).reshape(len(got), REGION_DTYPE.itemsize)[~live].any(), "%s: bytes beyond the written records are not zero" % what


def push_and_check(ctx, mask, conn, min_area=1, max_regions=256, flow=None, pad=0, lead=0, inplace=False, labels=True, stream=0, opened=False,
                   pushes=1, prims=True, what=""):
    """one push with every output between fences; returns the statement's result"""
    h, w = mask.shape
    what = "%s %dx%d conn %d min_area %d max %d" % (what, w, h, conn, min_area, max_regions)
    if not opened:
        ctx.regions_open(w, h, conn, min_area, max_regions, stream=stream)
    want = R.regions(mask, conn, min_area, max_regions, flow, pushes)
    dm = Fenced(h, w, torch.uint8, pad, lead, mask)
    df = Fenced(h, 2 * w, torch.float32, 2 * pad, 2 * (lead % 2), flow) if flow is not None else None
    dl = Fenced(h, w, torch.int32, pad, lead) if labels else None
    do = dm if inplace else Fenced(h, w, torch.uint8, pad + 3, lead + 1)
    dr = Fenced(1, max_regions * 144, torch.uint8, 0, 8)
    ds = Fenced(1, 8, torch.int64, 0, 1)
    ctx.regions_push(dm.view, flow=None if df is None else torch.as_strided(df.view, (h, w, 2), (df.step, 2, 1), df.view.storage_offset()),
                     labels=None if dl is None else dl.view, mask_out=do.view, regions=dr.view.reshape(-1), summary=ds.view.reshape(-1),
                     stream=stream)
    got_sum = ds.numpy().reshape(-1)
    assert np.array_equal(got_sum, want["summary"]), "%s: summary %s, expected %s" % (what, got_sum, want["summary"])
    if labels:
        got = dl.numpy()
        assert np.array_equal(got, want["labels"]), "%s: %d label pixels differ" % (what, int((got != want["labels"]).sum()))
        dl.check("labels")
    assert np.array_equal(do.numpy(), want["mask_out"]), "%s: the opened mask differs" % what
    do.check("mask_out")
    if not inplace:
        assert np.array_equal(dm.numpy(), mask), "%s: the input mask changed" % what
        dm.check("mask")
    dr.check("regions")
    ds.check("summary")
    compare_records(dr.numpy().reshape(-1).view(REGION_DTYPE), want["records"], what)
    rec, summ = ctx.regions_read(stream=stream)
    nrec = int(want["summary"][2])
    assert len(rec) == nrec and list(summ.values()) == want["summary"].tolist(), what
    compare_records(rec, want["records"][:nrec], what + " (read)")
    if prims:
        dp = Fenced(1, 6 * max_regions * 32, torch.uint8, 0, 4)
        ctx.regions_prims(0x20c0ff, 2, 3, 1.5, out=dp.view.reshape(-1), stream=stream)
        gp = dp.numpy().reshape(-1).view(DRAW_PRIM_DTYPE)
        assert np.array_equal(gp, R.prims(want["records"], 0x20c0ff, 2, 3, 1.5).astype(DRAW_PRIM_DTYPE)), "%s: primitives differ" % what
        dp.check("prims")
    return want


# ---------------------------------------------------------------------------- masks
def spiral(h, w):
    """a one-pixel path that winds inward from the corner, its arms one pixel apart: one component, long merge chains"""
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 255

    def free(y, x, dy, dx):
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < h and 0 <= nx < w) or m[ny, nx]:
            return False
        return not (0 <= ay < h and 0 <= ax < w and m[ay, ax])

    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy                                  # turn right (y runs down)
            if not free(y, x, dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = 255


def comb(h, w):
    """teeth in every other column hanging on a spine along the bottom row: one component that closes in the last row"""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 255
    m[h - 1, :] = 255
    return m


def rings(h, w):
    m = np.zeros((h, w), np.uint8)
    k = 0
    while 2 * k < min(h, w):
        m[k, k:w - k] = m[h - 1 - k, k:w - k] = 255
        m[k:h - k, k] = m[k:h - k, w - 1 - k] = 255
        k += 2
    return m


def smooth_noise(h, w, seed, thresh=0.55):
    """thresholded low-pass noise: a few hundred to a few thousand blobs"""
    rng = np.random.RandomState(seed)
    f = np.fft.rfft2(rng.rand(h, w).astype(np.float32))
    ky, kx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    g = np.fft.irfft2(f * np.exp(-(kx * kx + ky * ky) * (2 * np.pi * 6.0) ** 2 / 2), (h, w))
    g = (g - g.min()) / (g.max() - g.min())
    return np.where(g > np.quantile(g, thresh), 255, 0).astype(np.uint8)


def field(h, w, seed=0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack([2.5 * np.sin(x / 31.0 + seed) + 1.5, 2.0 * np.cos(y / 27.0 - seed) - 0.5 + x / 100.0], -1).astype(np.float32)


def stress_masks(h, w):
    rng = np.random.RandomState(h * 1000 + w)
    yield "empty", np.zeros((h, w), np.uint8)
    yield "full", np.full((h, w), 255, np.uint8)
    yield "checkerboard", ((np.indices((h, w)).sum(0) % 2) == 0).astype(np.uint8) * 255
    yield "spiral", spiral(h, w)
    yield "comb", comb(h, w)
    yield "rings", rings(h, w)
    for d in (0.1, 0.5, 0.593, 0.9):
        yield "random %.3f" % d, (rng.rand(h, w) < d).astype(np.uint8) * 255


SIZES = [(1, 1), (257, 1), (1, 257), (5, 7), (16, 64), (17, 65), (80, 96), (480, 640)]       # (h, w)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("h,w", SIZES)
def test_stress_patterns(ctx, h, w, conn):
    for i, (name, m) in enumerate(stress_masks(h, w)):
        want = push_and_check(ctx, m, conn, 1, 65536 if name == "checkerboard" else 512, flow=field(h, w, i) if i % 2 else None,
                              pad=(0, 5)[i % 2], lead=(0, 1, 3)[i % 3], what=name)
        if name == "checkerboard" and (conn == 4 or min(h, w) > 1):    # one pixel wide, the diagonal neighbours are missing
            assert want["K"] == ((h * w + 1) // 2 if conn == 4 else 1)
        if name in ("spiral", "comb", "full"):
            assert want["summary"][0] == 1, "%s is %d components in the statement" % (name, want["summary"][0])
    ctx.regions_close()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840)])
def test_full_size_masks(ctx, h, w, conn):
    m = smooth_noise(h, w, 7 + conn)
    want = push_and_check(ctx, m, conn, 1, 4096, flow=field(h, w), what="smooth noise")
    assert 100 <= want["K"] <= 4096
    push_and_check(ctx, m, conn, 64, 4096, opened=False, what="smooth noise, min_area 64")
    push_and_check(ctx, np.full((h, w), 1, np.uint8), conn, 1, 16, flow=field(h, w, 2), pad=8, lead=1, what="full")
    ctx.regions_close()


def test_options(ctx):
    h, w = 480, 640
    rng = np.random.RandomState(21)
    m = smooth_noise(h, w, 3, 0.5)
    m[rng.rand(h, w) < 0.02] = 255                          # speckle beside the blobs
    vals = m.copy()
    vals[m > 0] = rng.choice([1, 128, 255, 7], int((m > 0).sum()))      # bytes 1 and 128 are foreground like 255
    flow = field(h, w, 1)
    bad = rng.rand(h, w) < 0.01
    flow[bad] = rng.choice([np.nan, np.inf, -np.inf, 2.0 ** 25, -2.0 ** 30], (int(bad.sum()), 1)).astype(np.float32)
    flow[10, 10] = (2.0 ** 24, -2.0 ** 24)                  # exactly on the bound: inside
    for conn in (4, 8):
        full = push_and_check(ctx, vals, conn, 1, 8192, flow=flow, pad=3, lead=1, what="bytes, bad flow")
        assert full["summary"][5] > 0
        largest = int(full["summary"][7])
        K64 = push_and_check(ctx, vals, conn, 64, 8192, flow=flow, what="min_area 64")["K"]
        assert 1 < K64 < full["K"]
        assert push_and_check(ctx, vals, conn, largest + 1, 16, flow=flow, what="min_area above the largest")["K"] == 0
        assert push_and_check(ctx, vals, conn, largest, 16, what="the largest alone")["K"] >= 1
        push_and_check(ctx, vals, conn, 64, 1, flow=flow, what="max_regions 1")
        over = push_and_check(ctx, vals, conn, 64, K64 - 1, flow=flow, what="one record short")
        assert over["K"] == K64 and over["labels"].max() == K64 and over["summary"][2] == K64 - 1
        push_and_check(ctx, vals, conn, 64, 256, flow=flow, inplace=True, pad=2, what="in place")
        push_and_check(ctx, vals, conn, 64, 256, labels=False, what="no labels")
    ctx.regions_close()


def test_repeat_then_another_mask(ctx):
    """scratch is cleared inside the sequence: the same mask twice gives the same bytes, another mask after it its own"""
    h, w = 251, 333
    a, b = smooth_noise(h, w, 1, 0.4), smooth_noise(h, w, 2, 0.7)
    ctx.regions_open(w, h, 8, 10, 64)
    for i, m in enumerate((a, a, b, np.zeros_like(a), a)):
        push_and_check(ctx, m, 8, 10, 64, flow=field(h, w, i % 2), opened=True, pushes=i + 1, what="push %d" % i)
    ctx.regions_close()


def test_set_reset_reopen_refusals(ctx):
    h, w = 120, 200
    m = smooth_noise(h, w, 5, 0.5)
    ctx.regions_open(w, h, 4, 5, 32)
    info = ctx.regions_info()
    assert (info["w"], info["h"], info["connectivity"], info["min_area"], info["max_regions"], info["pushes"]) == (w, h, 4, 5, 32, 0)
    assert info["launches_per_push"] == RC_REGIONS_LAUNCHES and info["device_bytes"] >= 8 * w * h
    rec, summ = ctx.regions_read()
    assert len(rec) == 0 and not any(summ.values())          # before the first push: zeros
    push_and_check(ctx, m, 4, 5, 32, opened=True, pushes=1)
    ctx.regions_set(20)
    assert ctx.regions_info()["min_area"] == 20
    push_and_check(ctx, m, 4, 20, 32, opened=True, pushes=2)
    # every refusal leaves info and the kept records as they were, and the next push gives what it would have given
    before = (ctx.regions_info(), ctx.regions_read())
    dm = torch.as_tensor(m).cuda()
    lab = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    fl = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    L, H, P = ctx._lib, ctx._h, lambda t: t.data_ptr()
    calls = [(lambda: L.rcflow_regions_push_dev(H, 0, None, w, None, 0, None, 0, None, 0, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w - 1, None, 0, None, 0, None, 0, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, P(fl), 8 * w - 8, None, 0, None, 0, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, P(fl) + 4, 8 * w, None, 0, None, 0, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, None, 0, P(lab), 4 * w + 2, None, 0, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, None, 0, P(lab) + 2, 4 * w, None, 0, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, None, 0, None, 0, P(dm), w + 1, None, None), EINVAL),      # in place needs the same step
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, None, 0, None, 0, P(dm) + 1, w, None, None), EINVAL),
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, None, 0, P(lab), 4 * w, P(lab), w, None, None), EINVAL),     # two outputs overlap
             (lambda: L.rcflow_regions_push_dev(H, 0, P(dm), w, P(fl), 8 * w, None, 0, P(fl), w, None, None), EINVAL),     # an output over an input
             (lambda: L.rcflow_regions_prims_dev(H, 0, 0, 0, 3, 0.0, P(lab)), EINVAL),
             (lambda: L.rcflow_regions_prims_dev(H, 0, 0, 1, -1, 0.0, P(lab)), EINVAL),
             (lambda: L.rcflow_regions_prims_dev(H, 0, 0, 1, 3, float("nan"), P(lab)), EINVAL),
             (lambda: L.rcflow_regions_set(H, 0, 0), EINVAL),
             (lambda: ctx.regions_open(w, h, 6, 1, 32), EINVAL),
             (lambda: ctx.regions_open(w, h, 8, 0, 32), EINVAL),
             (lambda: ctx.regions_open(w, h, 8, 1, 0), EINVAL),
             (lambda: ctx.regions_open(w, h, 8, 1, 65537), EINVAL),
             (lambda: ctx.regions_open(5000, 100, 8, 1, 32), ESIZE)]
    for i, (call, code) in enumerate(calls):
        try:
            rc = call()
        except RcflowError as e:
            rc = e.code
        assert rc == code, "refusal %d gave %d" % (i, rc)
        after = (ctx.regions_info(), ctx.regions_read())
        assert after[0] == before[0] and np.array_equal(after[1][0], before[1][0]) and after[1][1] == before[1][1], "refusal %d changed the state" % i
    want = push_and_check(ctx, m, 4, 20, 32, opened=True, pushes=3)
    # an accepted boundary: the labels begin at the first byte after the mask's range, in one allocation
    one = torch.full((5 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tm, tl = one[:h * w].view(h, w), one[h * w:5 * h * w].view(torch.int32).view(h, w)
    assert tl.data_ptr() == tm.data_ptr() + (h - 1) * tm.stride(0) + w
    tm.copy_(dm)
    ctx.regions_push(tm, labels=tl)
    touching = ctx.regions_read()
    ctx.regions_push(dm, labels=lab)                          # the same with separate allocations
    apart = ctx.regions_read()
    assert np.array_equal(tl.cpu().numpy(), lab.cpu().numpy()) and np.array_equal(tl.cpu().numpy(), want["labels"])
    assert np.array_equal(tm.cpu().numpy(), m) and (one[5 * h * w:] == SENTINEL).all()
    assert touching[0].tobytes() == apart[0].tobytes() and dict(touching[1], pushes=5) == apart[1] and touching[1]["pushes"] == 4
    ctx.regions_reset()
    assert ctx.regions_info()["pushes"] == 0 and ctx.regions_info()["min_area"] == 20
    rec, summ = ctx.regions_read()
    assert len(rec) == 0 and not any(summ.values())
    push_and_check(ctx, m, 4, 20, 32, opened=True, pushes=1)
    m2 = smooth_noise(77, 130, 9, 0.5)                        # re-open with another size
    push_and_check(ctx, m2, 8, 1, 64)
    assert ctx.regions_info()["min_area"] == 1
    ctx.regions_close()
    ctx.regions_close()
    for call in (ctx.regions_info, ctx.regions_read, ctx.regions_reset, lambda: ctx.regions_set(3), ctx.regions_prims):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE


def test_two_slots_on_two_streams(ctx):
    h, w = 251, 333
    ma, mb = smooth_noise(h, w, 11, 0.5), smooth_noise(h, w, 12, 0.6)
    masks, conns, mins = {0: ma, 1: mb}, {0: 8, 1: 4}, {0: 4, 1: 9}
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = {0: [], 1: []}
    for st, ts in ((0, s0), (1, s1)):
        with torch.cuda.stream(ts):
            ctx.regions_open(w, h, conns[st], mins[st], 128, stream=st)
    for rep in range(4):
        for st, ts in ((0, s0), (1, s1)):
            with torch.cuda.stream(ts):
                dm, fl = torch.as_tensor(masks[st]).cuda(), torch.as_tensor(field(h, w, st)).cuda()
                lab = torch.empty((h, w), dtype=torch.int32, device="cuda")
                out = torch.empty((h, w), dtype=torch.uint8, device="cuda")
                rec = torch.empty(128 * 144, dtype=torch.uint8, device="cuda")
                summ = torch.empty(8, dtype=torch.int64, device="cuda")
                ctx.regions_push(dm, flow=fl, labels=lab, mask_out=out, regions=rec, summary=summ, stream=st)
                prims = ctx.regions_prims(0x20c0ff, 2, 3, 1.5, stream=st)
                outs[st].append((lab, out, rec, summ, prims, dm, fl))
    torch.cuda.synchronize()
    for st in (0, 1):
        for rep, (lab, out, rec, summ, prims, _, _) in enumerate(outs[st]):
            want = R.regions(masks[st], conns[st], mins[st], 128, field(h, w, st), rep + 1)
            assert np.array_equal(lab.cpu().numpy(), want["labels"]) and np.array_equal(out.cpu().numpy(), want["mask_out"])
            assert np.array_equal(summ.cpu().numpy(), want["summary"])
            compare_records(rec.cpu().numpy().view(REGION_DTYPE), want["records"], "slot %d" % st)
            assert np.array_equal(prims.cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE),
                                  R.prims(want["records"], 0x20c0ff, 2, 3, 1.5).astype(DRAW_PRIM_DTYPE))
    for st, ts in ((0, s0), (1, s1)):
        with torch.cuda.stream(ts):
            ctx.regions_close(st)


def test_launches_per_push(ctx):
    """a push is RC_REGIONS_LAUNCHES launches whatever the mask holds; the primitives are one more"""
    h, w = 480, 640
    ctx.regions_open(w, h, 8, 1, 256)
    prims = torch.empty(6 * 256 * 32, dtype=torch.uint8, device="cuda")
    fl = torch.as_tensor(field(h, w)).cuda()
    ctx.profile_enable(True)
    for name, m in stress_masks(h, w):
        dm = torch.as_tensor(m).cuda()
        ctx.profile_reset()
        for rep in range(3):
            ctx.regions_push(dm, flow=fl if rep else None, mask_out=dm)
        ctx.regions_prims(out=prims)
        torch.cuda.synchronize()
        prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
        assert prof == dict([("regions@%d" % k, 3) for k in range(RC_REGIONS_LAUNCHES)] + [("regions@%d" % RC_REGIONS_LAUNCHES, 1)]), (name, prof)
    assert RC_REGIONS_LAUNCHES == 7
    buckets = ctx.profile_read_buckets()
    assert buckets["threshold"] > 0 and sorted(buckets) == sorted(["farneback", "polar", "threshold", "overlay", "erosion", "codec", "stream"])
    ctx.profile_enable(False)
    ctx.regions_close()


def test_product_chain_without_a_host_round_trip(ctx):
    """40 frames of synthetic surf through the frame loop; its outmask and the resident flow go straight into the regions, the
    opposing-flow map's mask likewise; the statement runs on the same mask and flow read back afterwards.  The primitives are
    drawn into a frame by rcflow_draw_dev and compared with the drawing statement on the statement's primitives."""
    w, h, T = 320, 240, 40
    clip = synth.surf_clip(w, h, T, seed=5)
    ctx.stream_reset()
    ctx.analysis_reset(w, h)
    ctx.regions_open(w, h, 8, 6, 64)
    ctx.ripmap_open(w, h, window=4, grid=(16, 12))
    outmask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    rmask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    labels = torch.empty((h, w), dtype=torch.int32, device="cuda")
    opened = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    regions = torch.empty(64 * 144, dtype=torch.uint8, device="cuda")
    summary = torch.empty(8, dtype=torch.int64, device="cuda")
    seen, pushes = 0, 0
    for t in range(T):
        ctx.frame_buffer(w, h)[:] = clip[t]
        flow = ctx.frame_loop_step(w, h, outmask=outmask)
        if flow is None:
            continue
        for src in ("outmask", "ripmap"):
            if src == "ripmap":
                ctx.ripmap_push(flow, mask=rmask)
            mask = outmask if src == "outmask" else rmask
            ctx.regions_push(mask, flow=flow, labels=labels, mask_out=opened, regions=regions, summary=summary)
            pushes += 1
            prims = ctx.regions_prims(0x20c0ff, 1, 2, 4.0)
            canvas_in = (np.arange(h * w * 3, dtype=np.int64) * 7 + t).astype(np.uint8).reshape(h, w, 3)
            canvas = torch.as_tensor(canvas_in).cuda()
            skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
            ctx.draw(canvas, prims, skipped=skipped)
            # only now the host looks
            hm, hf = mask.cpu().numpy(), flow.cpu().numpy().copy()
            want = R.regions(hm, 8, 6, 64, hf, pushes)
            assert np.array_equal(labels.cpu().numpy(), want["labels"]) and np.array_equal(opened.cpu().numpy(), want["mask_out"]), (t, src)
            assert np.array_equal(summary.cpu().numpy(), want["summary"]), (t, src)
            compare_records(regions.cpu().numpy().view(REGION_DTYPE), want["records"], "frame %d %s" % (t, src))
            wp = R.prims(want["records"], 0x20c0ff, 1, 2, 4.0)
            assert np.array_equal(prims.cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE), wp.astype(DRAW_PRIM_DTYPE))
            ref = canvas_in.copy()
            nskip = TR.draw(ref, wp.astype(TR.PRIM))
            assert np.array_equal(canvas.cpu().numpy(), ref) and int(skipped.item()) == nskip
            seen += want["K"]
    assert seen > 0, "no frame of the chain had a region"
    ctx.regions_close()
    ctx.ripmap_close()
    ctx.stream_reset()


def test_cpp_regions_against_the_statement(ctx, tmp_path):
    """rc::Regions (include/rcflow_module.hpp) compiled as tests/cpp's programs are and run on seeded masks; what it prints
    equals the numpy statement on the same masks."""
    w, h, n = 200, 120, 4
    lines = [l for l in _cpp.run("test_regions", tmp_path, w, h, n, gxx=True).splitlines() if l.startswith("push ")]
    assert len(lines) == n

    def fnv(a):
        s = 1469598103934665603
        for v in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
            s = ((s ^ v) * 1099511628211) & (2 ** 64 - 1)
        return "%016x" % s

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    for t, l in enumerate(lines):
        u, v = x + 3 * t + 1000, y + t + 1000
        mask = np.where(((u // 5) * (v // 7) + (u // 11) + t) % 5 < 2, 255, 0).astype(np.uint8)
        want = R.regions(mask, 8, 4, 64, None, t + 1)
        img = ((np.arange(w * h * 3, dtype=np.int64) * 7 + t) % 256).astype(np.uint8).reshape(h, w, 3)
        TR.draw(img, R.prims(want["records"], 0x20c0ff, 2, 3, 0.0).astype(TR.PRIM))
        parts = l.split(" | ")
        assert parts[0].split() == ["push", str(t), fnv(want["labels"]), fnv(want["mask_out"]), fnv(img)], "checksums at push %d" % t
        assert [int(q) for q in parts[1].split()] == want["summary"].tolist()
        nrec = int(want["summary"][2])
        assert len(parts) - 2 == nrec and nrec > 3
        for q, part in zip(want["records"][:nrec], parts[2:]):
            assert [int(s) for s in part.split()] == [int(q[k]) for k in ("label", "area", "x0", "y0", "x1", "y1", "first_x", "first_y", "edges",
                                                                          "sx", "sy", "sxx", "syy", "sxy")]
