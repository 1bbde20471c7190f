"""Rip tracks on the device (track_kernels.hip) against the numpy statement (tests/_tracks_ref.py): after every push every byte
of the table (all integer fields, mean_fx / mean_fy as bits), track_of_label, the confirmed mask, the summary and the footprint
(through rcflow_tracks_read) is compared with np.array_equal.  No tolerance anywhere.  Outputs and the padded label image sit
between fence bytes."""
import itertools

import numpy as np
import pytest
import torch

import _cpp
import _regions_ref as R
import _tracers_ref as TR
import _tracks_ref as T
from _dev import EINVAL, ESIZE, ESTATE, Fenced
from ripcurrents_amd._lib import RC_REGIONS_LAUNCHES, RC_TRACKS_LAUNCHES, RcflowError
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, TRACK_DTYPE

pytestmark = pytest.mark.gpu


def same_table(got, want, what):
    """every byte: the integer fields by name for the message, then the records as bytes (the floats as bits, the padding none)"""
    assert got.dtype == TRACK_DTYPE and len(got) == len(want), what
    for k in T.TRACK.names:
        a, b = got[k], want[k]
        if k.startswith("mean_"):
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), "%s: field %s differs: slots %s" % (what, k, np.flatnonzero(a != b)[:8])
    assert np.array_equal(got.view(np.uint8), want.astype(TRACK_DTYPE).view(np.uint8)), what


class Device:
    """one tracks state on the device beside the statement; push() compares everything"""

    def __init__(self, ctx, w, h, stream=0, **prm):
        self.ctx, self.w, self.h, self.stream = ctx, w, h, stream
        self.ref = T.Tracks(w, h, **prm)
        ctx.tracks_open(w, h, stream=stream, **prm)
        self.NR, self.NT = self.ref.max_regions, self.ref.max_tracks

    def push(self, labels, records, regions_summary, pad=0, lead=0, what=""):
        ctx, h, w = self.ctx, self.h, self.w
        want = self.ref.push(labels, records, regions_summary[2])
        what = "%s %dx%d push %d" % (what, w, h, self.ref.n)
        dl = Fenced(h, w, torch.int32, pad, lead, np.asarray(labels).astype(np.int32))
        nrec = max(len(records), self.NR)
        rec = np.zeros(nrec, R.REGION)
        rec[:len(records)] = records
        dr = torch.as_tensor(rec.view(np.uint8)).cuda()
        dsum = torch.as_tensor(np.asarray(regions_summary, np.int64)).cuda()
        dt = Fenced(1, self.NT * 128, torch.uint8, 0, 8)
        dtol = Fenced(1, self.NR + 1, torch.int32, 0, 1)
        dm = Fenced(h, w, torch.uint8, pad + 3, lead + 1)
        ds = Fenced(1, 8, torch.int64, 0, 1)
        ctx.tracks_push(dl.view, dr, dsum, tracks=dt.view.reshape(-1), track_of_label=dtol.view.reshape(-1), mask_out=dm.view,
                        summary=ds.view.reshape(-1), stream=self.stream)
        got_sum = ds.numpy().reshape(-1)
        assert np.array_equal(got_sum, want["summary"]), "%s: summary %s, expected %s" % (what, got_sum, want["summary"])
        same_table(dt.numpy().reshape(-1).view(TRACK_DTYPE), want["tracks"], what)
        assert np.array_equal(dtol.numpy().reshape(-1), want["track_of_label"]), "%s: track_of_label differs" % what
        assert np.array_equal(dm.numpy(), want["mask_out"]), "%s: %d mask pixels differ" % (what, int((dm.numpy() != want["mask_out"]).sum()))
        for f, name in ((dt, "tracks"), (dtol, "track_of_label"), (dm, "mask_out"), (ds, "summary"), (dl, "labels")):
            f.check(name)
        assert np.array_equal(dl.numpy(), np.asarray(labels).astype(np.int32)), "%s: the label image changed" % what
        tab, foot, summ = ctx.tracks_read(stream=self.stream)
        same_table(tab, want["tracks"], what + " (read)")
        assert np.array_equal(foot, want["footprint"]), "%s: %d footprint pixels differ" % (what, int((foot != want["footprint"]).sum()))
        assert list(summ.values()) == want["summary"].tolist(), what
        return want

    def push_mask(self, mask, conn, flow=None, **kw):
        g = R.regions(mask, conn, 1, self.NR, flow)
        return self.push(g["labels"], g["records"], g["summary"], **kw)


def field(h, w, seed=0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack([2.5 * np.sin(x / 31.0 + seed) + 1.5, 2.0 * np.cos(y / 27.0 - seed) - 0.5 + x / 100.0], -1).astype(np.float32)


def sequence(h, w, pushes, seed):
    """seeded blobs (boxes and discs) that drift up to 2 pixels per push, appear, vanish and flicker"""
    rng = np.random.RandomState(seed)
    n = max(1, min(24, h * w // 150))
    blobs = [dict(x=rng.uniform(0, w), y=rng.uniform(0, h), r=rng.uniform(0.6, 1 + min(h, w) / 9.0), vx=rng.uniform(-2, 2), vy=rng.uniform(-2, 2),
                  t0=rng.randint(0, pushes // 2), t1=rng.randint(pushes // 2, pushes + 3), disc=rng.rand() < 0.5,
                  off=set(rng.randint(0, pushes, 2).tolist()) if rng.rand() < 0.5 else set()) for _ in range(n)]
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(pushes):
        m = np.zeros((h, w), np.uint8)
        for b in blobs:
            if not (b["t0"] <= t < b["t1"]) or t in b["off"]:
                continue
            cx, cy = b["x"] + b["vx"] * t, b["y"] + b["vy"] * t
            d = (xx - cx) ** 2 + (yy - cy) ** 2 <= b["r"] ** 2 if b["disc"] else (np.abs(xx - cx) <= b["r"]) & (np.abs(yy - cy) <= b["r"])
            m[d] = 255
        yield m


SIZES = [(1, 1), (5, 7), (16, 64), (17, 65), (37, 53), (70, 130)]       # (h, w)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("h,w", SIZES)
def test_seeded_sequences(ctx, h, w, conn):
    seen = dict(coast=0, ended=0, born=0, split=0, merged=0, conf=0, untracked=0)
    for i, (nt, mo, mm) in enumerate(itertools.product((1, 3, 64), (1, 5), (0, 2))):
        pushes = 8 + i % 5
        dev = Device(ctx, w, h, max_regions=32, max_tracks=nt, min_overlap=mo, max_misses=mm, min_hits=1 + i % 3)
        for t, m in enumerate(sequence(h, w, pushes, 100 * h + w + i)):
            want = dev.push_mask(m, conn, field(h, w, t) if (i + t) % 2 else None, pad=(0, 5)[i % 2], lead=(0, 1, 3)[i % 3],
                                 what="conn %d tracks %d overlap %d misses %d" % (conn, nt, mo, mm))
            s, f = want["summary"], want["tracks"]["flags"]
            seen["coast"] += s[5]; seen["ended"] += s[3]; seen["born"] += s[2]; seen["untracked"] += s[6]; seen["conf"] += s[1]
            seen["split"] += int(((f & T.SPLIT) != 0).sum()); seen["merged"] += int(((f & T.MERGED) != 0).sum())
    ctx.tracks_close()
    assert seen["born"]
    if h * w >= 1000:                                                     # the sequences reach every branch of the rules
        assert all(seen.values()), seen


def full_frame(h, w):
    g = R.regions(np.full((h, w), 255, np.uint8), 8, 1, 4, field(h, w))
    return g["labels"], g["records"], g["summary"]


def checkerboard(h, w, max_regions, phase):
    """the conn-4 checkerboard without labelling every pixel on the host: every set pixel is its own component, numbered in
    raster order, and the first max_regions records depend on the top rows alone (their `edges` word, which the tracks do not
    read, aside)"""
    m = (np.indices((h, w)).sum(0) % 2) == phase
    labels = np.where(m, np.cumsum(m.reshape(-1)).reshape(h, w), 0).astype(np.int32)
    rows = min(h, 2 + 2 * max_regions // max(w // 2, 1) + 2)
    g = R.regions(m[:rows].astype(np.uint8), 4, 1, max_regions, field(h, w)[:rows])
    K = int(m.sum())
    assert np.array_equal(g["labels"], np.where(labels[:rows] <= g["K"], labels[:rows], 0)) and (rows == h or g["K"] >= max_regions)
    summary = g["summary"].copy()
    summary[0] = summary[1] = K
    return labels, g["records"], summary


@pytest.mark.parametrize("h,w", [(70, 130), (1080, 1920)])
def test_one_region_over_the_whole_frame(ctx, h, w):
    """every pixel adds to one word of the overlap table"""
    dev = Device(ctx, w, h, max_regions=16, max_tracks=4, min_overlap=1, max_misses=1, min_hits=2)
    full = full_frame(h, w)
    none = (np.zeros((h, w), np.int32), full[1], np.zeros(8, np.int64))
    for i, inp in enumerate((full, full, full, none, full, none, none, full)):
        want = dev.push(*inp, pad=i % 2, what="full frame")
        if i in (1, 2, 4):
            assert want["tracks"][0]["overlap"] == h * w and want["tracks"][0]["id"] == 1
    assert want["tracks"]["id"].tolist() == [2, 0, 0, 0]                # two misses ended the first track
    ctx.tracks_close()


@pytest.mark.parametrize("h,w", [(70, 130), (1080, 1920)])
def test_checkerboard_of_single_pixels(ctx, h, w):
    """almost every label is above R; the first R are as many distinct pairs per row as there are pixels"""
    NR = 1024
    dev = Device(ctx, w, h, max_regions=NR, max_tracks=64, min_overlap=1, max_misses=2, min_hits=2)
    a, b = checkerboard(h, w, NR, 0), checkerboard(h, w, NR, 1)
    assert a[0].max() > NR and a[2][2] == NR
    for i, inp in enumerate((a, a, b, a, b, b)):
        want = dev.push(*inp, pad=3 * (i % 2), lead=i % 2, what="checkerboard")
        if i == 0:
            assert want["summary"][2] == 64 and want["summary"][6] == NR - 64
        if i == 1:
            assert want["summary"][4] == 64 and (want["tracks"]["overlap"] == 1).all()
    # all slots: the table is as wide as it gets, and so is the prefix sum of the births
    dev = Device(ctx, w, h, max_regions=NR, max_tracks=1024, min_overlap=1, max_misses=0, min_hits=1)
    for i, inp in enumerate((a, b, a, a)):
        want = dev.push(*inp, what="checkerboard, 1024 slots")
    assert want["summary"][4] == 1024
    ctx.tracks_close()


def test_labels_that_are_no_regions(ctx):
    """negative labels, labels beyond max_regions and labels beyond the records written are background and index nothing"""
    h, w = 37, 53
    dev = Device(ctx, w, h, max_regions=6, max_tracks=8, min_overlap=1, max_misses=2, min_hits=1)
    rng = np.random.RandomState(4)
    beyond = 0
    for t, m in enumerate(sequence(h, w, 9, 79)):
        g = R.regions(m, 8, 1, 64)
        lab = g["labels"].copy()
        beyond += int(lab.max() > 6)
        bg = np.flatnonzero(lab.reshape(-1) == 0)
        pick = rng.choice(bg, 40, replace=False)
        lab.reshape(-1)[pick] = rng.choice([-1, -2 ** 31, 2 ** 31 - 1, 7, 1025, 65536, 10 ** 6], 40)
        summary = g["summary"].copy()
        if t % 3 == 2:
            summary[2] = (2, -1, 0)[t // 3]                              # fewer records than labels, a word that is no count
        dev.push(lab, g["records"], summary, pad=t % 2, what="odd labels")
    assert beyond >= 4, "the sequence has too few pushes with regions beyond max_regions"
    ctx.tracks_close()


def test_product_chain_without_a_host_round_trip(ctx):
    """mask -> rcflow_regions_push_dev -> rcflow_tracks_push_dev -> rcflow_tracks_prims_dev -> rcflow_draw_dev, every link a
    device tensor; the host looks when the last push has been queued"""
    h, w, n = 70, 130, 10
    masks = list(sequence(h, w, n, 5))
    ctx.regions_open(w, h, 8, 2, 32)
    ctx.tracks_open(w, h, max_regions=32, max_tracks=16, min_overlap=2, max_misses=1, min_hits=2)
    flow = torch.as_tensor(field(h, w)).cuda()
    labels = torch.empty((h, w), dtype=torch.int32, device="cuda")
    regions = torch.empty(32 * 144, dtype=torch.uint8, device="cuda")
    rsum = torch.empty(8, dtype=torch.int64, device="cuda")
    dmasks = [torch.as_tensor(m).cuda() for m in masks]
    canvas_in = [(np.arange(h * w * 3, dtype=np.int64) * 7 + t).astype(np.uint8).reshape(h, w, 3) for t in range(n)]
    outs = []
    for t in range(n):
        tab = torch.empty(16 * 128, dtype=torch.uint8, device="cuda")
        tol = torch.empty(33, dtype=torch.int32, device="cuda")
        conf = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        summ = torch.empty(8, dtype=torch.int64, device="cuda")
        canvas = torch.as_tensor(canvas_in[t]).cuda()
        skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.regions_push(dmasks[t], flow=flow, labels=labels, regions=regions, summary=rsum)
        ctx.tracks_push(labels, regions, rsum, tracks=tab, track_of_label=tol, mask_out=conf, summary=summ)
        prims = ctx.tracks_prims(0x20c0ff, 1, 2)
        ctx.draw(canvas, prims, skipped=skipped)
        outs.append((tab, tol, conf, summ, prims, canvas, skipped))
    # only now the host looks
    ref = T.Tracks(w, h, max_regions=32, max_tracks=16, min_overlap=2, max_misses=1, min_hits=2)
    drawn = 0
    for t, (tab, tol, conf, summ, prims, canvas, skipped) in enumerate(outs):
        g = R.regions(masks[t], 8, 2, 32, field(h, w), t + 1)
        want = ref.push(g["labels"], g["records"], g["summary"][2])
        same_table(tab.cpu().numpy().view(TRACK_DTYPE), want["tracks"], "chain push %d" % t)
        assert np.array_equal(tol.cpu().numpy(), want["track_of_label"]) and np.array_equal(conf.cpu().numpy(), want["mask_out"]), t
        assert np.array_equal(summ.cpu().numpy(), want["summary"]), t
        wp = T.prims(want["tracks"], 0x20c0ff, 1, 2)
        assert np.array_equal(prims.cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE), wp.astype(DRAW_PRIM_DTYPE)), t
        img = canvas_in[t].copy()
        nskip = TR.draw(img, wp.astype(TR.PRIM))
        assert np.array_equal(canvas.cpu().numpy(), img) and int(skipped.item()) == nskip, t
        drawn += int((wp["kind"] != 0).sum())
    assert drawn > 0, "no push of the chain had a confirmed track"
    assert np.array_equal(ctx.tracks_read()[1], ref.P)
    ctx.regions_close()
    ctx.tracks_close()


def test_launches_per_push(ctx):
    """a push is RC_TRACKS_LAUNCHES launches whatever the labels hold; the primitives are one more"""
    h, w = 70, 130
    ctx.tracks_open(w, h, max_regions=1024, max_tracks=64)
    assert ctx.tracks_info()["launches_per_push"] == RC_TRACKS_LAUNCHES == 6
    prims = torch.empty(5 * 64 * 32, dtype=torch.uint8, device="cuda")
    seq = list(sequence(h, w, 3, 9))
    inputs = [("empty", (np.zeros((h, w), np.int32), np.zeros(1, R.REGION), np.zeros(8, np.int64))), ("full", full_frame(h, w)),
              ("checkerboard", checkerboard(h, w, 1024, 0))]
    for i, m in enumerate(seq):
        g = R.regions(m, 8, 1, 1024)
        inputs.append(("blobs %d" % i, (g["labels"], g["records"], g["summary"])))
    ctx.profile_enable(True)
    for name, (lab, rec, summ) in inputs:
        full = np.zeros(1024, R.REGION)
        full[:min(len(rec), 1024)] = rec[:1024]
        dl, dr, ds = torch.as_tensor(np.asarray(lab, np.int32)).cuda(), torch.as_tensor(full.view(np.uint8)).cuda(), torch.as_tensor(np.asarray(summ, np.int64)).cuda()
        mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        ctx.profile_reset()
        for rep in range(3):
            ctx.tracks_push(dl, dr, ds, mask_out=mask if rep else None)
        ctx.tracks_prims(out=prims)
        torch.cuda.synchronize()
        prof = {r["kernel"]: r["launches"] for r in ctx.profile_read() if r["launches"]}
        assert prof == dict([("tracks@%d" % k, 3) for k in range(RC_TRACKS_LAUNCHES)] + [("tracks@%d" % RC_TRACKS_LAUNCHES, 1)]), (name, prof)
    # booked where regions@* are booked
    ctx.profile_reset()
    ctx.tracks_push(dl, dr, ds)
    torch.cuda.synchronize()
    only_tracks = ctx.profile_read_buckets()
    assert only_tracks["threshold"] > 0 and all(v == 0 for k, v in only_tracks.items() if k != "threshold"), only_tracks
    ctx.profile_enable(False)
    ctx.tracks_close()
    assert RC_REGIONS_LAUNCHES == 7


def test_two_slots_on_two_streams(ctx):
    h, w, n = 37, 53, 8
    prm = {0: dict(max_regions=32, max_tracks=8, min_overlap=1, max_misses=2, min_hits=2), 1: dict(max_regions=16, max_tracks=3, min_overlap=3, max_misses=0, min_hits=1)}
    seqs = {0: list(sequence(h, w, n, 31)), 1: list(sequence(h, w, n, 32))}
    regs = {st: [R.regions(m, 8, 1, prm[st]["max_regions"], field(h, w, st)) for m in seqs[st]] for st in (0, 1)}
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = {0: [], 1: []}
    for st, ts in ((0, s0), (1, s1)):
        with torch.cuda.stream(ts):
            ctx.tracks_open(w, h, stream=st, **prm[st])
    for t in range(n):
        for st, ts in ((0, s0), (1, s1)):
            with torch.cuda.stream(ts):
                g = regs[st][t]
                dl, dr, ds = torch.as_tensor(g["labels"]).cuda(), torch.as_tensor(g["records"].view(np.uint8)).cuda(), torch.as_tensor(g["summary"]).cuda()
                tab = torch.empty(prm[st]["max_tracks"] * 128, dtype=torch.uint8, device="cuda")
                tol = torch.empty(prm[st]["max_regions"] + 1, dtype=torch.int32, device="cuda")
                conf = torch.empty((h, w), dtype=torch.uint8, device="cuda")
                summ = torch.empty(8, dtype=torch.int64, device="cuda")
                ctx.tracks_push(dl, dr, ds, tracks=tab, track_of_label=tol, mask_out=conf, summary=summ, stream=st)
                prims = ctx.tracks_prims(0x20c0ff, 2, 3, stream=st)
                outs[st].append((tab, tol, conf, summ, prims, dl, dr, ds))
    torch.cuda.synchronize()
    for st in (0, 1):
        ref = T.Tracks(w, h, **prm[st])
        for t, (tab, tol, conf, summ, prims, _, _, _) in enumerate(outs[st]):
            want = ref.push(regs[st][t]["labels"], regs[st][t]["records"], regs[st][t]["summary"][2])
            same_table(tab.cpu().numpy().view(TRACK_DTYPE), want["tracks"], "slot %d push %d" % (st, t))
            assert np.array_equal(tol.cpu().numpy(), want["track_of_label"]) and np.array_equal(conf.cpu().numpy(), want["mask_out"])
            assert np.array_equal(summ.cpu().numpy(), want["summary"])
            assert np.array_equal(prims.cpu().numpy().reshape(-1).view(DRAW_PRIM_DTYPE), T.prims(want["tracks"], 0x20c0ff, 2, 3).astype(DRAW_PRIM_DTYPE))
    for st, ts in ((0, s0), (1, s1)):
        with torch.cuda.stream(ts):
            ctx.tracks_close(st)


def test_refusals_reset_reopen(ctx):
    h, w = 37, 53
    prm = dict(max_regions=32, max_tracks=8, min_overlap=1, max_misses=2, min_hits=2)
    dev = Device(ctx, w, h, **prm)
    info = ctx.tracks_info()
    assert (info["w"], info["h"], info["pushes"]) == (w, h, 0) and all(info[k] == v for k, v in prm.items())
    assert info["device_bytes"] >= 4 * w * h + 33 * 8 * 4 + 8 * 128
    tab, foot, summ = ctx.tracks_read()
    assert not tab.view(np.uint8).any() and not foot.any() and not any(summ.values())        # before the first push: zeros
    seq = list(sequence(h, w, 8, 3))
    for m in seq[:4]:
        dev.push_mask(m, 8)
    assert ctx.tracks_info()["pushes"] == 4
    # every refusal leaves info, the table, the footprint and the summary as they were
    before = (ctx.tracks_info(), ctx.tracks_read())
    g = R.regions(seq[4], 8, 1, 32)
    dl, dr, ds = torch.as_tensor(g["labels"]).cuda(), torch.as_tensor(g["records"].view(np.uint8)).cuda(), torch.as_tensor(g["summary"]).cuda()
    tab = torch.zeros(8 * 128 + 64, dtype=torch.uint8, device="cuda")
    tol = torch.zeros(64, dtype=torch.int32, device="cuda")
    msk = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    sm = torch.zeros(16, dtype=torch.int64, device="cuda")
    L, H, P = ctx._lib, ctx._h, lambda t: t.data_ptr()
    push = L.rcflow_tracks_push_dev
    calls = [(lambda: push(H, 0, None, 4 * w, P(dr), P(ds), None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, None, P(ds), None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), None, None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w - 4, P(dr), P(ds), None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w + 2, P(dr), P(ds), None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl) + 2, 4 * w, P(dr), P(ds), None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr) + 4, P(ds), None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds) + 4, None, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), P(tab) + 4, None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), None, P(tol) + 2, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), None, None, None, 0, P(sm) + 4), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), None, None, P(msk), w - 1, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), None, None, P(dl), w, None), EINVAL),              # an output over an input
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), P(dr), None, None, 0, None), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), None, None, None, 0, P(ds)), EINVAL),
             (lambda: push(H, 0, P(dl), 4 * w, P(dr), P(ds), P(tab), P(tab) + 8 * 128 - 4, None, 0, None), EINVAL),   # two outputs overlap
             (lambda: L.rcflow_tracks_prims_dev(H, 0, 0, 0, 3, P(tab)), EINVAL),
             (lambda: L.rcflow_tracks_prims_dev(H, 0, 0, 9, 3, P(tab)), EINVAL),
             (lambda: L.rcflow_tracks_prims_dev(H, 0, 0, 1, -1, P(tab)), EINVAL),
             (lambda: L.rcflow_tracks_prims_dev(H, 0, 0, 1, 3, None), EINVAL),
             (lambda: L.rcflow_tracks_read(H, 0, None, 4, None, None), EINVAL),
             (lambda: ctx.tracks_open(w, h, max_regions=0), EINVAL),
             (lambda: ctx.tracks_open(w, h, max_regions=1025), EINVAL),
             (lambda: ctx.tracks_open(w, h, max_tracks=0), EINVAL),
             (lambda: ctx.tracks_open(w, h, max_tracks=1025), EINVAL),
             (lambda: ctx.tracks_open(w, h, min_overlap=0), EINVAL),
             (lambda: ctx.tracks_open(w, h, max_misses=-1), EINVAL),
             (lambda: ctx.tracks_open(w, h, max_misses=65536), EINVAL),
             (lambda: ctx.tracks_open(w, h, min_hits=0), EINVAL),
             (lambda: ctx.tracks_open(0, h), EINVAL),
             (lambda: ctx.tracks_open(5000, 100), ESIZE)]
    for i, (call, code) in enumerate(calls):
        try:
            rc = call()
        except RcflowError as e:
            rc = e.code
        assert rc == code, "refusal %d gave %d" % (i, rc)
        after = (ctx.tracks_info(), ctx.tracks_read())
        assert after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1][:2], before[1][:2])) and after[1][2] == before[1][2], \
            "refusal %d changed the state" % i
    for m in seq[4:6]:                                                    # the sequence goes on as if nothing had been tried
        dev.push_mask(m, 8)
    ctx.tracks_reset()
    assert ctx.tracks_info()["pushes"] == 0
    tab, foot, summ = ctx.tracks_read()
    assert not tab.view(np.uint8).any() and not foot.any() and not any(summ.values())
    dev.ref.reset()
    for m in seq[2:6]:                                                    # ids and n start again
        want = dev.push_mask(m, 8)
    assert want["summary"][7] == 4
    dev = Device(ctx, 65, 17, max_regions=8, max_tracks=3, min_overlap=2, max_misses=0, min_hits=1)      # re-open with another size
    for m in sequence(17, 65, 4, 8):
        dev.push_mask(m, 4)
    assert ctx.tracks_info()["max_tracks"] == 3
    ctx.tracks_close()
    ctx.tracks_close()
    for call in (ctx.tracks_info, ctx.tracks_read, ctx.tracks_reset, ctx.tracks_prims, lambda: ctx.tracks_push(dl, dr, ds)):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE


def test_push_refuses_fewer_records_than_max_regions(ctx):
    """the push reads up to max_regions records whatever the summary says: the binding takes no shorter tensor"""
    h, w = 5, 7
    ctx.tracks_open(w, h, max_regions=32, max_tracks=4)
    dl = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ds = torch.zeros(8, dtype=torch.int64, device="cuda")
    for nrec in (1, 31):
        with pytest.raises(ValueError, match="max_regions"):
            ctx.tracks_push(dl, torch.zeros(nrec * 144, dtype=torch.uint8, device="cuda"), ds)
    assert ctx.tracks_info()["pushes"] == 0
    ctx.tracks_push(dl, torch.zeros(32 * 144, dtype=torch.uint8, device="cuda"), ds)
    ctx.tracks_push(dl, torch.zeros(40 * 144, dtype=torch.uint8, device="cuda"), ds)
    assert ctx.tracks_info()["pushes"] == 2 and ctx.tracks_read()[2]["pushes"] == 2
    ctx.tracks_close()


def test_cpp_tracks_against_the_statement(ctx, tmp_path):
    """rc::Tracks (include/rcflow_module.hpp) compiled as tests/cpp's programs are and run on seeded masks; what it prints
    equals the numpy statements on the same masks."""
    w, h, n = 200, 120, 9
    lines = [l for l in _cpp.run("test_tracks", tmp_path, w, h, n, gxx=True).splitlines() if l.startswith("push ")]
    assert len(lines) == n

    def fnv(a):
        s = 1469598103934665603
        for v in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
            s = ((s ^ v) * 1099511628211) & (2 ** 64 - 1)
        return "%016x" % s

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    ref = T.Tracks(w, h, max_regions=64, max_tracks=32, min_overlap=2, max_misses=1, min_hits=2)
    kinds = 0
    for t, l in enumerate(lines):
        u, v = x + t + 1000, y + 1000
        mask = np.where(((u // 9) * (v // 7) + (u // 13) + t // 4) % 5 < 2, 255, 0).astype(np.uint8)
        g = R.regions(mask, 8, 4, 64, None, t + 1)
        want = ref.push(g["labels"], g["records"], g["summary"][2])
        img = ((np.arange(w * h * 3, dtype=np.int64) * 7 + t) % 256).astype(np.uint8).reshape(h, w, 3)
        TR.draw(img, T.prims(want["tracks"], 0x20c0ff, 2, 3).astype(TR.PRIM))
        parts = l.split(" | ")
        assert parts[0].split() == ["push", str(t), fnv(want["mask_out"]), fnv(want["footprint"]), fnv(img)], "checksums at push %d" % t
        assert [int(q) for q in parts[1].split()] == want["summary"].tolist()
        live = want["tracks"][want["tracks"]["id"] != 0]
        assert len(parts) - 2 == len(live) and len(live) > 3
        for q, part in zip(live, parts[2:]):
            assert [int(s) for s in part.split()] == [int(q[k]) for k in ("id", "parent", "first_push", "area_sum", "slot", "label", "flags", "age",
                                                                          "hits", "misses", "area", "x0", "y0", "x1", "y1", "px", "py", "px0",
                                                                          "py0", "overlap")]
        kinds |= int(np.bitwise_or.reduce(live["flags"]))
    assert kinds & T.CONFIRMED and kinds & T.COASTING, "the program's masks exercise too little"
