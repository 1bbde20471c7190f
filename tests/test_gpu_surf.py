"""The surf zone on the device (surf_kernels.hip) against its numpy statement (tests/_surf_ref.py): the table, the six pictures, the
line records, the channel records, the summary and the primitives of every push, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _regions_ref as RG
import _surf_ref as S
import _tracers_ref as TR
from _dev import EINVAL, ESIZE, ESTATE, NULL as null, SENTINEL, Outputs, Padded, ptr, raw
from _shoreline_ref import ragged_lines
from ripcurrents_amd._lib import RC_SURF_LAUNCHES, RcflowError, SurfInfo, SurfParams, TransectLine
from ripcurrents_amd.api import DRAW_PRIM_DTYPE, SURF_CHANNEL_DTYPE, SURF_LINE_DTYPE, SURF_SUMMARY, Surf

pytestmark = pytest.mark.gpu

IMAGES = ("now", "surf", "q", "mean", "sd", "picture")
ARRAYS = ("lines", "channels", "summary")
dev_image = Padded.of                                             # a picture on the device, rows `pad` pixels longer and the sentinel there


def views(d):
    d["q"] = d["q"].view(np.uint16)
    if "lines" in d:
        d["lines"], d["channels"] = d["lines"].view(SURF_LINE_DTYPE), d["channels"].view(SURF_CHANNEL_DTYPE)


def outputs(L, w, h, pad=0):
    """a session without lines takes no line and no channel records"""
    planes = {k: ((h, w), torch.uint8) for k in ("now", "surf", "mean", "sd")}
    planes.update(q=((h, w), torch.int16), picture=((h, w, 3), torch.uint8))
    flat = dict(summary=((8,), torch.int64, -1))
    if L:
        flat.update(lines=((L * 64,), torch.uint8, None), channels=((32 * 32,), torch.uint8, None))
    return Outputs(planes, flat, pad, views)


def compare(got, read, want, what):
    for k in IMAGES + ("summary",):
        assert np.array_equal(got[k], want[k]), "%s differs %s: %s, wanted %s" % (k, what, got[k], want[k])
    if "lines" in got:
        for k in ("lines", "channels"):
            for f in want[k].dtype.names:
                assert got[k][f].tobytes() == want[k][f].tobytes(), "%s.%s differs %s: %s, wanted %s" % (k, f, what, got[k][f], want[k][f])
    if read is not None:
        rl, rc, rs = read
        assert rl.tobytes() == want["lines"].tobytes(), "the slot's lines differ " + what
        assert rc.tobytes() == want["channels"][:len(rc)].tobytes() and len(rc) == min(int(want["summary"][6]), 32), "the slot's channels differ " + what
        assert [rs[k] for k in SURF_SUMMARY] == [int(v) for v in want["summary"]], "the slot's summary differs " + what


def run(ctx, w, h, lines, p, frames, pad=0, stream=0, keep_open=False, compare_from=0):
    """a sequence of frames through the device session and the statement, every output compared after every push from push
    `compare_from` on (the pushes before it ask for no output) -> (the statement, its outputs of every compared push)"""
    ref = S.SurfRef(w, h, lines, p, ctx.jet_lut())
    ctx.surf_open(w, h, lines, stream=stream, **p.kw())
    info = ctx.surf_info(stream=stream)
    assert (info["lines"], info["samples"], info["launches_per_push"]) == (ref.L, len(ref.table), RC_SURF_LAUNCHES if ref.L else 1)
    assert info["device_bytes"] >= S.state_bytes(w, h, p.window)
    table, geom = ctx.surf_table(stream=stream)
    assert table.tobytes() == ref.table.tobytes() and geom.tobytes() == ref.geom.tobytes()
    out, wants = outputs(ref.L, w, h, pad), []
    for t, img in enumerate(frames):
        d = dev_image(img, pad)
        want = ref.push(img)
        if t < compare_from:
            ctx.surf_push(d.view, stream=stream)
            continue
        ctx.surf_push(d.view, stream=stream, **out.kw())
        what = "after push %d" % (t + 1)
        compare(out.host(), ctx.surf_read(stream=stream), want, what)
        assert np.array_equal(d.view.cpu().numpy(), img), "the frame was written"
        d.check("the frame")
        info = ctx.surf_info(stream=stream)
        assert (info["held"], info["pushes"]) == (min(t + 1, p.window), t + 1)
        wants.append(want)
    if not keep_open:
        ctx.surf_close(stream=stream)
    return ref, wants


def flags_seen(wants):
    return int(np.bitwise_or.reduce(np.concatenate([x["lines"]["flags"] for x in wants])))


def lines_for(w, h):
    """the shoreline's ragged lines where they fit; two diagonals on a small picture; none on a single pixel"""
    if w >= 8 and h >= 19:
        return ragged_lines(w, h)
    if w > 1 and h > 1:
        return [(0.0, 0.0, float(w - 1), float(h - 1), 8), (float(w - 1), 0.25, 0.5, float(h - 1), 9)]
    return []


def random_frames(w, h, n, seed):
    """noise with flat bright and dark patches of frames in it: pixels break, stay broken for a while, and stop"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        f = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if t % 5 == 3:
            f[:, w // 3:] = 250
        if t % 7 == 4:
            f[h // 2:] = 3
        out.append(f)
    return out


# ---------------------------------------------------------------------------- the scene
@pytest.mark.parametrize("foam,pushes", [(False, 40), (True, 40), (False, 70), (True, 70)])
def test_scene_every_output_after_every_push(ctx, foam, pushes):
    """the scene of the CPU tier; 40 pushes fill the window of 32, 70 wrap the ring twice"""
    ref, wants = run(ctx, S.SCENE_W, S.SCENE_H, S.scene_lines(), S.SCENE, [S.surf_scene(t, foam=foam) for t in range(pushes)])
    last = wants[-1]
    assert tuple(np.flatnonzero(last["lines"]["flags"] & S.CHANNEL)) == S.CHANNEL_LINES and int(last["summary"][6]) == 2


# ---------------------------------------------------------------------------- ragged pixels
@pytest.mark.parametrize("W", [2, 3, 33, 64])
@pytest.mark.parametrize("w,h", [(67, 35), (5, 4), (1, 1), (130, 3), (257, 9), (640, 360)])
def test_ragged_with_padded_steps(ctx, w, h, W):
    """67 x 35: a partial wave and a partial dword; 5 x 4: one wave; 130 x 3: just past two ballots; 257 x 9: just past a wave's 256
    pixels; every window is wrapped"""
    p = S.Params(window=W, bright=128, delta=20, q_min=300, min_run=2, span=2, ratio=800, min_lines=1, vis_permille=700)
    pushes = W + 6 if W > 3 else 3 * W + 1
    ref, wants = run(ctx, w, h, lines_for(w, h), p, random_frames(w, h, pushes, seed=w + W), pad=5)
    assert any(x["now"].any() for x in wants) and any(x["surf"].any() for x in wants) and wants[-1]["sd"].max() > 0


def test_more_pixels_than_one_pass_of_the_grid(ctx):
    """surf@0 is launched with at most 256 blocks of 4 waves of 256 pixels, 262144 pixels a pass, which no other case here reaches
    (640 x 360 is 230400): at 1024 x 520 every block walks a second tile and some a third"""
    w, h = 1024, 520
    assert 640 * 360 < 256 * 4 * 256 < 2 * 256 * 4 * 256 < w * h
    run(ctx, w, h, lines_for(w, h), S.Params(window=2, bright=100, delta=10), random_frames(w, h, 3, seed=1), pad=3)


# ---------------------------------------------------------------------------- extremes
def test_all_255_all_0_and_alternating(ctx):
    w, h = 67, 35
    full, none = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    p = S.Params(window=4, bright=180, delta=40)
    ref, wants = run(ctx, w, h, lines_for(w, h), p, [full] * 6 + [none] * 6, pad=2)
    assert not any(x["now"].any() for x in wants)                      # bright, never above its own mean by delta
    ref, wants = run(ctx, w, h, lines_for(w, h), p, [full, none] * 6, pad=2)
    assert all((x["sd"] == 255).all() for x in wants[1::2]) and wants[-2]["now"].all()    # as many of 255 as of 0: the largest variance, sd = 255
    assert int(ref.S2.max()) == 2 * 255 * 255


def test_bright_0_delta_0_breaks_everywhere_and_delta_255_nowhere(ctx):
    w, h = 67, 35
    frames = random_frames(w, h, 9, seed=2)
    ref, wants = run(ctx, w, h, lines_for(w, h), S.Params(window=5, bright=0, delta=0), [np.zeros((h, w), np.uint8)] + frames[:3] + [np.zeros((h, w), np.uint8)])
    assert (wants[0]["q"] == 1).all() and wants[0]["now"].all()        # 0 >= 0 and 0 >= its mean: every pixel breaks
    ref, wants = run(ctx, w, h, lines_for(w, h), S.Params(window=5, bright=0, delta=0), [np.full((h, w), 9, np.uint8)] * 7)
    assert all((x["q"] == min(t + 1, 5)).all() for t, x in enumerate(wants)) and int(wants[-1]["summary"][3]) == 5 * w * h      # Q = n
    ref, wants = run(ctx, w, h, lines_for(w, h), S.Params(window=5, bright=0, delta=255), frames)
    assert not any(x["q"].any() for x in wants)                      # no grey level is 255 above a mean it is part of


def test_window_4096_the_bound_of_s2_and_the_wrap(ctx):
    """4100 pushes of 255 into W = 4096 on 5 x 4: S2 = 4096 * 255^2, Q = 4096; the last 8 pushes are compared"""
    w, h = 5, 4
    full = np.full((h, w), 255, np.uint8)
    ref, wants = run(ctx, w, h, lines_for(w, h), S.Params(window=4096, bright=0, delta=0, q_min=1000, vis_permille=1000), [full] * 4100, compare_from=4092)
    assert len(wants) == 8 and int(ref.S2.max()) == 4096 * 255 * 255 and (wants[-1]["q"] == 4096).all() and wants[-1]["surf"].all()
    assert (wants[-1]["mean"] == 255).all() and not wants[-1]["sd"].any() and int(wants[-1]["summary"][3]) == 4096 * w * h


# ---------------------------------------------------------------------------- lines
def load_frames(w, h, loads, n=8, gaps=()):
    """n frames of 0 and 255 that leave, with bright 128 and delta 0, row i with a load of loads[i]: Q = n on the row's first
    pixels and the rest on the next one.  Rows in `gaps` get theirs on every second pixel: a load without a run"""
    q = np.zeros((h, w), np.int64)
    for i, B in enumerate(loads):
        xs = range(0, w, 2) if i in gaps else range(w)
        for x in xs:
            q[i, x] = min(n, B)
            B -= q[i, x]
        assert B == 0
    return [np.where(q > t, 255, 0).astype(np.uint8) for t in range(n)]


def row_lines(w, h):
    return [(0.0, float(i), float(w - 1), float(i), w) for i in range(h)]


LOADS = S.Params(window=8, bright=128, delta=0, q_min=1000, min_run=2, span=6, ratio=500, min_lines=2)


def run_loads(ctx, w, loads, p, gaps=()):
    h = len(loads)
    ref, wants = run(ctx, w, h, row_lines(w, h), p, load_frames(w, h, loads, gaps=gaps), compare_from=7)
    assert wants[-1]["B"].tolist() == list(loads)
    return wants[-1]


def test_one_line_is_never_a_channel(ctx):
    last = run_loads(ctx, 16, [40], LOADS)
    assert last["lines"]["ref"][0] == 40 and last["lines"]["share"][0] == 1000 and not last["lines"]["flags"][0] and int(last["summary"][6]) == 0


@pytest.mark.parametrize("span", [0, 32])
def test_span_0_and_32(ctx, span):
    loads = [64] * 20 + [8, 8] + [64] * 48
    last = run_loads(ctx, 16, loads, S.Params(**dict(S.asdict(LOADS), span=span)))
    assert int(last["summary"][6]) == (0 if span == 0 else 1)          # span 0: the reference is the line itself


def test_channels_at_the_first_and_the_last_line_and_between_lines_without_a_band(ctx):
    """a flank is missing at line 0 and at line L - 1; the channel in the middle has flanks that carry a load but no run, so E is
    empty and the centre point is the middle of the centre line.  (E cannot be empty for want of lines: with L = min_lines every
    line would be a channel line, and the line of the largest load never is.)"""
    loads = [6, 6] + [60] * 8 + [64, 4, 2, 64] + [60] * 8 + [8, 7, 6]
    last = run_loads(ctx, 16, loads, LOADS, gaps=(10, 13))
    ch = last["channels"]
    assert [(int(c["first"]), int(c["count"]), int(c["centre"])) for c in ch[:3]] == [(0, 2, 0), (11, 2, 12), (22, 3, 24)] and int(last["summary"][6]) == 3
    assert (last["lines"]["flags"][[10, 13]] & S.NOBAND).all() and ch[1]["cx"] == 1920 and ch[0]["cx"] == 768
    assert ch[0]["cx"] != ch[1]["cx"] and [float(c["width_m"]) for c in ch[:3]] == [2.0, 3.0, 3.0]


def test_more_channels_than_are_recorded(ctx):
    """70 lines of alternating loads, min_lines 1, span 1: every low line between two high ones is a channel of its own, 34 of
    them (the 35th low line is the last line: its window is two lines, whose lower median is its own load); 32 are recorded"""
    loads = [64, 8] * 35
    last = run_loads(ctx, 16, loads, S.Params(**dict(S.asdict(LOADS), span=1, min_lines=1)))
    assert int(last["summary"][6]) == 34 and int(last["summary"][5]) == 34 and (last["channels"]["count"] == 1).all()
    assert last["channels"]["first"].tolist() == list(range(1, 65, 2))


def test_equal_loads_tie_in_rank_and_centre(ctx):
    last = run_loads(ctx, 16, [32] * 12, LOADS)
    assert (last["lines"]["share"] == 1000).all() and int(last["summary"][6]) == 0
    last = run_loads(ctx, 16, [64] * 6 + [8, 8, 8] + [64] * 6, LOADS)
    assert [(int(c["first"]), int(c["count"]), int(c["centre"])) for c in last["channels"][:1]] == [(6, 3, 6)]      # the lowest index of equals


def test_min_load_above_every_reference_and_min_run_above_n(ctx):
    last = run_loads(ctx, 16, [64] * 6 + [8, 8] + [64] * 6, S.Params(**dict(S.asdict(LOADS), min_load=65)))
    assert (last["lines"]["flags"] & S.NOREF).all() and not (last["lines"]["flags"] & S.CHANNEL).any() and int(last["summary"][6]) == 0
    last = run_loads(ctx, 80, [640] * 6 + [8, 8] + [640] * 6, S.Params(**dict(S.asdict(LOADS), min_run=64)))
    assert int(last["summary"][4]) == 6 + 6 and (last["lines"]["k1"][:6] == 79).all()       # 80 samples in a row: a run of 64 and more
    last = run_loads(ctx, 16, [64] * 6 + [8, 8] + [64] * 6, S.Params(**dict(S.asdict(LOADS), min_run=64)))
    assert (last["lines"]["flags"] & S.NOBAND).all() and int(last["summary"][4]) == 0 and int(last["summary"][6]) == 1


def test_ragged_lines_with_bands(ctx):
    """the shoreline's ragged lines over frames with a bright moving stripe: bands on diagonals, clamps at the last row and column"""
    w, h = 67, 35
    rng = np.random.default_rng(4)
    frames = []
    for t in range(12):
        f = rng.integers(0, 90, (h, w), dtype=np.uint8)
        f[:, 20 + (3 * t) % 9: 40 + (3 * t) % 9] = 240 if t % 2 else 60
        frames.append(f)
    ref, wants = run(ctx, w, h, ragged_lines(w, h), S.Params(window=6, bright=180, delta=30, q_min=300, min_run=3, span=2, ratio=900, min_lines=1), frames, pad=3)
    seen = flags_seen(wants)
    assert any((x["lines"]["k0"] > 0).any() for x in wants) and seen & S.NOBAND


# ---------------------------------------------------------------------------- a pixels-only session
def test_pixels_only_session(ctx):
    w, h = 67, 35
    p = S.Params(window=3, bright=128, delta=20)
    ref, wants = run(ctx, w, h, [], p, random_frames(w, h, 5, seed=6), pad=4, keep_open=True)
    assert all(int(x["summary"][4]) == 0 and int(x["summary"][1]) == int((x["now"] != 0).sum()) for x in wants)
    lib, hdl = raw(ctx)
    img = dev_image(random_frames(w, h, 1, seed=7)[0]).view
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    before = ctx.surf_info()
    args = lambda lines, chans: (hdl, 0, ptr(img), w, 1) + (null, 0) * 6 + (lines, chans, null)
    for lines, chans in ((ptr(buf), null), (null, ptr(buf))):
        assert lib.rcflow_surf_push_dev(*args(lines, chans)) == EINVAL and (lib.rcflow_last_error() or b"").decode().startswith("rcflow_surf_push_dev")
    assert lib.rcflow_surf_prims_dev(hdl, 0, 1, 1, 2, ptr(buf)) == EINVAL
    assert ctx.surf_info() == before
    rl, rc, rs = ctx.surf_read()
    assert rl.size == 0 and rc.size == 0 and rs["pushes"] == 5
    ctx.surf_close()


# ---------------------------------------------------------------------------- outputs
def test_each_output_alone_and_a_push_with_none(ctx):
    """what a push gives does not depend on which outputs it or earlier pushes asked for"""
    w, h = 67, 35
    lines, p = lines_for(w, h), S.Params(window=3, bright=128, delta=20, q_min=300, min_run=2, span=2, ratio=800, min_lines=1)
    keys = IMAGES + ARRAYS + (None, "all")
    frames = random_frames(w, h, len(keys), seed=8)
    ref = S.SurfRef(w, h, lines, p, ctx.jet_lut())
    ctx.surf_open(w, h, lines, **p.kw())
    out = outputs(ref.L, w, h)
    for t, key in enumerate(keys):
        d = dev_image(frames[t]).view
        want = ref.push(frames[t])
        fresh, untouched = outputs(ref.L, w, h), outputs(ref.L, w, h)
        if key == "all":
            ctx.surf_push(d, **out.kw())
            compare(out.host(), ctx.surf_read(), want, "after the single outputs")
            continue
        ctx.surf_push(d, **({} if key is None else {key: fresh.kw()[key]}))
        got = fresh.host()
        if key is not None:
            assert got[key].tobytes() == want[key].tobytes(), "%s alone differs" % key
        for other in IMAGES + ARRAYS:
            if other != key:
                assert torch.equal(fresh.kw()[other], untouched.kw()[other]), "%s was written" % other
        rl, rc, rs = ctx.surf_read()
        assert rl.tobytes() == want["lines"].tobytes() and [rs[k] for k in SURF_SUMMARY] == [int(v) for v in want["summary"]]
    ctx.surf_close()


def test_surf_mask_goes_straight_into_regions(ctx):
    w, h = S.SCENE_W, S.SCENE_H
    ref = S.SurfRef(w, h, S.scene_lines(), S.SCENE, ctx.jet_lut())
    ctx.surf_open(w, h, S.scene_lines(), **S.SCENE.kw())
    ctx.regions_open(w, h, connectivity=8, min_area=16, max_regions=16)
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    for t in range(34):
        f = S.surf_scene(t)
        want = ref.push(f)
        ctx.surf_push(dev_image(f).view, surf=mask)
    ctx.regions_push(mask)                                        # the same stream: no host round trip in between
    rec, summ = ctx.regions_read()
    wr = RG.regions(want["surf"], 8, 16, 16, None, 1)
    assert summ["kept"] == int(wr["summary"][1]) == 3 and np.array_equal(rec["area"], wr["records"]["area"][:len(rec)])     # the band, cut by two channels
    ctx.regions_close()
    ctx.surf_close()


def test_primitives_painted_by_draw(ctx):
    w, h = S.SCENE_W, S.SCENE_H
    ref = S.SurfRef(w, h, S.scene_lines(), S.SCENE, ctx.jet_lut())
    ctx.surf_open(w, h, S.scene_lines(), **S.SCENE.kw())
    empty = ctx.surf_prims(color=0x3060f0, thickness=2, disc_radius=3).cpu().numpy().view(DRAW_PRIM_DTYPE).ravel()
    assert empty.size == ref.L - 1 + 32 and not empty.view(np.uint8).any()                 # before the first push
    for t in range(12):
        f = S.surf_scene(t)
        ref.push(f)
        ctx.surf_push(dev_image(f).view)
    prims = ctx.surf_prims(color=0x3060f0, thickness=2, disc_radius=3)
    got, wp = prims.cpu().numpy().view(DRAW_PRIM_DTYPE).ravel(), ref.prims(0x3060f0, 2, 3)
    assert got.tobytes() == wp.tobytes()
    assert (wp["kind"] == S.LINE_PRIM).sum() == 32 - 5 - 1 and (wp["kind"] == S.DISC).sum() == 2 and (wp["kind"][:31] == 0).sum() == 5
    canvas = dev_image(np.repeat(f[..., None], 3, axis=2), 4)
    ctx.draw(canvas.view, prims)
    painted = np.repeat(f[..., None], 3, axis=2)
    TR.draw(painted, wp)
    assert np.array_equal(canvas.view.cpu().numpy(), painted) and not np.array_equal(painted, np.repeat(f[..., None], 3, axis=2))
    canvas.check("the canvas")
    ctx.surf_close()


# ---------------------------------------------------------------------------- set, reset, slots
def test_set_acts_from_the_next_push_and_reset_keeps_it(ctx):
    w, h = S.SCENE_W, S.SCENE_H
    lines, p = S.scene_lines(), S.Params(**dict(S.asdict(S.SCENE), window=6))
    ref = S.SurfRef(w, h, lines, p, ctx.jet_lut())
    ctx.surf_open(w, h, lines, **p.kw())
    out = outputs(ref.L, w, h)

    def push(t):
        f = S.surf_scene(t)
        ctx.surf_push(dev_image(f).view, **out.kw())
        compare(out.host(), ctx.surf_read(), ref.push(f), "push %d" % t)
    for t in range(4):
        push(t)
    new = (200, 10, 400, 950, 30, 250)
    ctx.surf_set(*new)
    ref.set(*new)
    info = ctx.surf_info()
    assert tuple(info[k] for k in ("bright", "delta", "q_min", "ratio", "min_load", "vis_permille", "pushes")) == new + (4,)
    push(4)
    push(5)
    ctx.surf_reset()
    ref.reset()
    info = ctx.surf_info()
    assert tuple(info[k] for k in ("bright", "delta", "q_min", "ratio", "min_load", "vis_permille", "pushes", "held")) == new + (0, 0)
    rl, rc, rs = ctx.surf_read()
    assert not rl.view(np.uint8).any() and rc.size == 0 and all(rs[k] == 0 for k in SURF_SUMMARY)
    for t in range(6, 14):                                        # from zero again: the window fills and wraps
        push(t)
    ctx.surf_close()


def test_two_slots(ctx):
    wa, ha, wb, hb = S.SCENE_W, S.SCENE_H, 67, 35
    pa, pb = S.Params(**dict(S.asdict(S.SCENE), window=4)), S.Params(window=3, bright=128, delta=20, q_min=300, min_run=2, span=2, ratio=800, min_lines=1)
    la, lb = S.scene_lines(), lines_for(wb, hb)
    ra, rb = S.SurfRef(wa, ha, la, pa, ctx.jet_lut()), S.SurfRef(wb, hb, lb, pb, ctx.jet_lut())
    ctx.surf_open(wa, ha, la, stream=0, **pa.kw())
    ctx.surf_open(wb, hb, lb, stream=1, **pb.kw())
    oa, ob = outputs(ra.L, wa, ha), outputs(rb.L, wb, hb)
    fb = random_frames(wb, hb, 6, seed=9)
    for t in range(6):
        ia, ib = S.surf_scene(t), fb[t]
        ctx.surf_push(dev_image(ia).view, stream=0, **oa.kw())
        ctx.surf_push(dev_image(ib).view, stream=1, **ob.kw())
        compare(oa.host(), ctx.surf_read(stream=0), ra.push(ia), "slot 0, push %d" % t)
        compare(ob.host(), ctx.surf_read(stream=1), rb.push(ib), "slot 1, push %d" % t)
    ctx.surf_close(stream=1)
    assert ctx.surf_info(stream=0)["pushes"] == 6
    ctx.surf_close(stream=0)


def test_product_object(ctx):
    w, h = S.SCENE_W, S.SCENE_H
    ref = S.SurfRef(w, h, S.scene_lines(), S.SCENE, ctx.jet_lut())
    with Surf(ctx, w, h, lines=S.scene_lines(), **S.SCENE.kw()) as sf:
        f = S.surf_scene(0)
        sd = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        sf.push(dev_image(f).view, sd=sd)
        want = ref.push(f)
        rl, rc, rs = sf.read()
        assert rl.tobytes() == want["lines"].tobytes() and rs["pushes"] == 1 and np.array_equal(sd.cpu().numpy(), want["sd"])
        assert sf.info()["pushes"] == 1 and sf.table()[0].size == len(ref.table) and sf.prims().shape == (ref.L - 1 + 32, 32)
        with pytest.raises(ValueError):
            sf.push(dev_image(np.repeat(f[..., None], 3, axis=2)).view)            # a colour frame into a grey session
        sf.set(200, 10, 400, 950, 30, 250)
        sf.reset()
        assert sf.info()["pushes"] == 0
    with pytest.raises(RcflowError):
        ctx.surf_info()


# ---------------------------------------------------------------------------- arguments and lifecycle
def test_refusals_and_lifecycle(ctx):
    w, h = S.SCENE_W, S.SCENE_H
    lines, good = S.scene_lines(), S.Params(**dict(S.asdict(S.SCENE), window=4))
    L = len(lines)
    ctx.surf_close()
    lib, hdl = raw(ctx)

    def text():
        return (lib.rcflow_last_error() or b"").decode()

    for call in (ctx.surf_info, ctx.surf_read, ctx.surf_reset, ctx.surf_table, lambda: ctx.surf_set(180, 40, 100, 500, 0, 500), ctx.surf_prims):
        with pytest.raises(RcflowError) as e:
            call()
        assert e.value.code == ESTATE
    buf = (C.c_longlong * 64)()
    for name, args in (("info", (C.byref(SurfInfo()),)), ("read", (buf, buf, buf)), ("reset", ()), ("table_read", (buf, buf)),
                       ("set", (180, 40, 100, 500, 0, 500)), ("prims_dev", (1, 1, 2, buf)), ("push_dev", (null, 0, 1) + (null, 0) * 6 + (null, null, null))):
        assert getattr(lib, "rcflow_surf_" + name)(hdl, 0, *args) == ESTATE and text().startswith("rcflow_surf_%s:" % name), text()
    nan, inf = float("nan"), float("inf")
    kw = good.kw()
    for bad in (dict(window=1), dict(window=4097), dict(bright=-1), dict(bright=256), dict(delta=-1), dict(delta=256), dict(q_min=0), dict(q_min=1001),
                dict(min_run=0), dict(min_run=65), dict(span=-1), dict(span=33), dict(ratio=0), dict(ratio=1000), dict(min_load=-1), dict(min_lines=0),
                dict(min_lines=65), dict(vis_permille=0), dict(vis_permille=1001), dict(metres_per_pixel=0.0), dict(metres_per_pixel=nan),
                dict(metres_per_pixel=inf)):
        assert S.open_error(w, h, lines, S.Params(**dict(kw, **bad))) == "parameters"
        with pytest.raises(RcflowError) as e:
            ctx.surf_open(w, h, lines, **dict(kw, **bad))
        assert e.value.code == EINVAL and text().startswith("rcflow_surf_open"), bad
    for bad_lines in ([(4.0, 4.0, 96.5, 4.0, 88)], [(4.0, 4.0, 91.0, 64.0, 88)], [(4.0, 4.0, 91.0, 4.0, 7)], [(4.0, 4.0, 91.0, 4.0, 1025)],
                      [(4.0, 4.0, 4.0, 4.0, 8)], lines * 100, [(4.0, 4.0, 91.0, 4.0, 1024)] * 257):
        with pytest.raises(RcflowError) as e:
            ctx.surf_open(w, h, bad_lines, **kw)                      # a line leaving the picture, n, no length, too many, S above the bound
        assert e.value.code == EINVAL and text().startswith("rcflow_surf_open"), bad_lines[0]
    arr = (TransectLine * L)(*[TransectLine(*l) for l in lines])
    p = SurfParams(window=4, bright=180, delta=40, q_min=100, min_run=3, span=6, ratio=500, min_load=0, min_lines=2, vis_permille=500, flags=1, pad=0,
                   metres_per_pixel=1.0)
    assert lib.rcflow_surf_open(hdl, 0, w, h, arr, L, C.byref(p)) == EINVAL               # unknown flag bits
    p.flags = 0
    assert lib.rcflow_surf_open(hdl, 0, w, h, arr, L, None) == EINVAL
    assert lib.rcflow_surf_open(hdl, 0, w, h, None, L, C.byref(p)) == EINVAL
    assert lib.rcflow_surf_open(hdl, 0, 0, h, arr, L, C.byref(p)) == EINVAL
    assert lib.rcflow_surf_open(hdl, 2, w, h, arr, L, C.byref(p)) == EINVAL               # no such slot
    with pytest.raises(RcflowError) as e:
        ctx.surf_open(4000, 2161, lines, **kw)                        # beyond the context
    assert e.value.code == ESIZE and text().startswith("rcflow_surf_open")
    with pytest.raises(RcflowError) as e:
        ctx.surf_open(1920, 1080, lines, **dict(kw, window=4096))     # 8 GiB of ring
    assert e.value.code == ESIZE and text().startswith("rcflow_surf_open") and str(S.state_bytes(1920, 1080, 4096)) in text()
    with pytest.raises(RcflowError):
        ctx.surf_info()                                               # nothing was left open by any of them

    ref, _ = run(ctx, w, h, lines, good, [S.surf_scene(0)], keep_open=True)
    assert lib.rcflow_surf_info(hdl, 0, None) == EINVAL
    before = ctx.surf_info()
    for bad in (dict(span=33), dict(window=1)):                       # a refused re-open keeps the state
        with pytest.raises(RcflowError):
            ctx.surf_open(w, h, lines, **dict(kw, **bad))
    assert ctx.surf_info() == before
    img = dev_image(S.surf_scene(1)).view
    big = torch.zeros(8 * h * w + 4096, dtype=torch.uint8, device="cuda")
    N = (null, 0)

    def push(image=None, step=w, ch=1, now=N, surf=N, q=N, mean=N, sd=N, pic=N, rec=null, chan=null, summ=null, slot=0):
        return lib.rcflow_surf_push_dev(hdl, slot, ptr(img) if image is None else image, step, ch, *now, *surf, *q, *mean, *sd, *pic, rec, chan, summ)

    refused = [
        push(image=null), push(step=w - 1), push(ch=3), push(ch=0), push(ch=2),                      # the wrong channel count
        push(now=(ptr(big), w - 1)), push(surf=(ptr(big), w - 1)), push(mean=(ptr(big), w - 1)), push(sd=(ptr(big), w - 1)),
        push(q=(ptr(big), 2 * w - 2)), push(q=(ptr(big, 1), 2 * w)), push(q=(ptr(big), 2 * w + 1)), push(pic=(ptr(big), 3 * w - 1)),
        push(rec=ptr(big, 2)), push(chan=ptr(big, 2)), push(summ=ptr(big, 4)),
        push(now=(ptr(img), w)),                                      # an output over the frame
        push(now=(ptr(big), w), q=(ptr(big, w * (h - 1)), 2 * w)),    # two outputs meeting in one row
        push(sd=(ptr(big), w), pic=(ptr(big, 16), 3 * w)), push(rec=ptr(big), chan=ptr(big, 64 * L - 4)), push(chan=ptr(big), summ=ptr(big, 1016)),
        push(mean=(ptr(big), w), summ=ptr(big)),
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert text().startswith("rcflow_surf_push_dev")
    assert push(ch=3) == EINVAL and "channel" in text()
    assert push(slot=2) == EINVAL
    for bad in ((256, 40, 100, 500, 0, 500), (180, -1, 100, 500, 0, 500), (180, 40, 0, 500, 0, 500), (180, 40, 100, 1000, 0, 500),
                (180, 40, 100, 500, -1, 500), (180, 40, 100, 500, 0, 1001)):
        with pytest.raises(RcflowError) as e:
            ctx.surf_set(*bad)
        assert e.value.code == EINVAL and text().startswith("rcflow_surf_set")
    assert lib.rcflow_surf_prims_dev(hdl, 0, 1, 0, 2, ptr(big)) == EINVAL and lib.rcflow_surf_prims_dev(hdl, 0, 1, 1, 2, null) == EINVAL
    assert text().startswith("rcflow_surf_prims_dev")
    assert ctx.surf_info() == before
    # nothing was queued and nothing changed: the second push gives what the statement gives
    out = outputs(L, w, h)
    ctx.surf_push(img, **out.kw())
    compare(out.host(), ctx.surf_read(), ref.push(S.surf_scene(1)), "(after the refusals)")
    # an accepted boundary: q begins at the first byte after now's range, in one allocation
    one = torch.full((3 * h * w + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    tn, tq = one[:h * w].view(h, w), one[h * w:3 * h * w].view(torch.int16).view(h, w)
    ctx.surf_push(img, now=tn, q=tq)
    want = ref.push(S.surf_scene(1))
    assert np.array_equal(tn.cpu().numpy(), want["now"]) and np.array_equal(tq.cpu().numpy().view(np.uint16), want["q"]) and (one[3 * h * w:] == SENTINEL).all()
    # a slot moved to another stream between pushes
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx.surf_push(img, **out.kw())
        got = ctx.surf_read()
    torch.cuda.synchronize()
    compare(out.host(), got, ref.push(S.surf_scene(1)), "(on another stream)")
    # re-open with another size replaces it
    run(ctx, 67, 35, lines_for(67, 35), S.Params(window=2, bright=128, delta=20), random_frames(67, 35, 3, seed=3))
    ctx.surf_close()                                                  # closing twice is fine
