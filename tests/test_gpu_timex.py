"""Time-exposure images on the device (timex_kernels.hip) against the numpy restatement of the reference's loops
(tests/_timex_ref.py): every comparison is bit-exact, after every push."""
import ctypes as C

import numpy as np
import pytest
import torch

import _timex_ref as R
from _dev import EINVAL, ESIZE, ESTATE
from ripcurrents_amd import synth
from ripcurrents_amd._lib import RcflowError

pytestmark = pytest.mark.gpu

ALL = ("mean", "average", "bright", "dark")


def colour_clip(w, h, frames, seed=7):
    """synth.surf_clip made three-channel: per-channel gains and offsets plus a noise channel -> (frames, h, w, 3) uint8, host."""
    g = synth.surf_clip(w, h, frames, seed=1234 + seed, device="cuda").float()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    noise = torch.randint(0, 64, g.shape, generator=gen, device="cuda").float()
    c0 = (g * 0.9 + 10).clamp(0, 255)
    c1 = (g * 1.2 - 20).clamp(0, 255)
    c2 = (255 - g * 0.8 + noise - 32).clamp(0, 255)
    return torch.stack([c0, c1, c2], -1).round().to(torch.uint8).cpu().numpy()


def run_and_compare(ctx, clip, window, products=ALL, stream=0, rows=None, reopen=True):
    """Pushes the clip into the device state and into the reference; compares every product after every push.
    rows: compare (and run the reference on) these rows only -- pixels are independent of each other."""
    n, h, w = clip.shape[:3]
    if reopen:
        ctx.timex_open(w, h, window, products, stream=stream)
    sel = slice(None) if rows is None else rows
    ref = R.TimexRef(w, len(np.arange(h)[sel]), window)
    for t in range(n):
        got = ctx.timex_push(torch.as_tensor(clip[t]).cuda(), stream=stream)
        want = ref.push(clip[t][sel], products)
        assert set(got) == set(products)
        for name in products:
            g = got[name].cpu().numpy()[sel]
            assert np.array_equal(g, want[name]), "%s differs after push %d: %d pixels" % (
                name, t + 1, int((g != want[name]).any(-1).sum()))


# ---------------------------------------------------------------------------- conversions
def test_conversions_on_all_triples(ctx):
    v = np.arange(1 << 24, dtype=np.uint32)
    allpx = np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(8, 1024, 2048, 3)
    for part in allpx:
        d = torch.as_tensor(part).cuda()
        assert np.array_equal(ctx.rgb_to_hsv_u8(d).cpu().numpy(), R.rgb_to_hsv_u8(part))
        assert np.array_equal(ctx.hsv_to_rgb_u8(d).cpu().numpy(), R.hsv_to_rgb_u8(part))


def test_conversions_odd_geometry(ctx):
    rng = np.random.RandomState(11)
    w, h, step = 97, 13, 3 * 97 + 5
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    base = torch.zeros(h * step + 8, dtype=torch.uint8, device="cuda")
    src = base[1:].as_strided((h, w, 3), (step, 3, 1))
    src.copy_(torch.as_tensor(img).cuda())
    obase = torch.full((h * step + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    dst = obase[3:].as_strided((h, w, 3), (step, 3, 1))
    ctx.rgb_to_hsv_u8(src, out=dst)
    assert np.array_equal(dst.cpu().numpy(), R.rgb_to_hsv_u8(img))
    keep = obase.cpu().numpy().copy()
    view = np.lib.stride_tricks.as_strided(keep[3:], (h, w, 3), (step, 3, 1))
    view[...] = 0xAB
    assert (keep == 0xAB).all(), "bytes between the rows were written"


def test_conversions_in_place_and_output_checks(ctx):
    rng = np.random.RandomState(12)
    img = rng.randint(0, 256, (37, 101, 3)).astype(np.uint8)
    d = torch.as_tensor(img).cuda()
    assert ctx.rgb_to_hsv_u8(d, out=d).data_ptr() == d.data_ptr()
    assert np.array_equal(d.cpu().numpy(), R.rgb_to_hsv_u8(img))
    ctx.hsv_to_rgb_u8(d, out=d)
    assert np.array_equal(d.cpu().numpy(), R.hsv_to_rgb_u8(R.rgb_to_hsv_u8(img)))
    for bad in (torch.zeros((37, 100, 3), dtype=torch.uint8, device="cuda"),          # another size
                torch.zeros((37, 101, 3), dtype=torch.int8, device="cuda"),           # another type
                torch.zeros((37, 101, 3), dtype=torch.uint8),                         # on the host
                torch.zeros((37, 101, 6), dtype=torch.uint8, device="cuda")[..., ::2]):   # pixels not dense
        with pytest.raises(ValueError):
            ctx.rgb_to_hsv_u8(d, out=bad)
        with pytest.raises(ValueError):
            ctx.hsv_to_rgb_u8(d, out=bad)


# ---------------------------------------------------------------------------- products on natural clips
@pytest.mark.parametrize("w, h, window, frames", [(97, 61, 1, 5), (97, 61, 2, 9), (160, 120, 10, 35), (640, 480, 50, 120),
                                                  (333, 77, 300, 320)])
def test_all_products_together(ctx, w, h, window, frames):
    clip = colour_clip(w, h, frames)
    run_and_compare(ctx, clip, window)


def test_all_products_1080p(ctx):
    """After every push on three bands and every 16th row (the reference is slow and pixels are independent of each
    other); the whole frame after the last push."""
    n, window = 60, 50
    clip = colour_clip(1920, 1080, n)
    rows = np.unique(np.r_[0:6, 537:545, 1074:1080, 0:1080:16])
    run_and_compare(ctx, clip[:n - 1], window, rows=rows)
    got = ctx.timex_push(torch.as_tensor(clip[n - 1]).cuda())
    ref = R.TimexRef(1920, 1080, window)
    for t in range(n - 1):
        ref.push_mean(clip[t])
    for t in range(n - window, n - 1):                                # the ring as 59 pushes left it, slot = frame % window
        ref.buffer_hsv[t % window] = R.rgb_to_hsv_u8(clip[t])
    ref.current = (n - 1) % window
    want = ref.push(clip[n - 1])
    for name in ALL:
        assert np.array_equal(got[name].cpu().numpy(), want[name]), name
    assert ctx.timex_info()["device_bytes"] >= 1920 * 1080 * 3 * window


@pytest.mark.parametrize("product", ALL)
def test_each_product_alone_equals_together(ctx, product):
    w, h, window = 160, 120, 10
    clip = colour_clip(w, h, 25, seed=3)
    run_and_compare(ctx, clip, window, (product,))
    ctx.timex_open(w, h, window, ALL)
    ctx.timex_open(w, h, window, (product,), stream=1)
    for f in clip:
        d = torch.as_tensor(f).cuda()
        together = ctx.timex_push(d)[product]
        alone = ctx.timex_push(d, stream=1)[product]
        assert torch.equal(together, alone)
    ctx.timex_close(stream=1)


# ---------------------------------------------------------------------------- adversarial rings for the winner rule
def _const(w, h, v):
    return np.full((h, w, 3), v, np.uint8)


def adversarial_clips(w, h):
    rng = np.random.RandomState(5)
    base = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    yield "static", np.stack([base] * 27)
    ramp = np.linspace(1.0, 0.1, 27)
    yield "ramp_down", np.stack([(base * a).astype(np.uint8) for a in ramp])         # every push expires the BRIGHT winner
    yield "ramp_up", np.stack([(base * a).astype(np.uint8) for a in ramp[::-1]])     # ... and the DARK winner
    yield "all_255", np.stack([_const(w, h, 255)] * 20)
    yield "all_0_after_255", np.stack([_const(w, h, 255)] * 9 + [_const(w, h, 0)] * 18)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    yield "checkerboard", np.stack([board if t % 3 else 255 - board for t in range(27)])
    yield "grey_steps", np.stack([_const(w, h, v) for v in (8, 8, 9, 7, 8, 200, 8, 8, 1, 8, 8, 8, 255, 0, 8, 8, 8, 8, 8)])


@pytest.mark.parametrize("window", [2, 8, 9])
def test_winner_rule_on_adversarial_rings(ctx, window):
    for name, clip in adversarial_clips(53, 11):
        try:
            run_and_compare(ctx, clip, window)
        except AssertionError as e:
            raise AssertionError("%s, window %d: %s" % (name, window, e))


# ---------------------------------------------------------------------------- geometry of the arguments
def test_odd_steps_offset_bases_and_null_outputs(ctx):
    w, h, window = 97, 31, 6
    step = 3 * w + 5
    clip = colour_clip(w, h, 14, seed=9)
    ctx.timex_open(w, h, window, ALL)
    ref = R.TimexRef(w, h, window)
    fbase = torch.zeros(h * step + 8, dtype=torch.uint8, device="cuda")
    frame = fbase[1:].as_strided((h, w, 3), (step, 3, 1))
    outs = {}
    for k, name in enumerate(ALL):
        ob = torch.zeros(h * (step + k) + 8, dtype=torch.uint8, device="cuda")
        outs[name] = ob[k:].as_strided((h, w, 3), (step + k, 3, 1))
    for t, f in enumerate(clip):
        frame.copy_(torch.as_tensor(f).cuda())
        want = ref.push(f)
        skip = ALL[t % 4]                       # one product without an image per push: its state is still updated
        got = ctx.timex_push(frame, out={n: (None if n == skip else outs[n]) for n in ALL})
        assert set(got) == set(ALL) - {skip}
        for name in got:
            assert got[name].data_ptr() == outs[name].data_ptr()
            assert np.array_equal(got[name].cpu().numpy(), want[name]), (name, t)


def test_reset_reopen_slots_and_info(ctx):
    a = colour_clip(80, 40, 12, seed=1)
    b = colour_clip(64, 48, 12, seed=2)
    run_and_compare(ctx, a, 5)
    info = ctx.timex_info()
    assert (info["w"], info["h"], info["window"], info["frames_pushed"]) == (80, 40, 5, 12)
    assert info["products"] == ALL
    plane = 80 * 40
    assert info["device_bytes"] >= plane * (12 + 3 * 5 + 6 + 2 * 6)
    ctx.timex_reset()
    assert ctx.timex_info()["frames_pushed"] == 0
    run_and_compare(ctx, a[::-1].copy(), 5, reopen=False)            # reset = a fresh open
    run_and_compare(ctx, b, 7, ("mean", "dark"))                     # re-open with another size, window and set
    info = ctx.timex_info()
    assert (info["w"], info["h"], info["window"], info["products"]) == (64, 48, 7, ("mean", "dark"))
    ctx.timex_open(64, 48, 1, ("mean",))
    assert ctx.timex_info()["window"] == 0                           # MEAN alone keeps no ring
    # two slots fed different clips, interleaved
    ctx.timex_open(80, 40, 4, ALL, stream=0)
    ctx.timex_open(64, 48, 3, ALL, stream=1)
    ra, rb = R.TimexRef(80, 40, 4), R.TimexRef(64, 48, 3)
    for fa, fb in zip(a, b):
        ga = ctx.timex_push(torch.as_tensor(fa).cuda(), stream=0)
        gb = ctx.timex_push(torch.as_tensor(fb).cuda(), stream=1)
        wa, wb = ra.push(fa), rb.push(fb)
        for name in ALL:
            assert np.array_equal(ga[name].cpu().numpy(), wa[name]) and np.array_equal(gb[name].cpu().numpy(), wb[name])
    ctx.timex_close(stream=1)
    ctx.timex_close(stream=0)


def test_first_pushes_on_a_fresh_context():
    """open / reset zero the state on the stream the slot has then; the pushes may run on another one.  A context of its
    own: its slot has never been bound to torch's stream (the session fixture's slots have)."""
    from ripcurrents_amd.api import Context
    w, h, window = 160, 120, 6
    clip = colour_clip(w, h, 2 * window + 3, seed=21)
    for open_on_own_stream in (False, True):
        junk = torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device="cuda")   # what a later allocation may be handed
        del junk
        torch.cuda.empty_cache()
        with Context(w, h) as fresh:
            if open_on_own_stream:            # the C caller's order: open on the slot's own stream, then move the slot
                fresh.use_own_stream()
                fresh.timex_open(w, h, window, ALL)
                fresh.use_torch_stream()
            run_and_compare(fresh, clip, window, reopen=open_on_own_stream is False)
            fresh.use_own_stream()
            fresh.timex_reset()               # zeroed on the own stream again
            fresh.use_torch_stream()
            run_and_compare(fresh, clip[::-1].copy(), window, reopen=False)


def test_refusals(ctx):
    lib, h_ = ctx._lib, ctx._h

    def code(fn):
        with pytest.raises(RcflowError) as e:
            fn()
        return e.value.code

    ctx.timex_close()
    ctx.timex_close()                                                # closing twice is fine
    frame = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    ptrs, steps = (C.c_void_p * 4)(), (C.c_size_t * 4)()
    assert lib.rcflow_timex_push_dev(h_, 0, C.c_void_p(frame.data_ptr()), 192, ptrs, steps) == ESTATE      # push before open
    assert lib.rcflow_timex_reset(h_, 0) == ESTATE
    assert code(lambda: ctx.timex_info()) == ESTATE
    assert lib.rcflow_timex_open(h_, 0, 64, 48, 50, 0) == EINVAL                                          # bad masks
    assert lib.rcflow_timex_open(h_, 0, 64, 48, 50, 16) == EINVAL
    assert lib.rcflow_timex_open(h_, 0, 64, 48, 0, 2) == EINVAL                                           # window < 1
    assert lib.rcflow_timex_open(h_, 0, 64, 48, 4097, 4) == EINVAL
    assert lib.rcflow_timex_open(h_, 0, 0, 48, 5, 1) == EINVAL
    assert lib.rcflow_timex_open(h_, 0, ctx.max_w + 1, 48, 5, 1) == ESIZE
    assert lib.rcflow_timex_open(h_, 9, 64, 48, 5, 1) == EINVAL                                           # no such slot
    assert lib.rcflow_timex_open(h_, 0, 64, 48, 0, 1) == 0                                                # window ignored for MEAN alone
    ctx.timex_open(64, 48, 5, ("mean", "bright"))
    out = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    assert lib.rcflow_timex_push_dev(h_, 0, None, 192, ptrs, steps) == EINVAL                             # null frame
    assert lib.rcflow_timex_push_dev(h_, 0, C.c_void_p(frame.data_ptr()), 191, ptrs, steps) == EINVAL     # step < 3 * w
    assert code(lambda: ctx.timex_push(frame, out={"dark": out})) == EINVAL                               # product not open
    ptrs[0], steps[0] = out.data_ptr(), 100
    assert lib.rcflow_timex_push_dev(h_, 0, C.c_void_p(frame.data_ptr()), 192, ptrs, steps) == EINVAL     # output step
    assert code(lambda: ctx.timex_push(frame, out={"mean": frame})) == EINVAL                             # in place
    assert code(lambda: ctx.timex_push(frame, out={"mean": out, "bright": out})) == EINVAL                # outputs overlap
    assert ctx.timex_info()["frames_pushed"] == 0                                                         # a refused push counts nothing
    assert lib.rcflow_timex_push_dev(h_, 0, C.c_void_p(frame.data_ptr()), 192, None, None) == 0           # no images at all
    assert ctx.timex_info()["frames_pushed"] == 1
    with pytest.raises(ValueError):
        ctx.timex_push(torch.zeros((48, 65, 3), dtype=torch.uint8, device="cuda"))
    from ripcurrents_amd.api import _check_out
    assert _check_out(out, ctx.device, torch.uint8, "out", shape=(48, 64, 3), dense=True) is out
    with pytest.raises(ValueError):                                                                       # an image of another GPU
        _check_out(out, torch.device("cuda", ctx.device.index + 1), torch.uint8, "out", shape=(48, 64, 3), dense=True)
    with pytest.raises(ValueError):
        ctx.timex_open(64, 48, 5, ("median",))
    ctx.timex_close()
    assert code(lambda: ctx.timex_push(frame)) == ESTATE                                                  # close, then push
    assert lib.rcflow_rgb_to_hsv_u8_dev(h_, 0, C.c_void_p(frame.data_ptr()), 191, 64, 48, C.c_void_p(out.data_ptr()), 192) == EINVAL
    assert lib.rcflow_hsv_to_rgb_u8_dev(h_, 0, None, 192, 64, 48, C.c_void_p(out.data_ptr()), 192) == EINVAL
    assert lib.rcflow_resize_bgr_dev(h_, 0, C.c_void_p(frame.data_ptr()), 192, 64, 48, C.c_void_p(out.data_ptr()), 10, 64, 48) == EINVAL


# ---------------------------------------------------------------------------- the colour resize
@pytest.mark.parametrize("sw, sh, dw, dh", [(640, 480, 320, 240), (333, 77, 640, 480), (1920, 1080, 640, 480)])
def test_resize_bgr(ctx, sw, sh, dw, dh):
    frame = colour_clip(sw, sh, 1, seed=4)[0]
    got = ctx.resize_bgr(frame, dw, dh).cpu().numpy()
    assert np.array_equal(got, R.resize_bgr(frame, dw, dh))
    gray = ctx.resize_bgr_to_gray(frame, dw, dh).cpu().numpy()
    assert np.array_equal(R.bgr_to_gray(got), gray)


# ---------------------------------------------------------------------------- a long run of the mean
def test_mean_past_exact_fp32_integers(ctx):
    n, frame = 70000, np.full((16, 16, 3), 255, np.uint8)
    d = torch.as_tensor(frame).cuda()
    ctx.timex_open(16, 16, 1, ("mean",))
    checkpoints = set(range(65500, 66100, 37)) | {1, 2, 3, 1000, 33000, n - 1, n}
    s = np.float32(0)
    for t in range(1, n + 1):
        s = np.float32(s + np.float32(255))                          # the numpy float32 loop: 255 * t is exact only below 2^24
        if t in checkpoints:
            got = ctx.timex_push(d)["mean"].cpu().numpy()
            want = int(np.clip(np.rint(s * np.float32(1.0 / t)), 0, 255))
            assert (got == want).all(), (t, got[0, 0], want)
        else:
            ctx.timex_push(d, out={"mean": None})
    assert float(s) != 255.0 * n                                     # the sum did leave the exact integers
    assert ctx.timex_info()["frames_pushed"] == n
    ctx.timex_close()


def test_profile_books_timex_under_overlay(ctx):
    frame = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    ctx.timex_open(64, 48, 4, ALL)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        for _ in range(3):
            ctx.timex_push(frame)
        ctx.rgb_to_hsv_u8(frame)
        ctx.sync()
    finally:
        ctx.profile_enable(False)
    rec = {r["kernel"]: r for r in ctx.profile_read()}
    assert rec["timex@0"]["launches"] == 3 and rec["timex@1"]["launches"] == 3 and rec["frame_color@0"]["launches"] == 1
    assert rec["timex@0"]["alg_bytes"] == 3 * 30 * 64 * 48
    assert rec["timex@1"]["alg_bytes"] == 3 * (6 + 18 + 15 + 15) * 64 * 48
    buckets = ctx.profile_read_buckets()
    assert buckets["overlay"] > 0 and buckets["farneback"] == 0
    ctx.profile_reset()
    ctx.timex_close()
