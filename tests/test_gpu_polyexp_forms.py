"""Every form of the polynomial-expansion kernel against the oracle's R (pyr_polyexp_kernels.hip, A2).

rc_launch_polyexp dispatches k_polyexp<R, U8, TH, MFMA, PYR> over nine template radii (3, 5, 7, 8, 9, 12, 16, 24, 32), an 8-bit
or a float source, 32- or 48-row tiles, a VALU or a matrix-core vertical pass, with or without the fused pyramid, and
k_polyexp_multi for calls of one or two frames.  Every case here compares what a launch wrote with oracle.polyexp of the same
image (oracle.pyr_level for the pyramid images, bit for bit); nothing is compared with another HIP form.

  A  the float form through rcflow_stage_polyexp_dev: every radius, the zero-padded tap tables (n_eff below the template
     radius), the sigma = 0.3 n branch of the plan, both tile heights and both vertical passes, at the smallest sizes at which
     a 64 x TH tile kernel can go wrong.
  B  the 8-bit forms through the level driver (two-image call, clip call), read back with rcflow_debug_level_R /
     rcflow_debug_level_image: plain, multi, fused pyramid, 48-row tiles, matrix cores, frames beyond the first, padded rows,
     and bytes chosen against the per-tile constant.

Which instantiation a case runs is stated per case and pinned by asserting n_eff from rcflow_debug_plan_poly first: the
launcher picks the smallest template radius >= n_eff; option poly_tile_h = 48 wins over poly_mfma and is used only for
radius <= 9 (larger radii fall back to 32 rows, where poly_mfma decides); the fused pyramid and the multi launch exist only
for 8-bit, 32 rows, VALU, n_eff 3 / 5 / 7.

Ring entries (rcflow_api.hip): the two-image calls expand prev into entry 0 and next into entry 1; the clip call puts frame t
into entry t % nslots with nslots = chunk + 1 = 33 by default, so the 4-frame clips here have frame t in entry t.  Every driver
case checks each entry against its own frame and states that neighbouring frames differ by far more than the bar.

Bar: |dR| <= 2e-4 absolute, the project's figure for this stage (tests/test_gpu_farneback.py), for every form on
surf-clip input.  The oracle's own rounding (oracle.polyexp against the float64 np_oracle.polyexp of the same float image) is
at most 4.3e-5 over the parameter sets and sizes of part A (poly_n = 1 at 193x101; 1.8e-5 at 15 / 1.2) and falls as the radius
grows: no reason for a looser bar anywhere.  For the hostile
bytes the bar is set from the reference alone: 2e-4 x max(1, s_hostile / s_surf), s the oracle-vs-float64 maximum at the same
size and parameters.  Every case prints its per-channel maxima before it asserts ("[forms] ..." lines;
scripts/polyexp_forms_table.py turns a log into profiles/polyexp_forms_parity.md).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ripcurrents_amd import synth

pytestmark = pytest.mark.gpu

CHANNELS = ("y", "x", "yy", "xx", "xy")
BAR = 2e-4
RADII = (3, 5, 7, 8, 9, 12, 16, 24, 32)

# (poly_n, poly_sigma, n_eff): sigma 0 is the plan's sigma = 0.3 n branch, where the outermost evaluated tap carries weight
# (exp(-1 / 0.18) of the centre's), so a dropped or misplaced last tap moves R far beyond the bar.  n_eff below the template
# radius (1, 2, 4, 6, 10, 13, 15, 20, 28) runs a zero-padded tap table.
SIGMA0 = [(n, 0.0, n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 20, 24, 28, 32)]
FLOAT_PARAMS = SIGMA0 + [(15, 1.2, 7), (15, 1.5, 9), (15, 2.0, 15), (32, 4.0, 32)]
# 64x32 one tile; 65x49 one more column, a 1-row remainder at 48 rows and a 17-row one at 32; 130x70 and 193x101 partial tiles
# both ways (48 + 22 and 48 + 48 + 5 rows); the rest are smaller than the radius, at every radius
SIZES = [(64, 32), (65, 49), (130, 70), (193, 101), (20, 12), (7, 5), (2, 37), (1, 1)]
FLOW = dict(pyr_scale=0.5, winsize=3, iterations=2, flags=0)      # a box window: option exact = -1 keeps the fast path


def _radius(n_eff):
    return next(r for r in RADII if r >= n_eff)


def _n_eff(ctx, n, sigma):
    """n_eff of the plan for (poly_n, poly_sigma), option exact_taps off: rcflow_debug_plan_poly."""
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    fn = ctx._lib.rcflow_debug_plan_poly
    fn.argtypes, fn.restype = [C.c_int, C.c_double, C.c_int, fp, fp, fp, dp, C.POINTER(C.c_int), dp], C.c_int
    g, xg, xxg, ig = np.zeros(40, np.float32), np.zeros(40, np.float32), np.zeros(40, np.float32), np.zeros(4)
    ne, kdc = C.c_int(), C.c_double()
    assert fn(n, sigma, 0, g.ctypes.data_as(fp), xg.ctypes.data_as(fp), xxg.ctypes.data_as(fp), ig.ctypes.data_as(dp), C.byref(ne),
              C.byref(kdc)) == 0
    return ne.value


def _float_form(n_eff, tile_h, mfma):
    r = _radius(n_eff)
    th = 48 if tile_h == 48 and r <= 9 else 32
    return "k_polyexp<%d,f32,%d,%s>" % (r, th, "MFMA" if mfma and th == 32 else "VALU")


def _u8_form(n_eff, tile_h=32, mfma=0, kind="plain"):
    """kind: what the driver may do for a default-form scale 0 -- "multi" (one or two frames, merge_small), "pyr" (a batch
    at exact half sizes, fuse_pyr), else "plain"; both need 32 rows, VALU and n_eff 3 / 5 / 7 and fall back to plain."""
    r = _radius(n_eff)
    th = 48 if tile_h == 48 and r <= 9 else 32
    vert = "MFMA" if mfma and th == 32 else "VALU"
    if kind != "plain" and th == 32 and vert == "VALU" and n_eff in (3, 5, 7):
        return "k_polyexp_multi<%d>" % r if kind == "multi" else "k_polyexp<%d,u8,32,VALU,PYR>" % r
    return "k_polyexp<%d,u8,%d,%s>" % (r, th, vert)


@functools.lru_cache(maxsize=None)
def _surf(size, frames, seed):
    w, h = size
    clip = synth.surf_clip(max(w, 8), max(h, 8), frames, seed=seed)[:, :h, :w].copy()
    clip.setflags(write=False)
    return clip


def _noise(I, n, sigma, ref):
    """The oracle's own rounding on this image: oracle.polyexp against the float64 restatement."""
    from oracle import np_oracle
    return float(np.abs(ref.astype(np.float64) - np_oracle.polyexp(I, n, sigma)).max())


@functools.lru_cache(maxsize=None)
def _float_case(size, n, sigma):
    """(scale-0 float image, oracle R, the oracle's own noise) of one size and tap set: computed once, shared, read-only."""
    from oracle import oracle
    w, h = size
    I = oracle.pyr_level(_surf(size, 1, 11)[0], 0.0, 3, w, h)
    ref = oracle.polyexp(I, n, sigma)
    ref.setflags(write=False)
    return I, ref, _noise(I, n, sigma, ref)


def _level_ref(orc, frame, pyr_scale, levels, k, n, sigma):
    """(oracle image, oracle R, noise) of scale k of one 8-bit frame."""
    h, w = frame.shape
    g = orc.level_geometry(w, h, pyr_scale, levels, k)
    I = orc.pyr_level(frame, g["sigma"], g["ksize"], g["w"], g["h"])
    ref = orc.polyexp(I, n, sigma)
    return I, ref, _noise(I, n, sigma, ref)


def _line(part, form, n, sigma, n_eff, what, err, noise, bar=BAR):
    print("[forms] %s | %s | n=%d sigma=%g n_eff=%d | %s | %s | max %.3g | oracle noise %.3g | bar %.3g" % (
        part, form, n, sigma, n_eff, what, " ".join("%s %.3g" % (c, e) for c, e in zip(CHANNELS, err)), err.max(), noise, bar))


class _Options:
    """Context options for the length of a with block, back to their defaults after it."""
    DEFAULTS = dict(poly_tile_h=32, poly_mfma=0, merge_small=1, fuse_pyr=1)

    def __init__(self, ctx, **opts):
        assert set(opts) <= set(self.DEFAULTS)
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *a):
        for k in self.opts:
            self.ctx.set_option(k, self.DEFAULTS[k])


# ---------------------------------------------------------------------------- A: the float form
@pytest.mark.parametrize("tile_h,mfma", [(32, 0), (32, 1), (48, 0), (48, 1)])
@pytest.mark.parametrize("n,sigma,n_eff", FLOAT_PARAMS)
def test_float_form_against_oracle(ctx, n, sigma, n_eff, tile_h, mfma):
    assert _n_eff(ctx, n, sigma) == n_eff
    form = _float_form(n_eff, tile_h, mfma)
    missed = []
    with _Options(ctx, poly_tile_h=tile_h, poly_mfma=mfma):
        for size in SIZES:
            I, ref, noise = _float_case(size, n, sigma)
            got = ctx.stage_polyexp(I, n, sigma).cpu().numpy()
            assert got.shape == ref.shape
            err = np.abs(got - ref).reshape(-1, 5).max(0)
            _line("A", form, n, sigma, n_eff, "%dx%d" % size, err, noise)
            if not err.max() <= BAR:
                missed.append("%dx%d: %.3g" % (size + (err.max(),)))
    assert not missed, "%s n=%d sigma=%g: %s" % (form, n, sigma, ", ".join(missed))


# ---------------------------------------------------------------------------- B: the 8-bit forms through the level driver
def _npyr(orc, w, h, levels):
    """Pyramid scales the scale-0 launch of a batch writes itself (expand_frames): exact half / quarter sizes, 3 / 9 taps."""
    L = orc.level_geometry(w, h, 0.5, levels, 0)["levels"]
    g = [orc.level_geometry(w, h, 0.5, levels, k) for k in range(min(L, 2) + 1)]
    if L < 1 or (2 * g[1]["w"], 2 * g[1]["h"]) != (w, h) or g[1]["ksize"] != 3:
        return 0
    return 2 if L >= 2 and (4 * g[2]["w"], 4 * g[2]["h"]) == (w, h) and g[2]["ksize"] == 9 else 1


def _check_entries(ctx, orc, part, call, frames, levels, n, sigma, n_eff, tile_h=32, mfma=0, merge=1, fuse=1, bar=BAR, what="",
                   distinct=True):
    """After a Farneback call on `frames` (frame t in ring entry t): R of every scale of every entry against the oracle,
    the pyramid images of scales >= 1 bit for bit.  `call` is "pair" (a frame per launch: merge_small may put scales 0..2
    into k_polyexp_multi) or "clip" (all frames per launch: fuse_pyr may select the PYR form).  Returns (the form scale 0
    ran, the cases that missed)."""
    h, w = frames[0].shape
    L = orc.level_geometry(w, h, 0.5, levels, 0)["levels"]
    kind = "plain"
    if call == "pair" and merge and L >= 1:
        kind = "multi"
    elif call == "clip" and fuse and _npyr(orc, w, h, levels):
        kind = "pyr"
    form0 = _u8_form(n_eff, tile_h, mfma, kind)
    missed = []
    for k in range(L + 1):
        refs = [_level_ref(orc, f, 0.5, levels, k, n, sigma) for f in frames]
        form = form0 if k == 0 or ("multi" in form0 and k <= 2) else _float_form(n_eff, tile_h, mfma)
        for t, (I, ref, noise) in enumerate(refs):
            got = ctx.debug_level_R(w, h, 0.5, k, t).cpu().numpy()
            assert got.shape == ref.shape
            err = np.abs(got - ref).reshape(-1, 5).max(0)
            _line(part, form, n, sigma, n_eff, "%dx%d%s scale %d frame %d" % (w, h, what, k, t), err, noise, bar)
            if not err.max() <= bar:
                missed.append("scale %d frame %d: R %.3g" % (k, t, err.max()))
            if k >= 1 and not np.array_equal(ctx.debug_level_image(w, h, 0.5, k, t).cpu().numpy(), I):
                missed.append("scale %d frame %d: pyramid image differs" % (k, t))
            if distinct and min(w, h) >= 12:        # the entry holds THIS frame: its neighbour's R is far outside the bar
                assert np.abs(refs[(t + 1) % len(refs)][1] - ref).max() > 100 * bar
    return form0, missed


def _pair_call(ctx, a, b, levels, n, sigma, pad=0):
    """The two-image call on device tensors; pad > 0: rows of w + pad bytes."""
    h, w = a.shape
    buf = torch.zeros((2, h, w + pad), dtype=torch.uint8, device="cuda")
    buf[0, :, :w] = torch.as_tensor(np.array(a))
    buf[1, :, :w] = torch.as_tensor(np.array(b))
    prev, nxt = buf[0, :, :w], buf[1, :, :w]
    assert prev.stride(0) == w + pad
    ctx.calcOpticalFlowFarneback(prev, nxt, None, levels=levels, poly_n=n, poly_sigma=sigma, **FLOW)


def _clip_call(ctx, frames, levels, n, sigma):
    ctx.farneback_clip(torch.as_tensor(np.array(frames)).cuda(), levels=levels, poly_n=n, poly_sigma=sigma, **FLOW)


# 15 / 1.2 is the reference's call; the level count comes from the min_size = 32 crop and is asserted per size
@pytest.mark.parametrize("size,levels,want_L", [((64, 32), 0, 0), ((65, 49), 0, 0), ((130, 70), 0, 0), ((193, 101), 0, 0), ((20, 12), 0, 0),
                                                ((7, 5), 0, 0), ((2, 37), 0, 0), ((1, 1), 0, 0),
                                                ((130, 70), 2, 1), ((193, 101), 2, 1), ((128, 128), 2, 2), ((193, 131), 2, 2), ((65, 49), 2, 0)])
@pytest.mark.parametrize("merge", [1, 0])
def test_two_image_call_8bit_forms(ctx, orc, size, levels, want_L, merge):
    """levels = 0: the plain 8-bit k_polyexp.  More scales with merge_small (default): k_polyexp_multi, two grids (130x70,
    193x101: the crop leaves one scale above 0) or three (128x128, 193x131) in one launch; merge_small = 0: a launch each."""
    n, sigma, n_eff = 15, 1.2, 7
    assert _n_eff(ctx, n, sigma) == n_eff
    assert ctx.level_geometry(size[0], size[1], 0.5, levels, 0)[0] == want_L == orc.level_geometry(size[0], size[1], 0.5, levels, 0)["levels"]
    frames = _surf(size, 2, 41)
    with _Options(ctx, merge_small=merge):
        _pair_call(ctx, frames[0], frames[1], levels, n, sigma)
        form, missed = _check_entries(ctx, orc, "B two-image", "pair", frames, levels, n, sigma, n_eff, merge=merge)
    assert form == ("k_polyexp_multi<7>" if merge and want_L else "k_polyexp<7,u8,32,VALU>")
    assert not missed, "%s %dx%d: %s" % (form, size[0], size[1], ", ".join(missed))


# exact half (and quarter) sizes select the fused pyramid: 130x70 halves exactly to 65x35 and takes it with partial tiles both
# ways; 72x40 is cropped to scale 0 alone (40 / 2 < 32); 131x71 (scale 1 is 66x36) is not exact and takes the pyramid kernels
@pytest.mark.parametrize("size,want_L,npyr", [((128, 64), 1, 1), ((72, 40), 0, 0), ((136, 72), 1, 1), ((128, 128), 2, 2), ((136, 132), 2, 2),
                                              ((130, 70), 1, 1), ((131, 71), 1, 0)])
@pytest.mark.parametrize("fuse", [1, 0])
def test_clip_call_fused_pyramid_and_frames_beyond_the_first(ctx, orc, size, want_L, npyr, fuse):
    """A clip of 4 frames in one launch per scale (blockIdx.z = frame, entry = slot0 + z * zstep): every frame, every
    scale.  With fuse_pyr the scale-0 launch also writes pyramid scales 1..npyr, compared bit for bit."""
    n, sigma, n_eff = 15, 1.2, 7
    assert _n_eff(ctx, n, sigma) == n_eff
    w, h = size
    assert orc.level_geometry(w, h, 0.5, 2, 0)["levels"] == want_L and _npyr(orc, w, h, 2) == npyr
    frames = _surf(size, 4, 43)
    with _Options(ctx, fuse_pyr=fuse):
        _clip_call(ctx, frames, 2, n, sigma)
        form, missed = _check_entries(ctx, orc, "B clip", "clip", frames, 2, n, sigma, n_eff, fuse=fuse)
    assert form == ("k_polyexp<7,u8,32,VALU,PYR>" if fuse and npyr else "k_polyexp<7,u8,32,VALU>")
    assert not missed, "%s %dx%d: %s" % (form, w, h, ", ".join(missed))


@pytest.mark.parametrize("tile_h,mfma", [(32, 0), (48, 0), (32, 1)])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 20, 24, 28, 32])
def test_two_image_call_every_radius_tile_height_and_vertical_pass(ctx, orc, n, tile_h, mfma):
    """sigma 0 at every template radius on the 8-bit form: 48-row tiles (no fused pyramid, no multi launch), the matrix-core
    vertical pass, and the default options, under which n_eff 3 / 5 / 7 take the multi launch with scale 1 (130x70,
    193x101; 65x49 is cropped to scale 0 alone and takes the plain form)."""
    sigma, n_eff = 0.0, n
    assert _n_eff(ctx, n, sigma) == n_eff
    missed = []
    with _Options(ctx, poly_tile_h=tile_h, poly_mfma=mfma):
        for size in ((65, 49), (130, 70), (193, 101)):
            frames = _surf(size, 2, 41)
            _pair_call(ctx, frames[0], frames[1], 1, n, sigma)
            form, m = _check_entries(ctx, orc, "B two-image", "pair", frames, 1, n, sigma, n_eff, tile_h, mfma)
            missed += ["%s %dx%d %s" % ((form,) + size + (x,)) for x in m]
    assert not missed, ", ".join(missed)


@pytest.mark.parametrize("n", [3, 5, 7, 9, 16])
def test_clip_call_other_radii(ctx, orc, n):
    """sigma 0 through the clip call: radii 3, 5, 7 take the fused pyramid at 128x128 (two scales) and 136x72 (one), 9 and
    16 the plain form beside the pyramid kernels."""
    sigma, n_eff = 0.0, n
    assert _n_eff(ctx, n, sigma) == n_eff
    missed = []
    for size in ((128, 128), (136, 72)):
        frames = _surf(size, 4, 43)
        _clip_call(ctx, frames, 2, n, sigma)
        form, m = _check_entries(ctx, orc, "B clip", "clip", frames, 2, n, sigma, n_eff)
        assert ("PYR" in form) == (n <= 7)
        missed += ["%s %dx%d %s" % ((form,) + size + (x,)) for x in m]
    assert not missed, ", ".join(missed)


@pytest.mark.parametrize("size", [(130, 70), (193, 101), (65, 49)])
def test_two_image_call_padded_rows(ctx, orc, size):
    """Frame rows of w + 13 bytes (rcflow_farneback_dev with a step): the rows are not 4-byte aligned, so every tile takes
    the per-byte staging path."""
    n, sigma, n_eff = 15, 1.2, 7
    assert _n_eff(ctx, n, sigma) == n_eff
    frames = _surf(size, 2, 41)
    missed = []
    for merge in (1, 0):
        with _Options(ctx, merge_small=merge):
            _pair_call(ctx, frames[0], frames[1], 1, n, sigma, pad=13)
            missed += _check_entries(ctx, orc, "B padded", "pair", frames, 1, n, sigma, n_eff, merge=merge, what=" step w+13")[1]
    assert not missed, ", ".join(missed)


def _hostile(kind, w, h):
    rng = np.random.RandomState(5)
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "noise":
        a, b = rng.randint(0, 256, (2, h, w))
    elif kind == "const255":
        a = b = np.full((h, w), 255)
    elif kind == "checker":
        a = 255 * ((xs + ys) & 1)
        b = 255 - a
    elif kind == "edge":
        a = np.where(xs >= 70, 255, 0)          # a half plane; the edge crosses a tile's interior
        b = np.where(ys >= 33, 255, 0)          # and one row past a tile boundary
    else:                                       # a large constant under a small signal
        a, b = 250 + rng.randint(-2, 3, (2, h, w))
    return np.stack([a, b]).astype(np.uint8)


@pytest.mark.parametrize("tile_h,mfma", [(32, 0), (48, 0), (32, 1)])
@pytest.mark.parametrize("kind", ["noise", "const255", "checker", "edge", "250pm2"])
def test_hostile_bytes(ctx, orc, kind, tile_h, mfma):
    """130x70 bytes chosen against the 8-bit tile: the integer 3x3 blur at its extremes, a per-tile constant of 255, a
    checker the blur flattens to 127.5 exactly, a step edge, and 250 +- 2.  The bar comes from the reference alone:
    2e-4 x max(1, s_hostile / s_surf), s the oracle's own maximum against float64 at this size and these parameters."""
    n, sigma, n_eff = 15, 1.2, 7
    assert _n_eff(ctx, n, sigma) == n_eff
    size = (130, 70)
    frames = _hostile(kind, *size)
    s_surf = max(_level_ref(orc, f, 0.5, 0, 0, n, sigma)[2] for f in _surf(size, 2, 41))
    s_host = max(_level_ref(orc, f, 0.5, 0, 0, n, sigma)[2] for f in frames)
    bar = BAR * max(1.0, s_host / s_surf)
    print("[forms] hostile %s: s_hostile %.3g, s_surf %.3g, bar %.3g" % (kind, s_host, s_surf, bar))
    with _Options(ctx, poly_tile_h=tile_h, poly_mfma=mfma):
        _pair_call(ctx, frames[0], frames[1], 1, n, sigma)
        form, missed = _check_entries(ctx, orc, "B hostile " + kind, "pair", frames, 1, n, sigma, n_eff, tile_h, mfma, bar=bar,
                                      distinct=False)
    assert not missed, "%s %s: %s" % (form, kind, ", ".join(missed))
