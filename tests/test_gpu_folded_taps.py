"""GPU tests of the folded expansion taps and of the stored scale of the R planes (DESIGN.md sections 3 and 4).

The fast expansion writes (y, x, yy, xx) x 1/2 and xy x 1/4 and the fast flow kernels read the planes at that scale; the
stage entry points keep speaking upstream's R.  What can go wrong is a tap table that is off (test 1), a writer and a
reader that disagree on the scale (test 2: a missed or doubled 1/2 moves the flow by whole pixels), and the branch of the
flow kernels that does not interpolate (test 3: samples that leave the image).
"""
import functools

import numpy as np
import pytest

from ripcurrents_amd import synth

pytestmark = pytest.mark.gpu

CHANNELS = ("y", "x", "yy", "xx", "xy")


@functools.lru_cache(maxsize=None)
def _poly_case(size, n, sigma):
    """(scale-0 image, oracle expansion) of one size and tap set: computed once, shared, read-only."""
    from oracle import oracle
    w, h = size
    img = synth.surf_clip(w, h, 1, seed=11)[0]
    I = oracle.pyr_level(img, 0.0, 3, w, h)
    ref = oracle.polyexp(I, n, sigma)
    ref.setflags(write=False)       # (I goes to torch.as_tensor, which warns about read-only arrays; nothing writes to it)
    return I, ref


# 130x70 and 193x101: partial 64x32 tiles in both directions and more than one tile row; 64x32: exactly one tile
@pytest.mark.parametrize("size", [(130, 70), (193, 101), (64, 32)])
@pytest.mark.parametrize("n,sigma,exact_taps", [(15, 1.2, 0), (15, 1.2, 1), (5, 1.1, 0), (7, 1.5, 0)])
@pytest.mark.parametrize("mfma", [0, 1])
def test_polyexp_folded_taps_against_oracle(ctx, orc, size, n, sigma, exact_taps, mfma):
    I, ref = _poly_case(size, n, sigma)
    ctx.set_option("poly_mfma", mfma)
    ctx.set_option("exact_taps", exact_taps)
    try:
        got = ctx.stage_polyexp(I, n, sigma).cpu().numpy()
    finally:
        ctx.set_option("poly_mfma", 0)
        ctx.set_option("exact_taps", 0)
    err = np.abs(got - ref).reshape(-1, 5).max(0)
    print("\n[parity] polyexp folded %dx%d n=%d sigma=%g exact_taps=%d mfma=%d: %s" % (
        size[0], size[1], n, sigma, exact_taps, mfma, " ".join("%s %.3g" % (c, e) for c, e in zip(CHANNELS, err))))
    assert err.max() <= 2e-4


# twice the maximum difference measured on the commit before this change (see the docstring below)
PARENT_STAGE_DIFF_BOUND = 2 * 1.505e-4


def test_stored_scale_writers_and_readers_agree(ctx):
    """The two-image call (fused 8-bit expansion -> fused two-iteration flow kernel, planes never leave the device)
    against the same work through the stage entry points (which unpack to and pack from upstream's R).

    The two paths are not bit-equal: the fused scale-0 expansion removes a per-tile constant taken from the 8-bit
    frame, the stage expansion one taken from the blurred float image, so their fp32 sums round differently.  The
    commit before the stored scale changed differs by 1.51e-4 px at most on this input (mean |flow| 1.58 px), printed
    to three digits; the bound is twice the lower end of what that print can stand for.  A missed or doubled factor
    of two moves the flow by whole pixels."""
    w, h = 96, 80
    clip = synth.surf_clip(w, h, 2, seed=31)
    whole = ctx.calcOpticalFlowFarneback(clip[0], clip[1], None, 0.5, 0, 3, 2, 15, 1.2, 0)
    I0 = ctx.stage_pyr_level(clip[0], 0.5, 0)
    I1 = ctx.stage_pyr_level(clip[1], 0.5, 0)
    R0 = ctx.stage_polyexp(I0, 15, 1.2)
    R1 = ctx.stage_polyexp(I1, 15, 1.2)
    f1 = ctx.stage_flow_iter(R0, R1, None, 3, 0)
    f2 = ctx.stage_flow_iter(R0, R1, f1, 3, 0).cpu().numpy()
    diff = np.abs(np.asarray(whole) - f2)
    print("\n[parity] two-image call vs stage composition 96x80: equal bits %s, max %.3g px, mean |flow| %.3g px" % (
        np.array_equal(np.asarray(whole), f2), diff.max(), np.abs(f2).mean()))
    assert diff.max() <= PARENT_STAGE_DIFF_BOUND


def test_flow_iter_samples_leaving_the_image(ctx, orc):
    """flow_in = 6 x N(0, 1) on a 64x48 image: many samples fall outside, where the flow kernels take R0 alone."""
    w, h = 64, 48
    clip = synth.surf_clip(w, h, 2, seed=23)
    I0 = orc.pyr_level(clip[0], 0.0, 3, w, h)
    I1 = orc.pyr_level(clip[1], 0.0, 3, w, h)
    R0, R1 = orc.polyexp(I0), orc.polyexp(I1)
    fin = (np.random.RandomState(3).randn(h, w, 2) * 6).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs + fin[..., 0], ys + fin[..., 1]
    outside = ~((np.floor(fx) >= 0) & (np.floor(fx) < w - 1) & (np.floor(fy) >= 0) & (np.floor(fy) < h - 1))
    assert outside.mean() > 0.1          # the branch under test is taken often
    M = orc.update_matrices(R0, R1, fin)
    ref = fin.copy()
    orc.update_flow(R0, R1, ref, M, 3, False, False)
    got = ctx.stage_flow_iter(R0, R1, fin, 3, 0).cpu().numpy()
    err = np.abs(got - ref).max(-1)
    frac = float((err <= 1e-3).mean())
    print("\n[parity] flow_iter 64x48, %.1f %% of samples outside: max %.3g px, within 1e-3 px %.5f" % (
        100 * outside.mean(), err.max(), frac))
    assert frac >= 0.999
