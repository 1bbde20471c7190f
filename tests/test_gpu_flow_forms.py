"""Every flow-iteration launch the driver makes, held to a float64 reference of that one launch (flow_iter_kernels.hip).

Part A compares what ONE launch wrote with tests/_flow_ref.launch (np_oracle.update_matrices + blur_solve in float64) on the
launch's own inputs: R0 and R1 as the GPU holds them (rcflow_debug_level_R) or as the stage entry is given them, and the flow
field the launch read -- a synthetic field, the previous launch's output (rcflow_debug_level_flow) or the coarser scale's
field up-sampled with oracle.resize_linear.  No error is inherited from another launch or another scale.

  stage   rcflow_stage_flow_iter_dev: k_flow_iter_w3 (winsize 2, 3), k_flow_iter_big (m = 2, 5, 10), k_flow_iter_sweep
          (m = 5, 10, forced) and the runtime-tile kernel (winsize 1, 7, 9, 15, 31, 49), box and Gaussian, flow in zeros / smooth /
          2 % outliers of 3..40 px / whole-pixel targets including the last column and row, at the sizes of _flow_ref.SIZES.
  driver  two-image calls with options fuse_iters = 0 and exact = 0, so every iteration is a launch of its own:
          - levels = 1: the coarse scale's launches (flow in zeros, then the previous iteration) and scale 0's launch fed from the
            coarser scale, at exactly 2:1 (the closed-form path) and at pyr_scale 0.5 on odd sizes, 0.6, 0.75, 0.8;
          - iterations = 0 with OPTFLOW_USE_INITIAL_FLOW: k_flow_iter<64,16,.> and <32,32,.> with solve == 0 write the up-sampled
            field itself, held to oracle.resize_linear;
          - levels = 0 with OPTFLOW_USE_INITIAL_FLOW: the synthetic fields reach k_flow_iter_w3 unchanged (asserted with
            rcflow_stage_initial_flow_dev), output rows at a caller stride of w + 13 pixels.

Part B compares the fused two-iteration kernel k_flow_iter2_rrc, in its 28 x 12, 28 x 20 and 28 x 28 forms, without and with
tile chains, bit for bit with the same call made of Part A's launches (fuse_iters = 0, chain = 1): every flow-in mode, both
windows, 2 to 5 iterations, the sizes from 27 x 29 up, a caller stride, and the large-displacement initial fields at levels = 0.

Every case first asserts, through rcflow_debug_flow_form (the function the launchers switch on), that the launch it is about
takes the form it claims to test.  The limit of that assertion: the form is computed from the launch's arguments as the test
restates them (the scale's size, the pairs of the call, consecutive ring slots, 32-bit offsets), not read back from the
RcIterArgs the driver built.  It cannot drift from the launchers' switch; it would not see a driver that split the pairs of a
call differently (every clip here fits one chunk of 32) or cleared addr32 (frames and strides beyond 4 GB: none here).

Still covered by the whole-path tests alone: the flow in from the coarser scale (in_mode 2) inside k_flow_iter_big, the sweep
kernel and the runtime-tile kernel -- their launches are held to the reference through the stage entry, in_mode 0 and 1.

Bars of Part A (tests/_flow_ref.py has the definitions and the floor's derivation): over EVERY pixel but the excluded ones,
q = e (det + 1e-3) at most 4x the C++ float oracle's maximum on the same inputs, and e at most 4x the oracle's maximum where
det > 1e-2; a pixel within 8 float32 ulps of the field's largest flow passes, and every line counts the pixels that pass that
way only ("under floor": the floor is 7.6e-6 to 2.4e-4 px here and decides many small cases).  Where a winsize-2 / 3 box launch
is beyond 4x, the form's own float32 order restated in numpy on the same inputs (_flow_ref.restate_w3_box_f32, pinned on the
CPU by tests/test_flow_forms_ref.py) is the evidence the issue asks for: the pixel must then be within 1.25x that restatement
and within 5x the oracle, and the line says so ("restated ...").  Only the launches fed from the coarser scale exclude pixels (displaced position within 1e-4 px of a border line; at most 0.5 % of a field, asserted).  Every case prints its
figures before it asserts ("[flow-forms] ..." lines; scripts/flow_iter_forms_table.py turns a log into
profiles/flow_iter_forms_parity.md).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import _flow_ref as fr
from ripcurrents_amd import synth
from ripcurrents_amd.api import Context

pytestmark = pytest.mark.gpu

DEFAULTS = dict(exact=-1, fuse_iters=1, chain=8, ablate=0, chain_min_blocks=0)
USE_INITIAL_FLOW, GAUSSIAN = 4, 256
FORCE_CHAIN = 33554432
PAD = 13                      # caller rows of w + 13 pixels


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, DEFAULTS[k])


def expect_form(kernel, w, h, pairs, winsize, flags, **kw):
    f = Context.debug_flow_form(w, h, pairs, winsize, flags & GAUSSIAN, **kw)
    assert f["kernel"] == kernel, (kernel, f)
    return f


def _name(f):
    if f["kernel"] == "rrc":
        return "rrc 28x%d%s" % (f["th"], " chains %d" % f["groups"] if f["groups"] else "")
    return "%s %dx%d" % (f["kernel"], f["tw"], f["th"])


def check_launch(orc, part, form, what, R0, R1, fin, got, winsize, flags, exclude=None, factor=fr.FACTOR):
    """One launch against the reference; prints the figures, returns the list of what missed its bar."""
    R0, R1, got = np.asarray(R0), np.asarray(R1), np.asarray(got)
    ref, det = fr.launch(R0, R1, fin, winsize, flags & GAUSSIAN)
    orf = fr.oracle_launch(orc, R0, R1, fin, *fr.yardstick_window(winsize, flags & GAUSSIAN))
    n, g = fr.violations(got, ref, det, orf, exclude, factor)
    restated = ""
    if n and not (flags & GAUSSIAN) and winsize // 2 == 1 and "nonfinite" not in g:
        # a winsize-3 box launch beyond 4x the oracle: the form's own float32 order, restated in numpy on the same inputs
        # (within 1.25x of it and within 5x the oracle: _flow_ref.RESTATED_FACTOR, RESTATED_CAP)
        n, g = fr.violations(got, ref, det, orf, exclude, factor, restated=fr.restate_w3_box_f32(R0, R1, fin, winsize))
        restated = " | restated q %.3g e %.3g" % (g["q_restated"], g["e_restated"])
    h, w = ref.shape[:2]
    if "nonfinite" in g:
        print("[flow-forms] %s | %s | %dx%d | %s | NON-FINITE output at %d pixels" % (part, form, w, h, what, n))
        return ["%s %s %dx%d %s: non-finite" % (part, form, w, h, what)]
    ratio = max(g["q_kernel"] / g["q_oracle"] if g["q_oracle"] > 0 else 0.0, g["e_kernel"] / g["e_oracle"] if g["e_oracle"] > 0 else 0.0)
    print("[flow-forms] %s | %s | %dx%d | %s | q oracle %.3g kernel %.3g | e(det>1e-2) oracle %.3g kernel %.3g | e(all) oracle %.3g kernel %.3g | "
          "ratio %.2f of %g | floor %.3g | under floor %d | excluded %.4f %% | miss %d%s" % (part, form, w, h, what, g["q_oracle"], g["q_kernel"], g["e_oracle"], g["e_kernel"],
                                                                  g["e_oracle_all"], g["e_kernel_all"], ratio, factor, g["floor"], g["under_floor"], 100 * g["excluded"], n, restated))
    return ["%s %s %dx%d %s: %d pixels miss the bar (%r)" % (part, form, w, h, what, n, g)] if n else []


@functools.lru_cache(maxsize=None)
def _stage_R(size):
    from oracle import oracle
    R0, R1 = fr.surf_R(oracle, *size)
    R0.setflags(write=False)
    R1.setflags(write=False)
    return R0, R1


@functools.lru_cache(maxsize=None)
def _clip(size, frames, seed=31):
    w, h = size
    clip = synth.surf_clip(max(w, 8), max(h, 8), frames, seed=seed)[:, :h, :w].copy()
    clip.setflags(write=False)
    return clip


# ============================================================================ Part A, the stage entry
@pytest.mark.parametrize("form", sorted(fr.STAGE_FORMS))
def test_stage_launch_against_the_reference(ctx, orc, form):
    winsize, flags, ablate, kernel = fr.STAGE_FORMS[form]
    missed, tiles = [], set()
    with options(ctx, exact=0, ablate=ablate):
        for (w, h) in fr.SIZES:
            for kind in ("zeros", "smooth", "outliers", "whole"):
                fin = fr.FIELDS[kind](w, h)
                f = expect_form(kernel, w, h, 1, winsize, flags, solve=1, in_mode=0 if fin is None else 1, ablate=ablate)
                tiles.add((f["tiles_x"] > 1, f["tiles_y"] > 1, w % f["tw"] != 0, h % f["th"] != 0))
                R0, R1 = _stage_R((w, h))
                got = ctx.stage_flow_iter(R0, R1, fin, winsize, flags).cpu().numpy()
                missed += check_launch(orc, "A stage", "%s (%s)" % (form, _name(f)), kind, R0, R1, fin, got, winsize, flags,
                                       factor=fr.factor_of(form))
    # the sizes reach more than one tile each way and ragged last tiles, whatever tile the form picked
    assert any(t[0] and t[2] for t in tiles) and any(t[1] and t[3] for t in tiles), tiles
    assert not missed, "\n".join(missed)


# ============================================================================ Part A, through the driver
def _two_image_call(ctx, clip, p, init=None):
    """calcOpticalFlowFarneback on device tensors, output rows of w + PAD pixels (in/out when `init` seeds the call)."""
    h, w = clip.shape[1:]
    buf = torch.full((h, w + PAD, 2), 7.0, dtype=torch.float32, device="cuda")
    out = buf[:, :w]
    if init is not None:
        out.copy_(torch.as_tensor(init).cuda())
    a, b = torch.as_tensor(clip[0].copy()).cuda(), torch.as_tensor(clip[1].copy()).cuda()
    ctx.calcOpticalFlowFarneback(a, b, out, **p)
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((buf[:, w:] == 7.0).all())              # nothing written past a row's w pixels
    return out


def _level_R(ctx, w, h, ps, k):
    return ctx.debug_level_R(w, h, ps, k, 0).cpu().numpy(), ctx.debug_level_R(w, h, ps, k, 1).cpu().numpy()


@pytest.mark.parametrize("flags", [0, GAUSSIAN])
@pytest.mark.parametrize("case", fr.UP_CASES, ids=lambda c: "%dx%d-%g" % c)
def test_driver_launches_fed_from_the_coarser_scale(ctx, orc, case, flags):
    """levels = 1, iterations 1 and 2, one launch per iteration: scale 1's launches (zeros in, then the previous iteration) and
    scale 0's (the coarser scale in, then the previous iteration), each on the GPU's own R and the GPU's own flow in."""
    w, h, ps = case
    clip = _clip((w, h), 2)
    L, cw, ch = ctx.level_geometry(w, h, ps, 1, 1)
    assert L == 1
    exact2 = (w == 2 * cw and h == 2 * ch)
    assert exact2 == (ps == 0.5 and w % 2 == 0 and h % 2 == 0)
    missed = []
    with options(ctx, exact=0, fuse_iters=0):
        for iters in (1, 2):
            p = dict(pyr_scale=ps, levels=1, winsize=3, iterations=iters, poly_n=15, poly_sigma=1.2, flags=flags)
            f1 = expect_form("w3", cw, ch, 1, 3, flags, solve=1, in_mode=0)
            f0 = expect_form("w3", w, h, 1, 3, flags, solve=1, in_mode=2)
            out = _two_image_call(ctx, clip, p).cpu().numpy()
            R10, R11 = _level_R(ctx, w, h, ps, 1)
            R00, R01 = _level_R(ctx, w, h, ps, 0)
            # buffers: the launches that do not write the caller's rows alternate A, B
            c_first = ctx.debug_level_flow(w, h, ps, 1, 0).cpu().numpy()
            coarse = c_first if iters == 1 else ctx.debug_level_flow(w, h, ps, 1, 1).cpu().numpy()
            fine_first = out if iters == 1 else ctx.debug_level_flow(w, h, ps, 0, 0).cpu().numpy()
            tag = "%s it%d ps%g" % ("gauss" if flags else "box", iters, ps)
            missed += check_launch(orc, "A driver", "w3 zeros in (%s)" % _name(f1), tag + " scale 1", R10, R11, None, c_first, 3, flags)
            if iters == 2:
                missed += check_launch(orc, "A driver", "w3 previous in (%s)" % _name(f1), tag + " scale 1", R10, R11, c_first, coarse, 3, flags)
            fin = fr.upsampled(orc, coarse, w, h, ps)
            excl = fr.border_excluded(fin)
            assert excl.mean() <= fr.EXCLUDE_CAP, excl.mean()
            missed += check_launch(orc, "A driver", "w3 coarse in %s (%s)" % ("2:1" if exact2 else "ratio", _name(f0)), tag + " scale 0",
                                   R00, R01, fin, fine_first, 3, flags, excl)
            if iters == 2:
                missed += check_launch(orc, "A driver", "w3 previous in (%s)" % _name(f0), tag + " scale 0, caller stride", R00, R01, fine_first, out, 3, flags)
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("winsize,flags,tile", [(3, 0, (64, 16)), (3, GAUSSIAN, (64, 16)), (5, 0, (64, 16)), (10, GAUSSIAN, (32, 32)), (20, 0, (32, 32))])
def test_driver_iterations_0_writes_the_upsampled_field(ctx, orc, winsize, flags, tile):
    """iterations = 0, levels = 1, OPTFLOW_USE_INITIAL_FLOW: k_flow_iter<64,16,.> / <32,32,.> with solve == 0.  Scale 1's launch
    copies the reduced initial field, scale 0's writes resize(INTER_LINEAR) of it times 1 / pyr_scale into the caller's rows.
    Bar: 4 float32 ulps of the largest flow -- two lerps of three roundings each and the product, against the same formula in
    the oracle's float arithmetic."""
    for (w, h, ps) in [(98, 70, 0.5), (332, 252, 0.5), (97, 70, 0.5), (131, 71, 0.75), (333, 251, 0.8), (333, 251, 0.6)]:
        L, cw, ch = ctx.level_geometry(w, h, ps, 1, 1)
        f = expect_form("tile", w, h, 1, winsize, flags, solve=0, in_mode=2)
        assert (f["tw"], f["th"]) == tile and expect_form("tile", cw, ch, 1, winsize, flags, solve=0, in_mode=1)["tw"] == tile[0]
        init = fr.outlier_field(w, h, seed=3)
        p = dict(pyr_scale=ps, levels=1, winsize=winsize, iterations=0, poly_n=15, poly_sigma=1.2, flags=flags | USE_INITIAL_FLOW)
        with options(ctx, exact=0, fuse_iters=0):
            out = _two_image_call(ctx, _clip((w, h), 2), p, init).cpu().numpy()
            coarse = ctx.debug_level_flow(w, h, ps, 1, 0)
            seeded = ctx.stage_initial_flow(init, ps, 1)
        assert coarse.shape == (ch, cw, 2) and torch.equal(coarse, seeded)
        ref = orc.resize_linear(coarse.cpu().numpy(), w, h).astype(np.float64) * np.float64(np.float32(1.0 / ps))
        err = float(np.abs(out - ref).max())
        bar = 4 * float(np.spacing(np.float32(np.abs(ref).max())))
        print("[flow-forms] A driver | %s winsize %d solve=0 (%s) | %dx%d | ps%g | max err %.3g | bar %.3g | max |flow| %.3g" % (
            "gauss" if flags else "box", winsize, _name(f), w, h, ps, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 1 and err <= bar


@pytest.mark.parametrize("flags", [0, GAUSSIAN])
@pytest.mark.parametrize("kind", ["smooth", "outliers", "whole"])
def test_driver_synthetic_initial_flow_at_levels_0(ctx, orc, kind, flags):
    """levels = 0 with OPTFLOW_USE_INITIAL_FLOW: the field reaches k_flow_iter_w3 unchanged; iterations 1 (caller rows out) and
    2 (buffer A, then the caller's rows)."""
    missed = []
    with options(ctx, exact=0, fuse_iters=0):
        for (w, h) in fr.SIZES:
            init = fr.FIELDS[kind](w, h, seed=5)
            assert torch.equal(ctx.stage_initial_flow(init, 0.5, 0).cpu(), torch.as_tensor(init))
            f = expect_form("w3", w, h, 1, 3, flags, solve=1, in_mode=1)
            for iters in (1, 2):
                p = dict(pyr_scale=0.5, levels=0, winsize=3, iterations=iters, poly_n=15, poly_sigma=1.2, flags=flags | USE_INITIAL_FLOW)
                out = _two_image_call(ctx, _clip((w, h), 2), p, init).cpu().numpy()
                R0, R1 = _level_R(ctx, w, h, 0.5, 0)
                tag = "%s %s it%d" % ("gauss" if flags else "box", kind, iters)
                first = out if iters == 1 else ctx.debug_level_flow(w, h, 0.5, 0, 0).cpu().numpy()
                missed += check_launch(orc, "A driver", "w3 initial flow (%s)" % _name(f), tag, R0, R1, init, first, 3, flags)
                if iters == 2:
                    missed += check_launch(orc, "A driver", "w3 previous in (%s)" % _name(f), tag + ", caller stride", R0, R1, first, out, 3, flags)
    assert not missed, "\n".join(missed)


# ============================================================================ Part B: fused and chained forms, same bits
def _clip_call(ctx, clip, p, pad=0):
    T, h, w = clip.shape
    buf = torch.full((T - 1, h, w + pad, 2), 7.0, dtype=torch.float32, device="cuda")
    out = ctx.farneback_clip(clip, buf[:, :, :w], **p)
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((buf[:, :, w:] == 7.0).all()) and bool(torch.isfinite(out).all())
    return out.clone()


@pytest.mark.parametrize("flags", [0, GAUSSIAN])
def test_driver_clip_call_pairs_beyond_the_first(ctx, orc, flags):
    """A clip call of three pairs, levels = 0, iterations = 2, one launch per iteration: pair z reads ring entries z and z + 1,
    its first launch writes pair z of buffer A (rcflow_debug_level_flow's pair offset), its second the caller's field z."""
    missed = []
    for (w, h) in ((131, 71), (57, 41)):
        clip = torch.as_tensor(_clip((w, h), 4, seed=15)).cuda()
        p = dict(pyr_scale=0.5, levels=0, winsize=3, iterations=2, poly_n=15, poly_sigma=1.2, flags=flags)
        f = expect_form("w3", w, h, 3, 3, flags, solve=1, in_mode=0)
        assert f["grid_y"] == 3
        with options(ctx, exact=0, fuse_iters=0, chain=1):
            out = _clip_call(ctx, clip, p, PAD).cpu().numpy()
            R = [ctx.debug_level_R(w, h, 0.5, 0, t).cpu().numpy() for t in range(4)]
            first = [ctx.debug_level_flow(w, h, 0.5, 0, 0, pair=z).cpu().numpy() for z in range(3)]
        assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])
        for z in (1, 2):
            tag = "%s clip pair %d" % ("gauss" if flags else "box", z)
            missed += check_launch(orc, "A driver", "w3 zeros in (%s)" % _name(f), tag, R[z], R[z + 1], None, first[z], 3, flags)
            missed += check_launch(orc, "A driver", "w3 previous in (%s)" % _name(f), tag + ", caller stride", R[z], R[z + 1], first[z], out[z], 3, flags)
    assert not missed, "\n".join(missed)


def _fused_launches(iters):
    """The first iteration of every fused (two-iteration) launch of a scale with `iters` iterations; the first of them reads the
    scale's flow in, the others the previous launch's field."""
    return list(range(0, iters - 1, 2))


@pytest.mark.parametrize("flags", [0, GAUSSIAN])
@pytest.mark.parametrize("pairs,nit", [(4, 2), (5, 3), (10, 4)])
def test_fused_forms_same_bits_as_single_launches(ctx, pairs, nit, flags):
    """333 x 251 (and 332 x 252 for the exact 2:1 flow in), 4 / 5 / 10 pairs = 432 / 540 / 1080 blocks: the 28 x 12, 28 x 20 and
    28 x 28 forms without chains, then tile chains of 2, 3 and 8 forced (always 28 x 28).  levels = 0: flow in zeros, then the
    previous iteration; levels = 1: the coarser scale at scale 0."""
    for (w, h) in ((333, 251), (332, 252)):
        clip = torch.as_tensor(_clip((w, h), pairs + 1, seed=12)).cuda()
        assert ((w + 27) // 28) * ((h + 27) // 28) * pairs == 108 * pairs
        for levels in (0, 1):
            for iters in (2, 3, 4, 5):
                p = dict(pyr_scale=0.5, levels=levels, winsize=3, iterations=iters, poly_n=15, poly_sigma=1.2, flags=flags)
                with options(ctx, exact=0, fuse_iters=0, chain=1):
                    for mode in ((2 if levels else 0), 1):
                        expect_form("w3", w, h, pairs, 3, flags, solve=1, in_mode=mode, fuse=1, chain=1)
                    want = _clip_call(ctx, clip, p, PAD if iters == 2 else 0)
                for mode in [(2 if levels else 0)] + [1] * (len(_fused_launches(iters)) - 1):
                    f = expect_form("rrc", w, h, pairs, 3, flags, solve=1, in_mode=mode, fuse=2, chain=1)
                    assert (f["nit"], f["th"], f["groups"]) == (nit, 8 * nit - 4, 0) and f["interior"] > 0
                if levels:
                    # scale 1 (167 x 126 or 166 x 126: 30 tiles) is the 28 x 12 form for 4, 5 and 10 pairs alike
                    _, cw, ch = ctx.level_geometry(w, h, 0.5, 1, 1)
                    f1 = expect_form("rrc", cw, ch, pairs, 3, flags, solve=1, in_mode=0, fuse=2, chain=1)
                    assert (cw, ch) in ((167, 126), (166, 126)) and (f1["nit"], f1["groups"]) == (2, 0) and f1["interior"] > 0
                with options(ctx, exact=0, chain=1):
                    got = _clip_call(ctx, clip, p, PAD if iters == 2 else 0)
                assert torch.equal(got, want), "fused 28x%d, %dx%d levels %d iterations %d" % (8 * nit - 4, w, h, levels, iters)
                if iters in (2, 5) or levels == 1:
                    for chain in (2, 3, 8):
                        f = expect_form("rrc", w, h, pairs, 3, flags, solve=1, in_mode=1, fuse=2, chain=chain, ablate=FORCE_CHAIN)
                        assert f["nit"] == 4 and f["groups"] >= 2 and f["grid_y"] == f["groups"] < pairs
                        with options(ctx, exact=0, chain=chain, ablate=FORCE_CHAIN):
                            got = _clip_call(ctx, clip, p)
                        assert torch.equal(got, want), "chains of %d, %dx%d levels %d iterations %d" % (chain, w, h, levels, iters)


@pytest.mark.parametrize("size", fr.SIZES_FUSED, ids=lambda s: "%dx%d" % s)
def test_fused_forms_same_bits_at_the_tile_edge_sizes(ctx, size):
    """Three pairs at every size from 27 x 29 up (28 x 12 form; scale 1 exists from 64 x 64 on), both windows, 2 to 4 iterations,
    caller rows of w + 13 pixels, without chains and with chains of 2 forced (groups of 2 and 1 pairs, 28 x 28 form)."""
    w, h = size
    clip = torch.as_tensor(_clip((w, h), 4, seed=13)).cuda()
    for flags in (0, GAUSSIAN):
        for iters in (2, 3, 4):
            p = dict(pyr_scale=0.5, levels=1, winsize=3, iterations=iters, poly_n=15, poly_sigma=1.2, flags=flags)
            with options(ctx, exact=0, fuse_iters=0, chain=1):
                want = _clip_call(ctx, clip, p, PAD)
            f = expect_form("rrc", w, h, 3, 3, flags, solve=1, in_mode=2 if ctx.level_geometry(w, h, 0.5, 1, 0)[0] else 0, fuse=2, chain=1)
            assert (f["nit"], f["groups"]) == (2, 0)
            with options(ctx, exact=0, chain=1):
                got = _clip_call(ctx, clip, p, PAD)
            assert torch.equal(got, want), "fused, %s iterations %d" % ("gauss" if flags else "box", iters)
            f = expect_form("rrc", w, h, 3, 3, flags, solve=1, in_mode=1, fuse=2, chain=2, ablate=FORCE_CHAIN)
            assert (f["nit"], f["groups"], f["grid_y"]) == (4, 2, 2), f
            with options(ctx, exact=0, chain=2, ablate=FORCE_CHAIN):
                got = _clip_call(ctx, clip, p, PAD)
            assert torch.equal(got, want), "chain of 2, %s iterations %d" % ("gauss" if flags else "box", iters)


@pytest.mark.parametrize("size,nit", [((333, 251), 2), ((700, 600), 3), ((1000, 800), 4)])
def test_fused_forms_same_bits_on_large_displacement_initial_flow(ctx, size, nit):
    """levels = 0, OPTFLOW_USE_INITIAL_FLOW: the 2 % outliers of 3..40 px and the whole-pixel field reach the fused kernel's first
    M evaluation (flow-in mode 1), from border tiles and interior ones -- the |flow| >= D redo from global memory of
    rc_rr_matrices and rc_gather_window.  One pair: 108, 550 and 1044 blocks are the 28 x 12, 28 x 20 and 28 x 28 forms."""
    w, h = size
    clip = _clip((w, h), 2, seed=14)
    f = expect_form("rrc", w, h, 1, 3, 0, solve=1, in_mode=1, fuse=2, chain=8)
    assert (f["nit"], f["groups"]) == (nit, 0) and f["interior"] > 0 and f["interior"] < f["tiles_x"] * f["tiles_y"]
    for kind in ("outliers", "whole"):
        init = fr.FIELDS[kind](w, h, seed=7)
        for flags in (0, GAUSSIAN):
            for iters in (2, 3, 4):
                p = dict(pyr_scale=0.5, levels=0, winsize=3, iterations=iters, poly_n=15, poly_sigma=1.2, flags=flags | USE_INITIAL_FLOW)
                with options(ctx, exact=0, fuse_iters=0):
                    want = _two_image_call(ctx, clip, p, init).clone()
                with options(ctx, exact=0):
                    got = _two_image_call(ctx, clip, p, init).clone()
                assert bool(torch.isfinite(want).all()) and torch.equal(got, want), (kind, flags, iters)
