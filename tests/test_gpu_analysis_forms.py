"""The analysis kernels in the forms a 1080p caller and bench.py launch, held to the CPU oracle.

tests/test_gpu_analysis.py compares every analysis row with the oracle in its shortest form: one field per launch, one
round of the histogram kernel's item loop, one pass of the grid-stride loops.  Here:

A. rcflow_histogram_clip_dev (count > 1, a frame stride, blockIdx.y as the frame index) against the oracle's
   flow_to_polar + create_histogram applied cumulatively field by field, with the launch sized -- through option
   "hist_blocks" and the frame -- so that k_polar_hist_rows makes 1, 2, 3, 4 and 5 rounds in its plain and its general form:
   the reload of the first register set (rounds >= 3), the odd-round tail, the plain form's dummy loads past the last round,
   the carry of the (row group, pair) advance, a span that is no power of two and one below a row.  Every case computes its
   round count from the launcher's arithmetic (analysis_kernels.hip, histogram_clip) and asserts the intended value first:
   should those constants change, the case fails with "premise gone" instead of quietly testing one round.
B. every launch sized by grid_for beyond its cap of 2048 blocks x 256 threads, at 1061 x 541 (574 001 pixels: two passes of
   the grid-stride loop, the second partial; (w - 20)(h - 20) = 542 361 for the shear kernel), dense and with padded rows.

Counts, thresholds, classes, masks, particles and colours are compared with np.array_equal; the three post-ops keep the
stated tolerances of test_flow_postops, the one of subtructMeanMagnitude worked out for this field (see that test).
"""
import numpy as np
import pytest
import torch

from _dev import Padded, same_bits
from ripcurrents_amd.api import Context, HistState

pytestmark = pytest.mark.gpu

# the launcher's constants (analysis_kernels.hip: RC_BLOCK, grid_for, histogram_clip; include/rcflow.h, rcflow_histogram_clip_dev)
BLOCK, GRID_CAP, HIST_BLOCKS_DEFAULT, HIST_BLOCKS_FLOOR = 256, 2048, 8192, 8
CAP_ITEMS = GRID_CAP * BLOCK                  # 524 288: what one pass of a capped grid covers
FSENT, BSENT = 123.5, 0xA5                    # sentinels of padded float / byte outputs
HSENT = 0.777                                 # sentinel around a flow view: (0.777, 0.777) is a counted vector (bin 21, direction 4)


def _hist_launch(w, h, T, hist_blocks):
    """(items, blocks per field, span, rounds) of the histogram launch for T fields of w x h: items of 2 x 4 pixels,
    grid_for's cap, cap = max(8, (hist_blocks or 8192) // T), span = blocks * 256 items per round."""
    items = ((w + 1) // 2) * ((h + 3) // 4)
    nb = min(max(1, -(-items // BLOCK)), GRID_CAP)
    nb = min(nb, max(HIST_BLOCKS_FLOOR, (hist_blocks or HIST_BLOCKS_DEFAULT) // T))
    span = nb * BLOCK
    return items, nb, span, -(-items // span)


def _plain(dev):
    """The launcher's test for the kernel's plain form, on a [T, h, w, 2] float32 device view."""
    T, h, w = dev.shape[:3]
    step, stride = dev.stride(1) * 4, dev.stride(0) * 4
    return ((w & 1) | (h & 3)) == 0 and ((dev.data_ptr() | step | (stride if T > 1 else 0)) & 15) == 0 and h * step < 1 << 32


def _smooth(w, h, seed, scale=1.0):
    """The smooth part of test_gpu_analysis._flow_field: the value range of real flows."""
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = np.empty((h, w, 2), np.float32)
    f[..., 0] = scale * (0.8 * np.sin(xs / 37.0) + 0.3 * np.cos(ys / 11.0) + 0.05 * rng.randn(h, w))
    f[..., 1] = scale * (0.6 * np.cos(xs / 23.0 + ys / 31.0) + 0.05 * rng.randn(h, w))
    return f


def _edge_hazards(rng, n):
    """n vectors, the hazards of test_histogram_key_on_bin_edges in turn: magnitudes on k / 20; directions on multiples of 10
    degrees nudged by up to 3 ulps; both at once; zeros, -0 and denormals; magnitudes beyond bin 49; +-Inf and NaN."""
    with np.errstate(all="ignore"):
        th = rng.rand(n) * 2 * np.pi
        k = rng.randint(1, 51, n) / 20.0
        m = rng.randint(0, 37, n) * (np.pi / 18)
        r = rng.rand(n) * 2.6
        v = np.zeros((6, n, 2), np.float32)
        v[0, :, 0] = k * np.cos(th); v[0, :, 1] = k * np.sin(th)
        v[1, :, 0] = r * np.cos(m); v[1, :, 1] = r * np.sin(m)
        v[1] = (v[1].view(np.int32) + rng.randint(-3, 4, (n, 2)).astype(np.int32)).view(np.float32)
        v[2, :, 0] = k * np.cos(m); v[2, :, 1] = k * np.sin(m)
        tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)
        v[3] = tiny[rng.randint(0, len(tiny), (n, 2))]
        far = np.array([2.5, -2.5, 2.55, 9.0, -9.0, 1e10, 1e20, 3e38], np.float32)
        v[4, :, 0] = far[rng.randint(0, len(far), n)]
        v[4, :, 1] = np.array([0.0, 1.0, -2.5, 1e20], np.float32)[rng.randint(0, 4, n)]
        wild = np.array([np.inf, -np.inf, np.nan], np.float32)
        v[5, :, 0] = wild[rng.randint(0, 3, n)]
        v[5, :, 1] = np.array([np.inf, -np.inf, np.nan, 0.3, 0.0, -1.0], np.float32)[rng.randint(0, 6, n)]
    out = v[np.arange(n) % 6, np.arange(n)]
    swap = (np.arange(n) // 6) % 2 == 1                  # every other one with x and y exchanged: the far / wild value in either component
    out[swap] = out[swap][:, ::-1]
    return out


def _hazard_positions(rng, w, h, frac):
    """Distinct pixel indices: seeded random positions over the whole frame, the whole last row and the whole last column."""
    n = w * h
    pos = rng.randint(0, n, max(64, int(frac * n)))
    return np.unique(np.concatenate([pos, (h - 1) * w + np.arange(w), np.arange(h) * w + (w - 1)]))


def _assert_every_round_is_hit(pos, w, h, T, hist_blocks):
    """Premise: the hazards lie in items of every round, in the last row and in the last column."""
    items, nb, span, rounds = _hist_launch(w, h, T, hist_blocks)
    y, x = pos // w, pos % w
    item = (y // 4) * ((w + 1) // 2) + x // 2
    assert np.array_equal(np.unique(item // span), np.arange(rounds)), "premise gone: hazards miss a round"
    assert (y == h - 1).any() and (x == w - 1).any() and item.max() == items - 1, "premise gone: hazards miss the last row / column"


def _clip(w, h, T, seed, hist_blocks, frac=0.02):
    """T different fields -- the smooth field at another seed and scale per frame -- each with hazards scattered over it."""
    flows = np.empty((T, h, w, 2), np.float32)
    for t in range(T):
        rng = np.random.RandomState(1000 * seed + t)
        flows[t] = _smooth(w, h, 10 * seed + t, scale=0.6 + 0.45 * t)
        pos = _hazard_positions(rng, w, h, frac)
        flows[t].reshape(-1, 2)[pos] = _edge_hazards(rng, pos.size)
        _assert_every_round_is_hit(pos, w, h, T, hist_blocks)
    return flows


def _oracle_add(orc, flows, ost):
    """The oracle, cumulatively field by field (ripcurrents.cpp:305-330 per frame)."""
    with np.errstate(all="ignore"):
        for f in flows:
            orc.create_histogram(orc.flow_to_polar(f), ost)
    return ost


def _assert_state(st, ost, what):
    assert np.array_equal(st.hist, ost.hist), what + ": hist"
    assert np.array_equal(st.hist2d, ost.hist2d), what + ": hist2d (%d cells differ)" % (st.hist2d != ost.hist2d).sum()
    assert st.histsum == ost.histsum.value, what + ": histsum"
    assert np.array_equal(st.histsum2d, ost.histsum2d), what + ": histsum2d"
    assert np.float32(st.UPPER) == np.float32(ost.UPPER), what + ": UPPER"
    assert np.array_equal(st.UPPER2d, ost.UPPER2d, equal_nan=True), what + ": UPPER2d"
    assert np.array_equal(st.prop_above_upper, ost.prop_above_upper, equal_nan=True), what + ": prop_above_upper"


def _check_clip(ctx, orc, dev, backing, flows):
    """One clip call on a reset slot == the oracle after T fields; a second one without a reset == the oracle after 2 T (the
    fold cleared the partial tables); after histogram_reset, T single calls give the words of the one clip call; the input
    (`backing`: the whole buffer `dev` is a view of) is unchanged."""
    T, h, w = dev.shape[:3]
    before = backing.clone()
    ctx.analysis_reset(w, h)
    ctx.histogram_accumulate_clip(dev)
    ctx.thresholds()
    st = ctx.histogram_read()
    words = ctx.histogram_words().cpu().numpy().copy()
    ost = _oracle_add(orc, flows, orc.HistState())
    _assert_state(st, ost, "one clip call")
    assert st.histsum > 0.5 * T * w * h and st.histsum < T * w * h          # most pixels counted, the far and wild ones not
    ctx.histogram_accumulate_clip(dev)
    ctx.thresholds()
    _assert_state(ctx.histogram_read(), _oracle_add(orc, flows, ost), "a second clip call without a reset")
    ctx.histogram_reset()
    for t in range(T):
        ctx.histogram_accumulate(dev[t])
    ctx.thresholds()
    assert np.array_equal(ctx.histogram_words().cpu().numpy(), words), "T single calls against one clip call"
    st1 = ctx.histogram_read()
    assert np.float32(st1.UPPER) == np.float32(st.UPPER) and np.array_equal(st1.UPPER2d, st.UPPER2d, equal_nan=True)
    assert same_bits(_np(backing), _np(before)), "the input was written"


# ---------------------------------------------------------------------------- A: sizing
#          name                w     h    T  hist_blocks  plain  rounds
SIZING = [("one_full_round", 512, 32, 2, 8, True, 1),        # span == total
          ("two", 512, 64, 3, 8, True, 2),                   # even, no reload of the first register set
          ("three_full", 512, 96, 2, 8, True, 3),            # the reload, the odd tail
          ("three_partial", 512, 88, 5, 8, True, 3),         # last round 3/4 full: dummy loads
          ("four", 512, 128, 2, 8, True, 4),                 # the bench launch's count, exactly full
          ("five", 512, 136, 5, 8, True, 5),                 # odd, partial
          ("carry", 250, 200, 3, 8, True, 4),                # w2 = 125, span = 16 * 125 + 48: the pair index carries
          ("carry_general", 251, 203, 3, 8, False, 4),       # odd width and ragged height with the carry
          ("nine_blocks", 250, 200, 3, 27, True, 3)]         # cap 9, span 2304: no power of two


@pytest.mark.parametrize("name,w,h,T,hist_blocks,plain,rounds", SIZING, ids=[c[0] for c in SIZING])
def test_clip_histogram_rounds(ctx, orc, name, w, h, T, hist_blocks, plain, rounds):
    """The clip histogram with 1 .. 5 rounds of the item loop per thread, against the cumulative oracle."""
    items, nb, span, got_rounds = _hist_launch(w, h, T, hist_blocks)
    assert got_rounds == rounds, "premise gone: %s makes %d rounds (%d items, %d blocks), not %d" % (name, got_rounds, items, nb, rounds)
    if name == "one_full_round":
        assert span == items, "premise gone"
    if name == "three_partial":
        assert 4 * (items - 2 * span) == 3 * span, "premise gone"
    if name.startswith("carry"):
        w2 = (w + 1) // 2
        assert span // w2 >= 1 and span % w2 > 0, "premise gone"      # dg >= 1 and dx > 0: xx + dx passes w2 for the lanes with xx >= w2 - dx
        assert name != "carry" or (w2, span) == (125, 16 * 125 + 48), "premise gone"
    if name == "nine_blocks":
        assert nb == 9, "premise gone"
    flows = _clip(w, h, T, len(name), hist_blocks)
    dev = torch.as_tensor(flows).cuda()
    assert _plain(dev) == plain, "premise gone: the launcher takes the other form"
    ctx.set_option("hist_blocks", hist_blocks)
    try:
        _check_clip(ctx, orc, dev, dev, flows)
    finally:
        ctx.set_option("hist_blocks", 0)


def test_clip_histogram_span_below_a_row(ctx, orc):
    """4100 x 12: a row of 2050 items is longer than the span of 2048, so the row-group advance per round is 0 and only the
    pair index moves; four rounds, the last holding 6 items.  (A context of its own: the shared one, asked for here so that
    the test skips where there is no GPU, stops at 3840 columns.)"""
    w, h, T, hist_blocks = 4100, 12, 2, 8
    items, nb, span, rounds = _hist_launch(w, h, T, hist_blocks)
    assert rounds == 4 and span < (w + 1) // 2 and items - 3 * span == 6, "premise gone"
    flows = _clip(w, h, T, 77, hist_blocks)
    own = Context(4104, 16)
    try:
        dev = torch.as_tensor(flows).cuda()
        assert _plain(dev), "premise gone"
        own.set_option("hist_blocks", hist_blocks)
        _check_clip(own, orc, dev, dev, flows)
    finally:
        own.close()


def test_clip_histogram_bench_shape(ctx, orc):
    """32 fields of 1920 x 1080 with default options: the launch bench.py times (cap 256 blocks per field, span 65 536 of
    259 200 items: four rounds, the only way to four rounds without an option).  The fields are built on the device -- one
    smooth base field times a scale per frame, hazards scattered into each -- and downloaded once for the oracle (0.03 s
    of oracle per field and pass)."""
    w, h, T = 1920, 1080, 32
    items, nb, span, rounds = _hist_launch(w, h, T, 0)
    assert (nb, span, rounds) == (256, 65536, 4), "premise gone: the bench launch is %d blocks, %d rounds" % (nb, rounds)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device="cuda"), torch.arange(w, dtype=torch.float32, device="cuda"),
                            indexing="ij")
    noise = 0.05 * torch.randn((h, w, 2), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    base = torch.stack([0.8 * torch.sin(xs / 37.0) + 0.3 * torch.cos(ys / 11.0), 0.6 * torch.cos(xs / 23.0 + ys / 31.0)], -1) + noise
    scales = torch.linspace(0.5, 2.0, T, device="cuda")
    dev = (base[None] * scales[:, None, None, None]).contiguous()
    for t in range(T):
        rng = np.random.RandomState(500 + t)
        pos = _hazard_positions(rng, w, h, 0.01)
        _assert_every_round_is_hit(pos, w, h, T, 0)
        dev[t].view(-1, 2)[torch.as_tensor(pos).cuda()] = torch.as_tensor(_edge_hazards(rng, pos.size)).cuda()
    flows = dev.cpu().numpy()
    assert _plain(dev), "premise gone"
    ctx.set_option("hist_blocks", 0)
    _check_clip(ctx, orc, dev, dev, flows)


# ---------------------------------------------------------------------------- A: layouts
def _view(kind, T, h, w):
    """(backing buffer filled with the sentinel vector, [T, h, w, 2] view into it) for one layout."""
    full = lambda *shape: torch.full(shape, HSENT, dtype=torch.float32, device="cuda")
    if kind in ("odd_width", "ragged_height"):
        big = full(T, (h + 3) // 4 * 4, (w + 1) // 2 * 2, 2)        # the rest of the last items is sentinel
        return big, big[:, :h, :w]
    if kind == "unaligned_base":
        big = full(T, h, w + 2, 2)
        return big, big[:, :, 1:w + 1]
    if kind == "unaligned_pitch":
        big = full(T, h, w + 1, 2)
        return big, big[:, :, :w]
    assert kind == "unaligned_frame_stride"
    stride = h * w * 2 + 2                                          # one float2 between the frames
    big = full(4 + T * stride)
    return big, torch.as_strided(big, (T, h, w, 2), (stride, w * 2, 2, 1), 4)


#           name                          kind                      w    h    T  plain
LAYOUTS = [("odd_width", "odd_width", 511, 136, 3, False),
           ("ragged_height_134", "ragged_height", 512, 134, 3, False),
           ("ragged_height_133", "ragged_height", 512, 133, 3, False),
           ("unaligned_base", "unaligned_base", 512, 136, 3, False),
           ("unaligned_pitch", "unaligned_pitch", 512, 136, 3, False),
           ("unaligned_frame_stride", "unaligned_frame_stride", 512, 136, 3, False),
           ("one_frame_stride_ignored", "unaligned_frame_stride", 512, 136, 1, True)]


@pytest.mark.parametrize("name,kind,w,h,T,plain", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_clip_histogram_layouts(ctx, orc, name, kind, w, h, T, plain):
    """Five rounds on views into sentinel-filled buffers: every layout that sends the launch to the general form -- the last
    being a frame stride of 8 mod 16 bytes under an aligned base and pitch, where only frames 1, 3, ... have misaligned rows
    and which no single-field call can reach -- and one field through the clip entry, whose frame stride is not looked at."""
    hist_blocks = 8
    assert _hist_launch(w, h, T, hist_blocks)[3] == 5, "premise gone: not five rounds"
    flows = _clip(w, h, T, 40 + len(name), hist_blocks)
    big, dev = _view(kind, T, h, w)
    dev.copy_(torch.as_tensor(flows).cuda())
    step, stride = dev.stride(1) * 4, dev.stride(0) * 4
    if kind == "unaligned_base":
        assert dev.data_ptr() % 16 == 8 and step % 16 == 0 and stride % 16 == 0, "premise gone"
    elif kind == "unaligned_pitch":
        assert dev.data_ptr() % 16 == 0 and step % 16 == 8 and stride % 16 == 0, "premise gone"
    elif kind == "unaligned_frame_stride":
        assert dev.data_ptr() % 16 == 0 and step % 16 == 0 and stride % 16 == 8, "premise gone"
    else:
        assert dev.data_ptr() % 16 == 0 and step % 16 == 0 and stride % 16 == 0, "premise gone"
    assert _plain(dev) == plain, "premise gone: the launcher takes the other form"
    ctx.set_option("hist_blocks", hist_blocks)
    try:
        _check_clip(ctx, orc, dev, big, flows)
    finally:
        ctx.set_option("hist_blocks", 0)


# ---------------------------------------------------------------------------- B: past the cap of grid_for
BW, BH = 1061, 541
_REFS = {}


def _ref(key, make):
    """An oracle result, computed once and shared by the dense and the padded case (never written by a test)."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _second_pass_positions(rng, w, h, count):
    """Pixel indices over the whole frame, a share of them forced beyond the first pass of a capped grid, the last pixel too."""
    n = w * h
    assert n > CAP_ITEMS and n < 2 * CAP_ITEMS, "premise gone: not two passes, the second partial"
    pos = np.unique(np.concatenate([rng.randint(0, n, count), rng.randint(CAP_ITEMS, n, count // 4), [CAP_ITEMS - 1, CAP_ITEMS, n - 1]]))
    assert (pos >= CAP_ITEMS).sum() >= count // 8
    return pos


def _finite_field(seed, scale=1.0, w=BW, h=BH):
    """test_gpu_analysis._flow_field at this size: smooth, with exact zeros, an angle that rounds to 360, -0, magnitudes
    beyond the last bin and axis-aligned vectors scattered over both passes."""
    def make():
        rng = np.random.RandomState(7000 + seed)
        f = _smooth(w, h, seed, scale)
        pos = _second_pass_positions(rng, w, h, 20000)
        ex = np.array([[0.0, 0.0], [3.0, -1e-9], [-0.0, 0.7], [9.0, 9.0], [0.0, -1.3], [-2.0, 0.0]], np.float32)
        f.reshape(-1, 2)[pos] = ex[np.arange(pos.size) % len(ex)]
        return f
    return _ref(("finite", seed, scale, w, h), make)


def _wild_field(seed, w=BW, h=BH):
    """test_gpu_analysis._adversarial_flow at this size: ordinary vectors mixed, everywhere, with zeros, denormals, magnitudes
    exactly on the 0.2 / 0.5 class thresholds, huge values, Inf and NaN; the histogram's edge hazards in both passes as well."""
    def make():
        n = w * h
        rng = np.random.RandomState(seed)
        ex = np.array([0.0, -0.0, 1e-45, 1e-39, 1e-20, 0.2, 0.5, 0.05, 1.0, 1.7, 2.5, 1e10, 3e38, np.inf, -np.inf, np.nan], np.float32)
        f = (rng.randn(n, 2) * 0.8).astype(np.float32)
        for c in (0, 1):
            idx = rng.rand(n) < 0.3
            f[idx, c] = ex[rng.randint(0, len(ex), idx.sum())]
        k = rng.rand(n) < 0.1
        th = rng.rand(k.sum()) * 2 * np.pi
        r = np.where(rng.rand(k.sum()) < 0.5, 0.2, 0.5)
        f[k, 0] = (r * np.cos(th)).astype(np.float32)
        f[k, 1] = (r * np.sin(th)).astype(np.float32)
        pos = _second_pass_positions(rng, w, h, 20000)
        f[pos] = _edge_hazards(rng, pos.size)
        assert not np.isfinite(f[CAP_ITEMS:]).all() and (f[CAP_ITEMS:] == 0.5).any()
        return f.reshape(h, w, 2)
    return _ref(("wild", seed, w, h), make)


def _flow_view(f, pad):
    """The field on the device with rows padded by `pad` sentinel pixels."""
    return Padded.of(f, pad, FSENT)


def _zeroed(shape, dtype, pad, fill):
    """An output of zeros in rows `pad` pixels longer and `fill` there."""
    p = Padded.empty(shape, dtype, pad, fill)
    p.view.zero_()
    return p


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _np(t):
    return t.cpu().numpy()


def _wild_hist(orc):
    """The oracle's histogram state of the wild field (the thresholds classify and advection take from the slot)."""
    def make():
        with np.errstate(all="ignore"):
            polar = orc.flow_to_polar(_wild_field(5))
            ost = orc.HistState()
            orc.create_histogram(polar, ost)
        return polar, ost
    return _ref("wild_hist", make)


PADS = pytest.mark.parametrize("pad", [0, 3], ids=["dense", "padded_rows"])


@PADS
def test_capped_classify_accumulate(ctx, orc, pad):
    """k_classify_accumulate over two passes: framecounts 1, 31, 32 and 40, all four outputs and the accumulator."""
    w, h = BW, BH
    f = _wild_field(5)
    polar, ost = _wild_hist(orc)

    def make():
        rows = []
        acc = np.zeros((h, w, 3), np.float32)
        with np.errstate(all="ignore"):
            for fc in (1, 31, 32, 40):
                wc, acc2, p2 = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32), polar.copy()
                orc.create_flow(p2, wc, acc2, ost.UPPER, 0.5, 0.2, ost.UPPER2d)
                out, mask = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.uint8)
                orc.create_accumulationbuffer(acc, acc2, out, mask, fc)
                rows.append((fc, wc, p2, out, mask, acc[..., 0].copy()))
        return rows
    rows = _ref("classify", make)
    fl = _flow_view(f, pad)
    fv, fbefore = fl.view, fl.base.clone()
    ctx.analysis_reset(w, h)
    st = HistState()
    ctx.create_histogram(fv, st)
    _assert_state(st, ost, "histogram of the field")
    for fc, wc, p2, out, mask, acc in rows:
        o = {n: Padded.empty((h, w, 3), torch.float32, pad, FSENT) for n in ("polar", "waterclass", "out")}
        o["outmask"] = Padded.empty((h, w), torch.uint8, pad, BSENT)
        ctx._bind(0)
        args = []
        for n in ("polar", "waterclass", "out", "outmask"):
            args += [o[n].view.data_ptr(), o[n].view.stride(0) * o[n].view.element_size()]
        assert ctx._lib.rcflow_classify_accumulate_dev(ctx._h, 0, fv.data_ptr(), fv.stride(0) * 4, w, h, fc, 0.5, 0.2, *args) == 0
        assert _eq(_np(o["waterclass"].view), wc) and _eq(_np(o["polar"].view), p2), fc
        assert _eq(_np(o["out"].view), out) and _eq(_np(o["outmask"].view), mask), fc
        assert _eq(ctx.accumulator(w, h), acc), fc
        for n in ("polar", "waterclass", "out", "outmask"):
            o[n].check(n)
    assert rows[-1][5].reshape(-1)[CAP_ITEMS:].max() >= 2.0          # the accumulator did count in the second pass
    assert same_bits(_np(fl.base), _np(fbefore))


@PADS
def test_capped_streamline_field(ctx, orc, pad):
    """k_advect_field over two passes: three calls of two iterations, with an explicit UPPER and with the slot's."""
    w, h = BW, BH
    f = _wild_field(5)
    _, ost = _wild_hist(orc)

    def make():
        res = []
        with np.errstate(all="ignore"):
            for upper in (1.7, ost.UPPER):
                pt, dist = np.zeros((h, w, 2), np.float32), np.zeros((h, w), np.float32)
                for _ in range(3):
                    orc.streamline_field(pt, dist, f, 2.0, 2, upper)
                res.append((pt, dist))
        return res
    (pt_e, dist_e), (pt_s, dist_s) = _ref("streamline", make)
    fl = _flow_view(f, pad)
    fv = fl.view
    ctx.analysis_reset(w, h)
    for _ in range(3):
        ctx.streamline_field(fv, 2.0, 2, UPPER=1.7)
    gpt, gdist = ctx.streamline_field_state(w, h)
    assert _eq(gpt, pt_e) and _eq(gdist, dist_e)
    assert np.nanmax(np.abs(pt_e.reshape(-1, 2)[CAP_ITEMS:])) > 1.0
    ctx.analysis_reset(w, h)
    st = HistState()
    ctx.create_histogram(fv, st)
    assert np.float32(st.UPPER) == np.float32(ost.UPPER) and st.UPPER < 100.0
    for _ in range(3):
        ctx.streamline_field(fv, 2.0, 2)                  # UPPER < 0: the slot's
    gpt, gdist = ctx.streamline_field_state(w, h)
    assert _eq(gpt, pt_s) and _eq(gdist, dist_s)
    fl.check("the field")


@PADS
def test_capped_get_delta_field(ctx, orc, pad):
    w, h = BW, BH
    f = _wild_field(5)

    def make():
        ref = np.zeros((h, w, 2), np.float32)
        with np.errstate(all="ignore"):
            for _ in range(3):
                orc.get_delta_field(ref, f, 2.0, 1.8)
        return ref
    ref = _ref("delta", make)
    fl, particles = _flow_view(f, pad), _zeroed((h, w, 2), torch.float32, pad, FSENT)
    fv, pt = fl.view, particles.view
    ctx._bind(0)
    for _ in range(3):
        assert ctx._lib.rcflow_get_delta_field_dev(ctx._h, 0, pt.data_ptr(), pt.stride(0) * 4, fv.data_ptr(), fv.stride(0) * 4, w, h, 2.0, 1.8) == 0
    assert _eq(_np(pt), ref) and np.nanmax(np.abs(ref.reshape(-1, 2)[CAP_ITEMS:])) > 1.0
    particles.check("the particles")
    fl.check("the field")


def test_capped_window_mean(ctx, orc):
    """k_window_mean over 1 148 002 floats: three passes, three updates."""
    w, h = BW, BH
    avg, slot = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 2), np.float32)
    davg, dslot = torch.as_tensor(avg).cuda(), torch.as_tensor(slot).cuda()
    assert avg.size > 2 * CAP_ITEMS, "premise gone"
    for t in range(3):
        cur = _finite_field(20 + t)
        orc.window_mean_update(avg, slot, cur, 10)
        ctx.window_mean(davg, dslot, torch.as_tensor(cur).cuda(), 10)
    assert np.array_equal(_np(davg), avg) and np.array_equal(_np(dslot), slot)


@PADS
def test_capped_colouring(ctx, orc, pad):
    """k_flow_stats_partial with all 2048 partials handed to k_flow_stats_final, k_vector_to_color and k_shear_to_color over
    two passes: pixels and the returned maxima over two frames each."""
    import ctypes as C
    w, h = BW, BH
    assert (w - 20) * (h - 20) > CAP_ITEMS, "premise gone"

    def make():
        vec, shear = [], []
        md = mf = 0.0
        for t in range(2):
            ref, md = orc.vector_to_color(_finite_field(30 + t, 2.0), md)
            vec.append((ref, md))
        for t in range(2):
            ref, mf = orc.shear_rate_to_color(_finite_field(40 + t, 2.0), mf)
            shear.append((ref, mf))
        return vec, shear
    vec, shear = _ref("colour", make)
    gmd = C.c_float(0.0)
    for t in range(2):          # the first frame divides by max_displacement == 0 like the reference
        fl, picture = _flow_view(_finite_field(30 + t, 2.0), pad), _zeroed((h, w, 3), torch.uint8, pad, BSENT)
        fv, hsv = fl.view, picture.view
        ctx._bind(0)
        assert ctx._lib.rcflow_vector_to_color_dev(ctx._h, 0, fv.data_ptr(), fv.stride(0) * 4, w, h, hsv.data_ptr(), hsv.stride(0), C.byref(gmd)) == 0
        assert gmd.value == vec[t][1] and np.array_equal(_np(hsv), vec[t][0])
        picture.check("the picture")
        fl.check("the field")
    gmf = 0.0
    for t in range(2):
        fl, picture = _flow_view(_finite_field(40 + t, 2.0), pad), _zeroed((h, w, 3), torch.uint8, pad, BSENT)
        got, gmf = ctx.shearRateToColor(fl.view, gmf, hsv=picture.view)
        assert gmf == shear[t][1] and gmf > 0 and np.array_equal(_np(got), shear[t][0])
        picture.check("the picture")
        fl.check("the field")


# the oracle's mean magnitude of _finite_field(4, 1.2) against the float64 sum of the same magnitudes, measured on the CPU
MEAN_MAG_REF_ERR = 1.993e-5


@PADS
def test_capped_postops(ctx, orc, pad):
    """k_flow_stats_partial / final and k_flow_postop over two passes.  subtructAverage and stabilizer keep the bar of
    test_flow_postops (the mean in double on both sides: one ulp).  subtructMeanMagnitude: the oracle's mean is the
    reference's sequential float32 running sum, the kernel sums in double, so the two results differ by the error of that
    running sum.  Measured on the CPU for this field (574 001 pixels): the float32 running sum of the float32 magnitudes
    against their float64 sum is off by 1.993e-5 relative (means 0.934918344 and
    0.934936978; rebuilding the oracle's result from that float32 mean gives its bits, so it is the oracle's mean).  The bar is four times that, times the mean, plus
    1e-6 absolute for the roundings of the per-pixel arithmetic (values below 4: ulp 2.4e-7, a few operations)."""
    w, h = BW, BH
    f = _finite_field(4, 1.2)

    def make():
        refs = []
        for op in (orc.subtract_average, orc.stabilizer, orc.subtract_mean_magnitude):
            r = f.copy()
            op(r)
            refs.append(r)
        return refs
    ref_avg, ref_stab, ref_mm = _ref("postops", make)
    mag32 = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]).ravel()          # float32 operation by operation, as the oracle forms it
    mean64 = mag32.astype(np.float64).sum() / (w * h)
    rel = abs(float(np.cumsum(mag32, dtype=np.float32)[-1]) / (w * h) - mean64) / mean64
    assert abs(rel - MEAN_MAG_REF_ERR) <= 0.02 * MEAN_MAG_REF_ERR, "premise gone: the field's reference error is %.4g" % rel
    for gpu, ref, bar in ((ctx.subtructAverage, ref_avg, 2.4e-7 * max(1.0, np.abs(ref_avg).max())),
                          (ctx.stabilizer, ref_stab, 2.4e-7 * max(1.0, np.abs(ref_stab).max())),
                          (ctx.subtructMeanMagnitude, ref_mm, 4 * MEAN_MAG_REF_ERR * mean64 + 1e-6)):
        fl = _flow_view(f, pad)
        got = _np(gpu(fl.view))
        err = np.abs(got - ref)
        print("[postops] %s pad %d: max error %.3g (first pass %.3g, second pass %.3g), bar %.3g" % (
            gpu.__name__, pad, err.max(), err.reshape(-1, 2)[:CAP_ITEMS].max(), err.reshape(-1, 2)[CAP_ITEMS:].max(), bar))
        assert err.max() <= bar, gpu.__name__
        fl.check("the field")
