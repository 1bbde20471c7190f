"""What the Python mirror (ripcurrents_amd/api.py) accepts and refuses before the C ABI is reached, for every tensor argument of
the per-slot products' pushes, of ripmap_mean and of the *_prims outputs; the product objects; the lifecycle.

One small context, frames of 37 x 23, every product opened with about the smallest parameters its open takes.  The tables
below name every argument once; the tests walk them.

The exception types are those of the commit before the mirror's shared helpers (one input-image rule, one output-or-new, one
summary read), so this file passes against that commit's api.py too, except for the cases of test_row_step_below_a_row named
in EARLIER: calls that commit let through to the C layer, which refused them there, and that are now refused here with a
ValueError.  Against that api.py, deselect those and nothing else."""
import numpy as np
import pytest
import torch

from ripcurrents_amd._lib import RcflowError
from ripcurrents_amd.api import MOTION_CELL_DTYPE, REGION_DTYPE, TRACK_DTYPE, Context, Piv, Waves

pytestmark = pytest.mark.gpu

EARLIER = ("ripmap-flow", "tracers_lk-gray", "tracers_flow-flow", "ftle-flow", "planview-flow", "planview-bgr", "waves-gray", "waves-mask",
           "piv-gray", "regions-flow")

W, H, PAD, FILL = 37, 23, 3, 0xA5
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64
WAVES_KW = dict(window=4, bin_lo=1, bin_hi=1, spacing=1, grid_x=2, grid_y=2)
PIV_KW = dict(window=8, range=1, step=8, ensemble=1)


class Arg:
    """One tensor argument.  takes: "tensor" (nothing else), "numpy" (numpy too, converted by _dev, which raises TypeError for
    a tensor of another dtype or on the host) or "copy" (by _img3: as "numpy", and a view whose pixels are not dense is copied,
    not refused).  image: (h, w[, ch]) with rows that may be padded; else a contiguous array."""

    def __init__(self, name, dtype, shape, takes="tensor", optional=False, image=True):
        self.name, self.dtype, self.shape, self.takes, self.optional, self.image = name, dtype, tuple(shape), takes, optional, image


class Product:
    """name: the prefix of the Context methods; args(info) -> (inputs, image outputs, array outputs); extras(info): the
    other methods that take an output, as (method, Arg); primes: pushes before the one whose outputs are compared."""

    def __init__(self, name, open, args, counter="pushes", extras=None, primes=1, id=None):
        self.name, self._open, self.args, self.counter, self.primes, self.id = name, open, args, counter, primes, id or name
        self.extras = extras or (lambda info: [])

    def open(self, ctx):
        self._open(ctx)
        return self.info(ctx)

    def info(self, ctx):
        return getattr(ctx, self.name + "_info")()

    def count(self, ctx):
        return self.info(ctx)[self.counter]

    def push(self, ctx, ins, outs):
        if self.name == "timex":
            return ctx.timex_push(ins["frame"], out=outs)
        return getattr(ctx, self.name + "_push")(**ins, **outs)


def img(h=H, w=W, ch=None):
    return (h, w) if ch is None else (h, w, ch)


def open_tracers(mover):
    def go(ctx):
        ctx.tracers_open(W, H, mover, max_lines=2, max_vertices=4, lk=dict(win=(7, 7), max_level=1) if mover == "lk" else None)
        ctx.tracers_add_streakline((10, 10))
        ctx.tracers_add("timeline", [[5, 5], [20, 15]])
    return go


PRODUCTS = [
    Product("timex", lambda c: c.timex_open(W, H, window=2, products=("mean", "average", "bright", "dark")),
            lambda i: ([Arg("frame", U8, img(ch=3), "copy")], [Arg(n, U8, img(ch=3)) for n in ("mean", "average", "bright", "dark")], []),
            counter="frames_pushed"),
    Product("framestab", lambda c: c.framestab_open(W, H, roi=(4, 4, 16, 16)),
            lambda i: ([Arg("frame", U8, img(ch=3), "copy")], [Arg("out", U8, img(ch=3))], [Arg("result", F64, (3,), image=False)]),
            counter="frames_pushed"),
    Product("ripmap", lambda c: c.ripmap_open(W, H, window=2, grid=(3, 2)),
            lambda i: ([Arg("flow", F32, img(ch=2), "numpy")], [Arg("hsv", U8, img(ch=3)), Arg("mask", U8, img())],
                       [Arg("cells", F32, (2, 3, 4), image=False), Arg("summary", F64, (8,), image=False)]),
            counter="frames_pushed", extras=lambda i: [("ripmap_mean", Arg("out", F32, img(ch=2)))]),
    Product("motion", lambda c: c.motion_open(W, H, grid=(3, 2)),
            lambda i: ([Arg("gray", U8, img())],
                       [Arg("mhi", F32, img()), Arg("orient", F32, img()), Arg("mask", U8, img()), Arg("vis", U8, img(ch=3))],
                       [Arg("cells", U8, (6 * MOTION_CELL_DTYPE.itemsize,), image=False),
                        Arg("frame", U8, (MOTION_CELL_DTYPE.itemsize,), image=False)]),
            extras=lambda i: [("motion_prims", Arg("out", U8, (2 * 7 * 32,), image=False))]),
    Product("tracers", open_tracers("lk"), lambda i: ([Arg("gray", U8, img(), "numpy")], [Arg("canvas", U8, img(ch=3))], []),
            primes=2, id="tracers_lk"),
    Product("tracers", open_tracers("flow"), lambda i: ([Arg("flow", F32, img(ch=2), "numpy")], [Arg("canvas", U8, img(ch=3))], []),
            id="tracers_flow"),
    Product("ftle", lambda c: c.ftle_open(W, H, window=2, spacing=1),
            lambda i: ([Arg("flow", F32, img(ch=2))],
                       [Arg("map", F32, img(ch=2)), Arg("steps", I32, img()), Arg("lam", F32, img()), Arg("ftle", F32, img()),
                        Arg("mask", U8, img()), Arg("vis", U8, img(ch=3))], [Arg("summary", I64, (8,), image=False)])),
    Product("planview", lambda c: c.planview_open(W, H, np.eye(3), 40.0, 40.0, 18.0, 11.0, x0=2.0, y0=2.0, dx=6.0, dy=5.0, nx=5, ny=4),
            lambda i: ([Arg("flow", F32, img(ch=2), optional=True), Arg("bgr", U8, img(ch=3), optional=True)],
                       [Arg("plan", F32, img(4, 5, 2)), Arg("mask", U8, img(4, 5)), Arg("plan_bgr", U8, img(4, 5, 3))],
                       [Arg("summary", I64, (8,), image=False)])),
    Product("waves", lambda c: c.waves_open(W, H, **WAVES_KW),
            lambda i: ([Arg("gray", U8, img()), Arg("mask", U8, img(), optional=True)], [Arg("bin_map", U8, img()), Arg("vis", U8, img(ch=3))],
                       [Arg("cells", U8, (4 * 32,), image=False), Arg("sums", I64, (4 * i["bins"] * 6,), image=False),
                        Arg("summary", I64, (8,), image=False)]), primes=4),
    Product("piv", lambda c: c.piv_open(W, H, **PIV_KW),
            lambda i: ([Arg("gray", U8, img())], [Arg("field", F32, img(i["grid_y"], i["grid_x"], 2)), Arg("vis", U8, img(ch=3))],
                       [Arg("cells", U8, (i["grid_y"] * i["grid_x"] * 32,), image=False), Arg("summary", I64, (8,), image=False)])),
    Product("regions", lambda c: c.regions_open(W, H, max_regions=4),
            lambda i: ([Arg("mask", U8, img()), Arg("flow", F32, img(ch=2), "numpy", optional=True)],
                       [Arg("labels", I32, img()), Arg("mask_out", U8, img())],
                       [Arg("regions", U8, (4 * REGION_DTYPE.itemsize,), image=False), Arg("summary", I64, (8,), image=False)]),
            extras=lambda i: [("regions_prims", Arg("out", U8, (6 * 4 * 32,), image=False))]),
    Product("tracks", lambda c: c.tracks_open(W, H, max_regions=4, max_tracks=3, min_hits=1),
            lambda i: ([Arg("labels", I32, img()), Arg("regions", U8, (4 * REGION_DTYPE.itemsize,), image=False),
                        Arg("regions_summary", I64, (8,), image=False)], [Arg("mask_out", U8, img())],
                       [Arg("tracks", U8, (3 * TRACK_DTYPE.itemsize,), image=False), Arg("track_of_label", I32, (5,), image=False),
                        Arg("summary", I64, (8,), image=False)]),
            extras=lambda i: [("tracks_prims", Arg("out", U8, (5 * 3 * 32,), image=False))]),
]
BY_ID = pytest.mark.parametrize("p", PRODUCTS, ids=[p.id for p in PRODUCTS])


@pytest.fixture(scope="module")
def small():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with Context(64, 32, device=0, streams=1) as c:
        yield c


# ---------------------------------------------------------------------------------------------------------- data and forms
def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def blobs(shift):
    m = np.zeros((H, W), np.uint8)
    m[3 + shift:9 + shift, 4 + shift:12 + shift] = 255
    m[12:20, 20 + shift:30 + shift] = 200
    return m


_DATA = {}


def data(ctx, p, ins):
    """the inputs of every push of a product's run, as numpy arrays: made once, never changed"""
    if p.id not in _DATA:
        rng, pushes = np.random.RandomState(len(p.id) * 131 + 7), []
        for k in range(p.primes + 1):
            d = {}
            for a in ins:
                if a.dtype == F32:
                    d[a.name] = (rng.standard_normal(a.shape) * 1.5).astype(np.float32)
                elif a.name == "mask":
                    d[a.name] = blobs(k % 3) if p.name == "regions" else (rng.randint(0, 4, a.shape) > 0).astype(np.uint8) * 255
                else:
                    d[a.name] = rng.randint(0, 256, a.shape).astype(np.uint8)
            pushes.append(d)
        if p.name == "tracks":                   # what regions_push leaves on the device for two masks
            ctx.regions_open(W, H, max_regions=4)
            for k, d in enumerate(pushes):
                out = dict(labels=torch.zeros((H, W), dtype=I32, device="cuda"), regions=torch.zeros(4 * REGION_DTYPE.itemsize, dtype=U8, device="cuda"),
                           summary=torch.zeros(8, dtype=I64, device="cuda"))
                ctx.regions_push(dev(blobs(k)), **out)
                ctx.sync()
                d.update(labels=out["labels"].cpu().numpy(), regions=out["regions"].cpu().numpy(), regions_summary=out["summary"].cpu().numpy())
            ctx.regions_close()
        _DATA[p.id] = pushes
    return _DATA[p.id]


def wider(shape, factor=1, pad=0):
    return (shape[0], shape[1] * factor + pad) + tuple(shape[2:])


def form(a, how):
    """a numpy image as the argument of a push: "dense", "padded" (a view of rows PAD pixels longer), "numpy", or a view whose
    pixels are not dense: "halved" (every second pixel of rows twice as long) and "channel" (a slice of a wider last dimension)"""
    if how == "numpy":
        return a
    if how == "padded":
        base = np.full(wider(a.shape, pad=PAD), 0, a.dtype)
        base.view(np.uint8)[...] = FILL
        base[:, :a.shape[1]] = a
        return dev(base)[:, :a.shape[1]]
    if how == "halved":
        base = np.zeros(wider(a.shape, 2), a.dtype)
        base[:, ::2] = a
        return dev(base)[:, ::2]
    if how == "channel":
        base = np.zeros(a.shape[:2] + ((2,) if a.ndim == 2 else (a.shape[2] + 1,)), a.dtype)
        if a.ndim == 2:
            base[..., 0] = a
            return dev(base)[..., 0]
        base[..., :a.shape[2]] = a
        return dev(base)[..., :a.shape[2]]
    return dev(a)


def blank(a, pad=0):
    """an output buffer with every byte FILL -> (the whole buffer, the view that is passed)"""
    shape = wider(a.shape, pad=pad) if a.image else a.shape
    base = torch.full((int(np.prod(shape)) * torch.empty((), dtype=a.dtype).element_size(),), FILL, dtype=U8, device="cuda").view(a.dtype).view(shape)
    return base, (base[:, :a.shape[1]] if a.image else base)


def raw(t):
    return t.cpu().numpy().tobytes()


def run(ctx, p, how="dense", pad_out=0):
    """Opens the product anew, pushes its data (the inputs that `how` applies to in that form, the others dense) and asks the
    last push for every output -> {name: bytes}, with the push's return value and the counter.  Padding must stay FILL."""
    info = p.open(ctx)
    ins, images, arrays = p.args(info)
    pushes = data(ctx, p, ins)

    def given(d):
        applies = {"dense": lambda a: False, "padded": lambda a: a.image, "numpy": lambda a: a.takes != "tensor",
                   "halved": lambda a: a.takes == "copy", "channel": lambda a: a.takes == "copy"}[how]
        return {a.name: form(d[a.name], how if applies(a) else "dense") for a in ins}
    for d in pushes[:-1]:
        p.push(ctx, given(d), {})                                 # None for every output
    bufs = {a.name: blank(a, pad_out) for a in images + arrays}
    ret = p.push(ctx, given(pushes[-1]), {k: v for k, (_, v) in bufs.items()})
    ctx.sync()
    got = {k: raw(v) for k, (_, v) in bufs.items()}
    for a in images:
        assert set(raw(bufs[a.name][0][:, a.shape[1]:])) <= {FILL}, "%s: row padding was written" % a.name
    if isinstance(ret, dict):
        assert all(ret[k] is bufs[k][1] for k in ret) and set(ret) == set(bufs)
    elif torch.is_tensor(ret):
        assert ret is bufs["out"][1]
    else:
        got["returned"] = ret
    got["count"] = p.count(ctx)
    return got


_DENSE = {}


def dense(ctx, p):
    """the run every other form is compared with, made once per product"""
    if p.id not in _DENSE:
        _DENSE[p.id] = run(ctx, p)
        written = [k for k, v in _DENSE[p.id].items() if isinstance(v, bytes) and set(v) != {FILL}]
        assert _DENSE[p.id]["count"] >= 1 and len(written) >= len(_DENSE[p.id]) // 2, "the push wrote only %s" % written
    return _DENSE[p.id]


# ---------------------------------------------------------------------------------------------------------- accepted
@BY_ID
def test_padded_rows_and_numpy_give_the_dense_call_s_bytes(small, p):
    ref = dense(small, p)
    assert run(small, p) == ref, "two dense runs differ: the comparison below would mean nothing"
    assert run(small, p, "padded") == ref
    assert run(small, p, pad_out=PAD) == ref
    ins = p.args(p.open(small))[0]
    if any(a.takes != "tensor" for a in ins):
        assert run(small, p, "numpy") == ref
    if any(a.takes == "copy" for a in ins):                      # _img3 copies what is not dense
        assert run(small, p, "halved") == ref and run(small, p, "channel") == ref
    getattr(small, p.name + "_close")()


@BY_ID
def test_none_for_every_optional_argument(small, p):
    ins, images, arrays = p.args(p.open(small))
    d = data(small, p, ins)[0]
    need = {a.name: dev(d[a.name]) for a in ins if not a.optional}
    if p.name == "planview":                                     # either input may be None, not both
        for a in ins:
            p.push(small, {a.name: dev(d[a.name])}, {})
        with pytest.raises(RcflowError):
            p.push(small, {}, {})
        assert p.count(small) == 2
    elif p.id in ("ripmap", "tracers_flow"):                     # None: the field the frame loop left on the slot; there is none
        with pytest.raises(RcflowError):
            p.push(small, {}, {})
        assert p.count(small) == 0
    else:
        p.push(small, need, {})
        p.push(small, need, {a.name: None for a in images + arrays})
        assert p.count(small) == (1 if p.id == "tracers_lk" else 2)
    getattr(small, p.name + "_close")()


# ---------------------------------------------------------------------------------------------------------- refused
def bad_forms(a, good):
    """(what is wrong, the argument) for everything this layer refuses in place of the tensor `good` of Arg `a`"""
    z = lambda shape, dtype=a.dtype: torch.zeros(tuple(shape), dtype=dtype, device="cuda")
    yield "dtype", good.to(F64 if a.dtype != F64 else F32)
    yield "host", good.cpu()
    if a.takes == "tensor":
        yield "numpy", good.cpu().numpy()
    if not a.image:
        yield "count", z(a.shape[:-1] + (a.shape[-1] + 1,))
        yield "not contiguous", z(a.shape[:-1] + (a.shape[-1] * 2,))[..., ::2]
        return
    for k in range(len(a.shape)):
        yield "shape[%d] + 1" % k, z(a.shape[:k] + (a.shape[k] + 1,) + a.shape[k + 1:])
    if a.takes != "copy":
        yield "halved", z(wider(a.shape, 2))[:, ::2]
        yield "channel", z(a.shape + (2,))[..., 0] if len(a.shape) == 2 else z(a.shape[:2] + (a.shape[2] + 1,))[..., :a.shape[2]]


def raises(a, what):
    return TypeError if a.takes != "tensor" and what in ("dtype", "host") else ValueError


@BY_ID
def test_refusals_and_nothing_queued(small, p):
    info = p.open(small)
    ins, images, arrays = p.args(info)
    d = data(small, p, ins)
    good_in = {a.name: dev(d[-1][a.name]) for a in ins}
    good_out = {a.name: blank(a)[1] for a in images + arrays}
    for k in range(p.primes):
        p.push(small, {a.name: dev(d[k][a.name]) for a in ins}, {})
    count, cases = p.count(small), 0
    for a, group in [(a, good_in) for a in ins] + [(a, good_out) for a in images + arrays]:
        for what, bad in bad_forms(a, group[a.name]):
            i, o = dict(good_in), dict(good_out)
            (i if group is good_in else o)[a.name] = bad
            with pytest.raises(raises(a, what)):
                p.push(small, i, o)
                pytest.fail("%s_push took %s: %s" % (p.name, a.name, what))
            assert p.count(small) == count, "%s: %s was refused after something was queued" % (a.name, what)
            cases += 1
    assert cases >= 5 * len(ins + images + arrays)
    p.push(small, good_in, good_out)                             # and the good call still goes through
    assert p.count(small) == count + 1
    getattr(small, p.name + "_close")()


@pytest.mark.parametrize("p", [p for p in PRODUCTS if p.extras({})], ids=lambda p: p.id)
def test_outputs_of_the_other_methods(small, p):
    """ripmap_mean and the *_prims: the caller's output gives the new tensor's bytes, padded too; a wrong one is refused"""
    info = p.open(small)
    ins = p.args(info)[0]
    for d in data(small, p, ins):
        p.push(small, {a.name: dev(d[a.name]) for a in ins}, {})
    count = p.count(small)
    for method, a in p.extras(info):
        call = getattr(small, method)
        fresh = call()
        assert fresh.dtype == a.dtype and fresh.numel() == int(np.prod(a.shape))
        for pad in (0, PAD) if a.image else (0,):
            base, view = blank(a, pad)
            assert call(out=view) is view
            small.sync()
            assert raw(view) == raw(fresh)
            assert not a.image or set(raw(base[:, a.shape[1]:])) <= {FILL}
        for what, bad in bad_forms(a, fresh):
            with pytest.raises(ValueError):
                call(out=bad)
                pytest.fail("%s took out: %s" % (method, what))
    assert p.count(small) == count
    getattr(small, p.name + "_close")()


ROW_STEP = [(p, a) for p in PRODUCTS for a in p.args(dict(bins=1, grid_x=1, grid_y=1))[0] if a.image and a.takes != "copy"]


@pytest.mark.parametrize("p,a", ROW_STEP, ids=["%s-%s" % (p.id, a.name) for p, a in ROW_STEP])
def test_row_step_below_a_row(small, p, a):
    """every row the same memory (row step 0): the input-image rule asks for a step of at least a row.  motion's gray, regions'
    mask and tracks' labels were held to it before; the cases of EARLIER were not."""
    ins = p.args(p.open(small))[0]
    good = {x.name: dev(data(small, p, ins)[0][x.name]) for x in ins}
    good[a.name] = good[a.name][0].expand(a.shape)
    with pytest.raises(ValueError):
        p.push(small, good, {})
    assert p.count(small) == 0
    getattr(small, p.name + "_close")()


# ---------------------------------------------------------------------------------------------------------- lifecycle, objects
@BY_ID
def test_reset_then_push_and_close_then_info(small, p):
    ins = p.args(p.open(small))[0]
    d = data(small, p, ins)
    for k in range(2):
        p.push(small, {a.name: dev(d[k][a.name]) for a in ins}, {})
    assert p.count(small) >= 1
    getattr(small, p.name + "_reset")()
    assert p.count(small) == 0
    for k in range(2):
        p.push(small, {a.name: dev(d[k][a.name]) for a in ins}, {})
    assert p.count(small) >= 1
    getattr(small, p.name + "_close")()
    with pytest.raises(RcflowError):
        p.info(small)


def same(a, b):
    """equality of what the read methods return: tuples, dicts, numpy arrays and numbers"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b


@pytest.mark.parametrize("cls,kw,setting,others", [(Waves, WAVES_KW, (0.9, 2, 5.0), ("spectrum", "table")),
                                                  (Piv, PIV_KW, (0.5, 0.2, 3.0, 2.0), ("sums",))], ids=["Waves", "Piv"])
def test_product_object_is_the_context_s_methods(small, cls, kw, setting, others):
    p = [q for q in PRODUCTS if q.name == cls.__name__.lower()][0]
    ins, images, arrays = p.args(p.open(small))
    frames = [dev(d["gray"]) for d in data(small, p, ins)]
    m = lambda verb: getattr(small, "%s_%s" % (p.name, verb))

    def through(push, set, read, info, reset, other):
        """the same session through either interface -> everything it returned"""
        outs = {a.name: blank(a)[1] for a in images + arrays}
        set(*setting)
        for f in frames[:-1]:
            assert push(f) is None
        assert push(frames[-1], **outs) is None
        got = [read(), info(), [o() for o in other], {k: raw(v) for k, v in outs.items()}]
        reset()
        return got + [info()]

    m("open")(W, H, **kw)
    ref = through(m("push"), m("set"), m("read"), m("info"), m("reset"), [m(o) for o in others])
    m("close")()
    with cls(small, W, H, **kw) as obj:
        assert obj.ctx is small and obj.stream == 0
        got = through(obj.push, obj.set, obj.read, obj.info, obj.reset, [getattr(obj, o) for o in others])
    assert same(got, ref) and ref[1][p.counter] == len(frames)
    with pytest.raises(RcflowError):
        obj.info()
    obj = cls(small, W, H, stream=0, **kw)                        # without the with block: close() is the caller's
    obj.close()
    with pytest.raises(RcflowError):
        obj.info()
