"""The numpy statement of the mean current (tests/_meanflow_ref.py) against a second, brute-force statement, its integer bounds,
and the two scenes the GPU tests use.  No GPU."""
import math

import numpy as np
import pytest

import _meanflow_ref as M

LUT = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], -1).astype(np.uint8)   # any table: the statement only indexes it


def brute_sums(fields, W):
    """every sum from the last W fields alone, in Python integers -> dict of [h][w] object arrays"""
    held = fields[-W:]
    h, w = held[0].shape[:2]
    out = {k: np.zeros((h, w), object) for k in ("n", "Su", "Sv", "Suu", "Svv", "Suv", "Sm")}
    for f in held:
        for y in range(h):
            for x in range(w):
                fu, fv = np.float32(f[y, x, 0]), np.float32(f[y, x, 1])
                if not (math.isfinite(fu) and math.isfinite(fv) and abs(fu) < np.float32(500.0) and abs(fv) < np.float32(500.0)):
                    continue
                u, v = int(np.rint(fu * np.float32(64.0))), int(np.rint(fv * np.float32(64.0)))
                assert abs(u) <= 32000 and abs(v) <= 32000
                out["n"][y, x] += 1
                out["Su"][y, x] += u
                out["Sv"][y, x] += v
                out["Suu"][y, x] += u * u
                out["Svv"][y, x] += v * v
                out["Suv"][y, x] += u * v
                out["Sm"][y, x] += math.isqrt(u * u + v * v)
    return out


def test_incremental_sums_equal_the_brute_force_statement():
    """after every push, over three wraps of the ring, with bad samples of every kind entering and leaving"""
    w, h, W = 7, 5, 4
    ref = M.MeanFlowRef(w, h, M.Params(window=W, grid_x=2, grid_y=2, min_fill=2), LUT)
    fields, saw_drop = [], False
    for t in range(3 * W + 2):
        f = M.hostile_field(w, h, t)
        if t == 5:
            f[...] = np.nan                                   # a whole field of bad samples
        fields.append(f)
        n_before = ref.n.copy()
        ref.push(f)
        want = brute_sums(fields, W)
        for k in want:
            assert (getattr(ref, k).astype(object) == want[k]).all(), (t, k)
        saw_drop |= bool((ref.n < n_before).any())
    assert saw_drop and (ref.n > 0).any()


def test_outputs_follow_from_the_sums():
    """the per-pixel outputs recomputed one pixel at a time with Python integers and floats"""
    w, h, W = 6, 4, 3
    p = M.Params(window=W, grid_x=3, grid_y=2, min_fill=2, steady_min=300, speed_min=0.25, min_cos2=0.25, dir_x=1.0, dir_y=-2.0)
    ref = M.MeanFlowRef(w, h, p, LUT)
    for t in range(7):
        out = ref.push(M.hostile_field(w, h, t, seed=11))
        smin_q = math.ceil(p.speed_min * 64.0)
        for y in range(h):
            for x in range(w):
                n, Su, Sv, Sm = (int(getattr(ref, k)[y, x]) for k in ("n", "Su", "Sv", "Sm"))
                if n < p.min_fill:
                    assert not out["mean"][y, x].any() and out["steady"][y, x] == 0 and not out["std"][y, x].any()
                    assert out["mask"][y, x] == 0 and not out["picture"][y, x].any()
                    continue
                R = math.isqrt(Su * Su + Sv * Sv)
                st = min(1000, R * 1000 // Sm) if Sm > 0 else 0
                assert out["steady"][y, x] == st and (out["picture"][y, x] == LUT[st * 255 // 1000]).all()
                assert out["mean"][y, x, 0] == np.float32(Su / 64.0 / n) and out["mean"][y, x, 1] == np.float32(Sv / 64.0 / n)
                a = n * int(ref.Suu[y, x]) - Su * Su
                c = n * int(ref.Svv[y, x]) - Sv * Sv
                b = n * int(ref.Suv[y, x]) - Su * Sv
                A, B, C = float(a), float(b), float(c)
                r = math.sqrt((A - C) * (A - C) + 4.0 * (B * B))
                l1, l2 = ((A + C) + r) * 0.5, max(((A + C) - r) * 0.5, 0.)
                assert out["std"][y, x, 0] == np.float32(math.sqrt(l1) / (64.0 * n)) and out["std"][y, x, 1] == np.float32(math.sqrt(l2) / (64.0 * n))
                dot = Su * p.dir_x + Sv * p.dir_y
                inside = st >= p.steady_min and R >= smin_q * n and dot > 0 and dot * dot >= p.min_cos2 * ((float(Su) ** 2 + float(Sv) ** 2) * 5.0)
                assert out["mask"][y, x] == (255 if inside else 0)
        s = out["summary"]
        assert s[0] == (ref.n >= p.min_fill).sum() and s[1] == (out["mask"] > 0).sum() and s[6] == min(t + 1, W) and s[7] == t + 1
        assert out["sums"][:, 0].sum() == s[0] and out["sums"][:, 5].sum() == s[1] and (out["sums"][:, 7] == 0).all()


def test_the_bounds_hold_at_the_largest_window_and_the_largest_sample():
    """W = 4096 with every component at +-499.999 (q = +-32000): asserted on Python integers, before anything is narrowed"""
    W, v = 4096, np.float32(499.999)
    assert int(np.rint(v * np.float32(64.0))) == 32000
    f = np.empty((2, 2, 2), np.float32)
    f[0, 0], f[0, 1], f[1, 0], f[1, 1] = (v, v), (-v, -v), (v, -v), (-v, v)
    ref = M.MeanFlowRef(2, 2, M.Params(window=W, min_fill=W), LUT)
    for _ in range(W):
        ref.update(f)
    b = ref.bounds()
    assert (ref.n == W).all()
    assert b["S"] == 4096 * 32000 < 2 ** 31                    # Su, Sv: int32
    assert b["Sm"] == 4096 * math.isqrt(2 * 32000 ** 2) < 2 ** 32       # Sm: uint32
    assert b["nS2"] == 4096 * 4096 * 32000 ** 2 < 1.8e16 < 2 ** 63      # n Suu in int64
    assert b["SS"] == 2 * (4096 * 32000) ** 2 < 2 ** 56 < 2 ** 63       # Su^2 + Sv^2 in int64; what the device's isqrt is given
    assert M.state_bytes(16, 8, W) == 16 * 8 * (4 * W + 38)
    out = ref.push(f)                                         # the wrap: one sample out, the same in
    assert (ref.n == W).all() and ref.bounds() == b
    assert (out["steady"] == 999).all() or (out["steady"] == 1000).all()      # m is a floor: R may pass Sm
    assert not out["std"].any()                               # a constant sample has no spread


SCENES = {"fixed": (M.NAMING, {}), "opposed": (M.OPPOSED, M.OPPOSED_SCENE)}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_scenes_name_the_jet(name):
    """20 x 12, W = 8, 20 pushes: the mask is the jet, exactly, with a clear margin in the steadiness on either side"""
    p, kw = SCENES[name]
    ref = M.MeanFlowRef(20, 12, p, LUT)
    jet = M.jet_mask(jet=kw.get("jet", (8, 12)))
    for t in range(20):
        out = ref.push(M.naming_scene(t, **kw))
        if t < p.window - 1:
            assert not out["mask"].any() and out["summary"][0] == 0
    assert (out["mask"] == jet).all()
    _, st = ref.steadiness()
    assert st[jet > 0].min() >= p.steady_min + 100 and st[jet == 0].max() <= p.steady_min - 100
    gx, gy = out["summary"][3], out["summary"][4]
    if name == "opposed":
        assert gy > 50 * abs(gx) and gy > 20 * 12 * 8 * 32    # G points down the picture, clearly: over half a pixel a sample
    assert (out["cells"]["flags"] == 0).all() and out["cells"]["mask"].sum() == (jet > 0).sum()


def test_open_and_set_refusals():
    ok = M.Params()
    assert M.open_error(20, 12, ok) is None
    for bad in (dict(window=1), dict(window=4097), dict(min_fill=0), dict(min_fill=9), dict(steady_min=-1), dict(steady_min=1001), dict(flags=0),
                dict(flags=3), dict(speed_min=-0.1), dict(speed_min=400.5), dict(speed_min=math.nan), dict(min_cos2=1.0), dict(min_cos2=-0.1),
                dict(dir_x=0., dir_y=0.), dict(dir_x=math.inf), dict(grid_x=21), dict(grid_y=0)):
        assert M.open_error(20, 12, M.Params(**{**ok.__dict__, **bad})) is not None, bad
    assert M.open_error(20, 12, M.Params(flags=M.DIR_OPPOSED, dir_x=0., dir_y=0.)) is None       # not looked at
    assert M.open_error(1 << 14, 1 << 14, M.Params(window=4, min_fill=4)) == "size"
