"""The numpy statement of the virtual drifters (tests/_drifters_ref.py) held to properties: the figures of the prototype on the
synthetic rip, a uniform field, conservation, a field of columns, RESPAWN, and the edge of every decision by constructed integers."""
import numpy as np
import pytest

import _drifters_ref as D
from ripcurrents_amd import synth

LUT = np.stack([np.arange(256)] * 3, 1).astype(np.uint8)


def session(w, h, homes, **kw):
    kw.setdefault("max_drifters", max(1, len(homes)))
    r = D.DriftersRef(w, h, D.Params(**kw), LUT)
    assert r.seed(homes)
    return r


def conserved(r, out, occ_total):
    s = out["summary"]
    assert s[2] == s[1] + s[8:].sum()
    assert out["place"][:, 0].sum() == occ_total == int(out["density"].astype(np.int64).sum())
    assert out["origin"][:, 0].sum() == s[2]
    assert out["hist"].sum() == s[8:].sum()


# ---------------------------------------------------------------------------- the prototype's figures
@pytest.fixture(scope="module")
def prototype():
    """the 301 pushes with max_age 300: (the summary after each push, the ages at the OFFSHORE deaths)"""
    f = D.field(*synth.surf_field(160, 120))
    r = session(160, 120, D.prototype_lattice(), max_age=300, grid_x=8, grid_y=6)
    z = D.prototype_zone()
    rows, ages, occ = [], [], 0
    for _ in range(301):
        out = r.push(f, z)
        occ += int(out["occupancy"].sum())
        conserved(r, out, occ)
        rows.append(out["summary"].copy())
        ages += list(out["age"][out["fate"] == D.OFFSHORE])
    return rows, ages, r


def test_prototype_census_with_max_age_300(prototype):
    rows, ages, r = prototype
    s = rows[-1]
    assert (s[0], s[1]) == (1520, 0)
    assert (s[8 + D.SHORE], s[8 + D.OFFSHORE], s[8 + D.AGED]) == (1235, 200, 85)
    assert (min(ages), float(np.median(ages)), max(ages)) == (7, 37.5, 271)
    assert s[5] == sum(ages)


def test_prototype_census_on_the_way(prototype):
    rows = prototype[0]
    got = [(int(rows[k - 1][8 + D.SHORE]), int(rows[k - 1][8 + D.OFFSHORE]), int(rows[k - 1][1])) for k in (50, 100, 200)]
    assert got == [(865, 144, 511), (1209, 187, 124), (1235, 196, 89)]


def test_prototype_without_old_age_and_the_homes_that_leave():
    f = D.field(*synth.surf_field(160, 120))
    r = session(160, 120, D.prototype_lattice())
    z = D.prototype_zone()
    for _ in range(2000):
        out = r.push(f, z)
    s = out["summary"]
    assert (s[8 + D.SHORE], s[8 + D.OFFSHORE], s[1]) == (1270, 246, 4)
    assert round(100.0 * 246 / 1520, 1) == 16.2 and round(100.0 * 1270 / 1520, 1) == 83.6
    hx = r.HX[r.st == D.OFFSHORE] / 64.0
    assert (round(float(hx.min()), 2), round(float(hx.max()), 2)) == (72.45, 102.66) and abs(hx.min() - 72.45) < 0.01 and abs(hx.max() - 102.65) < 0.01
    # wider than the band where the jet's own v is negative: the feeders count too
    assert hx.min() < 88 - 12.5 and hx.max() > 88 + 12.5


# ---------------------------------------------------------------------------- a uniform field
def test_uniform_field_steps_and_the_right_edge():
    w, h = 40, 60
    r = session(w, h, [[3.0, 50.0]])
    f = D.uniform_field(w, h, 1.25, -0.75)
    out = r.push(f)
    assert (r.X[0], r.Y[0], r.st[0], r.age[0]) == (192, 3200, D.ALIVE, 0) and (out["step"] == 0).all()
    k = 0
    while True:
        out = r.push(f)
        k += 1
        if r.st[0] != D.ALIVE:
            break
        assert (r.X[0], r.Y[0], r.age[0]) == (192 + 80 * k, 3200 - 48 * k, k)
    # 192 + 80 k > 64 * 39 first at k = 29; the position is kept
    assert (k, r.st[0], r.X[0], r.Y[0], r.age[0]) == (29, D.EDGE_RIGHT, 192 + 80 * 28, 3200 - 48 * 28, 29)
    assert out["state"][0] == D.EDGE_RIGHT and out["summary"][8 + D.EDGE_RIGHT] == 1
    assert out["xy"][0, 0] == np.float32((192 + 80 * 28) / 64.0)


@pytest.mark.parametrize("u, v, fate", [(-2.0, 0.0, D.EDGE_LEFT), (0.0, -2.0, D.EDGE_TOP), (0.0, 2.0, D.EDGE_BOTTOM), (-2.0, -2.0, D.EDGE_LEFT)])
def test_edges_and_their_order(u, v, fate):
    r = session(9, 9, [[4.0, 4.0]])
    f = D.uniform_field(9, 9, u, v)
    for _ in range(4):
        r.push(f)
    assert r.st[0] == fate


# ---------------------------------------------------------------------------- columns
def column_scene(w=60, h=40, a=20, b=40):
    f = np.zeros((h, w, 2), np.float32)
    f[..., 1] = 1.0
    f[:, a:b, 1] = -1.5
    z = np.zeros((h, w), np.uint8)
    z[:4], z[h - 4:] = 2, 1
    homes = D.lattice(2.0 + 2.0 * np.arange(28), 8.0 + 4.0 * np.arange(6))
    return f, z, homes


def test_columns_exactly_the_band_leaves():
    f, z, homes = column_scene()
    r = session(60, 40, homes, grid_x=3, grid_y=2, age_bin=4)
    occ = 0
    for _ in range(40):
        out = r.push(f, z)
        occ += int(out["occupancy"].sum())
        conserved(r, out, occ)
    inband = (homes[:, 0] >= 20) & (homes[:, 0] < 40)
    assert (r.st[inband] == D.OFFSHORE).all() and (r.st[~inband] == D.SHORE).all() and out["summary"][1] == 0
    c = out["cells"].reshape(2, 3)
    assert (c["escape"][:, 1] == 1).all() and (c["escape"][:, [0, 2]] == 0).all()
    assert (c["beached"][:, 1] == 0).all() and (c["beached"][:, [0, 2]] == 1).all() and (c["mean_u"] == 0).all()
    # what tests/cpp/test_drifters.cpp says of the first exits: age 4, bin 1
    assert out["hist"][1, 0] == 0 and out["hist"][1, 1] > 0
    assert (c["mean_exit_age"][:, 1] == (out["origin"].reshape(2, 3, 8)[:, 1, 6] / out["origin"].reshape(2, 3, 8)[:, 1, 2]).astype(np.float32)).all()


def test_respawn_keeps_the_population():
    f, z, homes = column_scene()
    r = session(60, 40, homes, flags=D.RESPAWN)
    prev_total = prev_released = last_deaths = 0
    for k in range(60):
        out = r.push(f, z)
        s = out["summary"]
        total = int(s[8:].sum())
        assert s[1] + (r.st > 0).sum() == len(homes)
        assert s[2] - prev_released == (len(homes) if k == 0 else last_deaths)
        last_deaths, prev_total, prev_released = total - prev_total, total, int(s[2])
        assert s[2] == s[1] + total
    assert s[2] > 2 * len(homes)
    # switched off, the dead stay dead and are counted nowhere
    r.set(flags=0)
    released = int(s[2])
    for _ in range(40):
        out = r.push(f, z)
    assert out["summary"][2] == released and out["summary"][1] == 0


def test_reset_and_seed_after_pushes():
    f, z, homes = column_scene()
    r = session(60, 40, homes[:50], max_drifters=200)
    first = [r.push(f, z)["summary"].copy() for _ in range(5)]
    assert r.seed(homes[50:100]) and (r.st[50:] == D.WAITING).all()
    out = r.push(f, z)
    assert out["summary"][0] == 100 and out["summary"][2] == 100 and (out["state"][50:] == 0).all() and (out["age"][50:] == 0).all()
    assert not r.seed(homes) and r.n == 100                   # too many: nothing added
    assert not r.seed([[60.0, 3.0]]) and not r.seed([[np.nan, 3.0]]) and not r.seed([[-0.01, 0.0]]) and r.n == 100
    r.reset()
    assert (r.st == D.WAITING).all() and (r.X == r.HX).all() and r.density.sum() == 0 and r.summary.sum() == 0
    r2 = session(60, 40, homes[:100], max_drifters=200)
    for k in range(5):
        assert (r.push(f, z)["summary"] == r2.push(f, z)["summary"]).all()


# ---------------------------------------------------------------------------- the edge of every decision
def one(w, h, X, Y, flow, zone=None, **kw):
    """a session whose one drifter is ALIVE at (X, Y) in 1/64 pixel -> (session, the push's outputs)"""
    r = session(w, h, [[X / 64.0, Y / 64.0]], **kw)
    r.push(np.zeros((h, w, 2), np.float32))
    assert (r.X[0], r.Y[0], r.st[0]) == (X, Y, D.ALIVE)
    return r, r.push(flow, zone)


def test_right_edge_against_one_more():
    w, h = 8, 8
    f = D.uniform_field(w, h, 1.0, 0.0)
    r, out = one(w, h, 64 * (w - 1) - 64, 128, f)
    assert r.st[0] == D.ALIVE and r.X[0] == 64 * (w - 1)
    r, out = one(w, h, 64 * (w - 1) - 63, 128, f)
    assert r.st[0] == D.EDGE_RIGHT and r.X[0] == 64 * (w - 1) - 63
    f = D.uniform_field(w, h, 0.0, 1.0)
    r, out = one(w, h, 128, 64 * (h - 1) - 64, f)
    assert r.st[0] == D.ALIVE and r.Y[0] == 64 * (h - 1)
    r, out = one(w, h, 128, 64 * (h - 1) - 63, f)
    assert r.st[0] == D.EDGE_BOTTOM


def test_step_rounding_is_a_floor():
    w, h = 8, 8
    # D = 4096 q; with dt_q = 1: D dt_q + 2^19 = 4096 q + 524288, a multiple of 2^20 when q = 128 (+1.0 -> exactly 1) and q = -128 (0)
    for q, dq, step in ((128, 1, 1), (127, 1, 0), (-128, 1, 0), (-129, 1, -1), (-384, 1, -1), (-385, 1, -2), (-1, 256, -1), (1, 128, 1), (-1, 128, 0)):
        r, out = one(w, h, 256, 256, D.uniform_field(w, h, q / 64.0, 0.0), dt=1.0)
        r2 = session(w, h, [[4.0, 4.0]], dt=dq / 256.0)
        r2.push(np.zeros((h, w, 2), np.float32))
        out = r2.push(D.uniform_field(w, h, q / 64.0, 0.0))
        assert out["step"][0, 0] == step == (4096 * q * dq + (1 << 19)) >> 20, (q, dq)


def test_bad_corner_under_weight_0_and_weight_1():
    w, h = 8, 8
    f = D.uniform_field(w, h, 0.5, 0.25)
    f[3, 4] = np.nan                                          # the right neighbour of pixel (3, 3)
    r, out = one(w, h, 3 * 64, 3 * 64, f)                     # fx = 0: its weight is 0, not looked at
    assert r.st[0] == D.ALIVE and (r.X[0], r.Y[0]) == (3 * 64 + 32, 3 * 64 + 16)
    r, out = one(w, h, 3 * 64 + 1, 3 * 64, f)                 # fx = 1: weight 64
    assert r.st[0] == D.BAD and (r.X[0], r.Y[0]) == (3 * 64 + 1, 3 * 64) and r.age[0] == 1
    f[3, 4] = (0.5, 0.25)
    f[4, 4] = np.inf                                          # the diagonal neighbour: weight fx fy
    r, out = one(w, h, 3 * 64 + 1, 3 * 64, f)
    assert r.st[0] == D.ALIVE
    r, out = one(w, h, 3 * 64 + 1, 3 * 64 + 1, f)             # weight 1
    assert r.st[0] == D.BAD


def test_500_against_the_float_below_it():
    w, h = 600, 4
    below = np.nextafter(np.float32(500.0), np.float32(0.0))
    r, out = one(w, h, 64, 64, D.uniform_field(w, h, below, 0.0))
    assert r.st[0] == D.ALIVE and out["step"][0, 0] == 32000
    r, out = one(w, h, 64, 64, D.uniform_field(w, h, 500.0, 0.0))
    assert r.st[0] == D.BAD
    r, out = one(w, h, 64 * 550, 64, D.uniform_field(w, h, 0.0, -500.0))
    assert r.st[0] == D.BAD
    r, out = one(w, h, 64, 64, D.uniform_field(w, h, -0.0, -0.0))
    assert r.st[0] == D.ALIVE and (out["step"] == 0).all()


def test_int64_product_at_dt_256():
    w, h = 700, 4
    r = session(w, h, [[1.0, 1.0]], dt=256.0)
    r.push(np.zeros((h, w, 2), np.float32))
    out = r.push(D.uniform_field(w, h, 499.0, 0.0))
    # D = 4096 * 31936, dt_q = 65536: the product is 8.6e12
    assert out["step"][0, 0] == (4096 * 31936 * 65536 + (1 << 19)) >> 20 == 31936 * 256 and r.st[0] == D.EDGE_RIGHT


def test_age_equals_max_age():
    w, h = 8, 8
    f = np.zeros((h, w, 2), np.float32)
    r = session(w, h, [[4.0, 4.0]], max_age=3)
    states = []
    for _ in range(5):
        out = r.push(f)
        states.append((int(r.st[0]), int(r.age[0])))
    assert states == [(0, 0), (0, 1), (0, 2), (D.AGED, 3), (D.AGED, 3)]
    assert out["hist"][3, 0] == 1 and out["summary"][8 + D.AGED] == 1


def test_zone_bytes_7_8_and_255_and_the_release_in_a_zone():
    w, h = 8, 8
    f = np.zeros((h, w, 2), np.float32)
    for byte, fate in ((1, 9), (2, 10), (6, 14), (7, 15), (8, 15), (255, 15)):
        z = np.zeros((h, w), np.uint8)
        z[4, 4] = byte
        r = session(w, h, [[4.0, 4.0], [3.49, 4.0], [3.5, 4.49]])
        out = r.push(f, z)                                    # released at home, inside the zone: dead at once, age 0
        assert list(r.st) == [fate, D.ALIVE, fate] and out["summary"][2] == 3 and out["summary"][8 + fate] == 2
        assert out["hist"][D.fate_class(fate), 0] == 2


def test_zones_helper_statement():
    wet = np.array([[0, 255, 1], [0, 0, 7]], np.uint8)
    inside = np.array([[0, 0, 9], [255, 0, 0]], np.uint8)
    assert (D.zones(wet, inside) == [[1, 2, 0], [1, 1, 2]]).all()
    assert (D.zones(wet, None) == [[1, 0, 0], [1, 1, 0]]).all()
    assert (D.zones(None, inside) == [[2, 2, 0], [0, 2, 2]]).all()


def test_open_and_set_errors():
    assert D.open_error(8, 8, D.Params()) is None
    for kw in (dict(max_drifters=0), dict(max_drifters=D.MAX_DRIFTERS + 1), dict(age_bin=0), dict(dt=0.0), dict(dt=256.01), dict(dt=float("nan")),
               dict(max_age=-1), dict(density_full=0), dict(live_min=0), dict(flags=2)):
        assert D.open_error(8, 8, D.Params(**kw)) == "parameters", kw
    assert D.open_error(8, 8, D.Params(grid_x=9)) == "grid" and D.open_error(200, 200, D.Params(grid_x=129, grid_y=128)) == "grid"
    assert D.dt_q(1.0) == 256 and D.dt_q(256.0) == 65536 and D.dt_q(1 / 256) == 1 and D.dt_q(0.001) is None
