"""The numpy statement of the flow map and FTLE (tests/_ftle_ref.py) against what is known without it: analytic fields, the
oracle's streamline_field for the forward map, and the conditions that make the mixed input worth testing on."""
import math

import numpy as np
import pytest

import _ftle_ref as F

f32 = np.float32
W, H, N = 131, 70, 6
LUT = np.zeros((256, 3), np.uint8)          # the colours are not this tier's subject


def session(fields, direction, spacing=1, threshold=0.15, dt=1.0):
    ref = F.FtleRef(fields[0].shape[1], fields[0].shape[0], LUT, window=len(fields), direction=direction, dt=dt, spacing=spacing,
                    threshold=threshold)
    out = None
    for f in fields:
        out = ref.push(f)
    return out


@pytest.fixture(scope="module")
def mixed():
    return F.mixed_fields(W, H, N)


@pytest.mark.parametrize("direction", [F.FORWARD, F.BACKWARD])
def test_uniform_translation_does_not_stretch(direction):
    out = session([F.uniform_field(W, H, 1.25, -0.75)] * N, direction)
    v = out["valid"]
    assert v.sum() > 0.5 * W * H and (out["steps"] < N).any()
    assert (out["lam"][v] == f32(1.0)).all() and (out["ftle"][v] == 0).all()
    assert not out["lam"][~v].any() and not out["mask"][~v].any()


@pytest.mark.parametrize("direction", [F.FORWARD, F.BACKWARD])
def test_saddle_gives_its_rate(direction):
    a = 0.01
    out = session([F.saddle_field(W, H, a)] * N, direction)
    v = out["valid"]
    assert v.sum() > 0.5 * W * H
    # forward the map stretches x by (1 + a)^n and shrinks y by (1 - a)^n; backward it is y that grows by (1 + a)^n.  Either
    # way the largest stretch per step is 1 + a
    err = np.abs(out["ftle"][v].astype(np.float64) - math.log(1 + a))
    print("saddle, direction %d: largest error %.3g" % (direction, err.max()))
    assert err.max() <= 1e-6


def test_rigid_rotation_grows_as_euler_does():
    om = 0.02
    out = session([F.rotation_field(W, H, om)] * N, F.FORWARD)
    v = out["valid"]
    assert v.sum() > 0.5 * W * H
    want = (1 + om * om) ** N
    rel = np.abs(out["lam"][v].astype(np.float64) / want - 1)
    print("rotation: largest relative error %.3g" % rel.max())
    assert rel.max() <= 1e-5


def test_forward_map_is_the_oracles_streamline_field(orc, mixed):
    pt, dist = np.zeros((H, W, 2), f32), np.zeros((H, W), f32)
    for f in mixed:
        orc.streamline_field(pt, dist, np.ascontiguousarray(f), 1.0, 1, float("inf"))
    D, steps = F.flow_map(mixed, F.FORWARD, 1.0)
    assert np.array_equal(D.view(np.uint32), pt.view(np.uint32))
    assert (steps < N).any() and (steps == N).any()


@pytest.mark.parametrize("direction", [F.FORWARD, F.BACKWARD])
@pytest.mark.parametrize("spacing", [1, 3])
def test_the_mixed_input_leaves_the_frame_and_stays_in_it(mixed, direction, spacing):
    out = session(mixed, direction, spacing=spacing, threshold=0.15)
    n, valid, nmask, stopped = (int(v) for v in out["summary"][:4])
    print("direction %d spacing %d: valid %.3f stopped %.3f mask %.3f of valid" % (direction, spacing, valid / (W * H), stopped / (W * H),
                                                                                nmask / max(valid, 1)))
    assert n == N and valid == out["valid"].sum() and nmask == (out["mask"] != 0).sum()
    assert valid >= 0.6 * W * H
    assert stopped >= 0.05 * W * H
    assert 0 < nmask < 0.5 * valid
    assert np.isfinite(out["map"]).all() and np.isfinite(out["lam"]).all()
    assert out["summary"][4] == out["lam"].view(np.uint32).max()


def test_backward_visits_the_newest_field_first(mixed):
    # one step backward through a window of two is a step through the NEWEST field with -dt
    a, b = mixed[0], mixed[1]
    D2, _ = F.flow_map([a, b], F.BACKWARD, 1.0)
    Db, sb = F.flow_map([b], F.BACKWARD, 1.0)
    moved = sb == 1
    ok, dx, dy = F.sample(a, (Db[..., 0] + np.arange(W, dtype=f32))[moved], (Db[..., 1] + np.arange(H, dtype=f32)[:, None])[moved])
    want = np.where(ok, Db[moved][:, 0] + dx * f32(-1.0), Db[moved][:, 0])
    assert np.array_equal(D2[moved][:, 0], want.astype(f32))
    fwd, bwd = session(mixed, F.FORWARD), session(mixed, F.BACKWARD)
    assert not np.array_equal(fwd["lam"], bwd["lam"]) and not np.array_equal(fwd["map"], -bwd["map"])


def test_directions_agree_in_lam_on_a_steady_translation():
    fields = [F.uniform_field(W, H, 1.25, -0.75)] * N
    fwd, bwd = session(fields, F.FORWARD), session(fields, F.BACKWARD)
    both = fwd["valid"] & bwd["valid"]
    assert both.sum() > 0.4 * W * H
    assert np.array_equal(fwd["lam"][both], bwd["lam"][both])
    assert np.array_equal(fwd["map"][both], -bwd["map"][both])


def test_ring_keeps_the_last_window_fields(mixed):
    ref = F.FtleRef(W, H, LUT, window=3, direction=F.BACKWARD)
    for k, f in enumerate(mixed):
        out = ref.push(f)
        assert out["n"] == min(k + 1, 3) and out["summary"][5] == k + 1
    D, steps = F.flow_map(mixed[-3:], F.BACKWARD, 1.0)
    assert np.array_equal(out["map"], D) and np.array_equal(out["steps"], steps)


def test_bad_values_stop_particles_and_never_reach_the_map(mixed):
    fields = [f.copy() for f in mixed]
    for k, (y, x, c, v) in enumerate([(20, 30, 0, np.nan), (40, 90, 1, np.inf), (33, 60, 0, -np.inf), (50, 20, 1, 1e30), (12, 100, 0, 1e30)]):
        fields[k % N][y, x, c] = v
        fields[N - 1][y + 3, x + 3, c] = v                                       # met at the last step as well
    for direction in (F.FORWARD, F.BACKWARD):
        clean, bad = session(mixed, direction), session(fields, direction)
        assert np.isfinite(bad["map"]).all()
        assert (bad["steps"] < clean["steps"]).any() and (bad["steps"] <= clean["steps"]).all()
        same = bad["steps"] == clean["steps"]
        assert same.mean() > 0.95


@pytest.mark.parametrize("w,h,spacing", [(4, 4, 1), (7, 7, 3), (1, 9, 1), (2, 6, 1)])
def test_sizes_without_a_valid_pixel(w, h, spacing):
    out = session([F.uniform_field(w, h, 0.25, 0.125)] * 2, F.FORWARD, spacing=spacing)
    assert out["summary"][1] == 0 and not out["lam"].any() and not out["mask"].any() and out["summary"][3] > 0
