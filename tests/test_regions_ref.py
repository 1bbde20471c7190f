"""The numpy statement of the rip regions (tests/_regions_ref.py) against a brute-force flood fill, scipy.ndimage where it is
installed and hand-built masks with known answers; and the interface of rcflow_regions_* through every layer."""
import ctypes
import os
import re

import numpy as np
import pytest

import _regions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_masks():
    rng = np.random.RandomState(3)
    for (h, w) in [(1, 1), (1, 9), (9, 1), (5, 7), (16, 64), (17, 65), (37, 53)]:
        for dens in (0.1, 0.45, 0.593, 0.9):
            yield (rng.rand(h, w) < dens).astype(np.uint8) * rng.choice([1, 128, 255])


@pytest.mark.parametrize("conn", [4, 8])
def test_statement_against_flood_fill(conn):
    for m in random_masks():
        got = R.regions(m, conn, 1, 4096)
        want = R.flood(m, conn)
        assert np.array_equal(got["labels"], want)
        K = int(want.max())
        assert got["K"] == K == got["summary"][0] == got["summary"][1]
        for k in range(1, K + 1):
            ys, xs = np.nonzero(want == k)
            q = got["records"][k - 1]
            assert (q["label"], q["area"], q["x0"], q["y0"], q["x1"], q["y1"]) == (k, len(xs), xs.min(), ys.min(), xs.max(), ys.max())
            f = (ys * m.shape[1] + xs).min()
            assert (q["first_x"], q["first_y"]) == (f % m.shape[1], f // m.shape[1])
            assert (q["sx"], q["sy"], q["sxx"], q["syy"], q["sxy"]) == (xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum())
            assert abs(q["cx"] - xs.mean()) < 1e-9 and abs(q["cy"] - ys.mean()) < 1e-9
            c = np.cov(np.stack([xs, ys]).astype(np.float64), bias=True) if len(xs) > 1 else np.zeros((2, 2))
            ev = np.linalg.eigvalsh(c)
            assert abs(q["var_major"] - ev[1]) < 1e-7 * max(1, ev[1]) and abs(q["var_minor"] - ev[0]) < 1e-7 * max(1, ev[1])


@pytest.mark.parametrize("conn", [4, 8])
def test_filter_renumbers_in_order(conn):
    rng = np.random.RandomState(11)
    m = (rng.rand(60, 80) < 0.5).astype(np.uint8)
    full = R.regions(m, conn, 1, 65536)
    areas = full["all_records"]["area"]
    for min_area in (2, 5, int(areas.max()), int(areas.max()) + 1):
        got = R.regions(m, conn, min_area, 65536)
        keep = areas >= min_area
        assert got["K"] == keep.sum()
        renum = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)])
        assert np.array_equal(got["labels"], renum[full["labels"]])
        assert np.array_equal(got["mask_out"], np.where(got["labels"] > 0, 255, 0))
        assert np.array_equal(got["all_records"]["first_x"], full["all_records"]["first_x"][keep])
        s = got["summary"]
        assert s[0] == len(areas) and s[3] == (m != 0).sum() and s[4] == areas[keep].sum() and s[7] == (areas[keep].max() if keep.any() else 0)
    # overflow: K and the label image are complete, the records stop at max_regions, the rest is zero bytes
    got = R.regions(m, conn, 1, 3)
    assert got["K"] == len(areas) and got["summary"][2] == 3 and got["labels"].max() == len(areas)
    assert np.array_equal(got["records"], full["records"][:3])


def test_statement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(5)
    for (h, w) in [(37, 53), (120, 200), (270, 480)]:
        for dens in (0.45, 0.593, 0.9):
            m = rng.rand(h, w) < dens
            for conn, st in ((4, ndi.generate_binary_structure(2, 1)), (8, np.ones((3, 3), int))):
                want, n = ndi.label(m, st)
                got = R.regions(m.astype(np.uint8), conn, 1, 65536)
                assert got["K"] == n and np.array_equal(got["labels"], want)
                rec = got["all_records"]
                assert np.array_equal(rec["area"], ndi.sum(m, want, np.arange(1, n + 1)).astype(np.int64))
                for q, sl in zip(rec, ndi.find_objects(want)):
                    assert (q["y0"], q["y1"] + 1, q["x0"], q["x1"] + 1) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)


def test_hand_built_masks():
    m = np.zeros((6, 6), np.uint8)
    m[0:2, 0:2] = 1
    m[2:4, 2:4] = 1                               # two squares touching at a corner
    assert R.regions(m, 8)["K"] == 1 and R.regions(m, 4)["K"] == 2
    assert np.array_equal(np.unique(R.regions(m, 4)["labels"][2:4, 2:4]), [2])
    # nested rings: three components at either connectivity, numbered outside in
    r = np.zeros((11, 11), np.uint8)
    for k in (0, 2, 4):
        r[k, k:11 - k] = r[10 - k, k:11 - k] = r[k:11 - k, k] = r[k:11 - k, 10 - k] = 255
    for conn in (4, 8):
        g = R.regions(r, conn)
        assert g["K"] == 3 and [tuple(q[k] for k in ("x0", "y0", "x1", "y1")) for q in g["records"][:3]] == [(0, 0, 10, 10), (2, 2, 8, 8), (4, 4, 6, 6)]
        assert list(g["records"]["edges"][:3]) == [15, 0, 0]
        assert abs(g["records"][0]["cx"] - 5) < 1e-12 and abs(g["records"][0]["var_major"] - g["records"][0]["var_minor"]) < 1e-9
    # a bar along the diagonal of y DOWN: the major axis points at 45 degrees
    d = np.eye(9, dtype=np.uint8)
    q = R.regions(d, 8)["records"][0]
    assert q["area"] == 9 and abs(q["angle"] - 45.0) < 1e-9 and abs(q["var_minor"]) < 1e-9
    assert R.regions(d, 4)["K"] == 9
    q = R.regions(d[:, ::-1], 8)["records"][0]
    assert abs(q["angle"] - 135.0) < 1e-9
    # checkerboard
    c = (np.indices((8, 8)).sum(0) % 2 == 0).astype(np.uint8)
    assert R.regions(c, 4, 1, 64)["K"] == 32 and R.regions(c, 8, 1, 64)["K"] == 1
    # empty and full
    assert R.regions(np.zeros((4, 5), np.uint8), 8)["K"] == 0
    f = R.regions(np.full((4, 5), 7, np.uint8), 4)
    assert f["K"] == 1 and f["records"][0]["area"] == 20 and f["records"][0]["edges"] == 15


def test_bad_pixel_rule_and_flow_means():
    m = np.ones((2, 4), np.uint8)
    m[:, 2] = 0                                    # two components: columns 0-1 and column 3
    flow = np.zeros((2, 4, 2), np.float32)
    flow[..., 0], flow[..., 1] = 1.5, -0.25
    flow[0, 0] = (np.nan, 1)
    flow[1, 0] = (3, np.inf)
    flow[0, 3] = (2.0 ** 25, 0)                   # 2^41 in fixed point: beyond the bound
    flow[1, 3] = (2.0 ** 24, -2.0 ** 24)          # exactly 2^40: inside
    flow[0, 2] = (np.nan, np.nan)                 # background: nobody counts it
    g = R.regions(m, 4, 1, 4, flow)
    a, b = g["records"][0], g["records"][1]
    assert (a["area"], a["bad"], a["fx"], a["fy"]) == (4, 2, 2 * 98304, 2 * -16384)
    assert (b["area"], b["bad"], b["fx"], b["fy"]) == (2, 1, 2 ** 40, -2 ** 40)
    assert a["mean_fx"] == np.float32(1.5) and a["mean_fy"] == np.float32(-0.25) and b["mean_fx"] == np.float32(2.0 ** 24)
    assert g["summary"][5] == 3
    # a component whose pixels are all bad: means 0, no flow line
    flow[:, 3] = np.nan
    g = R.regions(m, 4, 1, 4, flow)
    assert g["records"][1]["bad"] == 2 and g["records"][1]["mean_fx"] == 0
    p = R.prims(g["records"], flow_scale=2.0).reshape(-1, 6)
    assert p[1, 5]["kind"] == 0 and p[0, 5]["kind"] == R.LINE and (p[2:]["kind"] == 0).all()
    assert (p[0, 5]["x1"] - p[0, 5]["x0"], p[0, 5]["y1"] - p[0, 5]["y0"]) == (3, 0)          # rint(3.0), rint(-0.5) = -0
    # dropped components count no bad pixels
    assert R.regions(m, 4, 3, 4, flow)["summary"][5] == 2


def test_integer_centroid_rounds_half_up():
    m = np.zeros((3, 4), np.uint8)
    m[0, 0:2] = 1                                  # centroid x = 0.5 -> 1
    m[2, 0:4] = 1                                  # centroid x = 1.5 -> 2
    p = R.prims(R.regions(m, 4)["records"][:2]).reshape(2, 6)
    assert (p[0, 4]["x0"], p[0, 4]["y0"], p[1, 4]["x0"], p[1, 4]["y0"]) == (1, 0, 2, 2)
    assert [tuple(p[1, j][k] for k in ("x0", "y0", "x1", "y1")) for j in range(4)] == [(0, 2, 3, 2), (3, 2, 3, 2), (3, 2, 0, 2), (0, 2, 0, 2)]
    m = np.zeros((2, 1), np.uint8) + 1             # centroid y = 0.5 -> 1
    assert R.prims(R.regions(m, 4)["records"][:1])[4]["y0"] == 1


def test_interface_through_every_layer():
    """every rcflow_regions_* name of include/rcflow.h has a ctypes signature and a Context method, rc_region has the size the
    header documents, and without a GPU the Python host refuses loudly"""
    hdr = open(os.path.join(ROOT, "include", "rcflow.h")).read()
    names = sorted(set(re.findall(r"\bint (rcflow_regions_\w+)\(", hdr)))
    assert names == ["rcflow_regions_close", "rcflow_regions_info", "rcflow_regions_open", "rcflow_regions_prims_dev",
                     "rcflow_regions_push_dev", "rcflow_regions_read", "rcflow_regions_reset", "rcflow_regions_set"]
    from ripcurrents_amd import _lib
    from ripcurrents_amd.api import REGION_DTYPE, Context
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
        method = n[len("rcflow_"):].replace("_dev", "")
        assert callable(getattr(Context, method)), method
    doc = int(re.search(r"typedef struct rc_region \{\s*/\* (\d+) bytes \*/", hdr).group(1))
    assert doc == ctypes.sizeof(_lib.Region) == REGION_DTYPE.itemsize == R.REGION.itemsize == 144
    assert [n for n, _ in _lib.Region._fields_] == list(REGION_DTYPE.names) == list(R.REGION.names)
    assert int(re.search(r"#define RC_REGIONS_LAUNCHES (\d+)", hdr).group(1)) == _lib.RC_REGIONS_LAUNCHES
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            Context(64, 64).regions_open(64, 64)
        assert lib.rcflow_regions_open(None, 0, 64, 64, None) == -1 and lib.rcflow_regions_info(None, 0, None) == -1
