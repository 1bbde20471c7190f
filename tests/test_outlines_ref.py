"""The sequential statement of the region outlines (tests/_outlines_ref.py) against what must be true of any boundary tracing, against
the regions' statement, and against cases small enough to do by hand."""
import numpy as np
import pytest

import _outlines_ref as R
import _regions_ref as RG


def planes():
    r = np.random.RandomState(7)
    for i in range(300):
        w, h = r.randint(1, 14), r.randint(1, 14)
        yield R.random_labels(w, h, r.randint(1, 4), 1000 + i, r.choice([0.3, 0.5, 0.8]))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_what_is_true_of_every_plane(connectivity):
    for lab in planes():
        lab64 = lab.astype(np.int64)
        keys = R.cracks_of(lab64)
        succ = [R.successor(lab64, k, connectivity) for k in keys]
        assert sorted(succ) == keys, "the successor is no permutation of the cracks"
        loops, n = R.loops_of(lab64, connectivity)
        assert n == len(keys) == sum(q["cracks"] for q in loops)
        for q in loops:
            side = q["leader"] & 3
            assert q["area2"] != 0 and (q["area2"] > 0) == (side == R.N) and (q["area2"] < 0) == (side == R.S)
            assert len(q["verts"]) % 2 == 0 and len(q["verts"]) >= 4
            x0, y0, x1, y1 = q["box"]
            assert 0 <= x0 < x1 <= lab.shape[1] and 0 <= y0 < y1 <= lab.shape[0]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_one_label_masks_against_the_regions(connectivity):
    r = np.random.RandomState(11)
    for i in range(100):
        w, h = r.randint(1, 14), r.randint(1, 14)
        mask = np.where(r.rand(h, w) < r.choice([0.3, 0.6, 0.9]), 255, 0).astype(np.uint8)
        loops, n = R.loops_of(R.plane_of(mask=mask), connectivity)
        comps = int(RG.regions(mask, connectivity)["summary"][0])
        assert sum(q["area2"] > 0 for q in loops) == comps
        assert sum(q["area2"] for q in loops) == 2 * int((mask != 0).sum())


def test_one_pixel():
    o = R.outlines(labels=np.array([[1]], np.int32), max_loops=2, max_vertices=8)
    r = o["loops"][0]
    assert list(o["summary"]) == [4, 1, 1, 1, 4, 4, 0, 1]
    assert (r["label"], r["flags"], r["x"], r["y"], r["cracks"], r["verts"], r["offset"], r["area2"]) == (1, 0, 0, 0, 4, 4, 0, 2)
    assert (r["x0"], r["y0"], r["x1"], r["y1"]) == (0, 0, 1, 1)
    assert o["verts"][:4].tolist() == [[1, 0], [1, 1], [0, 1], [0, 0]] and not o["verts"][4:].any() and not o["loops"][1:].view(np.uint8).any()


def test_the_diagonal_pair():
    lab = np.array([[1, 0], [0, 1]], np.int32)
    o4 = R.outlines(labels=lab, connectivity=4)
    assert o4["summary"][1] == 2 and list(o4["loops"]["cracks"][:2]) == [4, 4] and list(o4["loops"]["area2"][:2]) == [2, 2]
    o8 = R.outlines(labels=lab, connectivity=8)
    r = o8["loops"][0]
    assert o8["summary"][1] == 1 and (r["cracks"], r["area2"], r["verts"]) == (8, 4, 8)


def test_a_ring_has_a_hole():
    lab = np.ones((3, 3), np.int32)
    lab[1, 1] = 0
    for c in (4, 8):
        o = R.outlines(labels=lab, connectivity=c)
        a, b = o["loops"][0], o["loops"][1]
        assert o["summary"][1] == 2 and (a["area2"], a["flags"], a["cracks"]) == (18, 0, 12) and (b["area2"], b["flags"], b["cracks"]) == (-2, R.HOLE, 4)
        assert (b["x"], b["y"]) == (1, 0)                  # the hole's leader is the south side of the pixel above it


def test_two_labels_sharing_an_edge_are_strangers():
    o = R.outlines(labels=np.array([[1, 2]], np.int32))
    assert o["summary"][1] == 2 and list(o["loops"]["label"][:2]) == [1, 2] and list(o["loops"]["cracks"][:2]) == [4, 4]


def test_filter_caps_and_overflow():
    lab = R.rings(9, 9)                                    # an outer loop, and a hole and an outer loop per ring inwards
    full = R.outlines(labels=lab)
    kept = int(full["summary"][2])
    assert kept >= 4 and full["summary"][4] == full["summary"][5] == 4 * kept
    few = R.outlines(labels=lab, max_loops=kept - 1)
    assert few["summary"][3] == kept - 1 and few["summary"][5] == 4 * (kept - 1) and few["summary"][4] == 4 * kept
    short = R.outlines(labels=lab, max_vertices=4 * kept - 1)
    last = short["loops"][kept - 1]
    assert last["offset"] == -1 and last["flags"] & R.NOVERTS and short["summary"][5] == 4 * (kept - 1) and not short["verts"][4 * (kept - 1):].any()
    big = R.outlines(labels=lab, min_cracks=5)
    assert big["summary"][2] == kept - 1 and big["summary"][1] == kept       # the one-pixel centre is dropped, the rest renumbered
    over = R.outlines(labels=lab, max_cracks=int(full["summary"][0]) - 1)
    assert list(over["summary"]) == [full["summary"][0], 0, 0, 0, 0, 0, 1, 1] and not over["loops"].view(np.uint8).any() and not over["verts"].any()


def test_the_serpentine_is_one_loop():
    lab = R.serpentine(96, 64)
    o = R.outlines(labels=lab, connectivity=4, max_vertices=1 << 12)
    assert o["summary"][1] == 1 and o["loops"][0]["cracks"] == o["summary"][0] > 6000 and o["loops"][0]["area2"] == 2 * lab.sum()


def test_prims_close_every_loop():
    lab = R.rings(5, 5)
    o = R.outlines(labels=lab, max_vertices=32)
    p = R.prims(o, 5, 5, 0x123456, 2)
    n = int(o["summary"][5])
    assert (p["kind"][:n] == R.LINE).all() and not p[n:].view(np.uint8).any() and p["x1"].max() == 4 and p["y1"].max() == 4
    for r in o["loops"][:int(o["summary"][3])]:
        a, b = r["offset"], r["offset"] + r["verts"]
        assert (p["x1"][a:b] == np.roll(p["x0"][a:b], -1)).all() and (p["y1"][a:b] == np.roll(p["y0"][a:b], -1)).all()
