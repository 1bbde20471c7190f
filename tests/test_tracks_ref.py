"""The numpy statement of the rip tracks (tests/_tracks_ref.py) held to hand-built sequences with known answers; and the
interface of rcflow_tracks_* through every layer."""
import ctypes
import os
import re

import numpy as np
import pytest

import _regions_ref as R
import _tracks_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blobs(h, w, *boxes):
    """a mask with the boxes (x0, y0, x1, y1), inclusive, set"""
    m = np.zeros((h, w), np.uint8)
    for (x0, y0, x1, y1) in boxes:
        m[y0:y1 + 1, x0:x1 + 1] = 255
    return m


def step(tr, mask, conn=4, max_regions=None):
    g = R.regions(mask, conn, 1, tr.max_regions if max_regions is None else max_regions)
    return tr.push(g["labels"], g["records"], g["summary"][2])


def used(out):
    return out["tracks"][out["tracks"]["id"] != 0]


def test_a_blob_moving_one_pixel_per_push_keeps_its_id():
    tr = T.Tracks(20, 10, max_tracks=4, min_hits=3)
    for n in range(1, 8):
        out = step(tr, blobs(10, 20, (n, 2, n + 2, 4)))
        q = used(out)
        assert len(q) == 1 and (q["id"][0], q["slot"][0], q["hits"][0], q["age"][0], q["misses"][0]) == (1, 0, n, n, 0)
        assert q["flags"][0] == (T.BORN | T.SEEN if n == 1 else T.SEEN | (T.CONFIRMED if n >= 3 else 0))
        assert (q["x0"][0], q["y0"][0], q["x1"][0], q["y1"][0], q["px"][0], q["py"][0]) == (n, 2, n + 2, 4, n + 1, 3)
        assert (q["px0"][0], q["py0"][0], q["first_push"][0], q["parent"][0]) == (2, 3, 1, 0)
        assert q["overlap"][0] == (0 if n == 1 else 6) and q["area_sum"][0] == 9 * n and q["label"][0] == 1
        assert out["summary"].tolist() == [1, int(n >= 3), int(n == 1), 0, 1, 0, 0, n]
        # elsewhere the old footprint stays with a track that goes on: the blob leaves a trail
        assert np.array_equal(out["footprint"], np.where(blobs(10, 20, (1, 2, n + 2, 4)) > 0, 1, 0))
        assert out["track_of_label"].tolist()[:2] == [0, 1]


@pytest.mark.parametrize("max_misses", [0, 2])
def test_a_blob_that_goes_missing(max_misses):
    b = blobs(8, 12, (3, 2, 6, 5))
    for k in range(1, max_misses + 2):
        tr = T.Tracks(12, 8, max_tracks=3, max_misses=max_misses, min_hits=1)
        step(tr, b)
        for miss in range(1, k + 1):
            out = step(tr, np.zeros_like(b))
            q = out["tracks"][0]
            assert q["id"] == 1 and q["misses"] == miss and q["label"] == 0 and q["area"] == 16 and q["age"] == 1 + miss
            gone = miss > max_misses
            assert q["flags"] == T.COASTING | T.CONFIRMED | (T.ENDED if gone else 0)
            # a coasting track keeps its footprint, an ended one gives it up
            assert np.array_equal(out["footprint"], np.where(b > 0, 0 if gone else 1, 0))
            assert not out["mask_out"].any()
            assert out["summary"].tolist() == [0 if gone else 1, 0 if gone else 1, 0, int(gone), 0, 1, 0, 1 + miss]
        out = step(tr, b)
        q = used(out)
        assert len(q) == 1
        if k <= max_misses:
            assert (q["id"][0], q["hits"][0], q["misses"][0], q["age"][0], q["flags"][0]) == (1, 2, 0, k + 2, T.SEEN | T.CONFIRMED)
        else:                                             # the slot was freed at the start of this push and taken again
            assert (q["id"][0], q["slot"][0], q["hits"][0], q["age"][0], q["first_push"][0]) == (2, 0, 1, 1, k + 2)
            assert q["flags"][0] == T.BORN | T.SEEN | T.CONFIRMED and tr.next_id == 3


def test_two_blobs_that_merge():
    tr = T.Tracks(20, 8, max_tracks=4, max_misses=1, min_hits=1)
    out = step(tr, blobs(8, 20, (1, 1, 6, 6), (10, 2, 12, 4)))          # 36 and 9 pixels
    assert used(out)["id"].tolist() == [1, 2]
    out = step(tr, blobs(8, 20, (1, 1, 12, 6)))                         # one region over both
    a, b = out["tracks"][0], out["tracks"][1]
    assert (a["id"], a["flags"], a["overlap"], a["area"]) == (1, T.SEEN | T.CONFIRMED, 36, 72)
    assert (b["id"], b["flags"], b["misses"], b["area"]) == (2, T.COASTING | T.MERGED | T.CONFIRMED, 1, 9)
    assert set(np.unique(out["footprint"])) == {0, 1}                   # the region took the loser's footprint
    assert out["summary"].tolist() == [2, 2, 0, 0, 1, 1, 0, 2]
    out = step(tr, blobs(8, 20, (1, 1, 12, 6)))
    b = out["tracks"][1]
    assert (b["id"], b["flags"], b["misses"]) == (2, T.COASTING | T.ENDED | T.CONFIRMED, 2)       # nothing of it is left to be merged
    assert out["summary"].tolist() == [1, 1, 0, 1, 1, 1, 0, 3]
    out = step(tr, blobs(8, 20, (1, 1, 12, 6)))
    assert not out["tracks"][1:].view(np.uint8).any() and out["tracks"][0]["hits"] == 4


def test_a_split_has_a_winner_and_a_child():
    tr = T.Tracks(20, 8, max_tracks=4, min_hits=2)
    step(tr, blobs(8, 20, (1, 1, 12, 4)))
    out = step(tr, blobs(8, 20, (1, 1, 3, 4), (6, 1, 12, 4)))           # 12 and 28 pixels of the old footprint
    a, b = out["tracks"][0], out["tracks"][1]
    assert (a["id"], a["label"], a["overlap"], a["flags"], a["parent"]) == (1, 2, 28, T.SEEN | T.SPLIT | T.CONFIRMED, 0)
    assert (b["id"], b["label"], b["parent"], b["flags"], b["first_push"], b["overlap"]) == (2, 1, 1, T.BORN | T.SEEN, 2, 0)
    assert out["track_of_label"].tolist()[:3] == [0, 2, 1]
    # the confirmed mask: the winner's region alone
    assert np.array_equal(out["mask_out"], blobs(8, 20, (6, 1, 12, 4)))
    # the gap between the two still belongs to the track that goes on
    assert (out["footprint"][1:5, 4:6] == 1).all() and (out["footprint"][1:5, 1:4] == 2).all()


def test_tie_rules():
    # step 5 first: the slot of a track that ended in this push is not free yet; it is at the next one
    tr = T.Tracks(24, 6, max_tracks=3, max_misses=0, min_hits=1)
    X, Y, Z = (1, 1, 4, 2), (10, 1, 13, 2), (1, 4, 4, 5)
    step(tr, blobs(6, 24, X))
    out = step(tr, blobs(6, 24, Y))
    assert out["tracks"]["id"].tolist() == [1, 2, 0] and out["tracks"][0]["flags"] & T.ENDED
    out = step(tr, blobs(6, 24, Y, (20, 4, 22, 5), Z))                  # labels: Y 1, Z 2, the third 3 (raster order of first pixels)
    assert out["tracks"]["id"].tolist() == [3, 2, 4] and out["track_of_label"].tolist()[:4] == [0, 2, 1, 3]
    # step 2: a region with 4 pixels on id 3 (slot 0) and 4 on id 2 (slot 1): the smaller id, not the smaller slot.
    # The footprint now: Y (id 2, slot 1) on rows 1-2, columns 10-13; Z (id 3, slot 0) on rows 4-5, columns 1-4; nothing
    # where X was, its track ended two pushes ago.
    bridge = np.zeros((6, 24), np.uint8)
    bridge[2, 1:14] = 255                                               # row 2: columns 10-13 are 4 pixels of id 2, the rest lies on nothing
    bridge[3, 1] = 255                                                  # joins the two rows, on nothing
    bridge[4, 1:5] = 255                                                # row 4: columns 1-4 are 4 pixels of id 3; 4 == 4
    out = step(tr, bridge)
    a, b = out["tracks"][0], out["tracks"][1]
    assert (b["id"], b["flags"] & T.SEEN, b["overlap"]) == (2, T.SEEN, 4)
    assert (a["id"], a["flags"]) == (3, T.COASTING | T.MERGED | T.ENDED | T.CONFIRMED)
    # step 3: two regions with the same overlap claim one track: the lower label wins, the other is its child
    tr = T.Tracks(12, 3, max_tracks=3, min_hits=1)
    step(tr, blobs(3, 12, (0, 1, 4, 1)))
    out = step(tr, blobs(3, 12, (0, 1, 1, 1), (3, 1, 4, 1)))
    a, b = out["tracks"][0], out["tracks"][1]
    assert (a["label"], a["overlap"], a["flags"]) == (1, 2, T.SEEN | T.SPLIT | T.CONFIRMED)
    assert (b["label"], b["parent"], b["id"]) == (2, 1, 2)
    # step 5: ascending labels take ascending free slots, ids in that order
    tr = T.Tracks(12, 3, max_tracks=4, min_hits=1)
    out = step(tr, blobs(3, 12, (0, 0, 0, 0), (3, 0, 3, 0), (6, 0, 6, 0)))
    assert [(q["slot"], q["id"], q["label"]) for q in used(out)] == [(0, 1, 1), (1, 2, 2), (2, 3, 3)] and tr.next_id == 4


def test_slot_exhaustion():
    tr = T.Tracks(12, 3, max_tracks=2, min_hits=1)
    m = blobs(3, 12, (0, 0, 1, 1), (4, 0, 5, 1), (8, 0, 9, 1))
    for n in (1, 2):
        out = step(tr, m)
        assert out["tracks"]["id"].tolist() == [1, 2] and out["summary"].tolist() == [2, 2, 2 if n == 1 else 0, 0, 2, 0, 1, n]
        assert out["track_of_label"].tolist()[:4] == [0, 1, 2, 0]
        assert np.array_equal(out["mask_out"], blobs(3, 12, (0, 0, 1, 1), (4, 0, 5, 1)))
        assert not out["footprint"][:, 8:].any() and tr.next_id == 3
    # an untracked region wipes the footprint it covers
    out = step(tr, blobs(3, 12, (0, 0, 1, 1), (3, 2, 3, 2), (4, 0, 5, 1)))       # labels 1, 3 (first pixel in row 2), 2
    out = step(tr, blobs(3, 12, (0, 0, 1, 1), (8, 0, 9, 1), (4, 0, 4, 0)))       # labels 1, 3, 2 by raster order: (0,0) (4,0) (8,0)
    assert out["tracks"]["hits"].tolist() == [4, 4]


@pytest.mark.parametrize("min_hits", [1, 3])
def test_confirmation_and_the_confirmed_mask(min_hits):
    tr = T.Tracks(10, 6, max_tracks=2, min_hits=min_hits, max_misses=2)
    b = blobs(6, 10, (2, 1, 5, 3))
    for n in range(1, 5):
        out = step(tr, b)
        conf = n >= min_hits
        assert bool(out["tracks"][0]["flags"] & T.CONFIRMED) == conf and out["summary"][1] == int(conf)
        assert np.array_equal(out["mask_out"], b if conf else np.zeros_like(b))
        p = T.prims(out["tracks"], 0x20c0ff, 2, 3).reshape(2, 5)
        assert (p[1]["kind"] == 0).all() and p[0]["kind"].tolist() == ([T.LINE] * 4 + [T.DISC] if conf else [0] * 5)
    assert [tuple(p[0, j][k] for k in ("x0", "y0", "x1", "y1")) for j in range(5)] == [(2, 1, 5, 1), (5, 1, 5, 3), (5, 3, 2, 3), (2, 3, 2, 1), (4, 2, 4, 2)]
    # hits are not lost over a gap; a confirmed track that coasts shows no mask but keeps its box until it ends
    out = step(tr, np.zeros_like(b))
    assert out["tracks"][0]["flags"] == T.COASTING | T.CONFIRMED and not out["mask_out"].any()
    assert T.prims(out["tracks"])["kind"][:5].tolist() == [T.LINE] * 4 + [T.DISC]


def test_labels_outside_the_records_are_background():
    tr = T.Tracks(12, 3, max_regions=2, max_tracks=4, min_hits=1)
    m = blobs(3, 12, (0, 0, 1, 1), (4, 0, 5, 1), (8, 0, 9, 1))
    g = R.regions(m, 4, 1, 8)
    lab = g["labels"].copy()
    lab[2, 11] = -5
    lab[2, 10] = 2 ** 31 - 1
    out = tr.push(lab, g["records"], g["summary"][2])                   # three records written, max_regions 2
    assert out["tracks"]["id"].tolist() == [1, 2, 0, 0] and out["summary"][6] == 0 and len(out["track_of_label"]) == 3
    assert not out["footprint"][:, 8:].any() and not out["mask_out"][:, 8:].any()
    # records written below max_regions: label 2 is background too, and the footprint under it stays with its track
    out = tr.push(lab, g["records"], 1)
    a, b = out["tracks"][0], out["tracks"][1]
    assert a["flags"] & T.SEEN and b["flags"] == T.COASTING | T.CONFIRMED and out["track_of_label"].tolist() == [0, 1, 0]
    assert (out["footprint"][0:2, 4:6] == 2).all() and not out["mask_out"][:, 2:].any()
    out = tr.push(lab, g["records"], -3)                                # a negative count is no records
    assert out["summary"][4] == 0 and out["summary"][5] == 2


def test_flow_sums_and_means():
    tr = T.Tracks(6, 2, max_tracks=2, min_hits=1)
    m = blobs(2, 6, (0, 0, 3, 1))
    flow = np.zeros((2, 6, 2), np.float32)
    flow[..., 0], flow[..., 1] = 1.5, -0.25
    flow[0, 0] = (np.nan, 0)
    for n in (1, 2, 3):
        g = R.regions(m, 4, 1, 4, flow * n)
        out = tr.push(g["labels"], g["records"], g["summary"][2])
    q = out["tracks"][0]
    assert (q["area_sum"], q["m_sum"], q["fx_sum"], q["fy_sum"]) == (24, 21, 7 * 98304 * 6, -7 * 16384 * 6)
    assert q["mean_fx"] == np.float32(3.0) and q["mean_fy"] == np.float32(-0.5)


def test_interface_through_every_layer():
    """every rcflow_tracks_* name of include/rcflow.h has a ctypes signature and a Context method, rc_track has the size the
    header documents in every layer, rc::Tracks is there, and without a GPU the Python host refuses loudly"""
    hdr = open(os.path.join(ROOT, "include", "rcflow.h")).read()
    names = sorted(set(re.findall(r"\bint (rcflow_tracks_\w+)\(", hdr)))
    assert names == ["rcflow_tracks_close", "rcflow_tracks_info", "rcflow_tracks_open", "rcflow_tracks_prims_dev", "rcflow_tracks_push_dev",
                     "rcflow_tracks_read", "rcflow_tracks_reset"]
    from ripcurrents_amd import _lib
    from ripcurrents_amd.api import TRACK_DTYPE, Context
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
        method = n[len("rcflow_"):].replace("_dev", "")
        assert callable(getattr(Context, method)), method
    doc = int(re.search(r"typedef struct rc_track \{\s*/\* (\d+) bytes", hdr).group(1))
    assert doc == ctypes.sizeof(_lib.Track) == TRACK_DTYPE.itemsize == T.TRACK.itemsize == 128
    assert [n for n, _ in _lib.Track._fields_] == list(TRACK_DTYPE.names) == list(T.TRACK.names)
    body = re.search(r"typedef struct rc_track \{(.*?)\} rc_track;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")] == list(T.TRACK.names)
    for k, v in (("RC_TRACKS_MAX_REGIONS", _lib.RC_TRACKS_MAX_REGIONS), ("RC_TRACKS_MAX", _lib.RC_TRACKS_MAX), ("RC_TRACKS_LAUNCHES", _lib.RC_TRACKS_LAUNCHES)):
        assert int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) == v
    flags = dict((k.lower(), int(v)) for k, v in re.findall(r"RC_TRACK_(\w+) = (\d+)", hdr))
    assert flags == _lib.TRACK_FLAGS == dict(seen=T.SEEN, born=T.BORN, coasting=T.COASTING, ended=T.ENDED, split=T.SPLIT, merged=T.MERGED,
                                             confirmed=T.CONFIRMED)
    prm = re.search(r"typedef struct rc_tracks_params \{(.*?)\} rc_tracks_params;", hdr, re.S).group(1)
    assert re.findall(r"int (\w+);", prm) == [n for n, _ in _lib.TracksParams._fields_]
    assert ctypes.sizeof(_lib.TracksParams) == 24
    mod = open(os.path.join(ROOT, "include", "rcflow_module.hpp")).read()
    assert "class Tracks {" in mod
    for n in names:
        assert n + "(" in mod, n
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            Context(64, 64).tracks_open(64, 64)
        assert lib.rcflow_tracks_open(None, 0, 64, 64, None) == -1 and lib.rcflow_tracks_info(None, 0, None) == -1
