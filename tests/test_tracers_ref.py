"""CPU tier of the tracer sessions: the numpy statement (tests/_tracers_ref.py) against answers a reader can check by hand."""
import numpy as np

import _tracers_ref as R


def _m(p, w, h):
    return R.mask(p[0], w, h)


def _rows(text):
    return np.array([[c == "#" for c in row] for row in text.split()])


def test_disc_pixel_counts_and_shapes():
    # dx^2 + dy^2 <= r^2 + r: counted by hand for the small ones, by the formula for r = 10
    for r, count in [(0, 1), (1, 9), (2, 21), (3, 37), (4, 69), (10, 349)]:
        m = _m(R.disc(12, 12, r), 25, 25)
        assert m.sum() == count, r
        assert np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1]) and np.array_equal(m, m.T)
    assert np.array_equal(_m(R.disc(2, 2, 1), 5, 5), _rows(".....\n.###.\n.###.\n.###.\n....."))   # 1 + 1 <= 1 + 1: the corners too
    assert np.array_equal(_m(R.disc(2, 2, 2), 5, 5), _rows(".###.\n#####\n#####\n#####\n.###."))
    # r = 3: rows of 3, 5, 7, 7, 7, 5, 3
    assert [int(v) for v in _m(R.disc(3, 3, 3), 7, 7).sum(1)] == [3, 5, 7, 7, 7, 5, 3]


def test_thin_lines_against_hand_written_masks():
    assert np.array_equal(_m(R.line(1, 1, 4, 1), 6, 3), _rows("......\n.####.\n......"))
    assert np.array_equal(_m(R.line(4, 1, 1, 1), 6, 3), _rows("......\n.####.\n......"))
    assert np.array_equal(_m(R.line(1, 0, 1, 3), 3, 4), _rows(".#.\n.#.\n.#.\n.#."))
    assert np.array_equal(_m(R.line(1, 3, 1, 0), 3, 4), _rows(".#.\n.#.\n.#.\n.#."))
    assert np.array_equal(_m(R.line(0, 0, 3, 3), 4, 4), _rows("#...\n.#..\n..#.\n...#"))
    assert np.array_equal(_m(R.line(3, 0, 0, 3), 4, 4), _rows("...#\n..#.\n.#..\n#..."))
    # shallow, (0,0) -> (5,2): y = (4 t + 5) / 10 = 0, 0, 1, 1, 2, 2
    assert np.array_equal(_m(R.line(0, 0, 5, 2), 6, 3), _rows("##....\n..##..\n....##"))
    # the other direction starts from the other end: y = 2 - (4 t + 5) / 10 over x = 5, 4, ... -- the same pixels here
    assert np.array_equal(_m(R.line(5, 2, 0, 0), 6, 3), _rows("##....\n..##..\n....##"))
    # (0,0) -> (4,1): y = (2 t + 4) / 8 = 0, 0, 1, 1, 1; from the other end y = 1 - (2 t + 4) / 8 = 1, 1, 0, 0, 0 over x = 4..0:
    # not symmetric in its ends
    assert np.array_equal(_m(R.line(0, 0, 4, 1), 5, 2), _rows("##...\n..###"))
    assert np.array_equal(_m(R.line(4, 1, 0, 0), 5, 2), _rows("###..\n...##"))
    # steep: the shallow one transposed
    assert np.array_equal(_m(R.line(0, 0, 2, 5), 3, 6), _rows("##....\n..##..\n....##").T)
    assert np.array_equal(_m(R.line(1, 4, 0, 0), 2, 5), _rows("###..\n...##").T)
    # zero length: its one pixel
    assert np.array_equal(_m(R.line(2, 1, 2, 1), 4, 3), _rows("....\n..#.\n...."))
    # every thin line is 8-connected with exactly max(adx, ady) + 1 pixels
    rng = np.random.RandomState(3)
    for _ in range(200):
        x0, y0, x1, y1 = rng.randint(0, 30, 4)
        m = _m(R.line(x0, y0, x1, y1), 30, 30)
        assert m.sum() == max(abs(x1 - x0), abs(y1 - y0)) + 1 and m[y0, x0] and m[y1, x1]


def test_thick_lines():
    # t = 2: distance <= 1.  Horizontal (1,2) -> (4,2): the rows 1..3 over x = 1..4 and the two end caps
    assert np.array_equal(_m(R.line(1, 2, 4, 2, 2), 6, 5), _rows("......\n.####.\n######\n.####.\n......"))
    # diagonal (1,1) -> (3,3): pixels within distance 1 of the segment: |x - y| <= 1 between the ends (cross^2 <= 2), caps
    assert np.array_equal(_m(R.line(1, 1, 3, 3, 2), 5, 5), _rows(".#...\n###..\n.###.\n..###\n...#."))
    # zero length: the disc of radius t / 2
    assert _m(R.line(3, 3, 3, 3, 2), 7, 7).sum() == 5 and _m(R.line(3, 3, 3, 3, 4), 7, 7).sum() == 13
    # t = 3 horizontal: distance <= 1.5 is the same rows as t = 2 (integer pixel centres), caps a pixel longer only on the axis
    assert np.array_equal(_m(R.line(2, 2, 3, 2, 3), 6, 5), _rows("......\n.####.\n.####.\n.####.\n......"))
    # a thick line contains the thin one and is symmetric in its ends
    rng = np.random.RandomState(4)
    for _ in range(100):
        x0, y0, x1, y1 = rng.randint(2, 28, 4)
        t = int(rng.randint(2, 9))
        a, b = _m(R.line(x0, y0, x1, y1, t), 30, 30), _m(R.line(x1, y1, x0, y0, t), 30, 30)
        assert np.array_equal(a, b) and not (_m(R.line(x0, y0, x1, y1), 30, 30) & ~a).any()


def test_blend_is_cvround_of_the_float_expression():
    c, p = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    want = np.rint(np.float32(0.5) * c.astype(np.float32) + np.float32(0.5) * p.astype(np.float32)).astype(np.uint8)
    assert np.array_equal(R.blend(c, p), want)
    assert R.blend(np.uint8(100), np.uint8(1)) == 50 and R.blend(np.uint8(100), np.uint8(3)) == 52     # 50.5 -> 50, 51.5 -> 52


def test_order_clipping_skipping_channels_and_padding():
    img = np.full((12, 20, 3), 7, np.uint8)
    prims = np.concatenate([R.disc(5, 5, 2, 0x0000ff), R.disc(6, 5, 1, 0x00ff00),                 # later overwrites
                            R.disc(5, 5, 0, 100 << 16, R.BLEND),                                 # blended over opaque
                            R.disc(15, 5, 1, 200, R.BLEND), R.line(14, 5, 16, 5, 1, 0x010203)])  # opaque over blended
    assert R.draw(img, prims) == 0
    assert tuple(img[5, 4]) == (255, 0, 0) and tuple(img[5, 6]) == (0, 255, 0) and tuple(img[4, 6]) == (0, 255, 0)
    assert tuple(img[5, 5]) == (0, 128, 50)                      # (0 + 0) / 2, (255 + 0) / 2 = 127.5 -> 128, (0 + 100) / 2
    assert tuple(img[5, 15]) == (3, 2, 1) and tuple(img[4, 15]) == (104, 4, 4)     # (200 + 7) / 2 = 103.5 -> 104; 3.5 -> 4
    assert tuple(img[0, 0]) == (7, 7, 7)
    # partly and wholly off the image; the skip bound; 1 channel; a view with padding keeps its padding
    buf = np.full((8, 16), 9, np.uint8)
    view = buf[:, :10]
    prims = np.concatenate([R.disc(-1, 3, 2, 50), R.disc(40, 40, 3, 60), R.line(-5, 7, 30, 7, 1, 70),
                            R.disc(16384, 0, 1, 80), R.line(0, 0, 0, -16384, 1, 80), R.line(0, 0, 5, 5, 9, 80),
                            R.line(0, 0, 5, 5, 0, 80), R.prim(3, 1, 1), R.disc(2, 2, -1, 80), R.disc(-2 ** 31, 0, 1, 80)])
    assert R.draw(view, prims) == 7
    assert (buf[:, 10:] == 9).all() and (view[7] == 70).all() and list(view[3, :3]) == [50, 50, 9] and view[1, 0] == 50
    assert not (view == 60).any() and not (view == 80).any()
    assert R.valid(R.disc(16383, -16383, 16383)[0]) and R.valid(R.line(-16383, 0, 16383, 1, 8)[0])


def test_coordinate_conversions():
    v = np.array([1.9, -1.9, 0.5, 1.5, 2.5, -0.5, np.nan, 3e9, -np.inf], np.float32)
    assert list(R.trunc_i32(v)) == [1, -1, 0, 1, 2, 0, -2 ** 31, -2 ** 31, -2 ** 31]
    assert list(R.round_i32(v)) == [2, -2, 0, 2, 2, 0, -2 ** 31, -2 ** 31, -2 ** 31]
    tr = np.array([[[1.5, 2.5], [3.4, 3.6], [3.4, 3.6]]], np.float32)
    p = R.trace_prims(tr)
    assert len(p) == 2 and tuple(p[0])[:6] == (R.LINE, 2, 2, 3, 4, 1) and tuple(p[1])[1:5] == (3, 4, 3, 4)
    p = R.trace_prims(tr, start=[[0.4, 0.6]])
    assert len(p) == 3 and tuple(p[0])[1:5] == (0, 1, 2, 2)


def test_bookkeeping_on_a_scripted_sequence():
    s = R.Session(640, 480, max_vertices=4)
    sid = s.add(R.STREAK, [[0, 0]])
    tid = s.add(R.TIMELINE, [[10, 10], [20, 10]])
    assert np.array_equal(s.all_vertices(), np.array([[0, 0], [10, 10], [20, 10]], np.float32))
    up64, up48 = np.nextafter(np.float32(64), np.float32(100)), np.nextafter(np.float32(48), np.float32(100))
    # |dx| = 64 is NOT a jump (640 * 0.1 = 64.0 exactly); the timeline takes anything
    s.push(np.array([[64, 0], [900, -5], [20, 11]], np.float32))
    assert np.array_equal(s.lines[sid].v, np.array([[0, 0], [64, 0]], np.float32))
    assert np.array_equal(s.lines[tid].v, np.array([[900, -5], [20, 11]], np.float32))
    # the next float above the threshold is a jump, on either axis: both vertices stay
    s.push(np.array([[up64, 0], [64, up48], [0, 0], [1, 1]], np.float32))
    assert np.array_equal(s.lines[sid].v, np.array([[0, 0], [0, 0], [64, 0]], np.float32))
    # |dy| = 48 = 480 * 0.1 exactly is not
    s.push(np.array([[0, 48], [1, 1], [64, 48], [0, 0], [1, 1]], np.float32))
    assert np.array_equal(s.lines[sid].v, np.array([[0, 0], [0, 48], [1, 1], [64, 48]], np.float32)) and s.lines[sid].dropped == 0
    # the ring holds 4: the oldest vertex goes
    s.push(np.array([[5, 5], [6, 50], [7, 7], [8, 8], [0, 0], [1, 1]], np.float32))
    assert np.array_equal(s.lines[sid].v, np.array([[0, 0], [5, 5], [6, 50], [7, 7]], np.float32)) and s.lines[sid].dropped == 1
    s.push(np.array([[1, 1], [2, 2], [3, 3], [4, 4], [0, 0], [1, 1]], np.float32))
    assert np.array_equal(s.lines[sid].v, np.array([[0, 0], [1, 1], [2, 2], [3, 3]], np.float32)) and s.lines[sid].dropped == 2
    s.lines[sid].v = np.array([[100, 100], [101, 101], [102, 102]], np.float32)
    s.lines[sid].first = np.array([[100, 100]], np.float32)
    p = s.lines[sid].prims()
    assert len(p) == 2 * 3 + 1
    assert [tuple(q)[:7] for q in p[:5]] == [(R.DISC, 100, 100, 100, 100, 3, R.GREEN), (R.LINE, 100, 100, 100, 100, 1, R.RED),
                                             (R.DISC, 100, 100, 100, 100, 2, R.BLUE), (R.DISC, 101, 101, 101, 101, 2, R.BLUE),
                                             (R.LINE, 100, 100, 101, 101, 1, R.RED)]
    p = s.lines[tid].prims()
    assert [tuple(q)[:7] for q in p] == [(R.DISC, 0, 0, 0, 0, 4, R.BLUE), (R.LINE, 0, 0, 1, 1, 2, R.RED), (R.DISC, 1, 1, 1, 1, 4, R.BLUE)]
    c = R.Line(R.CLOUD, [[5.9, -0.9]], 3).prims()
    assert tuple(c[0]) == (R.DISC, 5, 0, 5, 0, 10, R.RED, R.BLEND)
    s.reset()
    assert np.array_equal(s.all_vertices(), np.array([[100, 100], [10, 10], [20, 10]], np.float32)) and s.lines[sid].dropped == 0


def test_python_signatures_and_record_match_the_header():
    import ctypes
    from ripcurrents_amd import _lib
    assert ctypes.sizeof(_lib.DrawPrim) == 32 == R.PRIM.itemsize
    assert [n for n, _ in _lib.DrawPrim._fields_] == list(R.PRIM.names)
    for name in ("rcflow_draw_dev", "rcflow_trace_prims_dev", "rcflow_tracers_open", "rcflow_tracers_add", "rcflow_tracers_push_dev",
                 "rcflow_tracers_read", "rcflow_tracers_prims", "rcflow_tracers_info", "rcflow_tracers_reset", "rcflow_tracers_close"):
        assert name in _lib.SIGNATURES
    assert (R.DISC, R.LINE, R.BLEND, R.COORD_MAX, R.MAX_THICKNESS) == (_lib.RC_DRAW_DISC, _lib.RC_DRAW_LINE, _lib.RC_DRAW_BLEND,
                                                                        _lib.RC_DRAW_COORD_MAX, _lib.RC_DRAW_MAX_THICKNESS)
