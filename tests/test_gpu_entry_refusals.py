"""Refusals of the stateless device entry points (analysis chain, colour, resize, post-ops, Farneback, PyrLK, draw, corners,
fit), through the C ABI: every refused call returns the code it always returned, sets a text that starts with the entry
point's name (and names the argument, for a pointer), and queues nothing.  The calls at the boundary -- every step exactly
the bytes of a row, a clip's frame stride exactly one frame -- are accepted and give what the oracle gives.

The frame is 33 x 23 (24 x 22 for the shear colouring, which returns early at <= 20): a refusal launches nothing, so nothing
larger is needed.  The refusals that need a primed stream, a primed batch, a plan or an acquired frame buffer (the flow
buffers of rcflow_push_frame_dev, rcflow_push_clip_dev and rcflow_push_batch_dev, the pointers of rc_frame_loop, the d_flow
of rcflow_debug_level_flow_ptr) have a test of their own, after the accepted calls that bring that state about.  The entry
points that take no context, and the null contexts of rcflow_profile_*, are in tests/test_cabi_and_host.py.
"""
import ctypes as C
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

from _dev import EINVAL, ESIZE, ESTATE, SENTINEL, raw
from ripcurrents_amd import synth
from ripcurrents_amd._lib import FarnebackParams, FitParams, FrameLoop
from ripcurrents_amd.api import HistState

pytestmark = pytest.mark.gpu

W, H = 33, 23
SW, SH = 24, 22                       # rcflow_shear_rate_to_color_dev
FS, S1, S3, S12 = W * 8, W, W * 3, W * 12    # the bytes of a row: float2, 8U, 8UC3, 32FC3

# one entry point: its arguments after (ctx, stream) in order, and the refused variations of them.  A variation is
# (changes, the argument the text must name or None for a scalar rule, the code the parent commit returned)
Entry = namedtuple("Entry", "name args bad head")


def _table(dev_in, dev_out, host_in, host_out):
    """dev_in / dev_out / host_in / host_out: base addresses of a zeroed device buffer, a sentinel-filled device buffer and
    the same two on the host, each 256 KiB."""
    I, I2, O = dev_in, dev_in + (64 << 10), [dev_out + (k << 15) for k in range(8)]
    HI, HI2, HO = host_in, host_in + (64 << 10), host_out
    P = C.byref(FarnebackParams(0.5, 1, 3, 1, 5, 1.1, 0))
    P_SEEDED = C.byref(FarnebackParams(0.5, 1, 3, 1, 5, 1.1, 4))       # RC_FARNEBACK_USE_INITIAL_FLOW
    FIT = C.byref(FitParams(model=1, hypotheses=0, seed=0, min_score=0, quality=0.0, max_shift=10.0, inlier_px=1.0))
    fl, i32, vp, sz = C.pointer(C.c_float(1.0)), C.pointer(C.c_int(0)), C.pointer(C.c_void_p(0)), C.pointer(C.c_size_t(0))
    T = []

    def entry(name, args, bad, head=2):
        T.append(Entry(name, args, bad, head))

    def ptr(name, step=None, align=None, row=None, who=None):
        """The refusals of one pointer argument: null, its step one byte below a row, its step off the alignment."""
        out = [({name: None}, who or name, EINVAL)]
        if step:
            out.append(({step: row - 1}, who or name, EINVAL))
            if align:
                out.append(({step: row + align // 2}, who or name, EINVAL))
        return out

    flow = [("d_flow", I), ("flow_step", FS), ("w", W), ("h", H)]
    flow_bad = ptr("d_flow", "flow_step", 8, FS)
    entry("rcflow_analysis_reset", [("w", W), ("h", H)], [({"w": 0}, None, EINVAL), ({"h": -1}, None, EINVAL), ({"w": 5000}, None, ESIZE)])
    entry("rcflow_histogram_dev", flow, flow_bad)
    entry("rcflow_histogram_clip_dev", [("d_flows", I), ("flow_frame_stride", FS * H), ("flow_step", FS), ("count", 2), ("w", W), ("h", H)],
          ptr("d_flows", "flow_step", 8, FS) + [({"flow_frame_stride": FS * (H - 1) + W * 8 - 1}, "d_flows", EINVAL), ({"count": 0}, None, EINVAL),
                                               ({"count": 65536}, None, EINVAL),
                                               # a frame stride off the 8 bytes of a float2: the rows of frame 1 would be 4-byte aligned
                                               ({"flow_frame_stride": FS * H + 4}, "d_flows", EINVAL)])
    entry("rcflow_thresholds_words_dev", [("d_words", I)], ptr("d_words"))
    entry("rcflow_histogram_write", [("words", HI)], ptr("words"))
    entry("rcflow_histogram_device_ptr", [("d_words", vp)], ptr("d_words"))
    entry("rcflow_classify_accumulate_dev",
          flow + [("framecount", 1), ("MID", 0.5), ("LOWER", 0.2), ("d_polar", O[0]), ("polar_step", S12), ("d_wclass", O[1]), ("wc_step", S12),
                  ("d_out", O[2]), ("out_step", S12), ("d_mask", O[3]), ("mask_step", S1)],
          flow_bad + [({"polar_step": S12 - 1}, "d_polar", EINVAL), ({"wc_step": S12 - 1}, "d_wclass", EINVAL), ({"out_step": S12 - 1}, "d_out", EINVAL),
                      ({"mask_step": S1 - 1}, "d_mask", EINVAL), ({"framecount": -1}, None, EINVAL)])
    entry("rcflow_accumulator_read", [("acc", HO)], ptr("acc"))
    entry("rcflow_advect_field_dev", flow + [("dt", 2.0), ("iterations", 1), ("UPPER", 1.0)],
          flow_bad + [({"iterations": -1}, None, EINVAL), ({"iterations": 1 << 30}, None, EINVAL)])
    entry("rcflow_advect_points_dev", [("d_pts", O[0]), ("n", 4)] + flow + [("dt", 2.0), ("iterations", 1), ("UPPER", 1.0), ("variant", 0), ("d_trace", None)],
          ptr("d_pts") + flow_bad + [({"n": -1}, None, EINVAL), ({"iterations": -1}, None, EINVAL), ({"variant": 5}, None, EINVAL)])
    entry("rcflow_get_delta_field_dev", [("d_pt", O[0]), ("pt_step", FS)] + flow + [("dt", 2.0), ("UPPER", 1.0)],
          ptr("d_pt", "pt_step", None, FS) + flow_bad)
    for name in ("rcflow_subtract_average_dev", "rcflow_subtract_mean_magnitude_dev", "rcflow_stabilizer_dev"):
        entry(name, [("d_flow", O[0]), ("step", FS), ("w", W), ("h", H)], ptr("d_flow", "step", 8, FS))
    entry("rcflow_window_mean_dev", [("d_avg", O[0]), ("d_slot", O[1]), ("d_cur", I), ("n", W * H * 2), ("window", 10)],
          ptr("d_avg") + ptr("d_slot") + ptr("d_cur") + [({"window": 0}, None, EINVAL)])
    entry("rcflow_vector_to_color_dev", [("d_flow", I), ("step", FS), ("w", W), ("h", H), ("d_hsv", O[0]), ("hsv_step", S3), ("max_io", fl)],
          ptr("d_flow", "step", 8, FS) + ptr("d_hsv", "hsv_step", None, S3) + ptr("max_io"))
    entry("rcflow_shear_rate_to_color_dev", [("d_flow", I), ("step", SW * 8), ("w", SW), ("h", SH), ("d_hsv", O[0]), ("hsv_step", SW * 3), ("max_io", fl)],
          ptr("d_flow", "step", 8, SW * 8) + ptr("d_hsv", "hsv_step", None, SW * 3) + ptr("max_io"))
    entry("rcflow_create_edges_dev", [("d_mask", I), ("mask_step", S1), ("w", W), ("h", H), ("d_out", O[0]), ("out_step", S1)],
          ptr("d_mask", "mask_step", None, S1) + ptr("d_out", "out_step", None, S1) + [({"d_out": I}, "d_mask", EINVAL)])     # in place
    entry("rcflow_create_output_dev", [("d_subframe_bgr", O[0]), ("step", S3), ("d_outmask", I), ("mask_step", S1), ("w", W), ("h", H)],
          ptr("d_subframe_bgr", "step", None, S3) + ptr("d_outmask", "mask_step", None, S1))
    for name, out, ch in (("rcflow_resize_bgr_to_gray_dev", "d_gray", 1), ("rcflow_resize_area_bgr_to_gray_dev", "d_gray", 1),
                          ("rcflow_resize_bgr_dev", "d_out", 3), ("rcflow_resize_area_bgr_dev", "d_out", 3)):
        ostep = "gray_step" if ch == 1 else "out_step"
        bad = ptr("d_bgr", "step", None, 2 * W * 3) + ptr(out, ostep, None, W * ch) + [({"sw": 0}, "d_bgr", EINVAL), ({"dh": 0}, out, EINVAL)]
        if "area" in name:
            bad.append(({"dw": 2 * W + 1, ostep: (2 * W + 1) * ch}, None, EINVAL))            # enlarging
        entry(name, [("d_bgr", I), ("step", 2 * W * 3), ("sw", 2 * W), ("sh", 2 * H), (out, O[0]), (ostep, W * ch), ("dw", W), ("dh", H)], bad)
    # the next two take the size from the slot's analysis state (33 x 23: the fixture resets it)
    entry("rcflow_streamline_display_dev", [("which", 0), ("d_bgr", O[0]), ("bgr_step", S3), ("max_out", None)],
          ptr("d_bgr", "bgr_step", None, S3) + [({"which": 3}, None, EINVAL), ({"which": -1}, None, EINVAL)])
    entry("rcflow_streamline_positions_dev", [("d_density", O[0]), ("density_step", S12)], ptr("d_density", "density_step", None, S12))
    entry("rcflow_hsv_to_bgr_dev", [("d_hsv", I), ("hsv_step", S12), ("w", W), ("h", H), ("d_bgr", O[0]), ("bgr_step", S12)],
          ptr("d_hsv", "hsv_step", None, S12) + ptr("d_bgr", "bgr_step", None, S12))
    entry("rcflow_analysis_size", [("w", i32), ("h", i32)], ptr("w") + ptr("h"))

    # ---- the Farneback entry points
    pair = [("d_prev", I), ("prev_step", S1), ("d_next", I2), ("next_step", S1), ("w", W), ("h", H), ("d_flow", O[0]), ("flow_step", FS)]
    entry("rcflow_farneback_dev", pair + [("p", P)],
          ptr("d_prev", "prev_step", None, S1) + ptr("d_next", "next_step", None, S1) + ptr("d_flow", "flow_step", None, FS) +
          [({"p": None}, None, EINVAL), ({"w": 5000, "prev_step": 5000, "next_step": 5000, "flow_step": 40000}, None, ESIZE)])
    entry("rcflow_farneback_u8",
          [("prev", HI), ("prev_step", S1), ("next", HI2), ("next_step", S1), ("w", W), ("h", H), ("flow", HO), ("flow_step", FS), ("pyr_scale", 0.5),
           ("levels", 1), ("winsize", 3), ("iterations", 1), ("poly_n", 5), ("poly_sigma", 1.1), ("flags", 0)],
          ptr("prev", "prev_step", None, S1) + ptr("next", "next_step", None, S1) + ptr("flow", "flow_step", None, FS) +
          [({"w": 0}, "prev", EINVAL), ({"winsize": 0}, None, EINVAL)])
    entry("rcflow_push_frame_dev", [("d_frame", I), ("step", S1), ("w", W), ("h", H), ("d_flow", O[0]), ("flow_step", FS), ("p", P)],
          ptr("d_frame", "step", None, S1))
    entry("rcflow_push_frame_u8", [("frame", HI), ("step", S1), ("w", W), ("h", H), ("p", P)], ptr("frame", "step", None, S1) + [({"h": 0}, "frame", EINVAL)])
    entry("rcflow_frame_buffer_acquire", [("w", W), ("h", H), ("host_frame", vp), ("step", sz)],
          ptr("host_frame") + [({"w": 0}, None, EINVAL), ({"h": 5000}, None, ESIZE)])
    entry("rcflow_stream_flow_ptr", [("d_flow", vp), ("w", i32), ("h", i32)], ptr("d_flow") + [({}, None, ESTATE)])           # the fixture reset the stream
    entry("rcflow_stream_flow_read", [("flow", HO), ("flow_step", FS)], ptr("flow") + [({}, None, ESTATE)])
    clip = [("d_frames", I), ("frame_stride", S1 * H), ("step", S1), ("nframes", 3), ("w", W), ("h", H), ("d_flows", O[0]), ("flow_frame_stride", FS * H),
            ("flow_step", FS), ("p", P)]
    frames_bad = ptr("d_frames", "step", None, S1) + [({"frame_stride": S1 * (H - 1) + W - 1}, "d_frames", EINVAL)]
    entry("rcflow_push_clip_dev", clip, frames_bad + [({"nframes": 0}, None, EINVAL), ({"p": P_SEEDED}, None, EINVAL)])
    entry("rcflow_farneback_clip_dev", clip,
          frames_bad + ptr("d_flows", "flow_step", None, FS) + [({"flow_frame_stride": FS * (H - 1) + W * 8 - 1}, "d_flows", EINVAL),
                                                                ({"nframes": 1}, None, EINVAL), ({"p": P_SEEDED}, None, EINVAL)])
    entry("rcflow_push_batch_dev", [(("nstreams", v) if n == "nframes" else (n, v)) for n, v in clip] + [("use_graph", 0)],
          frames_bad + [({"nstreams": 0}, None, EINVAL), ({"nstreams": 4097}, None, EINVAL)])
    entry("rcflow_frame_loop_step", [("p", P), ("loop", C.byref(FrameLoop()))], ptr("p") + ptr("loop"))        # the null checks come before `loop` is read
    entry("rcflow_stage_pyr_level_dev", [("d_img", I), ("step", S1), ("w", W), ("h", H), ("pyr_scale", 0.5), ("k", 1), ("d_out", O[0])],
          ptr("d_img") + ptr("d_out") + [({"k": -1}, None, EINVAL), ({"k": 12}, None, EINVAL), ({"pyr_scale": 1.0}, None, EINVAL)])
    entry("rcflow_stage_polyexp_dev", [("d_I", I), ("w", W), ("h", H), ("poly_n", 5), ("poly_sigma", 1.1), ("d_R5", O[0])],
          ptr("d_I") + ptr("d_R5") + [({"w": 0}, None, EINVAL), ({"poly_n": 0}, None, EINVAL), ({"poly_n": 33}, None, EINVAL)])
    entry("rcflow_stage_flow_iter_dev", [("d_R0", I), ("d_R1", I2), ("d_flow_in", None), ("w", W), ("h", H), ("winsize", 3), ("flags", 0), ("d_flow_out", O[0])],
          ptr("d_R0") + ptr("d_R1") + ptr("d_flow_out") + [({"h": 0}, None, EINVAL), ({"winsize": 0}, None, EINVAL), ({"winsize": 50}, None, EINVAL),
                                                          ({"flags": 1}, None, EINVAL)])
    entry("rcflow_stage_initial_flow_dev", [("d_flow_xy", I), ("flow_step", FS), ("w", W), ("h", H), ("pyr_scale", 0.5), ("levels", 1), ("d_out", O[0])],
          ptr("d_flow_xy", "flow_step", 8, FS) + ptr("d_out") + [({"d_flow_xy": I + 4}, "d_flow_xy", EINVAL), ({"levels": -1}, None, EINVAL),
                                                                 ({"levels": 12}, None, EINVAL), ({"pyr_scale": 0.0}, None, EINVAL)])
    entry("rcflow_set_option", [("name", b"chunk"), ("value", 8)],
          [({"name": None}, "name", EINVAL), ({"name": b"no_such_option"}, None, EINVAL)] +
          [({"name": n, "value": v}, None, EINVAL) for n, v in ((b"chunk", 0), (b"chunk", 65), (b"exact", 2), (b"exact", -2), (b"chain", 0), (b"chain", 65),
                                                                (b"chain_min_blocks", -1), (b"hist_blocks", -1), (b"hist_blocks", 65536),
                                                                (b"frame_overlap", 3), (b"frame_overlap", -1), (b"poly_tile_h", 40))], head=1)
    entry("rcflow_debug_level_flow_ptr", [("level", 0), ("which", 0), ("d_flow", vp), ("w", i32), ("h", i32)], [({"level": -1}, None, EINVAL), ({"level": 99}, None, EINVAL)])

    # ---- PyrLK at its smallest configuration (a 3 x 3 window on level 0), draw, corners, fit
    def lk(d):
        args = [(d + "prev", I if d else HI), ("prev_step", S1), (d + "next", I2 if d else HI2), ("next_step", S1), ("w", W), ("h", H),
                (d + "prev_pts", I if d else HI), (d + "next_pts", O[0] if d else HO), ("npts", 4), (d + "status", O[1] if d else HO + 4096), (d + "err", None),
                ("win_w", 3), ("win_h", 3), ("max_level", 0), ("crit_type", 3), ("max_count", 30), ("epsilon", 0.01), ("flags", 0), ("min_eig_threshold", 1e-4)]
        bad = (ptr(d + "prev", "prev_step", None, S1) + ptr(d + "next", "next_step", None, S1) + ptr(d + "prev_pts") + ptr(d + "next_pts") + ptr(d + "status") +
               [({"npts": -1}, None, EINVAL), ({"w": 0}, d + "prev", EINVAL)])
        return args, bad
    window_bad = [({"win_w": 2}, None, EINVAL), ({"win_h": 2}, None, EINVAL), ({"max_level": -1}, None, EINVAL), ({"max_level": 64}, None, EINVAL),
                  ({"win_w": 129, "win_h": 128}, None, EINVAL)]
    args, bad = lk("d_")
    entry("rcflow_pyrlk_dev", args, bad + window_bad)
    args, bad = lk("")
    entry("rcflow_pyrlk_u8", args, bad)               # (its window rules are the device form's, reached after the upload was queued)
    entry("rcflow_draw_dev", [("d_img", O[0]), ("step", S3), ("w", W), ("h", H), ("channels", 3), ("d_prims", I), ("n", 1), ("d_skipped", None)],
          ptr("d_img", "step", None, S3) + ptr("d_prims") + [({"d_prims": I + 8}, "d_prims", EINVAL), ({"d_skipped": O[1] + 4}, "d_skipped", EINVAL),
                                                              ({"channels": 2}, None, EINVAL), ({"n": -1}, None, EINVAL),
                                                              ({"w": 16385, "step": 3 * 16385}, None, ESIZE), ({"n": (1 << 24) + 1}, None, ESIZE)])
    entry("rcflow_trace_prims_dev", [("d_start", None), ("d_trace", I), ("n", 2), ("iters", 3), ("color", 0xffffff), ("d_prims", O[0])],
          ptr("d_trace") + ptr("d_prims") + [({"d_prims": O[0] + 8}, "d_prims", EINVAL), ({"n": -1}, None, EINVAL), ({"iters": 0}, None, EINVAL),
                                             ({"iters": 65537}, None, EINVAL), ({"n": 1 << 20, "iters": 64}, None, ESIZE)])
    entry("rcflow_corners_dev", [("d_gray", I), ("step", S1), ("w", W), ("h", H), ("cells_x", 1), ("cells_y", 1), ("margin", 2), ("min_score", 1),
                                 ("d_pts", O[0]), ("d_scores", O[1])],
          ptr("d_gray", "step", None, S1) + ptr("d_pts") + ptr("d_scores") + [({"margin": 1}, None, EINVAL), ({"cells_x": 0}, None, EINVAL),
                                                                             ({"cells_x": 4}, None, EINVAL)])
    entry("rcflow_fit_motion_dev", [("d_p", I), ("d_q", I2), ("d_status", I), ("d_scores", None), ("n", 4), ("w", W), ("h", H), ("prm", FIT),
                                    ("d_result", O[0]), ("d_inlier", O[1]), ("d_samples", None)],
          ptr("d_p") + ptr("d_q") + ptr("d_status") + ptr("d_result") + ptr("d_inlier") + [({"n": -1}, None, EINVAL), ({"prm": None}, None, EINVAL)])
    return T


def refused_calls(ctx, table):
    """Makes every refused call of the table: (entry point, changes, named argument, expected code, returned code, text,
    whether the text is still the planted one)."""
    lib, hdl = raw(ctx)
    rows = []
    for e in table:
        fn = getattr(lib, e.name)
        names = [n for n, _ in e.args]
        for changes, named, code in e.bad:
            assert set(changes) <= set(names), (e.name, changes)
            vals = [changes.get(n, v) for n, v in e.args]
            assert lib.rcflow_sync(hdl, 2) == EINVAL                  # slot index = nstreams: plants a text of another call
            planted = lib.rcflow_last_error()
            rc = fn(*([hdl, 0][:e.head] + vals))
            text = (lib.rcflow_last_error() or b"").decode()
            rows.append((e.name, changes, named, code, rc, text, text == planted.decode()))
    return rows


@pytest.fixture()
def buffers(ctx):
    dev_in = torch.zeros(256 << 10, dtype=torch.uint8, device="cuda")
    dev_out = torch.full((256 << 10,), SENTINEL, dtype=torch.uint8, device="cuda")
    host_in, host_out = np.zeros(256 << 10, np.uint8), np.full(256 << 10, SENTINEL, np.uint8)
    torch.cuda.synchronize()
    ctx._bind(0)
    ctx.analysis_reset(W, H)
    ctx.stream_reset()
    ctx.batch_reset()
    return dev_in, dev_out, host_in, host_out


def primed_refusals(ctx, dev_in, dev_out):
    """The refusals that come after state: primes the stream, then the batch, acquires a frame buffer, and makes the refused
    calls of each state in between.  The accepted calls queue work on dev_in only.  Rows as refused_calls gives them."""
    lib, hdl = raw(ctx)
    I, O = dev_in, dev_out
    p = FarnebackParams(0.5, 1, 3, 1, 5, 1.1, 0)
    P = C.byref(p)
    vp, i32 = C.pointer(C.c_void_p(0)), C.pointer(C.c_int(0))
    flows = [("d_flows", O), ("flow_frame_stride", FS * H), ("flow_step", FS), ("p", P)]
    flows_bad = [({"d_flows": None}, "d_flows", EINVAL), ({"flow_step": FS - 1}, "d_flows", EINVAL),
                 ({"flow_frame_stride": FS * (H - 1) + W * 8 - 1}, "d_flows", EINVAL)]
    clip = [("d_frames", I), ("frame_stride", S1 * H), ("step", S1), ("nframes", 3), ("w", W), ("h", H)]
    assert lib.rcflow_stream_reset(hdl, 0) == 0
    assert lib.rcflow_push_frame_dev(hdl, 0, I, S1, W, H, None, 0, P) == 1                     # primes the stream: no flow buffer asked yet
    rows = refused_calls(ctx, [
        Entry("rcflow_push_frame_dev", [("d_frame", I), ("step", S1), ("w", W), ("h", H), ("d_flow", O), ("flow_step", FS), ("p", P)],
              [({"d_flow": None}, "d_flow", EINVAL), ({"flow_step": FS - 1}, "d_flow", EINVAL)], 2),
        Entry("rcflow_push_clip_dev", clip + flows, flows_bad, 2),
        Entry("rcflow_debug_level_flow_ptr", [("level", 0), ("which", 0), ("d_flow", vp), ("w", i32), ("h", i32)], [({"d_flow": None}, "d_flow", EINVAL)], 2)])
    batch = [(("nstreams", 2) if n == "nframes" else (n, v)) for n, v in clip]
    assert lib.rcflow_push_batch_dev(hdl, 0, I, S1 * H, S1, 2, W, H, None, 0, 0, P, 0) == 1    # primes the batch
    rows += refused_calls(ctx, [Entry("rcflow_push_batch_dev", batch + flows + [("use_graph", 0)], flows_bad, 2)])
    assert lib.rcflow_batch_reset(hdl, 0) == 0
    assert lib.rcflow_frame_buffer_acquire(hdl, 0, W, H, C.pointer(C.c_void_p(0)), None) == 0
    loops = [FrameLoop(dt=2.0, iterations=1, nseeds=2), FrameLoop(dt=2.0, iterations=1, d_edges=O), FrameLoop(dt=2.0, iterations=1, nseeds=-1),
             FrameLoop(dt=2.0, iterations=-1)]
    rows += refused_calls(ctx, [Entry("rcflow_frame_loop_step", [("p", P), ("loop", C.byref(loops[0]))],
                                      [({"loop": C.byref(loops[0])}, "loop->d_seeds", EINVAL), ({"loop": C.byref(loops[1])}, "loop->d_outmask", EINVAL),
                                       ({"loop": C.byref(loops[2])}, None, EINVAL), ({"loop": C.byref(loops[3])}, None, EINVAL)], 2)])
    assert lib.rcflow_push_frame_acquired(hdl, 0, P) == 1                                      # hands the acquired buffer back (a priming push)
    assert lib.rcflow_stream_reset(hdl, 0) == 0
    return rows


def _wrong(rows):
    wrong = []
    for name, changes, named, code, rc, text, stale in rows:
        what = None
        if rc != code:
            what = "returned %d, the parent commit %d" % (rc, code)
        elif stale:
            what = "left the text of an earlier call"
        elif not text.startswith(name + ":"):
            what = "a text that does not start with its name"
        elif named is not None and not re.search(r"\b%s\b" % re.escape(named), text[len(name):]):
            what = "a text that does not name " + named
        if what:
            wrong.append("%s %r: %s (\"%s\")" % (name, changes, what, text))
    return wrong


def test_every_refusal_keeps_its_code_names_itself_and_queues_nothing(ctx, buffers):
    dev_in, dev_out, host_in, host_out = buffers
    table = _table(dev_in.data_ptr(), dev_out.data_ptr(), host_in.ctypes.data, host_out.ctypes.data)
    assert len(table) >= 50 and len({e.name for e in table}) == len(table)
    rows = refused_calls(ctx, table)
    print("[refusals] %d refused calls of %d entry points" % (len(rows), len(table)))
    wrong = _wrong(rows)
    assert not wrong, "\n".join(wrong)
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((dev_out == SENTINEL).all()) and (host_out == SENTINEL).all() and not bool(dev_in.any()) and not host_in.any()
    # the slot kept its analysis size
    w, h = C.c_int(), C.c_int()
    assert ctx._lib.rcflow_analysis_size(ctx._h, 0, C.byref(w), C.byref(h)) == 0 and (w.value, h.value) == (W, H)


def test_refusals_after_priming_acquiring_and_planning(ctx, buffers):
    """Asked only once the stream or the batch is primed, a frame buffer acquired or a plan built: the same assertions on the code
    and the text; the outputs named in the refused calls keep their sentinel."""
    dev_in, dev_out, host_in, host_out = buffers
    rows = primed_refusals(ctx, dev_in.data_ptr(), dev_out.data_ptr())
    print("[refusals] %d refused calls after state" % len(rows))
    wrong = _wrong(rows)
    assert len(rows) == 13 and not wrong, "\n".join(wrong)
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((dev_out == SENTINEL).all()) and not bool(dev_in.any())


def test_level_diagnostics_refuse_without_a_plan_and_outside_it(ctx, buffers):
    """rcflow_debug_level_R / rcflow_debug_level_image (not part of include/rcflow.h): RC_ESTATE while the slot has no plan (an
    option change drops it), RC_EINVAL for a level or a ring entry outside the plan, a null or misaligned output and scale 0's
    image on the fast path; nothing is written."""
    dev_in, dev_out, host_in, host_out = buffers
    I, O = dev_in.data_ptr(), dev_out.data_ptr()
    i32 = C.pointer(C.c_int(0))
    P = C.byref(FarnebackParams(0.5, 1, 3, 1, 5, 1.1, 0))
    names = (("rcflow_debug_level_R", "d_R5"), ("rcflow_debug_level_image", "d_I"))

    def entries(bad_of):
        return [Entry(name, [("level", 0), ("slot", 0), (out, O), ("w", i32), ("h", i32)], bad_of(name, out), 2) for name, out in names]

    ctx.set_option("chunk", 32)                  # its default: every slot's plan is dropped
    rows = refused_calls(ctx, entries(lambda name, out: [({}, None, ESTATE), ({"level": 99}, None, ESTATE), ({out: None}, None, ESTATE)]))
    # a plan of 2 scales (33 x 23 is cropped to scale 0 alone at levels = 1; 80 x 72 keeps scale 1) and chunk + 1 = 33 entries
    w, h = 80, 72
    assert ctx._lib.rcflow_level_geometry(w, h, 0.5, 1, 0, None, None) == 1
    assert ctx._lib.rcflow_farneback_dev(ctx._h, 0, I, w, I + w * h, w, w, h, I + (64 << 10), w * 8, P) == 0
    rows += refused_calls(ctx, entries(lambda name, out: [({"level": -1}, None, EINVAL), ({"level": 2}, None, EINVAL), ({"slot": -1}, None, EINVAL),
                                                          ({"slot": 33}, None, EINVAL), ({out: None}, out, EINVAL), ({out: O + 2}, out, EINVAL)] +
                                       ([({}, None, EINVAL)] if name.endswith("image") else [])))
    print("[refusals] %d refused calls of the level diagnostics" % len(rows))
    wrong = _wrong(rows)
    assert len(rows) == 19 and not wrong, "\n".join(wrong)
    # accepted at the edge of the plan: the last scale, the last ring entry
    for name, _ in names:
        assert getattr(ctx._lib, name)(ctx._h, 0, 1, 32, I + (128 << 10), i32, i32) == 0 and i32.contents.value == 36
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((dev_out == SENTINEL).all())


def test_level_flow_diagnostic_refuses_without_a_plan_and_outside_it(ctx, buffers):
    """rcflow_debug_level_flow (not part of include/rcflow.h; the copy form of rcflow_debug_level_flow_ptr): RC_ESTATE while the
    slot has no plan, RC_EINVAL for a level, a buffer or a pair outside the plan and for a null or misaligned output; nothing is
    written.  Accepted at the edge of the plan: the last scale, buffer B, the plan's last pair."""
    dev_in, dev_out, host_in, host_out = buffers
    I, O = dev_in.data_ptr(), dev_out.data_ptr()
    i32 = C.pointer(C.c_int(0))
    P = C.byref(FarnebackParams(0.5, 1, 3, 2, 5, 1.1, 0))
    name = "rcflow_debug_level_flow"
    args = [("level", 0), ("which", 0), ("pair", 0), ("d_out", O), ("w", i32), ("h", i32)]
    ctx.set_option("chunk", 32)                  # its default: every slot's plan is dropped
    rows = refused_calls(ctx, [Entry(name, args, [({}, None, ESTATE), ({"level": 99}, None, ESTATE), ({"d_out": None}, None, ESTATE)], 2)])
    w, h = 80, 72                                # two scales (see the test above), chunk 32
    assert ctx._lib.rcflow_farneback_dev(ctx._h, 0, I, w, I + w * h, w, w, h, I + (64 << 10), w * 8, P) == 0
    rows += refused_calls(ctx, [Entry(name, args, [({"level": -1}, None, EINVAL), ({"level": 2}, None, EINVAL), ({"which": -1}, None, EINVAL),
                                                   ({"which": 2}, None, EINVAL), ({"pair": -1}, None, EINVAL), ({"pair": 32}, None, EINVAL),
                                                   ({"d_out": None}, "d_out", EINVAL), ({"d_out": O + 2}, "d_out", EINVAL)], 2)])
    wrong = _wrong(rows)
    assert len(rows) == 11 and not wrong, "\n".join(wrong)
    assert ctx._lib.rcflow_debug_level_flow(ctx._h, 0, 1, 1, 31, I + (128 << 10), i32, i32) == 0 and i32.contents.value == 36
    ctx.sync()
    torch.cuda.synchronize()
    assert bool((dev_out == SENTINEL).all())


def test_stage_polyexp_takes_a_negative_sigma_as_the_default(ctx):
    """Accepted, as it always was: the plan arithmetic reads any poly_sigma below FLT_EPSILON as 0.3 n (rc_plan.cpp), so -1 gives the
    planes of 0, bit for bit; the level drivers refuse a negative sigma, this stage entry point never did."""
    img = torch.as_tensor(synth.surf_clip(W, H, 1, seed=9)[0].astype(np.float32)).cuda()
    want = ctx.stage_polyexp(img, poly_n=5, poly_sigma=0.0)
    got = ctx.stage_polyexp(img, poly_n=5, poly_sigma=-1.0)
    assert torch.equal(got, want) and bool(want.abs().sum() > 0)
    assert not torch.equal(want, ctx.stage_polyexp(img, poly_n=5, poly_sigma=1.1))


# ---------------------------------------------------------------------------- the accepted boundary
def _field(w, h, seed, scale=1.5):
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = np.stack([0.8 * np.sin(xs / 7.0) + 0.3 * np.cos(ys / 5.0), 0.6 * np.cos(xs / 9.0 + ys / 4.0)], -1) + 0.05 * rng.randn(h, w, 2)
    return (scale * f).astype(np.float32)


def test_analysis_chain_at_the_exact_steps(ctx, orc):
    """Dense tensors: every step is exactly the bytes of a row.  The statements are those of tests/test_gpu_analysis.py."""
    w, h = W, H
    rng = np.random.RandomState(1)
    f = _field(w, h, 1)
    ctx.analysis_reset(w, h)
    st, ost = HistState(), orc.HistState()
    ctx.create_histogram(f, st)
    polar = orc.flow_to_polar(f)
    orc.create_histogram(polar, ost)
    assert np.array_equal(st.hist2d, ost.hist2d) and st.histsum == ost.histsum.value and st.UPPER == ost.UPPER
    outs = ctx.create_flow_accumulate(f, 40)
    wc, acc2 = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    orc.create_flow(polar, wc, acc2, ost.UPPER, 0.5, 0.2, ost.UPPER2d)
    acc, out, mask = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.uint8)
    orc.create_accumulationbuffer(acc, acc2, out, mask, 40)
    assert np.array_equal(outs["waterclass"].cpu().numpy(), wc) and np.array_equal(outs["polar"].cpu().numpy(), polar)
    assert np.array_equal(outs["out"].cpu().numpy(), out) and np.array_equal(outs["outmask"].cpu().numpy(), mask)
    assert np.array_equal(ctx.accumulator(w, h), acc[..., 0])
    assert np.array_equal(ctx.hsv_to_bgr(outs["polar"]).cpu().numpy(), orc.hsv_to_bgr(polar))
    blobs = (rng.rand(h, w) > 0.9).astype(np.uint8) * 255
    edges = ctx.create_edges(blobs).cpu().numpy()
    assert np.array_equal(edges, orc.create_edges(blobs)) and edges.any()
    frame = rng.randint(0, 255, (h, w, 3)).astype(np.uint8)
    ref = frame.copy(); ref[..., 2][edges > 0] = 255
    assert np.array_equal(ctx.create_output(frame, edges).cpu().numpy(), ref)
    # advection, display
    pt, dist = np.zeros((h, w, 2), np.float32), np.zeros((h, w), np.float32)
    for _ in range(2):
        ctx.streamline_field(f, 2.0, 1, UPPER=100.0)
        orc.streamline_field(pt, dist, f, 2.0, 1, 100.0)
    gpt, gdist = ctx.streamline_field_state(w, h)
    assert np.array_equal(gpt, pt) and np.array_equal(gdist, dist)
    for which in (0, 1, 2):
        assert np.array_equal(ctx.streamline_display(which)[0].cpu().numpy(), orc.streamline_display(pt, dist, which)[0])
    assert np.array_equal(ctx.streamline_positions().cpu().numpy(), orc.streamline_positions(pt))
    seeds = np.stack([rng.uniform(-2, w + 2, 9), rng.uniform(-2, h + 2, 9)], axis=1).astype(np.float32)
    ref_seeds = seeds.copy()
    moved, _ = ctx.streamline(seeds, f, 2.0, 3, 100.0, variant=3)
    orc.streamline_points(ref_seeds, f, 2.0, 3, 100.0, variant=3)
    assert np.array_equal(moved.cpu().numpy(), ref_seeds)
    ref = np.zeros((h, w, 2), np.float32)
    orc.get_delta_field(ref, f, 2.0, 1.8)
    assert np.array_equal(ctx.get_delta_field(torch.zeros((h, w, 2), device="cuda"), f, 2.0, 1.8).cpu().numpy(), ref)
    # post-ops (the tolerances of test_flow_postops: one ulp of the double mean; 1e-4 relative on the float running sum)
    for gpu, cpu in ((ctx.subtructAverage, orc.subtract_average), (ctx.stabilizer, orc.stabilizer)):
        og = f.copy(); cpu(og)
        assert np.abs(gpu(f.copy()).cpu().numpy() - og).max() <= 2.4e-7 * max(1.0, np.abs(og).max())
    og = f.copy(); orc.subtract_mean_magnitude(og)
    mean_mag = np.sqrt((f.astype(np.float64) ** 2).sum(-1)).mean()
    assert np.abs(ctx.subtructMeanMagnitude(f.copy()).cpu().numpy() - og).max() <= 1e-4 * mean_mag + 1e-6
    avg, slot = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 2), np.float32)
    davg, dslot = torch.as_tensor(avg).cuda(), torch.as_tensor(slot).cuda()
    for t in range(2):
        cur = _field(w, h, 20 + t)
        orc.window_mean_update(avg, slot, cur, 10)
        ctx.window_mean(davg, dslot, torch.as_tensor(cur).cuda(), 10)
    assert np.array_equal(davg.cpu().numpy(), avg) and np.array_equal(dslot.cpu().numpy(), slot)
    # colour
    ref, md = orc.vector_to_color(f, 0.7)
    got, gmd = ctx.vectorToColor(f, 0.7)
    assert gmd == md and np.array_equal(got.cpu().numpy(), ref)
    fs = _field(SW, SH, 3)
    ref, mf = orc.shear_rate_to_color(fs, 0.4)
    got, gmf = ctx.shearRateToColor(fs, 0.4)
    assert gmf == mf and mf > 0 and np.array_equal(got.cpu().numpy(), ref)
    # resize
    big = rng.randint(0, 256, (2 * h + 1, 2 * w + 3, 3)).astype(np.uint8)
    assert np.array_equal(ctx.resize_bgr_to_gray(big, w, h).cpu().numpy(), orc.resize_bgr_to_gray(big, w, h))
    assert np.array_equal(ctx.resize_bgr_to_gray(big, w, h, interpolation="area").cpu().numpy(), orc.resize_area_bgr_to_gray(big, w, h))


def test_clips_with_the_stride_of_exactly_one_frame(ctx, orc):
    """Three dense fields / frames one after the other: frame_stride = step * (h - 1) + the bytes of a row."""
    w, h = W, H
    flows = np.stack([_field(w, h, 30 + t) for t in range(3)])
    ctx.analysis_reset(w, h)
    ost = orc.HistState()
    d = torch.as_tensor(flows).cuda()
    assert d.stride(0) * 4 == FS * (h - 1) + w * 8
    ctx.histogram_accumulate_clip(d)
    for t in range(3):
        orc.histogram_accumulate(orc.flow_to_polar(flows[t]), ost)
    st = ctx.histogram_read()
    assert np.array_equal(st.hist2d, ost.hist2d) and st.histsum == ost.histsum.value
    # the clip call solves the same pairs as the two-image call
    kw = dict(pyr_scale=0.5, levels=2, winsize=5, iterations=2, poly_n=5, poly_sigma=1.1, flags=0)
    clip = torch.as_tensor(synth.surf_clip(w, h, 3, seed=4)).cuda()
    assert clip.stride(0) == S1 * (h - 1) + w
    got = ctx.farneback_clip(clip, **kw)
    assert got.stride(0) * 4 == FS * (h - 1) + w * 8
    for t in range(2):
        assert np.array_equal(got[t].cpu().numpy(), ctx.calcOpticalFlowFarneback(clip[t], clip[t + 1], None, **kw).cpu().numpy()), t
    ctx.stream_reset()
    pushed = ctx.push_clip(clip, **kw)
    assert pushed.shape[0] == 2 and np.array_equal(pushed.cpu().numpy(), got.cpu().numpy())
    ctx.stream_reset()


def test_pyrlk_at_its_smallest_configuration(ctx, orc):
    w, h = W, H
    fr = synth.surf_clip(w, h, 2, seed=6)
    rng = np.random.RandomState(2)
    pts = np.stack([rng.uniform(2, w - 3, 12), rng.uniform(2, h - 3, 12)], 1).astype(np.float32)
    q, st, er = ctx.calcOpticalFlowPyrLK(fr[0], fr[1], pts, win=(3, 3), max_level=0)
    with np.errstate(all="ignore"):
        rq, rst, rer = orc.pyrlk(fr[0], fr[1], pts, win=(3, 3), max_level=0, exact_sums=True)
    st = st.cpu().numpy()
    assert np.array_equal(st, rst)
    ok = st > 0
    assert np.array_equal(q.cpu().numpy()[ok], rq[ok]) and np.array_equal(er.cpu().numpy()[ok], rer[ok])
