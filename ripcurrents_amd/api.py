"""Host-side mirror of the reference's interface for the hot path, over librcflow's C ABI.

Names, argument order and meaning follow the reference (paths relative to
/root/reference/RipCurrents_main):
  calcOpticalFlowFarneback   cv:: call at ripcurrents.cpp:215, main.cpp:264,...
  create_histogram           ripcurrents_module.cpp:89-144   (ripcurrents.hpp:39)
  create_flow                ripcurrents_module.cpp:153-182  (ripcurrents.hpp:50)
  create_accumulationbuffer  ripcurrents_module.cpp:189-212  (ripcurrents.hpp:52)
  streamline_field           ripcurrents_module.cpp:608-648  (ripcurrents.hpp:22)
  streamline / _2 / _3       ripcurrents_module.cpp:486-606  (ripcurrents.hpp:23-25)
  get_delta                  ripcurrents_module.cpp:650-679  (ripcurrents.hpp:58)
  Streakline                 Streakline.hpp:8-20, Streakline.cpp:11-71
  subtructAverage / subtructMeanMagnitude / stabilizer / vectorToColor / shearRateToColor
  timex_*                    compute_timex main.cpp:1195-1263, compute_brightColor main.cpp:1265-1383
  framestab_*                compute_phaseCorrelate main.cpp:1684-1775 (phase_correlate, warp_translate: its stages)
  ripmap_*                   averageVector ripcurrents_module.cpp:386-484, finished (the opposing-flow map)
  motion_* / globalOrientation  ripcurrents_module.cpp:319-359: motion history, gradient and orientation kept on the device
  tracers_* / draw           compute_streaklines / compute_timelines / compute_populationMap main.cpp:78-176 with the vertices
                             and the drawing (Streakline.cpp:57-66, ripcurrents_module.cpp:800-805, :1186-1194) on the device

torch is used for device memory and streams only; all compute is in the HIP library.
Arrays cross this layer as torch CUDA tensors (zero copy) or numpy arrays (copied).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import FarnebackParams, HIST_BINS, HIST_DIRECTIONS, HIST_WORDS, RC_FARNEBACK_USE_INITIAL_FLOW, TIMEX_PRODUCTS, RcflowError, check
from ._lib import RC_STAB_ANCHOR_FIRST, RC_STAB_MAX_PATCHES, RC_WARP_INVERSE_MAP, STAB_MODELS, FIT_MODELS, FitParams, StabTracks
from ._lib import RC_RIPMAP_WAIT_FULL, RIPMAP_SOURCES
from ._lib import TRACERS_MOVERS, TRACER_KINDS, TracersInfo, TracersParams
from ._lib import RegionsInfo, RegionsParams
from ._lib import TracksInfo, TracksParams
from ._lib import RC_MOTION_AUTO_TIME, RC_MOTION_FRESH, MotionInfo, MotionParams
from ._lib import FTLE_DIRECTIONS, FtleInfo, FtleParams
from ._lib import PlanViewInfo, PlanViewParams
from ._lib import WavesInfo, WavesParams
from ._lib import RC_PIV_REPLACE, PivInfo, PivParams
from ._lib import RC_TRANSECTS_FLOW, RC_TRANSECTS_GRAY, RC_TRANSECTS_SUMS, TransectLine, TransectsInfo, TransectsParams
from ._lib import RC_KINEMATICS_MAX_RADIUS, RC_KINEMATICS_RELATIVE, RC_KINEMATICS_SUMS, KinematicsInfo, KinematicsParams
from ._lib import RC_SHORE_HIST, SHORE_SOURCES, ShorelineInfo, ShorelineParams
from ._lib import RC_SURF_MAX_CHANNELS, SurfInfo, SurfParams
from ._lib import RC_MEANFLOW_DIR_FIXED, RC_MEANFLOW_DIR_OPPOSED, RC_MEANFLOW_SUMS, MeanflowInfo, MeanflowParams
from ._lib import RC_FLOWCHECK_FILL_NAN, RC_FLOWCHECK_FILL_ZERO, RC_FLOWCHECK_SUMMARY, RC_FLOWCHECK_SUMS, RC_FLOWCHECK_TESTS, FlowcheckInfo, FlowcheckParams
from ._lib import RC_DRIFTERS_HIST_BINS, RC_DRIFTERS_RESPAWN, RC_DRIFTERS_SUMMARY, RC_DRIFTERS_SUMS, DriftersInfo, DriftersParams
from ._lib import RC_INFILL_LEAVE_NAN, RC_INFILL_LEAVE_ZERO, RC_INFILL_SUMMARY, RC_INFILL_SUMS, InfillInfo, InfillParams
from ._lib import RC_OFFSHORE_STATION_X, RC_OFFSHORE_STATION_Y, RC_OFFSHORE_SUMMARY, RC_OFFSHORE_SUMS, OffshoreInfo, OffshoreParams
from ._lib import RC_OUTLINES_SUMMARY, OutlinesInfo, OutlinesParams

__all__ = ["Context", "FarnebackParams", "Streakline", "Timeline", "PopulationMap", "HistState", "Waves", "Piv", "Transects", "Kinematics",
           "Shoreline", "Surf", "MeanFlow", "FlowCheck", "Drifters", "Infill", "Offshore", "Outlines"]


# rc_draw_prim as a numpy record (32 bytes): what Context.draw takes and Context.tracers_prims returns
DRAW_PRIM_DTYPE = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"),
                            ("color", "<u4"), ("flags", "<u4")])

# rc_region as a numpy record (144 bytes): what Context.regions_read returns
REGION_DTYPE = np.dtype([("label", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                         ("first_x", "<i4"), ("first_y", "<i4"), ("edges", "<i4"), ("bad", "<i4"),
                         ("sx", "<i8"), ("sy", "<i8"), ("sxx", "<i8"), ("syy", "<i8"), ("sxy", "<i8"), ("fx", "<i8"), ("fy", "<i8"),
                         ("cx", "<f8"), ("cy", "<f8"), ("var_major", "<f8"), ("var_minor", "<f8"), ("angle", "<f8"),
                         ("mean_fx", "<f4"), ("mean_fy", "<f4")])
# the eight words of a regions summary, in order
REGIONS_SUMMARY = ("components", "kept", "records", "foreground", "kept_pixels", "bad_pixels", "pushes", "largest_area")
# the eight words of an FTLE, a plan view, a waves and a PIV summary, in order
FTLE_SUMMARY = ("held", "valid", "mask", "stopped", "max_lam_bits", "pushes", "reserved0", "reserved1")
PLANVIEW_SUMMARY = ("usable", "seen", "valid", "max_speed2_bits", "pushes", "reserved0", "reserved1", "reserved2")
WAVES_SUMMARY = ("held", "participating", "nonempty", "with_depth", "pushes", "reserved0", "reserved1", "reserved2")
PIV_SUMMARY = ("pairs", "cells", "valid", "flat", "lowpeak", "edge", "outliers", "pushes")
# rc_wave_cell as a numpy record (32 bytes): what Context.waves_read returns
WAVE_CELL_DTYPE = np.dtype([("bin", "<i4"), ("flags", "<i4"), ("freq_hz", "<f4"), ("kx", "<f4"), ("ky", "<f4"), ("celerity", "<f4"),
                            ("depth", "<f4"), ("quality", "<f4")])
# rc_piv_cell as a numpy record (32 bytes): what Context.piv_read returns
PIV_CELL_DTYPE = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("peak", "<f4"), ("resid", "<f4"), ("ix", "<i4"), ("iy", "<i4"), ("flags", "<i4"),
                           ("pairs", "<i4")])
# the eight words of a transects summary, in order
TRANSECTS_SUMMARY = ("held", "pairs", "with_velocity", "with_jet", "jets", "bad", "pushes", "reserved")
# rc_transect as a numpy record (64 bytes): what Context.transects_read returns
TRANSECT_DTYPE = np.dtype([("flags", "<i4"), ("pairs", "<i4"), ("peak_shift", "<i4"), ("v_along", "<f4"), ("corr_peak", "<f4"),
                           ("mean_along", "<f4"), ("mean_cross", "<f4"), ("flux_out", "<f4"), ("flux_in", "<f4"), ("jets", "<i4"),
                           ("jet_start", "<i4"), ("jet_len", "<i4"), ("jet_flux", "<f4"), ("jet_peak", "<f4"), ("jet_peak_at", "<i4"), ("bad", "<i4")])
# rc_transect_sample (16 bytes) and rc_transect_geom (48 bytes): what transects_plan and Context.transects_table return
TRANSECT_SAMPLE_DTYPE = np.dtype([("X", "<i4"), ("Y", "<i4"), ("line", "<i4"), ("offset", "<i4")])
TRANSECT_GEOM_DTYPE = np.dtype([("first", "<i4"), ("n", "<i4"), ("ex", "<f4"), ("ey", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("scale", "<f4"),
                                ("pad", "<i4"), ("len", "<f8"), ("ds", "<f8")])
# the int64 of a line in d_sums / the sums output of transects_push
TRANSECTS_SUMS = ("flux_pos", "flux_neg", "flux_along", "valid", "bad", "jets", "jet_start", "jet_len", "jet_sum", "jet_peak", "jet_peak_at",
                  "N", "num", "va", "vb", "q")
# the eight words of a kinematics summary, in order
KINEMATICS_SUMMARY = ("valid", "bad", "cores_cw", "cores_ccw", "t2_bits", "cells_both", "pushes", "max_omega_bits")
# rc_kinematics_cell as a numpy record (48 bytes): what Context.kinematics_read returns
KINEMATICS_CELL_DTYPE = np.dtype([("flags", "<i4"), ("n", "<i4"), ("bad", "<i4"), ("mean_vorticity", "<f4"), ("circulation", "<f4"),
                                  ("mean_divergence", "<f4"), ("enstrophy", "<f4"), ("mean_ow", "<f4"), ("cores_cw", "<i4"),
                                  ("cores_ccw", "<i4"), ("circulation_cw", "<f4"), ("circulation_ccw", "<f4")])
# the int64 of a cell in d_sums / the sums output of kinematics_push
KINEMATICS_SUMS = ("n_valid", "n_bad", "omega", "div", "e", "ow", "w2", "cores_cw", "cores_ccw", "omega_cw", "omega_ccw")
# the eight words of a shoreline summary, in order
SHORELINE_SUMMARY = ("thr", "N", "eta_q32", "positions", "dry", "wet", "outliers", "pushes")
# rc_shoreline as a numpy record (64 bytes): what Context.shoreline_read returns
SHORELINE_DTYPE = np.dtype([("flags", "<i4"), ("k", "<i4"), ("pos", "<i4"), ("agree", "<i4"), ("wx", "<i4"), ("wy", "<i4"), ("x", "<f4"),
                            ("y", "<f4"), ("dist_m", "<f4"), ("nv", "<i4"), ("pos_min", "<i4"), ("pos_max", "<i4"), ("pos_q", "<i4"),
                            ("pos_mean", "<f4"), ("excursion_m", "<f4"), ("pad", "<i4")])
# the eight words of a surf summary, in order
SURF_SUMMARY = ("n", "now", "surf", "sum_q", "bands", "channel_lines", "channels", "pushes")
# rc_surf_line (64 bytes) and rc_surf_channel (32 bytes) as numpy records: what Context.surf_read returns
SURF_LINE_DTYPE = np.dtype([("flags", "<i4"), ("k0", "<i4"), ("k1", "<i4"), ("load", "<i4"), ("peak", "<i4"), ("kpeak", "<i4"), ("ix", "<i4"),
                            ("iy", "<i4"), ("ox", "<i4"), ("oy", "<i4"), ("ref", "<i4"), ("share", "<i4"), ("width_m", "<f4"), ("pad", "<i4", (3,))])
SURF_CHANNEL_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("centre", "<i4"), ("share", "<i4"), ("cx", "<i4"), ("cy", "<i4"),
                               ("width_m", "<f4"), ("pad", "<i4")])
# rc_track as a numpy record (128 bytes): what Context.tracks_read returns
TRACK_DTYPE = np.dtype([("id", "<i8"), ("parent", "<i8"), ("first_push", "<i8"), ("area_sum", "<i8"), ("fx_sum", "<i8"), ("fy_sum", "<i8"),
                        ("m_sum", "<i8"), ("slot", "<i4"), ("label", "<i4"), ("flags", "<i4"), ("age", "<i4"), ("hits", "<i4"),
                        ("misses", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("px", "<i4"),
                        ("py", "<i4"), ("px0", "<i4"), ("py0", "<i4"), ("overlap", "<i4"), ("mean_fx", "<f4"), ("mean_fy", "<f4")])
# the eight words of a tracks summary, in order
TRACKS_SUMMARY = ("alive", "confirmed", "born", "ended", "seen", "coasting", "untracked", "pushes")
# rc_motion_cell as a numpy record (40 bytes): what Context.motion_read returns, per cell and for the frame
MOTION_CELL_DTYPE = np.dtype([("angle", "<f8"), ("S", "<i8"), ("W", "<i8"), ("tsmax", "<f4"), ("n_masked", "<i4"), ("n_used", "<i4"),
                              ("peak_bin", "<i4")])
# the name tables of _lib read the other way: the C ABI's number -> the name this layer takes and returns
FIT_MODEL_NAMES = {v: k for k, v in FIT_MODELS.items()}
FTLE_DIRECTION_NAMES = {v: k for k, v in FTLE_DIRECTIONS.items()}
# the eight words of a mean-flow summary and of a cell's sums, in order; rc_meanflow_cell (32 bytes) as a numpy record
MEANFLOW_SUMMARY = ("filled", "mask", "bad", "gx", "gy", "sum_m", "held", "pushes")
MEANFLOW_SUMS = ("filled", "n", "su", "sv", "sm", "mask", "bad", "zero")
MEANFLOW_CELL_DTYPE = np.dtype([("flags", "<i4"), ("filled", "<i4"), ("mask", "<i4"), ("bad", "<i4"), ("mean_x", "<f4"), ("mean_y", "<f4"),
                                ("steadiness", "<f4"), ("pad", "<i4")])
# the ten words of a flow-check summary and of a cell's sums, in order; the flags of a pixel by name; rc_flowcheck_cell (32 bytes)
FLOWCHECK_SUMMARY = ("valid", "bad", "out", "flat", "resid", "nogain", "fb", "fast", "computing", "pushes")
FLOWCHECK_SUMS = ("valid", "bad", "out", "flat", "resid", "nogain", "fb", "fast", "sum_qx", "sum_qy")
FLOWCHECK_FLAGS = {"bad": 1, "out": 2, "flat": 4, "resid": 8, "nogain": 16, "fb": 32, "fast": 64}
FLOWCHECK_CELL_DTYPE = np.dtype([("flags", "<i4"), ("pixels", "<i4"), ("valid", "<i4"), ("valid_pm", "<i4"), ("mean_x", "<f4"), ("mean_y", "<f4"),
                                 ("pad", "<i4", (2,))])
# the 24 words of a drifters summary and the eight of a cell in each table, in order; rc_drifters_cell (32 bytes) as a numpy record
DRIFTERS_SUMMARY = ("drifters", "alive", "released", "pushes", "age_shore", "age_offshore", "zero6", "zero7") + tuple("fate%d" % f for f in range(16))
DRIFTERS_PLACE = ("visits", "su", "sv", "shore", "offshore", "edge", "other", "age_offshore")
DRIFTERS_ORIGIN = ("released", "shore", "offshore", "edge", "other", "age_shore", "age_offshore", "zero")
DRIFTERS_CELL_DTYPE = np.dtype([("flags", "<i4"), ("pad0", "<i4"), ("mean_u", "<f4"), ("mean_v", "<f4"), ("escape", "<f4"), ("beached", "<f4"),
                                ("mean_exit_age", "<f4"), ("pad1", "<i4")])
# the 16 words of an infill summary and the eight of a cell's sums, in order; the source bytes by name; rc_infill_cell (32 bytes)
INFILL_SUMMARY = ("known", "held", "filled", "unfilled", "outside", "pushes", "zero6", "zero7") + tuple("lev%d" % k for k in range(8))
INFILL_SUMS = ("known", "held", "filled", "unfilled", "outside", "sum_fx", "sum_fy", "sum_lev")
INFILL_SOURCES = {"known": 0, "held": 64, "outside": 254, "unfilled": 255}
INFILL_CELL_DTYPE = np.dtype([("flags", "<i4"), ("pixels", "<i4"), ("known_pm", "<i4"), ("valued_pm", "<i4"), ("mean_x", "<f4"), ("mean_y", "<f4"),
                              ("mean_level", "<f4"), ("pad", "<i4")])
# the eight words of an offshore map summary and of a push summary, the four of a table cell, the classes by name; rc_offshore_station
# (48 bytes)
OFFSHORE_MAP_SUMMARY = ("wet", "dry", "wet_near_shore", "max_d2", "sum_d2_wet", "sum_d2_dry", "zero", "maps")
OFFSHORE_PUSH_SUMMARY = ("ok", "near", "far", "dry", "bad", "mask", "rips", "pushes")
OFFSHORE_SUMS = ("count", "sum_cross", "sum_along", "mask")
OFFSHORE_CLASSES = {"ok": 0, "near": 1, "far": 2, "dry": 3, "bad": 4}
OFFSHORE_STATION_DTYPE = np.dtype([("flags", "<i4"), ("first", "<i4"), ("reach_end", "<i4"), ("peak_bin", "<i4"), ("peak_cross", "<i4"),
                                   ("count", "<i4"), ("beyond", "<i4"), ("pad0", "<i4"), ("mean_cross", "<f4"), ("mean_along", "<f4"),
                                   ("pad1", "<i4", (2,))])
# the eight words of an outlines summary; rc_outline_loop (56 bytes) and its flags by name
OUTLINES_SUMMARY = ("cracks", "loops", "kept", "records", "vertices_kept", "vertices", "overflow", "pushes")
OUTLINE_FLAGS = {"hole": 1, "noverts": 2}
OUTLINE_LOOP_DTYPE = np.dtype([("label", "<i4"), ("flags", "<i4"), ("x", "<i4"), ("y", "<i4"), ("cracks", "<i4"), ("verts", "<i4"), ("offset", "<i4"),
                               ("pad", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area2", "<i8")])
RIPMAP_SOURCE_NAMES = {v: k for k, v in RIPMAP_SOURCES.items()}
TRACERS_MOVER_NAMES = {v: k for k, v in TRACERS_MOVERS.items()}
SHORE_SOURCE_NAMES = {v: k for k, v in SHORE_SOURCES.items()}


def _params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    return FarnebackParams(float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n),
                           float(poly_sigma), int(flags))


def _is_t(x):
    return isinstance(x, torch.Tensor)


def _fits(t, device, dtype, shape=None, numel=None, dense=False):
    """Whether `t` can go to a kernel as it is: a tensor on `device`, of `dtype`, of `shape` or of `numel` elements;
    contiguous, or with dense=True an image (h, w[, ch]) of dense pixels whose row step covers a row and may be padded."""
    if not (_is_t(t) and t.is_cuda and t.device == device and t.dtype == dtype):
        return False
    size, step = t.shape, t.stride()
    if shape is not None and size != tuple(shape):
        return False
    if numel is not None and t.numel() != numel:
        return False
    if not dense:
        return t.is_contiguous()
    inner = 1                                      # the step of the contiguous tensor at this depth, from the innermost out
    for k in range(len(size) - 1, 1, -1):
        if step[k] != inner:
            return False
        inner *= size[k]
    return step[1] == inner and step[0] >= inner * size[1]


def _check_out(t, device, dtype, what, shape=None, numel=None, dense=False):
    """A caller's output tensor, held to _fits (a view is taken as it is) -> the tensor."""
    if not _fits(t, device, dtype, shape, numel, dense):
        raise ValueError("%s must be a %s tensor on %s, %s, %s" % (
            what, str(dtype).replace("torch.", ""), device, "of shape %s" % (tuple(shape),) if shape is not None else "of %d" % numel,
            "with dense pixels" if dense else "contiguous"))
    return t


def _record(rec, skip=()):
    """A ctypes record as a dict, the fields of a nested `prm` beside the rest, without those named in `skip`."""
    d = {}
    for k, _ in rec._fields_:
        if k == "prm":
            d.update(_record(rec.prm, skip))
        elif k not in skip:
            d[k] = getattr(rec, k)
    return d


def _check_initial_flow(prev, flow):
    """OPTFLOW_USE_INITIAL_FLOW: `flow` is HxWx2 float32 with dense pixels, on the side (host / device) of the images."""
    if _is_t(prev):
        ok = _is_t(flow) and flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 3 and \
            flow.stride(2) == 1 and flow.stride(1) == 2
    else:
        ok = isinstance(flow, np.ndarray) and flow.dtype == np.float32 and flow.ndim == 3 and \
            flow.strides[2] == 4 and flow.strides[1] == 8
    if not ok or tuple(flow.shape) != (prev.shape[0], prev.shape[1], 2):
        raise RcflowError(-1, "OPTFLOW_USE_INITIAL_FLOW: `flow` must be HxWx2 float32 with dense pixels, where the images are")


class HistState:
    """Host copy of the caller-owned arrays of create_histogram (ripcurrents.cpp:147-154)."""

    def __init__(self):
        self.hist = np.zeros(HIST_BINS, np.int32)
        self.histsum = 0
        self.hist2d = np.zeros((HIST_DIRECTIONS, HIST_BINS), np.int32)
        self.histsum2d = np.zeros(HIST_DIRECTIONS, np.int32)
        self.UPPER = 100.0
        self.UPPER2d = np.zeros(HIST_DIRECTIONS, np.float32)
        self.prop_above_upper = np.zeros(HIST_DIRECTIONS, np.float32)


class Context:
    """One GPU context with `streams` independent stream slots (rcflow_create)."""

    def __init__(self, max_w, max_h, device=0, streams=1):
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("ripcurrents_amd needs a HIP device; there is no CPU fallback")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        check(self._lib.rcflow_create(C.byref(h), device, max_w, max_h, streams))
        self._h = h
        self.max_w, self.max_h = max_w, max_h
        self._own, self._bound = set(), {}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rcflow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ plumbing
    def sync(self, stream=0):
        check(self._lib.rcflow_sync(self._h, stream))

    def use_torch_stream(self, stream=0, torch_stream=None):
        """Run the slot on a torch stream (default: torch's current stream)."""
        ts = torch_stream if torch_stream is not None else torch.cuda.current_stream(self.device)
        self._own.discard(stream)
        self._bound[stream] = ts.cuda_stream
        check(self._lib.rcflow_set_hip_stream(self._h, stream, C.c_void_p(ts.cuda_stream)))

    def use_own_stream(self, stream=0):
        self._own.add(stream)
        check(self._lib.rcflow_use_own_stream(self._h, stream))

    def _bind(self, stream):
        """Device entry points run on torch's current stream (so tensor lifetimes and
        torch.cuda events order against them) unless use_own_stream() was asked for."""
        if stream not in self._own:
            ts = torch.cuda.current_stream(self.device).cuda_stream
            if self._bound.get(stream) != ts:
                check(self._lib.rcflow_set_hip_stream(self._h, stream, C.c_void_p(ts)))
                self._bound[stream] = ts

    def set_option(self, name, value):
        check(self._lib.rcflow_set_option(self._h, name.encode(), int(value)))

    def _dev(self, a, dtype):
        if _is_t(a):
            if not a.is_cuda or a.dtype != dtype:
                raise TypeError("expected a CUDA tensor of dtype %s" % dtype)
            return a
        return torch.as_tensor(np.ascontiguousarray(a)).to(self.device, dtype)

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr())

    # ------------------------------------------------------------------ A: Farneback
    def calcOpticalFlowFarneback(self, prev, next, flow=None, pyr_scale=0.5, levels=2, winsize=3,
                                 iterations=2, poly_n=15, poly_sigma=1.2, flags=0, stream=0):
        """cv::calcOpticalFlowFarneback(prev, next, flow, ...) -> flow (HxWx2 float32).

        numpy inputs use the host-pointer entry point (copy in, compute, copy out);
        CUDA tensors use the device entry point and return a CUDA tensor (asynchronous).
        With flags & 4 (OPTFLOW_USE_INITIAL_FLOW) `flow` is in/out: its content starts the coarsest scale
        (HxWx2 float32, a numpy array for numpy images, a CUDA tensor for tensors) and the result replaces it.
        """
        if int(flags) & RC_FARNEBACK_USE_INITIAL_FLOW:
            if flow is None:        # OpenCV asserts on an empty initial flow
                raise RcflowError(-1, "OPTFLOW_USE_INITIAL_FLOW needs the initial flow field in `flow`")
            _check_initial_flow(prev, flow)
        if _is_t(prev):
            if prev.shape != next.shape or prev.dim() != 2:
                raise ValueError("prev and next must be HxW and equal in size")
            h, w = prev.shape
            if flow is None:
                flow = torch.empty((h, w, 2), dtype=torch.float32, device=prev.device)
            p = _params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
            self._bind(stream)
            check(self._lib.rcflow_farneback_dev(
                self._h, stream, self._ptr(prev), prev.stride(0), self._ptr(next), next.stride(0), w, h,
                self._ptr(flow), flow.stride(0) * 4, C.byref(p)))
            return flow
        prev = np.asarray(prev)
        next = np.asarray(next)
        if prev.dtype != np.uint8 or next.dtype != np.uint8 or prev.ndim != 2 or prev.shape != next.shape:
            raise ValueError("prev and next must be HxW uint8 and equal in size")
        if prev.strides[1] != 1:
            prev = np.ascontiguousarray(prev)
        if next.strides[1] != 1:
            next = np.ascontiguousarray(next)
        h, w = prev.shape
        if flow is None:
            flow = np.empty((h, w, 2), np.float32)
        check(self._lib.rcflow_farneback_u8(
            self._h, stream, prev.ctypes.data, prev.strides[0], next.ctypes.data, next.strides[0], w, h,
            flow.ctypes.data, flow.strides[0], pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
            flags))
        return flow

    def push_frame(self, frame, flow=None, stream=0, **kw):
        """Streaming frame loop (ripcurrents.cpp:194-221): returns None for the first frame.
        With flags=4 `flow` is in/out: pass the same tensor every frame for the temporal warm start."""
        frame = self._dev(frame, torch.uint8)
        h, w = frame.shape
        p = _params(kw.get("pyr_scale", 0.5), kw.get("levels", 2), kw.get("winsize", 3),
                    kw.get("iterations", 2), kw.get("poly_n", 15), kw.get("poly_sigma", 1.2),
                    kw.get("flags", 0))
        if flow is None:
            flow = torch.empty((h, w, 2), dtype=torch.float32, device=frame.device)
        self._bind(stream)
        rc = check(self._lib.rcflow_push_frame_dev(self._h, stream, self._ptr(frame), frame.stride(0), w, h,
                                                   self._ptr(flow), flow.stride(0) * 4, C.byref(p)))
        return None if rc == 1 else flow

    def push_frame_host(self, frame, stream=0, **kw):
        """The frame loop with HOST frames (rcflow_push_frame_u8): numpy HxW uint8 in, page-locked
        double-buffered upload, the flow field stays on the device.  Returns None when the call primed
        the stream, else a CUDA tensor aliasing the slot's resident flow field (valid until the next push)."""
        frame = np.asarray(frame)
        if frame.dtype != np.uint8 or frame.ndim != 2 or frame.strides[1] != 1:
            frame = np.ascontiguousarray(frame, np.uint8)
        h, w = frame.shape
        p = _params(kw.get("pyr_scale", 0.5), kw.get("levels", 2), kw.get("winsize", 3),
                    kw.get("iterations", 2), kw.get("poly_n", 15), kw.get("poly_sigma", 1.2),
                    kw.get("flags", 0))
        self._bind(stream)
        rc = check(self._lib.rcflow_push_frame_u8(self._h, stream, frame.ctypes.data, frame.strides[0], w, h, C.byref(p)))
        if rc == 1:
            return None
        d = C.c_void_p()
        check(self._lib.rcflow_stream_flow_ptr(self._h, stream, C.byref(d), None, None))
        return _alias_tensor(d.value, h * w * 2, torch.float32, self.device).view(h, w, 2)

    def frame_buffer(self, w, h, stream=0):
        """The next page-locked staging buffer of the slot as a numpy HxW uint8 view (rcflow_frame_buffer_acquire): produce
        the frame into it, then push_frame_acquired() -- the frame loop without the staging copy.  The view is valid until
        that push; a later acquire with a LARGER frame reallocates the slot's staging memory, so never keep a view across
        a size change (take a new one per frame, as the loop does anyway)."""
        ptr, step = C.c_void_p(), C.c_size_t()
        check(self._lib.rcflow_frame_buffer_acquire(self._h, stream, w, h, C.byref(ptr), C.byref(step)))
        buf = (C.c_uint8 * (h * step.value)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.uint8).reshape(h, step.value)[:, :w]

    def push_frame_acquired(self, w, h, stream=0, **kw):
        p = _params(kw.get("pyr_scale", 0.5), kw.get("levels", 2), kw.get("winsize", 3),
                    kw.get("iterations", 2), kw.get("poly_n", 15), kw.get("poly_sigma", 1.2),
                    kw.get("flags", 0))
        self._bind(stream)
        rc = check(self._lib.rcflow_push_frame_acquired(self._h, stream, C.byref(p)))
        if rc == 1:
            return None
        d = C.c_void_p()
        check(self._lib.rcflow_stream_flow_ptr(self._h, stream, C.byref(d), None, None))
        return _alias_tensor(d.value, h * w * 2, torch.float32, self.device).view(h, w, 2)

    def frame_loop_step(self, w, h, seeds=None, outmask=None, edges=None, dt=2.0, iterations=1, seed_dt=2.0,
                        seed_iterations=1, seed_upper=100.0, seed_variant=3, MID=0.5, LOWER=0.2, use_graph=False,
                        stream=0, **kw):
        """One iteration of the reference's frame loop (ripcurrents.cpp:194-479) on the frame produced into frame_buffer():
        flow against the previous frame, streamline_field, seed streamlines, histogram + thresholds, classify / accumulate
        (framecount counted on the device), mask edges -- rcflow_frame_loop_step.  Returns the resident flow field, or
        None for the call that primes the stream."""
        from ._lib import FrameLoop
        p = _params(kw.get("pyr_scale", 0.5), kw.get("levels", 2), kw.get("winsize", 3), kw.get("iterations_flow", 2),
                    kw.get("poly_n", 15), kw.get("poly_sigma", 1.2), kw.get("flags", 0))
        L = FrameLoop()
        L.dt, L.iterations = dt, iterations
        if seeds is not None:
            L.d_seeds, L.nseeds = self._ptr(seeds), seeds.shape[0]
        L.seed_variant, L.seed_dt, L.seed_iterations, L.seed_upper = seed_variant, seed_dt, seed_iterations, seed_upper
        L.MID, L.LOWER = MID, LOWER
        if outmask is not None:
            L.d_outmask, L.mask_step = self._ptr(outmask), outmask.stride(0)
        if edges is not None:
            L.d_edges, L.edges_step = self._ptr(edges), edges.stride(0)
        L.use_graph = 1 if use_graph else 0
        self._bind(stream)
        rc = check(self._lib.rcflow_frame_loop_step(self._h, stream, C.byref(p), C.byref(L)))
        if rc == 1:
            return None
        d = C.c_void_p()
        check(self._lib.rcflow_stream_flow_ptr(self._h, stream, C.byref(d), None, None))
        return _alias_tensor(d.value, h * w * 2, torch.float32, self.device).view(h, w, 2)

    def stream_flow_read(self, w, h, stream=0):
        out = np.empty((h, w, 2), np.float32)
        self._bind(stream)
        check(self._lib.rcflow_stream_flow_read(self._h, stream, out.ctypes.data, out.strides[0]))
        return out

    def push_clip(self, frames, flows=None, stream=0, **kw):
        """The next [T,H,W] frames of the slot's stream in one call (rcflow_push_clip_dev): every frame is
        expanded once however the segment is cut into calls.  Returns the flow fields written ([T,H,W,2] when
        the stream was primed -- flow 0 runs from the previous call's last frame to frames[0] -- else [T-1,...])."""
        frames = self._dev(frames, torch.uint8)
        T, h, w = frames.shape
        p = _params(kw.get("pyr_scale", 0.5), kw.get("levels", 2), kw.get("winsize", 3),
                    kw.get("iterations", 2), kw.get("poly_n", 15), kw.get("poly_sigma", 1.2),
                    kw.get("flags", 0))
        if flows is None:
            flows = torch.empty((T, h, w, 2), dtype=torch.float32, device=frames.device)
        self._bind(stream)
        n = check(self._lib.rcflow_push_clip_dev(
            self._h, stream, self._ptr(frames), frames.stride(0), frames.stride(1), T, w, h,
            self._ptr(flows), flows.stride(0) * 4, flows.stride(1) * 4, C.byref(p)))
        return flows[:n]

    def stream_reset(self, stream=0):
        check(self._lib.rcflow_stream_reset(self._h, stream))

    def farneback_clip(self, frames, flows=None, stream=0, pyr_scale=0.5, levels=2, winsize=3, iterations=2,
                       poly_n=15, poly_sigma=1.2, flags=0):
        """[T,H,W] uint8 CUDA clip -> [T-1,H,W,2] flows (pair t = frames t, t+1)."""
        frames = self._dev(frames, torch.uint8)
        T, h, w = frames.shape
        if flows is None:
            flows = torch.empty((T - 1, h, w, 2), dtype=torch.float32, device=frames.device)
        p = _params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
        self._bind(stream)
        check(self._lib.rcflow_farneback_clip_dev(
            self._h, stream, self._ptr(frames), frames.stride(0), frames.stride(1), T, w, h,
            self._ptr(flows), flows.stride(0) * 4, flows.stride(1) * 4, C.byref(p)))
        return flows

    def push_batch(self, frames, flows=None, use_graph=True, stream=0, **kw):
        """Lockstep batch of streams: frames [S,H,W] uint8 -> flows [S,H,W,2] (None on the priming call)."""
        frames = self._dev(frames, torch.uint8)
        S, h, w = frames.shape
        p = _params(kw.get("pyr_scale", 0.5), kw.get("levels", 2), kw.get("winsize", 3), kw.get("iterations", 2),
                    kw.get("poly_n", 15), kw.get("poly_sigma", 1.2), kw.get("flags", 0))
        if flows is None:
            flows = torch.empty((S, h, w, 2), dtype=torch.float32, device=frames.device)
        self._bind(stream)
        rc = check(self._lib.rcflow_push_batch_dev(self._h, stream, self._ptr(frames), frames.stride(0), frames.stride(1),
                                                   S, w, h, self._ptr(flows), flows.stride(0) * 4, flows.stride(1) * 4,
                                                   C.byref(p), 1 if use_graph else 0))
        return None if rc == 1 else flows

    def batch_reset(self, stream=0):
        check(self._lib.rcflow_batch_reset(self._h, stream))

    def level_geometry(self, w, h, pyr_scale, levels, k):
        wk, hk = C.c_int(), C.c_int()
        L = check(self._lib.rcflow_level_geometry(w, h, pyr_scale, levels, k, C.byref(wk), C.byref(hk)))
        return L, wk.value, hk.value

    # stage-level entry points (parity tests)
    def stage_pyr_level(self, img, pyr_scale, k, stream=0):
        img = self._dev(img, torch.uint8)
        h, w = img.shape
        _, wk, hk = self.level_geometry(w, h, pyr_scale, 64, k)
        out = torch.empty((hk, wk), dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_stage_pyr_level_dev(self._h, stream, self._ptr(img), img.stride(0), w, h,
                                                   pyr_scale, k, self._ptr(out)))
        return out

    def stage_polyexp(self, I, poly_n=15, poly_sigma=1.2, stream=0):
        I = self._dev(I, torch.float32).contiguous()
        h, w = I.shape
        R = torch.empty((h, w, 5), dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_stage_polyexp_dev(self._h, stream, self._ptr(I), w, h, poly_n, poly_sigma,
                                                 self._ptr(R)))
        return R

    def debug_level_R(self, w, h, pyr_scale, level, slot, stream=0):
        """Diagnostic (rcflow_debug_level_R): upstream's R (h_k x w_k x 5) that the slot's last Farneback call, on w x h
        frames at `pyr_scale`, left in ring entry `slot` of scale `level`."""
        return self._debug_level(self._lib.rcflow_debug_level_R, w, h, pyr_scale, level, slot, stream, (5,))

    def debug_level_image(self, w, h, pyr_scale, level, slot, stream=0):
        """Diagnostic (rcflow_debug_level_image): the pyramid image (h_k x w_k) of ring entry `slot` of scale `level` >= 1."""
        return self._debug_level(self._lib.rcflow_debug_level_image, w, h, pyr_scale, level, slot, stream, ())

    def debug_level_flow(self, w, h, pyr_scale, level, which, pair=0, stream=0):
        """Diagnostic (rcflow_debug_level_flow): buffer A (which = 0) or B (1) of scale `level`, pair `pair` of the slot's last
        Farneback call, as h_k x w_k x 2 -- the flow field one of the scale's launches wrote (see rcflow_api.hip)."""
        fn = self._lib.rcflow_debug_level_flow
        return self._debug_level(lambda hdl, st, lv, sl, out, gw, gh: fn(hdl, st, lv, which, sl, out, gw, gh), w, h, pyr_scale, level, pair,
                                 stream, (2,))

    @staticmethod
    def debug_flow_form(w, h, pairs, winsize, flags=0, solve=1, in_mode=1, fuse=1, chain=1, chain_min_blocks=0, ablate=0):
        """Diagnostic (rcflow_debug_flow_form; host logic, no context, no GPU): the kernel and tile a flow-iteration launch
        takes, as a dict (kernel: one of _lib.FLOW_KERNELS' names)."""
        fn = _lib.load().rcflow_debug_flow_form
        buf = (C.c_int * 16)()
        n = check(fn(w, h, pairs, winsize, flags, solve, in_mode, fuse, chain, chain_min_blocks, ablate, buf, 16))
        names = ("kernel", "tw", "th", "nt", "nit", "d", "groups", "tiles_x", "tiles_y", "grid_y", "interior")
        assert n == len(names)
        f = dict(zip(names, buf[:n]))
        f["kernel"] = _lib.FLOW_KERNELS[f["kernel"]]
        return f

    def _debug_level(self, fn, w, h, pyr_scale, level, slot, stream, tail):
        _, wk, hk = self.level_geometry(w, h, pyr_scale, 64, max(level, 0))
        # the plan's own size of the scale, asked before anything is written (rcflow_debug_level_flow_ptr reports it whether
        # or not the scale has a flow field yet)
        gw, gh, p = C.c_int(), C.c_int(), C.c_void_p()
        rc = self._lib.rcflow_debug_level_flow_ptr(self._h, C.c_int(stream), C.c_int(level), C.c_int(0), C.byref(p), C.byref(gw), C.byref(gh))
        if rc in (0, -6) and (gw.value, gh.value) != (wk, hk):
            raise RcflowError(-1, "the slot's plan has %d x %d at scale %d, not %d x %d" % (gw.value, gh.value, level, wk, hk))
        out = torch.empty((hk, wk) + tail, dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(fn(self._h, stream, level, slot, self._ptr(out), None, None))
        return out

    def stage_initial_flow(self, flow, pyr_scale, levels, stream=0):
        """The reduction OPTFLOW_USE_INITIAL_FLOW applies to the initial field (rcflow_stage_initial_flow_dev):
        HxWx2 float32 (any row stride) -> the coarsest scale's h_k x w_k x 2, times pyr_scale^k."""
        flow = self._dev(flow, torch.float32)
        if flow.dim() != 3 or flow.shape[2] != 2 or flow.stride(2) != 1 or flow.stride(1) != 2:
            flow = flow.contiguous()
        h, w = flow.shape[:2]
        L, _, _ = self.level_geometry(w, h, pyr_scale, levels, 0)
        _, wk, hk = self.level_geometry(w, h, pyr_scale, levels, L)
        out = torch.empty((hk, wk, 2), dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_stage_initial_flow_dev(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h,
                                                      pyr_scale, levels, self._ptr(out)))
        return out

    def stage_flow_iter(self, R0, R1, flow_in, winsize, flags, stream=0):
        R0 = self._dev(R0, torch.float32).contiguous()
        R1 = self._dev(R1, torch.float32).contiguous()
        h, w = R0.shape[:2]
        fin = None if flow_in is None else self._dev(flow_in, torch.float32).contiguous()
        out = torch.empty((h, w, 2), dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_stage_flow_iter_dev(self._h, stream, self._ptr(R0), self._ptr(R1),
                                                   None if fin is None else self._ptr(fin), w, h, winsize,
                                                   flags, self._ptr(out)))
        return out

    # ------------------------------------------------------------------ B: analysis
    def analysis_reset(self, w, h, stream=0):
        self._bind(stream)
        check(self._lib.rcflow_analysis_reset(self._h, stream, w, h))

    def _flow(self, flow):
        flow = self._dev(flow, torch.float32)
        if flow.dim() != 3 or flow.shape[2] != 2 or flow.stride(2) != 1 or flow.stride(1) != 2:
            flow = flow.contiguous()
        return flow

    def create_histogram(self, current, st=None, stream=0):
        """create_histogram(current, hist, histsum, hist2d, histsum2d, UPPER, UPPER2d, prop_above_upper).

        `current` is the flow field (HxWx2); the polar conversion the reference does first
        (ripcurrents.cpp:305-309) is fused into the kernel.  The cumulative counters live in the
        slot; `st` (HistState) receives a host copy, like the reference's in/out arrays.
        """
        flow = self._flow(current)
        h, w = flow.shape[:2]
        self._bind(stream)
        check(self._lib.rcflow_histogram_dev(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h))
        self._bind(stream)
        check(self._lib.rcflow_thresholds_dev(self._h, stream))
        if st is not None:
            self.histogram_read(st, stream)
        return st

    def histogram_accumulate(self, current, stream=0):
        flow = self._flow(current)
        h, w = flow.shape[:2]
        self._bind(stream)
        check(self._lib.rcflow_histogram_dev(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h))

    def histogram_accumulate_clip(self, flows, stream=0):
        """Counts of a whole segment's flow fields ([T,H,W,2]) in one launch."""
        T, h, w = flows.shape[:3]
        self._bind(stream)
        check(self._lib.rcflow_histogram_clip_dev(self._h, stream, self._ptr(flows), flows.stride(0) * 4,
                                                  flows.stride(1) * 4, T, w, h))

    def thresholds(self, stream=0):
        self._bind(stream)
        check(self._lib.rcflow_thresholds_dev(self._h, stream))

    def thresholds_from_words(self, words, stream=0):
        """UPPER / UPPER2d / prop_above_upper from a device block of histogram words (e.g. the
        all-reduced global histogram); the slot's own counters stay as they are."""
        wds = self._dev(words, torch.int32).contiguous()
        if wds.numel() != HIST_WORDS:
            raise ValueError("expected %d histogram words" % HIST_WORDS)
        self._bind(stream)
        check(self._lib.rcflow_thresholds_words_dev(self._h, stream, self._ptr(wds)))

    def histogram_read(self, st=None, stream=0):
        st = st or HistState()
        hs, up = C.c_int32(), C.c_float()
        self._bind(stream)
        check(self._lib.rcflow_histogram_read(
            self._h, stream, st.hist.ctypes.data, st.hist2d.ctypes.data, C.addressof(hs),
            st.histsum2d.ctypes.data, C.addressof(up), st.UPPER2d.ctypes.data,
            st.prop_above_upper.ctypes.data))
        st.histsum, st.UPPER = hs.value, up.value
        return st

    def histogram_words(self, stream=0):
        """The RC_HIST_WORDS int32 block as a CUDA tensor aliasing the slot's counters
        (what torch.distributed.all_reduce sums across ranks)."""
        p = C.c_void_p()
        self._bind(stream)
        check(self._lib.rcflow_histogram_device_ptr(self._h, stream, C.byref(p)))
        return _alias_tensor(p.value, HIST_WORDS, torch.int32, self.device)

    def histogram_write(self, words, stream=0):
        words = np.ascontiguousarray(words, np.int32)
        assert words.size == HIST_WORDS
        self._bind(stream)
        check(self._lib.rcflow_histogram_write(self._h, stream, words.ctypes.data))

    def histogram_reset(self, stream=0):
        """Starts a new segment: zeroes the cumulative counters (asynchronous, on the slot's stream)."""
        self._bind(stream)
        check(self._lib.rcflow_histogram_reset_dev(self._h, stream))

    # ------------------------------------------------------------------ multi-GPU: global histogram (C ABI over RCCL)
    def comm_unique_id(self):
        """rank 0: the RCCL unique id (bytes) the host distributes to the other ranks."""
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        check(self._lib.rcflow_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, world, unique_id=None):
        check(self._lib.rcflow_comm_init(self._h, unique_id, rank, world))

    def comm_destroy(self):
        check(self._lib.rcflow_comm_destroy(self._h))

    def allreduce_hist(self, stream=0, out=None):
        """Starts the all-rank sum of the slot's histogram counters (asynchronous, on the collective's own
        stream); returns the device tensor that will hold the result once allreduce_hist_join() has ordered
        the slot's stream after it."""
        self._bind(stream)
        if out is None:
            check(self._lib.rcflow_allreduce_hist(self._h, stream, None))
            p = C.c_void_p()
            check(self._lib.rcflow_allreduce_hist_result(self._h, C.byref(p)))
            return _alias_tensor(p.value, HIST_WORDS, torch.int32, self.device)
        check(self._lib.rcflow_allreduce_hist(self._h, stream, self._ptr(out)))
        return out

    def allreduce_hist_join(self, stream=0):
        self._bind(stream)
        check(self._lib.rcflow_allreduce_hist_join(self._h, stream))

    def allreduce_hist_status(self):
        """Host wait for the collective started last, then the verdict every rank shares (rcflow_allreduce_hist_status):
        raises RcflowError(RC_ESTATE) when the ranks together counted more pixels than an int32 histsum holds; returns the
        upper bound of the pixels counted otherwise."""
        n = C.c_longlong(0)
        check(self._lib.rcflow_allreduce_hist_status(self._h, C.byref(n)))
        return n.value

    def create_flow_accumulate(self, current, framecount, MID=0.5, LOWER=0.2, want=("polar", "waterclass",
                               "out", "outmask"), stream=0):
        """create_flow + create_accumulationbuffer (ripcurrents_module.cpp:153-212) in one pass.
        Returns a dict of the requested device outputs."""
        flow = self._flow(current)
        h, w = flow.shape[:2]
        outs = {}
        def mk(name, shape, dt):
            if name in want:
                outs[name] = torch.empty(shape, dtype=dt, device=self.device)
                return self._ptr(outs[name]), outs[name].stride(0) * outs[name].element_size()
            return None, 0
        pp, ps = mk("polar", (h, w, 3), torch.float32)
        wp, ws = mk("waterclass", (h, w, 3), torch.float32)
        op, os_ = mk("out", (h, w, 3), torch.float32)
        mp, ms = mk("outmask", (h, w), torch.uint8)
        self._bind(stream)
        check(self._lib.rcflow_classify_accumulate_dev(
            self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h, framecount, MID, LOWER, pp, ps, wp, ws,
            op, os_, mp, ms))
        return outs

    def accumulator(self, w, h, stream=0):
        acc = np.empty((h, w), np.float32)
        self._bind(stream)
        check(self._lib.rcflow_accumulator_read(self._h, stream, acc.ctypes.data))
        return acc

    def streamline_field(self, flow, dt, iterations, UPPER=-1.0, stream=0):
        """streamlines_mat.forEach(streamline_field(...)) ripcurrents.cpp:229-231; state in the slot."""
        flow = self._flow(flow)
        h, w = flow.shape[:2]
        self._bind(stream)
        check(self._lib.rcflow_advect_field_dev(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h, dt,
                                                iterations, UPPER))

    def streamline_field_state(self, w, h, stream=0):
        pt = np.empty((h, w, 2), np.float32)
        dist = np.empty((h, w), np.float32)
        self._bind(stream)
        check(self._lib.rcflow_advect_field_read(self._h, stream, pt.ctypes.data, dist.ctypes.data))
        return pt, dist

    def streamline(self, pts, flow, dt, iterations, UPPER, variant=0, trace=False, stream=0):
        """Seed loops over streamline()/streamline_2()/streamline_3() (variant 0/1/2),
        ripcurrents.cpp's copy (3) and pathlines.cpp (4).  pts: n x 2, returns (pts, trace)."""
        flow = self._flow(flow)
        h, w = flow.shape[:2]
        d_pts = self._dev(np.ascontiguousarray(pts, np.float32) if not _is_t(pts) else pts, torch.float32).contiguous()
        n = d_pts.shape[0]
        iters = 100 if variant == 2 else iterations
        tr = torch.zeros((n, iters, 2), dtype=torch.float32, device=self.device) if trace else None
        self._bind(stream)
        check(self._lib.rcflow_advect_points_dev(
            self._h, stream, self._ptr(d_pts), n, self._ptr(flow), flow.stride(0) * 4, w, h, dt, iterations,
            UPPER, variant, None if tr is None else self._ptr(tr)))
        return d_pts, tr

    def get_delta_field(self, pt, flow, dt, UPPER, stream=0):
        flow = self._flow(flow)
        h, w = flow.shape[:2]
        pt = self._dev(pt, torch.float32).contiguous()
        self._bind(stream)
        check(self._lib.rcflow_get_delta_field_dev(self._h, stream, self._ptr(pt), pt.stride(0) * 4,
                                                   self._ptr(flow), flow.stride(0) * 4, w, h, dt, UPPER))
        return pt

    def _postop(self, fn, current, stream):
        flow = self._flow(current)
        h, w = flow.shape[:2]
        self._bind(stream)
        check(fn(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h))
        return flow

    def subtructAverage(self, current, stream=0):
        return self._postop(self._lib.rcflow_subtract_average_dev, current, stream)

    def subtructMeanMagnitude(self, current, stream=0):
        return self._postop(self._lib.rcflow_subtract_mean_magnitude_dev, current, stream)

    def stabilizer(self, current, stream=0):
        return self._postop(self._lib.rcflow_stabilizer_dev, current, stream)

    def window_mean(self, avg, slot, cur, window, stream=0):
        self._bind(stream)
        check(self._lib.rcflow_window_mean_dev(self._h, stream, self._ptr(avg), self._ptr(slot), self._ptr(cur),
                                               avg.numel(), window))

    def vectorToColor(self, current, max_displacement, stream=0):
        flow = self._flow(current)
        h, w = flow.shape[:2]
        hsv = torch.zeros((h, w, 3), dtype=torch.uint8, device=self.device)
        md = C.c_float(max_displacement)
        self._bind(stream)
        check(self._lib.rcflow_vector_to_color_dev(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h,
                                                   self._ptr(hsv), hsv.stride(0), C.byref(md)))
        return hsv, md.value

    def shearRateToColor(self, current, max_frobenius, hsv=None, stream=0):
        flow = self._flow(current)
        h, w = flow.shape[:2]
        if hsv is None:
            hsv = torch.zeros((h, w, 3), dtype=torch.uint8, device=self.device)
        mf = C.c_float(max_frobenius)
        self._bind(stream)
        check(self._lib.rcflow_shear_rate_to_color_dev(self._h, stream, self._ptr(flow), flow.stride(0) * 4, w, h,
                                                       self._ptr(hsv), hsv.stride(0), C.byref(mf)))
        return hsv, mf.value

    # ------------------------------------------------------------------ SURVEY 8(f) next rows
    def create_edges(self, outmask, stream=0):
        """create_edges(outmask) ripcurrents_module.cpp:216-220: returns the edge mask."""
        m = self._dev(outmask, torch.uint8)
        if m.stride(1) != 1:
            m = m.contiguous()
        h, w = m.shape
        out = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_create_edges_dev(self._h, stream, self._ptr(m), m.stride(0), w, h, self._ptr(out),
                                                out.stride(0)))
        return out

    def create_output(self, subframe, outmask, stream=0):
        """create_output(subframe, outmask) ripcurrents_module.cpp:225-244: paints the edge mask into the
        red channel of the 8UC3 frame, in place when `subframe` is already a device tensor; returns it."""
        f = self._dev(subframe, torch.uint8).contiguous()
        m = self._dev(outmask, torch.uint8).contiguous()
        h, w = m.shape
        if tuple(f.shape) != (h, w, 3):
            raise ValueError("subframe must be HxWx3 uint8 of the mask's size")
        self._bind(stream)
        check(self._lib.rcflow_create_output_dev(self._h, stream, self._ptr(f), f.stride(0), self._ptr(m), m.stride(0), w, h))
        return f

    def resize_bgr_to_gray(self, frame, dw, dh, stream=0, interpolation="linear"):
        """resize(frame, Size(dw,dh), INTER_LINEAR) + cvtColor(BGR2GRAY) (ripcurrents.cpp:209-210);
        interpolation="area": INTER_AREA, as the reference resizes the first frame (ripcurrents.cpp:186)."""
        f = self._dev(frame, torch.uint8).contiguous()
        sh, sw = f.shape[:2]
        out = torch.empty((dh, dw), dtype=torch.uint8, device=self.device)
        self._bind(stream)
        fn = self._lib.rcflow_resize_area_bgr_to_gray_dev if interpolation == "area" else self._lib.rcflow_resize_bgr_to_gray_dev
        check(fn(self._h, stream, self._ptr(f), f.stride(0), sw, sh, self._ptr(out), out.stride(0), dw, dh))
        return out

    def resize_bgr(self, frame, dw, dh, stream=0, interpolation="linear"):
        """resize(frame, Size(dw,dh), 0, 0, INTER_LINEAR) on an 8UC3 frame (main.cpp:1227, :1302) -> (dh, dw, 3) uint8;
        interpolation="area": INTER_AREA, as compute_phaseCorrelate resizes every frame (main.cpp:1707, :1723)."""
        if interpolation not in ("linear", "area"):
            raise ValueError("interpolation must be \"linear\" or \"area\"")
        f = self._img3(frame)
        sh, sw = f.shape[:2]
        out = torch.empty((dh, dw, 3), dtype=torch.uint8, device=self.device)
        self._bind(stream)
        fn = self._lib.rcflow_resize_area_bgr_dev if interpolation == "area" else self._lib.rcflow_resize_bgr_dev
        check(fn(self._h, stream, self._ptr(f), f.stride(0), sw, sh, self._ptr(out), out.stride(0), dw, dh))
        return out

    # ------------------------------------------------------------------ the per-slot products: what they share
    def _in_image(self, t, dtype, name, shape, optional=False):
        """An input image -> (pointer, byte step); with optional=True (NULL, 0) for None.  The one rule for it: a tensor on the
        context's device, of `dtype` and of `shape` = (h, w[, ch]), with dense pixels and a row step of at least a row (rows
        may be padded; a view is taken as it is).  The methods that also take numpy convert first (_dev, _img3)."""
        if t is None and optional:
            return C.c_void_p(None), 0
        if not _fits(t, self.device, dtype, shape=shape, dense=True):
            raise ValueError("%s must be a %s %s tensor on %s with dense pixels, as opened" % (
                name, "x".join(str(n) for n in shape), str(dtype).replace("torch.", ""), self.device))
        return self._ptr(t), t.stride(0) * t.element_size()

    def _out_image(self, t, dtype, name, shape):
        """An optional output image of dense pixels -> (pointer, byte step); (NULL, 0) for None."""
        if t is None:
            return C.c_void_p(None), 0
        _check_out(t, self.device, dtype, name, shape=shape, dense=True)
        return self._ptr(t), t.stride(0) * t.element_size()

    def _out_array(self, t, dtype, name, numel):
        """An optional contiguous output of `numel` elements -> its pointer; NULL for None."""
        return C.c_void_p(None) if t is None else self._ptr(_check_out(t, self.device, dtype, name, numel=numel))

    def _out_or_new(self, out, dtype, name, shape, dense=False, any_shape=False):
        """The caller's output, checked, or a new tensor of `shape`.  The caller's is contiguous, or with dense=True an image
        whose rows may be padded; with any_shape=True only its element count is held to `shape`."""
        if out is None:
            return torch.empty(tuple(shape), dtype=dtype, device=self.device)
        if any_shape:
            return _check_out(out, self.device, dtype, name, numel=int(np.prod(shape)))
        return _check_out(out, self.device, dtype, name, shape=shape, dense=dense)

    def _prims_out(self, out, n):
        """The output of a *_prims method: n rc_draw_prim records."""
        return self._out_or_new(out, torch.uint8, "out", (n, 32), any_shape=True)

    def _summary(self, fn, stream, names, *args, bits=None):
        """Calls a *_read entry point, whose last argument is the slot's summary of 8 int64, on the slot's stream -> the
        summary as a dict by `names`.  bits = (key, new_name, transform): the word `key` holds the bits of a float32, and
        transform of that float is added as new_name."""
        summ = np.zeros(8, np.int64)
        self._bind(stream)
        check(fn(self._h, stream, *args, summ.ctypes.data_as(C.POINTER(C.c_longlong))))
        out = dict(zip(names, (int(v) for v in summ)))
        if bits is not None:
            key, new_name, transform = bits
            out[new_name] = float(transform(np.array([out[key]], np.uint32).view(np.float32)[0]))
        return out

    def _info(self, product, rec, stream):
        """rcflow_<product>_info into the ctypes record `rec` -> rec; never blocks.  A push reads the geometry it holds its
        arguments to from the record; <product>_info returns it as a dict."""
        check(getattr(self._lib, "rcflow_%s_info" % product)(self._h, stream, C.byref(rec)))
        return rec

    def _lifecycle(self, product, verb, stream):
        """rcflow_<product>_reset / _close.  Both bind the slot to the stream the pushes ran on first: the reset is queued
        behind them, and the close waits for the pushes queued on that stream before it frees the state."""
        self._bind(stream)
        check(getattr(self._lib, "rcflow_%s_%s" % (product, verb))(self._h, stream))

    # ------------------------------------------------------------------ time-exposure images
    def _img3(self, a):
        """An (h, w, 3) uint8 device image with dense pixels; rows may have any step (views are taken as they are)."""
        t = self._dev(a, torch.uint8)
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("expected an HxWx3 uint8 image")
        if t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * t.shape[1]:
            t = t.contiguous()
        return t

    def _cvt_u8(self, fn, img, out, stream):
        a = self._img3(img)
        h, w = a.shape[:2]
        out = self._out_or_new(out, torch.uint8, "out", a.shape, dense=True)
        self._bind(stream)
        check(fn(self._h, stream, self._ptr(a), a.stride(0), w, h, self._ptr(out), out.stride(0)))
        return out

    def rgb_to_hsv_u8(self, img, out=None, stream=0):
        """cvtColor(img, COLOR_RGB2HSV) on 8UC3 (main.cpp:1308): byte 0 of `img` plays R; H in 0..179.
        `out` (optional): the image to write, `img` itself for in place."""
        return self._cvt_u8(self._lib.rcflow_rgb_to_hsv_u8_dev, img, out, stream)

    def hsv_to_rgb_u8(self, img, out=None, stream=0):
        """cvtColor(img, COLOR_HSV2RGB) on 8UC3 (main.cpp:1361)."""
        return self._cvt_u8(self._lib.rcflow_hsv_to_rgb_u8_dev, img, out, stream)

    def timex_open(self, w, h, window=50, products=("mean",), stream=0):
        """Opens the slot's time-exposure state: products out of "mean" (compute_timex, main.cpp:1195-1263), "average",
        "bright", "dark" (compute_brightColor options 0, 1, 2, main.cpp:1265-1383, over a ring of `window` frames)."""
        mask = 0
        for name in products:
            if name not in TIMEX_PRODUCTS:
                raise ValueError("unknown time-exposure product %r" % (name,))
            mask |= TIMEX_PRODUCTS[name]
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_timex_open(self._h, stream, int(w), int(h), int(window), mask))

    def timex_info(self, stream=0):
        """dict(w, h, window, products (names, in output order), frames_pushed, device_bytes) of the open state."""
        w, h, win, prod = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        frames, nbytes = C.c_longlong(0), C.c_size_t(0)
        check(self._lib.rcflow_timex_info(self._h, stream, C.byref(w), C.byref(h), C.byref(win), C.byref(prod),
                                          C.byref(frames), C.byref(nbytes)))
        return dict(w=w.value, h=h.value, window=win.value,
                    products=tuple(n for n, bit in TIMEX_PRODUCTS.items() if prod.value & bit),
                    frames_pushed=frames.value, device_bytes=nbytes.value)

    def timex_push(self, frame, out=None, stream=0):
        """One frame (HxWx3 uint8) into the slot's time-exposure state -> {product name: (h, w, 3) uint8 device image}
        for every open product, as the reference shows after this frame.  `out` (optional) maps product names to
        preallocated images to write into, or to None to update that product's state without producing its image."""
        info = self.timex_info(stream)
        shape = (info["h"], info["w"], 3)
        f = self._img3(frame)       # held to the end of the call: it may be a copy made here
        fp, fstep = self._in_image(f, torch.uint8, "frame", shape)
        out = dict(out or {})
        res = {}
        ptrs, steps = (C.c_void_p * 4)(), (C.c_size_t * 4)()
        for k, name in enumerate(TIMEX_PRODUCTS):
            if out[name] is None if name in out else name not in info["products"]:
                continue            # asked not to produce it, or not open and not asked for
            res[name] = t = self._out_or_new(out.get(name), torch.uint8, "out[%r]" % name, shape, dense=True)
            ptrs[k], steps[k] = t.data_ptr(), t.stride(0)
        self._bind(stream)
        check(self._lib.rcflow_timex_push_dev(self._h, stream, fp, fstep, ptrs, steps))
        return res

    def timex_reset(self, stream=0):
        self._lifecycle("timex", "reset", stream)

    def timex_close(self, stream=0):
        self._lifecycle("timex", "close", stream)

    # ------------------------------------------------------------------ frame stabilisation
    def phase_correlate(self, a, b, window=True, out=None, stream=0):
        """cv::phaseCorrelate(a, b, hann) of two float32 patches (main.cpp:1745; `window=False`: without the Hann
        window) -> device tensor of 3 float64: shift_x, shift_y, response.  b(x) = a(x - d) gives shift +d.
        `out` (optional): a float64 device tensor of 3 to write.  Asynchronous: read the result after a sync."""
        ta, tb = self._dev(a, torch.float32), self._dev(b, torch.float32)
        if ta.dim() != 2 or ta.shape != tb.shape:
            raise ValueError("expected two 2-D float32 patches of one size")
        ta = ta if ta.stride(1) == 1 else ta.contiguous()
        tb = tb if tb.stride(1) == 1 else tb.contiguous()
        h, w = ta.shape
        out = self._out_or_new(out, torch.float64, "out", (3,), any_shape=True)
        self._bind(stream)
        check(self._lib.rcflow_phase_correlate_dev(self._h, stream, self._ptr(ta), ta.stride(0) * 4, self._ptr(tb),
                                                   tb.stride(0) * 4, w, h, 1 if window else 0, self._ptr(out)))
        return out

    def warp_translate(self, frame, shift_x, shift_y, out=None, stream=0):
        """warpAffine(frame, [1 0 -shift_x; 0 1 -shift_y]) on an 8UC3 frame (main.cpp:1749-1751): out(x, y) =
        frame(x + shift_x, y + shift_y), bilinear in 1/32 px, zero outside.  `out` (optional): the image to write."""
        f = self._img3(frame)
        out = self._out_or_new(out, torch.uint8, "out", f.shape, dense=True)
        self._bind(stream)
        check(self._lib.rcflow_warp_translate_bgr_dev(self._h, stream, self._ptr(f), f.stride(0), f.shape[1], f.shape[0],
                                                      self._ptr(out), out.stride(0), float(shift_x), float(shift_y)))
        return out

    def _warp(self, fn, nm, frame, M, inverse_map, dsize, out, stream):
        f = self._img3(frame)
        dw, dh = (f.shape[1], f.shape[0]) if dsize is None else (int(dsize[0]), int(dsize[1]))
        m = np.ascontiguousarray(np.asarray(M, np.float64)).reshape(-1)
        if m.size != nm:
            raise ValueError("expected a matrix of %d entries" % nm)
        out = self._out_or_new(out, torch.uint8, "out", (dh, dw, 3), dense=True)
        self._bind(stream)
        check(fn(self._h, stream, self._ptr(f), f.stride(0), f.shape[1], f.shape[0], self._ptr(out), out.stride(0), dw, dh,
                 m.ctypes.data_as(C.POINTER(C.c_double)), RC_WARP_INVERSE_MAP if inverse_map else 0))
        return out

    def warp_affine(self, frame, M, inverse_map=False, dsize=None, out=None, stream=0):
        """cv::warpAffine(frame, M (2 x 3), dsize = (dw, dh), INTER_LINEAR [| WARP_INVERSE_MAP]) on an 8UC3 frame, zero
        outside.  inverse_map: M maps destination to source as given (the form the bit-exact contract is stated on);
        otherwise it is inverted on the host first.  dsize: default the source's; `out`: the image to write."""
        return self._warp(self._lib.rcflow_warp_affine_bgr_dev, 6, frame, M, inverse_map, dsize, out, stream)

    def warp_perspective(self, frame, M, inverse_map=False, dsize=None, out=None, stream=0):
        """cv::warpPerspective(frame, M (3 x 3), dsize, INTER_LINEAR [| WARP_INVERSE_MAP]) on an 8UC3 frame: as warp_affine."""
        return self._warp(self._lib.rcflow_warp_perspective_bgr_dev, 9, frame, M, inverse_map, dsize, out, stream)

    def framestab_open(self, w, h, roi=None, stream=0, rois=None, model="similarity", min_response=0.0, anchor="previous"):
        """Opens the slot's stabilisation state (compute_phaseCorrelate, main.cpp:1684-1775) for w x h frames.
        roi = (x, y, w, h) of the static patch to track; default: the reference's (w - 50, 50, 50, 50).
        rois = [(x, y, w, h), ...] instead: 1..16 static patches of one size, and a motion fitted to their shifts
        (model "translation" | "similarity" | "affine") over the patches whose response is at least min_response;
        anchor "previous" registers every frame against the last corrected one, "first" against the first frame after
        open / reset.  The frame is then corrected for roll and zoom too (see framestab_motion)."""
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        if rois is None:
            x, y, rw, rh = (int(w) - 50, 50, 50, 50) if roi is None else (int(v) for v in roi)
            check(self._lib.rcflow_framestab_open(self._h, stream, int(w), int(h), x, y, rw, rh))
            return
        if roi is not None:
            raise ValueError("give roi or rois, not both")
        if model not in STAB_MODELS or anchor not in ("previous", "first"):
            raise ValueError("model must be one of %s, anchor \"previous\" or \"first\"" % sorted(STAB_MODELS))
        r = np.ascontiguousarray(np.asarray(rois, np.int32)).reshape(-1, 4)
        check(self._lib.rcflow_framestab_open_multi(self._h, stream, int(w), int(h), r.ctypes.data_as(C.POINTER(C.c_int)), len(r),
                                                    STAB_MODELS[model], float(min_response),
                                                    RC_STAB_ANCHOR_FIRST if anchor == "first" else 0))

    def framestab_motion(self, stream=0):
        """Waits for the slot's stream -> dict(motion (2 x 3 float64: T maps the corrected frame to the incoming one,
        corrected(p) = frame(T p)), model_used ("translation" | "similarity" | "affine" | None: the identity),
        patches_used, shifts (n x 3: dx, dy, response of every patch), frames_pushed, rois, model, min_response, anchor)."""
        n, model, flags, minr = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.)
        rois = (C.c_int * (4 * RC_STAB_MAX_PATCHES))()
        check(self._lib.rcflow_framestab_info_multi(self._h, stream, C.byref(n), rois, RC_STAB_MAX_PATCHES, C.byref(model),
                                                    C.byref(minr), C.byref(flags)))
        mo, sh = (C.c_double * 6)(), (C.c_double * (3 * RC_STAB_MAX_PATCHES))()
        used, cnt, frames = C.c_int(0), C.c_int(0), C.c_longlong(0)
        self._bind(stream)
        check(self._lib.rcflow_framestab_read_motion(self._h, stream, mo, C.byref(used), C.byref(cnt), sh, C.byref(frames)))
        return dict(motion=np.array(mo[:]).reshape(2, 3), model_used=FIT_MODEL_NAMES.get(used.value), patches_used=cnt.value,
                    shifts=np.array(sh[:3 * n.value]).reshape(n.value, 3), frames_pushed=frames.value,
                    rois=[tuple(rois[4 * k:4 * k + 4]) for k in range(n.value)], model=FIT_MODEL_NAMES[model.value],
                    min_response=minr.value, anchor="first" if flags.value & RC_STAB_ANCHOR_FIRST else "previous")

    def framestab_info(self, stream=0):
        """dict(w, h, roi, dft_size (N, M), launches_per_push, frames_pushed, device_bytes) of the open state."""
        w, h, lp = C.c_int(0), C.c_int(0), C.c_int(0)
        roi, dft = (C.c_int * 4)(), (C.c_int * 2)()
        frames, nbytes = C.c_longlong(0), C.c_size_t(0)
        check(self._lib.rcflow_framestab_info(self._h, stream, C.byref(w), C.byref(h), roi, dft, C.byref(lp),
                                              C.byref(frames), C.byref(nbytes)))
        return dict(w=w.value, h=h.value, roi=tuple(roi), dft_size=tuple(dft), launches_per_push=lp.value,
                    frames_pushed=frames.value, device_bytes=nbytes.value)

    def framestab_push(self, frame, out=None, result=None, stream=0):
        """One frame (HxWx3 uint8) -> the corrected frame (device image; `out`: a preallocated one to write).
        `result` (optional): a contiguous float64 device tensor of 3 that receives shift_x, shift_y, response of this
        push; nothing is synchronised, so a row of a larger tensor per push collects a whole clip's track."""
        info = self.framestab_info(stream)
        f = self._img3(frame)       # held to the end of the call: it may be a copy made here
        fp, fstep = self._in_image(f, torch.uint8, "frame", (info["h"], info["w"], 3))
        out = self._out_or_new(out, torch.uint8, "out", f.shape, dense=True)
        rp = self._out_array(result, torch.float64, "result", 3)
        self._bind(stream)
        check(self._lib.rcflow_framestab_push_dev(self._h, stream, fp, fstep, self._ptr(out), out.stride(0), rp))
        return out

    def framestab_read(self, stream=0):
        """Waits for the slot's stream -> ((shift_x, shift_y, response) of the last push, frames pushed)."""
        r = (C.c_double * 3)()
        n = C.c_longlong(0)
        self._bind(stream)
        check(self._lib.rcflow_framestab_read(self._h, stream, r, C.byref(n)))
        return (r[0], r[1], r[2]), n.value

    def framestab_reset(self, stream=0):
        self._lifecycle("framestab", "reset", stream)

    def framestab_close(self, stream=0):
        self._lifecycle("framestab", "close", stream)

    # ------------------------------------------------------------------ tracked corners, a robust fitted motion
    def corners(self, gray, cells=(16, 12), margin=12, min_score=1, pts=None, scores=None, stream=0):
        """One best Shi-Tomasi corner per grid cell of an 8UC1 image (include/rcflow.h states the integer response and the
        cells) -> (pts [cells, 2] float32 (x, y), scores [cells] int32; 0 and the cell centre for a cell without a
        corner), on the device, in cell order.  `pts`, `scores` (optional): tensors to write."""
        g = self._dev(gray, torch.uint8)
        if g.dim() != 2:
            raise ValueError("expected a 2-D uint8 image")
        g = g if g.stride(1) == 1 else g.contiguous()
        h, w = g.shape
        n = int(cells[0]) * int(cells[1])
        pts = self._out_or_new(pts, torch.float32, "pts", (max(n, 0), 2))
        scores = self._out_or_new(scores, torch.int32, "scores", (max(n, 0),))
        self._bind(stream)
        check(self._lib.rcflow_corners_dev(self._h, stream, self._ptr(g), g.stride(0), w, h, int(cells[0]), int(cells[1]), int(margin),
                                           int(min_score), self._ptr(pts), self._ptr(scores)))
        return pts, scores

    def fit_motion(self, p, q, status, size, scores=None, model="similarity", hypotheses=0, seed=0, min_score=0, quality=0.0,
                   max_shift=0.0, inlier_px=0.0, want_samples=False, stream=0):
        """Robust fit of q ~ T p over point pairs (RANSAC with the stated counter-based sampler, two least-squares refits,
        the ladder; include/rcflow.h).  p, q: [n, 2] float32; status: [n] uint8; scores: [n] int32 or None; size = (w, h).
        Waits for the stream -> dict(T (3 x 3 float64), model_used (name or None), n_valid, n_inliers, winner,
        inlier ([n] uint8), samples ([hypotheses, 4] int32 when asked for))."""
        if model not in FIT_MODELS:
            raise ValueError("model must be one of %s" % sorted(FIT_MODELS))
        tp = self._dev(p, torch.float32).reshape(-1, 2).contiguous()
        tq = self._dev(q, torch.float32).reshape(-1, 2).contiguous()
        ts = self._dev(status, torch.uint8).reshape(-1).contiguous()
        n = tp.shape[0]
        if tq.shape[0] != n or ts.shape[0] != n:
            raise ValueError("p, q and status differ in length")
        tsc = None
        if scores is not None:
            tsc = self._dev(scores, torch.int32).reshape(-1).contiguous()
            if tsc.shape[0] != n:
                raise ValueError("scores and p differ in length")
        prm = FitParams(FIT_MODELS[model], int(hypotheses), int(seed) & 0xffffffff, int(min_score), float(quality), float(max_shift),
                        float(inlier_px))
        res = torch.zeros(11, dtype=torch.float64, device=self.device)
        inl = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        nh = int(hypotheses) if hypotheses else 512
        smp = torch.full((max(nh, 1), 4), -1, dtype=torch.int32, device=self.device) if want_samples else None
        self._bind(stream)
        check(self._lib.rcflow_fit_motion_dev(self._h, stream, self._ptr(tp), self._ptr(tq), self._ptr(ts),
                                              self._ptr(tsc) if tsc is not None else C.c_void_p(None), n, int(size[0]), int(size[1]),
                                              C.byref(prm), self._ptr(res), self._ptr(inl),
                                              self._ptr(smp) if smp is not None else C.c_void_p(None)))
        self.sync(stream)
        raw = res.cpu().numpy()
        ints = raw[9:].view(np.int32)
        out = dict(T=raw[:9].reshape(3, 3).copy(), model_used=FIT_MODEL_NAMES.get(int(ints[0])), n_valid=int(ints[1]), n_inliers=int(ints[2]),
                   winner=int(ints[3]), inlier=inl[:n].cpu().numpy())
        if smp is not None:
            out["samples"] = smp.cpu().numpy()
        return out

    def framestab_open_tracks(self, w, h, model="similarity", cells=(0, 0), min_score=0, quality=0.0, win=21, max_level=3, max_count=30,
                              epsilon=0.01, max_shift=0.0, hypotheses=0, seed=0, inlier_px=0.0, anchor="previous", stream=0):
        """Opens the slot's stabilisation state in its tracking form: corners of the reference frame chosen on the device
        (one per grid cell), tracked by PyrLK, a robust fit (model "translation" | "similarity" | "affine" | "homography"),
        the warp.  framestab_push / _read / _reset / _close serve it; framestab_read_tracks returns T and the tracks.
        cells (0, 0): about 40 x 40 px each; anchor as framestab_open."""
        if model not in FIT_MODELS or anchor not in ("previous", "first"):
            raise ValueError("model must be one of %s, anchor \"previous\" or \"first\"" % sorted(FIT_MODELS))
        prm = StabTracks(int(cells[0]), int(cells[1]), int(min_score), float(quality), int(win), int(max_level), int(max_count),
                         float(epsilon), float(max_shift), FIT_MODELS[model], int(hypotheses), int(seed) & 0xffffffff, float(inlier_px),
                         RC_STAB_ANCHOR_FIRST if anchor == "first" else 0)
        self._bind(stream)
        check(self._lib.rcflow_framestab_open_tracks(self._h, stream, int(w), int(h), C.byref(prm)))

    def framestab_read_tracks(self, stream=0):
        """Waits for the slot's stream -> dict(T (3 x 3: corrected(p) = frame(T p)), model_used (name or None), n_valid,
        n_inliers, pts ([cells, 4]: corner x, y in the reference frame, its track x, y), inlier, scores, frames_pushed)."""
        cells, used, nv, ni, frames = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
        T = (C.c_double * 9)()
        self._bind(stream)
        check(self._lib.rcflow_framestab_read_tracks(self._h, stream, None, None, None, None, None, None, None, 0, C.byref(cells), None))
        n = cells.value
        pts, inl, sc = np.zeros((n, 4), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.int32)
        check(self._lib.rcflow_framestab_read_tracks(self._h, stream, T, C.byref(used), C.byref(nv), C.byref(ni), pts.ctypes.data,
                                                     inl.ctypes.data, sc.ctypes.data, n, C.byref(cells), C.byref(frames)))
        return dict(T=np.array(T[:]).reshape(3, 3), model_used=FIT_MODEL_NAMES.get(used.value), n_valid=nv.value, n_inliers=ni.value, pts=pts,
                    inlier=inl, scores=sc, frames_pushed=frames.value)

    # ------------------------------------------------------------------ the opposing-flow map
    def ripmap_open(self, w, h, window=300, grid=(30, 30), source="flow", wait_full=False, stream=0):
        """Opens the slot's opposing-flow map (averageVector, ripcurrents_module.cpp:386-484, finished) for w x h flow
        fields: a mean over the last `window` fields, summed per cell of a grid = (grid_x, grid_y), and the cells whose
        summed mean points away from the frame's.  source "flow": the field as it is; "delta": get_delta from a zero point
        with dt = 2 and the slot's UPPER.  wait_full: no cell is opposed until `window` fields have been pushed.
        The ring takes window * h * w * 8 bytes of device memory."""
        if source not in RIPMAP_SOURCES:
            raise ValueError("source must be one of %s" % sorted(RIPMAP_SOURCES))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_ripmap_open(self._h, stream, int(w), int(h), int(window), int(grid[0]), int(grid[1]),
                                           RIPMAP_SOURCES[source], RC_RIPMAP_WAIT_FULL if wait_full else 0))

    def ripmap_info(self, stream=0):
        """dict(w, h, window, grid, source, wait_full, min_opposition_cos2, min_cell_mag, frames_pushed, device_bytes)."""
        v = [C.c_int(0) for _ in range(7)]
        k, m = C.c_double(0.), C.c_double(0.)
        frames, nbytes = C.c_longlong(0), C.c_size_t(0)
        check(self._lib.rcflow_ripmap_info(self._h, stream, *[C.byref(x) for x in v], C.byref(k), C.byref(m), C.byref(frames),
                                           C.byref(nbytes)))
        w, h, window, gx, gy, source, flags = (x.value for x in v)
        return dict(w=w, h=h, window=window, grid=(gx, gy), source=RIPMAP_SOURCE_NAMES[source],
                    wait_full=bool(flags & RC_RIPMAP_WAIT_FULL), min_opposition_cos2=k.value, min_cell_mag=m.value,
                    frames_pushed=frames.value, device_bytes=nbytes.value)

    def ripmap_set(self, min_opposition_cos2=0.3454915028125263, min_cell_mag=0.0, stream=0):
        """The decision's numbers: a cell is opposed when cos^2 of its angle to the frame's direction exceeds
        min_opposition_cos2 on the far side (default: 0.7 pi, the reference's) and its mean is at least min_cell_mag px."""
        check(self._lib.rcflow_ripmap_set(self._h, stream, float(min_opposition_cos2), float(min_cell_mag)))

    def ripmap_push(self, flow=None, hsv=None, mask=None, cells=None, summary=None, stream=0):
        """One flow field (HxWx2 float32, pixels dense, rows may be padded; None: the field push_frame_host / frame_loop_step
        left on the slot).
        Outputs are preallocated device tensors, each optional: hsv HxWx3 uint8 (vectorToColor of the mean, scaled by the
        previous push's maximum), mask HxW uint8 (255 inside an opposed cell), cells grid_y x grid_x x 4 float32
        (mean x, mean y, angle to the frame's direction, opposed), summary 8 float64.  Nothing is synchronised."""
        info = self.ripmap_info(stream)
        h, w, (gx, gy) = info["h"], info["w"], info["grid"]
        if flow is not None:
            flow = self._dev(flow, torch.float32)
        fp, fstep = self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True)
        hp, hstep = self._out_image(hsv, torch.uint8, "hsv", (h, w, 3))
        mp, mstep = self._out_image(mask, torch.uint8, "mask", (h, w))
        cp = C.c_void_p(None) if cells is None else self._ptr(_check_out(cells, self.device, torch.float32, "cells", shape=(gy, gx, 4)))
        sp = self._out_array(summary, torch.float64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_ripmap_push_dev(self._h, stream, fp, fstep, hp, hstep, mp, mstep, cp, sp))

    def ripmap_mean(self, out=None, stream=0):
        """The window mean as it stands -> HxWx2 float32 device tensor (a copy, queued on the slot's stream)."""
        info = self.ripmap_info(stream)
        out = self._out_or_new(out, torch.float32, "out", (info["h"], info["w"], 2), dense=True)
        self._bind(stream)
        check(self._lib.rcflow_ripmap_mean_dev(self._h, stream, self._ptr(out), out.stride(0) * 4))
        return out

    def ripmap_read(self, stream=0):
        """Waits for the slot's stream -> dict(cells (grid_y x grid_x x 4 float32), opposed (bool grid), summary (8 float64),
        direction, mean_magnitude, opposed_cells, live_cells, bad_pixels, max_magnitude, sums (grid_y x grid_x x 3 int64:
        Sx, Sy, n), frames_pushed) of the last push."""
        gx, gy = self.ripmap_info(stream)["grid"]
        cells, summary = np.zeros((gy, gx, 4), np.float32), np.zeros(8, np.float64)
        sums, frames = np.zeros((gy, gx, 3), np.int64), C.c_longlong(0)
        self._bind(stream)
        check(self._lib.rcflow_ripmap_read(self._h, stream, cells.ctypes.data, summary.ctypes.data, sums.ctypes.data,
                                           C.byref(frames)))
        return dict(cells=cells, opposed=cells[..., 3] != 0, summary=summary, direction=summary[0], mean_magnitude=summary[1],
                    opposed_cells=int(summary[2]), live_cells=int(summary[3]), bad_pixels=int(summary[4]),
                    max_magnitude=summary[6], sums=sums, frames_pushed=frames.value)

    def ripmap_reset(self, stream=0):
        self._lifecycle("ripmap", "reset", stream)

    def ripmap_close(self, stream=0):
        self._lifecycle("ripmap", "close", stream)

    # ------------------------------------------------------------------ motion templates
    def motion_open(self, w, h, diff_threshold=30, duration=1.0, delta1=0.25, delta2=1.0, grid=(1, 1), fresh=False, stream=0):
        """Opens the slot's motion templates for w x h gray frames (include/rcflow.h, "motion templates"): a motion history
        kept on the device from push to push, its gradient, and the orientation of every cell of grid = (grid_x, grid_y) and
        of the frame.  The defaults are the reference's numbers (globalOrientation, ripcurrents_module.cpp:319-359); its
        arrows every 30 px are grid=(w // 30, h // 30).  fresh: the reference's literal call, the history zeroed before
        every update (RC_MOTION_FRESH).  The state takes about 10 bytes per pixel of device memory."""
        p = MotionParams(diff_threshold=int(diff_threshold), duration=float(duration), delta1=float(delta1), delta2=float(delta2),
                         grid_x=int(grid[0]), grid_y=int(grid[1]), flags=RC_MOTION_FRESH if fresh else 0)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_motion_open(self._h, stream, int(w), int(h), C.byref(p)))

    def motion_info(self, stream=0):
        """dict(w, h, diff_threshold, duration, delta1, delta2, grid, fresh, launches_per_push, pushes, last_timestamp,
        device_bytes); never blocks."""
        i = self._info("motion", MotionInfo(), stream)
        d = _record(i, skip=("flags", "grid_x", "grid_y"))
        d.update(grid=(i.prm.grid_x, i.prm.grid_y), fresh=bool(i.prm.flags & RC_MOTION_FRESH))
        return d

    def motion_push(self, gray, timestamp=None, mhi=None, orient=None, mask=None, vis=None, cells=None, frame=None, stream=0):
        """One gray frame (HxW uint8 device tensor, dense pixels, rows may be padded): three launches, nothing is synchronised.
        timestamp: None for "pushes so far + 1", else a number greater than the last push's.  Outputs are preallocated
        device tensors, each optional: mhi and orient HxW float32, mask HxW uint8 (255 / 0), vis HxWx3 uint8 (the history as
        a grey picture), cells a contiguous uint8 tensor of grid_y * grid_x * 40 bytes (rc_motion_cell records,
        MOTION_CELL_DTYPE), frame one such record.  The records also stay on the slot for motion_read / motion_prims."""
        i = self._info("motion", MotionInfo(), stream)
        h, w, gx, gy = i.h, i.w, i.prm.grid_x, i.prm.grid_y
        gp, gstep = self._in_image(gray, torch.uint8, "gray", (h, w))
        images = (self._out_image(mhi, torch.float32, "mhi", (h, w)) + self._out_image(orient, torch.float32, "orient", (h, w)) +
                  self._out_image(mask, torch.uint8, "mask", (h, w)) + self._out_image(vis, torch.uint8, "vis", (h, w, 3)))
        cp = self._out_array(cells, torch.uint8, "cells", gx * gy * MOTION_CELL_DTYPE.itemsize)
        fp = self._out_array(frame, torch.uint8, "frame", MOTION_CELL_DTYPE.itemsize)
        self._bind(stream)
        check(self._lib.rcflow_motion_push_dev(self._h, stream, gp, gstep,
                                               RC_MOTION_AUTO_TIME if timestamp is None else float(timestamp), *images, cp, fp))

    def motion_read(self, stream=0):
        """Waits for the slot's stream -> dict(cells (grid_y x grid_x numpy array of MOTION_CELL_DTYPE), frame (one record),
        angle (the frame's, degrees in [0, 360), y down), silhouette (pixels of the last silhouette)) of the last push."""
        gx, gy = self.motion_info(stream)["grid"]
        cells, frame, sil = np.zeros(gx * gy, MOTION_CELL_DTYPE), np.zeros(1, MOTION_CELL_DTYPE), C.c_longlong(0)
        self._bind(stream)
        check(self._lib.rcflow_motion_read(self._h, stream, cells.ctypes.data, gx * gy, frame.ctypes.data, C.byref(sil)))
        return dict(cells=cells.reshape(gy, gx), frame=frame[0], angle=float(frame[0]["angle"]), silhouette=sil.value)

    def motion_prims(self, color=0x00ffff, thickness=1, disc_radius=2, length=15.0, out=None, stream=0):
        """The records of the last push as 2 * (cells + 1) primitives for draw() -> a device uint8 tensor of rc_draw_prim
        records: per cell a disc at its centre and a line of `length` pixels along its angle, the frame's pair last at the
        image centre; a set without a direction (W == 0) gives kind 0, which draw() skips (and counts)."""
        gx, gy = self.motion_info(stream)["grid"]
        n = 2 * (gx * gy + 1)
        out = self._prims_out(out, n)
        self._bind(stream)
        check(self._lib.rcflow_motion_prims_dev(self._h, stream, int(color), int(thickness), int(disc_radius), float(length), self._ptr(out)))
        return out

    def motion_reset(self, stream=0):
        self._lifecycle("motion", "reset", stream)

    def motion_close(self, stream=0):
        self._lifecycle("motion", "close", stream)

    def globalOrientation(self, prev, cur, stream=0):
        """The reference's call in one line (ripcurrents_module.cpp:319-359): the direction of the motion between two gray
        frames -> (angle in degrees, HxWx3 uint8 picture of the silhouette: its hist_gray before the arrows).  Opens the
        slot's motion templates with fresh=True and the reference's numbers unless a session of that size is open; with an
        open session of another kind its parameters hold."""
        prev, cur = self._dev(prev, torch.uint8), self._dev(cur, torch.uint8)
        h, w = int(cur.shape[0]), int(cur.shape[1])
        try:
            info = self.motion_info(stream)
        except RcflowError:
            info = None
        if info is None or (info["w"], info["h"]) != (w, h):
            self.motion_open(w, h, fresh=True, stream=stream)
        else:
            self.motion_reset(stream)
        vis = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
        self.motion_push(prev, stream=stream)
        self.motion_push(cur, vis=vis, stream=stream)
        return self.motion_read(stream)["angle"], vis

    # ------------------------------------------------------------------ tracer lines and drawing
    def draw(self, img, prims, skipped=None, stream=0):
        """rcflow_draw_dev: paints the primitives into img (HxW or HxWx3 uint8 device tensor, dense pixels, rows may be
        padded) in place, in list order, by the rules of include/rcflow.h.  prims: a device uint8 / int32 tensor holding
        32-byte rc_draw_prim records, or a numpy array of DRAW_PRIM_DTYPE (copied to the device).  skipped: an optional
        one-element int64 device tensor that is increased by the number of skipped primitives."""
        ch = int(img.shape[2]) if _is_t(img) and img.dim() == 3 else 1
        if not (_is_t(img) and img.dim() in (2, 3) and ch in (1, 3) and _fits(img, self.device, torch.uint8, dense=True)):
            raise ValueError("img must be a uint8 tensor on %s of shape HxW or HxWx3, with dense pixels" % self.device)
        if isinstance(prims, np.ndarray):
            if prims.dtype != DRAW_PRIM_DTYPE:
                raise ValueError("prims must have dtype DRAW_PRIM_DTYPE")
            prims = torch.from_numpy(np.ascontiguousarray(prims).view(np.uint8).reshape(-1)).to(self.device)
        if not (_is_t(prims) and prims.is_cuda and prims.device == self.device and prims.is_contiguous()):
            raise ValueError("prims must be a contiguous tensor on %s or a numpy array of DRAW_PRIM_DTYPE" % self.device)
        nbytes = prims.numel() * prims.element_size()
        if nbytes % 32:
            raise ValueError("prims must hold whole 32-byte records")
        sp = C.c_void_p(None)
        if skipped is not None:
            sp = self._ptr(_check_out(skipped, self.device, torch.int64, "skipped", numel=1))
        self._bind(stream)
        check(self._lib.rcflow_draw_dev(self._h, stream, self._ptr(img), img.stride(0), int(img.shape[1]), int(img.shape[0]), ch,
                                        self._ptr(prims), nbytes // 32, sp))
        return img

    def trace_prims(self, trace, start=None, color=0xffffff, stream=0):
        """rcflow_trace_prims_dev: the trace of streamline(..., trace=True) (n x iters x 2 float32 on the device) as thin
        lines with rounded ends -> a device uint8 tensor of rc_draw_prim records for draw().  start: the n seeds before
        the advection (n x 2), optional."""
        tr = _check_out(trace, self.device, torch.float32, "trace", shape=tuple(trace.shape[:2]) + (2,))
        n, iters = int(tr.shape[0]), int(tr.shape[1])
        st = None if start is None else self._dev(start, torch.float32).reshape(n, 2).contiguous()
        per = iters if st is not None else iters - 1
        out = torch.empty((n * per, 32), dtype=torch.uint8, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_trace_prims_dev(self._h, stream, None if st is None else self._ptr(st), self._ptr(tr), n, iters,
                                               int(color), self._ptr(out)))
        return out

    def tracers_open(self, w, h, mover="lk", max_lines=16, max_vertices=1024, max_points=0, lk=None, dt=1.0, stream=0):
        """Opens the slot's tracer session for w x h frames: streaklines, timelines and point clouds whose vertices stay on
        the device (compute_streaklines / compute_timelines / compute_populationMap, main.cpp:78-176).  mover "lk": sparse
        PyrLK between consecutive gray frames; lk = dict(win=(w, h), max_level, crit_type, max_count, epsilon, flags,
        min_eig_threshold), None: the reference's call (Streakline.cpp:32).  mover "flow": one step of the dense field
        with dt (Streakline.run).  A streakline is a ring of max_vertices; max_points bounds all vertices together
        (0: max_lines * max_vertices)."""
        if mover not in TRACERS_MOVERS:
            raise ValueError("mover must be one of %s" % sorted(TRACERS_MOVERS))
        p = TracersParams(mover=TRACERS_MOVERS[mover], max_lines=int(max_lines), max_vertices=int(max_vertices),
                          max_points=int(max_points), dt=float(dt))
        if lk is not None:
            win = lk.get("win", (50, 50))
            p.win_w, p.win_h, p.max_level = int(win[0]), int(win[1]), int(lk.get("max_level", 3))
            p.crit_type, p.max_count, p.epsilon = int(lk.get("crit_type", 3)), int(lk.get("max_count", 30)), float(lk.get("epsilon", 0.1))
            p.lk_flags, p.min_eig = int(lk.get("flags", 10)), float(lk.get("min_eig_threshold", 1e-4))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_tracers_open(self._h, stream, int(w), int(h), C.byref(p)))

    def tracers_add(self, kind, xy, stream=0):
        """Adds a line from host points -> its id.  kind "streak": xy is the generation point; "timeline", "cloud": the
        n x 2 vertices.  Blocking."""
        if kind not in TRACER_KINDS:
            raise ValueError("kind must be one of %s" % sorted(TRACER_KINDS))
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        self._bind(stream)
        return check(self._lib.rcflow_tracers_add(self._h, stream, TRACER_KINDS[kind], a.ctypes.data, a.shape[0]))

    def tracers_add_streakline(self, pixel, stream=0):
        return self.tracers_add("streak", [pixel], stream)

    def tracers_add_timeline(self, lineStart, lineEnd, numberOfVertices, stream=0):
        """Timeline's constructor (ripcurrents_module.cpp:751-762): numberOfVertices + 1 points on the segment."""
        return self.tracers_add("timeline", Timeline(lineStart, lineEnd, numberOfVertices).vertices, stream)

    def tracers_add_cloud(self, rectStart, rectEnd, numberOfVertices, rng=None, stream=0):
        """PopulationMap's constructor (ripcurrents_module.cpp:1140-1152) with `rng` in place of rand()."""
        return self.tracers_add("cloud", PopulationMap(rectStart, rectEnd, numberOfVertices, rng).vertices, stream)

    def tracers_info(self, stream=0):
        """dict of rc_tracers_info; never blocks."""
        info = self._info("tracers", TracersInfo(), stream)
        d = _record(info)
        d.update(mover=TRACERS_MOVER_NAMES[info.mover], primed=bool(info.primed))
        return d

    def tracers_push(self, gray=None, flow=None, canvas=None, stream=0):
        """One frame: moves every vertex of every line, does the reference's book-keeping and, with canvas (HxWx3 uint8
        device tensor, dense pixels), draws the lines into it in place.  gray: HxW uint8 (mover "lk"); flow: HxWx2 float32
        (mover "flow"; None: the field push_frame_host / frame_loop_step left on the slot).  Nothing is synchronised.
        Returns False from a priming push (mover "lk": the first frame), else True."""
        i = self._info("tracers", TracersInfo(), stream)
        h, w = i.h, i.w
        lk = i.mover == TRACERS_MOVERS["lk"]        # the mover's own input is looked at, the other one ignored
        gray = self._dev(gray, torch.uint8) if lk else None
        flow = self._dev(flow, torch.float32) if not lk and flow is not None else None
        gp, gstep = self._in_image(gray, torch.uint8, "gray", (h, w), optional=not lk)
        fp, fstep = self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True)
        cp, cstep = self._out_image(canvas, torch.uint8, "canvas", (h, w, 3))
        self._bind(stream)
        return check(self._lib.rcflow_tracers_push_dev(self._h, stream, gp, gstep, fp, fstep, cp, cstep)) == 0

    def tracers_read(self, line, stream=0):
        """Waits for the slot's stream -> (vertices n x 2 float32 in the reference's order: a streakline newest first,
        primitives skipped by the session's drawing so far)."""
        n, sk = C.c_int(0), C.c_longlong(0)
        self._bind(stream)
        check(self._lib.rcflow_tracers_read(self._h, stream, int(line), None, 0, C.byref(n), None))
        xy = np.zeros((max(n.value, 1), 2), np.float32)
        check(self._lib.rcflow_tracers_read(self._h, stream, int(line), xy.ctypes.data, xy.shape[0], C.byref(n), C.byref(sk)))
        return xy[:n.value], sk.value

    def tracers_prims(self, stream=0):
        """The primitives of the last push -> numpy array of DRAW_PRIM_DTYPE (waits for the slot's stream; for tests and
        hosts that paint elsewhere)."""
        ptr, n = C.c_void_p(None), C.c_int(0)
        check(self._lib.rcflow_tracers_prims(self._h, stream, C.byref(ptr), C.byref(n)))
        if not n.value:
            return np.zeros(0, DRAW_PRIM_DTYPE)
        self._bind(stream)          # the copy below runs on torch's current stream, behind the pushes
        if stream in self._own:
            self.sync(stream)
        host = _alias_tensor(ptr.value, n.value * 8, torch.int32, self.device).cpu()
        return host.numpy().view(DRAW_PRIM_DTYPE).reshape(-1).copy()

    def tracers_reset(self, stream=0):
        self._lifecycle("tracers", "reset", stream)

    def tracers_close(self, stream=0):
        self._lifecycle("tracers", "close", stream)

    # ------------------------------------------------------------------ flow map and FTLE
    def ftle_open(self, w, h, window=30, direction="backward", dt=1.0, spacing=1, threshold=0.1, vis_max=0.5, stream=0):
        """Opens the slot's flow map and FTLE for w x h flow fields (include/rcflow.h, "flow map and FTLE"): a ring of the
        last `window` fields, a particle from every pixel carried through them ("backward": newest to oldest with -dt, whose
        ridges are where the water gathers; "forward": oldest to newest), the largest eigenvalue of the Cauchy-Green tensor
        from central differences at +-spacing, its logarithm per frame, a mask at ftle >= threshold and a JET picture
        scaled to vis_max.  The ring takes 8 bytes per pixel and field of device memory (0.5 GB at 1080p and window 30)."""
        p = FtleParams(window=int(window), direction=FTLE_DIRECTIONS[direction] if isinstance(direction, str) else int(direction),
                       dt=float(dt), spacing=int(spacing), threshold=float(threshold), vis_max=float(vis_max), flags=0)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_ftle_open(self._h, stream, int(w), int(h), C.byref(p)))

    def ftle_info(self, stream=0):
        """dict(w, h, window, direction, dt, spacing, threshold, vis_max, launches_per_push, held, pushes, device_bytes);
        never blocks."""
        i = self._info("ftle", FtleInfo(), stream)
        d = _record(i, skip=("flags",))
        d["direction"] = FTLE_DIRECTION_NAMES[d["direction"]]
        return d

    def ftle_push(self, flow, map=None, steps=None, lam=None, ftle=None, mask=None, vis=None, summary=None, stream=0):
        """One flow field (HxWx2 float32 device tensor, dense pixels, rows may be padded) into the ring; nothing is
        synchronised.  Outputs are preallocated device tensors, each optional: map HxWx2 float32 (the displacements), steps
        HxW int32, lam and ftle HxW float32, mask HxW uint8 (255 / 0: what regions_push takes), vis HxWx3 uint8, summary
        8 int64 (FTLE_SUMMARY).  Without any output the push is one launch that stores the field; with any it is
        RC_FTLE_LAUNCHES.  The summary also stays on the slot for ftle_read."""
        i = self._info("ftle", FtleInfo(), stream)
        h, w = i.h, i.w
        fp, fstep = self._in_image(flow, torch.float32, "flow", (h, w, 2))
        images = (self._out_image(map, torch.float32, "map", (h, w, 2)) + self._out_image(steps, torch.int32, "steps", (h, w)) +
                  self._out_image(lam, torch.float32, "lam", (h, w)) + self._out_image(ftle, torch.float32, "ftle", (h, w)) +
                  self._out_image(mask, torch.uint8, "mask", (h, w)) + self._out_image(vis, torch.uint8, "vis", (h, w, 3)))
        sp = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_ftle_push_dev(self._h, stream, fp, fstep, *images, sp))

    def ftle_read(self, stream=0):
        """Waits for the slot's stream -> dict of the summary of the last push that computed one (FTLE_SUMMARY names, and
        max_lam: the largest eigenvalue as a float); zeros before that."""
        return self._summary(self._lib.rcflow_ftle_read, stream, FTLE_SUMMARY, bits=("max_lam_bits", "max_lam", float))

    def ftle_set(self, threshold, vis_max, stream=0):
        """threshold and vis_max from the next push on."""
        check(self._lib.rcflow_ftle_set(self._h, stream, float(threshold), float(vis_max)))

    def ftle_reset(self, stream=0):
        self._lifecycle("ftle", "reset", stream)

    def ftle_close(self, stream=0):
        self._lifecycle("ftle", "close", stream)

    # ------------------------------------------------------------------ plan view
    def planview_open(self, w, h, H, fx, fy, cx, cy, k1=0.0, k2=0.0, x0=0.0, y0=0.0, dx=1.0, dy=1.0, nx=1, ny=1, fps=1.0,
                      max_gsd=float("inf"), stream=0):
        """Opens the slot's plan view for w x h fields and frames (include/rcflow.h, "plan view"): a ground grid of nx x ny
        cells of dx x dy metres from (x0, y0), seen through H (3 x 3, ground (X, Y, 1) in metres -> homogeneous ideal pixel)
        and the radial distortion k1, k2 about (cx, cy) with focal lengths fx, fy.  The push resamples the field onto the
        grid in metres per second (fps fields per second) and the frame beside it; cells whose pixel covers more than max_gsd
        metres, or that the camera does not see, are left out.  The table takes 32 bytes per cell of device memory and is
        built here, once, on the device; re-opening is how parameters change."""
        p = PlanViewParams(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), k1=float(k1), k2=float(k2), x0=float(x0), y0=float(y0),
                           dx=float(dx), dy=float(dy), nx=int(nx), ny=int(ny), fps=float(fps), max_gsd=float(max_gsd), flags=0)
        p.H[:] = [float(v) for v in np.asarray(H, np.float64).reshape(9)]
        self._bind(stream)          # the table is built and the state zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_planview_open(self._h, stream, int(w), int(h), C.byref(p)))

    def planview_info(self, stream=0):
        """dict(w, h, the parameters (H a tuple of 9), launches_per_push, pushes, device_bytes); never blocks."""
        i = self._info("planview", PlanViewInfo(), stream)
        d = _record(i, skip=("H", "flags"))
        d["H"] = tuple(i.prm.H)
        return d

    def planview_push(self, flow=None, bgr=None, plan=None, mask=None, plan_bgr=None, summary=None, stream=0):
        """One launch; nothing is synchronised.  Inputs (device tensors with dense pixels, rows may be padded; either may be
        None, not both): flow HxWx2 float32, bgr HxWx3 uint8.  Outputs are preallocated device tensors, each optional: plan
        NYxNXx2 float32 (metres per second; what ripmap_push, regions_push and ftle_push take), mask NYxNX uint8 (255 where
        the cell is valid, else 0) and summary 8 int64 (PLANVIEW_SUMMARY) need the field, plan_bgr NYxNXx3 uint8 the frame.
        The summary also stays on the slot for planview_read."""
        i = self._info("planview", PlanViewInfo(), stream)
        h, w, ny, nx = i.h, i.w, i.prm.ny, i.prm.nx
        ins = (self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True) +
               self._in_image(bgr, torch.uint8, "bgr", (h, w, 3), optional=True))
        images = (self._out_image(plan, torch.float32, "plan", (ny, nx, 2)) + self._out_image(mask, torch.uint8, "mask", (ny, nx)) +
                  self._out_image(plan_bgr, torch.uint8, "plan_bgr", (ny, nx, 3)))
        sp = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_planview_push_dev(self._h, stream, *ins, *images, sp))

    def planview_read(self, stream=0):
        """Waits for the slot's stream -> dict of the summary of the last push (PLANVIEW_SUMMARY names, and max_speed: the
        largest plan speed in metres per second as a float); zeros before the first."""
        return self._summary(self._lib.rcflow_planview_read, stream, PLANVIEW_SUMMARY, bits=("max_speed2_bits", "max_speed", np.sqrt))

    def planview_table(self, stream=0):
        """Waits for the slot's stream -> the table, NY x NX x 8 float32: U, V (the pixel of the cell's centre), m00, m01, m10,
        m11 (pixels per field -> metres per second), gsd (metres per pixel), 1; eight zeros where the cell is not usable."""
        info = self.planview_info(stream)
        tab = np.empty((info["ny"], info["nx"], 8), np.float32)
        self._bind(stream)
        check(self._lib.rcflow_planview_table_read(self._h, stream, tab.ctypes.data))
        return tab

    def planview_reset(self, stream=0):
        self._lifecycle("planview", "reset", stream)

    def planview_close(self, stream=0):
        self._lifecycle("planview", "close", stream)

    # ------------------------------------------------------------------ wave spectra
    def waves_open(self, w, h, window=256, bin_lo=1, bin_hi=1, spacing=2, grid_x=1, grid_y=1, min_pixels=1, fps=2.0, metres_per_pixel_x=1.0,
                   metres_per_pixel_y=1.0, gravity=9.81, tanh_max=0.95, vis_max_depth=10.0, stream=0):
        """Opens the slot's wave spectra for w x h grey frames (include/rcflow.h, "wave spectra"): a ring of the last `window`
        frames, a sliding DFT at bins bin_lo..bin_hi per pixel (bin b is b * fps / window Hz), and per cell of a grid_x x grid_y
        grid the strongest bin, the wavenumber from its phase differences over 2 * spacing pixels, the celerity and the depth.
        The state takes window + 8 * bins bytes per pixel of device memory (0.8 GB at 1080p, window 256 and 16 bins)."""
        p = WavesParams(window=int(window), bin_lo=int(bin_lo), bin_hi=int(bin_hi), spacing=int(spacing), grid_x=int(grid_x), grid_y=int(grid_y),
                        min_pixels=int(min_pixels), flags=0, fps=float(fps), metres_per_pixel_x=float(metres_per_pixel_x),
                        metres_per_pixel_y=float(metres_per_pixel_y), gravity=float(gravity), tanh_max=float(tanh_max),
                        vis_max_depth=float(vis_max_depth))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_waves_open(self._h, stream, int(w), int(h), C.byref(p)))

    def waves_info(self, stream=0):
        """dict(w, h, the parameters, launches_per_push, bins, shift, held, pushes, device_bytes); never blocks."""
        i = self._info("waves", WavesInfo(), stream)
        return _record(i, skip=("flags",))

    def waves_push(self, gray, mask=None, cells=None, sums=None, bin_map=None, vis=None, summary=None, stream=0):
        """One grey frame (HxW uint8 device tensor, rows may be padded) into the ring and the spectrum; nothing is synchronised.
        mask (HxW uint8, optional) limits the pixels that take part.  Outputs are preallocated device tensors, each optional:
        cells GYxGXx32 uint8 (rc_wave_cell records; view the host copy as WAVE_CELL_DTYPE), sums GYxGXxKx6 int64, bin_map HxW
        uint8, vis HxWx3 uint8, summary 8 int64 (WAVES_SUMMARY).  Without any output the push is one launch; with any it is at
        most RC_WAVES_LAUNCHES.  Records, sums and summary also stay on the slot for waves_read."""
        i = self._info("waves", WavesInfo(), stream)
        h, w, gx, gy, K = i.h, i.w, i.prm.grid_x, i.prm.grid_y, i.bins
        ins = self._in_image(gray, torch.uint8, "gray", (h, w)) + self._in_image(mask, torch.uint8, "mask", (h, w), optional=True)
        cp = self._out_array(cells, torch.uint8, "cells", gy * gx * 32)
        sp = self._out_array(sums, torch.int64, "sums", gy * gx * K * 6)
        images = self._out_image(bin_map, torch.uint8, "bin_map", (h, w)) + self._out_image(vis, torch.uint8, "vis", (h, w, 3))
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_waves_push_dev(self._h, stream, *ins, cp, sp, *images, up))

    def waves_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX WAVE_CELL_DTYPE, sums GYxGXxKx6 int64, dict of the summary by
        WAVES_SUMMARY names) of the last push that computed them; zeros before that."""
        info = self.waves_info(stream)
        gx, gy, K = info["grid_x"], info["grid_y"], info["bins"]
        cells = np.zeros((gy, gx), WAVE_CELL_DTYPE)
        sums = np.zeros((gy, gx, K, 6), np.int64)
        return cells, sums, self._summary(self._lib.rcflow_waves_read, stream, WAVES_SUMMARY, cells.ctypes.data, sums.ctypes.data)

    def waves_spectrum(self, stream=0):
        """Waits for the slot's stream -> the accumulators, K x H x W x 2 int32 (re, im); for tests."""
        info = self.waves_info(stream)
        out = np.empty((info["bins"], info["h"], info["w"], 2), np.int32)
        self._bind(stream)
        check(self._lib.rcflow_waves_spectrum_read(self._h, stream, out.ctypes.data))
        return out

    def waves_table(self, stream=0):
        """-> (Tc, Ts), `window` int32 each: the twiddle table open built; never blocks."""
        n = self.waves_info(stream)["window"]
        tc, ts = np.empty(n, np.int32), np.empty(n, np.int32)
        check(self._lib.rcflow_waves_table_read(self._h, stream, tc.ctypes.data, ts.ctypes.data))
        return tc, ts

    def waves_set(self, tanh_max, min_pixels, vis_max_depth, stream=0):
        """tanh_max, min_pixels and vis_max_depth from the next push on."""
        check(self._lib.rcflow_waves_set(self._h, stream, float(tanh_max), int(min_pixels), float(vis_max_depth)))

    def waves_reset(self, stream=0):
        self._lifecycle("waves", "reset", stream)

    def waves_close(self, stream=0):
        self._lifecycle("waves", "close", stream)

    # ------------------------------------------------------------------ ensemble PIV
    def piv_open(self, w, h, window=32, range=8, step=16, ensemble=1, replace=False, min_peak=0.25, median_eps=0.1, median_thr=2.0,
                 vis_max=4.0, stream=0):
        """Opens the slot's ensemble PIV for w x h grey frames (include/rcflow.h, "ensemble PIV"): interrogation windows of
        `window` pixels every `step` pixels, searched over +-`range` pixels, the correlation sums added over the last `ensemble`
        frame pairs before the peak is taken.  The state takes (24 + 12 * ensemble) * (2 * range + 1)^2 bytes per cell of device
        memory, without the ring term for an ensemble of 1."""
        p = PivParams(window=int(window), range=int(range), step=int(step), ensemble=int(ensemble), flags=RC_PIV_REPLACE if replace else 0,
                      min_peak=float(min_peak), median_eps=float(median_eps), median_thr=float(median_thr), vis_max=float(vis_max))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_piv_open(self._h, stream, int(w), int(h), C.byref(p)))

    def piv_info(self, stream=0):
        """dict(w, h, the parameters, replace, grid_x, grid_y, launches_per_push, pairs, pushes, device_bytes); never blocks."""
        i = self._info("piv", PivInfo(), stream)
        d = _record(i, skip=("flags",))
        d["replace"] = bool(i.prm.flags & RC_PIV_REPLACE)
        return d

    def piv_push(self, gray, cells=None, field=None, vis=None, summary=None, stream=0):
        """One grey frame (HxW uint8 device tensor, rows may be padded), correlated against the slot's previous one; nothing is
        synchronised.  Outputs are preallocated device tensors, each optional: cells GYxGXx32 uint8 (rc_piv_cell records; view
        the host copy as PIV_CELL_DTYPE), field GYxGXx2 float32 (pixels per frame: the small flow field ripmap_push and the
        others take), vis HxWx3 uint8, summary 8 int64 (PIV_SUMMARY).  Without any output the push is one launch; with any it
        is RC_PIV_LAUNCHES.  Records and summary also stay on the slot for piv_read."""
        i = self._info("piv", PivInfo(), stream)
        h, w, gx, gy = i.h, i.w, i.grid_x, i.grid_y
        gp = self._in_image(gray, torch.uint8, "gray", (h, w))
        cp = self._out_array(cells, torch.uint8, "cells", gy * gx * 32)
        fp = self._out_image(field, torch.float32, "field", (gy, gx, 2))
        vp = self._out_image(vis, torch.uint8, "vis", (h, w, 3))
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_piv_push_dev(self._h, stream, *gp, cp, *fp, *vp, up))

    def piv_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX PIV_CELL_DTYPE, dict of the summary by PIV_SUMMARY names) of the last
        push that computed them; zeros before that."""
        info = self.piv_info(stream)
        cells = np.zeros((info["grid_y"], info["grid_x"]), PIV_CELL_DTYPE)
        return cells, self._summary(self._lib.rcflow_piv_read, stream, PIV_SUMMARY, cells.ctypes.data)

    def piv_sums(self, stream=0):
        """Waits for the slot's stream -> (the accumulators GYxGXxDxDx3 int64: Tab, Tb, Tbb per displacement; GYxGXx2 int64: Ta,
        Taa); for tests."""
        info = self.piv_info(stream)
        gx, gy, D = info["grid_x"], info["grid_y"], 2 * info["range"] + 1
        sums, cell = np.empty((gy, gx, D, D, 3), np.int64), np.empty((gy, gx, 2), np.int64)
        self._bind(stream)
        check(self._lib.rcflow_piv_sums_read(self._h, stream, sums.ctypes.data, cell.ctypes.data))
        return sums, cell

    def piv_set(self, min_peak, median_eps, median_thr, vis_max, stream=0):
        """min_peak, median_eps, median_thr and vis_max from the next push on."""
        check(self._lib.rcflow_piv_set(self._h, stream, float(min_peak), float(median_eps), float(median_thr), float(vis_max)))

    def piv_reset(self, stream=0):
        self._lifecycle("piv", "reset", stream)

    def piv_close(self, stream=0):
        self._lifecycle("piv", "close", stream)

    # ------------------------------------------------------------------ transects
    def transects_open(self, w, h, lines, window=256, gray=True, flow=True, lag=1, range=0, fps=1.0, metres_per_pixel=1.0, jet_min=0.25,
                       vis_max=2.0, stream=0):
        """Opens the slot's transects on w x h frames (include/rcflow.h, "transects"): `lines` is a sequence of (x0, y0, x1, y1, n),
        straight lines in pixels with n samples each; the last `window` rows are held, of the grey frame (gray), of the field's
        components along and across each line (flow) or of both.  range >= 1 correlates every grey row with the one `lag` pushes
        later over +-range samples, for the drift along the line.  The rings take window * samples * (1 + 8) bytes."""
        arr = _transect_lines(lines)
        p = TransectsParams(window=int(window), sources=(RC_TRANSECTS_GRAY if gray else 0) | (RC_TRANSECTS_FLOW if flow else 0), lag=int(lag),
                            range=int(range), flags=0, pad=0, fps=float(fps), metres_per_pixel=float(metres_per_pixel), jet_min=float(jet_min),
                            vis_max=float(vis_max))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_transects_open(self._h, stream, int(w), int(h), arr, len(arr), C.byref(p)))

    def transects_info(self, stream=0):
        """dict(w, h, the parameters, gray, flow, lines, samples, launches_per_push, held, pairs, pushes, device_bytes); never blocks."""
        i = self._info("transects", TransectsInfo(), stream)
        d = _record(i, skip=("flags", "pad", "sources"))
        d["gray"], d["flow"] = bool(i.prm.sources & RC_TRANSECTS_GRAY), bool(i.prm.sources & RC_TRANSECTS_FLOW)
        return d

    def transects_push(self, gray=None, flow=None, records=None, sums=None, profile=None, stack=None, hov=None, summary=None, stream=0):
        """One frame: gray (HxW uint8 device tensor) and / or flow (HxWx2 float32), exactly what was opened, rows may be padded;
        nothing is synchronised.  Outputs are preallocated device tensors, each optional: records LINESx64 uint8 (rc_transect
        records; view the host copy as TRANSECT_DTYPE), sums LINESx16 int64 (TRANSECTS_SUMS), profile SAMPLESx2 float32 (the window
        means along and across), stack WINDOWxSAMPLES uint8 (the time stack, oldest row first), hov WINDOWxSAMPLESx3 uint8 (the
        cross-line velocity against time), summary 8 int64 (TRANSECTS_SUMMARY).  Without any output the push is one launch."""
        i = self._info("transects", TransectsInfo(), stream)
        h, w, L, S, T = i.h, i.w, i.lines, i.samples, i.prm.window
        gp = self._in_image(gray, torch.uint8, "gray", (h, w), optional=True)
        fp = self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True)
        rp = self._out_array(records, torch.uint8, "records", L * 64)
        sp = self._out_array(sums, torch.int64, "sums", L * RC_TRANSECTS_SUMS)
        pp = self._out_array(profile, torch.float32, "profile", S * 2)
        kp = self._out_image(stack, torch.uint8, "stack", (T, S))
        hp = self._out_image(hov, torch.uint8, "hov", (T, S, 3))
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_transects_push_dev(self._h, stream, *gp, *fp, rp, sp, pp, *kp, *hp, up))

    def transects_read(self, stream=0):
        """Waits for the slot's stream -> (records LINES TRANSECT_DTYPE, dict of the summary by TRANSECTS_SUMMARY names) of the
        last push that computed them; zeros before that."""
        rec = np.zeros(self.transects_info(stream)["lines"], TRANSECT_DTYPE)
        return rec, self._summary(self._lib.rcflow_transects_read, stream, TRANSECTS_SUMMARY, rec.ctypes.data)

    def transects_sums(self, stream=0):
        """Waits for the slot's stream -> (the accumulators LINESx(2 range + 1)x3 int64: Tab, Tb, Tbb per shift; LINESx2 int64:
        Ta, Taa); for tests."""
        info = self.transects_info(stream)
        sums, line = np.empty((info["lines"], 2 * info["range"] + 1, 3), np.int64), np.empty((info["lines"], 2), np.int64)
        self._bind(stream)
        check(self._lib.rcflow_transects_sums_read(self._h, stream, sums.ctypes.data, line.ctypes.data))
        return sums, line

    def transects_table(self, stream=0):
        """Waits -> (SAMPLES TRANSECT_SAMPLE_DTYPE, LINES TRANSECT_GEOM_DTYPE): the open session's table, from the device."""
        info = self.transects_info(stream)
        table, geom = np.zeros(info["samples"], TRANSECT_SAMPLE_DTYPE), np.zeros(info["lines"], TRANSECT_GEOM_DTYPE)
        self._bind(stream)
        check(self._lib.rcflow_transects_table_read(self._h, stream, table.ctypes.data, geom.ctypes.data))
        return table, geom

    def transects_set(self, jet_min, vis_max, stream=0):
        """jet_min and vis_max from the next push on."""
        check(self._lib.rcflow_transects_set(self._h, stream, float(jet_min), float(vis_max)))

    def transects_reset(self, stream=0):
        self._lifecycle("transects", "reset", stream)

    def transects_close(self, stream=0):
        self._lifecycle("transects", "close", stream)

    # ------------------------------------------------------------------ flow kinematics
    def kinematics_open(self, w, h, radius=2, sigma=1.5, spacing=1, grid_x=1, grid_y=1, scale=1.0, pixel_area=1.0, ow_k=0.2, ow_min=0.0,
                        omega_min=0.0, min_core=1, vis_max=0.5, relative=True, stream=0):
        """Opens the slot's flow kinematics for w x h flow fields (include/rcflow.h, "flow kinematics"): the field smoothed with
        Gaussian taps of half-width `radius`, central differences at +-spacing times `scale` (frames per second for a pixel field),
        vorticity (positive: clockwise on the picture), divergence and the Okubo-Weiss parameter, the vortex cores (ow below
        -ow_k standard deviations of ow with relative=True, else below -ow_min; |omega| at least omega_min) and a record per cell
        of a grid_x x grid_y grid.  The state takes 8 bytes per pixel of device memory."""
        p = KinematicsParams(radius=int(radius), spacing=int(spacing), grid_x=int(grid_x), grid_y=int(grid_y), min_core=int(min_core),
                             flags=RC_KINEMATICS_RELATIVE if relative else 0, sigma=float(sigma), scale=float(scale),
                             pixel_area=float(pixel_area), ow_k=float(ow_k), ow_min=float(ow_min), omega_min=float(omega_min),
                             vis_max=float(vis_max))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_kinematics_open(self._h, stream, int(w), int(h), C.byref(p)))

    def kinematics_info(self, stream=0):
        """dict(w, h, the parameters, relative, margin, launches_per_push, pushes, device_bytes); never blocks."""
        i = self._info("kinematics", KinematicsInfo(), stream)
        d = _record(i, skip=("flags", "pad"))
        d["relative"] = bool(i.prm.flags & RC_KINEMATICS_RELATIVE)
        return d

    def kinematics_push(self, flow, omega=None, div=None, ow=None, mask=None, vis=None, cells=None, sums=None, summary=None, stream=0):
        """One flow field (HxWx2 float32 device tensor, dense pixels, rows may be padded); nothing is synchronised.  Outputs are
        preallocated device tensors, each optional: omega, div and ow HxW float32, mask HxW uint8 (255 at a vortex core: what
        regions_push takes), vis HxWx3 uint8, cells GYxGXx48 uint8 (rc_kinematics_cell records; view the host copy as
        KINEMATICS_CELL_DTYPE), sums GYxGXx11 int64 (KINEMATICS_SUMS), summary 8 int64 (KINEMATICS_SUMMARY).  Without any output
        the push only counts; with any it is RC_KINEMATICS_LAUNCHES.  Records, sums and summary also stay on the slot for
        kinematics_read."""
        i = self._info("kinematics", KinematicsInfo(), stream)
        h, w, nc = i.h, i.w, i.prm.grid_x * i.prm.grid_y
        fp, fstep = self._in_image(flow, torch.float32, "flow", (h, w, 2))
        images = (self._out_image(omega, torch.float32, "omega", (h, w)) + self._out_image(div, torch.float32, "div", (h, w)) +
                  self._out_image(ow, torch.float32, "ow", (h, w)) + self._out_image(mask, torch.uint8, "mask", (h, w)) +
                  self._out_image(vis, torch.uint8, "vis", (h, w, 3)))
        cp = self._out_array(cells, torch.uint8, "cells", nc * 48)
        sp = self._out_array(sums, torch.int64, "sums", nc * RC_KINEMATICS_SUMS)
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_kinematics_push_dev(self._h, stream, fp, fstep, *images, cp, sp, up))

    def kinematics_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX KINEMATICS_CELL_DTYPE, sums GYxGXx11 int64, dict of the summary by
        KINEMATICS_SUMMARY names, with t2: the squared threshold, and max_omega: the largest |omega| as a float) of the last push
        that had an output; zeros before that."""
        info = self.kinematics_info(stream)
        gx, gy = info["grid_x"], info["grid_y"]
        cells, sums = np.zeros((gy, gx), KINEMATICS_CELL_DTYPE), np.zeros((gy, gx, RC_KINEMATICS_SUMS), np.int64)
        out = self._summary(self._lib.rcflow_kinematics_read, stream, KINEMATICS_SUMMARY, cells.ctypes.data, sums.ctypes.data,
                            bits=("max_omega_bits", "max_omega", float))
        out["t2"] = float(np.array([out["t2_bits"]], np.int64).view(np.float64)[0])
        return cells, sums, out

    def kinematics_set(self, ow_k, ow_min, omega_min, vis_max, stream=0):
        """ow_k, ow_min, omega_min and vis_max from the next push on."""
        check(self._lib.rcflow_kinematics_set(self._h, stream, float(ow_k), float(ow_min), float(omega_min), float(vis_max)))

    def kinematics_reset(self, stream=0):
        self._lifecycle("kinematics", "reset", stream)

    def kinematics_close(self, stream=0):
        self._lifecycle("kinematics", "close", stream)

    # ------------------------------------------------------------------ shoreline
    def shoreline_open(self, w, h, lines, source="rmb", radius=2, wet_is_high=0, threshold=-1, window=512, permille=20, min_sep=0.0,
                       max_jump=8.0, metres_per_pixel=1.0, stream=0):
        """Opens the slot's shoreline on w x h pictures (include/rcflow.h, "shoreline"): `lines` is a sequence of (x0, y0, x1, y1, n),
        straight lines in pixels FROM LAND TO SEA with n samples each, listed in alongshore order.  source: "rmb" (R - B + 255 of a
        BGR picture), "gray", or "plane" (an HxW uint8 indicator of the caller's); the indicator is smoothed by a box of half-width
        `radius` and split at Otsu's threshold (threshold=-1) or a fixed one; the last `window` positions of every line are held
        for the runup statistics.  The state takes 2 bytes per pixel and 4 * window bytes per line of device memory."""
        arr = _transect_lines(lines)
        p = ShorelineParams(source=SHORE_SOURCES[source], radius=int(radius), wet_is_high=int(wet_is_high), threshold=int(threshold),
                            window=int(window), permille=int(permille), flags=0, pad=0, min_sep=float(min_sep), max_jump=float(max_jump),
                            metres_per_pixel=float(metres_per_pixel))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_shoreline_open(self._h, stream, int(w), int(h), arr, len(arr), C.byref(p)))

    def shoreline_info(self, stream=0):
        """dict(w, h, the parameters, source by name, lines, samples, launches_per_push, held, pushes, device_bytes); never blocks."""
        i = self._info("shoreline", ShorelineInfo(), stream)
        d = _record(i, skip=("flags", "pad"))
        d["source"] = SHORE_SOURCE_NAMES[i.prm.source]
        return d

    def shoreline_push(self, image, roi=None, records=None, mask=None, plane=None, hist=None, summary=None, stream=0):
        """One picture: HxWx3 uint8 (HxW for the "plane" source) device tensor, rows may be padded; roi: HxW uint8, the histogram
        counts where it is non-zero; nothing is synchronised.  Outputs are preallocated device tensors, each optional: records
        LINESx64 uint8 (rc_shoreline records; view the host copy as SHORELINE_DTYPE), mask HxW uint8 (255 where wet: what
        regions_push takes), plane HxW int16 (the smoothed indicator, 0..510), hist 512 int32, summary 8 int64 (SHORELINE_SUMMARY).
        Records and summary also stay on the slot for shoreline_read."""
        i = self._info("shoreline", ShorelineInfo(), stream)
        h, w, ch = i.h, i.w, 1 if i.prm.source == SHORE_SOURCES["plane"] else 3
        if not _is_t(image) or image.dim() != (2 if ch == 1 else 3):
            raise ValueError("image must be an %s uint8 device tensor, as opened" % ("HxW" if ch == 1 else "HxWx3"))
        ip = self._in_image(image, torch.uint8, "image", (h, w) if ch == 1 else (h, w, 3))
        qp = self._in_image(roi, torch.uint8, "roi", (h, w), optional=True)
        rp = self._out_array(records, torch.uint8, "records", i.lines * 64)
        mp = self._out_image(mask, torch.uint8, "mask", (h, w))
        pp = self._out_image(plane, torch.int16, "plane", (h, w))
        hp = self._out_array(hist, torch.int32, "hist", RC_SHORE_HIST)
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_shoreline_push_dev(self._h, stream, *ip, ch, *qp, rp, *mp, *pp, hp, up))

    def shoreline_prims(self, color=0x00ffff, thickness=1, disc_radius=2, out=None, stream=0):
        """The waterline of the last push as 2 * lines - 1 primitives for draw() -> a device uint8 tensor of rc_draw_prim records:
        a disc per line with a position that is no outlier and a segment to the next such line; kind 0 elsewhere."""
        out = self._prims_out(out, 2 * self.shoreline_info(stream)["lines"] - 1)
        self._bind(stream)
        check(self._lib.rcflow_shoreline_prims_dev(self._h, stream, int(color), int(thickness), int(disc_radius), self._ptr(out)))
        return out

    def shoreline_read(self, stream=0):
        """Waits for the slot's stream -> (records LINES SHORELINE_DTYPE, dict of the summary by SHORELINE_SUMMARY names, with eta:
        Otsu's separability as a float) of the last push; zeros before the first."""
        rec = np.zeros(self.shoreline_info(stream)["lines"], SHORELINE_DTYPE)
        out = self._summary(self._lib.rcflow_shoreline_read, stream, SHORELINE_SUMMARY, rec.ctypes.data)
        out["eta"] = out["eta_q32"] / 4294967296.0
        return rec, out

    def shoreline_ring(self, stream=0):
        """Waits -> LINESxWINDOW int32, the runup time series: per line the held positions (1/256 sample) oldest first, -1 where
        the line had none, and -1 past what is held."""
        info = self.shoreline_info(stream)
        ring = np.empty((info["lines"], info["window"]), np.int32)
        self._bind(stream)
        check(self._lib.rcflow_shoreline_ring_read(self._h, stream, ring.ctypes.data))
        return ring

    def shoreline_table(self, stream=0):
        """Waits -> (SAMPLES TRANSECT_SAMPLE_DTYPE, LINES TRANSECT_GEOM_DTYPE): the open session's table, from the device."""
        info = self.shoreline_info(stream)
        table, geom = np.zeros(info["samples"], TRANSECT_SAMPLE_DTYPE), np.zeros(info["lines"], TRANSECT_GEOM_DTYPE)
        self._bind(stream)
        check(self._lib.rcflow_shoreline_table_read(self._h, stream, table.ctypes.data, geom.ctypes.data))
        return table, geom

    def shoreline_set(self, threshold, min_sep, max_jump, stream=0):
        """threshold, min_sep and max_jump from the next push on."""
        check(self._lib.rcflow_shoreline_set(self._h, stream, int(threshold), float(min_sep), float(max_jump)))

    def shoreline_reset(self, stream=0):
        self._lifecycle("shoreline", "reset", stream)

    def shoreline_close(self, stream=0):
        self._lifecycle("shoreline", "close", stream)

    # ------------------------------------------------------------------ surf zone
    def surf_open(self, w, h, lines=(), window=256, bright=180, delta=40, q_min=100, min_run=3, span=6, ratio=500, min_load=0, min_lines=2,
                  vis_permille=500, metres_per_pixel=1.0, stream=0):
        """Opens the slot's surf zone on w x h grey frames (include/rcflow.h, "surf"): `lines` is a sequence of (x0, y0, x1, y1, n),
        straight lines in pixels FROM LAND TO SEA with n samples each, listed in alongshore order; without lines the session is
        pixels only.  A pixel breaks in a frame when it is at least `bright` and at least `delta` above its mean over the last
        `window` frames; it is in the surf zone when it broke in q_min per mille of them; a line whose load falls below `ratio` per
        mille of the lower median of the lines within `span` of it is a channel line.  The state takes about window + 10 bytes
        per pixel of device memory."""
        arr = _transect_lines(lines) if len(lines) else None
        p = SurfParams(window=int(window), bright=int(bright), delta=int(delta), q_min=int(q_min), min_run=int(min_run), span=int(span),
                       ratio=int(ratio), min_load=int(min_load), min_lines=int(min_lines), vis_permille=int(vis_permille), flags=0, pad=0,
                       metres_per_pixel=float(metres_per_pixel))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_surf_open(self._h, stream, int(w), int(h), arr, len(lines), C.byref(p)))

    def surf_info(self, stream=0):
        """dict(w, h, the parameters, lines, samples, launches_per_push, held, pushes, device_bytes); never blocks."""
        return _record(self._info("surf", SurfInfo(), stream), skip=("flags", "pad"))

    def surf_push(self, gray, now=None, surf=None, q=None, mean=None, sd=None, picture=None, lines=None, channels=None, summary=None, stream=0):
        """One grey frame: HxW uint8 device tensor, rows may be padded; nothing is synchronised.  Outputs are preallocated device
        tensors, each optional: now HxW uint8 (255 where the pixel breaks in this frame), surf HxW uint8 (255 in the surf zone: what
        regions_push takes), q HxW int16 (frames of the window in which the pixel broke), mean HxW uint8, sd HxW uint8 (twice the
        standard deviation: the variance image), picture HxWx3 uint8 (q in JET colours), lines LINESx64 uint8 (rc_surf_line
        records; view the host copy as SURF_LINE_DTYPE), channels 32x32 uint8 (rc_surf_channel; SURF_CHANNEL_DTYPE), summary 8 int64
        (SURF_SUMMARY).  Records and summary also stay on the slot for surf_read."""
        i = self._info("surf", SurfInfo(), stream)
        h, w = i.h, i.w
        if not _is_t(gray) or gray.dim() != 2:
            raise ValueError("gray must be an HxW uint8 device tensor, as opened")
        gp = self._in_image(gray, torch.uint8, "gray", (h, w))
        np_ = self._out_image(now, torch.uint8, "now", (h, w))
        sp = self._out_image(surf, torch.uint8, "surf", (h, w))
        qp = self._out_image(q, torch.int16, "q", (h, w))
        mp = self._out_image(mean, torch.uint8, "mean", (h, w))
        dp = self._out_image(sd, torch.uint8, "sd", (h, w))
        pp = self._out_image(picture, torch.uint8, "picture", (h, w, 3))
        lp = self._out_array(lines, torch.uint8, "lines", i.lines * 64)
        cp = self._out_array(channels, torch.uint8, "channels", RC_SURF_MAX_CHANNELS * 32)
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_surf_push_dev(self._h, stream, *gp, 1, *np_, *sp, *qp, *mp, *dp, *pp, lp, cp, up))

    def surf_prims(self, color=0x00ffff, thickness=1, disc_radius=3, out=None, stream=0):
        """The breaker line and the channels of the last push as lines - 1 + 32 primitives for draw() -> a device uint8 tensor of
        rc_draw_prim records: a segment from the outer edge of every line with a band to that of the next such line, a disc at
        every recorded channel's centre; kind 0 elsewhere."""
        out = self._prims_out(out, self.surf_info(stream)["lines"] - 1 + RC_SURF_MAX_CHANNELS)
        self._bind(stream)
        check(self._lib.rcflow_surf_prims_dev(self._h, stream, int(color), int(thickness), int(disc_radius), self._ptr(out)))
        return out

    def surf_read(self, stream=0):
        """Waits for the slot's stream -> (lines LINES SURF_LINE_DTYPE, channels SURF_CHANNEL_DTYPE: the recorded ones, dict of the
        summary by SURF_SUMMARY names) of the last push; zeros before the first."""
        rec = np.zeros(self.surf_info(stream)["lines"], SURF_LINE_DTYPE)
        chan = np.zeros(RC_SURF_MAX_CHANNELS, SURF_CHANNEL_DTYPE)
        out = self._summary(self._lib.rcflow_surf_read, stream, SURF_SUMMARY, rec.ctypes.data if rec.size else None, chan.ctypes.data)
        return rec, chan[:min(out["channels"], RC_SURF_MAX_CHANNELS)], out

    def surf_table(self, stream=0):
        """Waits -> (SAMPLES TRANSECT_SAMPLE_DTYPE, LINES TRANSECT_GEOM_DTYPE): the open session's table, from the device."""
        info = self.surf_info(stream)
        table, geom = np.zeros(info["samples"], TRANSECT_SAMPLE_DTYPE), np.zeros(info["lines"], TRANSECT_GEOM_DTYPE)
        self._bind(stream)
        check(self._lib.rcflow_surf_table_read(self._h, stream, table.ctypes.data if table.size else None, geom.ctypes.data if geom.size else None))
        return table, geom

    def surf_set(self, bright, delta, q_min, ratio, min_load, vis_permille, stream=0):
        """bright, delta, q_min, ratio, min_load and vis_permille from the next push on."""
        check(self._lib.rcflow_surf_set(self._h, stream, int(bright), int(delta), int(q_min), int(ratio), int(min_load), int(vis_permille)))

    def surf_reset(self, stream=0):
        self._lifecycle("surf", "reset", stream)

    def surf_close(self, stream=0):
        self._lifecycle("surf", "close", stream)

    # ------------------------------------------------------------------ mean flow
    def meanflow_open(self, w, h, window=300, grid_x=30, grid_y=30, min_fill=None, steady_min=600, opposed=False, speed_min=0.5, min_cos2=0.5,
                      dir_x=0.0, dir_y=-1.0, stream=0):
        """Opens the slot's mean current on w x h flow fields (include/rcflow.h, "mean flow"): per pixel the exact mean of the last
        `window` samples in 1/64 pixel, the steadiness |sum of vectors| / sum of magnitudes in per mille, the major and minor
        standard deviation, and a mask of the pixels with at least min_fill (default: window) valid samples that are steady
        (steady_min per mille), at least speed_min pixels per field fast and within min_cos2 of the direction (dir_x, dir_y), or
        with opposed=True of the direction against the picture's own summed mean vector.  The state takes 4 * window + 38 bytes
        per pixel of device memory."""
        p = MeanflowParams(window=int(window), grid_x=int(grid_x), grid_y=int(grid_y), min_fill=int(window if min_fill is None else min_fill),
                           steady_min=int(steady_min), flags=RC_MEANFLOW_DIR_OPPOSED if opposed else RC_MEANFLOW_DIR_FIXED,
                           speed_min=float(speed_min), min_cos2=float(min_cos2), dir_x=float(dir_x), dir_y=float(dir_y))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_meanflow_open(self._h, stream, int(w), int(h), C.byref(p)))

    def meanflow_info(self, stream=0):
        """dict(w, h, the parameters, opposed, launches_per_push, held, pushes, device_bytes); never blocks."""
        i = self._info("meanflow", MeanflowInfo(), stream)
        d = _record(i, skip=("flags", "pad"))
        d["opposed"] = i.prm.flags == RC_MEANFLOW_DIR_OPPOSED
        return d

    def meanflow_push(self, flow=None, mean=None, steady=None, std=None, mask=None, picture=None, cells=None, sums=None, summary=None, stream=0):
        """One flow field (HxWx2 float32 device tensor, dense pixels, rows may be padded; None: the field push_frame_host /
        frame_loop_step left on the slot); nothing is synchronised.  Outputs are preallocated device tensors, each optional: mean
        HxWx2 float32 (the field every flow consumer takes), steady HxW int16 (per mille), std HxWx2 float32 (major, minor), mask
        HxW uint8 (255 in a steady jet: what regions_push takes), picture HxWx3 uint8 (the steadiness in JET colours), cells
        GYxGXx32 uint8 (rc_meanflow_cell records; view the host copy as MEANFLOW_CELL_DTYPE), sums GYxGXx8 int64 (MEANFLOW_SUMS),
        summary 8 int64 (MEANFLOW_SUMMARY).  Records, sums and summary also stay on the slot for meanflow_read."""
        i = self._info("meanflow", MeanflowInfo(), stream)
        h, w, nc = i.h, i.w, i.prm.grid_x * i.prm.grid_y
        fp, fstep = self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True)
        images = (self._out_image(mean, torch.float32, "mean", (h, w, 2)) + self._out_image(steady, torch.int16, "steady", (h, w)) +
                  self._out_image(std, torch.float32, "std", (h, w, 2)) + self._out_image(mask, torch.uint8, "mask", (h, w)) +
                  self._out_image(picture, torch.uint8, "picture", (h, w, 3)))
        cp = self._out_array(cells, torch.uint8, "cells", nc * 32)
        sp = self._out_array(sums, torch.int64, "sums", nc * RC_MEANFLOW_SUMS)
        up = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_meanflow_push_dev(self._h, stream, fp, fstep, *images, cp, sp, up))

    def meanflow_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX MEANFLOW_CELL_DTYPE, sums GYxGXx8 int64, dict of the summary by
        MEANFLOW_SUMMARY names) of the last push; zeros before the first."""
        info = self.meanflow_info(stream)
        gx, gy = info["grid_x"], info["grid_y"]
        cells, sums = np.zeros((gy, gx), MEANFLOW_CELL_DTYPE), np.zeros((gy, gx, RC_MEANFLOW_SUMS), np.int64)
        out = self._summary(self._lib.rcflow_meanflow_read, stream, MEANFLOW_SUMMARY, cells.ctypes.data, sums.ctypes.data)
        return cells, sums, out

    def meanflow_set(self, steady_min, speed_min, min_cos2, dir_x, dir_y, min_fill, stream=0):
        """steady_min, speed_min, min_cos2, dir_x, dir_y and min_fill from the next push on."""
        check(self._lib.rcflow_meanflow_set(self._h, stream, int(steady_min), float(speed_min), float(min_cos2), float(dir_x), float(dir_y),
                                            int(min_fill)))

    def meanflow_reset(self, stream=0):
        self._lifecycle("meanflow", "reset", stream)

    def meanflow_close(self, stream=0):
        self._lifecycle("meanflow", "close", stream)

    # ------------------------------------------------------------------ flow check
    def flowcheck_open(self, w, h, radius=4, grid_x=30, grid_y=30, tests=RC_FLOWCHECK_TESTS, fill="nan", tex_min=1, gain_pm=0, res_max=1.5,
                       fb_rel=0.01, fb_abs=0.7071067811865476, speed_max=1000.0, stream=0):
        """Opens the slot's flow check on w x h frames and fields (include/rcflow.h, "flow check"): per pixel the residual of the
        match its vector claims, the texture of the previous frame and the round trip against a backward field, over a clipped
        (2 radius + 1)^2 window, and from them the flags (FLOWCHECK_FLAGS), the mask of the valid pixels and the field with the
        rejected vectors replaced by NaN (fill="nan") or zero (fill="zero").  tests: which of flat, resid, nogain, fb and fast run,
        as the sum of their FLOWCHECK_FLAGS."""
        if fill not in ("nan", "zero"):
            raise ValueError("fill is 'nan' or 'zero'")
        p = FlowcheckParams(radius=int(radius), grid_x=int(grid_x), grid_y=int(grid_y), tests=int(tests),
                            flags=RC_FLOWCHECK_FILL_NAN if fill == "nan" else RC_FLOWCHECK_FILL_ZERO, tex_min=int(tex_min), gain_pm=int(gain_pm),
                            res_max=float(res_max), fb_rel=float(fb_rel), fb_abs=float(fb_abs), speed_max=float(speed_max))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_flowcheck_open(self._h, stream, int(w), int(h), C.byref(p)))

    def flowcheck_info(self, stream=0):
        """dict(w, h, the parameters, fill, launches_per_push, held, pushes, computing, device_bytes); never blocks."""
        i = self._info("flowcheck", FlowcheckInfo(), stream)
        d = _record(i, skip=("flags", "pad"))
        d["fill"] = "nan" if i.prm.flags == RC_FLOWCHECK_FILL_NAN else "zero"
        return d

    def flowcheck_push(self, next, prev=None, flow=None, back=None, flags=None, mask=None, checked=None, resid=None, texture=None, picture=None,
                       cells=None, sums=None, summary=None, stream=0):
        """One pair of grey frames (HxW uint8 device tensors; prev None: the frame of the push before, which the slot holds) and
        the field from prev to next (HxWx2 float32, dense pixels, rows may be padded; None: the field push_frame_host /
        frame_loop_step left on the slot); back: the field from next to prev for the round-trip test, or None.  Nothing is
        synchronised.  Outputs are preallocated device tensors, each optional: flags and mask HxW uint8 (mask: 255 where valid, what
        regions_push takes), checked HxWx2 float32 (what meanflow_push, ripmap_push and kinematics_push take), resid HxWx2 float32
        (window-mean residual with the flow and with no motion, grey levels), texture HxW float32, picture HxWx3 uint8, cells
        GYxGXx32 uint8 (rc_flowcheck_cell records; view the host copy as FLOWCHECK_CELL_DTYPE), sums GYxGXx10 int64
        (FLOWCHECK_SUMS), summary 10 int64 (FLOWCHECK_SUMMARY).  Records, sums and summary also stay on the slot for
        flowcheck_read.  The first push after the open with prev None only stores its frame."""
        i = self._info("flowcheck", FlowcheckInfo(), stream)
        h, w, nc = i.h, i.w, i.prm.grid_x * i.prm.grid_y
        ins = (self._in_image(next, torch.uint8, "next", (h, w)) + self._in_image(prev, torch.uint8, "prev", (h, w), optional=True) +
               self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True) + self._in_image(back, torch.float32, "back", (h, w, 2), optional=True))
        images = (self._out_image(flags, torch.uint8, "flags", (h, w)) + self._out_image(mask, torch.uint8, "mask", (h, w)) +
                  self._out_image(checked, torch.float32, "checked", (h, w, 2)) + self._out_image(resid, torch.float32, "resid", (h, w, 2)) +
                  self._out_image(texture, torch.float32, "texture", (h, w)) + self._out_image(picture, torch.uint8, "picture", (h, w, 3)))
        cp = self._out_array(cells, torch.uint8, "cells", nc * 32)
        sp = self._out_array(sums, torch.int64, "sums", nc * RC_FLOWCHECK_SUMS)
        up = self._out_array(summary, torch.int64, "summary", RC_FLOWCHECK_SUMMARY)
        self._bind(stream)
        check(self._lib.rcflow_flowcheck_push_dev(self._h, stream, *ins, *images, cp, sp, up))

    def flowcheck_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX FLOWCHECK_CELL_DTYPE, sums GYxGXx10 int64, dict of the summary by
        FLOWCHECK_SUMMARY names) of the last computing push; zeros before the first."""
        info = self.flowcheck_info(stream)
        gx, gy = info["grid_x"], info["grid_y"]
        cells, sums = np.zeros((gy, gx), FLOWCHECK_CELL_DTYPE), np.zeros((gy, gx, RC_FLOWCHECK_SUMS), np.int64)
        summ = np.zeros(RC_FLOWCHECK_SUMMARY, np.int64)
        self._bind(stream)
        check(self._lib.rcflow_flowcheck_read(self._h, stream, cells.ctypes.data, sums.ctypes.data, summ.ctypes.data_as(C.POINTER(C.c_longlong))))
        return cells, sums, dict(zip(FLOWCHECK_SUMMARY, (int(v) for v in summ)))

    def flowcheck_set(self, tests, tex_min, res_max, gain_pm, fb_rel, fb_abs, speed_max, stream=0):
        """tests, tex_min, res_max, gain_pm, fb_rel, fb_abs and speed_max from the next push on."""
        check(self._lib.rcflow_flowcheck_set(self._h, stream, int(tests), int(tex_min), float(res_max), int(gain_pm), float(fb_rel), float(fb_abs),
                                             float(speed_max)))

    def flowcheck_reset(self, stream=0):
        self._lifecycle("flowcheck", "reset", stream)

    def flowcheck_close(self, stream=0):
        self._lifecycle("flowcheck", "close", stream)

    # ------------------------------------------------------------------ drifters
    def drifters_open(self, w, h, max_drifters=1 << 16, grid_x=30, grid_y=30, dt=1.0, max_age=0, age_bin=8, density_full=16, live_min=1,
                      respawn=False, stream=0):
        """Opens the slot's virtual drifters on w x h flow fields (include/rcflow.h, "drifters"): up to max_drifters points that
        every push moves dt fields through the field in exact integers, until they die by a fate (an edge, a bad vector, max_age
        pushes, a zone of the push's byte map); with respawn=True the dead are released again at their homes.  Keeps the visit
        density, the census by place and by origin on a grid_x x grid_y grid, and residence-time histograms of age_bin pushes a
        bin.  The state takes 24 bytes a drifter and 8 a pixel of device memory."""
        p = DriftersParams(max_drifters=int(max_drifters), grid_x=int(grid_x), grid_y=int(grid_y), max_age=int(max_age), age_bin=int(age_bin),
                           density_full=int(density_full), live_min=int(live_min), flags=RC_DRIFTERS_RESPAWN if respawn else 0, dt=float(dt))
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_drifters_open(self._h, stream, int(w), int(h), C.byref(p)))

    def drifters_info(self, stream=0):
        """dict(w, h, the parameters, respawn, launches_per_push, drifters, pushes, device_bytes); never blocks."""
        i = self._info("drifters", DriftersInfo(), stream)
        d = _record(i, skip=("flags",))
        d["respawn"] = bool(i.prm.flags & RC_DRIFTERS_RESPAWN)
        return d

    def drifters_seed(self, xy, stream=0):
        """Appends the host points xy (N x 2, pixels) as waiting drifters; they are released at these homes by the next push.
        Blocks."""
        pts = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        self._bind(stream)
        check(self._lib.rcflow_drifters_seed(self._h, stream, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0]))

    def drifters_push(self, flow=None, zone=None, now=None, density=None, live=None, picture=None, xy=None, age=None, state=None, cells=None,
                      place=None, origin=None, hist=None, summary=None, stream=0):
        """One flow field (HxWx2 float32 device tensor, dense pixels, rows may be padded; None: the field push_frame_host /
        frame_loop_step left on the slot) and the zones (HxW uint8: 1 shore, 2 offshore, up to 7; None: no zone; drifters_zones
        makes it); nothing is synchronised.  Outputs are preallocated device tensors, each optional: now HxW int16 (this push's
        occupancy, saturated, as uint16 bits), density HxW int32 (uint32 bits), live HxW uint8 (255 where at least live_min
        drifters are: what regions_push takes), picture HxWx3 uint8 (the density in JET colours); per drifter xy Nx2 float32, age
        N int32, state N uint8 (0 alive, 255 waiting, else the fate); cells GYxGXx32 uint8 (rc_drifters_cell records; view the
        host copy as DRIFTERS_CELL_DTYPE), place and origin GYxGXx8 int64 (DRIFTERS_PLACE, DRIFTERS_ORIGIN), hist 4x32 int64
        (uint64 bits), summary 24 int64 (DRIFTERS_SUMMARY).  All of the last five also stay on the slot for drifters_read."""
        i = self._info("drifters", DriftersInfo(), stream)
        h, w, nc, n = i.h, i.w, i.prm.grid_x * i.prm.grid_y, i.drifters
        ins = self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True) + self._in_image(zone, torch.uint8, "zone", (h, w), optional=True)
        images = (self._out_image(now, torch.int16, "now", (h, w)) + self._out_image(density, torch.int32, "density", (h, w)) +
                  self._out_image(live, torch.uint8, "live", (h, w)) + self._out_image(picture, torch.uint8, "picture", (h, w, 3)))
        arrays = (self._out_array(xy, torch.float32, "xy", 2 * n), self._out_array(age, torch.int32, "age", n),
                  self._out_array(state, torch.uint8, "state", n), self._out_array(cells, torch.uint8, "cells", nc * 32),
                  self._out_array(place, torch.int64, "place", nc * RC_DRIFTERS_SUMS), self._out_array(origin, torch.int64, "origin", nc * RC_DRIFTERS_SUMS),
                  self._out_array(hist, torch.int64, "hist", 4 * RC_DRIFTERS_HIST_BINS), self._out_array(summary, torch.int64, "summary", RC_DRIFTERS_SUMMARY))
        self._bind(stream)
        check(self._lib.rcflow_drifters_push_dev(self._h, stream, *ins, *images, *arrays))

    def drifters_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX DRIFTERS_CELL_DTYPE, place GYxGXx8 int64, origin GYxGXx8 int64, hist 4x32
        uint64, dict of the summary by DRIFTERS_SUMMARY names): the records and the summary of the last push, zeros before the
        first; the tables and the histograms as they stand."""
        info = self.drifters_info(stream)
        gx, gy = info["grid_x"], info["grid_y"]
        cells = np.zeros((gy, gx), DRIFTERS_CELL_DTYPE)
        place, origin = np.zeros((gy, gx, RC_DRIFTERS_SUMS), np.int64), np.zeros((gy, gx, RC_DRIFTERS_SUMS), np.int64)
        hist, summ = np.zeros((4, RC_DRIFTERS_HIST_BINS), np.uint64), np.zeros(RC_DRIFTERS_SUMMARY, np.int64)
        self._bind(stream)
        check(self._lib.rcflow_drifters_read(self._h, stream, cells.ctypes.data, place.ctypes.data, origin.ctypes.data, hist.ctypes.data,
                                             summ.ctypes.data_as(C.POINTER(C.c_longlong))))
        return cells, place, origin, hist, dict(zip(DRIFTERS_SUMMARY, (int(v) for v in summ)))

    def drifters_set(self, dt, max_age, density_full, live_min, respawn, stream=0):
        """dt, max_age, density_full, live_min and respawn from the next push on."""
        check(self._lib.rcflow_drifters_set(self._h, stream, float(dt), int(max_age), int(density_full), int(live_min),
                                            RC_DRIFTERS_RESPAWN if respawn else 0))

    def drifters_reset(self, stream=0):
        self._lifecycle("drifters", "reset", stream)

    def drifters_close(self, stream=0):
        self._lifecycle("drifters", "close", stream)

    def drifters_zones(self, wet=None, inside=None, out=None, stream=0):
        """The zones a push takes from the shoreline's wet mask and the surf zone's mask (HxW uint8 device tensors, either may be
        None, not both): 1 (shore) where wet is 0, else 2 (offshore) where inside is 0, else 0 -> HxW uint8; one launch, nothing
        is synchronised."""
        src = wet if wet is not None else inside
        if src is None:
            raise ValueError("wet and inside are both None")
        h, w = int(src.shape[0]), int(src.shape[1])
        ins = self._in_image(wet, torch.uint8, "wet", (h, w), optional=True) + self._in_image(inside, torch.uint8, "inside", (h, w), optional=True)
        out = self._out_or_new(out, torch.uint8, "out", (h, w), dense=True)
        self._bind(stream)
        check(self._lib.rcflow_drifters_zones_dev(self._h, stream, *ins, w, h, self._ptr(out), out.stride(0)))
        return out

    # ------------------------------------------------------------------ flow infill
    def infill_open(self, w, h, levels=7, min_known=1, hold=0, grid_x=30, grid_y=30, leave="nan", stream=0):
        """Opens the slot's flow infill on w x h fields (include/rcflow.h, "flow infill"): the vectors that are not finite or that
        the valid mask rejects are replaced by a mix of their valid neighbours, taken from a pyramid of `levels` levels of block
        sums; a cell of the pyramid with at least min_known known pixels takes its own mean.  hold: the pushes a pixel keeps its
        last known vector before it counts as a hole.  leave: what a pixel without a value gets, "nan" or "zero"."""
        if leave not in ("nan", "zero"):
            raise ValueError("leave is 'nan' or 'zero'")
        p = InfillParams(levels=int(levels), min_known=int(min_known), hold=int(hold), grid_x=int(grid_x), grid_y=int(grid_y),
                         flags=RC_INFILL_LEAVE_NAN if leave == "nan" else RC_INFILL_LEAVE_ZERO)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_infill_open(self._h, stream, int(w), int(h), C.byref(p)))

    def infill_info(self, stream=0):
        """dict(w, h, the parameters, leave, launches_per_push, pushes, device_bytes); never blocks."""
        i = self._info("infill", InfillInfo(), stream)
        d = _record(i, skip=("flags", "pad"))
        d["leave"] = "nan" if i.prm.flags == RC_INFILL_LEAVE_NAN else "zero"
        return d

    def infill_push(self, flow=None, valid=None, domain=None, filled=None, source=None, mask=None, picture=None, cells=None, sums=None,
                    summary=None, stream=0):
        """One field (HxWx2 float32 device tensor, dense pixels, rows may be padded; None: the field push_frame_host /
        frame_loop_step left on the slot), the mask of its valid vectors (HxW uint8, what flowcheck_push writes as mask; None: every
        finite vector is valid) and the domain a value is wanted in (HxW uint8; None: everywhere).  Nothing is synchronised.
        Outputs are preallocated device tensors, each optional: filled HxWx2 float32 (what ftle_push, drifters_push and
        planview_push take), source HxW uint8 (0 known, 1..7 the level a value came from, INFILL_SOURCES), mask HxW uint8 (255
        where the pixel has a value, what regions_push takes), picture HxWx3 uint8, cells GYxGXx32 uint8 (rc_infill_cell records;
        view the host copy as INFILL_CELL_DTYPE), sums GYxGXx8 int64 (INFILL_SUMS), summary 16 int64 (INFILL_SUMMARY).  Records,
        sums and summary also stay on the slot for infill_read."""
        i = self._info("infill", InfillInfo(), stream)
        h, w, nc = i.h, i.w, i.prm.grid_x * i.prm.grid_y
        ins = (self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True) + self._in_image(valid, torch.uint8, "valid", (h, w), optional=True) +
               self._in_image(domain, torch.uint8, "domain", (h, w), optional=True))
        images = (self._out_image(filled, torch.float32, "filled", (h, w, 2)) + self._out_image(source, torch.uint8, "source", (h, w)) +
                  self._out_image(mask, torch.uint8, "mask", (h, w)) + self._out_image(picture, torch.uint8, "picture", (h, w, 3)))
        cp = self._out_array(cells, torch.uint8, "cells", nc * 32)
        sp = self._out_array(sums, torch.int64, "sums", nc * RC_INFILL_SUMS)
        up = self._out_array(summary, torch.int64, "summary", RC_INFILL_SUMMARY)
        self._bind(stream)
        check(self._lib.rcflow_infill_push_dev(self._h, stream, *ins, *images, cp, sp, up))

    def infill_read(self, stream=0):
        """Waits for the slot's stream -> (cells GYxGX INFILL_CELL_DTYPE, sums GYxGXx8 int64, dict of the summary by
        INFILL_SUMMARY names) of the last push; zeros before the first and after a reset."""
        info = self.infill_info(stream)
        gx, gy = info["grid_x"], info["grid_y"]
        cells, sums = np.zeros((gy, gx), INFILL_CELL_DTYPE), np.zeros((gy, gx, RC_INFILL_SUMS), np.int64)
        summ = np.zeros(RC_INFILL_SUMMARY, np.int64)
        self._bind(stream)
        check(self._lib.rcflow_infill_read(self._h, stream, cells.ctypes.data, sums.ctypes.data, summ.ctypes.data_as(C.POINTER(C.c_longlong))))
        return cells, sums, dict(zip(INFILL_SUMMARY, (int(v) for v in summ)))

    def infill_set(self, levels, min_known, leave, stream=0):
        """levels, min_known and leave ("nan" or "zero") from the next push on."""
        if leave not in ("nan", "zero"):
            raise ValueError("leave is 'nan' or 'zero'")
        check(self._lib.rcflow_infill_set(self._h, stream, int(levels), int(min_known), RC_INFILL_LEAVE_NAN if leave == "nan" else RC_INFILL_LEAVE_ZERO))

    def infill_reset(self, stream=0):
        self._lifecycle("infill", "reset", stream)

    def infill_close(self, stream=0):
        self._lifecycle("infill", "close", stream)

    # ------------------------------------------------------------------ offshore frame
    @staticmethod
    def _offshore_params(min_dist, max_dist, stations, bins, bin_width, min_count, rip_bins, cross_min, station):
        if station not in ("x", "y"):
            raise ValueError("station is 'x' or 'y'")
        return OffshoreParams(min_dist=int(min_dist), max_dist=int(max_dist), stations=int(stations), bins=int(bins), bin_width=int(bin_width),
                              min_count=int(min_count), rip_bins=int(rip_bins), cross_min=float(cross_min),
                              flags=RC_OFFSHORE_STATION_X if station == "x" else RC_OFFSHORE_STATION_Y)

    def offshore_open(self, w, h, min_dist=2, max_dist=200, stations=16, bins=20, bin_width=10, min_count=16, rip_bins=3, cross_min=0.25,
                      station="x", stream=0):
        """Opens the slot's offshore frame on w x h pictures (include/rcflow.h, "offshore frame"): the exact distance of every pixel
        to the shore and, per push, the flow across and along the local shore normal.  Wet pixels between min_dist and max_dist
        pixels from the shore take part; they are summed in a table of `stations` places along the beach (by the pixel's x or y:
        station "x" or "y") times `bins` rings of bin_width pixels of distance.  A bin passes with at least min_count pixels and a
        mean cross flow of at least cross_min pixels per field; rip_bins passing bins in a row from the shore out flag a station."""
        p = self._offshore_params(min_dist, max_dist, stations, bins, bin_width, min_count, rip_bins, cross_min, station)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the calls will run on
        check(self._lib.rcflow_offshore_open(self._h, stream, int(w), int(h), C.byref(p)))

    def offshore_info(self, stream=0):
        """dict(w, h, the parameters, station, launches_per_map, launches_per_push, have_map, maps, pushes, device_bytes); never blocks."""
        i = self._info("offshore", OffshoreInfo(), stream)
        d = _record(i, skip=("flags", "pad"))
        d["station"] = "x" if i.prm.flags == RC_OFFSHORE_STATION_X else "y"
        return d

    def offshore_map(self, wet, dist2=None, near=None, sdist=None, picture=None, summary=None, stream=0):
        """The map, when the shore has moved: wet HxW uint8 device tensor (non-zero is water: what shoreline_push writes as mask; rows
        may be padded).  Nothing is synchronised.  Outputs are preallocated device tensors, each optional: dist2 HxW int32 (the
        squared distance to the nearest pixel of the other class, negated on land), near HxW int32 (that pixel's raster index), sdist
        HxW int32 (the distance in 1/64 pixel, negated on land), picture HxWx3 uint8, summary 8 int64 (OFFSHORE_MAP_SUMMARY).  The
        map stays on the slot for offshore_push and offshore_band, the summary for offshore_read."""
        i = self._info("offshore", OffshoreInfo(), stream)
        h, w = i.h, i.w
        args = (self._in_image(wet, torch.uint8, "wet", (h, w)) + self._out_image(dist2, torch.int32, "dist2", (h, w)) +
                self._out_image(near, torch.int32, "near", (h, w)) + self._out_image(sdist, torch.int32, "sdist", (h, w)) +
                self._out_image(picture, torch.uint8, "picture", (h, w, 3)))
        up = self._out_array(summary, torch.int64, "summary", RC_OFFSHORE_SUMMARY)
        self._bind(stream)
        check(self._lib.rcflow_offshore_map_dev(self._h, stream, *args, up))

    def offshore_push(self, flow=None, cross_along=None, cls=None, mask=None, picture=None, stations=None, table=None, summary=None, stream=0):
        """One field (HxWx2 float32 device tensor, dense pixels, rows may be padded; None: the field push_frame_host /
        frame_loop_step left on the slot) on the slot's map.  Nothing is synchronised.  Outputs are preallocated device tensors, each
        optional: cross_along HxWx2 float32 (the flow away from the shore and along it, NaN where the pixel takes no part), cls HxW
        uint8 (OFFSHORE_CLASSES), mask HxW uint8 (255 where the cross flow reaches cross_min: what regions_push takes), picture
        HxWx3 uint8, stations STATIONSx48 uint8 (rc_offshore_station records; view the host copy as OFFSHORE_STATION_DTYPE), table
        STATIONSxBINSx4 int64 (OFFSHORE_SUMS), summary 8 int64 (OFFSHORE_PUSH_SUMMARY).  Records, table and summary also stay on the
        slot for offshore_read."""
        i = self._info("offshore", OffshoreInfo(), stream)
        h, w, ns, nb = i.h, i.w, i.prm.stations, i.prm.bins
        args = (self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True) +
                self._out_image(cross_along, torch.float32, "cross_along", (h, w, 2)) + self._out_image(cls, torch.uint8, "cls", (h, w)) +
                self._out_image(mask, torch.uint8, "mask", (h, w)) + self._out_image(picture, torch.uint8, "picture", (h, w, 3)))
        rp = self._out_array(stations, torch.uint8, "stations", ns * 48)
        tp = self._out_array(table, torch.int64, "table", ns * nb * RC_OFFSHORE_SUMS)
        up = self._out_array(summary, torch.int64, "summary", RC_OFFSHORE_SUMMARY)
        self._bind(stream)
        check(self._lib.rcflow_offshore_push_dev(self._h, stream, *args, rp, tp, up))

    def offshore_band(self, lo, hi, out=None, stream=0):
        """-> HxW uint8: 255 where the pixel is wet and lo <= its distance to the shore < hi, in pixels, on the slot's map; one launch,
        nothing is synchronised.  The `inside` of drifters_zones, a domain for infill_push."""
        i = self._info("offshore", OffshoreInfo(), stream)
        out = self._out_or_new(out, torch.uint8, "out", (i.h, i.w), dense=True)
        self._bind(stream)
        check(self._lib.rcflow_offshore_band_dev(self._h, stream, float(lo), float(hi), self._ptr(out), out.stride(0)))
        return out

    def offshore_read(self, stream=0):
        """Waits for the slot's stream -> (stations OFFSHORE_STATION_DTYPE, table STATIONSxBINSx4 int64, dict of the last push's
        summary by OFFSHORE_PUSH_SUMMARY names, dict of the last map's by OFFSHORE_MAP_SUMMARY names); zeros before the first and
        after a reset."""
        i = self._info("offshore", OffshoreInfo(), stream)
        recs = np.zeros(i.prm.stations, OFFSHORE_STATION_DTYPE)
        table = np.zeros((i.prm.stations, i.prm.bins, RC_OFFSHORE_SUMS), np.int64)
        ps, ms = np.zeros(RC_OFFSHORE_SUMMARY, np.int64), np.zeros(RC_OFFSHORE_SUMMARY, np.int64)
        self._bind(stream)
        ll = C.POINTER(C.c_longlong)
        check(self._lib.rcflow_offshore_read(self._h, stream, recs.ctypes.data, table.ctypes.data, ps.ctypes.data_as(ll), ms.ctypes.data_as(ll)))
        return (recs, table, dict(zip(OFFSHORE_PUSH_SUMMARY, (int(v) for v in ps))), dict(zip(OFFSHORE_MAP_SUMMARY, (int(v) for v in ms))))

    def offshore_set(self, min_dist, max_dist, bin_width, min_count, rip_bins, cross_min, station, stream=0):
        """Everything but stations and bins, from the next call on."""
        i = self._info("offshore", OffshoreInfo(), stream)
        p = self._offshore_params(min_dist, max_dist, i.prm.stations, i.prm.bins, bin_width, min_count, rip_bins, cross_min, station)
        check(self._lib.rcflow_offshore_set(self._h, stream, C.byref(p)))

    def offshore_reset(self, stream=0):
        self._lifecycle("offshore", "reset", stream)

    def offshore_close(self, stream=0):
        self._lifecycle("offshore", "close", stream)

    # ------------------------------------------------------------------ region outlines
    def outlines_open(self, w, h, connectivity=8, min_cracks=4, max_cracks=1 << 20, max_loops=1024, max_vertices=1 << 16, stream=0):
        """Opens the slot's boundary tracing for w x h label planes and masks (include/rcflow.h, "region outlines"): every boundary
        as an ordered polygon of lattice corners, outer boundaries and holes told apart.  Loops shorter than min_cracks pixel sides
        are dropped; the first max_loops of the rest get a record, and their vertices are stored while they fit max_vertices.  A
        picture with more than max_cracks boundary sides gives no loops and says so in the summary.  36 bytes of device memory per
        crack of max_cracks and 5 per pixel."""
        p = OutlinesParams(connectivity=int(connectivity), min_cracks=int(min_cracks), max_cracks=int(max_cracks), max_loops=int(max_loops),
                           max_vertices=int(max_vertices), flags=0)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_outlines_open(self._h, stream, int(w), int(h), C.byref(p)))

    def outlines_info(self, stream=0):
        """dict(w, h, the parameters, rounds, launches_per_push, pushes, device_bytes); never blocks."""
        return _record(self._info("outlines", OutlinesInfo(), stream), skip=("flags", "pad"))

    def outlines_set(self, min_cracks, stream=0):
        """min_cracks from the next push on."""
        check(self._lib.rcflow_outlines_set(self._h, stream, int(min_cracks)))

    def outlines_push(self, labels=None, mask=None, loops=None, verts=None, summary=None, stream=0):
        """One picture, exactly one of labels (HxW int32 device tensor: what regions_push writes as labels, the tracks' footprint) and
        mask (HxW uint8, non-zero is label 1); dense pixels, rows may be padded.  Nothing is synchronised.  Outputs are preallocated
        device tensors, each optional: loops a contiguous uint8 tensor of max_loops * 56 bytes (rc_outline_loop records; view the
        host copy as OUTLINE_LOOP_DTYPE), verts max_vertices x 2 int32 (x, y of lattice corners), summary 8 int64
        (OUTLINES_SUMMARY).  All three also stay on the slot for outlines_read / outlines_prims."""
        i = self._info("outlines", OutlinesInfo(), stream)
        h, w = i.h, i.w
        if (labels is None) == (mask is None):
            raise ValueError("exactly one of labels and mask")
        args = self._in_image(labels, torch.int32, "labels", (h, w), optional=True) + self._in_image(mask, torch.uint8, "mask", (h, w), optional=True)
        lp = self._out_array(loops, torch.uint8, "loops", i.prm.max_loops * OUTLINE_LOOP_DTYPE.itemsize)
        vp = self._out_array(verts, torch.int32, "verts", i.prm.max_vertices * 2)
        up = self._out_array(summary, torch.int64, "summary", RC_OUTLINES_SUMMARY)
        self._bind(stream)
        check(self._lib.rcflow_outlines_push_dev(self._h, stream, *args, lp, vp, up))

    def outlines_prims(self, color=0x00ffff, thickness=1, out=None, stream=0):
        """The stored vertices of the last push as max_vertices primitives for draw() -> a device uint8 tensor of rc_draw_prim records:
        per stored vertex a line to its loop's next vertex; every other slot is kind 0, which draw() skips (and counts)."""
        out = self._prims_out(out, self._info("outlines", OutlinesInfo(), stream).prm.max_vertices)
        self._bind(stream)
        check(self._lib.rcflow_outlines_prims_dev(self._h, stream, int(color), int(thickness), self._ptr(out)))
        return out

    def outlines_read(self, stream=0):
        """Waits for the slot's stream -> (the records of the last push as a numpy array of OUTLINE_LOOP_DTYPE, its stored vertices
        Nx2 int32, dict of the summary by OUTLINES_SUMMARY names).  Loop r's polygon is verts[r.offset:r.offset + r.verts] unless
        r.offset is -1."""
        i = self._info("outlines", OutlinesInfo(), stream)
        rec, verts = np.zeros(i.prm.max_loops, OUTLINE_LOOP_DTYPE), np.zeros((i.prm.max_vertices, 2), np.int32)
        n, nv = C.c_int(0), C.c_int(0)
        summ = self._summary(self._lib.rcflow_outlines_read, stream, OUTLINES_SUMMARY, rec.ctypes.data, len(rec), C.byref(n), verts.ctypes.data,
                             len(verts), C.byref(nv))
        return rec[:n.value].copy(), verts[:nv.value].copy(), summ

    def outlines_reset(self, stream=0):
        self._lifecycle("outlines", "reset", stream)

    def outlines_close(self, stream=0):
        self._lifecycle("outlines", "close", stream)

    # ------------------------------------------------------------------ rip regions
    def regions_open(self, w, h, connectivity=8, min_area=1, max_regions=1024, stream=0):
        """Opens the slot's region labelling for w x h masks: connected components (4 or 8 neighbours) numbered in raster
        order of their first pixel, those below min_area pixels dropped, the first max_regions of the rest measured
        (include/rcflow.h, "rip regions").  Labels and area scratch take 8 bytes per pixel of device memory."""
        p = RegionsParams(connectivity=int(connectivity), min_area=int(min_area), max_regions=int(max_regions), flags=0)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_regions_open(self._h, stream, int(w), int(h), C.byref(p)))

    def regions_info(self, stream=0):
        """dict of rc_regions_info; never blocks."""
        info = self._info("regions", RegionsInfo(), stream)
        return _record(info)

    def regions_set(self, min_area, stream=0):
        """min_area from the next push on."""
        check(self._lib.rcflow_regions_set(self._h, stream, int(min_area)))

    def regions_push(self, mask, flow=None, labels=None, mask_out=None, regions=None, summary=None, stream=0):
        """One mask (HxW uint8 device tensor, dense pixels, rows may be padded; non-zero is foreground): RC_REGIONS_LAUNCHES
        launches, nothing is synchronised.  flow: HxWx2 float32 (dense pixels) for the per-region flow sums, or None.
        Outputs are preallocated device tensors, each optional: labels HxW int32, mask_out HxW uint8 (255 inside a kept
        component; may be `mask` itself), regions a contiguous uint8 tensor of max_regions * 144 bytes (rc_region records,
        REGION_DTYPE), summary 8 int64.  The records and the summary also stay on the slot for regions_read / regions_prims."""
        i = self._info("regions", RegionsInfo(), stream)
        h, w = i.h, i.w
        mp, mstep = self._in_image(mask, torch.uint8, "mask", (h, w))
        if flow is not None:
            flow = self._dev(flow, torch.float32)
        fp, fstep = self._in_image(flow, torch.float32, "flow", (h, w, 2), optional=True)
        lp, lstep = self._out_image(labels, torch.int32, "labels", (h, w))
        op, ostep = self._out_image(mask_out, torch.uint8, "mask_out", (h, w))
        rp = self._out_array(regions, torch.uint8, "regions", i.max_regions * REGION_DTYPE.itemsize)
        sp = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_regions_push_dev(self._h, stream, mp, mstep, fp, fstep, lp, lstep, op, ostep, rp, sp))

    def regions_prims(self, color=0x00ffff, thickness=1, disc_radius=3, flow_scale=0.0, out=None, stream=0):
        """The records of the last push as 6 * max_regions primitives for draw() -> a device uint8 tensor of rc_draw_prim
        records: per record its box (four lines), a disc at the centroid and, with flow_scale != 0, a line along the mean
        flow times flow_scale; slots without a record are kind 0, which draw() skips (and counts)."""
        n = 6 * self.regions_info(stream)["max_regions"]
        out = self._prims_out(out, n)
        self._bind(stream)
        check(self._lib.rcflow_regions_prims_dev(self._h, stream, int(color), int(thickness), int(disc_radius), float(flow_scale),
                                                 self._ptr(out)))
        return out

    def regions_read(self, stream=0):
        """Waits for the slot's stream -> (records of the last push as a numpy array of REGION_DTYPE, dict of the summary
        with the names of REGIONS_SUMMARY)."""
        cap = self.regions_info(stream)["max_regions"]
        rec, n = np.zeros(cap, REGION_DTYPE), C.c_int(0)
        summ = self._summary(self._lib.rcflow_regions_read, stream, REGIONS_SUMMARY, rec.ctypes.data, cap, C.byref(n))
        return rec[:n.value].copy(), summ

    def regions_reset(self, stream=0):
        self._lifecycle("regions", "reset", stream)

    def regions_close(self, stream=0):
        self._lifecycle("regions", "close", stream)

    # ------------------------------------------------------------------ rip tracks
    def tracks_open(self, w, h, max_regions=1024, max_tracks=64, min_overlap=1, max_misses=2, min_hits=3, stream=0):
        """Opens the slot's region tracking for w x h label images: the regions of regions_push followed from push to push
        by the overlap of their pixels with the footprint the tracks left, with hits, misses and confirmation
        (include/rcflow.h, "rip tracks").  The footprint takes 4 bytes per pixel of device memory."""
        p = TracksParams(max_regions=int(max_regions), max_tracks=int(max_tracks), min_overlap=int(min_overlap),
                         max_misses=int(max_misses), min_hits=int(min_hits), flags=0)
        self._bind(stream)          # the state is zeroed on the slot's stream: the one the pushes will run on
        check(self._lib.rcflow_tracks_open(self._h, stream, int(w), int(h), C.byref(p)))

    def tracks_info(self, stream=0):
        """dict of rc_tracks_info, the parameters beside the rest; never blocks."""
        info = self._info("tracks", TracksInfo(), stream)
        return _record(info)

    def tracks_push(self, labels, regions, regions_summary, tracks=None, track_of_label=None, mask_out=None, summary=None, stream=0):
        """One set of regions, as regions_push left it on the device: labels HxW int32 (dense pixels, rows may be padded),
        regions the uint8 tensor of rc_region records, at least the max_regions of tracks_open (the push reads up to that
        many, whatever the summary says), regions_summary its 8 int64.  RC_TRACKS_LAUNCHES launches, nothing is
        synchronised.  Outputs are preallocated device tensors, each optional: tracks a contiguous uint8 tensor of
        max_tracks * 128 bytes (rc_track records, TRACK_DTYPE), track_of_label max_regions + 1 int32, mask_out HxW uint8
        (255 inside the regions of confirmed tracks), summary 8 int64.  The table and the summary also stay on the slot for
        tracks_read / tracks_prims."""
        i = self._info("tracks", TracksInfo(), stream)
        h, w, max_regions = i.h, i.w, i.prm.max_regions
        lbl = self._in_image(labels, torch.int32, "labels", (h, w))
        ok = _is_t(regions) and regions.is_cuda and regions.device == self.device and regions.dtype == torch.uint8 and regions.is_contiguous()
        if not ok or regions.numel() % REGION_DTYPE.itemsize or regions.numel() < max_regions * REGION_DTYPE.itemsize:
            raise ValueError("regions must be a contiguous uint8 tensor of at least max_regions (%d) rc_region records on %s" % (
                max_regions, self.device))
        _check_out(regions_summary, self.device, torch.int64, "regions_summary", numel=8)
        tp = self._out_array(tracks, torch.uint8, "tracks", i.prm.max_tracks * TRACK_DTYPE.itemsize)
        lp = self._out_array(track_of_label, torch.int32, "track_of_label", max_regions + 1)
        op, ostep = self._out_image(mask_out, torch.uint8, "mask_out", (h, w))
        sp = self._out_array(summary, torch.int64, "summary", 8)
        self._bind(stream)
        check(self._lib.rcflow_tracks_push_dev(self._h, stream, *lbl, self._ptr(regions),
                                               self._ptr(regions_summary), tp, lp, op, ostep, sp))

    def tracks_prims(self, color=0x00ffff, thickness=1, disc_radius=3, out=None, stream=0):
        """The table of the last push as 5 * max_tracks primitives for draw() -> a device uint8 tensor of rc_draw_prim
        records: per confirmed track that has not ended its box (four lines) and a disc at its centroid; every other slot
        is kind 0, which draw() skips (and counts)."""
        n = 5 * self.tracks_info(stream)["max_tracks"]
        out = self._prims_out(out, n)
        self._bind(stream)
        check(self._lib.rcflow_tracks_prims_dev(self._h, stream, int(color), int(thickness), int(disc_radius), self._ptr(out)))
        return out

    def tracks_read(self, stream=0):
        """Waits for the slot's stream -> (the table as a numpy array of max_tracks TRACK_DTYPE records in slot order, the
        footprint as an HxW int32 array, dict of the summary with the names of TRACKS_SUMMARY)."""
        info = self.tracks_info(stream)
        tab, foot = np.zeros(info["max_tracks"], TRACK_DTYPE), np.zeros((info["h"], info["w"]), np.int32)
        return tab, foot, self._summary(self._lib.rcflow_tracks_read, stream, TRACKS_SUMMARY, tab.ctypes.data, len(tab), foot.ctypes.data)

    def tracks_reset(self, stream=0):
        self._lifecycle("tracks", "reset", stream)

    def tracks_close(self, stream=0):
        self._lifecycle("tracks", "close", stream)

    def _an_size(self, stream):
        w, h = C.c_int(0), C.c_int(0)
        check(self._lib.rcflow_analysis_size(self._h, stream, C.byref(w), C.byref(h)))
        if w.value <= 0 or h.value <= 0:
            raise RuntimeError("the slot has no analysis state yet")
        return w.value, h.value

    def streamline_display(self, which, stream=0):
        """streamline_displacement (0) / _total_motion (1) / _ratio (2), ripcurrents_module.cpp:13-40, on the
        slot's streamline field: returns (8UC3 BGR image on the device, the minMaxLoc maximum)."""
        w, h = self._an_size(stream)
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
        mx = C.c_float(0)
        self._bind(stream)
        check(self._lib.rcflow_streamline_display_dev(self._h, stream, int(which), self._ptr(out), out.stride(0),
                                                      C.byref(mx)))
        return out, mx.value

    def streamline_positions(self, stream=0):
        """streamline_positions ripcurrents_module.cpp:44-60: 32FC3 image, (1,1,1) where particles sit."""
        w, h = self._an_size(stream)
        out = torch.zeros((h, w, 3), dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_streamline_positions_dev(self._h, stream, self._ptr(out), out.stride(0) * 4))
        return out

    def hsv_to_bgr(self, hsv, stream=0):
        """cvtColor(current, current, CV_HSV2BGR) on the 32FC3 display image (ripcurrents.cpp:405)."""
        a = self._dev(hsv, torch.float32).contiguous()
        h, w = a.shape[:2]
        out = torch.empty_like(a)
        self._bind(stream)
        check(self._lib.rcflow_hsv_to_bgr_dev(self._h, stream, self._ptr(a), a.stride(0) * 4, w, h, self._ptr(out),
                                              out.stride(0) * 4))
        return out

    def jet_lut(self):
        lut = np.zeros((256, 3), np.uint8)
        check(self._lib.rcflow_jet_lut(lut.ctypes.data))
        return lut

    def calcOpticalFlowPyrLK(self, prev, nxt, prev_pts, next_pts=None, win=(21, 21), max_level=3,
                             crit_type=3, max_count=30, epsilon=0.01, flags=0, min_eig_threshold=1e-4, stream=0):
        """cv::calcOpticalFlowPyrLK on 8UC1 images (Streakline.cpp:32, ripcurrents_module.cpp:716,738,775,
        1162).  crit_type: 1 = COUNT, 2 = EPS; flags: 4 = OPTFLOW_USE_INITIAL_FLOW, 8 =
        OPTFLOW_LK_GET_MIN_EIGENVALS.  Returns (next_pts [n,2] f32, status [n] u8, err [n] f32) on the device."""
        a = self._dev(prev, torch.uint8)
        b = self._dev(nxt, torch.uint8)
        if a.stride(1) != 1:
            a = a.contiguous()
        if b.stride(1) != 1:
            b = b.contiguous()
        h, w = a.shape
        if tuple(b.shape) != (h, w):
            raise ValueError("prev and next differ in size")
        p = self._dev(prev_pts, torch.float32).reshape(-1, 2).contiguous()
        n = p.shape[0]
        if next_pts is None:
            q = torch.zeros((n, 2), dtype=torch.float32, device=self.device)
        else:
            q = self._dev(next_pts, torch.float32).reshape(-1, 2).contiguous().clone()
        status = torch.zeros((n,), dtype=torch.uint8, device=self.device)
        err = torch.zeros((n,), dtype=torch.float32, device=self.device)
        self._bind(stream)
        check(self._lib.rcflow_pyrlk_dev(self._h, stream, self._ptr(a), a.stride(0), self._ptr(b), b.stride(0), w, h,
                                         self._ptr(p), self._ptr(q), n, self._ptr(status), self._ptr(err),
                                         int(win[0]), int(win[1]), int(max_level), int(crit_type), int(max_count),
                                         float(epsilon), int(flags), float(min_eig_threshold)))
        return q, status, err

    def calcOpticalFlowPyrLK_host(self, prev, nxt, prev_pts, win=(21, 21), max_level=3, crit_type=3, max_count=30,
                                  epsilon=0.01, flags=0, min_eig_threshold=1e-4, stream=0):
        """Host-pointer form (rcflow_pyrlk_u8): numpy in, numpy out, blocking."""
        a = np.ascontiguousarray(prev, np.uint8)
        b = np.ascontiguousarray(nxt, np.uint8)
        h, w = a.shape
        p = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        n = p.shape[0]
        q = np.zeros((n, 2), np.float32)
        status = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        self._bind(stream)
        check(self._lib.rcflow_pyrlk_u8(self._h, stream, a.ctypes.data, a.strides[0], b.ctypes.data, b.strides[0], w, h,
                                        p.ctypes.data, q.ctypes.data, n, status.ctypes.data, err.ctypes.data,
                                        int(win[0]), int(win[1]), int(max_level), int(crit_type), int(max_count),
                                        float(epsilon), int(flags), float(min_eig_threshold)))
        return q, status, err

    def pyrlk_levels(self, w, h, win, max_level):
        return check(self._lib.rcflow_pyrlk_levels(w, h, int(win[0]), int(win[1]), int(max_level)))

    # ------------------------------------------------------------------ measurement
    def profile_enable(self, on=True):
        check(self._lib.rcflow_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        check(self._lib.rcflow_profile_reset(self._h))

    def profile_read(self):
        cap = 256
        names = (C.c_char_p * cap)()
        launches = (C.c_int * cap)()
        ms = (C.c_double * cap)()
        by = (C.c_double * cap)()
        mb = (C.c_double * cap)()
        n = check(self._lib.rcflow_profile_read(self._h, cap, names, launches, ms, by, mb))
        return [dict(kernel=names[i].decode(), launches=launches[i], total_ms=ms[i], alg_bytes=by[i],
                     model_bytes=mb[i]) for i in range(n)]

    def profile_read_buckets(self):
        """GPU time per bucket of the reference's own timing printout (ripcurrents.cpp:518-524):
        {"farneback": ms, "polar": ms, "threshold": ..., "overlay", "erosion", "codec", "stream"}."""
        names = (C.c_char_p * 7)()
        ms = (C.c_double * 7)()
        n = check(self._lib.rcflow_profile_read_buckets(self._h, names, ms))
        return {names[i].decode(): ms[i] for i in range(n)}


class _Product:
    """One per-slot product as an object: Context.<product>_* with the context and the slot bound.  Opens on construction,
    closes on close() or at the end of a with block.  A subclass names its product and adds what only that product has."""
    product = None

    def __init__(self, ctx, w, h, stream=0, **params):
        self.ctx, self.stream = ctx, stream
        self._method("open")(w, h, stream=stream, **params)

    def _method(self, verb):
        return getattr(self.ctx, "%s_%s" % (self.product, verb))

    def push(self, gray, **outputs):
        self._method("push")(gray, stream=self.stream, **outputs)

    def read(self):
        return self._method("read")(self.stream)

    def info(self):
        return self._method("info")(self.stream)

    def reset(self):
        self._method("reset")(self.stream)

    def close(self):
        self._method("close")(self.stream)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Waves(_Product):
    """The wave spectra of one slot as an object: Context.waves_* with the context and the slot bound.  Opens on construction,
    closes on close() or at the end of a with block."""
    product = "waves"

    def spectrum(self):
        return self.ctx.waves_spectrum(self.stream)

    def table(self):
        return self.ctx.waves_table(self.stream)

    def set(self, tanh_max, min_pixels, vis_max_depth):
        self.ctx.waves_set(tanh_max, min_pixels, vis_max_depth, self.stream)


class Piv(_Product):
    """The ensemble PIV of one slot as an object: Context.piv_* with the context and the slot bound.  Opens on construction,
    closes on close() or at the end of a with block."""
    product = "piv"

    def sums(self):
        return self.ctx.piv_sums(self.stream)

    def set(self, min_peak, median_eps, median_thr, vis_max):
        self.ctx.piv_set(min_peak, median_eps, median_thr, vis_max, self.stream)


class Transects(_Product):
    """The transects of one slot as an object: Context.transects_* with the context and the slot bound.  Opens on construction
    (lines and the parameters of Context.transects_open as keywords), closes on close() or at the end of a with block."""
    product = "transects"

    def push(self, gray=None, flow=None, **outputs):
        self.ctx.transects_push(gray, flow, stream=self.stream, **outputs)

    def sums(self):
        return self.ctx.transects_sums(self.stream)

    def table(self):
        return self.ctx.transects_table(self.stream)

    def set(self, jet_min, vis_max):
        self.ctx.transects_set(jet_min, vis_max, self.stream)


class Kinematics(_Product):
    """The flow kinematics of one slot as an object: Context.kinematics_* with the context and the slot bound.  Opens on
    construction (the parameters of Context.kinematics_open as keywords), closes on close() or at the end of a with block."""
    product = "kinematics"

    def set(self, ow_k, ow_min, omega_min, vis_max):
        self.ctx.kinematics_set(ow_k, ow_min, omega_min, vis_max, self.stream)


class Shoreline(_Product):
    """The shoreline of one slot as an object: Context.shoreline_* with the context and the slot bound.  Opens on construction
    (lines and the parameters of Context.shoreline_open as keywords), closes on close() or at the end of a with block."""
    product = "shoreline"

    def push(self, image, roi=None, **outputs):
        self.ctx.shoreline_push(image, roi, stream=self.stream, **outputs)

    def prims(self, **kw):
        return self.ctx.shoreline_prims(stream=self.stream, **kw)

    def ring(self):
        return self.ctx.shoreline_ring(self.stream)

    def table(self):
        return self.ctx.shoreline_table(self.stream)

    def set(self, threshold, min_sep, max_jump):
        self.ctx.shoreline_set(threshold, min_sep, max_jump, self.stream)


class Surf(_Product):
    """The surf zone of one slot as an object: Context.surf_* with the context and the slot bound.  Opens on construction (lines
    and the parameters of Context.surf_open as keywords), closes on close() or at the end of a with block."""
    product = "surf"

    def prims(self, **kw):
        return self.ctx.surf_prims(stream=self.stream, **kw)

    def table(self):
        return self.ctx.surf_table(self.stream)

    def set(self, bright, delta, q_min, ratio, min_load, vis_permille):
        self.ctx.surf_set(bright, delta, q_min, ratio, min_load, vis_permille, self.stream)


class MeanFlow(_Product):
    """The mean current of one slot as an object: Context.meanflow_* with the context and the slot bound.  Opens on construction
    (the parameters of Context.meanflow_open as keywords), closes on close() or at the end of a with block."""
    product = "meanflow"

    def push(self, flow=None, **outputs):
        self.ctx.meanflow_push(flow, stream=self.stream, **outputs)

    def set(self, steady_min, speed_min, min_cos2, dir_x, dir_y, min_fill):
        self.ctx.meanflow_set(steady_min, speed_min, min_cos2, dir_x, dir_y, min_fill, self.stream)


class FlowCheck(_Product):
    """The flow check of one slot as an object: Context.flowcheck_* with the context and the slot bound.  Opens on construction
    (the parameters of Context.flowcheck_open as keywords), closes on close() or at the end of a with block."""
    product = "flowcheck"

    def push(self, next, prev=None, flow=None, back=None, **outputs):
        self.ctx.flowcheck_push(next, prev, flow, back, stream=self.stream, **outputs)

    def set(self, tests, tex_min, res_max, gain_pm, fb_rel, fb_abs, speed_max):
        self.ctx.flowcheck_set(tests, tex_min, res_max, gain_pm, fb_rel, fb_abs, speed_max, self.stream)


class Drifters(_Product):
    """The virtual drifters of one slot as an object: Context.drifters_* with the context and the slot bound.  Opens on construction
    (the parameters of Context.drifters_open as keywords), closes on close() or at the end of a with block."""
    product = "drifters"

    def seed(self, xy):
        self.ctx.drifters_seed(xy, self.stream)

    def push(self, flow=None, zone=None, **outputs):
        self.ctx.drifters_push(flow, zone, stream=self.stream, **outputs)

    def set(self, dt, max_age, density_full, live_min, respawn):
        self.ctx.drifters_set(dt, max_age, density_full, live_min, respawn, self.stream)


class Infill(_Product):
    """The flow infill of one slot as an object: Context.infill_* with the context and the slot bound.  Opens on construction
    (the parameters of Context.infill_open as keywords), closes on close() or at the end of a with block."""
    product = "infill"

    def push(self, flow=None, valid=None, domain=None, **outputs):
        self.ctx.infill_push(flow, valid, domain, stream=self.stream, **outputs)

    def set(self, levels, min_known, leave):
        self.ctx.infill_set(levels, min_known, leave, self.stream)


class Offshore(_Product):
    """The offshore frame of one slot as an object: Context.offshore_* with the context and the slot bound.  Opens on construction
    (the parameters of Context.offshore_open as keywords), closes on close() or at the end of a with block."""
    product = "offshore"

    def map(self, wet, **outputs):
        self.ctx.offshore_map(wet, stream=self.stream, **outputs)

    def push(self, flow=None, **outputs):
        self.ctx.offshore_push(flow, stream=self.stream, **outputs)

    def band(self, lo, hi, out=None):
        return self.ctx.offshore_band(lo, hi, out, self.stream)

    def set(self, min_dist, max_dist, bin_width, min_count, rip_bins, cross_min, station):
        self.ctx.offshore_set(min_dist, max_dist, bin_width, min_count, rip_bins, cross_min, station, self.stream)


class Outlines(_Product):
    """The region outlines of one slot as an object: Context.outlines_* with the context and the slot bound.  Opens on construction
    (the parameters of Context.outlines_open as keywords), closes on close() or at the end of a with block."""
    product = "outlines"

    def push(self, labels=None, mask=None, **outputs):
        self.ctx.outlines_push(labels, mask, stream=self.stream, **outputs)

    def prims(self, color=0x00ffff, thickness=1, out=None):
        return self.ctx.outlines_prims(color, thickness, out, self.stream)

    def set(self, min_cracks):
        self.ctx.outlines_set(min_cracks, self.stream)


def kinematics_taps(radius, sigma):
    """rcflow_kinematics_taps: the smoothing taps g_0..g_radius as float32, without a context or a GPU."""
    taps = np.zeros(max(0, min(int(radius), RC_KINEMATICS_MAX_RADIUS)) + 1, np.float32)
    check(_lib.load().rcflow_kinematics_taps(int(radius), float(sigma), taps.ctypes.data_as(C.POINTER(C.c_float))))
    return taps


def _transect_lines(lines):
    """(x0, y0, x1, y1, n) per line -> the ctypes array of rc_transect_line"""
    rows = [tuple(l) for l in lines]
    if not rows or any(len(r) != 5 for r in rows):
        raise ValueError("lines must be a non-empty sequence of (x0, y0, x1, y1, n)")
    return (TransectLine * len(rows))(*[TransectLine(float(r[0]), float(r[1]), float(r[2]), float(r[3]), int(r[4])) for r in rows])


def transects_plan(w, h, lines, metres_per_pixel=1.0, fps=1.0):
    """rcflow_transects_plan: the sample table and the per-line constants of `lines` on a w x h picture, without a context or a
    GPU -> (SAMPLES TRANSECT_SAMPLE_DTYPE, LINES TRANSECT_GEOM_DTYPE)."""
    lib = _lib.load()
    arr = _transect_lines(lines)
    total = C.c_int(0)
    check(lib.rcflow_transects_plan(int(w), int(h), arr, len(arr), float(metres_per_pixel), float(fps), None, None, C.byref(total)))
    table, geom = np.zeros(total.value, TRANSECT_SAMPLE_DTYPE), np.zeros(len(arr), TRANSECT_GEOM_DTYPE)
    check(lib.rcflow_transects_plan(int(w), int(h), arr, len(arr), float(metres_per_pixel), float(fps), table.ctypes.data, geom.ctypes.data, None))
    return table, geom


def shoreline_plan(w, h, lines, metres_per_pixel=1.0):
    """rcflow_shoreline_plan: the sample table and the per-line constants of `lines` (land to sea) on a w x h picture, without a
    context or a GPU -> (SAMPLES TRANSECT_SAMPLE_DTYPE, LINES TRANSECT_GEOM_DTYPE)."""
    lib = _lib.load()
    arr = _transect_lines(lines)
    total = C.c_int(0)
    check(lib.rcflow_shoreline_plan(int(w), int(h), arr, len(arr), float(metres_per_pixel), None, None, C.byref(total)))
    table, geom = np.zeros(total.value, TRANSECT_SAMPLE_DTYPE), np.zeros(len(arr), TRANSECT_GEOM_DTYPE)
    check(lib.rcflow_shoreline_plan(int(w), int(h), arr, len(arr), float(metres_per_pixel), table.ctypes.data, geom.ctypes.data, None))
    return table, geom


def surf_plan(w, h, lines, metres_per_pixel=1.0):
    """rcflow_surf_plan: the sample table and the per-line constants of `lines` (land to sea) on a w x h picture, without a context
    or a GPU -> (SAMPLES TRANSECT_SAMPLE_DTYPE, LINES TRANSECT_GEOM_DTYPE)."""
    lib = _lib.load()
    arr = _transect_lines(lines) if len(lines) else None
    total = C.c_int(0)
    check(lib.rcflow_surf_plan(int(w), int(h), arr, len(lines), float(metres_per_pixel), None, None, C.byref(total)))
    table, geom = np.zeros(total.value, TRANSECT_SAMPLE_DTYPE), np.zeros(len(lines), TRANSECT_GEOM_DTYPE)
    if len(lines):
        check(lib.rcflow_surf_plan(int(w), int(h), arr, len(lines), float(metres_per_pixel), table.ctypes.data, geom.ctypes.data, None))
    return table, geom


def _alias_tensor(ptr, n, dtype, device):
    """A torch tensor aliasing `n` elements of device memory the library owns."""
    itemsize = torch.empty((), dtype=dtype).element_size()

    class _Holder:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<i%d" % itemsize if dtype != torch.float32 else "<f4",
                                    "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Holder(), device=device)


class Streakline:
    """Streakline.hpp:8-20 / Streakline.cpp:11-71 with the vertices moved through the dense
    flow field (the compute_timelinesFarne precedent, main.cpp:961-977) instead of sparse LK.
    Fields as in the reference: generationPoint, vertices, numberOfVertices, frameCount."""

    def __init__(self, pixel):
        self.generationPoint = (float(pixel[0]), float(pixel[1]))
        self.vertices = [self.generationPoint]
        self.numberOfVertices = 1
        self.frameCount = 1

    def run(self, ctx, flow, width, height, dt=1.0, stream=0):
        """runLK's bookkeeping: move every vertex, reject jumps > 0.1*dim (Streakline.cpp:35-40),
        insert the generation point in front (:46-48)."""
        v = np.asarray(self.vertices, np.float32).reshape(-1, 2)
        # variant 4 = `p += delta*dt/iterations` with no cutoff; one step
        moved, _ = ctx.streamline(v, flow, dt, 1, 0.0, variant=4, stream=stream)
        nxt = moved.cpu().numpy()
        big = (np.abs(v[:, 0] - nxt[:, 0]) > width * 0.1) | (np.abs(v[:, 1] - nxt[:, 1]) > height * 0.1)
        nxt[big] = v[big]
        self.vertices = [self.generationPoint] + [tuple(map(float, p)) for p in nxt]
        self.numberOfVertices = len(self.vertices)
        self.frameCount += 1
        return self.vertices

    def runLK(self, ctx, u_prev, u_current, stream=0):
        """Streakline::runLK (Streakline.cpp:22-71) with the reference's own mover: PyrLK 50x50, maxLevel 3,
        COUNT+EPS (30, 0.1), flags 10, minEigThreshold 1e-4 (:32); XDIM/YDIM are the frame size."""
        height, width = u_prev.shape[:2]
        v = np.asarray(self.vertices, np.float32).reshape(-1, 2)
        q, _, _ = ctx.calcOpticalFlowPyrLK(u_prev, u_current, v, win=(50, 50), max_level=3, crit_type=3,
                                           max_count=30, epsilon=0.1, flags=10, min_eig_threshold=1e-4,
                                           stream=stream)
        nxt = q.cpu().numpy()
        big = (np.abs(v[:, 0] - nxt[:, 0]) > width * 0.1) | (np.abs(v[:, 1] - nxt[:, 1]) > height * 0.1)
        nxt[big] = v[big]
        self.vertices = [self.generationPoint] + [tuple(map(float, p)) for p in nxt]
        self.numberOfVertices = len(self.vertices)
        self.frameCount += 1
        return self.vertices


def _run_lk_all(ctx, vertices, u_prev, u_current, stream=0):
    """The PyrLK call shared by Timeline::runLK and PopulationMap::runLK (ripcurrents_module.cpp:775,
    :1162): 50x50 window, maxLevel 3, COUNT+EPS (30, 0.1), flags 10, minEigThreshold 1e-4; every vertex
    takes its tracked position (the jump rejection is commented out in the reference)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 2)
    q, _, _ = ctx.calcOpticalFlowPyrLK(u_prev, u_current, v, win=(50, 50), max_level=3, crit_type=3, max_count=30,
                                       epsilon=0.1, flags=10, min_eig_threshold=1e-4, stream=stream)
    return [tuple(map(float, p)) for p in q.cpu().numpy()]


class Timeline:
    """Timeline (ripcurrents.hpp:64-75, ripcurrents_module.cpp:751-807): numberOfVertices + 1 points on
    the segment lineStart..lineEnd, moved by sparse PyrLK every frame; drawing stays with the caller."""

    def __init__(self, lineStart, lineEnd, numberOfVertices):
        diffX = np.float32(np.float32(lineEnd[0] - lineStart[0]) / np.float32(numberOfVertices))
        diffY = np.float32(np.float32(lineEnd[1] - lineStart[1]) / np.float32(numberOfVertices))
        self.vertices = [(float(np.float32(lineStart[0]) + diffX * np.float32(i)),
                          float(np.float32(lineStart[1]) + diffY * np.float32(i))) for i in range(numberOfVertices + 1)]

    def runLK(self, ctx, u_prev, u_current, stream=0):
        self.vertices = _run_lk_all(ctx, self.vertices, u_prev, u_current, stream)
        return self.vertices


class PopulationMap:
    """PopulationMap (ripcurrents.hpp:86-95, ripcurrents_module.cpp:1140-1196): random points
    rectStart + (rectEnd - rectStart) * (u + 1), u uniform in [0, 1] -- the reference's formula,
    which lands them in the rectangle mirrored beyond rectEnd (`rand()/RAND_MAX + 1`) -- moved by
    sparse PyrLK.  `rng` replaces the reference's sranddev()/rand() (not reproducible by design)."""

    def __init__(self, rectStart, rectEnd, numberOfVertices, rng=None):
        rng = rng or np.random.RandomState()
        self.vertices = []
        for _ in range(numberOfVertices):
            randX = np.float32((rectEnd[0] - rectStart[0]) * (rng.uniform(0.0, 1.0) + 1) + rectStart[0])
            randY = np.float32((rectEnd[1] - rectStart[1]) * (rng.uniform(0.0, 1.0) + 1) + rectStart[1])
            self.vertices.append((float(randX), float(randY)))

    def runLK(self, ctx, u_prev, u_current, stream=0):
        self.vertices = _run_lk_all(ctx, self.vertices, u_prev, u_current, stream)
        return self.vertices
