"""ctypes binding of librcflow.so (the C ABI declared in include/rcflow.h).

The library is the product: there is no CPU fallback.  Loading fails loudly when the
built extension is missing.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RCFLOW_LIB selects another build of the same library (e.g. for an A/B run of two builds)
LIB_PATH = os.environ.get("RCFLOW_LIB") or os.path.join(_HERE, "librcflow.so")

RC_OK = 0
RC_FARNEBACK_GAUSSIAN = 256
RC_FARNEBACK_USE_INITIAL_FLOW = 4
HIST_BINS, HIST_DIRECTIONS, HIST_RESOLUTION = 50, 36, 20
HIST_WORDS = HIST_BINS + HIST_DIRECTIONS * HIST_BINS + 1 + HIST_DIRECTIONS
COMM_ID_BYTES = 128     # RC_COMM_ID_BYTES = sizeof(ncclUniqueId)
# RC_TIMEX_*: product name -> mask bit; the order is the order of rcflow_timex_push_dev's d_out[4]
TIMEX_PRODUCTS = {"mean": 1, "average": 2, "bright": 4, "dark": 8}
RC_WARP_INVERSE_MAP = 16
# RC_STAB_*: the motion models of rcflow_framestab_open_multi, and its one flag
STAB_MODELS = {"translation": 1, "similarity": 2, "affine": 3}
# rcflow_fit_motion_dev / rcflow_framestab_open_tracks add the homography
FIT_MODELS = dict(STAB_MODELS, homography=4)
RC_CORNER_MAX_CELLS = 4096
RC_FIT_MAX_POINTS = 4096
RC_STAB_ANCHOR_FIRST = 1
RC_STAB_MAX_PATCHES = 16
# rcflow_ripmap_open: its one flag, and the source names
RC_RIPMAP_WAIT_FULL = 1
RIPMAP_SOURCES = {"flow": 0, "delta": 1}

# rcflow_draw_dev: rc_draw_prim::kind / flags and the bounds of include/rcflow.h
RC_DRAW_DISC, RC_DRAW_LINE, RC_DRAW_BLEND = 1, 2, 1
RC_DRAW_COORD_MAX, RC_DRAW_MAX_THICKNESS = 16383, 8
# rcflow_tracers_*: movers and line kinds
TRACERS_MOVERS = {"lk": 0, "flow": 1}
TRACER_KINDS = {"streak": 0, "timeline": 1, "cloud": 2}
# rcflow_regions_*: the bound on max_regions, the launches of a push
RC_REGIONS_MAX, RC_REGIONS_LAUNCHES = 65536, 7
# rcflow_tracks_*: the bounds on max_regions and max_tracks, the launches of a push, rc_track::flags
RC_TRACKS_MAX_REGIONS, RC_TRACKS_MAX, RC_TRACKS_LAUNCHES = 1024, 1024, 6
TRACK_FLAGS = {"seen": 1, "born": 2, "coasting": 4, "ended": 8, "split": 16, "merged": 32, "confirmed": 64}
# rcflow_motion_*: its one flag, the automatic stamp, the launches of a push
RC_MOTION_FRESH, RC_MOTION_AUTO_TIME, RC_MOTION_LAUNCHES = 1, -1.0, 3
# rcflow_ftle_*: the directions, the bounds, the launches of a push that computes
FTLE_DIRECTIONS = {"forward": 0, "backward": 1}
RC_FTLE_MAX_WINDOW, RC_FTLE_MAX_SPACING, RC_FTLE_LAUNCHES = 256, 16, 3
# rcflow_planview_*: the launches of a push
RC_PLANVIEW_LAUNCHES = 1
# rcflow_waves_*: the record's flags, the bounds, the launches of a push that computes everything
RC_WAVES_EMPTY, RC_WAVES_NOWAVE, RC_WAVES_DEEP = 1, 2, 4
RC_WAVES_MAX_WINDOW, RC_WAVES_MAX_BINS, RC_WAVES_MAX_SPACING, RC_WAVES_MAX_STATE_BYTES, RC_WAVES_LAUNCHES = 4096, 16, 16, 4 << 30, 3
# rcflow_piv_*: the record's flags, the parameter flag, the bounds, the launches of a push that computes
RC_PIV_EMPTY, RC_PIV_FLAT, RC_PIV_EDGE, RC_PIV_LOWPEAK, RC_PIV_OUTLIER = 1, 2, 4, 8, 16
RC_PIV_REPLACE = 1
RC_PIV_MAX_WINDOW, RC_PIV_MAX_RANGE, RC_PIV_MAX_ENSEMBLE, RC_PIV_MAX_PIXEL_PAIRS, RC_PIV_MAX_STATE_BYTES, RC_PIV_LAUNCHES = 64, 16, 256, 1 << 18, 4 << 30, 3
# rcflow_transects_*: the sources, the record's flags, the bounds, the int64 per line of d_sums, the launches of a push that asks for everything
RC_TRANSECTS_GRAY, RC_TRANSECTS_FLOW = 1, 2
RC_TRANSECTS_EMPTY, RC_TRANSECTS_FLAT, RC_TRANSECTS_EDGE = 1, 2, 4
RC_TRANSECTS_MAX_LINES, RC_TRANSECTS_MAX_SAMPLES, RC_TRANSECTS_MAX_TOTAL, RC_TRANSECTS_MAX_WINDOW = 64, 1024, 65536, 4096
RC_TRANSECTS_MAX_LAG, RC_TRANSECTS_MAX_RANGE, RC_TRANSECTS_MAX_STATE_BYTES, RC_TRANSECTS_SUMS, RC_TRANSECTS_LAUNCHES = 8, 16, 1 << 30, 16, 3
# rcflow_kinematics_*: the parameter flag, the record's flags, the bounds, the int64 per cell of d_sums, the launches of a push with an output
RC_KINEMATICS_RELATIVE = 1
RC_KINEMATICS_EMPTY, RC_KINEMATICS_CW, RC_KINEMATICS_CCW = 1, 2, 4
RC_KINEMATICS_MAX_RADIUS, RC_KINEMATICS_MAX_SPACING, RC_KINEMATICS_MAX_PIXELS, RC_KINEMATICS_SUMS, RC_KINEMATICS_LAUNCHES = 8, 8, 1 << 25, 11, 2
# rcflow_shoreline_*: the sources, the record's flags, the bounds, the words of d_hist, the launches of a push that asks for a picture
SHORE_SOURCES = {"rmb": 0, "gray": 1, "plane": 2}
RC_SHORE_EMPTY, RC_SHORE_DRY, RC_SHORE_WET, RC_SHORE_UNSURE, RC_SHORE_OUTLIER, RC_SHORE_NO_WINDOW = 1, 2, 4, 8, 16, 32
RC_SHORE_MAX_LINES, RC_SHORE_MIN_SAMPLES, RC_SHORE_MAX_SAMPLES, RC_SHORE_MAX_TOTAL, RC_SHORE_MAX_RADIUS, RC_SHORE_MAX_WINDOW = 1024, 8, 1024, 262144, 7, 4096
RC_SHORE_MAX_PIXELS, RC_SHORE_MAX_STATE_BYTES, RC_SHORE_HIST, RC_SHORE_LAUNCHES = 1 << 25, 64 << 20, 512, 4
# rcflow_surf_*: the line record's flags, the bounds, the channel records of a push, the launches of a push with lines
RC_SURF_NOBAND, RC_SURF_NOREF, RC_SURF_CHANNEL, RC_SURF_IN_CHANNEL = 1, 2, 4, 8
RC_SURF_MAX_LINES, RC_SURF_MIN_SAMPLES, RC_SURF_MAX_SAMPLES, RC_SURF_MAX_TOTAL, RC_SURF_MAX_WINDOW, RC_SURF_MAX_SPAN = 1024, 8, 1024, 262144, 4096, 32
RC_SURF_MAX_CHANNELS, RC_SURF_MAX_SHARE, RC_SURF_MAX_PIXELS, RC_SURF_MAX_STATE_BYTES, RC_SURF_LAUNCHES = 32, 1000000, 1 << 25, 4 << 30, 3
# rcflow_meanflow_*: the direction flags, the record's flag, the bounds, the words of a cell's sums, the launches of a push
RC_MEANFLOW_DIR_FIXED, RC_MEANFLOW_DIR_OPPOSED, RC_MEANFLOW_EMPTY = 1, 2, 1
RC_MEANFLOW_MAX_WINDOW, RC_MEANFLOW_SUMS, RC_MEANFLOW_MAX_STATE_BYTES, RC_MEANFLOW_LAUNCHES = 4096, 8, 4 << 30, 2
# rcflow_flowcheck_*: a pixel's flags, the tests that can be switched, the fills, the record's flag, the bounds, the launches of a push
RC_FLOWCHECK_BAD, RC_FLOWCHECK_OUT, RC_FLOWCHECK_FLAT, RC_FLOWCHECK_RESID, RC_FLOWCHECK_NOGAIN, RC_FLOWCHECK_FB, RC_FLOWCHECK_FAST = 1, 2, 4, 8, 16, 32, 64
RC_FLOWCHECK_TESTS, RC_FLOWCHECK_FILL_NAN, RC_FLOWCHECK_FILL_ZERO, RC_FLOWCHECK_NONE_VALID = 124, 1, 2, 1
RC_FLOWCHECK_MAX_RADIUS, RC_FLOWCHECK_SUMS, RC_FLOWCHECK_SUMMARY, RC_FLOWCHECK_LAUNCHES = 7, 10, 10, 2
# rcflow_drifters_*: the bounds, the words of a cell's sums and of the summary, the launches of a push, the flags, the fates
RC_DRIFTERS_MAX, RC_DRIFTERS_SUMS, RC_DRIFTERS_HIST_BINS, RC_DRIFTERS_SUMMARY, RC_DRIFTERS_LAUNCHES = 1 << 22, 8, 32, 24, 2
RC_DRIFTERS_RESPAWN, RC_DRIFTERS_EMPTY = 1, 1
# rcflow_infill_*: the flags, the source bytes, the record's flag, the bounds, the words of a cell's sums and of the summary, the most launches of a push
RC_INFILL_LEAVE_NAN, RC_INFILL_LEAVE_ZERO, RC_INFILL_HELD, RC_INFILL_OUTSIDE, RC_INFILL_UNFILLED, RC_INFILL_NONE = 1, 2, 64, 254, 255, 1
RC_INFILL_MAX_LEVELS, RC_INFILL_MAX_MIN_KNOWN, RC_INFILL_MAX_HOLD, RC_INFILL_SUMS, RC_INFILL_SUMMARY, RC_INFILL_LAUNCHES = 7, 16384, 254, 8, 16, 4
# rcflow_offshore_*: the far value, the station flags, the classes, the record's flags, the bounds, the words of a cell and of a summary, the launches
RC_OFFSHORE_FAR, RC_OFFSHORE_STATION_X, RC_OFFSHORE_STATION_Y, RC_OFFSHORE_EMPTY, RC_OFFSHORE_RIP = 0x7fffffff, 1, 2, 1, 2
RC_OFFSHORE_C_OK, RC_OFFSHORE_C_NEAR, RC_OFFSHORE_C_FAR, RC_OFFSHORE_C_DRY, RC_OFFSHORE_C_BAD = 0, 1, 2, 3, 4
RC_OFFSHORE_MAX_DIST, RC_OFFSHORE_MAX_STATIONS, RC_OFFSHORE_MAX_BINS, RC_OFFSHORE_MAX_BIN_WIDTH, RC_OFFSHORE_MAX_SIDE = 4095, 256, 256, 256, 32767
RC_OFFSHORE_SUMS, RC_OFFSHORE_SUMMARY, RC_OFFSHORE_MAP_LAUNCHES, RC_OFFSHORE_PUSH_LAUNCHES = 4, 8, 3, 2
# rcflow_outlines_*: the bounds, the words of a summary, the launches that do not depend on the rounds, the record's flags
RC_OUTLINES_MAX_SIDE, RC_OUTLINES_MAX_CRACKS, RC_OUTLINES_MAX_LOOPS, RC_OUTLINES_MAX_VERTICES = 16383, 1 << 25, 1 << 20, 1 << 24
RC_OUTLINES_SUMMARY, RC_OUTLINES_FIXED_LAUNCHES, RC_OUTLINE_HOLE, RC_OUTLINE_NOVERTS = 8, 13, 1, 2
DRIFTERS_FATES = {"edge_left": 1, "edge_top": 2, "edge_right": 3, "edge_bottom": 4, "bad": 5, "aged": 6, "shore": 9, "offshore": 10}

ERRORS = {-1: "RC_EINVAL", -2: "RC_ENOMEM", -3: "RC_EHIP", -4: "RC_ENODEV", -5: "RC_ESIZE",
          -6: "RC_ESTATE", -7: "RC_ECOMM"}


class RcflowError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "RC_E?"), code, text))
        self.code = code


class FarnebackParams(C.Structure):
    _fields_ = [("pyr_scale", C.c_double), ("levels", C.c_int), ("winsize", C.c_int),
                ("iterations", C.c_int), ("poly_n", C.c_int), ("poly_sigma", C.c_double),
                ("flags", C.c_int)]


class FrameLoop(C.Structure):
    """rc_frame_loop (include/rcflow.h): the per-frame analysis chain of rcflow_frame_loop_step."""
    _fields_ = [("dt", C.c_float), ("iterations", C.c_int), ("d_seeds", C.c_void_p), ("nseeds", C.c_int),
                ("seed_variant", C.c_int), ("seed_dt", C.c_float), ("seed_iterations", C.c_int), ("seed_upper", C.c_float),
                ("MID", C.c_float), ("LOWER", C.c_float), ("d_outmask", C.c_void_p), ("mask_step", C.c_size_t),
                ("d_edges", C.c_void_p), ("edges_step", C.c_size_t), ("use_graph", C.c_int)]


class DrawPrim(C.Structure):
    """rc_draw_prim (include/rcflow.h), 32 bytes; numpy: api.DRAW_PRIM_DTYPE."""
    _fields_ = [("kind", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("size", C.c_int32), ("color", C.c_uint32), ("flags", C.c_uint32)]


class TracersParams(C.Structure):
    """rc_tracers_params (include/rcflow.h)."""
    _fields_ = [("mover", C.c_int), ("max_lines", C.c_int), ("max_vertices", C.c_int), ("max_points", C.c_int),
                ("win_w", C.c_int), ("win_h", C.c_int), ("max_level", C.c_int), ("crit_type", C.c_int),
                ("max_count", C.c_int), ("lk_flags", C.c_int), ("epsilon", C.c_double), ("min_eig", C.c_double),
                ("dt", C.c_float)]


class TracersInfo(C.Structure):
    """rc_tracers_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("mover", C.c_int), ("max_lines", C.c_int), ("max_vertices", C.c_int),
                ("max_points", C.c_int), ("lines", C.c_int), ("points", C.c_int), ("prims", C.c_int), ("primed", C.c_int),
                ("pushes", C.c_longlong), ("dropped", C.c_longlong), ("device_bytes", C.c_size_t)]


class RegionsParams(C.Structure):
    """rc_regions_params (include/rcflow.h)."""
    _fields_ = [("connectivity", C.c_int), ("min_area", C.c_int), ("max_regions", C.c_int), ("flags", C.c_int)]


class Region(C.Structure):
    """rc_region (include/rcflow.h), 144 bytes; numpy: api.REGION_DTYPE."""
    _fields_ = [("label", C.c_int32), ("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32), ("first_x", C.c_int32), ("first_y", C.c_int32), ("edges", C.c_int32), ("bad", C.c_int32),
                ("sx", C.c_int64), ("sy", C.c_int64), ("sxx", C.c_int64), ("syy", C.c_int64), ("sxy", C.c_int64),
                ("fx", C.c_int64), ("fy", C.c_int64), ("cx", C.c_double), ("cy", C.c_double), ("var_major", C.c_double),
                ("var_minor", C.c_double), ("angle", C.c_double), ("mean_fx", C.c_float), ("mean_fy", C.c_float)]


class RegionsInfo(C.Structure):
    """rc_regions_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("connectivity", C.c_int), ("min_area", C.c_int), ("max_regions", C.c_int),
                ("flags", C.c_int), ("launches_per_push", C.c_int), ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class TracksParams(C.Structure):
    """rc_tracks_params (include/rcflow.h)."""
    _fields_ = [("max_regions", C.c_int), ("max_tracks", C.c_int), ("min_overlap", C.c_int), ("max_misses", C.c_int),
                ("min_hits", C.c_int), ("flags", C.c_int)]


class Track(C.Structure):
    """rc_track (include/rcflow.h), 128 bytes; numpy: api.TRACK_DTYPE."""
    _fields_ = [("id", C.c_int64), ("parent", C.c_int64), ("first_push", C.c_int64), ("area_sum", C.c_int64), ("fx_sum", C.c_int64),
                ("fy_sum", C.c_int64), ("m_sum", C.c_int64), ("slot", C.c_int32), ("label", C.c_int32), ("flags", C.c_int32),
                ("age", C.c_int32), ("hits", C.c_int32), ("misses", C.c_int32), ("area", C.c_int32), ("x0", C.c_int32),
                ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("px", C.c_int32), ("py", C.c_int32), ("px0", C.c_int32),
                ("py0", C.c_int32), ("overlap", C.c_int32), ("mean_fx", C.c_float), ("mean_fy", C.c_float)]


class TracksInfo(C.Structure):
    """rc_tracks_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", TracksParams), ("launches_per_push", C.c_int), ("pushes", C.c_longlong),
                ("device_bytes", C.c_size_t)]


class MotionParams(C.Structure):
    """rc_motion_params (include/rcflow.h)."""
    _fields_ = [("diff_threshold", C.c_int), ("duration", C.c_double), ("delta1", C.c_double), ("delta2", C.c_double),
                ("grid_x", C.c_int), ("grid_y", C.c_int), ("flags", C.c_int)]


class MotionCell(C.Structure):
    """rc_motion_cell (include/rcflow.h), 40 bytes; numpy: api.MOTION_CELL_DTYPE."""
    _fields_ = [("angle", C.c_double), ("S", C.c_longlong), ("W", C.c_longlong), ("tsmax", C.c_float), ("n_masked", C.c_int),
                ("n_used", C.c_int), ("peak_bin", C.c_int)]


class MotionInfo(C.Structure):
    """rc_motion_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", MotionParams), ("launches_per_push", C.c_int), ("pushes", C.c_longlong),
                ("last_timestamp", C.c_double), ("device_bytes", C.c_size_t)]


class FtleParams(C.Structure):
    """rc_ftle_params (include/rcflow.h)."""
    _fields_ = [("window", C.c_int), ("direction", C.c_int), ("dt", C.c_float), ("spacing", C.c_int), ("threshold", C.c_double),
                ("vis_max", C.c_double), ("flags", C.c_int)]


class FtleInfo(C.Structure):
    """rc_ftle_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", FtleParams), ("launches_per_push", C.c_int), ("held", C.c_int),
                ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class PlanViewParams(C.Structure):
    """rc_planview_params (include/rcflow.h)."""
    _fields_ = [("H", C.c_double * 9), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("x0", C.c_double), ("y0", C.c_double), ("dx", C.c_double), ("dy", C.c_double),
                ("nx", C.c_int), ("ny", C.c_int), ("fps", C.c_double), ("max_gsd", C.c_double), ("flags", C.c_int)]


class PlanViewInfo(C.Structure):
    """rc_planview_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", PlanViewParams), ("launches_per_push", C.c_int), ("pushes", C.c_longlong),
                ("device_bytes", C.c_size_t)]


class WavesParams(C.Structure):
    """rc_waves_params (include/rcflow.h)."""
    _fields_ = [("window", C.c_int), ("bin_lo", C.c_int), ("bin_hi", C.c_int), ("spacing", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int),
                ("min_pixels", C.c_int), ("flags", C.c_int), ("fps", C.c_double), ("metres_per_pixel_x", C.c_double),
                ("metres_per_pixel_y", C.c_double), ("gravity", C.c_double), ("tanh_max", C.c_double), ("vis_max_depth", C.c_double)]


class WavesInfo(C.Structure):
    """rc_waves_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", WavesParams), ("launches_per_push", C.c_int), ("bins", C.c_int), ("shift", C.c_int),
                ("held", C.c_int), ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class PivParams(C.Structure):
    """rc_piv_params (include/rcflow.h)."""
    _fields_ = [("window", C.c_int), ("range", C.c_int), ("step", C.c_int), ("ensemble", C.c_int), ("flags", C.c_int),
                ("min_peak", C.c_double), ("median_eps", C.c_double), ("median_thr", C.c_double), ("vis_max", C.c_double)]


class PivInfo(C.Structure):
    """rc_piv_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", PivParams), ("grid_x", C.c_int), ("grid_y", C.c_int), ("launches_per_push", C.c_int),
                ("pairs", C.c_int), ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class TransectLine(C.Structure):
    """rc_transect_line (include/rcflow.h)."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("n", C.c_int)]


class TransectsParams(C.Structure):
    """rc_transects_params (include/rcflow.h)."""
    _fields_ = [("window", C.c_int), ("sources", C.c_int), ("lag", C.c_int), ("range", C.c_int), ("flags", C.c_int), ("pad", C.c_int),
                ("fps", C.c_double), ("metres_per_pixel", C.c_double), ("jet_min", C.c_double), ("vis_max", C.c_double)]


class TransectsInfo(C.Structure):
    """rc_transects_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", TransectsParams), ("lines", C.c_int), ("samples", C.c_int),
                ("launches_per_push", C.c_int), ("held", C.c_int), ("pairs", C.c_int), ("pad", C.c_int), ("pushes", C.c_longlong),
                ("device_bytes", C.c_size_t)]


class KinematicsParams(C.Structure):
    """rc_kinematics_params (include/rcflow.h)."""
    _fields_ = [("radius", C.c_int), ("spacing", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("min_core", C.c_int), ("flags", C.c_int),
                ("pad", C.c_int * 2), ("sigma", C.c_double), ("scale", C.c_double), ("pixel_area", C.c_double), ("ow_k", C.c_double),
                ("ow_min", C.c_double), ("omega_min", C.c_double), ("vis_max", C.c_double)]


class KinematicsCell(C.Structure):
    """rc_kinematics_cell (include/rcflow.h), 48 bytes; numpy: api.KINEMATICS_CELL_DTYPE."""
    _fields_ = [("flags", C.c_int), ("n", C.c_int), ("bad", C.c_int), ("mean_vorticity", C.c_float), ("circulation", C.c_float),
                ("mean_divergence", C.c_float), ("enstrophy", C.c_float), ("mean_ow", C.c_float), ("cores_cw", C.c_int), ("cores_ccw", C.c_int),
                ("circulation_cw", C.c_float), ("circulation_ccw", C.c_float)]


class KinematicsInfo(C.Structure):
    """rc_kinematics_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", KinematicsParams), ("margin", C.c_int), ("launches_per_push", C.c_int),
                ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class ShorelineParams(C.Structure):
    """rc_shoreline_params (include/rcflow.h), 56 bytes."""
    _fields_ = [("source", C.c_int), ("radius", C.c_int), ("wet_is_high", C.c_int), ("threshold", C.c_int), ("window", C.c_int),
                ("permille", C.c_int), ("flags", C.c_int), ("pad", C.c_int), ("min_sep", C.c_double), ("max_jump", C.c_double),
                ("metres_per_pixel", C.c_double)]


class ShorelineRecord(C.Structure):
    """rc_shoreline (include/rcflow.h), 64 bytes; numpy: api.SHORELINE_DTYPE."""
    _fields_ = [("flags", C.c_int), ("k", C.c_int), ("pos", C.c_int), ("agree", C.c_int), ("wx", C.c_int), ("wy", C.c_int), ("x", C.c_float),
                ("y", C.c_float), ("dist_m", C.c_float), ("nv", C.c_int), ("pos_min", C.c_int), ("pos_max", C.c_int), ("pos_q", C.c_int),
                ("pos_mean", C.c_float), ("excursion_m", C.c_float), ("pad", C.c_int)]


class ShorelineInfo(C.Structure):
    """rc_shoreline_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", ShorelineParams), ("lines", C.c_int), ("samples", C.c_int),
                ("launches_per_push", C.c_int), ("held", C.c_int), ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class SurfParams(C.Structure):
    """rc_surf_params (include/rcflow.h), 56 bytes."""
    _fields_ = [("window", C.c_int), ("bright", C.c_int), ("delta", C.c_int), ("q_min", C.c_int), ("min_run", C.c_int), ("span", C.c_int),
                ("ratio", C.c_int), ("min_load", C.c_int), ("min_lines", C.c_int), ("vis_permille", C.c_int), ("flags", C.c_int), ("pad", C.c_int),
                ("metres_per_pixel", C.c_double)]


class SurfLine(C.Structure):
    """rc_surf_line (include/rcflow.h), 64 bytes; numpy: api.SURF_LINE_DTYPE."""
    _fields_ = [("flags", C.c_int), ("k0", C.c_int), ("k1", C.c_int), ("load", C.c_int), ("peak", C.c_int), ("kpeak", C.c_int), ("ix", C.c_int),
                ("iy", C.c_int), ("ox", C.c_int), ("oy", C.c_int), ("ref", C.c_int), ("share", C.c_int), ("width_m", C.c_float), ("pad", C.c_int * 3)]


class SurfChannel(C.Structure):
    """rc_surf_channel (include/rcflow.h), 32 bytes; numpy: api.SURF_CHANNEL_DTYPE."""
    _fields_ = [("first", C.c_int), ("count", C.c_int), ("centre", C.c_int), ("share", C.c_int), ("cx", C.c_int), ("cy", C.c_int),
                ("width_m", C.c_float), ("pad", C.c_int)]


class MeanflowParams(C.Structure):
    """rc_meanflow_params (include/rcflow.h), 56 bytes."""
    _fields_ = [("window", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("min_fill", C.c_int), ("steady_min", C.c_int), ("flags", C.c_int),
                ("speed_min", C.c_double), ("min_cos2", C.c_double), ("dir_x", C.c_double), ("dir_y", C.c_double)]


class MeanflowCell(C.Structure):
    """rc_meanflow_cell (include/rcflow.h), 32 bytes; numpy: api.MEANFLOW_CELL_DTYPE."""
    _fields_ = [("flags", C.c_int), ("filled", C.c_int), ("mask", C.c_int), ("bad", C.c_int), ("mean_x", C.c_float), ("mean_y", C.c_float),
                ("steadiness", C.c_float), ("pad", C.c_int)]


class MeanflowInfo(C.Structure):
    """rc_meanflow_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", MeanflowParams), ("launches_per_push", C.c_int), ("held", C.c_int),
                ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class FlowcheckParams(C.Structure):
    """rc_flowcheck_params (include/rcflow.h), 64 bytes."""
    _fields_ = [("radius", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("tests", C.c_int), ("flags", C.c_int), ("tex_min", C.c_int),
                ("gain_pm", C.c_int), ("pad", C.c_int), ("res_max", C.c_double), ("fb_rel", C.c_double), ("fb_abs", C.c_double),
                ("speed_max", C.c_double)]


class FlowcheckCell(C.Structure):
    """rc_flowcheck_cell (include/rcflow.h), 32 bytes; numpy: api.FLOWCHECK_CELL_DTYPE."""
    _fields_ = [("flags", C.c_int), ("pixels", C.c_int), ("valid", C.c_int), ("valid_pm", C.c_int), ("mean_x", C.c_float), ("mean_y", C.c_float),
                ("pad", C.c_int * 2)]


class FlowcheckInfo(C.Structure):
    """rc_flowcheck_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", FlowcheckParams), ("launches_per_push", C.c_int), ("held", C.c_int),
                ("pushes", C.c_longlong), ("computing", C.c_longlong), ("device_bytes", C.c_size_t)]


class InfillParams(C.Structure):
    """rc_infill_params (include/rcflow.h), 48 bytes."""
    _fields_ = [("levels", C.c_int), ("min_known", C.c_int), ("hold", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("flags", C.c_int),
                ("pad", C.c_int * 6)]


class InfillCell(C.Structure):
    """rc_infill_cell (include/rcflow.h), 32 bytes; numpy: api.INFILL_CELL_DTYPE."""
    _fields_ = [("flags", C.c_int), ("pixels", C.c_int), ("known_pm", C.c_int), ("valued_pm", C.c_int), ("mean_x", C.c_float), ("mean_y", C.c_float),
                ("mean_level", C.c_float), ("pad", C.c_int)]


class InfillInfo(C.Structure):
    """rc_infill_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", InfillParams), ("launches_per_push", C.c_int), ("pad", C.c_int),
                ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class OffshoreParams(C.Structure):
    """rc_offshore_params (include/rcflow.h), 48 bytes."""
    _fields_ = [("min_dist", C.c_int), ("max_dist", C.c_int), ("stations", C.c_int), ("bins", C.c_int), ("bin_width", C.c_int),
                ("min_count", C.c_int), ("rip_bins", C.c_int), ("cross_min", C.c_float), ("flags", C.c_int), ("pad", C.c_int * 3)]


class OffshoreStation(C.Structure):
    """rc_offshore_station (include/rcflow.h), 48 bytes; numpy: api.OFFSHORE_STATION_DTYPE."""
    _fields_ = [("flags", C.c_int), ("first", C.c_int), ("reach_end", C.c_int), ("peak_bin", C.c_int), ("peak_cross", C.c_int), ("count", C.c_int),
                ("beyond", C.c_int), ("pad0", C.c_int), ("mean_cross", C.c_float), ("mean_along", C.c_float), ("pad1", C.c_int * 2)]


class OffshoreInfo(C.Structure):
    """rc_offshore_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", OffshoreParams), ("launches_per_map", C.c_int), ("launches_per_push", C.c_int),
                ("have_map", C.c_int), ("pad", C.c_int), ("maps", C.c_longlong), ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class OutlinesParams(C.Structure):
    """rc_outlines_params (include/rcflow.h), 32 bytes."""
    _fields_ = [("connectivity", C.c_int), ("min_cracks", C.c_int), ("max_cracks", C.c_int), ("max_loops", C.c_int), ("max_vertices", C.c_int),
                ("flags", C.c_int), ("pad", C.c_int * 2)]


class OutlineLoop(C.Structure):
    """rc_outline_loop (include/rcflow.h), 56 bytes; numpy: api.OUTLINE_LOOP_DTYPE."""
    _fields_ = [("label", C.c_int32), ("flags", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("cracks", C.c_int32), ("verts", C.c_int32),
                ("offset", C.c_int32), ("pad", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("area2", C.c_longlong)]


class OutlinesInfo(C.Structure):
    """rc_outlines_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", OutlinesParams), ("rounds", C.c_int), ("launches_per_push", C.c_int),
                ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class DriftersParams(C.Structure):
    """rc_drifters_params (include/rcflow.h), 40 bytes."""
    _fields_ = [("max_drifters", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("max_age", C.c_int), ("age_bin", C.c_int),
                ("density_full", C.c_int), ("live_min", C.c_int), ("flags", C.c_int), ("dt", C.c_double)]


class DriftersCell(C.Structure):
    """rc_drifters_cell (include/rcflow.h), 32 bytes; numpy: api.DRIFTERS_CELL_DTYPE."""
    _fields_ = [("flags", C.c_int), ("pad0", C.c_int), ("mean_u", C.c_float), ("mean_v", C.c_float), ("escape", C.c_float),
                ("beached", C.c_float), ("mean_exit_age", C.c_float), ("pad1", C.c_int)]


class DriftersInfo(C.Structure):
    """rc_drifters_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", DriftersParams), ("launches_per_push", C.c_int), ("drifters", C.c_int),
                ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class SurfInfo(C.Structure):
    """rc_surf_info (include/rcflow.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("prm", SurfParams), ("lines", C.c_int), ("samples", C.c_int),
                ("launches_per_push", C.c_int), ("held", C.c_int), ("pushes", C.c_longlong), ("device_bytes", C.c_size_t)]


class FitParams(C.Structure):
    """rc_fit_params (include/rcflow.h)."""
    _fields_ = [("model", C.c_int), ("hypotheses", C.c_int), ("seed", C.c_uint), ("min_score", C.c_int),
                ("quality", C.c_double), ("max_shift", C.c_double), ("inlier_px", C.c_double)]


class FitResult(C.Structure):
    """rc_fit_result (include/rcflow.h): 88 bytes on the device."""
    _fields_ = [("T", C.c_double * 9), ("model_used", C.c_int), ("n_valid", C.c_int), ("n_inliers", C.c_int),
                ("winner", C.c_int)]


class StabTracks(C.Structure):
    """rc_stab_tracks (include/rcflow.h)."""
    _fields_ = [("cells_x", C.c_int), ("cells_y", C.c_int), ("min_score", C.c_int), ("quality", C.c_double),
                ("win", C.c_int), ("max_level", C.c_int), ("max_count", C.c_int), ("epsilon", C.c_double),
                ("max_shift", C.c_double), ("model", C.c_int), ("hypotheses", C.c_int), ("seed", C.c_uint),
                ("inlier_px", C.c_double), ("flags", C.c_int)]


_vp, _sz, _i, _f, _d = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_double
_pp = C.POINTER(FarnebackParams)

# name -> argtypes; every symbol include/rcflow.h declares (tests check the export list)
SIGNATURES = {
    "rcflow_create": [C.POINTER(_vp), _i, _i, _i, _i],
    "rcflow_destroy": [_vp],
    "rcflow_abi_version": [],
    "rcflow_last_error": [],
    "rcflow_sync": [_vp, _i],
    "rcflow_set_hip_stream": [_vp, _i, _vp],
    "rcflow_use_own_stream": [_vp, _i],
    "rcflow_set_option": [_vp, C.c_char_p, _i],
    "rcflow_farneback_u8": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _vp, _sz, _d, _i, _i, _i, _i, _d, _i],
    "rcflow_farneback_dev": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _vp, _sz, _pp],
    "rcflow_push_frame_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _pp],
    "rcflow_stream_reset": [_vp, _i],
    "rcflow_push_frame_u8": [_vp, _i, _vp, _sz, _i, _i, _pp],
    "rcflow_frame_buffer_acquire": [_vp, _i, _i, _i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "rcflow_push_frame_acquired": [_vp, _i, _pp],
    "rcflow_stream_flow_ptr": [_vp, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)],
    "rcflow_stream_flow_read": [_vp, _i, _vp, _sz],
    "rcflow_frame_loop_step": [_vp, _i, _pp, C.POINTER(FrameLoop)],
    "rcflow_farneback_clip_dev": [_vp, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _sz, _sz, _pp],
    "rcflow_push_clip_dev": [_vp, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _sz, _sz, _pp],
    "rcflow_push_batch_dev": [_vp, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _sz, _sz, _pp, _i],
    "rcflow_batch_reset": [_vp, _i],
    "rcflow_level_geometry": [_i, _i, _d, _i, _i, C.POINTER(_i), C.POINTER(_i)],
    "rcflow_stage_pyr_level_dev": [_vp, _i, _vp, _sz, _i, _i, _d, _i, _vp],
    "rcflow_stage_polyexp_dev": [_vp, _i, _vp, _i, _i, _i, _d, _vp],
    "rcflow_stage_flow_iter_dev": [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "rcflow_stage_initial_flow_dev": [_vp, _i, _vp, _sz, _i, _i, _d, _i, _vp],
    "rcflow_analysis_reset": [_vp, _i, _i, _i],
    "rcflow_histogram_dev": [_vp, _i, _vp, _sz, _i, _i],
    "rcflow_histogram_clip_dev": [_vp, _i, _vp, _sz, _sz, _i, _i, _i],
    "rcflow_thresholds_dev": [_vp, _i],
    "rcflow_thresholds_words_dev": [_vp, _i, _vp],
    "rcflow_histogram_read": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rcflow_histogram_write": [_vp, _i, _vp],
    "rcflow_histogram_reset_dev": [_vp, _i],
    "rcflow_histogram_device_ptr": [_vp, _i, C.POINTER(_vp)],
    "rcflow_classify_accumulate_dev": [_vp, _i, _vp, _sz, _i, _i, _i, _f, _f, _vp, _sz, _vp, _sz,
                                       _vp, _sz, _vp, _sz],
    "rcflow_accumulator_read": [_vp, _i, _vp],
    "rcflow_advect_field_dev": [_vp, _i, _vp, _sz, _i, _i, _f, _i, _f],
    "rcflow_advect_field_read": [_vp, _i, _vp, _vp],
    "rcflow_advect_points_dev": [_vp, _i, _vp, _i, _vp, _sz, _i, _i, _f, _i, _f, _i, _vp],
    "rcflow_get_delta_field_dev": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _f, _f],
    "rcflow_subtract_average_dev": [_vp, _i, _vp, _sz, _i, _i],
    "rcflow_subtract_mean_magnitude_dev": [_vp, _i, _vp, _sz, _i, _i],
    "rcflow_stabilizer_dev": [_vp, _i, _vp, _sz, _i, _i],
    "rcflow_window_mean_dev": [_vp, _i, _vp, _vp, _vp, _sz, _i],
    "rcflow_vector_to_color_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, C.POINTER(_f)],
    "rcflow_shear_rate_to_color_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, C.POINTER(_f)],
    "rcflow_create_edges_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz],
    "rcflow_create_output_dev": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i],
    "rcflow_resize_bgr_to_gray_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _i, _i],
    "rcflow_resize_area_bgr_to_gray_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _i, _i],
    "rcflow_resize_bgr_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _i, _i],
    "rcflow_resize_area_bgr_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _i, _i],
    "rcflow_phase_correlate_dev": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _i, _vp],
    "rcflow_warp_translate_bgr_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _d, _d],
    "rcflow_framestab_open": [_vp, _i, _i, _i, _i, _i, _i, _i],
    "rcflow_framestab_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp],
    "rcflow_framestab_read": [_vp, _i, C.POINTER(_d), C.POINTER(C.c_longlong)],
    "rcflow_framestab_reset": [_vp, _i],
    "rcflow_framestab_close": [_vp, _i],
    "rcflow_framestab_info": [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                              C.POINTER(C.c_longlong), C.POINTER(_sz)],
    "rcflow_warp_affine_bgr_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _i, _i, C.POINTER(_d), _i],
    "rcflow_warp_perspective_bgr_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz, _i, _i, C.POINTER(_d), _i],
    "rcflow_framestab_open_multi": [_vp, _i, _i, _i, C.POINTER(_i), _i, _i, _d, _i],
    "rcflow_framestab_read_motion": [_vp, _i, C.POINTER(_d), C.POINTER(_i), C.POINTER(_i), C.POINTER(_d), C.POINTER(C.c_longlong)],
    "rcflow_framestab_info_multi": [_vp, _i, C.POINTER(_i), C.POINTER(_i), _i, C.POINTER(_i), C.POINTER(_d), C.POINTER(_i)],
    "rcflow_corners_dev": [_vp, _i, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "rcflow_fit_motion_dev": [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(FitParams), _vp, _vp, _vp],
    "rcflow_framestab_open_tracks": [_vp, _i, _i, _i, C.POINTER(StabTracks)],
    "rcflow_framestab_read_tracks": [_vp, _i, C.POINTER(_d), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _i,
                                     C.POINTER(_i), C.POINTER(C.c_longlong)],
    "rcflow_timex_open": [_vp, _i, _i, _i, _i, _i],
    "rcflow_timex_push_dev": [_vp, _i, _vp, _sz, C.POINTER(_vp), C.POINTER(_sz)],
    "rcflow_timex_reset": [_vp, _i],
    "rcflow_timex_close": [_vp, _i],
    "rcflow_timex_info": [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_longlong),
                          C.POINTER(_sz)],
    "rcflow_ripmap_open": [_vp, _i, _i, _i, _i, _i, _i, _i, _i],
    "rcflow_ripmap_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp],
    "rcflow_ripmap_mean_dev": [_vp, _i, _vp, _sz],
    "rcflow_ripmap_read": [_vp, _i, _vp, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_ripmap_set": [_vp, _i, _d, _d],
    "rcflow_ripmap_reset": [_vp, _i],
    "rcflow_ripmap_close": [_vp, _i],
    "rcflow_ripmap_info": [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                           C.POINTER(_i), C.POINTER(_d), C.POINTER(_d), C.POINTER(C.c_longlong), C.POINTER(_sz)],
    "rcflow_rgb_to_hsv_u8_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz],
    "rcflow_hsv_to_rgb_u8_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz],
    "rcflow_streamline_display_dev": [_vp, _i, _i, _vp, _sz, C.POINTER(_f)],
    "rcflow_streamline_positions_dev": [_vp, _i, _vp, _sz],
    "rcflow_hsv_to_bgr_dev": [_vp, _i, _vp, _sz, _i, _i, _vp, _sz],
    "rcflow_jet_lut": [_vp],
    "rcflow_analysis_size": [_vp, _i, C.POINTER(_i), C.POINTER(_i)],
    "rcflow_pyrlk_dev": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _d, _i, _d],
    "rcflow_pyrlk_u8": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _d, _i, _d],
    "rcflow_pyrlk_levels": [_i, _i, _i, _i, _i],
    "rcflow_draw_dev": [_vp, _i, _vp, _sz, _i, _i, _i, _vp, _i, _vp],
    "rcflow_trace_prims_dev": [_vp, _i, _vp, _vp, _i, _i, C.c_uint32, _vp],
    "rcflow_tracers_open": [_vp, _i, _i, _i, C.POINTER(TracersParams)],
    "rcflow_tracers_add": [_vp, _i, _i, _vp, _i],
    "rcflow_tracers_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz],
    "rcflow_tracers_read": [_vp, _i, _i, _vp, _i, C.POINTER(_i), C.POINTER(C.c_longlong)],
    "rcflow_tracers_prims": [_vp, _i, C.POINTER(_vp), C.POINTER(_i)],
    "rcflow_tracers_info": [_vp, _i, C.POINTER(TracersInfo)],
    "rcflow_tracers_reset": [_vp, _i],
    "rcflow_tracers_close": [_vp, _i],
    "rcflow_regions_open": [_vp, _i, _i, _i, C.POINTER(RegionsParams)],
    "rcflow_regions_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp],
    "rcflow_regions_prims_dev": [_vp, _i, C.c_uint32, _i, _i, _d, _vp],
    "rcflow_regions_read": [_vp, _i, _vp, _i, C.POINTER(_i), _vp],
    "rcflow_regions_set": [_vp, _i, _i],
    "rcflow_regions_reset": [_vp, _i],
    "rcflow_regions_close": [_vp, _i],
    "rcflow_regions_info": [_vp, _i, C.POINTER(RegionsInfo)],
    "rcflow_tracks_open": [_vp, _i, _i, _i, C.POINTER(TracksParams)],
    "rcflow_tracks_push_dev": [_vp, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "rcflow_tracks_prims_dev": [_vp, _i, C.c_uint32, _i, _i, _vp],
    "rcflow_tracks_read": [_vp, _i, _vp, _i, _vp, _vp],
    "rcflow_tracks_info": [_vp, _i, C.POINTER(TracksInfo)],
    "rcflow_tracks_reset": [_vp, _i],
    "rcflow_tracks_close": [_vp, _i],
    "rcflow_motion_open": [_vp, _i, _i, _i, C.POINTER(MotionParams)],
    "rcflow_motion_push_dev": [_vp, _i, _vp, _sz, _d, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp],
    "rcflow_motion_prims_dev": [_vp, _i, C.c_uint32, _i, _i, _d, _vp],
    "rcflow_motion_read": [_vp, _i, _vp, _i, _vp, C.POINTER(C.c_longlong)],
    "rcflow_motion_reset": [_vp, _i],
    "rcflow_motion_close": [_vp, _i],
    "rcflow_motion_info": [_vp, _i, C.POINTER(MotionInfo)],
    "rcflow_ftle_open": [_vp, _i, _i, _i, C.POINTER(FtleParams)],
    "rcflow_ftle_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp],
    "rcflow_ftle_read": [_vp, _i, C.POINTER(C.c_longlong)],
    "rcflow_ftle_set": [_vp, _i, _d, _d],
    "rcflow_ftle_reset": [_vp, _i],
    "rcflow_ftle_close": [_vp, _i],
    "rcflow_ftle_info": [_vp, _i, C.POINTER(FtleInfo)],
    "rcflow_planview_open": [_vp, _i, _i, _i, C.POINTER(PlanViewParams)],
    "rcflow_planview_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp],
    "rcflow_planview_read": [_vp, _i, C.POINTER(C.c_longlong)],
    "rcflow_planview_table_read": [_vp, _i, _vp],
    "rcflow_planview_reset": [_vp, _i],
    "rcflow_planview_close": [_vp, _i],
    "rcflow_planview_info": [_vp, _i, C.POINTER(PlanViewInfo)],
    "rcflow_waves_open": [_vp, _i, _i, _i, C.POINTER(WavesParams)],
    "rcflow_waves_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp],
    "rcflow_waves_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_waves_spectrum_read": [_vp, _i, _vp],
    "rcflow_waves_table_read": [_vp, _i, _vp, _vp],
    "rcflow_waves_set": [_vp, _i, C.c_double, _i, C.c_double],
    "rcflow_waves_reset": [_vp, _i],
    "rcflow_waves_close": [_vp, _i],
    "rcflow_waves_info": [_vp, _i, C.POINTER(WavesInfo)],
    "rcflow_piv_open": [_vp, _i, _i, _i, C.POINTER(PivParams)],
    "rcflow_piv_push_dev": [_vp, _i, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp],
    "rcflow_piv_read": [_vp, _i, _vp, C.POINTER(C.c_longlong)],
    "rcflow_piv_sums_read": [_vp, _i, _vp, _vp],
    "rcflow_piv_set": [_vp, _i, C.c_double, C.c_double, C.c_double, C.c_double],
    "rcflow_piv_reset": [_vp, _i],
    "rcflow_piv_close": [_vp, _i],
    "rcflow_piv_info": [_vp, _i, C.POINTER(PivInfo)],
    "rcflow_transects_plan": [_i, _i, C.POINTER(TransectLine), _i, C.c_double, C.c_double, _vp, _vp, C.POINTER(C.c_int)],
    "rcflow_transects_open": [_vp, _i, _i, _i, C.POINTER(TransectLine), _i, C.POINTER(TransectsParams)],
    "rcflow_transects_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp],
    "rcflow_transects_read": [_vp, _i, _vp, C.POINTER(C.c_longlong)],
    "rcflow_transects_sums_read": [_vp, _i, _vp, _vp],
    "rcflow_transects_table_read": [_vp, _i, _vp, _vp],
    "rcflow_transects_set": [_vp, _i, C.c_double, C.c_double],
    "rcflow_transects_reset": [_vp, _i],
    "rcflow_transects_close": [_vp, _i],
    "rcflow_transects_info": [_vp, _i, C.POINTER(TransectsInfo)],
    "rcflow_kinematics_taps": [_i, _d, C.POINTER(C.c_float)],
    "rcflow_kinematics_open": [_vp, _i, _i, _i, C.POINTER(KinematicsParams)],
    "rcflow_kinematics_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp],
    "rcflow_kinematics_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_kinematics_set": [_vp, _i, _d, _d, _d, _d],
    "rcflow_kinematics_reset": [_vp, _i],
    "rcflow_kinematics_close": [_vp, _i],
    "rcflow_kinematics_info": [_vp, _i, C.POINTER(KinematicsInfo)],
    "rcflow_shoreline_plan": [_i, _i, C.POINTER(TransectLine), _i, C.c_double, _vp, _vp, C.POINTER(C.c_int)],
    "rcflow_shoreline_open": [_vp, _i, _i, _i, C.POINTER(TransectLine), _i, C.POINTER(ShorelineParams)],
    "rcflow_shoreline_push_dev": [_vp, _i, _vp, _sz, _i, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp],
    "rcflow_shoreline_prims_dev": [_vp, _i, C.c_uint32, _i, _i, _vp],
    "rcflow_shoreline_read": [_vp, _i, _vp, C.POINTER(C.c_longlong)],
    "rcflow_shoreline_ring_read": [_vp, _i, _vp],
    "rcflow_shoreline_table_read": [_vp, _i, _vp, _vp],
    "rcflow_shoreline_set": [_vp, _i, _i, _d, _d],
    "rcflow_shoreline_reset": [_vp, _i],
    "rcflow_shoreline_close": [_vp, _i],
    "rcflow_shoreline_info": [_vp, _i, C.POINTER(ShorelineInfo)],
    "rcflow_surf_plan": [_i, _i, C.POINTER(TransectLine), _i, C.c_double, _vp, _vp, C.POINTER(C.c_int)],
    "rcflow_surf_open": [_vp, _i, _i, _i, C.POINTER(TransectLine), _i, C.POINTER(SurfParams)],
    "rcflow_surf_push_dev": [_vp, _i, _vp, _sz, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp],
    "rcflow_surf_prims_dev": [_vp, _i, C.c_uint32, _i, _i, _vp],
    "rcflow_surf_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_surf_table_read": [_vp, _i, _vp, _vp],
    "rcflow_surf_set": [_vp, _i, _i, _i, _i, _i, _i, _i],
    "rcflow_surf_reset": [_vp, _i],
    "rcflow_surf_close": [_vp, _i],
    "rcflow_surf_info": [_vp, _i, C.POINTER(SurfInfo)],
    "rcflow_meanflow_open": [_vp, _i, _i, _i, C.POINTER(MeanflowParams)],
    "rcflow_meanflow_push_dev": [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp],
    "rcflow_meanflow_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_meanflow_set": [_vp, _i, _i, C.c_double, C.c_double, C.c_double, C.c_double, _i],
    "rcflow_meanflow_reset": [_vp, _i],
    "rcflow_meanflow_close": [_vp, _i],
    "rcflow_meanflow_info": [_vp, _i, C.POINTER(MeanflowInfo)],
    "rcflow_flowcheck_open": [_vp, _i, _i, _i, C.POINTER(FlowcheckParams)],
    "rcflow_flowcheck_push_dev": [_vp, _i] + [_vp, _sz] * 10 + [_vp, _vp, _vp],
    "rcflow_flowcheck_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_flowcheck_set": [_vp, _i, _i, _i, C.c_double, _i, C.c_double, C.c_double, C.c_double],
    "rcflow_flowcheck_reset": [_vp, _i],
    "rcflow_flowcheck_close": [_vp, _i],
    "rcflow_flowcheck_info": [_vp, _i, C.POINTER(FlowcheckInfo)],
    "rcflow_drifters_open": [_vp, _i, _i, _i, C.POINTER(DriftersParams)],
    "rcflow_drifters_seed": [_vp, _i, C.POINTER(C.c_double), _i],
    "rcflow_drifters_push_dev": [_vp, _i] + [_vp, _sz] * 6 + [_vp] * 8,
    "rcflow_drifters_read": [_vp, _i, _vp, _vp, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_drifters_set": [_vp, _i, C.c_double, _i, _i, _i, _i],
    "rcflow_drifters_reset": [_vp, _i],
    "rcflow_drifters_close": [_vp, _i],
    "rcflow_drifters_info": [_vp, _i, C.POINTER(DriftersInfo)],
    "rcflow_drifters_zones_dev": [_vp, _i, _vp, _sz, _vp, _sz, _i, _i, _vp, _sz],
    "rcflow_infill_open": [_vp, _i, _i, _i, C.POINTER(InfillParams)],
    "rcflow_infill_push_dev": [_vp, _i] + [_vp, _sz] * 7 + [_vp, _vp, _vp],
    "rcflow_infill_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong)],
    "rcflow_infill_set": [_vp, _i, _i, _i, _i],
    "rcflow_infill_reset": [_vp, _i],
    "rcflow_infill_close": [_vp, _i],
    "rcflow_infill_info": [_vp, _i, C.POINTER(InfillInfo)],
    "rcflow_offshore_open": [_vp, _i, _i, _i, C.POINTER(OffshoreParams)],
    "rcflow_offshore_map_dev": [_vp, _i] + [_vp, _sz] * 5 + [_vp],
    "rcflow_offshore_push_dev": [_vp, _i] + [_vp, _sz] * 5 + [_vp, _vp, _vp],
    "rcflow_offshore_band_dev": [_vp, _i, C.c_float, C.c_float, _vp, _sz],
    "rcflow_offshore_read": [_vp, _i, _vp, _vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)],
    "rcflow_offshore_set": [_vp, _i, C.POINTER(OffshoreParams)],
    "rcflow_offshore_reset": [_vp, _i],
    "rcflow_offshore_close": [_vp, _i],
    "rcflow_offshore_info": [_vp, _i, C.POINTER(OffshoreInfo)],
    "rcflow_outlines_open": [_vp, _i, _i, _i, C.POINTER(OutlinesParams)],
    "rcflow_outlines_push_dev": [_vp, _i] + [_vp, _sz] * 2 + [_vp, _vp, _vp],
    "rcflow_outlines_prims_dev": [_vp, _i, C.c_uint32, _i, _vp],
    "rcflow_outlines_read": [_vp, _i, _vp, _i, C.POINTER(_i), _vp, _i, C.POINTER(_i), C.POINTER(C.c_longlong)],
    "rcflow_outlines_set": [_vp, _i, _i],
    "rcflow_outlines_reset": [_vp, _i],
    "rcflow_outlines_close": [_vp, _i],
    "rcflow_outlines_info": [_vp, _i, C.POINTER(OutlinesInfo)],
    "rcflow_comm_unique_id": [_vp],
    "rcflow_comm_init": [_vp, _vp, _i, _i],
    "rcflow_comm_destroy": [_vp],
    "rcflow_comm_rank": [_vp, C.POINTER(_i), C.POINTER(_i)],
    "rcflow_allreduce_hist": [_vp, _i, _vp],
    "rcflow_allreduce_hist_join": [_vp, _i],
    "rcflow_allreduce_hist_status": [_vp, C.POINTER(C.c_longlong)],
    "rcflow_allreduce_hist_result": [_vp, C.POINTER(_vp)],
    "rcflow_profile_enable": [_vp, _i],
    "rcflow_profile_reset": [_vp],
    "rcflow_profile_read_buckets": [_vp, C.POINTER(C.c_char_p), C.POINTER(_d)],
    "rcflow_profile_read": [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(_i), C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)],
}

# diagnostics librcflow.so exports beside the interface of include/rcflow.h (the test hooks of rcflow_api.hip that take a
# context): name -> argtypes
DEBUG_SIGNATURES = {
    "rcflow_debug_level_R": [_vp, _i, _i, _i, _vp, C.POINTER(_i), C.POINTER(_i)],
    "rcflow_debug_level_image": [_vp, _i, _i, _i, _vp, C.POINTER(_i), C.POINTER(_i)],
}

# diagnostics of the flow iteration (tests/test_gpu_flow_forms.py): the copy form of rcflow_debug_level_flow_ptr, which takes a
# context, and the host-only form function, which takes none
DEBUG_FLOW_SIGNATURES = {
    "rcflow_debug_level_flow": [_vp, _i, _i, _i, _i, _vp, C.POINTER(_i), C.POINTER(_i)],
    "rcflow_debug_flow_form": [_i] * 11 + [C.POINTER(_i), _i],
}
# RcFlowKernel of csrc/rc_common.h (tests/test_cabi_and_host.py compares the two)
FLOW_KERNELS = {1: "w3", 2: "tile", 3: "big", 4: "sweep", 5: "runtime", 6: "rrc"}

_LIB = None


def load():
    """Loads librcflow.so; raises if the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "librcflow.so is missing at %s: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.argtypes = args
        fn.restype = C.c_char_p if name == "rcflow_last_error" else C.c_int
    lib.rcflow_destroy.restype = None
    for name, args in list(DEBUG_SIGNATURES.items()) + list(DEBUG_FLOW_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    _LIB = lib
    return lib


def check(rc):
    if rc < 0:
        raise RcflowError(rc, (load().rcflow_last_error() or b"").decode())
    return rc
