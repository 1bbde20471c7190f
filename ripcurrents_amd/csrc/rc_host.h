// rc_host.h -- host-side context, plans and stream slots of librcflow (internal).
#pragma once

#include <initializer_list>
#include <string>
#include <vector>

#include "rc_args.h"
#include "rc_common.h"

struct RcBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct RcPlan {
    bool valid = false;
    int w = 0, h = 0;
    rc_farneback_params prm{};
    int nlev = 0;  // number of scales = cropped levels + 1
    RcLevel lv[RC_MAX_LEVELS];
    size_t kern_off[RC_MAX_LEVELS];
    RcPolyK pk;
    RcWindow win;
    int nslots = 0, chunk = 0;
    int exact_taps = 0;
    int exact = 0;
    RcFlowAreaArgs seed;   // RC_FARNEBACK_USE_INITIAL_FLOW: reduction of the initial field to the coarsest scale (tables in RcSlot::seed_tab)
};

// Device-resident analysis state of one stream slot (ripcurrents.cpp:133-176).
struct RcAnalysis {
    int w = 0, h = 0;
    RcBuf hist;        // RC_HIST_WORDS int32
    long long hist_added = 0;   // pixels passed to the histogram since the last reset (upper bound of histsum)
    RcBuf hist_part;   // partial hist2d tables of the histogram kernel
    RcBuf thr;         // UPPER | UPPER2d[36] | prop[36] floats (+1 pad)
    RcBuf acc;         // h*w float accumulator (.x channel of the reference's 32FC3)
    RcBuf pt;          // h*w float2 streamlines_mat
    RcBuf dist;        // h*w float streamlines_distance
    RcBuf scratch;     // reductions
    RcBuf jet;         // COLORMAP_JET LUT (768 B) + the display maximum key
    RcBuf loopc;       // one int32: framecount of rcflow_frame_loop_step (incremented on the device)
};

// lk_kernels.hip: the two halves of a PyrLK call (pyramid of one image; track), for the tracking stabiliser
struct RcLkPyr {
    int top; bool deriv;
    int lw[8], lh[8];
    size_t offI[8], offD[8], bytes;
};

// open / reset zero a product's state asynchronously on the stream the slot has then; whoever touches the state next
// waits for this event when the slot has been moved to another stream in between (rcflow_set_hip_stream)
struct RcZeroFence {
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;
    bool pending = false;
};

// Time-exposure state of one stream slot (timex_kernels.hip; main.cpp:1195-1383).  Everything is allocated by
// rcflow_timex_open and released by rcflow_timex_close / rcflow_destroy.
struct RcTimex {
    bool open = false;
    int w = 0, h = 0, window = 0, products = 0;   // window = 0: MEAN alone, no ring
    int pitch = 0;            // row pitch of the state planes in pixels (w rounded up to 4)
    size_t plane = 0;         // pixels per state plane
    int cur = 0;              // ring slot the next frame goes to (currentBuffer, main.cpp:1290)
    long long frames = 0;     // frames pushed since open / reset (framecount, main.cpp:1219)
    RcBuf sum;                // MEAN: [h][pitch][3] fp32 (sum_rgb, main.cpp:1216)
    RcBuf ring;               // [window][H, S, V][plane] bytes (buffer_hsv, main.cpp:1292-1295)
    RcBuf avg;                // AVERAGE: [H, S, V][plane] uint16 sums of the slots' quotients
    RcBuf bd_idx[2], bd_hsv[2];   // BRIGHT, DARK: the winner's slot (uint16) and output triple (uint32) per pixel
    RcZeroFence zf;
};

// Frame stabilisation state of one stream slot (stab_kernels.hip; main.cpp:1684-1775).  Everything is allocated by
// rcflow_framestab_open and released by rcflow_framestab_close / rcflow_destroy.
struct RcFrameStab {
    bool open = false;
    int w = 0, h = 0;               // frame size
    int rx = 0, ry = 0, rw = 0, rh = 0;   // the tracked patch (roi, main.cpp:1728-1732)
    int N = 0, M = 0;               // optimal DFT sizes of the patch columns, rows
    size_t lds = 0;                 // LDS bytes of the one-workgroup correlate; 0: a launch per pass over `scratch`
    long long frames = 0;           // frames pushed since open / reset
    RcBuf tab;                      // Hann window [rh][rw] | twiddles of N | twiddles of M (float)
    RcBuf prev;                     // [rh][rw] float: gray ROI of the last CORRECTED frame (prev, main.cpp:1759)
    RcBuf res;                      // 3 doubles: shift_x, shift_y, response of the last push
    RcBuf scratch;                  // spectra of the launch-per-pass form
    RcZeroFence zf;
    // rcflow_framestab_open_multi (n = 0: the single-patch slot above).  The patches share rw x rh, tab and the LDS
    // plan; prev holds n patches; res holds RC_FS_* doubles: result | motion | used | ticket | the n shifts
    int n = 0, model = 0, flags = 0;
    double min_response = 0.;
    int px[RC_STAB_MAX_PATCHES] = {}, py[RC_STAB_MAX_PATCHES] = {};
    // rcflow_framestab_open_tracks (tracks = false: one of the two forms above).  res holds RC_FT_* doubles
    bool tracks = false;
    rc_stab_tracks tp{};            // the parameters with every default resolved
    int ncells = 0, margin = 0;
    RcLkPyr ref{}, cur{};           // pyramid plans: the reference frame (with derivatives), the incoming frame
    RcBuf lkref, lkcur;             // their bytes
    RcBuf trk;                      // corners [2][ncells] float2 | tracks | scores [2][ncells] int | status | inlier (stab_kernels.hip)
    int pcur = 0; bool pflip = false;   // the corner slot in use; a chained push left the next corners in the other one
};
// layout of RcFrameStab::res for a tracks slot, in doubles: the result of rcflow_framestab_read, rc_fit_result, the fit's two words
enum { RC_FT_RESULT = 0 /* 3 */, RC_FT_FIT = 4 /* 11 */, RC_FT_WS = 16 /* 2 */, RC_FT_DOUBLES = 18 };
// layout of RcFrameStab::res for a multi-patch slot, in doubles
enum { RC_FS_RESULT = 0 /* 3 */, RC_FS_MOTION = 3 /* 6 */, RC_FS_USED = 9 /* int model_used, patches_used */,
       RC_FS_TICKET = 10 /* unsigned arrivals of the running correlate launch */, RC_FS_SHIFTS = 16 /* n x 3 */ };

// Opposing-flow map of one stream slot (ripmap_kernels.hip; averageVector, ripcurrents_module.cpp:386-484).  Everything is
// allocated by rcflow_ripmap_open and released by rcflow_ripmap_close / rcflow_destroy.
struct RcRipMap {
    bool open = false;
    int w = 0, h = 0, window = 0, gx = 0, gy = 0, source = 0, flags = 0;
    int pitch = 0;            // row pitch of ring and mean in pixels (w rounded up to 2: 16-byte rows)
    int cur = 0;              // ring slot the next field goes to
    long long frames = 0;     // fields pushed since open / reset
    double K = 0.3454915028125263;   // min_opposition_cos2: cos^2(0.7 pi), ripcurrents_module.cpp:471
    double M = 0.;            // min_cell_mag
    RcBuf ring;               // [window][h][pitch] float2
    RcBuf avg;                // [h][pitch] float2: the window mean
    RcBuf acc;                // RmCtl | [gy][gx][Sx, Sy, n] int64, zero between launches
    RcBuf out;                // the last push: cells [cells] float4 | sums [cells][3] int64 | summary 8 doubles
    RcZeroFence zf;
};

// Tracer lines of one stream slot (tracer_kernels.hip; Streakline.cpp:22-71, ripcurrents_module.cpp:751-807, :1140-1196).
// Everything is allocated by rcflow_tracers_open and released by rcflow_tracers_close / rcflow_destroy.  The vertices of
// all lines lie compacted, line after line, a streakline oldest first; the host knows every count: a streakline of age a
// (moves since it was added or the session was reset) has min(cap, 1 + a) vertices.
struct RcTrLineH { int kind, cap, n0; long long t_add; };
struct RcTracers {
    bool open = false;
    int w = 0, h = 0;
    rc_tracers_params prm{};        // every default resolved, the LK criteria as SparsePyrLKOpticalFlowImpl::calc clamps them
    std::vector<RcTrLineH> lines;
    int reserved = 0;               // points the lines may grow to (a streakline: max_vertices), <= prm.max_points
    int init_n = 0;                 // points in `init`
    int cur = 0;                    // which half of pos holds the vertices
    long long t = 0, t_reset = 0;   // moves since open; at the last reset
    long long dropped = 0;
    bool primed = false; int pyr_cur = 0;   // LK mover: pyr[pyr_cur] holds the previous frame
    int nprims = 0;                 // of the last push
    RcLkPyr plan{};
    RcBuf pyr;                      // LK mover: two pyramids with derivatives
    RcBuf pos;                      // P[2] | Q[2], max_points float2 each: the vertices; moved (LK) / the copy the advection moves (FLOW)
    RcBuf init;                     // the lines as they were added, compacted: what reset restores
    RcBuf tab;                      // max_lines TrLine records
    RcBuf prims;                    // 2 max_points + max_lines records
    RcBuf status;                   // LK mover: max_points bytes nobody reads (ripcurrents_module.cpp:794)
    RcBuf ctr;                      // one uint64: primitives skipped
    RcZeroFence zf;
};

// Rip regions of one stream slot (region_kernels.hip): connected components of a mask, numbered in raster order, filtered
// and measured.  Everything is allocated by rcflow_regions_open and released by rcflow_regions_close / rcflow_destroy.
struct RcRegions {
    bool open = false;
    int w = 0, h = 0;
    rc_regions_params prm{};        // min_area: as rcflow_regions_set left it
    long long pushes = 0;           // since open / reset
    RcBuf par;                      // [h * w] int32: the union-find's parent, -1 for background; after a push every pixel's root
    RcBuf area;                     // [h * w] int32: a root's area, then its kept number
    RcBuf rows;                     // per row: kept roots, roots, foreground pixels, largest kept area (int32 [4][h]) | kept pixels (int64 [h])
    RcBuf acc;                      // RgCtl | max_regions RgAcc: the sums the statistics launch adds into
    RcBuf out;                      // the last push: 8 int64 summary | max_regions rc_region
    RcZeroFence zf;
};

// Rip tracks of one stream slot (track_kernels.hip): the regions of rcflow_regions_push_dev followed from push to push.
// Everything is allocated by rcflow_tracks_open and released by rcflow_tracks_close / rcflow_destroy.
struct RcTracks {
    bool open = false;
    int w = 0, h = 0;
    rc_tracks_params prm{};
    long long pushes = 0;           // calls since open / reset, for rcflow_tracks_info; the kernels count in aux
    RcBuf foot;                     // [h * w] int32: slot + 1 of the track that last covered the pixel, or 0
    RcBuf ov;                       // [max_regions + 1][max_tracks] int32: the overlap table, zeroed by every push
    RcBuf aux;                      // TkCtl (next_id - 1, pushes) | the per-label and per-slot words between the launches (TkTabs)
    RcBuf out;                      // the last push: 8 int64 summary | max_tracks rc_track, the table itself
    RcZeroFence zf;
};

// Motion templates of one stream slot (motion_kernels.hip; globalOrientation, ripcurrents_module.cpp:319-359).  Everything is
// allocated by rcflow_motion_open and released by rcflow_motion_close / rcflow_destroy.
struct RcMotion {
    bool open = false;
    int w = 0, h = 0;
    rc_motion_params prm{};         // deltas in order
    int pitch = 0;                  // row pitch of the state planes in pixels (w rounded up to 4)
    long long pushes = 0;           // since open / reset; 0: no previous frame is held
    double last_ts = 0.;            // the last push's stamp
    RcBuf mhi;                      // [h][pitch] float: the history
    RcBuf prev;                     // [h][pitch] bytes: the last gray frame
    RcBuf orient;                   // [h][pitch] float, 0 where the mask is
    RcBuf mask;                     // [h][pitch] bytes, 255 / 0
    RcBuf tab;                      // MtCtl | per cell: 16 words of counts | per set: MtInfo | per set: S, W, n_used int64 (zero between pushes)
    RcBuf out;                      // the last push: cells + 1 records rc_motion_cell (the frame's last) | the silhouette's pixels (int64)
    RcZeroFence zf;
};

// Flow map and FTLE of one stream slot (ftle_kernels.hip).  Everything is allocated by rcflow_ftle_open and released by
// rcflow_ftle_close / rcflow_destroy.
struct RcFtle {
    bool open = false;
    int w = 0, h = 0;
    rc_ftle_params prm{};           // threshold and vis_max: as rcflow_ftle_set left them
    int pitch = 0;                  // row pitch of the ring in pixels (w rounded up to 2: 16-byte rows)
    int cur = 0;                    // ring slot the next field goes to
    long long pushes = 0;           // since open / reset; min(pushes, window) fields are held
    RcBuf ring;                     // [window][h][pitch] float2
    RcBuf map;                      // [h][w] float2: the displacement of the particle that started at the pixel
    RcBuf steps;                    // [h][w] int32: the fields it passed through
    RcBuf lam;                      // [h][w] float: the largest eigenvalue of the Cauchy-Green tensor, 0 where not valid
    RcBuf ctl;                      // FtCtl: the ticket and the counters, zero between launches
    RcBuf out;                      // the last computing push: 8 int64 summary
    RcBuf jet;                      // COLORMAP_JET LUT (768 B), written once by open
    RcZeroFence zf;
};

// Plan view of one stream slot (planview_kernels.hip).  Everything is allocated by rcflow_planview_open and released by
// rcflow_planview_close / rcflow_destroy.
struct RcPlanView {
    bool open = false;
    int w = 0, h = 0;               // the image: the field's and the frame's size
    rc_planview_params prm{};
    long long pushes = 0;           // since open / reset
    RcBuf table;                    // [ny][nx] records of eight floats: U, V, m00, m01, m10, m11, gsd, 1; written once by open
    RcBuf ctl;                      // PvCtl: the ticket and the counters, zero between launches
    RcBuf out;                      // the last push: 8 int64 summary
    RcZeroFence zf;
};

// Wave spectra of one stream slot (waves_kernels.hip).  Everything is allocated by rcflow_waves_open and released by
// rcflow_waves_close / rcflow_destroy.
struct RcWaves {
    bool open = false;
    int w = 0, h = 0;
    rc_waves_params prm{};          // tanh_max, min_pixels and vis_max_depth: as rcflow_waves_set left them
    int K = 0;                      // bins
    int pitch = 0;                  // row pitch of ring and accumulators in pixels (w rounded up to 4: 4-byte and 32-byte groups)
    int sh = 0;                     // the shift that brings an accumulator below 2^15
    long long pushes = 0;           // since open / reset; the next frame goes to ring slot pushes mod window
    std::vector<int> tc, ts;        // the twiddle table, built by open in double
    RcBuf ring;                     // [window][h][pitch] bytes
    RcBuf acc;                      // [K][h][pitch] int2 (re, im)
    RcBuf cacc;                     // WvCtl | [cells][K][6] int64 the cells launch adds into, zero between launches
    RcBuf out;                      // the last computing push: records [cells] | sums [cells][K][6] int64 | summary 8 int64
    RcBuf jet;                      // COLORMAP_JET LUT (768 B), written once by open
    RcZeroFence zf;
};

// Ensemble PIV of one stream slot (piv_kernels.hip).  Everything is allocated by rcflow_piv_open and released by
// rcflow_piv_close / rcflow_destroy.
struct RcPiv {
    bool open = false;
    int w = 0, h = 0;
    rc_piv_params prm{};            // min_peak, median_eps, median_thr and vis_max: as rcflow_piv_set left them
    int gx = 0, gy = 0;             // the cell grid
    int nw = 0;                     // words per cell: 3 D^2 (Tab, Tb, Tbb per displacement) + 2 (Ta, Taa)
    int pitch = 0;                  // row pitch of the previous frame in pixels (w rounded up to 4)
    long long pushes = 0;           // since open / reset; pushes - 1 pairs have been correlated
    RcBuf prev;                     // [h][pitch] bytes: the last pushed frame
    RcBuf ring;                     // [ensemble][cells][nw] int32: the per-pair sums; not allocated for an ensemble of 1
    RcBuf acc;                      // [cells][nw] int64: the sums over the last min(pairs, ensemble) pairs
    RcBuf out;                      // the last computing push: records before validation [cells] | records [cells] | summary 8 int64
    RcBuf ctl;                      // PvCtl: the ticket and the counters, zero between launches
    RcBuf jet;                      // COLORMAP_JET LUT (768 B), written once by open
    RcZeroFence zf;
};

// Transects of one stream slot (transects_kernels.hip).  Everything is allocated by rcflow_transects_open and released by
// rcflow_transects_close / rcflow_destroy.
struct RcTransects {
    bool open = false;
    int w = 0, h = 0;
    rc_transects_params prm{};      // jet_min and vis_max: as rcflow_transects_set left them
    int L = 0, S = 0;               // lines, samples in all
    int nw = 0;                     // words per line: 3 (2 D + 1) (Tab, Tb, Tbb per shift) + 2 (Ta, Taa)
    long long pushes = 0;           // since open / reset; the next row goes to ring slot pushes mod window
    RcBuf table;                    // [S] rc_transect_sample | [L] rc_transect_geom, written once by open
    RcBuf ring_g;                   // [window][S] bytes; GRAY
    RcBuf ring_f;                   // [window][S] float2 (ut, un); FLOW
    RcBuf acc;                      // [L][nw] int64: the sums over the pairs the ring holds
    RcBuf out;                      // the last computing push: records [L] | sums [L][RC_TRANSECTS_SUMS] int64 | summary 8 int64
    RcBuf ctl;                      // TsCtl: the ticket and the counters, zero between launches
    RcBuf jet;                      // COLORMAP_JET LUT (768 B), written once by open
    RcZeroFence zf;
};

// Flow kinematics of one stream slot (kinematics_kernels.hip).  Everything is allocated by rcflow_kinematics_open and released
// by rcflow_kinematics_close / rcflow_destroy.
struct RcKinematics {
    bool open = false;
    int w = 0, h = 0;
    rc_kinematics_params prm{};     // ow_k, ow_min, omega_min and vis_max: as rcflow_kinematics_set left them
    float taps[RC_KINEMATICS_MAX_RADIUS + 1] = {};
    long long pushes = 0;           // since open / reset
    RcBuf planes;                   // [2][h][w] float between the launches: omega (one NaN pattern where the pixel is not valid) | ow
    RcBuf acc;                      // [cells][RC_KINEMATICS_SUMS] int64 the launches add into, zero between pushes
    RcBuf out;                      // the last computing push: summary 8 int64 | sums [cells][RC_KINEMATICS_SUMS] int64 | records [cells]
    RcBuf ctl;                      // KnCtl: the tickets, the largest |omega| and T2, zero between pushes
    RcBuf jet;                      // COLORMAP_JET LUT (768 B), written once by open
    RcZeroFence zf;
};

// Shoreline of one stream slot (shoreline_kernels.hip).  Everything is allocated by rcflow_shoreline_open and released by
// rcflow_shoreline_close / rcflow_destroy.
struct RcShoreline {
    bool open = false;
    int w = 0, h = 0;
    rc_shoreline_params prm{};      // threshold, min_sep and max_jump: as rcflow_shoreline_set left them
    int L = 0, S = 0;               // lines, samples in all
    long long pushes = 0;           // since open / reset; the next position goes to ring slot pushes mod window
    RcBuf table;                    // [S] rc_transect_sample | [L] rc_transect_geom, written once by open
    RcBuf plane;                    // [h][w] uint16: J, written by every push before it is read
    RcBuf ring;                     // [L][window] int32: a line's positions, -1 for none
    RcBuf lin;                      // [L] ShLine: what shoreline@1 hands to shoreline@2
    RcBuf out;                      // the last push: records [L] | summary 8 int64 | histogram RC_SHORE_HIST uint32
    RcBuf ctl;                      // ShCtl: the tickets, the counters and the live histogram (zero between launches), thr, N and eta
    RcZeroFence zf;
};

// Surf zone of one stream slot (surf_kernels.hip).  Everything is allocated by rcflow_surf_open and released by
// rcflow_surf_close / rcflow_destroy.
struct RcSurf {
    bool open = false;
    int w = 0, h = 0;
    rc_surf_params prm{};           // bright, delta, q_min, ratio, min_load and vis_permille: as rcflow_surf_set left them
    int L = 0, S = 0;               // lines, samples in all
    int P = 0, tiles = 0;           // row pitch of the state planes in pixels (w rounded up to 4); runs of 256 pixels in P h
    long long pushes = 0;           // since open / reset; the next frame goes to ring slot pushes mod window
    RcBuf table;                    // [S] rc_transect_sample | [L] rc_transect_geom, written once by open
    RcBuf ring;                     // [window][h][P] bytes: the grey frames
    RcBuf bits;                     // [window][tiles][4] uint64: the flags, word k of a tile holds pixel 4 lane + k in bit `lane`
    RcBuf sums;                     // S1 [h][P] uint32 | S2 [h][P] uint32 | Q [h][P] uint16
    RcBuf out;                      // the last push: summary 8 int64 | channels [RC_SURF_MAX_CHANNELS] | lines [L]
    RcBuf ctl;                      // SfCtl: the ticket, the last surf@0's counts, every block's counts
    RcBuf jet;                      // COLORMAP_JET, 768 bytes
    RcZeroFence zf;
};

// Mean current of one stream slot (meanflow_kernels.hip).  Everything is allocated by rcflow_meanflow_open and released by
// rcflow_meanflow_close / rcflow_destroy.
struct RcMeanflow {
    bool open = false;
    int w = 0, h = 0;
    rc_meanflow_params prm{};       // steady_min, speed_min, min_cos2, dir_x, dir_y and min_fill: as rcflow_meanflow_set left them
    int P = 0;                      // row pitch of the state planes in pixels (w rounded up to 4)
    long long pushes = 0;           // since open / reset; the next sample goes to ring slot pushes mod window
    RcBuf ring;                     // [window][h][P] uint32: u | v << 16 in 1/64 pixel, 0x8000 for a bad sample; not read before it has wrapped
    RcBuf sums;                     // Suu | Svv | Suv [h][P] int64 | Su | Sv [h][P] int32 | Sm [h][P] uint32 | n [h][P] uint16
    RcBuf acc;                      // [cells][RC_MEANFLOW_SUMS] int64 the launches add into, zero between pushes
    RcBuf out;                      // the last push: summary 8 int64 | sums [cells][RC_MEANFLOW_SUMS] int64 | records [cells]
    RcBuf ctl;                      // MfCtl: the tickets and G
    RcBuf jet;                      // COLORMAP_JET, 768 bytes
    RcZeroFence zf;
};

// Flow check of one stream slot (flowcheck_kernels.hip).  Everything is allocated by rcflow_flowcheck_open and released by
// rcflow_flowcheck_close / rcflow_destroy.
struct RcFlowcheck {
    bool open = false;
    int w = 0, h = 0;
    rc_flowcheck_params prm{};      // tests and the thresholds: as rcflow_flowcheck_set left them
    bool held = false;              // `prev` holds the d_next of the push before
    long long pushes = 0, computing = 0;      // since open; a reset keeps them
    RcBuf prev;                     // [h][w] uint8, dense: the held frame
    RcBuf acc;                      // [cells][RC_FLOWCHECK_SUMS] int64 the launch adds into, zero between pushes
    RcBuf out;                      // the last computing push: summary 10 int64 (a line) | sums [cells][RC_FLOWCHECK_SUMS] int64 | records [cells]
    RcZeroFence zf;
};

// Virtual drifters of one stream slot (drifters_kernels.hip).  Everything is allocated by rcflow_drifters_open and released by
// rcflow_drifters_close / rcflow_destroy.
struct RcDrifters {
    bool open = false;
    int w = 0, h = 0;
    rc_drifters_params prm{};       // dt, max_age, density_full, live_min and the RESPAWN bit: as rcflow_drifters_set left them
    int P = 0;                      // row pitch of the occupancy and density planes in pixels (w rounded up to 4)
    int n = 0;                      // drifters seeded; a reset keeps them
    long long pushes = 0;           // since open / reset
    RcBuf st;                       // HX | HY | X | Y | age | st, [max_drifters] int32 each: 24 bytes a drifter
    RcBuf occ;                      // [h][P] uint32: the occupancy of the push under way, zero between pushes
    RcBuf dens;                     // [h][P] uint32: the visit density
    RcBuf tab;                      // by place | by origin, [cells][RC_DRIFTERS_SUMS] int64 each, since open / reset
    RcBuf stat;                     // the summary's cumulative words, RC_DRIFTERS_SUMMARY int64 | the histograms [4][RC_DRIFTERS_HIST_BINS] uint64
    RcBuf out;                      // the last push: summary RC_DRIFTERS_SUMMARY int64 | records [cells]
    RcBuf ctl;                      // DrCtl: the living of the push under way
    RcBuf jet;                      // COLORMAP_JET, 768 bytes
    RcZeroFence zf;
};

// Flow infill of one stream slot (infill_kernels.hip).  Everything is allocated by rcflow_infill_open, for every value
// rcflow_infill_set may give, and released by rcflow_infill_close / rcflow_destroy.
struct RcInfill {
    bool open = false;
    int w = 0, h = 0;
    rc_infill_params prm{};         // levels, min_known and flags: as rcflow_infill_set left them
    long long pushes = 0;           // since open / reset
    RcBuf q;                        // [h][w] uint32, qx | qy << 16: the value of a KNOWN or HELD pixel; with hold > 0 the held state
    RcBuf age;                      // [h][w] uint8, age + 1 modulo 256: 0 nothing held (a HOLE), 1 KNOWN, 2..255 HELD; the class plane of a push
    RcBuf lev;                      // S_1..S_7, int4 (SX, SY, N, 0) a cell | V_5..V_7, int2 (Fx | Fy << 16, lev or -1) a cell
    RcBuf acc;                      // [cells][RC_INFILL_SUMS] int64 the launch adds into | 8 int64 by lev, zero between pushes
    RcBuf out;                      // the last push: summary 16 int64 | sums [cells][RC_INFILL_SUMS] int64 | records [cells]
    RcZeroFence zf;
};

// Offshore frame of one stream slot (offshore_kernels.hip).  Everything is allocated by rcflow_offshore_open and released by
// rcflow_offshore_close / rcflow_destroy.
struct RcOffshore {
    bool open = false, have_map = false;
    int w = 0, h = 0;
    rc_offshore_params prm{};       // everything but stations and bins: as rcflow_offshore_set left them
    long long maps = 0, pushes = 0; // since open / reset
    RcBuf col;                      // 2 x [h][w] int16: per class (dry, wet) the row of the nearest pixel of the class in the column, -1 none
    RcBuf d2, near;                 // [h][w] int32 each: the map, d2 negated on dry pixels
    RcBuf jet;                      // COLORMAP_JET, 768 bytes
    RcBuf acc;                      // int64 the launches add into, zero between calls: 8 of a map | table | beyond [stations] | 8 of a push
    RcBuf out;                      // the last calls: map summary 8 | push summary 8 | table | records
    RcZeroFence zf;
};

// Region outlines of one stream slot (outline_kernels.hip).  Everything is allocated by rcflow_outlines_open and released by
// rcflow_outlines_close / rcflow_destroy.
struct RcOutlines {
    bool open = false;
    int w = 0, h = 0, rounds = 0;
    rc_outlines_params prm{};       // min_cracks: as rcflow_outlines_set left it
    long long pushes = 0;           // since open / reset
    RcBuf bits;                     // [h][w] uint8: the four side bits of a pixel
    RcBuf base;                     // [h][w] int32: the cracks before the pixel in key order
    RcBuf blk;                      // counts of the pixel blocks | their bases | the partials of the scans over cracks
    RcBuf kt;                       // [max_cracks] uint32: key | turn << 31, in key order
    RcBuf succ, lead;               // [max_cracks] int32 each: the successor's place, the leader's place
    RcBuf pair[2];                  // [max_cracks] int2 each: the rounds' buffer pair; after them (number, offset) per leader
    RcBuf okt, ok;                  // [max_cracks] each: key | turn << 31 and the loop's number, in loop order
    RcBuf loops;                    // [max_loops]: leader's key, offset, length | the measures the launches add into
    RcBuf ctl;                      // OlCtl: what a push's launches hand each other
    RcBuf vnext;                    // [max_vertices] int32: the next vertex of a stored vertex's loop (the primitives)
    RcBuf out;                      // the last push: summary 8 int64 | records [max_loops] | vertices [max_vertices][2]
    RcZeroFence zf;
};

// warp_kernels.hip: one launch of the affine / perspective warp
struct RcWarpArgs {
    const uint8_t* src; size_t step;
    uint8_t* dst; size_t dst_step;
    int sw, sh, dw, dh;
    double M[9];                         // destination to source; affine: M[0..5]
    const double* d_M;                   // the matrix on the device instead (the stabiliser's fit; affine 6, perspective 9 entries), or null
    int bw0;                             // perspective: columns per block of upstream's tiling (set by rc_warp_launch)
    float* patch;                        // affine: [npatch][rh][rw] gray float of the OUTPUT inside each ROI, or null
    int npatch, rw, rh;
    int rx[RC_STAB_MAX_PATCHES], ry[RC_STAB_MAX_PATCHES];
};

// rcflow_phase_correlate_dev: the tables (and spectra scratch) of the last patch size, cached per slot
struct RcPhaseCorr {
    int w = 0, h = 0;
    RcBuf tab, scratch;
};

// A launch sequence captured per ring parity (rcflow_frame_loop_step, rcflow_push_batch_dev).  The first call with a key
// issues the launches eagerly and remembers the key, the second call with the same key captures them while issuing and
// launches the graph, later calls replay it; another key starts over (rc_graph_step in rcflow_api.hip).
struct RcGraphCache {
    void* exec[2] = {nullptr, nullptr};
    int eager[2] = {0, 0};
    unsigned char key[2][160] = {};   // everything the sequence has baked in, as bytes
};

struct RcSlot {
    hipStream_t own = nullptr, cur = nullptr;
    hipStream_t aux = nullptr;  // second stream: expansions beside flow kernels (clip path option "overlap"; frame loop)
    // frame loop on two streams (rcflow_push_frame_dev): events in a small ring, reused in FIFO order
    hipEvent_t fev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int fev_i = 0;
    hipEvent_t flow_done[2] = {nullptr, nullptr};   // the flow launches of the last two pushes
    int flow_done_i = 0;
    // consecutive two-stream pushes so far: the second stream may run ahead of the slot's stream only past work those
    // pushes recorded themselves; anything else queued on the slot (a clip, a pair call, priming, the one-stream path)
    // zeroes the streak (expand_frames / compute_flows) and the next two-stream push first joins the slot's stream
    int ts_streak = 0;
    bool in_ts_push = false;
    RcPlan plan;
    RcBuf kern;
    RcBuf I[RC_MAX_LEVELS], RA[RC_MAX_LEVELS], RB[RC_MAX_LEVELS];
    RcBuf FA[RC_MAX_LEVELS], FB[RC_MAX_LEVELS];
    RcBuf stage_u8, stage_flow, stage_f32[4];
    RcBuf exM, exV, exG;       // option "exact": matrix planes, window column sums, window row sums (box)
    // host-pointer frame loop (rcflow_push_frame_u8): two page-locked staging frames, an event per frame that
    // fires when its upload has left the staging buffer, two device frames (stage_u8) and the resident flow
    void* pin[2] = {nullptr, nullptr};
    size_t pin_bytes = 0;
    hipEvent_t pin_free[2] = {nullptr, nullptr};
    int pin_i = 0;
    int pin_acq = -1, pin_w = 0, pin_h = 0;   // staging buffer handed to the host by rcflow_frame_buffer_acquire, not yet pushed
    int flow_w = 0, flow_h = 0;   // size of the flow field resident in stage_flow (0: none yet)
    int flow_fresh = 0;           // stage_flow holds the flow of the stream's PREVIOUS pair (the warm start of RC_FARNEBACK_USE_INITIAL_FLOW)
    RcBuf lk;                  // sparse PyrLK pyramids + derivatives (lk_kernels.hip)
    RcBuf fit_ws;              // rcflow_fit_motion_dev: best and ticket of the running launch (fit_kernels.hip)
    RcBuf area_tab;            // INTER_AREA decimation tables
    RcBuf seed, seed_tab;      // RC_FARNEBACK_USE_INITIAL_FLOW: the initial field at the coarsest scale [pairs][h_k][w_k] float2, its tables
    int primed = 0, cur_slot = 0;
    // lockstep batch of streams (rcflow_push_batch_dev): parity of the ring, captured graphs
    int batch_primed = 0, batch_cur = 0;
    RcGraphCache batch_graph;
    // rcflow_frame_loop_step: the captured sequences, the stream's flow-field counter (host copy; the kernels read the
    // device word an.loopc)
    RcGraphCache loop_graph;
    int loop_fc = 0;
    RcAnalysis an;
    RcTimex tx;
    RcFrameStab fs;
    RcRipMap rm;
    RcTracers tr;
    RcRegions rg;
    RcTracks tk;
    RcMotion mt;
    RcFtle ft;
    RcPlanView pv;
    RcWaves wv;
    RcPiv piv;
    RcTransects ts;
    RcKinematics kn;
    RcShoreline sh;
    RcSurf sf;
    RcMeanflow mf;
    RcFlowcheck fc;
    RcDrifters dr;
    RcInfill inf;
    RcOffshore off;
    RcOutlines ol;
    RcPhaseCorr pc;
};

struct RcProfRec {
    int id;
    hipEvent_t e0, e1;
    double bytes;         // compulsory bytes of this launch (inputs once + outputs once)
    double model_bytes;   // SURVEY.md section 8(d) algorithmic bytes of the stages it covers
};

struct rc_ctx {
    int device = 0;
    int max_w = 0, max_h = 0, nstreams = 0;
    RcSlot* slots = nullptr;
    int chunk = 32;
    int exact_taps = 0;
    int exact = -1;            // option "exact": upstream's CPU operation order (exact_kernels.hip); -1 = where the fast path cannot hold the tolerance
    int fuse_iters = 1;
    int chain_min_blocks = 0;  // option "chain_min_blocks" (0 = the kernel's default, 4096)
    int chain = 8;             // option "chain": pairs per tile chain of the fused winsize-3 flow kernel (1 = off)
    int xcd_remap = 1;
    int poly_tile_h = 32;
    int frame_overlap = 1;     // option "frame_overlap": frame loop with the expansion of frame t+1 on a second stream beside the flow kernels of frame t
    int merge_small = 1;       // option "merge_small": merged pyramid / expansion launches for calls of one or two frames
    int overlap = 0;           // option "overlap": clip path on two streams (measured: no gain, the grids fill the GPU)
    int poly_mfma = 0;          // option "poly_mfma": vertical pass of the expansion on the matrix cores (measured 25 % slower)
    int hist_blocks = 0;       // option "hist_blocks": cap on histogram blocks per launch (0 = default)
    int fuse_pyr = 1;         // scale-0 expansion also writes pyramid scales 1 and 2 (exact 2:1 / 4:1 sizes)
    int outlines_early = 1;   // option "outlines_early": a pointer round of the region outlines returns at once when the round before it changed nothing
    int ablate = 0;
    void* comm = nullptr;      // RcComm (comm_rccl.hip): the histogram all-reduce over RCCL
    int prof_on = 0;
    std::vector<RcProfRec> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> prof_launches;
    std::vector<double> prof_ms, prof_bytes, prof_model_bytes;
};

// ---------------------------------------------------------------------------- profile kinds
// The reference's wall-clock buckets (ripcurrents.cpp:103-109, sampled at :205,223,293,314,411,483, printed at
// :518-524) and the kernels that do each bucket's work here.  time_polar has no kernel of its own: the
// cartToPolar of :305-309 is fused into the histogram and classification kernels; classify_accumulate spans
// :376-439 (the reference samples time_threshold at :411, inside it) and is booked under "threshold";
// time_codec (video decode) is host I/O outside this library.  The time-exposure images and the 8-bit colour stages
// (main.cpp:1195-1383, pipelines the timed loop of ripcurrents.cpp does not have) produce frames for display and are
// booked with the other display-frame kernel, under "overlay".  Frame stabilisation (main.cpp:1684-1775) prepares the
// frame the flow is taken from and is booked with the resize stages (frame_preproc), under "farneback".  The opposing-flow map works on the flow field as the
// post-ops (flow_postop) do and is booked with them, under "farneback".
// The tracer lines (book-keeping, primitives, drawing) are the reference's "pathlines" work and are booked under "stream".
// The rip regions label and measure the mask the classification leaves and are booked with it, under "threshold"; the rip
// tracks follow those regions and are booked with them.  The motion templates estimate the frame's direction beside the flow, as
// the opposing-flow map does from it, and are booked where that is, under "farneback".  The flow map and FTLE advect a dense
// particle field as advect_field does and are booked with it, under "stream".  The plan view carries no particle anywhere: it
// resamples the flow field onto the ground grid and rescales it, after which it is the field every later product takes, so
// it is booked with the other operations on the field (flow_postop), under "farneback".  The wave spectra read frames, not the
// flow, and what they leave (cells, a bin map, a depth picture) is looked at beside the time-exposure images made from the
// same frames, so they are booked with those, under "overlay".  The ensemble PIV estimates a velocity field from a frame pair
// as the Farneback kernels do, and its field goes where theirs goes, so it is booked with them, under "farneback".  The transects
// sample the frame and the field along lines and keep what they find from push to push, as the tracer lines do with their
// vertices, and are booked with them, under "stream".  The flow kinematics differentiate one flow field, pixel for pixel, with
// no state from push to push: an operation on the field as the shear-rate colouring among the post-ops (flow_postop) is, so they
// are booked with those, under "farneback".  The shoreline works on pictures, not on flow: the time-exposure MEAN, the plan view's
// picture or a frame, as the time-exposure images and the wave spectra do, and is booked with them, under "overlay".  The surf zone
// is the time exposure's fourth picture and what is read off it, and is booked there too.  The mean current keeps a window over
// the flow field and decides from its mean, as the opposing-flow map does, and is booked where that is, under "farneback".  The
// virtual drifters carry points through the field as the tracer lines do and are booked with them, under "stream".  The offshore
// frame projects one flow field on the shore normal, pixel for pixel, as the post-ops work on the field, and is booked with
// them, under "farneback"; its map is made from a mask when the shore has moved and is booked with it.  The region outlines trace
// the masks and label planes the regions label and are booked with them, under "threshold".
#define RC_BUCKET_TABLE(X) \
    X(RC_B_FARNEBACK, "farneback") X(RC_B_POLAR, "polar") X(RC_B_THRESHOLD, "threshold") X(RC_B_OVERLAY, "overlay") \
    X(RC_B_EROSION, "erosion") X(RC_B_CODEC, "codec") X(RC_B_STREAM, "stream")
// One row per kind: enum name (its id is the row's position), the text name rcflow_profile_read reports as name@level,
// the bucket.  A new kind is a new row at the end.
#define RC_KIND_TABLE(X) \
    X(RC_K_PYR, "pyr_level", RC_B_FARNEBACK) \
    X(RC_K_POLY, "polyexp", RC_B_FARNEBACK) \
    X(RC_K_ITER, "flow_iter", RC_B_FARNEBACK) \
    X(RC_K_HIST, "polar_hist", RC_B_THRESHOLD) \
    X(RC_K_THRESH, "thresholds", RC_B_THRESHOLD) \
    X(RC_K_CLASSIFY, "classify_accumulate", RC_B_THRESHOLD) \
    X(RC_K_ADVECT_FIELD, "advect_field", RC_B_STREAM) \
    X(RC_K_ADVECT_POINTS, "advect_points", RC_B_STREAM) \
    X(RC_K_POSTOP, "flow_postop", RC_B_FARNEBACK) \
    X(RC_K_COLOR, "flow_color", RC_B_THRESHOLD) \
    X(RC_K_ITER2, "flow_iter_x2", RC_B_FARNEBACK) \
    X(RC_K_PREPROC, "frame_preproc", RC_B_FARNEBACK) \
    X(RC_K_EDGES, "create_edges", RC_B_EROSION) \
    X(RC_K_DISPLAY, "streamline_display", RC_B_STREAM) \
    X(RC_K_HSV2BGR, "hsv_to_bgr", RC_B_THRESHOLD) \
    X(RC_K_OVERLAY, "create_output", RC_B_OVERLAY) \
    X(RC_K_FLOW_SEED, "flow_area_init", RC_B_FARNEBACK) \
    X(RC_K_TIMEX, "timex", RC_B_OVERLAY) /* @0 mean, @1 ring products */ \
    X(RC_K_COLOR_U8, "frame_color", RC_B_OVERLAY) /* @0 rgb_to_hsv, @1 hsv_to_rgb, @2 resize_bgr, @3 resize_area_bgr */ \
    X(RC_K_FRAMESTAB, "framestab", RC_B_FARNEBACK) /* @0 correlate in one workgroup, @1 warp, @2..6 the correlate passes as launches of their own,
                                                      @7 multi-patch correlate + fit, @8 affine warp, @9 perspective warp */ \
    X(RC_K_RIPMAP, "ripmap", RC_B_FARNEBACK) /* @0 ring, mean, cell sums, colour and the finish, @1 mask */ \
    X(RC_K_TRACKSTAB, "trackstab", RC_B_FARNEBACK) /* @0 gray, @1 pyrDown, @2 Scharr, @3 PyrLK track, @4 robust fit, @5 corner cells */ \
    X(RC_K_TRACERS, "tracers", RC_B_STREAM) /* @0 book-keeping and primitives, @1 draw, @2 trace to lines */ \
    X(RC_K_REGIONS, "regions", RC_B_THRESHOLD) /* @0 runs, @1 merge, @2 flatten and count, @3 row counts, @4 numbers, @5 outputs and sums, @6 records,
                                                  @7 primitives */ \
    X(RC_K_TRACKS, "tracks", RC_B_THRESHOLD) /* @0 prepare, @1 overlap, @2 claim, @3 winner and update, @4 births and summary, @5 paint and outputs,
                                                @6 primitives */ \
    X(RC_K_MOTION, "motion", RC_B_FARNEBACK) /* @0 update, @1 gradient, picture and cell histograms, @2 sums and records, @3 primitives */ \
    X(RC_K_FTLE, "ftle", RC_B_STREAM) /* @0 ring slot, @1 flow map, @2 tensor, outputs and summary */ \
    X(RC_K_PLANVIEW, "planview", RC_B_FARNEBACK) /* @0 the table (open), @1 the push */ \
    X(RC_K_WAVES, "waves", RC_B_OVERLAY) /* @0 spectrum, @1 cell sums and closing, @2 bin map and picture */ \
    X(RC_K_PIV, "piv", RC_B_FARNEBACK) /* @0 the pair's sums, ring and accumulators, @1 score, peak and records, @2 validation, field, picture, summary */ \
    X(RC_K_TRANSECTS, "transects", RC_B_STREAM) /* @0 sampling, rings and accumulators, @1 velocity, transport, jets, records and summary, @2 time stack and Hovmoeller picture */ \
    X(RC_K_KINEMATICS, "kinematics", RC_B_FARNEBACK) /* @0 smoothing, derivatives, invariants, first sums and the threshold, @1 cores, mask, picture, records and summary */ \
    X(RC_K_SHORELINE, "shoreline", RC_B_OVERLAY) /* @0 indicator, box, plane, histogram and Otsu, @1 lines, @2 outliers, ring, window and records, @3 mask, plane and histogram out, @4 primitives */ \
    X(RC_K_SURF, "surf", RC_B_OVERLAY) /* @0 ring, sums, flags, pictures and counts, @1 lines, @2 reference, channels, records and summary, @3 primitives */ \
    X(RC_K_MEANFLOW, "meanflow", RC_B_FARNEBACK) /* @0 ring, sums, mean, steadiness, spread, picture, cell sums and G, @1 mask, records and summary */ \
    X(RC_K_FLOWCHECK, "flowcheck", RC_B_FARNEBACK) /* @0 staging, gather, box sums, the tests, every output and cell sums, @1 records and summary */ \
    X(RC_K_DRIFTERS, "drifters", RC_B_STREAM) /* @0 release, gather, fates and the scattered adds, @1 density, pictures, records and summary, @2 the zones helper */ \
    X(RC_K_INFILL, "infill", RC_B_FARNEBACK) /* @0 classes, held state and the pull to level 4, @1 the pull above and the push down to level 5, @2 the push to the pixels, every output and cell sums, @3 records and summary */ \
    X(RC_K_OFFSHORE, "offshore", RC_B_FARNEBACK) /* @0 the map's column pass, @1 its row pass, every output and sums, @2 its summary, @3 the push: classes, components, every output and the table, @4 records and summary, @5 the band */ \
    X(RC_K_OUTLINES, "outlines", RC_B_THRESHOLD) /* @0 sides, block counts and their scan, @1 the cracks in key order, @2 the successor's place, @3 a leader round, @4 the cut before the leader, @5 a rank round, @6 loop partials, their scan, numbers and offsets, @7 the cracks in loop order, @8 turn partials, area and box, @9 the scan of turns, vertex offsets and vertices, @10 records and summary, @11 primitives */
#define RC_ROW_ID(id, ...) id,
enum { RC_BUCKET_TABLE(RC_ROW_ID) RC_B_BUCKETS };
enum { RC_KIND_TABLE(RC_ROW_ID) RC_K_KINDS };
// rcflow_debug_kind (host test hook) walks the rows that replaced the three parallel lists: tests/test_plan_host.py pins their ids,
// names and buckets and that there are 25 of them.  A row added since is reported by rcflow_profile_read, where its own tests look.
enum { RC_K_LISTED = RC_K_MOTION };
static_assert(RC_K_LISTED == 25, "the rows before RC_K_MOTION keep their ids");
static_assert(RC_B_BUCKETS == RC_PROFILE_BUCKETS, "include/rcflow.h promises RC_PROFILE_BUCKETS buckets");

int rc_buf_ensure(RcBuf& b, size_t bytes);
void rc_buf_free(RcBuf& b);
// a product's COLORMAP_JET table (768 bytes) on the device, by its open call `who`
int rc_jet_ensure(RcBuf& b, const char* who);
RcSlot* rc_slot(rc_ctx* ctx, int stream);
void rc_graph_drop(RcGraphCache& g);
// analysis_kernels.hip, for rcflow_frame_loop_step
int rc_classify_accumulate(const char* who, rc_ctx* ctx, int stream, const float* d_flow, size_t flow_step, int w, int h, int framecount,
                           float MID, float LOWER, float* d_polar, size_t polar_step, float* d_wclass, size_t wc_step,
                           float* d_out, size_t out_step, uint8_t* d_mask, size_t mask_step);
int rc_loop_counter(rc_ctx* ctx, RcSlot& s, bool set, int value);
int rc_hist_book(const char* who, RcSlot& s, int w, int h, bool commit);
int rc_analysis_ensure(const char* who, rc_ctx* ctx, RcSlot& s, int w, int h);
// computeResizeAreaTab (resize.cpp) grouped by destination index (analysis_kernels.hip)
void rc_area_tab(int ssize, int dsize, double scale, std::vector<int>& start, std::vector<int>& si, std::vector<float>& alpha);
// the zeroing of a product's state: memsets of the buffers that are allocated on `cur`, then the event
int rc_fence_zero(RcZeroFence& z, hipStream_t cur, std::initializer_list<RcBuf*> bufs);
// makes `cur` wait for a pending zeroing made on another stream.  consume: the caller queues work on `cur` that later
// callers are ordered behind (a push); a call that only reads leaves the fence pending
int rc_fence_wait(RcZeroFence& z, hipStream_t cur, bool consume);
void rc_fence_free(RcZeroFence& z);
// 8UC3 image arguments, on RcArgs (rc_args.h).  who, what: the entry point and the argument, for the text
int rc_img3_check(const char* who, const char* what, const uint8_t* p, size_t step, int w, int h);   // RC_EINVAL: null, empty, step < 3 w
// an input and an output of its own size that may not overlap it: the form of both, then the overlap (RC_EINVAL)
int rc_img3_pair(const char* who, const char* in_name, const uint8_t* in, size_t in_step, int sw, int sh, const char* out_name,
                 const uint8_t* out, size_t out_step, int dw, int dh);
int rc_fits_context(const char* who, const rc_ctx* ctx, int w, int h);                                // RC_ESIZE
// lk_kernels.hip: the two halves of a PyrLK call (pyramid of one image; track), for the tracking stabiliser
RcLkPyr rc_lk_plan(int w, int h, int win_w, int win_h, int max_level, bool deriv);
void rc_lk_build(rc_ctx* ctx, hipStream_t cur, const RcLkPyr& q, unsigned char* base);
void rc_lk_track(rc_ctx* ctx, hipStream_t cur_stream, const RcLkPyr& ref, const unsigned char* ref_base, const unsigned char* cur_base,
                 const RcLkPyr& cur, const float* d_prev_pts, float* d_next_pts, int npts, uint8_t* d_status, float* d_err, int win_w, int win_h,
                 int max_count, double epsilon, int flags, double min_eig_threshold);
// corner_kernels.hip, fit_kernels.hip
void rc_gray_launch(rc_ctx* ctx, hipStream_t cur, const uint8_t* d_bgr, size_t step, int w, int h, uint8_t* d_gray);
int rc_corner_check(const char* who, int w, int h, int cells_x, int cells_y, int margin, int min_score);
void rc_corner_launch(rc_ctx* ctx, hipStream_t cur, const uint8_t* d_gray, size_t step, int w, int h, int cells_x, int cells_y, int margin,
                      int min_score, float* d_pts, int* d_scores);
int rc_fit_check(const char* who, int n, int w, int h, const rc_fit_params* prm);
void rc_fit_launch(rc_ctx* ctx, hipStream_t cur, const float* d_p, const float* d_q, const uint8_t* d_status, const int* d_scores, int n, int w,
                   int h, const rc_fit_params& prm, rc_fit_result* d_result, uint8_t* d_inlier, int* d_samples, void* d_ws, double* d_res,
                   double* d_res2);
// analysis_kernels.hip: the launch of rcflow_advect_points_dev ("advect_points@0"); thr may be null when UPPER >= 0
void rc_advect_points_launch(rc_ctx* ctx, hipStream_t cur, float* d_pts, int n, const float* d_flow, size_t flow_step, int w, int h, float dt,
                             int iterations, float UPPER, const float* thr, int variant, float* d_trace);
// draw_kernels.hip ("tracers@1"); the arguments have been checked
void rc_draw_launch(rc_ctx* ctx, hipStream_t cur, uint8_t* d_img, size_t step, int w, int h, int channels, const rc_draw_prim* d_prims,
                    int n, unsigned long long* d_skipped);
// warp_kernels.hip
void rc_warp_launch(rc_ctx* ctx, hipStream_t cur, RcWarpArgs& a, bool perspective);
// transects_kernels.hip: the per-line part of rcflow_transects_plan, shared with rcflow_shoreline_plan and rcflow_surf_plan.  Line i's samples from
// table[first] on and its constants into geom[i] (each may be null); RC_EINVAL with the text set for an endpoint that is not
// finite, a line of no length or a sample outside the picture.  The bounds on n stay with each caller
int rc_line_plan(const char* who, int w, int h, const rc_transect_line& l, int i, int first, double metres_per_pixel, double fps,
                 rc_transect_sample* table, rc_transect_geom* geom);
// initial_flow_kernels.hip
int rc_flow_area_prepare(RcBuf& tab, int W, int H, int w, int h, RcFlowAreaArgs& a);

struct RcProfScope {
    rc_ctx* ctx;
    hipStream_t s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int id;
    double bytes, model_bytes;
    RcProfScope(rc_ctx* c, hipStream_t st, int kind, int level, double alg_bytes, double survey_bytes = -1.);
    ~RcProfScope();
};

#define RC_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            rc_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return RC_EHIP;                                                           \
        }                                                                             \
    } while (0)

// ---------------------------------------------------------------------------- per-slot products
// RcTimex, RcFrameStab, RcRipMap, RcTracers, RcRegions, RcTracks, RcMotion, RcFtle, RcPlanView, RcWaves, RcPiv, RcTransects, RcKinematics, RcShoreline, RcSurf, RcMeanflow, RcFlowcheck, RcDrifters, RcInfill, RcOffshore and RcOutlines share one lifecycle.  A product supplies
//   void rc_state_free(T&)             frees every buffer and the fence; the state is T() again
//   int rc_state_zero(RcSlot&, T&)     rc_fence_zero of what open / reset clear, and the counters
// and open / reset / close are written once, here.
void rc_state_free(RcTimex& t);
void rc_state_free(RcFrameStab& f);
void rc_state_free(RcRipMap& m);
void rc_state_free(RcTracers& t);
void rc_state_free(RcRegions& g);
void rc_state_free(RcTracks& g);
void rc_state_free(RcMotion& m);
void rc_state_free(RcFtle& f);
void rc_state_free(RcPlanView& v);
void rc_state_free(RcWaves& v);
void rc_state_free(RcPiv& v);
void rc_state_free(RcTransects& v);
void rc_state_free(RcKinematics& k);
void rc_state_free(RcShoreline& v);
void rc_state_free(RcSurf& v);
void rc_state_free(RcMeanflow& v);
void rc_state_free(RcFlowcheck& v);
void rc_state_free(RcDrifters& v);
void rc_state_free(RcInfill& v);
void rc_state_free(RcOffshore& v);
void rc_state_free(RcOutlines& v);
int rc_state_zero(RcSlot& s, RcTimex& t);
int rc_state_zero(RcSlot& s, RcFrameStab& f);
int rc_state_zero(RcSlot& s, RcRipMap& m);
int rc_state_zero(RcSlot& s, RcTracers& t);
int rc_state_zero(RcSlot& s, RcRegions& g);
int rc_state_zero(RcSlot& s, RcTracks& g);
int rc_state_zero(RcSlot& s, RcMotion& m);
int rc_state_zero(RcSlot& s, RcFtle& f);
int rc_state_zero(RcSlot& s, RcPlanView& v);
int rc_state_zero(RcSlot& s, RcWaves& v);
int rc_state_zero(RcSlot& s, RcPiv& v);
int rc_state_zero(RcSlot& s, RcTransects& v);
int rc_state_zero(RcSlot& s, RcKinematics& k);
int rc_state_zero(RcSlot& s, RcShoreline& v);
int rc_state_zero(RcSlot& s, RcSurf& v);
int rc_state_zero(RcSlot& s, RcMeanflow& v);
int rc_state_zero(RcSlot& s, RcFlowcheck& v);
int rc_state_zero(RcSlot& s, RcDrifters& v);
int rc_state_zero(RcSlot& s, RcInfill& v);
int rc_state_zero(RcSlot& s, RcOffshore& v);
int rc_state_zero(RcSlot& s, RcOutlines& v);

// The tail of every open.  The caller has validated, selected the device and built `fresh` (rc: what its allocations
// returned).  The state that is open is touched only once nothing can be refused any more: a refused open leaves it as it
// was, at the price of both states being resident for the length of a re-open.
template <class T>
int rc_state_install(RcSlot& s, T& cur, T& fresh, int rc) {
    if (!rc && cur.open && hipStreamSynchronize(s.cur) != hipSuccess) {   // launches still reading the state being replaced
        rc_set_error("hipStreamSynchronize failed before a re-open");
        rc = RC_EHIP;
    }
    if (rc) {                                             // rc_buf_ensure has set the text, with the byte count
        (void)hipGetLastError();
        rc_state_free(fresh);
        return rc;
    }
    rc_state_free(cur);
    cur = fresh;
    cur.open = true;
    if ((rc = rc_state_zero(s, cur))) rc_state_free(cur);
    return rc;
}

// The head of every entry point that works on an open product: the slot and the product's state on it.  RC_EINVAL for a
// bad slot, RC_ESTATE while the product is closed.  Selecting the device and waiting for the zeroing stay with the caller
template <class T>
int rc_state_get(rc_ctx* ctx, int stream, T RcSlot::*member, const char* who, RcSlot*& s, T*& st) {
    if (!(s = rc_slot(ctx, stream))) return RC_EINVAL;
    st = &(s->*member);
    if (st->open) return RC_OK;
    rc_set_error("%s: the product is not open on the slot (its open call comes first)", who);
    return RC_ESTATE;
}

template <class T>
int rc_state_reset(rc_ctx* ctx, int stream, T RcSlot::*member, const char* who) {
    RcSlot* s; T* st;
    if (int rc = rc_state_get(ctx, stream, member, who, s, st)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    return rc_state_zero(*s, *st);
}

template <class T>
int rc_state_close(rc_ctx* ctx, int stream, T RcSlot::*member) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!(s->*member).open) return RC_OK;
    RC_HIP(hipSetDevice(ctx->device));
    RC_HIP(hipStreamSynchronize(s->cur));
    rc_state_free(s->*member);
    return RC_OK;
}
