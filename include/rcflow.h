/*
 * rcflow.h -- C ABI of librcflow.so: MI355X (gfx950) dense Farneback optical flow and
 * the per-pixel rip-current analysis that consumes it.
 *
 * This is the drop-in boundary for the one hot path of borgor/ripcurrents (SURVEY.md
 * section 8b).  Every entry point names the reference interface it replaces; paths are
 * relative to /root/reference/RipCurrents_main.  Plain pointers and sizes only; image
 * arguments are (pointer, byte step) pairs laid out like cv::Mat (interleaved channels).
 *
 * Conventions
 *  - returns RC_OK (0) or a negative RC_E* code; nothing throws across the ABI;
 *  - the caller owns every buffer; the context owns its device workspaces;
 *  - a context is bound to one GPU; `stream` selects one of its independent stream
 *    slots (own HIP stream, workspaces and analysis state).  Calls on one slot are
 *    ordered; distinct slots may be driven from distinct host threads;
 *  - *_dev entry points take DEVICE pointers, enqueue on the slot's HIP stream and
 *    return without waiting (rcflow_sync waits); the host-pointer forms copy in,
 *    compute, copy out and return when the result is in the caller's buffer;
 *  - there is no CPU fallback: without a usable HIP device rcflow_create fails.
 */
#ifndef RCFLOW_H
#define RCFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCFLOW_ABI_VERSION 1

typedef struct rc_ctx rc_ctx;

enum {
    RC_OK = 0,
    RC_EINVAL = -1,   /* bad argument (what cv::Exception / CV_Assert is in the reference) */
    RC_ENOMEM = -2,   /* device or host allocation failed */
    RC_EHIP = -3,     /* a HIP runtime call failed; rcflow_last_error() has the text */
    RC_ENODEV = -4,   /* no usable gfx950 device */
    RC_ESIZE = -5,    /* frame larger than the context was created for */
    RC_ESTATE = -6,   /* call order violated (e.g. analysis before any flow) */
    RC_ECOMM = -7     /* collective layer not initialised / failed */
};

/* cv::OPTFLOW_FARNEBACK_GAUSSIAN and cv::OPTFLOW_USE_INITIAL_FLOW; any other bit is RC_EINVAL.
 * RC_FARNEBACK_USE_INITIAL_FLOW: the flow argument is in/out.  As in optflow.cpp calc(), its content is reduced to the
 * coarsest scale with resize(INTER_AREA), multiplied by pyr_scale^levels (levels as cropped, rcflow_level_geometry) and
 * starts that scale instead of zeros; every finer scale proceeds as without the flag.  The field must be 8-byte aligned
 * (pointer and strides).  Where the initial field comes from, per entry point:
 *   rcflow_farneback_dev / _u8          d_flow_xy / flow_xy, in/out;
 *   rcflow_push_frame_dev               d_flow_xy, in/out: the same buffer passed every frame gives the temporal warm start
 *                                       (pair t starts from the field of pair t - 1); a priming call (returns 1) neither
 *                                       reads nor writes it;
 *   rcflow_push_frame_u8 / _acquired,   the slot's resident field of the previous pair (rcflow_stream_flow_ptr); the first
 *   rcflow_frame_loop_step              pair after a priming call starts from zero, bit-identical to the flag unset;
 *   rcflow_push_batch_dev               d_flows_xy[z], in/out per stream z (the captured launch sequence includes the
 *                                       reduction);
 *   rcflow_push_clip_dev,               RC_EINVAL: the pairs of a clip are solved together, a pair cannot wait for its
 *   rcflow_farneback_clip_dev           predecessor's field.
 * The bit is part of rc_farneback_params: a stream that toggles it primes again like after any other parameter change. */
#define RC_FARNEBACK_GAUSSIAN 256
#define RC_FARNEBACK_USE_INITIAL_FLOW 4

/* ripcurrents.hpp:7-9 */
#define RC_HIST_BINS 50
#define RC_HIST_DIRECTIONS 36
#define RC_HIST_RESOLUTION 20
/* hist[50] | hist2d[36*50] | histsum | histsum2d[36]: the all-reduce payload */
#define RC_HIST_WORDS (RC_HIST_BINS + RC_HIST_DIRECTIONS * RC_HIST_BINS + 1 + RC_HIST_DIRECTIONS)

/* Parameters of cv::calcOpticalFlowFarneback, in its argument order. */
typedef struct rc_farneback_params {
    double pyr_scale;
    int levels;
    int winsize;
    int iterations;
    int poly_n;
    double poly_sigma;
    int flags;
} rc_farneback_params;

/* ------------------------------------------------------------------ lifetime */

/* Creates a context on HIP device `device` with `max_streams` stream slots, each able to
 * hold frames up to max_w x max_h. */
int rcflow_create(rc_ctx** out, int device, int max_w, int max_h, int max_streams);
void rcflow_destroy(rc_ctx* ctx);
int rcflow_abi_version(void);
/* The text of the calling thread's last failed call.  Every return other than RC_OK has set it, and it starts with the
 * name of the function that refused (a bad context or slot index, and a failed HIP call, carry no name). */
const char* rcflow_last_error(void);
/* Waits for everything enqueued on the slot. */
int rcflow_sync(rc_ctx* ctx, int stream);
/* Runs the slot on a caller-owned hipStream_t (e.g. the host framework's current
 * stream; NULL is the device's null stream).  rcflow_use_own_stream restores the slot's
 * own non-blocking stream. */
int rcflow_set_hip_stream(rc_ctx* ctx, int stream, void* hip_stream);
int rcflow_use_own_stream(rc_ctx* ctx, int stream);
/* "exact" (-1 | 0 | 1, default -1): 1 runs every Farneback stage in the operation order of OpenCV's CPU path
 * (float / double exactly where optflow.cpp has them, no fused multiply-adds): the flow field is then
 * bit-identical to the CPU path (tests/test_gpu_exact.py), at 2-15x the time.  0 always takes the fast kernels
 * (reordered fp32 sums: within SURVEY 8(d)'s tolerance wherever the 2x2 system is well conditioned).  -1 picks
 * exact only where the fast kernels cannot hold that tolerance: the near-pointwise windows (Gaussian winsize < 7,
 * i.e. main.cpp:264, :742, ripcurrents_module.cpp:712, main_old.cpp:324, and winsize 1), whose determinant
 * vanishes on smooth regions so that any rounding difference is amplified from scale to scale.
 * Tunables: "chunk" = frame pairs per launch in clip mode (default 32);
 * "exact_taps" = 1 keeps every polynomial-expansion tap instead of dropping taps whose
 * total weight is below 1e-8 of the kernel mass (default 0);
 * "fuse_iters" = 0 runs every Farneback iteration as its own launch instead of two per
 * launch (default 1; results are bit-identical either way);
 * "chain" = consecutive frame pairs a block of the fused winsize-3 flow kernel walks on its tile, taking pair
 * z + 1's previous-frame coefficients out of pair z's next-frame window in LDS (the reference's u_f1.copyTo(u_f2),
 * ripcurrents.cpp:194-221, at tile level; default 8, 1 = off; halved for small launches until "chain_min_blocks" blocks
 * (default 4096) remain; same bits).
 * Measurement switches, all speed-only except where noted: "xcd_remap" (1) XCD-aware tile order;
 * "poly_tile_h" (32 | 48) rows per expansion block -- changes the per-tile DC and with it the last
 * bits of R; "poly_mfma" (0) vertical pass of the expansion on the matrix cores -- different
 * summation order, same tolerance; "overlap" (0) clip path on two streams; "hist_blocks" (0 = default, 8192)
 * cap on histogram blocks per launch: divided by the launch's field count, with a floor of 8 blocks per field (see
 * rcflow_histogram_clip_dev); "frame_overlap" (0 | 1 | 2, default 1): the frame loop on two streams -- upload and expansion of
 * frame t+1 beside the flow kernels of frame t; 1 = rcflow_push_frame_u8 only (the library owns the upload), 2 = also
 * rcflow_push_frame_dev, the caller then guaranteeing that d_frame is complete when the call is made; "merge_small" (1) merged launches for calls of one or two frames; "fuse_pyr" (1)
 * pyramid scales 1 and 2 written by the scale-0 expansion launch (pyr_scale 0.5, exact half / quarter sizes);
 * "outlines_early" (1) a pointer round of rcflow_outlines_push_dev returns at once when the round before it changed nothing (0: every
 * round does its work; same bits);
 * "ablate" bit field selecting the alternative kernel forms the bit-identity tests compare against (0 in production):
 * 2 option exact, box windows of winsize 3 / 5: plain scans; 16 the same with the matrices inside the column scan;
 * 4096 earlier pyramid kernels; 65536 tile kernel for Gaussian winsize 10 / 20 whatever the launch size; 8388608
 * strip-sweep kernel for them whatever the launch size; 33554432 tile chains whatever the launch size (enum RcAblate
 * in csrc/rc_common.h). */
int rcflow_set_option(rc_ctx* ctx, const char* name, int value);

/* ------------------------------------------------------------------ A: Farneback
 * Replaces  cv::calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize,
 *           iterations, poly_n, poly_sigma, flags)
 * as called at ripcurrents.cpp:215, main.cpp:264,609,742,961,1119,1481,
 * ripcurrents_module.cpp:712, main_old.cpp:324 (8UC1 in, CV_32FC2 out). */
int rcflow_farneback_u8(rc_ctx* ctx, int stream, const uint8_t* prev, size_t prev_step,
                        const uint8_t* next, size_t next_step, int w, int h, float* flow_xy,
                        size_t flow_step, double pyr_scale, int levels, int winsize,
                        int iterations, int poly_n, double poly_sigma, int flags);
/* Same, device pointers, asynchronous. */
int rcflow_farneback_dev(rc_ctx* ctx, int stream, const uint8_t* d_prev, size_t prev_step,
                         const uint8_t* d_next, size_t next_step, int w, int h,
                         float* d_flow_xy, size_t flow_step, const rc_farneback_params* p);
/* Streaming form of the frame loop ripcurrents.cpp:194-221 (`u_f1.copyTo(u_f2)` at :216):
 * the slot keeps the previous frame's polynomial expansion, so each call does one
 * pyramid + expansion.  The first call after rcflow_stream_reset only primes the state
 * and writes no flow (returns 1 instead of RC_OK); so does the first call with a different
 * frame size or different parameters (the cached expansion belongs to the old ones). */
int rcflow_push_frame_dev(rc_ctx* ctx, int stream, const uint8_t* d_frame, size_t step,
                          int w, int h, float* d_flow_xy, size_t flow_step,
                          const rc_farneback_params* p);
/* The same loop with HOST frames, as the reference holds them after video.read / resize / cvtColor
 * (ripcurrents.cpp:198-213): the frame is copied into one of two page-locked staging buffers and uploaded
 * asynchronously; the call returns once the copy into the staging buffer is done, so upload and kernels of frame t
 * overlap the host's decode of frame t + 1.  The flow field stays on the device (rcflow_stream_flow_ptr: input of the
 * analysis entry points) and crosses PCIe only through rcflow_stream_flow_read.  Returns 1 when the call primed the
 * stream.  Interoperates with rcflow_push_frame_dev / rcflow_push_clip_dev on the same slot. */
int rcflow_push_frame_u8(rc_ctx* ctx, int stream, const uint8_t* frame, size_t step, int w, int h,
                         const rc_farneback_params* p);
/* Without the copy: rcflow_frame_buffer_acquire hands out the next of the slot's two page-locked staging buffers (w x h
 * bytes, dense rows; it waits until the upload that last read that buffer has left it) for the host to produce the frame
 * INTO -- e.g. as the destination Mat of the cvtColor at ripcurrents.cpp:210 -- and rcflow_push_frame_acquired pushes it
 * like rcflow_push_frame_u8 does (same return values, asynchronous).  One buffer is out at a time: acquiring again, or a
 * rcflow_push_frame_u8 on the slot, takes the same buffer back (RC_ESTATE from a push without an acquisition). */
int rcflow_frame_buffer_acquire(rc_ctx* ctx, int stream, int w, int h, uint8_t** host_frame, size_t* step);
int rcflow_push_frame_acquired(rc_ctx* ctx, int stream, const rc_farneback_params* p);
int rcflow_stream_flow_ptr(rc_ctx* ctx, int stream, float** d_flow_xy, int* w, int* h);
int rcflow_stream_flow_read(rc_ctx* ctx, int stream, float* flow_xy, size_t flow_step);

/* One whole iteration of the reference's frame loop (ripcurrents.cpp:194-479) per call, on the device (with use_graph:
 * as ONE hipGraph launch per frame once the slot has seen the same configuration twice): the frame the host produced into the buffer of
 * rcflow_frame_buffer_acquire is uploaded and expanded, the flow against the previous frame is computed (:215), then on
 * that resident field: streamline_field(dt, iterations) with the PREVIOUS frame's UPPER (:229-231), the seed
 * streamlines (:283-285, rcflow_advect_points_dev semantics; nseeds may be 0), the cumulative histogram and the
 * thresholds (:319-366), create_flow + create_accumulationbuffer with framecount = the number of flow fields of this
 * stream so far (:376-439; the counter lives on the device so that the captured launch sequence stays valid), and the
 * mask's edges (:477-479; d_edges and d_outmask may be NULL).  Same kernels, same order, same bits as the separate
 * calls.  Returns 1 when the call only primed the stream (first frame, or another size / other parameters: no flow
 * yet), RC_ESTATE without an acquired frame buffer.  The slot keeps a ring of two expansions while it is driven this
 * way; rcflow_stream_reset (or any other entry point on the slot) restarts it. */
typedef struct rc_frame_loop {
    float dt; int iterations;                 /* streamline_field */
    float* d_seeds; int nseeds;               /* device, nseeds x (x, y), advanced in place */
    int seed_variant; float seed_dt; int seed_iterations; float seed_upper;
    float MID, LOWER;                         /* ripcurrents.cpp:142-143: 0.5, 0.2 */
    uint8_t* d_outmask; size_t mask_step;     /* device 8UC1, optional */
    uint8_t* d_edges; size_t edges_step;      /* device 8UC1, optional (needs d_outmask) */
    int use_graph;                            /* 0 (default): the launches are issued one by one, upload and expansion on the slot's
                                               * second stream; 1: one captured hipGraph launch per frame on a ring of two expansions */
} rc_frame_loop;
int rcflow_frame_loop_step(rc_ctx* ctx, int stream, const rc_farneback_params* p, const rc_frame_loop* loop);
/* Batched form of the same stream: the nframes frames continue the slot's stream, every frame is expanded
 * once however the segment is cut into calls.  Returns the number of flow fields written to d_flows[0..):
 * nframes if the stream was primed (flow 0 = last frame of the previous call -> d_frames[0]), nframes - 1 if
 * this call primed it; negative RC_E* on error.  Interoperates with rcflow_push_frame_dev. */
int rcflow_push_clip_dev(rc_ctx* ctx, int stream, const uint8_t* d_frames, size_t frame_stride, size_t step,
                         int nframes, int w, int h, float* d_flows_xy, size_t flow_frame_stride,
                         size_t flow_step, const rc_farneback_params* p);
int rcflow_stream_reset(rc_ctx* ctx, int stream);
/* A whole resident clip: nframes frames -> nframes-1 flow fields (pair t = frames t,t+1),
 * processed `chunk` pairs per launch.  The bench path. */
int rcflow_farneback_clip_dev(rc_ctx* ctx, int stream, const uint8_t* d_frames,
                              size_t frame_stride, size_t step, int nframes, int w, int h,
                              float* d_flows_xy, size_t flow_frame_stride, size_t flow_step,
                              const rc_farneback_params* p);
/* Lockstep batch of `nstreams` independent video streams (BASELINE config 5): frame t of every
 * stream arrives together as d_frames[nstreams][h][w]; the slot keeps every stream's previous
 * expansion, so each call is one pyramid + expansion + flow per stream, all streams in the same
 * launches.  The first call after rcflow_batch_reset primes the state and returns 1.  With
 * use_graph != 0 the launch sequence is captured into a hipGraph the second time the same
 * buffers are seen and replayed from then on (two graphs, one per ring parity). */
int rcflow_push_batch_dev(rc_ctx* ctx, int stream, const uint8_t* d_frames, size_t frame_stride,
                          size_t step, int nstreams, int w, int h, float* d_flows_xy,
                          size_t flow_frame_stride, size_t flow_step,
                          const rc_farneback_params* p, int use_graph);
int rcflow_batch_reset(rc_ctx* ctx, int stream);
/* Level geometry actually used (levels cropped at min_size 32, cvRound sizes).
 * Returns the cropped `levels`; scales are k = 0..levels. */
int rcflow_level_geometry(int w, int h, double pyr_scale, int levels, int k, int* wk, int* hk);

/* Stage-level entry points (device pointers; used by the parity tests to compare each
 * kernel with the oracle stage by stage; interleaved layouts as in OpenCV). */
int rcflow_stage_pyr_level_dev(rc_ctx* ctx, int stream, const uint8_t* d_img, size_t step,
                               int w, int h, double pyr_scale, int k, float* d_out /* hk*wk */);
int rcflow_stage_polyexp_dev(rc_ctx* ctx, int stream, const float* d_I, int w, int h,
                             int poly_n, double poly_sigma, float* d_R5 /* h*w*5 */);
/* One FarnebackUpdateMatrices + FarnebackUpdateFlow_* application:
 * flow_out = solve(blur(M(R0, R1, flow_in))) */
int rcflow_stage_flow_iter_dev(rc_ctx* ctx, int stream, const float* d_R0_5,
                               const float* d_R1_5, const float* d_flow_in, int w, int h,
                               int winsize, int flags, float* d_flow_out);
/* The reduction RC_FARNEBACK_USE_INITIAL_FLOW applies to the initial field: resize(flow, Size(wk, hk), INTER_AREA) to the
 * coarsest scale k = cropped levels, times (float)pyr_scale^k.  d_flow_xy: h x w float2 with a byte step;
 * d_out: hk x wk float2, dense. */
int rcflow_stage_initial_flow_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step,
                                  int w, int h, double pyr_scale, int levels, float* d_out /* hk*wk*2 */);

/* ------------------------------------------------------------------ B: analysis
 * Per-slot device-resident state mirrors the locals of ripcurrents.cpp:133-176:
 * hist/hist2d/histsum/histsum2d (cumulative, never reset by the reference), UPPER (=100
 * initially), UPPER2d, prop_above_upper, accumulator, streamlines_mat/_distance. */
int rcflow_analysis_reset(rc_ctx* ctx, int stream, int w, int h);

/* Replaces the counting loop of create_histogram (ripcurrents_module.cpp:94-107,
 * ripcurrents.cpp:319-330) fused with the polar conversion ripcurrents.cpp:305-309.
 * Adds this flow field's counts to the slot's cumulative histogram. */
int rcflow_histogram_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step,
                         int w, int h);
/* The counters are int32 like the reference's (`int hist[50]`, ripcurrents.cpp:147-150, which wrap after
 * 2^31 / (w*h) frames): a call that could carry histsum past INT32_MAX returns RC_ESTATE and counts nothing;
 * rcflow_histogram_reset_dev starts a new segment (asynchronous zero of the counters only). */
int rcflow_histogram_reset_dev(rc_ctx* ctx, int stream);
/* The same for `count` resident flow fields in one launch (a segment's flows), flow_frame_stride bytes apart: for
 * count > 1 at least one frame's range and a multiple of 8 (RC_EINVAL otherwise); ignored for count == 1.  The launch is
 * (blocks per field) x count blocks of 256 threads, a thread taking items of 2 x 4 pixels in rounds: blocks per field =
 * min(ceil(items / 256), 2048, max(8, B / count)) with B = option "hist_blocks", or 8192 when that is 0 -- the option is
 * divided by `count` and has a floor of 8 blocks per field.  32 fields of 1920 x 1080 with the default: 256 blocks per
 * field and four rounds. */
int rcflow_histogram_clip_dev(rc_ctx* ctx, int stream, const float* d_flows_xy,
                              size_t flow_frame_stride, size_t flow_step, int count, int w, int h);
/* Replaces the threshold scans of create_histogram (ripcurrents_module.cpp:109-144):
 * derives UPPER, UPPER2d[36], prop_above_upper[36] on the device from the slot's counts. */
int rcflow_thresholds_dev(rc_ctx* ctx, int stream);
/* the same scans on a caller-held block of RC_HIST_WORDS device counters (the all-reduced global
 * histogram); the slot's own cumulative counters are not touched */
int rcflow_thresholds_words_dev(rc_ctx* ctx, int stream, const int32_t* d_words);
/* Copies the slot's histogram words (RC_HIST_WORDS int32: hist, hist2d, histsum,
 * histsum2d) and thresholds to the host; any pointer may be NULL.  Synchronises. */
int rcflow_histogram_read(rc_ctx* ctx, int stream, int32_t* hist, int32_t* hist2d,
                          int32_t* histsum, int32_t* histsum2d, float* UPPER, float* UPPER2d,
                          float* prop_above_upper);
int rcflow_histogram_write(rc_ctx* ctx, int stream, const int32_t* words /* RC_HIST_WORDS */);
/* Device address of the RC_HIST_WORDS int32 block (for an RCCL all-reduce issued by the
 * host framework on the slot's stream). */
int rcflow_histogram_device_ptr(rc_ctx* ctx, int stream, int32_t** d_words);

/* Replaces create_flow + create_accumulationbuffer (ripcurrents_module.cpp:153-212,
 * ripcurrents.cpp:376-439) fused with the polar conversion.  Uses the slot's UPPER /
 * UPPER2d; MID/LOWER are ripcurrents.cpp:142-143.  Optional outputs (device, may be
 * NULL): polar_hsv 32FC3 (angle, sat, val rescaled: the `current` the reference displays),
 * waterclass 32FC3, out 32FC3, outmask 8UC1.  The slot's accumulator (.x channel of the
 * reference's 32FC3 accumulator) is updated when framecount > 30. */
int rcflow_classify_accumulate_dev(rc_ctx* ctx, int stream, const float* d_flow_xy,
                                   size_t flow_step, int w, int h, int framecount, float MID,
                                   float LOWER, float* d_polar_hsv, size_t polar_step,
                                   float* d_waterclass, size_t wc_step, float* d_out,
                                   size_t out_step, uint8_t* d_outmask, size_t mask_step);
int rcflow_accumulator_read(rc_ctx* ctx, int stream, float* acc /* h*w */);

/* Replaces streamlines_mat.forEach(streamline_field(...)) ripcurrents.cpp:229-231
 * (ripcurrents_module.cpp:608-648): one particle per pixel, state in the slot.
 * UPPER < 0 means "use the slot's current UPPER" (the value the previous frame's
 * histogram produced, as in the reference's call order).  iterations: 0..65536 (the reference
 * passes 1 or 100), RC_EINVAL beyond -- the loop runs on the device. */
int rcflow_advect_field_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step,
                            int w, int h, float dt, int iterations, float UPPER);
int rcflow_advect_field_read(rc_ctx* ctx, int stream, float* pt_xy /* h*w*2 */,
                             float* dist /* h*w */);
/* Replaces the seed loops over streamline()/streamline_2()/streamline_3()/pathlines
 * (ripcurrents.cpp:283-285, ripcurrents_module.cpp:72-75): variants
 * 0 ripcurrents_module.cpp:486-528, 1 :531-569, 2 :572-606, 3 ripcurrents.cpp:656-698,
 * 4 pathlines.cpp:9-46.  d_pts is n x (x,y), updated in place; d_trace (optional)
 * receives the position after every step (n*iters*2 floats), for the host to draw or for rcflow_trace_prims_dev
 * and rcflow_draw_dev to draw where it lies. */
int rcflow_advect_points_dev(rc_ctx* ctx, int stream, float* d_pts, int n,
                             const float* d_flow_xy, size_t flow_step, int w, int h, float dt,
                             int iterations, float UPPER, int variant, float* d_trace);
/* get_delta over every pixel (ripcurrents_module.cpp:395-397,650-679). */
int rcflow_get_delta_field_dev(rc_ctx* ctx, int stream, float* d_pt_xy, size_t pt_step,
                               const float* d_flow_xy, size_t flow_step, int w, int h,
                               float dt, float UPPER);

/* Flow-field post-ops (in place on device flow fields) */
int rcflow_subtract_average_dev(rc_ctx* ctx, int stream, float* d_flow_xy, size_t flow_step,
                                int w, int h);                 /* ripcurrents_module.cpp:810-898 */
int rcflow_subtract_mean_magnitude_dev(rc_ctx* ctx, int stream, float* d_flow_xy,
                                       size_t flow_step, int w, int h);   /* :900-1015 */
int rcflow_stabilizer_dev(rc_ctx* ctx, int stream, float* d_flow_xy, size_t flow_step, int w,
                          int h);                              /* :279-308 */
int rcflow_window_mean_dev(rc_ctx* ctx, int stream, float* d_avg, float* d_slot,
                           const float* d_cur, size_t n, int window);     /* main.cpp:1142-1153 */
/* Colouring: HSV triples as the reference builds them before cvtColor(HSV2BGR). */
int rcflow_vector_to_color_dev(rc_ctx* ctx, int stream, const float* d_flow_xy,
                               size_t flow_step, int w, int h, uint8_t* d_hsv, size_t hsv_step,
                               float* max_displacement_io);    /* :1017-1057 */
int rcflow_shear_rate_to_color_dev(rc_ctx* ctx, int stream, const float* d_flow_xy,
                                   size_t flow_step, int w, int h, uint8_t* d_hsv,
                                   size_t hsv_step, float* max_frobenius_io); /* :1059-1138 */

/* ------------------------------------------------------------------ SURVEY 8(f) "next" rows
 * create_edges(outmask) ripcurrents_module.cpp:216-220 (ripcurrents.cpp:477-479): 5x5
 * MORPH_ELLIPSE dilate followed by the morphological gradient, fused.  Not in place. */
int rcflow_create_edges_dev(rc_ctx* ctx, int stream, const uint8_t* d_outmask, size_t mask_step,
                            int w, int h, uint8_t* d_edges, size_t edges_step);
/* create_output(subframe, outmask) ripcurrents_module.cpp:225-244 (ripcurrents.cpp:487-505): in place,
 * red channel of the 8UC3 frame := 255 wherever the edge mask is non-zero. */
int rcflow_create_output_dev(rc_ctx* ctx, int stream, uint8_t* d_subframe_bgr, size_t step,
                             const uint8_t* d_outmask, size_t mask_step, int w, int h);
/* resize(frame, subframe, Size(dw,dh), 0, 0, INTER_LINEAR) + cvtColor(COLOR_BGR2GRAY)
 * (ripcurrents.cpp:209-210, main.cpp:258-259): 8UC3 BGR frame in, 8UC1 out. */
int rcflow_resize_bgr_to_gray_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step,
                                  int sw, int sh, uint8_t* d_gray, size_t gray_step, int dw, int dh);
/* The same with INTER_AREA, as the reference resizes the FIRST frame of a run (ripcurrents.cpp:186,
 * main.cpp:126, 223, ...); shrinking only. */
int rcflow_resize_area_bgr_to_gray_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step,
                                       int sw, int sh, uint8_t* d_gray, size_t gray_step, int dw, int dh);

/* The resize alone, 8UC3 out: resize(frame, resized_frame, Size(dw,dh), 0, 0, INTER_LINEAR) as the time-exposure
 * pipelines call it (main.cpp:1227, :1302).  Same fixed-point arithmetic as rcflow_resize_bgr_to_gray_dev. */
int rcflow_resize_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int sw, int sh,
                          uint8_t* d_out, size_t out_step, int dw, int dh);

/* The INTER_AREA resize alone, 8UC3 out: resize(frame, frame, Size(dw,dh), 0, 0, INTER_AREA) as compute_phaseCorrelate
 * calls it on every frame (main.cpp:1707, :1723).  Same arithmetic and the same refusals as
 * rcflow_resize_area_bgr_to_gray_dev (shrinking only).  Recorded as "frame_color@3". */
int rcflow_resize_area_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int sw, int sh,
                               uint8_t* d_out, size_t out_step, int dw, int dh);

/* ------------------------------------------------------------------ frame stabilisation
 * compute_phaseCorrelate (main.cpp:1684-1775) on frames resident on the device: every frame is registered to the last
 * CORRECTED frame on a patch that does not move (the reference: 50 x 50 at (XDIM - 50, 50)) by
 * cv::phaseCorrelate(prev_patch, curr_patch, hann) and translated back by cv::warpAffine, before any flow is taken
 * from it.  (rcflow_stabilizer_dev above is a different thing: it corrects a flow field after the fact.)
 * The OpenCV functions are restated from upstream 4.1.0 (phasecorr.cpp, imgwarp.cpp), parity-unpinned:
 *   patches zero-padded to getOptimalDFTSize (2^a 3^b 5^c) N x M, multiplied by createHanningWindow of the unpadded
 *   size (the square root of the product of the raised cosines), P = F(a) conj F(b), C = P |P| / (|P|^2 + FLT_EPSILON),
 *   unscaled inverse DFT, fftShift, first maximum in row-major order, 5 x 5 centroid in double clipped to the surface
 *   (values as they are), response = sum of the box / (M N), shift = (N / 2.0, M / 2.0) - centroid: b(x) = a(x - d)
 *   gives +d.  fftShift sends index i to (i + floor(n / 2)) mod n while the centre stays n / 2.0, so an odd optimal
 *   size reports a constant +0.5 px on that axis; reproduced.
 *   warpAffine(src, [1 0 -sx; 0 1 -sy]) is dst(x, y) = src(x + sx, y + sy), INTER_LINEAR in 8-bit fixed point
 *   (X0 = cvRound(sx * 1024) + 16, Y0 = cvRound((y + sy) * 1024) + 16 per row, fractions of 1/32 px, weights of 2^15,
 *   out = (sum + 2^14) >> 15), BORDER_CONSTANT 0 tap by tap; at fraction (0, 0) the source pixel itself.
 * The DFTs are direct sums in fp32 against twiddle tables made on the host in double (no rocFFT / hipFFT).
 * When profiling is on: "framestab@0" the correlation as one workgroup (patch in LDS; optimal sizes up to about
 * 100 x 100), "framestab@1" the warp, "framestab@2..6" the correlation's passes as launches of their own for larger
 * patches; rcflow_profile_read_buckets books them under "farneback" with the resize stages. */
/* Stage: phaseCorrelate of two 32FC1 patches on the device, w, h in 8..256 with optimal DFT sizes up to 256 x 256
 * (RC_EINVAL / RC_ESIZE otherwise).  d_result: three doubles on the device (shift_x, shift_y, response).
 * Asynchronous; the tables of the last patch size are cached per slot (a change of size synchronises the slot). */
int rcflow_phase_correlate_dev(rc_ctx* ctx, int stream, const float* d_a, size_t a_step, const float* d_b, size_t b_step,
                               int w, int h, int use_hann, double* d_result);
/* Stage: the reference's warpAffine call for a shift known to the host.  Not in place (RC_EINVAL when d_out overlaps
 * d_bgr); RC_EINVAL for a shift that is not finite or beyond 2^20 px. */
int rcflow_warp_translate_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int w, int h,
                                  uint8_t* d_out, size_t out_step, double shift_x, double shift_y);
/* Opens the slot's stabilisation state for 8UC3 frames of w x h and the patch (roi_x, roi_y, roi_w, roi_h): inside the
 * frame, at least 8 x 8 (RC_EINVAL), optimal DFT sizes up to 256 x 256 and the frame within the context's size
 * (RC_ESIZE).  Builds the window and the twiddle tables on the host in double and allocates everything a push needs;
 * re-opening replaces the state, and a refused open (RC_ENOMEM included) leaves the open state as it was: the new state is
 * allocated before the old one is freed, so both are resident for the length of a re-open.  Stream rules as for
 * rcflow_timex_open: the state is zeroed on the stream the slot has at this call (so does rcflow_framestab_reset) and the
 * first push waits for that. */
int rcflow_framestab_open(rc_ctx* ctx, int stream, int w, int h, int roi_x, int roi_y, int roi_w, int roi_h);
/* One frame in, the corrected frame out (both 8UC3 of the opened size).  d_result (device, three doubles, may be
 * NULL) receives shift_x, shift_y, response.  The first push after open / reset has nothing to register against: it
 * copies the frame, reports (0, 0, 0) and becomes `prev` (the reference emits nothing for its first frame: the one
 * stated deviation).  The state keeps the gray patch of the corrected frame itself; d_out is the caller's to overwrite.
 * No host synchronisation and no device-to-host copy: the warp reads the shift from device memory.  RC_EINVAL for a
 * step below 3 * w, a null image, or d_out overlapping d_frame; RC_ESTATE before rcflow_framestab_open; a refused
 * push leaves the state as it was. */
int rcflow_framestab_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_frame, size_t step, uint8_t* d_out,
                              size_t out_step, double* d_result);
/* Blocks until the slot's stream has finished; result = shift_x, shift_y, response of the last push. */
int rcflow_framestab_read(rc_ctx* ctx, int stream, double result[3], long long* frames_pushed);
/* the next push is a first push again; keeps the allocation */
int rcflow_framestab_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_framestab_close(rc_ctx* ctx, int stream);
/* any pointer may be NULL; roi = x, y, w, h; dft_size = N (columns), M (rows); launches_per_push = 2 when the
 * correlation runs as one workgroup, 6 otherwise.  RC_ESTATE when nothing is open on the slot. */
int rcflow_framestab_info(rc_ctx* ctx, int stream, int* w, int* h, int roi[4], int dft_size[2], int* launches_per_push,
                          long long* frames_pushed, size_t* device_bytes);

/* ------------------------------------------------------------------ general warps; several patches, a fitted motion
 * What the reference's other stabiliser, stabilize (main.cpp:1556-1682), does to a frame -- a planar correction,
 * warpPerspective(curr, M.inv()) -- without its AKAZE features, matcher and RANSAC: the motion is estimated by the
 * patch correlation above on SEVERAL static patches, gated by their response, fitted on the device, and the frame is
 * corrected by cv::warpAffine.  cv::warpAffine and cv::warpPerspective are also stages for a matrix the caller has.
 * Both are restated from upstream 4.1.0 (imgwarp.cpp, the CPU path), parity-unpinned; 8UC3, INTER_LINEAR,
 * BORDER_CONSTANT value 0, a destination size of its own.  THE BIT-EXACT CONTRACT IS STATED ON THE
 * DESTINATION-TO-SOURCE MATRIX M (what RC_WARP_INVERSE_MAP passes as given):
 *   affine       adelta[x] = cvRound(M0 x 1024), bdelta[x] = cvRound(M3 x 1024); per row X0 = cvRound((M1 y + M2) 1024) + 16,
 *                Y0 = cvRound((M4 y + M5) 1024) + 16; X = (X0 + adelta[x]) >> 5, Y = (Y0 + bdelta[x]) >> 5; source pixel
 *                (sat_short(X >> 5), sat_short(Y >> 5)), fractions X & 31, Y & 31 (1/32 px).  cvRound is round-half-even;
 *                every product and sum rounds on its own.  M = [1 0 sx; 0 1 sy] is rcflow_warp_translate_bgr_dev bit for bit.
 *   perspective  double per pixel, AND THE BITS DEPEND ON UPSTREAM'S TILING: the destination is walked in blocks of bw0
 *                columns, bh0 = min(16, dh), bw0 = min(1024 / bh0, dw) (64 for any real frame).  With xb the block's
 *                first column and x1 = x - xb: X0 = M0 xb + M1 y + M2, Y0 = M3 xb + M4 y + M5, W0 = M6 xb + M7 y + M8 (left
 *                to right); W = W0 + M6 x1; W = W ? 32 / W : 0; X = cvRound(max(INT_MIN, min(INT_MAX, (X0 + M0 x1) W))), Y
 *                likewise; then >> 5, & 31 and sat_short as above.  Nothing is refused for its range: a point at infinity
 *                (W = 0) reads source pixel (0, 0), and beyond it, where W changes sign, the other sheet of the map.
 *   sample       as rcflow_warp_translate_bgr_dev: weights (32 - fy)(32 - fx) 32, (32 - fy) fx 32, fy (32 - fx) 32,
 *                fy fx 32 of 2^15, out = (sum + 2^14) >> 15 per channel, a tap outside the source counts 0.
 * Without RC_WARP_INVERSE_MAP the matrix is inverted on the host in double first (affine: warpAffine's own sequence,
 * D = M0 M4 - M1 M3, ..., b1 = -M0 M2 - M1 M5; perspective: the cofactor inverse times 1 / det); that is a convenience,
 * held to a tolerance on the matrix, not to bits on the image.
 * RC_EINVAL: a null pointer, a step below 3 * w, d_out overlapping d_bgr (not in place), an entry that is not finite,
 * a singular matrix in the forward form, unknown flag bits; for the affine form a matrix whose terms carry a
 * destination corner beyond 2^20 px (|M0| (dw - 1) + |M1| (dh - 1) + |M2| and the same of M3..M5: the translate warp's
 * bound, it keeps every cvRound within int).  RC_ESIZE: source or destination beyond the context's size.  A refused
 * call writes nothing.  Asynchronous.  Recorded as "framestab@8" (affine) and "framestab@9" (perspective). */
#define RC_WARP_INVERSE_MAP 16      /* cv::WARP_INVERSE_MAP: M maps destination to source as given */
int rcflow_warp_affine_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int sw, int sh,
                               uint8_t* d_out, size_t out_step, int dw, int dh, const double M[6], int flags);
int rcflow_warp_perspective_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int sw, int sh,
                                    uint8_t* d_out, size_t out_step, int dw, int dh, const double M[9], int flags);

/* A stabilisation slot with 1..RC_STAB_MAX_PATCHES static patches and a fitted motion.  rcflow_framestab_push_dev /
 * _read / _reset / _close / _info serve a slot opened either way; a slot opened by rcflow_framestab_open runs the code it
 * always ran.
 *   patches    rois = n x (x, y, w, h), all of ONE size (one window, one twiddle set), each inside the frame, at least
 *              8 x 8 (RC_EINVAL) and small enough for the one-workgroup correlation (optimal sizes up to about
 *              100 x 100; RC_ESIZE beyond: the launch-per-pass form stays single-patch).  They may overlap.
 *   correlate  ONE launch of n workgroups ("framestab@7"), workgroup k the single-patch correlation of patch k: shift k
 *              is what a single-patch slot on that patch computes, bit for bit.
 *   gate       patch k takes part iff response_k >= min_response (NaN fails).
 *   fit        fp64, by the workgroup of that launch that finishes last.  Patch centre c_k = (x + (w - 1) / 2,
 *              y + (h - 1) / 2); with d_k the shift of patch k, T(c_k) ~ c_k + d_k: T maps the corrected frame to the
 *              incoming one and the correction is dst(p) = src(T p), rcflow_warp_affine_bgr_dev with RC_WARP_INVERSE_MAP
 *              reading T from device memory.  The DISPLACEMENT d = B (p - pbar) + t is fitted by unweighted least squares
 *              over the gated patches on coordinates centred on their mean pbar (t = the mean shift), so a still scene
 *              gives T = I exactly: RC_STAB_TRANSLATION B = 0; RC_STAB_SIMILARITY B = [a -b; b a],
 *              a = sum(u.d) / sum(u.u), b = sum(u x d) / sum(u.u); RC_STAB_AFFINE the two rows of B from the 2 x 2 normal
 *              matrix [Sxx Sxy; Sxy Syy].  T = [I + B | t - B pbar].
 *   ladder     affine needs 3 gated patches and det > 1e-12 Sxx Syy (not collinear), else similarity; similarity needs
 *              2 and sum(u.u) > 0, else translation; translation needs 1; none: the identity, model_used = 0 and the
 *              frame is copied.  One patch with RC_STAB_TRANSLATION gives T = [1 0 dx; 0 1 dy] and a frame, result and kept
 *              patch bit-identical to rcflow_framestab_open's slot.
 *   previous   default: every frame is registered against the last CORRECTED frame, the warp writes the gray patches
 *              of its output (the reference's chain).  RC_STAB_ANCHOR_FIRST: against the first frame after open / reset,
 *              whose patches are kept for good; the residual cannot walk (total excursion must stay within a patch).
 * A push is two launches ("framestab@7", "framestab@8"), free of host synchronisation and device-to-host copies; the
 * first push after open / reset copies the frame and reports zeros and the identity.  For such a slot
 * rcflow_framestab_read and d_result give the displacement of the frame centre ((w - 1) / 2, (h - 1) / 2) under T and the
 * smallest response among the patches used (0 when none); rcflow_framestab_info reports patch 0. */
enum { RC_STAB_TRANSLATION = 1, RC_STAB_SIMILARITY = 2, RC_STAB_AFFINE = 3 };
#define RC_STAB_ANCHOR_FIRST 1      /* register against the first frame after open / reset, not the last corrected one */
#define RC_STAB_MAX_PATCHES 16
/* RC_EINVAL: n outside 1..16, a patch outside the frame, below 8 x 8 or of another size than patch 0, an unknown model
 * or flag bit, a min_response that is NaN; RC_ESIZE: see above, or a frame beyond the context's size.  A refused open
 * leaves the slot's state as it was.  Stream rules as rcflow_framestab_open. */
int rcflow_framestab_open_multi(rc_ctx* ctx, int stream, int w, int h, const int* rois /* n x (x, y, w, h) */, int n,
                                int model, double min_response, int flags);
/* Blocks until the slot's stream has finished.  motion = T (row-major 2 x 3) of the last push, model_used = the rung
 * of the ladder it came from (0: identity), shifts = n x (dx, dy, response) of every patch, gated or not (may be NULL,
 * as any other pointer).  Before the second push: the identity, 0, 0, zeros.  For a slot opened by
 * rcflow_framestab_open: [1 0 dx; 0 1 dy], RC_STAB_TRANSLATION, 1, its one shift. */
int rcflow_framestab_read_motion(rc_ctx* ctx, int stream, double motion[6], int* model_used, int* patches_used,
                                 double* shifts /* n x (dx, dy, response), may be NULL */, long long* frames_pushed);
/* any pointer may be NULL; rois receives min(n, cap) patches.  A slot opened by rcflow_framestab_open reports n = 1,
 * RC_STAB_TRANSLATION, min_response = -infinity (it has no gate), flags = 0.  RC_ESTATE when nothing is open. */
int rcflow_framestab_info_multi(rc_ctx* ctx, int stream, int* n, int* rois, int cap, int* model, double* min_response, int* flags);

/* ---- Tracked corners and a robust fitted motion (corner_kernels.hip, fit_kernels.hip).
 *
 * CORNER CELLS.  One best Shi-Tomasi corner per grid cell of an 8UC1 image (bucketed selection; the greedy
 * minimum-distance pass of goodFeaturesToTrack is not offered).  All integers:
 *   dx = (p(x+1,y-1) + 2 p(x+1,y) + p(x+1,y+1)) - (p(x-1,y-1) + 2 p(x-1,y) + p(x-1,y+1)), dy likewise (3 x 3 Sobel pair);
 *   a = sum dx dx, b = sum dx dy, c = sum dy dy over the 3 x 3 block around the pixel;
 *   R = (a + c) - ceil(sqrt((a - c)^2 + 4 b^2)), the root exact (int64): twice the smaller eigenvalue of [a b; b c]
 *   rounded down, the ordering of cv::cornerMinEigenVal(blockSize 3, ksize 3).  R >= 0.
 * Candidates are the pixels at least `margin` (>= 2) from every border; the candidate rectangle is cut into
 * cells_x x cells_y cells of floor(width / cells_x) x floor(height / cells_y) pixels, the last column and row taking the
 * remainder.  Per cell the largest R, ties to the lowest (y, x).  A cell whose best R is 0 or below min_score reports
 * score 0 and its centre ((x0 + x1 - 1) / 2, (y0 + y1 - 1) / 2).  Output in cell order (row-major): d_pts = cells x
 * (x, y) float, d_scores = cells int32.  RC_EINVAL: margin < 2, min_score < 0, cells outside 1..RC_CORNER_MAX_CELLS, a
 * cell side below 8 px; RC_ESIZE beyond the context's size.  One launch ("trackstab@5"), asynchronous. */
#define RC_CORNER_MAX_CELLS 4096
int rcflow_corners_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, int w, int h, int cells_x, int cells_y,
                       int margin, int min_score, float* d_pts, int* d_scores);

/* ROBUST FIT.  From n <= RC_FIT_MAX_POINTS pairs p_i -> q_i (float x, y), a status byte and optionally a score each, the
 * 3 x 3 double T with q ~ T p, by RANSAC whose sampler is a stated function of (seed, hypothesis, draw): the result is a
 * function of the input.  Everything below is fp64, one rounding per written operation (no fused multiply-add).
 *   valid      status == 1, |q - p|^2 <= max_shift^2 (NaN fails) and, when scores are given, score > 0, score >= min_score
 *              and score >= quality * (the largest of all n scores).  The valid pairs keep their input order.
 *   sampler    mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32).
 *              draw(seed, j, d) = mix(mix(seed + 0x9E3779B9 (j + 1)) + 0x85EBCA6B (d + 1)); index = draw * n_valid >> 32
 *              (64-bit product).  Hypothesis j takes draws d = 0, 1, ... and skips an index it already holds; without its
 *              k distinct indices after 16 draws, or with n_valid < k, it is void (0 inliers).  k = 1, 2, 3, 4 pairs for
 *              RC_STAB_TRANSLATION, _SIMILARITY, _AFFINE, _HOMOGRAPHY.
 *   coordinates  S = max(w, h), c = (w / 2, h / 2): P = (p - c) / S, Q = (q - c) / S, D = (q - p) / S.  The DISPLACEMENT
 *              is fitted, E = T_norm - I, so a still scene gives T = I exactly.
 *   solve      translation: E = [0 0 mean Dx; 0 0 mean Dy].  Similarity / affine: the closed forms of
 *              rcflow_framestab_open_multi above on P centred on its mean and D centred on its mean (affine needs
 *              det > 1e-12 Sxx Syy, similarity Sxx + Syy > 0).  Homography: unknowns z = (e00 e01 e02 e10 e11 e12 g0 g1),
 *              rows [Px Py 1 0 0 0 -Qx Px -Qx Py | Dx] and [0 0 0 Px Py 1 -Qy Px -Qy Py | Dy]; the minimal sample is the
 *              8 x 8 system solved by Gaussian elimination with partial pivoting (first largest |pivot|; void below 1e-9),
 *              row update m[r][k] - f m[c][k] with f = m[r][c] / m[c][c], back substitution s - m[c][k] z[k] for
 *              ascending k.  A least-squares homography solves the normal equations (entry (r, k) = sum of
 *              r1[r] r1[k] + r2[r] r2[k]) by the same elimination (fails below 1e-12).
 *   to pixels  F[i][0] = E[i][0] / S, F[i][1] = E[i][1] / S, F[i][2] = E[i][2] - (E[i][0] cx + E[i][1] cy) / S;
 *              G[0][j] = S F[0][j] + cx F[2][j], G[1][j] = S F[1][j] + cy F[2][j], G[2][j] = F[2][j]; T = I + G; a
 *              homography is divided by T[8], which must exceed 0.1.  Any entry not finite: the solve failed.
 *   inlier     X = (T0 px + T1 py) + T2, Y, W likewise; W > 0 and (X / W - qx)^2 + (Y / W - qy)^2 <= inlier_px^2.
 *   best       most inliers, ties to the lowest hypothesis index.
 *   refit      by the workgroup that finishes last: least squares of the model on the winner's inliers, recount under
 *              the refit, refit again, recount.  Sums run over the valid list in a fixed order: partial sum t of 256 adds
 *              the terms of the pairs t, t + 256, ... (0.0 for a pair that is no inlier); each group of 64 partial sums is
 *              folded by halves (v[i] + v[i + 32], then 16, ... 1); the four results are added as ((s0 + s1) + s2) + s3.
 *   ladder     the model needs max(2 k, k + 2) inliers after the refits (3, 4, 6, 8) and solves that succeed; else the
 *              next simpler model is fitted once to the inliers at hand and recounted, down to the identity with
 *              model_used = 0 (the inliers are then those of the identity).  When every hypothesis is void (all samples
 *              degenerate, e.g. collinear pairs under RC_STAB_AFFINE) there is no inlier to step down with: the identity.
 * Defaults: hypotheses 0 = RC_FIT_DEFAULT_HYPOTHESES, max_shift 0 = 0.1 max(w, h), inlier_px 0 = 1.  Output on the
 * device: *d_result, d_inlier[n] (1 for an inlier of the final T), d_samples (may be NULL) = hypotheses x 4 input
 * indices, -1 where unused or void.  RC_EINVAL: n outside 0..RC_FIT_MAX_POINTS, an unknown model, hypotheses beyond
 * RC_FIT_MAX_HYPOTHESES, a gate that is negative or not finite, quality outside 0..1, a null pointer.  One launch
 * ("trackstab@4"), asynchronous; calls on one slot are ordered by its stream. */
#define RC_STAB_HOMOGRAPHY 4
#define RC_FIT_MAX_POINTS 4096
#define RC_FIT_MAX_HYPOTHESES 4096
#define RC_FIT_DEFAULT_HYPOTHESES 512
typedef struct rc_fit_params {
    int model, hypotheses;
    unsigned seed;
    int min_score;
    double quality, max_shift, inlier_px;
} rc_fit_params;
typedef struct rc_fit_result {
    double T[9];
    int model_used, n_valid, n_inliers, winner;
} rc_fit_result;
int rcflow_fit_motion_dev(rc_ctx* ctx, int stream, const float* d_p, const float* d_q, const uint8_t* d_status,
                          const int* d_scores /* may be NULL */, int n, int w, int h, const rc_fit_params* prm,
                          rc_fit_result* d_result, uint8_t* d_inlier, int* d_samples /* may be NULL */);

/* A stabilisation slot that finds its own points: corners of the reference frame, tracked into the incoming frame by the
 * sparse PyrLK of rcflow_pyrlk_dev, a robust fit of the tracks, the warp.  Served by rcflow_framestab_push_dev / _read /
 * _reset / _close like the other two forms; no host synchronisation and no device-to-host copy in a push:
 *   gray of the incoming frame (COLOR_BGR2GRAY, 14-bit fixed point)   "trackstab@0"
 *   its pyramid                                                        "trackstab@1" per level
 *   PyrLK from the kept corners of the reference frame                 "trackstab@3" (err not computed, min eigenvalue 1e-4)
 *   the fit above on (corner, track, status, corner score)             "trackstab@4"
 *   dst(p) = src(T p): the affine warp ("framestab@8") or, when the model asked for is RC_STAB_HOMOGRAPHY, the
 *   perspective warp ("framestab@9"), reading T from device memory
 *   unless RC_STAB_ANCHOR_FIRST: gray, pyramid, Scharr derivatives ("trackstab@2") and corner cells ("trackstab@5") of
 *   the CORRECTED frame, kept for the next push.  Anchored, those of the first frame are kept for good.
 * cells 0 x 0: cells of about `side` x `side` px, side = 40 raised in steps of 8 until round(w / side) round(h / side)
 * <= RC_CORNER_MAX_CELLS (16 x 12 at 640 x 480).  margin = win / 2 + 2.  win 0: 21; max_level < 0: 3; max_count 0: 30;
 * epsilon 0: 0.01; min_score 0: 1.  The first push after open / reset copies the frame and reports the identity and zeros.
 * rcflow_framestab_read / d_result give the displacement of the frame centre under T and n_inliers / n_valid (0 when
 * none).  rcflow_framestab_read_motion returns the 2 x 3 of T, RC_EINVAL when the model used was a homography;
 * rcflow_framestab_info_multi reports n = 0; rcflow_framestab_info reports roi = the candidate rectangle.
 * RC_EINVAL: a bad frame size, a null params, win even or outside 3..63, max_level > 7, an unknown model or flag bit, gates
 * as rcflow_fit_motion_dev, cells as rcflow_corners_dev; RC_ESIZE beyond the context's size.  A refused open leaves the
 * slot's state as it was. */
typedef struct rc_stab_tracks {
    int cells_x, cells_y;
    int min_score; double quality;
    int win, max_level, max_count; double epsilon;
    double max_shift;
    int model, hypotheses; unsigned seed; double inlier_px;
    int flags;
} rc_stab_tracks;
int rcflow_framestab_open_tracks(rc_ctx* ctx, int stream, int w, int h, const rc_stab_tracks* prm);
/* Blocks until the slot's stream has finished.  Any pointer may be NULL.  pts = min(cells, cap) x (px, py, qx, qy): the
 * corner in the reference frame and its track in the last frame pushed; inlier = one byte each; cells = their number.
 * Before the second push: the identity and zeros.  RC_ESTATE unless the slot was opened by rcflow_framestab_open_tracks. */
int rcflow_framestab_read_tracks(rc_ctx* ctx, int stream, double T[9], int* model_used, int* n_valid, int* n_inliers,
                                 float* pts, uint8_t* inlier, int* scores, int cap, int* cells, long long* frames_pushed);

/* ------------------------------------------------------------------ time-exposure images
 * compute_timex (main.cpp:1195-1263) and compute_brightColor (main.cpp:1265-1383) on frames resident on the device.
 * All images are 8UC3; "channel 0 / 1 / 2" are the bytes as they come (the reference feeds BGR frames to
 * COLOR_RGB2HSV and back through COLOR_HSV2RGB, so byte 0 plays "R" both ways).
 *   RC_TIMEX_MEAN     sum (fp32) += frame; out = convertTo(8U) of sum * (float)(1.0 / n), n = frames so far (:1231-1241).
 *   The ring products keep the last `window` frames in HSV (all zero at open), slot c = (frames so far) % window
 *   written before the product is taken (:1305-1363), with q(v) = convertTo(8U) of v * (float)(1.0 / window):
 *   RC_TIMEX_AVERAGE  per channel min(255, sum of q(slot)) -- the reference's saturating adds of non-negative terms;
 *   RC_TIMEX_BRIGHT   the triple of the slot with the largest V, RC_TIMEX_DARK the smallest, where slot 0 takes part
 *                     DIVIDED (q of all three channels: the reference seeds with buffer_hsv[0] / windowSize) and the
 *                     lowest slot index wins ties (its walk replaces on strictly better only).
 * Every product is the bits of the reference's rescan of the whole ring, kept incrementally: bytes per frame do not
 * grow with the window, except that a pixel whose BRIGHT / DARK winner is overwritten by a worse sample walks the V
 * plane of the ring again.  When profiling is on the launches are recorded as "timex@0" (mean) and "timex@1" (ring
 * products), the stage kernels below as "frame_color@0..1", the colour resizes as "frame_color@2..3"; rcflow_profile_read_buckets books them under "overlay". */
#define RC_TIMEX_MEAN 1      /* main.cpp:1195-1263 */
#define RC_TIMEX_AVERAGE 2   /* main.cpp:1265-1383, option 0 */
#define RC_TIMEX_BRIGHT 4    /* option 1 */
#define RC_TIMEX_DARK 8      /* option 2 */
/* Opens the slot's time-exposure state for w x h frames: `products` is a mask of the above; the three ring products
 * share one ring of `window` frames (1..4096; ignored for MEAN alone).  Allocates everything it will ever need
 * (window * 3 bytes per pixel for the ring; RC_ENOMEM with the byte count in rcflow_last_error if it does not fit);
 * re-opening replaces the state, and a refused open (RC_ENOMEM included) leaves the open state as it was: the new state is
 * allocated before the old one is freed, so both are resident for the length of a re-open (rcflow_timex_close first
 * where two rings do not fit).  RC_EINVAL for a bad mask or window, RC_ESIZE beyond the context's max_w x max_h.
 * The state is zeroed asynchronously on the stream the slot has at this call (so does rcflow_timex_reset).  The first
 * push after it waits for that zeroing even if rcflow_set_hip_stream moved the slot in between; beyond that, as for
 * every entry point, work queued on the slot's former stream is the caller's to order when the slot changes stream. */
int rcflow_timex_open(rc_ctx* ctx, int stream, int w, int h, int window, int products);
/* One frame: d_frame 8UC3 of the opened size.  d_out[4]: device 8UC3 images for MEAN, AVERAGE, BRIGHT, DARK in that
 * order; an entry (or d_out itself) may be NULL: the state is still updated.  RC_EINVAL for an entry of a product that
 * is not open, for a step below 3 * w, and for an output that overlaps the frame or another output (in place is not
 * supported); RC_ESTATE before rcflow_timex_open.  Asynchronous on the slot's stream, one launch for MEAN and one for
 * all ring products. */
int rcflow_timex_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_frame, size_t step,
                          uint8_t* const d_out[4], const size_t out_step[4]);
/* zeroes sums, ring, slot index and frame count; keeps the allocation */
int rcflow_timex_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_timex_close(rc_ctx* ctx, int stream);
/* any pointer may be NULL; window is 0 for MEAN alone; device_bytes = everything the state holds on the device.
 * RC_ESTATE when nothing is open on the slot. */
int rcflow_timex_info(rc_ctx* ctx, int stream, int* w, int* h, int* window, int* products,
                      long long* frames_pushed, size_t* device_bytes);
/* cvtColor(COLOR_RGB2HSV) and cvtColor(COLOR_HSV2RGB) on 8UC3 images (color_hsv.cpp, hue range 180), the stages of
 * the ring products: integer forward (H = hue / 2, S, V in 0..255), through float back; a hue byte above 179 wraps.
 * In place (same pointer and step) is allowed. */
int rcflow_rgb_to_hsv_u8_dev(rc_ctx* ctx, int stream, const uint8_t* d_rgb, size_t step, int w, int h,
                             uint8_t* d_hsv, size_t hsv_step);
int rcflow_hsv_to_rgb_u8_dev(rc_ctx* ctx, int stream, const uint8_t* d_hsv, size_t hsv_step, int w, int h,
                             uint8_t* d_rgb, size_t step);

/* ------------------------------------------------------------------ opposing-flow map
 * Where does the water run against the waves?  averageVector (ripcurrents_module.cpp:386-484; its call is commented out at
 * main_old.cpp:352) finished: a window mean of the flow field, a global direction, a grid of cells, and the cells whose
 * summed mean vector points away from the global one.  One launch per push ("ripmap@0"; "ripmap@1" only for a mask),
 * nothing synchronises.  Per pixel:
 *   v      the flow (source 0, main.cpp:1142-1153), or get_delta from a zero point with dt = 2 and the slot's UPPER
 *          (source 1, ripcurrents_module.cpp:395-397: rcflow_get_delta_field_dev's arithmetic; needs rcflow_analysis_reset);
 *   mean   a = avg - slot * inv; slot = v; avg = a + v * inv, inv = 1 / window: the bits of a chain of
 *          rcflow_window_mean_dev calls over a ring the library owns ([window][h][w rounded up to 2] float2);
 *   sums   q = (int64)rint(avg * 65536) per component, added per cell with the cell's pixel count n; a pixel with a
 *          component that is not finite or beyond 2^40 in |q| (2^24 px) is left out and counted as bad.  Integer sums do
 *          not depend on the order of addition.  Cell of pixel (x, y): (min(x / (w / grid_x), grid_x - 1), likewise y):
 *          the reference's integer cell size, the remainder columns and rows going to the last cell;
 *   colour rcflow_vector_to_color_dev's triple of the mean, scaled by the PREVIOUS push's maximum |avg| (the first push:
 *          the reference's 1e-6); this push's maximum stays on the device for the next one.
 * Then the launch's last-arriving workgroup: G = the sum of all cells' (Sx, Sy); for every cell, in double, each
 * operation rounded on its own: dot = Sx*Gx + Sy*Gy, cc = Sx*Sx + Sy*Sy, gg = Gx*Gx + Gy*Gy;
 *   opposed  iff  n > 0 && dot < 0 && dot*dot > K*(cc*gg) && cc >= ((M*65536)*n)^2
 * K = min_opposition_cos2 (default 0.3454915028125263 = cos^2(0.7 pi), ripcurrents_module.cpp:471), M = min_cell_mag
 * (px, default 0: off).
 *   cells    grid_y x grid_x x (mean x, mean y, angle to G in degrees [0, 180], opposed ? 1 : 0) floats,
 *            means as (float)((double)S / 65536 / n), zeros for an empty cell;
 *   summary  8 doubles: direction of G in degrees [0, 360), |mean of the frame| in px, opposed cells, cells with n > 0,
 *            bad pixels, frames pushed, this push's maximum |avg|, 0.
 * Angles are atan2 in double and for people (tolerance 1e-9 degrees); no decision depends on them.  While fewer than
 * `window` fields have been pushed the mean is a partial one (zeros in the unfilled slots, as the reference's);
 * RC_RIPMAP_WAIT_FULL holds every cell at "not opposed" until the ring is full.
 * THE RING IS window * h * w * 8 BYTES: 5 GB for the reference's 300 fields at 1080p, 0.74 GB at 640 x 480. */
#define RC_RIPMAP_WAIT_FULL 1      /* flags bit 0 */
#define RC_RIPMAP_MAX_CELLS 16384
/* Opens the slot's map for w x h fields.  Allocates everything it will ever need (RC_ENOMEM with the byte count in
 * rcflow_last_error if it does not fit); re-opening replaces the state, a refused open leaves it as it was (as
 * rcflow_timex_open: old and new state are resident together for the length of a re-open).  RC_EINVAL:
 * window outside 1..4096, a grid below 1 x 1, wider or higher than the frame (w < grid_x, h < grid_y) or beyond
 * RC_RIPMAP_MAX_CELLS cells, source other than 0 / 1, unknown flag bits; RC_ESIZE beyond the context's max_w x max_h.
 * Zeroed asynchronously on the stream the slot has at this call; stream rules as rcflow_timex_open. */
int rcflow_ripmap_open(rc_ctx* ctx, int stream, int w, int h, int window, int grid_x, int grid_y, int source, int flags);
/* One field.  d_flow_xy: CV_32FC2 of the opened size (flow_step a multiple of 8), or NULL: the field the slot's frame
 * loop left resident (rcflow_stream_flow_ptr: after rcflow_push_frame_u8 / _acquired / rcflow_frame_loop_step; RC_ESTATE
 * when there is none, RC_ESIZE when it has another size).
 * Each output may be NULL: d_hsv 8UC3 (h x w), d_mask h x w bytes, 255 inside an opposed cell (what
 * rcflow_create_edges_dev / rcflow_create_output_dev take; costs the second launch), d_cells and d_summary as above.
 * The state is updated whatever is asked for.  RC_ESTATE before rcflow_ripmap_open; a refused push changes nothing. */
int rcflow_ripmap_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, uint8_t* d_hsv,
                           size_t hsv_step, uint8_t* d_mask, size_t mask_step, float* d_cells, double* d_summary);
/* Copies the window mean as it stands (CV_32FC2, mean_step >= 8 * w) to device memory, asynchronously on the slot's
 * stream: the field rcflow_vector_to_color_dev, rcflow_subtract_average_dev ... take. */
int rcflow_ripmap_mean_dev(rc_ctx* ctx, int stream, float* d_mean_xy, size_t mean_step);
/* Blocks until the slot's stream has finished; for hosts and tests.  cells, summary as above; sums: grid_y x grid_x x
 * (Sx, Sy, n) int64 of the last push.  Any pointer may be NULL.  Before the first push: zeros. */
int rcflow_ripmap_read(rc_ctx* ctx, int stream, float* cells, double* summary, long long* sums, long long* frames_pushed);
/* the decision's two numbers, from the next push on.  RC_EINVAL unless 0 <= min_opposition_cos2 < 1 and
 * 0 <= min_cell_mag < 1e6; open restores the defaults, reset keeps what was set. */
int rcflow_ripmap_set(rc_ctx* ctx, int stream, double min_opposition_cos2, double min_cell_mag);
/* zeroes ring, mean, maximum and frame count; keeps the allocation and what rcflow_ripmap_set set */
int rcflow_ripmap_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_ripmap_close(rc_ctx* ctx, int stream);
/* any pointer may be NULL; device_bytes = everything the state holds on the device.  RC_ESTATE when nothing is open. */
int rcflow_ripmap_info(rc_ctx* ctx, int stream, int* w, int* h, int* window, int* grid_x, int* grid_y, int* source,
                       int* flags, double* min_opposition_cos2, double* min_cell_mag, long long* frames_pushed,
                       size_t* device_bytes);

/* ------------------------------------------------------------------ drawing: discs and lines into 8-bit images
 * What circle(..., FILLED), line(..., thickness, 8) and the addWeighted(overlay, .5, img, .5) of the tracer pipelines leave
 * in a frame (Streakline.cpp:57-66, ripcurrents_module.cpp:800-805, :1186-1194, :522), painted on the device.  The painting
 * rules are this library's own, in integers only; they are NOT a restatement of OpenCV's drawing.cpp (DESIGN 7f says
 * where they are known to differ):
 *  - order: primitives paint in list order; a later one overwrites (or blends over) an earlier one;
 *  - disc of radius r at (x0, y0): pixel (x, y) is lit iff (x - x0)^2 + (y - y0)^2 <= r^2 + r (radius r + 1/2);
 *  - line of thickness 1 from (x0, y0) to (x1, y1), 8-connected: with adx = |x1 - x0| >= ady = |y1 - y0|, for every x
 *    between the ends the one pixel y = y0 + sgn(y1 - y0) * ((2 ady |x - x0| + adx) / (2 adx)) (integer division); the steep
 *    case with x and y exchanged; a zero-length line is its one pixel.  Not symmetric in its ends;
 *  - line of thickness t = 2..8: lit iff 4 d^2 <= t^2, d the exact distance from the pixel centre to the segment
 *    (projection inside the segment: 4 cross^2 <= t^2 |b|^2; outside: the distance to the nearer end);
 *  - blend (RC_DRAW_BLEND): per channel p <- cvRound(0.5 c + 0.5 p), half to even: s = c + p, s >> 1 for even s, else
 *    (s >> 1) + ((s >> 1) & 1); only covered pixels change;
 *  - a primitive with a coordinate beyond |v| <= RC_DRAW_COORD_MAX, a radius outside 0..RC_DRAW_COORD_MAX, a thickness
 *    outside 1..RC_DRAW_MAX_THICKNESS or an unknown kind is skipped and counted, never clamped.  Within the bound no product
 *    of the tests leaves 64 bits.  Primitives may lie partly or wholly off the image;
 *  - a pixel no primitive covers keeps its bytes: a lane that covers nothing stores nothing, so row padding is never written.
 * Colour: byte0 | byte1 << 8 | byte2 << 16, the 8UC3 pixel's bytes in memory order (CV_RGB(r, g, b) is b | g << 8 | r << 16);
 * a 1-channel image takes byte0. */
#define RC_DRAW_DISC 1
#define RC_DRAW_LINE 2
#define RC_DRAW_BLEND 1            /* rc_draw_prim::flags */
#define RC_DRAW_COORD_MAX 16383
#define RC_DRAW_MAX_THICKNESS 8
#define RC_DRAW_MAX_PRIMS (1 << 24)
typedef struct rc_draw_prim {      /* 32 bytes */
    int32_t kind;                  /* RC_DRAW_DISC | RC_DRAW_LINE */
    int32_t x0, y0;                /* the centre; a line's first end */
    int32_t x1, y1;                /* a line's second end (a disc ignores them) */
    int32_t size;                  /* radius; thickness */
    uint32_t color;
    uint32_t flags;                /* RC_DRAW_BLEND */
} rc_draw_prim;
/* Stage: paints n primitives (device memory) into a w x h image of 1 or 3 channels in place, on the slot's stream.  One
 * launch ("tracers@1"): a workgroup per 64 x 16 tile gathers the primitives whose box meets the tile, in list order, and
 * every pixel is painted by the one lane that owns it; no atomics, no scratch.  d_skipped (optional, device) is
 * INCREASED by the number of skipped primitives.  w, h <= RC_DRAW_COORD_MAX + 1, n <= RC_DRAW_MAX_PRIMS (RC_ESIZE beyond);
 * n = 0 launches nothing. */
int rcflow_draw_dev(rc_ctx* ctx, int stream, uint8_t* d_img, size_t step, int w, int h, int channels,
                    const rc_draw_prim* d_prims, int n, unsigned long long* d_skipped);
/* Stage: the d_trace of rcflow_advect_points_dev as thin lines, what the pathline overlay paints with
 * cv::line(overlay, *pt, newpt, color, 1) per step (ripcurrents_module.cpp:522, :563, :600).  d_start (optional): the n
 * seeds before the advection; with it seed s gives iters lines (start -> step 0 -> ...), without it iters - 1.  Seed after
 * seed, step after step, into d_prims (n * (iters - (d_start ? 0 : 1)) records).  Coordinates are ROUNDED half to even
 * (the Point2f -> Point conversion of that call; a value that is not finite or beyond int32 becomes INT32_MIN and is
 * skipped by the drawing).  "tracers@2". */
int rcflow_trace_prims_dev(rc_ctx* ctx, int stream, const float* d_start, const float* d_trace, int n, int iters,
                           uint32_t color, rc_draw_prim* d_prims);

/* ------------------------------------------------------------------ tracer lines: streaklines, timelines, point clouds
 * compute_streaklines / compute_timelines / compute_populationMap (main.cpp:78-176; Streakline.cpp:22-71,
 * ripcurrents_module.cpp:751-807, :1140-1196) with every vertex of every line of a stream resident on the device.  Per
 * push, on the slot's stream, with no host synchronisation and no device-to-host copy:
 *   1. move.  RC_TRACERS_LK: pyramid and Scharr derivatives of the incoming gray frame only, ONE sparse PyrLK launch over
 *      all vertices of all lines from the kept pyramid of the previous frame, then the pyramids swap.  The first push (and
 *      the first after a reset) primes: nothing moves, nothing is drawn, the call returns 1.  RC_TRACERS_FLOW: one step of
 *      rcflow_advect_points_dev's variant 4 with the slot's dt on the caller's field or the slot's resident one;
 *   2. book-keeping and primitives, one launch ("tracers@0").  Streakline: a moved vertex with |dx| > 0.1 w or
 *      |dy| > 0.1 h (float difference, compared in double) keeps its old position, then the generation point becomes the
 *      newest vertex.  Timeline, cloud: every vertex takes its moved position, whatever PyrLK's status says.  The
 *      primitives, in the reference's painting order, with coordinates TRUNCATED toward zero (Point(float, float)):
 *      streakline: disc 3 CV_RGB(0,100,0) at the generation point, line to vertex 0, disc 2 CV_RGB(0,0,100) at vertex 0,
 *      per edge a disc 2 at its far vertex and a line CV_RGB(100,0,0); timeline: disc 4, per edge a line of thickness 2 and
 *      a disc 4; cloud: per vertex a disc 10 CV_RGB(100,0,0) blended at 0.5;
 *   3. draw (rcflow_draw_dev's launch) into d_canvas, when one is given.
 * Deviation: the reference's streakline grows without bound; here it is a ring of max_vertices, and once full every push
 * drops the oldest vertex (counted in rcflow_tracers_info).  The host knows every count without reading the device. */
#define RC_TRACERS_LK 0
#define RC_TRACERS_FLOW 1
#define RC_TRACER_STREAK 0
#define RC_TRACER_TIMELINE 1
#define RC_TRACER_CLOUD 2
#define RC_TRACERS_MAX_LINES 256
#define RC_TRACERS_MAX_POINTS (1 << 20)
typedef struct rc_tracers_params {
    int mover;          /* RC_TRACERS_LK | RC_TRACERS_FLOW */
    int max_lines;      /* 1..RC_TRACERS_MAX_LINES */
    int max_vertices;   /* ring length of a streakline, >= 2 */
    int max_points;     /* all vertices of the session together, <= RC_TRACERS_MAX_POINTS; 0: max_lines * max_vertices */
    /* LK mover; win_w = 0 takes the reference's whole call (Streakline.cpp:32): 50 x 50, 3, COUNT+EPS, 30, 0.1, flags 10, 1e-4 */
    int win_w, win_h, max_level, crit_type, max_count, lk_flags;
    double epsilon, min_eig;
    float dt;           /* FLOW mover */
} rc_tracers_params;
typedef struct rc_tracers_info {
    int w, h, mover, max_lines, max_vertices, max_points;
    int lines, points, prims;          /* as they stand; prims: of the last drawing push */
    int primed;                        /* LK mover: a previous frame is held */
    long long pushes;                  /* moves since open / reset (a priming push is none) */
    long long dropped;                 /* streakline vertices the rings have let go */
    size_t device_bytes;
} rc_tracers_info;
/* Allocates the state on the slot.  Re-opening replaces it; a refused open leaves the open state as it was. */
int rcflow_tracers_open(rc_ctx* ctx, int stream, int w, int h, const rc_tracers_params* prm);
/* Adds a line from n host points (x, y) and returns its id (0, 1, ...), or a negative code.  RC_TRACER_STREAK: n = 1, the
 * generation point; RC_TRACER_TIMELINE, RC_TRACER_CLOUD: the n vertices.  Lines paint in the order they were added.
 * Blocking (a set-up call): it waits for the slot's stream.  RC_ESIZE when max_lines or max_points would be passed
 * (a streakline reserves max_vertices points). */
int rcflow_tracers_add(rc_ctx* ctx, int stream, int kind, const float* xy, int n);
/* One frame.  d_gray (8UC1, w x h): LK mover, else ignored.  d_flow_xy (32FC2): FLOW mover, NULL = the slot's resident
 * field (RC_ESTATE when there is none, RC_ESIZE when its size differs).  d_canvas (8UC3, w x h, drawn in place): optional.
 * Every refusal is decided before anything is queued and leaves the session as it was.  Returns RC_OK, or 1 from a
 * priming push. */
int rcflow_tracers_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t gray_step, const float* d_flow_xy,
                            size_t flow_step, uint8_t* d_canvas, size_t canvas_step);
/* Blocks until the slot's stream has finished; for hosts and tests.  The vertices of `line` in the reference's order
 * (a streakline newest first) into xy (cap points; RC_ESIZE when it holds more), their number into n; skipped (may be
 * NULL): primitives the session's drawing has skipped since open / reset. */
int rcflow_tracers_read(rc_ctx* ctx, int stream, int line, float* xy, int cap, int* n, long long* skipped);
/* The primitives of the last push (device memory owned by the session, valid until the next call on it) and their number:
 * for a caller that paints them elsewhere with rcflow_draw_dev.  Either pointer may be NULL. */
int rcflow_tracers_prims(rc_ctx* ctx, int stream, const rc_draw_prim** d_prims, int* n);
/* never blocks; RC_ESTATE when nothing is open */
int rcflow_tracers_info(rc_ctx* ctx, int stream, rc_tracers_info* info);
/* Back to the lines as they were added: every line keeps its id and its first vertices, the counters and the skipped word
 * are zero, the LK mover primes again.  Asynchronous, on the slot's stream. */
int rcflow_tracers_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_tracers_close(rc_ctx* ctx, int stream);

/* ------------------------------------------------------------------ rip regions: connected components, labelled and measured
 * From pixels to detections: the components of a mask (the outmask of rcflow_classify_accumulate_dev, the d_mask of
 * rcflow_ripmap_push_dev) numbered, filtered by area and measured on the device.  A push is SEVEN launches
 * ("regions@0" .. "regions@6") whatever the mask holds, with no host synchronisation and no device-to-host copy;
 * rcflow_regions_prims_dev is one more ("regions@7").  All integers are exact and do not depend on the order of addition.
 *
 * Input per push: d_mask, 8UC1, w x h, step >= w; a pixel is foreground iff its byte is non-zero (1 and 128 count like
 * 255).  Optionally d_flow_xy (CV_32FC2, 8-byte aligned, flow_step a multiple of 8), or NULL: no flow statistics (zeros).
 * Connectivity 4 or 8, fixed at open.
 *  1. Components.  Maximal 4- or 8-connected sets of foreground pixels.  first(C) = the smallest y * w + x of a
 *     component.  Components are numbered 1, 2, ... in increasing order of first (raster order of first appearance: the
 *     numbering of scipy.ndimage.label with the cross / the full 3 x 3 structure).
 *  2. Filter.  area(C) = number of pixels.  Components with area < min_area are dropped; the kept ones are renumbered
 *     1..K in the same order.  min_area = 1 keeps everything.
 *  3. Outputs of a push (device memory, each may be NULL; the state is updated whatever is asked for):
 *     d_labels   int32 h x w (4-byte aligned, labels_step a multiple of 4, >= 4 w): the kept number of the pixel's
 *                component, 0 for background and for dropped components.  All K numbers appear, also beyond max_regions.
 *     d_mask_out 8UC1: 255 where d_labels would be non-zero, else 0 (an area opening: what rcflow_create_edges_dev /
 *                rcflow_create_output_dev take next).  It may be d_mask itself with the same step (in place); any other
 *                overlap of the byte ranges [first byte, past the last) of an input or output with another output is RC_EINVAL.
 *     d_regions  max_regions records rc_region (8-byte aligned), the first min(K, max_regions) kept components in
 *                order; the rest of the array is zero bytes.
 *     d_summary  8 int64: components before the filter, K, records written, foreground pixels, pixels in kept
 *                components, flow pixels left out as bad (kept components only, also those beyond max_regions), pushes
 *                since open / reset (this one included), largest kept area.
 *     Row padding of every output is never written.
 *  4. rc_region: the integer part: label, area, the inclusive box x0, y0, x1, y1, first_x, first_y, edges (bit 0..3:
 *     touches column 0, row 0, column w - 1, row h - 1), bad; sx, sy, sxx, syy, sxy: sums of x, y, x*x, y*y, x*y over its
 *     pixels; fx, fy: sums of q = (int64)rint(v * 65536) per flow component over its pixels, where a pixel with a
 *     component that is not finite or with |q| > 2^40 is left out of both sums and counted in bad: the rule and the
 *     scale of rcflow_ripmap_* ("sums" above), so a region's mean flow and a cell's mean flow are the same kind of number.
 *     The derived part, in double, each operation rounded on its own (no fused multiply-add), n = area, m = n - bad:
 *       cx = sx / n;  cy = sy / n;
 *       mean_fx = m ? (float)(fx / 65536 / m) : 0;  mean_fy likewise;
 *       mxx = sxx / n - cx * cx;  myy = syy / n - cy * cy;  mxy = sxy / n - cx * cy;
 *       t = (mxx + myy) * 0.5;  d = (mxx - myy) * 0.5;  r = sqrt(d * d + mxy * mxy);
 *       var_major = t + r;  var_minor = t - r   (px^2; rounding may leave var_minor a hair below 0);
 *       angle = atan2(mxy, d) * 0.5 * (180 / pi), + 180 when negative, 0 when that gives 180: the major axis, degrees in
 *       [0, 180), x to the right and y DOWN.
 *     The derived part is for people: no decision in the library depends on it.
 *  5. Primitives.  rcflow_regions_prims_dev turns the records of the last push into 6 * max_regions primitives for
 *     rcflow_draw_dev, record after record: the four box edges as lines of `thickness` (top (x0,y0)-(x1,y0), right
 *     (x1,y0)-(x1,y1), bottom (x1,y1)-(x0,y1), left (x0,y1)-(x0,y0)), a disc of disc_radius at the centroid rounded in
 *     integers (px = (2 sx + n) / (2 n), py likewise), and, when flow_scale != 0 and n > bad, a line of `thickness` from
 *     there to (px + (int32)rint(fx / 65536 / m * flow_scale), py + ...) with the mean taken in double as above (a step
 *     that is not finite or beyond 2^30 gives the coordinate INT32_MIN, which the drawing skips).  Slots without a record
 *     (and the flow line when it is off) are all-zero records, kind = 0: rcflow_draw_dev skips them as an unknown kind AND
 *     COUNTS THEM in d_skipped when one is given.  The count is fixed, so the host never reads the device to know it. */
typedef struct rc_regions_params {
    int connectivity;   /* 4 | 8 */
    int min_area;       /* >= 1 */
    int max_regions;    /* 1..RC_REGIONS_MAX */
    int flags;          /* 0 */
} rc_regions_params;
#define RC_REGIONS_MAX 65536
#define RC_REGIONS_LAUNCHES 7      /* per push, whatever the mask holds */
typedef struct rc_region {         /* 144 bytes */
    int32_t label, area;
    int32_t x0, y0, x1, y1;
    int32_t first_x, first_y;
    int32_t edges, bad;
    int64_t sx, sy, sxx, syy, sxy;
    int64_t fx, fy;
    double cx, cy;
    double var_major, var_minor, angle;
    float mean_fx, mean_fy;
} rc_region;
typedef struct rc_regions_info {
    int w, h, connectivity, min_area, max_regions, flags;
    int launches_per_push;             /* RC_REGIONS_LAUNCHES */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_regions_info;
/* Allocates everything the slot will ever need (labels and area scratch: 4 bytes per pixel each; RC_ENOMEM with the
 * byte count in rcflow_last_error).  Re-opening replaces the state; a refused open leaves the open state as it was.
 * RC_EINVAL: connectivity other than 4 / 8, min_area < 1, max_regions outside 1..RC_REGIONS_MAX, unknown flag bits, a
 * frame of 2^31 pixels or more; RC_ESIZE beyond the context's max_w x max_h. */
int rcflow_regions_open(rc_ctx* ctx, int stream, int w, int h, const rc_regions_params* prm);
/* One mask.  Every refusal is decided before anything is queued and leaves the state as it was. */
int rcflow_regions_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_mask, size_t mask_step,
                            const float* d_flow_xy, size_t flow_step,
                            int32_t* d_labels, size_t labels_step, uint8_t* d_mask_out, size_t mask_out_step,
                            rc_region* d_regions, long long* d_summary);
/* 6 * max_regions primitives from the records of the last push (before the first push: all kind 0) into d_prims.
 * RC_EINVAL: thickness outside 1..RC_DRAW_MAX_THICKNESS, disc_radius outside 0..RC_DRAW_COORD_MAX, flow_scale not finite. */
int rcflow_regions_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, double flow_scale,
                             rc_draw_prim* d_prims);
/* Blocks until the slot's stream has finished; for hosts and tests.  The records of the last push: min(cap, records
 * written) of them into regions, records written into n, the summary; any pointer may be NULL.  Before the first push: zeros. */
int rcflow_regions_read(rc_ctx* ctx, int stream, rc_region* regions, int cap, int* n, long long summary[8]);
/* min_area from the next push on (RC_EINVAL below 1); open restores the parameter, reset keeps what was set */
int rcflow_regions_set(rc_ctx* ctx, int stream, int min_area);
/* zeroes the kept records, the summary and the push count; asynchronous, on the slot's stream */
int rcflow_regions_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_regions_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open */
int rcflow_regions_info(rc_ctx* ctx, int stream, rc_regions_info* info);

/* ------------------------------------------------------------------ rip tracks: regions followed from push to push
 * The numbers of rcflow_regions_* are raster-order numbers of one mask.  This state gives every region an identity that
 * lasts: it consumes the device outputs of rcflow_regions_push_dev (label image, records, summary), keeps a table of tracks
 * with hits, misses and confirmation, and emits a mask of the confirmed regions that does not flicker with the input.  A push
 * is SIX launches ("tracks@0" .. "tracks@5") whatever the labels hold, with no host synchronisation and no device-to-host
 * copy; rcflow_tracks_prims_dev is one more ("tracks@6").  The rules are integer-only: nothing depends on the order of
 * atomics, and numbers are given by rank, never by arrival.
 *
 * State: the footprint P, int32 [h][w]: slot + 1 of the track that last covered the pixel, or 0; the table of max_tracks
 * records rc_track (a free slot is all zero bytes, a used one has id >= 1); next_id (1 after open / reset); the push count
 * (on the device, so a captured launch sequence stays valid); the overlap table [max_regions + 1][max_tracks] int32.
 *
 * One push, n = 1, 2, ...  R = min(d_regions_summary[2], max_regions) (records written, read on the device; a negative
 * word counts as 0).  A label outside 1..R is background: negative labels, labels beyond max_regions, the components
 * beyond the records.  Nothing is indexed with such a label.  Record c is d_regions[c - 1]; its area is >= 1, as in every
 * record rcflow_regions_push_dev writes (a record with area <= 0 gives px = py = 0).
 *  0. Free.  A slot whose record carried RC_TRACK_ENDED after the previous push becomes zero bytes.  The tracks alive "at
 *     the start" are the other used slots.
 *  1. Overlap.  ov[c][t] = number of pixels with label c in 1..R and P = t + 1.
 *  2. Claim.  best(c) = the alive track with the largest ov[c][t] among those with ov[c][t] >= min_overlap, the smaller
 *     id among equals; there may be none.
 *  3. Winner.  For an alive t, among the c with best(c) = t: the one with the largest ov[c][t], the lowest c among equals.
 *  4. Update.  Every alive track: age += 1.  With a winner c: flags = SEEN (| SPLIT when more than one c claimed it),
 *     hits += 1, misses = 0, label = c, overlap = ov[c][t]; area, x0, y0, x1, y1 from record c; px = (2 sx + area) /
 *     (2 area), py likewise (the integers of rcflow_regions_prims_dev); area_sum += area, fx_sum += fx, fy_sum += fy,
 *     m_sum += area - bad.  Without one: flags = COASTING (| MERGED when some c has ov[c][t] >= min_overlap),
 *     misses += 1, label = 0, overlap = 0, the geometry stays as last seen; misses > max_misses adds ENDED.  Then
 *     CONFIRMED is added whenever hits >= min_hits, and mean_fx = m_sum ? (float)((double)fx_sum / 65536 / m_sum) : 0,
 *     each operation rounded on its own; mean_fy likewise.
 *  5. Births.  The regions c in 1..R that won no track, in ascending c, take the free slots in ascending slot (those freed
 *     in step 0 count, those that ended in this push do not): the k-th region the k-th slot, id = next_id + k (k from 0);
 *     next_id grows by the number born.  parent = the id of best(c) when there is one (a split child), else 0; flags =
 *     BORN | SEEN (| CONFIRMED when min_hits <= 1); age = hits = 1, first_push = n, overlap = 0; px0 = px, py0 = py, kept
 *     for life; the sums are those of this region alone.  Regions beyond the free slots stay untracked and are counted.
 *  6. Paint.  P = slot(c) + 1 where the pixel's label c is in 1..R (0 when c is untracked); elsewhere the old P when that
 *     track is alive and not ENDED after step 4, else 0.  So a coasting track keeps what is left of its last footprint,
 *     and a region that comes back there within max_misses pushes gets its id back.
 *  7. Outputs (device memory, each may be NULL; the state is updated whatever is asked for; row padding is never written):
 *     d_tracks          max_tracks records in slot order (8-byte aligned).
 *     d_track_of_label  int32 [max_regions + 1]: slot + 1 of the label's track; entry 0, untracked labels and entries
 *                       above R are 0.
 *     d_mask_out        8UC1: 255 where the pixel's label is in 1..R and its track is CONFIRMED, else 0: what
 *                       rcflow_create_edges_dev / rcflow_create_output_dev take next.
 *     d_summary         8 int64: tracks alive and not ended; confirmed among them; born; ended; seen (births included);
 *                       coasting (those that ended in this push included); regions left untracked; n.
 * rc_track: slot is the record's index; the other fields as the steps name them.
 * Primitives: rcflow_tracks_prims_dev writes 5 * max_tracks primitives, slot after slot: for a track that is CONFIRMED and
 * not ENDED the four box edges in the order of rcflow_regions_prims_dev and a disc at (px, py); all-zero records else. */
#define RC_TRACKS_MAX_REGIONS 1024
#define RC_TRACKS_MAX 1024
#define RC_TRACKS_LAUNCHES 6       /* per push, whatever the labels hold */
enum { RC_TRACK_SEEN = 1, RC_TRACK_BORN = 2, RC_TRACK_COASTING = 4, RC_TRACK_ENDED = 8,
       RC_TRACK_SPLIT = 16, RC_TRACK_MERGED = 32, RC_TRACK_CONFIRMED = 64 };
typedef struct rc_tracks_params {
    int max_regions;   /* 1..RC_TRACKS_MAX_REGIONS: labels above it are background */
    int max_tracks;    /* 1..RC_TRACKS_MAX slots */
    int min_overlap;   /* >= 1 pixels */
    int max_misses;    /* 0..65535 consecutive pushes a track may go unseen */
    int min_hits;      /* >= 1: pushes seen before RC_TRACK_CONFIRMED */
    int flags;         /* 0 */
} rc_tracks_params;
typedef struct rc_track {          /* 128 bytes; a free slot is all zero bytes */
    int64_t id, parent, first_push;
    int64_t area_sum, fx_sum, fy_sum, m_sum;
    int32_t slot, label, flags, age, hits, misses;
    int32_t area, x0, y0, x1, y1, px, py, px0, py0, overlap;
    float mean_fx, mean_fy;
} rc_track;
typedef struct rc_tracks_info {
    int w, h;
    rc_tracks_params prm;
    int launches_per_push;             /* RC_TRACKS_LAUNCHES */
    long long pushes;                  /* calls since open / reset */
    size_t device_bytes;
} rc_tracks_info;
/* Allocates everything the slot will ever need (the footprint: 4 bytes per pixel; the overlap table; RC_ENOMEM with the
 * byte count in rcflow_last_error).  Re-opening replaces the state; a refused open leaves the open state as it was.
 * RC_EINVAL: a parameter out of range, unknown flag bits, a frame of 2^31 pixels or more; RC_ESIZE beyond the context's
 * max_w x max_h. */
int rcflow_tracks_open(rc_ctx* ctx, int stream, int w, int h, const rc_tracks_params* prm);
/* One set of regions.  d_labels: int32 h x w (4-byte aligned, labels_step a multiple of 4, >= 4 w); d_regions: at least
 * max_regions records or as many as d_regions_summary[2] says (8-byte aligned); d_regions_summary: the 8 int64 of
 * rcflow_regions_push_dev.  Every refusal is decided before anything is queued and leaves the state as it was: RC_EINVAL
 * for a NULL input, a bad step, a pointer without the natural alignment of its element, an output whose byte range
 * [first byte, past the last) overlaps an input's or another output's (d_regions counts as max_regions records); RC_ESTATE
 * before open. */
int rcflow_tracks_push_dev(rc_ctx* ctx, int stream, const int32_t* d_labels, size_t labels_step,
                           const rc_region* d_regions, const long long* d_regions_summary,
                           rc_track* d_tracks, int32_t* d_track_of_label, uint8_t* d_mask_out, size_t mask_out_step,
                           long long* d_summary);
/* 5 * max_tracks primitives from the table as the last push left it (before the first push: all kind 0) into d_prims.
 * RC_EINVAL: thickness outside 1..RC_DRAW_MAX_THICKNESS, disc_radius outside 0..RC_DRAW_COORD_MAX. */
int rcflow_tracks_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, rc_draw_prim* d_prims);
/* Blocks until the slot's stream has finished; for hosts and tests.  The first min(cap, max_tracks) records of the table
 * in slot order, the footprint (h * w int32, dense), the summary of the last push; any pointer may be NULL.  Before the
 * first push: zeros. */
int rcflow_tracks_read(rc_ctx* ctx, int stream, rc_track* tracks, int cap, int32_t* footprint /* h*w */, long long summary[8]);
/* never blocks; RC_ESTATE when nothing is open */
int rcflow_tracks_info(rc_ctx* ctx, int stream, rc_tracks_info* info);
/* no track, an empty footprint, next_id 1, n 0; keeps the allocation; asynchronous, on the slot's stream */
int rcflow_tracks_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_tracks_close(rc_ctx* ctx, int stream);

/* ------------------------------------------------------------------ motion templates: history, gradient, wave direction
 * globalOrientation (ripcurrents.hpp, ripcurrents_module.cpp:319-359): where the waves are going, taken from frame
 * differences alone, with no flow field: the second opinion beside the direction rcflow_ripmap_* sums from the flow.  It is
 * the reference's one use of OpenCV's motion templates (motempl::updateMotionHistory, calcMotionGradient,
 * calcGlobalOrientation); the arithmetic below restates optflow/src/motempl.cpp and is not pinned to an OpenCV build
 * (DESIGN 7i lists the constants to re-verify).  The history lives on the device from push to push.  A push is THREE
 * launches ("motion@0" .. "motion@2") with no host synchronisation and no device-to-host copy; rcflow_motion_prims_dev is
 * one more ("motion@3").  All fp32 unless stated, each operation rounded on its own (no fused multiply-add).
 *
 *  1. Update ("motion@0").  ts = (float)timestamp, delbound = (float)(timestamp - duration) (the difference in double).
 *       s   = |cur - prev| > diff_threshold, in integers: the absdiff + threshold(THRESH_BINARY) of :321-323;
 *       mhi = s ? ts : (mhi < delbound ? 0 : mhi);      prev = cur, kept by the library.
 *     The first push after open / reset has no previous frame: its silhouette is empty and the outputs are those of the
 *     history as it stands (zeros).
 *  2. Gradient ("motion@1"), aperture 3, replicate border, p = mhi, indices [row][col]:
 *       dx = (p[-1][+1] - p[-1][-1]) + 2 * (p[0][+1] - p[0][-1]) + (p[+1][+1] - p[+1][-1])   in this order of operations,
 *       dy likewise with rows and columns exchanged;
 *       orient = fastAtan2(dy, dx) in degrees (OpenCV's polynomial; 360.0f occurs);
 *       mask = !(|dx| < eps && |dy| < eps), eps = 1e-4f * 9;
 *       mn, mx = minimum and maximum of the 3 x 3 neighbourhood (erode / dilate, one iteration), d0 = mx - mn:
 *       mask = 0 where d0 < (float)delta1 or (float)delta2 < d0;  orient = 0 wherever mask == 0.
 *  3. Orientation of a set of pixels: every grid cell, and the whole frame.  Cell of pixel (x, y) as rcflow_ripmap_*:
 *     (min(x / (w / grid_x), grid_x - 1), likewise y).
 *       histogram  12 bins over the set's masked pixels, idx = floor((double)orient * (12.0 / 360.0)); a pixel whose idx is
 *                  outside 0..11 (orient == 360.0f) is masked but not counted.  peak_bin = the fullest bin, the lowest on a
 *                  tie; base = (float)(peak_bin * 30);
 *       tsmax      the maximum mhi over the set's masked pixels, 0 for none;
 *       a = (float)(254. / 255. / duration);  b = (float)(1. - (double)tsmax * (double)a);
 *       del = (float)((double)tsmax - duration);
 *       per pixel with mask && mhi > del:  wgt = mhi * a + b;  rel = orient - base;  rel += rel < -180 ? 360 : 0;  then
 *                  rel += rel > 180 ? -360 : 0;  if |rel| < 45:  t = wgt * rel,
 *                  S += (int64)rint((double)t * 2^32),  W += (int64)rint((double)wgt * 2^32),  n_used += 1;
 *       angle = (double)base + (W ? (double)S / (double)W : 0), - 360 when >= 360, + 360 when < 0.
 *     S and W are integer sums and do not depend on the order of addition (upstream adds floats in raster order, which no
 *     parallel sum reproduces); |t| < 46 and at most 2^24 pixels keep |S| < 2^62.  The quantisation moves the angle by at
 *     most 46 * 2^-33 * 255 = 1.4e-6 degrees, every weight being above 1 / 255.
 *  4. Picture (d_vis, 8UC3): v = mhi > delbound ? (mhi - delbound) / (float)duration : 0; byte = rint(v * 255) (half to
 *     even) saturated to 0..255, in all three channels.
 *  5. Primitives.  rcflow_motion_prims_dev turns the records of the last push into 2 * (cells + 1) primitives for
 *     rcflow_draw_dev: per cell, in row order, a disc at the cell's centre (px, py) = ((first column + last column) / 2,
 *     likewise rows) and a line of `thickness` from there to (px + (int32)rint(length * cos(angle)), py + (int32)rint(length
 *     * sin(angle))), the angle in radians as angle * (pi / 180) in double, y DOWN; the frame's pair comes last, at
 *     ((w - 1) / 2, (h - 1) / 2).  cos and sin are the device's, in double: a line's far end is good to one pixel.  A set
 *     with W == 0 gives two all-zero records (kind 0), which rcflow_draw_dev skips AND COUNTS in d_skipped.  No arrowheads.
 *
 * RC_MOTION_FRESH: the reference's literal call (:321-333): the history is zeroed before every update, the stamp is 1 and
 * the duration is 1 whatever the parameters and the timestamp say (the timestamp is still checked).  The history is then
 * the silhouette as 0.0 / 1.0 (the reference's "min-max normalised" image) and the picture 0 / 255 (its hist_gray).
 * Deviations from the reference: an empty silhouette gives an all-zero history, an empty mask and angle 0 (it divides 0 by
 * 0 there); its read of the float orientation image as double (:352) is not reproduced. */
#define RC_MOTION_FRESH 1          /* flags bit 0 */
#define RC_MOTION_AUTO_TIME (-1.0) /* timestamp: pushes since open / reset + 1 */
#define RC_MOTION_LAUNCHES 3       /* per push, whatever is asked for */
#define RC_MOTION_MAX_PIXELS (1 << 24)
typedef struct rc_motion_params {
    int diff_threshold;     /* 0..255; the reference: 30 */
    double duration;        /* finite, > 0; the reference: 1 */
    double delta1, delta2;  /* finite, > 0; swapped when delta1 > delta2; the reference: 0.25, 1 */
    int grid_x, grid_y;     /* >= 1, <= w, h, at most RC_RIPMAP_MAX_CELLS cells; the reference's arrows: (w / 30, h / 30) */
    int flags;              /* RC_MOTION_FRESH */
} rc_motion_params;
typedef struct rc_motion_cell {    /* 40 bytes */
    double angle;                  /* degrees in [0, 360), x to the right, y DOWN; base when W == 0 */
    long long S, W;
    float tsmax;
    int n_masked, n_used, peak_bin;
} rc_motion_cell;
typedef struct rc_motion_info {
    int w, h;
    rc_motion_params prm;              /* deltas in order */
    int launches_per_push;             /* RC_MOTION_LAUNCHES */
    long long pushes;                  /* since open / reset */
    double last_timestamp;             /* of the last push; 0 before the first */
    size_t device_bytes;
} rc_motion_info;
/* Allocates everything the slot will ever need: history 4 B/px, previous gray frame 1 B/px, orientation 4 B/px, mask
 * 1 B/px (rows of w rounded up to 4 pixels), the cell tables.  Re-opening replaces the state; a refused open leaves the
 * open state as it was.  RC_EINVAL: no parameters, diff_threshold outside 0..255, duration or a delta not finite or <= 0,
 * a grid below 1 x 1, wider or higher than the frame or beyond RC_RIPMAP_MAX_CELLS cells, unknown flag bits; RC_ESIZE
 * beyond the context's max_w x max_h or more than RC_MOTION_MAX_PIXELS pixels (the bound the integer sums are sized for). */
int rcflow_motion_open(rc_ctx* ctx, int stream, int w, int h, const rc_motion_params* prm);
/* One gray frame (8UC1, w x h, step >= w).  timestamp: RC_MOTION_AUTO_TIME, or finite, >= 0 and <= 2^24; either way the
 * stamp must be greater than the last push's (RC_EINVAL).  Outputs (device memory, each may be NULL; the state is updated
 * whatever is asked for): d_mhi, d_orient 32FC1 (4-byte aligned, a step that is a multiple of 4 and >= 4 w), d_mask 8UC1
 * (255 / 0, step >= w), d_vis 8UC3 (step >= 3 w), d_cells grid_y x grid_x records and d_frame one record (8-byte aligned).
 * An output whose byte range [first byte, past the last) overlaps the frame's or another output's is RC_EINVAL.  Row padding
 * is never written.  Every refusal is decided before anything is queued and leaves the state as it was; RC_ESTATE before
 * rcflow_motion_open. */
int rcflow_motion_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, double timestamp,
                           float* d_mhi, size_t mhi_step, float* d_orient, size_t orient_step, uint8_t* d_mask, size_t mask_step,
                           uint8_t* d_vis, size_t vis_step, rc_motion_cell* d_cells, rc_motion_cell* d_frame);
/* 2 * (grid_x * grid_y + 1) primitives from the records of the last push (before the first push: all kind 0) into d_prims.
 * RC_EINVAL: d_prims NULL or not 4-byte aligned, thickness outside 1..RC_DRAW_MAX_THICKNESS, disc_radius outside
 * 0..RC_DRAW_COORD_MAX, length not finite or beyond RC_DRAW_COORD_MAX in magnitude. */
int rcflow_motion_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, double length,
                            rc_draw_prim* d_prims);
/* Blocks until the slot's stream has finished; for hosts and tests.  The records of the last push: the first min(cap,
 * cells) cells in row order, the frame's record, the pixels of the last silhouette; any pointer may be NULL.  Before the
 * first push: zeros. */
int rcflow_motion_read(rc_ctx* ctx, int stream, rc_motion_cell* cells, int cap, rc_motion_cell* frame, long long* silhouette);
/* zeroes the history, forgets the previous frame, the last stamp and the push count; asynchronous, on the slot's stream */
int rcflow_motion_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_motion_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open */
int rcflow_motion_info(rc_ctx* ctx, int stream, rc_motion_info* info);

/* ------------------------------------------------------------------ flow map and FTLE: Lagrangian ridges from a field ring
 * "Where did the water that is here come from, over the last T frames", as a per-pixel number a detector can threshold: the
 * finite-time Lyapunov exponent of the flow map over a sliding window of fields.  In backward time its ridges are the
 * attracting lines along which foam and sediment collect, the feeder and the neck of a rip.  The reference has no such
 * product (its streamline_field, ripcurrents_module.cpp:608-648, integrates forward from the first frame for ever); the
 * sampler and the Euler step are its own, and RC_FTLE_FORWARD over fields that all fit the window is bit for bit what
 * rcflow_advect_field_dev leaves after the same fields with iterations 1 and UPPER +inf.  tests/_ftle_ref.py states the
 * following in numpy.  All fp32 unless stated, each operation rounded on its own (no fused multiply-add).
 *
 *  State: a ring of the last `window` fields; n = min(pushes, window) of them are held.
 *  1. Flow map ("ftle@1").  A particle starts at every pixel (xo, yo) with displacement D = (0, 0), alive, steps = 0.
 *     RC_FTLE_FORWARD visits the held fields oldest to newest with sdt = dt, RC_FTLE_BACKWARD newest to oldest with
 *     sdt = -dt.  At each field, while the particle is alive: x = D.x + xo, y = D.y + yo; the bilinear sample (dx, dy) of
 *     the field at (x, y) exactly as the streamline sampler takes it (ripcurrents_module.cpp:494-508): indices (int)floorf(.)
 *     as x86 converts (NaN and out of range: INT_MIN), rejected when xind < 1 || yind < 1 || xind + 2 > w || yind + 2 > h,
 *     the weights, the four products and the three additions in its order.  The particle stops for good when the sample is
 *     rejected or dx or dy is not finite; else D.x = D.x + dx * sdt, D.y = D.y + dy * sdt (one multiply, one add each) and
 *     steps += 1.  A stopped particle keeps its D.  There is no UPPER cut-off.  D is always finite.
 *  2. Deformation ("ftle@2"), s = spacing.  Pixel (x, y) is VALID when s <= x < w - s, s <= y < h - s and the pixel and its
 *     four neighbours at +-s in x and in y all have steps == n.  inv = 1.0f / (float)(2 s); E, W, S, N the neighbours at
 *     x + s, x - s, y + s, y - s:
 *       a = 1 + (D_E.x - D_W.x) * inv    b = (D_S.x - D_N.x) * inv    c = (D_E.y - D_W.y) * inv    d = 1 + (D_S.y - D_N.y) * inv
 *       c11 = a*a + c*c    c12 = a*b + c*d    c22 = b*b + d*d    m = (c11 + c22) * 0.5f    q = (c11 - c22) * 0.5f
 *       lam = m + sqrtf(q*q + c12*c12)                 the largest eigenvalue of the Cauchy-Green tensor
 *       ftle = (float)(log((double)lam) / (double)(2 n))      per frame: the caller multiplies by frames per second.
 *     The logarithm is the device's, in double: its last-place error moves the float by at most one unit in the last place.
 *     Displacements near the top of the float range (a field value like 1e30 met at the last step) can overflow the
 *     products: lam is then +inf, or NaN, which is stored as the one pattern 0x7fc00000 in lam and in ftle.  Where the
 *     pixel is not valid lam, ftle and mask are 0.
 *  3. Mask (8UC1, 255 / 0): valid && lam >= lam_thr, lam_thr = (float)exp(2.0 * n * threshold), computed on the host in
 *     double for every push: decided on lam, never on the logarithm.  It is what rcflow_regions_push_dev takes.
 *  4. Picture (8UC3): entry i of rcflow_jet_lut, i = rint(ftle / (float)vis_max * 255) saturated to 0..255 (NaN: 0); black
 *     where the pixel is not valid.
 *  5. Summary, 8 int64: n | valid pixels | mask pixels | particles with steps < n | the bits of the largest lam over the
 *     valid pixels as uint32 (NaN excepted; 0 for none) | pushes since open / reset | 0 | 0. */
#define RC_FTLE_FORWARD 0
#define RC_FTLE_BACKWARD 1
#define RC_FTLE_MAX_WINDOW 256
#define RC_FTLE_MAX_SPACING 16
#define RC_FTLE_MAX_RING_BYTES (4ull << 30)
#define RC_FTLE_LAUNCHES 3         /* of a push that computes; a push with no output is one */
typedef struct rc_ftle_params {
    int window;             /* 1..RC_FTLE_MAX_WINDOW fields */
    int direction;          /* RC_FTLE_FORWARD, RC_FTLE_BACKWARD */
    float dt;               /* finite, > 0: frames per field */
    int spacing;            /* 1..RC_FTLE_MAX_SPACING: half-width of the central differences */
    double threshold;       /* finite: the mask's bound on ftle, per frame */
    double vis_max;         /* finite, > 0: the ftle the picture's last colour stands for */
    int flags;              /* 0 */
} rc_ftle_params;
typedef struct rc_ftle_info {
    int w, h;
    rc_ftle_params prm;                /* threshold and vis_max as rcflow_ftle_set left them */
    int launches_per_push;             /* RC_FTLE_LAUNCHES */
    int held;                          /* n: fields in the ring */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_ftle_info;
/* Allocates everything the slot will ever need: the ring (8 B/px per field, rows of w rounded up to 2 pixels: 16.6 MB a
 * field at 1080p), the map 8 B/px, steps 4 B/px, lam 4 B/px, the counters.  Re-opening replaces the state; a refused open
 * leaves the open state as it was.  RC_EINVAL: no parameters, a value outside the ranges above, unknown flag bits; RC_ESIZE
 * beyond the context's max_w x max_h or a ring above RC_FTLE_MAX_RING_BYTES. */
int rcflow_ftle_open(rc_ctx* ctx, int stream, int w, int h, const rc_ftle_params* prm);
/* One flow field (32FC2, w x h, pointer and step multiples of 8, step >= 8 w) into the ring.  Outputs (device memory, each
 * may be NULL): d_map_xy 32FC2 (the displacements D; 8-byte aligned, step a multiple of 8), d_steps 32SC1, d_lam and d_ftle
 * 32FC1 (4-byte aligned, steps multiples of 4), d_mask 8UC1, d_vis 8UC3, d_summary 8 int64 (8-byte aligned).  With every
 * output NULL the push is ONE launch ("ftle@0", the ring slot): push every frame, ask for the map every k-th.  With any
 * output it is RC_FTLE_LAUNCHES ("ftle@0" .. "ftle@2"), and what they give does not depend on which earlier pushes
 * computed.  No host synchronisation, no device-to-host copy.  An output whose byte range [first byte, past the last)
 * overlaps the field's or another output's is RC_EINVAL.  Row padding is never written.  Every refusal is decided before
 * anything is queued and leaves the state as it was; RC_ESTATE before rcflow_ftle_open. */
int rcflow_ftle_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step,
                         float* d_map_xy, size_t map_step, int32_t* d_steps, size_t steps_step,
                         float* d_lam, size_t lam_step, float* d_ftle, size_t ftle_step,
                         uint8_t* d_mask, size_t mask_step, uint8_t* d_vis, size_t vis_step, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  The summary of the last push that computed one; zeros
 * before that. */
int rcflow_ftle_read(rc_ctx* ctx, int stream, long long summary[8]);
/* threshold and vis_max from the next push on; RC_EINVAL as rcflow_ftle_open */
int rcflow_ftle_set(rc_ctx* ctx, int stream, double threshold, double vis_max);
/* empties the ring and zeroes the summary and the push count; keeps the allocation; asynchronous, on the slot's stream */
int rcflow_ftle_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_ftle_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open */
int rcflow_ftle_info(rc_ctx* ctx, int stream, rc_ftle_info* info);

/* ------------------------------------------------------------------ plan view: the flow in metres per second on a ground grid
 * A shore camera looks along the water at a shallow angle, so every product above mixes near and far water: equal pixels are
 * wildly unequal areas, and a current far out moves a fraction of the pixels the same current moves close by.  The plan view
 * resamples the flow field and the frame onto a regular grid on the water surface, through the camera's ground-to-image map
 * and its radial distortion, and pushes the sampled vector through the inverse of the map's Jacobian: velocities come out in
 * metres per second, and rcflow_ripmap_*, rcflow_regions_*, rcflow_tracks_* and rcflow_ftle_*, which take any 32FC2 field,
 * are metric when they are given the plan field.  The reference has no such product.  tests/_planview_ref.py states the
 * following in numpy and the kernels equal it bit for bit.
 *
 *  1. Table ("planview@0"), built once by open on the device.  All DOUBLE, every operation rounded on its own (no fused
 *     multiply-add), sums left to right; only + - * /, fabs and sqrt:
 *       project(X, Y):  px = H0*X + H1*Y + H2    py = H3*X + H4*Y + H5    pz = H6*X + H7*Y + H8
 *                       u = px / pz    v = py / pz    xn = (u - cx) / fx    yn = (v - cy) / fy    r2 = xn*xn + yn*yn    r4 = r2*r2
 *                       s = 1 + k1*r2 + k2*r4        g = 1 + 3*k1*r2 + 5*k2*r4      (g <= 0: past the fold of the distortion)
 *                       U = cx + fx*(xn*s)           V = cy + fy*(yn*s)
 *       cell (i, j):    X = x0 + i*dx, Y = y0 + j*dy; the centre and E/W = (X +- 0.5*dx, Y), S/N = (X, Y +- 0.5*dy) are projected
 *                       a = (U_E - U_W)/dx   b = (U_S - U_N)/dy   c = (V_E - V_W)/dx   d = (V_S - V_N)/dy   det = a*d - b*c
 *                       m00 = d/det*fps   m01 = -b/det*fps   m10 = -c/det*fps   m11 = a/det*fps   gsd = sqrt(fabs(1/det))
 *     The cell is USABLE when pz > 0 and g > 0 at all five points, the centre's U and V, det, the four m and gsd are finite
 *     (as doubles), det != 0 and gsd <= max_gsd.  gsd is the ground footprint of an image pixel in metres per pixel.  The
 *     central difference over one cell works for any camera model, needs no inverse of the distortion and is exact for the
 *     affine part of the map.  A record is eight floats, 32 bytes, each the double rounded once: U, V, m00, m01, m10, m11,
 *     gsd, 1.0f; eight zeros where the cell is not usable (U = 0 is then rejected by the sampler: the push has one test).
 *  2. Push ("planview@1"), per cell, fp32, each operation rounded on its own:
 *     SEEN: the record's (U, V) passes the streamline sampler's test (ripcurrents_module.cpp:494-508) for the w x h image:
 *     xind = (int)floorf(U), yind likewise, as x86 converts; xind < 1 || yind < 1 || xind + 2 > w || yind + 2 > h rejects.
 *     VALID: seen, the field is given, and its bilinear sample (sx, sy) at (U, V), with that sampler's weights, products and
 *     additions in its order, is finite in both components.
 *     Plan field: Vx = m00*sx + m01*sy, Vy = m10*sx + m11*sy (two multiplies, one add) where valid, else (0, 0).  A large
 *     sample may overflow them to +-inf, or to NaN: they are stored as they come.
 *     Mask (8UC1): 255 where valid, else 0: the form rcflow_regions_push_dev takes.
 *     Picture (8UC3), where seen: ix = (int)rintf(U * 32.f), iy likewise; source pixel (ix >> 5, iy >> 5), fractions ix & 31,
 *     iy & 31, the 8-bit sample of the warps (weights of 2^15, rounded per channel, a tap outside the frame counts 0); black
 *     elsewhere.  It does not depend on the field.
 *     Summary, 8 int64: usable cells | seen cells | valid cells | the bits, as uint32, of the largest Vx*Vx + Vy*Vy over the
 *     valid cells (NaN excepted; 0 for none) | pushes since open / reset | 0 | 0 | 0.  A push without the field has no valid
 *     cell. */
#define RC_PLANVIEW_LAUNCHES 1     /* of a push */
#define RC_PLANVIEW_MAX_CELLS (1ll << 30)   /* a table of 32 GiB */
typedef struct rc_planview_params {
    double H[9];            /* row-major: ground (X, Y, 1) in metres -> homogeneous IDEAL (undistorted) pixel; all finite */
    double fx, fy, cx, cy;  /* focal lengths and principal point of the distortion model, pixels; finite, fx, fy > 0 */
    double k1, k2;          /* radial distortion (OpenCV's model without the tangential terms); finite; both 0: none */
    double x0, y0, dx, dy;  /* ground position of plan cell (0, 0) and the cell pitch, metres; finite; dx, dy not 0, may be negative */
    int nx, ny;             /* plan size in cells; >= 1, within the context's max_w x max_h */
    double fps;             /* fields per second (1: metres per field); finite, > 0 */
    double max_gsd;         /* largest ground footprint of an image pixel a cell may have, metres per pixel; > 0; +inf: no cut */
    int flags;              /* 0 */
} rc_planview_params;
typedef struct rc_planview_info {
    int w, h;                          /* the image: the field's and the frame's size */
    rc_planview_params prm;
    int launches_per_push;             /* RC_PLANVIEW_LAUNCHES */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_planview_info;
/* Allocates the table (32 B per plan cell) and the counters and builds the table on the slot's stream ("planview@0").
 * Re-opening replaces the state, and is how parameters change (another tide level: another H); a refused open leaves the open
 * state as it was.  RC_EINVAL: no parameters, w or h < 1, a value outside the ranges above, unknown flag bits; RC_ESIZE: w x h
 * or nx x ny beyond the context's max_w x max_h, or more than RC_PLANVIEW_MAX_CELLS cells. */
int rcflow_planview_open(rc_ctx* ctx, int stream, int w, int h, const rc_planview_params* prm);
/* One launch ("planview@1"); no host synchronisation, no device-to-host copy.  Inputs (device memory, either may be NULL,
 * not both): d_flow_xy 32FC2 w x h (pointer and step multiples of 8, step >= 8 w), d_bgr 8UC3 w x h.  Outputs, each may be
 * NULL: d_plan_xy 32FC2 nx x ny (pointer and step multiples of 8), d_mask 8UC1 nx x ny and d_summary 8 int64 (8-byte
 * aligned) need the field, d_plan_bgr 8UC3 nx x ny needs the frame.  RC_EINVAL: both inputs NULL, an output whose input is
 * NULL, a bad pointer or step, an output whose byte range [first byte, past the last) overlaps an input's or another
 * output's.  Row padding is never written.  Every refusal is decided before anything is queued and leaves the state as it
 * was; RC_ESTATE before rcflow_planview_open. */
int rcflow_planview_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step,
                             const uint8_t* d_bgr, size_t bgr_step, float* d_plan_xy, size_t plan_step,
                             uint8_t* d_mask, size_t mask_step, uint8_t* d_plan_bgr, size_t plan_bgr_step,
                             long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  The summary of the last push; zeros before the first. */
int rcflow_planview_read(rc_ctx* ctx, int stream, long long summary[8]);
/* Blocks; copies the table out (host memory, ny * nx * 8 floats): for tests, and for drawing what was detected on the plan
 * grid back into the image (a usable cell's U, V is its centre's pixel). */
int rcflow_planview_table_read(rc_ctx* ctx, int stream, float* table);
/* zeroes the summary and the push count; keeps the table; asynchronous, on the slot's stream */
int rcflow_planview_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_planview_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open */
int rcflow_planview_info(rc_ctx* ctx, int stream, rc_planview_info* info);

/* ------------------------------------------------------------------ wave spectra: period, wavenumber, celerity and depth
 * What are the waves doing, and how deep is the water under them?  Every product above looks at the flow; this one looks at
 * the grey value of every pixel over time.  It keeps a sliding discrete Fourier transform of the last `window` frames at a
 * few frequency bins per pixel, and per grid cell picks the bin that carries the most power, takes the wavenumber from the
 * phase gradient of that bin across the cell, and from frequency and wavenumber the celerity and, through the linear
 * dispersion relation omega^2 = g k tanh(k h), the depth: the first stage of what the coastal-imaging literature calls
 * cBathy.  A rip channel is the deep gap in the bar; the windows of ripmap and ftle are best chosen from the wave period.
 * The input is a grey frame, normally the plan picture greyed with rcflow_resize_bgr_to_gray_dev, so that a pixel is
 * metres_per_pixel_x by metres_per_pixel_y metres.  The reference has no such product.  tests/_waves_ref.py states the
 * following in numpy.  Everything up to the cell sums is integer and exact, whatever the tiling.
 *
 *  State: a ring of `window` (W) grey frames, zero at open and reset; per pixel and bin b in bin_lo..bin_hi (K of them; bin b
 *  is b * fps / W Hz) one complex accumulator A_b of two int32; the host's table Tc[j] = lrint(2048 cos((2 pi j) / W)),
 *  Ts[j] = lrint(2048 sin((2 pi j) / W)), j in 0..W-1, in double.
 *  1. Spectrum ("waves@0"), every push.  c = pushes mod W; d = new - ring[c] as int; ring[c] = new; for every bin, with
 *     j = (b c) mod W: A_b.re += d Tc[j], A_b.im -= d Ts[j].  A_b is therefore always the table's DFT of the ring as it stands,
 *     frames not yet pushed counting as zero.  |component| <= 255 * 2048 * W < 2^31 for W <= 4096: int32 never wraps.
 *  2. Cell sums ("waves@1"), when any output is asked for.  sh = max(0, bit_length(255 * 2048 * W) - 15); Xs = A >> sh, an
 *     arithmetic shift of each component, so |Xs| < 2^15.  s = spacing.  Pixel (x, y) TAKES PART when s <= x < w - s and
 *     s <= y < h - s and, where d_mask is given, the mask is non-zero at the pixel and at its four neighbours at +-s in x and
 *     in y.  Its cell is (min(x / (w / grid_x), grid_x - 1), min(y / (h / grid_y), grid_y - 1)), as the opposing-flow map's.
 *     Per cell and bin six int64, in this order, over the pixels that take part (C the pixel, E, W, S, N at x+s, x-s, y+s, y-s):
 *       n += 1    P += |Xs_C|^2    Re Cx, Im Cx += Xs_E conj(Xs_W)    Re Cy, Im Cy += Xs_S conj(Xs_N)
 *  3. Closing per cell, in DOUBLE, every operation rounded on its own, left to right; a record is 32 bytes (rc_wave_cell).
 *     RC_WAVES_EMPTY when n < min_pixels or every P is 0: the record is otherwise zero.  Else b* is the bin of the largest P,
 *     the lowest bin winning ties, and with that bin's sums, every int64 converted to double once (Im negated as an integer):
 *       kx = atan2(-Im Cx, Re Cx) / (2 s) / metres_per_pixel_x      ky likewise from Cy and metres_per_pixel_y      rad/m
 *       kmag = sqrt(kx*kx + ky*ky)    freq_hz = b* * fps / W    omega = 6.283185307179586 * b* * fps / W
 *       quality = (sqrt(ReCx^2 + ImCx^2) + sqrt(ReCy^2 + ImCy^2)) / (2 * P)
 *     The sign: a wave I = cos(k.x - omega t) gives A proportional to e^{-i k.x}, so (kx, ky) points where the wave travels.
 *     quality is near 1 for one plane wave and near 0 for noise; it is NOT bounded by 1 (Cauchy-Schwarz bounds |Cx| by the
 *     geometric mean of the power at E and at W, not by the power at C).  RC_WAVES_NOWAVE when kmag is 0: celerity and depth
 *     are 0.  Else celerity = omega / kmag (m/s) and t = omega*omega / (gravity * kmag): depth = atanh(t) / kmag (m) when
 *     t < tanh_max, otherwise RC_WAVES_DEEP and depth 0 (the water is too deep for the wave to feel the bed, or k was
 *     underestimated).  atan2 and atanh are the device's, in double: their last-place error may move a stored float by one unit
 *     in the last place, and a t within that error of tanh_max may fall on either side.  Every integer is exact.
 *  4. Bin map (8UC1): b* of the pixel's cell, 0 where the cell is EMPTY; a byte holds it, so a session opened with bin_hi above
 *     255 has no bin map (RC_EINVAL when one is asked for; the records carry b* as an int).  Picture (8UC3): entry i of rcflow_jet_lut,
 *     i = rint(depth / (float)vis_max_depth * 255) saturated to 0..255, from the record's float, as the FTLE picture; black where
 *     the cell is EMPTY, NOWAVE or DEEP ("waves@2", when either is asked for).
 *  5. Summary, 8 int64: held frames min(pushes, W) | pixels that take part | cells not EMPTY | cells with a depth (flags 0) |
 *     pushes since open / reset | 0 | 0 | 0. */
#define RC_WAVES_EMPTY 1
#define RC_WAVES_NOWAVE 2
#define RC_WAVES_DEEP 4
#define RC_WAVES_MAX_WINDOW 4096
#define RC_WAVES_MAX_BINS 16
#define RC_WAVES_MAX_SPACING 16
#define RC_WAVES_MAX_STATE_BYTES (4ull << 30)   /* ring plus accumulators */
#define RC_WAVES_LAUNCHES 3        /* of a push that computes everything; a push with no output is one */
typedef struct rc_waves_params {
    int window;             /* W: 2..RC_WAVES_MAX_WINDOW frames */
    int bin_lo, bin_hi;     /* 1 <= bin_lo <= bin_hi < W / 2 (2 bin_hi < W), at most RC_WAVES_MAX_BINS bins */
    int spacing;            /* s: 1..RC_WAVES_MAX_SPACING pixels, half the baseline of the phase differences */
    int grid_x, grid_y;     /* >= 1, <= w, h, at most RC_RIPMAP_MAX_CELLS cells */
    int min_pixels;         /* >= 1: a cell with fewer pixels taking part is EMPTY */
    int flags;              /* 0 */
    double fps;             /* frames per second; finite, > 0 */
    double metres_per_pixel_x, metres_per_pixel_y;   /* finite, > 0 */
    double gravity;         /* m/s^2; finite, > 0 */
    double tanh_max;        /* in (0, 1): the largest tanh(k h) a depth is given for */
    double vis_max_depth;   /* finite, > 0: the depth the picture's last colour stands for */
} rc_waves_params;
typedef struct rc_wave_cell {
    int bin;                /* b*, 0 for an EMPTY cell */
    int flags;              /* RC_WAVES_EMPTY, RC_WAVES_NOWAVE, RC_WAVES_DEEP, or 0: every field holds */
    float freq_hz, kx, ky, celerity, depth, quality;
} rc_wave_cell;
typedef struct rc_waves_info {
    int w, h;
    rc_waves_params prm;               /* tanh_max, min_pixels and vis_max_depth as rcflow_waves_set left them */
    int launches_per_push;             /* RC_WAVES_LAUNCHES */
    int bins;                          /* K */
    int shift;                         /* sh */
    int held;                          /* min(pushes, W) */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_waves_info;
/* Allocates everything the slot will ever need: the ring (1 B/px per frame, rows of w rounded up to 4 pixels), the
 * accumulators (8 B/px per bin), the cell sums and records.  Re-opening replaces the state; a refused open leaves the open
 * state as it was.  RC_EINVAL: no parameters, w or h < 1, a value outside the ranges above, unknown flag bits; RC_ESIZE beyond
 * the context's max_w x max_h, or ring plus accumulators above RC_WAVES_MAX_STATE_BYTES. */
int rcflow_waves_open(rc_ctx* ctx, int stream, int w, int h, const rc_waves_params* prm);
/* One grey frame (8UC1, w x h, step >= w) into the ring and the accumulators ("waves@0").  d_mask (8UC1, may be NULL) limits
 * the pixels that take part.  Outputs (device memory, each may be NULL): d_cells grid_y x grid_x rc_wave_cell (4-byte aligned),
 * d_sums grid_y x grid_x x K x 6 int64 (8-byte aligned), d_bin_map 8UC1 and d_vis 8UC3 (w x h), d_summary 8 int64 (8-byte
 * aligned).  With every output NULL the push is ONE launch: push every frame, ask for the cells every k-th.  With any output
 * "waves@1" follows, and "waves@2" when d_bin_map or d_vis is asked for: RC_WAVES_LAUNCHES at most, and what they give does
 * not depend on which earlier pushes computed.  No host synchronisation, no device-to-host copy.  An output whose byte range
 * [first byte, past the last) overlaps an input's or another output's is RC_EINVAL, as is d_bin_map when bin_hi > 255; a mask
 * given with every output NULL is checked and not read.  Row padding is never written.  Every refusal is decided before
 * anything is queued and leaves the state as it was; RC_ESTATE before rcflow_waves_open. */
int rcflow_waves_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, const uint8_t* d_mask, size_t mask_step,
                          rc_wave_cell* d_cells, long long* d_sums, uint8_t* d_bin_map, size_t bin_map_step,
                          uint8_t* d_vis, size_t vis_step, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records, the sums and the summary
 * of the last push that computed them (host memory, the sizes of rcflow_waves_push_dev's outputs); zeros before that. */
int rcflow_waves_read(rc_ctx* ctx, int stream, rc_wave_cell* cells, long long* sums, long long summary[8]);
/* Blocks; the accumulators as K x h x w x 2 int32 (re, im), whatever the layout on the device; for tests */
int rcflow_waves_spectrum_read(rc_ctx* ctx, int stream, int32_t* spectrum);
/* never blocks; the host's table, W ints each (either may be NULL) */
int rcflow_waves_table_read(rc_ctx* ctx, int stream, int32_t* tc, int32_t* ts);
/* tanh_max, min_pixels and vis_max_depth from the next push on; RC_EINVAL as rcflow_waves_open */
int rcflow_waves_set(rc_ctx* ctx, int stream, double tanh_max, int min_pixels, double vis_max_depth);
/* zeroes the ring, the accumulators, the records, the summary and the push count; keeps the allocation; asynchronous, on
 * the slot's stream */
int rcflow_waves_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_waves_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_waves_info(rc_ctx* ctx, int stream, rc_waves_info* info);

/* ------------------------------------------------------------------ ensemble PIV: cross-correlation flow on a cell grid
 * Every velocity above comes from a differential estimator (Farneback, PyrLK): it follows the wave orbital motion frame by
 * frame and has no answer where foam moves several pixels between frames.  This one is particle image velocimetry as the
 * coastal-imaging literature uses it for surf-zone currents: block cross-correlation of interrogation windows between
 * consecutive grey frames, the correlation sums added over the last `ensemble` frame pairs BEFORE the peak is taken
 * (ensemble correlation), so that the wave-by-wave motion averages out of the summed surface and the mean current is left.
 * It shares nothing with the polynomial expansion and serves as its cross-check.  The reference has no such product.
 * tests/_piv_ref.py states the following in numpy.  Every sum is an integer and exact, whatever the tiling.
 *
 *  Grid.  M = window, R = range, D = 2 R + 1.  grid_x = (w - M - 2 R) / step + 1, grid_y likewise from h.  Cell (cx, cy) has
 *  its template's top-left corner at (x0, y0) = (R + cx step, R + cy step).
 *  1. Per pair and cell ("piv@0"), every push but the first after open / reset.  A is the slot's previous frame, B the pushed
 *     one.  Sa = sum A, Saa = sum A^2 over the M x M template at (x0, y0); for every displacement (j, i) in [-R, R]^2, with B
 *     taken at (x0 + i, y0 + j): Sab = sum A B, Sb = sum B, Sbb = sum B^2.  Every one is at most 255^2 * 64^2 < 2^31.
 *     The ensemble: T* are the same sums over the last n = min(pairs, ensemble) pairs, as int64.  For ensemble > 1 the per-pair
 *     int32 planes are kept in a ring, zero at open and reset: T += new - ring[slot], ring[slot] = new, slot = pair number mod
 *     ensemble, so T always equals a rescan of the last n pairs; for ensemble = 1 T = new and there is no ring.  The pushed
 *     frame then becomes A (a device-to-device copy on the slot's stream).  The first push after open / reset only stores its
 *     frame: n = 0 and every record is RC_PIV_EMPTY.
 *  2. Score, peak and record ("piv@1"), when any output is asked for.  N = n M^2.  In int64, exact, every magnitude below 2^53:
 *       num = N Tab - Ta Tb      va = N Taa - Ta^2      vb = N Tbb - Tb^2
 *       s = (va > 0 && vb > 0) ? ((double)num * fabs((double)num)) / ((double)va * (double)vb) : 0
 *     each operation rounded on its own: the signed square of the zero-normalised cross-correlation.  The peak is the largest
 *     s, scanning j outer and i inner, the first occurrence winning.  peak = (float)s.  RC_PIV_FLAT when va == 0 or the peak
 *     s <= 0: ix, iy, dx, dy are 0.  Else ix = i, iy = j; RC_PIV_EDGE when |i| = R or |j| = R: dx = i, dy = j, no sub-pixel
 *     step.  Otherwise per axis, in double, with r = copysign(sqrt(|s|), s) of the peak (c) and its two neighbours on the axis
 *     (l at -1, rr at +1): e = (l - c) + (rr - c), off = e < 0 ? (l - rr) / (2 e) : 0; dx = (float)(i + off_x), dy likewise.
 *     RC_PIV_LOWPEAK (beside EDGE or alone) when the peak s < min_peak.  The sign is Farneback's: content that moved by
 *     (u, v) from A to B gives (u, v), in pixels per frame.
 *  3. Validation ("piv@2"): the normalised median test of Westerweel and Scarano, in float, each operation rounded on its own.
 *     A cell is VALID when it carries none of EMPTY, FLAT, LOWPEAK.  The valid ones among a valid cell's 8 neighbours are its
 *     candidates.  Fewer than 3: resid = 0, not tested.  Else per component: um the median of the candidates' values (an even
 *     count: (a + b) * 0.5f of the two middle ones), rm the median of |v_k - um|, res = |v - um| / (rm + (float)median_eps);
 *     resid = max(res_x, res_y), RC_PIV_OUTLIER when resid > (float)median_thr.  The candidates' values are those of step 2.
 *  4. Field (32FC2, grid_y x grid_x): (dx, dy) of a valid cell, (um_x, um_y) for an OUTLIER under RC_PIV_REPLACE, zero where the
 *     cell is not valid: the small flow field rcflow_ripmap_push_dev, rcflow_ftle_push_dev, rcflow_regions_push_dev and the
 *     colouring entry points take.  Picture (8UC3, w x h): the cell of pixel (x, y) is (min((x - R) / step, grid_x - 1),
 *     min((y - R) / step, grid_y - 1)); entry i of rcflow_jet_lut, i = rint(hypotf(fx, fy) / (float)vis_max * 255) saturated to
 *     0..255, from the cell's field value, as the FTLE picture; black where x < R or y < R and where the cell is not valid.
 *  5. Summary, 8 int64: n | cells | valid | FLAT | LOWPEAK | EDGE | OUTLIER | pushes since open / reset. */
#define RC_PIV_EMPTY 1
#define RC_PIV_FLAT 2
#define RC_PIV_EDGE 4
#define RC_PIV_LOWPEAK 8
#define RC_PIV_OUTLIER 16
#define RC_PIV_REPLACE 1           /* rc_piv_params.flags: outliers hold their neighbours' median in the field */
#define RC_PIV_MAX_WINDOW 64
#define RC_PIV_MAX_RANGE 16
#define RC_PIV_MAX_ENSEMBLE 256
#define RC_PIV_MAX_PIXEL_PAIRS (1 << 18)        /* ensemble * window^2 at most: N Tab stays below 2^53 */
#define RC_PIV_MAX_STATE_BYTES (4ull << 30)     /* ring plus accumulators */
#define RC_PIV_LAUNCHES 3          /* of a push that computes; a push with no output is one */
typedef struct rc_piv_params {
    int window;             /* M: a multiple of 4, 8..RC_PIV_MAX_WINDOW: side of the interrogation window */
    int range;              /* R: 1..RC_PIV_MAX_RANGE: search radius */
    int step;               /* 1..M: cell pitch */
    int ensemble;           /* E: 1..RC_PIV_MAX_ENSEMBLE frame pairs summed, E M^2 <= RC_PIV_MAX_PIXEL_PAIRS */
    int flags;              /* RC_PIV_REPLACE or 0 */
    double min_peak;        /* in [0, 1]: lowest accepted peak score */
    double median_eps;      /* finite, > 0: epsilon of the median test, pixels */
    double median_thr;      /* finite, > 0: bound of the median test */
    double vis_max;         /* finite, > 0: the magnitude (pixels per frame) the picture's last colour stands for */
} rc_piv_params;
typedef struct rc_piv_cell {
    float dx, dy;           /* pixels per frame */
    float peak;             /* the peak's s */
    float resid;            /* of the median test; 0 where not tested */
    int ix, iy;             /* the integer peak */
    int flags;              /* RC_PIV_EMPTY, FLAT, EDGE, LOWPEAK, OUTLIER */
    int pairs;              /* n */
} rc_piv_cell;
typedef struct rc_piv_info {
    int w, h;
    rc_piv_params prm;                 /* min_peak, median_eps, median_thr and vis_max as rcflow_piv_set left them */
    int grid_x, grid_y;
    int launches_per_push;             /* RC_PIV_LAUNCHES */
    int pairs;                         /* n = min(pairs, E) */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_piv_info;
/* Allocates everything the slot will ever need: the previous frame, the accumulators (24 D^2 + 16 bytes per cell), for
 * ensemble > 1 the ring (12 D^2 + 8 bytes per cell and pair), the records.  Re-opening replaces the state; a refused open
 * leaves the open state as it was.  RC_EINVAL: no parameters, a value outside the ranges above, unknown flag bits, w or h below
 * M + 2 R, more than RC_RIPMAP_MAX_CELLS cells; RC_ESIZE beyond the context's max_w x max_h, or ring plus accumulators above
 * RC_PIV_MAX_STATE_BYTES. */
int rcflow_piv_open(rc_ctx* ctx, int stream, int w, int h, const rc_piv_params* prm);
/* One grey frame (8UC1, w x h, step >= w): correlated against the slot's previous frame ("piv@0"), then kept as the next
 * pair's A.  Outputs (device memory, each may be NULL): d_cells grid_y x grid_x rc_piv_cell (4-byte aligned), d_field 32FC2
 * grid_y x grid_x (pointer and step multiples of 8), d_vis 8UC3 w x h, d_summary 8 int64 (8-byte aligned).  With every output
 * NULL the push is "piv@0" alone: push every frame, ask every k-th time.  With any output "piv@1" and "piv@2" follow,
 * RC_PIV_LAUNCHES in all, and what they give does not depend on which earlier pushes computed.  No host synchronisation, no
 * device-to-host copy.  An output whose byte range [first byte, past the last) overlaps the input's or another output's is
 * RC_EINVAL.  Row padding is never written.  Every refusal is decided before anything is queued and leaves the state as it
 * was; RC_ESTATE before rcflow_piv_open. */
int rcflow_piv_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, rc_piv_cell* d_cells, float* d_field,
                        size_t field_step, uint8_t* d_vis, size_t vis_step, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records and the summary of the
 * last push that computed them (host memory); zeros before that. */
int rcflow_piv_read(rc_ctx* ctx, int stream, rc_piv_cell* cells, long long summary[8]);
/* Blocks; for tests.  Each may be NULL: the accumulators as grid_y x grid_x x D x D x 3 int64 (Tab, Tb, Tbb; j outer, i
 * inner) and the cells' own as grid_y x grid_x x 2 int64 (Ta, Taa), whatever the layout on the device */
int rcflow_piv_sums_read(rc_ctx* ctx, int stream, long long* sums, long long* cell_sums);
/* min_peak, median_eps, median_thr and vis_max from the next push on; RC_EINVAL as rcflow_piv_open */
int rcflow_piv_set(rc_ctx* ctx, int stream, double min_peak, double median_eps, double median_thr, double vis_max);
/* forgets the previous frame, zeroes the ring, the accumulators, the records, the summary and the push count; keeps the
 * allocation; asynchronous, on the slot's stream */
int rcflow_piv_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_piv_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_piv_info(rc_ctx* ctx, int stream, rc_piv_info* info);

/* ------------------------------------------------------------------ transects: time stacks, line velocity, flux and jets
 * Every product above answers "what does the field look like?".  This one answers what is asked once a rip has been found:
 * how strong is it, how wide is its neck, how does it pulse?  In shore-camera work those numbers come from lines laid across
 * the picture ("pixel instruments"): the grey values along a line, one row per frame, are a time stack; the cross-line velocity
 * along an alongshore line against time shows the pulsation; its integral along the line is the offshore transport, and the
 * stretches where it exceeds a threshold are the rip necks; the slope of the streaks in a time stack gives the along-line drift
 * of foam.  The reference has no such product.  tests/_transects_ref.py states the following in numpy.  Every integer is exact;
 * every float operation is rounded on its own.
 *
 *  Geometry (host, in double, once; rcflow_transects_plan gives it without a context).  Line i runs from (x0, y0) to (x1, y1) in
 *  pixels and has n samples, 2..RC_TRANSECTS_MAX_SAMPLES; at most RC_TRANSECTS_MAX_LINES lines, S = sum of n at most
 *  RC_TRANSECTS_MAX_TOTAL.  Sample j: t = j / (n - 1), x = x0 + (x1 - x0) t, X = lrint(16 x), Y likewise: positions are
 *  quantised to 1/16 pixel; 0 <= X <= 16 (w - 1) and 0 <= Y <= 16 (h - 1).  The endpoints are the floats' values taken to
 *  double.  dx = x1 - x0, dy = y1 - y0, len = hypot(dx, dy) > 0; tangent e = (dx, dy) / len, normal nrm = (dy, -dx) / len, both
 *  stored as floats: positive cross-line velocity is to the left of the direction of travel as the picture shows it (y down): a
 *  line drawn left to right has its positive side up the picture.  ds = len * metres_per_pixel / (n - 1) (left to right);
 *  scale = (float)(metres_per_pixel * fps).  The table is in line order, `first` of a line being the sum of the n before it.
 *  1. Every push ("transects@0", one launch, a block per line).  c = pushes mod T.  Per sample, ix = X >> 4, fx = X & 15, iy and
 *     fy likewise, ix1 = min(ix + 1, w - 1), iy1 likewise; p00 = (ix, iy), p10 = (ix1, iy), p01 = (ix, iy1), p11 = (ix1, iy1).
 *     GRAY: g = ((16 - fx) (16 - fy) p00 + fx (16 - fy) p10 + (16 - fx) fy p01 + fx fy p11 + 128) >> 8 into ring_g[c][s].
 *     FLOW: a = fx / 16.f, b = fy / 16.f; per component top = p00 + a (p10 - p00), bot = p01 + a (p11 - p01),
 *     val = top + b (bot - top); ut = (u ex + v ey) scale, un = (u nx + v ny) scale into ring_f[c][s].
 *     Correlation (D = range >= 1): the interior of a line is j in [D, n - D).  For a pair of rows (A older, B pushed lag pushes
 *     later), sums over the interior, d in -D..D: Tab[d] = sum A[j] B[j + d], Tb[d] = sum B[j + d], Tbb[d] = sum B[j + d]^2,
 *     Ta = sum A[j], Taa = sum A[j]^2.  The int64 accumulators of a line are at all times these sums over every pair (r, r + lag)
 *     whose two rows the ring holds: pairs = max(0, min(pushes, T) - lag) of them.  The pushed row's pair is added; the pair whose
 *     older row the push overwrites is computed again from the ring rows and taken off, before the slot is written: no per-pair
 *     memory.  With D = 0 nothing is correlated and pairs is 0.
 *  2. Records ("transects@1", a block per line, when d_records, d_sums, d_profile or d_summary is asked for).
 *     Velocity along the line.  N = pairs (n - 2 D); in int64, exact, below 2^61: num = N Tab - Ta Tb, va = N Taa - Ta^2,
 *     vb = N Tbb - Tb^2; s[d] = (va > 0 && vb > 0) ? ((double)num * fabs((double)num)) / ((double)va * (double)vb) : 0.
 *     RC_TRANSECTS_EMPTY when pairs = 0, RC_TRANSECTS_FLAT when every s is 0: peak_shift, v_along, corr_peak are 0.  Else q is
 *     the first largest s (d = q - D), r = copysign(sqrt|s|, s); when 0 < q < 2 D and den = (r[q-1] - 2 r[q]) + r[q+1] < 0,
 *     delta = 0.5 (r[q-1] - r[q+1]) / den, else delta = 0; q at the rim also sets RC_TRANSECTS_EDGE.  peak_shift = q - D,
 *     v_along = (float)((((q - D) + delta) * ds * fps) / lag), corr_peak = (float)r[q].  Foam that moves towards (x1, y1) gives
 *     a positive v_along, in metres per second.
 *     Transport across the line (FLOW).  held = min(pushes, T).  Per sample and component the window mean is the sequential
 *     float sum over the held rows, oldest first, divided by (float)held: d_profile, S x (ut, un).  Q(x) = (int64)rint((double)x
 *     * 65536).  A sample either of whose means is not finite or reaches 2^20 in magnitude is bad: counted, part of nothing.
 *     Per line, exact: Fpos = sum max(Q(un), 0), Fneg = sum min(Q(un), 0), Ft = sum Q(ut), n_valid.  A sample is IN when it
 *     is not bad and Q(un) >= Q(jet_min) (of the double); a jet is a maximal run of consecutive IN samples of one line.  The
 *     record keeps the number of jets and, for the jet of the largest sum of Q(un) (the first winning ties): start, length,
 *     sum, the largest Q(un) in it and the sample that has it (the first).  Without FLOW every one of these is 0.
 *     Record: mean_along = (float)(((double)Ft / 65536) / n_valid), mean_cross likewise from Fpos + Fneg (0 for n_valid = 0);
 *     flux_out = (float)(((double)Fpos / 65536) * ds), flux_in from Fneg, jet_flux from the jet's sum, in m^2/s;
 *     jet_peak = (float)((double)peak / 65536).  d_sums, 16 int64 per line: Fpos, Fneg, Ft, n_valid, bad, jets, jet_start,
 *     jet_len, jet sum, jet peak, jet_peak_at, N, num, va, vb (of q; 0 when EMPTY or FLAT), q.
 *     Summary, 8 int64: held | pairs | lines with a velocity (neither EMPTY nor FLAT) | lines with a jet | jets | bad samples |
 *     pushes since open / reset | 0.
 *  3. Pictures ("transects@2", when d_stack or d_hov is asked for), S wide and T high: row r is the r-th oldest held row, so the
 *     newest is lowest; rows past held are 0.  d_stack (8UC1, needs GRAY): the grey ring.  d_hov (8UC3, needs FLOW): entry i of
 *     rcflow_jet_lut, i = rint(un / (float)vis_max * 127.5f + 127.5f) saturated to 0..255, un from the ring; black where un is
 *     not finite.
 * The rules that are not obvious from the above.  RC_TRANSECTS_MAX_TOTAL is RC_TRANSECTS_MAX_LINES * RC_TRANSECTS_MAX_SAMPLES:
 * every line may be of full length, and it is RC_TRANSECTS_MAX_STATE_BYTES that bounds the rings (4096 rows of 65536 samples
 * would be 2.4 GB: RC_ESIZE).  The square of num is taken in double, as the PIV score is.  FLAT is "every s is 0".  jet_min is
 * below 2^20, the magnitude at which a mean is bad, so Q(jet_min) is below 2^36.  d_stack on a session without GRAY and d_hov on
 * one without FLOW are RC_EINVAL.  With range 0 nothing is correlated: pairs is 0 and every record is EMPTY. */
#define RC_TRANSECTS_GRAY 1
#define RC_TRANSECTS_FLOW 2
#define RC_TRANSECTS_EMPTY 1
#define RC_TRANSECTS_FLAT 2
#define RC_TRANSECTS_EDGE 4
#define RC_TRANSECTS_MAX_LINES 64
#define RC_TRANSECTS_MAX_SAMPLES 1024
#define RC_TRANSECTS_MAX_TOTAL 65536       /* S at most: MAX_LINES * MAX_SAMPLES, so that every line may be of full length */
#define RC_TRANSECTS_MAX_WINDOW 4096
#define RC_TRANSECTS_MAX_LAG 8
#define RC_TRANSECTS_MAX_RANGE 16
#define RC_TRANSECTS_MAX_STATE_BYTES (1ull << 30)     /* the rings */
#define RC_TRANSECTS_SUMS 16             /* int64 per line in d_sums */
#define RC_TRANSECTS_LAUNCHES 3          /* of a push that asks for everything; a push with no output is one */
typedef struct rc_transect_line {
    float x0, y0, x1, y1;   /* pixels */
    int n;                  /* samples, 2..RC_TRANSECTS_MAX_SAMPLES */
} rc_transect_line;
typedef struct rc_transect_sample {
    int X, Y;               /* position in 1/16 pixel */
    int line;               /* the line it belongs to */
    int offset;             /* j: its place on that line */
} rc_transect_sample;
typedef struct rc_transect_geom {
    int first, n;           /* the line's samples are table[first .. first + n) */
    float ex, ey;           /* tangent */
    float nx, ny;           /* normal */
    float scale;            /* (float)(metres_per_pixel * fps) */
    int pad;
    double len;             /* pixels */
    double ds;              /* metres between neighbouring samples */
} rc_transect_geom;
typedef struct rc_transects_params {
    int window;             /* T: 2..RC_TRANSECTS_MAX_WINDOW rows held */
    int sources;            /* RC_TRANSECTS_GRAY, RC_TRANSECTS_FLOW or both */
    int lag;                /* 1..RC_TRANSECTS_MAX_LAG frames between the rows of a pair */
    int range;              /* D: 0..RC_TRANSECTS_MAX_RANGE samples; 0: no correlation.  D >= 1 needs GRAY, T > lag, every n >= 2 D + 8 */
    int flags;              /* 0 */
    int pad;
    double fps;             /* finite, > 0 */
    double metres_per_pixel; /* finite, > 0; for metric numbers push the plan view's picture and field */
    double jet_min;         /* > 0 and below 2^20 (no mean reaches that): m/s; a sample at or above it belongs to a jet */
    double vis_max;         /* finite, > 0: m/s; the speed the Hovmoeller picture's end colours stand for */
} rc_transects_params;
typedef struct rc_transect {
    int flags;              /* RC_TRANSECTS_EMPTY, FLAT, EDGE */
    int pairs;
    int peak_shift;         /* q - D, samples per lag frames */
    float v_along;          /* m/s */
    float corr_peak;        /* r[q] */
    float mean_along, mean_cross;   /* m/s, of the window means over the valid samples */
    float flux_out, flux_in;        /* m^2/s: the positive and the negative part of the cross-line transport */
    int jets;
    int jet_start, jet_len; /* of the strongest jet, in samples of the line */
    float jet_flux;         /* m^2/s */
    float jet_peak;         /* m/s */
    int jet_peak_at;        /* sample */
    int bad;                /* samples */
} rc_transect;
typedef struct rc_transects_info {
    int w, h;
    rc_transects_params prm;           /* jet_min and vis_max as rcflow_transects_set left them */
    int lines, samples;                /* S */
    int launches_per_push;             /* RC_TRANSECTS_LAUNCHES */
    int held;                          /* min(pushes, T) */
    int pairs;
    int pad;
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_transects_info;
/* The geometry alone: no context, no GPU.  table: S records in line order, geom: n_lines records, total: S; each may be NULL.
 * RC_EINVAL: no lines, more than RC_TRANSECTS_MAX_LINES, an n outside 2..RC_TRANSECTS_MAX_SAMPLES, S above RC_TRANSECTS_MAX_TOTAL, an
 * endpoint that is not finite, a line of no length, a sample outside the picture, fps or metres_per_pixel not finite and > 0. */
int rcflow_transects_plan(int w, int h, const rc_transect_line* lines, int n_lines, double metres_per_pixel, double fps,
                          rc_transect_sample* table, rc_transect_geom* geom, int* total);
/* Allocates everything the slot will ever need: the table, the rings (T S bytes of grey, 8 T S bytes of flow), the accumulators,
 * the records.  Re-opening replaces the state; a refused open leaves the open state as it was.  RC_EINVAL as
 * rcflow_transects_plan, no parameters, a value outside the ranges above, unknown source or flag bits; RC_ESIZE beyond the
 * context's max_w x max_h, or rings above RC_TRANSECTS_MAX_STATE_BYTES. */
int rcflow_transects_open(rc_ctx* ctx, int stream, int w, int h, const rc_transect_line* lines, int n_lines, const rc_transects_params* prm);
/* One frame: d_gray (8UC1, w x h, step >= w) when GRAY was opened and NULL otherwise, d_flow_xy (32FC2, w x h, pointer and step
 * multiples of 8) when FLOW was opened and NULL otherwise; anything else is RC_EINVAL.  Outputs (device memory, each may be
 * NULL): d_records lines x rc_transect (4-byte aligned), d_sums lines x RC_TRANSECTS_SUMS int64 (8-byte aligned), d_profile S x 2
 * float (8-byte aligned), d_stack 8UC1 and d_hov 8UC3, S wide and T high, d_summary 8 int64 (8-byte aligned).  With every
 * output NULL the push is "transects@0" alone; "transects@1" follows for records, sums, profile or summary and "transects@2"
 * for a picture, and what they give does not depend on which earlier pushes computed.  No host synchronisation, no
 * device-to-host copy.  An output whose byte range overlaps an input's or another output's is RC_EINVAL.  Row padding is never
 * written.  Every refusal is decided before anything is queued and leaves the state as it was; RC_ESTATE before
 * rcflow_transects_open.  RC_EHIP (the runtime refused a launch) is no refusal: launches before it may have written the rings and
 * the accumulators while the push count stays, so the state is undefined until rcflow_transects_reset. */
int rcflow_transects_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, const float* d_flow_xy, size_t flow_step,
                              rc_transect* d_records, long long* d_sums, float* d_profile, uint8_t* d_stack, size_t stack_step,
                              uint8_t* d_hov, size_t hov_step, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records and the summary of the last
 * push that computed them (host memory); zeros before that. */
int rcflow_transects_read(rc_ctx* ctx, int stream, rc_transect* records, long long summary[8]);
/* Blocks; for tests.  Each may be NULL: the accumulators as lines x (2 D + 1) x 3 int64 (Tab, Tb, Tbb; d = -D first) and the
 * lines' own as lines x 2 int64 (Ta, Taa) */
int rcflow_transects_sums_read(rc_ctx* ctx, int stream, long long* sums, long long* line_sums);
/* Blocks.  Each may be NULL: the open session's table (S records) and per-line constants (lines records), from the device */
int rcflow_transects_table_read(rc_ctx* ctx, int stream, rc_transect_sample* table, rc_transect_geom* geom);
/* jet_min and vis_max from the next push on; RC_EINVAL unless jet_min is > 0 and below 2^20 and vis_max finite and > 0 */
int rcflow_transects_set(rc_ctx* ctx, int stream, double jet_min, double vis_max);
/* zeroes the rings, the accumulators, the records, the summary and the push count; keeps the table and the allocation;
 * asynchronous, on the slot's stream */
int rcflow_transects_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_transects_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_transects_info(rc_ctx* ctx, int stream, rc_transects_info* info);

/* ------------------------------------------------------------------ flow kinematics: vorticity, divergence, Okubo-Weiss, cores
 * Every product above says where the water goes.  This one says how the field turns and spreads at a point, which is what a
 * rip looks like in a velocity field: the neck is a jet between two shear layers of opposite vorticity, the head a
 * counter-rotating vortex pair, the feeders converge (negative divergence).  It is the Eulerian counterpart of the FTLE: one
 * field in, no ring, stateless in time (time averaging is the caller's: push rcflow_ripmap_mean_dev's window mean).  It takes
 * every 32FC2 field the library makes (Farneback, the window mean, the plan view's metric field, the PIV field) and its mask
 * goes into rcflow_regions_* / rcflow_tracks_* unchanged.  The reference has only the display colouring of the raw one-pixel
 * Jacobian's norm (rcflow_shear_rate_to_color_dev).  tests/_kinematics_ref.py states the following in numpy and the kernels
 * equal it bit for bit.  All fp32 unless stated, each operation rounded on its own (no fused multiply-add); every integer
 * is exact.  Picture coordinates: x to the right, y DOWN, so positive vorticity turns CLOCKWISE as the picture shows it.
 *
 *  Taps (host, double; rcflow_kinematics_taps gives them without a context).  R = radius.  e_k = exp(-k^2 / (2 sigma^2)) for
 *  k = 0..R; Z = e_0 + 2 (e_1 + ... + e_R), the bracket summed ascending, then doubled, then e_0 added; g_k = (float)(e_k / Z).
 *  R = 0: g_0 = 1 and sigma is ignored.
 *  Interior.  m = R + s, s = spacing.  A pixel is INTERIOR when m <= x < w - m and m <= y < h - m.  No index is ever clamped:
 *  nothing outside the picture is read (a replicated border would bias the derivatives).
 *
 *  1. "kinematics@0".  Per component F of the field, horizontally: H = g_0 * F(x, y), then for k = 1..R
 *     H = H + g_k * (F(x - k, y) + F(x + k, y)), the bracket rounded first.  Then vertically, the same recurrence on H:
 *     S = g_0 * H(x, y), S = S + g_k * (H(x, y - k) + H(x, y + k)).  inv = (float)(scale / (2 s)); E, W, S, N the smoothed
 *     values at x + s, x - s, y + s, y - s:
 *       ux = (S_E.x - S_W.x) * inv    vx = (S_E.y - S_W.y) * inv    uy = (S_S.x - S_N.x) * inv    vy = (S_S.y - S_N.y) * inv
 *     An interior pixel is BAD when any of the four is not finite or reaches 8 in magnitude; it is counted, its omega, div
 *     and ow are 0 and it is part of nothing.  VALID: interior and not bad.  For a valid pixel
 *       omega = vx - uy    div = ux + vy    sn = ux - vy    ss = vx + uy    ow = (sn*sn + ss*ss) - omega*omega
 *       e = omega*omega    w2 = ow*ow
 *     Outside the interior omega, div and ow are 0.  Q(x) = (int64)rint((double)x * 65536); the bound 8 gives |omega| < 16,
 *     |ow| < 512 and w2 < 2^18, so with w * h <= 2^25 every sum stays below 2^59.  Per cell (ripmap's rule: column
 *     min(x / (w / grid_x), grid_x - 1), likewise for rows), int64: n_valid, n_bad, sum Q(omega), sum Q(div), sum Q(e),
 *     sum Q(ow), sum Q(w2).  Also the largest |omega| over the valid pixels.  d_omega, d_div and d_ow are written here.
 *     Threshold, by the launch's last-arriving workgroup, in double with + - * / only: n, SW, SW2 the sums of n_valid,
 *     Q(ow), Q(w2) over the cells; mean = ((double)SW / 65536) / n; m2 = ((double)SW2 / 65536) / n; var = m2 - mean * mean,
 *     0 when that is negative or n = 0.  With RC_KINEMATICS_RELATIVE T2 = (ow_k * ow_k) * var (the usual "W below -0.2 sigma_W"
 *     with no square root in it), else T2 = ow_min * ow_min, computed on the host.
 *  2. "kinematics@1".  A valid pixel is a CORE when ow < 0, (double)ow * (double)ow > T2 (the product is exact) and
 *     fabsf(omega) >= (float)omega_min.  Mask (8UC1): 255 at a core, else 0; it is what rcflow_regions_push_dev takes.
 *     Picture (8UC3): entry i of rcflow_jet_lut, i = rint(omega / (float)vis_max * 127.5f + 127.5f) saturated to 0..255, as the
 *     transects' Hovmoeller picture; black where the pixel is not valid.  Per cell four more int64: core pixels with
 *     omega > 0, core pixels with omega < 0, sum Q(omega) over each kind: RC_KINEMATICS_SUMS words per cell in that order
 *     after the seven above.  The last-arriving workgroup closes the records in double: flags RC_KINEMATICS_EMPTY when
 *     n_valid = 0, RC_KINEMATICS_CW when positive cores >= min_core, RC_KINEMATICS_CCW likewise; with S the cell's sum Q(.)
 *     a mean is (float)(((double)S / 65536) / n_valid) and a circulation (float)(((double)S / 65536) * pixel_area).  For an
 *     empty cell every value except flags is 0.
 *     Summary, 8 int64: valid pixels | bad pixels | cores cw | cores ccw | the bits of T2 (a double) | cells with both CW and
 *     CCW | pushes since open / reset | the bits of the largest |omega| as uint32. */
#define RC_KINEMATICS_RELATIVE 1         /* rc_kinematics_params::flags: the threshold is ow_k^2 times the variance of ow */
#define RC_KINEMATICS_EMPTY 1            /* rc_kinematics_cell::flags */
#define RC_KINEMATICS_CW 2
#define RC_KINEMATICS_CCW 4
#define RC_KINEMATICS_MAX_RADIUS 8
#define RC_KINEMATICS_MAX_SPACING 8
#define RC_KINEMATICS_MAX_PIXELS (1 << 25)
#define RC_KINEMATICS_SUMS 11            /* int64 per cell in d_sums */
#define RC_KINEMATICS_LAUNCHES 2         /* of a push with any output; a push with none queues nothing */
typedef struct rc_kinematics_params {
    int radius;             /* R: 0..RC_KINEMATICS_MAX_RADIUS, half-width of the smoothing; 0: none */
    int spacing;            /* s: 1..RC_KINEMATICS_MAX_SPACING, half-width of the central differences */
    int grid_x, grid_y;     /* >= 1, <= w, h, at most RC_RIPMAP_MAX_CELLS cells */
    int min_core;           /* >= 1: core pixels of one sign that flag a cell */
    int flags;              /* RC_KINEMATICS_RELATIVE or 0 */
    int pad[2];             /* so that the doubles are aligned; not read */
    double sigma;           /* finite, > 0; ignored when R = 0 */
    double scale;           /* finite, > 0: differences into rates: fps for a pixel field, 1 / metres per cell for the plan view's */
    double pixel_area;      /* finite, > 0: the area one pixel stands for */
    double ow_k;            /* finite, >= 0: RELATIVE */
    double ow_min;          /* finite, >= 0: otherwise */
    double omega_min;       /* finite, >= 0 */
    double vis_max;         /* finite, > 0: the |omega| the picture's end colours stand for */
} rc_kinematics_params;
typedef struct rc_kinematics_cell {
    int flags;              /* RC_KINEMATICS_EMPTY, CW, CCW */
    int n, bad;             /* the cell's n_valid, n_bad */
    float mean_vorticity, circulation, mean_divergence, enstrophy, mean_ow;
    int cores_cw, cores_ccw;
    float circulation_cw, circulation_ccw;
} rc_kinematics_cell;       /* 48 bytes */
typedef struct rc_kinematics_info {
    int w, h;
    rc_kinematics_params prm;          /* ow_k, ow_min, omega_min and vis_max as rcflow_kinematics_set left them */
    int margin;                        /* m = R + s */
    int launches_per_push;             /* RC_KINEMATICS_LAUNCHES */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_kinematics_info;
/* The taps g_0..g_radius into taps[radius + 1]; needs no context and no GPU.  RC_EINVAL: radius outside
 * 0..RC_KINEMATICS_MAX_RADIUS, no buffer, or with radius > 0 a sigma that is not finite and > 0. */
int rcflow_kinematics_taps(int radius, double sigma, float* taps);
/* Allocates two planes of 4 B/px, the cell sums and the records.  Re-opening replaces the state; a refused open leaves the open
 * state as it was.  RC_EINVAL: no parameters, a value outside the ranges above, unknown flag bits, w < 2 m + 1 or h < 2 m + 1;
 * RC_ESIZE beyond the context's max_w x max_h or w * h above RC_KINEMATICS_MAX_PIXELS. */
int rcflow_kinematics_open(rc_ctx* ctx, int stream, int w, int h, const rc_kinematics_params* prm);
/* One flow field (32FC2, w x h, pointer and step multiples of 8, step >= 8 w).  Outputs (device memory, each may be NULL):
 * d_omega, d_div, d_ow 32FC1 (4-byte aligned, steps multiples of 4), d_mask 8UC1, d_vis 8UC3, d_cells grid_y x grid_x
 * rc_kinematics_cell (4-byte aligned), d_sums grid_y x grid_x x RC_KINEMATICS_SUMS int64 and d_summary 8 int64 (8-byte
 * aligned).  With every output NULL the push only counts and queues no launch; with any it is RC_KINEMATICS_LAUNCHES, and
 * what they give depends neither on which outputs were asked for nor on earlier pushes.  No host synchronisation, no
 * device-to-host copy.  An output whose byte range overlaps the field's or another output's is RC_EINVAL.  Row padding is never
 * written.  Every refusal is decided before anything is queued and leaves the state as it was; RC_ESTATE before
 * rcflow_kinematics_open. */
int rcflow_kinematics_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step,
                               float* d_omega, size_t omega_step, float* d_div, size_t div_step, float* d_ow, size_t ow_step,
                               uint8_t* d_mask, size_t mask_step, uint8_t* d_vis, size_t vis_step,
                               rc_kinematics_cell* d_cells, long long* d_sums, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Records, sums and summary of the last push that had an
 * output (each may be NULL); zeros before that. */
int rcflow_kinematics_read(rc_ctx* ctx, int stream, rc_kinematics_cell* cells, long long* sums, long long summary[8]);
/* ow_k, ow_min, omega_min and vis_max from the next push on; RC_EINVAL as rcflow_kinematics_open */
int rcflow_kinematics_set(rc_ctx* ctx, int stream, double ow_k, double ow_min, double omega_min, double vis_max);
/* zeroes the records, the sums, the summary and the push count; keeps the parameters as set and the allocation; asynchronous,
 * on the slot's stream */
int rcflow_kinematics_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_kinematics_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer (as rcflow_transects_info) */
int rcflow_kinematics_info(rc_ctx* ctx, int stream, rc_kinematics_info* info);

/* ------------------------------------------------------------------ shoreline: wet/dry split, waterline per line, runup
 * Every product above measures the water; this one says where it ends.  The waterline fixes where "offshore" is and bounds the
 * surf zone the opposing-flow map, the regions and the transects are read in; its movement over a window is the runup, whose
 * excursion and per-mille exceedance position are the statistics of the swash.  It takes the pictures that are already on the
 * device: the time-exposure MEAN, the plan view's picture, a raw 8UC3 frame, or an 8UC1 plane of the caller's.  The reference
 * has no such product.  tests/_shoreline_ref.py states the following in numpy and the kernels equal it bit for bit on every
 * output.  Everything is exact integer arithmetic except the two places that say double; there every operation is rounded on
 * its own.
 *
 *  Geometry (host, once; rcflow_shoreline_plan gives it without a context).  Lines are rc_transect_line records running FROM
 *  LAND (x0, y0) TO SEA (x1, y1), listed in alongshore order.  The table (rc_transect_sample) and the per-line constants
 *  (rc_transect_geom) are those of rcflow_transects_plan with fps = 1: positions quantised to 1/16 pixel, ds in metres.  Limits
 *  of its own: 1..RC_SHORE_MAX_LINES lines, n in RC_SHORE_MIN_SAMPLES..RC_SHORE_MAX_SAMPLES, S = sum of n at most
 *  RC_SHORE_MAX_TOTAL.
 *  1. "shoreline@0", pixels.  Indicator I per pixel: RC_SHORE_RMB byte2 - byte0 + 255 (R - B + 255 of a BGR picture, 0..510),
 *     RC_SHORE_GRAY (byte0 * 1868 + byte1 * 9617 + byte2 * 4899 + 8192) >> 14 (the library's BGR -> grey integers),
 *     RC_SHORE_PLANE the byte of the caller's 8UC1 plane.  Box sum over (2 r + 1)^2 with a REPLICATED border (coordinates clamped
 *     to the picture: harmless for an intensity, unlike the kinematics' derivatives).  A = (2 r + 1)^2; J = (2 sum + A) / (2 A),
 *     uint16 in 0..510, kept in a state plane.  Histogram of J, 511 live bins of uint32, over every pixel or over those where
 *     the push's d_roi (8UC1) is non-zero; N its total.  Otsu, by the launch's last-arriving workgroup: S1 = sum i h[i],
 *     S2 = sum i^2 h[i]; for t = 0..509 in order w0 += h[t], m0 += t h[t], w1 = N - w0, t skipped when w0 or w1 is 0;
 *     a = S1 w0 - m0 N (int64); s = ((double)a * (double)a) / ((double)w0 * (double)w1); the FIRST largest s wins, thr its t.
 *     tot = (double)N * (double)S2 - (double)S1 * (double)S1; eta = tot > 0 ? s / tot : 0, Otsu's separability in 0..1.  With
 *     no admissible t (N = 0, or one bin) thr = -1 and eta = 0.  A fixed threshold >= 0 is used as given, eta is s / tot of
 *     that t (0 when it is skipped), and thr is still -1 when N = 0.  With thr = -1 every line is RC_SHORE_EMPTY (k 0, pos -1,
 *     agree 0) and the mask is 0.  w * h <= RC_SHORE_MAX_PIXELS keeps every int64 below 2^59.
 *  2. "shoreline@1", lines, a wave a line.  V[j]: the integer bilinear sample of J at the table position, the GRAY formula of the
 *     transects (weights in 16ths, + 128 >> 8, ix1 = min(ix + 1, w - 1), iy1 likewise).  wet[j] = V[j] <= thr, or V[j] > thr with
 *     wet_is_high.  BEST SPLIT, not first crossing: for k in 0..n, score(k) = #dry in [0, k) + #wet in [k, n); k* is the smallest
 *     k of the largest score (the most landward among equals), agree = score(k*).  k* = n: RC_SHORE_DRY, k* = 0: RC_SHORE_WET,
 *     both with pos = -1 and wx = wy = 0.  Otherwise sample k* - 1 is dry and k* is wet; a = V[k* - 1], b = V[k*], d = |b - a|,
 *     e = |2 thr + 1 - 2 a|; frac = (e * 256 + d) / (2 d), 0..256; pos = (k* - 1) * 256 + frac, in 1/256 sample.
 *     RC_SHORE_UNSURE on every line that is not EMPTY when eta < min_sep.  The waterline point in 1/256 pixel, from the table's
 *     end positions Xa, Xb (1/16 px): wx = 16 Xa + floor((16 (Xb - Xa) pos + 128 (n - 1)) / (256 (n - 1))), wy likewise.
 *  3. "shoreline@2", along the shore and over the window, a workgroup a line.  On each side of line i the neighbour is the
 *     nearest line within 2 places that has a position in this push (outliers included).  A line with a position and a neighbour
 *     is RC_SHORE_OUTLIER when for every such neighbour max(|dwx|, |dwy|) > (int64)rint(max_jump * 256).  It keeps pos, wx and wy.
 *     Ring: slot pushes mod T of the line takes pos, or -1 for no position or an outlier.  Over the held = min(pushes + 1, T)
 *     slots, on the values >= 0: nv, pos_min, pos_max, the int64 sum, and pos_q = the value at ascending rank
 *     (nv * p + 999) / 1000 - 1, the position that p per mille of the waterlines reached or passed landward; all 0 with
 *     RC_SHORE_NO_WINDOW when nv = 0.  Record: x = (float)((double)wx / 256), y likewise, dist_m = (float)(((double)pos / 256)
 *     * ds) (0 without a position), pos_mean = (float)((double)sum / (double)nv), excursion_m = (float)(((double)(pos_max -
 *     pos_min) / 256) * ds).  Summary, 8 int64: thr | N | (int64)rint(eta * 2^32) | lines with a position and no OUTLIER | DRY
 *     lines | WET lines | outliers | pushes since open / reset.
 *  4. "shoreline@3", when a picture is asked for: d_mask 8UC1, 255 where J is wet (what rcflow_regions_push_dev and
 *     rcflow_create_edges_dev take); d_plane 16UC1, J; d_hist 512 uint32, the last bin 0.
 *  5. "shoreline@4": rcflow_shoreline_prims_dev gives 2 lines - 1 primitives of the last push for rcflow_draw_dev: record 2 i a
 *     disc at ((wx + 128) >> 8, (wy + 128) >> 8) for line i when it has a position and is no OUTLIER; record 2 i + 1 the
 *     segment from such a line i to the next such line after it (lines between them that have none are bridged); all-zero
 *     records elsewhere, as rcflow_regions_prims_dev leaves them. */
#define RC_SHORE_RMB 0                   /* rc_shoreline_params::source */
#define RC_SHORE_GRAY 1
#define RC_SHORE_PLANE 2
#define RC_SHORE_EMPTY 1                 /* rc_shoreline::flags */
#define RC_SHORE_DRY 2
#define RC_SHORE_WET 4
#define RC_SHORE_UNSURE 8
#define RC_SHORE_OUTLIER 16
#define RC_SHORE_NO_WINDOW 32
#define RC_SHORE_MAX_LINES 1024
#define RC_SHORE_MIN_SAMPLES 8
#define RC_SHORE_MAX_SAMPLES 1024
#define RC_SHORE_MAX_TOTAL 262144
#define RC_SHORE_MAX_RADIUS 7
#define RC_SHORE_MAX_WINDOW 4096
#define RC_SHORE_MAX_PIXELS (1 << 25)
#define RC_SHORE_MAX_STATE_BYTES (64ull << 20)   /* the ring: window x lines int32 */
#define RC_SHORE_HIST 512                /* uint32 in d_hist: 511 live bins and a zero */
#define RC_SHORE_LAUNCHES 4              /* of a push that asks for a picture; 3 otherwise */
typedef struct rc_shoreline_params {
    int source;             /* RC_SHORE_RMB, RC_SHORE_GRAY (both 8UC3) or RC_SHORE_PLANE (8UC1) */
    int radius;             /* r: 0..RC_SHORE_MAX_RADIUS, half-width of the box */
    int wet_is_high;        /* 0: wet where J <= thr; 1: wet where J > thr */
    int threshold;          /* -1: Otsu; 0..509: fixed */
    int window;             /* T: 2..RC_SHORE_MAX_WINDOW pushes held per line */
    int permille;           /* p: 1..999 */
    int flags;              /* 0 */
    int pad;
    double min_sep;         /* 0..1: below this separability every line is RC_SHORE_UNSURE */
    double max_jump;        /* pixels, > 0 and <= 16384: the outlier test */
    double metres_per_pixel; /* finite, > 0 */
} rc_shoreline_params;
typedef struct rc_shoreline {
    int flags;              /* RC_SHORE_EMPTY, DRY, WET, UNSURE, OUTLIER, NO_WINDOW */
    int k;                  /* k*: the first wet sample of the best split */
    int pos;                /* 1/256 sample from the land end, or -1 */
    int agree;              /* score(k*): samples on the side the split puts them */
    int wx, wy;             /* the waterline point in 1/256 pixel */
    float x, y;             /* the same in pixels */
    float dist_m;           /* metres from the land end */
    int nv;                 /* positions in the window */
    int pos_min, pos_max, pos_q;
    float pos_mean;
    float excursion_m;      /* metres between pos_min and pos_max */
    int pad;
} rc_shoreline;             /* 64 bytes */
typedef struct rc_shoreline_info {
    int w, h;
    rc_shoreline_params prm;           /* threshold, min_sep and max_jump as rcflow_shoreline_set left them */
    int lines, samples;                /* S */
    int launches_per_push;             /* RC_SHORE_LAUNCHES */
    int held;                          /* min(pushes, T) */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_shoreline_info;
/* The geometry alone: no context, no GPU.  table: S records in line order, geom: n_lines records, total: S; each may be NULL.
 * RC_EINVAL: no lines, more than RC_SHORE_MAX_LINES, an n outside RC_SHORE_MIN_SAMPLES..RC_SHORE_MAX_SAMPLES, S above
 * RC_SHORE_MAX_TOTAL, an endpoint that is not finite, a line of no length, a sample outside the picture, metres_per_pixel not
 * finite and > 0. */
int rcflow_shoreline_plan(int w, int h, const rc_transect_line* lines, int n_lines, double metres_per_pixel,
                          rc_transect_sample* table, rc_transect_geom* geom, int* total);
/* Allocates everything the slot will ever need: the table, the plane (2 B/px), the ring (4 T lines bytes), the records.
 * Re-opening replaces the state; a refused open leaves the open state as it was.  RC_EINVAL as rcflow_shoreline_plan, no
 * parameters, a value outside the ranges above, unknown flag bits; RC_ESIZE beyond the context's max_w x max_h, w * h above
 * RC_SHORE_MAX_PIXELS, or a ring above RC_SHORE_MAX_STATE_BYTES. */
int rcflow_shoreline_open(rc_ctx* ctx, int stream, int w, int h, const rc_transect_line* lines, int n_lines, const rc_shoreline_params* prm);
/* One picture: d_image w x h with `channels` bytes a pixel, 3 for RC_SHORE_RMB and RC_SHORE_GRAY, 1 for RC_SHORE_PLANE (anything
 * else is RC_EINVAL); d_roi (8UC1, may be NULL): the histogram counts where it is non-zero.  Outputs (device memory, each may be
 * NULL): d_records lines x rc_shoreline (4-byte aligned), d_mask 8UC1, d_plane 16UC1 (pointer and step multiples of 2), d_hist
 * RC_SHORE_HIST uint32 (4-byte aligned), d_summary 8 int64 (8-byte aligned).  "shoreline@0..@2" run on every push, because the
 * ring must be fed; "shoreline@3" follows when d_mask, d_plane or d_hist is asked for; what a push gives does not depend on which
 * outputs earlier pushes asked for.  No host synchronisation, no device-to-host copy.  An output whose byte range overlaps an
 * input's or another output's is RC_EINVAL.  Row padding is never written.  Every refusal is decided before anything is queued
 * and leaves the state as it was; RC_ESTATE before rcflow_shoreline_open.  RC_EHIP (the runtime refused a launch) is no refusal:
 * launches before it may have written the ring while the push count stays, so the state is undefined until
 * rcflow_shoreline_reset. */
int rcflow_shoreline_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_image, size_t step, int channels, const uint8_t* d_roi, size_t roi_step,
                              rc_shoreline* d_records, uint8_t* d_mask, size_t mask_step, uint16_t* d_plane, size_t plane_step,
                              uint32_t* d_hist, long long* d_summary);
/* 2 lines - 1 primitives of the last push into d_prims ("shoreline@4"); thickness and disc_radius as rcflow_regions_prims_dev */
int rcflow_shoreline_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, rc_draw_prim* d_prims);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records and the summary of the last
 * push (host memory); zeros before the first. */
int rcflow_shoreline_read(rc_ctx* ctx, int stream, rc_shoreline* records, long long summary[8]);
/* Blocks.  The runup time series, lines x T int32 (host memory): per line the held positions oldest first, then -1 up to T */
int rcflow_shoreline_ring_read(rc_ctx* ctx, int stream, int* ring);
/* Blocks.  Each may be NULL: the open session's table (S records) and per-line constants (lines records), from the device */
int rcflow_shoreline_table_read(rc_ctx* ctx, int stream, rc_transect_sample* table, rc_transect_geom* geom);
/* threshold, min_sep and max_jump from the next push on; RC_EINVAL as rcflow_shoreline_open */
int rcflow_shoreline_set(rc_ctx* ctx, int stream, int threshold, double min_sep, double max_jump);
/* zeroes the ring, the records, the summary and the push count; keeps the table, the allocation and the parameters as
 * rcflow_shoreline_set left them; asynchronous, on the slot's stream */
int rcflow_shoreline_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_shoreline_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_shoreline_info(rc_ctx* ctx, int stream, rc_shoreline_info* info);

/* ------------------------------------------------------------------ surf: breaking fraction, variance image, rip channels
 * The shoreline bounds the surf zone on the land side; this product says where the waves break, how often, and where the band of
 * breaking has a hole.  A rip channel shows as a gap in that band: dark in a time exposure, quiet in the variance image, with a
 * low fraction of time breaking.  It uses no flow at all, so it cross-checks the flow-side detectors where Farneback is least to
 * be trusted: inside the foam.  It takes grey frames (8UC1: rcflow_resize_bgr_to_gray_dev, the plan view's picture).  The
 * reference has no such product.  tests/_surf_ref.py states the following in numpy and the kernels equal it bit for bit on every
 * output of every push.  Everything is exact integer arithmetic except the float conversions named under the records; those are
 * computed in double, each operation rounded on its own.
 *
 *  Geometry (host, once; rcflow_surf_plan gives it without a context).  Lines are rc_transect_line records FROM LAND TO SEA in
 *  alongshore order; the table and the per-line constants are the shoreline's (positions in 1/16 pixel, fps = 1), the limits its
 *  own: 0..RC_SURF_MAX_LINES lines, n in RC_SURF_MIN_SAMPLES..RC_SURF_MAX_SAMPLES, S = sum of n at most RC_SURF_MAX_TOTAL.  With
 *  ZERO lines the session is pixels only: "surf@1" and "surf@2" do not run and the line outputs must be NULL.
 *  State.  A ring of W = window grey frames, zero at open and reset.  Per pixel S1 = sum of the ring (uint32), S2 = sum of its
 *  squares (uint32: 4096 * 255^2 < 2^32), Q (uint16) = flags set among the held frames; a flag ring of one bit per pixel and held
 *  frame.  The planes have a row pitch P = w rounded up to 4 and the flags are kept per run of 256 pixels of P h, so the state is
 *  P h (W + 10) + 32 W ceil(P h / 256) bytes; beyond RC_SURF_MAX_STATE_BYTES rcflow_surf_open answers RC_ESIZE with the count.
 *  1. "surf@0", pixels, every push.  g: the frame.  c = pushes mod W; old = ring[c]; S1 += g - old; S2 += g^2 - old^2; ring[c] = g.
 *     n = min(pushes + 1, W).  b = (g >= bright) and (g n >= S1 + delta n), S1 after the update: bright now AND at least delta above
 *     the pixel's own window mean; persistent foam, white sand and a saturated sky are bright but not above their mean; on the
 *     very first push nothing breaks when delta > 0.  Q += b - bit[c]; bit[c] = b.  Outputs of the same launch, each optional:
 *     d_now 8UC1 255 where b; d_surf 8UC1 255 where Q 1000 >= q_min n (what rcflow_regions_push_dev takes); d_q 16UC1 Q;
 *     d_mean 8UC1 (2 S1 + n) / (2 n); d_sd 8UC1 min(255, isqrt(4 (n S2 - S1^2) / n^2)), twice the standard deviation, the
 *     variance image: int64, the inner division floors, isqrt the exact floor square root; d_picture 8UC3 entry i of
 *     rcflow_jet_lut, i = min(255, Q 255000 / (vis_permille n)).  Counts for the summary, by the launch's last-arriving
 *     workgroup: pixels with b, pixels in surf, sum of Q.
 *  2. "surf@1", lines, a wave a line.  V[j]: the integer bilinear sample of the Q plane at the table position (the shoreline's
 *     formula: weights in 16ths, + 128 >> 8, ix1 = min(ix + 1, w - 1), iy1 likewise).  in[j] = V[j] 1000 >= q_min n.  Runs are the
 *     maximal runs of consecutive in-samples at least min_run long; k0 the first sample of the first run, k1 the last sample of
 *     the last run; RC_SURF_NOBAND with k0 = k1 = -1, the edge points and width_m 0 when there is none.  load B = sum of V over
 *     all samples; peak = max V, kpeak its first index.  The inner (ix, iy) and outer (ox, oy) edge points in 1/256 pixel by the
 *     shoreline's formula, X = 16 Xa + floor((16 (Xb - Xa) pos + 128 (n - 1)) / (256 (n - 1))) with pos = 256 k0 and 256 k1.
 *     width_m = (float)((double)(k1 - k0 + 1) * ds).
 *  3. "surf@2", along the shore, one workgroup.  For line i of L: lo = max(0, i - span), hi = min(L - 1, i + span), m = hi - lo + 1;
 *     ref = the value of ascending rank (m - 1) / 2 among B[lo..hi], the lower median with the line itself included.
 *     RC_SURF_NOREF when ref < max(min_load, 1); otherwise RC_SURF_CHANNEL when B 1000 < ratio ref (int64).  share = ref > 0 ?
 *     min(B 1000 / ref, RC_SURF_MAX_SHARE) : 1000.  Channels are the maximal runs of consecutive CHANNEL lines at least min_lines
 *     long, in line order; their lines also carry RC_SURF_IN_CHANNEL.  The first RC_SURF_MAX_CHANNELS are recorded (the records
 *     past them are zero), the summary counts them all.  rc_surf_channel: first, count, centre = the line of least share (lowest
 *     index on ties), its share; the centre point (cx, cy) in 1/256 pixel on the centre line (n_c samples) at pos: the flanking
 *     lines are first - 1 and first + count, E those that exist and have a band; pos = (sum over E of 128 (k0 + k1)) / |E|
 *     (integer division) clamped to 256 (n_c - 1), and 128 (n_c - 1) with E empty.  width_m: with (dx, dy) in 1/16 pixel between
 *     the land ends (the table's first samples) of lines max(first - 1, 0) and min(first + count, L - 1),
 *     (float)((sqrt((double)(dx^2 + dy^2)) / 16) * metres_per_pixel).
 *     Summary, 8 int64: n | pixels breaking now | surf pixels | sum of Q | lines with a band | CHANNEL lines | channels (all) |
 *     pushes since open / reset.
 *  4. "surf@3": rcflow_surf_prims_dev gives L - 1 + RC_SURF_MAX_CHANNELS primitives of the last push for rcflow_draw_dev: record
 *     i < L - 1 the segment from line i's outer edge point ((ox + 128) >> 8, (oy + 128) >> 8) to that of the next line that has a
 *     band, when line i has one (the breaker line, bridged over channel lines as the shoreline bridges); record L - 1 + k a disc
 *     at channel k's centre; all-zero records elsewhere and before the first push. */
#define RC_SURF_NOBAND 1                 /* rc_surf_line::flags */
#define RC_SURF_NOREF 2
#define RC_SURF_CHANNEL 4
#define RC_SURF_IN_CHANNEL 8
#define RC_SURF_MAX_LINES 1024
#define RC_SURF_MIN_SAMPLES 8
#define RC_SURF_MAX_SAMPLES 1024
#define RC_SURF_MAX_TOTAL 262144
#define RC_SURF_MAX_WINDOW 4096
#define RC_SURF_MAX_SPAN 32
#define RC_SURF_MAX_CHANNELS 32
#define RC_SURF_MAX_SHARE 1000000
#define RC_SURF_MAX_PIXELS (1 << 25)
#define RC_SURF_MAX_STATE_BYTES (4ull << 30)     /* ring, flag ring, S1, S2 and Q */
#define RC_SURF_LAUNCHES 3               /* of a push of a session with lines; 1 without */
typedef struct rc_surf_params {
    int window;             /* W: 2..RC_SURF_MAX_WINDOW frames held per pixel */
    int bright;             /* 0..255: a breaking pixel is at least this bright */
    int delta;              /* 0..255: and at least this far above its window mean */
    int q_min;              /* per mille, 1..1000: fraction of time breaking that puts a pixel in the surf zone */
    int min_run;            /* 1..64 samples in a surf run */
    int span;               /* a: 0..RC_SURF_MAX_SPAN lines on either side for the alongshore reference */
    int ratio;              /* per mille, 1..999: a line below this share of the reference is a channel line */
    int min_load;           /* >= 0: the smallest reference that counts */
    int min_lines;          /* 1..64 lines in a channel */
    int vis_permille;       /* 1..1000: the fraction the picture's last colour stands for */
    int flags;              /* 0 */
    int pad;
    double metres_per_pixel; /* finite, > 0 */
} rc_surf_params;
typedef struct rc_surf_line {
    int flags;              /* RC_SURF_NOBAND, NOREF, CHANNEL, IN_CHANNEL */
    int k0, k1;             /* the band's first and last sample, or -1 */
    int load;               /* B */
    int peak, kpeak;        /* the largest V and its first sample */
    int ix, iy;             /* the inner edge point in 1/256 pixel */
    int ox, oy;             /* the outer edge point */
    int ref;                /* the alongshore reference */
    int share;              /* per mille of it */
    float width_m;          /* the band's width in metres */
    int pad[3];
} rc_surf_line;             /* 64 bytes */
typedef struct rc_surf_channel {
    int first, count;       /* its lines */
    int centre;             /* the line of least share */
    int share;              /* there */
    int cx, cy;             /* the centre point in 1/256 pixel */
    float width_m;          /* alongshore, in metres */
    int pad;
} rc_surf_channel;          /* 32 bytes */
typedef struct rc_surf_info {
    int w, h;
    rc_surf_params prm;                /* as rcflow_surf_set left them */
    int lines, samples;                /* S */
    int launches_per_push;             /* RC_SURF_LAUNCHES, or 1 without lines */
    int held;                          /* min(pushes, W) */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_surf_info;
/* The geometry alone: no context, no GPU.  table: S records in line order, geom: n_lines records, total: S; each may be NULL.
 * RC_EINVAL as rcflow_shoreline_plan, except that no lines at all are allowed (lines may then be NULL). */
int rcflow_surf_plan(int w, int h, const rc_transect_line* lines, int n_lines, double metres_per_pixel, rc_transect_sample* table,
                     rc_transect_geom* geom, int* total);
/* Allocates everything the slot will ever need (the state above, the table, the records).  Re-opening replaces the state; a
 * refused open leaves the open state as it was.  RC_EINVAL as rcflow_surf_plan, no parameters, a value outside the ranges above,
 * unknown flag bits; RC_ESIZE beyond the context's max_w x max_h, w * h above RC_SURF_MAX_PIXELS, or a state above
 * RC_SURF_MAX_STATE_BYTES. */
int rcflow_surf_open(rc_ctx* ctx, int stream, int w, int h, const rc_transect_line* lines, int n_lines, const rc_surf_params* prm);
/* One grey frame: d_gray w x h, channels = 1 (anything else is RC_EINVAL).  Outputs (device memory, each may be NULL): d_now,
 * d_surf, d_mean, d_sd 8UC1; d_q 16UC1 (pointer and step multiples of 2); d_picture 8UC3; d_lines lines x rc_surf_line and
 * d_channels RC_SURF_MAX_CHANNELS x rc_surf_channel (4-byte aligned; RC_EINVAL on a session without lines); d_summary 8 int64
 * (8-byte aligned).  Every launch runs on every push, because the state must be fed; what a push gives does not depend on which
 * outputs it or earlier pushes asked for.  No host synchronisation, no device-to-host copy.  An output whose byte range overlaps
 * the frame's or another output's is RC_EINVAL.  Row padding is never written.  Every refusal is decided before anything is
 * queued and leaves the state as it was; RC_ESTATE before rcflow_surf_open.  RC_EHIP (the runtime refused a launch) is no
 * refusal: the state is undefined until rcflow_surf_reset. */
int rcflow_surf_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, int channels, uint8_t* d_now, size_t now_step,
                         uint8_t* d_surf, size_t surf_step, uint16_t* d_q, size_t q_step, uint8_t* d_mean, size_t mean_step, uint8_t* d_sd,
                         size_t sd_step, uint8_t* d_picture, size_t picture_step, rc_surf_line* d_lines, rc_surf_channel* d_channels,
                         long long* d_summary);
/* lines - 1 + RC_SURF_MAX_CHANNELS primitives of the last push into d_prims ("surf@3"); thickness and disc_radius as
 * rcflow_regions_prims_dev; RC_EINVAL on a session without lines */
int rcflow_surf_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, rc_draw_prim* d_prims);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the line records, the
 * RC_SURF_MAX_CHANNELS channel records and the summary of the last push (host memory); zeros before the first. */
int rcflow_surf_read(rc_ctx* ctx, int stream, rc_surf_line* lines, rc_surf_channel* channels, long long summary[8]);
/* Blocks.  Each may be NULL: the open session's table (S records) and per-line constants (lines records), from the device */
int rcflow_surf_table_read(rc_ctx* ctx, int stream, rc_transect_sample* table, rc_transect_geom* geom);
/* bright, delta, q_min, ratio, min_load and vis_permille from the next push on; RC_EINVAL as rcflow_surf_open */
int rcflow_surf_set(rc_ctx* ctx, int stream, int bright, int delta, int q_min, int ratio, int min_load, int vis_permille);
/* zeroes the ring, the flags, the sums, the records, the summary and the push count; keeps the table, the allocation and the
 * parameters as rcflow_surf_set left them; asynchronous, on the slot's stream */
int rcflow_surf_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_surf_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_surf_info(rc_ctx* ctx, int stream, rc_surf_info* info);

/* ------------------------------------------------------------------ mean flow: mean current, steadiness, spread, seaward-jet mask
 * What the water does on average over some wave periods, per pixel, and how reliably it does it: the quantity time-averaged
 * optical-flow rip detection rests on.  A rip neck is a place where the flow is steady (|mean vector| close to the mean speed), fast
 * enough to matter, and runs seaward; wave orbital motion is fast but unsteady, noise is steady nowhere.  The mask goes straight
 * into rcflow_regions_push_dev / rcflow_tracks_push_dev, the exact mean field into the kinematics, FTLE, the transects and the plan
 * view.  The reference has no such product.  tests/_meanflow_ref.py states the following in numpy and the kernels equal it bit for
 * bit on every output of every push.  Integers are exact; the few float results are computed in double, each operation rounded
 * on its own; no atan2 and no angle is computed anywhere on the device.
 *
 *  Sample.  The input is a flow field, w x h CV_32FC2 (pointer and step multiples of 8); d_flow_xy NULL is the field the slot's
 *  frame loop left resident (rcflow_stream_flow_ptr), as rcflow_ripmap_push_dev takes it.  A pixel's sample is BAD when a component
 *  is not finite or fabsf(component) >= 500.0f; otherwise q = (int)rintf(component * 64.0f) per component: 1/64 pixel, |q| <= 32000.
 *  State.  A ring of W = window entries (int16 u, int16 v) per pixel, u = -32768 for a bad sample; an entry that was never written
 *  counts as bad.  Per pixel, over the valid entries held: n their count (uint16), Su, Sv (int32: 4096 * 32000 < 2^31), Suu, Svv,
 *  Suv (int64), Sm = the sum of m = isqrt(u^2 + v^2), the exact floor square root (uint32).  A push at slot c = pushes mod W takes
 *  the old entry out of the sums if it was valid, puts the new one in if it is valid, and stores the new entry or the bad marker.
 *  The planes have a row pitch P = w rounded up to 4, so the state is P h (4 W + 38) bytes; beyond RC_MEANFLOW_MAX_STATE_BYTES
 *  rcflow_meanflow_open answers RC_ESIZE with the count.
 *  1. "meanflow@0", every push.  After the update a pixel is FILLED when n >= min_fill; a pixel that is not gives zeros in every
 *     picture.  d_mean 32FC2 (pointer and step multiples of 8): (float)(((double)Su / 64.0) / (double)n), likewise v: the field
 *     every flow consumer takes.  d_steady 16UC1, per mille: R = isqrt(Su^2 + Sv^2) in int64; st = Sm > 0 ? min(1000, R 1000 / Sm)
 *     : 0.  d_std 32FC2, the major and the minor standard deviation in pixels: a = n Suu - Su^2, c = n Svv - Sv^2, b = n Suv -
 *     Su Sv in int64 (n Suu stays below 1.8e16); A, B, C their doubles; r = sqrt((A - C) (A - C) + 4.0 (B B)); l1 = ((A + C) + r)
 *     0.5; l2 = max(((A + C) - r) 0.5, 0); major = (float)(sqrt(l1) / (64.0 (double)n)), minor the same from l2.  The ellipse's
 *     orientation is not part of this product.  d_picture 8UC3: entry st 255 / 1000 of rcflow_jet_lut, black where the pixel is
 *     not filled.  Cells are the opposing-flow map's: grid_x x grid_y of them, w / grid_x by h / grid_y pixels, the remainder
 *     columns and rows to the last cell, at most RC_RIPMAP_MAX_CELLS.  RC_MEANFLOW_SUMS = 8 int64 per cell: filled pixels | sum of
 *     n | sum of Su | sum of Sv | sum of Sm | mask pixels | pixels whose newest sample was bad | 0; all over the cell's filled
 *     pixels, except the bad count, which is over all of them.  G = the sum over all cells of (sum of Su, sum of Sv).
 *  2. "meanflow@1", every push.  d_mask 8UC1, 255 / 0 (what rcflow_regions_push_dev takes).  A pixel is in when it is filled,
 *     st >= steady_min, R >= smin_q n in int64 with smin_q = ceil(speed_min * 64) taken on the host, and it runs along D, decided
 *     in double as the opposing-flow map decides its cells: S = ((double)Su, (double)Sv); D = (dir_x, dir_y) with
 *     RC_MEANFLOW_DIR_FIXED, D = (-(double)Gx, -(double)Gy) of THIS push with RC_MEANFLOW_DIR_OPPOSED; dot = Sx Dx + Sy Dy;
 *     cc = Sx Sx + Sy Sy; dd = Dx Dx + Dy Dy; in iff dot > 0 && dot dot >= min_cos2 (cc dd).  With G = 0 nothing is opposed.
 *     Records, rc_meanflow_cell, closed by the launch's last-arriving workgroup in double: RC_MEANFLOW_EMPTY when the cell has no
 *     filled pixel (the floats are then 0); mean_x = (float)(((double)(sum of Su) / 64.0) / (double)(sum of n)), mean_y likewise;
 *     steadiness = (float)((sqrt(sx sx + sy sy) / (double)(sum of Sm)) * 1000.0) with sx, sy the doubles of the sums of Su and Sv,
 *     and 0 when the sum of Sm is 0.  Summary, 8 int64: filled pixels | mask pixels | newest-bad pixels | Gx | Gy | sum of Sm |
 *     held = min(pushes, W) | pushes since open / reset. */
#define RC_MEANFLOW_DIR_FIXED 1          /* rc_meanflow_params::flags: exactly one of the two */
#define RC_MEANFLOW_DIR_OPPOSED 2
#define RC_MEANFLOW_EMPTY 1              /* rc_meanflow_cell::flags */
#define RC_MEANFLOW_MAX_WINDOW 4096
#define RC_MEANFLOW_SUMS 8
#define RC_MEANFLOW_MAX_STATE_BYTES (4ull << 30)     /* ring and sum planes */
#define RC_MEANFLOW_LAUNCHES 2           /* of every push */
typedef struct rc_meanflow_params {
    int window;             /* W: 2..RC_MEANFLOW_MAX_WINDOW samples held per pixel */
    int grid_x, grid_y;     /* cells, as rcflow_ripmap_open */
    int min_fill;           /* 1..window valid samples make a pixel filled */
    int steady_min;         /* per mille, 0..1000 */
    int flags;              /* RC_MEANFLOW_DIR_FIXED or RC_MEANFLOW_DIR_OPPOSED */
    double speed_min;       /* pixels per field, finite, 0..400: the least |mean vector| of a mask pixel */
    double min_cos2;        /* K: 0 <= K < 1, the least squared cosine between the mean vector and D */
    double dir_x, dir_y;    /* D with RC_MEANFLOW_DIR_FIXED: finite, not both 0; not looked at otherwise */
} rc_meanflow_params;       /* 56 bytes */
typedef struct rc_meanflow_cell {
    int flags;              /* RC_MEANFLOW_EMPTY */
    int filled;             /* filled pixels */
    int mask;               /* mask pixels */
    int bad;                /* pixels whose newest sample was bad */
    float mean_x, mean_y;   /* pixels per field */
    float steadiness;       /* per mille, of the cell's summed vector */
    int pad;
} rc_meanflow_cell;         /* 32 bytes */
typedef struct rc_meanflow_info {
    int w, h;
    rc_meanflow_params prm;            /* as rcflow_meanflow_set left them */
    int launches_per_push;             /* RC_MEANFLOW_LAUNCHES */
    int held;                          /* min(pushes, W) */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_meanflow_info;
/* Allocates everything the slot will ever need (the state above, the records).  Re-opening replaces the state; a refused open
 * leaves the open state as it was.  RC_EINVAL without parameters, for a value outside the ranges above, flags that are not
 * exactly one of the two directions, a grid that does not fit; RC_ESIZE beyond the context's max_w x max_h or for a state above
 * RC_MEANFLOW_MAX_STATE_BYTES. */
int rcflow_meanflow_open(rc_ctx* ctx, int stream, int w, int h, const rc_meanflow_params* prm);
/* One flow field.  Outputs (device memory, each may be NULL): d_mean and d_std 32FC2 (pointer and step multiples of 8), d_steady
 * 16UC1 (multiples of 2), d_mask 8UC1, d_picture 8UC3; d_cells cells x rc_meanflow_cell (4-byte aligned), d_sums cells x
 * RC_MEANFLOW_SUMS int64 and d_summary 8 int64 (8-byte aligned).  Both launches run on every push, because the state must be fed;
 * what a push gives does not depend on which outputs it or earlier pushes asked for.  No host synchronisation, no device-to-host
 * copy.  An output whose byte range overlaps the field's or another output's is RC_EINVAL.  Row padding is never written.  Every
 * refusal is decided before anything is queued and leaves the state as it was; RC_ESTATE before rcflow_meanflow_open, and with
 * d_flow_xy NULL while no field is resident (RC_ESIZE when the resident field has another size).  RC_EHIP (the runtime refused a
 * launch) is no refusal: the state is undefined until rcflow_meanflow_reset. */
int rcflow_meanflow_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, float* d_mean, size_t mean_step,
                             uint16_t* d_steady, size_t steady_step, float* d_std, size_t std_step, uint8_t* d_mask, size_t mask_step,
                             uint8_t* d_picture, size_t picture_step, rc_meanflow_cell* d_cells, long long* d_sums, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records, the cell sums and the summary
 * of the last push (host memory); zeros before the first. */
int rcflow_meanflow_read(rc_ctx* ctx, int stream, rc_meanflow_cell* cells, long long* sums, long long summary[8]);
/* steady_min, speed_min, min_cos2, dir_x, dir_y and min_fill from the next push on; RC_EINVAL as rcflow_meanflow_open */
int rcflow_meanflow_set(rc_ctx* ctx, int stream, int steady_min, double speed_min, double min_cos2, double dir_x, double dir_y, int min_fill);
/* empties the ring and zeroes the sums, the records, the summary and the push count; keeps the allocation and the parameters as
 * rcflow_meanflow_set left them; asynchronous, on the slot's stream */
int rcflow_meanflow_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_meanflow_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_meanflow_info(rc_ctx* ctx, int stream, rc_meanflow_info* info);

/* ------------------------------------------------------------------ flow check: residual, texture, round trip, valid mask
 * Which vectors of a dense flow field mean anything.  Farneback answers at every pixel: on sky, dry sand, glare and textureless
 * water there is nothing to match, along a straight crest only the normal component is defined, and where foam moves several
 * pixels a frame the match is lost.  Sparse PyrLK returns status and err; this is the dense counterpart.  One launch per push looks
 * at both grey frames and the field (a second, of one workgroup, closes the records) and gives per pixel a set of flags, the mask of the VALID pixels (what
 * rcflow_regions_push_dev takes) and the field with the rejected vectors replaced by NaN or zero: every consumer of a field (the
 * opposing-flow map, the mean flow, the kinematics, the transects) leaves a sample that is not finite out and counts it, so the
 * checked field goes into them as it is.  The reference has no such product.  tests/_flowcheck_ref.py states the following in numpy
 * and the kernel equals it bit for bit on every output of every push.  Every decision is integer and exact; the few float outputs
 * are computed in double, each operation rounded on its own; no atan2 and no float bilinear weight anywhere.
 *
 *  Inputs of a push.  d_next 8UC1, w x h.  d_prev 8UC1, or NULL: the frame the slot holds, which is the d_next of the push before
 *  (every push ends in a device-to-device copy of d_next on the slot's stream, behind the launch).  d_flow_xy 32FC2 from prev to
 *  next with next(x + u) ~ prev(x) (Farneback's convention; pointer and step multiples of 8); NULL is the field the slot's frame
 *  loop left resident (rcflow_stream_flow_ptr), with the rules of rcflow_meanflow_push_dev.  d_back_xy 32FC2 from next to prev, or
 *  NULL: no round-trip test.  The two-image entry point with the frames swapped gives the backward field.
 *  With d_prev NULL and no frame held, the FIRST push since rcflow_flowcheck_open is the copy alone (as the first push of
 *  rcflow_piv_push_dev): no launch, no output written, RC_OK; it counts in `pushes` and not in `computing pushes`.  After
 *  rcflow_flowcheck_reset, which forgets the held frame but not the counts, such a push is RC_ESTATE.
 *  Sample (the mean flow's rule).  A pixel is BAD when a component of u is not finite or fabsf(component) >= 500.0f; otherwise
 *  q = (int)rintf(component * 64.0f) per component: 1/64 pixel, |q| <= 32000.
 *  Target.  X = 64 x + qx, Y = 64 y + qy.  The pixel is OUT when X < 0, Y < 0, X > 64 (w - 1) or Y > 64 (h - 1).  Otherwise
 *  x0 = X >> 6, fx = X & 63, x1 = min(x0 + 1, w - 1), likewise y, and Wn = (64-fx)(64-fy) next[y0,x0] + fx (64-fy) next[y0,x1] +
 *  (64-fx) fy next[y1,x0] + fx fy next[y1,x1], an integer not above 255 * 4096.  A pixel is OK when it is neither BAD nor OUT; then
 *  res = |Wn - 4096 prev[y,x]| and res0 = 4096 |next[y,x] - prev[y,x]|.
 *  Window.  The (2 r + 1)^2 box, r = radius, clipped to the picture: N its pixels inside the picture, Nr those of them that are
 *  OK; R, R0 the sums of res, res0 over the OK ones, each with its own flow (both stay below 2^31); gx = prev[y, min(x+1,w-1)] -
 *  prev[y, max(x-1,0)] and gy likewise (central differences, replicated border); a, c, b the sums of gx^2, gy^2, gx gy over the N
 *  pixels, in int32.
 *  Tests.  rc_flowcheck_params::tests says which of FLAT, RESID, NOGAIN, FB and FAST run; one that is off sets no bit.  BAD and OUT
 *  always run.  A BAD pixel has bit BAD only; an OUT pixel has OUT and whatever FLAT and FAST give.
 *   FLAT    t = tex_min N; the pixel passes iff a + c >= 2 t and (a - t)(c - t) >= b b in int64: the smaller eigenvalue of the mean
 *           structure tensor is at least tex_min, without a square root.
 *   RESID   (OK pixels) res_q = floor(res_max * 4096) taken on the host; set iff R > res_q Nr in int64.
 *   NOGAIN  (OK pixels with q != (0, 0), gain_pm > 0) set iff 1000 R > gain_pm R0: the flow must explain the change between the
 *           frames better than no motion does.
 *   FB      (OK pixels, d_back_xy given) the back field's samples follow the sample rule.  If any of the four back samples at
 *           (x0,y0), (x1,y0), (x0,y1), (x1,y1) is BAD the bit is set.  Otherwise bx = the sum of the same four integer weights
 *           times qbx, in int32, bxr = floor((bx + 2048) / 4096), and by, byr likewise; ex = qx + bxr, ey = qy + byr; e2 = ex^2 +
 *           ey^2, m2 = qx^2 + qy^2 + bxr^2 + byr^2; set iff 1024 e2 > fb_rel_q m2 + fb_abs_q, with fb_rel_q = rint(fb_rel * 1024)
 *           and fb_abs_q = floor(fb_abs * fb_abs * 4194304.0) taken on the host.  fb_rel = 0.01 and fb_abs^2 = 0.5 (fb_abs =
 *           0.70710678) are the usual pair.
 *   FAST    smax_q = floor(speed_max * 64); set iff qx^2 + qy^2 > smax_q^2.
 *  A pixel is VALID iff its flags are 0.
 *  Outputs, each may be NULL.  d_flags 8UC1.  d_mask 8UC1, 255 / 0.  d_checked 32FC2: the input's bits where the pixel is VALID,
 *  else both components 0x7fc00000 (RC_FLOWCHECK_FILL_NAN) or 0.0f (RC_FLOWCHECK_FILL_ZERO).  d_resid 32FC2: ((float)((double)R /
 *  (4096.0 * (double)Nr)), the same from R0), zeros where the pixel is not OK.  d_texture 32FC1, every pixel: with A, B, C the
 *  doubles of a, b, c: l = ((A + C) - sqrt((A - C)(A - C) + 4.0 (B B))) * 0.5, clamped below at 0, and (float)(l / (double)N).
 *  d_picture 8UC3: (g, g, g) with g = prev[y,x] where VALID, else the colour of the lowest set bit, in B, G, R: BAD (255, 0, 255),
 *  OUT (128, 128, 128), FLAT (255, 0, 0), RESID (0, 0, 255), NOGAIN (0, 165, 255), FB (0, 255, 255), FAST (0, 255, 0).
 *  Cells are the opposing-flow map's grid.  RC_FLOWCHECK_SUMS = 10 int64 per cell: the pixels that are VALID | that have BAD | OUT |
 *  FLAT | RESID | NOGAIN | FB | FAST | the sum of qx over the VALID | of qy.  Records, rc_flowcheck_cell, closed by a second, small launch
 *  ("flowcheck@1"): valid_pm = valid * 1000 / pixels; mean_x = (float)(((double)(sum of qx) / 64.0) / (double)valid),
 *  mean_y likewise; both 0 and RC_FLOWCHECK_NONE_VALID set with none valid.  Summary, 10 int64: the eight counts over the picture
 *  | computing pushes | pushes, both since open. */
#define RC_FLOWCHECK_BAD 1               /* the flags of a pixel */
#define RC_FLOWCHECK_OUT 2
#define RC_FLOWCHECK_FLAT 4
#define RC_FLOWCHECK_RESID 8
#define RC_FLOWCHECK_NOGAIN 16
#define RC_FLOWCHECK_FB 32
#define RC_FLOWCHECK_FAST 64
#define RC_FLOWCHECK_TESTS 124           /* what rc_flowcheck_params::tests may hold */
#define RC_FLOWCHECK_FILL_NAN 1          /* rc_flowcheck_params::flags: exactly one of the two */
#define RC_FLOWCHECK_FILL_ZERO 2
#define RC_FLOWCHECK_NONE_VALID 1        /* rc_flowcheck_cell::flags */
#define RC_FLOWCHECK_MAX_RADIUS 7
#define RC_FLOWCHECK_SUMS 10
#define RC_FLOWCHECK_SUMMARY 10
#define RC_FLOWCHECK_LAUNCHES 2          /* of a computing push */
typedef struct rc_flowcheck_params {
    int radius;             /* r: 0..RC_FLOWCHECK_MAX_RADIUS */
    int grid_x, grid_y;     /* cells, as rcflow_ripmap_open */
    int tests;              /* a subset of RC_FLOWCHECK_TESTS */
    int flags;              /* RC_FLOWCHECK_FILL_NAN or RC_FLOWCHECK_FILL_ZERO */
    int tex_min;            /* 0..65025: the least smaller eigenvalue of the mean structure tensor, grey levels squared */
    int gain_pm;            /* 0..1000 per mille; 0: NOGAIN sets nothing */
    int pad;
    double res_max;         /* grey levels, 0..255: the largest window-mean residual */
    double fb_rel;          /* 0..1 */
    double fb_abs;          /* pixels, 0..500 */
    double speed_max;       /* pixels per frame, 0..1000 */
} rc_flowcheck_params;      /* 64 bytes */
typedef struct rc_flowcheck_cell {
    int flags;              /* RC_FLOWCHECK_NONE_VALID */
    int pixels;
    int valid;
    int valid_pm;           /* valid * 1000 / pixels */
    float mean_x, mean_y;   /* of the VALID pixels, pixels per frame */
    int pad[2];
} rc_flowcheck_cell;        /* 32 bytes */
typedef struct rc_flowcheck_info {
    int w, h;
    rc_flowcheck_params prm;           /* as rcflow_flowcheck_set left them */
    int launches_per_push;             /* RC_FLOWCHECK_LAUNCHES */
    int held;                          /* 1 while a frame is held */
    long long pushes, computing;       /* since open */
    size_t device_bytes;
} rc_flowcheck_info;
/* Allocates everything the slot will ever need.  Re-opening replaces the state; a refused open leaves the open state as it was.
 * RC_EINVAL without parameters, for a value outside the ranges above (or not finite), an unknown bit in tests, flags that are not
 * exactly one of the two fills, a grid that does not fit; RC_ESIZE beyond the context's max_w x max_h. */
int rcflow_flowcheck_open(rc_ctx* ctx, int stream, int w, int h, const rc_flowcheck_params* prm);
/* One pair of frames and its field.  Images: d_next, d_prev, d_flags, d_mask 8UC1; d_flow_xy, d_back_xy, d_checked, d_resid 32FC2
 * (pointer and step multiples of 8); d_texture 32FC1 (multiples of 4); d_picture 8UC3; d_cells cells x rc_flowcheck_cell (4-byte
 * aligned), d_sums cells x RC_FLOWCHECK_SUMS int64 and d_summary RC_FLOWCHECK_SUMMARY int64 (8-byte aligned).  What a push gives
 * does not depend on which outputs it asked for.  No host synchronisation, no device-to-host copy.  An output whose byte range
 * overlaps an input's or another output's is RC_EINVAL: d_checked over the field too, because a workgroup reads its neighbours'
 * vectors.  Row padding is never written.  Every refusal is decided before anything is queued and leaves the state as it was;
 * RC_ESTATE before rcflow_flowcheck_open, with d_prev NULL while no frame is held (but see the first push, above), and with
 * d_flow_xy NULL while no field is resident (RC_ESIZE when the resident field has another size).  RC_EHIP (the runtime refused a
 * launch) is no refusal: the state is undefined until rcflow_flowcheck_reset. */
int rcflow_flowcheck_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_next, size_t next_step, const uint8_t* d_prev, size_t prev_step,
                              const float* d_flow_xy, size_t flow_step, const float* d_back_xy, size_t back_step, uint8_t* d_flags,
                              size_t flags_step, uint8_t* d_mask, size_t mask_step, float* d_checked, size_t checked_step, float* d_resid,
                              size_t resid_step, float* d_texture, size_t texture_step, uint8_t* d_picture, size_t picture_step,
                              rc_flowcheck_cell* d_cells, long long* d_sums, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records, the cell sums and the summary
 * of the last computing push (host memory), zeros before the first; the summary's last two words are the counts as they stand. */
int rcflow_flowcheck_read(rc_ctx* ctx, int stream, rc_flowcheck_cell* cells, long long* sums, long long summary[RC_FLOWCHECK_SUMMARY]);
/* tests, tex_min, res_max, gain_pm, fb_rel, fb_abs and speed_max from the next push on; RC_EINVAL as rcflow_flowcheck_open */
int rcflow_flowcheck_set(rc_ctx* ctx, int stream, int tests, int tex_min, double res_max, int gain_pm, double fb_rel, double fb_abs,
                         double speed_max);
/* forgets the held frame and zeroes the records, the sums and the summary's counts of pixels; keeps the allocation, the
 * parameters as rcflow_flowcheck_set left them and the push counts; asynchronous, on the slot's stream */
int rcflow_flowcheck_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_flowcheck_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_flowcheck_info(rc_ctx* ctx, int stream, rc_flowcheck_info* info);

/* ------------------------------------------------------------------ drifters: fates, retention, escape by origin
 * From where on this beach is a swimmer carried out, where does everything else end, and how fast?  A population of up to
 * RC_DRIFTERS_MAX virtual drifters is kept on the device.  Every push moves them through one flow field in exact integers and lets
 * them die by a named fate; dead drifters are released again at their homes on request.  The product keeps the visit density (the
 * reference's population map, as a picture), a census by place and by origin cell, and residence-time histograms: the surf-zone
 * retention and exit rate of field drifter studies.  The reference moves a cloud and draws it (PopulationMap::runLK) and counts
 * nothing.  tests/_drifters_ref.py states the following in numpy and the kernels equal it bit for bit on every output of every push.
 * Integers are exact; sums are integer atomics, so no result depends on the order of addition; the few floats for people are
 * computed in double, each operation rounded on its own.
 *
 *  Field sample (the mean flow's rule, word for word).  d_flow_xy 32FC2, pointer and step multiples of 8; NULL is the field the slot's
 *  frame loop left resident (rcflow_stream_flow_ptr), with the rules of rcflow_meanflow_push_dev.  A pixel is BAD when a component is
 *  not finite or fabsf(component) >= 500.0f; otherwise q = (int)rintf(component * 64.0f) per component.
 *  State, 24 bytes a drifter: home (HX, HY) and position (X, Y), int32 in 1/64 pixel, always inside 0..64 (w-1) x 0..64 (h-1); age,
 *  int32; st, int32: -1 WAITING, 0 ALIVE, f > 0 dead by fate f.  The pixel of a position is ((X + 32) >> 6, (Y + 32) >> 6).
 *  Fates: 1 EDGE_LEFT, 2 EDGE_TOP, 3 EDGE_RIGHT, 4 EDGE_BOTTOM, 5 BAD, 6 AGED, 8 + z ZONE z (z = 1..7); RC_DRIFTERS_SHORE is 9 (zone
 *  1) and RC_DRIFTERS_OFFSHORE 10 (zone 2).  There are 16 slots; 0 and 7 are never used.
 *  One push ("drifters@0"), per drifter, in this order:
 *   1. Release.  A drifter is released when st == -1, or when st > 0 and RC_DRIFTERS_RESPAWN is set: its position becomes its home,
 *      its age 0, and it is counted as released in the summary and in its origin cell; its step is (0, 0), T is its home, and
 *      nothing is sampled.  Without RESPAWN a dead drifter does nothing and is counted nowhere.  A drifter with st == 0 moves.
 *   2. Move.  ix = X >> 6, fx = X & 63, likewise y; the right and lower neighbours are clamped to w - 1, h - 1.  The four weights
 *      (64-fx)(64-fy), fx (64-fy), (64-fx) fy, fx fy sum to 4096.  A corner of weight 0 is not looked at; a corner of weight > 0
 *      that is BAD makes the fate BAD and the position is kept.  Otherwise D = sum of w_i q_i per component (int32), step =
 *      (D * dt_q + 2^19) >> 20 in int64 with an arithmetic shift (floor), dt_q = rint(dt * 256) taken on the host, 1..65536; T =
 *      position + step in int64.
 *   3. Edge, the first that holds: Tx < 0 -> 1; Tx > 64 (w-1) -> 3; Ty < 0 -> 2; Ty > 64 (h-1) -> 4.  The position is kept.
 *   4. Zone, only when no fate is set so far, a drifter just released (at its home) included: z = min(d_zone byte at T's pixel, 7);
 *      z > 0 -> fate 8 + z and the position becomes T.  d_zone (8UC1) NULL means every byte is 0.
 *   5. Age.  A drifter that moved (st was 0; whatever became of it) gets age + 1.  If it has no fate, max_age > 0 and age >= max_age,
 *      the fate is AGED and the position becomes T.
 *   6. Alive.  With no fate the position becomes T and st = 0; the drifter adds 1 to the per-push occupancy word of its pixel, 1 to
 *      the visits of that pixel's by-place cell and its step to that cell's step sums.  Otherwise st = fate, and the death is booked
 *      in the by-place cell of the pixel of the position it ends on, in the by-origin cell of its home's pixel, in the histogram
 *      and in the summary.
 *  Cells are the opposing-flow map's: grid_x x grid_y, the remainder to the last cell, at most RC_RIPMAP_MAX_CELLS.  Both tables are
 *  RC_DRIFTERS_SUMS = 8 int64 a cell, accumulated since open or reset.  Fates fall in four classes: SHORE, OFFSHORE, EDGE (1..4),
 *  other.
 *   By place:  visits | sum of step u | sum of step v | deaths SHORE | OFFSHORE | EDGE | other | sum of age at the OFFSHORE deaths.
 *   By origin: released | deaths SHORE | OFFSHORE | EDGE | other | sum of age at SHORE deaths | at OFFSHORE deaths | 0.
 *  Histograms: 4 classes x RC_DRIFTERS_HIST_BINS = 32 bins of uint64, bin = min(31, age / age_bin), since open or reset.
 *  Summary, RC_DRIFTERS_SUMMARY = 24 int64: drifters | alive after this push | released | pushes since open / reset | sum of age at
 *  SHORE deaths | at OFFSHORE deaths | 0 | 0 | deaths by fate 0..15; all but the first two since open or reset.
 *  Records, rc_drifters_cell, floats for people on which no decision depends, taken in double: RC_DRIFTERS_EMPTY when the cell's
 *  visits and released are both 0; mean_u = (float)(((double)sum of u / 64.0) / (double)visits), mean_v likewise (by place); escape =
 *  (float)((double)OFFSHORE / (double)all deaths), beached likewise with SHORE, mean_exit_age = (float)((double)sum of age at the
 *  OFFSHORE deaths / (double)OFFSHORE) (all three by origin); each 0 when its denominator is 0.
 *  The per-pixel launch ("drifters@1") adds the occupancy plane into the density plane and zeroes it; the density is uint32 state,
 *  exact while drifters x pushes < 2^32.  It also closes the records and the summary.  Outputs, each may be NULL: d_now 16UC1,
 *  min(occupancy, 65535); d_density 32-bit unsigned; d_live 8UC1, 255 where occupancy >= live_min, else 0 (what
 *  rcflow_regions_push_dev takes: where drifters crowd is where foam gathers); d_picture 8UC3, entry min(255, density * 255 /
 *  density_full) of rcflow_jet_lut in uint64, black where the density is 0.  Per drifter, each may be NULL: d_xy 32FC1 n x 2,
 *  (float)X / 64.0f, which is exact; d_age int32; d_state uint8, 0 alive, 255 waiting, else the fate.  Row padding is never written. */
#define RC_DRIFTERS_MAX (1 << 22)
#define RC_DRIFTERS_SUMS 8
#define RC_DRIFTERS_HIST_BINS 32
#define RC_DRIFTERS_SUMMARY 24
#define RC_DRIFTERS_LAUNCHES 2           /* of every push */
#define RC_DRIFTERS_RESPAWN 1            /* rc_drifters_params::flags */
#define RC_DRIFTERS_EMPTY 1              /* rc_drifters_cell::flags */
#define RC_DRIFTERS_EDGE_LEFT 1          /* the fates */
#define RC_DRIFTERS_EDGE_TOP 2
#define RC_DRIFTERS_EDGE_RIGHT 3
#define RC_DRIFTERS_EDGE_BOTTOM 4
#define RC_DRIFTERS_BAD 5
#define RC_DRIFTERS_AGED 6
#define RC_DRIFTERS_ZONE 8               /* + z, z = 1..7 */
#define RC_DRIFTERS_SHORE 9
#define RC_DRIFTERS_OFFSHORE 10
typedef struct rc_drifters_params {
    int max_drifters;       /* 1..RC_DRIFTERS_MAX */
    int grid_x, grid_y;     /* cells, as rcflow_ripmap_open */
    int max_age;            /* >= 0; 0: nobody dies of age */
    int age_bin;            /* >= 1: pushes per histogram bin */
    int density_full;       /* >= 1: the density the picture's last colour stands for */
    int live_min;           /* >= 1 */
    int flags;              /* 0 or RC_DRIFTERS_RESPAWN */
    double dt;              /* fields per push: rint(dt * 256) in 1..65536 */
} rc_drifters_params;       /* 40 bytes */
typedef struct rc_drifters_cell {
    int flags;              /* RC_DRIFTERS_EMPTY */
    int pad0;
    float mean_u, mean_v;   /* by place: the mean step of the visits, pixels per push */
    float escape, beached;  /* by origin: the shares of the deaths that were OFFSHORE, SHORE */
    float mean_exit_age;    /* by origin: pushes from release to an OFFSHORE death */
    int pad1;
} rc_drifters_cell;         /* 32 bytes */
typedef struct rc_drifters_info {
    int w, h;
    rc_drifters_params prm;            /* as rcflow_drifters_set left them */
    int launches_per_push;             /* RC_DRIFTERS_LAUNCHES */
    int drifters;                      /* seeded so far */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_drifters_info;
/* Allocates everything the slot will ever need.  Re-opening replaces the state; a refused open leaves the open state as it was.
 * RC_EINVAL without parameters, for a value outside the ranges above (or a dt that is not finite), a grid that does not fit;
 * RC_ESIZE beyond the context's max_w x max_h. */
int rcflow_drifters_open(rc_ctx* ctx, int stream, int w, int h, const rc_drifters_params* prm);
/* Appends n drifters as WAITING from host points, n x (x, y) doubles in pixels: X = llrint(x * 64.0) taken on the host.  A point
 * that is not finite or lies outside 0..w-1 x 0..h-1 is RC_EINVAL and nothing is added; more than max_drifters in all is RC_ESIZE.
 * Blocks, as rcflow_tracers_add does.  Drifters seeded after pushes are released by the next push. */
int rcflow_drifters_seed(rc_ctx* ctx, int stream, const double* xy, int n);
/* One field.  d_zone 8UC1 or NULL; d_now 16UC1 (pointer and step multiples of 2), d_density 32-bit (multiples of 4), d_live 8UC1,
 * d_picture 8UC3; d_xy n x 2 floats (8-byte aligned), d_age n int32, d_state n bytes, n the drifters seeded; d_cells cells x
 * rc_drifters_cell (4-byte aligned), d_place and d_origin cells x RC_DRIFTERS_SUMS int64, d_hist 4 x RC_DRIFTERS_HIST_BINS uint64 and
 * d_summary RC_DRIFTERS_SUMMARY int64 (8-byte aligned).  What a push does to the state does not depend on which outputs it asked
 * for.  No host synchronisation, no device-to-host copy.  An output whose byte range overlaps an input's or another output's is
 * RC_EINVAL.  Every refusal is decided before anything is queued and leaves the state as it was; RC_ESTATE before
 * rcflow_drifters_open, with no drifter seeded, and with d_flow_xy NULL while no field is resident (RC_ESIZE when the resident
 * field has another size).  RC_EHIP (the runtime refused a launch) is no refusal: the state is undefined until
 * rcflow_drifters_reset. */
int rcflow_drifters_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, const uint8_t* d_zone, size_t zone_step,
                             uint16_t* d_now, size_t now_step, uint32_t* d_density, size_t density_step, uint8_t* d_live, size_t live_step,
                             uint8_t* d_picture, size_t picture_step, float* d_xy, int32_t* d_age, uint8_t* d_state, rc_drifters_cell* d_cells,
                             long long* d_place, long long* d_origin, unsigned long long* d_hist, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL (host memory): the records and the summary of
 * the last push, zeros before the first; both tables and the histograms as they stand. */
int rcflow_drifters_read(rc_ctx* ctx, int stream, rc_drifters_cell* cells, long long* place, long long* origin, unsigned long long* hist,
                         long long summary[RC_DRIFTERS_SUMMARY]);
/* dt, max_age, density_full, live_min and flags (the RESPAWN bit) from the next push on; RC_EINVAL as rcflow_drifters_open */
int rcflow_drifters_set(rc_ctx* ctx, int stream, double dt, int max_age, int density_full, int live_min, int flags);
/* every drifter goes to WAITING at its home with age 0; tables, histograms, density, the last push's records and summary and the
 * push count go to zero; keeps the allocation, the drifters and the parameters as rcflow_drifters_set left them; asynchronous, on
 * the slot's stream */
int rcflow_drifters_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_drifters_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_drifters_info(rc_ctx* ctx, int stream, rc_drifters_info* info);
/* The zones helper ("drifters@2"), stateless and one launch: the shoreline's wet mask and the surf zone's mask into the byte map a
 * push takes, without a host round trip.  A pixel with a zero d_wet byte is zone 1 (SHORE); otherwise a pixel with a zero d_inside
 * byte is zone 2 (OFFSHORE); otherwise 0.  All three 8UC1, w x h.  Either input may be NULL (no such zone), not both (RC_EINVAL);
 * d_zone may overlap neither. */
int rcflow_drifters_zones_dev(rc_ctx* ctx, int stream, const uint8_t* d_wet, size_t wet_step, const uint8_t* d_inside, size_t inside_step, int w,
                              int h, uint8_t* d_zone, size_t zone_step);

/* ------------------------------------------------------------------ flow infill: holes of a checked field filled from a pyramid
 * The flow check hands on a field with the rejected vectors replaced by NaN.  The mean flow, the opposing-flow map, the kinematics
 * and the transects leave such a sample out; the Lagrangian products cannot: the flow map's particle stops for good at a rejected
 * sample, a drifter dies BAD, the plan view resamples the NaN.  This is the "replace" that closes every PIV validation: the rejected
 * vectors are interpolated from their valid neighbours, by pull-push over a pyramid of block sums, O(pixels) whatever the size of
 * the holes, and a byte per pixel says how far the value was fetched from, so that nobody mistakes an interpolated vector for a
 * measured one.  A vector the caller had an answer for is never changed.  The reference has no such product.
 * tests/_infill_ref.py states the following in numpy and the kernels equal it bit for bit on every output of every push.  Every
 * decision and every output value is an exact integer in 1/64 pixel; the only floats produced are (float)F / 64.0f with |F| <= 32000,
 * which are exact, and the records' means, taken in double, each operation rounded on its own.
 *
 *  Inputs of a push.  d_flow_xy 32FC2 (pointer and step multiples of 8); NULL is the field the slot's frame loop left resident
 *  (rcflow_stream_flow_ptr), with the rules of rcflow_meanflow_push_dev.  d_valid 8UC1 or NULL: what rcflow_flowcheck_push_dev
 *  writes as d_mask.  d_domain 8UC1 or NULL: where a value is wanted, the shoreline's wet mask or a region of interest.
 *  Sizes.  w_0 = w, h_0 = h, w_(l+1) = (w_l + 1) >> 1 and h likewise; a level may shrink to 1 x 1 and stay there.  L = levels.
 *  1. Classes, per pixel (the mean flow's sample rule).  The pixel is BAD when a component is not finite or fabsf(component) >=
 *     500.0f; otherwise q = (int)rintf(component * 64.0f) per component.  It is KNOWN iff it is not BAD and (d_valid is NULL or its
 *     byte != 0).  With hold > 0 there is a state per pixel, a held q and an age byte, 255 (nothing held) after open and reset: a
 *     KNOWN pixel stores (q, 0); a pixel that is not KNOWN with age < hold is HELD, its value the held q, and its age becomes
 *     age + 1; any other pixel is a HOLE and its age becomes 255.  With hold = 0 a pixel is KNOWN or a HOLE.  The state does not look
 *     at d_domain, nor at which outputs a push asks for.
 *  2. Pull.  S_0 = (qx, qy, 1) at KNOWN and HELD pixels, (0, 0, 0) at holes.  S_(l+1)[Y, X] = the sum of S_l over rows 2Y, 2Y + 1
 *     and columns 2X, 2X + 1 that lie inside level l, l = 0..L-1, in int32: |SX| <= 4^7 * 32000 < 2^30.
 *  3. Push.  rdiv(a, b) = floor((2 a + b) / (2 b)), b > 0, the floor towards minus infinity.  A cell of level l >= 1 is OWN iff
 *     N_l >= min_known; at level 0 OWN means KNOWN or HELD.  Level L: a cell has a value iff it is OWN; then F = (rdiv(SX, N),
 *     rdiv(SY, N)) and lev = L.  Level l < L, from L - 1 down to 0: an OWN cell has F = its own mean (its q at level 0) and lev = l.
 *     Any other cell (x, y) looks at four entries of level l + 1: X0 = x >> 1, X1 = clamp(X0 + (x & 1 ? 1 : -1), 0, w_(l+1) - 1),
 *     Y0 and Y1 likewise; (Y0, X0), (Y0, X1), (Y1, X0), (Y1, X1) weigh 9, 3, 3, 1, each counted also where the clamp makes two of
 *     them one cell.  A = the weights of the entries that have a value.  A = 0: the cell has none.  Otherwise F = rdiv(sum of
 *     weight * F_entry, A) per component in int32 and lev = the largest lev among those entries: the coarsest level that
 *     contributed.
 *  4. Outputs, each may be NULL.  A pixel is WANTED iff d_domain is NULL or its byte != 0.  The pattern is both components
 *     0x7fc00000 (RC_INFILL_LEAVE_NAN) or 0.0f (RC_INFILL_LEAVE_ZERO).  By the first class that holds:
 *       KNOWN          d_source 0                       d_filled the input's bits, unchanged
 *       not WANTED     RC_INFILL_OUTSIDE 254            the pattern
 *       HELD           RC_INFILL_HELD 64                (float)q_held / 64.0f
 *       has a value    lev, 1..7                        (float)F / 64.0f
 *       else           RC_INFILL_UNFILLED 255           the pattern
 *     d_mask 8UC1: 255 where d_source <= 64, else 0 (what rcflow_regions_push_dev takes).  d_picture 8UC3 in B, G, R: KNOWN (64, 64,
 *     64), HELD (255, 255, 255), lev l entry l * 255 / 7 of rcflow_jet_lut, UNFILLED (255, 0, 255), OUTSIDE (0, 0, 0).
 *  5. Cells are the opposing-flow map's grid.  RC_INFILL_SUMS = 8 int64 per cell, the counts by the source byte: KNOWN | HELD |
 *     FILLED (1..7) | UNFILLED | OUTSIDE | the sum of Fx over the pixels with a value (source <= 64; q for KNOWN and HELD) | of Fy |
 *     the sum of lev over FILLED.  Records, rc_infill_cell, closed by a last, small launch: known_pm = KNOWN * 1000 / pixels,
 *     valued_pm = (KNOWN + HELD + FILLED) * 1000 / pixels, mean_x = (float)(((double)(sum of Fx) / 64.0) / (double)valued), mean_y
 *     likewise, mean_level = (float)((double)(sum of lev) / (double)FILLED); each float is 0 when its denominator is 0, and
 *     RC_INFILL_NONE is set when no pixel of the cell has a value.  Summary, RC_INFILL_SUMMARY = 16 int64: the five counts over the
 *     picture | pushes since open / reset | 0 | 0 | the FILLED pixels by lev 0..7 (the first is always 0). */
#define RC_INFILL_LEAVE_NAN 1            /* rc_infill_params::flags: exactly one of the two */
#define RC_INFILL_LEAVE_ZERO 2
#define RC_INFILL_HELD 64                /* d_source; 0 is KNOWN, 1..7 the level a value came from */
#define RC_INFILL_OUTSIDE 254
#define RC_INFILL_UNFILLED 255
#define RC_INFILL_NONE 1                 /* rc_infill_cell::flags */
#define RC_INFILL_MAX_LEVELS 7
#define RC_INFILL_MAX_MIN_KNOWN 16384
#define RC_INFILL_MAX_HOLD 254
#define RC_INFILL_SUMS 8
#define RC_INFILL_SUMMARY 16
#define RC_INFILL_LAUNCHES 4             /* of a push with levels >= 5; one fewer below: "infill@1" has nothing to do */
typedef struct rc_infill_params {
    int levels;             /* L: 1..RC_INFILL_MAX_LEVELS */
    int min_known;          /* 1..RC_INFILL_MAX_MIN_KNOWN: the KNOWN and HELD pixels a cell of level >= 1 needs to take its own mean */
    int hold;               /* 0..RC_INFILL_MAX_HOLD pushes a pixel keeps its last KNOWN vector; fixed at open */
    int grid_x, grid_y;     /* cells, as rcflow_ripmap_open */
    int flags;              /* RC_INFILL_LEAVE_NAN or RC_INFILL_LEAVE_ZERO */
    int pad[6];             /* zero */
} rc_infill_params;         /* 48 bytes */
typedef struct rc_infill_cell {
    int flags;              /* RC_INFILL_NONE */
    int pixels;
    int known_pm;           /* KNOWN * 1000 / pixels */
    int valued_pm;          /* (KNOWN + HELD + FILLED) * 1000 / pixels */
    float mean_x, mean_y;   /* of the pixels with a value, pixels per frame */
    float mean_level;       /* of the FILLED pixels */
    int pad;
} rc_infill_cell;           /* 32 bytes */
typedef struct rc_infill_info {
    int w, h;
    rc_infill_params prm;              /* as rcflow_infill_set left them */
    int launches_per_push;             /* RC_INFILL_LAUNCHES with levels >= 5, one fewer below */
    int pad;
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_infill_info;
/* Allocates everything the slot will ever need, for every value rcflow_infill_set may give.  Re-opening replaces the state; a
 * refused open leaves the open state as it was.  RC_EINVAL without parameters, for a value outside the ranges above, flags that are
 * not exactly one of the two, a pad word that is not zero, a grid that does not fit; RC_ESIZE beyond the context's max_w x max_h. */
int rcflow_infill_open(rc_ctx* ctx, int stream, int w, int h, const rc_infill_params* prm);
/* One field.  Images: d_valid, d_domain, d_source, d_mask 8UC1; d_flow_xy, d_filled 32FC2 (pointer and step multiples of 8);
 * d_picture 8UC3; d_cells cells x rc_infill_cell (4-byte aligned), d_sums cells x RC_INFILL_SUMS int64 and d_summary
 * RC_INFILL_SUMMARY int64 (8-byte aligned).  What a push gives and what it does to the held state do not depend on which outputs
 * it asked for.  No host synchronisation, no device-to-host copy.  An output whose byte range overlaps an input's or another
 * output's is RC_EINVAL, d_filled over the field too: filling in place is not part of this product.  Row padding is never written.
 * Every refusal is decided before anything is queued and leaves state and outputs as they were; RC_ESTATE before
 * rcflow_infill_open and with d_flow_xy NULL while no field is resident (RC_ESIZE when the resident field has another size).
 * RC_EHIP (the runtime refused a launch) is no refusal: the state is undefined until rcflow_infill_reset. */
int rcflow_infill_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, const uint8_t* d_valid, size_t valid_step,
                           const uint8_t* d_domain, size_t domain_step, float* d_filled, size_t filled_step, uint8_t* d_source,
                           size_t source_step, uint8_t* d_mask, size_t mask_step, uint8_t* d_picture, size_t picture_step,
                           rc_infill_cell* d_cells, long long* d_sums, long long* d_summary);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records, the cell sums and the summary
 * of the last push (host memory), zeros before the first and after a reset. */
int rcflow_infill_read(rc_ctx* ctx, int stream, rc_infill_cell* cells, long long* sums, long long summary[RC_INFILL_SUMMARY]);
/* levels, min_known and flags from the next push on; RC_EINVAL as rcflow_infill_open.  hold is fixed at open */
int rcflow_infill_set(rc_ctx* ctx, int stream, int levels, int min_known, int flags);
/* forgets the held state and zeroes the records, the sums, the summary and the push count; keeps the allocation and the parameters
 * as rcflow_infill_set left them; asynchronous, on the slot's stream */
int rcflow_infill_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_infill_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_infill_info(rc_ctx* ctx, int stream, rc_infill_info* info);

/* ------------------------------------------------------------------ offshore frame: exact distance to shore, cross / along flow
 * The shoreline gives a wet mask, the flow products give a field; this joins them.  For every pixel the exact Euclidean distance to
 * the shore and the shore point it is nearest to (the map, made when the shore has moved), and per push the field projected on the
 * local shore normal: how fast the water runs away from the shore, how far out, and at which place along the beach, also on a curved
 * beach or behind a headland, where one direction for the whole picture is wrong.  The reference has no such product.
 * tests/_offshore_ref.py states the following in numpy and the kernels equal it bit for bit on every output of every call.  Every
 * decision and every stored value is an exact integer; the only floats produced are (float)v / 64.0f with |v| < 2^24, which are
 * exact, and the records' means, taken in double, each operation rounded on its own.
 *
 *  1. The map (rcflow_offshore_map_dev).  d_wet 8UC1, non-zero is water: what rcflow_shoreline_push_dev writes as its wet mask.  A
 *     pixel's class is wet or dry.  For a pixel p = (x, y) the candidates are the pixels of the OTHER class; d2(p) = the least
 *     (x - x')^2 + (y - y')^2 over them, int32; near(p) = the raster index y' * w + x' of the candidate that attains it, the smallest
 *     index when several do.  With no pixel of the other class in the picture d2 = RC_OFFSHORE_FAR and near = -1.  Exact and
 *     uncapped: no chamfer, no search radius.  r = floor(sqrt(4096 * d2)) taken exactly in int64: the distance in 1/64 pixel.  Both
 *     planes stay in the slot's state until the next map or a reset.  Outputs, each may be NULL:
 *       d_dist2 32SC1    d2, negated on dry pixels; FAR stays +-0x7fffffff
 *       d_near 32SC1     near
 *       d_sdist 32SC1    r, negated on dry pixels; FAR stays +-0x7fffffff
 *       d_picture 8UC3   B, G, R by the first rule that holds: FAR (0, 0, 0); dry (64, 64, 64); wet entry
 *                        min(r / 64, max_dist) * 255 / max_dist of rcflow_jet_lut, in integers, max_dist as it stands at the call
 *     Map summary, RC_OFFSHORE_SUMMARY = 8 int64: wet pixels | dry pixels | wet pixels that are not FAR | the largest d2 over those |
 *     the sum of d2 over those | the sum of d2 over the dry pixels that are not FAR | 0 | maps since open / reset.
 *  2. The push (rcflow_offshore_push_dev), one flow field on the slot's map.  Each pixel takes the first class that holds:
 *       RC_OFFSHORE_C_DRY 3    the pixel is dry
 *       RC_OFFSHORE_C_FAR 2    d2 is FAR or d2 > max_dist^2
 *       RC_OFFSHORE_C_NEAR 1   d2 < min_dist^2
 *       RC_OFFSHORE_C_BAD 4    the mean current's sample rule: a component is not finite or fabsf(component) >= 500.0f
 *       RC_OFFSHORE_C_OK 0     otherwise
 *     At an OK pixel q = (int)rintf(component * 64.0f) per component and n = (x - near % w, y - near / w): the vector from the
 *     nearest shore point to the pixel, |n|^2 = d2.  C = qx nx + qy ny and A = -qx ny + qy nx fit int32 because max_dist <= 4095.
 *     rdiv(a, b) = floor((2 a + b) / (2 b)), b > 0, the floor towards minus infinity, in int64.  cross = rdiv(64 C, r) and along =
 *     rdiv(64 A, r), in 1/64 pixel per field.  Positive cross is away from the shore.  Along is the component on the normal turned
 *     by a quarter from +x towards +y: with the land at the top of the picture (n = (0, 1)) positive along runs towards -x.
 *     Outputs, each may be NULL:
 *       d_cross_along 32FC2   ((float)cross / 64.0f, (float)along / 64.0f); 0x7fc00000 in both components at every pixel not OK
 *       d_class 8UC1          the class
 *       d_mask 8UC1           255 where the pixel is OK and cross >= cmin_q, cmin_q = (int)ceil((double)cross_min * 64.0) taken on
 *                             the host; 0 elsewhere.  What rcflow_regions_push_dev takes
 *       d_picture 8UC3        OK: with S = max(4 cmin_q, 1), c = clamp(cross, -S, S) and m = |c| * 255 / S in integers, B, G, R =
 *                             (255 - m, 255 - m, 255) for c >= 0 (white to red: seaward) and (255, 255 - m, 255 - m) for c < 0
 *                             (white to blue: shoreward); DRY (64, 64, 64), FAR (0, 0, 0), NEAR (128, 128, 128), BAD (255, 0, 255)
 *  3. The table, stations x bins cells of RC_OFFSHORE_SUMS = 4 int64, station-major: count | sum of cross | sum of along | mask
 *     pixels.  An OK pixel's bin is r / (64 * bin_width); its station x * stations / w with RC_OFFSHORE_STATION_X, y * stations / h
 *     with RC_OFFSHORE_STATION_Y (the nearest point's own coordinate was tried as the station and dropped: on a cuspate shore the
 *     few protruding points collect every far pixel).  An OK pixel whose bin is >= bins is counted per station as "beyond" and
 *     enters no cell.
 *  4. Records, rc_offshore_station, one per station, closed by a last, small launch.  first = the lowest bin with count >=
 *     min_count; when there is none RC_OFFSHORE_EMPTY is set and every number but `beyond` is 0.  From first outwards a bin PASSES
 *     when count >= min_count and sum of cross >= cmin_q * count.  reach_end = one past the last bin of the unbroken run of passing
 *     bins that starts at first, 0 when first itself fails.  peak_bin = the passing bin (inside the run or beyond a break) with the
 *     largest rdiv(sum of cross, count), the lowest such bin, -1 when no bin passes; peak_cross is that value.  count, mean_cross
 *     = (float)(((double)(sum of cross over the run) / 64.0) / (double)(count over the run)) and mean_along likewise are of the run's
 *     bins, 0 with an empty run.  RC_OFFSHORE_RIP is set when reach_end - first >= rip_bins.
 *     Push summary, 8 int64: the pixels by class 0..4 (OK, NEAR, FAR, DRY, BAD) | mask pixels | stations flagged RIP | pushes since
 *     open / reset.
 *  5. The band (rcflow_offshore_band_dev), one launch on the slot's map: 255 where the pixel is wet, not FAR and
 *     (int)ceil((double)lo * 64.0) <= r < (int)ceil((double)hi * 64.0), 0 elsewhere.  The "inside" mask of
 *     rcflow_drifters_zones_dev, a d_domain for rcflow_infill_push_dev. */
#define RC_OFFSHORE_FAR 0x7fffffff       /* d2 and r where the picture has no pixel of the other class */
#define RC_OFFSHORE_STATION_X 1          /* rc_offshore_params::flags: exactly one of the two */
#define RC_OFFSHORE_STATION_Y 2
#define RC_OFFSHORE_C_OK 0               /* d_class */
#define RC_OFFSHORE_C_NEAR 1
#define RC_OFFSHORE_C_FAR 2
#define RC_OFFSHORE_C_DRY 3
#define RC_OFFSHORE_C_BAD 4
#define RC_OFFSHORE_EMPTY 1              /* rc_offshore_station::flags */
#define RC_OFFSHORE_RIP 2
#define RC_OFFSHORE_MAX_DIST 4095
#define RC_OFFSHORE_MAX_STATIONS 256
#define RC_OFFSHORE_MAX_BINS 256
#define RC_OFFSHORE_MAX_BIN_WIDTH 256
#define RC_OFFSHORE_MAX_SIDE 32767       /* of the picture: d2 and the raster index are int32 */
#define RC_OFFSHORE_SUMS 4
#define RC_OFFSHORE_SUMMARY 8
#define RC_OFFSHORE_MAP_LAUNCHES 3
#define RC_OFFSHORE_PUSH_LAUNCHES 2
typedef struct rc_offshore_params {
    int min_dist;           /* 0..max_dist, pixels: nearer pixels are NEAR (swash, the waterline's own error) */
    int max_dist;           /* 1..RC_OFFSHORE_MAX_DIST, pixels: farther pixels are FAR */
    int stations;           /* 1..RC_OFFSHORE_MAX_STATIONS along the beach; fixed at open */
    int bins;               /* 1..RC_OFFSHORE_MAX_BINS of distance; fixed at open */
    int bin_width;          /* 1..RC_OFFSHORE_MAX_BIN_WIDTH pixels */
    int min_count;          /* >= 1: the OK pixels a bin needs to count */
    int rip_bins;           /* 1..bins: the passing bins in a row that make a station a rip */
    float cross_min;        /* finite, 0..400 pixels per field: the mean cross flow a bin needs to pass, the cross flow of the mask */
    int flags;              /* RC_OFFSHORE_STATION_X or RC_OFFSHORE_STATION_Y */
    int pad[3];             /* zero */
} rc_offshore_params;       /* 48 bytes */
typedef struct rc_offshore_station {
    int flags;              /* RC_OFFSHORE_EMPTY, RC_OFFSHORE_RIP */
    int first;              /* the lowest bin with count >= min_count */
    int reach_end;          /* one past the run of passing bins from first; reach_end * bin_width pixels is the rip's reach */
    int peak_bin;           /* -1: no bin passes */
    int peak_cross;         /* rdiv(sum of cross, count) of peak_bin, 1/64 pixel per field */
    int count;              /* OK pixels of the run's bins */
    int beyond;             /* OK pixels of the station past the last bin */
    int pad0;
    float mean_cross, mean_along;   /* of the run, pixels per field */
    int pad1[2];
} rc_offshore_station;      /* 48 bytes */
typedef struct rc_offshore_info {
    int w, h;
    rc_offshore_params prm;            /* as rcflow_offshore_set left them */
    int launches_per_map;              /* RC_OFFSHORE_MAP_LAUNCHES */
    int launches_per_push;             /* RC_OFFSHORE_PUSH_LAUNCHES */
    int have_map;                      /* 1 after a map, 0 after open and reset */
    int pad;
    long long maps, pushes;            /* since open / reset */
    size_t device_bytes;
} rc_offshore_info;
/* Allocates everything the slot will ever need, for every value rcflow_offshore_set may give.  Re-opening replaces the state; a
 * refused open leaves the open state as it was.  RC_EINVAL without parameters, for a value outside the ranges above, flags that are
 * not exactly one of the two, a pad word that is not zero; RC_ESIZE beyond the context's max_w x max_h or RC_OFFSHORE_MAX_SIDE. */
int rcflow_offshore_open(rc_ctx* ctx, int stream, int w, int h, const rc_offshore_params* prm);
/* Called when the shore has moved, not every push: RC_OFFSHORE_MAP_LAUNCHES launches.  d_wet 8UC1; d_dist2, d_near, d_sdist 32SC1
 * (pointer and step multiples of 4); d_picture 8UC3; d_summary RC_OFFSHORE_SUMMARY int64 (8-byte aligned).  What a call gives does
 * not depend on which outputs it asked for.  No host synchronisation, no device-to-host copy.  An output whose byte range overlaps
 * the input's or another output's is RC_EINVAL.  Row padding is never written.  Every refusal is decided before anything is queued
 * and leaves state and outputs as they were; RC_ESTATE before rcflow_offshore_open.  RC_EHIP (the runtime refused a launch) is no
 * refusal: the state is undefined until rcflow_offshore_reset. */
int rcflow_offshore_map_dev(rc_ctx* ctx, int stream, const uint8_t* d_wet, size_t wet_step, int* d_dist2, size_t dist2_step, int* d_near,
                            size_t near_step, int* d_sdist, size_t sdist_step, uint8_t* d_picture, size_t picture_step, long long* d_summary);
/* One field: RC_OFFSHORE_PUSH_LAUNCHES launches.  d_flow_xy 32FC2 (pointer and step multiples of 8); NULL is the field the slot's
 * frame loop left resident (rcflow_stream_flow_ptr), with the rules of rcflow_meanflow_push_dev: RC_ESTATE while none is resident,
 * RC_ESIZE when its size differs.  d_cross_along 32FC2; d_class, d_mask 8UC1; d_picture 8UC3; d_stations stations x
 * rc_offshore_station (4-byte aligned); d_table stations x bins x RC_OFFSHORE_SUMS int64 and d_summary RC_OFFSHORE_SUMMARY int64
 * (8-byte aligned).  RC_ESTATE before any map (after open and after a reset).  Otherwise the rules of rcflow_offshore_map_dev. */
int rcflow_offshore_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, float* d_cross_along, size_t cross_along_step,
                             uint8_t* d_class, size_t class_step, uint8_t* d_mask, size_t mask_step, uint8_t* d_picture, size_t picture_step,
                             rc_offshore_station* d_stations, long long* d_table, long long* d_summary);
/* One launch on the slot's map: d_band 8UC1, required.  lo and hi in pixels, finite, 0 <= lo <= hi <= 65536 (RC_EINVAL otherwise).
 * RC_ESTATE before any map.  Changes nothing of the state. */
int rcflow_offshore_band_dev(rc_ctx* ctx, int stream, float lo, float hi, uint8_t* d_band, size_t band_step);
/* Blocks until the slot's stream has finished; for hosts and tests.  Each may be NULL: the records and the table of the last push,
 * the summary of the last push and of the last map (host memory), zeros before the first and after a reset. */
int rcflow_offshore_read(rc_ctx* ctx, int stream, rc_offshore_station* stations, long long* table, long long push_summary[RC_OFFSHORE_SUMMARY],
                         long long map_summary[RC_OFFSHORE_SUMMARY]);
/* everything but stations and bins, which must be the values given at open, from the next call on; RC_EINVAL as rcflow_offshore_open */
int rcflow_offshore_set(rc_ctx* ctx, int stream, const rc_offshore_params* prm);
/* forgets the map and zeroes the records, the table, the summaries and the counts; keeps the allocation and the parameters as
 * rcflow_offshore_set left them; asynchronous, on the slot's stream */
int rcflow_offshore_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_offshore_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_offshore_info(rc_ctx* ctx, int stream, rc_offshore_info* info);

/* ------------------------------------------------------------------ region outlines: boundaries traced into ordered polygons
 * Every product above that ends in a mask (the regions' and the tracks' label planes, the shoreline's wet mask, the surf-zone mask,
 * the offshore band, the vortex cores, the FTLE ridges) can be handed on as a shape: the boundary of every region as an ordered
 * polygon of lattice corners, holes told apart from outer boundaries, with perimeter and signed area.  Everything is an integer and
 * does not depend on the order in which the device arrives at it; tests/_outlines_ref.py states it by a sequential walk.
 *
 *  1. Input.  Exactly one of d_labels (32SC1: the label plane of rcflow_regions_push_dev, the footprint of the tracks; pointer and
 *     step multiples of 4) and d_mask (8UC1: a non-zero byte is label 1).  A pixel with label 0 belongs to nothing.  A side of the
 *     picture is at most RC_OUTLINES_MAX_SIDE, so that a corner stays within RC_DRAW_COORD_MAX and a crack's key within int32.
 *  2. Cracks.  A crack is one side of a pixel, directed.  Pixel P = (x, y) with label L != 0 has the sides s = 0 N, 1 E, 2 S, 3 W;
 *     side s is a crack when the 4-neighbour across it lies outside the picture or has a label other than L (another non-zero label
 *     counts like background).  A crack runs with P on its right, y down: N (x, y) -> (x+1, y); E (x+1, y) -> (x+1, y+1);
 *     S (x+1, y+1) -> (x, y+1); W (x, y+1) -> (x, y).  Its key is (y * w + x) * 4 + s.
 *  3. Successor.  For side s: d the crack's direction, (1,0), (0,1), (-1,0), (0,-1); a the step across it, (0,-1), (1,0), (0,1),
 *     (-1,0); R = P + d; Lp = P + d + a; same(X): X is inside the picture and has label L.  Connectivity 8 takes the first that
 *     holds of: same(Lp): turn left, to (Lp, (s+3)%4); same(R): straight on, to (R, s); else turn right, to (P, (s+1)%4).
 *     Connectivity 4 takes the first that holds of: not same(R): turn right; same(Lp): turn left; else straight on.  The successor is
 *     a permutation of the cracks, which therefore fall into disjoint closed loops.
 *  4. Loops.  A loop's leader is its crack with the smallest key; a crack's rank is its number of steps from the leader; loops are
 *     numbered in increasing order of their leader's key.  cracks: the loop's length, the perimeter in pixel sides.  area2: the sum
 *     over its cracks of x0 * y1 - x1 * y0 from (x0, y0) to (x1, y1), twice the signed area, positive for an outer boundary and
 *     negative for a hole.  A turn crack is one whose successor has another side; vertex j of a loop is the second corner of its
 *     j-th turn crack in rank order; verts is their number, always even and at least 4.  The box x0, y0, x1, y1 is the inclusive box
 *     of the loop's corners.
 *  5. Filter and caps.  Loops with cracks < min_cracks are dropped and the rest renumbered in order (min_cracks <= 4 keeps all).
 *     The first min(kept, max_loops) get a record.  Vertex offsets are the running sum of verts over the kept loops in order; a
 *     loop is stored whole when offset + verts <= max_vertices, otherwise its offset is -1, RC_OUTLINE_NOVERTS is set and none of
 *     its vertices is written.  A picture with more cracks than max_cracks gives no loops: records and vertices are zero bytes, the
 *     summary carries the true crack count and the overflow word, and the host re-opens larger.  Nothing is truncated silently and
 *     nothing is written past a cap.
 *  6. Outputs.  d_loops: max_loops records, zero bytes beyond the written ones.  d_verts: max_vertices pairs (x, y) of int32, lattice
 *     corners in 0..w and 0..h, zero beyond the written ones.  d_summary, RC_OUTLINES_SUMMARY int64: 0 the cracks of the picture (true
 *     also on overflow), 1 the loops before the filter, 2 the loops kept, 3 the records written, 4 the vertices of the kept loops,
 *     5 the vertices written, 6 1 when the cracks overflowed, else 0, 7 the pushes since open or reset.
 *  7. Primitives.  rcflow_outlines_prims_dev gives max_vertices records of rc_draw_prim from the last push: stored vertex i of a loop
 *     gives a line of `thickness` and `color` from it to the loop's next vertex, the last one to the first, every coordinate
 *     min(x, w - 1), min(y, h - 1); every other slot is an all-zero record, which rcflow_draw_dev skips AND COUNTS, as it does with
 *     the regions' primitives.  The count is fixed, so the host never reads the device to know it.
 *
 * A push is RC_OUTLINES_FIXED_LAUNCHES + 2 * rounds launches, rounds = ceil(log2(max_cracks)), whatever the picture holds
 * ("outlines@0".."outlines@10", launches that belong together under one name; the primitives are "outlines@11"): the sides and their
 * count per block of pixels, and a scan of the block counts; the cracks compacted in key order with their successor's key; the
 * successor's place in that list; `rounds` rounds of pointer doubling that carry the smallest key of the window, each its own launch
 * from one buffer pair into the other, after which every crack knows its loop's leader; every loop cut before its leader; `rounds`
 * rounds of list ranking; the loops numbered; the cracks scattered to loop order; area, box and turns added per loop; the turns
 * scanned into vertex places and the vertices written; the records closed.  A round that finds that the round before it changed
 * nothing returns at once; the launch count stays what rcflow_outlines_info says.
 * Simplifying a polygon (Douglas-Peucker) is left to the host, which does it on a few thousand vertices in microseconds. */
#define RC_OUTLINES_MAX_SIDE 16383
#define RC_OUTLINES_MAX_CRACKS (1 << 25)     /* 36 bytes of state a crack */
#define RC_OUTLINES_MAX_LOOPS (1 << 20)
#define RC_OUTLINES_MAX_VERTICES (1 << 24)   /* RC_DRAW_MAX_PRIMS: the primitives of one call to rcflow_draw_dev */
#define RC_OUTLINES_SUMMARY 8
#define RC_OUTLINES_FIXED_LAUNCHES 13
#define RC_OUTLINE_HOLE 1                    /* rc_outline_loop::flags: area2 < 0 */
#define RC_OUTLINE_NOVERTS 2                 /* the loop's vertices did not fit max_vertices: offset -1, none written */
typedef struct rc_outlines_params {
    int connectivity;       /* 4 or 8 */
    int min_cracks;         /* >= 1: shorter loops are dropped */
    int max_cracks;         /* 4..RC_OUTLINES_MAX_CRACKS: the cracks of a picture the slot has room for */
    int max_loops;          /* 1..RC_OUTLINES_MAX_LOOPS: the records */
    int max_vertices;       /* 4..RC_OUTLINES_MAX_VERTICES: the vertices, and the primitives of rcflow_outlines_prims_dev */
    int flags;              /* 0 */
    int pad[2];             /* zero */
} rc_outlines_params;       /* 32 bytes */
typedef struct rc_outline_loop {
    int32_t label;
    int32_t flags;          /* RC_OUTLINE_HOLE, RC_OUTLINE_NOVERTS */
    int32_t x, y;           /* the leader's pixel: of an outer boundary the first pixel of the region in raster order */
    int32_t cracks;         /* the perimeter in pixel sides */
    int32_t verts;
    int32_t offset;         /* of the loop's first vertex in d_verts, in vertices; -1 with RC_OUTLINE_NOVERTS */
    int32_t pad;
    int32_t x0, y0, x1, y1; /* the inclusive box of the corners */
    long long area2;        /* twice the signed area */
} rc_outline_loop;          /* 56 bytes, 8-byte aligned */
typedef struct rc_outlines_info {
    int w, h;
    rc_outlines_params prm;            /* min_cracks as rcflow_outlines_set left it */
    int rounds;                        /* ceil(log2(max_cracks)) */
    int launches_per_push;             /* RC_OUTLINES_FIXED_LAUNCHES + 2 * rounds */
    long long pushes;                  /* since open / reset */
    size_t device_bytes;
} rc_outlines_info;
/* Allocates everything the slot will ever need.  Re-opening replaces the state; a refused open leaves the open state as it was.
 * RC_EINVAL without parameters, for a value outside the ranges above, flags or a pad word that is not zero; RC_ESIZE beyond the
 * context's max_w x max_h or RC_OUTLINES_MAX_SIDE. */
int rcflow_outlines_open(rc_ctx* ctx, int stream, int w, int h, const rc_outlines_params* prm);
/* One picture.  Exactly one of d_labels and d_mask (RC_EINVAL for both or neither); d_loops max_loops x rc_outline_loop and d_summary
 * RC_OUTLINES_SUMMARY int64 (8-byte aligned), d_verts 2 * max_vertices int32 (4-byte aligned), each optional: the state is updated
 * whatever is asked for, and what a call gives does not depend on what it asked for.  No host synchronisation, no device-to-host
 * copy.  An output whose byte range overlaps the input's or another output's is RC_EINVAL.  The input is never written.  Every
 * refusal is decided before anything is queued and leaves state and outputs as they were; RC_ESTATE before rcflow_outlines_open.
 * RC_EHIP (the runtime refused a launch) is no refusal: the state is undefined until rcflow_outlines_reset. */
int rcflow_outlines_push_dev(rc_ctx* ctx, int stream, const int32_t* d_labels, size_t labels_step, const uint8_t* d_mask, size_t mask_step,
                             rc_outline_loop* d_loops, int32_t* d_verts, long long* d_summary);
/* max_vertices primitives of the last push into d_prims ("outlines@11"; all zero before the first and after a reset).  RC_EINVAL:
 * d_prims NULL or not 4-byte aligned, thickness outside 1..RC_DRAW_MAX_THICKNESS. */
int rcflow_outlines_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, rc_draw_prim* d_prims);
/* Blocks until the slot's stream has finished; for hosts and tests.  The first min(written, cap) records of the last push into
 * `loops` and the first min(written, vcap) vertices into `verts` (2 int32 each); *n the records written, *nv the vertices written;
 * each pointer may be NULL (with its cap 0).  Zeros before the first push and after a reset.  RC_EINVAL for a negative cap or a cap
 * without a buffer. */
int rcflow_outlines_read(rc_ctx* ctx, int stream, rc_outline_loop* loops, int cap, int* n, int32_t* verts, int vcap, int* nv,
                         long long summary[RC_OUTLINES_SUMMARY]);
/* min_cracks >= 1 (RC_EINVAL otherwise), from the next push on */
int rcflow_outlines_set(rc_ctx* ctx, int stream, int min_cracks);
/* zeroes the records, the vertices, the summary and the push count; keeps the allocation and min_cracks; asynchronous, on the slot's stream */
int rcflow_outlines_reset(rc_ctx* ctx, int stream);
/* frees the state (rcflow_destroy does the same); RC_OK when nothing is open */
int rcflow_outlines_close(rc_ctx* ctx, int stream);
/* never blocks; RC_ESTATE when nothing is open, RC_EINVAL without a buffer */
int rcflow_outlines_info(rc_ctx* ctx, int stream, rc_outlines_info* info);

/* Display path, ripcurrents.cpp:233-273 (= streamline_displacement / _total_motion / _ratio /
 * _positions, ripcurrents_module.cpp:13-60) on the slot's streamline field (rcflow_advect_field_dev):
 * which 0 = |pt|, 1 = dist, 2 = |pt| / dist; minMaxLoc + convertTo(CV_8UC1, 255/max) +
 * applyColorMap(COLORMAP_JET) -> 8UC3 BGR.  max_out (host, may be NULL) receives the maximum (blocks). */
int rcflow_streamline_display_dev(rc_ctx* ctx, int stream, int which, uint8_t* d_bgr, size_t bgr_step,
                                  float* max_out);
/* marks (1,1,1) in a 32FC3 image where each pixel's particle sits (:44-60); the caller zeroes it */
int rcflow_streamline_positions_dev(rc_ctx* ctx, int stream, float* d_density, size_t density_step);
/* cvtColor(current, current, CV_HSV2BGR) on the 32FC3 display image (ripcurrents.cpp:405); H in degrees */
int rcflow_hsv_to_bgr_dev(rc_ctx* ctx, int stream, const float* d_hsv, size_t hsv_step, int w, int h,
                          float* d_bgr, size_t bgr_step);
/* frame size of the slot's analysis state (0, 0 before rcflow_analysis_reset / the first analysis call) */
int rcflow_analysis_size(rc_ctx* ctx, int stream, int* w, int* h);
/* the 256 x BGR table of applyColorMap(COLORMAP_JET) (host) */
int rcflow_jet_lut(uint8_t* lut_bgr /* 768 */);

/* Sparse pyramidal Lucas-Kanade: cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err,
 * winSize, maxLevel, criteria, flags, minEigThreshold) on 8UC1 device images -- Streakline.cpp:32,
 * ripcurrents_module.cpp:716, :738, :775, :1162.  d_prev_pts / d_next_pts: npts x (x, y) floats on the
 * device; d_status npts bytes; d_err npts floats or NULL (without it, as upstream, the residual pass and
 * the bounds test of the final position in it are skipped).  crit_type bit 0 = TermCriteria::COUNT,
 * bit 1 = EPS; flags: 4 = OPTFLOW_USE_INITIAL_FLOW (d_next_pts is then also an input), 8 =
 * OPTFLOW_LK_GET_MIN_EIGENVALS.  maxLevel < 8, windows up to 128x128. */
int rcflow_pyrlk_dev(rc_ctx* ctx, int stream, const uint8_t* d_prev, size_t prev_step,
                     const uint8_t* d_next, size_t next_step, int w, int h, const float* d_prev_pts,
                     float* d_next_pts, int npts, uint8_t* d_status, float* d_err, int win_w, int win_h,
                     int max_level, int crit_type, int max_count, double epsilon, int flags,
                     double min_eig_threshold);
/* the same with host pointers (the cv:: signature's form): copies in, tracks, copies out, blocking */
int rcflow_pyrlk_u8(rc_ctx* ctx, int stream, const uint8_t* prev, size_t prev_step, const uint8_t* next,
                    size_t next_step, int w, int h, const float* prev_pts, float* next_pts, int npts,
                    uint8_t* status, float* err, int win_w, int win_h, int max_level, int crit_type,
                    int max_count, double epsilon, int flags, double min_eig_threshold);
/* last pyramid level buildOpticalFlowPyramid keeps for this size and window */
int rcflow_pyrlk_levels(int w, int h, int win_w, int win_h, int max_level);

/* ------------------------------------------------------------------ multi-GPU: the global flow histogram
 * one process per GPU, each on its own video segment; the only exchange is the integer sum of
 * the RC_HIST_WORDS histogram counters (7548 B) over RCCL, after which every rank derives the same global
 * UPPER / UPPER2d / prop_above_upper (what ripcurrents.cpp:333-366 computes from one stream's counters).
 * librccl is opened at run time by these calls only.  A world of one rank with a NULL id is the identity and needs no
 * RCCL; with an id it is a one-rank RCCL communicator like any other. */
#define RC_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */
/* rank 0: creates the id; the host distributes it to the other ranks (MPI, a socket, a file) */
int rcflow_comm_unique_id(void* id_out /* RC_COMM_ID_BYTES */);
/* every rank, collectively: joins the communicator on the context's GPU.  RC_ECOMM when RCCL fails. */
int rcflow_comm_init(rc_ctx* ctx, const void* unique_id /* RC_COMM_ID_BYTES; NULL when world == 1: no RCCL */,
                     int rank, int world);
int rcflow_comm_destroy(rc_ctx* ctx);
int rcflow_comm_rank(rc_ctx* ctx, int* rank, int* world);
/* Starts the sum over all ranks of the slot's histogram counters as they are at this point of the slot's
 * stream; the result goes to d_words_out (device, RC_HIST_WORDS int32) or, when NULL, to a context-owned
 * buffer (rcflow_allreduce_hist_result).  Asynchronous and off the slot's stream: the collective runs on its
 * own HIP stream beside whatever the slot does next.  Collective: every rank calls it the same number of times,
 * and no rank ever skips the reduction on a local condition (a rank that did would leave the others waiting). */
int rcflow_allreduce_hist(rc_ctx* ctx, int stream, int32_t* d_words_out);
/* Verdict on the collective started last, the same on every rank (it comes from a reduced word): waits for the
 * collective on the host, then RC_ESTATE when the ranks together counted more pixels than the int32 histsum of the
 * reference (ripcurrents.cpp:147-150) can hold -- reduce per shorter segment -- else RC_OK.  pixels_counted (may be
 * NULL): the upper bound used. */
int rcflow_allreduce_hist_status(rc_ctx* ctx, long long* pixels_counted);
/* Orders the slot's stream after the collective started last (no host wait): call it before
 * rcflow_thresholds_words_dev(ctx, stream, d_words_out). */
int rcflow_allreduce_hist_join(rc_ctx* ctx, int stream);
int rcflow_allreduce_hist_result(rc_ctx* ctx, int32_t** d_words);

/* ------------------------------------------------------------------ measurement */
/* When enabled every kernel launch is bracketed by HIP events on the slot's stream.  Measurement
 * aid: while it is on, drive the context from one thread only (the event list is per context). */
int rcflow_profile_enable(rc_ctx* ctx, int on);
int rcflow_profile_reset(rc_ctx* ctx);
/* Resolves pending events and returns per-kernel totals.  names[i] points to a static
 * string "kernel@level"; returns the number of entries written (<= cap).  alg_bytes = the
 * launches' compulsory bytes (inputs once + outputs once); model_bytes = SURVEY.md section
 * 8(d)'s algorithmic bytes of the stages those launches stand for. */
int rcflow_profile_read(rc_ctx* ctx, int cap, const char** names, int* launches,
                        double* total_ms, double* alg_bytes, double* model_bytes);

/* The same totals under the reference's own bucket names, in the order it prints them (ripcurrents.cpp:103-109,
 * :518-524): farneback, polar, threshold, overlay, erosion, codec, stream ("pathlines").  GPU time of the kernels
 * that do each bucket's work ("overlay" includes the time-exposure images, the 8-bit colour stages, the wave spectra, the shoreline and the surf zone, "farneback" the frame stabilisation, the opposing-flow map, the motion templates, the plan view, the ensemble PIV, the flow kinematics, the mean flow and the flow check, "stream" the flow map and FTLE, the transects and the drifters); "polar" is 0 (the cartToPolar of :305-309 is fused into the histogram and
 * classification kernels, booked under "threshold"), "codec" is 0 (video decode is host I/O outside the library).
 * names / ms: RC_PROFILE_BUCKETS entries each (either may be NULL).  Returns RC_PROFILE_BUCKETS. */
#define RC_PROFILE_BUCKETS 7
int rcflow_profile_read_buckets(rc_ctx* ctx, const char** names, double* ms);

#ifdef __cplusplus
}
#endif
#endif
