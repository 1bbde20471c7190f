// rcflow_module.hpp -- C++ host-side mirror of the reference's interface for the hot path,
// over the C ABI of librcflow (include/rcflow.h).  Header-only; needs the HIP runtime API
// for host<->device copies (compile with hipcc, or g++ -D__HIP_PLATFORM_AMD__
// -I/opt/rocm/include ... -lamdhip64 -lrcflow).
//
// Names, argument order and meaning follow /root/reference/RipCurrents_main:
//   calcOpticalFlowFarneback   the cv:: call at ripcurrents.cpp:215, main.cpp:264,...
//   create_histogram           ripcurrents.hpp:39   ripcurrents_module.cpp:89-144
//   create_flow                ripcurrents.hpp:50   ripcurrents_module.cpp:153-182
//   create_accumulationbuffer  ripcurrents.hpp:52   ripcurrents_module.cpp:189-212
//   streamline_field           ripcurrents.hpp:22   ripcurrents_module.cpp:608-648
//   streamline                 ripcurrents.hpp:23   ripcurrents_module.cpp:486-528
//   Streakline                 Streakline.hpp:8-20  Streakline.cpp:11-71
//   Timeline, PopulationMap    ripcurrents.hpp:64-75, 86-95  ripcurrents_module.cpp:751-807, 1140-1196
//   timexOpen / timexPush      compute_timex main.cpp:1195-1263, compute_brightColor main.cpp:1265-1383
//   framestabOpen / framestabPush   compute_phaseCorrelate main.cpp:1684-1775
//   framestabOpenMulti, warpAffine, warpPerspective   the correction of stabilize (main.cpp:1556-1682) by that estimator
//   RipMap                     averageVector ripcurrents_module.cpp:386-484, finished (the opposing-flow map)
// rc::Mat is a non-owning view with cv::Mat's fields (data, step, rows, cols); with OpenCV
// present, include/rcflow_cv.hpp converts cv::Mat to it.  Errors are thrown as
// rc::Error (the reference's OpenCV calls throw cv::Exception and are never caught).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "rcflow.h"

namespace rc {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc) {
    if (rc < 0) throw Error(rc, std::string("rcflow error ") + std::to_string(rc) + ": " + rcflow_last_error());
}
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(RC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// cv::Mat-compatible view of host memory (interleaved channels, byte step).
struct Mat {
    void* data = nullptr;
    size_t step = 0;
    int rows = 0, cols = 0;
    int channels = 1, elem = 1;   // elem = bytes per channel
    Mat() = default;
    Mat(int r, int c, int ch, int el, void* d, size_t st = 0)
        : data(d), step(st ? st : (size_t)c * ch * el), rows(r), cols(c), channels(ch), elem(el) {}
    size_t row_bytes() const { return (size_t)cols * channels * elem; }
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
};

typedef struct { float x, y; } Pixel2;   // cv::Point_<float> (ripcurrents.hpp:19)

// ---- the staging layer: how every class below checks a host image and moves it to and from the device ----

// a non-empty view of exactly this geometry (elem = bytes per channel)
inline bool is_image(const Mat& m, int cols, int rows, int channels, int elem) {
    return !m.empty() && m.cols == cols && m.rows == rows && m.channels == channels && m.elem == elem;
}

// m's rows between the host view (its own step) and device memory of pitch `pitch`
inline void copy_in(void* d, size_t pitch, const Mat& m, const char* what) {
    hip_check(hipMemcpy2D(d, pitch, m.data, m.step, m.row_bytes(), m.rows, hipMemcpyHostToDevice), what);
}
inline void copy_out(const Mat& m, const void* d, size_t pitch, const char* what) {
    hip_check(hipMemcpy2D(m.data, m.step, d, pitch, m.row_bytes(), m.rows, hipMemcpyDeviceToHost), what);
}

// One device image with dense rows, allocated at first use and freed with its owner.
class DeviceImage {
  public:
    DeviceImage() = default;
    ~DeviceImage() { if (d_) (void)hipFree(d_); }
    DeviceImage(const DeviceImage&) = delete;
    DeviceImage& operator=(const DeviceImage&) = delete;

    // allocates at the first call, which is all that an image only the device writes needs; the geometry of that call
    // stays, and a later call, upload or download with another is refused before anything is copied
    void reserve(int cols, int rows, int channels, int elem) {
        const size_t pitch = (size_t)cols * channels * elem;
        if (d_) {
            if (pitch != pitch_ || rows != rows_) throw Error(RC_EINVAL, "DeviceImage: not the geometry the image was allocated with");
            return;
        }
        hip_check(hipMalloc(&d_, pitch * rows), "hipMalloc staging image");
        pitch_ = pitch; rows_ = rows;
    }
    void upload(const Mat& m) { reserve(m.cols, m.rows, m.channels, m.elem); copy_in(d_, pitch_, m, "upload image"); }
    void download(Mat& m) { reserve(m.cols, m.rows, m.channels, m.elem); copy_out(m, d_, pitch_, "download image"); }
    // wanted = false: null, for an optional argument of the library that this call does not ask for
    template <class T> T* ptr(bool wanted = true) const { return wanted ? (T*)d_ : nullptr; }
    size_t pitch() const { return pitch_; }

  private:
    void* d_ = nullptr;
    size_t pitch_ = 0;
    int rows_ = 0;
};

struct StageIn { DeviceImage& dev; const Mat* host; };    // host null: not given
struct StageOut { DeviceImage& dev; Mat* host; };         // host null: not asked for

// The one order of a call that takes host images, after the caller has validated every argument: the staging images
// of what was given and asked for are allocated, the stream is drained once before they are overwritten (the library
// call of the last push may still be reading them), the inputs go up, `call` (the library's, returning its code) runs,
// and only when a host output was asked for the stream is drained once more and the outputs come down.  A call without
// host outputs returns with its work in flight; one without host inputs overwrites nothing and does not drain first.
// Returns call's code.
template <class Call>
int staged(rc_ctx* ctx, std::initializer_list<StageIn> ins, Call&& call, std::initializer_list<StageOut> outs) {
    auto given = [](const auto& s) { return s.host != nullptr; };
    auto reserve = [](const auto& s) { if (s.host) s.dev.reserve(s.host->cols, s.host->rows, s.host->channels, s.host->elem); };
    std::for_each(ins.begin(), ins.end(), reserve);
    std::for_each(outs.begin(), outs.end(), reserve);
    if (std::any_of(ins.begin(), ins.end(), given)) check(rcflow_sync(ctx, 0));
    for (const StageIn& i : ins) if (i.host) i.dev.upload(*i.host);
    const int rc = call();
    check(rc);
    if (std::any_of(outs.begin(), outs.end(), given)) check(rcflow_sync(ctx, 0));
    for (const StageOut& o : outs) if (o.host) o.dev.download(*o.host);
    return rc;
}

// The draw path of Regions, Tracks and MotionTemplates: the canvas goes up, `fill` writes `n` primitives on the device,
// rcflow_draw_dev paints them, the canvas comes down.
template <class Fill>
void staged_draw(rc_ctx* ctx, DeviceImage& canvas, DeviceImage& prims, int n, Mat& img, Fill&& fill) {
    prims.reserve(n, 1, 1, (int)sizeof(rc_draw_prim));
    staged(ctx, {{canvas, &img}}, [&] {
        const int rc = fill(prims.ptr<rc_draw_prim>());
        if (rc < 0) return rc;
        return rcflow_draw_dev(ctx, 0, canvas.ptr<uint8_t>(), canvas.pitch(), img.cols, img.rows, 3, prims.ptr<const rc_draw_prim>(), n, nullptr);
    }, {{canvas, &img}});
}

// One stream slot of one GPU context plus the device copies the module functions work on.
// The flow field stays resident on the device between calcOpticalFlowFarneback and the
// analysis calls, like `current` does on the host in ripcurrents.cpp:221-440.
class Pipeline {
  public:
    Pipeline(int xdim, int ydim, int device = 0) : w_(xdim), h_(ydim) {
        check(rcflow_create(&ctx_.p, device, xdim, ydim, 1));
        d_frames_.reserve(w_, 2 * h_, 1, 1);                     // prev above next
        d_flow_.reserve(w_, h_, 2, 4);
        d_mask_.reserve(w_, h_, 1, 1);
        flow_src_ = d_flow_.ptr<float>();
        check(rcflow_analysis_reset(ctx_, 0, w_, h_));
    }
    ~Pipeline() { if (d_scratch_) (void)hipFree(d_scratch_); }
    Pipeline(const Pipeline&) = delete;
    Pipeline& operator=(const Pipeline&) = delete;

    rc_ctx* context() { return ctx_; }
    const float* device_flow() const { return flow_src_; }

    // cv::calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations,
    // poly_n, poly_sigma, flags): 8UC1 in, CV_32FC2 out (flow.data may be null: the field then
    // only stays resident for the analysis calls).  flags & RC_FARNEBACK_USE_INITIAL_FLOW: the two-image call takes `flow`
    // as in/out; pushFrame / pushAcquired / loopStep start every pair from the resident field of the previous one.
    // The frame loop itself (ripcurrents.cpp:194-221: capture, calcOpticalFlowFarneback(u_f2, u_f1, ...),
    // u_f1.copyTo(u_f2)) with the previous frame kept on the device: one upload and one pyramid + expansion
    // per frame (rcflow_push_frame_dev).  Returns false for the call that primes the stream (the first one, or
    // the first with other parameters): no flow yet.  The flow equals calcOpticalFlowFarneback(previous, frame).
    // The upload goes through the library's page-locked double buffer (rcflow_push_frame_u8) and is
    // asynchronous: with a null `flow` view the call returns while upload and kernels are still running, and the
    // analysis calls below queue behind them on the same stream; only a non-null `flow` waits and downloads.
    bool pushFrame(const Mat& frame, Mat& flow, double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                   double poly_sigma, int flags) {
        if (!is_image(frame, w_, h_, 1, 1)) throw Error(RC_EINVAL, "pushFrame: frame must be 8UC1 of the pipeline's size");
        const bool read = wanted(flow);
        rc_farneback_params p = {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags};
        return pushed(rcflow_push_frame_u8(ctx_, 0, (const uint8_t*)frame.data, frame.step, w_, h_, &p), read ? &flow : nullptr);
    }

    // The same loop without the staging copy: frameBuffer() is the slot's next page-locked staging buffer as an 8UC1
    // view of the pipeline's size -- make it the destination of the cvtColor at ripcurrents.cpp:210 -- and pushAcquired()
    // pushes it (rcflow_frame_buffer_acquire / rcflow_push_frame_acquired).
    Mat frameBuffer() {
        uint8_t* p = nullptr;
        size_t step = 0;
        check(rcflow_frame_buffer_acquire(ctx_, 0, w_, h_, &p, &step));
        return Mat(h_, w_, 1, 1, p, step);
    }
    bool pushAcquired(Mat& flow, double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma,
                      int flags) {
        const bool read = wanted(flow);
        rc_farneback_params p = {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags};
        return pushed(rcflow_push_frame_acquired(ctx_, 0, &p), read ? &flow : nullptr);
    }

    // One whole iteration of the frame loop (ripcurrents.cpp:194-479) behind one call: the frame produced into
    // frameBuffer() is pushed, then streamline_field, the seed streamlines (d_seeds: device, n x (x, y), advanced in
    // place; may be null), histogram + thresholds, create_flow + create_accumulationbuffer (the frame counter lives on the
    // device) and the mask's edges run on the resident field (rcflow_frame_loop_step).  Returns false for the call that
    // primes the stream.  The masks stay on the device: outmaskDevice() / edgesDevice(), or read them back as needed.
    bool loopStep(double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags,
                  float dt = 2.f, int streamline_iterations = 1, float* d_seeds = nullptr, int nseeds = 0, float seed_upper = 100.f,
                  float MID = 0.5f, float LOWER = 0.2f, bool use_graph = false) {
        d_edges_.reserve(w_, h_, 1, 1);
        rc_farneback_params p = {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags};
        rc_frame_loop L;
        std::memset(&L, 0, sizeof(L));
        L.dt = dt; L.iterations = streamline_iterations;
        L.d_seeds = d_seeds; L.nseeds = nseeds; L.seed_variant = 3; L.seed_dt = dt; L.seed_iterations = streamline_iterations; L.seed_upper = seed_upper;
        L.MID = MID; L.LOWER = LOWER;
        L.d_outmask = d_mask_.ptr<uint8_t>(); L.mask_step = d_mask_.pitch(); L.d_edges = d_edges_.ptr<uint8_t>(); L.edges_step = d_edges_.pitch();
        L.use_graph = use_graph ? 1 : 0;
        return pushed(rcflow_frame_loop_step(ctx_, 0, &p, &L), nullptr);
    }
    const uint8_t* outmaskDevice() const { return d_mask_.ptr<const uint8_t>(); }
    const uint8_t* edgesDevice() const { return d_edges_.ptr<const uint8_t>(); }

    void calcOpticalFlowFarneback(const Mat& prev, const Mat& next, Mat& flow, double pyr_scale, int levels,
                                  int winsize, int iterations, int poly_n, double poly_sigma, int flags) {
        require_pair(prev, next, "calcOpticalFlowFarneback");
        const bool initial = (flags & RC_FARNEBACK_USE_INITIAL_FLOW) != 0;
        // OPTFLOW_USE_INITIAL_FLOW: `flow` is in/out -- its content starts the coarsest scale (include/rcflow.h)
        if (initial && !is_image(flow, w_, h_, 2, 4))
            throw Error(RC_EINVAL, "OPTFLOW_USE_INITIAL_FLOW: flow must hold a CV_32FC2 field of the frame size");
        const bool read = wanted(flow);
        uint8_t* df = upload_pair(prev, next);
        if (initial) d_flow_.upload(flow);
        rc_farneback_params p = {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags};
        check(rcflow_farneback_dev(ctx_, 0, df, w_, df + (size_t)w_ * h_, w_, w_, h_, d_flow_.ptr<float>(), d_flow_.pitch(), &p));
        flow_src_ = d_flow_.ptr<float>();
        check(rcflow_sync(ctx_, 0));
        if (read) d_flow_.download(flow);
    }

    // cv::calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, status, err, winSize, maxLevel,
    // criteria(type, maxCount, epsilon), flags, minEigThreshold) on 8UC1 frames -- Streakline.cpp:32,
    // ripcurrents_module.cpp:716, :738, :775, :1162.  criteria type: 1 = COUNT, 2 = EPS.
    void calcOpticalFlowPyrLK(const Mat& prev, const Mat& next, const std::vector<Pixel2>& prevPts,
                              std::vector<Pixel2>& nextPts, std::vector<unsigned char>& status, std::vector<float>& err,
                              int win_w = 21, int win_h = 21, int maxLevel = 3, int crit_type = 3, int maxCount = 30,
                              double epsilon = 0.01, int flags = 0, double minEigThreshold = 1e-4) {
        require_pair(prev, next, "calcOpticalFlowPyrLK");
        const int n = (int)prevPts.size();
        const bool initial = (flags & 4) != 0;
        if (initial && (int)nextPts.size() != n) throw Error(RC_EINVAL, "OPTFLOW_USE_INITIAL_FLOW needs nextPts of prevPts' size");
        nextPts.resize(n); status.assign(n, 0); err.assign(n, 0.f);
        if (n == 0) return;
        uint8_t* df = upload_pair(prev, next);
        // prevPts | nextPts | err | status in the pipeline's grow-only scratch buffer (no allocation in the frame loop)
        const size_t off_n = (size_t)n * 8, off_e = 2 * off_n, off_s = off_e + (size_t)n * 4;
        char* b = (char*)scratch(off_s + n);
        hipError_t e = hipMemcpy(b, prevPts.data(), off_n, hipMemcpyHostToDevice);
        if (e == hipSuccess && initial) e = hipMemcpy(b + off_n, nextPts.data(), off_n, hipMemcpyHostToDevice);
        int rc = e == hipSuccess ? rcflow_pyrlk_dev(ctx_, 0, df, w_, df + (size_t)w_ * h_, w_, w_, h_, (const float*)b,
                                                    (float*)(b + off_n), n, (uint8_t*)(b + off_s), (float*)(b + off_e), win_w,
                                                    win_h, maxLevel, crit_type, maxCount, epsilon, flags, minEigThreshold)
                                 : RC_EHIP;
        if (rc == RC_OK) rc = rcflow_sync(ctx_, 0);
        if (rc == RC_OK) {
            e = hipMemcpy(nextPts.data(), b + off_n, off_n, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(err.data(), b + off_e, (size_t)n * 4, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(status.data(), b + off_s, n, hipMemcpyDeviceToHost);
        }
        check(rc);
        hip_check(e, "PyrLK point transfer");
    }

    // Replace the resident flow field (e.g. after host-side edits of `current`).
    void upload_flow(const Mat& current) {
        if (!is_image(current, w_, h_, 2, 4)) throw Error(RC_EINVAL, "current must be CV_32FC2 of the frame size");
        d_flow_.upload(current);
        flow_src_ = d_flow_.ptr<float>();
    }

    // create_histogram(current, hist, histsum, hist2d, histsum2d, UPPER, UPPER2d, prop_above_upper)
    // on the resident flow field.  The counters are cumulative in the slot (never reset by the
    // reference); the arrays receive their current values.
    void create_histogram(int hist[RC_HIST_BINS], int& histsum, int hist2d[RC_HIST_DIRECTIONS][RC_HIST_BINS],
                          int histsum2d[RC_HIST_DIRECTIONS], float& UPPER, float UPPER2d[RC_HIST_DIRECTIONS],
                          float prop_above_upper[RC_HIST_DIRECTIONS]) {
        check(rcflow_histogram_dev(ctx_, 0, flow_src_, (size_t)w_ * 8, w_, h_));
        check(rcflow_thresholds_dev(ctx_, 0));
        int32_t hs = 0;
        check(rcflow_histogram_read(ctx_, 0, hist, &hist2d[0][0], &hs, histsum2d, &UPPER, UPPER2d, prop_above_upper));
        histsum = hs;
    }

    // create_flow + create_accumulationbuffer in one pass; outmask (8UC1, may be null view)
    // receives the wave mask.  UPPER / UPPER2d are the slot's (from create_histogram).
    void create_flow_and_accumulationbuffer(Mat& outmask, int framecount, float MID = 0.5f, float LOWER = 0.2f) {
        check(rcflow_classify_accumulate_dev(ctx_, 0, flow_src_, (size_t)w_ * 8, w_, h_, framecount, MID,
                                             LOWER, nullptr, 0, nullptr, 0, nullptr, 0, d_mask_.ptr<uint8_t>(), d_mask_.pitch()));
        check(rcflow_sync(ctx_, 0));
        // deliberately as it always was: only outmask's data and step are read, its own geometry is not asked, and the
        // pipeline's rows are written -- the one host image here that does not pass is_image
        if (outmask.data) copy_out(Mat(h_, w_, 1, 1, outmask.data, outmask.step), d_mask_.ptr<void>(), d_mask_.pitch(), "download mask");
    }
    void accumulator(float* acc_x) { check(rcflow_accumulator_read(ctx_, 0, acc_x)); }

    // streamlines_mat.forEach(streamline_field(&pixel, distance, x, y, current, dt, iterations,
    // UPPER, prop_above_upper)) -- ripcurrents.cpp:229-231.  UPPER < 0: the slot's UPPER.
    void streamline_field(float dt, int iterations, float UPPER = -1.f) {
        check(rcflow_advect_field_dev(ctx_, 0, flow_src_, (size_t)w_ * 8, w_, h_, dt, iterations, UPPER));
    }
    void streamline_field_state(Pixel2* streamlines_mat, float* streamlines_distance) {
        check(rcflow_advect_field_read(ctx_, 0, (float*)streamlines_mat, streamlines_distance));
    }

    // streamline_displacement / streamline_total_motion / streamline_ratio
    // (ripcurrents_module.cpp:13-40, ripcurrents.cpp:233-257) on the resident streamline field:
    // streamoverlay_color must be 8UC3 of the frame size; only that image crosses PCIe.
    void streamline_displacement(Mat& streamoverlay_color) { display(0, streamoverlay_color); }
    void streamline_total_motion(Mat& streamoverlay_color) { display(1, streamoverlay_color); }
    void streamline_ratio(Mat& streamoverlay_color) { display(2, streamoverlay_color); }

    // for (s...) streamline(streampt + s, color, current, overlay, dt, iterations, UPPER, ...):
    // advances the seeds; `trace` (optional, n*iterations points) is what the host draws with
    // cv::line.  variant: see rcflow_advect_points_dev.
    void streamline(Pixel2* streampt, int n, float dt, int iterations, float UPPER, int variant = 0,
                    std::vector<Pixel2>* trace = nullptr) {
        if (n <= 0) return;
        const int iters = variant == 2 ? 100 : iterations;
        const size_t pts_bytes = ((size_t)n * 8 + 255) & ~(size_t)255;
        char* b = (char*)scratch(pts_bytes + (trace ? (size_t)n * iters * 8 : 0));     // grow-only, no per-frame allocation
        void *d_pts = b, *d_tr = trace ? b + pts_bytes : nullptr;
        hip_check(hipMemcpy(d_pts, streampt, (size_t)n * 8, hipMemcpyHostToDevice), "upload seeds");
        int rc = rcflow_advect_points_dev(ctx_, 0, (float*)d_pts, n, flow_src_, (size_t)w_ * 8, w_, h_, dt,
                                          iterations, UPPER, variant, (float*)d_tr);
        if (rc == RC_OK) rc = rcflow_sync(ctx_, 0);
        if (rc == RC_OK) {
            (void)hipMemcpy(streampt, d_pts, (size_t)n * 8, hipMemcpyDeviceToHost);
            if (trace) {
                trace->resize((size_t)n * iters);
                (void)hipMemcpy(trace->data(), d_tr, (size_t)n * iters * 8, hipMemcpyDeviceToHost);
            }
        }
        check(rc);
    }

    // The time-exposure pipelines on frames of the pipeline's size: compute_timex (main.cpp:1195-1263, RC_TIMEX_MEAN)
    // and compute_brightColor (main.cpp:1265-1383: RC_TIMEX_AVERAGE / _BRIGHT / _DARK = its options 0 / 1 / 2 over a
    // ring of `window` frames).  timexPush takes the resized 8UC3 frame (main.cpp:1227, :1302) and fills the images
    // asked for (8UC3 of the frame size; an empty Mat skips that product's image, its state is still updated) with
    // what the reference writes to its output video after this frame.
    void timexOpen(int window, int products) { check(rcflow_timex_open(ctx_, 0, w_, h_, window, products)); }
    void timexPush(const Mat& frame, Mat& mean, Mat& average, Mat& bright, Mat& dark) {
        Mat* outs[4] = {&mean, &average, &bright, &dark};
        const size_t img = ((size_t)w_ * h_ * 3 + 255) & ~(size_t)255;
        if (!is_image(frame, w_, h_, 3, 1)) throw Error(RC_EINVAL, "timexPush: frame must be 8UC3 of the pipeline's size");
        for (Mat* m : outs)
            if (!m->empty() && !is_image(*m, w_, h_, 3, 1)) throw Error(RC_EINVAL, "timexPush: images must be 8UC3 of the frame size");
        uint8_t* b = (uint8_t*)scratch(5 * img);                 // grow-only: the frame and the four images
        const size_t pitch = frame.row_bytes();
        copy_in(b, pitch, frame, "upload frame");
        uint8_t* d_out[4];
        size_t out_step[4];
        for (int k = 0; k < 4; k++) {
            d_out[k] = outs[k]->empty() ? nullptr : b + (k + 1) * img;
            out_step[k] = pitch;
        }
        check(rcflow_timex_push_dev(ctx_, 0, b, pitch, d_out, out_step));
        check(rcflow_sync(ctx_, 0));
        for (int k = 0; k < 4; k++)
            if (d_out[k]) copy_out(*outs[k], d_out[k], pitch, "download time-exposure image");
    }
    void timexReset() { check(rcflow_timex_reset(ctx_, 0)); }
    void timexClose() { check(rcflow_timex_close(ctx_, 0)); }

    // compute_phaseCorrelate (main.cpp:1684-1775) on frames of the pipeline's size: framestabPush takes the resized
    // 8UC3 frame (main.cpp:1723) and fills `corrected` (8UC3 of the frame size) with what the reference writes to its
    // output video, registered to the last corrected frame on the patch given at open (default: the reference's
    // roi, main.cpp:1728-1732).  shift (optional): shift_x, shift_y, response of this frame (main.cpp:1745).
    void framestabOpen() { framestabOpen(w_ - 50, 50, 50, 50); }
    void framestabOpen(int roi_x, int roi_y, int roi_w, int roi_h) { check(rcflow_framestab_open(ctx_, 0, w_, h_, roi_x, roi_y, roi_w, roi_h)); }
    void framestabPush(const Mat& frame, Mat& corrected, double shift[3] = nullptr) {
        const size_t img = ((size_t)w_ * h_ * 3 + 255) & ~(size_t)255;
        if (!is_image(frame, w_, h_, 3, 1) || !is_image(corrected, w_, h_, 3, 1))
            throw Error(RC_EINVAL, "framestabPush: frame and corrected must be 8UC3 of the pipeline's size");
        uint8_t* b = (uint8_t*)scratch(2 * img);                 // grow-only: the frame and the corrected frame
        const size_t pitch = frame.row_bytes();
        copy_in(b, pitch, frame, "upload frame");
        check(rcflow_framestab_push_dev(ctx_, 0, b, pitch, b + img, pitch, nullptr));
        double r[3] = {0., 0., 0.};
        check(rcflow_framestab_read(ctx_, 0, r, nullptr));       // waits for the push
        copy_out(corrected, b + img, pitch, "download corrected frame");
        if (shift) { shift[0] = r[0]; shift[1] = r[1]; shift[2] = r[2]; }
    }
    // Several static patches (n x (x, y, w, h), one size) and a fitted motion: model RC_STAB_TRANSLATION / _SIMILARITY /
    // _AFFINE over the patches whose response reaches min_response; flags: RC_STAB_ANCHOR_FIRST.  framestabPush then
    // corrects roll and zoom too, and framestabMotion reads the 2 x 3 motion of the last push (corrected(p) = frame(T p)).
    void framestabOpenMulti(const std::vector<int>& rois, int model = RC_STAB_SIMILARITY, double min_response = 0., int flags = 0) {
        check(rcflow_framestab_open_multi(ctx_, 0, w_, h_, rois.data(), (int)(rois.size() / 4), model, min_response, flags));
    }
    void framestabMotion(double motion[6], int* model_used = nullptr, int* patches_used = nullptr) {
        check(rcflow_framestab_read_motion(ctx_, 0, motion, model_used, patches_used, nullptr, nullptr));
    }
    // cv::warpAffine / cv::warpPerspective(src, dst, M, dst.size(), INTER_LINEAR [| WARP_INVERSE_MAP]) on 8UC3 host
    // images of any size within the pipeline's (flags: 0 or RC_WARP_INVERSE_MAP).
    void warpAffine(const Mat& src, Mat& dst, const double M[6], int flags = 0) { warp(src, dst, M, flags, false); }
    void warpPerspective(const Mat& src, Mat& dst, const double M[9], int flags = 0) { warp(src, dst, M, flags, true); }
    void framestabReset() { check(rcflow_framestab_reset(ctx_, 0)); }
    void framestabClose() { check(rcflow_framestab_close(ctx_, 0)); }

    int width() const { return w_; }
    int height() const { return h_; }

  private:
    void warp(const Mat& src, Mat& dst, const double* M, int flags, bool perspective) {
        // 8UC3 of any size: each view's own
        if (!is_image(src, src.cols, src.rows, 3, 1) || !is_image(dst, dst.cols, dst.rows, 3, 1))
            throw Error(RC_EINVAL, "warp: src and dst must be 8UC3");
        const size_t sb = (src.row_bytes() * src.rows + 255) & ~(size_t)255, db = dst.row_bytes() * dst.rows;
        uint8_t* b = (uint8_t*)scratch(sb + db);
        copy_in(b, src.row_bytes(), src, "upload image");
        check((perspective ? rcflow_warp_perspective_bgr_dev : rcflow_warp_affine_bgr_dev)(
            ctx_, 0, b, src.row_bytes(), src.cols, src.rows, b + sb, dst.row_bytes(), dst.cols, dst.rows, M, flags));
        check(rcflow_sync(ctx_, 0));
        copy_out(dst, b + sb, dst.row_bytes(), "download warped image");
    }
    // grow-only device scratch for the per-frame helpers (seeds, traces, display image, LK points)
    void* scratch(size_t bytes) {
        if (bytes > scratch_bytes_) {
            check(rcflow_sync(ctx_, 0));
            if (d_scratch_) (void)hipFree(d_scratch_);
            d_scratch_ = nullptr; scratch_bytes_ = 0;
            const size_t want = bytes + bytes / 2;
            hip_check(hipMalloc(&d_scratch_, want), "hipMalloc scratch");
            scratch_bytes_ = want;
        }
        return d_scratch_;
    }
    void display(int which, Mat& bgr) {
        if (!is_image(bgr, w_, h_, 3, 1)) throw Error(RC_EINVAL, "streamoverlay_color must be 8UC3 of the frame size");
        void* d = scratch(bgr.row_bytes() * h_);
        check(rcflow_streamline_display_dev(ctx_, 0, which, (uint8_t*)d, bgr.row_bytes(), nullptr));
        check(rcflow_sync(ctx_, 0));
        copy_out(bgr, d, bgr.row_bytes(), "download display image");
    }
    // a null `flow` view: the field is not wanted on the host; any other must be CV_32FC2 of the frame size
    bool wanted(const Mat& flow) const {
        if (flow.data && !is_image(flow, w_, h_, 2, 4)) throw Error(RC_EINVAL, "flow must be CV_32FC2 of the frame size");
        return flow.data != nullptr;
    }
    // the tail of a frame push: rc 1 primed the stream (no flow yet); otherwise the analysis calls read the stream's
    // resident field from here on, and `flow` (when given) receives it
    bool pushed(int rc, Mat* flow) {
        check(rc);
        if (rc == 1) return false;
        float* d = nullptr;
        check(rcflow_stream_flow_ptr(ctx_, 0, &d, nullptr, nullptr));
        flow_src_ = d;
        if (flow) check(rcflow_stream_flow_read(ctx_, 0, (float*)flow->data, flow->step));
        return true;
    }
    // prev above next in d_frames_, for the two-image calls
    void require_pair(const Mat& prev, const Mat& next, const char* who) const {
        if (!is_image(prev, w_, h_, 1, 1) || !is_image(next, w_, h_, 1, 1))
            throw Error(RC_EINVAL, std::string(who) + ": prev/next must be 8UC1 of the pipeline's size");
    }
    uint8_t* upload_pair(const Mat& prev, const Mat& next) {
        uint8_t* df = d_frames_.ptr<uint8_t>();
        copy_in(df, w_, prev, "upload prev");
        copy_in(df + (size_t)w_ * h_, w_, next, "upload next");
        return df;
    }
    // declared first, so destroyed last: the buffers below are freed, then the context
    struct Context {
        rc_ctx* p = nullptr;
        ~Context() { if (p) rcflow_destroy(p); }
        operator rc_ctx*() const { return p; }
    } ctx_;
    int w_, h_;
    DeviceImage d_frames_, d_flow_, d_mask_, d_edges_;
    void* d_scratch_ = nullptr;
    size_t scratch_bytes_ = 0;
    const float* flow_src_ = nullptr;     // the field the analysis calls read: d_flow_ or the stream's resident field
};

// The reference's sparse mover: PyrLK with 50x50, maxLevel 3, COUNT+EPS 30 / 0.1, flags 10, 1e-4 (Streakline.cpp:32,
// ripcurrents_module.cpp:775, :1162).  Returns where `pts` went.
inline std::vector<Pixel2> track_lk(Pipeline& pipe, const Mat& u_prev, const Mat& u_current, const std::vector<Pixel2>& pts) {
    std::vector<Pixel2> next;
    std::vector<unsigned char> status;
    std::vector<float> err;
    pipe.calcOpticalFlowPyrLK(u_prev, u_current, pts, next, status, err, 50, 50, 3, 3, 30, 0.1, 10, 1e-4);
    return next;
}

// Streakline.hpp:8-20.  run(): runLK's bookkeeping (Streakline.cpp:22-71) with the vertices moved
// through the dense flow field resident in the pipeline (the main.cpp:961-977 precedent);
// runLK(): the same with the reference's own mover, sparse PyrLK.  Drawing stays with the caller (rc::Tracers keeps the
// vertices on the device and draws there).
class Streakline {
  public:
    int numberOfVertices;
    Pixel2 generationPoint;
    std::vector<Pixel2> vertices;
    int frameCount;

    explicit Streakline(Pixel2 pixel) : numberOfVertices(1), generationPoint(pixel), frameCount(1) {
        vertices.push_back(pixel);
    }

    void run(Pipeline& pipe, float dt = 1.f) {
        std::vector<Pixel2> next = vertices;
        pipe.streamline(next.data(), (int)next.size(), dt, 1, 0.f, /*variant=*/4);
        advance(pipe, next);
    }

    // Streakline::runLK(u_prev, u_current, outImg) as the reference runs it: the vertices are
    // moved by PyrLK (track_lk).
    void runLK(Pipeline& pipe, const Mat& u_prev, const Mat& u_current) { advance(pipe, track_lk(pipe, u_prev, u_current, vertices)); }

  private:
    // runLK's bookkeeping after the move (Streakline.cpp:35-48)
    void advance(Pipeline& pipe, std::vector<Pixel2> next) {
        for (size_t i = 0; i < next.size(); i++)   // eliminate any large movement (Streakline.cpp:35-40)
            if (std::fabs(vertices[i].x - next[i].x) > pipe.width() * 0.1 ||
                std::fabs(vertices[i].y - next[i].y) > pipe.height() * 0.1)
                next[i] = vertices[i];
        vertices = next;
        vertices.insert(vertices.begin(), generationPoint);   // frameCount % 1 == 0 (Streakline.cpp:46-48)
        numberOfVertices = (int)vertices.size();
        frameCount++;
    }
};

// Timeline (ripcurrents.hpp:64-75, ripcurrents_module.cpp:751-807) and PopulationMap
// (ripcurrents.hpp:86-95, ripcurrents_module.cpp:1140-1196): point sets moved by sparse PyrLK with the
// parameters of :775 / :1162; every vertex takes its tracked position.  Drawing stays with the caller.
class Timeline {
  public:
    std::vector<Pixel2> vertices;
    Timeline(Pixel2 lineStart, Pixel2 lineEnd, int numberOfVertices) {
        float diffX = (lineEnd.x - lineStart.x) / numberOfVertices, diffY = (lineEnd.y - lineStart.y) / numberOfVertices;
        for (int i = 0; i <= numberOfVertices; i++) vertices.push_back(Pixel2{lineStart.x + diffX * i, lineStart.y + diffY * i});
    }
    void runLK(Pipeline& pipe, const Mat& u_prev, const Mat& u_current) { vertices = track_lk(pipe, u_prev, u_current, vertices); }
};

class PopulationMap {
  public:
    std::vector<Pixel2> vertices;
    // `unit_random` returns u in [0, 1] (the reference calls sranddev(); rand() / RAND_MAX); the
    // reference's formula start + (end - start) * (u + 1) is kept as written.
    template <class Rng>
    PopulationMap(Pixel2 rectStart, Pixel2 rectEnd, int numberOfVertices, Rng&& unit_random) {
        for (int i = 0; i < numberOfVertices; i++) {
            float randX = (float)((rectEnd.x - rectStart.x) * ((double)unit_random() + 1) + rectStart.x);
            float randY = (float)((rectEnd.y - rectStart.y) * ((double)unit_random() + 1) + rectStart.y);
            vertices.push_back(Pixel2{randX, randY});
        }
    }
    void runLK(Pipeline& pipe, const Mat& u_prev, const Mat& u_current) { vertices = track_lk(pipe, u_prev, u_current, vertices); }
};

// The opposing-flow map (rcflow_ripmap_*): averageVector (ripcurrents.hpp, ripcurrents_module.cpp:386-484) finished.  Works
// on the flow field resident in the pipeline: push() after calcOpticalFlowFarneback / pushFrame / loopStep, or
// push(flow) with a host field.  One launch per push, nothing waits until read().
class RipMap {
  public:
    struct Cell { float mean_x, mean_y, angle, opposed; };
    struct Result {
        std::vector<Cell> cells;            // grid_y x grid_x
        std::vector<long long> sums;        // grid_y x grid_x x (Sx, Sy, n)
        double direction = 0, mean_magnitude = 0, max_magnitude = 0;
        long long opposed_cells = 0, live_cells = 0, bad_pixels = 0, frames_pushed = 0;
        int grid_x = 0, grid_y = 0;
        bool opposed(int cx, int cy) const { return cells[(size_t)cy * grid_x + cx].opposed != 0.f; }
    };

    RipMap(Pipeline& pipe, int window = 300, int grid_x = 30, int grid_y = 30, int source = 0, int flags = 0)
        : pipe_(pipe), gx_(grid_x), gy_(grid_y) {
        check(rcflow_ripmap_open(pipe.context(), 0, pipe.width(), pipe.height(), window, grid_x, grid_y, source, flags));
    }
    ~RipMap() { (void)rcflow_ripmap_close(pipe_.context(), 0); }
    RipMap(const RipMap&) = delete;
    RipMap& operator=(const RipMap&) = delete;

    void set(double min_opposition_cos2, double min_cell_mag) {
        check(rcflow_ripmap_set(pipe_.context(), 0, min_opposition_cos2, min_cell_mag));
    }
    // the pipeline's resident flow field
    void push() { check(rcflow_ripmap_push_dev(pipe_.context(), 0, pipe_.device_flow(), (size_t)pipe_.width() * 8, nullptr, 0, nullptr, 0, nullptr, nullptr)); }
    // a host field (CV_32FC2 of the pipeline's size)
    void push(const Mat& flow) {
        if (!is_image(flow, pipe_.width(), pipe_.height(), 2, 4))
            throw Error(RC_EINVAL, "RipMap::push: flow must be CV_32FC2 of the pipeline's size");
        staged(pipe_.context(), {{d_field_, &flow}}, [&] {
            return rcflow_ripmap_push_dev(pipe_.context(), 0, d_field_.ptr<const float>(), d_field_.pitch(), nullptr, 0, nullptr, 0, nullptr, nullptr);
        }, {});
    }
    // waits for the pipeline's stream
    Result read() {
        Result r;
        r.grid_x = gx_; r.grid_y = gy_;
        r.cells.resize((size_t)gx_ * gy_);
        r.sums.resize((size_t)gx_ * gy_ * 3);
        double s[8];
        check(rcflow_ripmap_read(pipe_.context(), 0, (float*)r.cells.data(), s, r.sums.data(), &r.frames_pushed));
        r.direction = s[0]; r.mean_magnitude = s[1]; r.opposed_cells = (long long)s[2]; r.live_cells = (long long)s[3];
        r.bad_pixels = (long long)s[4]; r.max_magnitude = s[6];
        return r;
    }
    // 8UC1 of the frame size, 255 inside the cells the last push found opposed: what create_edges / create_output take
    void mask(Mat& m) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(m, w, h, 1, 1)) throw Error(RC_EINVAL, "RipMap::mask: the mask must be 8UC1 of the pipeline's size");
        Result r = read();
        for (int y = 0; y < h; y++) {
            unsigned char* row = (unsigned char*)m.data + (size_t)y * m.step;
            const int cy = std::min(y / (h / gy_), gy_ - 1);
            for (int x = 0; x < w; x++) row[x] = r.opposed(std::min(x / (w / gx_), gx_ - 1), cy) ? 255 : 0;
        }
    }
    void reset() { check(rcflow_ripmap_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int gx_, gy_;
    DeviceImage d_field_;
};

// Tracer lines on the device (rcflow_tracers_*): compute_streaklines / compute_timelines / compute_populationMap
// (main.cpp:78-176) with every vertex resident, moved once per push and drawn into the caller's frame by the library.
// Host images in, host images out, as the rest of this class family; nothing is read back but the frame.
class Tracers {
  public:
    // mover RC_TRACERS_LK: the reference's PyrLK call (Streakline.cpp:32); RC_TRACERS_FLOW: one step of the flow field
    // resident in the pipeline with dt
    Tracers(Pipeline& pipe, int mover = RC_TRACERS_LK, int max_lines = 16, int max_vertices = 1024, float dt = 1.f) : pipe_(pipe) {
        rc_tracers_params p{};
        p.mover = mover; p.max_lines = max_lines; p.max_vertices = max_vertices; p.dt = dt;
        check(rcflow_tracers_open(pipe.context(), 0, pipe.width(), pipe.height(), &p));
    }
    ~Tracers() { (void)rcflow_tracers_close(pipe_.context(), 0); }
    Tracers(const Tracers&) = delete;
    Tracers& operator=(const Tracers&) = delete;

    int addStreakline(Pixel2 pixel) { const float xy[2] = {pixel.x, pixel.y}; return checked(rcflow_tracers_add(pipe_.context(), 0, RC_TRACER_STREAK, xy, 1)); }
    // Timeline's constructor arithmetic (ripcurrents_module.cpp:751-762): numberOfVertices + 1 points on the segment
    int addTimeline(Pixel2 lineStart, Pixel2 lineEnd, int numberOfVertices) {
        const float diffX = (lineEnd.x - lineStart.x) / (float)numberOfVertices, diffY = (lineEnd.y - lineStart.y) / (float)numberOfVertices;
        std::vector<float> xy;
        for (int i = 0; i <= numberOfVertices; i++) { xy.push_back(lineStart.x + diffX * (float)i); xy.push_back(lineStart.y + diffY * (float)i); }
        return checked(rcflow_tracers_add(pipe_.context(), 0, RC_TRACER_TIMELINE, xy.data(), numberOfVertices + 1));
    }
    int addCloud(const std::vector<Pixel2>& pts) {
        std::vector<float> xy;
        for (const Pixel2& p : pts) { xy.push_back(p.x); xy.push_back(p.y); }
        return checked(rcflow_tracers_add(pipe_.context(), 0, RC_TRACER_CLOUD, xy.data(), (int)pts.size()));
    }
    // LK mover: the gray frame (8UC1) moves the lines; outImg (8UC3, optional) gets them drawn, as runLK(u_prev, u_current, outImg)
    // does.  Returns false from the priming push (the first frame).
    bool push(const Mat& gray, Mat* outImg = nullptr) {
        if (!is_image(gray, pipe_.width(), pipe_.height(), 1, 1))
            throw Error(RC_EINVAL, "Tracers::push: the frame must be 8UC1 of the pipeline's size");
        return run(&gray, outImg);
    }
    // FLOW mover: the pipeline's resident flow field
    bool push(Mat* outImg = nullptr) { return run(nullptr, outImg); }
    // waits for the pipeline's stream; the reference's order (a streakline newest first)
    std::vector<Pixel2> vertices(int line) {
        int n = 0;
        check(rcflow_tracers_read(pipe_.context(), 0, line, nullptr, 0, &n, nullptr));
        std::vector<float> xy((size_t)2 * (n > 0 ? n : 1));
        check(rcflow_tracers_read(pipe_.context(), 0, line, xy.data(), n, &n, nullptr));
        std::vector<Pixel2> v;
        for (int i = 0; i < n; i++) v.push_back(Pixel2{xy[2 * i], xy[2 * i + 1]});
        return v;
    }
    rc_tracers_info info() { rc_tracers_info i; check(rcflow_tracers_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_tracers_reset(pipe_.context(), 0)); }

  private:
    static int checked(int rc) { check(rc); return rc; }
    bool run(const Mat* gray, Mat* outImg) {
        if (outImg && !is_image(*outImg, pipe_.width(), pipe_.height(), 3, 1))
            throw Error(RC_EINVAL, "Tracers::push: outImg must be 8UC3 of the pipeline's size");
        return staged(pipe_.context(), {{d_gray_, gray}, {d_canvas_, outImg}}, [&] {
            return rcflow_tracers_push_dev(pipe_.context(), 0, d_gray_.ptr<const uint8_t>(gray), d_gray_.pitch(), nullptr, 0,
                                           d_canvas_.ptr<uint8_t>(outImg), d_canvas_.pitch());
        }, {{d_canvas_, outImg}}) == 0;
    }
    Pipeline& pipe_;
    DeviceImage d_gray_, d_canvas_;
};

// Rip regions on the device (rcflow_regions_*): the connected components of a mask (outmask of the classification, the
// opposing-flow map's mask) numbered in raster order, filtered by area and measured.  Host images in, host images and
// records out, as the rest of this class family.
class Regions {
  public:
    Regions(Pipeline& pipe, int connectivity = 8, int min_area = 1, int max_regions = 1024) : pipe_(pipe), max_regions_(max_regions) {
        rc_regions_params p{};
        p.connectivity = connectivity; p.min_area = min_area; p.max_regions = max_regions;
        check(rcflow_regions_open(pipe.context(), 0, pipe.width(), pipe.height(), &p));
    }
    ~Regions() { (void)rcflow_regions_close(pipe_.context(), 0); }
    Regions(const Regions&) = delete;
    Regions& operator=(const Regions&) = delete;

    // mask: 8UC1 of the pipeline's size, non-zero is foreground.  with_flow: the pipeline's resident flow field gives the
    // records their flow sums.  labels (32SC1, optional) and maskOut (8UC1, optional; may be `mask`) are filled when given.
    void push(const Mat& mask, bool with_flow = false, Mat* labels = nullptr, Mat* maskOut = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(mask, w, h, 1, 1)) throw Error(RC_EINVAL, "Regions::push: the mask must be 8UC1 of the pipeline's size");
        if (labels && !is_image(*labels, w, h, 1, 4)) throw Error(RC_EINVAL, "Regions::push: labels must be 32SC1 of the pipeline's size");
        if (maskOut && !is_image(*maskOut, w, h, 1, 1)) throw Error(RC_EINVAL, "Regions::push: maskOut must be 8UC1 of the pipeline's size");
        if (with_flow && !pipe_.device_flow()) throw Error(RC_ESTATE, "Regions::push: the pipeline holds no flow field");
        // maskOut is written in place, through the mask's own staging image
        staged(pipe_.context(), {{d_mask_, &mask}}, [&] {
            return rcflow_regions_push_dev(pipe_.context(), 0, d_mask_.ptr<const uint8_t>(), d_mask_.pitch(), with_flow ? pipe_.device_flow() : nullptr,
                                           (size_t)w * 8, d_labels_.ptr<int32_t>(labels), d_labels_.pitch(),
                                           d_mask_.ptr<uint8_t>(maskOut), d_mask_.pitch(), nullptr, nullptr);
        }, {{d_labels_, labels}, {d_mask_, maskOut}});
    }
    // waits for the pipeline's stream: the records of the last push, in order; summary (optional): the 8 words of include/rcflow.h
    std::vector<rc_region> regions(long long* summary = nullptr) {
        std::vector<rc_region> r((size_t)max_regions_);
        int n = 0;
        check(rcflow_regions_read(pipe_.context(), 0, r.data(), max_regions_, &n, summary));
        r.resize((size_t)n);
        return r;
    }
    // paints the boxes, centroids and (flow_scale != 0) mean-flow lines of the last push into img (8UC3)
    void draw(Mat& img, uint32_t color = 0x00ffff, int thickness = 1, int disc_radius = 3, double flow_scale = 0.) {
        if (!is_image(img, pipe_.width(), pipe_.height(), 3, 1)) throw Error(RC_EINVAL, "Regions::draw: img must be 8UC3 of the pipeline's size");
        staged_draw(pipe_.context(), d_canvas_, d_prims_, 6 * max_regions_, img, [&](rc_draw_prim* prims) {
            return rcflow_regions_prims_dev(pipe_.context(), 0, color, thickness, disc_radius, flow_scale, prims);
        });
    }
    void setMinArea(int min_area) { check(rcflow_regions_set(pipe_.context(), 0, min_area)); }
    rc_regions_info info() { rc_regions_info i; check(rcflow_regions_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_regions_reset(pipe_.context(), 0)); }
    int maxRegions() const { return max_regions_; }

  private:
    Pipeline& pipe_;
    int max_regions_;
    DeviceImage d_mask_, d_labels_, d_prims_, d_canvas_;
};

// Rip tracks on the device (rcflow_tracks_*): the regions of a Regions object followed from push to push, with hits, misses
// and confirmation.  push() labels the mask with the Regions state and hands its label image, records and summary to the
// tracks without any of them leaving the device.  Host images in, host images and records out.
class Tracks {
  public:
    Tracks(Pipeline& pipe, Regions& regions, int max_tracks = 64, int min_overlap = 1, int max_misses = 2, int min_hits = 3)
        : pipe_(pipe), max_regions_(std::min(regions.maxRegions(), RC_TRACKS_MAX_REGIONS)), rg_records_(regions.maxRegions()), max_tracks_(max_tracks) {
        rc_tracks_params p{};
        p.max_regions = max_regions_; p.max_tracks = max_tracks; p.min_overlap = min_overlap; p.max_misses = max_misses; p.min_hits = min_hits;
        check(rcflow_tracks_open(pipe.context(), 0, pipe.width(), pipe.height(), &p));
    }
    ~Tracks() { (void)rcflow_tracks_close(pipe_.context(), 0); }
    Tracks(const Tracks&) = delete;
    Tracks& operator=(const Tracks&) = delete;

    // mask: 8UC1 of the pipeline's size, non-zero is foreground: one regions push and one tracks push.  with_flow: the
    // pipeline's resident flow field gives regions and tracks their flow sums.  maskOut (8UC1, optional; may be `mask`): 255
    // inside the regions of confirmed tracks.
    void push(const Mat& mask, bool with_flow = false, Mat* maskOut = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(mask, w, h, 1, 1)) throw Error(RC_EINVAL, "Tracks::push: the mask must be 8UC1 of the pipeline's size");
        if (maskOut && !is_image(*maskOut, w, h, 1, 1)) throw Error(RC_EINVAL, "Tracks::push: maskOut must be 8UC1 of the pipeline's size");
        if (with_flow && !pipe_.device_flow()) throw Error(RC_ESTATE, "Tracks::push: the pipeline holds no flow field");
        d_labels_.reserve(w, h, 1, 4);
        d_records_.reserve(rg_records_, 1, 1, (int)sizeof(rc_region));
        d_summary_.reserve(8, 1, 1, 8);
        staged(pipe_.context(), {{d_mask_, &mask}}, [&] {
            const int rc = rcflow_regions_push_dev(pipe_.context(), 0, d_mask_.ptr<const uint8_t>(), d_mask_.pitch(),
                                                   with_flow ? pipe_.device_flow() : nullptr, (size_t)w * 8, d_labels_.ptr<int32_t>(), d_labels_.pitch(),
                                                   nullptr, 0, d_records_.ptr<rc_region>(), d_summary_.ptr<long long>());
            if (rc < 0) return rc;
            return rcflow_tracks_push_dev(pipe_.context(), 0, d_labels_.ptr<const int32_t>(), d_labels_.pitch(), d_records_.ptr<const rc_region>(),
                                          d_summary_.ptr<const long long>(), nullptr, nullptr, d_out_.ptr<uint8_t>(maskOut), d_out_.pitch(),
                                          nullptr);
        }, {{d_out_, maskOut}});
    }
    // waits for the pipeline's stream: the used slots of the table after the last push, in slot order; summary (optional):
    // the 8 words of include/rcflow.h; footprint (optional): h * w words, slot + 1 of the track that last covered the pixel
    std::vector<rc_track> tracks(long long* summary = nullptr, std::vector<int32_t>* footprint = nullptr) {
        std::vector<rc_track> t((size_t)max_tracks_), usedSlots;
        if (footprint) footprint->resize((size_t)pipe_.width() * pipe_.height());
        check(rcflow_tracks_read(pipe_.context(), 0, t.data(), max_tracks_, footprint ? footprint->data() : nullptr, summary));
        for (const rc_track& q : t) if (q.id) usedSlots.push_back(q);
        return usedSlots;
    }
    // paints the boxes and centroids of the confirmed tracks into img (8UC3)
    void draw(Mat& img, uint32_t color = 0x00ffff, int thickness = 1, int disc_radius = 3) {
        if (!is_image(img, pipe_.width(), pipe_.height(), 3, 1)) throw Error(RC_EINVAL, "Tracks::draw: img must be 8UC3 of the pipeline's size");
        staged_draw(pipe_.context(), d_canvas_, d_prims_, 5 * max_tracks_, img, [&](rc_draw_prim* prims) {
            return rcflow_tracks_prims_dev(pipe_.context(), 0, color, thickness, disc_radius, prims);
        });
    }
    rc_tracks_info info() { rc_tracks_info i; check(rcflow_tracks_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_tracks_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int max_regions_, rg_records_, max_tracks_;
    DeviceImage d_mask_, d_labels_, d_records_, d_summary_, d_out_, d_prims_, d_canvas_;
};

// Motion templates on the device (rcflow_motion_*): globalOrientation (ripcurrents.hpp, ripcurrents_module.cpp:319-359) with
// a history that lives from push to push; fresh = true is the reference's literal call (the history zeroed before every
// update).  Host gray frames in; the direction, the per-cell records and the picture out.
class MotionTemplates {
  public:
    // the reference's numbers; its arrows every 30 px are grid (width / 30, height / 30)
    MotionTemplates(Pipeline& pipe, int diff_threshold = 30, double duration = 1., double delta1 = 0.25, double delta2 = 1., int grid_x = 1,
                    int grid_y = 1, bool fresh = false)
        : pipe_(pipe), cells_(grid_x * grid_y) {
        rc_motion_params p{};
        p.diff_threshold = diff_threshold; p.duration = duration; p.delta1 = delta1; p.delta2 = delta2;
        p.grid_x = grid_x; p.grid_y = grid_y; p.flags = fresh ? RC_MOTION_FRESH : 0;
        check(rcflow_motion_open(pipe.context(), 0, pipe.width(), pipe.height(), &p));
    }
    ~MotionTemplates() { (void)rcflow_motion_close(pipe_.context(), 0); }
    MotionTemplates(const MotionTemplates&) = delete;
    MotionTemplates& operator=(const MotionTemplates&) = delete;

    // gray: 8UC1 of the pipeline's size.  picture (8UC3, optional): the history as a grey image (hist_gray of :333).
    void push(const Mat& gray, double timestamp = RC_MOTION_AUTO_TIME, Mat* picture = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(gray, w, h, 1, 1)) throw Error(RC_EINVAL, "MotionTemplates::push: the frame must be 8UC1 of the pipeline's size");
        if (picture && !is_image(*picture, w, h, 3, 1))
            throw Error(RC_EINVAL, "MotionTemplates::push: the picture must be 8UC3 of the pipeline's size");
        staged(pipe_.context(), {{d_gray_, &gray}}, [&] {
            return rcflow_motion_push_dev(pipe_.context(), 0, d_gray_.ptr<const uint8_t>(), d_gray_.pitch(), timestamp, nullptr, 0, nullptr, 0, nullptr, 0,
                                          d_vis_.ptr<uint8_t>(picture), d_vis_.pitch(), nullptr, nullptr);
        }, {{d_vis_, picture}});
    }
    // waits for the pipeline's stream: the frame's record of the last push; cells (optional): grid_y x grid_x records
    rc_motion_cell read(std::vector<rc_motion_cell>* cells = nullptr, long long* silhouette = nullptr) {
        rc_motion_cell f;
        if (cells) cells->resize((size_t)cells_);
        check(rcflow_motion_read(pipe_.context(), 0, cells ? cells->data() : nullptr, cells ? cells_ : 0, &f, silhouette));
        return f;
    }
    // degrees in [0, 360), x to the right, y down
    double angle() { return read().angle; }
    // paints a disc and a line of `length` pixels per cell and for the frame into img (8UC3); no arrowheads
    void draw(Mat& img, uint32_t color = 0x00ffff, int thickness = 1, int disc_radius = 2, double length = 15.) {
        if (!is_image(img, pipe_.width(), pipe_.height(), 3, 1))
            throw Error(RC_EINVAL, "MotionTemplates::draw: img must be 8UC3 of the pipeline's size");
        // d_vis_ serves push's picture and this canvas: both 8UC3 of the pipeline's size, never in use at once
        staged_draw(pipe_.context(), d_vis_, d_prims_, 2 * (cells_ + 1), img, [&](rc_draw_prim* prims) {
            return rcflow_motion_prims_dev(pipe_.context(), 0, color, thickness, disc_radius, length, prims);
        });
    }
    rc_motion_info info() { rc_motion_info i; check(rcflow_motion_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_motion_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int cells_;
    DeviceImage d_gray_, d_vis_, d_prims_;
};


// Flow map and FTLE on the device (rcflow_ftle_*): a ring of the last `window` flow fields, a particle from every pixel
// carried through them, the largest eigenvalue of the Cauchy-Green tensor and its logarithm per frame.  Backward (the
// default) its ridges are where the water gathers.  Host flow fields in; the exponent, the mask and the picture out.
class Ftle {
  public:
    Ftle(Pipeline& pipe, int window = 30, int direction = RC_FTLE_BACKWARD, float dt = 1.f, int spacing = 1, double threshold = 0.1,
         double vis_max = 0.5)
        : pipe_(pipe) {
        rc_ftle_params p{};
        p.window = window; p.direction = direction; p.dt = dt; p.spacing = spacing; p.threshold = threshold; p.vis_max = vis_max;
        check(rcflow_ftle_open(pipe.context(), 0, pipe.width(), pipe.height(), &p));
    }
    ~Ftle() { (void)rcflow_ftle_close(pipe_.context(), 0); }
    Ftle(const Ftle&) = delete;
    Ftle& operator=(const Ftle&) = delete;

    // flow: 32FC2 of the pipeline's size.  Each output is optional: ftle 32FC1, mask 8UC1 (255 / 0), picture 8UC3 (JET).
    // Without any the field only enters the ring (one launch).
    void push(const Mat& flow, Mat* ftle = nullptr, Mat* mask = nullptr, Mat* picture = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(flow, w, h, 2, 4)) throw Error(RC_EINVAL, "Ftle::push: the field must be 32FC2 of the pipeline's size");
        if ((ftle && !is_image(*ftle, w, h, 1, 4)) || (mask && !is_image(*mask, w, h, 1, 1)) || (picture && !is_image(*picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Ftle::push: ftle 32FC1, mask 8UC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_flow_, &flow}}, [&] {
            return rcflow_ftle_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(), d_flow_.pitch(), nullptr, 0, nullptr, 0, nullptr, 0,
                                        d_ftle_.ptr<float>(ftle), d_ftle_.pitch(), d_mask_.ptr<uint8_t>(mask), d_mask_.pitch(),
                                        d_vis_.ptr<uint8_t>(picture), d_vis_.pitch(), nullptr);
        }, {{d_ftle_, ftle}, {d_mask_, mask}, {d_vis_, picture}});
    }
    // waits for the pipeline's stream: the summary of the last push that had an output (include/rcflow.h: n, valid, mask,
    // stopped, bits of the largest eigenvalue, pushes, 0, 0)
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_ftle_read(pipe_.context(), 0, s.data()));
        return s;
    }
    void set(double threshold, double vis_max) { check(rcflow_ftle_set(pipe_.context(), 0, threshold, vis_max)); }
    rc_ftle_info info() { rc_ftle_info i; check(rcflow_ftle_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_ftle_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    DeviceImage d_flow_, d_ftle_, d_mask_, d_vis_;
};

// Plan view on the device (rcflow_planview_*): the flow field in metres per second, and the frame, on a regular grid on the
// water, through the camera's ground-to-image map and its radial distortion.  Host fields and frames of the pipeline's size
// in; the plan field, its mask and the plan picture (each nx x ny of the parameters) out.
class PlanView {
  public:
    PlanView(Pipeline& pipe, const rc_planview_params& prm) : pipe_(pipe), nx_(prm.nx), ny_(prm.ny) {
        check(rcflow_planview_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~PlanView() { (void)rcflow_planview_close(pipe_.context(), 0); }
    PlanView(const PlanView&) = delete;
    PlanView& operator=(const PlanView&) = delete;

    // flow: 32FC2, frame: 8UC3, each of the pipeline's size; either may be null, not both.  plan 32FC2 and mask 8UC1 (255 / 0)
    // need the field, picture 8UC3 the frame; each nx x ny and optional.
    void push(const Mat* flow, const Mat* frame, Mat* plan = nullptr, Mat* mask = nullptr, Mat* picture = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if ((flow && !is_image(*flow, w, h, 2, 4)) || (frame && !is_image(*frame, w, h, 3, 1)) || (!flow && !frame))
            throw Error(RC_EINVAL, "PlanView::push: the field 32FC2, the frame 8UC3, each of the pipeline's size, and one of them at least");
        if ((plan && !is_image(*plan, nx_, ny_, 2, 4)) || (mask && !is_image(*mask, nx_, ny_, 1, 1)) || (picture && !is_image(*picture, nx_, ny_, 3, 1)) ||
            (!flow && (plan || mask)) || (!frame && picture))
            throw Error(RC_EINVAL, "PlanView::push: plan 32FC2 and mask 8UC1 need the field, picture 8UC3 the frame, each of the plan's size");
        staged(pipe_.context(), {{d_flow_, flow}, {d_bgr_, frame}}, [&] {
            return rcflow_planview_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(flow), d_flow_.pitch(),
                                            d_bgr_.ptr<const uint8_t>(frame), d_bgr_.pitch(),
                                            d_plan_.ptr<float>(plan), d_plan_.pitch(), d_mask_.ptr<uint8_t>(mask), d_mask_.pitch(),
                                            d_pic_.ptr<uint8_t>(picture), d_pic_.pitch(), nullptr);
        }, {{d_plan_, plan}, {d_mask_, mask}, {d_pic_, picture}});
    }
    // waits for the pipeline's stream: the summary of the last push (include/rcflow.h: usable, seen, valid, bits of the
    // largest squared speed, pushes, 0, 0, 0)
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_planview_read(pipe_.context(), 0, s.data()));
        return s;
    }
    // waits: ny x nx records of eight floats (U, V, m00, m01, m10, m11, gsd, 1; zeros where the cell is not usable)
    std::vector<float> table() {
        std::vector<float> t((size_t)nx_ * ny_ * 8);
        check(rcflow_planview_table_read(pipe_.context(), 0, t.data()));
        return t;
    }
    rc_planview_info info() { rc_planview_info i; check(rcflow_planview_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_planview_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int nx_, ny_;
    DeviceImage d_flow_, d_bgr_, d_plan_, d_mask_, d_pic_;
};

// Wave spectra on the device (rcflow_waves_*): a sliding DFT of the last `window` grey frames at a few bins per pixel, and per
// grid cell the strongest bin, its wavenumber, the celerity and the depth.  Host grey frames of the pipeline's size in; the
// cells' records, the bin map and the depth picture out.
class Waves {
  public:
    Waves(Pipeline& pipe, const rc_waves_params& prm) : pipe_(pipe) {
        check(rcflow_waves_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
        rc_waves_info i;
        try {
            check(rcflow_waves_info(pipe.context(), 0, &i));
        } catch (...) {                                          // no destructor runs: close what was opened
            (void)rcflow_waves_close(pipe.context(), 0);
            throw;
        }
        cells_ = (size_t)prm.grid_x * prm.grid_y;
        bins_ = i.bins;
    }
    ~Waves() { (void)rcflow_waves_close(pipe_.context(), 0); }
    Waves(const Waves&) = delete;
    Waves& operator=(const Waves&) = delete;

    // gray: 8UC1 of the pipeline's size; mask (8UC1, optional) limits the pixels that take part.  Each output is optional:
    // bin_map 8UC1, picture 8UC3 (JET of the depth); compute asks for records, sums and summary, which read() and cells()
    // then return.  Without any the frame only enters the ring and the spectrum (one launch).
    void push(const Mat& gray, const Mat* mask = nullptr, bool compute = false, Mat* bin_map = nullptr, Mat* picture = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(gray, w, h, 1, 1) || (mask && !is_image(*mask, w, h, 1, 1)))
            throw Error(RC_EINVAL, "Waves::push: the frame and the mask must be 8UC1 of the pipeline's size");
        if ((bin_map && !is_image(*bin_map, w, h, 1, 1)) || (picture && !is_image(*picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Waves::push: bin_map 8UC1, picture 8UC3, each of the pipeline's size");
        if (compute) d_summary_.reserve(8, 1, 1, 8);
        staged(pipe_.context(), {{d_gray_, &gray}, {d_mask_, mask}}, [&] {
            return rcflow_waves_push_dev(pipe_.context(), 0, d_gray_.ptr<const uint8_t>(), d_gray_.pitch(), d_mask_.ptr<const uint8_t>(mask),
                                         d_mask_.pitch(), nullptr, nullptr, d_bin_.ptr<uint8_t>(bin_map), d_bin_.pitch(),
                                         d_vis_.ptr<uint8_t>(picture), d_vis_.pitch(), d_summary_.ptr<long long>(compute));
        }, {{d_bin_, bin_map}, {d_vis_, picture}});
    }
    // each waits for the pipeline's stream: of the last push that computed (include/rcflow.h).  The summary: held frames, pixels
    // that take part, cells not empty, cells with a depth, pushes, 0, 0, 0; the records, grid_y x grid_x; the sums,
    // grid_y x grid_x x bins x 6
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_waves_read(pipe_.context(), 0, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_wave_cell> cells() {
        std::vector<rc_wave_cell> c(cells_);
        check(rcflow_waves_read(pipe_.context(), 0, c.data(), nullptr, nullptr));
        return c;
    }
    std::vector<long long> sums() {
        std::vector<long long> s(cells_ * bins_ * 6);
        check(rcflow_waves_read(pipe_.context(), 0, nullptr, s.data(), nullptr));
        return s;
    }
    // waits: the accumulators, bins x rows x cols x (re, im)
    std::vector<int32_t> spectrum() {
        std::vector<int32_t> a((size_t)bins_ * pipe_.width() * pipe_.height() * 2);
        check(rcflow_waves_spectrum_read(pipe_.context(), 0, a.data()));
        return a;
    }
    void set(double tanh_max, int min_pixels, double vis_max_depth) { check(rcflow_waves_set(pipe_.context(), 0, tanh_max, min_pixels, vis_max_depth)); }
    rc_waves_info info() { rc_waves_info i; check(rcflow_waves_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_waves_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    size_t cells_ = 0;
    int bins_ = 0;
    DeviceImage d_gray_, d_mask_, d_bin_, d_vis_, d_summary_;
};

// Ensemble PIV on the device (rcflow_piv_*): block cross-correlation between consecutive grey frames, the correlation sums added
// over the last `ensemble` pairs, on a grid of cells.  Host grey frames of the pipeline's size in; the cells' records, the small
// flow field (grid_y x grid_x, 32FC2) and the picture out.
class Piv {
  public:
    Piv(Pipeline& pipe, const rc_piv_params& prm) : pipe_(pipe) {
        check(rcflow_piv_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
        rc_piv_info i;
        try {
            check(rcflow_piv_info(pipe.context(), 0, &i));
        } catch (...) {                                          // no destructor runs: close what was opened
            (void)rcflow_piv_close(pipe.context(), 0);
            throw;
        }
        gx_ = i.grid_x; gy_ = i.grid_y;
        disp_ = (size_t)(2 * prm.range + 1) * (2 * prm.range + 1);
    }
    ~Piv() { (void)rcflow_piv_close(pipe_.context(), 0); }
    Piv(const Piv&) = delete;
    Piv& operator=(const Piv&) = delete;

    int grid_x() const { return gx_; }
    int grid_y() const { return gy_; }

    // gray: 8UC1 of the pipeline's size.  Each output is optional: field 32FC2 of grid_y x grid_x (pixels per frame), picture 8UC3
    // of the pipeline's size (JET of the magnitude); compute asks for records and summary, which read() and cells() then return.
    // Without any the frame is only correlated into the sums (one launch).
    void push(const Mat& gray, bool compute = false, Mat* field = nullptr, Mat* picture = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(gray, w, h, 1, 1)) throw Error(RC_EINVAL, "Piv::push: the frame must be 8UC1 of the pipeline's size");
        if (field && !is_image(*field, gx_, gy_, 2, 4)) throw Error(RC_EINVAL, "Piv::push: field 32FC2 of grid_y x grid_x");
        if (picture && !is_image(*picture, w, h, 3, 1)) throw Error(RC_EINVAL, "Piv::push: picture 8UC3 of the pipeline's size");
        if (compute) d_summary_.reserve(8, 1, 1, 8);
        staged(pipe_.context(), {{d_gray_, &gray}}, [&] {
            return rcflow_piv_push_dev(pipe_.context(), 0, d_gray_.ptr<const uint8_t>(), d_gray_.pitch(), nullptr,
                                       d_field_.ptr<float>(field), d_field_.pitch(), d_vis_.ptr<uint8_t>(picture), d_vis_.pitch(),
                                       d_summary_.ptr<long long>(compute));
        }, {{d_field_, field}, {d_vis_, picture}});
    }
    // each waits for the pipeline's stream: of the last push that computed (include/rcflow.h).  The summary: pairs summed, cells,
    // valid, flat, low peak, edge, outliers, pushes; the records, grid_y x grid_x
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_piv_read(pipe_.context(), 0, nullptr, s.data()));
        return s;
    }
    std::vector<rc_piv_cell> cells() {
        std::vector<rc_piv_cell> c((size_t)gx_ * gy_);
        check(rcflow_piv_read(pipe_.context(), 0, c.data(), nullptr));
        return c;
    }
    // waits: the accumulators, grid_y x grid_x x D x D x (Tab, Tb, Tbb); the cells' own, grid_y x grid_x x (Ta, Taa)
    std::vector<long long> sums() {
        std::vector<long long> s((size_t)gx_ * gy_ * disp_ * 3);
        check(rcflow_piv_sums_read(pipe_.context(), 0, s.data(), nullptr));
        return s;
    }
    std::vector<long long> cell_sums() {
        std::vector<long long> s((size_t)gx_ * gy_ * 2);
        check(rcflow_piv_sums_read(pipe_.context(), 0, nullptr, s.data()));
        return s;
    }
    void set(double min_peak, double median_eps, double median_thr, double vis_max) {
        check(rcflow_piv_set(pipe_.context(), 0, min_peak, median_eps, median_thr, vis_max));
    }
    rc_piv_info info() { rc_piv_info i; check(rcflow_piv_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_piv_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int gx_ = 0, gy_ = 0;
    size_t disp_ = 0;
    DeviceImage d_gray_, d_field_, d_vis_, d_summary_;
};

// Transects on the device (rcflow_transects_*): straight lines across the picture, sampled at every push into rings of the last
// `window` rows.  Host grey frames and flow fields of the pipeline's size in, whichever the parameters' sources name; the
// lines' records (drift along the line, transport across it, jets), the window means, the time stack and the Hovmoeller
// picture out.
class Transects {
  public:
    Transects(Pipeline& pipe, const std::vector<rc_transect_line>& lines, const rc_transects_params& prm) : pipe_(pipe) {
        check(rcflow_transects_open(pipe.context(), 0, pipe.width(), pipe.height(), lines.data(), (int)lines.size(), &prm));
        rc_transects_info i;
        try {
            check(rcflow_transects_info(pipe.context(), 0, &i));
        } catch (...) {                                          // no destructor runs: close what was opened
            (void)rcflow_transects_close(pipe.context(), 0);
            throw;
        }
        lines_ = i.lines; samples_ = i.samples; window_ = prm.window; shifts_ = 2 * prm.range + 1;
    }
    ~Transects() { (void)rcflow_transects_close(pipe_.context(), 0); }
    Transects(const Transects&) = delete;
    Transects& operator=(const Transects&) = delete;

    int lines() const { return lines_; }
    int samples() const { return samples_; }

    // gray: 8UC1, flow: 32FC2, both of the pipeline's size; exactly those the session was opened for, the other null.  Each
    // output is optional: profile 32FC2 of 1 x samples (the window means along and across), stack 8UC1 and hov 8UC3 of
    // window x samples; compute asks for records, sums and summary, which read(), records() and line_sums() then return.
    // Without any the frame is only sampled into the rings (one launch).
    void push(const Mat* gray, const Mat* flow, bool compute = false, Mat* profile = nullptr, Mat* stack = nullptr, Mat* hov = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (gray && !is_image(*gray, w, h, 1, 1)) throw Error(RC_EINVAL, "Transects::push: the frame must be 8UC1 of the pipeline's size");
        if (flow && !is_image(*flow, w, h, 2, 4)) throw Error(RC_EINVAL, "Transects::push: the field must be 32FC2 of the pipeline's size");
        if (profile && !is_image(*profile, samples_, 1, 2, 4)) throw Error(RC_EINVAL, "Transects::push: profile 32FC2 of 1 x samples");
        if (stack && !is_image(*stack, samples_, window_, 1, 1)) throw Error(RC_EINVAL, "Transects::push: stack 8UC1 of window x samples");
        if (hov && !is_image(*hov, samples_, window_, 3, 1)) throw Error(RC_EINVAL, "Transects::push: hov 8UC3 of window x samples");
        if (compute) { d_summary_.reserve(8, 1, 1, 8); d_sums_.reserve(RC_TRANSECTS_SUMS, lines_, 1, 8); }
        staged(pipe_.context(), {{d_gray_, gray}, {d_flow_, flow}}, [&] {
            return rcflow_transects_push_dev(pipe_.context(), 0, d_gray_.ptr<const uint8_t>(gray), d_gray_.pitch(), d_flow_.ptr<const float>(flow),
                                             d_flow_.pitch(), nullptr, d_sums_.ptr<long long>(compute), d_profile_.ptr<float>(profile),
                                             d_stack_.ptr<uint8_t>(stack), d_stack_.pitch(), d_hov_.ptr<uint8_t>(hov), d_hov_.pitch(),
                                             d_summary_.ptr<long long>(compute));
        }, {{d_profile_, profile}, {d_stack_, stack}, {d_hov_, hov}});
    }
    // each waits for the pipeline's stream: of the last push that computed (include/rcflow.h).  The summary: rows held, pairs,
    // lines with a velocity, lines with a jet, jets, bad samples, pushes, 0; the records, one per line
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_transects_read(pipe_.context(), 0, nullptr, s.data()));
        return s;
    }
    std::vector<rc_transect> records() {
        std::vector<rc_transect> r((size_t)lines_);
        check(rcflow_transects_read(pipe_.context(), 0, r.data(), nullptr));
        return r;
    }
    // waits: the RC_TRANSECTS_SUMS int64 of every line of the last push that computed
    std::vector<long long> line_sums() {
        std::vector<long long> s((size_t)lines_ * RC_TRANSECTS_SUMS);
        if (d_sums_.pitch()) {
            check(rcflow_sync(pipe_.context(), 0));
            Mat m(lines_, RC_TRANSECTS_SUMS, 1, 8, s.data());
            d_sums_.download(m);
        }
        return s;
    }
    // waits: the accumulators, lines x (2 range + 1) x (Tab, Tb, Tbb)
    std::vector<long long> sums() {
        std::vector<long long> s((size_t)lines_ * shifts_ * 3);
        check(rcflow_transects_sums_read(pipe_.context(), 0, s.data(), nullptr));
        return s;
    }
    // waits: the session's table, one record per sample in line order
    std::vector<rc_transect_sample> table() {
        std::vector<rc_transect_sample> t((size_t)samples_);
        check(rcflow_transects_table_read(pipe_.context(), 0, t.data(), nullptr));
        return t;
    }
    std::vector<rc_transect_geom> geometry() {
        std::vector<rc_transect_geom> g((size_t)lines_);
        check(rcflow_transects_table_read(pipe_.context(), 0, nullptr, g.data()));
        return g;
    }
    void set(double jet_min, double vis_max) { check(rcflow_transects_set(pipe_.context(), 0, jet_min, vis_max)); }
    rc_transects_info info() { rc_transects_info i; check(rcflow_transects_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_transects_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int lines_ = 0, samples_ = 0, window_ = 0, shifts_ = 0;
    DeviceImage d_gray_, d_flow_, d_profile_, d_stack_, d_hov_, d_sums_, d_summary_;
};

// Flow kinematics on the device (rcflow_kinematics_*): vorticity (positive: clockwise on the picture), divergence and the
// Okubo-Weiss parameter of one flow field, the vortex cores and a record per cell of a grid.  Stateless in time.  Host flow
// fields of the pipeline's size in; the planes, the core mask and the picture out.
class Kinematics {
  public:
    Kinematics(Pipeline& pipe, const rc_kinematics_params& prm) : pipe_(pipe), cells_(prm.grid_x * prm.grid_y) {
        check(rcflow_kinematics_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~Kinematics() { (void)rcflow_kinematics_close(pipe_.context(), 0); }
    Kinematics(const Kinematics&) = delete;
    Kinematics& operator=(const Kinematics&) = delete;

    // the taps of the smoothing, g_0..g_radius; needs no GPU
    static std::vector<float> taps(int radius, double sigma) {
        std::vector<float> g((size_t)(radius < 0 ? 0 : radius) + 1);
        check(rcflow_kinematics_taps(radius, sigma, g.data()));
        return g;
    }
    // flow: 32FC2 of the pipeline's size.  Each output is optional: omega, div and ow 32FC1, mask 8UC1 (255 at a core), picture
    // 8UC3 (JET of the vorticity); compute asks for the records, the sums and the summary alone.  Those stay on the session
    // after any push with an output, for read(), cells() and sums().  Without any the push is only counted.
    void push(const Mat& flow, Mat* omega = nullptr, Mat* div = nullptr, Mat* ow = nullptr, Mat* mask = nullptr, Mat* picture = nullptr,
              bool compute = false) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(flow, w, h, 2, 4)) throw Error(RC_EINVAL, "Kinematics::push: the field must be 32FC2 of the pipeline's size");
        if ((omega && !is_image(*omega, w, h, 1, 4)) || (div && !is_image(*div, w, h, 1, 4)) || (ow && !is_image(*ow, w, h, 1, 4)) ||
            (mask && !is_image(*mask, w, h, 1, 1)) || (picture && !is_image(*picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Kinematics::push: omega, div and ow 32FC1, mask 8UC1, picture 8UC3, each of the pipeline's size");
        if (compute) d_summary_.reserve(8, 1, 1, 8);
        staged(pipe_.context(), {{d_flow_, &flow}}, [&] {
            return rcflow_kinematics_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(), d_flow_.pitch(), d_omega_.ptr<float>(omega),
                                              d_omega_.pitch(), d_div_.ptr<float>(div), d_div_.pitch(), d_ow_.ptr<float>(ow), d_ow_.pitch(),
                                              d_mask_.ptr<uint8_t>(mask), d_mask_.pitch(), d_vis_.ptr<uint8_t>(picture), d_vis_.pitch(), nullptr,
                                              nullptr, d_summary_.ptr<long long>(compute));
        }, {{d_omega_, omega}, {d_div_, div}, {d_ow_, ow}, {d_mask_, mask}, {d_vis_, picture}});
    }
    // each waits for the pipeline's stream: of the last push that had an output (include/rcflow.h).  The summary: valid pixels, bad
    // pixels, cores cw, cores ccw, the bits of the squared threshold (a double), cells with both, pushes, the bits of the largest |omega|
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_kinematics_read(pipe_.context(), 0, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_kinematics_cell> cells() {
        std::vector<rc_kinematics_cell> r((size_t)cells_);
        check(rcflow_kinematics_read(pipe_.context(), 0, r.data(), nullptr, nullptr));
        return r;
    }
    std::vector<long long> sums() {
        std::vector<long long> s((size_t)cells_ * RC_KINEMATICS_SUMS);
        check(rcflow_kinematics_read(pipe_.context(), 0, nullptr, s.data(), nullptr));
        return s;
    }
    void set(double ow_k, double ow_min, double omega_min, double vis_max) {
        check(rcflow_kinematics_set(pipe_.context(), 0, ow_k, ow_min, omega_min, vis_max));
    }
    rc_kinematics_info info() { rc_kinematics_info i; check(rcflow_kinematics_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_kinematics_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int cells_ = 0;
    DeviceImage d_flow_, d_omega_, d_div_, d_ow_, d_mask_, d_vis_, d_summary_;
};

// Shoreline on the device (rcflow_shoreline_*): the wet/dry split of a picture, the waterline along lines laid from land to sea
// and its runup statistics over the last `window` pushes.  Host pictures of the pipeline's size in (8UC3, or 8UC1 for
// RC_SHORE_PLANE); the records, the wet mask and the smoothed plane out.
class Shoreline {
  public:
    Shoreline(Pipeline& pipe, const std::vector<rc_transect_line>& lines, const rc_shoreline_params& prm)
        : pipe_(pipe), lines_((int)lines.size()), window_(prm.window), channels_(prm.source == RC_SHORE_PLANE ? 1 : 3) {
        check(rcflow_shoreline_open(pipe.context(), 0, pipe.width(), pipe.height(), lines.data(), (int)lines.size(), &prm));
    }
    ~Shoreline() { (void)rcflow_shoreline_close(pipe_.context(), 0); }
    Shoreline(const Shoreline&) = delete;
    Shoreline& operator=(const Shoreline&) = delete;

    int lines() const { return lines_; }

    // image: 8UC3 (8UC1 for RC_SHORE_PLANE) of the pipeline's size; roi: 8UC1, the histogram counts where it is non-zero.  Each
    // output is optional: mask 8UC1 (255 where wet), plane 16UC1 (the smoothed indicator).  The records and the summary stay on
    // the session after every push, for read() and records().
    void push(const Mat& image, const Mat* roi = nullptr, Mat* mask = nullptr, Mat* plane = nullptr) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(image, w, h, channels_, 1)) throw Error(RC_EINVAL, "Shoreline::push: the picture must be 8UC3 (8UC1 for a plane) of the pipeline's size");
        if ((roi && !is_image(*roi, w, h, 1, 1)) || (mask && !is_image(*mask, w, h, 1, 1)) || (plane && !is_image(*plane, w, h, 1, 2)))
            throw Error(RC_EINVAL, "Shoreline::push: roi and mask 8UC1, plane 16UC1, each of the pipeline's size");
        staged(pipe_.context(), {{d_image_, &image}, {d_roi_, roi}}, [&] {
            return rcflow_shoreline_push_dev(pipe_.context(), 0, d_image_.ptr<const uint8_t>(), d_image_.pitch(), channels_,
                                             d_roi_.ptr<const uint8_t>(roi), d_roi_.pitch(), nullptr, d_mask_.ptr<uint8_t>(mask), d_mask_.pitch(),
                                             d_plane_.ptr<uint16_t>(plane), d_plane_.pitch(), nullptr, nullptr);
        }, {{d_mask_, mask}, {d_plane_, plane}});
    }
    // each waits for the pipeline's stream: of the last push (include/rcflow.h).  The summary: threshold, pixels counted, the
    // separability times 2^32, lines with a position, dry lines, wet lines, outliers, pushes; the records, one per line
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_shoreline_read(pipe_.context(), 0, nullptr, s.data()));
        return s;
    }
    std::vector<rc_shoreline> records() {
        std::vector<rc_shoreline> r((size_t)lines_);
        check(rcflow_shoreline_read(pipe_.context(), 0, r.data(), nullptr));
        return r;
    }
    // waits: the runup time series, lines x window, per line the held positions oldest first, then -1
    std::vector<int> ring() {
        std::vector<int> r((size_t)lines_ * window_);
        check(rcflow_shoreline_ring_read(pipe_.context(), 0, r.data()));
        return r;
    }
    void set(int threshold, double min_sep, double max_jump) { check(rcflow_shoreline_set(pipe_.context(), 0, threshold, min_sep, max_jump)); }
    rc_shoreline_info info() { rc_shoreline_info i; check(rcflow_shoreline_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_shoreline_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int lines_ = 0, window_ = 0, channels_ = 3;
    DeviceImage d_image_, d_roi_, d_mask_, d_plane_;
};

// the pictures of a Surf::push, each optional: now, surf, mean and sd 8UC1, q 16UC1, picture 8UC3
struct SurfPictures { Mat* now = nullptr; Mat* surf = nullptr; Mat* q = nullptr; Mat* mean = nullptr; Mat* sd = nullptr; Mat* picture = nullptr; };

// Surf zone on the device (rcflow_surf_*): per pixel the fraction of the last `window` frames in which it broke, the window mean
// and the variance image; along lines laid from land to sea the band of breaking, and along the shore the rip channels: the
// holes in that band.  Host grey frames (8UC1) of the pipeline's size in; the pictures, the line and the channel records out.
// Without lines the session is pixels only.
class Surf {
  public:
    using Pictures = SurfPictures;

    Surf(Pipeline& pipe, const std::vector<rc_transect_line>& lines, const rc_surf_params& prm) : pipe_(pipe), lines_((int)lines.size()) {
        check(rcflow_surf_open(pipe.context(), 0, pipe.width(), pipe.height(), lines.empty() ? nullptr : lines.data(), (int)lines.size(), &prm));
    }
    ~Surf() { (void)rcflow_surf_close(pipe_.context(), 0); }
    Surf(const Surf&) = delete;
    Surf& operator=(const Surf&) = delete;

    int lines() const { return lines_; }

    // gray: 8UC1 of the pipeline's size.  The records and the summary stay on the session after every push, for read(), records()
    // and channels().
    void push(const Mat& gray, const Pictures& out = Pictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(gray, w, h, 1, 1)) throw Error(RC_EINVAL, "Surf::push: the frame must be 8UC1 of the pipeline's size");
        for (const Mat* m : {out.now, out.surf, out.mean, out.sd})
            if (m && !is_image(*m, w, h, 1, 1)) throw Error(RC_EINVAL, "Surf::push: now, surf, mean and sd 8UC1, each of the pipeline's size");
        if ((out.q && !is_image(*out.q, w, h, 1, 2)) || (out.picture && !is_image(*out.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Surf::push: q 16UC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_gray_, &gray}}, [&] {
            return rcflow_surf_push_dev(pipe_.context(), 0, d_gray_.ptr<const uint8_t>(), d_gray_.pitch(), 1, d_now_.ptr<uint8_t>(out.now), d_now_.pitch(),
                                        d_surf_.ptr<uint8_t>(out.surf), d_surf_.pitch(), d_q_.ptr<uint16_t>(out.q), d_q_.pitch(),
                                        d_mean_.ptr<uint8_t>(out.mean), d_mean_.pitch(), d_sd_.ptr<uint8_t>(out.sd), d_sd_.pitch(),
                                        d_picture_.ptr<uint8_t>(out.picture), d_picture_.pitch(), nullptr, nullptr, nullptr);
        }, {{d_now_, out.now}, {d_surf_, out.surf}, {d_q_, out.q}, {d_mean_, out.mean}, {d_sd_, out.sd}, {d_picture_, out.picture}});
    }
    // each waits for the pipeline's stream: of the last push (include/rcflow.h).  The summary: frames held, pixels breaking now,
    // surf pixels, the sum of Q, lines with a band, channel lines, channels, pushes; the line records, one per line; the
    // recorded channels
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_surf_read(pipe_.context(), 0, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_surf_line> records() {
        std::vector<rc_surf_line> r((size_t)lines_);
        check(rcflow_surf_read(pipe_.context(), 0, r.empty() ? nullptr : r.data(), nullptr, nullptr));
        return r;
    }
    std::vector<rc_surf_channel> channels() {
        std::vector<rc_surf_channel> c(RC_SURF_MAX_CHANNELS);
        long long s[8];
        check(rcflow_surf_read(pipe_.context(), 0, nullptr, c.data(), s));
        c.resize((size_t)std::min<long long>(s[6], RC_SURF_MAX_CHANNELS));
        return c;
    }
    void set(int bright, int delta, int q_min, int ratio, int min_load, int vis_permille) {
        check(rcflow_surf_set(pipe_.context(), 0, bright, delta, q_min, ratio, min_load, vis_permille));
    }
    rc_surf_info info() { rc_surf_info i; check(rcflow_surf_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_surf_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int lines_ = 0;
    DeviceImage d_gray_, d_now_, d_surf_, d_q_, d_mean_, d_sd_, d_picture_;
};

// the pictures of a MeanFlow::push, each optional: mean and stddev (major, minor) 32FC2, steady 16UC1, mask 8UC1, picture 8UC3
struct MeanFlowPictures { Mat* mean = nullptr; Mat* steady = nullptr; Mat* stddev = nullptr; Mat* mask = nullptr; Mat* picture = nullptr; };

// Mean current on the device (rcflow_meanflow_*): per pixel the exact mean of the last `window` flow samples, the steadiness
// |sum of vectors| / sum of magnitudes in per mille, the major and minor standard deviation, and the mask of the pixels that are
// steady, fast enough and run along a direction, or against the picture's own mean vector.  Host flow fields (32FC2) of the
// pipeline's size in; the pictures and a record per cell of a grid out.
class MeanFlow {
  public:
    using Pictures = MeanFlowPictures;

    MeanFlow(Pipeline& pipe, const rc_meanflow_params& prm) : pipe_(pipe), cells_(prm.grid_x * prm.grid_y) {
        check(rcflow_meanflow_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~MeanFlow() { (void)rcflow_meanflow_close(pipe_.context(), 0); }
    MeanFlow(const MeanFlow&) = delete;
    MeanFlow& operator=(const MeanFlow&) = delete;

    // flow: 32FC2 of the pipeline's size.  The records, the sums and the summary stay on the session after every push, for read(),
    // cells() and sums().
    void push(const Mat& flow, const Pictures& out = Pictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(flow, w, h, 2, 4)) throw Error(RC_EINVAL, "MeanFlow::push: the field must be 32FC2 of the pipeline's size");
        if ((out.mean && !is_image(*out.mean, w, h, 2, 4)) || (out.stddev && !is_image(*out.stddev, w, h, 2, 4)) ||
            (out.steady && !is_image(*out.steady, w, h, 1, 2)) || (out.mask && !is_image(*out.mask, w, h, 1, 1)) ||
            (out.picture && !is_image(*out.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "MeanFlow::push: mean and std 32FC2, steady 16UC1, mask 8UC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_flow_, &flow}}, [&] {
            return rcflow_meanflow_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(), d_flow_.pitch(), d_mean_.ptr<float>(out.mean), d_mean_.pitch(),
                                            d_steady_.ptr<uint16_t>(out.steady), d_steady_.pitch(), d_std_.ptr<float>(out.stddev), d_std_.pitch(),
                                            d_mask_.ptr<uint8_t>(out.mask), d_mask_.pitch(), d_picture_.ptr<uint8_t>(out.picture), d_picture_.pitch(),
                                            nullptr, nullptr, nullptr);
        }, {{d_mean_, out.mean}, {d_steady_, out.steady}, {d_std_, out.stddev}, {d_mask_, out.mask}, {d_picture_, out.picture}});
    }
    // each waits for the pipeline's stream: of the last push (include/rcflow.h).  The summary: filled pixels, mask pixels, pixels
    // whose newest sample was bad, Gx, Gy, the sum of Sm, samples held, pushes
    std::vector<long long> read() {
        std::vector<long long> s(8);
        check(rcflow_meanflow_read(pipe_.context(), 0, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_meanflow_cell> cells() {
        std::vector<rc_meanflow_cell> r((size_t)cells_);
        check(rcflow_meanflow_read(pipe_.context(), 0, r.data(), nullptr, nullptr));
        return r;
    }
    std::vector<long long> sums() {
        std::vector<long long> s((size_t)cells_ * RC_MEANFLOW_SUMS);
        check(rcflow_meanflow_read(pipe_.context(), 0, nullptr, s.data(), nullptr));
        return s;
    }
    void set(int steady_min, double speed_min, double min_cos2, double dir_x, double dir_y, int min_fill) {
        check(rcflow_meanflow_set(pipe_.context(), 0, steady_min, speed_min, min_cos2, dir_x, dir_y, min_fill));
    }
    rc_meanflow_info info() { rc_meanflow_info i; check(rcflow_meanflow_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_meanflow_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int cells_ = 0;
    DeviceImage d_flow_, d_mean_, d_steady_, d_std_, d_mask_, d_picture_;
};

// the pictures of a FlowCheck::push, each optional: flags and mask 8UC1, checked and resid 32FC2, texture 32FC1, picture 8UC3
struct FlowCheckPictures {
    Mat* flags = nullptr; Mat* mask = nullptr; Mat* checked = nullptr; Mat* resid = nullptr; Mat* texture = nullptr; Mat* picture = nullptr;
};

// Flow check on the device (rcflow_flowcheck_*): which vectors of a dense field mean anything.  Host grey frames (8UC1) and flow
// fields (32FC2) of the pipeline's size in; per pixel the flags, the mask of the valid pixels and the field with the rejected
// vectors replaced by NaN or zero out, and a record per cell of a grid.
class FlowCheck {
  public:
    using Pictures = FlowCheckPictures;

    FlowCheck(Pipeline& pipe, const rc_flowcheck_params& prm) : pipe_(pipe), cells_(prm.grid_x * prm.grid_y) {
        check(rcflow_flowcheck_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~FlowCheck() { (void)rcflow_flowcheck_close(pipe_.context(), 0); }
    FlowCheck(const FlowCheck&) = delete;
    FlowCheck& operator=(const FlowCheck&) = delete;

    // next: 8UC1; prev: 8UC1, or null for the frame of the push before (the first push then only stores its frame); flow: 32FC2 from
    // prev to next; back: 32FC2 from next to prev, or null for no round-trip test.  The records, the sums and the summary stay on
    // the session after every push, for read(), cells() and sums().  The pictures of a push that only stores its frame are left as they were.
    void push(const Mat& next, const Mat* prev, const Mat& flow, const Mat* back = nullptr, const Pictures& asked = Pictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(next, w, h, 1, 1) || (prev && !is_image(*prev, w, h, 1, 1)))
            throw Error(RC_EINVAL, "FlowCheck::push: the frames must be 8UC1 of the pipeline's size");
        if (!is_image(flow, w, h, 2, 4) || (back && !is_image(*back, w, h, 2, 4)))
            throw Error(RC_EINVAL, "FlowCheck::push: the fields must be 32FC2 of the pipeline's size");
        if ((asked.flags && !is_image(*asked.flags, w, h, 1, 1)) || (asked.mask && !is_image(*asked.mask, w, h, 1, 1)) ||
            (asked.checked && !is_image(*asked.checked, w, h, 2, 4)) || (asked.resid && !is_image(*asked.resid, w, h, 2, 4)) ||
            (asked.texture && !is_image(*asked.texture, w, h, 1, 4)) || (asked.picture && !is_image(*asked.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "FlowCheck::push: flags and mask 8UC1, checked and resid 32FC2, texture 32FC1, picture 8UC3, each of the pipeline's size");
        const Pictures out = prev || info().held ? asked : Pictures();        // a push that only stores its frame writes no picture
        staged(pipe_.context(), {{d_next_, &next}, {d_prev_, prev}, {d_flow_, &flow}, {d_back_, back}}, [&] {
            return rcflow_flowcheck_push_dev(pipe_.context(), 0, d_next_.ptr<const uint8_t>(), d_next_.pitch(), d_prev_.ptr<const uint8_t>(prev), d_prev_.pitch(),
                                             d_flow_.ptr<const float>(), d_flow_.pitch(), d_back_.ptr<const float>(back), d_back_.pitch(),
                                             d_flags_.ptr<uint8_t>(out.flags), d_flags_.pitch(), d_mask_.ptr<uint8_t>(out.mask), d_mask_.pitch(),
                                             d_checked_.ptr<float>(out.checked), d_checked_.pitch(), d_resid_.ptr<float>(out.resid), d_resid_.pitch(),
                                             d_texture_.ptr<float>(out.texture), d_texture_.pitch(), d_picture_.ptr<uint8_t>(out.picture),
                                             d_picture_.pitch(), nullptr, nullptr, nullptr);
        }, {{d_flags_, out.flags}, {d_mask_, out.mask}, {d_checked_, out.checked}, {d_resid_, out.resid}, {d_texture_, out.texture},
            {d_picture_, out.picture}});
    }
    // each waits for the pipeline's stream: of the last computing push (include/rcflow.h).  The summary: the pixels that are VALID,
    // that have BAD, OUT, FLAT, RESID, NOGAIN, FB, FAST, the computing pushes, the pushes
    std::vector<long long> read() {
        std::vector<long long> s(RC_FLOWCHECK_SUMMARY);
        check(rcflow_flowcheck_read(pipe_.context(), 0, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_flowcheck_cell> cells() {
        std::vector<rc_flowcheck_cell> r((size_t)cells_);
        check(rcflow_flowcheck_read(pipe_.context(), 0, r.data(), nullptr, nullptr));
        return r;
    }
    std::vector<long long> sums() {
        std::vector<long long> s((size_t)cells_ * RC_FLOWCHECK_SUMS);
        check(rcflow_flowcheck_read(pipe_.context(), 0, nullptr, s.data(), nullptr));
        return s;
    }
    void set(int tests, int tex_min, double res_max, int gain_pm, double fb_rel, double fb_abs, double speed_max) {
        check(rcflow_flowcheck_set(pipe_.context(), 0, tests, tex_min, res_max, gain_pm, fb_rel, fb_abs, speed_max));
    }
    rc_flowcheck_info info() { rc_flowcheck_info i; check(rcflow_flowcheck_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_flowcheck_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int cells_ = 0;
    DeviceImage d_next_, d_prev_, d_flow_, d_back_, d_flags_, d_mask_, d_checked_, d_resid_, d_texture_, d_picture_;
};

// the pictures of a Drifters::push, each optional: now 16UC1, density 32-bit unsigned (one channel of 4 bytes), live 8UC1, picture 8UC3
struct DriftersPictures { Mat* now = nullptr; Mat* density = nullptr; Mat* live = nullptr; Mat* picture = nullptr; };

// Virtual drifters on the device (rcflow_drifters_*): a population of points that every push moves through a flow field in exact
// integers until they die by a named fate, released again at their homes on request.  Host flow fields (32FC2) and zone maps (8UC1)
// of the pipeline's size in; the visit density as pictures, the census by place and by origin cell, the residence-time histograms
// and a summary out.  The per-drifter arrays of the entry point are for consumers on the device and are not staged here.
class Drifters {
  public:
    using Pictures = DriftersPictures;

    Drifters(Pipeline& pipe, const rc_drifters_params& prm) : pipe_(pipe), cells_(prm.grid_x * prm.grid_y) {
        check(rcflow_drifters_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~Drifters() { (void)rcflow_drifters_close(pipe_.context(), 0); }
    Drifters(const Drifters&) = delete;
    Drifters& operator=(const Drifters&) = delete;

    // n x (x, y) in pixels: waiting drifters, released at these homes by the next push
    void seed(const std::vector<double>& xy) { check(rcflow_drifters_seed(pipe_.context(), 0, xy.data(), (int)(xy.size() / 2))); }

    // flow: 32FC2 of the pipeline's size; zone: 8UC1 (1 shore, 2 offshore, up to 7), or null for none.  The records, both tables, the
    // histograms and the summary stay on the session after every push.
    void push(const Mat& flow, const Mat* zone = nullptr, const Pictures& out = Pictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(flow, w, h, 2, 4)) throw Error(RC_EINVAL, "Drifters::push: the field must be 32FC2 of the pipeline's size");
        if (zone && !is_image(*zone, w, h, 1, 1)) throw Error(RC_EINVAL, "Drifters::push: the zones must be 8UC1 of the pipeline's size");
        if ((out.now && !is_image(*out.now, w, h, 1, 2)) || (out.density && !is_image(*out.density, w, h, 1, 4)) ||
            (out.live && !is_image(*out.live, w, h, 1, 1)) || (out.picture && !is_image(*out.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Drifters::push: now 16UC1, density one channel of 4 bytes, live 8UC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_flow_, &flow}, {d_zone_, zone}}, [&] {
            return rcflow_drifters_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(), d_flow_.pitch(), d_zone_.ptr<const uint8_t>(zone), d_zone_.pitch(),
                                            d_now_.ptr<uint16_t>(out.now), d_now_.pitch(), d_density_.ptr<uint32_t>(out.density), d_density_.pitch(),
                                            d_live_.ptr<uint8_t>(out.live), d_live_.pitch(), d_picture_.ptr<uint8_t>(out.picture), d_picture_.pitch(),
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        }, {{d_now_, out.now}, {d_density_, out.density}, {d_live_, out.live}, {d_picture_, out.picture}});
    }
    // each waits for the pipeline's stream (include/rcflow.h).  The summary: drifters, alive, released, pushes, the sums of age at the
    // SHORE and at the OFFSHORE deaths, 0, 0, the deaths by fate 0..15
    std::vector<long long> read() {
        std::vector<long long> s(RC_DRIFTERS_SUMMARY);
        check(rcflow_drifters_read(pipe_.context(), 0, nullptr, nullptr, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_drifters_cell> cells() {
        std::vector<rc_drifters_cell> r((size_t)cells_);
        check(rcflow_drifters_read(pipe_.context(), 0, r.data(), nullptr, nullptr, nullptr, nullptr));
        return r;
    }
    std::vector<long long> place() {
        std::vector<long long> s((size_t)cells_ * RC_DRIFTERS_SUMS);
        check(rcflow_drifters_read(pipe_.context(), 0, nullptr, s.data(), nullptr, nullptr, nullptr));
        return s;
    }
    std::vector<long long> origin() {
        std::vector<long long> s((size_t)cells_ * RC_DRIFTERS_SUMS);
        check(rcflow_drifters_read(pipe_.context(), 0, nullptr, nullptr, s.data(), nullptr, nullptr));
        return s;
    }
    std::vector<unsigned long long> hist() {
        std::vector<unsigned long long> s((size_t)4 * RC_DRIFTERS_HIST_BINS);
        check(rcflow_drifters_read(pipe_.context(), 0, nullptr, nullptr, nullptr, s.data(), nullptr));
        return s;
    }
    void set(double dt, int max_age, int density_full, int live_min, int flags) {
        check(rcflow_drifters_set(pipe_.context(), 0, dt, max_age, density_full, live_min, flags));
    }
    rc_drifters_info info() { rc_drifters_info i; check(rcflow_drifters_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_drifters_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int cells_ = 0;
    DeviceImage d_flow_, d_zone_, d_now_, d_density_, d_live_, d_picture_;
};

// the pictures of an Infill::push, each optional: filled 32FC2, source and mask 8UC1, picture 8UC3
struct InfillPictures { Mat* filled = nullptr; Mat* source = nullptr; Mat* mask = nullptr; Mat* picture = nullptr; };

// Flow infill on the device (rcflow_infill_*): the holes of a checked flow field filled from a pyramid of block sums.  Host flow
// fields (32FC2), valid masks and domains (8UC1) of the pipeline's size in; the filled field, a byte per pixel that says where the
// value came from, the mask of the pixels with a value and a picture out, and a record per cell of a grid.
class Infill {
  public:
    using Pictures = InfillPictures;

    Infill(Pipeline& pipe, const rc_infill_params& prm) : pipe_(pipe), cells_(prm.grid_x * prm.grid_y) {
        check(rcflow_infill_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~Infill() { (void)rcflow_infill_close(pipe_.context(), 0); }
    Infill(const Infill&) = delete;
    Infill& operator=(const Infill&) = delete;

    // flow: 32FC2; valid: 8UC1 (what FlowCheck writes as mask), or null: every finite vector is valid; domain: 8UC1, or null: a
    // value is wanted everywhere.  The records, the sums and the summary stay on the session after every push, for read(), cells()
    // and sums().
    void push(const Mat& flow, const Mat* valid = nullptr, const Mat* domain = nullptr, const Pictures& out = Pictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(flow, w, h, 2, 4)) throw Error(RC_EINVAL, "Infill::push: the field must be 32FC2 of the pipeline's size");
        if ((valid && !is_image(*valid, w, h, 1, 1)) || (domain && !is_image(*domain, w, h, 1, 1)))
            throw Error(RC_EINVAL, "Infill::push: valid and domain must be 8UC1 of the pipeline's size");
        if ((out.filled && !is_image(*out.filled, w, h, 2, 4)) || (out.source && !is_image(*out.source, w, h, 1, 1)) ||
            (out.mask && !is_image(*out.mask, w, h, 1, 1)) || (out.picture && !is_image(*out.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Infill::push: filled 32FC2, source and mask 8UC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_flow_, &flow}, {d_valid_, valid}, {d_domain_, domain}}, [&] {
            return rcflow_infill_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(), d_flow_.pitch(), d_valid_.ptr<const uint8_t>(valid), d_valid_.pitch(),
                                          d_domain_.ptr<const uint8_t>(domain), d_domain_.pitch(), d_filled_.ptr<float>(out.filled), d_filled_.pitch(),
                                          d_source_.ptr<uint8_t>(out.source), d_source_.pitch(), d_mask_.ptr<uint8_t>(out.mask), d_mask_.pitch(),
                                          d_picture_.ptr<uint8_t>(out.picture), d_picture_.pitch(), nullptr, nullptr, nullptr);
        }, {{d_filled_, out.filled}, {d_source_, out.source}, {d_mask_, out.mask}, {d_picture_, out.picture}});
    }
    // each waits for the pipeline's stream (include/rcflow.h).  The summary: the pixels that are KNOWN, HELD, FILLED, UNFILLED,
    // OUTSIDE, the pushes, 0, 0, the FILLED pixels by lev 0..7
    std::vector<long long> read() {
        std::vector<long long> s(RC_INFILL_SUMMARY);
        check(rcflow_infill_read(pipe_.context(), 0, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_infill_cell> cells() {
        std::vector<rc_infill_cell> r((size_t)cells_);
        check(rcflow_infill_read(pipe_.context(), 0, r.data(), nullptr, nullptr));
        return r;
    }
    std::vector<long long> sums() {
        std::vector<long long> s((size_t)cells_ * RC_INFILL_SUMS);
        check(rcflow_infill_read(pipe_.context(), 0, nullptr, s.data(), nullptr));
        return s;
    }
    void set(int levels, int min_known, int flags) { check(rcflow_infill_set(pipe_.context(), 0, levels, min_known, flags)); }
    rc_infill_info info() { rc_infill_info i; check(rcflow_infill_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_infill_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int cells_ = 0;
    DeviceImage d_flow_, d_valid_, d_domain_, d_filled_, d_source_, d_mask_, d_picture_;
};

// the pictures of an Offshore::map, each optional: dist2, near and sdist 32SC1, picture 8UC3
struct OffshoreMapPictures { Mat* dist2 = nullptr; Mat* near = nullptr; Mat* sdist = nullptr; Mat* picture = nullptr; };
// the pictures of an Offshore::push, each optional: cross_along 32FC2, cls and mask 8UC1, picture 8UC3
struct OffshorePushPictures { Mat* cross_along = nullptr; Mat* cls = nullptr; Mat* mask = nullptr; Mat* picture = nullptr; };

// Offshore frame on the device (rcflow_offshore_*): the exact distance of every pixel to the shore, and a flow field projected on
// the local shore normal.  Host wet masks (8UC1) and flow fields (32FC2) of the pipeline's size in; the distance planes, the cross /
// along field, the class, the mask of the seaward flow and pictures out, a record per station along the beach and a table of
// stations x bins of distance.
class Offshore {
  public:
    using MapPictures = OffshoreMapPictures;
    using PushPictures = OffshorePushPictures;

    Offshore(Pipeline& pipe, const rc_offshore_params& prm) : pipe_(pipe), stations_(prm.stations), bins_(prm.bins) {
        check(rcflow_offshore_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~Offshore() { (void)rcflow_offshore_close(pipe_.context(), 0); }
    Offshore(const Offshore&) = delete;
    Offshore& operator=(const Offshore&) = delete;

    // wet: 8UC1, non-zero is water (what Shoreline writes as its wet mask).  Called when the shore has moved; the map stays on the
    // session for push() and band(), its summary for map_summary()
    void map(const Mat& wet, const MapPictures& out = MapPictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(wet, w, h, 1, 1)) throw Error(RC_EINVAL, "Offshore::map: the wet mask must be 8UC1 of the pipeline's size");
        if ((out.dist2 && !is_image(*out.dist2, w, h, 1, 4)) || (out.near && !is_image(*out.near, w, h, 1, 4)) ||
            (out.sdist && !is_image(*out.sdist, w, h, 1, 4)) || (out.picture && !is_image(*out.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Offshore::map: dist2, near and sdist 32SC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_wet_, &wet}}, [&] {
            return rcflow_offshore_map_dev(pipe_.context(), 0, d_wet_.ptr<const uint8_t>(), d_wet_.pitch(), d_dist2_.ptr<int>(out.dist2), d_dist2_.pitch(),
                                           d_near_.ptr<int>(out.near), d_near_.pitch(), d_sdist_.ptr<int>(out.sdist), d_sdist_.pitch(),
                                           d_picture_.ptr<uint8_t>(out.picture), d_picture_.pitch(), nullptr);
        }, {{d_dist2_, out.dist2}, {d_near_, out.near}, {d_sdist_, out.sdist}, {d_picture_, out.picture}});
    }
    // flow: 32FC2.  The records, the table and the summary stay on the session after every push, for stations(), table() and read()
    void push(const Mat& flow, const PushPictures& out = PushPictures()) {
        const int w = pipe_.width(), h = pipe_.height();
        if (!is_image(flow, w, h, 2, 4)) throw Error(RC_EINVAL, "Offshore::push: the field must be 32FC2 of the pipeline's size");
        if ((out.cross_along && !is_image(*out.cross_along, w, h, 2, 4)) || (out.cls && !is_image(*out.cls, w, h, 1, 1)) ||
            (out.mask && !is_image(*out.mask, w, h, 1, 1)) || (out.picture && !is_image(*out.picture, w, h, 3, 1)))
            throw Error(RC_EINVAL, "Offshore::push: cross_along 32FC2, cls and mask 8UC1, picture 8UC3, each of the pipeline's size");
        staged(pipe_.context(), {{d_flow_, &flow}}, [&] {
            return rcflow_offshore_push_dev(pipe_.context(), 0, d_flow_.ptr<const float>(), d_flow_.pitch(), d_ca_.ptr<float>(out.cross_along), d_ca_.pitch(),
                                            d_cls_.ptr<uint8_t>(out.cls), d_cls_.pitch(), d_mask_.ptr<uint8_t>(out.mask), d_mask_.pitch(),
                                            d_picture_.ptr<uint8_t>(out.picture), d_picture_.pitch(), nullptr, nullptr, nullptr);
        }, {{d_ca_, out.cross_along}, {d_cls_, out.cls}, {d_mask_, out.mask}, {d_picture_, out.picture}});
    }
    // band: 8UC1 of the pipeline's size: 255 where the pixel is wet and lo <= its distance to the shore < hi, in pixels
    void band(float lo, float hi, Mat& band) {
        if (!is_image(band, pipe_.width(), pipe_.height(), 1, 1)) throw Error(RC_EINVAL, "Offshore::band: the band must be 8UC1 of the pipeline's size");
        staged(pipe_.context(), {}, [&] {
            return rcflow_offshore_band_dev(pipe_.context(), 0, lo, hi, d_band_.ptr<uint8_t>(), d_band_.pitch());
        }, {{d_band_, &band}});
    }
    // each waits for the pipeline's stream (include/rcflow.h).  The push summary: the pixels that are OK, NEAR, FAR, DRY, BAD, the mask
    // pixels, the stations flagged RIP, the pushes.  The map summary: wet, dry, wet and not FAR, the largest d2 and the sum of d2 over
    // those, the sum of d2 over the dry pixels, 0, the maps
    std::vector<long long> read() {
        std::vector<long long> s(RC_OFFSHORE_SUMMARY);
        check(rcflow_offshore_read(pipe_.context(), 0, nullptr, nullptr, s.data(), nullptr));
        return s;
    }
    std::vector<long long> map_summary() {
        std::vector<long long> s(RC_OFFSHORE_SUMMARY);
        check(rcflow_offshore_read(pipe_.context(), 0, nullptr, nullptr, nullptr, s.data()));
        return s;
    }
    std::vector<rc_offshore_station> stations() {
        std::vector<rc_offshore_station> r((size_t)stations_);
        check(rcflow_offshore_read(pipe_.context(), 0, r.data(), nullptr, nullptr, nullptr));
        return r;
    }
    std::vector<long long> table() {
        std::vector<long long> t((size_t)stations_ * bins_ * RC_OFFSHORE_SUMS);
        check(rcflow_offshore_read(pipe_.context(), 0, nullptr, t.data(), nullptr, nullptr));
        return t;
    }
    void set(const rc_offshore_params& prm) { check(rcflow_offshore_set(pipe_.context(), 0, &prm)); }
    rc_offshore_info info() { rc_offshore_info i; check(rcflow_offshore_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_offshore_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    int stations_ = 0, bins_ = 0;
    DeviceImage d_wet_, d_flow_, d_dist2_, d_near_, d_sdist_, d_ca_, d_cls_, d_mask_, d_band_, d_picture_;
};

// the loops of an Outlines::read: the records written, in order, and the stored vertices, (x, y) pairs of lattice corners; loop r's
// polygon is vertices 2 * r.offset .. 2 * (r.offset + r.verts) unless r.offset is -1.  summary: the 8 words of include/rcflow.h
struct OutlinesResult {
    std::vector<rc_outline_loop> loops;
    std::vector<int32_t> verts;
    long long summary[RC_OUTLINES_SUMMARY] = {};
};

// Region outlines on the device (rcflow_outlines_*): the boundaries of a label plane (32SC1: what Regions::push writes as labels) or
// of a mask (8UC1, non-zero is label 1) of the pipeline's size traced into ordered polygons, outer boundaries and holes told apart.
// Host images in, records and vertices out.
class Outlines {
  public:
    Outlines(Pipeline& pipe, const rc_outlines_params& prm) : pipe_(pipe), prm_(prm) {
        check(rcflow_outlines_open(pipe.context(), 0, pipe.width(), pipe.height(), &prm));
    }
    ~Outlines() { (void)rcflow_outlines_close(pipe_.context(), 0); }
    Outlines(const Outlines&) = delete;
    Outlines& operator=(const Outlines&) = delete;

    // plane: 32SC1 labels or an 8UC1 mask.  Records, vertices and summary stay on the session after every push, for read() and draw()
    void push(const Mat& plane) {
        const int w = pipe_.width(), h = pipe_.height();
        const bool labels = is_image(plane, w, h, 1, 4);
        if (!labels && !is_image(plane, w, h, 1, 1)) throw Error(RC_EINVAL, "Outlines::push: the plane must be 32SC1 or 8UC1 of the pipeline's size");
        DeviceImage& d = labels ? d_labels_ : d_mask_;
        staged(pipe_.context(), {{d, &plane}}, [&] {
            return rcflow_outlines_push_dev(pipe_.context(), 0, d_labels_.ptr<const int32_t>(labels), labels ? d_labels_.pitch() : 0,
                                            d_mask_.ptr<const uint8_t>(!labels), labels ? 0 : d_mask_.pitch(), nullptr, nullptr, nullptr);
        }, {});
    }
    // waits for the pipeline's stream
    OutlinesResult read() {
        OutlinesResult r;
        r.loops.resize((size_t)prm_.max_loops);
        r.verts.resize(2 * (size_t)prm_.max_vertices);
        int n = 0, nv = 0;
        check(rcflow_outlines_read(pipe_.context(), 0, r.loops.data(), prm_.max_loops, &n, r.verts.data(), prm_.max_vertices, &nv, r.summary));
        r.loops.resize((size_t)n);
        r.verts.resize(2 * (size_t)nv);
        return r;
    }
    // paints the stored polygons of the last push into img (8UC3), every vertex clamped into the picture
    void draw(Mat& img, uint32_t color = 0x00ffff, int thickness = 1) {
        if (!is_image(img, pipe_.width(), pipe_.height(), 3, 1)) throw Error(RC_EINVAL, "Outlines::draw: img must be 8UC3 of the pipeline's size");
        staged_draw(pipe_.context(), d_canvas_, d_prims_, prm_.max_vertices, img, [&](rc_draw_prim* prims) {
            return rcflow_outlines_prims_dev(pipe_.context(), 0, color, thickness, prims);
        });
    }
    void setMinCracks(int min_cracks) { check(rcflow_outlines_set(pipe_.context(), 0, min_cracks)); }
    rc_outlines_info info() { rc_outlines_info i; check(rcflow_outlines_info(pipe_.context(), 0, &i)); return i; }
    void reset() { check(rcflow_outlines_reset(pipe_.context(), 0)); }

  private:
    Pipeline& pipe_;
    rc_outlines_params prm_;
    DeviceImage d_labels_, d_mask_, d_prims_, d_canvas_;
};

}  // namespace rc
