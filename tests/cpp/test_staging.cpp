// The staging layer of include/rcflow_module.hpp held to the two things the per-product programs never exercise, on a pipeline
// of 37 x 23 (odd, so no row is a multiple of 4 bytes) with plan and grid sizes of their own.
//   1. Padded rows equal dense rows.  The whole sequence -- the two-image flow call, upload_flow, the classification mask, the
//      streamline display, timexPush, framestabPush, warpAffine and four pushes of each of the nine product classes, the last
//      asking for every host output -- runs twice, each time on a fresh Pipeline: with dense host images, then with every host
//      image, input and output, on rows of row_bytes() + 5 whose padding holds 0xA5.  Every output pixel and every record read
//      back must be equal between the two, and every padding byte must still be 0xA5.  That the dense run is right is what the
//      per-product tests establish.
//   2. Refusals.  For every host-image argument of every class: one row too many, a wrong channel count, a wrong elem and an
//      empty view are each refused with RC_EINVAL, the object's count of pushes is unchanged (the pipeline keeps none), and a
//      correct call follows.  Left out are only the views that are no mistake or that the header did not always refuse this way:
//      an empty view where it means "not wanted" (the `flow` of the flow calls, timexPush's four images) or where the copy
//      used to fail instead (upload_flow, the display calls); a row too many for warpAffine, which takes any size; the channel
//      count and elem of `next` in the two-image calls, which were not always asked; and the outmask of
//      create_flow_and_accumulationbuffer, of which only data and step are read.
// Inputs are made from integers.  Prints "test_staging: ok".
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "rcflow_module.hpp"

static int g_pad = 0, g_fails = 0;
static void fail(const std::string& what) { std::printf("FAILED (padding %d): %s\n", g_pad, what.c_str()); g_fails++; }

// a host image on rows of row_bytes() + g_pad, everything 0xA5 until written; one spare row, so that no wrong view reaches past it
struct Img {
    int rows, cols, ch, el;
    size_t step;
    std::vector<unsigned char> buf;
    Img(int r, int c, int channels, int elem) : rows(r), cols(c), ch(channels), el(elem), step((size_t)c * channels * elem + g_pad), buf(step * (r + 1), 0xA5) {}
    rc::Mat mat() { return rc::Mat(rows, cols, ch, el, buf.data(), step); }
    unsigned char* row(int y) { return buf.data() + (size_t)y * step; }
    size_t row_bytes() const { return (size_t)cols * ch * el; }
    bool padding_intact() const {
        for (int y = 0; y <= rows; y++)
            for (size_t k = y < rows ? row_bytes() : 0; k < step; k++)
                if (buf[(size_t)y * step + k] != 0xA5) return false;
        return true;
    }
};

// what a run gave, by name and in order: the pixels of every output image and the bytes of every record read back
typedef std::vector<std::pair<std::string, std::vector<unsigned char>>> Results;
static void keep(Results& out, const std::string& name, const void* p, size_t bytes) {
    out.emplace_back(name, std::vector<unsigned char>((const unsigned char*)p, (const unsigned char*)p + bytes));
}
template <class T> static void keep(Results& out, const std::string& name, const std::vector<T>& v) { keep(out, name, v.data(), v.size() * sizeof(T)); }
static void keep(Results& out, const std::string& name, Img& m) {
    if (!m.padding_intact()) fail(name + ": padding written");
    std::vector<unsigned char> px;
    for (int y = 0; y < m.rows; y++) px.insert(px.end(), m.row(y), m.row(y) + m.row_bytes());
    out.emplace_back(name, px);
}

static void fill_gray(Img& g, int t) {      // a pattern that moves two pixels right and one down per frame
    for (int y = 0; y < g.rows; y++)
        for (int x = 0; x < g.cols; x++) {
            const int xs = x - 2 * t + 64, ys = y - t + 64;
            g.row(y)[x] = (unsigned char)(((xs * xs * 7 + ys * ys * 13 + xs * ys * 3) % 251 + (x * y + t) % 5) % 256);
        }
}
static void fill_bgr(Img& g, int t) {
    for (int y = 0; y < g.rows; y++)
        for (int x = 0; x < g.cols * 3; x++) g.row(y)[x] = (unsigned char)(((x / 3 - t) * 7 + y * 13 + (x % 3) * 5 + (x / 3) * y) % 256);
}
static void fill_flow(Img& g, int t) {
    for (int y = 0; y < g.rows; y++) {
        float* f = (float*)g.row(y);
        for (int x = 0; x < g.cols; x++) {
            f[2 * x] = (float)((x * 7 + y * 3 + t * 5) % 32 - 12) / 16.f;
            f[2 * x + 1] = (float)((x * 5 + y * 11 + t * 3) % 32 - 18) / 16.f;
        }
    }
}
static void fill_mask(Img& g, int t) {      // blobs that drift to the right
    for (int y = 0; y < g.rows; y++)
        for (int x = 0; x < g.cols; x++) g.row(y)[x] = (unsigned char)((((x - t) / 5 + y / 4) % 3 == 0 && (x - t) % 5 != 4 && y % 4 != 3) ? 255 : 0);
}

// one row too many, a wrong channel count, a wrong elem, empty: `call` must refuse each of `cases` with RC_EINVAL and `pushes`
// must not move
enum { ROW = 1, CHANNELS = 2, ELEM = 4, EMPTY = 8, GEOMETRY = ROW | CHANNELS | ELEM, ALL = GEOMETRY | EMPTY };
template <class Call, class Pushes>
static void refusals(const std::string& who, Img& good, Call&& call, Pushes&& pushes, int cases = ALL) {
    rc::Mat v[4] = {good.mat(), good.mat(), good.mat(), rc::Mat()};
    v[0].rows++; v[1].channels++; v[2].elem = good.el == 1 ? 4 : 1;
    const char* kind[4] = {"a row too many", "a wrong channel count", "a wrong elem", "an empty view"};
    for (int k = 0; k < 4; k++) {
        if (!(cases & (1 << k))) continue;
        const long long before = pushes();
        int code = 0;
        try { call(v[k]); } catch (const rc::Error& e) { code = e.code; }
        if (code != RC_EINVAL || pushes() != before) fail(who + ": " + kind[k] + " was not refused with RC_EINVAL and the state left alone");
    }
}

static void run(Results& out) {
    const int w = 37, h = 23;
    rc::Pipeline pipe(w, h);
    Img gray(h, w, 1, 1), gray2(h, w, 1, 1), mask(h, w, 1, 1), bgr(h, w, 3, 1), flow(h, w, 2, 4);
    Img out1(h, w, 1, 1), out3(h, w, 3, 1), canvas(h, w, 3, 1), labels(h, w, 1, 4), scalar(h, w, 1, 4);
    rc::Mat m_gray = gray.mat(), m_gray2 = gray2.mat(), m_mask = mask.mat(), m_bgr = bgr.mat(), m_flow = flow.mat();
    rc::Mat m_out1 = out1.mat(), m_out3 = out3.mat(), m_canvas = canvas.mat(), m_labels = labels.mat(), m_scalar = scalar.mat(), none;

    {   // the pipeline's own calls
        Img f(h, w, 2, 4);
        rc::Mat m_f = f.mat();
        fill_gray(gray, 0); fill_gray(gray2, 1);
        pipe.calcOpticalFlowFarneback(m_gray, m_gray2, m_f, 0.5, 2, 3, 2, 15, 1.2, 0);
        keep(out, "calcOpticalFlowFarneback", f);
        auto still = [] { return 0ll; };                          // the pipeline counts no pushes; the call that follows shows it works
        const int initial = RC_FARNEBACK_USE_INITIAL_FLOW;
        refusals("calcOpticalFlowFarneback prev", gray, [&](rc::Mat& v) { pipe.calcOpticalFlowFarneback(v, m_gray2, m_f, 0.5, 2, 3, 2, 15, 1.2, 0); }, still);
        refusals("calcOpticalFlowFarneback next", gray2, [&](rc::Mat& v) { pipe.calcOpticalFlowFarneback(m_gray, v, m_f, 0.5, 2, 3, 2, 15, 1.2, 0); }, still, ROW | EMPTY);
        refusals("calcOpticalFlowFarneback flow", f, [&](rc::Mat& v) { pipe.calcOpticalFlowFarneback(m_gray, m_gray2, v, 0.5, 2, 3, 2, 15, 1.2, 0); }, still, GEOMETRY);
        refusals("calcOpticalFlowFarneback initial flow", f, [&](rc::Mat& v) { pipe.calcOpticalFlowFarneback(m_gray, m_gray2, v, 0.5, 2, 3, 2, 15, 1.2, initial); }, still);
        fill_flow(f, 9);
        pipe.calcOpticalFlowFarneback(m_gray, m_gray2, m_f, 0.5, 2, 3, 2, 15, 1.2, RC_FARNEBACK_USE_INITIAL_FLOW);
        keep(out, "calcOpticalFlowFarneback from an initial flow", f);
        std::vector<rc::Pixel2> pts = {rc::Pixel2{18.f, 11.f}, rc::Pixel2{10.f, 8.f}, rc::Pixel2{27.f, 15.f}}, moved;
        std::vector<unsigned char> status;
        std::vector<float> err;
        refusals("calcOpticalFlowPyrLK prev", gray, [&](rc::Mat& v) { pipe.calcOpticalFlowPyrLK(v, m_gray2, pts, moved, status, err); }, still);
        refusals("calcOpticalFlowPyrLK next", gray2, [&](rc::Mat& v) { pipe.calcOpticalFlowPyrLK(m_gray, v, pts, moved, status, err); }, still, ROW | EMPTY);
        pipe.calcOpticalFlowPyrLK(m_gray, m_gray2, pts, moved, status, err);
        keep(out, "calcOpticalFlowPyrLK: nextPts", moved); keep(out, "calcOpticalFlowPyrLK: status", status);
        fill_flow(flow, 2);
        refusals("upload_flow", flow, [&](rc::Mat& v) { pipe.upload_flow(v); }, still, GEOMETRY);
        pipe.upload_flow(m_flow);
        int hist[RC_HIST_BINS], histsum = 0, hist2d[RC_HIST_DIRECTIONS][RC_HIST_BINS], histsum2d[RC_HIST_DIRECTIONS];
        float UPPER = 0.f, UPPER2d[RC_HIST_DIRECTIONS], prop[RC_HIST_DIRECTIONS];
        pipe.create_histogram(hist, histsum, hist2d, histsum2d, UPPER, UPPER2d, prop);
        keep(out, "upload_flow: hist2d", &hist2d[0][0], sizeof(hist2d));
        pipe.create_flow_and_accumulationbuffer(m_out1, 30);
        keep(out, "create_flow_and_accumulationbuffer", out1);
        pipe.streamline_field(2.f, 1);
        refusals("streamline_displacement", out3, [&](rc::Mat& v) { pipe.streamline_displacement(v); }, still, GEOMETRY);
        pipe.streamline_displacement(m_out3);
        keep(out, "streamline_displacement", out3);

        Img mean(h, w, 3, 1), average(h, w, 3, 1), bright(h, w, 3, 1), dark(h, w, 3, 1);
        rc::Mat m_mean = mean.mat(), m_average = average.mat(), m_bright = bright.mat(), m_dark = dark.mat();
        pipe.timexOpen(3, RC_TIMEX_MEAN | RC_TIMEX_AVERAGE | RC_TIMEX_BRIGHT | RC_TIMEX_DARK);
        for (int t = 0; t < 4; t++) {
            fill_bgr(bgr, t);
            if (t < 3) pipe.timexPush(m_bgr, none, none, none, none);
            else pipe.timexPush(m_bgr, m_mean, m_average, m_bright, m_dark);
        }
        keep(out, "timexPush: mean", mean); keep(out, "timexPush: average", average);
        keep(out, "timexPush: bright", bright); keep(out, "timexPush: dark", dark);
        refusals("timexPush frame", bgr, [&](rc::Mat& v) { pipe.timexPush(v, m_mean, m_average, m_bright, m_dark); }, still);
        refusals("timexPush mean", mean, [&](rc::Mat& v) { pipe.timexPush(m_bgr, v, m_average, m_bright, m_dark); }, still, GEOMETRY);
        refusals("timexPush average", average, [&](rc::Mat& v) { pipe.timexPush(m_bgr, m_mean, v, m_bright, m_dark); }, still, GEOMETRY);
        refusals("timexPush bright", bright, [&](rc::Mat& v) { pipe.timexPush(m_bgr, m_mean, m_average, v, m_dark); }, still, GEOMETRY);
        refusals("timexPush dark", dark, [&](rc::Mat& v) { pipe.timexPush(m_bgr, m_mean, m_average, m_bright, v); }, still, GEOMETRY);
        pipe.timexPush(m_bgr, m_mean, m_average, m_bright, m_dark);
        pipe.timexClose();

        pipe.framestabOpen(4, 4, 16, 16);
        double shift[3];
        for (int t = 0; t < 4; t++) {
            fill_bgr(bgr, t);
            pipe.framestabPush(m_bgr, m_out3, shift);
        }
        keep(out, "framestabPush", out3); keep(out, "framestabPush: shift", shift, sizeof(shift));
        refusals("framestabPush frame", bgr, [&](rc::Mat& v) { pipe.framestabPush(v, m_out3); }, still);
        refusals("framestabPush corrected", out3, [&](rc::Mat& v) { pipe.framestabPush(m_bgr, v); }, still);
        pipe.framestabPush(m_bgr, m_out3);
        pipe.framestabClose();

        Img small(17, 29, 3, 1);
        rc::Mat m_small = small.mat();
        const double M[6] = {1., 0.125, 1.5, -0.125, 1., 0.5};
        refusals("warpAffine src", bgr, [&](rc::Mat& v) { pipe.warpAffine(v, m_small, M); }, still, CHANNELS | ELEM | EMPTY);
        refusals("warpAffine dst", small, [&](rc::Mat& v) { pipe.warpAffine(m_bgr, v, M); }, still, CHANNELS | ELEM | EMPTY);
        pipe.warpAffine(m_bgr, m_small, M);
        keep(out, "warpAffine", small);

        // the frame loop's pushes; afterwards the uploaded field is the resident one again
        refusals("pushFrame frame", gray, [&](rc::Mat& v) { pipe.pushFrame(v, none, 0.5, 2, 3, 2, 15, 1.2, 0); }, still);
        refusals("pushFrame flow", f, [&](rc::Mat& v) { pipe.pushFrame(m_gray, v, 0.5, 2, 3, 2, 15, 1.2, 0); }, still, GEOMETRY);
        pipe.pushFrame(m_gray, none, 0.5, 2, 3, 2, 15, 1.2, 0);   // primes the stream
        if (!pipe.pushFrame(m_gray2, m_f, 0.5, 2, 3, 2, 15, 1.2, 0)) fail("pushFrame: no flow from the second frame");
        keep(out, "pushFrame", f);
        fill_gray(gray, 2);
        rc::Mat staging = pipe.frameBuffer();
        for (int y = 0; y < h; y++) std::memcpy((unsigned char*)staging.data + (size_t)y * staging.step, gray.row(y), (size_t)w);
        refusals("pushAcquired flow", f, [&](rc::Mat& v) { pipe.pushAcquired(v, 0.5, 2, 3, 2, 15, 1.2, 0); }, still, GEOMETRY);
        if (!pipe.pushAcquired(m_f, 0.5, 2, 3, 2, 15, 1.2, 0)) fail("pushAcquired: no flow from the third frame");
        keep(out, "pushAcquired", f);
        pipe.upload_flow(m_flow);
    }
    {
        rc::RipMap rm(pipe, 3, 3, 2);
        for (int t = 0; t < 4; t++) { fill_flow(flow, t); rm.push(m_flow); }
        const rc::RipMap::Result r = rm.read();
        keep(out, "RipMap: cells", r.cells); keep(out, "RipMap: sums", r.sums);
        rm.mask(m_out1);
        keep(out, "RipMap::mask", out1);
        auto pushes = [&] { return rm.read().frames_pushed; };
        refusals("RipMap::push flow", flow, [&](rc::Mat& v) { rm.push(v); }, pushes);
        refusals("RipMap::mask", out1, [&](rc::Mat& v) { rm.mask(v); }, pushes);
        rm.push(m_flow);
        if (pushes() != 5) fail("RipMap: the push after the refusals");
    }
    {
        rc::Tracers tr(pipe, RC_TRACERS_LK, 4, 8);
        tr.addStreakline(rc::Pixel2{18.f, 11.f});
        tr.addTimeline(rc::Pixel2{8.f, 6.f}, rc::Pixel2{28.f, 16.f}, 4);
        for (int t = 0; t < 4; t++) {
            fill_gray(gray, t);
            if (t < 3) { tr.push(m_gray); continue; }
            fill_bgr(canvas, t);
            tr.push(m_gray, &m_canvas);
        }
        keep(out, "Tracers: outImg", canvas); keep(out, "Tracers: streakline", tr.vertices(0)); keep(out, "Tracers: timeline", tr.vertices(1));
        auto pushes = [&] { return tr.info().pushes; };
        refusals("Tracers::push gray", gray, [&](rc::Mat& v) { tr.push(v, &m_canvas); }, pushes);
        refusals("Tracers::push outImg", canvas, [&](rc::Mat& v) { tr.push(m_gray, &v); }, pushes);
        tr.push(m_gray, &m_canvas);
        if (pushes() != 4) fail("Tracers: the push after the refusals");
    }
    {
        rc::Regions rg(pipe);
        for (int t = 0; t < 4; t++) {
            fill_mask(mask, t);
            if (t < 3) rg.push(m_mask);
            else rg.push(m_mask, true, &m_labels, &m_out1);
        }
        long long summary[8];
        keep(out, "Regions: labels", labels); keep(out, "Regions: maskOut", out1);
        keep(out, "Regions: records", rg.regions(summary)); keep(out, "Regions: summary", summary, sizeof(summary));
        fill_bgr(canvas, 1);
        rg.draw(m_canvas, 0x00ffff, 1, 2, 2.);
        keep(out, "Regions::draw", canvas);
        auto pushes = [&] { return rg.info().pushes; };
        refusals("Regions::push mask", mask, [&](rc::Mat& v) { rg.push(v, false, &m_labels, &m_out1); }, pushes);
        refusals("Regions::push labels", labels, [&](rc::Mat& v) { rg.push(m_mask, false, &v, &m_out1); }, pushes);
        refusals("Regions::push maskOut", out1, [&](rc::Mat& v) { rg.push(m_mask, false, &m_labels, &v); }, pushes);
        refusals("Regions::draw img", canvas, [&](rc::Mat& v) { rg.draw(v); }, pushes);
        rg.push(m_mask, false, nullptr, &m_mask);                 // in place
        keep(out, "Regions: maskOut in place", mask);
        if (pushes() != 5) fail("Regions: the push after the refusals");

        rc::Tracks tk(pipe, rg);
        for (int t = 0; t < 4; t++) {
            fill_mask(mask, t);
            if (t < 3) tk.push(m_mask);
            else tk.push(m_mask, true, &m_out1);
        }
        std::vector<int32_t> footprint;
        keep(out, "Tracks: maskOut", out1);
        keep(out, "Tracks: tracks", tk.tracks(summary, &footprint)); keep(out, "Tracks: summary", summary, sizeof(summary));
        keep(out, "Tracks: footprint", footprint);
        fill_bgr(canvas, 2);
        tk.draw(m_canvas);
        keep(out, "Tracks::draw", canvas);
        auto tpushes = [&] { return tk.info().pushes; };
        refusals("Tracks::push mask", mask, [&](rc::Mat& v) { tk.push(v, false, &m_out1); }, tpushes);
        refusals("Tracks::push maskOut", out1, [&](rc::Mat& v) { tk.push(m_mask, false, &v); }, tpushes);
        refusals("Tracks::draw img", canvas, [&](rc::Mat& v) { tk.draw(v); }, tpushes);
        tk.push(m_mask, false, &m_out1);
        if (tpushes() != 5) fail("Tracks: the push after the refusals");
    }
    {
        rc::MotionTemplates mt(pipe, 30, 1., 0.25, 1., 3, 2);
        for (int t = 0; t < 4; t++) {
            fill_gray(gray, t);
            if (t < 3) mt.push(m_gray);
            else mt.push(m_gray, RC_MOTION_AUTO_TIME, &m_out3);
        }
        std::vector<rc_motion_cell> cells;
        const rc_motion_cell frame = mt.read(&cells);
        keep(out, "MotionTemplates: picture", out3); keep(out, "MotionTemplates: cells", cells); keep(out, "MotionTemplates: frame", &frame, sizeof(frame));
        fill_bgr(canvas, 3);
        mt.draw(m_canvas);
        keep(out, "MotionTemplates::draw", canvas);
        auto pushes = [&] { return mt.info().pushes; };
        refusals("MotionTemplates::push gray", gray, [&](rc::Mat& v) { mt.push(v, RC_MOTION_AUTO_TIME, &m_out3); }, pushes);
        refusals("MotionTemplates::push picture", out3, [&](rc::Mat& v) { mt.push(m_gray, RC_MOTION_AUTO_TIME, &v); }, pushes);
        refusals("MotionTemplates::draw img", canvas, [&](rc::Mat& v) { mt.draw(v); }, pushes);
        mt.push(m_gray, RC_MOTION_AUTO_TIME, &m_out3);
        if (pushes() != 5) fail("MotionTemplates: the push after the refusals");
    }
    {
        rc::Ftle ft(pipe, 3);
        for (int t = 0; t < 4; t++) {
            fill_flow(flow, t);
            if (t < 3) ft.push(m_flow);
            else ft.push(m_flow, &m_scalar, &m_out1, &m_out3);
        }
        keep(out, "Ftle: ftle", scalar); keep(out, "Ftle: mask", out1); keep(out, "Ftle: picture", out3); keep(out, "Ftle: summary", ft.read());
        auto pushes = [&] { return ft.info().pushes; };
        refusals("Ftle::push flow", flow, [&](rc::Mat& v) { ft.push(v, &m_scalar, &m_out1, &m_out3); }, pushes);
        refusals("Ftle::push ftle", scalar, [&](rc::Mat& v) { ft.push(m_flow, &v, &m_out1, &m_out3); }, pushes);
        refusals("Ftle::push mask", out1, [&](rc::Mat& v) { ft.push(m_flow, &m_scalar, &v, &m_out3); }, pushes);
        refusals("Ftle::push picture", out3, [&](rc::Mat& v) { ft.push(m_flow, &m_scalar, &m_out1, &v); }, pushes);
        ft.push(m_flow, &m_scalar, &m_out1, &m_out3);
        if (pushes() != 5) fail("Ftle: the push after the refusals");
    }
    {
        const int nx = 11, ny = 7;
        rc_planview_params p{};
        const double H[9] = {3., 0., 2., 0., 3., 1., 0., 0., 1.};   // a cell of one metre is three pixels
        std::memcpy(p.H, H, sizeof(H));
        p.fx = 30.; p.fy = 30.; p.cx = 18.; p.cy = 11.; p.k1 = -0.0625; p.k2 = 0.;
        p.x0 = 0.; p.y0 = 0.; p.dx = 1.; p.dy = 1.; p.nx = nx; p.ny = ny; p.fps = 10.; p.max_gsd = 4.;
        rc::PlanView pv(pipe, p);
        Img plan(ny, nx, 2, 4), pmask(ny, nx, 1, 1), ppic(ny, nx, 3, 1);
        rc::Mat m_plan = plan.mat(), m_pmask = pmask.mat(), m_ppic = ppic.mat();
        for (int t = 0; t < 4; t++) {
            fill_flow(flow, t); fill_bgr(bgr, t);
            if (t < 3) pv.push(&m_flow, &m_bgr);
            else pv.push(&m_flow, &m_bgr, &m_plan, &m_pmask, &m_ppic);
        }
        keep(out, "PlanView: plan", plan); keep(out, "PlanView: mask", pmask); keep(out, "PlanView: picture", ppic);
        keep(out, "PlanView: summary", pv.read()); keep(out, "PlanView: table", pv.table());
        auto pushes = [&] { return pv.info().pushes; };
        refusals("PlanView::push flow", flow, [&](rc::Mat& v) { pv.push(&v, &m_bgr, &m_plan, &m_pmask, &m_ppic); }, pushes);
        refusals("PlanView::push frame", bgr, [&](rc::Mat& v) { pv.push(&m_flow, &v, &m_plan, &m_pmask, &m_ppic); }, pushes);
        refusals("PlanView::push plan", plan, [&](rc::Mat& v) { pv.push(&m_flow, &m_bgr, &v, &m_pmask, &m_ppic); }, pushes);
        refusals("PlanView::push mask", pmask, [&](rc::Mat& v) { pv.push(&m_flow, &m_bgr, &m_plan, &v, &m_ppic); }, pushes);
        refusals("PlanView::push picture", ppic, [&](rc::Mat& v) { pv.push(&m_flow, &m_bgr, &m_plan, &m_pmask, &v); }, pushes);
        pv.push(&m_flow, &m_bgr, &m_plan, &m_pmask, &m_ppic);
        if (pushes() != 5) fail("PlanView: the push after the refusals");
    }
    {
        rc_waves_params p{};
        p.window = 8; p.bin_lo = 1; p.bin_hi = 3; p.spacing = 2; p.grid_x = 3; p.grid_y = 2; p.min_pixels = 1;
        p.fps = 1.; p.metres_per_pixel_x = 1.; p.metres_per_pixel_y = 0.5; p.gravity = 9.8125; p.tanh_max = 0.9375; p.vis_max_depth = 2.;
        rc::Waves wv(pipe, p);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) mask.row(y)[x] = (unsigned char)((x >= 20 && x < 24 && y >= 10 && y < 14) ? 0 : 1 + (x + y) % 255);
        for (int t = 0; t < 4; t++) {
            fill_gray(gray, t);
            if (t < 3) wv.push(m_gray);
            else wv.push(m_gray, &m_mask, true, &m_out1, &m_out3);
        }
        keep(out, "Waves: bin_map", out1); keep(out, "Waves: picture", out3); keep(out, "Waves: summary", wv.read());
        keep(out, "Waves: cells", wv.cells()); keep(out, "Waves: sums", wv.sums());
        auto pushes = [&] { return wv.info().pushes; };
        refusals("Waves::push gray", gray, [&](rc::Mat& v) { wv.push(v, &m_mask, true, &m_out1, &m_out3); }, pushes);
        refusals("Waves::push mask", mask, [&](rc::Mat& v) { wv.push(m_gray, &v, true, &m_out1, &m_out3); }, pushes);
        refusals("Waves::push bin_map", out1, [&](rc::Mat& v) { wv.push(m_gray, &m_mask, true, &v, &m_out3); }, pushes);
        refusals("Waves::push picture", out3, [&](rc::Mat& v) { wv.push(m_gray, &m_mask, true, &m_out1, &v); }, pushes);
        wv.push(m_gray, &m_mask, true, &m_out1, &m_out3);
        if (pushes() != 5) fail("Waves: the push after the refusals");
    }
    {
        rc_piv_params p{};
        p.window = 8; p.range = 2; p.step = 5; p.ensemble = 2; p.flags = RC_PIV_REPLACE;
        p.min_peak = 0.25; p.median_eps = 0.125; p.median_thr = 2.; p.vis_max = 4.;
        rc::Piv piv(pipe, p);
        Img field(piv.grid_y(), piv.grid_x(), 2, 4);
        rc::Mat m_field = field.mat();
        for (int t = 0; t < 4; t++) {
            fill_gray(gray, t);
            if (t < 3) piv.push(m_gray);
            else piv.push(m_gray, true, &m_field, &m_out3);
        }
        keep(out, "Piv: field", field); keep(out, "Piv: picture", out3); keep(out, "Piv: summary", piv.read());
        keep(out, "Piv: cells", piv.cells()); keep(out, "Piv: sums", piv.sums());
        auto pushes = [&] { return piv.info().pushes; };
        refusals("Piv::push gray", gray, [&](rc::Mat& v) { piv.push(v, true, &m_field, &m_out3); }, pushes);
        refusals("Piv::push field", field, [&](rc::Mat& v) { piv.push(m_gray, true, &v, &m_out3); }, pushes);
        refusals("Piv::push picture", out3, [&](rc::Mat& v) { piv.push(m_gray, true, &m_field, &v); }, pushes);
        piv.push(m_gray, true, &m_field, &m_out3);
        if (pushes() != 5) fail("Piv: the push after the refusals");
    }
}

int main() {
    Results dense, padded;
    try {
        g_pad = 0; run(dense);
        g_pad = 5; run(padded);
    } catch (const std::exception& e) {
        std::printf("exception (padding %d): %s\n", g_pad, e.what());
        return 1;
    }
    if (dense.size() != padded.size()) fail("the two runs kept different numbers of results");
    for (size_t k = 0; k < dense.size() && k < padded.size(); k++)
        if (dense[k] != padded[k]) fail(dense[k].first + ": padded rows gave something else than dense rows");
    if (g_fails) return 1;
    std::printf("test_staging: ok (%zu results equal)\n", dense.size());
    return 0;
}
