// rc::Outlines (include/rcflow_module.hpp) against the C ABI it wraps and against figures of the sequential statement
// (tests/_outlines_ref.py) compiled in: 96 x 64 labels, label 1 a rectangle x 10..39, y 8..29 with a hole x 20..24, y 15..19, label 2
// a disc of radius 15 at (70, 40), label 3 the diagonal pair (50, 50), (51, 51); connectivity 8, 16 records, 512 vertices.
//   test_outlines
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)
#define HIP(call) do { if ((call) != hipSuccess) FAIL("%s failed", #call); } while (0)

static const int W = 96, H = 64, LOOPS = 16, VERTS = 512;
static const long long SUMMARY[RC_OUTLINES_SUMMARY] = {256, 4, 4, 4, 92, 92, 0, 1};
// label, flags, x, y, cracks, verts, offset, pad, x0, y0, x1, y1, area2
static const long long RECORDS[4][13] = {{1, 0, 10, 8, 104, 4, 0, 0, 10, 8, 40, 30, 1320},
                                         {1, RC_OUTLINE_HOLE, 20, 14, 20, 4, 4, 0, 20, 15, 25, 20, -50},
                                         {2, 0, 70, 25, 124, 76, 8, 0, 55, 25, 86, 56, 1418},
                                         {3, 0, 50, 50, 8, 8, 84, 0, 50, 50, 52, 52, 4}};

static bool record_is(const rc_outline_loop& r, const long long* q) {
    const long long got[13] = {r.label, r.flags, r.x, r.y, r.cracks, r.verts, r.offset, r.pad, r.x0, r.y0, r.x1, r.y1, r.area2};
    return !std::memcmp(got, q, sizeof(got));
}

int main() {
    try {
        rc::Pipeline pipe(W, H);
        rc_outlines_params p;
        std::memset(&p, 0, sizeof(p));
        p.connectivity = 8; p.min_cracks = 4; p.max_cracks = 4096; p.max_loops = LOOPS; p.max_vertices = VERTS;
        const size_t N = (size_t)W * H;
        std::vector<int32_t> lab(N, 0);
        std::vector<unsigned char> mask(N), img(3 * N, 0), img2(3 * N, 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                int32_t& l = lab[(size_t)y * W + x];
                if (x >= 10 && x < 40 && y >= 8 && y < 30) l = 1;
                if (x >= 20 && x < 25 && y >= 15 && y < 20) l = 0;
                if ((x - 70) * (x - 70) + (y - 40) * (y - 40) <= 225) l = 2;
            }
        lab[(size_t)50 * W + 50] = lab[(size_t)51 * W + 51] = 3;
        for (size_t i = 0; i < N; i++) mask[i] = lab[i] ? 255 : 0;
        rc::OutlinesResult a;
        {
            rc::Outlines ol(pipe, p);
            rc::Mat mlab(H, W, 1, 4, lab.data()), mmask(H, W, 1, 1, mask.data()), mimg(H, W, 3, 1, img.data());
            const rc_outlines_info info = ol.info();
            if (info.rounds != 12 || info.launches_per_push != RC_OUTLINES_FIXED_LAUNCHES + 24 || info.pushes != 0) FAIL("info");
            if (!ol.read().loops.empty() || ol.read().summary[0]) FAIL("records before any push");
            ol.push(mlab);
            a = ol.read();
            for (int k = 0; k < RC_OUTLINES_SUMMARY; k++)
                if (a.summary[k] != SUMMARY[k]) FAIL("summary word %d: %lld, the statement %lld", k, a.summary[k], SUMMARY[k]);
            if (a.loops.size() != 4 || a.verts.size() != 2 * 92) FAIL("sizes %zu %zu", a.loops.size(), a.verts.size());
            for (int k = 0; k < 4; k++)
                if (!record_is(a.loops[k], RECORDS[k])) FAIL("record %d", k);
            // every polygon is closed and rectilinear, its sides alternate, and its shoelace sum is the record's area2
            for (const rc_outline_loop& r : a.loops) {
                long long s = 0;
                for (int j = 0; j < r.verts; j++) {
                    const int32_t* u = &a.verts[2 * (size_t)(r.offset + j)];
                    const int32_t* v = &a.verts[2 * (size_t)(r.offset + (j + 1) % r.verts)];
                    const int32_t* t = &a.verts[2 * (size_t)(r.offset + (j + 2) % r.verts)];
                    if ((u[0] == v[0]) == (u[1] == v[1]) || (u[0] == v[0]) == (v[0] == t[0])) FAIL("loop %d is not rectilinear at vertex %d", r.label, j);
                    s += (long long)u[0] * v[1] - (long long)v[0] * u[1];
                }
                if (s != r.area2) FAIL("loop of label %d: shoelace %lld, area2 %lld", r.label, s, r.area2);
            }
            if (a.verts[0] != 40 || a.verts[1] != 8) FAIL("the first vertex is (%d, %d)", a.verts[0], a.verts[1]);
            ol.draw(mimg, 0x0000ff, 1);
            // the mask: the same shapes as one label
            ol.push(mmask);
            const rc::OutlinesResult m = ol.read();
            if (m.summary[0] != 256 || m.summary[1] != 4 || m.summary[7] != 2 || m.loops[0].label != 1 || m.loops[2].label != 1 || m.loops[2].cracks != 124) FAIL("the mask");
            ol.setMinCracks(9);
            ol.push(mlab);
            const rc::OutlinesResult f = ol.read();
            if (f.summary[1] != 4 || f.summary[2] != 3 || f.loops.size() != 3 || f.loops[2].label != 2 || f.loops[2].offset != 8) FAIL("the filter");
            bool threw = false;
            std::vector<float> flow(2 * N);
            rc::Mat mflow(H, W, 2, 4, flow.data());
            try { ol.push(mflow); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw) FAIL("a flow field was accepted as a plane");
            threw = false;
            rc_outlines_params q = p;
            q.connectivity = 6;
            try { rc::Outlines two(pipe, q); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw || ol.info().pushes != 3 || ol.info().prm.min_cracks != 9) FAIL("connectivity 6 was accepted, or the refusal touched the state");
            ol.reset();
            if (ol.info().pushes != 0 || !ol.read().loops.empty()) FAIL("reset");
        }
        // the same through the entry points themselves
        rc_ctx* ctx = pipe.context();
        if (rcflow_outlines_open(ctx, 0, W, H, &p) != RC_OK) FAIL("open: %s", rcflow_last_error());
        int32_t *dlab = nullptr, *dverts = nullptr; rc_outline_loop* dloops = nullptr; long long* dsum = nullptr; rc_draw_prim* dprims = nullptr;
        unsigned char* dimg = nullptr;
        HIP(hipMalloc((void**)&dlab, 4 * N)); HIP(hipMalloc((void**)&dverts, 8 * VERTS)); HIP(hipMalloc((void**)&dloops, LOOPS * sizeof(rc_outline_loop)));
        HIP(hipMalloc((void**)&dsum, 8 * RC_OUTLINES_SUMMARY)); HIP(hipMalloc((void**)&dprims, VERTS * sizeof(rc_draw_prim))); HIP(hipMalloc((void**)&dimg, 3 * N));
        HIP(hipMemcpy(dlab, lab.data(), 4 * N, hipMemcpyHostToDevice)); HIP(hipMemset(dimg, 0, 3 * N));
        if (rcflow_outlines_push_dev(ctx, 0, dlab, 4 * W, nullptr, 0, dloops, dverts, dsum) != RC_OK) FAIL("push: %s", rcflow_last_error());
        if (rcflow_outlines_prims_dev(ctx, 0, 0x0000ff, 1, dprims) != RC_OK) FAIL("prims: %s", rcflow_last_error());
        if (rcflow_draw_dev(ctx, 0, dimg, 3 * W, W, H, 3, dprims, VERTS, nullptr) != RC_OK) FAIL("draw: %s", rcflow_last_error());
        std::vector<rc_outline_loop> lb(LOOPS), lr(LOOPS);
        std::vector<int32_t> vb(2 * VERTS), vr(2 * VERTS);
        long long sb[RC_OUTLINES_SUMMARY], sr[RC_OUTLINES_SUMMARY];
        int n = 0, nv = 0;
        if (rcflow_outlines_read(ctx, 0, lr.data(), LOOPS, &n, vr.data(), VERTS, &nv, sr) != RC_OK) FAIL("read: %s", rcflow_last_error());
        HIP(hipMemcpy(lb.data(), dloops, LOOPS * sizeof(rc_outline_loop), hipMemcpyDeviceToHost)); HIP(hipMemcpy(vb.data(), dverts, 8 * VERTS, hipMemcpyDeviceToHost));
        HIP(hipMemcpy(sb, dsum, sizeof(sb), hipMemcpyDeviceToHost)); HIP(hipMemcpy(img2.data(), dimg, 3 * N, hipMemcpyDeviceToHost));
        if (n != 4 || nv != 92 || std::memcmp(sb, a.summary, sizeof(sb)) || std::memcmp(sr, a.summary, sizeof(sr))) FAIL("the entry points' summary");
        if (std::memcmp(lb.data(), a.loops.data(), 4 * sizeof(rc_outline_loop)) || std::memcmp(lr.data(), a.loops.data(), 4 * sizeof(rc_outline_loop))) FAIL("the entry points' records");
        if (std::memcmp(vb.data(), a.verts.data(), 8 * 92) || std::memcmp(vr.data(), a.verts.data(), 8 * 92)) FAIL("the entry points' vertices");
        for (size_t i = 4 * sizeof(rc_outline_loop); i < LOOPS * sizeof(rc_outline_loop); i++) if (((const char*)lb.data())[i]) FAIL("the records' tail is not zero");
        for (size_t i = 2 * 92; i < 2 * (size_t)VERTS; i++) if (vb[i]) FAIL("the vertices' tail is not zero");
        long long lit = 0;
        for (size_t i = 0; i < N; i++) lit += img[3 * i] == 255;
        if (img != img2 || lit < 150 || img[3 * ((size_t)8 * W + 10)] != 255 || img[3 * ((size_t)30 * W + 40)] != 255 || img[3 * ((size_t)12 * W + 15)]) FAIL("the drawing (%lld pixels)", lit);
        if (rcflow_outlines_close(ctx, 0) != RC_OK) FAIL("close");
        (void)hipFree(dlab); (void)hipFree(dverts); (void)hipFree(dloops); (void)hipFree(dsum); (void)hipFree(dprims); (void)hipFree(dimg);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_outlines: ok\n");
    return 0;
}
