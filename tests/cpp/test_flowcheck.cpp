// rc::FlowCheck (include/rcflow_module.hpp) against the C ABI it wraps, on one case of 70 x 50 pixels: a pattern made from integers
// that moves two pixels right and one down per frame, the true field (2, 1) with a patch of vectors that point the wrong way, one
// vector that is not a number and a backward field that closes the round trip outside the patch.  The class and the entry points
// called directly give the same flags, the same mask and the same summary; what must hold of them is computed here.
//   test_flowcheck
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)
#define HIP(call) do { if ((call) != hipSuccess) FAIL("%s failed", #call); } while (0)

static const int W = 70, H = 50;

static std::vector<unsigned char> frame(int t) {
    std::vector<unsigned char> f((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const int xs = x - 2 * t + 64, ys = y - t + 64;
            f[(size_t)y * W + x] = (unsigned char)((xs * xs * 7 + ys * ys * 13 + xs * ys * 3) % 251);
        }
    return f;
}

int main() {
    try {
        rc::Pipeline pipe(W, H);
        rc_flowcheck_params p;
        std::memset(&p, 0, sizeof(p));
        p.radius = 2; p.grid_x = 3; p.grid_y = 2; p.tests = RC_FLOWCHECK_RESID | RC_FLOWCHECK_FB | RC_FLOWCHECK_FAST; p.flags = RC_FLOWCHECK_FILL_NAN;
        p.tex_min = 0; p.gain_pm = 0; p.res_max = 1.5; p.fb_rel = 0.01; p.fb_abs = std::sqrt(0.5); p.speed_max = 4.0;
        const size_t N = (size_t)W * H;
        std::vector<unsigned char> f0 = frame(0), f1 = frame(1), f2 = frame(2);
        std::vector<float> flow(2 * N), back(2 * N);
        for (size_t i = 0; i < N; i++) { flow[2 * i] = 2.f; flow[2 * i + 1] = 1.f; back[2 * i] = -2.f; back[2 * i + 1] = -1.f; }
        for (int y = 20; y < 32; y++)
            for (int x = 30; x < 46; x++) { flow[2 * ((size_t)y * W + x)] = -1.5f; flow[2 * ((size_t)y * W + x) + 1] = 2.25f; }
        flow[2 * ((size_t)5 * W + 7)] = std::numeric_limits<float>::quiet_NaN();
        flow[2 * ((size_t)40 * W + 9)] = 4.5f;                    // faster than speed_max, and wrong
        std::vector<unsigned char> flags(N), mask(N), pic(3 * N);
        std::vector<float> checked(2 * N), resid(2 * N), texture(N);
        std::vector<long long> sa, sums_a;
        std::vector<rc_flowcheck_cell> cells_a;
        {
            rc::FlowCheck fc(pipe, p);
            rc::Mat m0(H, W, 1, 1, f0.data()), m1(H, W, 1, 1, f1.data()), m2(H, W, 1, 1, f2.data());
            rc::Mat mflow(H, W, 2, 4, flow.data()), mback(H, W, 2, 4, back.data());
            rc::Mat mflags(H, W, 1, 1, flags.data()), mmask(H, W, 1, 1, mask.data()), mpic(H, W, 3, 1, pic.data());
            rc::Mat mchecked(H, W, 2, 4, checked.data()), mresid(H, W, 2, 4, resid.data()), mtexture(H, W, 1, 4, texture.data());
            rc::FlowCheck::Pictures all;
            all.flags = &mflags; all.mask = &mmask; all.checked = &mchecked; all.resid = &mresid; all.texture = &mtexture; all.picture = &mpic;
            std::memset(flags.data(), 0xA5, N);
            fc.push(m0, nullptr, mflow, nullptr, all);            // the first push only stores its frame
            if (fc.read()[9] != 1 || fc.read()[8] != 0 || fc.info().held != 1 || flags[0] != 0xA5) FAIL("the first push computed");
            fc.push(m1, nullptr, mflow, &mback, all);             // frames 0 and 1
            sa = fc.read();
            if (sa[8] != 1 || sa[9] != 2) FAIL("counts %lld %lld", sa[8], sa[9]);
            fc.push(m2, &m1, mflow, &mback, all);                 // frames 1 and 2, both named: the same motion
            sa = fc.read(); cells_a = fc.cells(); sums_a = fc.sums();
            // what must hold
            long long valid = 0, cnt[7] = {0, 0, 0, 0, 0, 0, 0};
            for (size_t i = 0; i < N; i++) {
                const int fl = flags[i];
                valid += fl == 0;
                for (int k = 0; k < 7; k++) cnt[k] += fl >> k & 1;
                if ((mask[i] == 255) != (fl == 0)) FAIL("mask %zu", i);
                if (fl == 0 ? (checked[2 * i] != flow[2 * i] || checked[2 * i + 1] != flow[2 * i + 1]) : !(std::isnan(checked[2 * i]) && std::isnan(checked[2 * i + 1])))
                    FAIL("checked %zu", i);
                if (fl == 0 && (pic[3 * i] != f1[i] || pic[3 * i + 1] != f1[i] || pic[3 * i + 2] != f1[i])) FAIL("picture %zu", i);
                if (!(texture[i] >= 0.f)) FAIL("texture %zu", i);
            }
            if (flags[(size_t)5 * W + 7] != RC_FLOWCHECK_BAD) FAIL("the NaN vector has flags %d", flags[(size_t)5 * W + 7]);
            if (!(flags[(size_t)40 * W + 9] & RC_FLOWCHECK_FAST)) FAIL("the fast vector has flags %d", flags[(size_t)40 * W + 9]);
            for (int y = 22; y < 30; y++)
                for (int x = 32; x < 44; x++)
                    if (!(flags[(size_t)y * W + x] & RC_FLOWCHECK_RESID) || !(flags[(size_t)y * W + x] & RC_FLOWCHECK_FB)) FAIL("the wrong patch at (%d, %d): %d", x, y, flags[(size_t)y * W + x]);
            for (int y = 4; y < 16; y++)
                for (int x = 12; x < 60; x++)
                    if (flags[(size_t)y * W + x] != 0 || resid[2 * ((size_t)y * W + x)] != 0.f) FAIL("the true field at (%d, %d): %d", x, y, flags[(size_t)y * W + x]);
            if (sa[0] != valid || valid == 0) FAIL("valid %lld, counted %lld", sa[0], valid);
            for (int k = 0; k < 7; k++)
                if (sa[1 + k] != cnt[k]) FAIL("count %d: %lld, counted %lld", k, sa[1 + k], cnt[k]);
            if (sa[8] != 2 || sa[9] != 3 || cnt[0] != 1 || cnt[1] == 0 || cnt[2] != 0 || cnt[4] != 0) FAIL("summary");
            long long cv = 0, cp = 0;
            for (size_t k = 0; k < cells_a.size(); k++) {
                if (cells_a[k].valid != sums_a[RC_FLOWCHECK_SUMS * k] || cells_a[k].valid_pm != cells_a[k].valid * 1000 / cells_a[k].pixels) FAIL("cell %zu", k);
                cv += cells_a[k].valid; cp += cells_a[k].pixels;
            }
            if (cells_a.size() != 6 || cv != valid || cp != (long long)N || std::fabs(cells_a[0].mean_x - 2.f) > 1e-6f) FAIL("cells");
            fc.set(RC_FLOWCHECK_FAST, 0, 0., 0, 0., 0., 1.0);     // from the next push on: every vector of this field is too fast
            fc.push(m2, &m1, mflow);
            if (fc.read()[0] != 0 || fc.read()[7] != (long long)N - 1) FAIL("after set: %lld valid", fc.read()[0]);
            fc.reset();
            if (fc.info().held != 0 || fc.info().pushes != 4 || fc.read()[0] != 0 || fc.info().prm.tests != RC_FLOWCHECK_FAST) FAIL("reset");
            bool threw = false;
            try { fc.push(m2, nullptr, mflow); } catch (const rc::Error& e) { threw = e.code == RC_ESTATE; }
            if (!threw) FAIL("a push without a previous frame after a reset was accepted");
            threw = false;
            try { fc.push(mflags, &m1, mflow, &mflags); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw) FAIL("a grey picture was accepted as a field");
            threw = false;
            rc_flowcheck_params q = p;
            q.flags = RC_FLOWCHECK_FILL_NAN | RC_FLOWCHECK_FILL_ZERO;
            try { rc::FlowCheck two(pipe, q); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw || fc.info().w != W) FAIL("both fills were accepted");
        }
        // the same pair through the entry points themselves
        rc_ctx* ctx = pipe.context();
        if (rcflow_flowcheck_open(ctx, 0, W, H, &p) != RC_OK) FAIL("open: %s", rcflow_last_error());
        unsigned char *d1 = nullptr, *d2 = nullptr, *dflags = nullptr, *dmask = nullptr;
        float *dflow = nullptr, *dback = nullptr;
        HIP(hipMalloc((void**)&d1, N)); HIP(hipMalloc((void**)&d2, N)); HIP(hipMalloc((void**)&dflags, N)); HIP(hipMalloc((void**)&dmask, N));
        HIP(hipMalloc((void**)&dflow, 8 * N)); HIP(hipMalloc((void**)&dback, 8 * N));
        HIP(hipMemcpy(d1, f1.data(), N, hipMemcpyHostToDevice)); HIP(hipMemcpy(d2, f2.data(), N, hipMemcpyHostToDevice));
        HIP(hipMemcpy(dflow, flow.data(), 8 * N, hipMemcpyHostToDevice)); HIP(hipMemcpy(dback, back.data(), 8 * N, hipMemcpyHostToDevice));
        for (int t = 0; t < 2; t++)                               // the counts of the class's session: a push that only stores, then one that computes
            if (rcflow_flowcheck_push_dev(ctx, 0, d1, W, nullptr, 0, dflow, 8 * W, dback, 8 * W, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0,
                                          nullptr, 0, nullptr, nullptr, nullptr) != RC_OK)
                FAIL("push: %s", rcflow_last_error());
        if (rcflow_flowcheck_push_dev(ctx, 0, d2, W, d1, W, dflow, 8 * W, dback, 8 * W, dflags, W, dmask, W, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0,
                                      nullptr, nullptr, nullptr) != RC_OK)
            FAIL("push: %s", rcflow_last_error());
        long long sb[RC_FLOWCHECK_SUMMARY];
        std::vector<long long> sums_b(sums_a.size());
        std::vector<rc_flowcheck_cell> cells_b(cells_a.size());
        if (rcflow_flowcheck_read(ctx, 0, cells_b.data(), sums_b.data(), sb) != RC_OK) FAIL("read: %s", rcflow_last_error());
        std::vector<unsigned char> flags_b(N), mask_b(N);
        HIP(hipMemcpy(flags_b.data(), dflags, N, hipMemcpyDeviceToHost)); HIP(hipMemcpy(mask_b.data(), dmask, N, hipMemcpyDeviceToHost));
        for (int k = 0; k < RC_FLOWCHECK_SUMMARY; k++)
            if (sb[k] != sa[k]) FAIL("summary word %d: the class %lld, the entry points %lld", k, sa[k], sb[k]);
        if (sums_b != sums_a || std::memcmp(cells_b.data(), cells_a.data(), cells_a.size() * sizeof(rc_flowcheck_cell))) FAIL("sums or records differ");
        if (flags_b != flags || mask_b != mask) FAIL("flags or mask differ");
        if (rcflow_flowcheck_close(ctx, 0) != RC_OK) FAIL("close");
        (void)hipFree(d1); (void)hipFree(d2); (void)hipFree(dflags); (void)hipFree(dmask); (void)hipFree(dflow); (void)hipFree(dback);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_flowcheck: ok\n");
    return 0;
}
