// rc::Transects (include/rcflow_module.hpp) against the C ABI on one case: 70 x 50 grey frames and flow fields made from
// integers, two lines (one slanted, at fractional positions), a window of 4 rows, grey rows correlated over +-3 samples with the
// row before.  The class gets every frame and computes at every third push; a second context gets the same frames through
// rcflow_transects_push_dev on device memory of its own and computes at every push.  Where both computed, every output must be
// equal byte for byte: records, summary, per-line sums, accumulators, profile, time stack and Hovmoeller picture.
//   test_transects PUSHES
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define HIP_OK(call) do { if ((call) != hipSuccess) { std::printf("%s failed\n", #call); return 1; } } while (0)
#define RC_OK_(call) do { if ((call) != RC_OK) { std::printf("%s failed: %s\n", #call, rcflow_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_transects PUSHES\n"); return 2; }
    const int w = 70, h = 50, n = std::atoi(argv[1]), T = 4;
    const std::vector<rc_transect_line> lines = {{4.f, 25.f, 65.f, 25.f, 62}, {10.5f, 45.25f, 60.f, 3.f, 33}};
    rc_transects_params p{};
    p.window = T; p.sources = RC_TRANSECTS_GRAY | RC_TRANSECTS_FLOW; p.lag = 1; p.range = 3;
    p.fps = 25.; p.metres_per_pixel = 0.25; p.jet_min = 0.5; p.vis_max = 4.;
    rc_ctx* abi = nullptr;
    try {
        rc::Pipeline pipe(w, h);
        rc::Transects ts(pipe, lines, p);
        const int L = ts.lines(), S = ts.samples();
        if (L != 2 || S != 95) { std::printf("bad geometry\n"); return 1; }
        RC_OK_(rcflow_create(&abi, 0, w, h, 1));
        RC_OK_(rcflow_transects_open(abi, 0, w, h, lines.data(), L, &p));
        // the table of the class is the stateless plan's
        std::vector<rc_transect_sample> tab((size_t)S);
        std::vector<rc_transect_geom> geo((size_t)L);
        int total = 0;
        RC_OK_(rcflow_transects_plan(w, h, lines.data(), L, p.metres_per_pixel, p.fps, tab.data(), geo.data(), &total));
        if (total != S || std::memcmp(tab.data(), ts.table().data(), (size_t)S * sizeof(rc_transect_sample)) ||
            std::memcmp(geo.data(), ts.geometry().data(), (size_t)L * sizeof(rc_transect_geom))) { std::printf("the table differs from the plan\n"); return 1; }

        unsigned char *d_g, *d_stack, *d_hov;
        float *d_f, *d_prof;
        rc_transect* d_rec;
        long long *d_sums, *d_summ;
        HIP_OK(hipMalloc(&d_g, (size_t)w * h)); HIP_OK(hipMalloc(&d_f, (size_t)w * h * 8));
        HIP_OK(hipMalloc(&d_stack, (size_t)S * T)); HIP_OK(hipMalloc(&d_hov, (size_t)S * T * 3));
        HIP_OK(hipMalloc(&d_prof, (size_t)S * 8)); HIP_OK(hipMalloc(&d_rec, (size_t)L * sizeof(rc_transect)));
        HIP_OK(hipMalloc(&d_sums, (size_t)L * RC_TRANSECTS_SUMS * 8)); HIP_OK(hipMalloc(&d_summ, 64));

        std::vector<unsigned char> g((size_t)w * h), stack((size_t)S * T), hov((size_t)S * T * 3), stack2(stack.size()), hov2(hov.size());
        std::vector<float> f((size_t)w * h * 2), prof((size_t)S * 2), prof2(prof.size());
        std::vector<rc_transect> rec2((size_t)L);
        std::vector<long long> sums2((size_t)L * RC_TRANSECTS_SUMS), summ2(8), acc2((size_t)L * 7 * 3);
        int velocities = 0, jets = 0;
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const int xs = x - 2 * t + 64, ys = y + 64;                      // the pattern moves two pixels right per frame
                    g[(size_t)y * w + x] = (unsigned char)((xs * xs * 7 + ys * ys * 13 + xs * ys * 3) % 251);
                    f[2 * ((size_t)y * w + x)] = (float)((x * 5 + y * 3 + t) % 17 - 8) / 8.f;
                    f[2 * ((size_t)y * w + x) + 1] = (float)((x * x + y + 2 * t) % 23 - 11) / 8.f;
                }
            HIP_OK(hipMemcpy(d_g, g.data(), g.size(), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(d_f, f.data(), f.size() * 4, hipMemcpyHostToDevice));
            RC_OK_(rcflow_transects_push_dev(abi, 0, d_g, (size_t)w, d_f, (size_t)w * 8, d_rec, d_sums, d_prof, d_stack, (size_t)S, d_hov, (size_t)S * 3, d_summ));
            rc::Mat gray(h, w, 1, 1, g.data()), flow(h, w, 2, 4, f.data());
            if (t % 3 != 2) { ts.push(&gray, &flow); continue; }
            rc::Mat mp(1, S, 2, 4, prof.data()), ms(T, S, 1, 1, stack.data()), mh(T, S, 3, 1, hov.data());
            ts.push(&gray, &flow, true, &mp, &ms, &mh);
            RC_OK_(rcflow_transects_read(abi, 0, rec2.data(), summ2.data()));
            RC_OK_(rcflow_transects_sums_read(abi, 0, acc2.data(), nullptr));
            HIP_OK(hipMemcpy(sums2.data(), d_sums, sums2.size() * 8, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(prof2.data(), d_prof, prof2.size() * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(stack2.data(), d_stack, stack2.size(), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(hov2.data(), d_hov, hov2.size(), hipMemcpyDeviceToHost));
            const std::vector<long long> s = ts.read(), ls = ts.line_sums(), acc = ts.sums();
            const std::vector<rc_transect> r = ts.records();
            const rc_transects_info i = ts.info();
            if (i.pushes != t + 1 || s[6] != t + 1 || i.pairs != s[1] || i.held != s[0] || i.launches_per_push != RC_TRANSECTS_LAUNCHES) { std::printf("bad counts\n"); return 1; }
            if (s != summ2 || ls != sums2 || acc != acc2 || std::memcmp(r.data(), rec2.data(), (size_t)L * sizeof(rc_transect))) {
                std::printf("records, sums or summary differ from the C ABI's at push %d\n", t + 1);
                return 1;
            }
            if (std::memcmp(prof.data(), prof2.data(), prof.size() * 4) || stack != stack2 || hov != hov2) {
                std::printf("profile or pictures differ from the C ABI's at push %d\n", t + 1);
                return 1;
            }
            // the newest row of the stack is the lowest held one and is not empty
            long long newest = 0;
            for (int k = 0; k < S; k++) newest += stack[(size_t)(i.held - 1) * S + k];
            if (!newest) { std::printf("the newest row of the stack is empty\n"); return 1; }
            for (const rc_transect& q : r) { velocities += !(q.flags & (RC_TRANSECTS_EMPTY | RC_TRANSECTS_FLAT)); jets += q.jets; }
            std::printf("push %d: held %lld pairs %lld shift %d v_along %g jets %d\n", t + 1, s[0], s[1], r[0].peak_shift, r[0].v_along, r[0].jets + r[1].jets);
        }
        if (n >= 3 && (!velocities || !jets)) { std::printf("no velocity or no jet in the whole run\n"); return 1; }
        // a refused open throws and leaves the session working; wrong views are refused before anything is copied
        const long long before = ts.info().pushes;
        bool threw = false;
        rc_transects_params bad = p;
        bad.window = 1;
        try { rc::Transects again(pipe, lines, bad); } catch (const rc::Error& e2) { threw = e2.code == RC_EINVAL; }
        if (!threw || ts.info().pushes != before || ts.info().prm.window != T) { std::printf("a window of 1 was accepted\n"); return 1; }
        threw = false;
        rc::Mat small(h, w - 1, 1, 1, g.data()), flow(h, w, 2, 4, f.data());
        try { ts.push(&small, &flow); } catch (const rc::Error& e2) { threw = e2.code == RC_EINVAL; }
        if (!threw || ts.info().pushes != before) { std::printf("a frame of another size was accepted\n"); return 1; }
        ts.set(1., 2.);
        if (ts.info().prm.jet_min != 1. || ts.info().prm.vis_max != 2.) { std::printf("set left the parameters\n"); return 1; }
        ts.reset();
        if (ts.info().pushes != 0 || ts.read()[6] != 0) { std::printf("reset left something\n"); return 1; }
        RC_OK_(rcflow_transects_close(abi, 0));
        for (void* q : {(void*)d_g, (void*)d_f, (void*)d_stack, (void*)d_hov, (void*)d_prof, (void*)d_rec, (void*)d_sums, (void*)d_summ}) (void)hipFree(q);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    if (abi) rcflow_destroy(abi);
    std::printf("test_transects: ok\n");
    return 0;
}
