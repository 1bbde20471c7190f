// rc::PlanView (include/rcflow_module.hpp) on 97 x 53 fields and frames made from integers (the field in sixteenths: exact in
// float, so tests/test_gpu_planview.py makes the same ones) through a camera whose numbers are all exact in double: plan
// 61 x 37 from (-30, -6) in cells of 1 x 1.5 m, k1 = -0.125, k2 = 0.03125, 10 fields per second, max_gsd 0.6.  Prints, per push,
// the summary, the counts of mask and picture pixels and the sum of the plan field's bit patterns for the test to hold
// against the numpy statement.
//   test_planview PUSHES
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_planview PUSHES\n"); return 2; }
    const int w = 97, h = 53, nx = 61, ny = 37, n = std::atoi(argv[1]);
    try {
        rc::Pipeline pipe(w, h);
        rc_planview_params p{};
        const double H[9] = {90., 45., 165., 0., -6.5625, 933.125, 0., 0.9375, 3.4375};
        std::memcpy(p.H, H, sizeof(H));
        p.fx = 90.; p.fy = 90.; p.cx = 48.; p.cy = 26.; p.k1 = -0.125; p.k2 = 0.03125;
        p.x0 = -30.; p.y0 = -6.; p.dx = 1.; p.dy = 1.5; p.nx = nx; p.ny = ny; p.fps = 10.; p.max_gsd = 0.6;
        rc::PlanView pv(pipe, p);
        const std::vector<float> tab = pv.table();
        long long usable = 0;
        for (size_t k = 0; k < (size_t)nx * ny; k++) usable += tab[8 * k + 7] != 0.f;
        std::printf("table %lld\n", usable);
        std::vector<float> f((size_t)w * h * 2), pl((size_t)nx * ny * 2);
        std::vector<unsigned char> img((size_t)w * h * 3), m((size_t)nx * ny), pic((size_t)nx * ny * 3);
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    f[2 * ((size_t)y * w + x)] = (float)((x * 7 + y * 3 + t * 5) % 32 - 12) / 16.f;
                    f[2 * ((size_t)y * w + x) + 1] = (float)((x * 5 + y * 11 + t * 3) % 32 - 18) / 16.f;
                    for (int c = 0; c < 3; c++) img[3 * ((size_t)y * w + x) + c] = (unsigned char)((x * 7 + y * 13 + c * 5 + t) % 256);
                }
            rc::Mat flow(h, w, 2, 4, f.data()), frame(h, w, 3, 1, img.data());
            rc::Mat plan(ny, nx, 2, 4, pl.data()), mask(ny, nx, 1, 1, m.data()), picture(ny, nx, 3, 1, pic.data());
            pv.push(&flow, &frame, &plan, &mask, &picture);
            const std::vector<long long> s = pv.read();
            const rc_planview_info i = pv.info();
            if (i.pushes != t + 1 || s[4] != t + 1 || s[0] != usable || i.launches_per_push != 1) { std::printf("bad counts\n"); return 1; }
            long long lit = 0, set = 0;
            unsigned long long bits = 0;
            for (size_t k = 0; k < m.size(); k++) {
                set += m[k] != 0;
                lit += (pic[3 * k] | pic[3 * k + 1] | pic[3 * k + 2]) != 0;
            }
            for (size_t k = 0; k < pl.size(); k++) { unsigned u; std::memcpy(&u, &pl[k], 4); bits += u; }
            std::printf("push %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %llu\n", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], set, lit, bits);
        }
        // the frame alone: no cell is valid, the picture is the same
        const std::vector<unsigned char> before = pic;
        rc::Mat frame(h, w, 3, 1, img.data()), picture(ny, nx, 3, 1, pic.data());
        pv.push(nullptr, &frame, nullptr, nullptr, &picture);
        const std::vector<long long> s = pv.read();
        if (pic != before || s[2] != 0 || s[3] != 0 || s[4] != n + 1) { std::printf("the push of the frame alone differs\n"); return 1; }
        // a refused open throws and leaves the session working
        bool threw = false;
        p.dx = 0.;
        try { rc::PlanView bad(pipe, p); } catch (const rc::Error& e2) { threw = e2.code == RC_EINVAL; }
        if (!threw || pv.info().pushes != n + 1 || pv.table() != tab) { std::printf("a pitch of 0 was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_planview: ok\n");
    return 0;
}
