// rc::Waves (include/rcflow_module.hpp) on 61 x 37 grey frames made from integers, so tests/test_gpu_waves.py makes the same
// ones: a window of 16 frames, bins 2..5, spacing 2, a grid of 3 x 2 cells, a mask with a hole.  Every push but the fourth of
// each five only stores; the computing ones print the summary, each cell's bin and flags, and the sums of the cell sums, of the
// spectrum, of the bin map and of the picture for the test to hold against the numpy statement.
//   test_waves PUSHES
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_waves PUSHES\n"); return 2; }
    const int w = 61, h = 37, n = std::atoi(argv[1]);
    try {
        rc::Pipeline pipe(w, h);
        rc_waves_params p{};
        p.window = 16; p.bin_lo = 2; p.bin_hi = 5; p.spacing = 2; p.grid_x = 3; p.grid_y = 2; p.min_pixels = 1;
        p.fps = 1.; p.metres_per_pixel_x = 1.; p.metres_per_pixel_y = 0.5; p.gravity = 9.8125; p.tanh_max = 0.9375; p.vis_max_depth = 2.;
        rc::Waves wv(pipe, p);
        std::vector<unsigned char> g((size_t)w * h), m((size_t)w * h), bm((size_t)w * h), pic((size_t)w * h * 3);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) m[(size_t)y * w + x] = (unsigned char)((x >= 30 && x < 34 && y >= 10 && y < 14) ? 0 : 1 + (x + y) % 255);
        rc::Mat mask(h, w, 1, 1, m.data()), bin_map(h, w, 1, 1, bm.data()), picture(h, w, 3, 1, pic.data());
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) g[(size_t)y * w + x] = (unsigned char)((x * 37 + y * 11 + t * 48 + (x * y * (t + 1)) % 23) % 256);
            rc::Mat gray(h, w, 1, 1, g.data());
            if (t % 5 != 3) { wv.push(gray); continue; }
            wv.push(gray, &mask, true, &bin_map, &picture);
            const std::vector<long long> s = wv.read(), cs = wv.sums();
            const std::vector<rc_wave_cell> c = wv.cells();
            const std::vector<int32_t> a = wv.spectrum();
            const rc_waves_info i = wv.info();
            if (i.pushes != t + 1 || s[4] != t + 1 || i.bins != 4 || i.launches_per_push != RC_WAVES_LAUNCHES) { std::printf("bad counts\n"); return 1; }
            long long sa = 0, sc = 0, sb = 0, sp = 0;
            for (int32_t v : a) sa += v;
            for (long long v : cs) sc += v;
            for (unsigned char v : bm) sb += v;
            for (unsigned char v : pic) sp += v;
            std::printf("push %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], sa, sc, sb, sp);
            for (const rc_wave_cell& r : c) std::printf(" %d %d", r.bin, r.flags);
            std::printf("\n");
        }
        // a refused open throws and leaves the session working
        const long long before = wv.info().pushes;
        bool threw = false;
        p.bin_hi = 8;                                             // 2 * 8 is not below 16
        try { rc::Waves bad(pipe, p); } catch (const rc::Error& e2) { threw = e2.code == RC_EINVAL; }
        if (!threw || wv.info().pushes != before || wv.info().prm.bin_hi != 5) { std::printf("a bin at half the window was accepted\n"); return 1; }
        wv.reset();
        if (wv.info().pushes != 0 || wv.read()[4] != 0) { std::printf("reset left something\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_waves: ok\n");
    return 0;
}
