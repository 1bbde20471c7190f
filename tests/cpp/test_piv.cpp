// rc::Piv (include/rcflow_module.hpp) on 70 x 50 grey frames made from integers, so tests/test_gpu_piv.py makes the same ones: a
// pattern that moves two pixels right and one down per frame, windows of 16 every 10 pixels searched over +-4, an ensemble of
// 3, outliers replaced.  Every third push computes and prints the summary, the sums of the accumulators, of the cells' own
// sums and of the picture, and each cell's integer peak and flags for the test to hold against the numpy statement.
//   test_piv PUSHES
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_piv PUSHES\n"); return 2; }
    const int w = 70, h = 50, n = std::atoi(argv[1]);
    try {
        rc::Pipeline pipe(w, h);
        rc_piv_params p{};
        p.window = 16; p.range = 4; p.step = 10; p.ensemble = 3; p.flags = RC_PIV_REPLACE;
        p.min_peak = 0.25; p.median_eps = 0.125; p.median_thr = 2.; p.vis_max = 4.;
        rc::Piv piv(pipe, p);
        if (piv.grid_x() != 5 || piv.grid_y() != 3) { std::printf("bad grid\n"); return 1; }
        std::vector<unsigned char> g((size_t)w * h), pic((size_t)w * h * 3);
        std::vector<float> fl((size_t)piv.grid_x() * piv.grid_y() * 2);
        rc::Mat picture(h, w, 3, 1, pic.data()), field(piv.grid_y(), piv.grid_x(), 2, 4, fl.data());
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const int xs = x - 2 * t + 64, ys = y - t + 64;
                    g[(size_t)y * w + x] = (unsigned char)(((xs * xs * 7 + ys * ys * 13 + xs * ys * 3) % 251 + (x * y + t) % 5) % 256);
                }
            rc::Mat gray(h, w, 1, 1, g.data());
            if (t % 3 != 2) { piv.push(gray); continue; }
            piv.push(gray, true, &field, &picture);
            const std::vector<long long> s = piv.read(), ts = piv.sums(), cs = piv.cell_sums();
            const std::vector<rc_piv_cell> c = piv.cells();
            const rc_piv_info i = piv.info();
            if (i.pushes != t + 1 || s[7] != t + 1 || i.pairs != s[0] || i.launches_per_push != RC_PIV_LAUNCHES) { std::printf("bad counts\n"); return 1; }
            long long st = 0, sc = 0, sp = 0;
            for (long long v : ts) st += v;
            for (long long v : cs) sc += v;
            for (unsigned char v : pic) sp += v;
            std::printf("push %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], st, sc, sp);
            for (size_t k = 0; k < c.size(); k++) {
                // the field is the record's displacement where the cell is valid and no outlier
                if (!(c[k].flags & (RC_PIV_EMPTY | RC_PIV_FLAT | RC_PIV_LOWPEAK | RC_PIV_OUTLIER)) && (fl[2 * k] != c[k].dx || fl[2 * k + 1] != c[k].dy)) {
                    std::printf("the field differs from the records\n");
                    return 1;
                }
                std::printf(" %d %d %d", c[k].ix, c[k].iy, c[k].flags);
            }
            std::printf("\n");
        }
        // a refused open throws and leaves the session working
        const long long before = piv.info().pushes;
        bool threw = false;
        p.window = 18;                                            // no multiple of 4
        try { rc::Piv bad(pipe, p); } catch (const rc::Error& e2) { threw = e2.code == RC_EINVAL; }
        if (!threw || piv.info().pushes != before || piv.info().prm.window != 16) { std::printf("a window of 18 was accepted\n"); return 1; }
        piv.reset();
        if (piv.info().pushes != 0 || piv.read()[7] != 0) { std::printf("reset left something\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_piv: ok\n");
    return 0;
}
