// rc::RipMap (include/rcflow_module.hpp) on a seeded sequence of flow fields; prints, per push, the counts and the cell
// sums for tests/test_gpu_ripmap.py to hold against the ctypes session on the same fields.
//   test_ripmap W H WINDOW GRID_X GRID_Y PUSHES
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: test_ripmap W H WINDOW GRID_X GRID_Y PUSHES\n"); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), window = std::atoi(argv[3]), gx = std::atoi(argv[4]),
              gy = std::atoi(argv[5]), n = std::atoi(argv[6]);
    try {
        rc::Pipeline pipe(w, h);
        rc::RipMap map(pipe, window, gx, gy);
        std::vector<float> f((size_t)w * h * 2);
        std::vector<unsigned char> mask((size_t)w * h);
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    f[((size_t)y * w + x) * 2] = (float)((x * 7 + y * 3 + t * 11) % 17 - 8) / 4.f;
                    f[((size_t)y * w + x) * 2 + 1] = (float)((x * 5 + y * 13 + t * 7) % 19 - 9) / 4.f;
                }
            rc::Mat flow(h, w, 2, 4, f.data());
            map.push(flow);
            const rc::RipMap::Result r = map.read();
            if (r.frames_pushed != t + 1 || (int)r.cells.size() != gx * gy) { std::printf("bad result shape\n"); return 1; }
            rc::Mat m(h, w, 1, 1, mask.data());
            map.mask(m);
            long long marked = 0, want = 0;
            for (unsigned char v : mask) marked += v == 255;
            for (int cy = 0; cy < gy; cy++)
                for (int cx = 0; cx < gx; cx++)
                    if (r.opposed(cx, cy)) want += r.sums[((size_t)cy * gx + cx) * 3 + 2];
            if (marked != want && r.bad_pixels == 0) { std::printf("mask marks %lld pixels, the cells hold %lld\n", marked, want); return 1; }
            std::printf("push %d %lld %lld %lld", t + 1, r.opposed_cells, r.live_cells, r.bad_pixels);
            for (long long v : r.sums) std::printf(" %lld", v);
            std::printf("\n");
        }
        // a refused open throws and leaves nothing behind
        bool threw = false;
        try { rc::RipMap bad(pipe, 0, gx, gy); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) { std::printf("window 0 was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_ripmap: ok\n");
    return 0;
}
