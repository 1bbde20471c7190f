// rc::MotionTemplates (include/rcflow_module.hpp) on the +x bar of tests/_motion_ref.py (9 px wide, 200 on 50, 1 px per frame
// on 67 x 45; threshold 30, duration 8, deltas 0.5 and 2.5, automatic stamps); prints, per push, the frame's record for
// tests/test_gpu_motion.py to hold against the numpy statement.
//   test_motion PUSHES
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_motion PUSHES\n"); return 2; }
    const int w = 67, h = 45, n = std::atoi(argv[1]);
    try {
        rc::Pipeline pipe(w, h);
        rc::MotionTemplates mt(pipe, 30, 8., 0.5, 2.5, 3, 2);
        std::vector<unsigned char> f((size_t)w * h), pic((size_t)w * h * 3);
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) f[(size_t)y * w + x] = x >= 5 + t && x < 5 + t + 9 ? 200 : 50;
            rc::Mat gray(h, w, 1, 1, f.data()), picture(h, w, 3, 1, pic.data());
            mt.push(gray, RC_MOTION_AUTO_TIME, &picture);
            std::vector<rc_motion_cell> cells;
            long long sil = 0;
            const rc_motion_cell r = mt.read(&cells, &sil);
            if ((int)cells.size() != 6 || mt.info().pushes != t + 1) { std::printf("bad result shape\n"); return 1; }
            long long lit = 0, used = 0;
            for (size_t i = 0; i < pic.size(); i += 3) lit += pic[i] != 0;
            for (const rc_motion_cell& c : cells) used += c.n_used;
            if (used != r.n_used) { std::printf("the cells use %lld pixels, the frame %d\n", used, r.n_used); return 1; }
            std::printf("push %d %.17g %lld %lld %d %d %d %lld %lld\n", t + 1, r.angle, r.S, r.W, r.n_masked, r.n_used, r.peak_bin, sil, lit);
        }
        rc::Mat img(h, w, 3, 1, pic.data());
        mt.draw(img);
        // a refused open throws and leaves the session working
        bool threw = false;
        try { rc::MotionTemplates bad(pipe, 300); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) { std::printf("threshold 300 was accepted\n"); return 1; }
        std::printf("angle %.17g\n", mt.angle());
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_motion: ok\n");
    return 0;
}
