// rc::Ftle (include/rcflow_module.hpp) on 67 x 45 fields made from integers (sixteenths: exact in float, so
// tests/test_gpu_ftle.py makes the same ones): window 4, backward, spacing 2, threshold 0.05, vis_max 0.25.  Prints, per push,
// the summary and the counts of mask and picture pixels for the test to hold against the numpy statement.
//   test_ftle PUSHES
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: test_ftle PUSHES\n"); return 2; }
    const int w = 67, h = 45, n = std::atoi(argv[1]);
    try {
        rc::Pipeline pipe(w, h);
        rc::Ftle ft(pipe, 4, RC_FTLE_BACKWARD, 1.f, 2, 0.05, 0.25);
        std::vector<float> f((size_t)w * h * 2), e((size_t)w * h);
        std::vector<unsigned char> m((size_t)w * h), pic((size_t)w * h * 3);
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    f[2 * ((size_t)y * w + x)] = (float)((x * 7 + y * 3 + t * 5) % 32 - 12) / 16.f;
                    f[2 * ((size_t)y * w + x) + 1] = (float)((x * 5 + y * 11 + t * 3) % 32 - 18) / 16.f;
                }
            rc::Mat flow(h, w, 2, 4, f.data()), ftle(h, w, 1, 4, e.data()), mask(h, w, 1, 1, m.data()), picture(h, w, 3, 1, pic.data());
            ft.push(flow, &ftle, &mask, &picture);
            const std::vector<long long> s = ft.read();
            const rc_ftle_info i = ft.info();
            if (i.pushes != t + 1 || i.held != (t + 1 < 4 ? t + 1 : 4) || s[0] != i.held) { std::printf("bad counts\n"); return 1; }
            long long lit = 0, set = 0, pos = 0;
            for (size_t k = 0; k < m.size(); k++) {
                set += m[k] != 0;
                lit += (pic[3 * k] | pic[3 * k + 1] | pic[3 * k + 2]) != 0;
                pos += e[k] >= 0.05f;
            }
            if (set > pos) { std::printf("%lld mask pixels, only %lld with ftle at the threshold\n", set, pos); return 1; }
            std::printf("push %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], set, lit);
        }
        // a push without outputs only stores the field; the summary stays the last computed one
        const std::vector<long long> before = ft.read();
        rc::Mat flow(h, w, 2, 4, f.data());
        ft.push(flow);
        if (ft.read() != before || ft.info().pushes != n + 1) { std::printf("a push without outputs changed the summary\n"); return 1; }
        // a refused open throws and leaves the session working
        bool threw = false;
        try { rc::Ftle bad(pipe, 0); } catch (const rc::Error& e2) { threw = e2.code == RC_EINVAL; }
        if (!threw || ft.info().pushes != n + 1) { std::printf("window 0 was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_ftle: ok\n");
    return 0;
}
