// rc::Tracers (include/rcflow_module.hpp) on a seeded sequence of gray frames: five streaklines, a timeline and a cloud
// moved by the reference's PyrLK call and drawn into a frame.  Prints, per push, every vertex as hexadecimal floats and a
// checksum of the drawn frame for tests/test_gpu_tracers.py to hold against the ctypes session on the same frames.
//   test_tracers W H PUSHES
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

// the program's frames: a texture that drifts by (t, t / 2) pixels
static unsigned char pixel(int x, int y, int t) {
    const int u = x - t + 1000, v = y - t / 2 + 1000;               // never negative: % and / mean the same everywhere
    return (unsigned char)(128 + ((u * u + 3 * v * v + 5 * u * v) % 97) - 48 + ((u / 8 + v / 8) & 1) * 40);
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: test_tracers W H PUSHES\n"); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[3]);
    try {
        rc::Pipeline pipe(w, h);
        rc::Tracers tr(pipe, RC_TRACERS_LK, 8, 6);
        for (int i = 0; i < 5; i++) tr.addStreakline(rc::Pixel2{(float)(w / 6 * (i + 1)), (float)(h / 2 + 7 * i)});
        const int tl = tr.addTimeline(rc::Pixel2{(float)w / 4, (float)h / 4}, rc::Pixel2{(float)w * 3 / 4, (float)h / 3}, 7);
        const int cl = tr.addCloud({rc::Pixel2{w * 0.3f, h * 0.7f}, rc::Pixel2{w * 0.5f, h * 0.75f}, rc::Pixel2{w * 0.7f, h * 0.6f}});
        if (tl != 5 || cl != 6) { std::printf("ids %d %d\n", tl, cl); return 1; }
        std::vector<unsigned char> gray((size_t)w * h), img((size_t)w * h * 3);
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) gray[(size_t)y * w + x] = pixel(x, y, t);
            for (size_t i = 0; i < img.size(); i++) img[i] = (unsigned char)(i * 7 + t);
            rc::Mat g(h, w, 1, 1, gray.data()), out(h, w, 3, 1, img.data());
            const bool moved = tr.push(g, &out);
            if (moved != (t > 0)) { std::printf("push %d: primed wrongly\n", t); return 1; }
            unsigned long long sum = 1469598103934665603ull;           // FNV-1a of the frame
            for (unsigned char v : img) { sum ^= v; sum *= 1099511628211ull; }
            std::printf("push %d %016llx", t, sum);
            for (int l = 0; l < 7; l++) {
                const std::vector<rc::Pixel2> v = tr.vertices(l);
                std::printf(" | %d", (int)v.size());
                for (const rc::Pixel2& p : v) {
                    uint32_t a, b;
                    std::memcpy(&a, &p.x, 4); std::memcpy(&b, &p.y, 4);
                    std::printf(" %08x %08x", a, b);
                }
            }
            std::printf("\n");
        }
        const rc_tracers_info i = tr.info();
        if (i.lines != 7 || i.pushes != n - 1) { std::printf("info: %d lines, %lld pushes\n", i.lines, i.pushes); return 1; }
        // a refused add throws and changes nothing
        bool threw = false;
        try { tr.addCloud(std::vector<rc::Pixel2>(100, rc::Pixel2{1.f, 1.f})); } catch (const rc::Error& e) { threw = e.code == RC_ESIZE; }
        if (!threw || tr.info().lines != 7) { std::printf("a cloud beyond max_points was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_tracers: ok\n");
    return 0;
}
