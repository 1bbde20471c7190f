// rc::Tracks (include/rcflow_module.hpp) on seeded masks: prints, per push, the summary, every used slot's integer fields and
// checksums of the confirmed mask, the footprint and the drawn frame for tests/test_gpu_tracks.py to hold against the numpy
// statements on the same masks.
//   test_tracks W H PUSHES
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

// the program's masks: blobs of an integer texture that drifts one pixel per push and changes every fourth
static unsigned char pixel(int x, int y, int t) {
    const int u = x + t + 1000, v = y + 1000;
    return (unsigned char)((((u / 9) * (v / 7) + (u / 13) + t / 4) % 5) < 2 ? 255 : 0);
}

template <class T>
static unsigned long long fnv(const std::vector<T>& a) {
    unsigned long long sum = 1469598103934665603ull;
    const unsigned char* p = (const unsigned char*)a.data();
    for (size_t i = 0; i < a.size() * sizeof(T); i++) { sum ^= p[i]; sum *= 1099511628211ull; }
    return sum;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: test_tracks W H PUSHES\n"); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[3]);
    try {
        rc::Pipeline pipe(w, h);
        rc::Regions rg(pipe, 8, 4, 64);
        rc::Tracks tk(pipe, rg, 32, 2, 1, 2);
        std::vector<unsigned char> mask((size_t)w * h), conf((size_t)w * h), img((size_t)w * h * 3);
        std::vector<int32_t> foot;
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) mask[(size_t)y * w + x] = pixel(x, y, t);
            for (size_t i = 0; i < img.size(); i++) img[i] = (unsigned char)(i * 7 + t);
            rc::Mat m(h, w, 1, 1, mask.data()), c(h, w, 1, 1, conf.data()), out(h, w, 3, 1, img.data());
            tk.push(m, false, &c);
            long long s[8];
            const std::vector<rc_track> r = tk.tracks(s, &foot);
            tk.draw(out, 0x20c0ff, 2, 3);
            std::printf("push %d %016llx %016llx %016llx |", t, fnv(conf), fnv(foot), fnv(img));
            for (int i = 0; i < 8; i++) std::printf(" %lld", s[i]);
            for (const rc_track& q : r)
                std::printf(" | %lld %lld %lld %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", (long long)q.id, (long long)q.parent,
                            (long long)q.first_push, (long long)q.area_sum, q.slot, q.label, q.flags, q.age, q.hits, q.misses, q.area, q.x0, q.y0,
                            q.x1, q.y1, q.px, q.py, q.px0, q.py0, q.overlap);
            std::printf("\n");
        }
        const rc_tracks_info i = tk.info();
        if (i.pushes != n || i.launches_per_push != RC_TRACKS_LAUNCHES || i.prm.max_tracks != 32 || i.prm.max_regions != 64) {
            std::printf("info: %lld pushes\n", i.pushes);
            return 1;
        }
        tk.reset();
        long long s[8];
        if (!tk.tracks(s).empty() || s[7] != 0) { std::printf("reset left tracks\n"); return 1; }
        bool threw = false;
        try { rc::Tracks bad(pipe, rg, 0); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw || tk.info().prm.max_tracks != 32) { std::printf("max_tracks 0 was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_tracks: ok\n");
    return 0;
}
