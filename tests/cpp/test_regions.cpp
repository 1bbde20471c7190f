// rc::Regions (include/rcflow_module.hpp) on seeded masks: prints, per push, the summary, every record's integer part and
// checksums of the label image, the opened mask and the drawn frame for tests/test_gpu_regions.py to hold against the numpy
// statement on the same masks.
//   test_regions W H PUSHES
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rcflow_module.hpp"

// the program's masks: blobs of a drifting integer texture
static unsigned char pixel(int x, int y, int t) {
    const int u = x + 3 * t + 1000, v = y + t + 1000;
    return (unsigned char)((((u / 5) * (v / 7) + (u / 11) + t) % 5) < 2 ? 255 : 0);
}

template <class T>
static unsigned long long fnv(const std::vector<T>& a) {
    unsigned long long sum = 1469598103934665603ull;
    const unsigned char* p = (const unsigned char*)a.data();
    for (size_t i = 0; i < a.size() * sizeof(T); i++) { sum ^= p[i]; sum *= 1099511628211ull; }
    return sum;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: test_regions W H PUSHES\n"); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[3]);
    try {
        rc::Pipeline pipe(w, h);
        rc::Regions rg(pipe, 8, 4, 64);
        std::vector<unsigned char> mask((size_t)w * h), img((size_t)w * h * 3);
        std::vector<int32_t> labels((size_t)w * h);
        for (int t = 0; t < n; t++) {
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) mask[(size_t)y * w + x] = pixel(x, y, t);
            for (size_t i = 0; i < img.size(); i++) img[i] = (unsigned char)(i * 7 + t);
            rc::Mat m(h, w, 1, 1, mask.data()), l(h, w, 1, 4, labels.data()), out(h, w, 3, 1, img.data());
            rg.push(m, false, &l, &m);                                   // the opened mask in place
            long long s[8];
            const std::vector<rc_region> r = rg.regions(s);
            rg.draw(out, 0x20c0ff, 2, 3, 0.);
            std::printf("push %d %016llx %016llx %016llx |", t, fnv(labels), fnv(mask), fnv(img));
            for (int i = 0; i < 8; i++) std::printf(" %lld", s[i]);
            for (const rc_region& q : r)
                std::printf(" | %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %lld", q.label, q.area, q.x0, q.y0, q.x1, q.y1, q.first_x, q.first_y,
                            q.edges, (long long)q.sx, (long long)q.sy, (long long)q.sxx, (long long)q.syy, (long long)q.sxy);
            std::printf("\n");
        }
        const rc_regions_info i = rg.info();
        if (i.pushes != n || i.launches_per_push != RC_REGIONS_LAUNCHES || i.min_area != 4) { std::printf("info: %lld pushes\n", i.pushes); return 1; }
        bool threw = false;
        try { rg.setMinArea(0); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw || rg.info().min_area != 4) { std::printf("min_area 0 was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_regions: ok\n");
    return 0;
}
