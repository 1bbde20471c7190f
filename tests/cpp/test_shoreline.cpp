// rc::Shoreline (include/rcflow_module.hpp) on a step picture of 64 x 48 pixels: sand (BGR 120, 170, 200) left of column c, water
// (170, 140, 90) from it on, so R - B + 255 is 335 and 175, with radius 0 Otsu's first largest score is at 175 with a
// separability of exactly 1, every line splits at sample c - 4, and the position follows from the two levels.  The numbers are
// computed here.
//   test_shoreline
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static void paint(std::vector<unsigned char>& img, int w, int h, int c) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            unsigned char* p = &img[3 * ((size_t)y * w + x)];
            if (x < c) { p[0] = 120; p[1] = 170; p[2] = 200; } else { p[0] = 170; p[1] = 140; p[2] = 90; }
        }
}

// the position of the split between sample k - 1 (335) and k (175) at threshold 175, in 1/256 sample
static int position(int k) {
    const int a = 335, b = 175, thr = 175, d = a - b, e = std::abs(2 * thr + 1 - 2 * a);
    return (k - 1) * 256 + (e * 256 + d) / (2 * d);
}

int main() {
    const int w = 64, h = 48, L = 5, n = 56, T = 4;
    try {
        rc::Pipeline pipe(w, h);
        rc_shoreline_params p;
        std::memset(&p, 0, sizeof(p));
        p.source = RC_SHORE_RMB; p.radius = 0; p.threshold = -1; p.window = T; p.permille = 500; p.min_sep = 0.5; p.max_jump = 16.0;   // the lines are 9 px apart
        p.metres_per_pixel = 0.5;
        std::vector<rc_transect_line> lines;
        for (int i = 0; i < L; i++) lines.push_back(rc_transect_line{4.f, 5.f + 9.f * i, 59.f, 5.f + 9.f * i, n});
        rc::Shoreline sh(pipe, lines, p);
        std::vector<unsigned char> img((size_t)w * h * 3), mk((size_t)w * h);
        std::vector<unsigned short> pl((size_t)w * h);
        rc::Mat image(h, w, 3, 1, img.data()), mask(h, w, 1, 1, mk.data()), plane(h, w, 1, 2, pl.data());
        const int cols[2] = {30, 40};
        for (int t = 0; t < 2; t++) {
            const int c = cols[t], k = c - 4, pos = position(k);
            paint(img, w, h, c);
            sh.push(image, nullptr, &mask, &plane);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++)
                    if (mk[(size_t)y * w + x] != (x >= c ? 255 : 0) || pl[(size_t)y * w + x] != (x >= c ? 175 : 335))
                        FAIL("push %d, pixel (%d, %d): mask %d, plane %d", t, x, y, mk[(size_t)y * w + x], pl[(size_t)y * w + x]);
            const std::vector<long long> s = sh.read();
            if (s[0] != 175 || s[1] != (long long)w * h || s[2] != (1ll << 32) || s[3] != L || s[4] || s[5] || s[6] || s[7] != t + 1)
                FAIL("push %d, summary %lld %lld %lld %lld %lld %lld %lld %lld", t, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
            const std::vector<rc_shoreline> r = sh.records();
            const long long num = 16ll * (16 * 59 - 16 * 4) * pos + 128ll * (n - 1), den = 256ll * (n - 1);
            const int wx = 16 * 16 * 4 + (int)(num / den);
            const int p0 = position(cols[0] - 4);
            for (int i = 0; i < L; i++) {
                const int wy = 256 * (5 + 9 * i);
                if (r[i].flags != 0 || r[i].k != k || r[i].pos != pos || r[i].agree != n || r[i].wx != wx || r[i].wy != wy)
                    FAIL("push %d, line %d: flags %d, k %d, pos %d, agree %d, point (%d, %d), wanted pos %d, (%d, %d)", t, i, r[i].flags, r[i].k,
                         r[i].pos, r[i].agree, r[i].wx, r[i].wy, pos, wx, wy);
                if (r[i].x != (float)(wx / 256.0) || r[i].y != (float)(wy / 256.0) || r[i].dist_m != (float)((pos / 256.0) * 0.5))
                    FAIL("push %d, line %d: x %.9g, y %.9g, dist_m %.9g", t, i, r[i].x, r[i].y, r[i].dist_m);
                if (r[i].nv != t + 1 || r[i].pos_min != p0 || r[i].pos_max != pos || r[i].pos_q != p0 ||
                    r[i].pos_mean != (float)((double)(t ? p0 + pos : p0) / (t + 1)) || r[i].excursion_m != (float)(((pos - p0) / 256.0) * 0.5))
                    FAIL("push %d, line %d: nv %d, %d..%d, q %d, mean %.9g, excursion %.9g", t, i, r[i].nv, r[i].pos_min, r[i].pos_max, r[i].pos_q,
                         r[i].pos_mean, r[i].excursion_m);
            }
        }
        const std::vector<int> ring = sh.ring();
        for (int i = 0; i < L; i++)
            if (ring[(size_t)i * T] != position(26) || ring[(size_t)i * T + 1] != position(36) || ring[(size_t)i * T + 2] != -1 || ring[(size_t)i * T + 3] != -1)
                FAIL("ring of line %d: %d %d %d %d", i, ring[(size_t)i * T], ring[(size_t)i * T + 1], ring[(size_t)i * T + 2], ring[(size_t)i * T + 3]);
        // a region of interest with water alone: one bin, no threshold, every line EMPTY, the mask 0
        std::vector<unsigned char> rv((size_t)w * h, 0);
        for (int y = 0; y < h; y++)
            for (int x = 50; x < w; x++) rv[(size_t)y * w + x] = 1;
        rc::Mat roi(h, w, 1, 1, rv.data());
        sh.push(image, &roi, &mask);
        std::vector<long long> s = sh.read();
        const std::vector<rc_shoreline> r = sh.records();
        if (s[0] != -1 || s[1] != (long long)(w - 50) * h || s[2] != 0 || s[3] != 0 || s[7] != 3) FAIL("one bin: summary %lld %lld %lld %lld", s[0], s[1], s[2], s[3]);
        for (int i = 0; i < L; i++)
            if (r[i].flags != RC_SHORE_EMPTY || r[i].pos != -1 || r[i].nv != 2) FAIL("one bin: line %d has flags %d, pos %d, nv %d", i, r[i].flags, r[i].pos, r[i].nv);
        for (size_t i = 0; i < mk.size(); i++)
            if (mk[i]) FAIL("one bin: the mask is not 0");
        // set acts from the next push: a fixed threshold between the levels, a separability bar nothing reaches
        sh.set(250, 1.0, 16.0);
        sh.push(image);
        s = sh.read();
        if (s[0] != 250 || s[2] != (1ll << 32) || s[3] != L) FAIL("after set: %lld %lld %lld", s[0], s[2], s[3]);
        sh.reset();
        if (sh.info().pushes != 0 || sh.info().prm.threshold != 250 || sh.read()[7] != 0 || sh.ring()[0] != -1) FAIL("reset");
        // wrong shapes are refused before anything is copied; a refused open throws and leaves the session working
        bool threw = false;
        rc::Mat small(h - 1, w, 1, 1, mk.data());
        try { sh.push(image, nullptr, &small); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) FAIL("a mask of another size was accepted");
        threw = false;
        p.radius = 8;
        try { rc::Shoreline bad(pipe, lines, p); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw || sh.info().w != w || sh.info().lines != L) FAIL("radius 8 was accepted");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_shoreline: ok\n");
    return 0;
}
