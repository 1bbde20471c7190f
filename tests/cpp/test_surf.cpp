// rc::Surf (include/rcflow_module.hpp) on a two-level picture of 64 x 48 pixels with one gap: frame A has a band of grey 240 in
// columns 20..39 on water of grey 60, except in rows 20..27, where the band has a hole; frame B is water alone.  A and B alternate
// into a window of 4, so from push 5 on a band pixel has broken in 2 of the 4 frames held, its window mean is 150 and twice its
// standard deviation 180; six lines cross the band, the one at y = 20 runs through the hole and is the one channel.  The numbers
// are computed here.
//   test_surf
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static const int W = 64, H = 48, X0 = 20, X1 = 40, G0 = 20, G1 = 28;
static bool in_band(int x, int y) { return x >= X0 && x < X1 && !(y >= G0 && y < G1); }

// the point at pos (1/256 sample) of a line of n samples from x = 4 to x = 59, in 1/256 pixel
static int point(long long pos, int n) { return 16 * 16 * 4 + (int)((16ll * (16 * 59 - 16 * 4) * pos + 128ll * (n - 1)) / (256ll * (n - 1))); }

int main() {
    const int L = 6, n = 56, T = 4;
    try {
        rc::Pipeline pipe(W, H);
        rc_surf_params p;
        std::memset(&p, 0, sizeof(p));
        p.window = T; p.bright = 200; p.delta = 50; p.q_min = 500; p.min_run = 2; p.span = 6; p.ratio = 500; p.min_load = 0; p.min_lines = 1;
        p.vis_permille = 1000; p.metres_per_pixel = 0.5;
        std::vector<rc_transect_line> lines;
        for (int i = 0; i < L; i++) lines.push_back(rc_transect_line{4.f, 4.f + 8.f * i, 59.f, 4.f + 8.f * i, n});
        rc::Surf sf(pipe, lines, p);
        std::vector<unsigned char> A((size_t)W * H), B((size_t)W * H, 60), now(A.size()), surf(A.size()), mean(A.size()), sd(A.size()), pic(3 * A.size());
        std::vector<unsigned short> q(A.size());
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) A[(size_t)y * W + x] = in_band(x, y) ? 240 : 60;
        rc::Mat fa(H, W, 1, 1, A.data()), fb(H, W, 1, 1, B.data());
        rc::Mat mnow(H, W, 1, 1, now.data()), msurf(H, W, 1, 1, surf.data()), mmean(H, W, 1, 1, mean.data()), msd(H, W, 1, 1, sd.data());
        rc::Mat mq(H, W, 1, 2, q.data()), mpic(H, W, 3, 1, pic.data());
        rc::Surf::Pictures all;
        all.now = &mnow; all.surf = &msurf; all.q = &mq; all.mean = &mmean; all.sd = &msd; all.picture = &mpic;
        unsigned char lut[768];
        rcflow_jet_lut(lut);
        // push 1: nothing breaks against a mean of one frame; push 3: 3 * 240 >= 540 + 3 * 50, the band breaks
        for (int t = 0; t < 6; t++) {
            sf.push(t % 2 ? fb : fa, all);
            const int breaks = t == 2 || t == 4, Q = t < 2 ? 0 : t < 4 ? 1 : 2, held = t + 1 < T ? t + 1 : T;
            const int s1 = 240 * ((t + 2) / 2 > 2 ? 2 : (t + 2) / 2) + 60 * ((t + 1) / 2 > 2 ? 2 : (t + 1) / 2);      // of a band pixel
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const size_t i = (size_t)y * W + x;
                    const int b = in_band(x, y), wq = b ? Q : 0, idx = wq * 255000 / (1000 * held) > 255 ? 255 : wq * 255000 / (1000 * held);
                    const int wmean = b ? (2 * s1 + held) / (2 * held) : 60;
                    if (now[i] != (b && breaks ? 255 : 0) || q[i] != wq || surf[i] != (wq * 1000 >= 500 * held && b ? 255 : 0) || mean[i] != wmean ||
                        std::memcmp(&pic[3 * i], lut + 3 * idx, 3))
                        FAIL("push %d, pixel (%d, %d): now %d, q %d, surf %d, mean %d (wanted %d)", t + 1, x, y, now[i], q[i], surf[i], mean[i], wmean);
                    if (t == 5 && sd[i] != (b ? 180 : 0)) FAIL("push 6, pixel (%d, %d): sd %d", x, y, sd[i]);
                }
        }
        const long long band_px = (long long)(X1 - X0) * (H - (G1 - G0));
        const std::vector<long long> s = sf.read();
        if (s[0] != T || s[1] != 0 || s[2] != band_px || s[3] != 2 * band_px || s[4] != L - 1 || s[5] != 1 || s[6] != 1 || s[7] != 6)
            FAIL("summary %lld %lld %lld %lld %lld %lld %lld %lld", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
        const std::vector<rc_surf_line> r = sf.records();
        const int k0 = X0 - 4, k1 = X1 - 1 - 4, load = 2 * (X1 - X0);
        for (int i = 0; i < L; i++) {
            const int y = 4 + 8 * i, gap = y >= G0 && y < G1;
            if (r[i].ref != load || r[i].peak != (gap ? 0 : 2) || r[i].kpeak != (gap ? 0 : k0)) FAIL("line %d: ref %d, peak %d at %d", i, r[i].ref, r[i].peak, r[i].kpeak);
            if (gap) {
                if (r[i].flags != (RC_SURF_NOBAND | RC_SURF_CHANNEL | RC_SURF_IN_CHANNEL) || r[i].k0 != -1 || r[i].k1 != -1 || r[i].load != 0 || r[i].share != 0 ||
                    r[i].ix || r[i].iy || r[i].ox || r[i].oy || r[i].width_m != 0.f)
                    FAIL("the gap's line %d: flags %d, k %d..%d, load %d, share %d", i, r[i].flags, r[i].k0, r[i].k1, r[i].load, r[i].share);
                continue;
            }
            if (r[i].flags != 0 || r[i].k0 != k0 || r[i].k1 != k1 || r[i].load != load || r[i].share != 1000)
                FAIL("line %d: flags %d, k %d..%d, load %d, share %d", i, r[i].flags, r[i].k0, r[i].k1, r[i].load, r[i].share);
            if (r[i].ix != point(256ll * k0, n) || r[i].ix != 256 * X0 || r[i].ox != point(256ll * k1, n) || r[i].ox != 256 * (X1 - 1) || r[i].iy != 256 * y ||
                r[i].oy != 256 * y || r[i].width_m != (float)((double)(k1 - k0 + 1) * 0.5))
                FAIL("line %d: inner (%d, %d), outer (%d, %d), width %.9g", i, r[i].ix, r[i].iy, r[i].ox, r[i].oy, r[i].width_m);
        }
        const std::vector<rc_surf_channel> c = sf.channels();
        const long long pos = (128ll * (k0 + k1) * 2) / 2;                        // both flanks have the band
        if (c.size() != 1 || c[0].first != 2 || c[0].count != 1 || c[0].centre != 2 || c[0].share != 0 || c[0].cx != point(pos, n) || c[0].cy != 256 * 20 ||
            c[0].width_m != (float)((std::sqrt((double)(16 * 16) * (16 * 16)) / 16.) * 0.5))
            FAIL("channel: %zu, first %d, count %d, centre %d, share %d, (%d, %d), width %.9g", c.size(), c.empty() ? -1 : c[0].first, c.empty() ? -1 : c[0].count,
                 c.empty() ? -1 : c[0].centre, c.empty() ? -1 : c[0].share, c.empty() ? -1 : c[0].cx, c.empty() ? -1 : c[0].cy, c.empty() ? -1. : c[0].width_m);
        // set acts from the next push: a share of time nothing reaches
        sf.set(200, 50, 1000, 500, 0, 1000);
        sf.push(fa);
        std::vector<long long> s2 = sf.read();
        if (s2[1] != band_px || s2[2] != 0 || s2[4] != 0 || s2[7] != 7) FAIL("after set: %lld %lld %lld %lld", s2[1], s2[2], s2[4], s2[7]);
        sf.reset();
        if (sf.info().pushes != 0 || sf.info().prm.q_min != 1000 || sf.read()[7] != 0 || sf.info().held != 0) FAIL("reset");
        // wrong shapes are refused before anything is copied; a refused open throws and leaves the session working
        bool threw = false;
        rc::Mat small(H - 1, W, 1, 1, now.data());
        rc::Surf::Pictures bad;
        bad.surf = &small;
        try { sf.push(fa, bad); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) FAIL("a mask of another size was accepted");
        threw = false;
        try { sf.push(mpic); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) FAIL("a colour frame was accepted");
        threw = false;
        p.span = 33;
        try { rc::Surf again(pipe, lines, p); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw || sf.info().w != W || sf.info().lines != L) FAIL("span 33 was accepted");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_surf: ok\n");
    return 0;
}
