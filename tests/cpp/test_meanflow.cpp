// rc::MeanFlow (include/rcflow_module.hpp) on the scene the product is named for, 20 x 12 pixels: waves v = 0.5 + 3 sin(2 pi t / 4 +
// 0.3 x), u = 0.7 cos(2 pi t / 4 + 0.2 y), a jet of -2.5 pixels in v on columns 8..11, and a noise of about 0.2 from a generator
// kept here.  20 fields go into a window of 8; with the direction (0, -1), K = 0.5, steady_min 600 and speed_min 0.5 the mask is
// the jet.  The sums, the mask, the mean, the steadiness and the summary are computed here, in integers and doubles as
// include/rcflow.h states them.
//   test_meanflow
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static const int W = 20, H = 12, T = 8, PUSHES = 20, J0 = 8, J1 = 12;

static unsigned lcg_state = 12345u;
static float noise() {                                        // four uniforms: sigma = 0.35 * sqrt(4 / 12) = 0.2
    float s = 0.f;
    for (int k = 0; k < 4; k++) {
        lcg_state = lcg_state * 1664525u + 1013904223u;
        s += (float)(lcg_state >> 8) / 16777216.f - 0.5f;
    }
    return 0.35f * s;
}

static long long isqrt(long long v) {
    long long r = (long long)std::sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

int main() {
    try {
        rc::Pipeline pipe(W, H);
        rc_meanflow_params p;
        std::memset(&p, 0, sizeof(p));
        p.window = T; p.grid_x = 4; p.grid_y = 3; p.min_fill = T; p.steady_min = 600; p.flags = RC_MEANFLOW_DIR_FIXED;
        p.speed_min = 0.5; p.min_cos2 = 0.5; p.dir_x = 0.; p.dir_y = -1.;
        rc::MeanFlow mf(pipe, p);
        const size_t N = (size_t)W * H;
        std::vector<std::vector<float>> fields;
        std::vector<float> mean(2 * N), sd(2 * N);
        std::vector<unsigned short> steady(N);
        std::vector<unsigned char> mask(N), pic(3 * N);
        rc::Mat mmean(H, W, 2, 4, mean.data()), msd(H, W, 2, 4, sd.data()), msteady(H, W, 1, 2, steady.data()), mmask(H, W, 1, 1, mask.data());
        rc::Mat mpic(H, W, 3, 1, pic.data());
        rc::MeanFlow::Pictures all;
        all.mean = &mmean; all.steady = &msteady; all.stddev = &msd; all.mask = &mmask; all.picture = &mpic;
        const double pi = 3.14159265358979323846;
        for (int t = 0; t < PUSHES; t++) {
            std::vector<float> f(2 * N);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const double v = 0.5 + 3.0 * std::sin(2 * pi * t / 4 + 0.3 * x) - (x >= J0 && x < J1 ? 2.5 : 0.);
                    const double u = 0.7 * std::cos(2 * pi * t / 4 + 0.2 * y);
                    f[2 * ((size_t)y * W + x)] = (float)u + noise();
                    f[2 * ((size_t)y * W + x) + 1] = (float)v + noise();
                }
            fields.push_back(f);
            rc::Mat mflow(H, W, 2, 4, fields.back().data());
            mf.push(mflow, all);
            if (t < T - 1)
                for (size_t i = 0; i < N; i++)
                    if (mask[i] || steady[i] || mean[2 * i] != 0.f || pic[3 * i] || pic[3 * i + 1] || pic[3 * i + 2]) FAIL("push %d: pixel %zu is filled", t + 1, i);
        }
        // the statement, from the last T fields
        unsigned char lut[768];
        rcflow_jet_lut(lut);
        long long filled = 0, in_mask = 0, Gx = 0, Gy = 0, SM = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                long long n = 0, Su = 0, Sv = 0, Sm = 0;
                for (int t = PUSHES - T; t < PUSHES; t++) {
                    const float fu = fields[t][2 * i], fv = fields[t][2 * i + 1];
                    if (!(std::fabs(fu) < 500.f && std::fabs(fv) < 500.f)) continue;
                    const long long u = (long long)std::rint(fu * 64.0f), v = (long long)std::rint(fv * 64.0f);
                    n++; Su += u; Sv += v; Sm += isqrt(u * u + v * v);
                }
                if (n != T) FAIL("pixel (%d, %d) holds %lld samples", x, y, n);
                const long long R = isqrt(Su * Su + Sv * Sv);
                const long long st = Sm > 0 ? (R * 1000 / Sm > 1000 ? 1000 : R * 1000 / Sm) : 0;
                const double dot = (double)Su * p.dir_x + (double)Sv * p.dir_y, cc = (double)Su * (double)Su + (double)Sv * (double)Sv;
                const bool in = st >= p.steady_min && R >= (long long)std::ceil(p.speed_min * 64.0) * n && dot > 0. && dot * dot >= p.min_cos2 * (cc * 1.0);
                if (in != (x >= J0 && x < J1)) FAIL("the statement does not name the jet at (%d, %d): steadiness %lld", x, y, st);
                if (mask[i] != (in ? 255 : 0)) FAIL("mask (%d, %d): %d", x, y, mask[i]);
                if (steady[i] != st) FAIL("steadiness (%d, %d): %d, wanted %lld", x, y, steady[i], st);
                const float mx = (float)(((double)Su / 64.0) / (double)n), my = (float)(((double)Sv / 64.0) / (double)n);
                if (mean[2 * i] != mx || mean[2 * i + 1] != my) FAIL("mean (%d, %d): %.9g %.9g, wanted %.9g %.9g", x, y, mean[2 * i], mean[2 * i + 1], mx, my);
                if (std::memcmp(&pic[3 * i], lut + 3 * (st * 255 / 1000), 3)) FAIL("picture (%d, %d)", x, y);
                if (!(sd[2 * i] >= sd[2 * i + 1] && sd[2 * i + 1] >= 0.f && sd[2 * i] > 0.05f)) FAIL("spread (%d, %d): %.9g %.9g", x, y, sd[2 * i], sd[2 * i + 1]);
                filled++; in_mask += in; Gx += Su; Gy += Sv; SM += Sm;
            }
        const std::vector<long long> s = mf.read();
        if (s[0] != filled || s[1] != in_mask || in_mask != (long long)(J1 - J0) * H || s[2] != 0 || s[3] != Gx || s[4] != Gy || s[5] != SM || s[6] != T ||
            s[7] != PUSHES)
            FAIL("summary %lld %lld %lld %lld %lld %lld %lld %lld", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
        const std::vector<rc_meanflow_cell> c = mf.cells();
        const std::vector<long long> sums = mf.sums();
        long long cf = 0, cm = 0;
        for (size_t k = 0; k < c.size(); k++) {
            if (c[k].flags || c[k].filled != sums[RC_MEANFLOW_SUMS * k] || c[k].mask != sums[RC_MEANFLOW_SUMS * k + 5]) FAIL("cell %zu", k);
            const float wx = (float)(((double)sums[RC_MEANFLOW_SUMS * k + 2] / 64.0) / (double)sums[RC_MEANFLOW_SUMS * k + 1]);
            if (c[k].mean_x != wx) FAIL("cell %zu: mean_x %.9g, wanted %.9g", k, c[k].mean_x, wx);
            cf += c[k].filled; cm += c[k].mask;
        }
        if (c.size() != 12 || cf != filled || cm != in_mask) FAIL("cells: %zu, %lld filled, %lld in the mask", c.size(), cf, cm);
        // set acts from the next push: a steadiness nothing in this scene reaches
        mf.set(1000, 0.5, 0.5, 0., -1., T);
        rc::Mat again(H, W, 2, 4, fields.back().data());
        mf.push(again);
        if (mf.read()[1] != 0 || mf.read()[7] != PUSHES + 1) FAIL("after set: %lld mask pixels", mf.read()[1]);
        mf.reset();
        if (mf.info().pushes != 0 || mf.info().prm.steady_min != 1000 || mf.read()[7] != 0 || mf.info().held != 0) FAIL("reset");
        // wrong shapes are refused before anything is copied; a refused open throws and leaves the session working
        bool threw = false;
        rc::Mat small(H - 1, W, 1, 1, mask.data());
        rc::MeanFlow::Pictures bad;
        bad.mask = &small;
        try { mf.push(again, bad); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) FAIL("a mask of another size was accepted");
        threw = false;
        try { mf.push(mmask); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) FAIL("a grey picture was accepted as a field");
        threw = false;
        p.flags = RC_MEANFLOW_DIR_FIXED | RC_MEANFLOW_DIR_OPPOSED;
        try { rc::MeanFlow two(pipe, p); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw || mf.info().w != W || mf.info().prm.window != T) FAIL("both directions were accepted");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_meanflow: ok\n");
    return 0;
}
