// plan_check.cpp -- the Farneback plan arithmetic (ripcurrents_amd/csrc/rc_plan.cpp) swept over everything
// rc_plan_params_valid admits, built from that file alone under AddressSanitizer + UBSan (tests/test_plan_host.py).
// Host code only; exits 0 and prints "plan_check: ok" when every invariant holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ripcurrents_amd/csrc/rc_plan.h"

static int g_checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        g_checks++;                                       \
        if (!(cond)) {                                    \
            fprintf(stderr, "plan_check: %s: ", #cond);   \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

// taps finite and summing to 1 within 1e-6
static void check_unit_taps(const float* k, int n, const char* what, int a, double b) {
    double sum = 0;
    for (int i = 0; i < n; i++) {
        CHECK(std::isfinite(k[i]), "%s(%d, %g) tap %d", what, a, b, i);
        sum += k[i];
    }
    CHECK(fabs(sum - 1.) <= 1e-6, "%s(%d, %g) sums to %.9g", what, a, b, sum);
}

int main() {
    // polynomial expansion: poly_n 1..32 at sigma 0 and 1.2, both exact_taps values
    for (int n = 1; n <= RC_MAX_POLY_N; n++)
        for (double sigma : {0., 1.2})
            for (int exact_taps = 0; exact_taps < 2; exact_taps++) {
                rc_farneback_params p = {0.5, 2, 3, 2, n, sigma, 0};
                CHECK(rc_plan_params_valid(&p), "poly_n %d sigma %g refused", n, sigma);
                RcPolyK pk;
                CHECK(rc_plan_prepare_poly(n, sigma, exact_taps, pk) == RC_OK, "poly(%d, %g, %d) not positive definite", n, sigma, exact_taps);
                CHECK(pk.n == n && pk.n_eff >= 1 && pk.n_eff <= n, "poly(%d, %g, %d): n_eff %d", n, sigma, exact_taps, pk.n_eff);
                CHECK(!exact_taps || pk.n_eff == n, "poly(%d, %g) exact_taps: n_eff %d", n, sigma, pk.n_eff);
                std::vector<float> full(2 * pk.n_eff + 1);
                for (int k = -pk.n_eff; k <= pk.n_eff; k++) {
                    full[k + pk.n_eff] = pk.g[abs(k)];
                    CHECK(std::isfinite(pk.xg[abs(k)]) && std::isfinite(pk.xxg[abs(k)]), "poly(%d, %g) tap %d", n, sigma, k);
                }
                check_unit_taps(full.data(), (int)full.size(), "poly", n, sigma);   // the dropped taps weigh less than 1e-8
                for (int k = pk.n_eff + 1; k <= RC_MAX_POLY_N; k++)
                    CHECK(pk.g[k] == 0 && pk.xg[k] == 0 && pk.xxg[k] == 0, "poly(%d, %g) tap %d beyond n_eff is not zero", n, sigma, k);
                CHECK(std::isfinite(pk.ig11) && std::isfinite(pk.ig03) && std::isfinite(pk.ig33) && std::isfinite(pk.ig55) && std::isfinite(pk.kdc),
                      "poly(%d, %g) scalars", n, sigma);
            }
    // window: winsize 1..49, box and Gaussian
    for (int winsize = 1; winsize <= 49; winsize++)
        for (int flags : {0, RC_FARNEBACK_GAUSSIAN}) {
            rc_farneback_params p = {0.5, 2, winsize, 2, 5, 1.1, flags};
            CHECK(rc_plan_params_valid(&p), "winsize %d refused", winsize);
            RcWindow win;
            rc_plan_window(winsize, flags, win);
            CHECK(win.m == winsize / 2 && win.m <= RC_MAX_WIN_M && win.gaussian == (flags != 0), "window(%d, %d): m %d", winsize, flags, win.m);
            CHECK(win.box_scale > 0 && std::isfinite(win.box_eps), "window(%d) box", winsize);
            std::vector<float> full(2 * win.m + 1);
            for (int k = -win.m; k <= win.m; k++) full[k + win.m] = win.k[abs(k)];
            check_unit_taps(full.data(), (int)full.size(), "window", winsize, (double)flags);
        }
    // geometry and pyramid tile: scales 0..11 at pyr_scale 0.5 and 0.8
    static const int sizes[][2] = {{33, 32}, {40, 36}, {257, 130}, {640, 480}, {1920, 1080}, {3840, 2160}};
    for (auto& sz : sizes)
        for (double pyr_scale : {0.5, 0.8}) {
            const int w = sz[0], h = sz[1];
            const int L = rc_plan_crop_levels(w, h, pyr_scale, RC_MAX_LEVELS - 1);
            CHECK(L >= 0 && L < RC_MAX_LEVELS, "crop_levels(%d, %d, %g) = %d", w, h, pyr_scale, L);
            for (int k = 0; k < RC_MAX_LEVELS; k++) {
                RcLevel lv;
                rc_plan_level_geom(w, h, pyr_scale, k, lv);
                CHECK(lv.ksize >= 3 && (lv.ksize & 1) && lv.w >= 0 && lv.h >= 0, "level_geom(%d, %d, %g, %d): ksize %d", w, h, pyr_scale, k, lv.ksize);
                // the driver plans scales 0..L only; the stage entry point takes any k
                if (k <= L)
                    CHECK(lv.w >= 32 && lv.h >= 32 && lv.ksize <= 1023, "level_geom(%d, %d, %g, %d): %d x %d ksize %d", w, h, pyr_scale, k, lv.w, lv.h, lv.ksize);
                lv.pyr_tw = lv.pyr_th = 0;
                rc_plan_pick_pyr_tile(lv, w, h);
                CHECK(lv.pyr_tw >= 1 && lv.pyr_th >= 1, "pick_pyr_tile(%d, %d, %g, %d): no tile", w, h, pyr_scale, k);
                CHECK(lv.pyr_lds <= 40 * 1024 || lv.pyr_tw == 1, "pick_pyr_tile(%d, %d, %g, %d): %zu LDS bytes", w, h, pyr_scale, k, lv.pyr_lds);
                double s = rc_plan_scale_pow(pyr_scale, k);
                CHECK(lv.sigma == (1. / s - 1) * 0.5, "scale_pow(%g, %d)", pyr_scale, k);
            }
        }
    // pyramid blur: every odd ksize the driver admits, at the fixed taps of sigma 0 and at a level's own sigma
    for (int ksize = 1; ksize <= 1023; ksize += 2)
        for (double sigma : {0., ksize / 5.}) {
            std::vector<float> taps(ksize);
            rc_plan_gaussian_kernel(ksize, sigma, taps.data());
            check_unit_taps(taps.data(), ksize, "gaussian_kernel", ksize, sigma);
        }
    printf("plan_check: ok (%d checks)\n", g_checks);
    return 0;
}
