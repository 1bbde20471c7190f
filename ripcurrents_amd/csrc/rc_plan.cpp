// rc_plan.cpp -- the Farneback plan arithmetic (see rc_plan.h).  Built with -ffp-contract=off: the constants are
// compared with upstream's bit for bit, so no expression and no order of operations here may change.

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "rc_plan.h"

static inline int cv_round(double v) { return (int)nearbyint(v); }   // round half to even

int rc_plan_crop_levels(int w, int h, double pyr_scale, int levels) {
    const int min_size = 32;   // optflow.cpp calc()
    int k;
    double scale = 1;
    for (k = 0; k < levels; k++) {
        scale *= pyr_scale;
        if (w * scale < min_size || h * scale < min_size) break;
    }
    return k;
}

void rc_plan_level_geom(int w, int h, double pyr_scale, int k, RcLevel& L) {
    double scale = 1;
    for (int i = 0; i < k; i++) scale *= pyr_scale;
    L.sigma = (1. / scale - 1) * 0.5;
    int smooth_sz = cv_round(L.sigma * 5) | 1;
    L.ksize = smooth_sz > 3 ? smooth_sz : 3;
    L.w = cv_round(w * scale);
    L.h = cv_round(h * scale);
    L.scale_x = 1. / ((double)L.w / w);
    L.scale_y = 1. / ((double)L.h / h);
}

double rc_plan_scale_pow(double pyr_scale, int L) {
    double scale = 1;
    for (int i = 0; i < L; i++) scale *= pyr_scale;
    return scale;
}

// smooth.cpp getGaussianKernel(n, sigma, CV_32F)
void rc_plan_gaussian_kernel(int n, double sigma, float* cf) {
    static const float tab1[] = {1.f};
    static const float tab3[] = {0.25f, 0.5f, 0.25f};
    static const float tab5[] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    static const float tab7[] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    const float* fixed = nullptr;
    if (n % 2 == 1 && n <= 7 && sigma <= 0) fixed = n == 1 ? tab1 : n == 3 ? tab3 : n == 5 ? tab5 : tab7;
    double sx = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    double scale2x = -0.5 / (sx * sx), sum = 0;
    for (int i = 0; i < n; i++) {
        double x = i - (n - 1) * 0.5;
        double t = fixed ? (double)fixed[i] : exp(scale2x * x * x);
        cf[i] = (float)t;
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) cf[i] = (float)(cf[i] * sum);
}

// optflow.cpp FarnebackPrepareGaussian; the 6x6 moment matrix is inverted by Cholesky.
int rc_plan_prepare_poly(int n, double sigma, int exact_taps, RcPolyK& pk) {
    if (sigma < FLT_EPSILON) sigma = n * 0.3;
    std::vector<float> gb(2 * n + 1), xgb(2 * n + 1), xxgb(2 * n + 1);
    float *g = gb.data() + n, *xg = xgb.data() + n, *xxg = xxgb.data() + n;
    double s = 0.;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)(g[x] * s);
        xg[x] = (float)(x * g[x]);
        xxg[x] = (float)(x * x * g[x]);
    }
    double G[6][6] = {{0}};
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0][0] += g[y] * g[x];
            G[1][1] += g[y] * g[x] * x * x;
            G[3][3] += g[y] * g[x] * x * x * x * x;
            G[5][5] += g[y] * g[x] * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    // invG = G.inv(DECOMP_CHOLESKY): cv::invert -> hal::Cholesky64f on the identity (core/src/matrix_decomp.cpp
    // CholImpl<double>: 1/sqrt(pivot) on the diagonal, forward then backward substitution), restated
    // operation for operation so that the four scalars carry upstream's bits.
    double L[6][6], inv[6][6];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) { L[i][j] = G[i][j]; inv[i][j] = i == j ? 1. : 0.; }
    for (int i = 0; i < 6; i++) {
        double v;
        int j, k;
        for (j = 0; j < i; j++) {
            v = L[i][j];
            for (k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v * L[j][j];
        }
        v = L[i][i];
        for (k = 0; k < j; k++) { double t = L[i][k]; v -= t * t; }
        if (!(v >= DBL_EPSILON)) return RC_EINVAL;
        L[i][i] = 1. / sqrt(v);
    }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double v = inv[i][j];
            for (int k = 0; k < i; k++) v -= L[i][k] * inv[k][j];
            inv[i][j] = v * L[i][i];
        }
    for (int i = 5; i >= 0; i--)
        for (int j = 0; j < 6; j++) {
            double v = inv[i][j];
            for (int k = 5; k > i; k--) v -= L[k][i] * inv[k][j];
            inv[i][j] = v * L[i][i];
        }
    pk.ig11 = inv[1][1];
    pk.ig03 = inv[0][3];
    pk.ig33 = inv[3][3];
    pk.ig55 = inv[5][5];
    pk.n = n;
    // Taps whose combined weight cannot change any sum beyond 1e-9 of its kernel mass are
    // dropped (poly_n = 15 with sigma = 1.2 evaluates 15 of its 31 taps: n_eff = 7; "exact_taps"
    // keeps all of them).
    int n_thr = n;
    if (!exact_taps) {
        double m0 = 0, m1 = 0, m2 = 0;
        for (int k = 1; k <= n; k++) { m0 += g[k]; m1 += fabs(xg[k]); m2 += xxg[k]; }
        double t0 = 0, t1 = 0, t2 = 0;
        for (int k = n; k >= 1; k--) {
            t0 += g[k]; t1 += fabs(xg[k]); t2 += xxg[k];
            if (t0 > 1e-8 * (m0 + g[0]) || t1 > 1e-8 * m1 || t2 > 1e-8 * m2) break;
            n_thr = k - 1;
        }
        if (n_thr < 1) n_thr = 1;
    }
    static const int inst[] = {3, 5, 7, 8, 9, 12, 16, 24, 32};
    int R = 32;
    for (int v : inst)
        if (v >= n_thr) { R = v; break; }
    pk.n_eff = R < n ? R : n;
    memset(pk.g, 0, sizeof(pk.g));
    memset(pk.xg, 0, sizeof(pk.xg));
    memset(pk.xxg, 0, sizeof(pk.xxg));
    double sg = 0, s2 = 0;
    for (int k = 0; k <= pk.n_eff; k++) {
        pk.g[k] = g[k];
        pk.xg[k] = xg[k];
        pk.xxg[k] = xxg[k];
        sg += (k ? 2. : 1.) * g[k];
        s2 += (k ? 2. : 0.) * xxg[k];
    }
    pk.kdc = sg * sg * pk.ig03 + sg * s2 * pk.ig33;
    // the derived taps (rc_plan.h): ig03 g + ig33 xxg cancels in double here, once, instead of per pixel in the kernel
    memset(pk.qh, 0, sizeof(pk.qh));
    memset(pk.xga, 0, sizeof(pk.xga));
    memset(pk.xgb, 0, sizeof(pk.xgb));
    const double sa = pk.ig11 * 0.5, sb = (pk.ig55 * 0.25) / sa;
    for (int k = 0; k <= pk.n_eff; k++) {
        pk.qh[k] = (float)(0.5 * (pk.ig03 * (double)g[k] + pk.ig33 * (double)xxg[k]));
        pk.xga[k] = (float)((double)xg[k] * sa);
        pk.xgb[k] = (float)((double)xg[k] * sb);
    }
    pk.kdch = 0.5 * pk.kdc;
    return RC_OK;
}

void rc_plan_window(int winsize, int flags, RcWindow& win) {
    int m = winsize / 2;
    memset(&win, 0, sizeof(win));
    win.m = m;
    win.gaussian = (flags & RC_FARNEBACK_GAUSSIAN) ? 1 : 0;
    win.box_scale = 1. / ((double)winsize * winsize);
    win.box_eps = 1e-3 / (win.box_scale * win.box_scale);
    double sigma = m * 0.3, s = 1;
    win.k[0] = (float)s;
    for (int i = 1; i <= m; i++) {
        float t = (float)exp(-i * i / (2 * sigma * sigma));
        win.k[i] = t;
        s += t * 2;
    }
    s = 1. / s;
    for (int i = 0; i <= m; i++) win.k[i] = (float)(win.k[i] * s);
}

void rc_plan_pick_pyr_tile(RcLevel& L, int W0, int H0) {
    // tw <= 128 and th <= 128 (the coordinate tables are filled by threads 0..127 / 128..255)
    static const int tiles[][2] = {{64, 16}, {64, 8}, {64, 4}, {32, 8}, {16, 8}, {16, 4}, {8, 4}, {4, 4}, {2, 2}, {1, 1}};
    int r = L.ksize / 2;
    for (auto& t : tiles) {
        int tw = t[0], th = t[1];
        int rw = (int)ceil(tw * L.scale_x) + 2 * r + 4;
        int rh = (int)ceil(th * L.scale_y) + 2 * r + 4;
        if (rw > W0 + 2 * r + 2) rw = W0 + 2 * r + 2;
        if (rh > H0 + 2 * r + 2) rh = H0 + 2 * r + 2;
        int rwp = (rw + 15) & ~15;
        size_t lds = (size_t)rh * rwp + sizeof(float) * ((size_t)rh * 2 * tw + 3 * tw + 3 * th + L.ksize);
        if (lds <= 40 * 1024 || tw == 1) {
            L.pyr_tw = tw; L.pyr_th = th; L.pyr_reg_w = rwp; L.pyr_reg_h = rh; L.pyr_lds = lds;
            return;
        }
    }
}

int rc_plan_params_valid(const rc_farneback_params* p) {
    if (!p) return 0;
    if (!(p->pyr_scale > 0 && p->pyr_scale < 1)) return 0;
    if (p->levels < 0 || p->levels >= RC_MAX_LEVELS) return 0;
    if (p->winsize < 1 || p->winsize / 2 > 24) return 0;
    if (p->iterations < 0 || p->iterations > 1000) return 0;
    if (p->poly_n < 1 || p->poly_n > RC_MAX_POLY_N) return 0;
    if (!(p->poly_sigma >= 0)) return 0;
    if (p->flags & ~(RC_FARNEBACK_GAUSSIAN | RC_FARNEBACK_USE_INITIAL_FLOW)) return 0;
    return 1;
}
