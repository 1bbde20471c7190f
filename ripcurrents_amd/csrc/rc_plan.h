// rc_plan.h -- the Farneback plan: every constant the kernels see, worked out on the host (rc_plan.cpp).  Host-only:
// no HIP header, so the unit also builds with a plain C++ compiler and is tested without a GPU (tests/test_plan_host.py).
#pragma once

#include <stddef.h>

#include "../../include/rcflow.h"

#define RC_MAX_LEVELS 12
#define RC_MAX_POLY_N 32      // taps -n..n kept on device
#define RC_MAX_WIN_M 32       // window radius winsize/2

// Geometry and constants of one pyramid scale.
struct RcLevel {
    int w, h;            // level size (cvRound(W*scale))
    double scale_x;      // W0 / w   (resize.cpp scale_x)
    double scale_y;
    double sigma;        // pyramid blur sigma
    int ksize;           // pyramid blur taps
    int pyr_tw, pyr_th;  // pyr_level tile
    int pyr_reg_w, pyr_reg_h;  // LDS source region bounds (bytes / rows)
    size_t pyr_lds;
};

// Polynomial-expansion constants (FarnebackPrepareGaussian), taps 0..n.
struct RcPolyK {
    float g[RC_MAX_POLY_N + 1];
    float xg[RC_MAX_POLY_N + 1];
    float xxg[RC_MAX_POLY_N + 1];
    double ig11, ig03, ig33, ig55;
    double kdc;   // coefficient of the removed DC term in the yy/xx outputs
    int n;        // requested radius
    int n_eff;    // radius actually evaluated
    // Derived taps of the fast expansion: the constants its outputs are multiplied with, folded into
    // the filters.  Each is formed in double from the values above and rounded to float once; the outputs come out at the
    // stored scale of the fast R planes ((y, x, yy, xx) / 2, xy / 4: DESIGN.md section 3).
    float qh[RC_MAX_POLY_N + 1];    // (ig03 g + ig33 xxg) / 2: yy = qh_v(g_h), xx = g_v(qh_h)
    float xga[RC_MAX_POLY_N + 1];   // xg ig11 / 2: y = xga_v(g_h), x = g_v(xga_h)
    float xgb[RC_MAX_POLY_N + 1];   // xg (ig55 / 4) / (ig11 / 2): xy = xgb_v(xga_h)
    double kdch;                    // kdc / 2
};

// Window of FarnebackUpdateFlow_*: box (scale = 1/bs^2) or Gaussian (float taps).
struct RcWindow {
    float k[RC_MAX_WIN_M + 1];
    double box_scale;
    double box_eps;           // 1e-3 / box_scale^2: regulariser for unscaled window sums
    int m;
    int gaussian;
};

int rc_plan_params_valid(const rc_farneback_params* p);
// optflow.cpp calc(): the levels left after the crop at 32 pixels; the geometry of scale k
int rc_plan_crop_levels(int w, int h, double pyr_scale, int levels);
void rc_plan_level_geom(int w, int h, double pyr_scale, int k, RcLevel& L);
// pyr_scale^L as calc() accumulates it (L multiplications from 1)
double rc_plan_scale_pow(double pyr_scale, int L);
// the pyr_level tile of a scale of a W0 x H0 frame and its LDS bytes (L.ksize and the scales set)
void rc_plan_pick_pyr_tile(RcLevel& L, int W0, int H0);
// smooth.cpp getGaussianKernel(n, sigma, CV_32F): n floats
void rc_plan_gaussian_kernel(int n, double sigma, float* cf);
// optflow.cpp FarnebackPrepareGaussian; RC_EINVAL when the moment matrix is not positive definite
int rc_plan_prepare_poly(int n, double sigma, int exact_taps, RcPolyK& pk);
void rc_plan_window(int winsize, int flags, RcWindow& win);
