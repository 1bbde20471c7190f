// warp_kernels.hip -- general image warps on the device: cv::warpAffine and cv::warpPerspective on 8UC3 frames
// (INTER_LINEAR, BORDER_CONSTANT 0, a destination size of its own), and the correcting warp of the multi-patch
// stabiliser (stab_kernels.hip), which reads its matrix from device memory.  The arithmetic is OpenCV 4.1.0's CPU path
// (imgwarp.cpp), restated here from knowledge of upstream: parity-unpinned.
//
// Coordinates, for the destination-to-source matrix M (a forward matrix is inverted on the host in double first):
//   affine       fixed point, 10 + 5 fraction bits: X = (cvRound((M1 y + M2) 1024) + 16 + cvRound(M0 x 1024)) >> 5,
//                Y likewise from M3..M5; source pixel (sat_short(X >> 5), sat_short(Y >> 5)), fractions X & 31, Y & 31.
//                M = [1 0 sx; 0 1 sy] is k_stab_warp's arithmetic (stab_kernels.hip) term by term.
//   perspective  double per pixel, in upstream's blocks of bw0 columns (64 for any real frame) starting at xb:
//                X0 = M0 xb + M1 y + M2 (Y0, W0 likewise), W = W0 + M6 (x - xb), W = W ? 32 / W : 0,
//                X = cvRound(max(INT_MIN, min(INT_MAX, (X0 + M0 (x - xb)) W))), then as above.  The bits of X depend on xb.
// Sample: remap's 8-bit table form (rc_pix3_bilinear, shared with k_stab_warp), a tap outside the source counts 0.
//
// A lane owns 4 consecutive destination pixels of a row and stores them as one dwordx3 (a w % 4 tail by bytes); a wave
// owns 256 pixels of one row.  The source is a gather: a pixel whose 2 x 2 footprint (and the byte pair behind it) lies
// inside the frame reads its two rows as unaligned 8-byte loads, any other pixel tap by tap with a bounds check on every
// tap, so no matrix, however wild, reads outside the source.  No LDS.

#include <limits.h>
#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_pix3.h"

__device__ __forceinline__ int wp_sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// std::max((double)INT_MIN, std::min((double)INT_MAX, v)) with the library's comparisons: a NaN becomes INT_MAX
__device__ __forceinline__ double wp_clamp_int(double v) {
    v = v < (double)INT_MAX ? v : (double)INT_MAX;
    return (double)INT_MIN < v ? v : (double)INT_MIN;
}

template <int PERSP>
__global__ __launch_bounds__(RC_BLOCK) void k_warp(const RcWarpArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int y = blockIdx.y * RC_PIX3_WAVES + wave;
    const int x0 = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), n = min(4, a.dw - x0);
    if (y >= a.dh || n <= 0) return;
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = a.M[i];
    if (a.d_M) {                                         // the stabiliser's fit: 2 x 3, or 3 x 3 for the perspective form
#pragma unroll
        for (int i = 0; i < (PERSP ? 9 : 6); i++) M[i] = a.d_M[i];
    }
    const double yd = (double)y;
    int X0 = 0, Y0 = 0;
    if (!PERSP) {
        X0 = __double2int_rn((M[1] * yd + M[2]) * 1024.0) + 16;
        Y0 = __double2int_rn((M[4] * yd + M[5]) * 1024.0) + 16;
    }
    const int xb0 = PERSP ? (x0 / a.bw0) * a.bw0 : 0;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x0 + k;
        int X, Y;
        if (PERSP) {
            // a lane's pixels share the block unless bw0 is no multiple of 4 (destinations below 16 rows or 64 columns)
            const int xb = x - xb0 >= a.bw0 ? xb0 + a.bw0 : xb0;
            const double xbd = (double)xb, x1 = (double)(x - xb);
            const double bX = M[0] * xbd + M[1] * yd + M[2], bY = M[3] * xbd + M[4] * yd + M[5], bW = M[6] * xbd + M[7] * yd + M[8];
            double W = bW + M[6] * x1;
            W = W != 0. ? 32.0 / W : 0.;
            X = __double2int_rn(wp_clamp_int((bX + M[0] * x1) * W));
            Y = __double2int_rn(wp_clamp_int((bY + M[3] * x1) * W));
        } else {
            // wrapping sums: a matrix from device memory is not range-checked, and every tap below is
            X = (int)((unsigned)X0 + (unsigned)__double2int_rn(M[0] * (double)x * 1024.0)) >> 5;
            Y = (int)((unsigned)Y0 + (unsigned)__double2int_rn(M[3] * (double)x * 1024.0)) >> 5;
        }
        const int sx = wp_sat_short(X >> 5), sy = wp_sat_short(Y >> 5), fx = X & 31, fy = Y & 31;
        uint32_t p00, p01, p10, p11;
        if (sx >= 0 && sx + 2 < a.sw && sy >= 0 && sy + 1 < a.sh) {
            // two pixels = 6 of the 8 bytes; pixel sx + 2 exists, so the load stays inside the row
            const uint8_t* s0 = a.src + (size_t)sy * a.step + 3 * (size_t)sx;
            rc_pix3_unpack2(s0, p00, p01);
            rc_pix3_unpack2(s0 + a.step, p10, p11);
        } else {
            p00 = rc_pix3_tap(a.src, a.step, a.sw, a.sh, sx, sy); p01 = rc_pix3_tap(a.src, a.step, a.sw, a.sh, sx + 1, sy);
            p10 = rc_pix3_tap(a.src, a.step, a.sw, a.sh, sx, sy + 1); p11 = rc_pix3_tap(a.src, a.step, a.sw, a.sh, sx + 1, sy + 1);
        }
        o[k] = rc_pix3_bilinear(p00, p01, p10, p11, fx, fy);
    }
    rc_pix3_store4(a.dst + (size_t)y * a.dst_step, x0, n, o);
    // the stabiliser's kept patches: gray float of the corrected frame inside every ROI (they may overlap)
    if (!PERSP && a.patch) {
        for (int r = 0; r < a.npatch; r++) {
            if ((unsigned)(y - a.ry[r]) >= (unsigned)a.rh) continue;      // wave-uniform: y and the ROI are
            float* row = a.patch + ((size_t)r * a.rh + (y - a.ry[r])) * a.rw;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int px = x0 + k - a.rx[r];
                if (k < n && (unsigned)px < (unsigned)a.rw) row[px] = rc_pix3_gray(o[k]);
            }
        }
    }
}

// ============================================================================ host side
// "framestab@8" the affine warp, "framestab@9" the perspective warp
void rc_warp_launch(rc_ctx* ctx, hipStream_t cur, RcWarpArgs& a, bool perspective) {
    const int bh0 = a.dh < 16 ? a.dh : 16;
    a.bw0 = 1024 / bh0 < a.dw ? 1024 / bh0 : a.dw;
    const dim3 grid = rc_pix3_grid(a.dw, a.dh, 1);
    // compulsory bytes: the destination once, as many source bytes (the footprint of a near-identity map), the patches
    const double bytes = 6. * a.dw * a.dh + (a.patch ? 4. * a.npatch * a.rw * a.rh : 0.) + (a.d_M ? (perspective ? 72. : 48.) : 0.);
    RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, perspective ? 9 : 8, bytes);
    if (perspective) hipLaunchKernelGGL(k_warp<1>, grid, dim3(RC_BLOCK), 0, cur, a);
    else hipLaunchKernelGGL(k_warp<0>, grid, dim3(RC_BLOCK), 0, cur, a);
}

static int wp_check(const char* who, rc_ctx* ctx, const uint8_t* d_bgr, size_t step, int sw, int sh, uint8_t* d_out, size_t out_step,
                    int dw, int dh, const double* M, int nm, int flags) {
    if (rc_img3_check(who, "d_bgr", d_bgr, step, sw, sh) || rc_img3_check(who, "d_out", d_out, out_step, dw, dh)) return RC_EINVAL;
    if (!M) { rc_set_error("%s: no matrix", who); return RC_EINVAL; }
    if (flags & ~RC_WARP_INVERSE_MAP) { rc_set_error("%s: unknown flag bits 0x%x", who, flags & ~RC_WARP_INVERSE_MAP); return RC_EINVAL; }
    for (int i = 0; i < nm; i++)
        if (!isfinite(M[i])) { rc_set_error("%s: matrix entry %d is not finite", who, i); return RC_EINVAL; }
    if (rc_fits_context(who, ctx, sw, sh) || rc_fits_context(who, ctx, dw, dh)) return RC_ESIZE;
    return rc_img3_pair(who, "d_bgr", d_bgr, step, sw, sh, "d_out", d_out, out_step, dw, dh);   // the warp is not in place
}

extern "C" int rcflow_warp_affine_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int sw, int sh, uint8_t* d_out,
                                          size_t out_step, int dw, int dh, const double M[6], int flags) {
    static const char* who = "rcflow_warp_affine_bgr_dev";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    int rc = wp_check(who, ctx, d_bgr, step, sw, sh, d_out, out_step, dw, dh, M, 6, flags);
    if (rc) return rc;
    double m[6];
    memcpy(m, M, sizeof(m));
    if (!(flags & RC_WARP_INVERSE_MAP)) {
        // warpAffine's own inversion, in its order of operations
        double D = m[0] * m[4] - m[1] * m[3];
        if (D == 0. || !isfinite(1. / D)) { rc_set_error("%s: the matrix is singular", who); return RC_EINVAL; }
        D = 1. / D;
        const double A11 = m[4] * D, A22 = m[0] * D;
        m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22;
        const double b1 = -m[0] * m[2] - m[1] * m[5], b2 = -m[3] * m[2] - m[4] * m[5];
        m[2] = b1; m[5] = b2;
    }
    // the fixed-point coordinates are 32-bit with 10 fraction bits: every term of a corner's coordinate, summed by
    // magnitude, stays within 2^20 px (for a translation: the translate warp's bound on the shift)
    const double bx = fabs(m[0]) * (dw - 1) + fabs(m[1]) * (dh - 1) + fabs(m[2]);
    const double by = fabs(m[3]) * (dw - 1) + fabs(m[4]) * (dh - 1) + fabs(m[5]);
    if (!(bx <= 1048576.) || !(by <= 1048576.)) {
        rc_set_error("%s: the matrix maps a destination corner beyond 2^20 px (|x| up to %g, |y| up to %g)", who, bx, by);
        return RC_EINVAL;
    }
    RC_HIP(hipSetDevice(ctx->device));
    RcWarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_bgr; a.step = step; a.sw = sw; a.sh = sh; a.dst = d_out; a.dst_step = out_step; a.dw = dw; a.dh = dh;
    memcpy(a.M, m, sizeof(m));
    rc_warp_launch(ctx, s->cur, a, false);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_warp_perspective_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int sw, int sh, uint8_t* d_out,
                                               size_t out_step, int dw, int dh, const double M[9], int flags) {
    static const char* who = "rcflow_warp_perspective_bgr_dev";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    int rc = wp_check(who, ctx, d_bgr, step, sw, sh, d_out, out_step, dw, dh, M, 9, flags);
    if (rc) return rc;
    double m[9];
    memcpy(m, M, sizeof(m));
    if (!(flags & RC_WARP_INVERSE_MAP)) {
        const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[3] * m[8] - m[5] * m[6], c02 = m[3] * m[7] - m[4] * m[6];
        const double det = m[0] * c00 - m[1] * c01 + m[2] * c02;
        if (det == 0. || !isfinite(1. / det)) { rc_set_error("%s: the matrix is singular", who); return RC_EINVAL; }
        const double d = 1. / det;
        const double o[9] = {c00 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
                             (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                             (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d};
        for (int i = 0; i < 9; i++)
            if (!isfinite(o[i])) { rc_set_error("%s: the inverse of the matrix is not finite", who); return RC_EINVAL; }
        memcpy(m, o, sizeof(m));
    }
    RC_HIP(hipSetDevice(ctx->device));
    RcWarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_bgr; a.step = step; a.sw = sw; a.sh = sh; a.dst = d_out; a.dst_step = out_step; a.dw = dw; a.dh = dh;
    memcpy(a.M, m, sizeof(m));
    rc_warp_launch(ctx, s->cur, a, true);
    RC_HIP(hipGetLastError());
    return RC_OK;
}
