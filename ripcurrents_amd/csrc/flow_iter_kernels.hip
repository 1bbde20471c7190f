// flow_iter_kernels.hip -- the fused Farneback iteration kernel (SURVEY.md section 8(a) rows
// A3 FarnebackUpdateMatrices, A4/A5 FarnebackUpdateFlow_Blur/_GaussianBlur, A6 stripe
// logic; call site RipCurrents_main/ripcurrents.cpp:215):
//
//     flow_out = solve( window( M( R0, R1 sampled at p + flow_in, flow_in ) ) )
//
// The 5-channel matrix image M of the upstream algorithm never goes to HBM: a block
// evaluates it for its tile plus the window halo straight into LDS (clamped coordinates =
// the replicate border of the window), applies the separable window there and solves the
// 2x2 system in double like upstream.  Upstream's in-loop stripe update (A6) equals
// "window+solve the whole image, then update all matrices" (a CPU test pins that
// equivalence), so one launch of this kernel is one iteration and the intermediate flow of
// iteration i only exists as this kernel's input for iteration i+1.
//
// HBM traffic per pixel: R0 20 B + R1 20 B (gathered; L2 serves the 4x bilinear overlap)
// + flow_in 8 B (2 B when it is the coarser level, 0 at the coarsest) + flow_out 8 B.
//
// Compile-time tile/window instantiations cover the reference's window sizes (3, 5, 10,
// 20: SURVEY.md section 2.2); any other winsize takes the generic runtime kernel.

#include <cstdlib>
#include <cstring>

#include "rc_device.h"

#define RC_ITER_BATCH 3
#define RC_RR_D 3         // displacements below this many pixels are served from the LDS window (28 x 28 tile)

// This file is compiled twice.  The default build (namespace rc_flow_fast) is the fast arithmetic:
// sums of products as fused multiply-adds, the winsize-3 solve in fp32 (Kahan).  With -DRC_EXACT_BUILD
// (namespace rc_flow_exact, object flow_iter_kernels_exact.o) the SAME kernels evaluate
// FarnebackUpdateMatrices in optflow.cpp's operation order without fused multiply-adds and solve every 2x2
// system in double like upstream: together with the Gaussian window sums -- which are upstream's order in
// both builds -- the iteration is then bit-identical to the CPU path.  Option "exact" selects that build
// for Gaussian windows (box windows need upstream's running sums: exact_kernels.hip).
#ifdef RC_EXACT_BUILD
#define RC_FLOW_NS rc_flow_exact
#else
#define RC_FLOW_NS rc_flow_fast
#endif
namespace RC_FLOW_NS {

// resize(prevFlow, INTER_LINEAR) then flow *= 1/pyr_scale (optflow.cpp calc()), or the
// same-resolution flow of the previous iteration, or zeros at the coarsest scale.
__device__ __forceinline__ float2 rc_flow_in(const RcIterArgs& a, const float2* fin, int gx, int gy) {
    if (a.in_mode == 0) return make_float2(0.f, 0.f);
    if (a.in_mode == 1) return fin[(size_t)gy * a.w + gx];
    float ax, ay;
    int sx = rc_src_x(gx, a.up_scale_x, a.fin_w, ax);
    int sx1 = min(sx + 1, a.fin_w - 1);
    int sy = rc_src_y(gy, a.up_scale_y, ay);
    int sy0 = rc_clampi(sy, 0, a.fin_h - 1), sy1 = rc_clampi(sy + 1, 0, a.fin_h - 1);
    const float2* S0 = fin + (size_t)sy0 * a.fin_w;
    const float2* S1 = fin + (size_t)sy1 * a.fin_w;
    float2 p00 = S0[sx], p01 = S0[sx1], p10 = S1[sx], p11 = S1[sx1];
    float a0 = 1.f - ax, a1 = ax, b0 = 1.f - ay, b1 = ay;
    float r0x = p00.x * a0 + p01.x * a1, r1x = p10.x * a0 + p11.x * a1;
    float r0y = p00.y * a0 + p01.y * a1, r1y = p10.y * a0 + p11.y * a1;
    float2 v;
    v.x = (r0x * b0 + r1x * b1) * a.up_mul;
    v.y = (r0y * b0 + r1y * b1) * a.up_mul;
    return v;
}

// FarnebackUpdateMatrices for one pixel, in two steps so that a thread can have the gathers of
// several pixels in flight: rc_gather_issue starts the loads, rc_matrices_reg consumes them.
// Every flow kernel goes through these two functions, so they all produce the same bits.
// Sums of products are written as fused multiply-adds (one rounding per term, like an
// FMA-enabled build of the upstream C++); the rest keeps optflow.cpp's operation order.
struct RcM5 { float m0, m1, m2, m3, m4; };

struct RcGather {
    float4 q00, q01, q10, q11;
    float e00, e01, e10, e11;
    float fx, fy;
    bool inside;
};

__device__ __forceinline__ void rc_gather_issue(RcGather& g, const float4* __restrict__ RA1,
                                                const float* __restrict__ RB1, int gx, int gy, float dx,
                                                float dy, int w, int h) {
    float fx = gx + dx, fy = gy + dy;
    int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
    g.fx = fx - x1;
    g.fy = fy - y1;
    g.inside = (unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1);
    const size_t p = g.inside ? (size_t)y1 * w + x1 : (size_t)gy * w + gx;
    const size_t pw = g.inside ? (size_t)w : 0, p1 = g.inside ? 1 : 0;
    g.q00 = RA1[p]; g.q01 = RA1[p + p1]; g.q10 = RA1[p + pw]; g.q11 = RA1[p + pw + p1];
    g.e00 = RB1[p]; g.e01 = RB1[p + p1]; g.e10 = RB1[p + pw]; g.e11 = RB1[p + pw + p1];
}

// Stored scale of the R planes.  The exact build reads R as upstream defines it.  The fast build
// reads what the fast expansion writes: (y, x, yy, xx) x 1/2 and xy x 1/4, so that R0 and the R1 texels enter
// rc_matrices_reg's chains as they are.

__device__ __forceinline__ RcM5 rc_matrices_reg(const float4 A0, const float B0, const RcGather& g, float dx,
                                                float dy, int X, int Y, int w, int h, bool BORDER = true) {
    float fx = g.fx, fy = g.fy;
#ifdef RC_EXACT_BUILD
    float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy);
    float a10 = (1.f - fx) * fy, a11 = fx * fy;
#define RC_BILIN(c, e) (a00 * e##00 c + a01 * e##01 c + a10 * e##10 c + a11 * e##11 c)
    float r2 = RC_BILIN(.x, g.q), r3 = RC_BILIN(.y, g.q), r4 = RC_BILIN(.z, g.q), r5 = RC_BILIN(.w, g.q);
    float r6 = RC_BILIN(, g.e);
#undef RC_BILIN
    r4 = (A0.z + r4) * 0.5f;
    r5 = (A0.w + r5) * 0.5f;
    r6 = (B0 + r6) * 0.25f;
    if (!g.inside) {
        r2 = r3 = 0.f;
        r4 = A0.z;
        r5 = A0.w;
        r6 = B0 * 0.5f;
    }
    r2 = (A0.x - r2) * 0.5f;
    r3 = (A0.y - r3) * 0.5f;
#else
    // The averages with R0 ((R0 -/+ bilinear) / 2, xy: / 4) folded into the interpolation: the planes are STORED at half
    // (xy: quarter) scale, so the chain starts at the stored R0 and adds the plain bilinear weights times the stored R1
    // texels -- four fused multiply-adds per coefficient instead of a product, three of them, a sum and a scaling.
    // Every term is a power of two times the term of (R0 -/+ bilinear R1) / 2 on unscaled planes: the same bits.
    const float hx0 = 1.f - fx, fy0 = 1.f - fy;
    const float h00 = hx0 * fy0, h01 = fx * fy0, h10 = hx0 * fy, h11 = fx * fy;
#define RC_BILIN_FROM(s0, sg, c, e) RC_FMA(sg h11, e##11 c, RC_FMA(sg h10, e##10 c, RC_FMA(sg h01, e##01 c, RC_FMA(sg h00, e##00 c, s0))))
    float r2 = RC_BILIN_FROM(A0.x, -, .x, g.q), r3 = RC_BILIN_FROM(A0.y, -, .y, g.q);
    float r4 = RC_BILIN_FROM(A0.z, +, .z, g.q), r5 = RC_BILIN_FROM(A0.w, +, .w, g.q);
    float r6 = RC_BILIN_FROM(B0, +, , g.e);
#undef RC_BILIN_FROM
    if (!g.inside) {
        r2 = A0.x;
        r3 = A0.y;
        r4 = 2.f * A0.z;
        r5 = 2.f * A0.w;
        r6 = 2.f * B0;
    }
#endif
#ifdef RC_EXACT_BUILD
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
#else
    r2 = RC_FMA(r6, dx, RC_FMA(r4, dy, r2));
    r3 = RC_FMA(r5, dx, RC_FMA(r6, dy, r3));
#endif
    if (BORDER && ((unsigned)(X - 5) >= (unsigned)(w - 10) || (unsigned)(Y - 5) >= (unsigned)(h - 10))) {
        float bl = X < 5 ? (X < 2 ? 0.14f : 0.4472f) : 1.f;
        int rx = w - X - 1;
        float br = X >= w - 5 ? (rx < 2 ? 0.14f : 0.4472f) : 1.f;
        float bt = Y < 5 ? (Y < 2 ? 0.14f : 0.4472f) : 1.f;
        int ry = h - Y - 1;
        float bb = Y >= h - 5 ? (ry < 2 ? 0.14f : 0.4472f) : 1.f;
        float scale = bl * br * bt * bb;
        r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
    }
    RcM5 o;
#ifdef RC_EXACT_BUILD
    o.m0 = r4 * r4 + r6 * r6;
    o.m1 = (r4 + r5) * r6;
    o.m2 = r5 * r5 + r6 * r6;
    o.m3 = r4 * r2 + r6 * r3;
    o.m4 = r6 * r2 + r5 * r3;
#else
    o.m0 = RC_FMA(r4, r4, r6 * r6);
    o.m1 = (r4 + r5) * r6;
    o.m2 = RC_FMA(r5, r5, r6 * r6);
    o.m3 = RC_FMA(r4, r2, r6 * r3);
    o.m4 = RC_FMA(r6, r2, r5 * r3);
#endif
    return o;
}

__device__ __forceinline__ RcM5 rc_matrices(const float4* __restrict__ RA0, const float* __restrict__ RB0,
                                            const float4* __restrict__ RA1, const float* __restrict__ RB1,
                                            int gx, int gy, int w, int h, float dx, float dy) {
    size_t p0 = (size_t)gy * w + gx;
    float4 A0 = RA0[p0];
    float B0 = RB0[p0];
    RcGather g;
    rc_gather_issue(g, RA1, RB1, gx, gy, dx, dy, w, h);
    return rc_matrices_reg(A0, B0, g, dx, dy, gx, gy, w, h);
}

__device__ __forceinline__ float2 rc_solve(const double* g) {
    double idet = 1. / (g[0] * g[2] - g[1] * g[1] + 1e-3);
    float2 f;
    f.x = (float)((g[0] * g[4] - g[1] * g[3]) * idet);
    f.y = (float)((g[2] * g[3] - g[1] * g[4]) * idet);
    return f;
}

// 2x2 solve from the UNSCALED window sums: with every g multiplied by s = 1/winsize^2 the
// factor s^2 cancels except in the +1e-3 regulariser, so eps = 1e-3 / s^2 is used instead.
// The differences of products cancel, so each is formed with Kahan's fma scheme
// (w = c*d; (fma(a,b,-w)) + fma(-c,d,w): within 1.5 ulp of the exact difference, no doubles);
// the final division is an fp32 reciprocal (1 ulp).  All far inside the parity tolerance.
__device__ __forceinline__ float rc_diff_of_products(float a, float b, float c, float d) {
    float w = c * d;
    float e = RC_FMA(-c, d, w);
    float f = RC_FMA(a, b, -w);
    return f + e;
}
__device__ __forceinline__ float2 rc_solve3(const float* g, float eps) {
#ifdef RC_EXACT_BUILD
    // upstream's solve (Gaussian windows only reach this build: the float window values, widened)
    (void)eps;
    const double d[5] = {g[0], g[1], g[2], g[3], g[4]};
    return rc_solve(d);
#endif
    float det = rc_diff_of_products(g[0], g[2], g[1], g[1]) + eps;
    float nx = rc_diff_of_products(g[0], g[4], g[1], g[3]);
    float ny = rc_diff_of_products(g[2], g[3], g[1], g[4]);
    float idet = __builtin_amdgcn_rcpf(det);
    return make_float2(nx * idet, ny * idet);
}

// TW, TH, M compile-time (TW = TH = 0: runtime values from the arguments).
template <int TW_, int TH_, int M_, int GAUSS_>
__global__ __launch_bounds__(RC_BLOCK) void k_flow_iter(RcIterArgs a) {
    extern __shared__ __align__(16) float smf[];
    constexpr bool RT = (TW_ == 0);
    const int tw = RT ? a.tw : TW_, th = RT ? a.th : TH_, m = RT ? a.win.m : M_;
    const bool gauss = RT ? (a.win.gaussian != 0) : (GAUSS_ != 0);
    const int tid = threadIdx.x;
    const int z = blockIdx.y;
    const int t = a.xcd_remap ? rc_xcd_remap(blockIdx.x, a.tiles_x * a.tiles_y) : (int)blockIdx.x;
    const int tx0 = (t % a.tiles_x) * tw, ty0 = (t / a.tiles_x) * th;
    const int w = a.w, h = a.h;
    const int MW = tw + 2 * m, MH = th + 2 * m, MP = MW | 1;
    float* Ms = smf;                    // [5][MH][MP]

    const size_t s0 = (size_t)((a.slot0 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const size_t s1 = (size_t)((a.slot1 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const float4* RA0 = a.RA + s0;  const float* RB0 = a.RB + s0;
    const float4* RA1 = a.RA + s1;  const float* RB1 = a.RB + s1;
    const float2* fin = a.fin ? a.fin + (size_t)z * a.fin_pair_stride : nullptr;
    char* fout = a.fout + (size_t)z * a.fout_pair_stride;

    if (!a.solve) {   // iterations == 0: the flow is the (up-sampled) initial flow
        for (int idx = tid; idx < tw * th; idx += RC_BLOCK) {
            int gx = tx0 + idx % tw, gy = ty0 + idx / tw;
            if (gx < w && gy < h)
                *(float2*)(fout + (size_t)gy * a.fout_step + (size_t)gx * 8) = rc_flow_in(a, fin, gx, gy);
        }
        return;
    }

    // ---- phase 1: matrices for tile + halo -> LDS.  Items are taken RC_ITER_BATCH at a
    // time so that a thread has that many flow loads, then that many gathers, in flight
    // (the gather address depends on the flow: two HBM round trips per item otherwise).
    for (int base = tid; base < MW * MH; base += RC_BLOCK * RC_ITER_BATCH) {
        float2 d[RC_ITER_BATCH];
        int gxs[RC_ITER_BATCH], gys[RC_ITER_BATCH];
#pragma unroll
        for (int q = 0; q < RC_ITER_BATCH; q++) {
            int idx = min(base + q * RC_BLOCK, MW * MH - 1);
            int ly = idx / MW, lx = idx - ly * MW;
            gxs[q] = rc_clampi(tx0 - m + lx, 0, w - 1);
            gys[q] = rc_clampi(ty0 - m + ly, 0, h - 1);
            d[q] = rc_flow_in(a, fin, gxs[q], gys[q]);
        }
        RcM5 v[RC_ITER_BATCH];
#pragma unroll
        for (int q = 0; q < RC_ITER_BATCH; q++)
            v[q] = rc_matrices(RA0, RB0, RA1, RB1, gxs[q], gys[q], w, h, d[q].x, d[q].y);
#pragma unroll
        for (int q = 0; q < RC_ITER_BATCH; q++) {
            int idx = base + q * RC_BLOCK;
            if (idx < MW * MH) {
                int ly = idx / MW, lx = idx - ly * MW;
                float* mp = Ms + ly * MP + lx;
                mp[0] = v[q].m0;
                mp[MH * MP] = v[q].m1;
                mp[2 * MH * MP] = v[q].m2;
                mp[3 * MH * MP] = v[q].m3;
                mp[4 * MH * MP] = v[q].m4;
            }
        }
    }
    __syncthreads();

    if constexpr (!RT && M_ == 1) {
        // ---- small window: each thread owns one column and RPT rows; the vertical sums of
        // its 2M+1 columns stay in registers (no second LDS buffer, no second barrier).
        constexpr int RPT = TH_ / (RC_BLOCK / TW_);
        constexpr int NC = 2 * M_ + 1;
        const int lx = tid % TW_, r0 = (tid / TW_) * RPT;
        const int gx = tx0 + lx;
        double g[RPT][5];
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const float* mc = Ms + c * MH * MP + r0 * MP + lx;
            float col[NC][RPT + 2 * M_];
#pragma unroll
            for (int j = 0; j < NC; j++)
#pragma unroll
                for (int r = 0; r < RPT + 2 * M_; r++) col[j][r] = mc[r * MP + j];
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                float v[NC];
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    if (GAUSS_) {
                        float s = col[j][r + M_] * a.win.k[0];
#pragma unroll
                        for (int i = 1; i <= M_; i++) s += (col[j][r + M_ + i] + col[j][r + M_ - i]) * a.win.k[i];
                        v[j] = s;
                    } else {
                        float s = col[j][r + M_];
#pragma unroll
                        for (int i = 1; i <= M_; i++) s += col[j][r + M_ + i] + col[j][r + M_ - i];
                        v[j] = s;
                    }
                }
                if (GAUSS_) {
                    float s = v[M_] * a.win.k[0];
#pragma unroll
                    for (int i = 1; i <= M_; i++) s += a.win.k[i] * (v[M_ - i] + v[M_ + i]);
                    g[r][c] = s;
                } else {
                    double s = v[M_];
#pragma unroll
                    for (int i = 1; i <= M_; i++) s += (double)v[M_ + i] + (double)v[M_ - i];
                    g[r][c] = s * a.win.box_scale;
                }
            }
        }
        if (gx < w) {
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                int gy = ty0 + r0 + r;
                if (gy < h) *(float2*)(fout + (size_t)gy * a.fout_step + (size_t)gx * 8) = rc_solve(g[r]);
            }
        }
    } else {
        // ---- large window: separable through a second LDS buffer
        float* Vs = smf + 5 * MH * MP;      // [5][th][MP]
        for (int idx = tid; idx < 5 * th * MW; idx += RC_BLOCK) {
            int c = idx / (th * MW), rem = idx - c * (th * MW);
            int o = rem / MW, col = rem - o * MW;
            const float* mc = Ms + c * MH * MP + (o + m) * MP + col;
            float s;
            if (gauss) {
                s = mc[0] * a.win.k[0];
                for (int i = 1; i <= m; i++) s += (mc[i * MP] + mc[-i * MP]) * a.win.k[i];
            } else {
                s = mc[0];
                for (int i = 1; i <= m; i++) s += mc[i * MP] + mc[-i * MP];
            }
            Vs[c * th * MP + o * MP + col] = s;
        }
        __syncthreads();
        for (int idx = tid; idx < tw * th; idx += RC_BLOCK) {
            int o = idx / tw, lx = idx - o * tw;
            int gx = tx0 + lx, gy = ty0 + o;
            if (gx >= w || gy >= h) continue;
            double g[5];
            const float* vc = Vs + o * MP + lx + m;
            if (gauss) {
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    const float* v = vc + c * th * MP;
                    float s = v[0] * a.win.k[0];
                    for (int i = 1; i <= m; i++) s += a.win.k[i] * (v[-i] + v[i]);
                    g[c] = s;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    const float* v = vc + c * th * MP;
                    double s = v[0];
                    for (int i = 1; i <= m; i++) s += (double)v[i] + (double)v[-i];
                    g[c] = s * a.win.box_scale;
                }
            }
            *(float2*)(fout + (size_t)gy * a.fout_step + (size_t)gx * 8) = rc_solve(g);
        }
    }
}

// ------------------------------------------------------------------------------------
// Large windows (winsize 5 / 10 / 20: the Android fork, main.cpp:1119, main.cpp:609): 32x32 tile,
// NT threads chosen so that the one to three blocks the LDS footprint allows still put 16 waves
// on a CU.  Same three phases and the same operation order as k_flow_iter (bit-identical), but
// the vertical pass walks each column with a register window (one LDS read per new row instead
// of 2M+1 per output).
template <int M_, int GAUSS_, int NT, int TW>
__global__ __launch_bounds__(NT) void k_flow_iter_big(RcIterArgs a) {
    constexpr int TH = 32, MW = TW + 2 * M_, MH = TH + 2 * M_, MP = MW | 1;
    constexpr int CH = 8, NCH = TH / CH;                 // vertical pass: chunks of CH output rows
    extern __shared__ __align__(16) float smf[];
    float* Ms = smf;                    // [5][MH][MP]
    float* Vs = smf + 5 * MH * MP;      // [5][TH][MP]
    const int tid = threadIdx.x;
    const int z = blockIdx.y;
    const int t = a.xcd_remap ? rc_xcd_remap(blockIdx.x, a.tiles_x * a.tiles_y) : (int)blockIdx.x;
    const int tx0 = (t % a.tiles_x) * TW, ty0 = (t / a.tiles_x) * TH;
    const int w = a.w, h = a.h;
    const size_t s0 = (size_t)((a.slot0 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const size_t s1 = (size_t)((a.slot1 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const float4* RA0 = a.RA + s0;  const float* RB0 = a.RB + s0;
    const float4* RA1 = a.RA + s1;  const float* RB1 = a.RB + s1;
    const float2* fin = a.fin ? a.fin + (size_t)z * a.fin_pair_stride : nullptr;
    char* fout = a.fout + (size_t)z * a.fout_pair_stride;

    // ---- phase 1: matrices for tile + halo -> LDS
    for (int base = tid; base < MW * MH; base += NT * RC_ITER_BATCH) {
        float2 d[RC_ITER_BATCH];
        int gxs[RC_ITER_BATCH], gys[RC_ITER_BATCH];
#pragma unroll
        for (int q = 0; q < RC_ITER_BATCH; q++) {
            int idx = min(base + q * NT, MW * MH - 1);
            int ly = idx / MW, lx = idx - ly * MW;
            gxs[q] = rc_clampi(tx0 - M_ + lx, 0, w - 1);
            gys[q] = rc_clampi(ty0 - M_ + ly, 0, h - 1);
            d[q] = rc_flow_in(a, fin, gxs[q], gys[q]);
        }
        RcM5 v[RC_ITER_BATCH];
#pragma unroll
        for (int q = 0; q < RC_ITER_BATCH; q++)
            v[q] = rc_matrices(RA0, RB0, RA1, RB1, gxs[q], gys[q], w, h, d[q].x, d[q].y);
#pragma unroll
        for (int q = 0; q < RC_ITER_BATCH; q++) {
            int idx = base + q * NT;
            if (idx < MW * MH) {
                int ly = idx / MW, lx = idx - ly * MW;
                float* mp = Ms + ly * MP + lx;
                mp[0] = v[q].m0;
                mp[MH * MP] = v[q].m1;
                mp[2 * MH * MP] = v[q].m2;
                mp[3 * MH * MP] = v[q].m3;
                mp[4 * MH * MP] = v[q].m4;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: vertical pass, item = (plane, chunk of CH rows, column); lanes walk columns
    for (int idx = tid; idx < 5 * NCH * MW; idx += NT) {
        const int c = idx / (NCH * MW), rem = idx - c * (NCH * MW);
        const int chunk = rem / MW, col = rem - chunk * MW;
        const float* mc = Ms + c * MH * MP + (chunk * CH) * MP + col;
        float v[CH + 2 * M_];
#pragma unroll
        for (int r = 0; r < CH + 2 * M_; r++) v[r] = mc[r * MP];
        float* vo = Vs + c * TH * MP + (chunk * CH) * MP + col;
#pragma unroll
        for (int j = 0; j < CH; j++) {
            float s;
            if (GAUSS_) {
                s = v[j + M_] * a.win.k[0];
#pragma unroll
                for (int i = 1; i <= M_; i++) s += (v[j + M_ + i] + v[j + M_ - i]) * a.win.k[i];
            } else {
                s = v[j + M_];
#pragma unroll
                for (int i = 1; i <= M_; i++) s += v[j + M_ + i] + v[j + M_ - i];
            }
            vo[j * MP] = s;
        }
    }
    __syncthreads();

    // ---- phase 3: horizontal pass + solve
    for (int idx = tid; idx < TW * TH; idx += NT) {
        int o = idx / TW, lx = idx - o * TW;
        int gx = tx0 + lx, gy = ty0 + o;
        if (gx >= w || gy >= h) continue;
        double g[5];
        const float* vc = Vs + o * MP + lx + M_;
        if (GAUSS_) {
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const float* v = vc + c * TH * MP;
                float s = v[0] * a.win.k[0];
#pragma unroll
                for (int i = 1; i <= M_; i++) s += a.win.k[i] * (v[-i] + v[i]);
                g[c] = s;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const float* v = vc + c * TH * MP;
                double s = v[0];
#pragma unroll
                for (int i = 1; i <= M_; i++) s += (double)v[i] + (double)v[-i];
                g[c] = s * a.win.box_scale;
            }
        }
        *(float2*)(fout + (size_t)gy * a.fout_step + (size_t)gx * 8) = rc_solve(g);
    }
}

// Every launcher below takes its tile and its grid from the launch's RcFlowForm (rc_flow_form), which also picked the
// launcher: the form the tests are told is the form that runs.  The tile rc_flow_form reports for a kernel and the tile
// the kernel's template is instantiated with come from the same constexpr functions, checked where each is instantiated.
constexpr int RC_W3_TW = 64, RC_W3_TH = 16;                                   // k_flow_iter_w3
constexpr int RC_SWEEP_TW = 64, RC_SWEEP_CH = 8, RC_SWEEP_NT = 1024;          // k_flow_iter_sweep
constexpr int RC_RRC_TW = 28, RC_RRC_NT = 256;                                // k_flow_iter2_rrc: 32 columns x 8 row groups
constexpr int rc_big_tw(int m) { return m == 10 ? 64 : 32; }                  // k_flow_iter_big (m = 5, 64 wide: 6 % slower, one block per CU)
constexpr int rc_big_nt(int m) { return m == 2 ? 512 : 1024; }
constexpr int rc_tile_tw(int m) { return m == 5 || m == 10 ? 32 : 64; }       // k_flow_iter<TW, TH, M, G>
constexpr int rc_tile_th(int m) { return m == 5 || m == 10 ? 32 : 16; }
constexpr int rc_rrc_d(int nit) { return nit == 4 ? RC_RR_D : 4; }
constexpr int rc_rrc_th(int nit) { return 8 * nit - 4; }
static void rc_form_grid(RcIterArgs& a, const RcFlowForm& f) {
    a.tw = f.tw; a.th = f.th;
    a.tiles_x = f.tiles_x; a.tiles_y = f.tiles_y;
}

template <int M, int G, int NT, int TW = 32>
static void launch_iter_big(RcIterArgs a, const RcFlowForm& f, int pairs, hipStream_t s) {
    constexpr int MW = TW + 2 * M, MH = 32 + 2 * M, MP = MW | 1;
    const size_t lds = sizeof(float) * 5 * (size_t)MP * (MH + 32);
    static_assert(TW == rc_big_tw(M) && NT == rc_big_nt(M), "rc_flow_form reports this kernel's tile and block");
    RC_ALLOW_LDS((k_flow_iter_big<M, G, NT, TW>), lds);
    rc_form_grid(a, f);
    hipLaunchKernelGGL((k_flow_iter_big<M, G, NT, TW>), dim3(a.tiles_x * a.tiles_y, pairs, 1), dim3(NT), lds, s, a);
}

// ------------------------------------------------------------------------------------
// Large Gaussian windows (winsize 10 / 20 x 3 iterations: main.cpp:609,961,1119,1481), one iteration
// per launch.  A block owns a strip of 64 output columns and sweeps a segment of a.th rows
// downwards, CH = 8 rows per step, with the matrices of the last CH + 2m rows in an LDS ring:
// every matrix row is evaluated once per strip (the tile kernel above re-evaluates the 2m halo
// rows of every 32-row tile: 2.1x the pixels at m = 10, here (64 + 2m)/64 x (rows + 2m)/rows).
//   a  matrices of the CH new rows (64 + 2m columns, global gathers, several pixels in flight)
//   b  vertical pass: item = (channel, column), register window of CH + 2m ring rows -> V
//   c1 horizontal pass: item = (channel, row, 4 pixels), 16-byte LDS reads of the V row
//   c2 solve + store.  The per-channel sums travel from c1 to c2 through the ring rows that
//      died with this step (the oldest CH), so the block needs no third buffer.
// Operation order of every sum is the tile kernel's (= optflow.cpp's): same bits.
template <int M_>
struct RcSweep {
    static constexpr int TW = 64, CH = 8, MW = TW + 2 * M_, MP = MW | 1;
    static constexpr int RING = ((CH + 2 * M_ + CH - 1) / CH) * CH;     // 32 rows (m = 10), 24 (m = 5)
    static constexpr int NQ = (4 + 2 * M_ + 3) / 4;                     // float4s under a 4-pixel group's taps
    static constexpr int VP = (MW + 3) & ~3;
    static_assert(4 * 15 + 4 * NQ <= VP, "V row holds the last group's taps");
    static_assert(CH * TW <= CH * MP, "c1 -> c2 sums fit the dead ring rows of one plane");
    static constexpr size_t LDS = sizeof(float) * (5 * RING * MP + 5 * CH * VP);
};

template <int M_, int NT, int START>
__device__ __forceinline__ void rc_sweep_bc(const RcIterArgs& a, float* ring, float* V, int tid, int tx0, int Y,
                                            int yend, char* fout) {
    using S = RcSweep<M_>;
    constexpr int CH = S::CH, MW = S::MW, MP = S::MP, RING = S::RING, VP = S::VP, NQ = S::NQ, TW = S::TW;
    // ---- b: vertical pass
    for (int idx = tid; idx < 5 * MW; idx += NT) {
        const int c = idx / MW, col = idx - c * MW;
        const float* mc = ring + c * RING * MP + col;
        float v[CH + 2 * M_];
#pragma unroll
        for (int r = 0; r < CH + 2 * M_; r++) v[r] = mc[((START + r) % RING) * MP];
        float* vo = V + c * CH * VP + col;
#pragma unroll
        for (int j = 0; j < CH; j++) {
            float s = v[j + M_] * a.win.k[0];
#pragma unroll
            for (int i = 1; i <= M_; i++) s += (v[j + M_ + i] + v[j + M_ - i]) * a.win.k[i];
            vo[j * VP] = s;
        }
    }
    __syncthreads();
    // ---- c1: horizontal pass, 4 pixels per item
    float* G = ring + START * MP;               // plane c at + c * RING * MP: CH * TW floats each
    for (int idx = tid; idx < 5 * CH * (TW / 4); idx += NT) {
        const int g4 = idx % (TW / 4), row = (idx / (TW / 4)) % CH, c = idx / (CH * (TW / 4));
        const float4* vp = (const float4*)(V + c * CH * VP + row * VP + 4 * g4);
        float v[4 * NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            float4 t = vp[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
        float o[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float s = v[M_ + p] * a.win.k[0];
#pragma unroll
            for (int i = 1; i <= M_; i++) s += a.win.k[i] * (v[M_ + p - i] + v[M_ + p + i]);
            o[p] = s;
        }
        *(float4*)(G + c * RING * MP + row * TW + 4 * g4) = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    // ---- c2: solve
    for (int px = tid; px < CH * TW; px += NT) {
        const int row = px / TW, lx = px - row * TW;
        const int gx = tx0 + lx, gy = Y + row;
        double g[5];
#pragma unroll
        for (int c = 0; c < 5; c++) g[c] = G[c * RING * MP + px];
        if (gx < a.w && gy < yend) *(float2*)(fout + (size_t)gy * a.fout_step + (size_t)gx * 8) = rc_solve(g);
    }
    __syncthreads();
}

template <int M_, int NT, int BATCH>
__global__ __launch_bounds__(NT) void k_flow_iter_sweep(RcIterArgs a) {
    using S = RcSweep<M_>;
    constexpr int CH = S::CH, MW = S::MW, MP = S::MP, RING = S::RING, TW = S::TW;
    extern __shared__ __align__(16) float smf[];
    float* ring = smf;                          // [5][RING][MP]
    float* V = smf + 5 * RING * MP;             // [5][CH][VP]
    const int tid = threadIdx.x;
    const int z = blockIdx.y;
    const int strip = blockIdx.x % a.tiles_x, seg = blockIdx.x / a.tiles_x;
    const int tx0 = strip * TW, y0 = seg * a.th;
    const int w = a.w, h = a.h;
    const int yend = min(y0 + a.th, h);
    const size_t s0 = (size_t)((a.slot0 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const size_t s1 = (size_t)((a.slot1 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const float4* RA0 = a.RA + s0;  const float* RB0 = a.RB + s0;
    const float4* RA1 = a.RA + s1;  const float* RB1 = a.RB + s1;
    const float2* fin = a.fin ? a.fin + (size_t)z * a.fin_pair_stride : nullptr;
    char* fout = a.fout + (size_t)z * a.fout_pair_stride;

    // ---- a: matrices of image rows r0 .. r0 + nrows - 1 (replicated outside the image) -> ring
    auto matrices_rows = [&](int r0, int nrows) {
        const int n = nrows * MW;
        for (int base = tid; base < n; base += NT * BATCH) {
            float2 d[BATCH];
            int gxs[BATCH], gys[BATCH];
#pragma unroll
            for (int q = 0; q < BATCH; q++) {
                const int idx = min(base + q * NT, n - 1);
                const int j = idx / MW, lx = idx - j * MW;
                gxs[q] = rc_clampi(tx0 - M_ + lx, 0, w - 1);
                gys[q] = rc_clampi(r0 + j, 0, h - 1);
                d[q] = rc_flow_in(a, fin, gxs[q], gys[q]);
            }
            RcM5 v[BATCH];
#pragma unroll
            for (int q = 0; q < BATCH; q++)
                v[q] = rc_matrices(RA0, RB0, RA1, RB1, gxs[q], gys[q], w, h, d[q].x, d[q].y);
#pragma unroll
            for (int q = 0; q < BATCH; q++) {
                const int idx = base + q * NT;
                if (idx < n) {
                    const int j = idx / MW, lx = idx - j * MW;
                    const int slot = (r0 + j - (y0 - M_)) % RING;
                    float* mp = ring + slot * MP + lx;
                    mp[0] = v[q].m0;
                    mp[RING * MP] = v[q].m1;
                    mp[2 * RING * MP] = v[q].m2;
                    mp[3 * RING * MP] = v[q].m3;
                    mp[4 * RING * MP] = v[q].m4;
                }
            }
        }
    };
    matrices_rows(y0 - M_, 2 * M_);
    const int nsteps = (yend - y0 + CH - 1) / CH;
    for (int s = 0; s < nsteps; s++) {
        matrices_rows(y0 + M_ + CH * s, CH);
        __syncthreads();
        const int Y = y0 + CH * s;
        switch (s % (RING / CH)) {
            case 0: rc_sweep_bc<M_, NT, 0>(a, ring, V, tid, tx0, Y, yend, fout); break;
            case 1: rc_sweep_bc<M_, NT, CH>(a, ring, V, tid, tx0, Y, yend, fout); break;
            case 2: rc_sweep_bc<M_, NT, 2 * CH>(a, ring, V, tid, tx0, Y, yend, fout); break;
            default: if constexpr (RING / CH > 3) rc_sweep_bc<M_, NT, 3 * CH>(a, ring, V, tid, tx0, Y, yend, fout); break;
        }
    }
}

template <int M, int NT, int BATCH>
static void launch_iter_sweep(RcIterArgs a, const RcFlowForm& f, int pairs, hipStream_t s) {
    using S = RcSweep<M>;
    static_assert(S::RING / S::CH <= 4, "step dispatch covers four ring phases");
    static_assert(S::TW == RC_SWEEP_TW && S::CH == RC_SWEEP_CH && NT == RC_SWEEP_NT, "rc_flow_form reports this kernel's strip, step and block");
    RC_ALLOW_LDS((k_flow_iter_sweep<M, NT, BATCH>), S::LDS);
    rc_form_grid(a, f);       // (th = rows per segment: rc_sweep_segment_rows)
    hipLaunchKernelGGL((k_flow_iter_sweep<M, NT, BATCH>), dim3(a.tiles_x * a.tiles_y, pairs, 1), dim3(NT), S::LDS, s, a);
}

// ------------------------------------------------------------------------------------
// The 3x3-window kernel (winsize 3: ripcurrents.cpp:215, main.cpp:264): 64x16 tile,
// 512 threads.  Latency is what bounds this stage, so the memory phases are explicit: every
// thread first has the flow of its (at most three) tile+halo pixels in flight, then all
// their polynomial gathers (8 x 16 B + 8 x 4 B + ... per pixel), and only then computes.
// IN_MODE is a template parameter so that no control flow separates the loads.
#define RC_W3_THREADS 512
template <int IN_MODE, int GAUSS_>
__global__ __launch_bounds__(RC_W3_THREADS) void k_flow_iter_w3(RcIterArgs a) {
    constexpr int TW = RC_W3_TW, TH = RC_W3_TH, MW = TW + 2, MH = TH + 2, MP = MW | 1;
    constexpr int NITEMS = MW * MH, NIT = (NITEMS + RC_W3_THREADS - 1) / RC_W3_THREADS;
    extern __shared__ __align__(16) float smf[];
    float* Ms = smf;                    // [5][MH][MP]
    const int tid = threadIdx.x;
    const int z = blockIdx.y;
    const int t = a.xcd_remap ? rc_xcd_remap(blockIdx.x, a.tiles_x * a.tiles_y) : (int)blockIdx.x;
    const int tx0 = (t % a.tiles_x) * TW, ty0 = (t / a.tiles_x) * TH;
    const int w = a.w, h = a.h;
    const size_t s0 = (size_t)((a.slot0 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const size_t s1 = (size_t)((a.slot1 + z * a.zstep) % a.nslots) * a.R_slot_stride;
    const float4* __restrict__ RA0 = a.RA + s0;  const float* __restrict__ RB0 = a.RB + s0;
    const float4* __restrict__ RA1 = a.RA + s1;  const float* __restrict__ RB1 = a.RB + s1;
    const float2* __restrict__ fin = a.fin + (size_t)z * a.fin_pair_stride;
    char* fout = a.fout + (size_t)z * a.fout_pair_stride;

    int gx[NIT], gy[NIT];
#pragma unroll
    for (int q = 0; q < NIT; q++) {
        int idx = min(tid + q * RC_W3_THREADS, NITEMS - 1);
        int ly = idx / MW, lx = idx - ly * MW;
        gx[q] = rc_clampi(tx0 - 1 + lx, 0, w - 1);
        gy[q] = rc_clampi(ty0 - 1 + ly, 0, h - 1);
    }
    // ---- flow_in: all loads, then the arithmetic
    float dx[NIT], dy[NIT];
    if constexpr (IN_MODE == 0) {
#pragma unroll
        for (int q = 0; q < NIT; q++) dx[q] = dy[q] = 0.f;
    } else if constexpr (IN_MODE == 1) {
        float2 d[NIT];
#pragma unroll
        for (int q = 0; q < NIT; q++) d[q] = fin[(size_t)gy[q] * w + gx[q]];
#pragma unroll
        for (int q = 0; q < NIT; q++) { dx[q] = d[q].x; dy[q] = d[q].y; }
    } else {
        float2 p00[NIT], p01[NIT], p10[NIT], p11[NIT];
        float ax[NIT], ay[NIT];
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            int sx = rc_src_x(gx[q], a.up_scale_x, a.fin_w, ax[q]);
            int sx1 = min(sx + 1, a.fin_w - 1);
            int sy = rc_src_y(gy[q], a.up_scale_y, ay[q]);
            int sy0 = rc_clampi(sy, 0, a.fin_h - 1), sy1 = rc_clampi(sy + 1, 0, a.fin_h - 1);
            const float2* S0 = fin + (size_t)sy0 * a.fin_w;
            const float2* S1 = fin + (size_t)sy1 * a.fin_w;
            p00[q] = S0[sx]; p01[q] = S0[sx1]; p10[q] = S1[sx]; p11[q] = S1[sx1];
        }
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            float a0 = 1.f - ax[q], a1 = ax[q], b0 = 1.f - ay[q], b1 = ay[q];
            float r0x = p00[q].x * a0 + p01[q].x * a1, r1x = p10[q].x * a0 + p11[q].x * a1;
            float r0y = p00[q].y * a0 + p01[q].y * a1, r1y = p10[q].y * a0 + p11[q].y * a1;
            dx[q] = (r0x * b0 + r1x * b1) * a.up_mul;
            dy[q] = (r0y * b0 + r1y * b1) * a.up_mul;
        }
    }
    // ---- polynomial coefficients: all gathers in flight
    float4 A0[NIT];
    float B0[NIT];
    RcGather gt[NIT];
#pragma unroll
    for (int q = 0; q < NIT; q++) {
        size_t p0 = (size_t)gy[q] * w + gx[q];
        A0[q] = RA0[p0];
        B0[q] = RB0[p0];
        rc_gather_issue(gt[q], RA1, RB1, gx[q], gy[q], dx[q], dy[q], w, h);
    }
    // ---- FarnebackUpdateMatrices
#pragma unroll
    for (int q = 0; q < NIT; q++) {
        RcM5 v = rc_matrices_reg(A0[q], B0[q], gt[q], dx[q], dy[q], gx[q], gy[q], w, h);
        int idx = tid + q * RC_W3_THREADS;
        if (idx < NITEMS) {
            int ly = idx / MW, lx = idx - ly * MW;
            float* mp = Ms + ly * MP + lx;
            mp[0] = v.m0;
            mp[MH * MP] = v.m1;
            mp[2 * MH * MP] = v.m2;
            mp[3 * MH * MP] = v.m3;
            mp[4 * MH * MP] = v.m4;
        }
    }
    __syncthreads();

    // ---- 3x3 window + solve: lane = column, RPT rows per thread
    constexpr int RPT = TH / (RC_W3_THREADS / TW);
    const int lx = tid % TW, r0 = (tid / TW) * RPT;
    const int ox = tx0 + lx;
    float g[RPT][5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const float* mc = Ms + c * MH * MP + r0 * MP + lx;
        float col[3][RPT + 2];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int r = 0; r < RPT + 2; r++) col[j][r] = mc[r * MP + j];
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            float v[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (GAUSS_) v[j] = col[j][r + 1] * a.win.k[0] + (col[j][r + 2] + col[j][r]) * a.win.k[1];
                else v[j] = col[j][r + 1] + (col[j][r + 2] + col[j][r]);
            }
            if (GAUSS_) g[r][c] = v[1] * a.win.k[0] + a.win.k[1] * (v[0] + v[2]);
            else g[r][c] = (v[1] + v[0]) + v[2];
        }
    }
    if (ox < w) {
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            int oy = ty0 + r0 + r;
            if (oy < h)
                *(float2*)(fout + (size_t)oy * a.fout_step + (size_t)ox * 8) =
                    rc_solve3(g[r], GAUSS_ ? 1e-3f : (float)a.win.box_eps);
        }
    }
}

template <int IN_MODE, int G>
static void launch_w3(RcIterArgs a, const RcFlowForm& f, int pairs, hipStream_t s) {
    rc_form_grid(a, f);
    size_t lds = sizeof(float) * 5 * 18 * 67;
    hipLaunchKernelGGL((k_flow_iter_w3<IN_MODE, G>), dim3(a.tiles_x * a.tiles_y, pairs, 1), dim3(RC_W3_THREADS), lds, s, a);
}

// Bilinear gather of the 5 coefficients of R1 at p + flow: from the block's LDS window when
// the 2x2 footprint lies inside it (|flow| < D), else from global memory.
template <int WW, int WH, int WP = WW>
__device__ __forceinline__ void rc_gather_window(RcGather& g, const float4* LA, const float* LB, int ox, int oy,
                                                 const float4* __restrict__ RA1, const float* __restrict__ RB1,
                                                 int gx, int gy, float dx, float dy, int w, int h) {
    float fx = gx + dx, fy = gy + dy;
    int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
    g.fx = fx - x1;
    g.fy = fy - y1;
    g.inside = (unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1);
    const int wx = x1 - ox, wy = y1 - oy;
    if (g.inside && (unsigned)wx < (unsigned)(WW - 1) && (unsigned)wy < (unsigned)(WH - 1)) {
        const int i = wy * WP + wx;
        g.q00 = LA[i]; g.q01 = LA[i + 1]; g.q10 = LA[i + WP]; g.q11 = LA[i + WP + 1];
        g.e00 = LB[i]; g.e01 = LB[i + 1]; g.e10 = LB[i + WP]; g.e11 = LB[i + WP + 1];
    } else {
        const size_t p = g.inside ? (size_t)y1 * w + x1 : (size_t)gy * w + gx;
        const size_t pw = g.inside ? (size_t)w : 0, p1 = g.inside ? 1 : 0;
        g.q00 = RA1[p]; g.q01 = RA1[p + p1]; g.q10 = RA1[p + pw]; g.q11 = RA1[p + pw + p1];
        g.e00 = RB1[p]; g.e01 = RB1[p + p1]; g.e10 = RB1[p + pw]; g.e11 = RB1[p + pw + p1];
    }
}

// ===================================================================== two iterations in one launch (3x3 window)
// Both iterations of a scale read the same R0 and R1, and iteration 2 needs iteration 1's flow only at the pixel
// itself, so a block runs   M0 (tile + 2 halo) -> flow1 (tile + 1 halo) -> M1 -> flow2 (tile)   entirely on chip:
// flow1 never exists in memory and R1's second gather (at p + flow1) reads the LDS window the first one used.
// The M grid of a block is 32 columns wide = half a wave, a thread owns NIT vertically adjacent positions of one
// column for ALL stages, and M0 / M1 stay in registers.  The 3x3 window is separable: the vertical 3-sum needs only
// the rows just above and below the thread's own run (exchanged through a small LDS buffer, two rows per group), the
// horizontal 3-sum takes its neighbours from the adjacent lanes with DPP wave shifts (v_add_f32_dpp), so the five M
// planes never go through LDS or HBM.  Arithmetic is operation for operation that of two launches of k_flow_iter_w3
// (bit-identical results).
//   tile = 28 x (8 NIT - 4) outputs, M grid 32 x 8 NIT (halo 2), R1 window = grid +- D in LDS.
// g[c] = (V[c] + V[c] of lane - 1) + V[c] of lane + 1 for the five planes, as ten v_add_f32_dpp
// (the compiler's DPP combiner folds only some of the equivalent builtin calls).  s_nop 1 covers
// the two wait states a DPP read needs after a VALU write of its source.
__device__ __forceinline__ void rc_hsum3_dpp(float (&g)[5], const float (&V)[5]) {
    // ONE asm statement: the compiler cannot place a copy or a reload of V between the two DPP groups,
    // so the only VALU write a DPP read can follow too closely is the one before the statement (s_nop 1),
    // and the second group reads V again five instructions after the first (its t operands are plain reads).
    float t0, t1, t2, t3, t4;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %5, %10, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %6, %11, %11 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %7, %12, %12 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %8, %13, %13 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %9, %14, %14 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %0, %10, %5 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %1, %11, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %2, %12, %7 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %3, %13, %8 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %4, %14, %9 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]),
          "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4)
        : "v"(V[0]), "v"(V[1]), "v"(V[2]), "v"(V[3]), "v"(V[4]));
}


// s[c] = V[c] of lane - 1  +  V[c] of lane + 1   (one asm statement, see rc_hsum3_dpp)
__device__ __forceinline__ void rc_hpair_dpp(float (&s)[5], const float (&V)[5]) {
    float t0, t1, t2, t3, t4;
    asm("s_nop 1\n\t"
        "v_mov_b32_dpp %5, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_mov_b32_dpp %6, %11 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_mov_b32_dpp %7, %12 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_mov_b32_dpp %8, %13 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_mov_b32_dpp %9, %14 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %0, %10, %5 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %1, %11, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %2, %12, %7 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %3, %13, %8 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %4, %14, %9 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3]), "=&v"(s[4]),
          "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4)
        : "v"(V[0]), "v"(V[1]), "v"(V[2]), "v"(V[3]), "v"(V[4]));
}

template <int GAUSS_, int NIT, int MW, int NG>
__device__ __forceinline__ void rc_rr_flows(const float (&m)[NIT][5], const float* XR, int grp, int x,
                                            const RcWindow& win, float2 (&f)[NIT]) {
    const int gu = max(grp - 1, 0), gd = min(grp + 1, NG - 1);
    // XR[group][first / last][channel][MW]: group stride 10 MW by a 24-bit multiply (a 32-bit one runs at quarter rate)
    const int bu = (int)__umul24((unsigned)gu, 10u * MW) + x, bd = (int)__umul24((unsigned)gd, 10u * MW) + x;
    float up[5], dn[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        up[c] = XR[bu + (5 + c) * MW];
        dn[c] = XR[bd + c * MW];
    }
    float V[NIT][5];
#pragma unroll
    for (int q = 0; q < NIT; q++)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            float u = q > 0 ? m[q - 1][c] : up[c], d = q < NIT - 1 ? m[q + 1][c] : dn[c];
            if (GAUSS_) V[q][c] = m[q][c] * win.k[0] + (d + u) * win.k[1];
            else V[q][c] = m[q][c] + (d + u);
        }
#pragma unroll
    for (int q = 0; q < NIT; q++) {
        float g[5];
        if (GAUSS_) {
            float lr[5];
            rc_hpair_dpp(lr, V[q]);
#pragma unroll
            for (int c = 0; c < 5; c++) g[c] = V[q][c] * win.k[0] + win.k[1] * lr[c];
        } else {
            rc_hsum3_dpp(g, V[q]);
        }
        f[q] = rc_solve3(g, GAUSS_ ? 1e-3f : (float)win.box_eps);
    }
}

template <int NIT, int MW>
__device__ __forceinline__ void rc_rr_exchange(const float (&m)[NIT][5], float* XR, int grp, int x) {
    const int b = (int)__umul24((unsigned)grp, 10u * MW) + x;
#pragma unroll
    for (int c = 0; c < 5; c++) {
        XR[b + c * MW] = m[0][c];
        XR[b + (5 + c) * MW] = m[NIT - 1][c];
    }
}

// flow_in of a thread's NIT grid positions (column gxo, rows gys[]): zeros at the coarsest scale, the previous
// iteration's field, or resize(prevFlow, INTER_LINEAR) * (1 / pyr_scale) of the coarser scale (optflow.cpp calc()).
// Shared by the register-row kernels, so they all see the same bits.
// INTERIOR (k_flow_iter2_rrc: the block's M grid lies at least 5 px inside the image): no coordinate of the block
// is clamped and offsets are 32-bit -- the same loads and the same arithmetic with fewer address instructions.
template <int IN_MODE, int NIT, int MW, int MH, bool INTERIOR = false>
__device__ __forceinline__ void rc_rr_flow_in(const RcIterArgs& a, const float2* __restrict__ fin, int tx0, int ty0,
                                              int gxo, const int (&gys)[NIT], float (&dx)[NIT], float (&dy)[NIT]) {
    const int w = a.w, h = a.h;
    if constexpr (IN_MODE == 0) {
#pragma unroll
        for (int q = 0; q < NIT; q++) dx[q] = dy[q] = 0.f;
    } else if constexpr (IN_MODE == 1) {
        float2 d[NIT];
#pragma unroll
        for (int q = 0; q < NIT; q++) d[q] = INTERIOR ? fin[(unsigned)(gys[q] * w + gxo)] : fin[(size_t)gys[q] * w + gxo];
#pragma unroll
        for (int q = 0; q < NIT; q++) { dx[q] = d[q].x; dy[q] = d[q].y; }
    } else if ((NIT % 2 == 0) && a.up_exact2 && (INTERIOR || (ty0 - 2 >= 0 && ty0 - 2 + MH <= h))) {
        // Exactly half-size coarse scale, no row of the block clamped: the thread's first row is even, so
        // its NIT rows read coarse rows rb .. rb + NIT/2 + 1 with rb = row/2 - 1 (row q: rb + (q+1)/2 and the
        // next, fraction 0.75 / 0.25 for even / odd q).  Each coarse row is loaded and interpolated
        // horizontally once instead of once per output row: NIT + 4 loads instead of 4 NIT, same values.
        constexpr int NR = NIT / 2 + 2;
        int sx = (gxo - 1) >> 1;
        float ax = (gxo & 1) ? 0.25f : 0.75f;
        if (!INTERIOR) {
            if (sx < 0) { ax = 0.f; sx = 0; }
            if (sx >= a.fin_w - 1) { ax = 0.f; sx = a.fin_w - 1; }
        }
        const int sx1 = min(sx + 1, a.fin_w - 1);
        const int rb = (gys[0] - 1) >> 1;
        float2 t0[NR], t1[NR];
        // no column of the block clamped either: texels sx and sx + 1 are one 16-byte load (8-byte aligned)
        typedef float rc_f4a8 __attribute__((ext_vector_type(4), aligned(8)));
        const bool cols_plain = INTERIOR || (tx0 - 2 >= 1 && tx0 - 2 + MW <= w && ((tx0 - 2 + MW - 2) >> 1) + 1 <= a.fin_w - 1);
        if (INTERIOR) {
            // (an interior block's coarse rows rb .. rb + NR - 1 and columns sx, sx + 1 all exist)
            unsigned co = (unsigned)(__mul24(rb, a.fin_w) + sx);
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const rc_f4a8 v = *(const rc_f4a8*)(fin + co);
                t0[j] = make_float2(v.x, v.y); t1[j] = make_float2(v.z, v.w);
                co += (unsigned)a.fin_w;
            }
        } else if (cols_plain) {
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const float2* S = fin + (size_t)rc_clampi(rb + j, 0, a.fin_h - 1) * a.fin_w;
                const rc_f4a8 v = *(const rc_f4a8*)(S + sx);
                t0[j] = make_float2(v.x, v.y); t1[j] = make_float2(v.z, v.w);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const float2* S = fin + (size_t)rc_clampi(rb + j, 0, a.fin_h - 1) * a.fin_w;
                t0[j] = S[sx]; t1[j] = S[sx1];
            }
        }
        const float a0 = 1.f - ax, a1 = ax;
        float hx[NR], hy[NR];
#pragma unroll
        for (int j = 0; j < NR; j++) {
            hx[j] = t0[j].x * a0 + t1[j].x * a1;
            hy[j] = t0[j].y * a0 + t1[j].y * a1;
        }
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const int j0 = (q + 1) >> 1;
            const float b1 = (q & 1) ? 0.25f : 0.75f, b0 = 1.f - b1;
            dx[q] = (hx[j0] * b0 + hx[j0 + 1] * b1) * a.up_mul;
            dy[q] = (hy[j0] * b0 + hy[j0 + 1] * b1) * a.up_mul;
        }
    } else {
        float2 p00[NIT], p01[NIT], p10[NIT], p11[NIT];
        float ax, ay[NIT];
        int sx, sys[NIT];
        if (a.up_exact2) {
            // exactly half-size coarse scale: (d + 0.5) * 0.5 - 0.5 = d/2 - 0.25 in closed form
            // (floor = (d - 1) >> 1, fraction 0.75 for even d, 0.25 for odd d): same values as
            // rc_src_x / rc_src_y without the double arithmetic
            sx = (gxo - 1) >> 1;
            ax = (gxo & 1) ? 0.25f : 0.75f;
            if (sx < 0) { ax = 0.f; sx = 0; }
            if (sx >= a.fin_w - 1) { ax = 0.f; sx = a.fin_w - 1; }
#pragma unroll
            for (int q = 0; q < NIT; q++) { sys[q] = (gys[q] - 1) >> 1; ay[q] = (gys[q] & 1) ? 0.25f : 0.75f; }
        } else {
            sx = rc_src_x(gxo, a.up_scale_x, a.fin_w, ax);
#pragma unroll
            for (int q = 0; q < NIT; q++) sys[q] = rc_src_y(gys[q], a.up_scale_y, ay[q]);
        }
        const int sx1 = min(sx + 1, a.fin_w - 1);
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            int sy = sys[q];
            int sy0 = rc_clampi(sy, 0, a.fin_h - 1), sy1 = rc_clampi(sy + 1, 0, a.fin_h - 1);
            const float2* S0 = fin + (size_t)sy0 * a.fin_w;
            const float2* S1 = fin + (size_t)sy1 * a.fin_w;
            p00[q] = S0[sx]; p01[q] = S0[sx1]; p10[q] = S1[sx]; p11[q] = S1[sx1];
        }
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            float a0 = 1.f - ax, a1 = ax, b0 = 1.f - ay[q], b1 = ay[q];
            float r0x = p00[q].x * a0 + p01[q].x * a1, r1x = p10[q].x * a0 + p11[q].x * a1;
            float r0y = p00[q].y * a0 + p01[q].y * a1, r1y = p10[q].y * a0 + p11[q].y * a1;
            dx[q] = (r0x * b0 + r1x * b1) * a.up_mul;
            dy[q] = (r0y * b0 + r1y * b1) * a.up_mul;
        }
    }
}


// ---- k_flow_iter2_rrc: the register-row kernel walking a CHAIN of consecutive frame pairs on one tile.
// Pair z + 1's "previous" expansion R0 is pair z's "next" expansion R1 (the reference's u_f1.copyTo(u_f2),
// ripcurrents.cpp:194-221, at tile level): when the block has finished the gathers of pair z, each thread takes
// its NIT texels of R1 at its own grid positions out of the LDS window into the registers that held R0 -- the
// next pair then needs only its own R1 window (LDS-DMA), its coarse flow and nothing of R0 from memory:
// HBM and L2 reads per pixel drop from R0 20 + R1 20 to R1 20 (+ 20 / chain).  The window's DMA for pair z + 1
// is issued as soon as the window of pair z is dead, ahead of pair z's last window sums, solve and stores.
// The DMA goes out from inline asm and the barriers inside the loop wait for LDS traffic only (the compiler
// would otherwise drain the outstanding DMA before every LDS read); one s_waitcnt vmcnt(0) per pair, at the
// top of the loop, closes it.  A launch of independent pairs is the same kernel with chains of one.
// barrier of the compute phase: LDS traffic only
__device__ __forceinline__ void rc_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void rc_all_barrier() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr bool rc_recip_exact(int nt, int wp) {
    const unsigned r = (65536u + wp - 1) / wp;
    for (int t = 0; t < nt; t++)
        if ((int)((t * r) >> 16) != t / wp) return false;
    return true;
}

// LDS-DMA with a wave-uniform base in SGPRs, a 32-bit byte offset per lane and the wave's LDS destination as a
// plain byte address in M0 (no 64-bit address arithmetic, no generic-pointer casts).
__device__ __forceinline__ void rc_glds16_s(const void* base, unsigned voff, uint32_t lds_wave_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(lds_wave_addr) : "memory");
}
__device__ __forceinline__ void rc_glds4_s(const void* base, unsigned voff, uint32_t lds_wave_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(base), "s"(lds_wave_addr) : "memory");
}

// The R1 window of one pair: texel idx = tid + q NT of the [WH][WP] window, q = 0 .. NWL - 1.  (wy, wx) and the
// texel's image offset advance by NT = QY WP + QX per step instead of being divided out each time.
// lds_a / lds_b: LDS byte addresses of the window's float4 plane and float plane.
template <bool INTERIOR, int NT, int WP, int WN, int NWL>
__device__ __forceinline__ void rc_rrc_issue_window(const float4* __restrict__ RA1, const float* __restrict__ RB1,
                                                    uint32_t lds_a, uint32_t lds_b, int tid, int ox, int oy, int w, int h) {
    constexpr int QY = NT / WP, QX = NT % WP;
    const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);
    // tid / WP by a 24-bit multiply and shift (checked at compile time for every tid < NT), no 32-bit integer multiply
    static_assert(rc_recip_exact(NT, WP), "tid / WP by multiply and shift must be exact for every thread");
    int wy = (int)(__umul24((unsigned)tid, (65536u + WP - 1) / WP) >> 16), wx = tid - (int)__umul24((unsigned)wy, (unsigned)WP);
    int off = __mul24(oy + wy, w) + ox + wx;
#pragma unroll
    for (int q = 0; q < NWL; q++) {
        bool ok = (q + 1) * NT <= WN || tid + q * NT < WN;
        if (!INTERIOR) ok = ok && (unsigned)(ox + wx) < (unsigned)w && (unsigned)(oy + wy) < (unsigned)h;
        const unsigned p = ok ? (unsigned)off : 0u;     // out-of-image texels are never read
        if (q * NT + wave_base < WN) {
            rc_glds16_s(RA1, p << 4, lds_a + (uint32_t)(q * NT + wave_base) * 16u);
            rc_glds4_s(RB1, p << 2, lds_b + (uint32_t)(q * NT + wave_base) * 4u);
        }
        wx += QX; wy += QY; off += QY * w + QX;
        if (wx >= WP) { wx -= WP; wy += 1; off += w - WP; }
    }
}

// FarnebackUpdateMatrices at a thread's NIT grid positions.  Interior blocks (the whole M grid at least 5 px
// inside the image: no border factors, no clamped coordinates, and a sample inside the window is inside the
// image) take a straight-line path: every lane gathers from the LDS window at an index clamped into it, and a
// lane whose displacement leaves the window (|flow| >= D, rare) is redone from global memory afterwards.  The
// values are those of rc_gather_window + rc_matrices_reg, which border blocks keep using: same bits.
template <bool INTERIOR, int NIT, int WW, int WH, int WP>
__device__ __forceinline__ void rc_rr_matrices(float (&m)[NIT][5], const float4 (&A0)[NIT], const float (&B0)[NIT],
                                               const float (&dx)[NIT], const float (&dy)[NIT], const float4* LA,
                                               const float* LB, int ox, int oy, const float4* __restrict__ RA1,
                                               const float* __restrict__ RB1, int gxo, const int (&gys)[NIT], int w, int h) {
    if constexpr (!INTERIOR) {
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            RcGather g;
            rc_gather_window<WW, WH, WP>(g, LA, LB, ox, oy, RA1, RB1, gxo, gys[q], dx[q], dy[q], w, h);
            RcM5 v = rc_matrices_reg(A0[q], B0[q], g, dx[q], dy[q], gxo, gys[q], w, h, true);
            m[q][0] = v.m0; m[q][1] = v.m1; m[q][2] = v.m2; m[q][3] = v.m3; m[q][4] = v.m4;
        }
    } else {
        unsigned far = 0;
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            RcGather g;
            const float fx = gxo + dx[q], fy = gys[q] + dy[q];
            // (float)(int)floorf(v) == floorf(v) for every coordinate an image can have: the fraction is taken against
            // the floor itself (one conversion less per coordinate), the index is a 24-bit multiply-add (full rate; a
            // 32-bit integer multiply runs at a quarter of it)
            const float flx = floorf(fx), fly = floorf(fy);
            const int x1 = (int)flx, y1 = (int)fly;
            g.fx = fx - flx;
            g.fy = fy - fly;
            g.inside = true;
            const int wx = x1 - ox, wy = y1 - oy;
            const bool in_win = (unsigned)wx < (unsigned)(WW - 1) && (unsigned)wy < (unsigned)(WH - 1);
            far |= in_win ? 0u : 1u << q;
            const unsigned i = in_win ? __umul24((unsigned)wy, (unsigned)WP) + (unsigned)wx : 0u;
            const float4* pa = (const float4*)((const char*)LA + (i << 4));      // (two shifts: the compiler otherwise derives the
            const float* pb = (const float*)((const char*)LB + (i << 2));        //  float plane's address by a 64-bit multiply-add)
            g.q00 = pa[0]; g.q01 = pa[1]; g.q10 = pa[WP]; g.q11 = pa[WP + 1];
            g.e00 = pb[0]; g.e01 = pb[1]; g.e10 = pb[WP]; g.e11 = pb[WP + 1];
            RcM5 v = rc_matrices_reg(A0[q], B0[q], g, dx[q], dy[q], gxo, gys[q], w, h, false);
            m[q][0] = v.m0; m[q][1] = v.m1; m[q][2] = v.m2; m[q][3] = v.m3; m[q][4] = v.m4;
        }
        if (__builtin_expect(far != 0, 0)) {
#pragma unroll
            for (int q = 0; q < NIT; q++) {
                if (far >> q & 1) {
                    RcGather g;
                    rc_gather_issue(g, RA1, RB1, gxo, gys[q], dx[q], dy[q], w, h);
                    RcM5 v = rc_matrices_reg(A0[q], B0[q], g, dx[q], dy[q], gxo, gys[q], w, h, false);
                    m[q][0] = v.m0; m[q][1] = v.m1; m[q][2] = v.m2; m[q][3] = v.m3; m[q][4] = v.m4;
                }
            }
        }
    }
}

template <bool INTERIOR, int IN_MODE, int GAUSS_, int NIT, int D, int MW, int NG>
__device__ __forceinline__ void rc_rrc_body(const RcIterArgs& a, const int zb, const int ze, float* smf, const uint32_t lds0, const int tx0, const int ty0) {
    constexpr int NT = NG * MW, MH = NG * NIT;
    constexpr int WW = MW + 2 * D, WH = MH + 2 * D, WP = WW, WN = WP * WH, NWL = (WN + NT - 1) / NT;
    constexpr int WNP = (WN + 63) & ~63;
    constexpr int MP = MW + 1, PLANE = MH * MP;
    static_assert(5 * PLANE <= 5 * WNP, "border-block M1 planes alias the R1 window");
    float4* LA = (float4*)smf;              // [WH][WW]  R1 (y, x, yy, xx)
    float* LB = smf + 4 * WNP;              // [WH][WW]  R1 xy
    float* XR = LB + WNP;                   // [NG][2][5][MW] first / last row of every group
    float* Ms = smf;                        // border blocks only: [5][MH][MP], after the window is dead
    const uint32_t lds_a = lds0, lds_b = lds0 + 16u * WNP;     // LDS byte addresses of LA and LB
    const int w = a.w, h = a.h;
    const int ox = tx0 - 2 - D, oy = ty0 - 2 - D;
    // Everything a thread derives from its index (grid position, clamped coordinates, DMA / coarse-flow / store
    // addresses) is re-derived per pair from an index the compiler cannot see through: hoisted out of the loop
    // these invariants cost ~60 registers and spill, recomputed they cost a few instructions.
#define RC_RRC_COORDS(tid_)                                                         \
    const int x = (tid_) & (MW - 1), grp = (tid_) / MW, ly0 = grp * NIT;            \
    const int px = tx0 - 2 + x;                                                     \
    const int gxo = INTERIOR ? px : rc_clampi(px, 0, w - 1);                        \
    int gys[NIT];                                                                   \
    _Pragma("unroll") for (int q = 0; q < NIT; q++)                                 \
        gys[q] = INTERIOR ? ty0 - 2 + ly0 + q : rc_clampi(ty0 - 2 + ly0 + q, 0, h - 1);

    // ---- head of the chain: the window of pair zb, R0 from memory, flow_in of pair zb
    float4 A0[NIT];
    float B0[NIT];
    float dx[NIT], dy[NIT];
    {
        const int tid = threadIdx.x;
        RC_RRC_COORDS(tid)
        const size_t s0 = (size_t)((a.slot0 + zb * a.zstep) % a.nslots) * a.R_slot_stride;
        const size_t s1 = (size_t)((a.slot1 + zb * a.zstep) % a.nslots) * a.R_slot_stride;
        rc_rrc_issue_window<INTERIOR, NT, WP, WN, NWL>(a.RA + s1, a.RB + s1, lds_a, lds_b, tid, ox, oy, w, h);
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const unsigned p0 = (unsigned)(gys[q] * w + gxo);
            A0[q] = (a.RA + s0)[p0];
            B0[q] = (a.RB + s0)[p0];
        }
        rc_rr_flow_in<IN_MODE, NIT, MW, MH, INTERIOR>(a, a.fin + (size_t)zb * a.fin_pair_stride, tx0, ty0, gxo, gys, dx, dy);
    }

    for (int z = zb; z < ze; z++) {
        const size_t s1 = (size_t)((a.slot1 + z * a.zstep) % a.nslots) * a.R_slot_stride;
        const float4* __restrict__ RA1 = a.RA + s1;
        const float* __restrict__ RB1 = a.RB + s1;
        const bool more = z + 1 < ze;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        RC_RRC_COORDS(tid)
        rc_all_barrier();     // this pair's window has landed (and the previous pair's exchange rows are dead)

        // ---- M0 on the whole grid, in registers
        float m[NIT][5];
        rc_rr_matrices<INTERIOR, NIT, WW, WH, WP>(m, A0, B0, dx, dy, LA, LB, ox, oy, RA1, RB1, gxo, gys, w, h);
        rc_rr_exchange<NIT, MW>(m, XR, grp, x);
        rc_lds_barrier();

        // ---- flow1, then M1 in place of M0
        {
            float2 f1[NIT];
            rc_rr_flows<GAUSS_, NIT, MW, NG>(m, XR, grp, x, a.win, f1);
            float f1x[NIT], f1y[NIT];
#pragma unroll
            for (int q = 0; q < NIT; q++) { f1x[q] = f1[q].x; f1y[q] = f1[q].y; }
            rc_rr_matrices<INTERIOR, NIT, WW, WH, WP>(m, A0, B0, f1x, f1y, LA, LB, ox, oy, RA1, RB1, gxo, gys, w, h);
        }
        // ---- the hand-over: this pair's R1 at the thread's own (clamped) grid positions is the next pair's R0
        if (more) {
#pragma unroll
            for (int q = 0; q < NIT; q++) {
                const int i = (int)__umul24((unsigned)(gys[q] - oy), (unsigned)WP) + (gxo - ox);
                A0[q] = LA[i];
                B0[q] = LB[i];
            }
        }
        rc_lds_barrier();     // the exchange rows and the R1 window have been read by everyone
        if constexpr (!INTERIOR) {
            // A grid position outside the image stands for the border pixel it replicates (the window's
            // replicate border): take that pixel's M1
#pragma unroll
            for (int q = 0; q < NIT; q++)
#pragma unroll
                for (int c = 0; c < 5; c++) Ms[c * PLANE + (ly0 + q) * MP + x] = m[q][c];
            rc_lds_barrier();
#pragma unroll
            for (int q = 0; q < NIT; q++) {
                const int py = ty0 - 2 + ly0 + q;
                if ((unsigned)px >= (unsigned)w || (unsigned)py >= (unsigned)h) {
                    const int cx = gxo - (tx0 - 2), cy = gys[q] - (ty0 - 2);
#pragma unroll
                    for (int c = 0; c < 5; c++) m[q][c] = Ms[c * PLANE + cy * MP + cx];
                }
            }
        }
        rc_rr_exchange<NIT, MW>(m, XR, grp, x);
        rc_lds_barrier();     // (border blocks: the aliased M1 planes have been read by everyone too)

        // ---- the next pair's window is requested before this pair's last window sums, solve and stores
        if (more) {
            const size_t n1 = (size_t)((a.slot1 + (z + 1) * a.zstep) % a.nslots) * a.R_slot_stride;
            rc_rrc_issue_window<INTERIOR, NT, WP, WN, NWL>(a.RA + n1, a.RB + n1, lds_a, lds_b, tid, ox, oy, w, h);
        }

        // ---- flow2 on the tile
        {
            char* fout = a.fout + (size_t)z * a.fout_pair_stride;
            float2 f2[NIT];
            rc_rr_flows<GAUSS_, NIT, MW, NG>(m, XR, grp, x, a.win, f2);
            if (x >= 2 && x < MW - 2 && (INTERIOR || px < w)) {
                // (a.addr32: 32-bit offsets; one multiply for the thread's first row, the others follow by addition)
                unsigned so = (unsigned)(ty0 - 2 + ly0) * (unsigned)a.fout_step + (unsigned)px * 8u;
#pragma unroll
                for (int q = 0; q < NIT; q++) {
                    const int ly = ly0 + q, py = ty0 - 2 + ly;
                    if (ly >= 2 && ly < MH - 2 && (INTERIOR || py < h)) *(float2*)(fout + so) = f2[q];
                    so += (unsigned)a.fout_step;
                }
            }
        }
        if (more) rc_rr_flow_in<IN_MODE, NIT, MW, MH, INTERIOR>(a, a.fin + (size_t)(z + 1) * a.fin_pair_stride, tx0, ty0, gxo, gys, dx, dy);
    }
#undef RC_RRC_COORDS
}

template <int IN_MODE, int GAUSS_, int NIT, int D, int MINB, int MW, int NG>
__global__ __launch_bounds__(NG * MW, MINB) void k_flow_iter2_rrc(RcIterArgs a, RcChainPlan cp) {
    constexpr int MH = NG * NIT, TW = MW - 4, TH = MH - 4;
    extern __shared__ __align__(16) float smf[];
    // (ngroups == 0: independent pairs, one per block row)
    const int zb = cp.ngroups ? cp.start[blockIdx.y] : (int)blockIdx.y, ze = cp.ngroups ? cp.start[blockIdx.y + 1] : zb + 1;
    const int t = a.xcd_remap ? rc_xcd_remap(blockIdx.x, a.tiles_x * a.tiles_y) : (int)blockIdx.x;
    const int tx0 = (t % a.tiles_x) * TW, ty0 = (t / a.tiles_x) * TH;
    const bool interior = tx0 - 2 >= 5 && tx0 - 2 + MW <= a.w - 5 && ty0 - 2 >= 5 && ty0 - 2 + MH <= a.h - 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smf;
    if (interior) rc_rrc_body<true, IN_MODE, GAUSS_, NIT, D, MW, NG>(a, zb, ze, smf, lds0, tx0, ty0);
    else rc_rrc_body<false, IN_MODE, GAUSS_, NIT, D, MW, NG>(a, zb, ze, smf, lds0, tx0, ty0);
}

template <int IN_MODE, int G, int NIT, int D, int MINB, int MW = 32, int NG = 8>
static void launch_rrc_t(RcIterArgs a, const RcFlowForm& f, const RcChainPlan& cp, int pairs, hipStream_t s) {
    constexpr int MH = NG * NIT, TW = MW - 4, TH = MH - 4;
    static_assert(TW == RC_RRC_TW && TH == rc_rrc_th(NIT) && D == rc_rrc_d(NIT) && NG * MW == RC_RRC_NT, "rc_flow_form reports this kernel's tile, margin and block");
    rc_form_grid(a, f);
    constexpr int WN = (MW + 2 * D) * (MH + 2 * D), WNP = (WN + 63) & ~63;
    const size_t lds = sizeof(float) * (5 * WNP + NG * 2 * 5 * MW);
    RC_ALLOW_LDS((k_flow_iter2_rrc<IN_MODE, G, NIT, D, MINB, MW, NG>), lds);
    hipLaunchKernelGGL((k_flow_iter2_rrc<IN_MODE, G, NIT, D, MINB, MW, NG>), dim3(a.tiles_x * a.tiles_y, cp.ngroups ? cp.ngroups : pairs, 1), dim3(NG * MW), lds, s, a, cp);
}

// Chain groups of a launch of `pairs` consecutive pairs: runs of `chain` pairs, then halving runs over the last
// `chain` pairs (8, 8, 8, 4, 2, 1, 1 for 32 pairs and chain 8) so that the blocks still running when the grid
// drains are short ones -- a long-lived block in the last wave of a launch idles the rest of the GPU.  The chain
// is halved until the launch still has ~4 blocks per block slot of the GPU (1024 = 256 CUs x 4; measured: 4096).
static void rc_chain_plan(const RcIterArgs& a, int pairs, long long tiles, RcChainPlan& cp) {
    cp.ngroups = 0;
    const bool chainable = a.chain > 1 && pairs > 1 && (a.slot0 + a.zstep) % a.nslots == a.slot1 % a.nslots;
    if (!chainable) return;
    int chain = a.chain;
    if (!(a.ablate & RC_ABL_FORCE_CHAIN))
        while (chain > 1 && tiles * pairs / chain < (a.chain_min_blocks > 0 ? a.chain_min_blocks : 4096)) chain >>= 1;
    if (chain <= 1) return;
    int n = 0, z = 0;
    cp.start[0] = 0;
    while (z < pairs) {
        int left = pairs - z, c = left > chain ? chain : (left + 1) / 2;
        if (n == RC_MAX_CHAIN_GROUPS - 1) c = left;
        z += c;
        cp.start[++n] = z;
    }
    cp.ngroups = n;
}

static void rc_flow_form_plan(const RcIterArgs& a, int pairs, int fuse, RcFlowForm& f, RcChainPlan& cp);

template <int IN_MODE, int G>
static void launch_w3x2(RcIterArgs a, int pairs, hipStream_t s) {
    RcFlowForm f;
    RcChainPlan cp;
    rc_flow_form_plan(a, pairs, 2, f, cp);
    switch (f.nit) {
        case 2: launch_rrc_t<IN_MODE, G, 2, 4, 6>(a, f, cp, pairs, s); break;             // 28x12 tile, 6 blocks per CU
        case 3: launch_rrc_t<IN_MODE, G, 3, 4, 5>(a, f, cp, pairs, s); break;             // 28x20 tile, 5 blocks per CU
        default: launch_rrc_t<IN_MODE, G, 4, RC_RR_D, 4>(a, f, cp, pairs, s); break;      // 28x28 tile, 4 blocks per CU, chains of pairs
    }
}

// (the fused kernel addresses with 32-bit offsets: frames or caller strides beyond 4 GB take one launch per iteration)
int rc_flow_iter_can_fuse2(const RcIterArgs& a) { return a.win.m == 1 && a.solve && a.addr32; }

// How many of the launch's `pairs` read their previous-frame coefficients R0 from memory (the head of every tile
// chain; the others take them from the previous pair's LDS window): the compulsory bytes of the launch as built.
int rc_flow_iter2_r0_reads(const RcIterArgs& a, int pairs) {
    RcChainPlan cp;
    rc_chain_plan(a, pairs, (long long)((a.w + 27) / 28) * ((a.h + 27) / 28), cp);
    return cp.ngroups ? cp.ngroups : pairs;
}

// The chain groups a launch would use (host logic only; the CPU tier checks its invariants through
// rcflow_debug_chain_plan): returns the number of groups, 0 = independent pairs.
int rc_flow_chain_groups(const RcIterArgs& a, int pairs, int* starts, int cap) {
    RcChainPlan cp;
    rc_chain_plan(a, pairs, (long long)((a.w + 27) / 28) * ((a.h + 27) / 28), cp);
    for (int i = 0; i <= cp.ngroups && i < cap; i++) starts[i] = cp.start[i];
    return cp.ngroups;
}

static size_t iter_lds(int tw, int th, int m, bool two_buffers) {
    int MW = tw + 2 * m, MH = th + 2 * m, MP = MW | 1;
    return sizeof(float) * (5 * (size_t)MH * MP + (two_buffers ? 5 * (size_t)th * MP : 0));
}

template <int TW, int TH, int M, int G>
static void launch_iter_t(RcIterArgs a, const RcFlowForm& f, int pairs, hipStream_t s) {
    size_t lds = iter_lds(TW, TH, M, M > 1);
    static_assert(TW == rc_tile_tw(M) && TH == rc_tile_th(M), "rc_flow_form reports this kernel's tile");
    RC_ALLOW_LDS((k_flow_iter<TW, TH, M, G>), lds);
    rc_form_grid(a, f);
    hipLaunchKernelGGL((k_flow_iter<TW, TH, M, G>), dim3(a.tiles_x * a.tiles_y, pairs, 1), dim3(RC_BLOCK), lds, s, a);
}

// Runtime tile for windows without an instantiation: best halo efficiency that fits LDS.
static void pick_runtime_tile(int m, int& tw, int& th) {
    static const int tiles[][2] = {{64, 16}, {32, 32}, {64, 8}, {32, 16}, {16, 16}, {16, 8}, {8, 8}};
    double best = -1;
    tw = 8; th = 8;
    for (auto& t : tiles) {
        size_t lds = iter_lds(t[0], t[1], m, true);
        if (lds > 150 * 1024) continue;
        double eff = (double)(t[0] * t[1]) / ((t[0] + 2 * m) * (t[1] + 2 * m));
        if (lds > 64 * 1024) eff *= 0.6;
        if (t[0] < 64) eff *= 0.95;
        if (eff > best) { best = eff; tw = t[0]; th = t[1]; }
    }
}

// Rows per segment of the strip-sweep kernel: as tall as still leaves every CU a few blocks.
static int rc_sweep_segment_rows(int w, int h, int pairs) {
    const int want = 4 * 512, strips = (w + RC_SWEEP_TW - 1) / RC_SWEEP_TW;
    int segs = (want + strips * pairs - 1) / (strips * pairs);
    int rs = (h + segs - 1) / segs;
    rs = ((rs + RC_SWEEP_CH - 1) / RC_SWEEP_CH) * RC_SWEEP_CH;
    return rs < 32 ? 32 : rs;
}

// The one place that decides which kernel a launch runs and on which tile.
static void rc_flow_form_plan(const RcIterArgs& a, int pairs, int fuse, RcFlowForm& f, RcChainPlan& cp) {
    const int m = a.win.m, g = a.win.gaussian ? 1 : 0;
    memset(&f, 0, sizeof(f));
    cp.ngroups = 0;
    if (fuse == 2) {
        // A launch of fewer blocks than the GPU holds at once (1024 = 256 CUs x 4) lasts one block's lifetime:
        // shorter tiles then finish sooner (frame-at-a-time calls, coarse scales).  Same bits.
        const long long tiles = (long long)((a.w + 27) / 28) * ((a.h + 27) / 28), blocks = tiles * pairs;
        // consecutive pairs of one stream (pair z + 1's previous frame is pair z's next frame): tile chains
        rc_chain_plan(a, pairs, tiles, cp);
        f.kernel = RC_FK_RRC; f.nt = RC_RRC_NT; f.groups = cp.ngroups;
        f.nit = (cp.ngroups || blocks >= 1024) ? 4 : blocks < 512 ? 2 : 3;
        f.d = rc_rrc_d(f.nit);
        f.tw = RC_RRC_TW; f.th = rc_rrc_th(f.nit);
    } else if (m == 1 && a.solve) {
        f.kernel = RC_FK_W3; f.tw = RC_W3_TW; f.th = RC_W3_TH; f.nt = RC_W3_THREADS;
    } else if (m == 1) {
        f.kernel = RC_FK_TILE; f.tw = rc_tile_tw(m); f.th = rc_tile_th(m); f.nt = RC_BLOCK;
    } else if (a.solve && (m == 2 || m == 5 || m == 10)) {
        // 16 waves per CU: LDS 50 KB (m = 2) -> 3 blocks x 512 threads, 64 KB (m = 5) -> 2 x 1024, 142 KB (m = 10, 64 x 32 tile) -> 1 x 1024
        // Gaussian winsize 10 / 20: the strip-sweep kernel once the launch is big enough to fill the GPU
        // with strips (measured crossover, scripts/exp21.py); bit-identical to the tile kernel
        // (RC_ABL_TILE_WINDOW forces the tile kernel, RC_ABL_FORCE_SWEEP the sweep)
        const long long work = (long long)a.w * a.h * pairs;
        if (g && m != 2 && !(a.ablate & RC_ABL_TILE_WINDOW) && ((a.ablate & RC_ABL_FORCE_SWEEP) || work >= (m == 10 ? 900000ll : 8000000ll))) {
            f.kernel = RC_FK_SWEEP; f.tw = RC_SWEEP_TW; f.th = rc_sweep_segment_rows(a.w, a.h, pairs); f.nt = RC_SWEEP_NT;
        } else {
            f.kernel = RC_FK_BIG; f.tw = rc_big_tw(m); f.th = 32; f.nt = rc_big_nt(m);
        }
    } else if (m == 2 || m == 5 || m == 10) {
        f.kernel = RC_FK_TILE; f.tw = rc_tile_tw(m); f.th = rc_tile_th(m); f.nt = RC_BLOCK;
    } else {
        f.kernel = RC_FK_RUNTIME; f.nt = RC_BLOCK;
        pick_runtime_tile(m, f.tw, f.th);
    }
    f.tiles_x = (a.w + f.tw - 1) / f.tw;
    f.tiles_y = (a.h + f.th - 1) / f.th;
    f.grid_y = cp.ngroups ? cp.ngroups : pairs;
    if (f.kernel == RC_FK_RRC) {
        // k_flow_iter2_rrc's own test, per tile: the 32 x 8 NIT grid of M starts 2 px before the tile
        int nx = 0, ny = 0;
        for (int t = 0; t < f.tiles_x; t++) nx += (t * f.tw - 2 >= 5 && t * f.tw - 2 + 32 <= a.w - 5) ? 1 : 0;
        for (int t = 0; t < f.tiles_y; t++) ny += (t * f.th - 2 >= 5 && t * f.th - 2 + 8 * f.nit <= a.h - 5) ? 1 : 0;
        f.interior = nx * ny;
    }
}

void rc_flow_form(const RcIterArgs& a, int pairs, int fuse, RcFlowForm& f) {
    RcChainPlan cp;
    rc_flow_form_plan(a, pairs, fuse, f, cp);
}

void rc_launch_flow_iter2(const RcIterArgs& a, int pairs, hipStream_t s) {
    const int g = a.win.gaussian ? 1 : 0;
    switch (a.in_mode * 2 + g) {
        case 0: launch_w3x2<0, 0>(a, pairs, s); break;
        case 1: launch_w3x2<0, 1>(a, pairs, s); break;
        case 2: launch_w3x2<1, 0>(a, pairs, s); break;
        case 3: launch_w3x2<1, 1>(a, pairs, s); break;
        case 4: launch_w3x2<2, 0>(a, pairs, s); break;
        default: launch_w3x2<2, 1>(a, pairs, s); break;
    }
}

void rc_launch_flow_iter(const RcIterArgs& a, int pairs, hipStream_t s) {
    const int m = a.win.m, g = a.win.gaussian ? 1 : 0;
    RcFlowForm f;
    rc_flow_form(a, pairs, 1, f);
    switch (f.kernel) {
        case RC_FK_W3:
            switch (a.in_mode * 2 + g) {
                case 0: launch_w3<0, 0>(a, f, pairs, s); break;
                case 1: launch_w3<0, 1>(a, f, pairs, s); break;
                case 2: launch_w3<1, 0>(a, f, pairs, s); break;
                case 3: launch_w3<1, 1>(a, f, pairs, s); break;
                case 4: launch_w3<2, 0>(a, f, pairs, s); break;
                default: launch_w3<2, 1>(a, f, pairs, s); break;
            }
            return;
        case RC_FK_SWEEP:
            m == 5 ? launch_iter_sweep<5, 1024, 1>(a, f, pairs, s) : launch_iter_sweep<10, 1024, 1>(a, f, pairs, s);
            return;
        case RC_FK_BIG:
            if (m == 2) { g ? launch_iter_big<2, 1, 512>(a, f, pairs, s) : launch_iter_big<2, 0, 512>(a, f, pairs, s); }
            else if (m == 5) { g ? launch_iter_big<5, 1, 1024>(a, f, pairs, s) : launch_iter_big<5, 0, 1024>(a, f, pairs, s); }
            else { g ? launch_iter_big<10, 1, 1024, 64>(a, f, pairs, s) : launch_iter_big<10, 0, 1024, 64>(a, f, pairs, s); }
            return;
        case RC_FK_TILE:
            if (m == 1) { g ? launch_iter_t<64, 16, 1, 1>(a, f, pairs, s) : launch_iter_t<64, 16, 1, 0>(a, f, pairs, s); }
            else if (m == 2) { g ? launch_iter_t<64, 16, 2, 1>(a, f, pairs, s) : launch_iter_t<64, 16, 2, 0>(a, f, pairs, s); }
            else if (m == 5) { g ? launch_iter_t<32, 32, 5, 1>(a, f, pairs, s) : launch_iter_t<32, 32, 5, 0>(a, f, pairs, s); }
            else { g ? launch_iter_t<32, 32, 10, 1>(a, f, pairs, s) : launch_iter_t<32, 32, 10, 0>(a, f, pairs, s); }
            return;
        default: break;
    }
    RcIterArgs b = a;
    rc_form_grid(b, f);
    size_t lds = iter_lds(b.tw, b.th, m, true);
    RC_ALLOW_LDS((k_flow_iter<0, 0, 0, 0>), lds);
    hipLaunchKernelGGL((k_flow_iter<0, 0, 0, 0>), dim3(b.tiles_x * b.tiles_y, pairs, 1), dim3(RC_BLOCK), lds, s, b);
}

}  // namespace RC_FLOW_NS
