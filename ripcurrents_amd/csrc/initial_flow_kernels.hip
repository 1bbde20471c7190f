// initial_flow_kernels.hip -- OPTFLOW_USE_INITIAL_FLOW: the caller's flow field reduced to the coarsest scale.
//
// optflow.cpp calc(), at the coarsest scale k only:   resize(flow0, flow_k, Size(w_k, h_k), 0, 0, INTER_AREA);
//                                                     flow_k *= scale            (scale = pyr_scale^k, a float multiply)
// INTER_AREA on CV_32FC2 (imgproc/resize.cpp, scalar code path), per channel:
//   both ratios integers (resizeAreaFast_): fp32 sum over the iy x ix block in row-major order, * (1.f / (ix * iy));
//   otherwise (resizeArea_ + computeResizeAreaTab): per source row buf = sum_k S[xsi[k]] * xalpha[k] in table order,
//   sum = beta * buf for the first source row of an output row, sum += beta * buf after it.
// One lane per output pixel keeps exactly that order; -ffp-contract=off keeps every product and sum rounded on its own.
// The kernel is bound by the read of the full-resolution field (8 W H bytes per pair): consecutive lanes take consecutive
// output pixels, so a wave reads one contiguous span of every source row, 16 bytes per load wherever the field's base,
// row step and pair stride allow it.

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "rc_device.h"
#include "rc_host.h"

#define RC_AREA_TX 64        // output pixels per block row (one wave)
#define RC_AREA_TY 4         // output rows per block
#define RC_AREA_LDS_TAPS 2048   // x-table entries a block can stage (16 KB)

__device__ __forceinline__ void rc_area_acc(float2& s, bool& first, float x, float y) {
    if (first) { s.x = x; s.y = y; first = false; }
    else { s.x += x; s.y += y; }
}

// Integer ratios IX x IY, 16-byte loads (IX == 1: the lane's block is one float2 wide).  The host has checked
// W == IX * w, H == IY * h and, for IX >= 2, that base, row step and pair stride are multiples of 16.
template <int IX, int IY>
__global__ __launch_bounds__(RC_BLOCK) void k_flow_area_init(RcFlowAreaArgs a) {
    const int dx = blockIdx.x * RC_AREA_TX + (threadIdx.x & 63), dy = blockIdx.y * RC_AREA_TY + (threadIdx.x >> 6);
    if (dx >= a.w || dy >= a.h) return;
    const int z = blockIdx.z;
    const char* S = a.src + (size_t)z * a.src_pair_stride + (size_t)dy * IY * a.src_step + (size_t)dx * (IX * 8);
    float2 sum = make_float2(0.f, 0.f);
    bool first = true;
    // at most 32 texels (16 loads) in flight per lane: the whole 16 x 16 block unrolled would not fit the registers
    constexpr int ROWS = IX * IY <= 32 ? IY : (32 / IX > 0 ? 32 / IX : 1);
    for (int ky0 = 0; ky0 < IY; ky0 += ROWS) {
        if constexpr (IX == 1) {
            float2 v[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) v[r] = *(const float2*)(S + (size_t)(ky0 + r) * a.src_step);
#pragma unroll
            for (int r = 0; r < ROWS; r++) rc_area_acc(sum, first, v[r].x, v[r].y);
        } else {
            float4 v[ROWS][IX / 2];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const float4* row = (const float4*)(S + (size_t)(ky0 + r) * a.src_step);
#pragma unroll
                for (int q = 0; q < IX / 2; q++) v[r][q] = row[q];
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++)
#pragma unroll
                for (int q = 0; q < IX / 2; q++) {
                    rc_area_acc(sum, first, v[r][q].x, v[r][q].y);
                    rc_area_acc(sum, first, v[r][q].z, v[r][q].w);
                }
        }
    }
    const float inv = 1.f / (float)(IX * IY);
    float2 o;
    o.x = (sum.x * inv) * a.mul;
    o.y = (sum.y * inv) * a.mul;
    a.dst[(size_t)z * a.dst_pair_stride + (size_t)dy * a.w + dx] = o;
}

// Integer ratios of any size and any 8-byte-aligned layout: the same sums with one float2 per load.
__global__ __launch_bounds__(RC_BLOCK) void k_flow_area_init_any(RcFlowAreaArgs a) {
    const int dx = blockIdx.x * RC_AREA_TX + (threadIdx.x & 63), dy = blockIdx.y * RC_AREA_TY + (threadIdx.x >> 6);
    if (dx >= a.w || dy >= a.h) return;
    const int z = blockIdx.z;
    const char* S = a.src + (size_t)z * a.src_pair_stride + (size_t)dy * a.iy * a.src_step + (size_t)dx * a.ix * 8;
    float2 sum = make_float2(0.f, 0.f);
    bool first = true;
    for (int ky = 0; ky < a.iy; ky++) {
        const float2* row = (const float2*)(S + (size_t)ky * a.src_step);
        int kx = 0;
        for (; kx + 4 <= a.ix; kx += 4) {
            const float2 v0 = row[kx], v1 = row[kx + 1], v2 = row[kx + 2], v3 = row[kx + 3];
            rc_area_acc(sum, first, v0.x, v0.y); rc_area_acc(sum, first, v1.x, v1.y);
            rc_area_acc(sum, first, v2.x, v2.y); rc_area_acc(sum, first, v3.x, v3.y);
        }
        for (; kx < a.ix; kx++) { const float2 v = row[kx]; rc_area_acc(sum, first, v.x, v.y); }
    }
    const float inv = 1.f / (float)(a.ix * a.iy);
    float2 o;
    o.x = (sum.x * inv) * a.mul;
    o.y = (sum.y * inv) * a.mul;
    a.dst[(size_t)z * a.dst_pair_stride + (size_t)dy * a.w + dx] = o;
}

// Fractional ratios: the DecimateAlpha tables.  A wave owns one output row, so the row table is read through
// wave-uniform (scalar) loads; the column table of the block's 64 output columns is staged in LDS once (LDS_TAB) --
// without it the lanes gather the entries from global memory (ratios beyond RC_AREA_LDS_TAPS / 64 only).
template <int LDS_TAB>
__global__ __launch_bounds__(RC_BLOCK) void k_flow_area_init_tab(RcFlowAreaArgs a) {
    __shared__ int s_xsi[LDS_TAB ? RC_AREA_LDS_TAPS : 1];
    __shared__ float s_xal[LDS_TAB ? RC_AREA_LDS_TAPS : 1];
    const int bx0 = blockIdx.x * RC_AREA_TX;
    const int dx = bx0 + (threadIdx.x & 63);
    const int dy = blockIdx.y * RC_AREA_TY + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int z = blockIdx.z;
    const int bx1 = min(bx0 + RC_AREA_TX, a.w);
    const int t0 = a.xstart[bx0];
    if (LDS_TAB) {
        const int t1 = a.xstart[bx1];              // t1 - t0 <= RC_AREA_LDS_TAPS: checked by the host for every block
        for (int i = threadIdx.x; i < t1 - t0; i += RC_BLOCK) { s_xsi[i] = a.xsi[t0 + i]; s_xal[i] = a.xalpha[t0 + i]; }
        __syncthreads();
    }
    if (dx >= a.w || dy >= a.h) return;
    const int* xsi = LDS_TAB ? s_xsi - t0 : a.xsi;
    const float* xal = LDS_TAB ? s_xal - t0 : a.xalpha;
    const int x0 = a.xstart[dx], x1 = a.xstart[dx + 1];
    const int y0 = a.ystart[dy], y1 = a.ystart[dy + 1];
    const char* base = a.src + (size_t)z * a.src_pair_stride;
    float2 sum = make_float2(0.f, 0.f);
    for (int j = y0; j < y1; j++) {
        const float2* S = (const float2*)(base + (size_t)a.ysi[j] * a.src_step);
        const float beta = a.yalpha[j];
        float2 buf = make_float2(0.f, 0.f);
        int k = x0;
        for (; k + 4 <= x1; k += 4) {
            const float2 v0 = S[xsi[k]], v1 = S[xsi[k + 1]], v2 = S[xsi[k + 2]], v3 = S[xsi[k + 3]];
            const float a0 = xal[k], a1 = xal[k + 1], a2 = xal[k + 2], a3 = xal[k + 3];
            buf.x += v0.x * a0; buf.y += v0.y * a0;
            buf.x += v1.x * a1; buf.y += v1.y * a1;
            buf.x += v2.x * a2; buf.y += v2.y * a2;
            buf.x += v3.x * a3; buf.y += v3.y * a3;
        }
        for (; k < x1; k++) {
            const float2 v = S[xsi[k]];
            const float al = xal[k];
            buf.x += v.x * al; buf.y += v.y * al;
        }
        if (j == y0) { sum.x = beta * buf.x; sum.y = beta * buf.y; }
        else { sum.x += beta * buf.x; sum.y += beta * buf.y; }
    }
    float2 o;
    o.x = sum.x * a.mul;
    o.y = sum.y * a.mul;
    a.dst[(size_t)z * a.dst_pair_stride + (size_t)dy * a.w + dx] = o;
}

// Geometry of the reduction W x H -> w x h (w <= W, h <= H) and, for fractional ratios, its tables uploaded into `tab`.
// Blocking (the tables are a few KB); the caller has made sure that no launch still reads `tab`.
int rc_flow_area_prepare(RcBuf& tab, int W, int H, int w, int h, RcFlowAreaArgs& a) {
    memset(&a, 0, sizeof(a));
    if (W <= 0 || H <= 0 || w <= 0 || h <= 0 || w > W || h > H) { rc_set_error("initial flow: bad reduction %dx%d -> %dx%d", W, H, w, h); return RC_EINVAL; }
    a.W = W; a.H = H; a.w = w; a.h = h;
    const double scale_x = (double)W / w, scale_y = (double)H / h;
    const int ix = (int)nearbyint(scale_x), iy = (int)nearbyint(scale_y);
    a.ix = ix; a.iy = iy;
    // resize.cpp is_area_fast; the products make the kernels' source bounds (dy * iy + ky < H) explicit
    a.fast = fabs(scale_x - ix) < DBL_EPSILON && fabs(scale_y - iy) < DBL_EPSILON && (long long)ix * w == W && (long long)iy * h == H;
    if (a.fast) return RC_OK;
    std::vector<int> xs, xi, ys, yi;
    std::vector<float> xa, ya;
    rc_area_tab(W, w, scale_x, xs, xi, xa);
    rc_area_tab(H, h, scale_y, ys, yi, ya);
    // every index a lane dereferences comes from these tables
    for (int v : xi) if (v < 0 || v >= W) { rc_set_error("initial flow: column table out of range"); return RC_EINVAL; }
    for (int v : yi) if (v < 0 || v >= H) { rc_set_error("initial flow: row table out of range"); return RC_EINVAL; }
    a.lds_tab = 1;
    for (int b = 0; b < w; b += RC_AREA_TX)
        if (xs[std::min(b + RC_AREA_TX, w)] - xs[b] > RC_AREA_LDS_TAPS) a.lds_tab = 0;
    const size_t nx = xi.size(), ny = yi.size();
    std::vector<int> host((size_t)(w + 1) + 2 * nx + (size_t)(h + 1) + 2 * ny);
    int* p = host.data();
    int* h_xs = p; p += w + 1;
    int* h_xi = p; p += nx;
    int* h_xa = p; p += nx;
    int* h_ys = p; p += h + 1;
    int* h_yi = p; p += ny;
    int* h_ya = p;
    memcpy(h_xs, xs.data(), 4 * (size_t)(w + 1)); memcpy(h_xi, xi.data(), 4 * nx); memcpy(h_xa, xa.data(), 4 * nx);
    memcpy(h_ys, ys.data(), 4 * (size_t)(h + 1)); memcpy(h_yi, yi.data(), 4 * ny); memcpy(h_ya, ya.data(), 4 * ny);
    int rc = rc_buf_ensure(tab, host.size() * 4);
    if (rc) return rc;
    RC_HIP(hipMemcpy(tab.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    const int* d = (const int*)tab.p;
    a.xstart = d + (h_xs - host.data()); a.xsi = d + (h_xi - host.data()); a.xalpha = (const float*)(d + (h_xa - host.data()));
    a.ystart = d + (h_ys - host.data()); a.ysi = d + (h_yi - host.data()); a.yalpha = (const float*)(d + (h_ya - host.data()));
    return RC_OK;
}

template <int IX>
static bool launch_area_iy(const RcFlowAreaArgs& a, dim3 grid, hipStream_t s) {
    switch (a.iy) {
        case 1: hipLaunchKernelGGL((k_flow_area_init<IX, 1>), grid, dim3(RC_BLOCK), 0, s, a); return true;
        case 2: hipLaunchKernelGGL((k_flow_area_init<IX, 2>), grid, dim3(RC_BLOCK), 0, s, a); return true;
        case 4: hipLaunchKernelGGL((k_flow_area_init<IX, 4>), grid, dim3(RC_BLOCK), 0, s, a); return true;
        case 8: hipLaunchKernelGGL((k_flow_area_init<IX, 8>), grid, dim3(RC_BLOCK), 0, s, a); return true;
        case 16: hipLaunchKernelGGL((k_flow_area_init<IX, 16>), grid, dim3(RC_BLOCK), 0, s, a); return true;
    }
    return false;
}

// a: geometry / tables from rc_flow_area_prepare, with src, src_step, src_pair_stride, dst, dst_pair_stride, mul filled in.
void rc_launch_flow_area_init(const RcFlowAreaArgs& a, int pairs, hipStream_t s) {
    const dim3 grid((a.w + RC_AREA_TX - 1) / RC_AREA_TX, (a.h + RC_AREA_TY - 1) / RC_AREA_TY, pairs);
    if (!a.fast) {
        if (a.lds_tab) hipLaunchKernelGGL(k_flow_area_init_tab<1>, grid, dim3(RC_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(k_flow_area_init_tab<0>, grid, dim3(RC_BLOCK), 0, s, a);
        return;
    }
    const bool al16 = a.ix == 1 || (((uintptr_t)a.src | a.src_step | a.src_pair_stride) & 15) == 0;
    bool done = false;
    if (al16) {
        switch (a.ix) {
            case 1: done = launch_area_iy<1>(a, grid, s); break;
            case 2: done = launch_area_iy<2>(a, grid, s); break;
            case 4: done = launch_area_iy<4>(a, grid, s); break;
            case 8: done = launch_area_iy<8>(a, grid, s); break;
            case 16: done = launch_area_iy<16>(a, grid, s); break;
        }
    }
    if (!done) hipLaunchKernelGGL(k_flow_area_init_any, grid, dim3(RC_BLOCK), 0, s, a);
}
