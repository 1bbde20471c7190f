// pyr_polyexp_kernels.hip -- gfx950 kernels for the image side of dense Farneback flow.
//
// Replaces the arithmetic behind cv::calcOpticalFlowFarneback as the reference calls it
// (RipCurrents_main/ripcurrents.cpp:215; main.cpp:264,609,742,961,1119,1481).  Stages
// follow SURVEY.md section 8(a):
//   k_pyr_level   A1  convertTo(32F) + GaussianBlur(full res, REFLECT_101) + resize(LINEAR)
//   k_polyexp     A2  FarnebackPolyExp            -> R = (y, x, yy, xx | xy) planes
//   (flow_iter_kernels.hip holds A3-A6)
// Data layout in HBM (all fp32):
//   I_k   [slot][h][w]            float
//   RA_k  [slot][h][w]            float4 (y, x, yy, xx)  -- one 16-B load per pixel/texel; stored at 1/2 of upstream's R
//   RB_k  [slot][h][w]            float  (xy)            -- stored at 1/4 (option "exact": unscaled)
//   flow  [pair][h][w]            float2 (x, y)  == CV_32FC2
// Compiled with -ffp-contract=off; fused multiply-adds are written explicitly (RC_FMA)
// in the convolution loops and nowhere else, so the gather / matrix / resize arithmetic
// rounds operation by operation like the scalar C++ it has to match.

#include "rc_device.h"

// ===================================================================== A1 pyramid
// One block = tw x th output pixels of scale k >= 1 (scale 0 is fused into k_polyexp).
// The 8-bit source region the tile needs (blur radius + resize footprint) is staged in
// LDS, the horizontal blur is evaluated only at the two source columns each output column
// samples, then each thread does the vertical blur at its 2x2 sample points and the
// bilinear resize.  The resize.cpp coordinate tables (xofs/alpha, yofs/beta) are built
// once per block in LDS; loops are row-per-wave so no index needs a division.
__global__ __launch_bounds__(RC_BLOCK) void k_pyr_level(RcPyrArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* reg = smem;                                    // [reg_hmax][reg_wp] u8
    float* rp = (float*)(smem + (size_t)a.reg_hmax * a.reg_wp);   // [reg_hmax][2*tw]
    int* xs = (int*)(rp + (size_t)a.reg_hmax * 2 * a.tw);         // [2*tw] source column per (dx, tap)
    float* xa = (float*)(xs + 2 * a.tw);                          // [tw]  alpha
    int* ys = (int*)(xa + a.tw);                                  // [2*th] clamped rows sy0, sy1
    float* ya = (float*)(ys + 2 * a.th);                          // [th]  beta
    float* ks = ya + a.th;                                        // [ksize] blur taps
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int z = blockIdx.z;
    const int tx0 = blockIdx.x * a.tw, ty0 = blockIdx.y * a.th;
    const int r = a.ksize >> 1;
    const int W0 = a.W0, H0 = a.H0;

    if (tid < a.tw) {
        float ax;
        int sx = rc_src_x(min(tx0 + tid, a.w - 1), a.scale_x, W0, ax);
        xs[2 * tid] = sx;
        xs[2 * tid + 1] = min(sx + 1, W0 - 1);
        xa[tid] = ax;
    } else if (tid >= 64 && tid < 128) {
        for (int k = tid - 64; k < a.ksize; k += 64) ks[k] = a.kern[k];
    } else if (tid >= 128 && tid < 128 + a.th) {
        int i = tid - 128;
        float ay;
        int sy = rc_src_y(min(ty0 + i, a.h - 1), a.scale_y, ay);
        ys[2 * i] = rc_clampi(sy, 0, H0 - 1);
        ys[2 * i + 1] = rc_clampi(sy + 1, 0, H0 - 1);
        ya[i] = ay;
    }
    __syncthreads();
    const int nx = min(a.tw, a.w - tx0), ny = min(a.th, a.h - ty0);
    const int reg_x0 = xs[0] - r, reg_x1 = xs[2 * nx - 1] + r;
    const int reg_y0 = ys[0] - r, reg_y1 = ys[2 * ny - 1] + r;
    const int reg_w = reg_x1 - reg_x0 + 1, reg_h = reg_y1 - reg_y0 + 1;

    // region load, 16 rows in flight per thread (a dependent load->LDS-store loop would
    // serialise one HBM round trip per element)
    const uint8_t* src = a.src + (size_t)z * a.src_frame_stride;
    for (int j = lane; j < reg_w; j += 64) {
        const int sx = rc_reflect101(reg_x0 + j, W0);
        for (int ib = wv; ib < reg_h; ib += 16 * (RC_BLOCK / 64)) {
            unsigned char v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) {
                int i = ib + q * (RC_BLOCK / 64);
                v[q] = i < reg_h ? src[(size_t)rc_reflect101(reg_y0 + i, H0) * a.src_step + sx] : 0;
            }
#pragma unroll
            for (int q = 0; q < 16; q++) {
                int i = ib + q * (RC_BLOCK / 64);
                if (i < reg_h) reg[i * a.reg_wp + j] = v[q];
            }
        }
    }
    __syncthreads();

    // horizontal blur (RowFilter order of smooth.cpp; SymmRowSmallFilter for ksize<=5)
    const int tw2 = 2 * a.tw;
    const float* kern = ks;
    for (int i = wv; i < reg_h; i += RC_BLOCK / 64) {
        for (int j = lane; j < tw2; j += 64) {
            const unsigned char* S = reg + i * a.reg_wp + (xs[j] - reg_x0);
            float s0;
            if (a.ksize == 3) {
                s0 = (float)S[0] * kern[1] + ((float)S[-1] + (float)S[1]) * kern[2];
            } else if (a.ksize == 5) {
                s0 = (float)S[0] * kern[2] + ((float)S[-1] + (float)S[1]) * kern[3] +
                     ((float)S[-2] + (float)S[2]) * kern[4];
            } else {
                s0 = kern[0] * (float)S[-r];
                for (int k = 1; k < a.ksize; k++) s0 += kern[k] * (float)S[k - r];
            }
            rp[i * tw2 + j] = s0;
        }
    }
    __syncthreads();

    const int slot = (a.dslot0 + z * a.zstep) % a.nslots;
    float* dst = a.dst + (size_t)slot * a.dst_slot_stride;
    for (int ly = wv; ly < ny; ly += RC_BLOCK / 64) {
        const int i0 = ys[2 * ly] - reg_y0, i1 = ys[2 * ly + 1] - reg_y0;
        const float ay = ya[ly];
        for (int lx = lane; lx < nx; lx += 64) {
            const float* c0 = rp + 2 * lx;
            // vertical blur (SymmColumnFilter order) at the four sample points
            float b00 = kern[r] * c0[i0 * tw2], b01 = kern[r] * c0[i0 * tw2 + 1];
            float b10 = kern[r] * c0[i1 * tw2], b11 = kern[r] * c0[i1 * tw2 + 1];
            for (int k = 1; k <= r; k++) {
                float kk = kern[r + k];
                b00 += kk * (c0[(i0 + k) * tw2] + c0[(i0 - k) * tw2]);
                b01 += kk * (c0[(i0 + k) * tw2 + 1] + c0[(i0 - k) * tw2 + 1]);
                b10 += kk * (c0[(i1 + k) * tw2] + c0[(i1 - k) * tw2]);
                b11 += kk * (c0[(i1 + k) * tw2 + 1] + c0[(i1 - k) * tw2 + 1]);
            }
            const float ax = xa[lx];
            float a0 = 1.f - ax, a1 = ax, w0 = 1.f - ay, w1 = ay;
            float r0 = b00 * a0 + b01 * a1;
            float r1 = b10 * a0 + b11 * a1;
            dst[(size_t)(ty0 + ly) * a.w + tx0 + lx] = r0 * w0 + r1 * w1;
        }
    }
}

// ------------------------------------------------------------------------------------
// Direct form for small blur radii (scales 1 and 2 at pyr_scale 0.5: 3 and 9 taps): one
// thread per output pixel, no LDS and no barrier.  Each needed source row arrives as a few
// aligned dwords (neighbouring threads share them in L1) and is byte-aligned with
// v_alignbyte; pixels whose footprint touches the image border take the per-byte
// REFLECT_101 path.  Same operation order as the tiled kernel (bit-identical results).
template <int R>
__device__ __forceinline__ float rc_rowpass(const float* b, const float* k) {
    if (R == 1) return b[1] * k[1] + (b[0] + b[2]) * k[2];
    if (R == 2) return b[2] * k[2] + (b[1] + b[3]) * k[3] + (b[0] + b[4]) * k[4];
    float s = k[0] * b[0];
#pragma unroll
    for (int j = 1; j < 2 * R + 1; j++) s += k[j] * b[j];
    return s;
}

template <int R>
__device__ __forceinline__ void rc_pyr_direct_body(const RcPyrArgs& a, int bx, int by, int z) {
    constexpr int KS = 2 * R + 1, NB = 2 * R + 2, NDW = (2 * R + 8) / 4, NROW = 2 * R + 2;
    const int dx = bx * 64 + (threadIdx.x & 63), dy = by * 4 + (threadIdx.x >> 6);
    if (dx >= a.w || dy >= a.h) return;
    const int W0 = a.W0, H0 = a.H0;
    float k[KS];
#pragma unroll
    for (int j = 0; j < KS; j++) k[j] = a.kern[j];
    float ax, ay;
    const int sx = rc_src_x(dx, a.scale_x, W0, ax);
    const int sx1 = min(sx + 1, W0 - 1);
    const int sy = rc_src_y(dy, a.scale_y, ay);
    const int y0 = rc_clampi(sy, 0, H0 - 1), y1 = rc_clampi(sy + 1, 0, H0 - 1);
    const uint8_t* src = a.src + (size_t)z * a.src_frame_stride;
    const int xs = sx - R, xa = xs & ~3, off = xs & 3;
    const bool aligned = ((((size_t)a.src) | a.src_step | a.src_frame_stride) & 3) == 0;
    const bool fast = aligned && sx1 == sx + 1 && y1 == y0 + 1 && xs >= 0 && xa + 4 * NDW <= W0 &&
                      sx1 + R <= W0 - 1 && y0 - R >= 0 && y1 + R <= H0 - 1;
    // row-pass results at columns sx and sx+1 for the NROW virtual source rows y0-R .. y0+R+1
    float rp0[NROW], rp1[NROW];
    if (fast) {
        unsigned int dw[NROW][NDW];
#pragma unroll
        for (int rr = 0; rr < NROW; rr++) {
            const unsigned int* row = (const unsigned int*)(src + (size_t)(y0 - R + rr) * a.src_step + xa);
#pragma unroll
            for (int j = 0; j < NDW; j++) dw[rr][j] = row[j];
        }
#pragma unroll
        for (int rr = 0; rr < NROW; rr++) {
            float b[NB];
#pragma unroll
            for (int j = 0; j < (NB + 3) / 4; j++) {
                unsigned int sd = j + 1 < NDW ? __builtin_amdgcn_alignbyte(dw[rr][j + 1], dw[rr][j], off)
                                              : (dw[rr][j] >> (8 * off));
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (4 * j + t < NB) b[4 * j + t] = (float)((sd >> (8 * t)) & 255u);
            }
            rp0[rr] = rc_rowpass<R>(b, k);
            rp1[rr] = rc_rowpass<R>(b + 1, k);
        }
    } else {
        // border footprint: per-byte REFLECT_101 addressing, same virtual rows/columns.  (When
        // sx+1 is clamped its weight a1 is 0, and when y1 == y0 the second row pair is a copy
        // of the first, so the virtual column sx+1 / row y0+R+1 only has to be finite.)
        int cx[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) cx[j] = rc_reflect101(xs + j, W0);
        constexpr int HALF = (NROW + 1) / 2;
#pragma unroll
        for (int part = 0; part < 2; part++) {
            unsigned char bytes[HALF][NB];
#pragma unroll
            for (int rh = 0; rh < HALF; rh++) {
                int rr = part * HALF + rh;
                const uint8_t* row = src + (size_t)rc_reflect101(y0 - R + min(rr, NROW - 1), H0) * a.src_step;
#pragma unroll
                for (int j = 0; j < NB; j++) bytes[rh][j] = row[cx[j]];
            }
#pragma unroll
            for (int rh = 0; rh < HALF; rh++) {
                int rr = part * HALF + rh;
                if (rr < NROW) {
                    float b[NB];
#pragma unroll
                    for (int j = 0; j < NB; j++) b[j] = (float)bytes[rh][j];
                    rp0[rr] = rc_rowpass<R>(b, k);
                    rp1[rr] = rc_rowpass<R>(b + 1, k);
                }
            }
        }
    }
    float b00 = k[R] * rp0[R], b01 = k[R] * rp1[R];
    float b10 = k[R] * rp0[R + 1], b11 = k[R] * rp1[R + 1];
#pragma unroll
    for (int j = 1; j <= R; j++) {
        b00 += k[R + j] * (rp0[R + j] + rp0[R - j]);
        b01 += k[R + j] * (rp1[R + j] + rp1[R - j]);
        b10 += k[R + j] * (rp0[R + 1 + j] + rp0[R + 1 - j]);
        b11 += k[R + j] * (rp1[R + 1 + j] + rp1[R + 1 - j]);
    }
    if (y1 == y0) { b10 = b00; b11 = b01; }
    float a0 = 1.f - ax, a1 = ax, w0 = 1.f - ay, w1 = ay;
    float r0 = b00 * a0 + b01 * a1;
    float r1 = b10 * a0 + b11 * a1;
    const int slot = (a.dslot0 + z * a.zstep) % a.nslots;
    a.dst[(size_t)slot * a.dst_slot_stride + (size_t)dy * a.w + dx] = r0 * w0 + r1 * w1;
}

template <int R>
__global__ __launch_bounds__(RC_BLOCK) void k_pyr_direct(RcPyrArgs a) {
    rc_pyr_direct_body<R>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// ------------------------------------------------------------------------------------
// Row-pass / column-pass form for any decimation (scales 1..4 at pyr_scale 0.5: 3, 9, 19 and 39
// taps): a block owns 32 x 8 outputs.  Phase 1: one item = (virtual source row, output column);
// the row filter at the two adjacent source columns that output column samples is evaluated
// straight from global memory (aligned dwords + v_alignbyte, per-byte REFLECT_101 at the
// borders) and stored as a float2 in LDS -- the 8-bit region itself is never staged.  Rows are
// shared by the outputs above and below (a 39-tap window at decimation 16 spans 2.4 output
// rows).  Phase 2: one thread per output does the four column filters and the bilinear
// resize.  Same operation order as k_pyr_level / k_pyr_direct (bit-identical results).
template <int R>
__device__ __forceinline__ void rc_pyr_rows_body(const RcPyrArgs& a, int bx, int by, int z, float2* rp) {
    constexpr int KS = 2 * R + 1, NB = 2 * R + 2, NDW = (2 * R + 8) / 4, TWO = 32, THO = 8;
    // rp: [reg_h][TWO]  row-pass results at (sx, sx + 1)
    const int tid = threadIdx.x;
    const int tx0 = bx * TWO, ty0 = by * THO;
    const int W0 = a.W0, H0 = a.H0;
    float k[KS];
#pragma unroll
    for (int j = 0; j < KS; j++) k[j] = a.kern[j];
    // virtual source rows of the block: [y_first - R, y_last + 1 + R]
    float ayf, ayl;
    const int ny = min(THO, a.h - ty0);
    const int sy_first = rc_clampi(rc_src_y(ty0, a.scale_y, ayf), 0, H0 - 1);
    const int sy_last = rc_clampi(rc_src_y(ty0 + ny - 1, a.scale_y, ayl) + 1, 0, H0 - 1);
    const int reg_y0 = sy_first - R, reg_h = sy_last + R - reg_y0 + 1;
    const uint8_t* src = a.src + (size_t)z * a.src_frame_stride;
    const bool aligned = ((((size_t)a.src) | a.src_step | a.src_frame_stride) & 3) == 0;

    {   // ---- phase 1: row filter
        const int col = tid & (TWO - 1), r0 = tid / TWO;
        const int dx = min(tx0 + col, a.w - 1);
        float ax;
        const int sx = rc_src_x(dx, a.scale_x, W0, ax);
        const int sx1 = min(sx + 1, W0 - 1);
        const int xs = sx - R, xa = xs & ~3, off = xs & 3;
        const bool fastx = aligned && sx1 == sx + 1 && xs >= 0 && xa + 4 * NDW <= W0 && sx1 + R <= W0 - 1;
        int cx[NB];
        if (!fastx) {
#pragma unroll
            for (int j = 0; j < NB; j++) cx[j] = rc_reflect101(xs + j, W0);
        }
        constexpr int RPI = RC_BLOCK / TWO;            // rows in flight per pass
        constexpr int UNR = R <= 4 ? 4 : 2;            // rows per thread per batch (loads first, then math)
        for (int ib = r0; ib < reg_h; ib += RPI * UNR) {
            float b[UNR][NB];
            if (fastx) {
                unsigned int dw[UNR][NDW];
#pragma unroll
                for (int u = 0; u < UNR; u++) {
                    const int i = min(ib + u * RPI, reg_h - 1);
                    const unsigned int* row = (const unsigned int*)(src + (size_t)rc_reflect101(reg_y0 + i, H0) * a.src_step + xa);
#pragma unroll
                    for (int j = 0; j < NDW; j++) dw[u][j] = row[j];
                }
#pragma unroll
                for (int u = 0; u < UNR; u++)
#pragma unroll
                    for (int j = 0; j < (NB + 3) / 4; j++) {
                        unsigned int sd = j + 1 < NDW ? __builtin_amdgcn_alignbyte(dw[u][j + 1], dw[u][j], off)
                                                      : (dw[u][j] >> (8 * off));
#pragma unroll
                        for (int t = 0; t < 4; t++)
                            if (4 * j + t < NB) b[u][4 * j + t] = (float)((sd >> (8 * t)) & 255u);
                    }
            } else {
                unsigned char by[UNR][NB];
#pragma unroll
                for (int u = 0; u < UNR; u++) {
                    const int i = min(ib + u * RPI, reg_h - 1);
                    const uint8_t* row = src + (size_t)rc_reflect101(reg_y0 + i, H0) * a.src_step;
#pragma unroll
                    for (int j = 0; j < NB; j++) by[u][j] = row[cx[j]];
                }
#pragma unroll
                for (int u = 0; u < UNR; u++)
#pragma unroll
                    for (int j = 0; j < NB; j++) b[u][j] = (float)by[u][j];
            }
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int i = ib + u * RPI;
                if (i < reg_h) rp[i * TWO + col] = make_float2(rc_rowpass<R>(b[u], k), rc_rowpass<R>(b[u] + 1, k));
            }
        }
    }
    __syncthreads();

    // ---- phase 2: column filter at the 2 x 2 sample points + bilinear resize
    const int lx = tid & (TWO - 1), ly = tid / TWO;
    const int dx = tx0 + lx, dy = ty0 + ly;
    if (dx >= a.w || dy >= a.h) return;
    float ax, ay;
    (void)rc_src_x(dx, a.scale_x, W0, ax);
    const int sy = rc_src_y(dy, a.scale_y, ay);
    const int y0 = rc_clampi(sy, 0, H0 - 1), y1 = rc_clampi(sy + 1, 0, H0 - 1);
    const float2* c0 = rp + (y0 - reg_y0) * TWO + lx;
    const float2* c1 = rp + (y1 - reg_y0) * TWO + lx;
    float2 m0 = c0[0], m1 = c1[0];
    float b00 = k[R] * m0.x, b01 = k[R] * m0.y, b10 = k[R] * m1.x, b11 = k[R] * m1.y;
#pragma unroll
    for (int j = 1; j <= R; j++) {
        const float2 p0 = c0[j * TWO], q0 = c0[-j * TWO], p1 = c1[j * TWO], q1 = c1[-j * TWO];
        b00 += k[R + j] * (p0.x + q0.x);
        b01 += k[R + j] * (p0.y + q0.y);
        b10 += k[R + j] * (p1.x + q1.x);
        b11 += k[R + j] * (p1.y + q1.y);
    }
    const float a0 = 1.f - ax, a1 = ax, w0 = 1.f - ay, w1 = ay;
    const float r0 = b00 * a0 + b01 * a1;
    const float r1 = b10 * a0 + b11 * a1;
    const int slot = (a.dslot0 + z * a.zstep) % a.nslots;
    a.dst[(size_t)slot * a.dst_slot_stride + (size_t)dy * a.w + dx] = r0 * w0 + r1 * w1;
}

template <int R>
__global__ __launch_bounds__(RC_BLOCK) void k_pyr_rows(RcPyrArgs a) {
    extern __shared__ __align__(16) float2 rc_pyr_smem[];
    rc_pyr_rows_body<R>(a, blockIdx.x, blockIdx.y, blockIdx.z, rc_pyr_smem);
}

// Scales 1 and 2 of a pyr_scale = 0.5 pyramid (3 and 9 taps) in ONE launch: the two grids are
// independent and, for a frame or two, each is smaller than the GPU; blocks below n1 take the
// scale-1 tile code, the rest the scale-2 tile code.  Same bits as the separate launches.
__global__ __launch_bounds__(RC_BLOCK) void k_pyr_pair_3_9(RcPyrArgs a1, RcPyrArgs a2, int gx1, int gy1, int n1,
                                                           int gx2, int gy2) {
    extern __shared__ __align__(16) float2 rc_pyr_smem[];
    int id = blockIdx.x;
    if (id < n1) {
        const int z = id / (gx1 * gy1), r = id - z * gx1 * gy1;
        rc_pyr_direct_body<1>(a1, r % gx1, r / gx1, z);
    } else {
        id -= n1;
        const int z = id / (gx2 * gy2), r = id - z * gx2 * gy2;
        rc_pyr_rows_body<4>(a2, r % gx2, r / gx2, z, rc_pyr_smem);
    }
}

// true when the pair launch applies: 3 + 9 taps, row-pass LDS within the default limit
int rc_pyr_pair_ok(const RcPyrArgs& a1, const RcPyrArgs& a2) {
    const size_t lds = ((size_t)ceil(8 * a2.scale_y) + a2.ksize + 3) * 32 * sizeof(float2);
    return a1.ksize == 3 && a2.ksize == 9 && !a1.direct && !a2.direct && lds <= 48 * 1024;
}
void rc_launch_pyr_pair(const RcPyrArgs& a1, const RcPyrArgs& a2, int frames, hipStream_t s) {
    const int gx1 = (a1.w + 63) / 64, gy1 = (a1.h + 3) / 4, gx2 = (a2.w + 31) / 32, gy2 = (a2.h + 7) / 8;
    const int n1 = gx1 * gy1 * frames, n2 = gx2 * gy2 * frames;
    const size_t lds = ((size_t)ceil(8 * a2.scale_y) + 2 * 4 + 4) * 32 * sizeof(float2);
    hipLaunchKernelGGL(k_pyr_pair_3_9, dim3(n1 + n2), dim3(RC_BLOCK), lds, s, a1, a2, gx1, gy1, n1, gx2, gy2);
}

template <int R>
static void launch_pyr_rows(const RcPyrArgs& a, int frames, hipStream_t s) {
    const int reg_h = (int)ceil(8 * a.scale_y) + 2 * R + 4;
    const size_t lds = (size_t)reg_h * 32 * sizeof(float2);
    RC_ALLOW_LDS((k_pyr_rows<R>), lds);
    dim3 grid((a.w + 31) / 32, (a.h + 7) / 8, frames);
    hipLaunchKernelGGL(k_pyr_rows<R>, grid, dim3(RC_BLOCK), lds, s, a);
}

// Scale 0 on its own (the exact path; the fast path blurs inside the expansion): convertTo + GaussianBlur with the fixed taps
// (1/4, 1/2, 1/4) of sigma <= 0 + an identity resize = S / 16 with S the nine bytes weighted (1 2 1; 2 4 2; 1 2 1) under
// BORDER_REFLECT_101 -- smooth.cpp's float row filter then column filter is exact on 8-bit input (every intermediate is a multiple
// of 1/16 below 256) and the resize at scale 1 multiplies by 1 and adds 0 times a finite neighbour.  A thread owns four pixels
// of a row: three aligned dwords per source row away from the borders, reflected bytes at them.
__global__ __launch_bounds__(RC_BLOCK) void k_pyr0_blur3(RcPyrArgs a) {
    const int W = a.W0, H = a.H0, z = blockIdx.z;
    const int x = 4 * ((int)blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const uint8_t* src = a.src + (size_t)z * a.src_frame_stride;
    const bool aligned = ((((size_t)a.src) | a.src_step | a.src_frame_stride) & 3) == 0;
    const bool fast = aligned && x >= 4 && x + 8 <= W;
    unsigned int A = 0, B = 0, C = 0, D = 0;     // 16-bit pairs (X0, X2) (X1, X3) (X2, X4) (X3, X5) summed over the rows, X0 = column x - 1
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const uint8_t* row = src + (size_t)rc_reflect101(y - 1 + t, H) * a.src_step;
        unsigned int pa, pb, pc, pd;
        if (fast) {
            const unsigned int* r = (const unsigned int*)(row + x - 4);
            const unsigned int d0 = r[0], d1 = r[1], d2 = r[2];
            pa = __builtin_amdgcn_perm(d0, d1, 0x0c010c07u);
            pb = __builtin_amdgcn_perm(d1, d1, 0x0c020c00u);
            pc = __builtin_amdgcn_perm(d1, d1, 0x0c030c01u);
            pd = __builtin_amdgcn_perm(d2, d1, 0x0c040c02u);
        } else {
            unsigned int X[6];
#pragma unroll
            for (int j = 0; j < 6; j++) X[j] = row[rc_reflect101(min(x - 1 + j, W), W)];      // (columns past the row are not stored)
            pa = X[0] | X[2] << 16; pb = X[1] | X[3] << 16; pc = X[2] | X[4] << 16; pd = X[3] | X[5] << 16;
        }
        const int sh = t == 1 ? 1 : 0;
        A += pa << sh; B += pb << sh; C += pc << sh; D += pd << sh;
    }
    const unsigned int o02 = A + 2 * B + C, o13 = B + 2 * C + D;
    float4 o;
    o.x = (float)(o02 & 0xffffu) * 0.0625f;
    o.y = (float)(o13 & 0xffffu) * 0.0625f;
    o.z = (float)(o02 >> 16) * 0.0625f;
    o.w = (float)(o13 >> 16) * 0.0625f;
    const int slot = (a.dslot0 + z * a.zstep) % a.nslots;
    float* d = a.dst + (size_t)slot * a.dst_slot_stride + (size_t)y * W + x;
    if (x + 4 <= W && ((W & 3) == 0) && ((((size_t)a.dst) | (a.dst_slot_stride * 4)) & 15) == 0) *(float4*)d = o;
    else {
        d[0] = o.x;
        if (x + 1 < W) d[1] = o.y;
        if (x + 2 < W) d[2] = o.z;
        if (x + 3 < W) d[3] = o.w;
    }
}

void rc_launch_pyr(const RcPyrArgs& a, int frames, size_t lds, hipStream_t s) {
    if (a.fixed3 && !a.direct) {
        hipLaunchKernelGGL(k_pyr0_blur3, dim3((a.W0 + 255) / 256, (a.H0 + 3) / 4, frames), dim3(RC_BLOCK), 0, s, a);
        return;
    }
    const size_t rows_lds = ((size_t)ceil(8 * a.scale_y) + a.ksize + 3) * 32 * sizeof(float2);
    if (!a.direct && rows_lds <= 64 * 1024) {
        switch (a.ksize) {
            // (3 taps at decimation 2: the per-pixel direct form below is 20 % faster)
            case 9: launch_pyr_rows<4>(a, frames, s); return;
            case 19: launch_pyr_rows<9>(a, frames, s); return;
            case 39: launch_pyr_rows<19>(a, frames, s); return;
            default: break;
        }
    }
    if (a.ksize == 3 || a.ksize == 9) {
        dim3 grid((a.w + 63) / 64, (a.h + 3) / 4, frames);
        if (a.ksize == 3) hipLaunchKernelGGL(k_pyr_direct<1>, grid, dim3(RC_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(k_pyr_direct<4>, grid, dim3(RC_BLOCK), 0, s, a);
        return;
    }
    dim3 grid((a.w + a.tw - 1) / a.tw, (a.h + a.th - 1) / a.th, frames);
    hipLaunchKernelGGL(k_pyr_level, grid, dim3(RC_BLOCK), lds, s, a);
}

// ===================================================================== A2 polyexp
// 64x32 output tile per 512-thread block.  Separable: horizontal pass first (three sums
// per pixel), staged through LDS, vertical pass last so that every lane of a wave owns one
// column and all LDS reads and the 16-B global stores are conflict-free and coalesced.
// Each thread of the vertical pass produces 4 rows from a register window.
// The constants upstream multiplies the six filter products with are folded into the taps
// on the host (RcPolyK::qh, xga, xgb; the planes come out at their stored scale, (y, x, yy,
// xx) / 2 and xy / 4):
//   h0 = g_h     h1 = xga_h     h2 = qh_h
//   y = xga_v(h0)   yy = qh_v(h0)   |   x = g_v(h1)   xy = xgb_v(h1)   |   xx = g_v(h2)
// five vertical filters instead of six, and yy / xx no longer formed per pixel as the
// difference ig03 b1 + ig33 b5 of O(100) sums: that cancellation happens once, in double,
// inside qh.  A per-tile constant is subtracted before the sums and its exact contribution
// to yy and xx (dc * pk.kdch) is added back in the epilogue.
// PYR = 1 (with U8): the block also writes its part of pyramid scales 1 and 2 (exact half / quarter
// sizes) from the staged bytes, so those scales need neither their own launch nor their own pass
// over the frame; the staging then covers virtual rows ty0 - R - 1 .. and (border tiles) virtual
// columns tx0 - RP - 1 .. with true REFLECT_101 instead of stopping one line past the image.
// U8 = 1 fuses scale 0 of the pyramid (A1 at scale 1: convertTo + 3x3 [1/4,1/2,1/4] blur,
// REFLECT_101; the resize is the identity) into the tile load, so the full-resolution
// float image never exists in HBM.
#define RC_POLY_BLOCK 512

typedef float rc_f32x4 __attribute__((ext_vector_type(4)));

// NB consecutive staged bytes from any LDS byte address as floats: aligned dword reads, v_alignbyte,
// v_cvt_f32_ubyteN (a byte-wise read costs the LDS pipe as much as a dword).  Reads up to 3 bytes past
// the last one asked for: the staging area is followed by the rest of the block's LDS.
template <int NB>
__device__ __forceinline__ void rc_lds_bytes_f32(const unsigned char* p, float* b) {
    constexpr int NV = (NB + 3) / 4, ND = NV + 1;
    const unsigned sh = (unsigned)(size_t)p & 3u;
    const unsigned int* q = (const unsigned int*)(p - sh);
    unsigned int d[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) d[i] = q[i];
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const unsigned int v = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (4 * i + t < NB) b[4 * i + t] = (float)((v >> (8 * t)) & 255u);
    }
}

__device__ __forceinline__ float rc_lane_xor1(float v) {       // the value of lane ^ 1 (quad_perm [1,0,3,2])
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));
}

// The tile's outputs of pyramid scales 1 (32 x 16) and 2 (16 x 8) at exact 2:1 / 4:1 sizes.
//
// Scale 2 (9 float taps, sigma 1.5) from the staged bytes, in two steps that every thread of the block shares:
//   rc_pyr2_rows  the row filter at the 32 sampled columns (two per output) of the 38 source rows the tile's 8 output
//                 rows touch -> LDS [38][32]   (1216 row filters per tile; a thread per output pair used to evaluate
//                 14 of them on its own -- 1792 per tile on 128 threads while the other 384 waited at the barrier:
//                 that phase was 32 % of the block's lifetime by s_memtime stamps)
//   rc_pyr2_cols  128 threads: column filter at the two sampled rows, bilinear weights (0.5, 0.5), store.
// Operation order per output is rc_pyr_direct_body's / the oracle's (row filter, column filter, resize): same bits.
//
__device__ __forceinline__ void rc_pyr2_rows(const RcPolyArgs& a, const unsigned char* ub, int pitch, int row0, int col0,
                                             int tx0, int ty0, int tid, float* rp2) {
    const RcPyrFused& P = a.py[1];
    float k[9];
#pragma unroll
    for (int j = 0; j < 9; j++) k[j] = P.kern[j];
    // an item = the two sampled columns 4 ox + 1, 4 ox + 2 of output ox in one source row: their 9-tap windows share
    // eight of ten bytes, so the bytes are fetched and converted once for both filters (608 items per tile)
    for (int item = tid; item < 38 * 16; item += RC_POLY_BLOCK) {
        const int r = item >> 4, ox = item & 15;
        // source row ty0 - 3 + r; taps -4 .. +4 around columns tx0 + 4 ox + 1 and + 2
        const unsigned char* u0 = ub + (ty0 - 3 + r - row0) * pitch + (tx0 + 4 * ox + 1 - 4 - col0);
        float b[10];
        rc_lds_bytes_f32<10>(u0, b);
        float2 o;
        o.x = rc_rowpass<4>(b, k);
        o.y = rc_rowpass<4>(b + 1, k);
        *(float2*)(rp2 + r * 32 + 2 * ox) = o;
    }
}

__device__ __forceinline__ void rc_pyr2_cols(const RcPolyArgs& a, const float* rp2, int tx0, int ty0, int slot, int t) {
    const RcPyrFused& P = a.py[1];
    const float a0 = 1.f - 0.5f, a1 = 0.5f;
    const int ox = t & 15, oy = t >> 4;
    const int dx = (tx0 >> 2) + ox, dy = (ty0 >> 2) + oy;
    if (dx >= P.w || dy >= P.h) return;
    float k[9];
#pragma unroll
    for (int j = 0; j < 9; j++) k[j] = P.kern[j];
    // sampled rows 4 dy + 1 and + 2 -> rp2 rows 4 oy + 4 and + 5; sampled columns 2 ox and 2 ox + 1
    const float* c0 = rp2 + (4 * oy + 4) * 32 + 2 * ox;
    float b0 = k[4] * c0[0], o0 = k[4] * c0[1], b1 = k[4] * c0[32], o1 = k[4] * c0[33];
#pragma unroll
    for (int j = 1; j <= 4; j++) {
        b0 += k[4 + j] * (c0[j * 32] + c0[-j * 32]);
        o0 += k[4 + j] * (c0[j * 32 + 1] + c0[-j * 32 + 1]);
        b1 += k[4 + j] * (c0[(j + 1) * 32] + c0[(1 - j) * 32]);
        o1 += k[4 + j] * (c0[(j + 1) * 32 + 1] + c0[(1 - j) * 32 + 1]);
    }
    const float r0 = b0 * a0 + o0 * a1;
    const float r1 = b1 * a0 + o1 * a1;
    P.dst[(size_t)slot * P.dst_slot_stride + (size_t)dy * P.w + dx] = r0 * a0 + r1 * a1;
}

// Scale 1 (3 float taps of sigma 0.5 -- NOT the fixed 1/4 1/2 1/4 of scale 0, so the tile's blurred image cannot be
// reused): one thread per pair of vertically adjacent outputs (they share 4 of their 6 row-filter rows), 256 threads.
__device__ __forceinline__ void rc_pyr1_pairs(const RcPolyArgs& a, const unsigned char* ub, int pitch, int row0, int col0,
                                              int tx0, int ty0, int slot, int t1) {
    const float a0 = 1.f - 0.5f, a1 = 0.5f;
    const RcPyrFused& P = a.py[0];
    const int ox = t1 & 31, oyp = t1 >> 5;
    const int dx = (tx0 >> 1) + ox, dy = (ty0 >> 1) + 2 * oyp;
    // source samples (2 dx + 0.5, 2 dy + 0.5): columns 2dx, 2dx+1, rows 2dy, 2dy+1; 3 taps
    const unsigned char* u0 = ub + (ty0 + 4 * oyp - 1 - row0) * pitch + (tx0 + 2 * ox - 1 - col0);
    float k[3];
#pragma unroll
    for (int j = 0; j < 3; j++) k[j] = P.kern[j];
    float rp0[6], rp1[6];
#pragma unroll
    for (int rr = 0; rr < 6; rr++) {
        float b[4];
        rc_lds_bytes_f32<4>(u0 + rr * pitch, b);
        rp0[rr] = rc_rowpass<1>(b, k);
        rp1[rr] = rc_rowpass<1>(b + 1, k);
    }
#pragma unroll
    for (int e = 0; e < 2; e++) {
        float b00 = k[1] * rp0[2 * e + 1], b01 = k[1] * rp1[2 * e + 1];
        float b10 = k[1] * rp0[2 * e + 2], b11 = k[1] * rp1[2 * e + 2];
        b00 += k[2] * (rp0[2 * e + 2] + rp0[2 * e]);
        b01 += k[2] * (rp1[2 * e + 2] + rp1[2 * e]);
        b10 += k[2] * (rp0[2 * e + 3] + rp0[2 * e + 1]);
        b11 += k[2] * (rp1[2 * e + 3] + rp1[2 * e + 1]);
        if (dx < P.w && dy + e < P.h) {
            float r0 = b00 * a0 + b01 * a1;
            float r1 = b10 * a0 + b11 * a1;
            P.dst[(size_t)slot * P.dst_slot_stride + (size_t)(dy + e) * P.w + dx] = r0 * a0 + r1 * a1;
        }
    }
}

template <int R, int U8, int TH, int MFMA, int PYR = 0>
__device__ __forceinline__ void rc_polyexp_body(const RcPolyArgs& a, int bx, int by, int z, float* smf) {
    static_assert(!PYR || (U8 && TH == 32 && R >= 2), "fused pyramid: 8-bit scale 0, 64 x 32 tiles");
    constexpr int TW = 64, RP = (R + 3) & ~3;
    constexpr int INW = TW + 2 * RP, INH = TH + 2 * R;
    constexpr int NV = 4 + 2 * RP;
    constexpr int NDW = (INW + 8) / 4, UBW = 4 * NDW, UBH = INH + 2;   // u8 staging: pitch UBW bytes
    float* tin = smf;                // [INH][INW]
    float* hs = smf + INH * INW;     // [3][INH][TW]
    const int tid = threadIdx.x;
    const int tx0 = bx * TW, ty0 = by * TH;
    const int w = a.w, h = a.h;
    const int slot = (a.slot0 + z * a.zstep) % a.nslots;
    float dc;

    if constexpr (U8) {
        // the u8 staging area lives in hs: it is dead before the horizontal pass writes there
        unsigned char* ub = (unsigned char*)hs;                    // [UBH][UBW]
        float* rp2 = (float*)(ub + ((UBH * UBW + 15) & ~15));      // [38][32] scale-2 row-filter results (PYR)
        static_assert(!PYR || ((UBH * UBW + 15) & ~15) + 38 * 32 * 4 <= 3 * INH * TW * 4, "scale-2 rows fit the dead planes");
        const uint8_t* src = a.src8 + (size_t)z * a.src8_frame_stride;
        dc = (float)src[(size_t)min(ty0 + TH / 2, h - 1) * a.src8_step + min(tx0 + TW / 2, w - 1)];
        const int ylo = PYR ? ty0 - R - 1 : rc_clampi(ty0 - R, 0, h - 1) - 1;   // image (PYR: virtual) row of staging row 0
        const int xs = tx0 - RP - 4;                               // fast path: image column of staging byte 0
        const bool fast = xs >= 0 && xs + UBW <= w && ((((size_t)a.src8) | a.src8_step | a.src8_frame_stride) & 3) == 0;
        if (fast) {
            // Tile away from the left/right borders, 4-byte aligned rows: aligned dword loads
            // (rows reflected), then a 3x3 blur in exact integer arithmetic on packed 16-bit
            // pairs.  smooth.cpp's float row filter then column filter with (1/4, 1/2, 1/4) is
            // exact on u8 input (every intermediate is a multiple of 1/16 below 256), so
            // S / 16 with S = sum of the nine bytes weighted (1 2 1; 2 4 2; 1 2 1) has the same bits.
            constexpr int NLD = (UBH * NDW + RC_POLY_BLOCK - 1) / RC_POLY_BLOCK;
            unsigned int v[NLD];
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                int idx = tid + q * RC_POLY_BLOCK;
                int i = idx / NDW, j = idx - i * NDW;
                int sy = rc_reflect101(PYR ? ylo + i : min(ylo + i, h), h);
                v[q] = idx < UBH * NDW ? *(const unsigned int*)(src + (size_t)sy * a.src8_step + xs + 4 * j) : 0u;
            }
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                int idx = tid + q * RC_POLY_BLOCK;
                if (idx < UBH * NDW) ((unsigned int*)ub)[idx] = v[q];
            }
            __syncthreads();
            if constexpr (PYR) {
                // scale 2's row filters on every wave, then the block splits: two waves finish scale 2, four do scale
                // 1, and whoever is free takes the next 64 blur items from a shared counter
                if (a.npyr >= 2) {       // block-uniform
                    rc_pyr2_rows(a, ub, UBW, ylo, xs, tx0, ty0, tid, rp2);
                    __syncthreads();
                    if (tid >= RC_POLY_BLOCK - 128) rc_pyr2_cols(a, rp2, tx0, ty0, slot, tid - (RC_POLY_BLOCK - 128));
                    else if (tid >= RC_POLY_BLOCK - 384) rc_pyr1_pairs(a, ub, UBW, ylo, xs, tx0, ty0, slot, tid - (RC_POLY_BLOCK - 384));
                } else if (tid < 256) {
                    rc_pyr1_pairs(a, ub, UBW, ylo, xs, tx0, ty0, slot, tid);
                }
            }
            const float mdc = -dc;
            // Blur items (4 pixels each).  With the fused pyramid the waves have unequal work behind them (waves 6-7:
            // scale-2 columns, waves 2-5: scale 1, waves 0-1: nothing), so the items are dealt in eight slots of 128:
            // slots 0-3 to waves 0-1 (four items per thread), 4-5 to waves 2-5, 6-7 to waves 6-7.
            constexpr int NBLUR = INH * (INW / 4);
            static_assert(!PYR || NBLUR <= 1024, "eight slots of 128 blur items");
            const bool dealt = PYR && a.npyr >= 2;
            const int nit = !dealt ? (NBLUR + RC_POLY_BLOCK - 1) / RC_POLY_BLOCK : (tid < 128 ? 4 : (tid < 384 ? 1 : 2));
            const int it0 = !dealt ? tid : (tid < 128 ? tid : 384 + tid), its = !dealt ? RC_POLY_BLOCK : 128;
            for (int q = 0; q < nit; q++) {
                const int idx = it0 + q * its;
                if (idx < NBLUR) {
                int i = idx / (INW / 4), j4 = idx - i * (INW / 4);
                // tin(i, 4 j4 + p) is centred on staging byte 4 j4 + 4 + p of the row of image line gy
                int gy = rc_clampi(ty0 - R + i, 0, h - 1);
                const unsigned int* U = (const unsigned int*)ub + (gy - ylo - 1) * NDW + j4;
                unsigned int A = 0, B = 0, C = 0, D = 0;
#pragma unroll
                for (int t = 0; t < 3; t++) {
                    unsigned int d0 = U[t * NDW], d1 = U[t * NDW + 1], d2 = U[t * NDW + 2];
                    // bytes X0..X5 = d0.b3, d1.b0..b3, d2.b0 as 16-bit pairs (low, high)
                    unsigned int pa = __builtin_amdgcn_perm(d0, d1, 0x0c010c07u);   // (X0, X2)
                    unsigned int pb = __builtin_amdgcn_perm(d1, d1, 0x0c020c00u);   // (X1, X3)
                    unsigned int pc = __builtin_amdgcn_perm(d1, d1, 0x0c030c01u);   // (X2, X4)
                    unsigned int pd = __builtin_amdgcn_perm(d2, d1, 0x0c040c02u);   // (X3, X5)
                    const int sh = t == 1 ? 1 : 0;
                    A += pa << sh; B += pb << sh; C += pc << sh; D += pd << sh;
                }
                unsigned int o02 = A + 2 * B + C, o13 = B + 2 * C + D;
                float4 o;
                o.x = RC_FMA((float)(o02 & 0xffffu), 0.0625f, mdc);
                o.y = RC_FMA((float)(o13 & 0xffffu), 0.0625f, mdc);
                o.z = RC_FMA((float)(o02 >> 16), 0.0625f, mdc);
                o.w = RC_FMA((float)(o13 >> 16), 0.0625f, mdc);
                *(float4*)(tin + i * INW + 4 * j4) = o;
                }
            }
        } else {
            const int xlo = PYR ? tx0 - RP - 1 : rc_clampi(tx0 - RP, 0, w - 1) - 1;
            constexpr int UBWS = INW + 2;       // bytes used per staging row on this path
            constexpr int NLD = (UBH * UBWS + RC_POLY_BLOCK - 1) / RC_POLY_BLOCK;
            unsigned char v[NLD];
#pragma unroll
            for (int q = 0; q < NLD; q++) {     // all loads in flight before the first LDS store
                int idx = tid + q * RC_POLY_BLOCK;
                int i = idx / UBWS, j = idx - i * UBWS;
                int sy = rc_reflect101(PYR ? ylo + i : min(ylo + i, h), h), sx = rc_reflect101(PYR ? xlo + j : min(xlo + j, w), w);
                v[q] = idx < UBH * UBWS ? src[(size_t)sy * a.src8_step + sx] : 0;
            }
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                int idx = tid + q * RC_POLY_BLOCK;
                int i = idx / UBWS, j = idx - i * UBWS;
                if (idx < UBH * UBWS) ub[i * UBW + j] = v[q];
            }
            __syncthreads();
            if constexpr (PYR) {
                if (a.npyr >= 2) {
                    rc_pyr2_rows(a, ub, UBW, ylo, xlo, tx0, ty0, tid, rp2);
                    __syncthreads();
                    if (tid < 128) rc_pyr2_cols(a, rp2, tx0, ty0, slot, tid);
                    else if (tid < 384) rc_pyr1_pairs(a, ub, UBW, ylo, xlo, tx0, ty0, slot, tid - 128);
                } else if (tid < 256) {
                    rc_pyr1_pairs(a, ub, UBW, ylo, xlo, tx0, ty0, slot, tid);
                }
            }
            for (int idx = tid; idx < INH * INW; idx += RC_POLY_BLOCK) {
                int i = idx / INW, j = idx - i * INW;
                int gy = rc_clampi(ty0 - R + i, 0, h - 1), gx = rc_clampi(tx0 - RP + j, 0, w - 1);
                const unsigned char* S = ub + (gy - ylo) * UBW + (gx - xlo);
                // smooth.cpp: row filter then column filter, ksize 3, kernel (1/4, 1/2, 1/4)
                float r0 = (float)S[-UBW] * 0.5f + ((float)S[-UBW - 1] + (float)S[-UBW + 1]) * 0.25f;
                float r1 = (float)S[0] * 0.5f + ((float)S[-1] + (float)S[1]) * 0.25f;
                float r2 = (float)S[UBW] * 0.5f + ((float)S[UBW - 1] + (float)S[UBW + 1]) * 0.25f;
                float v = 0.5f * r1 + 0.25f * (r2 + r0);
                tin[idx] = v - dc;
            }
        }
    } else {
        const float* I = a.I + (size_t)slot * a.I_slot_stride;
        dc = I[(size_t)min(ty0 + TH / 2, h - 1) * w + min(tx0 + TW / 2, w - 1)];
        constexpr int NLD = (INH * INW + RC_POLY_BLOCK - 1) / RC_POLY_BLOCK;
        float v[NLD];
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            int idx = tid + q * RC_POLY_BLOCK;
            int i = idx / INW, j = idx - i * INW;
            int gy = rc_clampi(ty0 - R + i, 0, h - 1), gx = rc_clampi(tx0 - RP + j, 0, w - 1);
            v[q] = idx < INH * INW ? I[(size_t)gy * w + gx] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < NLD; q++) {
            int idx = tid + q * RC_POLY_BLOCK;
            if (idx < INH * INW) tin[idx] = v[q] - dc;
        }
    }
    __syncthreads();

    // horizontal pass: item = (row i, group of 4 pixels)
    for (int idx = tid; idx < INH * (TW / 4); idx += RC_POLY_BLOCK) {
        int i = idx / (TW / 4), g4 = idx - i * (TW / 4);
        float v[NV];
        // 16-byte LDS reads, forced: left to itself the compiler drops the two taps of the window it never uses
        // and fetches the other 18 floats as nine ds_read2_b32 at odd dword offsets -- a stride-4-dword pattern
        // that lands the wave's 64 lanes on 16 banks (4-way conflicts).  Measured: -1.2 % of the kernel.
        {
            const unsigned la = (unsigned)(size_t)((__attribute__((address_space(3))) float*)(tin + i * INW + 4 * g4));
            rc_f32x4 t[NV / 4];
#pragma unroll
            for (int q = 0; q < NV / 4; q++) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(t[q]) : "v"(la), "n"(16 * q));
            if constexpr (NV / 4 == 3) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]));
            else if constexpr (NV / 4 == 5) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]));
            else {
#pragma unroll
                for (int q = 0; q < NV / 4; q++) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[q]));
            }
#pragma unroll
            for (int q = 0; q < NV / 4; q++) { v[4 * q] = t[q].x; v[4 * q + 1] = t[q].y; v[4 * q + 2] = t[q].z; v[4 * q + 3] = t[q].w; }
        }
        float h0[4], h1[4], h2[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int c = RP + p;
            float s0 = v[c] * a.pk.g[0], s1 = 0.f, s2 = v[c] * a.pk.qh[0];
#pragma unroll
            for (int k = 1; k <= R; k++) {
                float sm = v[c + k] + v[c - k], df = v[c + k] - v[c - k];
                s0 = RC_FMA(sm, a.pk.g[k], s0);
                s1 = RC_FMA(df, a.pk.xga[k], s1);
                s2 = RC_FMA(sm, a.pk.qh[k], s2);
            }
            h0[p] = s0; h1[p] = s1; h2[p] = s2;
        }
        float4* o = (float4*)(hs + i * TW + 4 * g4);
        o[0] = make_float4(h0[0], h0[1], h0[2], h0[3]);
        o[INH * TW / 4] = make_float4(h1[0], h1[1], h1[2], h1[3]);
        o[2 * INH * TW / 4] = make_float4(h2[0], h2[1], h2[2], h2[3]);
    }
    __syncthreads();

    if constexpr (MFMA) {
        // ---- vertical pass on the matrix cores: Out(16 x 16) = T(16 x K) x In(K x 16) per wave, T the
        // banded Toeplitz matrix of a vertical filter (K = 16 + 2R rows in, rounded up to 4s).
        // v_mfma_f32_16x16x4_f32 is an exact f32 fmaf chain in k order, runs beside the VALU
        // (which is what bounds this kernel) and takes the 5 filter x plane products
        //   b3 = xga.h0  b5 = qh.h0 | b2 = g.h1  b6 = xgb.h1 | b4 = g.h2.
        // Lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; D: row 4 (l >> 4) + r, col l & 15.
        static_assert(TH == 32, "8 waves = 2 x 4 sub-tiles of 16 x 16");
        constexpr int KS = (16 + 2 * R + 3) / 4;
        float* wt = hs + 3 * INH * TW;                  // [4][2R+1] taps by offset -R..R: g, xga (odd), qh, xgb (odd)
        if (tid < 4 * (2 * R + 1)) {
            const int f4 = tid / (2 * R + 1), t = tid - f4 * (2 * R + 1), k = t < R ? R - t : t - R;
            const float odd = f4 == 1 ? a.pk.xga[k] : a.pk.xgb[k];
            wt[tid] = f4 == 0 ? a.pk.g[k] : (f4 == 2 ? a.pk.qh[k] : (t < R ? -odd : (t == R ? 0.f : odd)));
        }
        __syncthreads();
        const int lane = tid & 63, wv = tid >> 6;
        const int i = lane & 15, kk = lane >> 4;
        const int y0 = 16 * (wv >> 2), x0 = 16 * (wv & 3);
        rc_f32x4 c2 = {0, 0, 0, 0}, c3 = c2, c4 = c2, c5 = c2, c6 = c2;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const int t = 4 * s + kk - i;               // tap index of A[i][4s + kk]
            const bool on = (unsigned)t <= (unsigned)(2 * R);
            const float wg = on ? wt[t] : 0.f, wx = on ? wt[2 * R + 1 + t] : 0.f, wq = on ? wt[2 * (2 * R + 1) + t] : 0.f;
            const float wy = on ? wt[3 * (2 * R + 1) + t] : 0.f;
            const int row = min(y0 + 4 * s + kk, INH - 1);          // rows past the band have zero weight
            const float* bp = hs + row * TW + x0 + i;
            const float p0 = bp[0], p1 = bp[INH * TW], p2 = bp[2 * INH * TW];
            c3 = __builtin_amdgcn_mfma_f32_16x16x4f32(wx, p0, c3, 0, 0, 0);
            c5 = __builtin_amdgcn_mfma_f32_16x16x4f32(wq, p0, c5, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wg, p1, c2, 0, 0, 0);
            c6 = __builtin_amdgcn_mfma_f32_16x16x4f32(wy, p1, c6, 0, 0, 0);
            c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wg, p2, c4, 0, 0, 0);
        }
        const int gx = tx0 + x0 + i;
        if (gx < w) {
            float4* RA = a.RA + (size_t)slot * a.R_slot_stride;
            float* RB = a.RB + (size_t)slot * a.R_slot_stride;
            const float dck = (float)((double)dc * a.pk.kdch);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int gy = ty0 + y0 + 4 * kk + r;
                if (gy < h) {
                    float4 ra;
                    ra.x = c3[r];
                    ra.y = c2[r];
                    ra.z = c5[r] + dck;
                    ra.w = c4[r] + dck;
                    size_t p = (size_t)gy * w + gx;
                    RA[p] = ra;
                    RB[p] = c6[r];
                }
            }
        }
        return;
    }
    // vertical pass: lane = column, NR output rows per thread
    constexpr int NR = TH / (RC_POLY_BLOCK / 64);
    static_assert(NR * (RC_POLY_BLOCK / 64) == TH, "tile height must be a multiple of 8");
    const int x = tid & 63, o0 = (tid >> 6) * NR;
    constexpr int NW = NR + 2 * R;
    float b2[NR], b3[NR], b4[NR], b5[NR], b6[NR];
    {
        float c[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) c[q] = hs[(o0 + q) * TW + x];
#pragma unroll
        for (int o = 0; o < NR; o++) {
            float s3 = 0.f, s5 = c[o + R] * a.pk.qh[0];
#pragma unroll
            for (int k = 1; k <= R; k++) {
                float sm = c[o + R + k] + c[o + R - k], df = c[o + R + k] - c[o + R - k];
                s3 = RC_FMA(df, a.pk.xga[k], s3);
                s5 = RC_FMA(sm, a.pk.qh[k], s5);
            }
            b3[o] = s3; b5[o] = s5;
        }
    }
    {
        float c[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) c[q] = hs[INH * TW + (o0 + q) * TW + x];
#pragma unroll
        for (int o = 0; o < NR; o++) {
            float s2 = c[o + R] * a.pk.g[0], s6 = 0.f;
#pragma unroll
            for (int k = 1; k <= R; k++) {
                s2 = RC_FMA(c[o + R + k] + c[o + R - k], a.pk.g[k], s2);
                s6 = RC_FMA(c[o + R + k] - c[o + R - k], a.pk.xgb[k], s6);
            }
            b2[o] = s2; b6[o] = s6;
        }
    }
    {
        float c[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) c[q] = hs[2 * INH * TW + (o0 + q) * TW + x];
#pragma unroll
        for (int o = 0; o < NR; o++) {
            float s4 = c[o + R] * a.pk.g[0];
#pragma unroll
            for (int k = 1; k <= R; k++) s4 = RC_FMA(c[o + R + k] + c[o + R - k], a.pk.g[k], s4);
            b4[o] = s4;
        }
    }
    const int gx = tx0 + x;
    if (gx < w) {
        float4* RA = a.RA + (size_t)slot * a.R_slot_stride;
        float* RB = a.RB + (size_t)slot * a.R_slot_stride;
        // the removed constant's share of yy and xx (the odd filters do not see it), at the stored scale
        const float dck = (float)((double)dc * a.pk.kdch);
#pragma unroll
        for (int o = 0; o < NR; o++) {
            int gy = ty0 + o0 + o;
            if (gy < h) {
                float4 ra;
                ra.x = b3[o];
                ra.y = b2[o];
                ra.z = b5[o] + dck;
                ra.w = b4[o] + dck;
                size_t p = (size_t)gy * w + gx;
                // streaming stores: R is written once here and read by the flow kernels much later (the
                // batch's R does not fit the caches), and this kernel is bound by its writes (-1.4 % per pair)
                __builtin_nontemporal_store(ra.x, &RA[p].x); __builtin_nontemporal_store(ra.y, &RA[p].y);
                __builtin_nontemporal_store(ra.z, &RA[p].z); __builtin_nontemporal_store(ra.w, &RA[p].w);
                __builtin_nontemporal_store(b6[o], &RB[p]);
            }
        }
    }
}

template <int R, int U8, int TH, int MFMA, int PYR = 0>
__global__ __launch_bounds__(RC_POLY_BLOCK) void k_polyexp(RcPolyArgs a) {
    extern __shared__ __align__(16) float rc_poly_smem[];
    rc_polyexp_body<R, U8, TH, MFMA, PYR>(a, blockIdx.x, blockIdx.y, blockIdx.z, rc_poly_smem);
}

// The expansions of up to three scales of one frame (or a few) in ONE launch: scale 0 from the 8-bit
// frames (pyramid fused), scales 1 and 2 from their pyramid images.  The grids are independent and each
// is no bigger than the GPU for a frame or two, so the launch lasts about as long as its largest part
// instead of the sum of three.  Same tile code, same bits.
template <int R>
__global__ __launch_bounds__(RC_POLY_BLOCK) void k_polyexp_multi(RcPolyArgs a0, RcPolyArgs a1, RcPolyArgs a2, int n0, int n1,
                                                                 int gx0, int gy0, int gx1, int gy1, int gx2, int gy2) {
    extern __shared__ __align__(16) float rc_poly_smem[];
    int id = blockIdx.x;
    if (id < n0) {
        const int z = id / (gx0 * gy0), r = id - z * gx0 * gy0;
        rc_polyexp_body<R, 1, 32, 0>(a0, r % gx0, r / gx0, z, rc_poly_smem);
    } else if (id < n0 + n1) {
        id -= n0;
        const int z = id / (gx1 * gy1), r = id - z * gx1 * gy1;
        rc_polyexp_body<R, 0, 32, 0>(a1, r % gx1, r / gx1, z, rc_poly_smem);
    } else {
        id -= n0 + n1;
        const int z = id / (gx2 * gy2), r = id - z * gx2 * gy2;
        rc_polyexp_body<R, 0, 32, 0>(a2, r % gx2, r / gx2, z, rc_poly_smem);
    }
}

static_assert(3 * sizeof(RcPolyArgs) + 10 * sizeof(int) <= 4096, "k_polyexp_multi's arguments fit the kernel-argument segment");
template <int R>
static void launch_polyexp_multi_t(const RcPolyArgs* a, int nlev, int frames, hipStream_t s) {
    constexpr int RP = (R + 3) & ~3;
    constexpr int INW = 64 + 2 * RP, INH = 32 + 2 * R;
    constexpr size_t lds_hs = sizeof(float) * (3 * (size_t)INH * 64 + 4 * (2 * R + 1)), lds_ub = (size_t)(INH + 2) * (INW + 8);
    constexpr size_t lds = sizeof(float) * (size_t)INH * INW + (lds_hs > lds_ub ? lds_hs : lds_ub);
    RC_ALLOW_LDS((k_polyexp_multi<R>), lds);
    int gx[3] = {1, 1, 1}, gy[3] = {1, 1, 1}, n[3] = {0, 0, 0};
    for (int k = 0; k < nlev; k++) { gx[k] = (a[k].w + 63) / 64; gy[k] = (a[k].h + 31) / 32; n[k] = gx[k] * gy[k] * frames; }
    const RcPolyArgs& a2 = nlev > 2 ? a[2] : a[1];
    hipLaunchKernelGGL((k_polyexp_multi<R>), dim3(n[0] + n[1] + n[2]), dim3(RC_POLY_BLOCK), lds, s, a[0], a[1], a2, n[0], n[1],
                       gx[0], gy[0], gx[1], gy[1], gx[2], gy[2]);
}

// a[0] must be the 8-bit scale 0, a[1..nlev-1] float scales; nlev = 2 or 3; the default 32-row VALU tiles
int rc_polyexp_multi_ok(const RcPolyArgs* a, int nlev) {
    if (nlev < 2 || nlev > 3 || !a[0].src8 || a[0].tile_h != 32 || !a[0].valu_vertical) return 0;
    for (int k = 1; k < nlev; k++) if (a[k].src8 || a[k].pk.n_eff != a[0].pk.n_eff) return 0;
    const int n = a[0].pk.n_eff;
    return n == 3 || n == 5 || n == 7;
}
void rc_launch_polyexp_multi(const RcPolyArgs* a, int nlev, int frames, hipStream_t s) {
    const int n = a[0].pk.n_eff;
    if (n <= 3) launch_polyexp_multi_t<3>(a, nlev, frames, s);
    else if (n <= 5) launch_polyexp_multi_t<5>(a, nlev, frames, s);
    else launch_polyexp_multi_t<7>(a, nlev, frames, s);
}

template <int R, int U8, int TH, int MFMA, int PYR = 0>
static void launch_polyexp_th(const RcPolyArgs& a, int frames, hipStream_t s) {
    constexpr int RP = (R + 3) & ~3;
    constexpr int INW = 64 + 2 * RP, INH = TH + 2 * R;
    constexpr size_t lds_hs = sizeof(float) * (3 * (size_t)INH * 64 + 4 * (2 * R + 1)), lds_ub = (size_t)(INH + 2) * (INW + 8);
    constexpr size_t lds = sizeof(float) * (size_t)INH * INW + (lds_hs > lds_ub ? lds_hs : lds_ub);
    RC_ALLOW_LDS((k_polyexp<R, U8, TH, MFMA, PYR>), lds);
    dim3 grid((a.w + 63) / 64, (a.h + TH - 1) / TH, frames);
    hipLaunchKernelGGL((k_polyexp<R, U8, TH, MFMA, PYR>), grid, dim3(RC_POLY_BLOCK), lds, s, a);
}

template <int R, int U8>
static void launch_polyexp_t(const RcPolyArgs& a, int frames, hipStream_t s) {
    if constexpr (R <= 9) {
        if (a.tile_h == 48) { launch_polyexp_th<R, U8, 48, 0>(a, frames, s); return; }
    }
    if (a.valu_vertical) launch_polyexp_th<R, U8, 32, 0>(a, frames, s);
    else launch_polyexp_th<R, U8, 32, 1>(a, frames, s);
}

template <int U8>
static void launch_polyexp_u(const RcPolyArgs& a, int frames, hipStream_t s) {
    int n = a.pk.n_eff;
    if (n <= 3) launch_polyexp_t<3, U8>(a, frames, s);
    else if (n <= 5) launch_polyexp_t<5, U8>(a, frames, s);
    else if (n <= 7) launch_polyexp_t<7, U8>(a, frames, s);
    else if (n <= 8) launch_polyexp_t<8, U8>(a, frames, s);
    else if (n <= 9) launch_polyexp_t<9, U8>(a, frames, s);
    else if (n <= 12) launch_polyexp_t<12, U8>(a, frames, s);
    else if (n <= 16) launch_polyexp_t<16, U8>(a, frames, s);
    else if (n <= 24) launch_polyexp_t<24, U8>(a, frames, s);
    else launch_polyexp_t<32, U8>(a, frames, s);
}

// Scale-0 expansion that also writes pyramid scales 1 (and 2): see PYR above.  The caller checked
// rc_polyexp_pyr_ok and filled a.npyr / a.py.
int rc_polyexp_pyr_ok(const RcPolyArgs& a) {
    const int n = a.pk.n_eff;
    return a.src8 && a.tile_h == 32 && a.valu_vertical && (n == 3 || n == 5 || n == 7);
}

void rc_launch_polyexp(const RcPolyArgs& a, int frames, hipStream_t s) {
    if (a.npyr > 0) {
        const int n = a.pk.n_eff;
        if (n == 3) launch_polyexp_th<3, 1, 32, 0, 1>(a, frames, s);
        else if (n == 5) launch_polyexp_th<5, 1, 32, 0, 1>(a, frames, s);
        else launch_polyexp_th<7, 1, 32, 0, 1>(a, frames, s);
        return;
    }
    if (a.src8) launch_polyexp_u<1>(a, frames, s);
    else launch_polyexp_u<0>(a, frames, s);
}

// ===================================================================== test helpers
// sa / sb: the stored scale of the (y, x, yy, xx) / xy planes over upstream's R: 1/2 and 1/4 for
// the fast kernels, 1 for option "exact"; powers of two, so packing and unpacking are exact
__global__ void k_pack_R5(const float* R5, float4* RA, float* RB, int n, float sa, float sb) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        RA[i] = make_float4(R5[5 * i] * sa, R5[5 * i + 1] * sa, R5[5 * i + 2] * sa, R5[5 * i + 3] * sa);
        RB[i] = R5[5 * i + 4] * sb;
    }
}
__global__ void k_unpack_R5(const float4* RA, const float* RB, float* R5, int n, float ua, float ub) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float4 v = RA[i];
        R5[5 * i] = v.x * ua; R5[5 * i + 1] = v.y * ua; R5[5 * i + 2] = v.z * ua; R5[5 * i + 3] = v.w * ua;
        R5[5 * i + 4] = RB[i] * ub;
    }
}
void rc_launch_pack_R5(const float* R5, float4* RA, float* RB, int n, int fast_scale, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_R5, dim3((n + 255) / 256), dim3(256), 0, s, R5, RA, RB, n, fast_scale ? 0.5f : 1.f,
                       fast_scale ? 0.25f : 1.f);
}
void rc_launch_unpack_R5(const float4* RA, const float* RB, float* R5, int n, int fast_scale, hipStream_t s) {
    hipLaunchKernelGGL(k_unpack_R5, dim3((n + 255) / 256), dim3(256), 0, s, RA, RB, R5, n, fast_scale ? 2.f : 1.f,
                       fast_scale ? 4.f : 1.f);
}
