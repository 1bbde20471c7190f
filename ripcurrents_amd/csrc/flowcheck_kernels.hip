// flowcheck_kernels.hip -- the flow check: which vectors of a dense flow field mean anything?
//
// Per pixel the residual of the match the vector claims (the next frame sampled at the displaced position against the previous
// frame, in 1/4096 grey level), the same with no motion, the structure tensor of the previous frame, all summed over a clipped
// (2 r + 1)^2 box, and from those sums and the vector itself a set of flags: BAD, OUT, FLAT, RESID, NOGAIN, FB (round trip against
// a backward field) and FAST.  include/rcflow.h ("flow check") is the specification; tests/_flowcheck_ref.py states it in numpy and
// the kernel is held to that bit for bit: everything that decides is integer, the float results are double, operation by
// operation.  A computing push is two launches and nothing synchronises:
//   flowcheck@0  a block of RC_BLOCK threads owns a tile of FC_TW x FC_TH pixels.
//                1. the previous frame's bytes of the tile with a halo of r + 1, coordinates clamped to the picture (the replicated
//                   border of the gradient), into LDS;
//                2. for every pixel of the tile with a halo of r: the gradient from LDS, the vector from memory, quantised as the
//                   mean flow quantises it, the four bytes of the next frame at the displaced position straight from memory (the
//                   displacements are small and neighbouring: the gather sits in L2), res, |next - prev| and the OK bit: two
//                   words a pixel in LDS, zero outside the picture;
//                3. the box, separably: the row sums of gx^2, gy^2, gx gy, res and (|next - prev|, OK) packed, five words for
//                   every tile column and halo row, in LDS; the column sums slide down a thread's FC_ROWS rows in registers.  N is
//                   arithmetic;
//                4. the tests, the outputs asked for, the cell sums.  A lane's column, hence its cell column, does not change: it
//                   adds its rows' counts and vector sums in registers while the cell row stays, then adds what is not zero to the
//                   block's table in LDS (per-lane LDS atomics, as meanflow@0: ballots and wave sums where a wave lies in one
//                   cell column were 3 to 6 % slower at 1080p, profiles/flowcheck_kernel_summary.md); the block issues one 64-bit
//                   atomic per sum and cell it touched;
//   flowcheck@1  one block closes sums, records and summary and leaves every accumulator zero for the next push.  Closing in the
//                last-arriving block of flowcheck@0 instead (rc_hand_off_release: every block waits for its stores, releases and
//                draws a ticket, 2040 blocks at 1080p, each having just dirtied its outputs) took 118 us where the two launches
//                take 77 together at 1080p, radius 2 (profiles/flowcheck_kernel_summary.md).
// The held frame is a device-to-device copy of d_next behind the launch, on the slot's stream.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define FC_TW 64                       // a wave is a row of the tile
#define FC_TH 16
#define FC_ROWS (FC_TH * FC_TW / RC_BLOCK)       // consecutive rows a thread decides
static_assert(RC_BLOCK == 256 && FC_ROWS == 4, "a block is four waves, each FC_ROWS rows of FC_TW columns");
#define FC_LDS_CELLS 32                // cells of a block's footprint met in LDS.  A larger footprint (cells of a few pixels under a
                                       // tile of 64 x 16) adds straight to memory: every lane up to 10 agent-scope 64-bit atomics a cell
                                       // row, for cells a pixel high that is a pixel row, many lanes on one word where a cell is wider
                                       // than a pixel.  That path is held to the statement and NOT timed: a grid of tiny cells pays
                                       // for it, the grids a detector uses (30 x 30 on a frame) never take it
#define FC_WORDS 5                     // row-sum planes: a, b, c, R, (D | Nr << 16)
static_assert(sizeof(rc_flowcheck_cell) == 32 && sizeof(rc_flowcheck_params) == 64, "the records of include/rcflow.h have the sizes the mirrors give them");
static_assert(RC_FLOWCHECK_MAX_RADIUS == 7 && RC_FLOWCHECK_SUMS == 10 && RC_FLOWCHECK_SUMMARY == 10,
              "225 pixels a window: R < 2^28, the sum of |next - prev| < 2^16; a cell has 10 words");

// the block's LDS, carved from the dynamic region in multiples of 16 bytes (the radius sets the sizes)
struct FcLds {
    int EW, EH, PW, PH;                // the tile with a halo of r, and of r + 1
    unsigned pb, p0, p1, H, tab, bytes;
};
__host__ __device__ inline FcLds fc_lds(int r) {
    FcLds l;
    l.EW = FC_TW + 2 * r; l.EH = FC_TH + 2 * r; l.PW = l.EW + 2; l.PH = l.EH + 2;
    unsigned o = 0;
    l.pb = o; o += ((unsigned)(l.PW * l.PH) + 15u) & ~15u;
    l.p0 = o; o += ((unsigned)(l.EW * l.EH) * 4u + 15u) & ~15u;
    l.p1 = o; o += ((unsigned)(l.EW * l.EH) * 4u + 15u) & ~15u;
    l.H = o; o += (unsigned)(FC_WORDS * l.EH * FC_TW) * 4u;
    l.tab = o; o += FC_LDS_CELLS * RC_FLOWCHECK_SUMS * 8u;
    l.bytes = o;
    return l;
}

struct FcArgs {
    const uint8_t* next; size_t next_step;
    const uint8_t* prev; size_t prev_step;
    const float* flow; size_t flow_step;
    const float* back; size_t back_step;         // or null
    uint8_t* flags; size_t flags_step;           // each output or null; the steps in bytes
    uint8_t* mask; size_t mask_step;
    float* checked; size_t checked_step;
    float* resid; size_t resid_step;
    float* texture; size_t texture_step;
    uint8_t* pic; size_t pic_step;
    long long* acc;                              // [cells][RC_FLOWCHECK_SUMS], zero between pushes
    long long* summary; long long* sums; rc_flowcheck_cell* cells;        // the state's copy
    long long* summary2; long long* sums2; rc_flowcheck_cell* cells2;     // the caller's, or null
    int w, h, r, gx, gy, cw, ch;
    int tests, tex_min, gain_pm, fill_nan;
    long long res_q, fb_rel_q, fb_abs_q, smax2;
    long long computing, pushes;
};

// the mean flow's sample rule -> false for a BAD sample
__device__ __forceinline__ bool fc_quant(const float2 f, int& qx, int& qy) {
    const bool good = fabsf(f.x) < 500.0f && fabsf(f.y) < 500.0f;         // NaN and the infinities fail the comparison
    qx = good ? (int)rintf(f.x * 64.0f) : 0;
    qy = good ? (int)rintf(f.y * 64.0f) : 0;
    return good;
}

typedef __attribute__((address_space(3))) unsigned long long fc_lds_u64;   // the block's table, said to be in LDS: no flat atomic

// the colour of a flag, B | G << 8 | R << 16, by the index of the lowest set bit
__device__ __forceinline__ unsigned fc_colour(int bit) {
    switch (bit) {
        case 0: return 0xff00ffu;      // BAD    (255, 0, 255)
        case 1: return 0x808080u;      // OUT    (128, 128, 128)
        case 2: return 0x0000ffu;      // FLAT   (255, 0, 0)
        case 3: return 0xff0000u;      // RESID  (0, 0, 255)
        case 4: return 0xffa500u;      // NOGAIN (0, 165, 255)
        case 5: return 0xffff00u;      // FB     (0, 255, 255)
        default: return 0x00ff00u;     // FAST   (0, 255, 0)
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_fc_check(const FcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FcLds L = fc_lds(a.r);
    uint8_t* pb = smem + L.pb;
    unsigned* p0 = (unsigned*)(smem + L.p0);
    unsigned* p1 = (unsigned*)(smem + L.p1);
    int* H = (int*)(smem + L.H);
    long long* tab = (long long*)(smem + L.tab);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = a.r, w = a.w, h = a.h;
    const int xb = blockIdx.x * FC_TW, yb = blockIdx.y * FC_TH;           // inside the picture by the grid's size
    // the block's footprint in cells; the remainder columns and rows belong to the last cell
    const int cxa = min(xb / a.cw, a.gx - 1), cxb = min((min(xb + FC_TW, w) - 1) / a.cw, a.gx - 1);
    const int cya = min(yb / a.ch, a.gy - 1), cyb = min((min(yb + FC_TH, h) - 1) / a.ch, a.gy - 1);
    const int nx = cxb - cxa + 1, ntab = nx * (cyb - cya + 1);
    const bool lds = ntab <= FC_LDS_CELLS;
    if (lds)
        for (int i = tid; i < RC_FLOWCHECK_SUMS * ntab; i += RC_BLOCK) tab[i] = 0;
    // 1. the previous frame with a halo of r + 1, clamped
    for (int i = tid; i < L.PW * L.PH; i += RC_BLOCK) {
        const int py = i / L.PW, px = i - py * L.PW;
        const int sx = min(max(xb - r - 1 + px, 0), w - 1), sy = min(max(yb - r - 1 + py, 0), h - 1);
        pb[i] = a.prev[(size_t)sy * a.prev_step + sx];
    }
    __syncthreads();
    // 2. gradient, vector, gather, residuals
    for (int i = tid; i < L.EW * L.EH; i += RC_BLOCK) {
        const int ey = i / L.EW, ex = i - ey * L.EW;
        const int x = xb - r + ex, y = yb - r + ey;
        unsigned w0 = 0u, w1 = 0u;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const uint8_t* c = pb + (ey + 1) * L.PW + ex + 1;
            const int g = (int)c[0];
            const int dx = (int)c[1] - (int)c[-1], dy = (int)c[L.PW] - (int)c[-L.PW];
            w0 = ((unsigned)dx & 0xffffu) | ((unsigned)dy << 16);
            int qx, qy;
            const float2 f = *(const float2*)((const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x);
            if (fc_quant(f, qx, qy)) {
                const int X = 64 * x + qx, Y = 64 * y + qy;
                if (X >= 0 && Y >= 0 && X <= 64 * (w - 1) && Y <= 64 * (h - 1)) {
                    const int x0 = X >> 6, fx = X & 63, x1 = min(x0 + 1, w - 1);
                    const int y0 = Y >> 6, fy = Y & 63, y1 = min(y0 + 1, h - 1);
                    const uint8_t* n0 = a.next + (size_t)y0 * a.next_step;
                    const uint8_t* n1 = a.next + (size_t)y1 * a.next_step;
                    const int Wn = (64 - fx) * (64 - fy) * (int)n0[x0] + fx * (64 - fy) * (int)n0[x1] + (64 - fx) * fy * (int)n1[x0] +
                                   fx * fy * (int)n1[x1];
                    const int res = abs(Wn - 4096 * g);
                    const int d = abs((int)a.next[(size_t)y * a.next_step + x] - g);
                    w1 = (unsigned)res | ((unsigned)d << 20) | (1u << 28);
                }
            }
        }
        p0[i] = w0; p1[i] = w1;
    }
    __syncthreads();
    // 3. the row sums
    const int nk = 2 * r + 1, HP = L.EH * FC_TW;
    for (int i = tid; i < HP; i += RC_BLOCK) {
        const int ey = i >> 6, tx = i & 63;
        const int j0 = ey * L.EW + tx;
        int sa = 0, sb = 0, sc = 0, sr = 0, sd = 0;
        for (int k = 0; k < nk; k++) {
            const unsigned g = p0[j0 + k], v = p1[j0 + k];
            const int dx = (int)(short)(g & 0xffffu), dy = (int)g >> 16;
            sa += dx * dx; sb += dx * dy; sc += dy * dy;
            sr += (int)(v & 0xfffffu);
            sd += (int)((v >> 20) & 0xffu) + (int)((v >> 28) << 16);
        }
        H[i] = sa; H[HP + i] = sb; H[2 * HP + i] = sc; H[3 * HP + i] = sr; H[4 * HP + i] = sd;
    }
    __syncthreads();
    // 4. the column sums, the tests, the outputs, the cell sums
    const int x = xb + lane;
    const bool in_x = x < w;
    const int cx = in_x ? min(x / a.cw, a.gx - 1) : -1;
    long long cs[RC_FLOWCHECK_SUMS];
#pragma unroll
    for (int k = 0; k < RC_FLOWCHECK_SUMS; k++) cs[k] = 0;
    int cur_cy = -1;
    const auto flush = [&](int cy) {
#pragma unroll
        for (int k = 0; k < RC_FLOWCHECK_SUMS; k++) {
            const long long v = cs[k];
            cs[k] = 0;
            if (!v || cx < 0) continue;
            if (lds) __hip_atomic_fetch_add((fc_lds_u64*)(tab + RC_FLOWCHECK_SUMS * ((cy - cya) * nx + (cx - cxa)) + k), (unsigned long long)v,
                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else rc_acc_add(a.acc + RC_FLOWCHECK_SUMS * ((size_t)cy * a.gx + cx) + k, v);
        }
    };
    const int ty0 = wv * FC_ROWS;
    int sa = 0, sb = 0, sc = 0, sr = 0, sd = 0;
    for (int e = ty0; e < ty0 + nk; e++) {
        const int i = e * FC_TW + lane;
        sa += H[i]; sb += H[HP + i]; sc += H[2 * HP + i]; sr += H[3 * HP + i]; sd += H[4 * HP + i];
    }
    for (int j = 0; j < FC_ROWS; j++) {
        const int ty = ty0 + j, y = yb + ty;
        if (y >= h) break;                                    // the whole wave leaves
        if (j > 0) {                                          // the window moves a row down
            const int i0 = (ty - 1) * FC_TW + lane, i1 = (ty + nk - 1) * FC_TW + lane;
            sa += H[i1] - H[i0]; sb += H[HP + i1] - H[HP + i0]; sc += H[2 * HP + i1] - H[2 * HP + i0];
            sr += H[3 * HP + i1] - H[3 * HP + i0]; sd += H[4 * HP + i1] - H[4 * HP + i0];
        }
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) flush(cur_cy);
            cur_cy = cy;
        }
        int fl = 0, qx = 0, qy = 0;
        bool ok = false;
        float2 f = make_float2(0.f, 0.f);
        int N = 1, Nr = 0;
        long long R = 0, R0 = 0;
        int g = 0;
        if (in_x) {
            N = (min(x + r, w - 1) - max(x - r, 0) + 1) * (min(y + r, h - 1) - max(y - r, 0) + 1);
            g = (int)pb[(ty + r + 1) * L.PW + lane + r + 1];
            f = *(const float2*)((const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x);
            if (!fc_quant(f, qx, qy)) {
                fl = RC_FLOWCHECK_BAD;
            } else {
                const int X = 64 * x + qx, Y = 64 * y + qy;
                ok = X >= 0 && Y >= 0 && X <= 64 * (w - 1) && Y <= 64 * (h - 1);
                if (!ok) fl |= RC_FLOWCHECK_OUT;
                if (a.tests & RC_FLOWCHECK_FLAT) {
                    const long long t = (long long)a.tex_min * N, A = sa, C = sc, B = sb;
                    if (!(A + C >= 2 * t && (A - t) * (C - t) >= B * B)) fl |= RC_FLOWCHECK_FLAT;
                }
                const long long q2 = (long long)(qx * qx) + (long long)(qy * qy);
                if ((a.tests & RC_FLOWCHECK_FAST) && q2 > a.smax2) fl |= RC_FLOWCHECK_FAST;
                if (ok) {
                    Nr = sd >> 16; R = sr; R0 = 4096ll * (sd & 0xffff);
                    if ((a.tests & RC_FLOWCHECK_RESID) && R > a.res_q * Nr) fl |= RC_FLOWCHECK_RESID;
                    if ((a.tests & RC_FLOWCHECK_NOGAIN) && a.gain_pm > 0 && (qx | qy) != 0 && 1000 * R > (long long)a.gain_pm * R0) fl |= RC_FLOWCHECK_NOGAIN;
                    if ((a.tests & RC_FLOWCHECK_FB) && a.back) {
                        const int x0 = X >> 6, fx = X & 63, x1 = min(x0 + 1, w - 1);
                        const int y0 = Y >> 6, fy = Y & 63, y1 = min(y0 + 1, h - 1);
                        const char* b0 = (const char*)a.back + (size_t)y0 * a.back_step;
                        const char* b1 = (const char*)a.back + (size_t)y1 * a.back_step;
                        int ux[4], uy[4];
                        bool good = fc_quant(((const float2*)b0)[x0], ux[0], uy[0]);
                        good = fc_quant(((const float2*)b0)[x1], ux[1], uy[1]) && good;
                        good = fc_quant(((const float2*)b1)[x0], ux[2], uy[2]) && good;
                        good = fc_quant(((const float2*)b1)[x1], ux[3], uy[3]) && good;
                        if (!good) {
                            fl |= RC_FLOWCHECK_FB;
                        } else {
                            const int k00 = (64 - fx) * (64 - fy), k10 = fx * (64 - fy), k01 = (64 - fx) * fy, k11 = fx * fy;
                            const int bx = k00 * ux[0] + k10 * ux[1] + k01 * ux[2] + k11 * ux[3];
                            const int by = k00 * uy[0] + k10 * uy[1] + k01 * uy[2] + k11 * uy[3];
                            const long long bxr = rc_floor_div((long long)bx + 2048, 4096), byr = rc_floor_div((long long)by + 2048, 4096);
                            const long long ex = qx + bxr, ey = qy + byr;
                            const long long e2 = ex * ex + ey * ey, m2 = q2 + bxr * bxr + byr * byr;
                            if (1024 * e2 > a.fb_rel_q * m2 + a.fb_abs_q) fl |= RC_FLOWCHECK_FB;
                        }
                    }
                }
            }
        }
        const bool valid = in_x && fl == 0;
        // the cell sums
        if (in_x) {
            cs[0] += valid;
#pragma unroll
            for (int k = 0; k < 7; k++) cs[1 + k] += fl >> k & 1;
            if (valid) { cs[8] += qx; cs[9] += qy; }
        }
        if (!in_x) continue;
        // the outputs
        if (a.flags) a.flags[(size_t)y * a.flags_step + x] = (uint8_t)fl;
        if (a.mask) a.mask[(size_t)y * a.mask_step + x] = valid ? 255 : 0;
        if (a.checked) {
            const float fill = a.fill_nan ? __uint_as_float(0x7fc00000u) : 0.0f;
            *(float2*)((char*)a.checked + (size_t)y * a.checked_step + 8 * (size_t)x) = valid ? f : make_float2(fill, fill);
        }
        if (a.resid) {
            float2 o = make_float2(0.f, 0.f);
            if (ok) {
                const double den = 4096.0 * (double)Nr;
                o.x = (float)((double)R / den);
                o.y = (float)((double)R0 / den);
            }
            *(float2*)((char*)a.resid + (size_t)y * a.resid_step + 8 * (size_t)x) = o;
        }
        if (a.texture) {
            const double A = (double)sa, B = (double)sb, C = (double)sc;
            const double l = fmax(((A + C) - sqrt((A - C) * (A - C) + 4.0 * (B * B))) * 0.5, 0.);
            *(float*)((char*)a.texture + (size_t)y * a.texture_step + 4 * (size_t)x) = (float)(l / (double)N);
        }
        if (a.pic) {
            const unsigned c = valid ? (unsigned)g * 0x010101u : fc_colour(__builtin_ctz((unsigned)fl));
            uint8_t* d = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x;
            d[0] = (uint8_t)c; d[1] = (uint8_t)(c >> 8); d[2] = (uint8_t)(c >> 16);
        }
    }
    if (cur_cy >= 0) flush(cur_cy);
    __syncthreads();
    if (lds)
        for (int i = tid; i < RC_FLOWCHECK_SUMS * ntab; i += RC_BLOCK) {
            const long long val = tab[i];
            const int c = i / RC_FLOWCHECK_SUMS, k = i - RC_FLOWCHECK_SUMS * c;
            if (val) rc_acc_add(a.acc + RC_FLOWCHECK_SUMS * ((size_t)(cya + c / nx) * a.gx + (cxa + c % nx)) + k, val);
        }
}

// ============================================================================ flowcheck@1: sums, records, summary
// One block behind flowcheck@0 on the stream: it takes the cells' accumulators, which leaves every one zero for the next push
__global__ __launch_bounds__(RC_BLOCK) void k_fc_close(const FcArgs a) {
    __shared__ long long red[4 * 8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = a.w, h = a.h;
    long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = tid; c < a.gx * a.gy; c += RC_BLOCK) {
        long long s[RC_FLOWCHECK_SUMS];
#pragma unroll
        for (int k = 0; k < RC_FLOWCHECK_SUMS; k++) s[k] = rc_acc_take(a.acc + (size_t)RC_FLOWCHECK_SUMS * c + k);    // in flight together
#pragma unroll
        for (int k = 0; k < RC_FLOWCHECK_SUMS; k++) {
            a.sums[(size_t)RC_FLOWCHECK_SUMS * c + k] = s[k];
            if (a.sums2) a.sums2[(size_t)RC_FLOWCHECK_SUMS * c + k] = s[k];
        }
        const int ccx = c % a.gx, ccy = c / a.gx;
        const int pw = ccx == a.gx - 1 ? w - a.cw * (a.gx - 1) : a.cw, ph = ccy == a.gy - 1 ? h - a.ch * (a.gy - 1) : a.ch;
        rc_flowcheck_cell rec;
        memset(&rec, 0, sizeof(rec));
        rec.pixels = pw * ph; rec.valid = (int)s[0];
        rec.valid_pm = (int)(s[0] * 1000 / rec.pixels);
        if (s[0] == 0) {
            rec.flags = RC_FLOWCHECK_NONE_VALID;
        } else {
            rec.mean_x = (float)(((double)s[8] / 64.0) / (double)s[0]);
            rec.mean_y = (float)(((double)s[9] / 64.0) / (double)s[0]);
        }
        a.cells[c] = rec;
        if (a.cells2) a.cells2[c] = rec;
#pragma unroll
        for (int k = 0; k < 8; k++) tot[k] += s[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        tot[k] = rc_wave_sum_lane0(tot[k]);
        if (lane == 0) red[8 * wv + k] = tot[k];
    }
    __syncthreads();
    if (tid != 0) return;
    long long s[RC_FLOWCHECK_SUMMARY];
    for (int k = 0; k < 8; k++) s[k] = red[k] + red[8 + k] + red[16 + k] + red[24 + k];
    s[8] = a.computing; s[9] = a.pushes;
    for (int k = 0; k < RC_FLOWCHECK_SUMMARY; k++) {
        a.summary[k] = s[k];
        if (a.summary2) a.summary2[k] = s[k];
    }
}

// ============================================================================ host side
void rc_state_free(RcFlowcheck& v) {
    rc_buf_free(v.prev); rc_buf_free(v.acc); rc_buf_free(v.out);
    rc_fence_free(v.zf);
    v = RcFlowcheck();
}

// open and reset: the accumulators, the last push's outputs; no frame is held.  The push counts stay: they are since
// open, and a state that has just been opened has none
int rc_state_zero(RcSlot& s, RcFlowcheck& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.acc, &v.out});
    if (rc) return rc;
    v.held = false;
    return RC_OK;
}

static bool fc_in(double v, double lo, double hi) { return v >= lo && v <= hi; }     // NaN fails
static bool fc_settable(const rc_flowcheck_params& p) {
    return !(p.tests & ~RC_FLOWCHECK_TESTS) && p.tex_min >= 0 && p.tex_min <= 65025 && p.gain_pm >= 0 && p.gain_pm <= 1000 &&
           fc_in(p.res_max, 0., 255.) && fc_in(p.fb_rel, 0., 1.) && fc_in(p.fb_abs, 0., 500.) && fc_in(p.speed_max, 0., 1000.);
}
static const char* fc_settable_text = "tests a subset of RC_FLOWCHECK_TESTS, tex_min 0..65025, gain_pm 0..1000, res_max 0..255, fb_rel 0..1, "
                                      "fb_abs 0..500, speed_max 0..1000, all finite";

static size_t fc_cells(const RcFlowcheck& v) { return (size_t)v.prm.grid_x * v.prm.grid_y; }
// RcFlowcheck::out: summary 10 int64 in 128 bytes | sums [cells][RC_FLOWCHECK_SUMS] int64 | records [cells]
static long long* fc_out_summary(const RcFlowcheck& v) { return (long long*)v.out.p; }
static long long* fc_out_sums(const RcFlowcheck& v) { return (long long*)v.out.p + 16; }
static rc_flowcheck_cell* fc_out_cells(const RcFlowcheck& v) { return (rc_flowcheck_cell*)((long long*)v.out.p + 16 + fc_cells(v) * RC_FLOWCHECK_SUMS); }

extern "C" int rcflow_flowcheck_open(rc_ctx* ctx, int stream, int w, int h, const rc_flowcheck_params* prm) {
    static const char* who = "rcflow_flowcheck_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad field size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (prm->radius < 0 || prm->radius > RC_FLOWCHECK_MAX_RADIUS || (prm->flags != RC_FLOWCHECK_FILL_NAN && prm->flags != RC_FLOWCHECK_FILL_ZERO) ||
        !fc_settable(*prm)) {
        rc_set_error("%s: radius 0..%d, flags RC_FLOWCHECK_FILL_NAN or RC_FLOWCHECK_FILL_ZERO (exactly one), %s", who, RC_FLOWCHECK_MAX_RADIUS,
                     fc_settable_text);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d field (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcFlowcheck n;
    n.w = w; n.h = h; n.prm = *prm;
    RC_HIP(hipSetDevice(ctx->device));
    const size_t nc = fc_cells(n);
    rc = rc_buf_ensure(n.prev, (size_t)w * h);
    if (!rc) rc = rc_buf_ensure(n.acc, nc * RC_FLOWCHECK_SUMS * 8);
    if (!rc) rc = rc_buf_ensure(n.out, 128 + nc * (RC_FLOWCHECK_SUMS * 8 + sizeof(rc_flowcheck_cell)));
    return rc_state_install(*s, s->fc, n, rc);
}

extern "C" int rcflow_flowcheck_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_next, size_t next_step, const uint8_t* d_prev, size_t prev_step,
                                         const float* d_flow_xy, size_t flow_step, const float* d_back_xy, size_t back_step, uint8_t* d_flags,
                                         size_t flags_step, uint8_t* d_mask, size_t mask_step, float* d_checked, size_t checked_step,
                                         float* d_resid, size_t resid_step, float* d_texture, size_t texture_step, uint8_t* d_picture,
                                         size_t picture_step, rc_flowcheck_cell* d_cells, long long* d_sums, long long* d_summary) {
    static const char* who = "rcflow_flowcheck_push_dev";
    RcSlot* s; RcFlowcheck* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fc, who, s, vp)) return rc;
    RcFlowcheck& v = *vp;
    const int w = v.w, h = v.h;
    const size_t nc = fc_cells(v);
    if (!d_flow_xy) {                                         // the slot's resident field (rcflow_stream_flow_ptr), as rcflow_meanflow_push_dev
        if (!s->flow_w) { rc_set_error("%s: no flow field is resident on the slot yet", who); return RC_ESTATE; }
        if (s->flow_w != w || s->flow_h != h) {
            rc_set_error("%s: the resident flow field is %d x %d, the session %d x %d", who, s->flow_w, s->flow_h, w, h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)w * 8;
    }
    RcArgsN<13> ar(who, w, h);
    ar.image("d_next", d_next, next_step, 1, 1, RC_ARG_IN);
    ar.image("d_prev", d_prev, prev_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    ar.image("d_back_xy", d_back_xy, back_step, 8, 8, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_flags", d_flags, flags_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_checked", d_checked, checked_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_resid", d_resid, resid_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_texture", d_texture, texture_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_cells", d_cells, nc * sizeof(rc_flowcheck_cell), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_sums", d_sums, nc * RC_FLOWCHECK_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, RC_FLOWCHECK_SUMMARY * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    const bool compute = d_prev || v.held;
    if (!compute && v.pushes > 0) {
        rc_set_error("%s: d_prev is NULL and no frame is held (rcflow_flowcheck_reset forgot it): the push after a reset names both frames", who);
        return RC_ESTATE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const rc_flowcheck_params& q = v.prm;
    FcArgs a_close;
    if (compute) {
        FcArgs a;
        a.next = d_next; a.next_step = next_step;
        a.prev = d_prev ? d_prev : (const uint8_t*)v.prev.p; a.prev_step = d_prev ? prev_step : (size_t)w;
        a.flow = d_flow_xy; a.flow_step = flow_step; a.back = d_back_xy; a.back_step = back_step;
        a.flags = d_flags; a.flags_step = flags_step; a.mask = d_mask; a.mask_step = mask_step;
        a.checked = d_checked; a.checked_step = checked_step; a.resid = d_resid; a.resid_step = resid_step;
        a.texture = d_texture; a.texture_step = texture_step; a.pic = d_picture; a.pic_step = picture_step;
        a.acc = (long long*)v.acc.p;
        a.summary = fc_out_summary(v); a.sums = fc_out_sums(v); a.cells = fc_out_cells(v);
        a.summary2 = d_summary; a.sums2 = d_sums; a.cells2 = d_cells;
        a.w = w; a.h = h; a.r = q.radius; a.gx = q.grid_x; a.gy = q.grid_y; a.cw = w / q.grid_x; a.ch = h / q.grid_y;
        a.tests = q.tests; a.tex_min = q.tex_min; a.gain_pm = q.gain_pm; a.fill_nan = q.flags == RC_FLOWCHECK_FILL_NAN;
        a.res_q = (long long)floor(q.res_max * 4096.0);
        a.fb_rel_q = (long long)rint(q.fb_rel * 1024.0);
        a.fb_abs_q = (long long)floor(q.fb_abs * q.fb_abs * 4194304.0);
        const long long smax_q = (long long)floor(q.speed_max * 64.0);
        a.smax2 = smax_q * smax_q;
        a.computing = v.computing + 1; a.pushes = v.pushes + 1;
        const dim3 grid((w + FC_TW - 1) / FC_TW, (h + FC_TH - 1) / FC_TH);
        // the two frames and the field in, the backward field where given, the outputs asked for
        RcProfScope ps(ctx, s->cur, RC_K_FLOWCHECK, 0, (double)w * h * (10. + (d_back_xy ? 8. : 0.) + (d_flags ? 1. : 0.) + (d_mask ? 1. : 0.) +
                                                                        (d_checked ? 8. : 0.) + (d_resid ? 8. : 0.) + (d_texture ? 4. : 0.) +
                                                                        (d_picture ? 3. : 0.)));
        hipLaunchKernelGGL(k_fc_check, grid, dim3(RC_BLOCK), fc_lds(q.radius).bytes, s->cur, a);
        a_close = a;
    }
    if (compute) {
        const double nc8 = (double)nc * 8.;                   // the accumulators in and zero out, the sums and records out, once or twice
        RcProfScope ps(ctx, s->cur, RC_K_FLOWCHECK, 1, nc8 * (2. * RC_FLOWCHECK_SUMS + (RC_FLOWCHECK_SUMS + 4.) * (1. + (d_sums || d_cells ? 1. : 0.))));
        hipLaunchKernelGGL(k_fc_close, dim3(1), dim3(RC_BLOCK), 0, s->cur, a_close);
    }
    // the pushed frame is the next push's previous frame; the launch above has read the old one (stream order)
    RC_HIP(hipMemcpy2DAsync(v.prev.p, (size_t)w, d_next, next_step, (size_t)w, h, hipMemcpyDeviceToDevice, s->cur));
    RC_HIP(hipGetLastError());
    v.held = true;                                            // a launch that failed is not a push
    v.pushes++;
    if (compute) v.computing++;
    return RC_OK;
}

extern "C" int rcflow_flowcheck_read(rc_ctx* ctx, int stream, rc_flowcheck_cell* cells, long long* sums, long long summary[RC_FLOWCHECK_SUMMARY]) {
    RcSlot* s; RcFlowcheck* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fc, "rcflow_flowcheck_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = fc_cells(*vp);
    if (cells) RC_HIP(hipMemcpyAsync(cells, fc_out_cells(*vp), nc * sizeof(rc_flowcheck_cell), hipMemcpyDeviceToHost, s->cur));
    if (sums) RC_HIP(hipMemcpyAsync(sums, fc_out_sums(*vp), nc * RC_FLOWCHECK_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, fc_out_summary(*vp), RC_FLOWCHECK_SUMMARY * 8, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    if (summary) { summary[8] = vp->computing; summary[9] = vp->pushes; }     // a push that only copied, and a reset, change no word on the device
    return RC_OK;
}

extern "C" int rcflow_flowcheck_set(rc_ctx* ctx, int stream, int tests, int tex_min, double res_max, int gain_pm, double fb_rel, double fb_abs,
                                    double speed_max) {
    RcSlot* s; RcFlowcheck* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fc, "rcflow_flowcheck_set", s, vp)) return rc;
    rc_flowcheck_params p = vp->prm;
    p.tests = tests; p.tex_min = tex_min; p.res_max = res_max; p.gain_pm = gain_pm; p.fb_rel = fb_rel; p.fb_abs = fb_abs; p.speed_max = speed_max;
    if (!fc_settable(p)) {
        rc_set_error("rcflow_flowcheck_set: %s", fc_settable_text);
        return RC_EINVAL;
    }
    vp->prm = p;
    return RC_OK;
}

extern "C" int rcflow_flowcheck_info(rc_ctx* ctx, int stream, rc_flowcheck_info* info) {
    RcSlot* s; RcFlowcheck* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fc, "rcflow_flowcheck_info", s, vp)) return rc;
    const RcFlowcheck& v = *vp;
    if (!info) { rc_set_error("rcflow_flowcheck_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->launches_per_push = RC_FLOWCHECK_LAUNCHES;
    info->held = v.held ? 1 : 0;
    info->pushes = v.pushes; info->computing = v.computing;
    info->device_bytes = v.prev.bytes + v.acc.bytes + v.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_flowcheck_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::fc, "rcflow_flowcheck_reset"); }
extern "C" int rcflow_flowcheck_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::fc); }
