// kinematics_kernels.hip -- flow kinematics: how does the field turn and spread at a point?
//
// Vorticity, divergence and the Okubo-Weiss parameter of one flow field from central differences of a separably smoothed copy,
// the vortex cores (ow below a threshold, |omega| above one), and per cell of a grid the exact sums, the circulation and the
// core counts of either sign.  A rip's neck is a jet between two shear layers of opposite vorticity, its head a
// counter-rotating pair, its feeders converge.  include/rcflow.h ("flow kinematics") is the specification;
// tests/_kinematics_ref.py states it in numpy and the kernels are held to that bit for bit: nothing here is transcendental and
// the only square root is not taken (the threshold compares squares).  A push with an output is two launches and nothing
// synchronises:
//   kinematics@0  A tile is 64 columns and 4 * rpw rows, a wave one row of it at a time; a block walks as many tiles, one below the
//                 other, as keep the launch to about KN_MAX_BLOCKS blocks.  The float2 field with a
//                 halo of m = R + s goes into LDS (F), the horizontal pass into a second array (H, halo s left and right), the
//                 vertical pass back over F (S, halo s all round), and a pixel's four neighbours at +-s come out of S.  A wave
//                 reads and writes 64 consecutive float2 of one LDS row in every pass: ds_read_b64 banks over a 256-byte row
//                 per half wave and ds_write_b64 over a 128-byte row per 16 lanes, so any pitch is free of bank conflicts and
//                 the arrays are packed.  The cell sums: a lane's column, hence its cell column, does not
//                 change from row to row, so it adds in registers while the cell row stays; then the wave reduces per cell
//                 column, the block's waves meet in LDS and the block issues one 64-bit atomic per sum and cell it touched
//                 (the pattern of ripmap_kernels.hip).  The last-arriving block takes the threshold from the sums
//                 (rc_hand_off_release of rc_reduce.h: one release a block).  omega and ow go to
//                 two state planes, omega as one NaN pattern where the pixel is not valid.
//   kinematics@1  streams the two planes, a wave 64 columns of as many rows as keep the launch to about KN_MAX_BLOCKS blocks: cores,
//                 mask, picture, four more sums per cell the same way; the last-arriving block
//                 closes records and summary and leaves every counter zero for the next push.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define KN_WAVES 4
static_assert(RC_BLOCK == 64 * KN_WAVES, "a block is KN_WAVES waves");
#define KN_TW 64
#define KN_RPW 4               // rows a wave walks; 2 where the tile with the largest halos would not fit KN_LDS_MAX
#define KN_MAX_BLOCKS 512      // every block ends in a release and a ticket on one line, which the whole launch queues behind: a block of
                               // kinematics@0 walks as many tiles, a wave of kinematics@1 as many rows, as keep a launch to about this
#define KN_LDS_MAX 61440       // of the tile; the block's tables take the rest of 64 KiB
#define KN_LDS_CELLS 64        // cells of a block's footprint met in LDS; a larger footprint (cells of a few pixels) adds straight to memory
#define KN_NVALID 0x7fc00000u  // the omega plane where the pixel is not valid
#define KN_S0 7                // sums of kinematics@0, then the four of kinematics@1
#define KN_S1 4
static_assert(KN_S0 + KN_S1 == RC_KINEMATICS_SUMS, "include/rcflow.h promises RC_KINEMATICS_SUMS words per cell");
static_assert(sizeof(rc_kinematics_cell) == 48, "rc_kinematics_cell is 48 bytes");

// RcKinematics::ctl.  Each ticket has a 128-byte line of its own: every block adds to it.
struct KnCtl {
    RcTicketLine t0, t1;
    unsigned maxbits; unsigned pad2; double t2; unsigned pad3[28];
};
static_assert(sizeof(KnCtl) == 384, "three lines");

// Q(x) = (int64)rint((double)x * 65536).  A scaling by 2^16 is exact in float as well, so the float's rounding to an integer is
// the double's; |x| < 2^15 (omega, div, e, ow) fits 32 bits, w2 < 2^18 does not
__device__ __forceinline__ long long kn_q(float x) { return (long long)(int)rintf(x * 65536.0f); }
__device__ __forceinline__ long long kn_q_wide(float x) { return (long long)rintf(x * 65536.0f); }

// a block's footprint in cells and where its sums meet
struct KnFoot {
    int cxa, cxb, cya, cyb, nx, ntab;
    bool lds;
};
__device__ __forceinline__ KnFoot kn_foot(int xb, int yb, int th, int w, int h, int cw, int ch, int gx, int gy) {
    KnFoot f;
    f.cxa = min(xb / cw, gx - 1); f.cxb = min((min(xb + KN_TW, w) - 1) / cw, gx - 1);
    f.cya = min(yb / ch, gy - 1); f.cyb = min((min(yb + th, h) - 1) / ch, gy - 1);
    f.nx = f.cxb - f.cxa + 1;
    f.ntab = f.nx * (f.cyb - f.cya + 1);
    f.lds = f.ntab <= KN_LDS_CELLS;
    return f;
}

typedef __attribute__((address_space(3))) unsigned long long kn_lds_u64;   // the block's table, said to be in LDS: no flat atomic

// The wave's register sums of one cell row -> the block's table (or memory).  N sums from word `off` of a cell's
// RC_KINEMATICS_SUMS; cxl: the lane's cell column.  Every cell column of the footprint costs N 64-bit wave reductions, at every
// change of cell row: made for cells of tens of pixels (two or three columns a tile).  With cells of a few pixels it is up to 64
// columns a flush; what that costs has not been measured apart from the last block's walk over the cells, which at 16384
// cells sets a push's time whatever the picture (profiles/kinematics_kernel_summary.md: 0.6 to 0.8 ms)
template <int N>
__device__ __forceinline__ void kn_flush(long long* acc, int off, long long* tab, const KnFoot& f, int gx, int cy, int cxl, long long (&v)[N]) {
    for (int cx = f.cxa; cx <= f.cxb; cx++) {
        long long t[N];
#pragma unroll
        for (int k = 0; k < N; k++) t[k] = rc_wave_sum_all(cxl == cx ? v[k] : 0ll);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < N; k++) {
                if (!t[k]) continue;
                if (f.lds) __hip_atomic_fetch_add((kn_lds_u64*)(tab + N * ((cy - f.cya) * f.nx + (cx - f.cxa)) + k), (unsigned long long)t[k],
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else rc_acc_add(acc + RC_KINEMATICS_SUMS * ((size_t)cy * gx + cx) + off + k, t[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = 0;
}

// the block's table -> memory: one atomic per sum and cell the block touched
template <int N>
__device__ __forceinline__ void kn_table_out(long long* acc, int off, const long long* tab, const KnFoot& f, int gx) {
    if (!f.lds) return;
    for (int i = threadIdx.x; i < N * f.ntab; i += RC_BLOCK) {
        const long long val = tab[i];
        const int c = i / N, k = i - N * c;
        const int cy = f.cya + c / f.nx, cx = f.cxa + c % f.nx;
        if (val) rc_acc_add(acc + RC_KINEMATICS_SUMS * ((size_t)cy * gx + cx) + off + k, val);
    }
}

// ============================================================================ kinematics@0
struct KnArgs0 {
    const float* flow; size_t flow_step;
    float* omega; float* ow;             // the state's planes, [h][w]
    float* o_omega; size_t o_omega_step; // the caller's, or null
    float* o_div; size_t o_div_step;
    float* o_ow; size_t o_ow_step;
    KnCtl* ctl;
    long long* acc;                      // [cells][RC_KINEMATICS_SUMS], zero between pushes
    int w, h, s, rpw, tiles, gx, gy, cw, ch;   // a block walks `tiles` tiles, one below the other
    float g[RC_KINEMATICS_MAX_RADIUS + 1];
    float inv;
    int relative;
    double k2, t2_abs;                   // ow_k * ow_k; ow_min * ow_min
    unsigned nblocks;
};

template <int R>
__global__ __launch_bounds__(RC_BLOCK) void k_kn_field(const KnArgs0 a) {
    extern __shared__ float2 kn_lds[];
    __shared__ long long tab[KN_LDS_CELLS * KN_S0];
    __shared__ long long red[KN_WAVES * 3];
    __shared__ unsigned bmax;
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int s = a.s, m = R + s, th = KN_WAVES * a.rpw;
    const int x0 = blockIdx.x * KN_TW;
    const int FW = KN_TW + 2 * m, FH = th + 2 * m, HW = KN_TW + 2 * s, SH = th + 2 * s;
    float2* F = kn_lds;                  // [FH][FW]: the field from (x0 - m, y0 - m), zero outside the picture
    float2* H = kn_lds + FW * FH;        // [FH][HW]: the horizontal pass from (x0 - s, y0 - m)
    float2* S = kn_lds;                  // [SH][HW]: both passes from (x0 - s, y0 - s), over F once H is complete
    const int x = x0 + lane;
    const bool in = x < a.w, xin = x >= m && x < a.w - m;
    const int cxl = min(x / a.cw, a.gx - 1);
    unsigned mb = 0;
    if (threadIdx.x == 0) bmax = 0;
  for (int t = 0; t < a.tiles; t++) {
    const int y0 = (blockIdx.y * a.tiles + t) * th;
    if (y0 >= a.h) break;                                     // the whole block leaves
    const KnFoot f = kn_foot(x0, y0, th, a.w, a.h, a.cw, a.ch, a.gx, a.gy);
    if (f.lds)
        for (int i = threadIdx.x; i < KN_S0 * f.ntab; i += RC_BLOCK) tab[i] = 0;

    // nothing outside the picture is read.  What a window that leaves the picture gives is used by no interior pixel
    for (int r = wv; r < FH; r += KN_WAVES) {
        const int y = y0 - m + r;
        const bool rowok = y >= 0 && y < a.h;
        for (int c = lane; c < FW; c += 64) {
            const int fx = x0 - m + c;
            float2 v = make_float2(0.f, 0.f);
            if (rowok && fx >= 0 && fx < a.w) v = rc_row2(a.flow, a.flow_step, y)[fx];
            F[r * FW + c] = v;
        }
    }
    __syncthreads();
    for (int r = wv; r < FH; r += KN_WAVES)
        for (int c = lane; c < HW; c += 64) {
            const float2* p = F + r * FW + c + R;
            float hx = a.g[0] * p[0].x, hy = a.g[0] * p[0].y;
#pragma unroll
            for (int k = 1; k <= R; k++) {
                hx = hx + a.g[k] * (p[-k].x + p[k].x);
                hy = hy + a.g[k] * (p[-k].y + p[k].y);
            }
            H[r * HW + c] = make_float2(hx, hy);
        }
    __syncthreads();
    for (int r = wv; r < SH; r += KN_WAVES)
        for (int c = lane; c < HW; c += 64) {
            const float2* p = H + (r + R) * HW + c;
            float sx = a.g[0] * p[0].x, sy = a.g[0] * p[0].y;
#pragma unroll
            for (int k = 1; k <= R; k++) {
                sx = sx + a.g[k] * (p[-k * HW].x + p[k * HW].x);
                sy = sy + a.g[k] * (p[-k * HW].y + p[k * HW].y);
            }
            S[r * HW + c] = make_float2(sx, sy);
        }
    __syncthreads();

    long long v[KN_S0] = {0, 0, 0, 0, 0, 0, 0};              // n_valid, n_bad, Q(omega), Q(div), Q(e), Q(ow), Q(w2)
    int cur_cy = -1;
    for (int j = 0; j < a.rpw; j++) {
        const int ly = wv * a.rpw + j, y = y0 + ly;
        if (y >= a.h) break;                                  // the whole wave leaves
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) kn_flush<KN_S0>(a.acc, 0, tab, f, a.gx, cur_cy, cxl, v);
            cur_cy = cy;
        }
        const bool interior = xin && y >= m && y < a.h - m;
        const float2 E = S[(ly + s) * HW + lane + 2 * s], W = S[(ly + s) * HW + lane];
        const float2 So = S[(ly + 2 * s) * HW + lane + s], N = S[ly * HW + lane + s];
        const float ux = (E.x - W.x) * a.inv, vx = (E.y - W.y) * a.inv;
        const float uy = (So.x - N.x) * a.inv, vy = (So.y - N.y) * a.inv;
        const bool valid = interior && fabsf(ux) < 8.f && fabsf(vx) < 8.f && fabsf(uy) < 8.f && fabsf(vy) < 8.f;   // NaN fails
        float omega = 0.f, dv = 0.f, ow = 0.f;
        if (valid) {
            omega = vx - uy;
            dv = ux + vy;
            const float sn = ux - vy, ss = vx + uy;
            ow = (sn * sn + ss * ss) - omega * omega;
            const float e = omega * omega, w2 = ow * ow;
            v[0] += 1; v[2] += kn_q(omega); v[3] += kn_q(dv); v[4] += kn_q(e); v[5] += kn_q(ow); v[6] += kn_q_wide(w2);
            mb = max(mb, __float_as_uint(fabsf(omega)));      // non-negative floats order as integers
        } else if (interior) {
            v[1] += 1;
        }
        if (in) {
            const size_t o = (size_t)y * a.w + x;
            a.omega[o] = valid ? omega : __uint_as_float(KN_NVALID);
            a.ow[o] = ow;
            if (a.o_omega) ((float*)((char*)a.o_omega + (size_t)y * a.o_omega_step))[x] = omega;
            if (a.o_div) ((float*)((char*)a.o_div + (size_t)y * a.o_div_step))[x] = dv;
            if (a.o_ow) ((float*)((char*)a.o_ow + (size_t)y * a.o_ow_step))[x] = ow;
        }
    }
    if (cur_cy >= 0) kn_flush<KN_S0>(a.acc, 0, tab, f, a.gx, cur_cy, cxl, v);
    __syncthreads();
    kn_table_out<KN_S0>(a.acc, 0, tab, f, a.gx);
    __syncthreads();                                          // the next tile overwrites the table and the arrays
  }
    mb = rc_wave_max_all(mb);
    if (lane == 0 && mb) atomicMax(&bmax, mb);
    __syncthreads();
    if (threadIdx.x == 0 && bmax) __hip_atomic_fetch_max(&a.ctl->maxbits, bmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!rc_hand_off_release(&a.ctl->t0.ticket, a.nblocks, &last)) return;

    // the threshold, by the last-arriving block: the sums stay for kinematics@1
    long long n = 0, sw = 0, sw2 = 0;
    for (int c = threadIdx.x; c < a.gx * a.gy; c += RC_BLOCK) {
        long long* q = a.acc + (size_t)RC_KINEMATICS_SUMS * c;
        n += rc_acc_load(q); sw += rc_acc_load(q + 5); sw2 += rc_acc_load(q + 6);
    }
    n = rc_wave_sum_all(n); sw = rc_wave_sum_all(sw); sw2 = rc_wave_sum_all(sw2);
    if (lane == 0) { red[3 * wv] = n; red[3 * wv + 1] = sw; red[3 * wv + 2] = sw2; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    n = sw = sw2 = 0;
    for (int k = 0; k < KN_WAVES; k++) { n += red[3 * k]; sw += red[3 * k + 1]; sw2 += red[3 * k + 2]; }
    double t2 = a.t2_abs;
    if (a.relative) {
        double var = 0.;
        if (n > 0) {
            const double mean = ((double)sw / 65536.0) / (double)n;
            const double m2 = ((double)sw2 / 65536.0) / (double)n;
            var = m2 - mean * mean;
            if (!(var > 0.)) var = 0.;
        }
        t2 = a.k2 * var;
    }
    a.ctl->t2 = t2;                                           // read by the next launch (stream order)
    __hip_atomic_store(&a.ctl->t0.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================================ kinematics@1
struct KnArgs1 {
    const float* omega; const float* ow; // the state's planes
    uint8_t* mask; size_t mask_step;     // the caller's, or null
    uint8_t* vis; size_t vis_step;
    const uint8_t* jet;                  // 768 bytes
    KnCtl* ctl;
    long long* acc;
    long long* summary; long long* sums; rc_kinematics_cell* cells;       // the state's copy
    long long* summary2; long long* sums2; rc_kinematics_cell* cells2;    // the caller's, or null
    int w, h, rpw, gx, gy, cw, ch, min_core;
    float omega_min, vis_max;
    double pixel_area;
    long long pushes;
    unsigned nblocks;
};

__global__ __launch_bounds__(RC_BLOCK) void k_kn_cores(const KnArgs1 a) {
    __shared__ uint8_t lut[768];
    __shared__ long long tab[KN_LDS_CELLS * KN_S1];
    __shared__ long long red[KN_WAVES * 5];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int th = KN_WAVES * a.rpw;
    const int x0 = blockIdx.x * KN_TW, y0 = blockIdx.y * th;
    const KnFoot f = kn_foot(x0, y0, th, a.w, a.h, a.cw, a.ch, a.gx, a.gy);
    if (f.lds)
        for (int i = threadIdx.x; i < KN_S1 * f.ntab; i += RC_BLOCK) tab[i] = 0;
    if (a.vis)
        rc_stage_jet(lut, a.jet);
    __syncthreads();
    const double t2 = a.ctl->t2;
    const int x = x0 + lane;
    const bool in = x < a.w;
    const int cxl = min(x / a.cw, a.gx - 1);
    long long v[KN_S1] = {0, 0, 0, 0};                       // cores cw, cores ccw, Q(omega) over each
    int cur_cy = -1;
    for (int j = 0; j < a.rpw; j++) {
        const int y = y0 + wv * a.rpw + j;
        if (y >= a.h) break;
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) kn_flush<KN_S1>(a.acc, KN_S0, tab, f, a.gx, cur_cy, cxl, v);
            cur_cy = cy;
        }
        if (!in) continue;
        const size_t o = (size_t)y * a.w + x;
        const float omega = a.omega[o], ow = a.ow[o];
        const bool valid = omega == omega;
        const bool core = valid && ow < 0.f && (double)ow * (double)ow > t2 && fabsf(omega) >= a.omega_min;
        if (core && omega > 0.f) { v[0] += 1; v[2] += kn_q(omega); }
        if (core && omega < 0.f) { v[1] += 1; v[3] += kn_q(omega); }
        if (a.mask) a.mask[(size_t)y * a.mask_step + x] = core ? 255 : 0;
        if (a.vis) {
            uint8_t* q = a.vis + (size_t)y * a.vis_step + 3 * (size_t)x;
            if (valid) {
                const float t = rintf(omega / a.vis_max * 127.5f + 127.5f);
                const int i = !(t > 0.f) ? 0 : (t > 255.f ? 255 : (int)t);
                q[0] = lut[3 * i]; q[1] = lut[3 * i + 1]; q[2] = lut[3 * i + 2];
            } else {
                q[0] = 0; q[1] = 0; q[2] = 0;
            }
        }
    }
    if (cur_cy >= 0) kn_flush<KN_S1>(a.acc, KN_S0, tab, f, a.gx, cur_cy, cxl, v);
    __syncthreads();
    kn_table_out<KN_S1>(a.acc, KN_S0, tab, f, a.gx);
    if (!rc_hand_off_release(&a.ctl->t1.ticket, a.nblocks, &last)) return;

    // records and summary, by the last-arriving block; every counter is left zero for the next push
    long long tv = 0, tb = 0, tcw = 0, tccw = 0, both = 0;
    for (int c = threadIdx.x; c < a.gx * a.gy; c += RC_BLOCK) {
        long long w[RC_KINEMATICS_SUMS];
        for (int k = 0; k < RC_KINEMATICS_SUMS; k++) {
            w[k] = rc_acc_take(a.acc + (size_t)RC_KINEMATICS_SUMS * c + k);
            a.sums[(size_t)RC_KINEMATICS_SUMS * c + k] = w[k];
            if (a.sums2) a.sums2[(size_t)RC_KINEMATICS_SUMS * c + k] = w[k];
        }
        rc_kinematics_cell r;
        memset(&r, 0, sizeof(r));
        if (w[0] == 0) {
            r.flags = RC_KINEMATICS_EMPTY;
        } else {
            const double n = (double)w[0];
            r.flags = (w[7] >= a.min_core ? RC_KINEMATICS_CW : 0) | (w[8] >= a.min_core ? RC_KINEMATICS_CCW : 0);
            r.n = (int)w[0];
            r.bad = (int)w[1];
            r.mean_vorticity = (float)(((double)w[2] / 65536.0) / n);
            r.circulation = (float)(((double)w[2] / 65536.0) * a.pixel_area);
            r.mean_divergence = (float)(((double)w[3] / 65536.0) / n);
            r.enstrophy = (float)(((double)w[4] / 65536.0) / n);
            r.mean_ow = (float)(((double)w[5] / 65536.0) / n);
            r.cores_cw = (int)w[7];
            r.cores_ccw = (int)w[8];
            r.circulation_cw = (float)(((double)w[9] / 65536.0) * a.pixel_area);
            r.circulation_ccw = (float)(((double)w[10] / 65536.0) * a.pixel_area);
        }
        a.cells[c] = r;
        if (a.cells2) a.cells2[c] = r;
        tv += w[0]; tb += w[1]; tcw += w[7]; tccw += w[8];
        both += (r.flags & (RC_KINEMATICS_CW | RC_KINEMATICS_CCW)) == (RC_KINEMATICS_CW | RC_KINEMATICS_CCW);
    }
    tv = rc_wave_sum_all(tv); tb = rc_wave_sum_all(tb); tcw = rc_wave_sum_all(tcw); tccw = rc_wave_sum_all(tccw); both = rc_wave_sum_all(both);
    if (lane == 0) { red[5 * wv] = tv; red[5 * wv + 1] = tb; red[5 * wv + 2] = tcw; red[5 * wv + 3] = tccw; red[5 * wv + 4] = both; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < KN_WAVES; k++)
        for (int i = 0; i < 4; i++) r[i] += red[5 * k + i];
    r[4] = __double_as_longlong(t2);
    for (int k = 0; k < KN_WAVES; k++) r[5] += red[5 * k + 4];
    r[6] = a.pushes;
    r[7] = (long long)__hip_atomic_exchange(&a.ctl->maxbits, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int k = 0; k < 8; k++) {
        a.summary[k] = r[k];
        if (a.summary2) a.summary2[k] = r[k];
    }
    __hip_atomic_store(&a.ctl->t1.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next push (stream order)
}

// ============================================================================ host side
void rc_state_free(RcKinematics& k) {
    rc_buf_free(k.planes); rc_buf_free(k.acc); rc_buf_free(k.out); rc_buf_free(k.ctl); rc_buf_free(k.jet);
    rc_fence_free(k.zf);
    k = RcKinematics();
}

// open and reset: the sums, the tickets, the records and the summary; the push count.  The planes are written before they are read
int rc_state_zero(RcSlot& s, RcKinematics& k) {
    const int rc = rc_fence_zero(k.zf, s.cur, {&k.ctl, &k.acc, &k.out});
    if (rc) return rc;
    k.pushes = 0;
    return RC_OK;
}

static bool kn_pos(double v) { return v > 0. && v <= 1.7976931348623157e308; }       // finite and > 0; NaN fails
static bool kn_nonneg(double v) { return v >= 0. && v <= 1.7976931348623157e308; }   // finite and >= 0
static bool kn_settable(double ow_k, double ow_min, double omega_min, double vis_max) {
    return kn_nonneg(ow_k) && kn_nonneg(ow_min) && kn_nonneg(omega_min) && kn_pos(vis_max);
}
static size_t kn_cells(const RcKinematics& k) { return (size_t)k.prm.grid_x * k.prm.grid_y; }
// RcKinematics::out: summary 8 int64 | sums [cells][RC_KINEMATICS_SUMS] int64 | records [cells]
static long long* kn_out_summary(const RcKinematics& k) { return (long long*)k.out.p; }
static long long* kn_out_sums(const RcKinematics& k) { return (long long*)k.out.p + 8; }
static rc_kinematics_cell* kn_out_cells(const RcKinematics& k) { return (rc_kinematics_cell*)((long long*)k.out.p + 8 + kn_cells(k) * RC_KINEMATICS_SUMS); }

extern "C" int rcflow_kinematics_taps(int radius, double sigma, float* taps) {
    static const char* who = "rcflow_kinematics_taps";
    if (radius < 0 || radius > RC_KINEMATICS_MAX_RADIUS || !taps || (radius > 0 && !kn_pos(sigma))) {
        rc_set_error("%s: radius 0..%d, a buffer of radius + 1 floats, sigma finite and > 0", who, RC_KINEMATICS_MAX_RADIUS);
        return RC_EINVAL;
    }
    if (radius == 0) { taps[0] = 1.f; return RC_OK; }
    double e[RC_KINEMATICS_MAX_RADIUS + 1], t = 0.;
    for (int k = 0; k <= radius; k++) e[k] = exp(-(double)(k * k) / (2.0 * sigma * sigma));
    for (int k = 1; k <= radius; k++) t += e[k];
    const double Z = e[0] + 2.0 * t;
    for (int k = 0; k <= radius; k++) taps[k] = (float)(e[k] / Z);
    return RC_OK;
}

extern "C" int rcflow_kinematics_open(rc_ctx* ctx, int stream, int w, int h, const rc_kinematics_params* prm) {
    static const char* who = "rcflow_kinematics_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad field size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (prm->radius < 0 || prm->radius > RC_KINEMATICS_MAX_RADIUS || (prm->radius > 0 && !kn_pos(prm->sigma)) || prm->spacing < 1 ||
        prm->spacing > RC_KINEMATICS_MAX_SPACING || !kn_pos(prm->scale) || !kn_pos(prm->pixel_area) ||
        !kn_settable(prm->ow_k, prm->ow_min, prm->omega_min, prm->vis_max) || prm->min_core < 1 || (prm->flags & ~RC_KINEMATICS_RELATIVE)) {
        rc_set_error("%s: radius 0..%d, sigma finite and > 0, spacing 1..%d, scale, pixel_area and vis_max finite and > 0, ow_k, ow_min and "
                     "omega_min finite and >= 0, min_core >= 1, flags RC_KINEMATICS_RELATIVE or 0", who, RC_KINEMATICS_MAX_RADIUS,
                     RC_KINEMATICS_MAX_SPACING);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d field (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    const int m = prm->radius + prm->spacing;
    if (w < 2 * m + 1 || h < 2 * m + 1) {
        rc_set_error("%s: a field of %d x %d has no interior with radius + spacing = %d (at least %d x %d)", who, w, h, m, 2 * m + 1, 2 * m + 1);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    if ((long long)w * h > RC_KINEMATICS_MAX_PIXELS) {
        rc_set_error("%s: %d x %d is more than RC_KINEMATICS_MAX_PIXELS pixels", who, w, h);
        return RC_ESIZE;
    }
    RcKinematics n;
    n.w = w; n.h = h; n.prm = *prm;
    n.prm.pad[0] = n.prm.pad[1] = 0;
    if ((rc = rcflow_kinematics_taps(prm->radius, prm->sigma, n.taps))) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, nc = kn_cells(n);
    rc = rc_buf_ensure(n.planes, px * 8);
    if (!rc) rc = rc_buf_ensure(n.acc, nc * RC_KINEMATICS_SUMS * 8);
    if (!rc) rc = rc_buf_ensure(n.out, 64 + nc * (RC_KINEMATICS_SUMS * 8 + sizeof(rc_kinematics_cell)));
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(KnCtl));
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    return rc_state_install(*s, s->kn, n, rc);
}

template <int R>
static void kn_launch0(dim3 grid, size_t lds, hipStream_t st, const KnArgs0& a) {
    hipLaunchKernelGGL(k_kn_field<R>, grid, dim3(RC_BLOCK), lds, st, a);
}

extern "C" int rcflow_kinematics_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, float* d_omega, size_t omega_step,
                                          float* d_div, size_t div_step, float* d_ow, size_t ow_step, uint8_t* d_mask, size_t mask_step,
                                          uint8_t* d_vis, size_t vis_step, rc_kinematics_cell* d_cells, long long* d_sums, long long* d_summary) {
    static const char* who = "rcflow_kinematics_push_dev";
    RcSlot* s; RcKinematics* kp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::kn, who, s, kp)) return rc;
    RcKinematics& k = *kp;
    const int w = k.w, h = k.h;
    const size_t nc = kn_cells(k);
    RcArgsN<9> ar(who, w, h);
    ar.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    ar.image("d_omega", d_omega, omega_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_div", d_div, div_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_ow", d_ow, ow_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_vis", d_vis, vis_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_cells", d_cells, nc * sizeof(rc_kinematics_cell), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_sums", d_sums, nc * RC_KINEMATICS_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    const long long pushes = k.pushes + 1;
    if (!(d_omega || d_div || d_ow || d_mask || d_vis || d_cells || d_sums || d_summary)) {
        k.pushes = pushes;                                    // nothing is kept from push to push: there is nothing to queue
        return RC_OK;
    }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(k.zf, s->cur, true);
    if (rc) return rc;
    const rc_kinematics_params& p = k.prm;
    const double px = (double)w * h;
    const int R = p.radius, sp = p.spacing, m = R + sp;
    {
        KnArgs0 a;
        a.flow = d_flow_xy; a.flow_step = flow_step;
        a.omega = (float*)k.planes.p; a.ow = (float*)k.planes.p + (size_t)w * h;
        a.o_omega = d_omega; a.o_omega_step = omega_step; a.o_div = d_div; a.o_div_step = div_step; a.o_ow = d_ow; a.o_ow_step = ow_step;
        a.ctl = (KnCtl*)k.ctl.p; a.acc = (long long*)k.acc.p;
        a.w = w; a.h = h; a.s = sp; a.gx = p.grid_x; a.gy = p.grid_y; a.cw = w / p.grid_x; a.ch = h / p.grid_y;
        memcpy(a.g, k.taps, sizeof(a.g));
        a.inv = (float)(p.scale / (double)(2 * sp));
        a.relative = (p.flags & RC_KINEMATICS_RELATIVE) != 0;
        a.k2 = p.ow_k * p.ow_k; a.t2_abs = p.ow_min * p.ow_min;
        size_t lds = 0;
        for (a.rpw = KN_RPW; ; a.rpw = 2) {                   // the largest halos (m = 16) need the lower tile
            const int th = KN_WAVES * a.rpw;
            lds = ((size_t)(KN_TW + 2 * m) + (KN_TW + 2 * sp)) * (th + 2 * m) * sizeof(float2);
            if (lds <= KN_LDS_MAX || a.rpw == 2) break;
        }
        const int tx = (w + KN_TW - 1) / KN_TW, ty = (h + KN_WAVES * a.rpw - 1) / (KN_WAVES * a.rpw);
        a.tiles = (int)(((long long)tx * ty + KN_MAX_BLOCKS - 1) / KN_MAX_BLOCKS);
        const dim3 grid(tx, (ty + a.tiles - 1) / a.tiles);
        a.nblocks = grid.x * grid.y;
        // the field 8 in; the two planes 8 out, and the caller's
        RcProfScope ps(ctx, s->cur, RC_K_KINEMATICS, 0, px * (16. + (d_omega ? 4. : 0.) + (d_div ? 4. : 0.) + (d_ow ? 4. : 0.)));
        switch (R) {
            case 0: kn_launch0<0>(grid, lds, s->cur, a); break;
            case 1: kn_launch0<1>(grid, lds, s->cur, a); break;
            case 2: kn_launch0<2>(grid, lds, s->cur, a); break;
            case 3: kn_launch0<3>(grid, lds, s->cur, a); break;
            case 4: kn_launch0<4>(grid, lds, s->cur, a); break;
            case 5: kn_launch0<5>(grid, lds, s->cur, a); break;
            case 6: kn_launch0<6>(grid, lds, s->cur, a); break;
            case 7: kn_launch0<7>(grid, lds, s->cur, a); break;
            default: kn_launch0<8>(grid, lds, s->cur, a); break;
        }
    }
    {
        KnArgs1 a;
        a.omega = (const float*)k.planes.p; a.ow = (const float*)k.planes.p + (size_t)w * h;
        a.mask = d_mask; a.mask_step = mask_step; a.vis = d_vis; a.vis_step = vis_step;
        a.jet = (const uint8_t*)k.jet.p; a.ctl = (KnCtl*)k.ctl.p; a.acc = (long long*)k.acc.p;
        a.summary = kn_out_summary(k); a.sums = kn_out_sums(k); a.cells = kn_out_cells(k);
        a.summary2 = d_summary; a.sums2 = d_sums; a.cells2 = d_cells;
        a.w = w; a.h = h; a.gx = p.grid_x; a.gy = p.grid_y; a.cw = w / p.grid_x; a.ch = h / p.grid_y; a.min_core = p.min_core;
        a.omega_min = (float)p.omega_min; a.vis_max = (float)p.vis_max;
        a.pixel_area = p.pixel_area;
        a.pushes = pushes;
        const int tx = (w + KN_TW - 1) / KN_TW, ty = (h + KN_WAVES - 1) / KN_WAVES;
        a.rpw = (int)(((long long)tx * ty + KN_MAX_BLOCKS - 1) / KN_MAX_BLOCKS);
        const dim3 grid(tx, (ty + a.rpw - 1) / a.rpw);
        a.nblocks = grid.x * grid.y;
        RcProfScope ps(ctx, s->cur, RC_K_KINEMATICS, 1, px * (8. + (d_mask ? 1. : 0.) + (d_vis ? 3. : 0.)));
        hipLaunchKernelGGL(k_kn_cores, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    k.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_kinematics_read(rc_ctx* ctx, int stream, rc_kinematics_cell* cells, long long* sums, long long summary[8]) {
    RcSlot* s; RcKinematics* kp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::kn, "rcflow_kinematics_read", s, kp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(kp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = kn_cells(*kp);
    if (cells) RC_HIP(hipMemcpyAsync(cells, kn_out_cells(*kp), nc * sizeof(rc_kinematics_cell), hipMemcpyDeviceToHost, s->cur));
    if (sums) RC_HIP(hipMemcpyAsync(sums, kn_out_sums(*kp), nc * RC_KINEMATICS_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, kn_out_summary(*kp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_kinematics_set(rc_ctx* ctx, int stream, double ow_k, double ow_min, double omega_min, double vis_max) {
    RcSlot* s; RcKinematics* kp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::kn, "rcflow_kinematics_set", s, kp)) return rc;
    if (!kn_settable(ow_k, ow_min, omega_min, vis_max)) {
        rc_set_error("rcflow_kinematics_set: ow_k, ow_min and omega_min finite and >= 0, vis_max finite and > 0");
        return RC_EINVAL;
    }
    kp->prm.ow_k = ow_k; kp->prm.ow_min = ow_min; kp->prm.omega_min = omega_min; kp->prm.vis_max = vis_max;
    return RC_OK;
}

extern "C" int rcflow_kinematics_info(rc_ctx* ctx, int stream, rc_kinematics_info* info) {
    RcSlot* s; RcKinematics* kp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::kn, "rcflow_kinematics_info", s, kp)) return rc;
    const RcKinematics& k = *kp;
    if (!info) { rc_set_error("rcflow_kinematics_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = k.w; info->h = k.h; info->prm = k.prm;
    info->margin = k.prm.radius + k.prm.spacing;
    info->launches_per_push = RC_KINEMATICS_LAUNCHES;
    info->pushes = k.pushes;
    info->device_bytes = k.planes.bytes + k.acc.bytes + k.out.bytes + k.ctl.bytes + k.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_kinematics_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::kn, "rcflow_kinematics_reset"); }
extern "C" int rcflow_kinematics_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::kn); }
