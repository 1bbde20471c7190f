// infill_kernels.hip -- the flow infill: the holes of a checked flow field filled from a pyramid of block sums.
//
// Pull-push: the sums of the known vectors and their count over 2 x 2, 4 x 4, ... 128 x 128 blocks (the pull), then from the
// coarsest level down every cell that holds enough known pixels takes its own mean and any other the 9/3/3/1 mix of its parents
// that have a value (the push).  include/rcflow.h ("flow infill") is the specification; tests/_infill_ref.py states it in numpy and
// the kernels are held to that bit for bit: everything is int32 in 1/64 pixel, the only float arithmetic is (float)F / 64.0f, which
// is exact, and the records' means in double.  A push is four launches (three with levels <= 4) and nothing synchronises:
//   infill@0  a block of RC_BLOCK threads owns a tile of IF_TW x IF_TH pixels: the class of every pixel, the held state, the value
//             plane q and the class plane (the age byte: with hold > 0 the push changes the state, so infill@2 cannot derive the
//             class from the input again); S_0 into LDS and S_1 .. S_4 of the tile from there: 256, 64, 16 and 4 cells
//   infill@1  one workgroup of IF_TOP threads, only with levels >= 5: the pull of levels 5..L from S_4 and the push of L..5,
//             looping over the cells of a level with a barrier between levels (2040 cells at level 5 of 1080p).  With the split at
//             level 4 (8160 cells to pull and to push) this launch took 33 us at 1080p, a third of the push
//   infill@2  the same tiles: the cells of levels 5 (or L, below 5) down to 1 that the tile's pixels can reach, in LDS (at most
//             6 x 5, 8 x 5, 12 x 6, 20 x 8 and 34 x 10), pushed there; then the pixels, every output and the cell sums as flowcheck@0
//             adds them (per lane while the cell row stays, the block's table in LDS, one 64-bit atomic per sum and cell)
//   infill@3  one block closes sums, records and summary and leaves every accumulator zero for the next push

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define IF_TW 64                       // a wave is a row of the tile
#define IF_TH 16
#define IF_ROWS (IF_TH * IF_TW / RC_BLOCK)
#define IF_TOP 1024                    // threads of infill@1
#define IF_SPLIT 5                     // infill@1 pushes down to this level, infill@2 from it: a tile of 64 x 16 pixels holds whole
                                       // cells up to level 4, so infill@0 pulls that far and the one workgroup starts at 2040 cells of 1080p
#define IF_LDS_CELLS 32                // cells of a block's footprint met in LDS, as FC_LDS_CELLS of flowcheck_kernels.hip
static_assert(RC_BLOCK == 256 && IF_ROWS == 4 && IF_TW == 64 && IF_TH == 16, "a block is four waves, each IF_ROWS rows of IF_TW columns");
static_assert(sizeof(rc_infill_cell) == 32 && sizeof(rc_infill_params) == 48, "the records of include/rcflow.h have the sizes the mirrors give them");
static_assert(RC_INFILL_MAX_LEVELS == 7 && RC_INFILL_SUMS == 8 && RC_INFILL_SUMMARY == 16, "4^7 * 32000 < 2^30: the sums are int32");

// the cells of level l + 1 that the cells lo..hi of level l look at lie in (lo >> 1) - 1 .. (hi >> 1) + 1: from a tile of 64 x 16
// pixels that is at most 34 x 10, 20 x 8, 12 x 6, 8 x 5 and 6 x 5 cells at levels 1 to 5
#define IF_R1 (34 * 10)
#define IF_R2 (20 * 8)
#define IF_R3 (12 * 6)
#define IF_R4 (8 * 5)
#define IF_R5 (6 * 5)
#define IF_RALL (IF_R1 + IF_R2 + IF_R3 + IF_R4 + IF_R5)

struct IfArgs {
    const float* flow; size_t flow_step;
    const uint8_t* valid; size_t valid_step;     // or null
    const uint8_t* domain; size_t domain_step;   // or null
    float* filled; size_t filled_step;           // each output or null; the steps in bytes
    uint8_t* source; size_t source_step;
    uint8_t* mask; size_t mask_step;
    uint8_t* pic; size_t pic_step;
    unsigned* q;                                 // [h][w] qx | qy << 16
    uint8_t* age;                                // [h][w] age + 1 modulo 256
    int4* S[RC_INFILL_MAX_LEVELS + 1];           // S[1..7]: (SX, SY, N, 0)
    int2* V[RC_INFILL_MAX_LEVELS + 1];           // V[5..7]: (Fx | Fy << 16, lev or -1)
    int lw[RC_INFILL_MAX_LEVELS + 1], lh[RC_INFILL_MAX_LEVELS + 1];
    long long* acc;                              // [cells][RC_INFILL_SUMS] | 8 by lev, zero between pushes
    long long* summary; long long* sums; rc_infill_cell* cells;           // the state's copy
    long long* summary2; long long* sums2; rc_infill_cell* cells2;        // the caller's, or null
    int w, h, L, min_known, hold, gx, gy, cw, ch, leave_nan;
    unsigned colour[RC_INFILL_MAX_LEVELS + 1];   // B | G << 8 | R << 16 of lev 1..7
    long long pushes;
};

// the mean flow's sample rule -> false for a BAD sample
__device__ __forceinline__ bool if_quant(const float2 f, int& qx, int& qy) {
    const bool good = fabsf(f.x) < 500.0f && fabsf(f.y) < 500.0f;         // NaN and the infinities fail the comparison
    qx = good ? (int)rintf(f.x * 64.0f) : 0;
    qy = good ? (int)rintf(f.y * 64.0f) : 0;
    return good;
}
__device__ __forceinline__ unsigned if_pack(int x, int y) { return ((unsigned)x & 0xffffu) | ((unsigned)y << 16); }
__device__ __forceinline__ int if_x(unsigned p) { return (int)(short)(p & 0xffffu); }
__device__ __forceinline__ int if_y(unsigned p) { return (int)p >> 16; }
// floor((2 a + b) / (2 b)), b > 0.  C's / truncates towards zero, the statement floors towards minus infinity: one less where the
// numerator is negative and the division is not exact.  |2 a + b| < 2^31 by the bound on the sums
__device__ __forceinline__ int if_rdiv(int a, int b) {
    const int n = 2 * a + b, d = 2 * b;
    const int q = n / d;
    return q - (n % d != 0 && n < 0);
}
// a cell's own value from its sums
__device__ __forceinline__ int2 if_own(const int4 s, int lev) { return make_int2((int)if_pack(if_rdiv(s.x, s.z), if_rdiv(s.y, s.z)), lev); }

// the 9/3/3/1 mix of the four entries of the level above; at(X, Y) -> (F packed, lev or -1) of a cell of that level, w1 x h1 cells
template <typename At>
__device__ __forceinline__ int2 if_mix(int x, int y, int w1, int h1, At at) {
    const int X0 = x >> 1, X1 = min(max(X0 + ((x & 1) ? 1 : -1), 0), w1 - 1);
    const int Y0 = y >> 1, Y1 = min(max(Y0 + ((y & 1) ? 1 : -1), 0), h1 - 1);
    const int2 e[4] = {at(X0, Y0), at(X1, Y0), at(X0, Y1), at(X1, Y1)};
    const int wt[4] = {9, 3, 3, 1};
    int A = 0, nx = 0, ny = 0, lev = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (e[k].y < 0) continue;
        A += wt[k];
        nx += wt[k] * if_x((unsigned)e[k].x);
        ny += wt[k] * if_y((unsigned)e[k].x);
        lev = max(lev, e[k].y);
    }
    if (A == 0) return make_int2(0, -1);
    return make_int2((int)if_pack(if_rdiv(nx, A), if_rdiv(ny, A)), lev);
}

// ============================================================================ infill@0: classes, held state, S_1..S_4
__global__ __launch_bounds__(RC_BLOCK) void k_if_pull(const IfArgs a) {
    __shared__ int s0[3][IF_TH * IF_TW];
    __shared__ int s1[3][256];
    __shared__ int s2[3][64];
    __shared__ int s3[3][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = a.w, h = a.h;
    const int xb = blockIdx.x * IF_TW, yb = blockIdx.y * IF_TH;           // inside the picture by the grid's size
    const int x = xb + lane;
#pragma unroll
    for (int j = 0; j < IF_ROWS; j++) {
        const int ty = wv * IF_ROWS + j, y = yb + ty;
        int vx = 0, vy = 0, have = 0;
        if (x < w && y < h) {
            const float2 f = *(const float2*)((const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x);
            const size_t i = (size_t)y * w + x;
            int qx, qy;
            const bool known = if_quant(f, qx, qy) && (!a.valid || a.valid[(size_t)y * a.valid_step + x] != 0);
            unsigned st = 0;                                  // a HOLE
            if (known) {
                vx = qx; vy = qy; have = 1; st = 1;
                a.q[i] = if_pack(qx, qy);
            } else if (a.hold > 0) {
                const int age = ((int)a.age[i] - 1) & 255;
                if (age < a.hold) {                           // HELD: hold <= 254, so the byte stays below 256
                    const unsigned p = a.q[i];
                    vx = if_x(p); vy = if_y(p); have = 1; st = (unsigned)age + 2u;
                }
            }
            a.age[i] = (uint8_t)st;
        }
        const int k = ty * IF_TW + lane;
        s0[0][k] = vx; s0[1][k] = vy; s0[2][k] = have;
    }
    __syncthreads();
    {   // level 1: 32 x 8 cells
        const int cx = tid & 31, cy = tid >> 5, k = 2 * cy * IF_TW + 2 * cx;
        int4 s = make_int4(0, 0, 0, 0);
        s.x = s0[0][k] + s0[0][k + 1] + s0[0][k + IF_TW] + s0[0][k + IF_TW + 1];
        s.y = s0[1][k] + s0[1][k + 1] + s0[1][k + IF_TW] + s0[1][k + IF_TW + 1];
        s.z = s0[2][k] + s0[2][k + 1] + s0[2][k + IF_TW] + s0[2][k + IF_TW + 1];
        s1[0][tid] = s.x; s1[1][tid] = s.y; s1[2][tid] = s.z;
        const int X = (xb >> 1) + cx, Y = (yb >> 1) + cy;
        if (X < a.lw[1] && Y < a.lh[1]) a.S[1][(size_t)Y * a.lw[1] + X] = s;
    }
    __syncthreads();
    if (tid < 64) {   // level 2: 16 x 4 cells
        const int cx = tid & 15, cy = tid >> 4, k = 2 * cy * 32 + 2 * cx;
        int4 s = make_int4(0, 0, 0, 0);
        s.x = s1[0][k] + s1[0][k + 1] + s1[0][k + 32] + s1[0][k + 33];
        s.y = s1[1][k] + s1[1][k + 1] + s1[1][k + 32] + s1[1][k + 33];
        s.z = s1[2][k] + s1[2][k + 1] + s1[2][k + 32] + s1[2][k + 33];
        s2[0][tid] = s.x; s2[1][tid] = s.y; s2[2][tid] = s.z;
        const int X = (xb >> 2) + cx, Y = (yb >> 2) + cy;
        if (X < a.lw[2] && Y < a.lh[2]) a.S[2][(size_t)Y * a.lw[2] + X] = s;
    }
    __syncthreads();
    if (tid < 16) {   // level 3: 8 x 2 cells
        const int cx = tid & 7, cy = tid >> 3, k = 2 * cy * 16 + 2 * cx;
        int4 s = make_int4(0, 0, 0, 0);
        s.x = s2[0][k] + s2[0][k + 1] + s2[0][k + 16] + s2[0][k + 17];
        s.y = s2[1][k] + s2[1][k + 1] + s2[1][k + 16] + s2[1][k + 17];
        s.z = s2[2][k] + s2[2][k + 1] + s2[2][k + 16] + s2[2][k + 17];
        const int X = (xb >> 3) + cx, Y = (yb >> 3) + cy;
        s3[0][tid] = s.x; s3[1][tid] = s.y; s3[2][tid] = s.z;
        if (X < a.lw[3] && Y < a.lh[3]) a.S[3][(size_t)Y * a.lw[3] + X] = s;
    }
    __syncthreads();
    if (tid < 4) {   // level 4: 4 x 1 cells
        const int k = 2 * tid;
        int4 s = make_int4(0, 0, 0, 0);
        s.x = s3[0][k] + s3[0][k + 1] + s3[0][k + 8] + s3[0][k + 9];
        s.y = s3[1][k] + s3[1][k + 1] + s3[1][k + 8] + s3[1][k + 9];
        s.z = s3[2][k] + s3[2][k + 1] + s3[2][k + 8] + s3[2][k + 9];
        const int X = (xb >> 4) + tid, Y = yb >> 4;
        if (X < a.lw[4] && Y < a.lh[4]) a.S[4][(size_t)Y * a.lw[4] + X] = s;
    }
}

// ============================================================================ infill@1: the pull of 5..L, the push of L..5
// One workgroup: what a thread stored before a barrier, every thread of the block reads after it
__global__ __launch_bounds__(IF_TOP) void k_if_top(const IfArgs a) {
    const int tid = threadIdx.x, L = a.L;
    for (int l = IF_SPLIT; l <= L; l++) {
        const int wl = a.lw[l], hl = a.lh[l], wc = a.lw[l - 1], hc = a.lh[l - 1];
        const int4* c = a.S[l - 1];
        for (int i = tid; i < wl * hl; i += IF_TOP) {
            const int Y = i / wl, X = i - Y * wl;
            const bool x1 = 2 * X + 1 < wc, y1 = 2 * Y + 1 < hc;
            const int4 z = make_int4(0, 0, 0, 0);
            const int4 s00 = c[(size_t)(2 * Y) * wc + 2 * X];
            const int4 s01 = x1 ? c[(size_t)(2 * Y) * wc + 2 * X + 1] : z;
            const int4 s10 = y1 ? c[(size_t)(2 * Y + 1) * wc + 2 * X] : z;
            const int4 s11 = x1 && y1 ? c[(size_t)(2 * Y + 1) * wc + 2 * X + 1] : z;
            a.S[l][i] = make_int4(s00.x + s01.x + s10.x + s11.x, s00.y + s01.y + s10.y + s11.y, s00.z + s01.z + s10.z + s11.z, 0);
        }
        __syncthreads();
    }
    for (int i = tid; i < a.lw[L] * a.lh[L]; i += IF_TOP) {
        const int4 s = a.S[L][i];
        a.V[L][i] = s.z >= a.min_known ? if_own(s, L) : make_int2(0, -1);
    }
    for (int l = L - 1; l >= IF_SPLIT; l--) {
        __syncthreads();
        const int wl = a.lw[l], hl = a.lh[l], w1 = a.lw[l + 1], h1 = a.lh[l + 1];
        const int2* up = a.V[l + 1];
        for (int i = tid; i < wl * hl; i += IF_TOP) {
            const int y = i / wl, x = i - y * wl;
            const int4 s = a.S[l][i];
            a.V[l][i] = s.z >= a.min_known ? if_own(s, l) : if_mix(x, y, w1, h1, [&](int X, int Y) { return up[(size_t)Y * w1 + X]; });
        }
    }
}

// ============================================================================ infill@2: the push to the pixels, the outputs
typedef __attribute__((address_space(3))) unsigned long long if_lds_u64;   // the block's table, said to be in LDS: no flat atomic

__global__ __launch_bounds__(RC_BLOCK) void k_if_push(const IfArgs a) {
    __shared__ int vf[IF_RALL], vl[IF_RALL];                  // F packed and lev (or -1) of the cells of levels 1..5 the tile reaches
    __shared__ long long tab[IF_LDS_CELLS * RC_INFILL_SUMS];
    __shared__ int hist[8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = a.w, h = a.h;
    const int xb = blockIdx.x * IF_TW, yb = blockIdx.y * IF_TH;
    const int cxa = min(xb / a.cw, a.gx - 1), cxb = min((min(xb + IF_TW, w) - 1) / a.cw, a.gx - 1);
    const int cya = min(yb / a.ch, a.gy - 1), cyb = min((min(yb + IF_TH, h) - 1) / a.ch, a.gy - 1);
    const int nx = cxb - cxa + 1, ntab = nx * (cyb - cya + 1);
    const bool lds = ntab <= IF_LDS_CELLS;
    if (lds)
        for (int i = tid; i < RC_INFILL_SUMS * ntab; i += RC_BLOCK) tab[i] = 0;
    if (tid < 8) hist[tid] = 0;
    // the regions: lo..hi of every level, the level's cells in vf / vl from off[l], rows of rw[l] cells
    const int top = min(a.L, IF_SPLIT);
    int lox[IF_SPLIT + 1], loy[IF_SPLIT + 1], rw[IF_SPLIT + 1], rh[IF_SPLIT + 1];
    const int off[IF_SPLIT + 1] = {0, 0, IF_R1, IF_R1 + IF_R2, IF_R1 + IF_R2 + IF_R3, IF_R1 + IF_R2 + IF_R3 + IF_R4};
    lox[0] = xb; loy[0] = yb; rw[0] = min(xb + IF_TW, w) - xb; rh[0] = min(yb + IF_TH, h) - yb;
#pragma unroll
    for (int l = 1; l <= IF_SPLIT; l++) {
        const int hx = min(((lox[l - 1] + rw[l - 1] - 1) >> 1) + 1, a.lw[l] - 1), hy = min(((loy[l - 1] + rh[l - 1] - 1) >> 1) + 1, a.lh[l] - 1);
        lox[l] = max((lox[l - 1] >> 1) - 1, 0); loy[l] = max((loy[l - 1] >> 1) - 1, 0);
        rw[l] = hx - lox[l] + 1; rh[l] = hy - loy[l] + 1;
    }
    // the top level: from infill@1 with levels above the split, else the level's own means
#pragma unroll
    for (int l = IF_SPLIT; l >= 1; l--) {
        if (l > top) continue;
        const int n = rw[l] * rh[l], wl = a.lw[l];
        for (int i = tid; i < n; i += RC_BLOCK) {
            const int ry = i / rw[l], rx = i - ry * rw[l];
            const int x = lox[l] + rx, y = loy[l] + ry;
            int2 v;
            if (l == IF_SPLIT) {
                v = a.V[IF_SPLIT][(size_t)y * wl + x];
            } else {
                const int4 s = a.S[l][(size_t)y * wl + x];
                if (s.z >= a.min_known) v = if_own(s, l);
                else if (l == top) v = make_int2(0, -1);
                else {
                    const int* pf = vf + off[l + 1]; const int* pl = vl + off[l + 1];
                    const int px = lox[l + 1], py = loy[l + 1], pw = rw[l + 1];
                    v = if_mix(x, y, a.lw[l + 1], a.lh[l + 1], [&](int X, int Y) { const int k = (Y - py) * pw + (X - px); return make_int2(pf[k], pl[k]); });
                }
            }
            vf[off[l] + i] = v.x; vl[off[l] + i] = v.y;
        }
        __syncthreads();
    }
    // the pixels
    const int x = xb + lane;
    const bool in_x = x < w;
    const int cx = in_x ? min(x / a.cw, a.gx - 1) : -1;
    long long cs[RC_INFILL_SUMS];
#pragma unroll
    for (int k = 0; k < RC_INFILL_SUMS; k++) cs[k] = 0;
    int cur_cy = -1;
    const auto flush = [&](int cy) {
#pragma unroll
        for (int k = 0; k < RC_INFILL_SUMS; k++) {
            const long long v = cs[k];
            cs[k] = 0;
            if (!v || cx < 0) continue;
            if (lds) __hip_atomic_fetch_add((if_lds_u64*)(tab + RC_INFILL_SUMS * ((cy - cya) * nx + (cx - cxa)) + k), (unsigned long long)v,
                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else rc_acc_add(a.acc + RC_INFILL_SUMS * ((size_t)cy * a.gx + cx) + k, v);
        }
    };
    const unsigned pattern = a.leave_nan ? 0x7fc00000u : 0u;
    for (int j = 0; j < IF_ROWS; j++) {
        const int y = yb + wv * IF_ROWS + j;
        if (y >= h) break;                                    // the whole wave leaves
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) flush(cur_cy);
            cur_cy = cy;
        }
        if (!in_x) continue;
        const size_t i = (size_t)y * w + x;
        const int st = (int)a.age[i];
        const bool wanted = !a.domain || a.domain[(size_t)y * a.domain_step + x] != 0;
        int src, Fx = 0, Fy = 0;
        if (st == 1) {
            const unsigned p = a.q[i];
            src = 0; Fx = if_x(p); Fy = if_y(p);
        } else if (!wanted) {
            src = RC_INFILL_OUTSIDE;
        } else if (st >= 2) {
            const unsigned p = a.q[i];
            src = RC_INFILL_HELD; Fx = if_x(p); Fy = if_y(p);
        } else {
            const int* pf = vf + off[1]; const int* pl = vl + off[1];
            const int px = lox[1], py = loy[1], pw = rw[1];
            const int2 v = if_mix(x, y, a.lw[1], a.lh[1], [&](int X, int Y) { const int k = (Y - py) * pw + (X - px); return make_int2(pf[k], pl[k]); });
            if (v.y < 0) src = RC_INFILL_UNFILLED;
            else { src = v.y; Fx = if_x((unsigned)v.x); Fy = if_y((unsigned)v.x); }
        }
        const bool valued = src <= RC_INFILL_HELD, is_filled = src >= 1 && src <= RC_INFILL_MAX_LEVELS;
        cs[0] += src == 0; cs[1] += src == RC_INFILL_HELD; cs[2] += is_filled; cs[3] += src == RC_INFILL_UNFILLED; cs[4] += src == RC_INFILL_OUTSIDE;
        if (valued) { cs[5] += Fx; cs[6] += Fy; }
        if (is_filled) {
            cs[7] += src;
            __hip_atomic_fetch_add(&hist[src], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // the outputs
        if (a.filled) {
            float2 o;
            if (src == 0) o = *(const float2*)((const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x);     // the input's bits
            else if (valued) o = make_float2((float)Fx / 64.0f, (float)Fy / 64.0f);
            else o = make_float2(__uint_as_float(pattern), __uint_as_float(pattern));
            *(float2*)((char*)a.filled + (size_t)y * a.filled_step + 8 * (size_t)x) = o;
        }
        if (a.source) a.source[(size_t)y * a.source_step + x] = (uint8_t)src;
        if (a.mask) a.mask[(size_t)y * a.mask_step + x] = valued ? 255 : 0;
        if (a.pic) {
            const unsigned c = src == 0 ? 0x404040u : src == RC_INFILL_HELD ? 0xffffffu : src == RC_INFILL_UNFILLED ? 0xff00ffu :
                               src == RC_INFILL_OUTSIDE ? 0u : a.colour[src];
            uint8_t* d = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x;
            d[0] = (uint8_t)c; d[1] = (uint8_t)(c >> 8); d[2] = (uint8_t)(c >> 16);
        }
    }
    if (cur_cy >= 0) flush(cur_cy);
    __syncthreads();
    if (lds)
        for (int i = tid; i < RC_INFILL_SUMS * ntab; i += RC_BLOCK) {
            const long long val = tab[i];
            const int c = i / RC_INFILL_SUMS, k = i - RC_INFILL_SUMS * c;
            if (val) rc_acc_add(a.acc + RC_INFILL_SUMS * ((size_t)(cya + c / nx) * a.gx + (cxa + c % nx)) + k, val);
        }
    if (tid < 8 && hist[tid]) rc_acc_add(a.acc + (size_t)RC_INFILL_SUMS * a.gx * a.gy + tid, (long long)hist[tid]);
}

// ============================================================================ infill@3: sums, records, summary
// One block behind infill@2 on the stream: it takes the accumulators, which leaves every one zero for the next push
__global__ __launch_bounds__(RC_BLOCK) void k_if_close(const IfArgs a) {
    __shared__ long long red[4 * 5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = a.w, h = a.h;
    long long tot[5] = {0, 0, 0, 0, 0};
    for (int c = tid; c < a.gx * a.gy; c += RC_BLOCK) {
        long long s[RC_INFILL_SUMS];
#pragma unroll
        for (int k = 0; k < RC_INFILL_SUMS; k++) s[k] = rc_acc_take(a.acc + (size_t)RC_INFILL_SUMS * c + k);    // in flight together
#pragma unroll
        for (int k = 0; k < RC_INFILL_SUMS; k++) {
            a.sums[(size_t)RC_INFILL_SUMS * c + k] = s[k];
            if (a.sums2) a.sums2[(size_t)RC_INFILL_SUMS * c + k] = s[k];
        }
        const int ccx = c % a.gx, ccy = c / a.gx;
        const int pw = ccx == a.gx - 1 ? w - a.cw * (a.gx - 1) : a.cw, ph = ccy == a.gy - 1 ? h - a.ch * (a.gy - 1) : a.ch;
        rc_infill_cell rec;
        memset(&rec, 0, sizeof(rec));
        const long long nv = s[0] + s[1] + s[2];
        rec.pixels = pw * ph;
        rec.known_pm = (int)(s[0] * 1000 / rec.pixels);
        rec.valued_pm = (int)(nv * 1000 / rec.pixels);
        if (nv == 0) {
            rec.flags = RC_INFILL_NONE;
        } else {
            rec.mean_x = (float)(((double)s[5] / 64.0) / (double)nv);
            rec.mean_y = (float)(((double)s[6] / 64.0) / (double)nv);
        }
        if (s[2]) rec.mean_level = (float)((double)s[7] / (double)s[2]);
        a.cells[c] = rec;
        if (a.cells2) a.cells2[c] = rec;
#pragma unroll
        for (int k = 0; k < 5; k++) tot[k] += s[k];
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        tot[k] = rc_wave_sum_lane0(tot[k]);
        if (lane == 0) red[5 * wv + k] = tot[k];
    }
    __syncthreads();
    if (tid >= RC_INFILL_SUMMARY) return;
    long long v = 0;
    if (tid < 5) v = red[tid] + red[5 + tid] + red[10 + tid] + red[15 + tid];
    else if (tid == 5) v = a.pushes;
    else if (tid >= 8) v = rc_acc_take(a.acc + (size_t)RC_INFILL_SUMS * a.gx * a.gy + (tid - 8));
    a.summary[tid] = v;
    if (a.summary2) a.summary2[tid] = v;
}

// ============================================================================ host side
void rc_state_free(RcInfill& v) {
    rc_buf_free(v.q); rc_buf_free(v.age); rc_buf_free(v.lev); rc_buf_free(v.acc); rc_buf_free(v.out);
    rc_fence_free(v.zf);
    v = RcInfill();
}

// open and reset: nothing is held (the age plane), the accumulators, the last push's outputs, the push count
int rc_state_zero(RcSlot& s, RcInfill& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.age, &v.acc, &v.out});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static bool if_settable(int levels, int min_known, int flags) {
    return levels >= 1 && levels <= RC_INFILL_MAX_LEVELS && min_known >= 1 && min_known <= RC_INFILL_MAX_MIN_KNOWN &&
           (flags == RC_INFILL_LEAVE_NAN || flags == RC_INFILL_LEAVE_ZERO);
}
static const char* if_settable_text = "levels 1..7, min_known 1..16384, flags RC_INFILL_LEAVE_NAN or RC_INFILL_LEAVE_ZERO (exactly one)";

static size_t if_cells(const RcInfill& v) { return (size_t)v.prm.grid_x * v.prm.grid_y; }
// RcInfill::out: summary 16 int64 | sums [cells][RC_INFILL_SUMS] int64 | records [cells]
static long long* if_out_summary(const RcInfill& v) { return (long long*)v.out.p; }
static long long* if_out_sums(const RcInfill& v) { return (long long*)v.out.p + RC_INFILL_SUMMARY; }
static rc_infill_cell* if_out_cells(const RcInfill& v) { return (rc_infill_cell*)((long long*)v.out.p + RC_INFILL_SUMMARY + if_cells(v) * RC_INFILL_SUMS); }

// the sizes of the levels and where each lies in RcInfill::lev -> the bytes of the whole
static size_t if_layout(int w, int h, int lw[], int lh[], size_t so[], size_t vo[]) {
    lw[0] = w; lh[0] = h;
    size_t o = 0;
    for (int l = 1; l <= RC_INFILL_MAX_LEVELS; l++) {
        lw[l] = (lw[l - 1] + 1) >> 1; lh[l] = (lh[l - 1] + 1) >> 1;
        so[l] = o; o += (size_t)lw[l] * lh[l] * sizeof(int4);
    }
    for (int l = IF_SPLIT; l <= RC_INFILL_MAX_LEVELS; l++) { vo[l] = o; o += (((size_t)lw[l] * lh[l] * sizeof(int2)) + 15) & ~(size_t)15; }
    return o;
}

extern "C" int rcflow_infill_open(rc_ctx* ctx, int stream, int w, int h, const rc_infill_params* prm) {
    static const char* who = "rcflow_infill_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad field size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    bool pad = false;
    for (int k = 0; k < 6; k++) pad = pad || prm->pad[k] != 0;
    if (!if_settable(prm->levels, prm->min_known, prm->flags) || prm->hold < 0 || prm->hold > RC_INFILL_MAX_HOLD || pad) {
        rc_set_error("%s: %s, hold 0..%d, the pad words zero", who, if_settable_text, RC_INFILL_MAX_HOLD);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d field (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcInfill n;
    n.w = w; n.h = h; n.prm = *prm;
    RC_HIP(hipSetDevice(ctx->device));
    const size_t nc = if_cells(n);
    int lw[RC_INFILL_MAX_LEVELS + 1], lh[RC_INFILL_MAX_LEVELS + 1];
    size_t so[RC_INFILL_MAX_LEVELS + 1], vo[RC_INFILL_MAX_LEVELS + 1];
    rc = rc_buf_ensure(n.q, (size_t)w * h * 4);
    if (!rc) rc = rc_buf_ensure(n.age, (size_t)w * h);
    if (!rc) rc = rc_buf_ensure(n.lev, if_layout(w, h, lw, lh, so, vo));
    if (!rc) rc = rc_buf_ensure(n.acc, (nc * RC_INFILL_SUMS + 8) * 8);
    if (!rc) rc = rc_buf_ensure(n.out, RC_INFILL_SUMMARY * 8 + nc * (RC_INFILL_SUMS * 8 + sizeof(rc_infill_cell)));
    return rc_state_install(*s, s->inf, n, rc);
}

extern "C" int rcflow_infill_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, const uint8_t* d_valid, size_t valid_step,
                                      const uint8_t* d_domain, size_t domain_step, float* d_filled, size_t filled_step, uint8_t* d_source,
                                      size_t source_step, uint8_t* d_mask, size_t mask_step, uint8_t* d_picture, size_t picture_step,
                                      rc_infill_cell* d_cells, long long* d_sums, long long* d_summary) {
    static const char* who = "rcflow_infill_push_dev";
    RcSlot* s; RcInfill* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::inf, who, s, vp)) return rc;
    RcInfill& v = *vp;
    const int w = v.w, h = v.h;
    const size_t nc = if_cells(v);
    if (!d_flow_xy) {                                         // the slot's resident field (rcflow_stream_flow_ptr), as rcflow_meanflow_push_dev
        if (!s->flow_w) { rc_set_error("%s: no flow field is resident on the slot yet", who); return RC_ESTATE; }
        if (s->flow_w != w || s->flow_h != h) {
            rc_set_error("%s: the resident flow field is %d x %d, the session %d x %d", who, s->flow_w, s->flow_h, w, h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)w * 8;
    }
    RcArgsN<10> ar(who, w, h);
    ar.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    ar.image("d_valid", d_valid, valid_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_domain", d_domain, domain_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_filled", d_filled, filled_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_source", d_source, source_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_cells", d_cells, nc * sizeof(rc_infill_cell), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_sums", d_sums, nc * RC_INFILL_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, RC_INFILL_SUMMARY * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const rc_infill_params& q = v.prm;
    IfArgs a;
    memset(&a, 0, sizeof(a));
    a.flow = d_flow_xy; a.flow_step = flow_step; a.valid = d_valid; a.valid_step = valid_step; a.domain = d_domain; a.domain_step = domain_step;
    a.filled = d_filled; a.filled_step = filled_step; a.source = d_source; a.source_step = source_step; a.mask = d_mask; a.mask_step = mask_step;
    a.pic = d_picture; a.pic_step = picture_step;
    a.q = (unsigned*)v.q.p; a.age = (uint8_t*)v.age.p;
    size_t so[RC_INFILL_MAX_LEVELS + 1], vo[RC_INFILL_MAX_LEVELS + 1];
    (void)if_layout(w, h, a.lw, a.lh, so, vo);
    for (int l = 1; l <= RC_INFILL_MAX_LEVELS; l++) a.S[l] = (int4*)((char*)v.lev.p + so[l]);
    for (int l = IF_SPLIT; l <= RC_INFILL_MAX_LEVELS; l++) a.V[l] = (int2*)((char*)v.lev.p + vo[l]);
    a.acc = (long long*)v.acc.p;
    a.summary = if_out_summary(v); a.sums = if_out_sums(v); a.cells = if_out_cells(v);
    a.summary2 = d_summary; a.sums2 = d_sums; a.cells2 = d_cells;
    a.w = w; a.h = h; a.L = q.levels; a.min_known = q.min_known; a.hold = q.hold;
    a.gx = q.grid_x; a.gy = q.grid_y; a.cw = w / q.grid_x; a.ch = h / q.grid_y; a.leave_nan = q.flags == RC_INFILL_LEAVE_NAN;
    uint8_t lut[768];
    rcflow_jet_lut(lut);
    for (int l = 1; l <= RC_INFILL_MAX_LEVELS; l++) {
        const uint8_t* c = lut + 3 * (l * 255 / 7);
        a.colour[l] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
    }
    a.pushes = v.pushes + 1;
    const dim3 grid((w + IF_TW - 1) / IF_TW, (h + IF_TH - 1) / IF_TH);
    const double px = (double)w * h;
    double lower = 0., upper = 0.;                            // the bytes of the levels below the split and from it on
    for (int l = 1; l <= RC_INFILL_MAX_LEVELS; l++) (l < IF_SPLIT ? lower : upper) += (double)a.lw[l] * a.lh[l] * 16.;
    {   // the field and the masks in, the value and class planes and S_1..S_4 out; the state in where something is held
        RcProfScope ps(ctx, s->cur, RC_K_INFILL, 0, px * (8. + (d_valid ? 1. : 0.) + 5. + (q.hold > 0 ? 5. : 0.)) + lower);
        hipLaunchKernelGGL(k_if_pull, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    if (q.levels >= IF_SPLIT) {
        RcProfScope ps(ctx, s->cur, RC_K_INFILL, 1, (double)a.lw[IF_SPLIT - 1] * a.lh[IF_SPLIT - 1] * 16. + 3. * upper);
        hipLaunchKernelGGL(k_if_top, dim3(1), dim3(IF_TOP), 0, s->cur, a);
    }
    {   // the planes and the levels in, the known vectors' bits again for d_filled, the outputs asked for
        RcProfScope ps(ctx, s->cur, RC_K_INFILL, 2, px * (5. + (d_domain ? 1. : 0.) + (d_filled ? 16. : 0.) + (d_source ? 1. : 0.) + (d_mask ? 1. : 0.) +
                                                          (d_picture ? 3. : 0.)) + lower);
        hipLaunchKernelGGL(k_if_push, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    {
        const double nc8 = (double)nc * 8.;                   // the accumulators in and zero out, the sums and records out, once or twice
        RcProfScope ps(ctx, s->cur, RC_K_INFILL, 3, nc8 * (2. * RC_INFILL_SUMS + (RC_INFILL_SUMS + 4.) * (1. + (d_sums || d_cells ? 1. : 0.))));
        hipLaunchKernelGGL(k_if_close, dim3(1), dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    v.pushes++;                                               // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_infill_read(rc_ctx* ctx, int stream, rc_infill_cell* cells, long long* sums, long long summary[RC_INFILL_SUMMARY]) {
    RcSlot* s; RcInfill* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::inf, "rcflow_infill_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = if_cells(*vp);
    if (cells) RC_HIP(hipMemcpyAsync(cells, if_out_cells(*vp), nc * sizeof(rc_infill_cell), hipMemcpyDeviceToHost, s->cur));
    if (sums) RC_HIP(hipMemcpyAsync(sums, if_out_sums(*vp), nc * RC_INFILL_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, if_out_summary(*vp), RC_INFILL_SUMMARY * 8, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_infill_set(rc_ctx* ctx, int stream, int levels, int min_known, int flags) {
    RcSlot* s; RcInfill* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::inf, "rcflow_infill_set", s, vp)) return rc;
    if (!if_settable(levels, min_known, flags)) {
        rc_set_error("rcflow_infill_set: %s", if_settable_text);
        return RC_EINVAL;
    }
    vp->prm.levels = levels; vp->prm.min_known = min_known; vp->prm.flags = flags;
    return RC_OK;
}

extern "C" int rcflow_infill_info(rc_ctx* ctx, int stream, rc_infill_info* info) {
    RcSlot* s; RcInfill* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::inf, "rcflow_infill_info", s, vp)) return rc;
    const RcInfill& v = *vp;
    if (!info) { rc_set_error("rcflow_infill_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->launches_per_push = v.prm.levels >= IF_SPLIT ? RC_INFILL_LAUNCHES : RC_INFILL_LAUNCHES - 1;
    info->pushes = v.pushes;
    info->device_bytes = v.q.bytes + v.age.bytes + v.lev.bytes + v.acc.bytes + v.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_infill_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::inf, "rcflow_infill_reset"); }
extern "C" int rcflow_infill_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::inf); }
