// meanflow_kernels.hip -- the mean current: what does the water do on average over some wave periods, and how reliably?
//
// Per pixel a ring of the last `window` flow samples in 1/64 pixel (int16 u, int16 v) and seven exact sums over the valid entries
// held: their count n, Su, Sv, Suu, Svv, Suv and Sm, the sum of the floor magnitudes.  From them the mean vector, the steadiness
// |sum of vectors| / sum of magnitudes in per mille (1000: the flow never turns; wave orbital motion and noise are low), the major
// and minor standard deviation, and a mask of the pixels that are steady, fast enough and run the way asked for: along a fixed
// direction or against the picture's own mean vector.  A rip neck is such a place.  include/rcflow.h ("mean flow") is the
// specification; tests/_meanflow_ref.py states it in numpy and the kernels are held to that bit for bit: everything that decides
// is integer, the float results are double, operation by operation, and no angle is computed.  A push is two launches and nothing
// synchronises:
//   meanflow@0  a streaming read-modify-write.  The planes have a row pitch of w rounded up to 4.  A lane takes 4 consecutive
//               pixels of a row: the field two dwordx4, the ring slot, Su, Sv and Sm a dwordx4 each, Suu, Svv and Suv two each, n
//               a dwordx2.  A wave takes 256 columns and `rows` consecutive rows, a block MF_WAVES waves one below the other, and
//               `rows` keeps the launch to MF_MAX_BLOCKS0 blocks.  The ring slot is read and written once in `window` pushes and
//               goes past the caches (non-temporal); the sum planes come back with every push and do not.  A lane's columns,
//               hence its cells' columns, do not change from row to row: it adds its cells' sums in registers while the cell row
//               stays, then adds them to the block's table in LDS, where the block's waves meet, and the block issues one 64-bit
//               atomic per sum and cell it touched (the tables of ripmap_kernels.hip and kinematics_kernels.hip).  The
//               last-arriving block (rc_hand_off_release of rc_reduce.h) adds the cells' Su and Sv up to G;
//   meanflow@1  streams n, Su, Sv and Sm again, in up to MF_MAX_BLOCKS1 blocks: the mask, which needs G, and its count per cell the
//               same way; the last-arriving
//               block closes sums, records and summary and leaves every counter zero for the next push.
// The integer square roots start from a float estimate, one Newton step in integers for the 64-bit one, and are put right by
// stepping; the quotient of the steadiness likewise.  No FP64 square root runs per pixel unless the spread is asked for (the
// kernel's other instance); a cell's record takes one, in the last block.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define MF_WAVES 4
static_assert(RC_BLOCK == 64 * MF_WAVES, "a block is MF_WAVES waves, a run of rows each");
#define MF_PX 4                // pixels a lane takes
#define MF_TW (64 * MF_PX)     // columns a wave takes
#define MF_MAX_BLOCKS0 256     // of meanflow@0.  Every block ends in a wait for its stores, a release and a ticket on one line, and this
                               // launch has dirtied 46 bytes a pixel: caps of 256, 512, 1024 and 2048 gave 52, 59, 73 and 83 us at 1080p
#define MF_MAX_BLOCKS1 1024    // of meanflow@1, which writes a byte a pixel at most and gains from the waves in flight: the same caps
                               // gave 45, 37, 34 and 37 us (profiles/meanflow_kernel_summary.md; tests/test_gpu_meanflow.py names both)
#define MF_LDS_CELLS 256       // cells of a block's footprint met in LDS (16 KiB); a larger footprint (cells of a pixel or two) adds straight to memory
#define MF_BAD 0x00008000u     // the ring's word of a bad sample: u = -32768, which no good sample has (|q| <= 32000)
static_assert(sizeof(rc_meanflow_cell) == 32 && sizeof(rc_meanflow_params) == 56, "the records of include/rcflow.h have the sizes the mirrors give them");
static_assert(RC_MEANFLOW_MAX_WINDOW == 4096 && RC_MEANFLOW_SUMS == 8, "Su and Sv are int32 (4096 * 32000 < 2^31), n uint16; a cell has 8 words");

// RcMeanflow::ctl.  Each ticket has a 128-byte line of its own: every block adds to it.
struct MfCtl {
    RcTicketLine t0, t1;
    long long G[2]; unsigned pad[28];                         // of the last meanflow@0, read by meanflow@1 (stream order)
};
static_assert(sizeof(MfCtl) == 384, "three lines");

typedef float mf_f4 __attribute__((ext_vector_type(4), aligned(8)));      // two pixels of a 32FC2 row: rows are 8-byte aligned
typedef unsigned mf_u4 __attribute__((ext_vector_type(4)));
typedef int mf_i4 __attribute__((ext_vector_type(4)));
typedef long long mf_l2 __attribute__((ext_vector_type(2)));

// floor(sqrt(x)), x < 2^31 (a sample's u^2 + v^2 <= 2 * 32000^2): the float root is within one of it
__device__ __forceinline__ unsigned mf_isqrt32(unsigned x) {
    unsigned r = (unsigned)sqrtf((float)x);
    while (r * r > x) r--;
    while ((r + 1u) * (r + 1u) <= x) r++;
    return r;
}
// floor(sqrt(x)), 0 <= x < 2^56 (Su^2 + Sv^2 <= 2 * (4096 * 32000)^2): the float root is within 2^-23 of it, one Newton step in
// integers takes that to one or two, the steps do the rest
__device__ __forceinline__ long long mf_isqrt64(long long x) {
    long long r = (long long)sqrtf((float)x);
    if (r > 0) r += (long long)floorf((float)(x - r * r) / (2.f * (float)r));
    while (r * r > x) r--;
    while ((r + 1) * (r + 1) <= x) r++;
    return r;
}
// min(1000, floor(R * 1000 / Sm)), 0 where Sm = 0.  R < Sm below the early answers: the quotient is under 1000 and the float one
// within one of it
__device__ __forceinline__ unsigned mf_steady(long long R, unsigned Sm) {
    if (Sm == 0u) return 0u;
    if (R >= (long long)Sm) return 1000u;
    const long long num = R * 1000;
    long long q = (long long)((float)R * 1000.f / (float)Sm);
    if (q > 999) q = 999;
    while (q * (long long)Sm > num) q--;
    while ((q + 1) * (long long)Sm <= num) q++;
    return (unsigned)q;
}

// a block's footprint in cells and where its sums meet.  The remainder columns and rows belong to the last cell
struct MfFoot {
    int cxa, cxb, cya, cyb, nx, ntab;
    bool lds;
};
__device__ __forceinline__ MfFoot mf_foot(int xb, int yb, int th, int w, int h, int cw, int ch, int gx, int gy) {
    MfFoot f;
    f.cxa = min(xb / cw, gx - 1); f.cxb = min((min(xb + MF_TW, w) - 1) / cw, gx - 1);
    f.cya = min(yb / ch, gy - 1); f.cyb = min((min(yb + th, h) - 1) / ch, gy - 1);
    f.nx = f.cxb - f.cxa + 1;
    f.ntab = f.nx * (f.cyb - f.cya + 1);
    f.lds = f.ntab <= MF_LDS_CELLS;
    return f;
}

typedef __attribute__((address_space(3))) unsigned long long mf_lds_u64;   // the block's table, said to be in LDS: no flat atomic

// A lane's register sums of one cell row -> the block's table (or memory): N sums a pixel slot, sum k into word word[k] of a cell's
// RC_MEANFLOW_SUMS; cxl: the cell columns of the lane's pixels, ascending, -1 past the field.  A lane adds up the run of its slots
// that share a cell column and issues one atomic per run and sum: no lane waits for another.  (Reducing across the wave per cell
// column first, as ripmap_kernels.hip does, is a chain of dependent cross-lane moves per column and sum;
// profiles/meanflow_kernel_summary.md has both.)
template <int N>
__device__ __forceinline__ void mf_flush(long long* acc, long long* tab, const MfFoot& f, int gx, int cy, const int (&cxl)[MF_PX],
                                         long long (&v)[MF_PX][N], const int (&word)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        long long run = 0;
#pragma unroll
        for (int j = 0; j < MF_PX; j++) {
            run += v[j][k];
            v[j][k] = 0;
            if (j + 1 < MF_PX && cxl[j + 1] == cxl[j]) continue;
            if (run && cxl[j] >= 0) {
                if (f.lds) __hip_atomic_fetch_add((mf_lds_u64*)(tab + RC_MEANFLOW_SUMS * ((cy - f.cya) * f.nx + (cxl[j] - f.cxa)) + word[k]),
                                                  (unsigned long long)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else rc_acc_add(acc + RC_MEANFLOW_SUMS * ((size_t)cy * gx + cxl[j]) + word[k], run);
            }
            run = 0;
        }
    }
}

// the block's table -> memory: one atomic per sum and cell the block touched
__device__ __forceinline__ void mf_table_out(long long* acc, const long long* tab, const MfFoot& f, int gx) {
    if (!f.lds) return;
    for (int i = threadIdx.x; i < RC_MEANFLOW_SUMS * f.ntab; i += RC_BLOCK) {
        const long long val = tab[i];
        const int c = i / RC_MEANFLOW_SUMS, k = i - RC_MEANFLOW_SUMS * c;
        const int cy = f.cya + c / f.nx, cx = f.cxa + c % f.nx;
        if (val) rc_acc_add(acc + RC_MEANFLOW_SUMS * ((size_t)cy * gx + cx) + k, val);
    }
}

// ============================================================================ meanflow@0: ring, sums, pictures, cell sums, G
struct MfArgs0 {
    const float* flow; size_t flow_step;
    uint32_t* ring;                              // the slot pushes mod W of the ring, [h][P]: u | v << 16
    long long* Suu; long long* Svv; long long* Suv;           // [h][P] each
    int32_t* Su; int32_t* Sv; uint32_t* Sm; uint16_t* n;
    float* mean; size_t mean_step;               // each output or null; the steps in bytes
    uint16_t* steady; size_t steady_step;
    float* sd; size_t sd_step;
    uint8_t* pic; size_t pic_step;
    const uint8_t* jet;                          // 768 bytes
    MfCtl* ctl;
    long long* acc;                              // [cells][RC_MEANFLOW_SUMS], zero between pushes
    int w, h, P, rows, gx, gy, cw, ch;
    int have_old;                                // the ring has wrapped: the slot holds the sample of `window` pushes ago
    int min_fill;
    unsigned nblocks;
};

template <int SD>
__global__ __launch_bounds__(RC_BLOCK) void k_mf_pixels(const MfArgs0 a) {
    __shared__ long long tab[MF_LDS_CELLS * RC_MEANFLOW_SUMS];
    __shared__ long long red[MF_WAVES * 2];
    __shared__ uint8_t jet[768];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int th = MF_WAVES * a.rows;
    const int xb = blockIdx.x * MF_TW, yb = blockIdx.y * th;  // inside the field by the grid's size
    const MfFoot f = mf_foot(xb, yb, th, a.w, a.h, a.cw, a.ch, a.gx, a.gy);
    if (f.lds)
        for (int i = threadIdx.x; i < RC_MEANFLOW_SUMS * f.ntab; i += RC_BLOCK) tab[i] = 0;
    if (a.pic) rc_stage_jet(jet, a.jet);
    __syncthreads();
    const int x0 = xb + MF_PX * lane;
    const int nv = min(MF_PX, a.w - x0);                      // <= 0: the lane has no pixel; it stays for the barriers
    int cxl[MF_PX];
#pragma unroll
    for (int j = 0; j < MF_PX; j++) cxl[j] = j < nv ? min((x0 + j) / a.cw, a.gx - 1) : -1;
    const int word[6] = {0, 1, 2, 3, 4, 6};                   // filled pixels, n, Su, Sv, Sm over them; pixels whose newest sample was bad
    long long cs[MF_PX][6];
#pragma unroll
    for (int j = 0; j < MF_PX; j++)
#pragma unroll
        for (int k = 0; k < 6; k++) cs[j][k] = 0;
    int cur_cy = -1;
    const int y0 = yb + wv * a.rows;
    for (int r = 0; r < a.rows; r++) {
        const int y = y0 + r;
        if (y >= a.h) break;                                  // the whole wave leaves
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) mf_flush<6>(a.acc, tab, f, a.gx, cur_cy, cxl, cs, word);
            cur_cy = cy;
        }
        if (nv <= 0) continue;
        // 1. the field and the state: P - w < 4, so a lane with a pixel has its 4 places in every plane
        const size_t o = (size_t)y * a.P + x0;
        float fl[2 * MF_PX] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const char* fr = (const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x0;
        if (nv == MF_PX) {
            const mf_f4 t0 = __builtin_nontemporal_load((const mf_f4*)fr), t1 = __builtin_nontemporal_load((const mf_f4*)(fr + 16));
            fl[0] = t0[0]; fl[1] = t0[1]; fl[2] = t0[2]; fl[3] = t0[3]; fl[4] = t1[0]; fl[5] = t1[1]; fl[6] = t1[2]; fl[7] = t1[3];
        } else {
            for (int j = 0; j < nv; j++) { const float2 t = ((const float2*)fr)[j]; fl[2 * j] = t.x; fl[2 * j + 1] = t.y; }
        }
        mf_u4 ow = {0u, 0u, 0u, 0u};
        if (a.have_old) ow = __builtin_nontemporal_load((const mf_u4*)(a.ring + o));
        const mf_i4 su4 = *(const mf_i4*)(a.Su + o), sv4 = *(const mf_i4*)(a.Sv + o);
        const mf_u4 sm4 = *(const mf_u4*)(a.Sm + o);
        const uint2 n2 = *(const uint2*)(a.n + o);
        const mf_l2 uu0 = *(const mf_l2*)(a.Suu + o), uu1 = *(const mf_l2*)(a.Suu + o + 2);
        const mf_l2 vv0 = *(const mf_l2*)(a.Svv + o), vv1 = *(const mf_l2*)(a.Svv + o + 2);
        const mf_l2 uv0 = *(const mf_l2*)(a.Suv + o), uv1 = *(const mf_l2*)(a.Suv + o + 2);
        int Su[MF_PX] = {su4[0], su4[1], su4[2], su4[3]}, Sv[MF_PX] = {sv4[0], sv4[1], sv4[2], sv4[3]};
        unsigned Sm[MF_PX] = {sm4[0], sm4[1], sm4[2], sm4[3]};
        unsigned nn[MF_PX] = {n2.x & 0xffffu, n2.x >> 16, n2.y & 0xffffu, n2.y >> 16};
        long long Suu[MF_PX] = {uu0[0], uu0[1], uu1[0], uu1[1]}, Svv[MF_PX] = {vv0[0], vv0[1], vv1[0], vv1[1]};
        long long Suv[MF_PX] = {uv0[0], uv0[1], uv1[0], uv1[1]};
        unsigned nw[MF_PX] = {0u, 0u, 0u, 0u};                // the ring's new words: the places past w hold zero
        // 2. the sample out, the sample in
#pragma unroll
        for (int j = 0; j < MF_PX; j++) {
            if (j >= nv) break;
            const float fu = fl[2 * j], fv = fl[2 * j + 1];
            const bool bad = !(fabsf(fu) < 500.0f && fabsf(fv) < 500.0f);      // NaN and the infinities fail the comparison
            const int u = bad ? 0 : (int)rintf(fu * 64.0f), v = bad ? 0 : (int)rintf(fv * 64.0f);
            int ou = (int)(short)(ow[j] & 0xffffu), ov = (int)(short)(ow[j] >> 16);
            const bool old = a.have_old && ow[j] != MF_BAD;
            if (!old) ou = ov = 0;
            nn[j] += (bad ? 0u : 1u) - (old ? 1u : 0u);
            Su[j] += u - ou;
            Sv[j] += v - ov;
            Suu[j] += (long long)(u * u - ou * ou);           // each square is at most 1.024e9
            Svv[j] += (long long)(v * v - ov * ov);
            Suv[j] += (long long)(u * v) - (long long)(ou * ov);
            Sm[j] += mf_isqrt32((unsigned)(u * u + v * v)) - mf_isqrt32((unsigned)(ou * ou + ov * ov));
            nw[j] = bad ? MF_BAD : (((unsigned)u & 0xffffu) | ((unsigned)v << 16));
            cs[j][5] += bad;
        }
        __builtin_nontemporal_store((mf_u4){nw[0], nw[1], nw[2], nw[3]}, (mf_u4*)(a.ring + o));
        *(mf_i4*)(a.Su + o) = (mf_i4){Su[0], Su[1], Su[2], Su[3]};
        *(mf_i4*)(a.Sv + o) = (mf_i4){Sv[0], Sv[1], Sv[2], Sv[3]};
        *(mf_u4*)(a.Sm + o) = (mf_u4){Sm[0], Sm[1], Sm[2], Sm[3]};
        *(uint2*)(a.n + o) = make_uint2(nn[0] | (nn[1] << 16), nn[2] | (nn[3] << 16));
        *(mf_l2*)(a.Suu + o) = (mf_l2){Suu[0], Suu[1]}; *(mf_l2*)(a.Suu + o + 2) = (mf_l2){Suu[2], Suu[3]};
        *(mf_l2*)(a.Svv + o) = (mf_l2){Svv[0], Svv[1]}; *(mf_l2*)(a.Svv + o + 2) = (mf_l2){Svv[2], Svv[3]};
        *(mf_l2*)(a.Suv + o) = (mf_l2){Suv[0], Suv[1]}; *(mf_l2*)(a.Suv + o + 2) = (mf_l2){Suv[2], Suv[3]};
        // 3. the cells' sums over the filled pixels
        bool filled[MF_PX];
#pragma unroll
        for (int j = 0; j < MF_PX; j++) {
            filled[j] = j < nv && nn[j] >= (unsigned)a.min_fill;
            if (filled[j]) { cs[j][0] += 1; cs[j][1] += nn[j]; cs[j][2] += Su[j]; cs[j][3] += Sv[j]; cs[j][4] += Sm[j]; }
        }
        // 4. the outputs
        if (a.mean) {
            float m[2 * MF_PX];
#pragma unroll
            for (int j = 0; j < MF_PX; j++) {
                const double dn = (double)nn[j];
                m[2 * j] = filled[j] ? (float)(((double)Su[j] / 64.0) / dn) : 0.f;
                m[2 * j + 1] = filled[j] ? (float)(((double)Sv[j] / 64.0) / dn) : 0.f;
            }
            char* dst = (char*)a.mean + (size_t)y * a.mean_step + 8 * (size_t)x0;
            if (nv == MF_PX) {
                *(mf_f4*)dst = (mf_f4){m[0], m[1], m[2], m[3]};
                *(mf_f4*)(dst + 16) = (mf_f4){m[4], m[5], m[6], m[7]};
            } else {
                for (int j = 0; j < nv; j++) ((float2*)dst)[j] = make_float2(m[2 * j], m[2 * j + 1]);
            }
        }
        if (SD) {
            float d[2 * MF_PX];
#pragma unroll
            for (int j = 0; j < MF_PX; j++) {
                d[2 * j] = d[2 * j + 1] = 0.f;
                if (!filled[j]) continue;
                const long long n = nn[j];
                const long long qa = n * Suu[j] - (long long)Su[j] * Su[j], qc = n * Svv[j] - (long long)Sv[j] * Sv[j];
                const long long qb = n * Suv[j] - (long long)Su[j] * Sv[j];
                const double A = (double)qa, B = (double)qb, C = (double)qc;
                const double rr = sqrt((A - C) * (A - C) + 4.0 * (B * B));
                const double l1 = ((A + C) + rr) * 0.5;
                const double l2 = fmax(((A + C) - rr) * 0.5, 0.);
                const double den = 64.0 * (double)n;
                d[2 * j] = (float)(sqrt(l1) / den);
                d[2 * j + 1] = (float)(sqrt(l2) / den);
            }
            char* dst = (char*)a.sd + (size_t)y * a.sd_step + 8 * (size_t)x0;
            if (nv == MF_PX) {
                *(mf_f4*)dst = (mf_f4){d[0], d[1], d[2], d[3]};
                *(mf_f4*)(dst + 16) = (mf_f4){d[4], d[5], d[6], d[7]};
            } else {
                for (int j = 0; j < nv; j++) ((float2*)dst)[j] = make_float2(d[2 * j], d[2 * j + 1]);
            }
        }
        if (a.steady || a.pic) {
            unsigned st[MF_PX];
#pragma unroll
            for (int j = 0; j < MF_PX; j++) {
                st[j] = 0u;
                if (filled[j]) st[j] = mf_steady(mf_isqrt64((long long)Su[j] * Su[j] + (long long)Sv[j] * Sv[j]), Sm[j]);
            }
            if (a.steady) {
                uint16_t* dst = (uint16_t*)((char*)a.steady + (size_t)y * a.steady_step) + x0;
                if (nv == MF_PX) {
                    const uint2 v = make_uint2(st[0] | (st[1] << 16), st[2] | (st[3] << 16));
                    __builtin_memcpy(dst, &v, 8);
                } else {
                    for (int j = 0; j < nv; j++) dst[j] = (uint16_t)st[j];
                }
            }
            if (a.pic) {
                uint8_t* dst = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x0;
                uint32_t px[MF_PX];
#pragma unroll
                for (int j = 0; j < MF_PX; j++) {
                    const uint8_t* e = jet + 3 * (st[j] * 255u / 1000u);
                    px[j] = filled[j] ? (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) : 0u;
                }
                if (nv == MF_PX) {
                    uint32_t wd[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
                    __builtin_memcpy(dst, wd, 12);
                } else {
                    for (int j = 0; j < nv; j++) { dst[3 * j] = (uint8_t)px[j]; dst[3 * j + 1] = (uint8_t)(px[j] >> 8); dst[3 * j + 2] = (uint8_t)(px[j] >> 16); }
                }
            }
        }
    }
    if (cur_cy >= 0) mf_flush<6>(a.acc, tab, f, a.gx, cur_cy, cxl, cs, word);
    __syncthreads();
    mf_table_out(a.acc, tab, f, a.gx);
    if (!rc_hand_off_release(&a.ctl->t0.ticket, a.nblocks, &last)) return;

    // G, by the last-arriving block: the sums stay for meanflow@1
    long long gx = 0, gy = 0;
#pragma unroll 4
    for (int c = threadIdx.x; c < a.gx * a.gy; c += RC_BLOCK) {
        long long* q = a.acc + (size_t)RC_MEANFLOW_SUMS * c;
        gx += rc_acc_load(q + 2); gy += rc_acc_load(q + 3);
    }
    gx = rc_wave_sum_lane0(gx); gy = rc_wave_sum_lane0(gy);
    if (lane == 0) { red[2 * wv] = gx; red[2 * wv + 1] = gy; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    gx = gy = 0;
    for (int k = 0; k < MF_WAVES; k++) { gx += red[2 * k]; gy += red[2 * k + 1]; }
    a.ctl->G[0] = gx; a.ctl->G[1] = gy;                       // read by the next launch (stream order)
    __hip_atomic_store(&a.ctl->t0.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================================ meanflow@1: mask, records, summary
struct MfArgs1 {
    const int32_t* Su; const int32_t* Sv; const uint32_t* Sm; const uint16_t* n;   // the state's planes
    uint8_t* mask; size_t mask_step;             // the caller's, or null
    MfCtl* ctl;
    long long* acc;
    long long* summary; long long* sums; rc_meanflow_cell* cells;         // the state's copy
    long long* summary2; long long* sums2; rc_meanflow_cell* cells2;      // the caller's, or null
    int w, h, P, rows, gx, gy, cw, ch;
    int min_fill, steady_min, fixed;
    long long smin_q;                            // ceil(speed_min * 64)
    double K, dir_x, dir_y;
    long long held, pushes;
    unsigned nblocks;
};

__global__ __launch_bounds__(RC_BLOCK) void k_mf_mask(const MfArgs1 a) {
    __shared__ long long tab[MF_LDS_CELLS * RC_MEANFLOW_SUMS];
    __shared__ long long red[MF_WAVES * 4];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int th = MF_WAVES * a.rows;
    const int xb = blockIdx.x * MF_TW, yb = blockIdx.y * th;
    const MfFoot f = mf_foot(xb, yb, th, a.w, a.h, a.cw, a.ch, a.gx, a.gy);
    if (f.lds)
        for (int i = threadIdx.x; i < RC_MEANFLOW_SUMS * f.ntab; i += RC_BLOCK) tab[i] = 0;
    __syncthreads();
    const long long G0 = a.ctl->G[0], G1 = a.ctl->G[1];
    const double Dx = a.fixed ? a.dir_x : -(double)G0, Dy = a.fixed ? a.dir_y : -(double)G1;
    const double dd = Dx * Dx + Dy * Dy;
    const int x0 = xb + MF_PX * lane;
    const int nv = min(MF_PX, a.w - x0);
    int cxl[MF_PX];
#pragma unroll
    for (int j = 0; j < MF_PX; j++) cxl[j] = j < nv ? min((x0 + j) / a.cw, a.gx - 1) : -1;
    const int word[1] = {5};                                  // mask pixels
    long long cs[MF_PX][1] = {{0}, {0}, {0}, {0}};
    int cur_cy = -1;
    const int y0 = yb + wv * a.rows;
    for (int r = 0; r < a.rows; r++) {
        const int y = y0 + r;
        if (y >= a.h) break;
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) mf_flush<1>(a.acc, tab, f, a.gx, cur_cy, cxl, cs, word);
            cur_cy = cy;
        }
        if (nv <= 0) continue;
        const size_t o = (size_t)y * a.P + x0;
        const mf_i4 su4 = *(const mf_i4*)(a.Su + o), sv4 = *(const mf_i4*)(a.Sv + o);
        const mf_u4 sm4 = *(const mf_u4*)(a.Sm + o);
        const uint2 n2 = *(const uint2*)(a.n + o);
        const unsigned nn[MF_PX] = {n2.x & 0xffffu, n2.x >> 16, n2.y & 0xffffu, n2.y >> 16};
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < MF_PX; j++) {
            if (j >= nv || nn[j] < (unsigned)a.min_fill) continue;
            // the direction in double, as the opposing-flow map decides its cells; it comes first because it is the cheapest
            const long long su = su4[j], sv = sv4[j];
            const double Sx = (double)su, Sy = (double)sv;
            const double dot = Sx * Dx + Sy * Dy;
            const double cc = Sx * Sx + Sy * Sy;
            if (!(dot > 0. && dot * dot >= a.K * (cc * dd))) continue;
            const long long R = mf_isqrt64(su * su + sv * sv);
            if (R < a.smin_q * (long long)nn[j] || (int)mf_steady(R, sm4[j]) < a.steady_min) continue;
            m |= 255u << (8 * j);
            cs[j][0] += 1;
        }
        if (a.mask) {
            uint8_t* q = a.mask + (size_t)y * a.mask_step + x0;
            if (nv == MF_PX) __builtin_memcpy(q, &m, 4);
            else
                for (int j = 0; j < nv; j++) q[j] = (uint8_t)(m >> (8 * j));
        }
    }
    if (cur_cy >= 0) mf_flush<1>(a.acc, tab, f, a.gx, cur_cy, cxl, cs, word);
    __syncthreads();
    mf_table_out(a.acc, tab, f, a.gx);
    if (!rc_hand_off_release(&a.ctl->t1.ticket, a.nblocks, &last)) return;

    // sums, records and summary, by the last-arriving block; every counter is left zero for the next push
    long long tf = 0, tm = 0, tb = 0, tsm = 0;
    for (int c = threadIdx.x; c < a.gx * a.gy; c += RC_BLOCK) {
        long long w[RC_MEANFLOW_SUMS];
#pragma unroll
        for (int k = 0; k < RC_MEANFLOW_SUMS - 1; k++) w[k] = rc_acc_take(a.acc + (size_t)RC_MEANFLOW_SUMS * c + k);      // in flight together
        w[RC_MEANFLOW_SUMS - 1] = 0;                          // the last word is never added to
#pragma unroll
        for (int k = 0; k < RC_MEANFLOW_SUMS; k++) {
            a.sums[(size_t)RC_MEANFLOW_SUMS * c + k] = w[k];
            if (a.sums2) a.sums2[(size_t)RC_MEANFLOW_SUMS * c + k] = w[k];
        }
        rc_meanflow_cell r;
        memset(&r, 0, sizeof(r));
        r.filled = (int)w[0]; r.mask = (int)w[5]; r.bad = (int)w[6];
        if (w[0] == 0) {
            r.flags = RC_MEANFLOW_EMPTY;
        } else {
            const double sx = (double)w[2], sy = (double)w[3], dn = (double)w[1];
            r.mean_x = (float)((sx / 64.0) / dn);
            r.mean_y = (float)((sy / 64.0) / dn);
            if (w[4] > 0) r.steadiness = (float)((sqrt(sx * sx + sy * sy) / (double)w[4]) * 1000.0);
        }
        a.cells[c] = r;
        if (a.cells2) a.cells2[c] = r;
        tf += w[0]; tm += w[5]; tb += w[6]; tsm += w[4];
    }
    tf = rc_wave_sum_lane0(tf); tm = rc_wave_sum_lane0(tm); tb = rc_wave_sum_lane0(tb); tsm = rc_wave_sum_lane0(tsm);
    if (lane == 0) { red[4 * wv] = tf; red[4 * wv + 1] = tm; red[4 * wv + 2] = tb; red[4 * wv + 3] = tsm; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long s[8] = {0, 0, 0, G0, G1, 0, a.held, a.pushes};
    for (int k = 0; k < MF_WAVES; k++) { s[0] += red[4 * k]; s[1] += red[4 * k + 1]; s[2] += red[4 * k + 2]; s[5] += red[4 * k + 3]; }
    for (int k = 0; k < 8; k++) {
        a.summary[k] = s[k];
        if (a.summary2) a.summary2[k] = s[k];
    }
    __hip_atomic_store(&a.ctl->t1.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next push (stream order)
}

// ============================================================================ host side
void rc_state_free(RcMeanflow& v) {
    rc_buf_free(v.ring); rc_buf_free(v.sums); rc_buf_free(v.acc); rc_buf_free(v.out); rc_buf_free(v.ctl); rc_buf_free(v.jet);
    rc_fence_free(v.zf);
    v = RcMeanflow();
}

// open and reset: the sums, the cells' accumulators, the last push's outputs, the tickets; the push count.  The ring is not read
// before it has wrapped: a slot is written before it is read
int rc_state_zero(RcSlot& s, RcMeanflow& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.sums, &v.acc, &v.out, &v.ctl});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static bool mf_in(double v, double lo, double hi) { return v >= lo && v <= hi; }     // NaN fails
static bool mf_settable(const rc_meanflow_params& p) {
    if (p.steady_min < 0 || p.steady_min > 1000 || p.min_fill < 1 || p.min_fill > p.window || !mf_in(p.speed_min, 0., 400.) ||
        !(p.min_cos2 >= 0. && p.min_cos2 < 1.))
        return false;
    if (p.flags == RC_MEANFLOW_DIR_FIXED)
        return mf_in(p.dir_x, -1.7976931348623157e308, 1.7976931348623157e308) && mf_in(p.dir_y, -1.7976931348623157e308, 1.7976931348623157e308) &&
               (p.dir_x != 0. || p.dir_y != 0.);
    return true;
}
static const char* mf_settable_text = "min_fill 1..window, steady_min 0..1000, speed_min finite and 0..400, min_cos2 in [0, 1), with "
                                      "RC_MEANFLOW_DIR_FIXED dir_x and dir_y finite and not both 0";

static size_t mf_cells(const RcMeanflow& v) { return (size_t)v.prm.grid_x * v.prm.grid_y; }
static size_t mf_px(const RcMeanflow& v) { return (size_t)v.P * v.h; }
// RcMeanflow::sums: Suu | Svv | Suv [h][P] int64 | Su | Sv [h][P] int32 | Sm [h][P] uint32 | n [h][P] uint16
static long long* mf_Suu(const RcMeanflow& v) { return (long long*)v.sums.p; }
static int32_t* mf_Su(const RcMeanflow& v) { return (int32_t*)(mf_Suu(v) + 3 * mf_px(v)); }
static uint16_t* mf_n(const RcMeanflow& v) { return (uint16_t*)(mf_Su(v) + 3 * mf_px(v)); }
// RcMeanflow::out: summary 8 int64 | sums [cells][RC_MEANFLOW_SUMS] int64 | records [cells]
static long long* mf_out_summary(const RcMeanflow& v) { return (long long*)v.out.p; }
static long long* mf_out_sums(const RcMeanflow& v) { return (long long*)v.out.p + 8; }
static rc_meanflow_cell* mf_out_cells(const RcMeanflow& v) { return (rc_meanflow_cell*)((long long*)v.out.p + 8 + mf_cells(v) * RC_MEANFLOW_SUMS); }

// a wave takes `rows` rows: as many as keep the launch to `cap` blocks
static dim3 mf_grid(int w, int h, int cap, int& rows) {
    const int tx = (w + MF_TW - 1) / MF_TW, bands = (h + MF_WAVES - 1) / MF_WAVES;
    const int by = cap / tx > 0 ? cap / tx : 1;
    rows = (bands + by - 1) / by;
    return dim3(tx, (h + MF_WAVES * rows - 1) / (MF_WAVES * rows));
}

extern "C" int rcflow_meanflow_open(rc_ctx* ctx, int stream, int w, int h, const rc_meanflow_params* prm) {
    static const char* who = "rcflow_meanflow_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad field size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    const int W = prm->window;
    if (W < 2 || W > RC_MEANFLOW_MAX_WINDOW || (prm->flags != RC_MEANFLOW_DIR_FIXED && prm->flags != RC_MEANFLOW_DIR_OPPOSED) || !mf_settable(*prm)) {
        rc_set_error("%s: window 2..%d, flags RC_MEANFLOW_DIR_FIXED or RC_MEANFLOW_DIR_OPPOSED (exactly one), %s", who, RC_MEANFLOW_MAX_WINDOW,
                     mf_settable_text);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d field (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcMeanflow n;
    n.w = w; n.h = h; n.prm = *prm;
    n.P = (w + 3) & ~3;
    const unsigned long long px = (unsigned long long)n.P * h, ring = px * 4ull * W, sums = px * 38ull, state = ring + sums;
    if (state > RC_MEANFLOW_MAX_STATE_BYTES) {
        rc_set_error("%s: %d fields of %d x %d are %llu bytes of ring and sums, more than RC_MEANFLOW_MAX_STATE_BYTES", who, W, w, h, state);
        return RC_ESIZE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    const size_t nc = mf_cells(n);
    rc = rc_buf_ensure(n.ring, (size_t)ring);
    if (!rc) rc = rc_buf_ensure(n.sums, (size_t)sums);
    if (!rc) rc = rc_buf_ensure(n.acc, nc * RC_MEANFLOW_SUMS * 8);
    if (!rc) rc = rc_buf_ensure(n.out, 64 + nc * (RC_MEANFLOW_SUMS * 8 + sizeof(rc_meanflow_cell)));
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(MfCtl));
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    return rc_state_install(*s, s->mf, n, rc);
}

extern "C" int rcflow_meanflow_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, float* d_mean, size_t mean_step,
                                        uint16_t* d_steady, size_t steady_step, float* d_std, size_t std_step, uint8_t* d_mask, size_t mask_step,
                                        uint8_t* d_picture, size_t picture_step, rc_meanflow_cell* d_cells, long long* d_sums, long long* d_summary) {
    static const char* who = "rcflow_meanflow_push_dev";
    RcSlot* s; RcMeanflow* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mf, who, s, vp)) return rc;
    RcMeanflow& v = *vp;
    const int w = v.w, h = v.h, W = v.prm.window;
    const size_t nc = mf_cells(v);
    if (!d_flow_xy) {                                         // the slot's resident field (rcflow_stream_flow_ptr), as rcflow_ripmap_push_dev
        if (!s->flow_w) { rc_set_error("%s: no flow field is resident on the slot yet", who); return RC_ESTATE; }
        if (s->flow_w != w || s->flow_h != h) {
            rc_set_error("%s: the resident flow field is %d x %d, the session %d x %d", who, s->flow_w, s->flow_h, w, h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)w * 8;
    }
    RcArgsN<9> ar(who, w, h);
    ar.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    ar.image("d_mean", d_mean, mean_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_steady", d_steady, steady_step, 2, 2, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_std", d_std, std_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_cells", d_cells, nc * sizeof(rc_meanflow_cell), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_sums", d_sums, nc * RC_MEANFLOW_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const long long p = v.pushes, pushes = p + 1;
    const int c = (int)(p % W);
    const rc_meanflow_params& q = v.prm;
    const size_t px = mf_px(v);
    const double dpx = (double)px;
    {
        MfArgs0 a;
        int rows = 1;
        const dim3 grid = mf_grid(w, h, MF_MAX_BLOCKS0, rows);
        a.flow = d_flow_xy; a.flow_step = flow_step;
        a.ring = (uint32_t*)v.ring.p + (size_t)c * px;
        a.Suu = mf_Suu(v); a.Svv = a.Suu + px; a.Suv = a.Svv + px;
        a.Su = mf_Su(v); a.Sv = a.Su + px; a.Sm = (uint32_t*)(a.Sv + px); a.n = mf_n(v);
        a.mean = d_mean; a.mean_step = mean_step; a.steady = d_steady; a.steady_step = steady_step; a.sd = d_std; a.sd_step = std_step;
        a.pic = d_picture; a.pic_step = picture_step;
        a.jet = (const uint8_t*)v.jet.p; a.ctl = (MfCtl*)v.ctl.p; a.acc = (long long*)v.acc.p;
        a.w = w; a.h = h; a.P = v.P; a.rows = rows; a.gx = q.grid_x; a.gy = q.grid_y; a.cw = w / q.grid_x; a.ch = h / q.grid_y;
        a.have_old = p >= W; a.min_fill = q.min_fill;
        a.nblocks = grid.x * grid.y;
        // the field 8 in; the ring slot 4 out, and 4 in once it has wrapped; the sums 38 in and 38 out; the outputs
        RcProfScope ps(ctx, s->cur, RC_K_MEANFLOW, 0, dpx * (8. + 4. + (a.have_old ? 4. : 0.) + 76. + (d_mean ? 8. : 0.) + (d_steady ? 2. : 0.) +
                                                            (d_std ? 8. : 0.) + (d_picture ? 3. : 0.)));
        if (d_std) hipLaunchKernelGGL(k_mf_pixels<1>, grid, dim3(RC_BLOCK), 0, s->cur, a);
        else hipLaunchKernelGGL(k_mf_pixels<0>, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    {
        MfArgs1 a;
        int rows = 1;
        const dim3 grid = mf_grid(w, h, MF_MAX_BLOCKS1, rows);
        a.Su = mf_Su(v); a.Sv = a.Su + px; a.Sm = (const uint32_t*)(a.Sv + px); a.n = mf_n(v);
        a.mask = d_mask; a.mask_step = mask_step;
        a.ctl = (MfCtl*)v.ctl.p; a.acc = (long long*)v.acc.p;
        a.summary = mf_out_summary(v); a.sums = mf_out_sums(v); a.cells = mf_out_cells(v);
        a.summary2 = d_summary; a.sums2 = d_sums; a.cells2 = d_cells;
        a.w = w; a.h = h; a.P = v.P; a.rows = rows; a.gx = q.grid_x; a.gy = q.grid_y; a.cw = w / q.grid_x; a.ch = h / q.grid_y;
        a.min_fill = q.min_fill; a.steady_min = q.steady_min; a.fixed = q.flags == RC_MEANFLOW_DIR_FIXED;
        a.smin_q = (long long)ceil(q.speed_min * 64.0);
        a.K = q.min_cos2; a.dir_x = q.dir_x; a.dir_y = q.dir_y;
        a.held = pushes < W ? pushes : W; a.pushes = pushes;
        a.nblocks = grid.x * grid.y;
        RcProfScope ps(ctx, s->cur, RC_K_MEANFLOW, 1, dpx * (14. + (d_mask ? 1. : 0.)));
        hipLaunchKernelGGL(k_mf_mask, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_meanflow_read(rc_ctx* ctx, int stream, rc_meanflow_cell* cells, long long* sums, long long summary[8]) {
    RcSlot* s; RcMeanflow* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mf, "rcflow_meanflow_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = mf_cells(*vp);
    if (cells) RC_HIP(hipMemcpyAsync(cells, mf_out_cells(*vp), nc * sizeof(rc_meanflow_cell), hipMemcpyDeviceToHost, s->cur));
    if (sums) RC_HIP(hipMemcpyAsync(sums, mf_out_sums(*vp), nc * RC_MEANFLOW_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, mf_out_summary(*vp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_meanflow_set(rc_ctx* ctx, int stream, int steady_min, double speed_min, double min_cos2, double dir_x, double dir_y, int min_fill) {
    RcSlot* s; RcMeanflow* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mf, "rcflow_meanflow_set", s, vp)) return rc;
    rc_meanflow_params p = vp->prm;
    p.steady_min = steady_min; p.speed_min = speed_min; p.min_cos2 = min_cos2; p.dir_x = dir_x; p.dir_y = dir_y; p.min_fill = min_fill;
    if (!mf_settable(p)) {
        rc_set_error("rcflow_meanflow_set: %s", mf_settable_text);
        return RC_EINVAL;
    }
    vp->prm = p;
    return RC_OK;
}

extern "C" int rcflow_meanflow_info(rc_ctx* ctx, int stream, rc_meanflow_info* info) {
    RcSlot* s; RcMeanflow* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mf, "rcflow_meanflow_info", s, vp)) return rc;
    const RcMeanflow& v = *vp;
    if (!info) { rc_set_error("rcflow_meanflow_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->launches_per_push = RC_MEANFLOW_LAUNCHES;
    info->held = (int)(v.pushes < v.prm.window ? v.pushes : v.prm.window);
    info->pushes = v.pushes;
    info->device_bytes = v.ring.bytes + v.sums.bytes + v.acc.bytes + v.out.bytes + v.ctl.bytes + v.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_meanflow_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::mf, "rcflow_meanflow_reset"); }
extern "C" int rcflow_meanflow_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::mf); }
