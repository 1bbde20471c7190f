// piv_kernels.hip -- ensemble PIV: where does the water go, when the foam moves several pixels a frame?
//
// Block cross-correlation of interrogation windows between consecutive grey frames, the correlation sums added over the last
// `ensemble` pairs before the peak is taken.  include/rcflow.h ("ensemble PIV") is the specification; tests/_piv_ref.py states
// it in numpy.  Everything up to the accumulators is integer and held to that bit for bit; the score, the peak and the sub-pixel
// step are double, the median test is float (a stored float within one unit in the last place).  A push is one launch when no
// output is asked for, else three, and nothing synchronises:
//   piv@0  correlate  the hot one.  A block owns up to eight neighbouring cells of one grid row, as many as fill its lanes.  Their
//                     search areas overlap and sit in LDS once, as a strip of M + 2R rows (rows padded to dwords plus one); the
//                     templates (M x M bytes each) beside it.  A lane owns the four displacements of one row j whose windows
//                     begin in one dword of the strip: per template dword (the same address for the cell's lanes: a broadcast)
//                     it reads ONE new strip dword, builds the byte-shifted ones with v_alignbyte_b32 and does four
//                     v_dot4_u32_u8.  Sb and Sbb come from the strip's column sums, slid down the D rows once per block; a
//                     lane adds M of them and slides over its three neighbours.  The LDS pitches put neighbouring lanes on
//                     neighbouring banks (pv_lds_plan).  Partial sums are 32-bit; a displacement's three words are written by
//                     one lane, widened at the accumulator update: acc += new - ring[slot], ring[slot] = new (E = 1: acc = new,
//                     no ring), a whole group of twelve words in 16-byte accesses.  No atomics, no hand-off between blocks;
//   piv@1  peak       a wave owns a cell: the scores in double from the accumulators, the first largest by a wave reduction
//                     on (score, index), the sub-pixel step and the record before validation by its first lane;
//   piv@2  validate   the first blocks a lane a cell: the median test, the record, the field, the counts (the launch's last
//                     such block writes the summary); the others a lane a pixel of the picture, after the lanes of the block
//                     validated the at most 256 cells its 64 x 4 pixels lie in.
// The pushed frame becomes the next pair's A by a device-to-device copy on the slot's stream after piv@0: cells overlap, so a
// block cannot overwrite what its neighbours still read.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define PV_WAVES 4
static_assert(RC_BLOCK == 64 * PV_WAVES, "a block is PV_WAVES waves");
#define PV_MAX_CPB 8               // piv@0: cells a block owns at most
#define PV_LDS_BUDGET (60 * 1024)  // piv@0: dynamic LDS of a block at most
#define PV_SEG 8                   // piv@0: rows j a column-sum task slides over

typedef uint32_t pv_u32u __attribute__((aligned(1)));     // four pixels of a caller's row: no alignment is asked of it

struct PvCtl { unsigned ticket, cnt[5], pad[2]; };        // zero between launches

// ============================================================================ piv@0: one pair's sums into the accumulators
struct PvCorrArgs {
    const uint8_t* A; size_t a_step;     // the previous frame
    const uint8_t* B; size_t b_step;     // the pushed frame
    int* ring;                           // the ring slot this pair replaces, [cells][nw], or null (E = 1)
    long long* acc;                      // [cells][nw]: D * D * (Tab, Tb, Tbb) | Ta, Taa
    int M, R, D, Gm, step, gx, bpr, cpb, tasks, sw, nw;
};

// the smallest v >= need with v = want (mod 32): a row pitch in dwords that puts consecutive tasks on consecutive LDS banks
__host__ __device__ __forceinline__ int pv_pitch(int need, int want) { return need + (((want - need) % 32) + 32) % 32; }
// LDS of a block of c cells: templates [c][M * M / 4 + 2] dwords | strip [sw][P4] dwords | colS, colQ [D][CP] int | template partial sums [c][2][M / 4] int.
// P4 = Gm (mod 32): the tasks (j, g), (j, g + 1), .. (j + 1, 0) read neighbouring banks of the strip; CP = 4 Gm + 1 (mod 32): their
// windows of column sums begin four banks apart and a row further one more; the templates two banks apart
struct PvLds { int SW, P4, CP, tslot; size_t bytes; };
__host__ __device__ __forceinline__ PvLds pv_lds_plan(int c, int M, int sw, int D, int step, int Gm) {
    PvLds l;
    l.SW = sw + (c - 1) * step;
    l.P4 = pv_pitch((l.SW + 3) / 4 + 1, Gm);
    l.CP = pv_pitch(l.SW, 4 * Gm + 1);
    l.tslot = M * M / 4 + 2;
    l.bytes = 4 * ((size_t)c * l.tslot + (size_t)sw * l.P4 + 2 * (size_t)D * l.CP + (size_t)c * 2 * (M / 4));
    return l;
}

typedef long long pv_ll2 __attribute__((ext_vector_type(2), aligned(8)));
typedef int pv_i4 __attribute__((ext_vector_type(4), aligned(4)));

// bytes [x, x + 4) of a row, those at or past xend as zero
__device__ __forceinline__ uint32_t pv_load4(const uint8_t* row, int x, int xend) {
    if (x + 4 <= xend) return *(const pv_u32u*)(row + x);
    uint32_t v = 0;
    for (int k = 0; x + k < xend; k++) v |= (uint32_t)row[x + k] << (8 * k);
    return v;
}

// n = 1, 3 or 12 consecutive words of a cell: the ring slot takes the new ones, the accumulators their difference to the old
__device__ __forceinline__ void pv_update(const PvCorrArgs& a, size_t o, const int* nv, int n) {
    if (n == 12) {                                                // a whole group: 16-byte accesses (the words are 4- and 8-byte aligned)
        pv_ll2* ap = (pv_ll2*)(a.acc + o);
        if (a.ring) {
            pv_i4* rp = (pv_i4*)(a.ring + o);
            int old[12];
#pragma unroll
            for (int e = 0; e < 3; e++) {
                const pv_i4 v = rp[e];
                old[4 * e] = v.x; old[4 * e + 1] = v.y; old[4 * e + 2] = v.z; old[4 * e + 3] = v.w;
            }
            pv_ll2 t[6];
#pragma unroll
            for (int e = 0; e < 6; e++) t[e] = ap[e];
#pragma unroll
            for (int e = 0; e < 3; e++) { pv_i4 v; v.x = nv[4 * e]; v.y = nv[4 * e + 1]; v.z = nv[4 * e + 2]; v.w = nv[4 * e + 3]; rp[e] = v; }
#pragma unroll
            for (int e = 0; e < 6; e++) {
                t[e].x += (long long)nv[2 * e] - (long long)old[2 * e];
                t[e].y += (long long)nv[2 * e + 1] - (long long)old[2 * e + 1];
                ap[e] = t[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 6; e++) { pv_ll2 v; v.x = nv[2 * e]; v.y = nv[2 * e + 1]; ap[e] = v; }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 3; e++) {
        if (e >= n) break;
        if (a.ring) {
            const int old = a.ring[o + e];
            a.ring[o + e] = nv[e];
            a.acc[o + e] += (long long)nv[e] - (long long)old;
        } else {
            a.acc[o + e] = nv[e];
        }
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_pv_correlate(const PvCorrArgs a) {
    extern __shared__ __align__(16) unsigned char pv_lds[];
    const int M = a.M, R = a.R, D = a.D, sw = a.sw, M4 = M / 4, nt = blockDim.x;
    // the block's cells: nhere neighbours of one grid row.  Their search areas overlap and are one strip of SW columns
    const int cy = blockIdx.x / a.bpr, cx0 = (blockIdx.x - cy * a.bpr) * a.cpb, nhere = min(a.cpb, a.gx - cx0);
    const PvLds L = pv_lds_plan(nhere, M, sw, D, a.step, a.Gm);
    const int SW = L.SW, P4 = L.P4, P = 4 * P4, CP = L.CP, tslot = L.tslot;
    const int xs = cx0 * a.step, ys = cy * a.step;                // the strip's first pixel
    const int tdw = M * M4;
    uint32_t* const Tl = (uint32_t*)pv_lds;
    unsigned char* const Sl = pv_lds + 4 * (size_t)nhere * tslot;
    int* const colS = (int*)(Sl + sw * P);
    int* const colQ = colS + D * CP;
    int* const part = colQ + D * CP;

    // ---- load: a thread a dword.  A template's dwords all lie inside the frame; the strip's last ones are cut at its end
#pragma unroll 4
    for (int t = threadIdx.x; t < nhere * tdw; t += nt) {
        const int sl = t / tdw, q = t - sl * tdw, r = q / M4, k = q - r * M4;
        Tl[sl * tslot + q] = *(const pv_u32u*)(a.A + (size_t)(ys + R + r) * a.a_step + xs + sl * a.step + R + 4 * k);
    }
    const int n4 = (SW + 3) / 4 + 1;                              // the dwords of a strip row that are read; the last one: zeros
    for (int t = threadIdx.x; t < sw * n4; t += nt) {
        const int r = t / n4, k = t - r * n4;
        ((uint32_t*)Sl)[r * P4 + k] = pv_load4(a.B + (size_t)(ys + r) * a.b_step, xs + 4 * k, xs + SW);
    }
    __syncthreads();

    // ---- Sa, Saa per dword column of a template, and the strip's column sums of B and B^2 over M rows, slid down PV_SEG rows j per task
    for (int t = threadIdx.x; t < nhere * M4; t += nt) {
        const int sl = t / M4, k = t - sl * M4;
        const uint32_t* T = Tl + sl * tslot + k;
        uint32_t s = 0, ss = 0;
        for (int r = 0; r < M; r++) {
            const uint32_t v = T[r * M4];
            s = __builtin_amdgcn_udot4(v, 0x01010101u, s, false);
            ss = __builtin_amdgcn_udot4(v, v, ss, false);
        }
        part[(2 * sl) * M4 + k] = (int)s; part[(2 * sl + 1) * M4 + k] = (int)ss;
    }
    const int nseg = (D + PV_SEG - 1) / PV_SEG;
    for (int t = threadIdx.x; t < nseg * SW; t += nt) {
        const int sg = t / SW, c = t - sg * SW;
        const unsigned char* S = Sl + c;
        const int j0 = sg * PV_SEG, j1 = min(j0 + PV_SEG, D);
        int s = 0, ss = 0;
        for (int r = 0; r < M; r++) {
            const int v = S[(j0 + r) * P];
            s += v; ss += v * v;
        }
        colS[j0 * CP + c] = s; colQ[j0 * CP + c] = ss;
        for (int j = j0 + 1; j < j1; j++) {
            const int o = S[(j - 1) * P], n = S[(j - 1 + M) * P];
            s += n - o; ss += n * n - o * o;
            colS[j * CP + c] = s; colQ[j * CP + c] = ss;
        }
    }
    __syncthreads();

    // ---- the correlation: a task is (cell, j, a dword of the strip): the four displacements whose windows begin in that dword.
    // The lanes of a cell read one template address
    for (int t = threadIdx.x; t < nhere * a.tasks; t += nt) {
        const int sl = t / a.tasks, q = t - sl * a.tasks, j = q / a.Gm, g = q - j * a.Gm;
        const int cb = sl * a.step, gabs = (cb >> 2) + g, c0 = 4 * gabs - cb;      // the group's first displacement column: -3 .. 2R
        const size_t cell = (size_t)(cy * a.gx + cx0 + sl) * a.nw;
        if (q < 2) {                                              // Ta, Taa by the cell's first two tasks
            int v = 0;
            for (int k = 0; k < M4; k++) v += part[(2 * sl + q) * M4 + k];
            pv_update(a, cell + 3 * (size_t)(D * D) + q, &v, 1);
        }
        if (c0 >= D) continue;
        const uint32_t* T = Tl + sl * tslot;
        const uint32_t* S = (const uint32_t*)Sl + (size_t)j * P4 + gabs;
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int r = 0; r < M; r++, T += M4, S += P4) {
            uint32_t lo = S[0];
#pragma unroll 4
            for (int k = 0; k < M4; k++) {
                const uint32_t hi = S[k + 1], tv = T[k];
                s0 = __builtin_amdgcn_udot4(tv, lo, s0, false);
                s1 = __builtin_amdgcn_udot4(tv, __builtin_amdgcn_alignbyte(hi, lo, 1), s1, false);
                s2 = __builtin_amdgcn_udot4(tv, __builtin_amdgcn_alignbyte(hi, lo, 2), s2, false);
                s3 = __builtin_amdgcn_udot4(tv, __builtin_amdgcn_alignbyte(hi, lo, 3), s3, false);
                lo = hi;
            }
        }
        const uint32_t sab[4] = {s0, s1, s2, s3};
        // Sb, Sbb: M column sums for the group's first displacement, slid over the others
        const int u0 = c0 < 0 ? -c0 : 0, u1 = min(4, D - c0);    // the displacements c0 + u0 .. c0 + u1 - 1 exist
        const int* cs = colS + j * CP + 4 * gabs + u0;
        const int* cq = colQ + j * CP + 4 * gabs + u0;
        int sb = 0, sbb = 0;
        for (int x = 0; x < M; x++) { sb += cs[x]; sbb += cq[x]; }
        int nv[12];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            nv[3 * u] = (int)sab[u]; nv[3 * u + 1] = sb; nv[3 * u + 2] = sbb;
            if (u >= u0 && u + 1 < u1) { sb += cs[M + u - u0] - cs[u - u0]; sbb += cq[M + u - u0] - cq[u - u0]; }
        }
        const size_t o = cell + (size_t)(3 * (long long)(j * D + c0));      // c0 < 0: the words before o are not touched (u0 > 0)
        if (u0 == 0 && u1 == 4) {
            pv_update(a, o, nv, 12);
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (u >= u0 && u < u1) pv_update(a, o + 3 * u, nv + 3 * u, 3);
        }
    }
}

// ============================================================================ piv@1: score, peak and the record
struct PvPeakArgs {
    const long long* acc;
    rc_piv_cell* raw;                    // the records before validation
    int ncell, M, R, D, nw, n;
    double min_peak;
};

// doubles round operation by operation (-ffp-contract=off) in the order of tests/_piv_ref.py
__device__ __forceinline__ double pv_score(const long long* t, long long N, long long Ta, long long va) {
    const long long Tab = t[0], Tb = t[1], Tbb = t[2];
    const long long num = N * Tab - Ta * Tb, vb = N * Tbb - Tb * Tb;
    if (!(va > 0 && vb > 0)) return 0.;
    const double nd = (double)num;
    return (nd * fabs(nd)) / ((double)va * (double)vb);
}
__device__ __forceinline__ double pv_root(double s) { return copysign(sqrt(fabs(s)), s); }
__device__ __forceinline__ double pv_offset(double l, double c, double rr) {
    l = pv_root(l); c = pv_root(c); rr = pv_root(rr);
    const double e = (l - c) + (rr - c);
    return e < 0. ? (l - rr) / (2. * e) : 0.;
}

__global__ __launch_bounds__(RC_BLOCK) void k_pv_peak(const PvPeakArgs a) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * PV_WAVES + (threadIdx.x >> 6);
    if (c >= a.ncell) return;                                     // the whole wave
    rc_piv_cell r;
    r.dx = r.dy = r.peak = r.resid = 0.f; r.ix = r.iy = 0; r.flags = RC_PIV_EMPTY; r.pairs = 0;
    if (a.n == 0) {
        if (lane == 0) a.raw[c] = r;
        return;
    }
    const int D = a.D, R = a.R, DD = D * D;
    const long long* t = a.acc + (size_t)c * a.nw;
    const long long N = (long long)a.n * a.M * a.M, Ta = t[3 * DD], Taa = t[3 * DD + 1], va = N * Taa - Ta * Ta;
    double best = -INFINITY;
    int bd = 0x7fffffff;
    for (int d = lane; d < DD; d += 64) {
        const double s = pv_score(t + 3 * d, N, Ta, va);
        if (s > best) { best = s; bd = d; }                       // the lane's first largest
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_down(best, o, 64);
        const int od = __shfl_down(bd, o, 64);
        if (os > best || (os == best && od < bd)) { best = os; bd = od; }
    }
    if (lane != 0) return;
    r.pairs = a.n;
    r.peak = (float)best;
    if (va == 0 || best <= 0.) {
        r.flags = RC_PIV_FLAT;
    } else {
        const int j = bd / D, i = bd - j * D;
        r.ix = i - R; r.iy = j - R;
        r.flags = 0;
        double ox = 0., oy = 0.;
        if (i == 0 || i == D - 1 || j == 0 || j == D - 1) {
            r.flags |= RC_PIV_EDGE;
        } else {
            ox = pv_offset(pv_score(t + 3 * (bd - 1), N, Ta, va), best, pv_score(t + 3 * (bd + 1), N, Ta, va));
            oy = pv_offset(pv_score(t + 3 * (bd - D), N, Ta, va), best, pv_score(t + 3 * (bd + D), N, Ta, va));
        }
        if (best < a.min_peak) r.flags |= RC_PIV_LOWPEAK;
        r.dx = (float)((double)(i - R) + ox);
        r.dy = (float)((double)(j - R) + oy);
    }
    a.raw[c] = r;
}

// ============================================================================ piv@2: validation, field, picture, summary
struct PvValArgs {
    const rc_piv_cell* raw;
    rc_piv_cell* cells; long long* summary;      // the state's copy
    rc_piv_cell* cells2; long long* summary2;    // the caller's, or null
    float* field; size_t field_step;             // or null
    uint8_t* vis; size_t vis_step;               // or null
    const uint8_t* jet;
    PvCtl* ctl;
    int w, h, gx, gy, R, step, replace, n, nbc;  // nbc: the blocks that own cells; the picture's come after them
    float eps, thr, vis_max;
    long long pushes;
};

#define PV_INVALID (RC_PIV_EMPTY | RC_PIV_FLAT | RC_PIV_LOWPEAK)

__device__ __forceinline__ void pv_sort8(float v[8]) {           // ascending
#pragma unroll
    for (int p = 0; p < 7; p++)
#pragma unroll
        for (int q = 0; q < 7 - p; q++) {
            const float lo = v[q] > v[q + 1] ? v[q + 1] : v[q], hi = v[q] > v[q + 1] ? v[q] : v[q + 1];
            v[q] = lo; v[q + 1] = hi;
        }
}
// The median of the k finite values among eight, the other places holding (8 - k) / 2 times -inf and the rest +inf: sorted, the
// middle one of an odd k lies at place 3, the two middle ones of an even k at 3 and 4, whatever k is, so nothing is indexed by k
__device__ __forceinline__ float pv_median(float v[8], int k) {
    pv_sort8(v);
    return (k & 1) ? v[3] : (v[3] + v[4]) * 0.5f;
}
// one component of the median test -> the residual; um: the candidates' median
__device__ __forceinline__ float pv_residual(float v[8], int k, float mine, float eps, float& um) {
    um = pv_median(v, k);
    float d[8];
#pragma unroll
    for (int q = 0; q < 8; q++) d[q] = isinf(v[q]) ? v[q] : fabsf(v[q] - um);
    const float rm = pv_median(d, k);
    return fabsf(mine - um) / (rm + eps);
}

struct PvVal { int flags; float resid, fx, fy; };

__device__ PvVal pv_validate(const PvValArgs& a, int cx, int cy) {
    const rc_piv_cell me = a.raw[(size_t)cy * a.gx + cx];
    PvVal o;
    o.flags = me.flags; o.resid = 0.f; o.fx = 0.f; o.fy = 0.f;
    if (me.flags & PV_INVALID) return o;
    o.fx = me.dx; o.fy = me.dy;
    float vx[8], vy[8];
    int fl[8], k = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {                                 // the neighbours in raster order, the cell itself left out
        const int s = q < 4 ? q : q + 1, x = cx + s % 3 - 1, y = cy + s / 3 - 1;
        fl[q] = RC_PIV_EMPTY; vx[q] = vy[q] = 0.f;
        if (x >= 0 && y >= 0 && x < a.gx && y < a.gy) {
            const rc_piv_cell nb = a.raw[(size_t)y * a.gx + x];
            fl[q] = nb.flags; vx[q] = nb.dx; vy[q] = nb.dy;
        }
        if (!(fl[q] & PV_INVALID)) k++;
    }
    const int low = (8 - k) / 2;
    int pads = 0;
#pragma unroll
    for (int q = 0; q < 8; q++)
        if (fl[q] & PV_INVALID) vx[q] = vy[q] = pads++ < low ? -INFINITY : INFINITY;
    if (k < 3) return o;
    float um[2], res[2];
    res[0] = pv_residual(vx, k, me.dx, a.eps, um[0]);
    res[1] = pv_residual(vy, k, me.dy, a.eps, um[1]);
    o.resid = fmaxf(res[0], res[1]);
    if (o.resid > a.thr) {
        o.flags |= RC_PIV_OUTLIER;
        if (a.replace) { o.fx = um[0]; o.fy = um[1]; }
    }
    return o;
}

__global__ __launch_bounds__(RC_BLOCK) void k_pv_validate(const PvValArgs a) {
    __shared__ unsigned cnt[5];
    __shared__ int last;
    __shared__ uint8_t lut[768];
    __shared__ uint32_t colour[RC_BLOCK];
    if ((int)blockIdx.x < a.nbc) {
        // ---- a lane a cell
        if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
        __syncthreads();
        const int c = blockIdx.x * RC_BLOCK + threadIdx.x, ncell = a.gx * a.gy;
        if (c < ncell) {
            const int cy = c / a.gx, cx = c - cy * a.gx;
            const PvVal v = pv_validate(a, cx, cy);
            rc_piv_cell r = a.raw[c];
            r.flags = v.flags; r.resid = v.resid;
            a.cells[c] = r;
            if (a.cells2) a.cells2[c] = r;
            if (a.field) {
                float* f = (float*)((char*)a.field + (size_t)cy * a.field_step) + 2 * cx;
                f[0] = v.fx; f[1] = v.fy;
            }
            if (!(v.flags & PV_INVALID)) atomicAdd(&cnt[0], 1u);
            if (v.flags & RC_PIV_FLAT) atomicAdd(&cnt[1], 1u);
            if (v.flags & RC_PIV_LOWPEAK) atomicAdd(&cnt[2], 1u);
            if (v.flags & RC_PIV_EDGE) atomicAdd(&cnt[3], 1u);
            if (v.flags & RC_PIV_OUTLIER) atomicAdd(&cnt[4], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < 5; k++)
                if (cnt[k]) rc_acc_add(&a.ctl->cnt[k], cnt[k]);
            last = rc_ticket_fenced(&a.ctl->ticket, (unsigned)a.nbc);                 // the counts before the ticket
            if (last) {
                long long s[8] = {a.n, ncell, 0, 0, 0, 0, 0, a.pushes};
                for (int k = 0; k < 5; k++) s[2 + k] = rc_acc_take(&a.ctl->cnt[k]);     // zero for the next push (stream order)
                rc_acc_take(&a.ctl->ticket);
                for (int k = 0; k < 8; k++) {
                    a.summary[k] = s[k];
                    if (a.summary2) a.summary2[k] = s[k];
                }
            }
        }
        return;
    }
    // ---- a lane a pixel: first the cells the block's pixels lie in, a lane a cell
    const int b = blockIdx.x - a.nbc, bx = (a.w + 63) / 64, xb = (b % bx) * 64, yb = (b / bx) * PV_WAVES;
    rc_stage_jet(lut, a.jet);
    const int xa = max(xb, a.R), xe = min(xb + 63, a.w - 1), ya = max(yb, a.R), ye = min(yb + PV_WAVES - 1, a.h - 1);
    int cxa = 0, cya = 0, ncx = 0, ncy = 0;
    if (xa <= xe && ya <= ye) {
        cxa = min((xa - a.R) / a.step, a.gx - 1); ncx = min((xe - a.R) / a.step, a.gx - 1) - cxa + 1;
        cya = min((ya - a.R) / a.step, a.gy - 1); ncy = min((ye - a.R) / a.step, a.gy - 1) - cya + 1;
    }
    __syncthreads();
    if ((int)threadIdx.x < ncx * ncy) {                           // at most 64 x PV_WAVES
        const int cy = cya + threadIdx.x / ncx, cx = cxa + threadIdx.x % ncx;
        const PvVal v = pv_validate(a, cx, cy);
        uint32_t col = 0;
        if (!(v.flags & PV_INVALID)) {
            const float f = rintf(hypotf(v.fx, v.fy) / a.vis_max * 255.f);
            const int i = !(f > 0.f) ? 0 : (f > 255.f ? 255 : (int)f);
            col = lut[3 * i] | (uint32_t)lut[3 * i + 1] << 8 | (uint32_t)lut[3 * i + 2] << 16;
        }
        colour[threadIdx.x] = col;
    }
    __syncthreads();
    const int x = xb + (threadIdx.x & 63), y = yb + (threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    uint32_t col = 0;
    if (x >= a.R && y >= a.R) {
        const int cx = min((x - a.R) / a.step, a.gx - 1), cy = min((y - a.R) / a.step, a.gy - 1);
        col = colour[(cy - cya) * ncx + (cx - cxa)];
    }
    uint8_t* q = a.vis + (size_t)y * a.vis_step + 3 * (size_t)x;
    q[0] = (uint8_t)col; q[1] = (uint8_t)(col >> 8); q[2] = (uint8_t)(col >> 16);
}

// ============================================================================ host side
void rc_state_free(RcPiv& v) {
    rc_buf_free(v.prev); rc_buf_free(v.ring); rc_buf_free(v.acc); rc_buf_free(v.out); rc_buf_free(v.ctl); rc_buf_free(v.jet);
    rc_fence_free(v.zf);
    v = RcPiv();
}

// open and reset: the ring, the accumulators, the last push's outputs, the counters; the push count (no previous frame)
int rc_state_zero(RcSlot& s, RcPiv& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.ring, &v.acc, &v.out, &v.ctl});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static size_t pv_cells(const RcPiv& v) { return (size_t)v.gx * v.gy; }
// RcPiv::out: records before validation [cells] | records [cells] | summary 8 int64
static rc_piv_cell* pv_out_raw(const RcPiv& v) { return (rc_piv_cell*)v.out.p; }
static rc_piv_cell* pv_out_cells(const RcPiv& v) { return pv_out_raw(v) + pv_cells(v); }
static long long* pv_out_summary(const RcPiv& v) { return (long long*)(pv_out_cells(v) + pv_cells(v)); }

static bool pv_pos(double v) { return v > 0. && v <= 1.7976931348623157e308; }      // finite and > 0; NaN fails
static bool pv_set_ok(double min_peak, double eps, double thr, double vis_max) {
    return min_peak >= 0. && min_peak <= 1. && pv_pos(eps) && pv_pos(thr) && pv_pos(vis_max);
}

extern "C" int rcflow_piv_open(rc_ctx* ctx, int stream, int w, int h, const rc_piv_params* prm) {
    static const char* who = "rcflow_piv_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad frame size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    const int M = prm->window, R = prm->range, E = prm->ensemble;
    if (M < 8 || M > RC_PIV_MAX_WINDOW || M % 4 || R < 1 || R > RC_PIV_MAX_RANGE || prm->step < 1 || prm->step > M || E < 1 ||
        E > RC_PIV_MAX_ENSEMBLE || (long long)E * M * M > RC_PIV_MAX_PIXEL_PAIRS || (prm->flags & ~RC_PIV_REPLACE) ||
        !pv_set_ok(prm->min_peak, prm->median_eps, prm->median_thr, prm->vis_max)) {
        rc_set_error("%s: window a multiple of 4 in 8..%d, range 1..%d, step 1..window, ensemble 1..%d with ensemble * window^2 <= %d, "
                     "min_peak in [0, 1], median_eps, median_thr and vis_max finite and > 0, flags RC_PIV_REPLACE or 0", who, RC_PIV_MAX_WINDOW,
                     RC_PIV_MAX_RANGE, RC_PIV_MAX_ENSEMBLE, RC_PIV_MAX_PIXEL_PAIRS);
        return RC_EINVAL;
    }
    if (w < M + 2 * R || h < M + 2 * R) {
        rc_set_error("%s: a %d x %d frame is smaller than one search area of %d pixels", who, w, h, M + 2 * R);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcPiv n;
    n.w = w; n.h = h; n.prm = *prm;
    n.gx = (w - M - 2 * R) / prm->step + 1; n.gy = (h - M - 2 * R) / prm->step + 1;
    if ((long long)n.gx * n.gy > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: a grid of %d x %d cells (at most %d)", who, n.gx, n.gy, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    const int D = 2 * R + 1;
    n.nw = 3 * D * D + 2;
    n.pitch = (w + 3) & ~3;
    const unsigned long long nc = pv_cells(n), words = nc * n.nw, state = words * 8ull + (E > 1 ? words * 4ull * E : 0ull);
    if (state > RC_PIV_MAX_STATE_BYTES) {
        rc_set_error("%s: %llu cells of %d displacements over %d pairs are %llu bytes, more than RC_PIV_MAX_STATE_BYTES", who, nc, D * D, E, state);
        return RC_ESIZE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    rc = rc_buf_ensure(n.prev, (size_t)h * n.pitch);
    if (!rc && E > 1) rc = rc_buf_ensure(n.ring, (size_t)(words * 4ull * E));
    if (!rc) rc = rc_buf_ensure(n.acc, (size_t)(words * 8ull));
    if (!rc) rc = rc_buf_ensure(n.out, nc * 64 + 64);
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(PvCtl));
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    return rc_state_install(*s, s->piv, n, rc);
}

extern "C" int rcflow_piv_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, rc_piv_cell* d_cells, float* d_field,
                                   size_t field_step, uint8_t* d_vis, size_t vis_step, long long* d_summary) {
    static const char* who = "rcflow_piv_push_dev";
    RcSlot* s; RcPiv* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::piv, who, s, vp)) return rc;
    RcPiv& v = *vp;
    const int w = v.w, h = v.h, M = v.prm.window, R = v.prm.range, E = v.prm.ensemble, D = 2 * R + 1;
    const size_t nc = pv_cells(v);
    RcArgs a(who, w, h);
    a.image("d_gray", d_gray, step, 1, 1, RC_ARG_IN);
    a.array("d_cells", d_cells, nc * 32, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_field", d_field, field_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL, v.gx, v.gy);
    a.image("d_vis", d_vis, vis_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const long long pairs = v.pushes;                             // after this push: pushes + 1 frames
    if (pairs > 0) {
        PvCorrArgs p;
        p.A = (const uint8_t*)v.prev.p; p.a_step = (size_t)v.pitch;
        p.B = d_gray; p.b_step = step;
        p.ring = E > 1 ? (int*)v.ring.p + (size_t)((pairs - 1) % E) * nc * v.nw : nullptr;
        p.acc = (long long*)v.acc.p;
        p.M = M; p.R = R; p.D = D; p.step = v.prm.step; p.gx = v.gx; p.sw = M + 2 * R; p.nw = v.nw;
        p.Gm = (D + 3) / 4 + (v.prm.step % 4 ? 1 : 0);            // dwords of the strip in which a cell's D windows begin, at most
        p.tasks = D * p.Gm;
        // cells per block: as many as fill its lanes, within the LDS budget
        const auto lds = [&](int c) { return pv_lds_plan(c, M, p.sw, D, p.step, p.Gm).bytes; };
        p.cpb = RC_BLOCK / p.tasks;
        if (p.cpb > PV_MAX_CPB) p.cpb = PV_MAX_CPB;
        if (p.cpb > v.gx) p.cpb = v.gx;
        if (p.cpb < 1) p.cpb = 1;
        while (p.cpb > 1 && lds(p.cpb) > PV_LDS_BUDGET) p.cpb--;
        p.bpr = (v.gx + p.cpb - 1) / p.cpb;
        int threads = (p.cpb * p.tasks + 63) & ~63;
        if (threads > RC_BLOCK) threads = RC_BLOCK;
        // both frames' pixels under the cells once, the accumulators in and out, the ring slot in and out
        RcProfScope ps(ctx, s->cur, RC_K_PIV, 0, 2. * w * h + (double)nc * v.nw * (E > 1 ? 24. : 8.));
        hipLaunchKernelGGL(k_pv_correlate, dim3(p.bpr * v.gy), dim3(threads), lds(p.cpb), s->cur, p);
    }
    // the pushed frame is the next pair's A; the launch above has read the old one (stream order)
    RC_HIP(hipMemcpy2DAsync(v.prev.p, (size_t)v.pitch, d_gray, step, (size_t)w, h, hipMemcpyDeviceToDevice, s->cur));
    const long long pushes = v.pushes + 1;
    if (d_cells || d_field || d_vis || d_summary) {
        const int n = (int)(pairs < E ? pairs : E);
        {
            PvPeakArgs q;
            q.acc = (const long long*)v.acc.p; q.raw = pv_out_raw(v);
            q.ncell = (int)nc; q.M = M; q.R = R; q.D = D; q.nw = v.nw; q.n = n; q.min_peak = v.prm.min_peak;
            RcProfScope ps(ctx, s->cur, RC_K_PIV, 1, (double)nc * (v.nw * 8. + 32.));
            hipLaunchKernelGGL(k_pv_peak, dim3(((int)nc + PV_WAVES - 1) / PV_WAVES), dim3(RC_BLOCK), 0, s->cur, q);
        }
        {
            PvValArgs q;
            q.raw = pv_out_raw(v); q.cells = pv_out_cells(v); q.summary = pv_out_summary(v);
            q.cells2 = d_cells; q.summary2 = d_summary; q.field = d_field; q.field_step = field_step; q.vis = d_vis; q.vis_step = vis_step;
            q.jet = (const uint8_t*)v.jet.p; q.ctl = (PvCtl*)v.ctl.p;
            q.w = w; q.h = h; q.gx = v.gx; q.gy = v.gy; q.R = R; q.step = v.prm.step; q.replace = (v.prm.flags & RC_PIV_REPLACE) != 0; q.n = n;
            q.nbc = ((int)nc + RC_BLOCK - 1) / RC_BLOCK;
            q.eps = (float)v.prm.median_eps; q.thr = (float)v.prm.median_thr; q.vis_max = (float)v.prm.vis_max;
            q.pushes = pushes;
            const int nbp = d_vis ? ((w + 63) / 64) * ((h + PV_WAVES - 1) / PV_WAVES) : 0;
            RcProfScope ps(ctx, s->cur, RC_K_PIV, 2, (double)nc * (64. + (d_field ? 8. : 0.)) + (d_vis ? 3. * w * h : 0.));
            hipLaunchKernelGGL(k_pv_validate, dim3(q.nbc + nbp), dim3(RC_BLOCK), 0, s->cur, q);
        }
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                            // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_piv_read(rc_ctx* ctx, int stream, rc_piv_cell* cells, long long summary[8]) {
    RcSlot* s; RcPiv* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::piv, "rcflow_piv_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    if (cells) RC_HIP(hipMemcpyAsync(cells, pv_out_cells(*vp), pv_cells(*vp) * 32, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, pv_out_summary(*vp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_piv_sums_read(rc_ctx* ctx, int stream, long long* sums, long long* cell_sums) {
    RcSlot* s; RcPiv* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::piv, "rcflow_piv_sums_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = pv_cells(*vp), row = (size_t)vp->nw * 8, head = row - 16;
    if (sums) RC_HIP(hipMemcpy2DAsync(sums, head, vp->acc.p, row, head, nc, hipMemcpyDeviceToHost, s->cur));
    if (cell_sums) RC_HIP(hipMemcpy2DAsync(cell_sums, 16, (const char*)vp->acc.p + head, row, 16, nc, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_piv_set(rc_ctx* ctx, int stream, double min_peak, double median_eps, double median_thr, double vis_max) {
    RcSlot* s; RcPiv* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::piv, "rcflow_piv_set", s, vp)) return rc;
    if (!pv_set_ok(min_peak, median_eps, median_thr, vis_max)) {
        rc_set_error("rcflow_piv_set: min_peak in [0, 1], median_eps, median_thr and vis_max finite and > 0");
        return RC_EINVAL;
    }
    vp->prm.min_peak = min_peak; vp->prm.median_eps = median_eps; vp->prm.median_thr = median_thr; vp->prm.vis_max = vis_max;
    return RC_OK;
}

extern "C" int rcflow_piv_info(rc_ctx* ctx, int stream, rc_piv_info* info) {
    RcSlot* s; RcPiv* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::piv, "rcflow_piv_info", s, vp)) return rc;
    const RcPiv& v = *vp;
    if (!info) { rc_set_error("rcflow_piv_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->grid_x = v.gx; info->grid_y = v.gy;
    info->launches_per_push = RC_PIV_LAUNCHES;
    const long long pairs = v.pushes > 0 ? v.pushes - 1 : 0;
    info->pairs = (int)(pairs < v.prm.ensemble ? pairs : v.prm.ensemble);
    info->pushes = v.pushes;
    info->device_bytes = v.prev.bytes + v.ring.bytes + v.acc.bytes + v.out.bytes + v.ctl.bytes + v.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_piv_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::piv, "rcflow_piv_reset"); }
extern "C" int rcflow_piv_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::piv); }
