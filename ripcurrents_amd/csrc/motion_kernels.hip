// motion_kernels.hip -- motion templates: where are the waves going, from frame differences alone?
//
// globalOrientation (ripcurrents_module.cpp:319-359) is the reference's one use of OpenCV's motion templates
// (motempl::updateMotionHistory, calcMotionGradient, calcGlobalOrientation).  It zeroes the history on every call, so its
// "history" is one silhouette; here the history lives on the device from push to push and the reference's literal call is
// the flag RC_MOTION_FRESH.  include/rcflow.h ("motion templates") is the specification; tests/_motion_ref.py states it in
// numpy and the kernels are held to that bit for bit.  A push is three launches and nothing synchronises:
//   motion@0  update    pointwise: silhouette, history, the previous frame; a lane owns 4 consecutive pixels (one 16-byte
//                       access per history row, the state planes being pitched to 4 pixels);
//   motion@1  gradient  a workgroup per 64 x 16 tile, the tile plus a one-pixel halo in LDS with the coordinates clamped
//                       into the image (the replicate border, and what keeps a tile that leaves the image on two sides
//                       inside it); orientation, mask and picture; per cell the 12 bin counts, the masked pixels outside
//                       the bins and the maximum history.  The lanes of a wave are grouped by (cell, bin) with ballots, a
//                       group costs one atomic; the block's cells meet in LDS.  The launch's last-arriving workgroup turns
//                       the counts into peak bin, base and the weight's constants per cell and for the frame;
//   motion@2  sums      S, W and n_used per cell and for the frame as 64-bit integers (no order of addition), summed in
//                       registers while a wave stays in a cell row, per wave over the lanes of a cell, then one atomic
//                       each; the last-arriving workgroup writes the records and leaves the tables zero.
// The hand-off to a launch's last workgroup is rc_hand_off_fenced (rc_reduce.h): every thread's atomics, __threadfence, the
// block's barrier, one ticket; the finish reads the tables with atomic exchanges, where the adds were made.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_pix3.h"
#include "rc_reduce.h"

#define MT_WAVES 4
static_assert(RC_BLOCK == 64 * MT_WAVES, "a block is MT_WAVES waves");
#define MT_TW 64               // the gradient's tile: a wave is a row of it
#define MT_TH 16
#define MT_LDS_CELLS 32        // cells of a tile's footprint met in LDS; a larger footprint (cells of a few pixels) adds straight to memory
#define MT_WORDS 16            // per cell in memory: bins 0..11 | 12: masked pixels outside the bins | 13: bits of the maximum history | 2 unused
#define MT_USED 14
#define MT_MAX_SPAN 8          // cell columns of a wave's 256 pixels reduced over the wave; beyond: every lane adds for itself

// control words at the start of RcMotion::tab.  Each ticket has a 128-byte line of its own: every block adds to it.
struct MtCtl {
    RcTicketLine t1, t2;
    unsigned long long sil;         // pixels of this push's silhouette
    unsigned pad2[30];
};
static_assert(sizeof(MtCtl) == 384, "the tables start 384 bytes into the buffer");

// what the gradient's finish leaves per set (cells, then the frame) for the sums
struct MtInfo { float base, b, del, tsmax; int n_masked, peak, pad0, pad1; };
static_assert(sizeof(MtInfo) == 32 && sizeof(rc_motion_cell) == 40, "table strides");

typedef float mt_f4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte access to a 4-byte aligned row

// ============================================================================ motion@0: update
struct MtUpdArgs {
    const uint8_t* gray; size_t step;
    float* mhi; uint8_t* prev;           // [h][pitch]
    float* out; size_t out_step;         // the caller's history, or null
    MtCtl* ctl;
    int w, h, pitch, thr;
    float ts, delbound;
    int first, fresh;                    // no previous frame: an empty silhouette; RC_MOTION_FRESH: the history counts as zero
};

__global__ __launch_bounds__(RC_BLOCK) void k_mt_update(const MtUpdArgs a) {
    const int q = a.pitch >> 2;
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;       // at most 2^24 pixels: no overflow
    int cnt = 0;
    if (i < q * a.h) {
        const int y = i / q, x0 = 4 * (i - y * q), n = min(4, a.w - x0);      // n >= 1: pitch - w < 4
        const uint8_t* g = a.gray + (size_t)y * a.step + x0;
        uint32_t cw = 0;
        if (n == 4) __builtin_memcpy(&cw, g, 4);             // the caller's rows have any alignment
        else
            for (int k = 0; k < n; k++) cw |= (uint32_t)g[k] << (8 * k);
        const size_t o = (size_t)y * a.pitch + x0;
        const uint32_t pw = *(const uint32_t*)(a.prev + o);
        float4* mp = (float4*)(a.mhi + o);
        const float4 m4 = *mp;
        float m[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = (cw >> (8 * k)) & 255, p = (pw >> (8 * k)) & 255;
            const bool s = !a.first && k < n && abs(c - p) > a.thr;
            const float old = a.fresh ? 0.f : m[k];
            m[k] = s ? a.ts : (old < a.delbound ? 0.f : old);  // the columns past w hold zeros and stay zero
            cnt += s;
        }
        *(uint32_t*)(a.prev + o) = cw;
        *mp = make_float4(m[0], m[1], m[2], m[3]);
        if (a.out) {
            float* r = (float*)((char*)a.out + (size_t)y * a.out_step) + x0;
            if (n == 4) { mt_f4u v; v[0] = m[0]; v[1] = m[1]; v[2] = m[2]; v[3] = m[3]; *(mt_f4u*)r = v; }
            else
                for (int k = 0; k < n; k++) r[k] = m[k];
        }
    }
    cnt = (int)rc_wave_sum_lane0((long long)cnt);
    if ((threadIdx.x & 63) == 0 && cnt)
        rc_acc_add(&a.ctl->sil, (unsigned long long)cnt);
}

// ============================================================================ motion@1: gradient
struct MtGradArgs {
    const float* mhi;                    // [h][pitch]
    float* orient; uint8_t* mask;        // the state's planes, [h][pitch]
    float* o_orient; size_t o_orient_step;   // the caller's, or null
    uint8_t* o_mask; size_t o_mask_step;
    uint8_t* vis; size_t vis_step;
    MtCtl* ctl;
    unsigned* hist;                      // [cells][MT_WORDS]: zero between launches
    MtInfo* info;                        // [cells + 1]
    int w, h, pitch, gx, gy, cw, ch;
    float d1, d2, delbound, dur, a;      // (float)delta1, (float)delta2, the picture's bound and divisor, the weight's slope
    double duration;
    unsigned nblocks;
};

__device__ __forceinline__ MtInfo mt_info(const unsigned cnt[13], unsigned maxbits, const MtGradArgs& a) {
    int peak = 0, nm = (int)cnt[12];
    for (int k = 0; k < 12; k++) {
        nm += (int)cnt[k];
        if (cnt[k] > cnt[peak]) peak = k;                    // the lowest bin wins a tie
    }
    MtInfo f;
    f.tsmax = __uint_as_float(maxbits);
    f.base = (float)(peak * 30);
    f.b = (float)(1. - (double)f.tsmax * (double)a.a);
    f.del = (float)((double)f.tsmax - a.duration);
    f.n_masked = nm; f.peak = peak; f.pad0 = f.pad1 = 0;
    return f;
}

// by every thread of the last-arriving block: counts -> MtInfo per cell and for the frame; the counts are zero afterwards
__device__ void mt_grad_finish(const MtGradArgs& a, unsigned* fr /* [MT_USED] */) {
    const int ncell = a.gx * a.gy;
    if (threadIdx.x < MT_USED) fr[threadIdx.x] = 0;
    __syncthreads();
    for (int c = threadIdx.x; c < ncell; c += RC_BLOCK) {
        unsigned cnt[13];
        for (int k = 0; k < 13; k++) cnt[k] = rc_acc_take(a.hist + (size_t)c * MT_WORDS + k);
        const unsigned mb = rc_acc_take(a.hist + (size_t)c * MT_WORDS + 13);
        a.info[c] = mt_info(cnt, mb, a);
        for (int k = 0; k < 13; k++)
            if (cnt[k]) atomicAdd(&fr[k], cnt[k]);
        if (mb) atomicMax(&fr[13], mb);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned cnt[13];
    for (int k = 0; k < 13; k++) cnt[k] = fr[k];
    a.info[ncell] = mt_info(cnt, fr[13], a);
    __hip_atomic_store(&a.ctl->t1.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next push (stream order)
}

__global__ __launch_bounds__(RC_BLOCK) void k_mt_gradient(const MtGradArgs a) {
    __shared__ float tile[MT_TH + 2][MT_TW + 2];
    __shared__ unsigned tab[MT_LDS_CELLS * MT_USED];
    __shared__ unsigned fr[MT_USED];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * MT_TW, y0 = blockIdx.y * MT_TH;              // inside the frame by the grid's size
    // the tile and its halo; clamped coordinates are the replicate border, and never leave the image
    for (int i = threadIdx.x; i < (MT_TH + 2) * (MT_TW + 2); i += RC_BLOCK) {
        const int r = i / (MT_TW + 2), c = i - r * (MT_TW + 2);
        const int yy = rc_clampi(y0 - 1 + r, 0, a.h - 1), xx = rc_clampi(x0 - 1 + c, 0, a.w - 1);
        tile[r][c] = a.mhi[(size_t)yy * a.pitch + xx];
    }
    // the tile's footprint in cells; the remainder columns / rows belong to the last cell
    const int cxa = min(x0 / a.cw, a.gx - 1), cxb = min((min(x0 + MT_TW, a.w) - 1) / a.cw, a.gx - 1);
    const int cya = min(y0 / a.ch, a.gy - 1), cyb = min((min(y0 + MT_TH, a.h) - 1) / a.ch, a.gy - 1);
    const int nx = cxb - cxa + 1, ntab = nx * (cyb - cya + 1);
    const bool lds = ntab <= MT_LDS_CELLS;
    if (lds)
        for (int i = threadIdx.x; i < ntab * MT_USED; i += RC_BLOCK) tab[i] = 0;
    __syncthreads();

    const int x = x0 + lane;
    const bool inx = x < a.w;
    const int cx = min(min(x, a.w - 1) / a.cw, a.gx - 1);
    const float eps = 1e-4f * 9.f;
    for (int k = 0; k < MT_TH / MT_WAVES; k++) {
        const int ly = wv * (MT_TH / MT_WAVES) + k, y = y0 + ly;
        if (y >= a.h) break;                                  // the whole wave leaves
        const float p00 = tile[ly][lane], p01 = tile[ly][lane + 1], p02 = tile[ly][lane + 2];
        const float p10 = tile[ly + 1][lane], p11 = tile[ly + 1][lane + 1], p12 = tile[ly + 1][lane + 2];
        const float p20 = tile[ly + 2][lane], p21 = tile[ly + 2][lane + 1], p22 = tile[ly + 2][lane + 2];
        const float dx = ((p02 - p00) + 2.f * (p12 - p10)) + (p22 - p20);
        const float dy = ((p20 - p00) + 2.f * (p21 - p01)) + (p22 - p02);
        const float mn = fminf(fminf(fminf(p00, p01), fminf(p02, p10)), fminf(fminf(p11, p12), fminf(fminf(p20, p21), p22)));
        const float mx = fmaxf(fmaxf(fmaxf(p00, p01), fmaxf(p02, p10)), fmaxf(fmaxf(p11, p12), fmaxf(fmaxf(p20, p21), p22)));
        const float d0 = mx - mn;
        bool m = !(fabsf(dx) < eps && fabsf(dy) < eps);
        if (d0 < a.d1 || a.d2 < d0) m = false;
        const float ori = m ? rc_fast_atan2_deg(dy, dx) : 0.f;
        if (inx) {
            const size_t o = (size_t)y * a.pitch + x;
            a.orient[o] = ori;
            a.mask[o] = m ? 255 : 0;
            if (a.o_orient) ((float*)((char*)a.o_orient + (size_t)y * a.o_orient_step))[x] = ori;
            if (a.o_mask) a.o_mask[(size_t)y * a.o_mask_step + x] = m ? 255 : 0;
            if (a.vis) {
                const float v = p11 > a.delbound ? (p11 - a.delbound) / a.dur : 0.f;
                const float r = rintf(v * 255.f);
                const uint8_t b = r < 0.f ? 0 : (r > 255.f ? 255 : (uint8_t)r);
                uint8_t* q = a.vis + (size_t)y * a.vis_step + 3 * (size_t)x;
                q[0] = b; q[1] = b; q[2] = b;
            }
        }
        // the cell tables: lanes grouped by (cell, bin), one atomic per group and word
        const int cy = min(y / a.ch, a.gy - 1);
        const int idx = (int)floor((double)ori * (12.0 / 360.0));
        const int bin = idx >= 0 && idx < 12 ? idx : 12;
        const int slot = lds ? (cy - cya) * nx + (cx - cxa) : cy * a.gx + cx;
        const int key = inx && m ? slot * 16 + bin : -1;
        const unsigned bits = __float_as_uint(p11);           // the history is never negative: its bits order as integers
        unsigned long long rem = __ballot(key >= 0);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int kk = __shfl(key, leader, 64);
            const bool mine = key == kk;
            const unsigned long long grp = __ballot(mine);
            unsigned gmax = mine ? bits : 0u;
            gmax = rc_wave_max_all(gmax);
            if (lane == leader) {
                const int sl = kk >> 4, bn = kk & 15;
                const unsigned n = (unsigned)__popcll(grp);
                if (lds) {
                    atomicAdd(&tab[sl * MT_USED + bn], n);
                    atomicMax(&tab[sl * MT_USED + 13], gmax);
                } else {
                    unsigned* t = a.hist + (size_t)sl * MT_WORDS;
                    rc_acc_add(t + bn, n);
                    __hip_atomic_fetch_max(t + 13, gmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            rem &= ~grp;
        }
    }
    __syncthreads();
    if (lds)
        for (int i = threadIdx.x; i < ntab * MT_USED; i += RC_BLOCK) {
            const unsigned val = tab[i];
            if (!val) continue;
            const int c = i / MT_USED, k = i - c * MT_USED;
            unsigned* t = a.hist + ((size_t)(cya + c / nx) * a.gx + (cxa + c % nx)) * MT_WORDS + k;
            if (k < 13) rc_acc_add(t, val);
            else __hip_atomic_fetch_max(t, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    if (rc_hand_off_fenced(&a.ctl->t1.ticket, a.nblocks, &last)) mt_grad_finish(a, fr);
}

// ============================================================================ motion@2: sums
struct MtSumArgs {
    const float* mhi; const float* orient; const uint8_t* mask;   // [h][pitch]
    MtCtl* ctl;
    const MtInfo* info;                  // [cells + 1]
    long long* acc;                      // [cells + 1][S, W, n_used]: zero between launches
    rc_motion_cell* rec;                 // the state's records, [cells + 1]
    long long* sil_out;
    rc_motion_cell* cells2; rc_motion_cell* frame2;   // the caller's, or null
    int w, h, pitch, rows, gx, gy, cw, ch;
    float a;
    unsigned nblocks;
};

// one pixel's term for a set: false when the pixel is outside the set's time window or the 45-degree gate
__device__ __forceinline__ bool mt_term(float mhi, float ori, const MtInfo& f, float a, long long& qs, long long& qw) {
    if (!(mhi > f.del)) return false;
    const float t0 = mhi * a;
    const float wgt = t0 + f.b;
    float rel = ori - f.base;
    rel += rel < -180.f ? 360.f : 0.f;
    rel += rel > 180.f ? -360.f : 0.f;
    if (!(fabsf(rel) < 45.f)) return false;
    const float t = wgt * rel;
    qs = (long long)rint((double)t * 4294967296.0);           // |t| < 46: below 2^38
    qw = (long long)rint((double)wgt * 4294967296.0);
    return true;
}

// The wave's register sums of one cell row -> memory.  Cell columns cxa..cxb are the wave's.
__device__ __forceinline__ void mt_flush(const MtSumArgs& a, int cxa, int cxb, int cy, const int cxl[4], long long s[4], long long wq[4],
                                         int n[4]) {
    if (cxb - cxa < MT_MAX_SPAN) {
        for (int cx = cxa; cx <= cxb; cx++) {
            long long vs = 0, vw = 0, vn = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (cxl[k] == cx) { vs += s[k]; vw += wq[k]; vn += n[k]; }
            vs = rc_wave_sum_lane0(vs); vw = rc_wave_sum_lane0(vw); vn = rc_wave_sum_lane0(vn);
            if ((threadIdx.x & 63) == 0 && vn) {
                long long* t = a.acc + 3 * ((size_t)cy * a.gx + cx);
                rc_acc_add(t, vs); rc_acc_add(t + 1, vw); rc_acc_add(t + 2, vn);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (n[k]) {
                long long* t = a.acc + 3 * ((size_t)cy * a.gx + cxl[k]);
                rc_acc_add(t, s[k]); rc_acc_add(t + 1, wq[k]); rc_acc_add(t + 2, (long long)n[k]);
            }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { s[k] = 0; wq[k] = 0; n[k] = 0; }
}

// by every thread of the last-arriving block: the records; sums, silhouette count and ticket are zero afterwards
__device__ void mt_sum_finish(const MtSumArgs& a) {
    const int ncell = a.gx * a.gy;
    for (int c = threadIdx.x; c <= ncell; c += RC_BLOCK) {
        const long long S = rc_acc_take(a.acc + 3 * (size_t)c), W = rc_acc_take(a.acc + 3 * (size_t)c + 1), n = rc_acc_take(a.acc + 3 * (size_t)c + 2);
        const MtInfo f = a.info[c];                           // the previous launch's
        rc_motion_cell r;
        double ang = (double)f.base + (W ? (double)S / (double)W : 0.);
        if (ang >= 360.) ang -= 360.;
        if (ang < 0.) ang += 360.;
        r.angle = ang; r.S = S; r.W = W; r.tsmax = f.tsmax; r.n_masked = f.n_masked; r.n_used = (int)n; r.peak_bin = f.peak;
        a.rec[c] = r;
        if (c < ncell) { if (a.cells2) a.cells2[c] = r; }
        else if (a.frame2) *a.frame2 = r;
    }
    if (threadIdx.x != 0) return;
    *a.sil_out = (long long)rc_acc_take(&a.ctl->sil);
    __hip_atomic_store(&a.ctl->t2.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next push (stream order)
}

__global__ __launch_bounds__(RC_BLOCK) void k_mt_sums(const MtSumArgs a) {
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xb = blockIdx.x * 256, x0 = xb + 4 * lane;      // xb is inside the frame by the grid's size
    const bool live = x0 < a.w;                               // then x0 + 3 < pitch: the planes' rows are whole 4-pixel groups
    const int cxa = min(xb / a.cw, a.gx - 1), cxb = min((min(xb + 256, a.w) - 1) / a.cw, a.gx - 1);
    int cxl[4];
#pragma unroll
    for (int k = 0; k < 4; k++) cxl[k] = min(min(x0 + k, a.w - 1) / a.cw, a.gx - 1);
    const MtInfo fi = a.info[a.gx * a.gy];
    MtInfo ci[4];
    long long s[4] = {0, 0, 0, 0}, wq[4] = {0, 0, 0, 0}, fs = 0, fw = 0;
    int n[4] = {0, 0, 0, 0}, fn = 0;
    int cur_cy = -1;
    const int y0 = (blockIdx.y * MT_WAVES + wv) * a.rows;
    for (int r = 0; r < a.rows; r++) {
        const int y = y0 + r;
        if (y >= a.h) break;                                  // the whole wave leaves
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) mt_flush(a, cxa, cxb, cur_cy, cxl, s, wq, n);
            cur_cy = cy;
#pragma unroll
            for (int k = 0; k < 4; k++) ci[k] = a.info[(size_t)cy * a.gx + cxl[k]];
        }
        if (!live) continue;
        const size_t o = (size_t)y * a.pitch + x0;
        const uint32_t mk = *(const uint32_t*)(a.mask + o);
        if (!mk) continue;
        const float4 h4 = *(const float4*)(a.mhi + o), o4 = *(const float4*)(a.orient + o);
        const float hv[4] = {h4.x, h4.y, h4.z, h4.w}, ov[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!((mk >> (8 * k)) & 255)) continue;           // the columns past w hold zeros
            long long qs, qw;
            if (mt_term(hv[k], ov[k], ci[k], a.a, qs, qw)) { s[k] += qs; wq[k] += qw; n[k]++; }
            if (mt_term(hv[k], ov[k], fi, a.a, qs, qw)) { fs += qs; fw += qw; fn++; }
        }
    }
    if (cur_cy >= 0) mt_flush(a, cxa, cxb, cur_cy, cxl, s, wq, n);
    fs = rc_wave_sum_lane0(fs); fw = rc_wave_sum_lane0(fw);
    const long long fnn = rc_wave_sum_lane0((long long)fn);
    if (lane == 0 && fnn) {
        long long* t = a.acc + 3 * (size_t)(a.gx * a.gy);
        rc_acc_add(t, fs); rc_acc_add(t + 1, fw); rc_acc_add(t + 2, fnn);
    }
    if (rc_hand_off_fenced(&a.ctl->t2.ticket, a.nblocks, &last)) mt_sum_finish(a);
}

// ============================================================================ motion@3: primitives
__device__ __forceinline__ int mt_round(double v) { return (int)rint(v); }   // |v| <= RC_DRAW_COORD_MAX by the host's check

__global__ __launch_bounds__(RC_BLOCK) void k_mt_prims(const rc_motion_cell* rec, int w, int h, int gx, int gy, uint32_t color, int thickness,
                                                       int radius, double length, rc_draw_prim* out) {
    const int ncell = gx * gy, c = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (c > ncell) return;
    rc_draw_prim p[2];
    memset(p, 0, sizeof(p));
    const rc_motion_cell q = rec[c];
    if (q.W) {
        int px = (w - 1) / 2, py = (h - 1) / 2;
        if (c < ncell) {
            const int cw = w / gx, ch = h / gy, cx = c % gx, cy = c / gx;
            px = (cx * cw + (cx == gx - 1 ? w : (cx + 1) * cw) - 1) / 2;
            py = (cy * ch + (cy == gy - 1 ? h : (cy + 1) * ch) - 1) / 2;
        }
        const double rad = q.angle * (3.14159265358979323846 / 180.0);
        p[0].kind = RC_DRAW_DISC; p[0].x0 = p[0].x1 = px; p[0].y0 = p[0].y1 = py; p[0].size = radius; p[0].color = color;
        p[1].kind = RC_DRAW_LINE; p[1].x0 = px; p[1].y0 = py; p[1].x1 = px + mt_round(length * cos(rad)); p[1].y1 = py + mt_round(length * sin(rad));
        p[1].size = thickness; p[1].color = color;
    }
    out[2 * (size_t)c] = p[0];
    out[2 * (size_t)c + 1] = p[1];
}

// ============================================================================ host side
void rc_state_free(RcMotion& m) {
    rc_buf_free(m.mhi); rc_buf_free(m.prev); rc_buf_free(m.orient); rc_buf_free(m.mask); rc_buf_free(m.tab); rc_buf_free(m.out);
    rc_fence_free(m.zf);
    m = RcMotion();
}

// open and reset: the history, the previous frame, the planes, the tables and the records; the push count and the last stamp
int rc_state_zero(RcSlot& s, RcMotion& m) {
    const int rc = rc_fence_zero(m.zf, s.cur, {&m.mhi, &m.prev, &m.orient, &m.mask, &m.tab, &m.out});
    if (rc) return rc;
    m.pushes = 0;
    m.last_ts = 0.;
    return RC_OK;
}

static size_t mt_cells(const RcMotion& m) { return (size_t)m.prm.grid_x * m.prm.grid_y; }
// RcMotion::tab: MtCtl | counts [cells][MT_WORDS] | MtInfo [cells + 1] | sums [cells + 1][3] int64
static unsigned* mt_hist(const RcMotion& m) { return (unsigned*)((char*)m.tab.p + sizeof(MtCtl)); }
static MtInfo* mt_infos(const RcMotion& m) { return (MtInfo*)((char*)mt_hist(m) + mt_cells(m) * MT_WORDS * 4); }
static long long* mt_acc(const RcMotion& m) { return (long long*)(mt_infos(m) + mt_cells(m) + 1); }
// RcMotion::out: records [cells + 1] | the silhouette's pixels
static rc_motion_cell* mt_records(const RcMotion& m) { return (rc_motion_cell*)m.out.p; }
static long long* mt_sil(const RcMotion& m) { return (long long*)(mt_records(m) + mt_cells(m) + 1); }

static bool mt_positive(double v) { return v > 0. && v <= 1.7976931348623157e308; }      // NaN fails

extern "C" int rcflow_motion_open(rc_ctx* ctx, int stream, int w, int h, const rc_motion_params* prm) {
    static const char* who = "rcflow_motion_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad frame size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (prm->diff_threshold < 0 || prm->diff_threshold > 255 || !mt_positive(prm->duration) || !mt_positive(prm->delta1) ||
        !mt_positive(prm->delta2) || (prm->flags & ~RC_MOTION_FRESH)) {
        rc_set_error("%s: diff_threshold 0..255, duration and deltas finite and > 0, flags RC_MOTION_FRESH or 0", who);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d frame (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    if ((long long)w * h > RC_MOTION_MAX_PIXELS) {
        rc_set_error("%s: %d x %d is more than %d pixels, the bound of the integer sums", who, w, h, RC_MOTION_MAX_PIXELS);
        return RC_ESIZE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    RcMotion n;
    n.w = w; n.h = h; n.prm = *prm;
    if (n.prm.delta1 > n.prm.delta2) { n.prm.delta1 = prm->delta2; n.prm.delta2 = prm->delta1; }
    n.pitch = (w + 3) & ~3;
    const size_t plane = (size_t)n.pitch * h, nc = mt_cells(n);
    rc = rc_buf_ensure(n.mhi, plane * 4);
    if (!rc) rc = rc_buf_ensure(n.prev, plane);
    if (!rc) rc = rc_buf_ensure(n.orient, plane * 4);
    if (!rc) rc = rc_buf_ensure(n.mask, plane);
    if (!rc) rc = rc_buf_ensure(n.tab, sizeof(MtCtl) + nc * MT_WORDS * 4 + (nc + 1) * (sizeof(MtInfo) + 24));
    if (!rc) rc = rc_buf_ensure(n.out, (nc + 1) * sizeof(rc_motion_cell) + 8);
    return rc_state_install(*s, s->mt, n, rc);
}

extern "C" int rcflow_motion_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, double timestamp, float* d_mhi,
                                      size_t mhi_step, float* d_orient, size_t orient_step, uint8_t* d_mask, size_t mask_step, uint8_t* d_vis,
                                      size_t vis_step, rc_motion_cell* d_cells, rc_motion_cell* d_frame) {
    static const char* who = "rcflow_motion_push_dev";
    RcSlot* s; RcMotion* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mt, who, s, mp)) return rc;
    RcMotion& m = *mp;
    const int w = m.w, h = m.h;
    const double ts = timestamp == RC_MOTION_AUTO_TIME ? (double)(m.pushes + 1) : timestamp;
    if (!(ts >= 0. && ts <= 16777216.)) { rc_set_error("%s: the timestamp must be RC_MOTION_AUTO_TIME or in 0..2^24", who); return RC_EINVAL; }
    if (m.pushes > 0 && !(ts > m.last_ts)) {
        rc_set_error("%s: timestamp %.17g is not greater than the last push's %.17g", who, ts, m.last_ts);
        return RC_EINVAL;
    }
    RcArgs a(who, w, h);
    a.image("d_gray", d_gray, step, 1, 1, RC_ARG_IN);
    a.image("d_mhi", d_mhi, mhi_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_orient", d_orient, orient_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_vis", d_vis, vis_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_cells", d_cells, mt_cells(m) * sizeof(rc_motion_cell), 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_frame", d_frame, sizeof(rc_motion_cell), 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(m.zf, s->cur, true);
    if (rc) return rc;
    const bool fresh = (m.prm.flags & RC_MOTION_FRESH) != 0;
    const double stamp = fresh ? 1. : ts, duration = fresh ? 1. : m.prm.duration;
    const float delbound = (float)(stamp - duration);
    const double px = (double)w * h;
    MtCtl* ctl = (MtCtl*)m.tab.p;
    {
        MtUpdArgs a;
        a.gray = d_gray; a.step = step;
        a.mhi = (float*)m.mhi.p; a.prev = (uint8_t*)m.prev.p;
        a.out = d_mhi; a.out_step = mhi_step;
        a.ctl = ctl;
        a.w = w; a.h = h; a.pitch = m.pitch; a.thr = m.prm.diff_threshold;
        a.ts = (float)stamp; a.delbound = delbound;
        a.first = m.pushes == 0; a.fresh = fresh;
        const int items = (m.pitch / 4) * h;
        // gray 1 + previous 1 + history 4 in, history 4 + previous 1 out
        RcProfScope ps(ctx, s->cur, RC_K_MOTION, 0, px * (11. + (d_mhi ? 4. : 0.)));
        hipLaunchKernelGGL(k_mt_update, dim3((items + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, a);
    }
    const int gx = m.prm.grid_x, gy = m.prm.grid_y;
    const float wa = (float)(254. / 255. / duration);
    {
        MtGradArgs a;
        a.mhi = (const float*)m.mhi.p; a.orient = (float*)m.orient.p; a.mask = (uint8_t*)m.mask.p;
        a.o_orient = d_orient; a.o_orient_step = orient_step;
        a.o_mask = d_mask; a.o_mask_step = mask_step;
        a.vis = d_vis; a.vis_step = vis_step;
        a.ctl = ctl; a.hist = mt_hist(m); a.info = mt_infos(m);
        a.w = w; a.h = h; a.pitch = m.pitch; a.gx = gx; a.gy = gy; a.cw = w / gx; a.ch = h / gy;
        a.d1 = (float)m.prm.delta1; a.d2 = (float)m.prm.delta2; a.delbound = delbound; a.dur = (float)duration; a.a = wa;
        a.duration = duration;
        const dim3 grid((w + MT_TW - 1) / MT_TW, (h + MT_TH - 1) / MT_TH);
        a.nblocks = grid.x * grid.y;
        // history 4 in, orientation 4 + mask 1 out
        RcProfScope ps(ctx, s->cur, RC_K_MOTION, 1, px * (9. + (d_orient ? 4. : 0.) + (d_mask ? 1. : 0.) + (d_vis ? 3. : 0.)));
        hipLaunchKernelGGL(k_mt_gradient, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    {
        MtSumArgs a;
        a.mhi = (const float*)m.mhi.p; a.orient = (const float*)m.orient.p; a.mask = (const uint8_t*)m.mask.p;
        a.ctl = ctl; a.info = mt_infos(m); a.acc = mt_acc(m);
        a.rec = mt_records(m); a.sil_out = mt_sil(m);
        a.cells2 = d_cells; a.frame2 = d_frame;
        a.w = w; a.h = h; a.pitch = m.pitch; a.rows = rc_rows_per_wave(w, h, 4);
        a.gx = gx; a.gy = gy; a.cw = w / gx; a.ch = h / gy;
        a.a = wa;
        const dim3 grid((w + 255) / 256, (h + MT_WAVES * a.rows - 1) / (MT_WAVES * a.rows));
        a.nblocks = grid.x * grid.y;
        RcProfScope ps(ctx, s->cur, RC_K_MOTION, 2, px * 9.);
        hipLaunchKernelGGL(k_mt_sums, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    m.pushes++;                                           // a launch that failed is not a push
    m.last_ts = ts;
    return RC_OK;
}

extern "C" int rcflow_motion_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, double length,
                                       rc_draw_prim* d_prims) {
    static const char* who = "rcflow_motion_prims_dev";
    RcSlot* s; RcMotion* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mt, who, s, mp)) return rc;
    RcMotion& m = *mp;
    if (rc_prims_check(who, d_prims, thickness, disc_radius)) return RC_EINVAL;
    if (!(fabs(length) <= (double)RC_DRAW_COORD_MAX)) { rc_set_error("%s: |length| <= %d", who, RC_DRAW_COORD_MAX); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(m.zf, s->cur, true);
    if (rc) return rc;
    const int sets = (int)mt_cells(m) + 1;
    RcProfScope ps(ctx, s->cur, RC_K_MOTION, 3, (double)sets * (sizeof(rc_motion_cell) + 2. * sizeof(rc_draw_prim)));
    hipLaunchKernelGGL(k_mt_prims, dim3((sets + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, mt_records(m), m.w, m.h, m.prm.grid_x,
                       m.prm.grid_y, color, thickness, disc_radius, length, d_prims);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_motion_read(rc_ctx* ctx, int stream, rc_motion_cell* cells, int cap, rc_motion_cell* frame, long long* silhouette) {
    RcSlot* s; RcMotion* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mt, "rcflow_motion_read", s, mp)) return rc;
    RcMotion& m = *mp;
    if (cap < 0 || (cap && !cells)) { rc_set_error("rcflow_motion_read: a bad buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(m.zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = mt_cells(m), take = (size_t)cap < nc ? (size_t)cap : nc;
    if (take) RC_HIP(hipMemcpyAsync(cells, mt_records(m), take * sizeof(rc_motion_cell), hipMemcpyDeviceToHost, s->cur));
    if (frame) RC_HIP(hipMemcpyAsync(frame, mt_records(m) + nc, sizeof(rc_motion_cell), hipMemcpyDeviceToHost, s->cur));
    if (silhouette) RC_HIP(hipMemcpyAsync(silhouette, mt_sil(m), 8, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_motion_info(rc_ctx* ctx, int stream, rc_motion_info* info) {
    RcSlot* s; RcMotion* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::mt, "rcflow_motion_info", s, mp)) return rc;
    const RcMotion& m = *mp;
    if (!info) return RC_OK;
    memset(info, 0, sizeof(*info));
    info->w = m.w; info->h = m.h; info->prm = m.prm;
    info->launches_per_push = RC_MOTION_LAUNCHES;
    info->pushes = m.pushes;
    info->last_timestamp = m.last_ts;
    info->device_bytes = m.mhi.bytes + m.prev.bytes + m.orient.bytes + m.mask.bytes + m.tab.bytes + m.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_motion_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::mt, "rcflow_motion_reset"); }
extern "C" int rcflow_motion_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::mt); }
