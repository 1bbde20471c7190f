// planview_kernels.hip -- plan view: the flow in metres per second, and the frame, on a regular grid on the water.
//
// Every product made from the flow works in image pixels, and a shore camera looks along the water at a shallow angle: a
// current 150 m out moves a fifth of the pixels the same current moves at 30 m.  This product resamples the field and the
// frame onto a ground grid through the camera's ground-to-image map, radial distortion included, and pushes the sampled
// vector through the inverse of the map's Jacobian, so that everything downstream (ripmap, regions, tracks, ftle: each takes
// any 32FC2 field) is metric without a line of change.  include/rcflow.h ("plan view") is the specification;
// tests/_planview_ref.py states it in numpy and both kernels are held to that bit for bit.
//   planview@0  table   once, by open: per cell the image position of its centre and the inverse Jacobian from central
//                       differences over one cell, all in double, each operation rounded on its own (only + - * /, fabs and
//                       sqrt); stored as eight floats, 32 bytes: U, V, m00, m01, m10, m11, gsd, 1; eight zeros where the
//                       cell is not usable, which the sampler's own test then rejects (U = 0);
//   planview@1  push    the only launch of a push.  A wave is 64 consecutive cells of a plan row, and walks several rows
//                       once the plan has more than PV_MAX_BLOCKS blocks of four.  Per cell the record as two 16-byte
//                       loads, the sampler of rc_sample_flow with the two texels of a row as one 16-byte load (8-byte
//                       aligned: the form of ftle@1), two multiplies and an add per component, the warps' 8-bit sample for
//                       the picture; counts by ballot and popcount, the maximum as integer bits, a block's sums met in
//                       LDS, three atomics per block on its shard's three lines, and the last-arriving block writes the
//                       summary and leaves the counters zero (a ticket without a fence: see the closing).

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_pix3.h"
#include "rc_reduce.h"

#define PV_WAVES 4
static_assert(RC_BLOCK == 64 * PV_WAVES, "a block is PV_WAVES waves");
#define PV_MAX_BLOCKS 4096     // planview@1: a wave walks several rows from here on (measured 512 .. 4096: DESIGN 7l)

// RcPlanView::ctl.  The three words a block adds to, each on a 128-byte line of its own; a set per shard and one on top.
// One word takes some 90 atomics a microsecond however many blocks queue for it, so a block arrives at the shard of its
// number modulo PV_SHARDS (blocks are handed to the eight XCDs in turn) and only a shard's last block goes on to the top
struct PvLines {
    unsigned long long cells; unsigned pad0[30];              // usable | seen << 32
    unsigned maxbits; unsigned pad1[31];
    unsigned long long ticket; unsigned pad2[30];             // valid | arrivals << 32
};
#define PV_SHARDS 8
struct PvCtl { PvLines shard[PV_SHARDS], top; };
static_assert(sizeof(PvLines) == 384, "three lines");
struct PvSums { unsigned usable, seen, valid, maxbits; };

typedef float pv_f4 __attribute__((ext_vector_type(4), aligned(8)));   // the two texels of a sampler row

// ============================================================================ planview@0: the table
struct PvProj { double U, V; bool ok; };

// ground point -> distorted pixel; ok: in front of the camera and before the fold of the distortion
__device__ __forceinline__ PvProj pv_project(const rc_planview_params& p, double X, double Y) {
    const double px = p.H[0] * X + p.H[1] * Y + p.H[2], py = p.H[3] * X + p.H[4] * Y + p.H[5], pz = p.H[6] * X + p.H[7] * Y + p.H[8];
    const double u = px / pz, v = py / pz;
    const double xn = (u - p.cx) / p.fx, yn = (v - p.cy) / p.fy;
    const double r2 = xn * xn + yn * yn, r4 = r2 * r2;
    const double s = 1. + p.k1 * r2 + p.k2 * r4, g = 1. + 3. * p.k1 * r2 + 5. * p.k2 * r4;
    PvProj o;
    o.U = p.cx + p.fx * (xn * s);
    o.V = p.cy + p.fy * (yn * s);
    o.ok = pz > 0. && g > 0.;                                 // NaN fails
    return o;
}

__global__ __launch_bounds__(RC_BLOCK) void k_pv_table(const rc_planview_params p, float4* table) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * PV_WAVES + (threadIdx.x >> 6);
    if (i >= p.nx || j >= p.ny) return;
    const double X = p.x0 + (double)i * p.dx, Y = p.y0 + (double)j * p.dy;
    const double hx = 0.5 * p.dx, hy = 0.5 * p.dy;
    const PvProj C = pv_project(p, X, Y), E = pv_project(p, X + hx, Y), W = pv_project(p, X - hx, Y);
    const PvProj S = pv_project(p, X, Y + hy), N = pv_project(p, X, Y - hy);
    const double a = (E.U - W.U) / p.dx, b = (S.U - N.U) / p.dy, c = (E.V - W.V) / p.dx, d = (S.V - N.V) / p.dy;
    const double det = a * d - b * c;
    const double m00 = d / det * p.fps, m01 = -b / det * p.fps, m10 = -c / det * p.fps, m11 = a / det * p.fps;
    const double gsd = sqrt(fabs(1. / det));
    const bool usable = C.ok && E.ok && W.ok && S.ok && N.ok && rc_finite(C.U) && rc_finite(C.V) && rc_finite(det) && rc_finite(m00) &&
                        rc_finite(m01) && rc_finite(m10) && rc_finite(m11) && rc_finite(gsd) && det != 0. && gsd <= p.max_gsd;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (usable) {
        r0 = make_float4((float)C.U, (float)C.V, (float)m00, (float)m01);
        r1 = make_float4((float)m10, (float)m11, (float)gsd, 1.f);
    }
    float4* q = table + 2 * ((size_t)j * p.nx + i);
    q[0] = r0;
    q[1] = r1;
}

// ============================================================================ planview@1: the push
struct PvPushArgs {
    const float4* table;                 // [ny][nx] records of two float4
    const float* flow; size_t flow_step; // 32FC2 w x h, or null
    const uint8_t* bgr; size_t bgr_step; // 8UC3 w x h, or null
    float* o_plan; size_t o_plan_step;   // the caller's, each or null
    uint8_t* o_mask; size_t o_mask_step;
    uint8_t* o_bgr; size_t o_bgr_step;
    PvCtl* ctl;
    long long* rec; long long* rec2;     // the state's summary; the caller's, or null
    int w, h, nx, ny;
    int rows;                            // a wave walks `rows` rows, PV_WAVES apart
    long long pushes;
    unsigned nblocks;
};

// The closing, without a fence: rc_reduce.h says why a launch that has just dirtied all of its output wants none, what gfx950
// gives instead and what a port needs (DESIGN 7l has the times).  Here a block's ticket is made from the values its two other
// atomics returned (`dep`, always 0: a count has no bit 63, the bits of a number that is no NaN and not negative no bit 31), so it
// is issued after they were performed; the last block's exchanges are issued after its ticket returned (the branch).  The valid
// count rides on the ticket word itself.
// Adds s to the lines; true for the last of n arrivals, which gets the totals in s and leaves the lines zero.
__device__ __forceinline__ bool pv_arrive(PvLines* L, PvSums& s, unsigned n) {
    const unsigned long long c0 =
        rc_acc_add_old(&L->cells, (unsigned long long)s.usable | ((unsigned long long)s.seen << 32));
    const unsigned m0 = s.maxbits ? __hip_atomic_fetch_max(&L->maxbits, s.maxbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const unsigned long long dep = (c0 >> 63) | (unsigned long long)(m0 >> 31);
    const unsigned long long t =
        rc_acc_add_old(&L->ticket, ((1ull << 32) | (unsigned long long)s.valid) + dep);
    if ((unsigned)(t >> 32) != n - 1u) return false;
    const unsigned long long c = rc_acc_take(&L->cells);
    s.usable = (unsigned)c;
    s.seen = (unsigned)(c >> 32);
    s.valid += (unsigned)t;
    s.maxbits = rc_acc_take(&L->maxbits);
    __hip_atomic_store(&L->ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next arrivals (stream order)
    return true;
}

__global__ __launch_bounds__(RC_BLOCK) void k_pv_push(const PvPushArgs a) {
    __shared__ unsigned sums[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    if (threadIdx.x < 4) sums[threadIdx.x] = 0;
    __syncthreads();
    unsigned nu = 0, ns = 0, nv = 0, mb = 0;                  // the wave's sums over its rows (mb: per lane until the end)
    for (int r = 0; r < a.rows; r++) {
        const int y = (blockIdx.y * a.rows + r) * PV_WAVES + wv;
        if (y >= a.ny) break;                                 // the whole wave leaves
        const bool in = x < a.nx;
        float4 t0 = make_float4(0.f, 0.f, 0.f, 0.f), t1 = t0;
        if (in) {
            const float4* q = a.table + 2 * ((size_t)y * a.nx + x);
            t0 = q[0];
            t1 = q[1];
        }
        const float U = t0.x, V = t0.y;
        const int xind = rc_cvt_i32_x86(floorf(U)), yind = rc_cvt_i32_x86(floorf(V));
        const bool seen = in && !(xind < 1 || yind < 1 || xind + 2 > a.w || yind + 2 > a.h);   // a zero record: xind = 0
        bool valid = false;
        float Vx = 0.f, Vy = 0.f;
        if (seen && a.flow) {                                 // 1 <= xind, xind + 1 <= w - 1; 1 <= yind, yind + 1 <= h - 1
            const float xrem = U - xind, yrem = V - yind;
            const float2* q = rc_row2(a.flow, a.flow_step, yind) + xind;
            const pv_f4 r0 = *(const pv_f4*)q;
            const pv_f4 r1 = *(const pv_f4*)((const char*)q + a.flow_step);
            // p00 = r0.xy, p01 = r0.zw, p10 = r1.xy, p11 = r1.zw: the products and additions in rc_sample_flow's order
            const float wa = 1 - xrem, wb = 1 - yrem;
            const float sx = r0[0] * wa * wb + r0[2] * xrem * wb + r1[0] * wa * yrem + r1[2] * xrem * yrem;
            const float sy = r0[1] * wa * wb + r0[3] * xrem * wb + r1[1] * wa * yrem + r1[3] * xrem * yrem;
            valid = fabsf(sx) <= 3.4028234663852886e38f && fabsf(sy) <= 3.4028234663852886e38f;   // NaN fails
            if (valid) {
                Vx = t0.z * sx + t0.w * sy;
                Vy = t1.x * sx + t1.y * sy;
                const float m2 = Vx * Vx + Vy * Vy;
                if (m2 == m2) mb = max(mb, __float_as_uint(m2));                    // m2 >= 0: its bits order as integers
            }
        }
        if (in) {
            if (a.o_plan) ((float2*)((char*)a.o_plan + (size_t)y * a.o_plan_step))[x] = make_float2(Vx, Vy);
            if (a.o_mask) a.o_mask[(size_t)y * a.o_mask_step + x] = valid ? 255 : 0;
            if (a.o_bgr) {
                uint32_t o = 0u;
                if (seen) {
                    const int ix = (int)rintf(U * 32.f), iy = (int)rintf(V * 32.f);
                    const int sx = ix >> 5, sy = iy >> 5;
                    uint32_t p00, p01, p10, p11;
                    if (sx + 2 < a.w && sy + 1 < a.h) {        // sx, sy >= 1; two pixels = 6 of the 8 bytes, and pixel sx + 2 exists
                        const uint8_t* s0 = a.bgr + (size_t)sy * a.bgr_step + 3 * (size_t)sx;
                        rc_pix3_unpack2(s0, p00, p01);
                        rc_pix3_unpack2(s0 + a.bgr_step, p10, p11);
                    } else {
                        p00 = rc_pix3_tap(a.bgr, a.bgr_step, a.w, a.h, sx, sy); p01 = rc_pix3_tap(a.bgr, a.bgr_step, a.w, a.h, sx + 1, sy);
                        p10 = rc_pix3_tap(a.bgr, a.bgr_step, a.w, a.h, sx, sy + 1); p11 = rc_pix3_tap(a.bgr, a.bgr_step, a.w, a.h, sx + 1, sy + 1);
                    }
                    o = rc_pix3_bilinear(p00, p01, p10, p11, ix & 31, iy & 31);
                }
                uint8_t* q = a.o_bgr + (size_t)y * a.o_bgr_step + 3 * (size_t)x;
                q[0] = (uint8_t)o; q[1] = (uint8_t)(o >> 8); q[2] = (uint8_t)(o >> 16);
            }
        }
        nu += (unsigned)__popcll(__ballot(t1.w != 0.f)); ns += (unsigned)__popcll(__ballot(seen)); nv += (unsigned)__popcll(__ballot(valid));
    }
    // the integer sums: per wave, then the block's in LDS, then one atomic per counter
    mb = rc_wave_max_all(mb);
    if (lane == 0) {
        if (nu) atomicAdd(&sums[0], nu);
        if (ns) atomicAdd(&sums[1], ns);
        if (nv) atomicAdd(&sums[2], nv);
        if (mb) atomicMax(&sums[3], mb);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    PvSums t;
    t.usable = sums[0]; t.seen = sums[1]; t.valid = sums[2]; t.maxbits = sums[3];
    const unsigned bid = blockIdx.y * gridDim.x + blockIdx.x, g = bid % PV_SHARDS;
    if (!pv_arrive(&a.ctl->shard[g], t, (a.nblocks - g + PV_SHARDS - 1) / PV_SHARDS)) return;      // blocks g, g + PV_SHARDS, ...
    if (!pv_arrive(&a.ctl->top, t, min(a.nblocks, (unsigned)PV_SHARDS))) return;
    const long long r[8] = {(long long)t.usable, (long long)t.seen, (long long)t.valid, (long long)t.maxbits, a.pushes, 0, 0, 0};
    for (int k = 0; k < 8; k++) {
        a.rec[k] = r[k];
        if (a.rec2) a.rec2[k] = r[k];
    }
}

// ============================================================================ host side
void rc_state_free(RcPlanView& v) {
    rc_buf_free(v.table); rc_buf_free(v.ctl); rc_buf_free(v.out);
    rc_fence_free(v.zf);
    v = RcPlanView();
}

// open and reset: the counters, the summary and the push count.  The table is written by open's own launch, before the
// fence's event on the same stream, and reset keeps it
int rc_state_zero(RcSlot& s, RcPlanView& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.ctl, &v.out});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static bool pv_host_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }   // NaN fails

extern "C" int rcflow_planview_open(rc_ctx* ctx, int stream, int w, int h, const rc_planview_params* prm) {
    static const char* who = "rcflow_planview_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad image size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    bool fin = true;
    for (int k = 0; k < 9; k++) fin = fin && pv_host_finite(prm->H[k]);
    for (double v : {prm->fx, prm->fy, prm->cx, prm->cy, prm->k1, prm->k2, prm->x0, prm->y0, prm->dx, prm->dy, prm->fps}) fin = fin && pv_host_finite(v);
    if (!fin || !(prm->fx > 0.) || !(prm->fy > 0.) || prm->dx == 0. || prm->dy == 0. || !(prm->fps > 0.) || !(prm->max_gsd > 0.) ||
        prm->nx < 1 || prm->ny < 1 || prm->flags) {
        rc_set_error("%s: H, fx, fy, cx, cy, k1, k2, x0, y0, dx, dy and fps finite, fx, fy and fps > 0, dx and dy not 0, max_gsd > 0 "
                     "(+inf: no cut), nx and ny >= 1, flags 0", who);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (!rc) rc = rc_fits_context(who, ctx, prm->nx, prm->ny);
    if (rc) return rc;
    if ((long long)prm->nx * prm->ny > RC_PLANVIEW_MAX_CELLS) {
        rc_set_error("%s: a plan of %d x %d is more than RC_PLANVIEW_MAX_CELLS cells", who, prm->nx, prm->ny);
        return RC_ESIZE;
    }
    RcPlanView n;
    n.w = w; n.h = h; n.prm = *prm;
    RC_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)prm->nx * prm->ny;
    rc = rc_buf_ensure(n.table, cells * 32);
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(PvCtl));
    if (!rc) rc = rc_buf_ensure(n.out, 64);
    if (!rc) {
        {
            RcProfScope ps(ctx, s->cur, RC_K_PLANVIEW, 0, (double)cells * 32.);
            hipLaunchKernelGGL(k_pv_table, dim3((prm->nx + 63) / 64, (prm->ny + PV_WAVES - 1) / PV_WAVES), dim3(RC_BLOCK), 0, s->cur, *prm,
                               (float4*)n.table.p);
        }
        if (hipGetLastError() != hipSuccess) { rc_set_error("%s: the table's launch failed", who); rc = RC_EHIP; }
    }
    return rc_state_install(*s, s->pv, n, rc);
}

extern "C" int rcflow_planview_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, const uint8_t* d_bgr, size_t bgr_step,
                                        float* d_plan_xy, size_t plan_step, uint8_t* d_mask, size_t mask_step, uint8_t* d_plan_bgr,
                                        size_t plan_bgr_step, long long* d_summary) {
    static const char* who = "rcflow_planview_push_dev";
    RcSlot* s; RcPlanView* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::pv, who, s, vp)) return rc;
    RcPlanView& v = *vp;
    const int w = v.w, h = v.h, nx = v.prm.nx, ny = v.prm.ny;
    if (!d_flow_xy && !d_bgr) { rc_set_error("%s: neither the field nor the frame", who); return RC_EINVAL; }
    if (!d_flow_xy && (d_plan_xy || d_mask || d_summary)) { rc_set_error("%s: d_plan_xy, d_mask and d_summary need the field", who); return RC_EINVAL; }
    if (!d_bgr && d_plan_bgr) { rc_set_error("%s: d_plan_bgr needs the frame", who); return RC_EINVAL; }
    RcArgs a(who, w, h);
    a.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN | RC_ARG_OPTIONAL);
    a.image("d_bgr", d_bgr, bgr_step, 3, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    a.image("d_plan_xy", d_plan_xy, plan_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL, nx, ny);
    a.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL, nx, ny);
    a.image("d_plan_bgr", d_plan_bgr, plan_bgr_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL, nx, ny);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const long long pushes = v.pushes + 1;
    PvPushArgs p;
    p.table = (const float4*)v.table.p;
    p.flow = d_flow_xy; p.flow_step = flow_step; p.bgr = d_bgr; p.bgr_step = bgr_step;
    p.o_plan = d_plan_xy; p.o_plan_step = plan_step; p.o_mask = d_mask; p.o_mask_step = mask_step;
    p.o_bgr = d_plan_bgr; p.o_bgr_step = plan_bgr_step;
    p.ctl = (PvCtl*)v.ctl.p; p.rec = (long long*)v.out.p; p.rec2 = d_summary;
    p.w = w; p.h = h; p.nx = nx; p.ny = ny;
    p.pushes = pushes;
    const int gx = (nx + 63) / 64, gy1 = (ny + PV_WAVES - 1) / PV_WAVES;
    p.rows = (int)(((long long)gx * gy1 + PV_MAX_BLOCKS - 1) / PV_MAX_BLOCKS);
    const dim3 grid(gx, (gy1 + p.rows - 1) / p.rows);
    p.nblocks = grid.x * grid.y;
    {
        // per cell: the record 32 in, the gather's two rows of 16, the plan 8 and the mask 1 out; the picture 12 in and 3 out
        RcProfScope ps(ctx, s->cur, RC_K_PLANVIEW, 1, (double)nx * ny * (32. + (d_flow_xy ? 32. : 0.) + (d_plan_xy ? 8. : 0.) + (d_mask ? 1. : 0.) +
                                                                      (d_plan_bgr ? 15. : 0.)));
        hipLaunchKernelGGL(k_pv_push, grid, dim3(RC_BLOCK), 0, s->cur, p);
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_planview_read(rc_ctx* ctx, int stream, long long summary[8]) {
    RcSlot* s; RcPlanView* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::pv, "rcflow_planview_read", s, vp)) return rc;
    if (!summary) { rc_set_error("rcflow_planview_read: no buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    RC_HIP(hipMemcpyAsync(summary, vp->out.p, 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_planview_table_read(rc_ctx* ctx, int stream, float* table) {
    RcSlot* s; RcPlanView* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::pv, "rcflow_planview_table_read", s, vp)) return rc;
    if (!table) { rc_set_error("rcflow_planview_table_read: no buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    RC_HIP(hipMemcpyAsync(table, vp->table.p, (size_t)vp->prm.nx * vp->prm.ny * 32, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_planview_info(rc_ctx* ctx, int stream, rc_planview_info* info) {
    RcSlot* s; RcPlanView* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::pv, "rcflow_planview_info", s, vp)) return rc;
    if (!info) return RC_OK;
    memset(info, 0, sizeof(*info));
    info->w = vp->w; info->h = vp->h; info->prm = vp->prm;
    info->launches_per_push = RC_PLANVIEW_LAUNCHES;
    info->pushes = vp->pushes;
    info->device_bytes = vp->table.bytes + vp->ctl.bytes + vp->out.bytes;
    return RC_OK;
}

extern "C" int rcflow_planview_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::pv, "rcflow_planview_reset"); }
extern "C" int rcflow_planview_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::pv); }
