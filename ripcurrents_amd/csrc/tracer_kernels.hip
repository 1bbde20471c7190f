// tracer_kernels.hip -- streaklines, timelines and point clouds resident on the device (rcflow_tracers_*): the
// book-keeping of Streakline::runLK / Timeline::runLK / PopulationMap::runLK (Streakline.cpp:35-48,
// ripcurrents_module.cpp:794, :1175) and their drawing calls (Streakline.cpp:57-66, ripcurrents_module.cpp:800-805,
// :1186-1194) as a list of primitives for draw_kernels.hip.  The movers are the existing kernels: k_lk_track
// (rc_lk_track) and k_advect_points (rc_advect_points_launch).
//
// Layout.  The vertices of all lines lie compacted in one array, line after line in the order the lines were added,
// a streakline OLDEST first (growing is an append; rcflow_tracers_read hands it out newest first, the reference's order).
// A line's vertex count follows from its age alone, so the host and every workgroup compute the same offsets and
// nothing is ever read back: count = kind == streakline ? min(cap, 1 + age) : n0, age = moves since the line was added or
// the session was reset.  A push reads the array P[cur] (the vertices) and Q[cur] (where the mover put them) and writes
// P[1 - cur] in the next layout (every streakline one longer, or its oldest vertex gone once it is full), Q[1 - cur] too
// for the FLOW mover, whose kernel moves points in place.
#include <hip/hip_runtime.h>

#include <string.h>

#include "rc_device.h"
#include "rc_host.h"

struct TrLine {                 // 32 bytes, device
    int kind, cap, n0, pad;
    long long t_add;
    float gx, gy;               // streakline: the generation point
};
static_assert(sizeof(TrLine) == 32, "TrLine");

struct TrArgs {
    const TrLine* tab; int nlines;
    long long t, t_reset;       // moves before this push; at the last reset
    const float2* P; const float2* Q;
    float2* Pn; float2* Qn;     // Qn: null for the LK mover
    rc_draw_prim* prims;
    double jx, jy;              // the jump thresholds: w * 0.1, h * 0.1 (Streakline.cpp:36-37)
    int new_total;
};

#define TR_GREEN (100u << 8)    // CV_RGB(0, 100, 0)
#define TR_BLUE 100u            // CV_RGB(0, 0, 100)
#define TR_RED (100u << 16)     // CV_RGB(100, 0, 0)

__host__ __device__ static inline int tr_count(int kind, int cap, int n0, long long t_add, long long t, long long t_reset) {
    if (kind != RC_TRACER_STREAK) return n0;
    const long long age = t - (t_add > t_reset ? t_add : t_reset);
    return (int)(1 + age < (long long)cap ? 1 + age : (long long)cap);
}
__host__ __device__ static inline int tr_prims(int kind, int n) {
    return kind == RC_TRACER_STREAK ? 2 * n + 1 : (kind == RC_TRACER_TIMELINE ? 2 * n - 1 : n);
}

struct TrSpan { int kind, oc, nc, ooff, noff, poff; float gx, gy; };

// vertex k (oldest first for a streakline) of a line after this push
__device__ __forceinline__ float2 tr_newpos(const TrArgs& a, const TrSpan& L, int k) {
    if (L.kind != RC_TRACER_STREAK) return a.Q[L.ooff + k];
    if (k == L.nc - 1) return make_float2(L.gx, L.gy);             // vertices.insert(begin(), generationPoint)
    const int ko = k + (L.oc + 1 - L.nc);                          // a full ring lets its oldest vertex go
    const float2 o = a.P[L.ooff + ko], m = a.Q[L.ooff + ko];
    // "eliminate any large movement": a float difference against a double threshold; a NaN compares false and is kept
    const bool big = (double)fabsf(o.x - m.x) > a.jx || (double)fabsf(o.y - m.y) > a.jy;
    return big ? o : m;
}

__device__ __forceinline__ rc_draw_prim tr_disc(float2 c, int r, uint32_t color, uint32_t flags) {
    rc_draw_prim p;
    p.kind = RC_DRAW_DISC;
    p.x0 = p.x1 = rc_cvt_i32_x86(c.x); p.y0 = p.y1 = rc_cvt_i32_x86(c.y);   // Point(float, float): truncation
    p.size = r; p.color = color; p.flags = flags;
    return p;
}
__device__ __forceinline__ rc_draw_prim tr_line(float2 s, float2 e, int t, uint32_t color) {
    rc_draw_prim p;
    p.kind = RC_DRAW_LINE;
    p.x0 = rc_cvt_i32_x86(s.x); p.y0 = rc_cvt_i32_x86(s.y);
    p.x1 = rc_cvt_i32_x86(e.x); p.y1 = rc_cvt_i32_x86(e.y);
    p.size = t; p.color = color; p.flags = 0;
    return p;
}

// "tracers@0": one thread per vertex of the NEW layout
__global__ __launch_bounds__(RC_BLOCK) void k_tracers_book(TrArgs a) {
    __shared__ int s_oc[RC_TRACERS_MAX_LINES], s_nc[RC_TRACERS_MAX_LINES];
    __shared__ int s_ooff[RC_TRACERS_MAX_LINES], s_noff[RC_TRACERS_MAX_LINES + 1], s_poff[RC_TRACERS_MAX_LINES];
    const int tid = threadIdx.x;
    if (tid < a.nlines) {
        const TrLine L = a.tab[tid];
        s_oc[tid] = tr_count(L.kind, L.cap, L.n0, L.t_add, a.t, a.t_reset);
        s_nc[tid] = tr_count(L.kind, L.cap, L.n0, L.t_add, a.t + 1, a.t_reset);
    }
    __syncthreads();
    if (tid == 0) {                                           // at most 256 lines: a serial prefix is a microsecond
        int o = 0, n = 0, p = 0;
        for (int l = 0; l < a.nlines; l++) {
            s_ooff[l] = o; s_noff[l] = n; s_poff[l] = p;
            o += s_oc[l]; n += s_nc[l]; p += tr_prims(a.tab[l].kind, s_nc[l]);
        }
        s_noff[a.nlines] = n;
    }
    __syncthreads();
    const int j = blockIdx.x * RC_BLOCK + tid;
    if (j >= a.new_total) return;
    int lo = 0, hi = a.nlines - 1;                            // the last line whose offset is <= j (empty lines have none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_noff[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const TrLine T = a.tab[lo];
    TrSpan L;
    L.kind = T.kind; L.oc = s_oc[lo]; L.nc = s_nc[lo]; L.ooff = s_ooff[lo]; L.noff = s_noff[lo]; L.poff = s_poff[lo];
    L.gx = T.gx; L.gy = T.gy;
    const int k = j - L.noff;
    const float2 v = tr_newpos(a, L, k);
    a.Pn[j] = v;
    if (a.Qn) a.Qn[j] = v;
    rc_draw_prim* out = a.prims + L.poff;
    if (L.kind == RC_TRACER_STREAK) {
        const int i = L.nc - 1 - k;                           // the reference's index: newest first
        if (i == 0) {
            out[0] = tr_disc(v, 3, TR_GREEN, 0);              // v is the generation point, and vertices[0]
            out[1] = tr_line(v, v, 1, TR_RED);
            out[2] = tr_disc(v, 2, TR_BLUE, 0);
        } else {
            out[3 + 2 * (i - 1)] = tr_disc(v, 2, TR_BLUE, 0);
            out[4 + 2 * (i - 1)] = tr_line(tr_newpos(a, L, k + 1), v, 1, TR_RED);
        }
    } else if (L.kind == RC_TRACER_TIMELINE) {
        if (k == 0) {
            out[0] = tr_disc(v, 4, TR_BLUE, 0);
        } else {
            out[1 + 2 * (k - 1)] = tr_line(tr_newpos(a, L, k - 1), v, 2, TR_RED);
            out[2 + 2 * (k - 1)] = tr_disc(v, 4, TR_BLUE, 0);
        }
    } else {
        out[k] = tr_disc(v, 10, TR_RED, RC_DRAW_BLEND);
    }
}

// ============================================================================ host side
void rc_state_free(RcTracers& t) {
    rc_buf_free(t.pyr); rc_buf_free(t.pos); rc_buf_free(t.init); rc_buf_free(t.tab); rc_buf_free(t.prims); rc_buf_free(t.status);
    rc_buf_free(t.ctr);
    rc_fence_free(t.zf);
    t = RcTracers();
}

static float2* tr_P(const RcTracers& t, int i) { return (float2*)t.pos.p + (size_t)i * t.prm.max_points; }
static float2* tr_Q(const RcTracers& t, int i) { return (float2*)t.pos.p + (size_t)(2 + i) * t.prm.max_points; }
static int tr_line_count(const RcTracers& t, const RcTrLineH& L) { return tr_count(L.kind, L.cap, L.n0, L.t_add, t.t, t.t_reset); }
static int tr_total(const RcTracers& t) {
    int n = 0;
    for (const RcTrLineH& L : t.lines) n += tr_line_count(t, L);
    return n;
}

// open and reset: the lines as they were added (none after open), the counters, the skipped word
int rc_state_zero(RcSlot& s, RcTracers& t) {
    if (t.init_n) {
        // with every age 0 the compacted layout IS the layout of `init`
        RC_HIP(hipMemcpyAsync(tr_P(t, t.cur), t.init.p, (size_t)t.init_n * 8, hipMemcpyDeviceToDevice, s.cur));
        RC_HIP(hipMemcpyAsync(tr_Q(t, t.cur), t.init.p, (size_t)t.init_n * 8, hipMemcpyDeviceToDevice, s.cur));
    }
    const int rc = rc_fence_zero(t.zf, s.cur, {&t.ctr});
    if (rc) return rc;
    t.t_reset = t.t;
    t.dropped = 0;
    t.primed = false;
    t.nprims = 0;
    return RC_OK;
}

extern "C" int rcflow_tracers_open(rc_ctx* ctx, int stream, int w, int h, const rc_tracers_params* prm) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("rcflow_tracers_open: bad frame size %d x %d or no parameters", w, h); return RC_EINVAL; }
    rc_tracers_params p = *prm;
    if ((p.mover != RC_TRACERS_LK && p.mover != RC_TRACERS_FLOW) || p.max_lines < 1 || p.max_lines > RC_TRACERS_MAX_LINES ||
        p.max_vertices < 2 || p.max_points < 0) {
        rc_set_error("rcflow_tracers_open: mover 0 | 1, max_lines 1..%d, max_vertices >= 2, max_points >= 0", RC_TRACERS_MAX_LINES);
        return RC_EINVAL;
    }
    const long long mp = p.max_points ? p.max_points : (long long)p.max_lines * p.max_vertices;
    if (mp > RC_TRACERS_MAX_POINTS) { rc_set_error("rcflow_tracers_open: more than %d points", RC_TRACERS_MAX_POINTS); return RC_EINVAL; }
    p.max_points = (int)mp;
    if (p.mover == RC_TRACERS_LK) {
        if (p.win_w == 0) {                                   // Streakline.cpp:32
            p.win_w = p.win_h = 50; p.max_level = 3; p.crit_type = 3; p.max_count = 30; p.epsilon = 0.1; p.lk_flags = 10; p.min_eig = 1e-4;
        }
        if (p.win_w <= 2 || p.win_h <= 2 || p.max_level < 0 || p.max_level >= 8 || (size_t)p.win_w * p.win_h > 128 * 128 || (p.lk_flags & 4)) {
            rc_set_error("rcflow_tracers_open: PyrLK windows from 3 x 3 to 128 x 128, maxLevel < 8, no OPTFLOW_USE_INITIAL_FLOW");
            return RC_EINVAL;
        }
        // SparsePyrLKOpticalFlowImpl::calc, as rcflow_pyrlk_dev
        if ((p.crit_type & 1) == 0) p.max_count = 30;
        else p.max_count = p.max_count < 0 ? 0 : (p.max_count > 100 ? 100 : p.max_count);
        if ((p.crit_type & 2) == 0) p.epsilon = 0.01;
        else p.epsilon = p.epsilon < 0. ? 0. : (p.epsilon > 10. ? 10. : p.epsilon);
    } else if (!(p.dt == p.dt) || fabsf(p.dt) > 1e6f) {
        rc_set_error("rcflow_tracers_open: dt is not finite");
        return RC_EINVAL;
    }
    int rc = rc_fits_context("rcflow_tracers_open", ctx, w, h);
    if (rc) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcTracers n;
    n.w = w; n.h = h; n.prm = p;
    const size_t np = (size_t)p.max_points;
    if (p.mover == RC_TRACERS_LK) {
        n.plan = rc_lk_plan(w, h, p.win_w, p.win_h, p.max_level, true);
        rc = rc_buf_ensure(n.pyr, 2 * n.plan.bytes);
        if (!rc) rc = rc_buf_ensure(n.status, np);
    }
    if (!rc) rc = rc_buf_ensure(n.pos, 4 * np * 8);
    if (!rc) rc = rc_buf_ensure(n.init, np * 8);
    if (!rc) rc = rc_buf_ensure(n.tab, (size_t)p.max_lines * sizeof(TrLine));
    if (!rc) rc = rc_buf_ensure(n.prims, (2 * np + p.max_lines) * sizeof(rc_draw_prim));
    if (!rc) rc = rc_buf_ensure(n.ctr, 8);
    return rc_state_install(*s, s->tr, n, rc);
}

extern "C" int rcflow_tracers_add(rc_ctx* ctx, int stream, int kind, const float* xy, int n) {
    RcSlot* s; RcTracers* tp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tr, "rcflow_tracers_add", s, tp)) return rc;
    RcTracers& t = *tp;
    if (kind < RC_TRACER_STREAK || kind > RC_TRACER_CLOUD || !xy || n < 1 || (kind == RC_TRACER_STREAK && n != 1)) {
        rc_set_error("rcflow_tracers_add: kind 0..2, n >= 1 points (a streakline: its generation point alone)");
        return RC_EINVAL;
    }
    const int cap = kind == RC_TRACER_STREAK ? t.prm.max_vertices : n;
    if ((int)t.lines.size() >= t.prm.max_lines || (long long)t.reserved + cap > t.prm.max_points) {
        rc_set_error("rcflow_tracers_add: the session holds %d of %d lines and %d of %d points", (int)t.lines.size(), t.prm.max_lines,
                     t.reserved, t.prm.max_points);
        return RC_ESIZE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(t.zf, s->cur, true);
    if (rc) return rc;
    const int id = (int)t.lines.size(), at = tr_total(t);
    TrLine L;
    memset(&L, 0, sizeof(L));
    L.kind = kind; L.cap = cap; L.n0 = n; L.t_add = t.t;
    L.gx = xy[0]; L.gy = xy[1];
    const size_t bytes = (size_t)n * 8;
    RC_HIP(hipMemcpyAsync((TrLine*)t.tab.p + id, &L, sizeof(L), hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemcpyAsync(tr_P(t, t.cur) + at, xy, bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemcpyAsync(tr_Q(t, t.cur) + at, xy, bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemcpyAsync((float2*)t.init.p + t.init_n, xy, bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));                 // L and xy are the caller's for the length of the call only
    t.lines.push_back({kind, cap, n, t.t});
    t.reserved += cap;
    t.init_n += n;
    return id;
}

extern "C" int rcflow_tracers_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t gray_step, const float* d_flow_xy,
                                       size_t flow_step, uint8_t* d_canvas, size_t canvas_step) {
    static const char* who = "rcflow_tracers_push_dev";
    RcSlot* s; RcTracers* tp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tr, who, s, tp)) return rc;
    RcTracers& t = *tp;
    const bool lk = t.prm.mover == RC_TRACERS_LK;
    if (lk) {
        if (rc_image_check(who, "d_gray", d_gray, gray_step, t.w, t.h, 1, 1, RC_ARG_IN)) return RC_EINVAL;
    } else if (!d_flow_xy) {                              // the slot's resident field (rcflow_stream_flow_ptr)
        if (!s->flow_w) { rc_set_error("no flow field is resident on the slot yet"); return RC_ESTATE; }
        if (s->flow_w != t.w || s->flow_h != t.h) {
            rc_set_error("the resident flow field is %d x %d, the tracers %d x %d", s->flow_w, s->flow_h, t.w, t.h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)t.w * 8;
    } else if (rc_image_check(who, "d_flow_xy", d_flow_xy, flow_step, t.w, t.h, 8, 8, RC_ARG_IN | RC_ARG_ANY_BASE)) {
        return RC_EINVAL;
    }
    if (rc_image_check(who, "d_canvas", d_canvas, canvas_step, t.w, t.h, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL)) return RC_EINVAL;
    if (d_canvas && (t.w > RC_DRAW_COORD_MAX + 1 || t.h > RC_DRAW_COORD_MAX + 1)) {
        rc_set_error("rcflow_tracers_push_dev: drawing takes frames up to %d x %d", RC_DRAW_COORD_MAX + 1, RC_DRAW_COORD_MAX + 1);
        return RC_ESIZE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(t.zf, s->cur, true);
    if (rc) return rc;
    const int total = tr_total(t);
    // 1. move
    if (lk) {
        unsigned char* ref = (unsigned char*)t.pyr.p + (size_t)t.pyr_cur * t.plan.bytes;
        unsigned char* inc = (unsigned char*)t.pyr.p + (size_t)(t.primed ? 1 - t.pyr_cur : t.pyr_cur) * t.plan.bytes;
        // level 0 is kept tightly (pitch = w), the tracker's one addressing form: a device-to-device copy of the gray frame
        RC_HIP(hipMemcpy2DAsync(inc + t.plan.offI[0], t.w, d_gray, gray_step, t.w, t.h, hipMemcpyDeviceToDevice, s->cur));
        rc_lk_build(ctx, s->cur, t.plan, inc);
        if (!t.primed) {
            t.primed = true;
            RC_HIP(hipGetLastError());
            return 1;
        }
        if (total)
            rc_lk_track(ctx, s->cur, t.plan, ref, inc, t.plan, (const float*)tr_P(t, t.cur), (float*)tr_Q(t, t.cur), total, (uint8_t*)t.status.p,
                        nullptr, t.prm.win_w, t.prm.win_h, t.prm.max_count, t.prm.epsilon, t.prm.lk_flags, t.prm.min_eig);
        t.pyr_cur = 1 - t.pyr_cur;
    } else if (total) {
        // Streakline.run: variant 4, one step, no cutoff
        rc_advect_points_launch(ctx, s->cur, (float*)tr_Q(t, t.cur), total, d_flow_xy, flow_step, t.w, t.h, t.prm.dt, 1, 0.f, nullptr, 4, nullptr);
    }
    // 2. book-keeping and primitives
    int new_total = 0, nprims = 0;
    for (const RcTrLineH& L : t.lines) {
        const int oc = tr_line_count(t, L), nc = tr_count(L.kind, L.cap, L.n0, L.t_add, t.t + 1, t.t_reset);
        if (L.kind == RC_TRACER_STREAK && oc == L.cap) t.dropped++;
        new_total += nc;
        nprims += tr_prims(L.kind, nc);
    }
    if (new_total) {
        TrArgs a;
        a.tab = (const TrLine*)t.tab.p; a.nlines = (int)t.lines.size();
        a.t = t.t; a.t_reset = t.t_reset;
        a.P = tr_P(t, t.cur); a.Q = tr_Q(t, t.cur);
        a.Pn = tr_P(t, 1 - t.cur); a.Qn = lk ? nullptr : tr_Q(t, 1 - t.cur);
        a.prims = (rc_draw_prim*)t.prims.p;
        a.jx = t.w * 0.1; a.jy = t.h * 0.1;
        a.new_total = new_total;
        RcProfScope ps(ctx, s->cur, RC_K_TRACERS, 0, 24. * new_total + 32. * nprims);
        hipLaunchKernelGGL(k_tracers_book, dim3((new_total + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, a);
    }
    t.cur = 1 - t.cur;
    t.t++;
    t.nprims = nprims;
    // 3. draw
    if (d_canvas && nprims)
        rc_draw_launch(ctx, s->cur, d_canvas, canvas_step, t.w, t.h, 3, (const rc_draw_prim*)t.prims.p, nprims, (unsigned long long*)t.ctr.p);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_tracers_read(rc_ctx* ctx, int stream, int line, float* xy, int cap, int* n, long long* skipped) {
    RcSlot* s; RcTracers* tp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tr, "rcflow_tracers_read", s, tp)) return rc;
    RcTracers& t = *tp;
    if (line < 0 || line >= (int)t.lines.size() || cap < 0 || (cap && !xy)) { rc_set_error("rcflow_tracers_read: no line %d, or a bad buffer", line); return RC_EINVAL; }
    int off = 0;
    for (int l = 0; l < line; l++) off += tr_line_count(t, t.lines[l]);
    const int cnt = tr_line_count(t, t.lines[line]);
    if (n) *n = cnt;
    if (xy && cnt > cap) { rc_set_error("rcflow_tracers_read: line %d holds %d vertices, the buffer %d", line, cnt, cap); return RC_ESIZE; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(t.zf, s->cur, true);
    if (rc) return rc;
    unsigned long long sk = 0;
    if (xy) RC_HIP(hipMemcpyAsync(xy, tr_P(t, t.cur) + off, (size_t)cnt * 8, hipMemcpyDeviceToHost, s->cur));
    if (skipped) RC_HIP(hipMemcpyAsync(&sk, t.ctr.p, 8, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    if (skipped) *skipped = (long long)sk;
    if (xy && t.lines[line].kind == RC_TRACER_STREAK)     // stored oldest first, handed out newest first
        for (int i = 0, j = cnt - 1; i < j; i++, j--) {
            const float x = xy[2 * i], y = xy[2 * i + 1];
            xy[2 * i] = xy[2 * j]; xy[2 * i + 1] = xy[2 * j + 1];
            xy[2 * j] = x; xy[2 * j + 1] = y;
        }
    return RC_OK;
}

extern "C" int rcflow_tracers_prims(rc_ctx* ctx, int stream, const rc_draw_prim** d_prims, int* n) {
    RcSlot* s; RcTracers* t;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tr, "rcflow_tracers_prims", s, t)) return rc;
    if (d_prims) *d_prims = (const rc_draw_prim*)t->prims.p;
    if (n) *n = t->nprims;
    return RC_OK;
}

extern "C" int rcflow_tracers_info(rc_ctx* ctx, int stream, rc_tracers_info* info) {
    RcSlot* s; RcTracers* tp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tr, "rcflow_tracers_info", s, tp)) return rc;
    const RcTracers& t = *tp;
    if (!info) return RC_OK;
    memset(info, 0, sizeof(*info));
    info->w = t.w; info->h = t.h; info->mover = t.prm.mover;
    info->max_lines = t.prm.max_lines; info->max_vertices = t.prm.max_vertices; info->max_points = t.prm.max_points;
    info->lines = (int)t.lines.size(); info->points = tr_total(t); info->prims = t.nprims;
    info->primed = t.primed ? 1 : 0;
    info->pushes = t.t - t.t_reset;
    info->dropped = t.dropped;
    info->device_bytes = t.pyr.bytes + t.pos.bytes + t.init.bytes + t.tab.bytes + t.prims.bytes + t.status.bytes + t.ctr.bytes;
    return RC_OK;
}

extern "C" int rcflow_tracers_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::tr, "rcflow_tracers_reset"); }
extern "C" int rcflow_tracers_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::tr); }
