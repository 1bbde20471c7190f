// ftle_kernels.hip -- flow map and finite-time Lyapunov exponent: where did the water that is here come from?
//
// Everything else the library makes from the flow looks at one field or at a window mean.  This product carries a particle
// from every pixel through the last `window` fields (Euler, one step per field, the sampler of rc_sample_flow) and turns the
// flow map's gradient into the largest eigenvalue of the Cauchy-Green tensor and its logarithm per frame, the FTLE.  In
// backward time its ridges are the lines foam and sediment collect along: the feeder and the neck of a rip.
// include/rcflow.h ("flow map and FTLE") is the specification; tests/_ftle_ref.py states it in numpy and the kernels are
// held to that bit for bit (the FTLE itself to one unit in the last place: its logarithm is the device's, in double).  A
// push is one launch when no output is asked for, else three, and nothing synchronises:
//   ftle@0  ring     the field into its ring slot, [window][h][pitch] float2 with 16-byte rows;
//   ftle@1  map      the hot one.  A block is a 64 x 4 tile, a wave a compact 16 x 4 patch of it, a lane one particle (two and
//                    four particles a lane were measured slower, DESIGN 7k: at 26 registers eight waves a SIMD hide the
//                    dependent gathers better than a lane's own second particle does).  Particles that start adjacent
//                    stay adjacent until the stretching is large, which keeps the 64 gathers of a step within a few cache
//                    lines of one ring slot.  The two texels of a sampler row are one 16-byte load (8-byte aligned): two
//                    loads per sample, the arithmetic and its order those of rc_sample_flow.  The ring slot of a step is
//                    uniform and computed in scalar registers;
//   ftle@2  tensor   central differences of the map at +-spacing, lam, ftle, mask, picture; the integer sums per wave by
//                    ballot and popcount over the rows it walks, met in LDS, one atomic per block and counter (the
//                    launch keeps to about FT_MAX_BLOCKS blocks: they all end on the same two lines); the last-arriving block
//                    writes the summary and leaves the counters zero (rc_hand_off_fenced of rc_reduce.h).

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define FT_WAVES 4
static_assert(RC_BLOCK == 64 * FT_WAVES, "a block is FT_WAVES waves");
#define FT_TW 64               // ftle@1: FT_WAVES patches of 16 columns side by side
#define FT_TH 4
#define FT_QNAN 0x7fc00000u    // the one NaN lam and ftle hold
#define FT_MAX_BLOCKS 1024     // ftle@2: every block ends in five atomics on two lines, which the whole launch queues behind

// RcFtle::ctl.  The ticket has a 128-byte line of its own: every block adds to it.
struct FtCtl {
    RcTicketLine t;
    unsigned valid, mask, stopped, maxbits; unsigned pad1[28];
};
static_assert(sizeof(FtCtl) == 256, "two lines");

typedef float ft_f4 __attribute__((ext_vector_type(4), aligned(8)));   // the two texels of a sampler row

// ============================================================================ ftle@0: the ring slot
__global__ __launch_bounds__(RC_BLOCK) void k_ft_store(const float* flow, size_t step, float2* slot, int w, int h, int pitch) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * FT_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    slot[(size_t)y * pitch + x] = rc_row2(flow, step, y)[x];
}

// ============================================================================ ftle@1: the flow map
struct FtMapArgs {
    const float2* ring;                  // [window][h][pitch]
    float2* map; int* steps;             // the state's, [h][w]
    float* o_map; size_t o_map_step;     // the caller's, or null
    int* o_steps; size_t o_steps_step;
    int w, h, pitch, window, n;
    int first, stride;                   // the slot of step j is (first + j * stride) mod window; stride is +1 or window - 1
    float sdt;
};

__global__ __launch_bounds__(RC_BLOCK) void k_ft_map(const FtMapArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xo = blockIdx.x * FT_TW + wv * 16 + (lane & 15), yo = blockIdx.y * FT_TH + (lane >> 4);
    const bool inside = xo < a.w && yo < a.h;
    const float fx = (float)xo, fy = (float)yo;
    float dX = 0.f, dY = 0.f;
    int st = 0;
    bool alive = inside;
    const size_t plane = (size_t)a.h * a.pitch;
    int slot = a.first;                                       // uniform: scalar registers
    for (int j = 0; j < a.n; j++) {
        if (!__any(alive)) break;                             // the whole wave has stopped
        const float2* f = a.ring + (size_t)slot * plane;
        slot += a.stride;
        if (slot >= a.window) slot -= a.window;
        const float x = dX + fx, y = dY + fy;
        const int xind = rc_cvt_i32_x86(floorf(x)), yind = rc_cvt_i32_x86(floorf(y));
        const float xrem = x - xind, yrem = y - yind;
        const bool ok = alive && !(xind < 1 || yind < 1 || xind + 2 > a.w || yind + 2 > a.h);
        ft_f4 r0 = (ft_f4)(0.f), r1 = (ft_f4)(0.f);
        if (ok) {                                             // 1 <= xind, xind + 1 <= w - 1 < pitch; 1 <= yind, yind + 1 <= h - 1
            const float2* q = f + (size_t)yind * a.pitch + xind;
            r0 = *(const ft_f4*)q;
            r1 = *(const ft_f4*)(q + a.pitch);
        }
        // p00 = r0.xy, p01 = r0.zw, p10 = r1.xy, p11 = r1.zw: the products and additions in rc_sample_flow's order
        const float wa = 1 - xrem, wb = 1 - yrem;
        const float dx = r0[0] * wa * wb + r0[2] * xrem * wb + r1[0] * wa * yrem + r1[2] * xrem * yrem;
        const float dy = r0[1] * wa * wb + r0[3] * xrem * wb + r1[1] * wa * yrem + r1[3] * xrem * yrem;
        alive = ok && fabsf(dx) <= 3.4028234663852886e38f && fabsf(dy) <= 3.4028234663852886e38f;   // NaN fails; stopped for good
        if (alive) {
            dX = dX + dx * a.sdt;
            dY = dY + dy * a.sdt;
            st++;
        }
    }
    if (!inside) return;
    const size_t o = (size_t)yo * a.w + xo;
    a.map[o] = make_float2(dX, dY);
    a.steps[o] = st;
    if (a.o_map) ((float2*)((char*)a.o_map + (size_t)yo * a.o_map_step))[xo] = make_float2(dX, dY);
    if (a.o_steps) ((int*)((char*)a.o_steps + (size_t)yo * a.o_steps_step))[xo] = st;
}

// ============================================================================ ftle@2: tensor, outputs, summary
struct FtTenArgs {
    const float2* map; const int* steps; // [h][w]
    float* lam;                          // the state's, [h][w]
    float* o_lam; size_t o_lam_step;     // the caller's, or null
    float* o_ftle; size_t o_ftle_step;
    uint8_t* o_mask; size_t o_mask_step;
    uint8_t* vis; size_t vis_step;
    const uint8_t* jet;                  // 768 bytes
    FtCtl* ctl;
    long long* rec; long long* rec2;     // the state's summary; the caller's, or null
    int w, h, s, n;
    int rows;                            // a wave walks `rows` rows, FT_WAVES apart: the launch keeps to about FT_MAX_BLOCKS blocks
    float inv, lam_thr, vis_max;
    double two_n;
    long long pushes;
    unsigned nblocks;
};

__global__ __launch_bounds__(RC_BLOCK) void k_ft_tensor(const FtTenArgs a) {
    __shared__ uint8_t lut[768];
    __shared__ unsigned sums[4];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    if (a.vis)
        rc_stage_jet(lut, a.jet);
    if (threadIdx.x < 4) sums[threadIdx.x] = 0;
    __syncthreads();
    const int s = a.s;
    unsigned nv = 0, nm = 0, ns = 0, mb = 0;                  // the wave's sums over its rows (mb: per lane until the end)
    for (int r = 0; r < a.rows; r++) {
        const int y = (blockIdx.y * a.rows + r) * FT_WAVES + wv;
        if (y >= a.h) break;                                  // the whole wave leaves
        const bool in = x < a.w;
        bool valid = false, stopped = false;
        float lam = 0.f, ft = 0.f;
        if (in) {
            const size_t o = (size_t)y * a.w + x;
            stopped = a.steps[o] < a.n;
            if (!stopped && x >= s && x < a.w - s && y >= s && y < a.h - s) {
                const size_t oe = o + s, ow = o - s, os = o + (size_t)s * a.w, on = o - (size_t)s * a.w;
                if (a.steps[oe] == a.n && a.steps[ow] == a.n && a.steps[os] == a.n && a.steps[on] == a.n) {
                    valid = true;
                    const float2 E = a.map[oe], W = a.map[ow], S = a.map[os], N = a.map[on];
                    const float ta = 1 + (E.x - W.x) * a.inv, tb = (S.x - N.x) * a.inv;
                    const float tc = (E.y - W.y) * a.inv, td = 1 + (S.y - N.y) * a.inv;
                    const float c11 = ta * ta + tc * tc, c12 = ta * tb + tc * td, c22 = tb * tb + td * td;
                    const float m = (c11 + c22) * 0.5f, q = (c11 - c22) * 0.5f;
                    lam = m + sqrtf(q * q + c12 * c12);
                    if (lam != lam) lam = ft = __uint_as_float(FT_QNAN);
                    else ft = (float)(log((double)lam) / a.two_n);
                }
            }
        }
        const bool mk = valid && lam >= a.lam_thr;
        if (in) {
            a.lam[(size_t)y * a.w + x] = lam;
            if (a.o_lam) ((float*)((char*)a.o_lam + (size_t)y * a.o_lam_step))[x] = lam;
            if (a.o_ftle) ((float*)((char*)a.o_ftle + (size_t)y * a.o_ftle_step))[x] = ft;
            if (a.o_mask) a.o_mask[(size_t)y * a.o_mask_step + x] = mk ? 255 : 0;
            if (a.vis) {
                uint8_t* q = a.vis + (size_t)y * a.vis_step + 3 * (size_t)x;
                if (valid) {
                    const float v = rintf(ft / a.vis_max * 255.f);
                    const int i = !(v > 0.f) ? 0 : (v > 255.f ? 255 : (int)v);    // NaN: 0
                    q[0] = lut[3 * i]; q[1] = lut[3 * i + 1]; q[2] = lut[3 * i + 2];
                } else {
                    q[0] = 0; q[1] = 0; q[2] = 0;
                }
            }
        }
        nv += (unsigned)__popcll(__ballot(valid)); nm += (unsigned)__popcll(__ballot(mk)); ns += (unsigned)__popcll(__ballot(stopped));
        if (valid && lam == lam) mb = max(mb, __float_as_uint(lam));              // lam >= 0: its bits order as integers
    }
    // the integer sums: per wave, then the block's in LDS, then one atomic per counter
    mb = rc_wave_max_all(mb);
    if (lane == 0) {
        if (nv) atomicAdd(&sums[0], nv);
        if (nm) atomicAdd(&sums[1], nm);
        if (ns) atomicAdd(&sums[2], ns);
        if (mb) atomicMax(&sums[3], mb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sums[0]) rc_acc_add(&a.ctl->valid, sums[0]);
        if (sums[1]) rc_acc_add(&a.ctl->mask, sums[1]);
        if (sums[2]) rc_acc_add(&a.ctl->stopped, sums[2]);
        if (sums[3]) __hip_atomic_fetch_max(&a.ctl->maxbits, sums[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the ticket: every thread's stores and the block's atomics, __threadfence, the barrier, one ticket
    if (!rc_hand_off_fenced(&a.ctl->t.ticket, a.nblocks, &last) || threadIdx.x != 0) return;
    long long r[8];
    r[0] = a.n;
    r[1] = (long long)rc_acc_take(&a.ctl->valid);
    r[2] = (long long)rc_acc_take(&a.ctl->mask);
    r[3] = (long long)rc_acc_take(&a.ctl->stopped);
    r[4] = (long long)rc_acc_take(&a.ctl->maxbits);
    r[5] = a.pushes; r[6] = 0; r[7] = 0;
    for (int k = 0; k < 8; k++) {
        a.rec[k] = r[k];
        if (a.rec2) a.rec2[k] = r[k];
    }
    __hip_atomic_store(&a.ctl->t.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next push (stream order)
}

// ============================================================================ host side
void rc_state_free(RcFtle& f) {
    rc_buf_free(f.ring); rc_buf_free(f.map); rc_buf_free(f.steps); rc_buf_free(f.lam); rc_buf_free(f.ctl); rc_buf_free(f.out); rc_buf_free(f.jet);
    rc_fence_free(f.zf);
    f = RcFtle();
}

// open and reset: the counters and the summary; the ring position and the push count.  The ring, the map, steps and lam are
// written before they are read (n = min(pushes, window) bounds what ftle@1 visits), so up to 4 GiB are not cleared
int rc_state_zero(RcSlot& s, RcFtle& f) {
    const int rc = rc_fence_zero(f.zf, s.cur, {&f.ctl, &f.out});
    if (rc) return rc;
    f.cur = 0;
    f.pushes = 0;
    return RC_OK;
}

static bool ft_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }      // NaN fails

extern "C" int rcflow_ftle_open(rc_ctx* ctx, int stream, int w, int h, const rc_ftle_params* prm) {
    static const char* who = "rcflow_ftle_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad field size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (prm->window < 1 || prm->window > RC_FTLE_MAX_WINDOW || (prm->direction != RC_FTLE_FORWARD && prm->direction != RC_FTLE_BACKWARD) ||
        !(prm->dt > 0.f && prm->dt <= 3.4028234663852886e38f) || prm->spacing < 1 || prm->spacing > RC_FTLE_MAX_SPACING ||
        !ft_finite(prm->threshold) || !(prm->vis_max > 0. && ft_finite(prm->vis_max)) || prm->flags) {
        rc_set_error("%s: window 1..%d, direction 0 or 1, dt finite and > 0, spacing 1..%d, threshold finite, vis_max finite and > 0, flags 0",
                     who, RC_FTLE_MAX_WINDOW, RC_FTLE_MAX_SPACING);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcFtle n;
    n.w = w; n.h = h; n.prm = *prm;
    n.pitch = (w + 1) & ~1;
    const unsigned long long ring = (unsigned long long)prm->window * h * n.pitch * 8ull;
    if (ring > RC_FTLE_MAX_RING_BYTES) {
        rc_set_error("%s: a ring of %d fields of %d x %d is %llu bytes, more than RC_FTLE_MAX_RING_BYTES", who, prm->window, w, h, ring);
        return RC_ESIZE;
    }
    RC_HIP(hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h;
    rc = rc_buf_ensure(n.ring, (size_t)ring);
    if (!rc) rc = rc_buf_ensure(n.map, px * 8);
    if (!rc) rc = rc_buf_ensure(n.steps, px * 4);
    if (!rc) rc = rc_buf_ensure(n.lam, px * 4);
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(FtCtl));
    if (!rc) rc = rc_buf_ensure(n.out, 64);
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    return rc_state_install(*s, s->ft, n, rc);
}

extern "C" int rcflow_ftle_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, float* d_map_xy, size_t map_step,
                                    int32_t* d_steps, size_t steps_step, float* d_lam, size_t lam_step, float* d_ftle, size_t ftle_step,
                                    uint8_t* d_mask, size_t mask_step, uint8_t* d_vis, size_t vis_step, long long* d_summary) {
    static const char* who = "rcflow_ftle_push_dev";
    RcSlot* s; RcFtle* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ft, who, s, fp)) return rc;
    RcFtle& f = *fp;
    const int w = f.w, h = f.h;
    RcArgsN<8> a(who, w, h);
    a.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    a.image("d_map_xy", d_map_xy, map_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_steps", d_steps, steps_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_lam", d_lam, lam_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_ftle", d_ftle, ftle_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_vis", d_vis, vis_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(f.zf, s->cur, true);
    if (rc) return rc;
    const double px = (double)w * h;
    const int window = f.prm.window, slot = f.cur;
    const size_t plane = (size_t)h * f.pitch;
    {
        RcProfScope ps(ctx, s->cur, RC_K_FTLE, 0, px * 16.);
        hipLaunchKernelGGL(k_ft_store, dim3((w + 63) / 64, (h + FT_WAVES - 1) / FT_WAVES), dim3(RC_BLOCK), 0, s->cur, d_flow_xy, flow_step,
                           (float2*)f.ring.p + (size_t)slot * plane, w, h, f.pitch);
    }
    const long long pushes = f.pushes + 1;
    const int n = (int)(pushes < window ? pushes : window);
    if (d_map_xy || d_steps || d_lam || d_ftle || d_mask || d_vis || d_summary) {
        {
            FtMapArgs m;
            m.ring = (const float2*)f.ring.p; m.map = (float2*)f.map.p; m.steps = (int*)f.steps.p;
            m.o_map = d_map_xy; m.o_map_step = map_step; m.o_steps = d_steps; m.o_steps_step = steps_step;
            m.w = w; m.h = h; m.pitch = f.pitch; m.window = window; m.n = n;
            const int oldest = pushes <= window ? 0 : (slot + 1) % window;         // slot holds the newest
            m.first = f.prm.direction == RC_FTLE_FORWARD ? oldest : slot;
            m.stride = f.prm.direction == RC_FTLE_FORWARD ? 1 : window - 1;
            m.sdt = f.prm.direction == RC_FTLE_FORWARD ? f.prm.dt : -f.prm.dt;
            // per particle and step two rows of 16 bytes in; map 8 + steps 4 out
            RcProfScope ps(ctx, s->cur, RC_K_FTLE, 1, px * (32. * n + 12. + (d_map_xy ? 8. : 0.) + (d_steps ? 4. : 0.)));
            hipLaunchKernelGGL(k_ft_map, dim3((w + FT_TW - 1) / FT_TW, (h + FT_TH - 1) / FT_TH), dim3(RC_BLOCK), 0, s->cur, m);
        }
        {
            FtTenArgs t;
            t.map = (const float2*)f.map.p; t.steps = (const int*)f.steps.p; t.lam = (float*)f.lam.p;
            t.o_lam = d_lam; t.o_lam_step = lam_step; t.o_ftle = d_ftle; t.o_ftle_step = ftle_step;
            t.o_mask = d_mask; t.o_mask_step = mask_step; t.vis = d_vis; t.vis_step = vis_step;
            t.jet = (const uint8_t*)f.jet.p; t.ctl = (FtCtl*)f.ctl.p; t.rec = (long long*)f.out.p; t.rec2 = d_summary;
            t.w = w; t.h = h; t.s = f.prm.spacing; t.n = n;
            t.inv = 1.0f / (float)(2 * f.prm.spacing);
            t.lam_thr = (float)exp(2.0 * n * f.prm.threshold);
            t.vis_max = (float)f.prm.vis_max;
            t.two_n = (double)(2 * n);
            t.pushes = pushes;
            const int gx = (w + 63) / 64, gy1 = (h + FT_WAVES - 1) / FT_WAVES;
            t.rows = (int)(((long long)gx * gy1 + FT_MAX_BLOCKS - 1) / FT_MAX_BLOCKS);
            const dim3 grid(gx, (gy1 + t.rows - 1) / t.rows);
            t.nblocks = grid.x * grid.y;
            // map 8 + steps 4 in, lam 4 out
            RcProfScope ps(ctx, s->cur, RC_K_FTLE, 2, px * (16. + (d_lam ? 4. : 0.) + (d_ftle ? 4. : 0.) + (d_mask ? 1. : 0.) + (d_vis ? 3. : 0.)));
            hipLaunchKernelGGL(k_ft_tensor, grid, dim3(RC_BLOCK), 0, s->cur, t);
        }
    }
    RC_HIP(hipGetLastError());
    f.pushes = pushes;                                        // a launch that failed is not a push
    f.cur = (slot + 1) % window;
    return RC_OK;
}

extern "C" int rcflow_ftle_read(rc_ctx* ctx, int stream, long long summary[8]) {
    RcSlot* s; RcFtle* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ft, "rcflow_ftle_read", s, fp)) return rc;
    if (!summary) { rc_set_error("rcflow_ftle_read: no buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(fp->zf, s->cur, true);
    if (rc) return rc;
    RC_HIP(hipMemcpyAsync(summary, fp->out.p, 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_ftle_set(rc_ctx* ctx, int stream, double threshold, double vis_max) {
    RcSlot* s; RcFtle* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ft, "rcflow_ftle_set", s, fp)) return rc;
    if (!ft_finite(threshold) || !(vis_max > 0. && ft_finite(vis_max))) {
        rc_set_error("rcflow_ftle_set: threshold finite, vis_max finite and > 0");
        return RC_EINVAL;
    }
    fp->prm.threshold = threshold;
    fp->prm.vis_max = vis_max;
    return RC_OK;
}

extern "C" int rcflow_ftle_info(rc_ctx* ctx, int stream, rc_ftle_info* info) {
    RcSlot* s; RcFtle* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ft, "rcflow_ftle_info", s, fp)) return rc;
    const RcFtle& f = *fp;
    if (!info) return RC_OK;
    memset(info, 0, sizeof(*info));
    info->w = f.w; info->h = f.h; info->prm = f.prm;
    info->launches_per_push = RC_FTLE_LAUNCHES;
    info->held = (int)(f.pushes < f.prm.window ? f.pushes : f.prm.window);
    info->pushes = f.pushes;
    info->device_bytes = f.ring.bytes + f.map.bytes + f.steps.bytes + f.lam.bytes + f.ctl.bytes + f.out.bytes + f.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_ftle_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::ft, "rcflow_ftle_reset"); }
extern "C" int rcflow_ftle_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::ft); }
