// draw_kernels.hip -- discs and lines into 8UC1 / 8UC3 images on the device (rcflow_draw_dev), and the trace of
// rcflow_advect_points_dev as thin lines (rcflow_trace_prims_dev).  The painting rules are stated in include/rcflow.h
// and again, in numpy, in tests/_tracers_ref.py.
//
// Gather, not scatter.  A workgroup owns a tile of 64 x 16 pixels, a lane 4 consecutive pixels of a row (rc_pix3.h), so
// a pixel is painted by exactly one lane, the list order is kept without atomics and nothing races.  The workgroup walks
// the list in chunks of RC_BLOCK: every thread tests one primitive's box against the tile, a ballot and a prefix count
// compact the hits IN LIST ORDER into LDS, and after the barrier every lane runs its pixels over the compacted hits.  A
// tile no primitive meets loads and stores nothing; the others load their pixels once, at the first hit.
#include <hip/hip_runtime.h>

#include "rc_host.h"
#include "rc_pix3.h"

#define DR_TILE_W 64
#define DR_TILE_H 16
#define DR_MAX_TRACE_ITERS 65536   // rcflow_advect_points_dev's bound
static_assert(DR_TILE_W / 4 * DR_TILE_H == RC_BLOCK, "a lane owns 4 pixels of the tile");

struct DrArgs {
    uint8_t* img; size_t step;
    int w, h;
    const rc_draw_prim* prims; int n;
    unsigned long long* skipped;
};

// a record that breaks a bound of rcflow.h is skipped (and counted by workgroup 0)
__device__ __forceinline__ bool dr_valid(const rc_draw_prim& p) {
    const int M = RC_DRAW_COORD_MAX;
    if (p.x0 < -M || p.x0 > M || p.y0 < -M || p.y0 > M) return false;
    if (p.kind == RC_DRAW_DISC) return p.size >= 0 && p.size <= M;
    if (p.kind != RC_DRAW_LINE) return false;
    return p.x1 >= -M && p.x1 <= M && p.y1 >= -M && p.y1 <= M && p.size >= 1 && p.size <= RC_DRAW_MAX_THICKNESS;
}

// the box of a valid primitive, grown by its radius / half its thickness
__device__ __forceinline__ void dr_box(const rc_draw_prim& p, int& xa, int& ya, int& xb, int& yb) {
    if (p.kind == RC_DRAW_DISC) {
        xa = p.x0 - p.size; xb = p.x0 + p.size; ya = p.y0 - p.size; yb = p.y0 + p.size;
    } else {
        const int g = p.size >> 1;                       // thickness 1: none; t: a distance of t / 2
        xa = min(p.x0, p.x1) - g; xb = max(p.x0, p.x1) + g;
        ya = min(p.y0, p.y1) - g; yb = max(p.y0, p.y1) + g;
    }
}

// is pixel (x, y) lit by the valid primitive p?  Every product stays inside 64 bits for |coordinate| <= RC_DRAW_COORD_MAX
// and 0 <= x, y <= RC_DRAW_COORD_MAX: differences are below 2^15, their products below 2^30.
__device__ __forceinline__ bool dr_lit(const rc_draw_prim& p, int x, int y) {
    const int px = x - p.x0, py = y - p.y0;
    if (p.kind == RC_DRAW_DISC) return px * px + py * py <= p.size * p.size + p.size;
    const int bx = p.x1 - p.x0, by = p.y1 - p.y0;
    if (p.size == 1) {
        const int adx = abs(bx), ady = abs(by);
        // major axis u, minor axis v; t = steps along the major axis from the first end, m = steps along the minor
        const bool steep = ady > adx;
        const int au = steep ? ady : adx, av = steep ? adx : ady;
        const int pu = steep ? py : px, pv = steep ? px : py, bu = steep ? by : bx, bv = steep ? bx : by;
        if (au == 0) return px == 0 && py == 0;
        const int t = bu < 0 ? -pu : pu, m = bv < 0 ? -pv : pv;
        if (t < 0 || t > au || m < 0) return false;
        // m == (2 av t + au) / (2 au)  <=>  2 au m <= 2 av t + au < 2 au (m + 1); all below 2^31
        const unsigned q = 2u * (unsigned)av * (unsigned)t + (unsigned)au, lo = 2u * (unsigned)au * (unsigned)m;
        return lo <= q && q < lo + 2u * (unsigned)au;
    }
    const long long tt = (long long)p.size * p.size;
    const long long dot = (long long)px * bx + (long long)py * by, bb = (long long)bx * bx + (long long)by * by;
    if (dot <= 0) return 4 * ((long long)px * px + (long long)py * py) <= tt;
    if (dot >= bb) {
        const long long qx = px - bx, qy = py - by;
        return 4 * (qx * qx + qy * qy) <= tt;
    }
    const long long cr = (long long)px * by - (long long)py * bx;      // |cr| < 2^31
    const unsigned long long c = (unsigned long long)(cr < 0 ? -cr : cr);
    return 4ull * c * c <= (unsigned long long)(tt * bb);               // 4 c^2 < 2^64
}

__device__ __forceinline__ uint32_t dr_blend(uint32_t c, uint32_t p, int channels) {
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k >= channels) break;
        const uint32_t s = ((c >> (8 * k)) & 255u) + ((p >> (8 * k)) & 255u), hs = s >> 1;
        o |= ((s & 1u) ? hs + (hs & 1u) : hs) << (8 * k);
    }
    return o;
}

template <int CH>
__global__ __launch_bounds__(RC_BLOCK) void k_draw(DrArgs a) {
    __shared__ rc_draw_prim hits[RC_BLOCK];
    __shared__ int wave_n[RC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx0 = blockIdx.x * DR_TILE_W, ty0 = blockIdx.y * DR_TILE_H;
    const int tx1 = min(tx0 + DR_TILE_W, a.w) - 1, ty1 = min(ty0 + DR_TILE_H, a.h) - 1;
    // this lane's pixels: x .. x + n - 1 of row y
    const int x = tx0 + 4 * (tid & 15), y = ty0 + (tid >> 4);
    const int n = y < a.h ? min(4, a.w - x) : 0;
    uint8_t* row = a.img + (size_t)y * a.step;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    bool loaded = false;
    unsigned dirty = 0;                                     // bit k: pixel k has been painted
    const bool counts = a.skipped && blockIdx.x == 0 && blockIdx.y == 0;
    unsigned nskip = 0;

    for (int base = 0; base < a.n; base += RC_BLOCK) {
        const int i = base + tid;
        rc_draw_prim p;
        bool hit = false;
        if (i < a.n) {
            p = a.prims[i];
            if (dr_valid(p)) {
                int xa, ya, xb, yb;
                dr_box(p, xa, ya, xb, yb);
                hit = xa <= tx1 && xb >= tx0 && ya <= ty1 && yb >= ty0;
            } else if (counts) {
                nskip++;
            }
        }
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wave_n[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < RC_BLOCK / 64; k++) {
            const int c = wave_n[k];
            if (k < wv) off += c;
            total += c;
        }
        if (hit) hits[off + __popcll(bal & ((1ull << lane) - 1ull))] = p;
        __syncthreads();
        if (total && n > 0) {
            if (!loaded) {
                if (CH == 3) rc_pix3_load4(row, x, n, px);
                else if (n == 4) {
                    uint32_t q;
                    __builtin_memcpy(&q, row + x, 4);
                    px[0] = q & 255u; px[1] = (q >> 8) & 255u; px[2] = (q >> 16) & 255u; px[3] = q >> 24;
                } else {
                    for (int k = 0; k < n; k++) px[k] = row[x + k];
                }
                loaded = true;
            }
            for (int j = 0; j < total; j++) {
                const rc_draw_prim q = hits[j];              // the same address for every lane: a broadcast
                int xa, ya, xb, yb;
                dr_box(q, xa, ya, xb, yb);
                if (y < ya || y > yb || x + n - 1 < xa || x > xb) continue;
                const uint32_t col = CH == 3 ? (q.color & 0xffffffu) : (q.color & 255u);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k < n && dr_lit(q, x + k, y)) {
                        px[k] = (q.flags & RC_DRAW_BLEND) ? dr_blend(col, px[k], CH) : col;
                        dirty |= 1u << k;
                    }
                }
            }
        }
        // no third barrier: the next chunk writes wave_n after this chunk's second barrier (every read of it lies before
        // that one) and writes hits after its own first barrier (every read of hits above lies before that one)
    }
    if (dirty) {
        if (CH == 3) {
            rc_pix3_store4(row, x, n, px);
        } else if (n == 4) {
            const uint32_t q = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
            __builtin_memcpy(row + x, &q, 4);
        } else {
            for (int k = 0; k < n; k++) row[x + k] = (uint8_t)px[k];
        }
    }
    if (counts) {
        // one workgroup counts what every workgroup skips alike
        __shared__ unsigned skip_n[RC_BLOCK / 64];
        for (int d = 32; d > 0; d >>= 1) nskip += __shfl_down(nskip, d, 64);
        if (lane == 0) skip_n[wv] = nskip;
        __syncthreads();
        if (tid == 0) {
            unsigned t = 0;
            for (int k = 0; k < RC_BLOCK / 64; k++) t += skip_n[k];
            if (t) __hip_atomic_fetch_add(a.skipped, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// "tracers@2": one thread per line of the trace.  cvRound of a float on x86: round half to even, INT32_MIN beyond int32
__device__ __forceinline__ int dr_round_i32(float v) { return rc_cvt_i32_x86(rintf(v)); }

__global__ __launch_bounds__(RC_BLOCK) void k_trace_prims(const float2* start, const float2* trace, int n, int iters, uint32_t color,
                                                          rc_draw_prim* prims) {
    const int per = start ? iters : iters - 1;
    const long long i = (long long)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= (long long)n * per) return;
    const int s = (int)(i / per), k = (int)(i - (long long)s * per);     // line k of seed s
    const float2* t = trace + (size_t)s * iters;
    const float2 p = start ? (k == 0 ? start[s] : t[k - 1]) : t[k];
    const float2 q = start ? t[k] : t[k + 1];
    rc_draw_prim o;
    o.kind = RC_DRAW_LINE;
    o.x0 = dr_round_i32(p.x); o.y0 = dr_round_i32(p.y);
    o.x1 = dr_round_i32(q.x); o.y1 = dr_round_i32(q.y);
    o.size = 1; o.color = color; o.flags = 0;
    prims[i] = o;
}

// ============================================================================ host side
// "tracers@1".  The arguments have been checked.
void rc_draw_launch(rc_ctx* ctx, hipStream_t cur, uint8_t* d_img, size_t step, int w, int h, int channels, const rc_draw_prim* d_prims,
                    int n, unsigned long long* d_skipped) {
    DrArgs a;
    a.img = d_img; a.step = step; a.w = w; a.h = h; a.prims = d_prims; a.n = n; a.skipped = d_skipped;
    const dim3 grid((w + DR_TILE_W - 1) / DR_TILE_W, (h + DR_TILE_H - 1) / DR_TILE_H);
    // every tile reads the list; the pixels move only where something is painted
    RcProfScope ps(ctx, cur, RC_K_TRACERS, 1, 32. * n);
    if (channels == 3) hipLaunchKernelGGL(k_draw<3>, grid, dim3(RC_BLOCK), 0, cur, a);
    else hipLaunchKernelGGL(k_draw<1>, grid, dim3(RC_BLOCK), 0, cur, a);
}

extern "C" int rcflow_draw_dev(rc_ctx* ctx, int stream, uint8_t* d_img, size_t step, int w, int h, int channels,
                               const rc_draw_prim* d_prims, int n, unsigned long long* d_skipped) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if ((channels != 1 && channels != 3) || n < 0) { rc_set_error("%s: channels %d (1 or 3) or n %d (>= 0)", __func__, channels, n); return RC_EINVAL; }
    int rc;
    if ((rc = rc_image_check(__func__, "d_img", d_img, step, w, h, channels, 1, RC_ARG_OUT))) return rc;
    if ((rc = rc_ptr_check(__func__, "d_prims", d_prims, 16, n ? RC_ARG_IN : RC_ARG_OPTIONAL))) return rc;
    if ((rc = rc_ptr_check(__func__, "d_skipped", d_skipped, 8, RC_ARG_OUT | RC_ARG_OPTIONAL))) return rc;
    if (w > RC_DRAW_COORD_MAX + 1 || h > RC_DRAW_COORD_MAX + 1 || n > RC_DRAW_MAX_PRIMS) {
        rc_set_error("rcflow_draw_dev: images up to %d x %d and %d primitives are supported", RC_DRAW_COORD_MAX + 1, RC_DRAW_COORD_MAX + 1,
                     RC_DRAW_MAX_PRIMS);
        return RC_ESIZE;
    }
    if (n == 0) return RC_OK;
    RC_HIP(hipSetDevice(ctx->device));
    rc_draw_launch(ctx, s->cur, d_img, step, w, h, channels, d_prims, n, d_skipped);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_trace_prims_dev(rc_ctx* ctx, int stream, const float* d_start, const float* d_trace, int n, int iters,
                                      uint32_t color, rc_draw_prim* d_prims) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    const int per = d_start ? iters : iters - 1;
    if (n < 0 || iters < 1 || iters > DR_MAX_TRACE_ITERS) { rc_set_error("%s: n %d (>= 0) or iters %d (1..%d)", __func__, n, iters, DR_MAX_TRACE_ITERS); return RC_EINVAL; }
    const int lines = n && per ? 0 : RC_ARG_OPTIONAL;   // a call that writes no line may pass null lists
    int rc;
    if ((rc = rc_ptr_check(__func__, "d_trace", d_trace, 1, RC_ARG_IN | lines))) return rc;
    if ((rc = rc_ptr_check(__func__, "d_prims", d_prims, 16, RC_ARG_OUT | lines))) return rc;
    if ((long long)n * per > RC_DRAW_MAX_PRIMS) {
        rc_set_error("rcflow_trace_prims_dev: more than %d lines", RC_DRAW_MAX_PRIMS);
        return RC_ESIZE;
    }
    if (n == 0 || per == 0) return RC_OK;
    RC_HIP(hipSetDevice(ctx->device));
    {
        const long long total = (long long)n * per;
        RcProfScope ps(ctx, s->cur, RC_K_TRACERS, 2, 40. * total);
        hipLaunchKernelGGL(k_trace_prims, dim3((unsigned)((total + RC_BLOCK - 1) / RC_BLOCK)), dim3(RC_BLOCK), 0, s->cur,
                           (const float2*)d_start, (const float2*)d_trace, n, iters, color, d_prims);
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}
