// waves_kernels.hip -- wave spectra: what are the waves doing, and how deep is the water under them?
//
// Every other product looks at the flow.  This one looks at a pixel's grey value over time: a sliding DFT of the last `window`
// frames at a few bins per pixel, and per grid cell the strongest bin, the wavenumber from that bin's phase gradient across the
// cell, the celerity, and the depth through omega^2 = g k tanh(k h).  include/rcflow.h ("wave spectra") is the specification;
// tests/_waves_ref.py states it in numpy.  Everything up to the cell sums is integer and held to that bit for bit, the
// closing is double with the device's atan2 and atanh (a stored float within one unit in the last place).  A push is one
// launch when no output is asked for, else two or three, and nothing synchronises:
//   waves@0  spectrum  the hot one: 2 B/px in, 16 K B/px in and out.  A lane owns 4 consecutive pixels: the frame and the
//                      ring slot as one 4-byte access each, and per bin the four accumulators (re, im interleaved, bin-planar,
//                      rows of w rounded up to 4 pixels) as two 16-byte loads and two 16-byte stores.  The twiddles of the
//                      push are K pairs of integers among the launch's arguments: j = (b c) mod W does not depend on the pixel;
//   waves@1  cells     grid z is the bin.  A lane owns a column and walks `rows` rows, four in flight; its cell column never
//                      changes, so it sums in registers (int64) while the cell row stays, then the wave reduces per cell column
//                      and one lane adds to the cell's words (the form of ripmap@0 without its LDS table).  Blocks arrive at
//                      sharded tickets without a fence; the launch's last block takes the words, closes every cell in double,
//                      writes records, sums and summary and leaves the words zero;
//   waves@2  paint     the bin map and the picture from the records, a lane a pixel.

#include <math.h>
#include <string.h>

#include <vector>

#include "rc_host.h"
#include "rc_reduce.h"

#define WV_WAVES 4
static_assert(RC_BLOCK == 64 * WV_WAVES, "a block is WV_WAVES waves");
#define WV_UNROLL 4            // waves@1: rows a wave has in flight
#define WV_MAX_BLOCKS 2048     // waves@1: every block ends in a ticket; a wave walks several rows from here on

// the head of RcWaves::cacc: the tickets, each on a 128-byte line of its own.  One word takes some 90 atomics a microsecond
// however many blocks queue for it (4096 blocks on one ticket: 45 us), so a block arrives at the shard of its number modulo
// WV_SHARDS and only a shard's last block goes on to the top (the two levels of planview@1)
#define WV_SHARDS 16
struct WvCtl { RcTicketLine shard[WV_SHARDS], top, unused; };
static_assert(sizeof(WvCtl) == 128 * (WV_SHARDS + 2), "the cell sums start after eighteen lines");

typedef uint32_t wv_u32u __attribute__((aligned(1)));     // four pixels of a caller's row: no alignment is asked of it

// ============================================================================ waves@0: the spectrum
struct WvSpecArgs {
    const uint8_t* gray; size_t step;
    uint8_t* slot;                       // the ring slot this push replaces, [h][pitch]
    int2* acc;                           // [K][h][pitch]
    int w, h, pitch, K;
    int tc[RC_WAVES_MAX_BINS], ts[RC_WAVES_MAX_BINS];   // Tc[j], Ts[j] of every bin for this push
};

__global__ __launch_bounds__(RC_BLOCK) void k_wv_spectrum(const WvSpecArgs a) {
    const int x0 = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), y = blockIdx.y * WV_WAVES + (threadIdx.x >> 6);
    if (x0 >= a.w || y >= a.h) return;
    const int np = min(4, a.w - x0);
    const uint8_t* g = a.gray + (size_t)y * a.step + x0;
    uint32_t nw = 0;
    if (np == 4) nw = *(const wv_u32u*)g;
    else
        for (int k = 0; k < np; k++) nw |= (uint32_t)g[k] << (8 * k);
    const size_t o = (size_t)y * a.pitch + x0;                // x0 + 3 < pitch
    uint32_t* rp = (uint32_t*)(a.slot + o);
    const uint32_t old = *rp;
    if (old == nw) return;                                    // d = 0 in all four: nothing moves
    *rp = nw;                                                 // the columns past w hold zeros and stay zero
    int d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = (int)((nw >> (8 * k)) & 255u) - (int)((old >> (8 * k)) & 255u);
    int4* ap = (int4*)(a.acc + o);
    const size_t plane4 = (size_t)a.h * a.pitch / 2;          // a plane in int4
#pragma unroll 4
    for (int k = 0; k < a.K; k++, ap += plane4) {
        int4 v0 = ap[0], v1 = ap[1];
        const int c = a.tc[k], s = a.ts[k];
        v0.x += d[0] * c; v0.y -= d[0] * s; v0.z += d[1] * c; v0.w -= d[1] * s;
        v1.x += d[2] * c; v1.y -= d[2] * s; v1.z += d[3] * c; v1.w -= d[3] * s;
        ap[0] = v0; ap[1] = v1;
    }
}

// ============================================================================ waves@1: cell sums and the closing
struct WvCellArgs {
    const int2* acc;                     // [K][h][pitch]
    const uint8_t* mask; size_t mask_step;   // or null
    WvCtl* ctl;
    long long* cacc;                     // [cells][K][6], zero between launches; n is added to bin 0's alone
    long long* sums; rc_wave_cell* cells; long long* summary;      // the state's copy
    long long* sums2; rc_wave_cell* cells2; long long* summary2;   // the caller's, or null
    int w, h, pitch, K, s, sh, rows, gx, gy, cw, ch;
    int bin_lo, window, min_pixels;
    double fps, mx, my, gravity, tanh_max;
    long long pushes, held;
    unsigned nblocks;
};

// true for the last of n arrivals, which leaves the ticket zero for the next push (stream order)
__device__ __forceinline__ bool wv_arrive(unsigned* ticket, unsigned n) {
    if (rc_acc_add_old(ticket, 1u) != n - 1u) return false;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// the wave's register sums of one cell row -> the cells' words.  Cell columns cxa..cxb are the wave's; cxl is the lane's
__device__ __forceinline__ void wv_flush(const WvCellArgs& a, int k, int cxa, int cxb, int cy, int cxl, long long v[6]) {
    for (int cx = cxa; cx <= cxb; cx++) {
        long long t[6];
#pragma unroll
        for (int q = 0; q < 6; q++) t[q] = rc_wave_sum_lane0(cxl == cx ? v[q] : 0ll);
        if ((threadIdx.x & 63) == 0 && t[0]) {
            long long* p = a.cacc + 6 * (((size_t)cy * a.gx + cx) * a.K + k);
            // the old values are asked for and thrown away: an atomic that returns has been performed once the wave's vmcnt
            // has counted it, which the hand-off at the end of the kernel waits for
            long long r[6];
            r[0] = k == 0 ? rc_acc_add_old(p, t[0]) : 0;
#pragma unroll
            for (int q = 1; q < 6; q++) r[q] = rc_acc_add_old(p + q, t[q]);
            asm volatile("" ::"v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]), "v"(r[4]), "v"(r[5]));
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) v[q] = 0;
}

// The closing, by every thread of the last-arriving block.  First a thread a word: the cells' words are taken (an exchange a
// word, eight in flight per thread: 81 of them one after the other for a cell of 16 bins took 70 us)
// into the state's sums; then a thread a cell.  Doubles round operation by operation (-ffp-contract=off) in the order of
// tests/_waves_ref.py
__device__ void wv_finish(const WvCellArgs& a, unsigned long long* red /* [3] */) {
    const int ncell = a.gx * a.gy, K = a.K;
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    const int nword = ncell * K * 6;
    for (int i0 = threadIdx.x; i0 < nword; i0 += 16 * RC_BLOCK) { // n of a bin above the first: nothing was added, 0 is taken
        long long t[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int i = i0 + u * RC_BLOCK;
            t[u] = i < nword ? rc_acc_take(a.cacc + i) : 0;
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int i = i0 + u * RC_BLOCK;
            if (i < nword) a.sums[i] = t[u];
        }
    }
    __threadfence_block();                                    // the sums are read below by other threads of this block
    __syncthreads();
    unsigned long long part = 0, nonempty = 0, depths = 0;
    for (int c = threadIdx.x; c < ncell; c += RC_BLOCK) {
        long long* dst = a.sums + 6 * (size_t)c * K;
        const long long n = dst[0];
        int kb = 0;
        long long pb = 0;
        bool any = false;
        for (int k = 0; k < K; k++) {
            dst[6 * k] = n;
            const long long P = dst[6 * k + 1];
            any = any || P != 0;
            if (P > pb) { pb = P; kb = k; }                   // the lowest bin wins ties
            if (a.sums2) {
                long long* d2 = a.sums2 + 6 * ((size_t)c * K + k);
                d2[0] = n;
                for (int q = 1; q < 6; q++) d2[q] = dst[6 * k + q];
            }
        }
        part += (unsigned long long)n;
        rc_wave_cell r;
        r.bin = 0; r.flags = RC_WAVES_EMPTY;
        r.freq_hz = r.kx = r.ky = r.celerity = r.depth = r.quality = 0.f;
        if (n >= a.min_pixels && any) {
            const long long cxr = dst[6 * kb + 2], cxi = dst[6 * kb + 3], cyr = dst[6 * kb + 4], cyi = dst[6 * kb + 5];
            const double b = (double)(a.bin_lo + kb), W = (double)a.window, two_s = (double)(2 * a.s);
            const double kx = atan2((double)(-cxi), (double)cxr) / two_s / a.mx;
            const double ky = atan2((double)(-cyi), (double)cyr) / two_s / a.my;
            const double kmag = sqrt(kx * kx + ky * ky);
            const double freq = b * a.fps / W;
            const double omega = 6.283185307179586 * b * a.fps / W;
            const double ax = (double)cxr, ay = (double)cxi, bx = (double)cyr, by = (double)cyi;
            const double quality = (sqrt(ax * ax + ay * ay) + sqrt(bx * bx + by * by)) / (2.0 * (double)pb);
            r.bin = a.bin_lo + kb;
            r.freq_hz = (float)freq; r.kx = (float)kx; r.ky = (float)ky; r.quality = (float)quality;
            nonempty++;
            if (kmag == 0.) {
                r.flags = RC_WAVES_NOWAVE;
            } else {
                r.celerity = (float)(omega / kmag);
                const double t = omega * omega / (a.gravity * kmag);
                if (t < a.tanh_max) {
                    r.flags = 0;
                    r.depth = (float)(atanh(t) / kmag);
                    depths++;
                } else {
                    r.flags = RC_WAVES_DEEP;
                }
            }
        }
        a.cells[c] = r;
        if (a.cells2) a.cells2[c] = r;
    }
    if (part) atomicAdd(&red[0], part);
    if (nonempty) atomicAdd(&red[1], nonempty);
    if (depths) atomicAdd(&red[2], depths);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long s[8] = {a.held, (long long)red[0], (long long)red[1], (long long)red[2], a.pushes, 0, 0, 0};
    for (int k = 0; k < 8; k++) {
        a.summary[k] = s[k];
        if (a.summary2) a.summary2[k] = s[k];
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_wv_cells(const WvCellArgs a) {
    __shared__ unsigned long long red[3];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, k = blockIdx.z, s = a.s;
    const int xb = blockIdx.x * 64, x = xb + lane;
    const int cxa = min(xb / a.cw, a.gx - 1), cxb = min((min(xb + 64, a.w) - 1) / a.cw, a.gx - 1);
    const int cxl = min(x / a.cw, a.gx - 1);
    const int2* A = a.acc + (size_t)k * a.h * a.pitch;
    const bool xin = x >= s && x < a.w - s;
    long long v[6] = {0, 0, 0, 0, 0, 0};
    int cur_cy = -1;
    const int y0 = (blockIdx.y * WV_WAVES + wv) * a.rows;
    // WV_UNROLL rows at a time: their masks, then their twenty loads, then the sums.  A row alone is one trip to memory after
    // the other (127 rows a wave at 1080p and 16 bins: 1 us each)
    for (int r = 0; r < a.rows; r += WV_UNROLL) {
        bool on[WV_UNROLL];
        int2 C[WV_UNROLL], E[WV_UNROLL], Wn[WV_UNROLL], S[WV_UNROLL], N[WV_UNROLL];
#pragma unroll
        for (int u = 0; u < WV_UNROLL; u++) {
            const int y = y0 + r + u;
            on[u] = r + u < a.rows && xin && y >= s && y < a.h - s;       // E, W, S, N exist where it holds
            if (on[u] && a.mask) {
                const uint8_t* m = a.mask + (size_t)y * a.mask_step + x;
                on[u] = m[0] && m[s] && m[-s] && m[(ptrdiff_t)s * (ptrdiff_t)a.mask_step] && m[-(ptrdiff_t)s * (ptrdiff_t)a.mask_step];
            }
        }
#pragma unroll
        for (int u = 0; u < WV_UNROLL; u++) {
            C[u] = E[u] = Wn[u] = S[u] = N[u] = make_int2(0, 0);
            if (on[u]) {
                const int2* p = A + (size_t)(y0 + r + u) * a.pitch + x;
                C[u] = p[0]; E[u] = p[s]; Wn[u] = p[-s]; S[u] = p[(ptrdiff_t)s * a.pitch]; N[u] = p[-(ptrdiff_t)s * a.pitch];
            }
        }
#pragma unroll
        for (int u = 0; u < WV_UNROLL; u++) {
            const int y = y0 + r + u;
            if (r + u >= a.rows || y >= a.h) break;           // the whole wave leaves
            const int cy = min(y / a.ch, a.gy - 1);
            if (cy != cur_cy) {
                if (cur_cy >= 0) wv_flush(a, k, cxa, cxb, cur_cy, cxl, v);
                cur_cy = cy;
            }
            if (!on[u]) continue;
            const int cx_ = C[u].x >> a.sh, cy_ = C[u].y >> a.sh, ex = E[u].x >> a.sh, ey = E[u].y >> a.sh, wx = Wn[u].x >> a.sh, wy = Wn[u].y >> a.sh;
            const int sx = S[u].x >> a.sh, sy = S[u].y >> a.sh, nx = N[u].x >> a.sh, ny = N[u].y >> a.sh;
            v[0] += 1;
            v[1] += (long long)cx_ * cx_ + (long long)cy_ * cy_;
            v[2] += (long long)ex * wx + (long long)ey * wy;
            v[3] += (long long)ey * wx - (long long)ex * wy;
            v[4] += (long long)sx * nx + (long long)sy * ny;
            v[5] += (long long)sy * nx - (long long)sx * ny;
        }
    }
    if (cur_cy >= 0) wv_flush(a, k, cxa, cxb, cur_cy, cxl, v);
    // The hand-off, without a fence: rc_reduce.h says why nothing but the wait is needed on gfx950 and what a port needs instead.
    // Every add above returned its old value, so a wave's vmcnt reaches 0 only when its adds have been performed; the barrier joins
    // the block's waves; then the block's ticket, and for a shard's last block the top's, each issued after the one before returned
    rc_wait_performed();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, g = bid % WV_SHARDS;
        bool l = wv_arrive(&a.ctl->shard[g].ticket, (a.nblocks - g + WV_SHARDS - 1) / WV_SHARDS);      // blocks g, g + WV_SHARDS, ...
        if (l) l = wv_arrive(&a.ctl->top.ticket, min(a.nblocks, (unsigned)WV_SHARDS));
        last = l;
    }
    __syncthreads();
    if (last) wv_finish(a, red);
}

// ============================================================================ waves@2: the bin map and the picture
__global__ __launch_bounds__(RC_BLOCK) void k_wv_paint(const rc_wave_cell* cells, const uint8_t* jet, int w, int h, int gx, int gy, int cw, int ch,
                                                       float vis_max, uint8_t* bin_map, size_t bin_map_step, uint8_t* vis, size_t vis_step) {
    __shared__ uint8_t lut[768];
    if (vis)
        for (int i = threadIdx.x; i < 768; i += RC_BLOCK) lut[i] = jet[i];
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * WV_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const rc_wave_cell r = cells[(size_t)min(y / ch, gy - 1) * gx + min(x / cw, gx - 1)];
    if (bin_map) bin_map[(size_t)y * bin_map_step + x] = (uint8_t)r.bin;
    if (vis) {
        uint8_t* q = vis + (size_t)y * vis_step + 3 * (size_t)x;
        if (r.flags == 0) {
            const float f = rintf(r.depth / vis_max * 255.f);
            const int i = !(f > 0.f) ? 0 : (f > 255.f ? 255 : (int)f);
            q[0] = lut[3 * i]; q[1] = lut[3 * i + 1]; q[2] = lut[3 * i + 2];
        } else {
            q[0] = 0; q[1] = 0; q[2] = 0;
        }
    }
}

// ============================================================================ host side
void rc_state_free(RcWaves& v) {
    rc_buf_free(v.ring); rc_buf_free(v.acc); rc_buf_free(v.cacc); rc_buf_free(v.out); rc_buf_free(v.jet);
    rc_fence_free(v.zf);
    v = RcWaves();
}

// open and reset: the ring, the accumulators, the cells' words, the last push's outputs; the push count
int rc_state_zero(RcSlot& s, RcWaves& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.ring, &v.acc, &v.cacc, &v.out});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static size_t wv_cells(const RcWaves& v) { return (size_t)v.prm.grid_x * v.prm.grid_y; }
// RcWaves::out: records [cells] | sums [cells][K][6] int64 | summary 8 int64
static rc_wave_cell* wv_out_cells(const RcWaves& v) { return (rc_wave_cell*)v.out.p; }
static long long* wv_out_sums(const RcWaves& v) { return (long long*)((char*)v.out.p + wv_cells(v) * 32); }
static long long* wv_out_summary(const RcWaves& v) { return wv_out_sums(v) + wv_cells(v) * v.K * 6; }

static bool wv_pos(double v) { return v > 0. && v <= 1.7976931348623157e308; }      // finite and > 0; NaN fails
static bool wv_set_ok(double tanh_max, int min_pixels, double vis_max_depth) {
    return tanh_max > 0. && tanh_max < 1. && min_pixels >= 1 && wv_pos(vis_max_depth);
}

extern "C" int rcflow_waves_open(rc_ctx* ctx, int stream, int w, int h, const rc_waves_params* prm) {
    static const char* who = "rcflow_waves_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad frame size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    const int W = prm->window;
    if (W < 2 || W > RC_WAVES_MAX_WINDOW || prm->bin_lo < 1 || prm->bin_hi < prm->bin_lo || 2 * (long long)prm->bin_hi >= W ||
        prm->bin_hi - prm->bin_lo + 1 > RC_WAVES_MAX_BINS || prm->spacing < 1 || prm->spacing > RC_WAVES_MAX_SPACING || prm->flags ||
        !wv_pos(prm->fps) || !wv_pos(prm->metres_per_pixel_x) || !wv_pos(prm->metres_per_pixel_y) || !wv_pos(prm->gravity) ||
        !wv_set_ok(prm->tanh_max, prm->min_pixels, prm->vis_max_depth)) {
        rc_set_error("%s: window 2..%d, 1 <= bin_lo <= bin_hi < window / 2 with at most %d bins, spacing 1..%d, fps, metres per pixel, gravity "
                     "and vis_max_depth finite and > 0, tanh_max in (0, 1), min_pixels >= 1, flags 0", who, RC_WAVES_MAX_WINDOW, RC_WAVES_MAX_BINS,
                     RC_WAVES_MAX_SPACING);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d frame (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcWaves n;
    n.w = w; n.h = h; n.prm = *prm;
    n.K = prm->bin_hi - prm->bin_lo + 1;
    n.pitch = (w + 3) & ~3;
    const unsigned long long plane = (unsigned long long)h * n.pitch, state = plane * W + plane * 8ull * n.K;
    if (state > RC_WAVES_MAX_STATE_BYTES) {
        rc_set_error("%s: a ring of %d frames and %d bins of %d x %d are %llu bytes, more than RC_WAVES_MAX_STATE_BYTES", who, W, n.K, w, h, state);
        return RC_ESIZE;
    }
    for (long long bound = 255ll * 2048 * W; bound >> (15 + n.sh); n.sh++) {}      // max(0, bit_length - 15)
    n.tc.resize(W); n.ts.resize(W);
    for (int j = 0; j < W; j++) {
        const double ang = (6.283185307179586 * (double)j) / (double)W;
        n.tc[j] = (int)lrint(2048. * cos(ang));
        n.ts[j] = (int)lrint(2048. * sin(ang));
    }
    RC_HIP(hipSetDevice(ctx->device));
    const size_t nc = wv_cells(n);
    rc = rc_buf_ensure(n.ring, (size_t)(plane * W));
    if (!rc) rc = rc_buf_ensure(n.acc, (size_t)(plane * 8ull * n.K));
    if (!rc) rc = rc_buf_ensure(n.cacc, sizeof(WvCtl) + nc * n.K * 48);
    if (!rc) rc = rc_buf_ensure(n.out, nc * 32 + nc * n.K * 48 + 64);
    if (!rc) rc = rc_buf_ensure(n.jet, 768);
    if (!rc) {
        uint8_t lut[768];
        rcflow_jet_lut(lut);
        if (hipMemcpy(n.jet.p, lut, 768, hipMemcpyHostToDevice) != hipSuccess) { rc_set_error("%s: the colour table's upload failed", who); rc = RC_EHIP; }
    }
    return rc_state_install(*s, s->wv, n, rc);
}

extern "C" int rcflow_waves_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, const uint8_t* d_mask, size_t mask_step,
                                     rc_wave_cell* d_cells, long long* d_sums, uint8_t* d_bin_map, size_t bin_map_step, uint8_t* d_vis,
                                     size_t vis_step, long long* d_summary) {
    static const char* who = "rcflow_waves_push_dev";
    RcSlot* s; RcWaves* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::wv, who, s, vp)) return rc;
    RcWaves& v = *vp;
    const int w = v.w, h = v.h, K = v.K, W = v.prm.window;
    const size_t nc = wv_cells(v);
    RcArgs a(who, w, h);
    a.image("d_gray", d_gray, step, 1, 1, RC_ARG_IN);
    a.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    a.array("d_cells", d_cells, nc * 32, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_sums", d_sums, nc * K * 48, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_bin_map", d_bin_map, bin_map_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_vis", d_vis, vis_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    if (d_bin_map && v.prm.bin_hi > 255) { rc_set_error("%s: d_bin_map holds a bin in a byte, and bin_hi is %d", who, v.prm.bin_hi); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const double px = (double)w * h;
    const size_t plane = (size_t)h * v.pitch;
    const int c = (int)(v.pushes % W);
    {
        WvSpecArgs p;
        p.gray = d_gray; p.step = step;
        p.slot = (uint8_t*)v.ring.p + plane * (size_t)c;
        p.acc = (int2*)v.acc.p;
        p.w = w; p.h = h; p.pitch = v.pitch; p.K = K;
        for (int k = 0; k < RC_WAVES_MAX_BINS; k++) {
            const int j = k < K ? (int)(((long long)(v.prm.bin_lo + k) * c) % W) : 0;
            p.tc[k] = v.tc[j]; p.ts[k] = v.ts[j];
        }
        RcProfScope ps(ctx, s->cur, RC_K_WAVES, 0, px * (3. + 16. * K));
        hipLaunchKernelGGL(k_wv_spectrum, dim3((v.pitch / 4 + 63) / 64, (h + WV_WAVES - 1) / WV_WAVES), dim3(RC_BLOCK), 0, s->cur, p);
    }
    const long long pushes = v.pushes + 1;
    if (d_cells || d_sums || d_bin_map || d_vis || d_summary) {
        const int cw = w / v.prm.grid_x, ch = h / v.prm.grid_y;
        {
            WvCellArgs q;
            q.acc = (const int2*)v.acc.p; q.mask = d_mask; q.mask_step = mask_step;
            q.ctl = (WvCtl*)v.cacc.p; q.cacc = (long long*)((char*)v.cacc.p + sizeof(WvCtl));
            q.sums = wv_out_sums(v); q.cells = wv_out_cells(v); q.summary = wv_out_summary(v);
            q.sums2 = d_sums; q.cells2 = d_cells; q.summary2 = d_summary;
            q.w = w; q.h = h; q.pitch = v.pitch; q.K = K; q.s = v.prm.spacing; q.sh = v.sh;
            const int bx = (w + 63) / 64, by1 = (h + WV_WAVES - 1) / WV_WAVES;
            q.rows = (int)(((long long)bx * by1 * K + WV_MAX_BLOCKS - 1) / WV_MAX_BLOCKS);
            q.gx = v.prm.grid_x; q.gy = v.prm.grid_y; q.cw = cw; q.ch = ch;
            q.bin_lo = v.prm.bin_lo; q.window = W; q.min_pixels = v.prm.min_pixels;
            q.fps = v.prm.fps; q.mx = v.prm.metres_per_pixel_x; q.my = v.prm.metres_per_pixel_y; q.gravity = v.prm.gravity;
            q.tanh_max = v.prm.tanh_max;
            q.pushes = pushes; q.held = pushes < W ? pushes : W;
            const dim3 grid(bx, (by1 + q.rows - 1) / q.rows, K);
            q.nblocks = grid.x * grid.y * grid.z;
            // the accumulators once (the four neighbours come from the caches), the mask
            RcProfScope ps(ctx, s->cur, RC_K_WAVES, 1, px * (8. * K + (d_mask ? 1. : 0.)));
            hipLaunchKernelGGL(k_wv_cells, grid, dim3(RC_BLOCK), 0, s->cur, q);
        }
        if (d_bin_map || d_vis) {
            RcProfScope ps(ctx, s->cur, RC_K_WAVES, 2, px * ((d_bin_map ? 1. : 0.) + (d_vis ? 3. : 0.)));
            hipLaunchKernelGGL(k_wv_paint, dim3((w + 63) / 64, (h + WV_WAVES - 1) / WV_WAVES), dim3(RC_BLOCK), 0, s->cur, wv_out_cells(v),
                               (const uint8_t*)v.jet.p, w, h, v.prm.grid_x, v.prm.grid_y, cw, ch, (float)v.prm.vis_max_depth, d_bin_map,
                               bin_map_step, d_vis, vis_step);
        }
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_waves_read(rc_ctx* ctx, int stream, rc_wave_cell* cells, long long* sums, long long summary[8]) {
    RcSlot* s; RcWaves* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::wv, "rcflow_waves_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = wv_cells(*vp);
    if (cells) RC_HIP(hipMemcpyAsync(cells, wv_out_cells(*vp), nc * 32, hipMemcpyDeviceToHost, s->cur));
    if (sums) RC_HIP(hipMemcpyAsync(sums, wv_out_sums(*vp), nc * vp->K * 48, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, wv_out_summary(*vp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_waves_spectrum_read(rc_ctx* ctx, int stream, int32_t* spectrum) {
    RcSlot* s; RcWaves* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::wv, "rcflow_waves_spectrum_read", s, vp)) return rc;
    if (!spectrum) { rc_set_error("rcflow_waves_spectrum_read: no buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t plane = (size_t)vp->h * vp->pitch, px = (size_t)vp->w * vp->h;
    for (int k = 0; k < vp->K; k++)
        RC_HIP(hipMemcpy2DAsync(spectrum + 2 * px * k, (size_t)vp->w * 8, (const int2*)vp->acc.p + plane * k, (size_t)vp->pitch * 8, (size_t)vp->w * 8,
                                vp->h, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_waves_table_read(rc_ctx* ctx, int stream, int32_t* tc, int32_t* ts) {
    RcSlot* s; RcWaves* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::wv, "rcflow_waves_table_read", s, vp)) return rc;
    if (tc) memcpy(tc, vp->tc.data(), vp->tc.size() * sizeof(int));
    if (ts) memcpy(ts, vp->ts.data(), vp->ts.size() * sizeof(int));
    return RC_OK;
}

extern "C" int rcflow_waves_set(rc_ctx* ctx, int stream, double tanh_max, int min_pixels, double vis_max_depth) {
    RcSlot* s; RcWaves* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::wv, "rcflow_waves_set", s, vp)) return rc;
    if (!wv_set_ok(tanh_max, min_pixels, vis_max_depth)) {
        rc_set_error("rcflow_waves_set: tanh_max in (0, 1), min_pixels >= 1, vis_max_depth finite and > 0");
        return RC_EINVAL;
    }
    vp->prm.tanh_max = tanh_max;
    vp->prm.min_pixels = min_pixels;
    vp->prm.vis_max_depth = vis_max_depth;
    return RC_OK;
}

extern "C" int rcflow_waves_info(rc_ctx* ctx, int stream, rc_waves_info* info) {
    RcSlot* s; RcWaves* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::wv, "rcflow_waves_info", s, vp)) return rc;
    const RcWaves& v = *vp;
    if (!info) { rc_set_error("rcflow_waves_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->launches_per_push = RC_WAVES_LAUNCHES;
    info->bins = v.K;
    info->shift = v.sh;
    info->held = (int)(v.pushes < v.prm.window ? v.pushes : v.prm.window);
    info->pushes = v.pushes;
    info->device_bytes = v.ring.bytes + v.acc.bytes + v.cacc.bytes + v.out.bytes + v.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_waves_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::wv, "rcflow_waves_reset"); }
extern "C" int rcflow_waves_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::wv); }
