// ripmap_kernels.hip -- the opposing-flow map: where does the water run against the waves?
//
// The reference sketched it and never finished it: averageVector (ripcurrents_module.cpp:386-484, its call commented
// out at main_old.cpp:352) keeps a 300-frame mean of the flow, takes a global direction, averages the direction inside
// a 30 x 30 grid of cells and marks the cells that point more than 0.7 pi away from it.  Its live successor
// (compute_subtructAverageVectorWithWindow, main.cpp:1023-1194) kept the window mean and the colour image and dropped
// the decision.  Here the whole of it is ONE launch per push and nothing synchronises:
//   per pixel   v = the flow (source 0) or get_delta from a zero point with dt = 2 (source 1); the ring slot and the
//               mean in k_window_mean's operation order; the mean in 16.16 fixed point summed per cell (int64: the sum
//               does not depend on the order of addition, so it equals numpy's whatever the tiling); the colour triple
//               of the mean scaled by the PREVIOUS push's maximum, this push's maximum kept on the device;
//   finish      the launch's last-arriving workgroup (rc_hand_off_release of rc_reduce.h) takes the global
//               vector, decides every cell in double in a fixed order, writes cells and summary and zeroes the sums.
// Deviations from averageVector as written, each because the original cannot work: the ring expires (it was passed by
// value there); a cell's mean divides by that cell's own population (there: cell (5, 5)'s); directions are compared
// through dot products of summed vectors (there: angles averaged linearly across the 0 / 360 seam); the remainder
// columns and rows of a frame that the grid does not divide go to the last cell (there: past the array).
//
// Layout: a lane owns 2 consecutive pixels (one 16-byte access per array), a wave 128 pixels of a row and `rows`
// consecutive rows, a block 4 waves stacked vertically.  A lane's columns, hence its cells' columns, do not change
// from row to row: it accumulates in registers while the cell row stays, then the wave reduces per cell column,
// the block's waves meet in LDS, and the block issues one 64-bit atomic per sum and cell it touched.

#include "rc_host.h"
#include "rc_pix3.h"
#include "rc_reduce.h"

#define RM_WAVES 4
static_assert(RC_BLOCK == 64 * RM_WAVES, "a block is RM_WAVES waves, a run of rows each");
#define RM_LDS_CELLS 64        // cells of a block's footprint met in LDS; a larger footprint (cells of a few pixels) adds straight to memory
#define RM_QMAX 1099511627776.f   // 2^40: bound of one pixel's |fixed-point mean|

// control words at the start of RcRipMap::acc.  The ticket has a 128-byte line of its own: every block adds to it.
struct RmCtl {
    RcTicketLine t;             // arrivals of the running launch
    unsigned max_acc;           // bits of this push's maximum |mean| so far (non-negative floats order as integers)
    float scale;                // the previous push's maximum: the colour scale of the next one
    unsigned long long bad;     // pixels left out of the sums by this push
    unsigned pad1[28];
};
static_assert(sizeof(RmCtl) == 256, "the cell sums start 256 bytes into the buffer");

struct RmArgs {
    const float* flow; size_t flow_step;
    const float* thr;                    // source 1: the slot's thresholds, UPPER first
    float2* slot;                        // the ring slot this push replaces, [h][pitch]
    float2* avg;                         // the mean, [h][pitch]
    uint8_t* hsv; size_t hsv_step;
    RmCtl* ctl;
    long long* acc;                      // [gy][gx][Sx, Sy, n]: zero between launches
    long long* sums;                     // the same of the last push, for rcflow_ripmap_read
    float4* cells; double* summary;      // the state's copy
    float4* cells2; double* summary2;    // the caller's, or null
    int w, h, pitch, rows, gx, gy, cw, ch;
    float inv, first_scale;              // first_scale > 0: the first push after open / reset (the reference's 1e-6)
    double K, M;
    int gate;                            // flags bit 0 and the ring not full yet: no cell is opposed
    long long frames;
    unsigned nblocks;
};

typedef float rm_f4u __attribute__((ext_vector_type(4), aligned(1)));   // a 16-byte access of unknown alignment

// get_delta from a zero point (ripcurrents_module.cpp:395-397, :650-679): k_get_delta_field's arithmetic with p = 0, dt = 2
__device__ __forceinline__ float2 rm_delta(const RmArgs& a, int xo, int yo, float UPPER) {
    float2 p = make_float2(0.f, 0.f);
    float dx, dy;
    if (!rc_sample_flow(a.flow, a.flow_step, a.w, a.h, p.x + xo, p.y + yo, dx, dy)) return p;
    const float r = sqrtf(dx * dx + dy * dy);
    if (r > UPPER) return p;
    const float dt = 2.f;
    p.x = p.x + dx * dt;
    p.y = p.y + dy * dt;
    return p;
}

// The wave's register sums of one cell row -> the block's table (or memory).  Cell columns cxa..cxb are the block's.
__device__ __forceinline__ void rm_flush(const RmArgs& a, long long* tab, bool lds, int cxa, int cxb, int cya, int cy,
                                         const int cxl[2], long long sx[2], long long sy[2], int sn[2]) {
    const int nx = cxb - cxa + 1;
    for (int cx = cxa; cx <= cxb; cx++) {
        long long vx = (cxl[0] == cx ? sx[0] : 0) + (cxl[1] == cx ? sx[1] : 0);
        long long vy = (cxl[0] == cx ? sy[0] : 0) + (cxl[1] == cx ? sy[1] : 0);
        long long vn = (cxl[0] == cx ? sn[0] : 0) + (cxl[1] == cx ? sn[1] : 0);
        vx = rc_wave_sum_lane0(vx); vy = rc_wave_sum_lane0(vy); vn = rc_wave_sum_lane0(vn);
        if ((threadIdx.x & 63) == 0 && vn) {
            if (lds) {
                long long* t = tab + 3 * ((cy - cya) * nx + (cx - cxa));
                atomicAdd((unsigned long long*)t, (unsigned long long)vx);
                atomicAdd((unsigned long long*)t + 1, (unsigned long long)vy);
                atomicAdd((unsigned long long*)t + 2, (unsigned long long)vn);
            } else {
                long long* t = a.acc + 3 * ((size_t)cy * a.gx + cx);
                rc_acc_add(t, vx); rc_acc_add(t + 1, vy); rc_acc_add(t + 2, vn);
            }
        }
    }
    sx[0] = sx[1] = sy[0] = sy[1] = 0;
    sn[0] = sn[1] = 0;
}

// The finish, by every thread of the last-arriving block.  Doubles round operation by operation (-ffp-contract=off) in
// the order of tests/_ripmap_ref.py; no transcendental function takes part in a decision.
__device__ void rm_finish(const RmArgs& a, long long* red /* [RM_WAVES][4] */) {
    const int ncell = a.gx * a.gy, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long gx = 0, gy = 0, gn = 0, live = 0;
    for (int c = threadIdx.x; c < ncell; c += RC_BLOCK) {
        const long long sx = rc_acc_take(a.acc + 3 * c), sy = rc_acc_take(a.acc + 3 * c + 1), n = rc_acc_take(a.acc + 3 * c + 2);
        a.sums[3 * c] = sx; a.sums[3 * c + 1] = sy; a.sums[3 * c + 2] = n;     // read back below by this same thread
        gx += sx; gy += sy; gn += n; live += n > 0;
    }
    gx = rc_wave_sum_lane0(gx); gy = rc_wave_sum_lane0(gy); gn = rc_wave_sum_lane0(gn); live = rc_wave_sum_lane0(live);
    if (lane == 0) { red[4 * wv] = gx; red[4 * wv + 1] = gy; red[4 * wv + 2] = gn; red[4 * wv + 3] = live; }
    __syncthreads();
    gx = gy = gn = live = 0;
    for (int k = 0; k < RM_WAVES; k++) { gx += red[4 * k]; gy += red[4 * k + 1]; gn += red[4 * k + 2]; live += red[4 * k + 3]; }
    __syncthreads();
    const double Gx = (double)gx, Gy = (double)gy;
    const double gg = Gx * Gx + Gy * Gy;
    const double deg = 180.0 / 3.14159265358979323846;
    long long opp = 0;
    for (int c = threadIdx.x; c < ncell; c += RC_BLOCK) {
        const long long sx = a.sums[3 * c], sy = a.sums[3 * c + 1], n = a.sums[3 * c + 2];
        const double Sx = (double)sx, Sy = (double)sy, dn = (double)n;
        const double dot = Sx * Gx + Sy * Gy;
        const double cc = Sx * Sx + Sy * Sy;
        const double need = (a.M * 65536.0) * dn;
        const bool opposed = !a.gate && n > 0 && dot < 0. && dot * dot > a.K * (cc * gg) && cc >= need * need;
        float4 o = make_float4(0.f, 0.f, 0.f, opposed ? 1.f : 0.f);
        if (n > 0) {
            o.x = (float)(Sx / 65536.0 / dn);
            o.y = (float)(Sy / 65536.0 / dn);
            const double cross = Sx * Gy - Sy * Gx;
            o.z = (float)(atan2(fabs(cross), dot) * deg);          // for people: held to a tolerance, never to bits
        }
        a.cells[c] = o;
        if (a.cells2) a.cells2[c] = o;
        opp += opposed;
    }
    opp = rc_wave_sum_lane0(opp);
    if (lane == 0) red[4 * wv] = opp;
    __syncthreads();
    if (threadIdx.x != 0) return;
    opp = 0;
    for (int k = 0; k < RM_WAVES; k++) opp += red[4 * k];
    const unsigned long long bad = rc_acc_take(&a.ctl->bad);
    const unsigned mbits = rc_acc_take(&a.ctl->max_acc);
    const float mx = __uint_as_float(mbits);
    a.ctl->scale = mx;                       // every block of this launch read the old one before it drew its ticket
    double dir = atan2(Gy, Gx) * deg;
    if (dir < 0.) dir += 360.;
    if (dir >= 360.) dir = 0.;
    double mag = 0.;
    if (gn > 0) {
        const double mxx = Gx / 65536.0 / (double)gn, myy = Gy / 65536.0 / (double)gn;
        mag = sqrt(mxx * mxx + myy * myy);
    }
    const double s[8] = {dir, mag, (double)opp, (double)live, (double)bad, (double)a.frames, (double)mx, 0.};
    for (int k = 0; k < 8; k++) {
        a.summary[k] = s[k];
        if (a.summary2) a.summary2[k] = s[k];
    }
    __hip_atomic_store(&a.ctl->t.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next push (stream order)
}

template <int SOURCE>
__global__ __launch_bounds__(RC_BLOCK) void k_ripmap(const RmArgs a) {
    __shared__ long long tab[RM_LDS_CELLS * 3];
    __shared__ long long red[RM_WAVES * 4];
    __shared__ float red_max[RM_WAVES];
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xb = blockIdx.x * 128, yb = blockIdx.y * (RM_WAVES * a.rows);          // inside the frame by the grid's size
    const int x0 = xb + 2 * lane, np = min(2, a.w - x0);
    // the block's footprint in cells; the remainder columns / rows belong to the last cell
    const int cxa = min(xb / a.cw, a.gx - 1), cxb = min((min(xb + 128, a.w) - 1) / a.cw, a.gx - 1);
    const int cya = min(yb / a.ch, a.gy - 1), cyb = min((min(yb + RM_WAVES * a.rows, a.h) - 1) / a.ch, a.gy - 1);
    const int ntab = (cxb - cxa + 1) * (cyb - cya + 1);
    const bool lds = ntab <= RM_LDS_CELLS;
    if (lds)
        for (int i = threadIdx.x; i < 3 * ntab; i += RC_BLOCK) tab[i] = 0;
    __syncthreads();

    const int cxl[2] = {min(x0 / a.cw, a.gx - 1), min((x0 + 1) / a.cw, a.gx - 1)};
    const float scale = a.first_scale > 0.f ? a.first_scale : a.ctl->scale;
    float UPPER = 0.f;
    if (SOURCE == 1) UPPER = a.thr[0];
    long long sx[2] = {0, 0}, sy[2] = {0, 0};
    int sn[2] = {0, 0};
    unsigned bad = 0;
    float mx = 0.f;
    int cur_cy = -1;
    const int y0 = yb + wv * a.rows;
    for (int r = 0; r < a.rows; r++) {
        const int y = y0 + r;
        if (y >= a.h) break;
        const int cy = min(y / a.ch, a.gy - 1);
        if (cy != cur_cy) {
            if (cur_cy >= 0) rm_flush(a, tab, lds, cxa, cxb, cya, cur_cy, cxl, sx, sy, sn);
            cur_cy = cy;
        }
        if (np <= 0) continue;
        // 1. the vector
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (SOURCE == 0) {
            // rows are 8-byte aligned only; global memory takes an unaligned dwordx4 on this target, and the compiler
            // emits one for a copy whose source alignment it does not know
            const char* fr = (const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x0;
            if (np == 2) {
                const rm_f4u t = *(const rm_f4u*)fr;
                v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
            } else {
                const float2 t = *(const float2*)fr;
                v[0] = t.x; v[1] = t.y;
            }
        } else {
            const float2 d0 = rm_delta(a, x0, y, UPPER);
            v[0] = d0.x; v[1] = d0.y;
            if (np == 2) { const float2 d1 = rm_delta(a, x0 + 1, y, UPPER); v[2] = d1.x; v[3] = d1.y; }
        }
        // 2. ring and mean, k_window_mean's order per float: a = avg - slot * inv; slot = v; avg = a + v * inv
        const size_t o = (size_t)y * a.pitch + x0;
        float4* sp = (float4*)(a.slot + o);
        float4* mp = (float4*)(a.avg + o);
        const float4 s4 = *sp, m4 = *mp;
        const float s[4] = {s4.x, s4.y, s4.z, s4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float t = s[k] * a.inv;
            const float d = m[k] - t;
            t = v[k] * a.inv;
            g[k] = d + t;
        }
        *sp = make_float4(v[0], v[1], v[2], v[3]);       // the column past an odd w holds zeros and stays zero
        *mp = make_float4(g[0], g[1], g[2], g[3]);
        uint8_t px[6];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (k >= np) break;
            const float ax = g[2 * k], ay = g[2 * k + 1];
            // 3. fixed point: a scaling by 2^16 is exact; NaN fails the comparison
            const float qx = ax * 65536.0f, qy = ay * 65536.0f;
            if (fabsf(qx) <= RM_QMAX && fabsf(qy) <= RM_QMAX) {
                sx[k] += (long long)rintf(qx);
                sy[k] += (long long)rintf(qy);
                sn[k]++;
            } else {
                bad++;
            }
            // 4. k_vector_to_color's triple of the mean (its expression, to the letter; tested byte for byte)
            float theta = (float)((float)atan2((double)ay, (double)ax) * 180 / 3.14159265358979323846);
            theta += theta < 0 ? 360 : 0;
            const float mag = sqrtf(ax * ax + ay * ay);
            mx = fmaxf(mx, mag);
            px[3 * k] = rc_f2u8(theta / 2);
            px[3 * k + 1] = 255;
            px[3 * k + 2] = rc_f2u8(mag * 255 / scale);
        }
        if (a.hsv) {
            uint8_t* q = a.hsv + (size_t)y * a.hsv_step + 3 * (size_t)x0;
            if (np == 2) __builtin_memcpy(q, px, 6);
            else { q[0] = px[0]; q[1] = px[1]; q[2] = px[2]; }
        }
    }
    if (cur_cy >= 0) rm_flush(a, tab, lds, cxa, cxb, cya, cur_cy, cxl, sx, sy, sn);
    bad = (unsigned)rc_wave_sum_lane0((long long)bad);
    mx = rc_wave_max_lane0(mx);
    if (lane == 0) { red[wv] = bad; red_max[wv] = mx; }
    __syncthreads();
    // one atomic per sum and cell the block touched, as lanes of one instruction
    if (lds && threadIdx.x < 3 * ntab) {
        const long long val = tab[threadIdx.x];
        const int c = threadIdx.x / 3, k = threadIdx.x - 3 * c, nx = cxb - cxa + 1;
        const int cy = cya + c / nx, cx = cxa + c % nx;
        if (val) rc_acc_add(a.acc + 3 * ((size_t)cy * a.gx + cx) + k, val);
    }
    if (threadIdx.x == 0) {
        unsigned b = 0;
        float m = 0.f;
        for (int k = 0; k < RM_WAVES; k++) { b += (unsigned)red[k]; m = fmaxf(m, red_max[k]); }
        if (b) rc_acc_add(&a.ctl->bad, (unsigned long long)b);
        // the maximum only grows: a block below what is there already has nothing to add
        const unsigned mb = __float_as_uint(m);
        if (mb > rc_acc_load(&a.ctl->max_acc))
            __hip_atomic_fetch_max(&a.ctl->max_acc, mb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (rc_hand_off_release(&a.ctl->t.ticket, a.nblocks, &last)) rm_finish(a, red);
}

// "ripmap@1": 255 inside an opposed cell.  A thread owns 4 consecutive pixels of a row (rc_pix3.h's span, one byte each).
__global__ __launch_bounds__(RC_BLOCK) void k_ripmap_mask(const float4* cells, int w, int h, int gx, int gy, int cw, int ch,
                                                          uint8_t* mask, size_t mask_step) {
    const RcPix3Span t = rc_pix3_span(w, 1);
    const int x0 = t.x0, n = t.n, y = t.y0;
    if (n <= 0 || y >= h) return;
    const float4* row = cells + (size_t)min(y / ch, gy - 1) * gx;
    uint8_t* q = mask + (size_t)y * mask_step + x0;
    uint32_t m = 0;
    for (int k = 0; k < n; k++)
        if (row[min((x0 + k) / cw, gx - 1)].w != 0.f) m |= 255u << (8 * k);
    if (n == 4) __builtin_memcpy(q, &m, 4);
    else
        for (int k = 0; k < n; k++) q[k] = (uint8_t)(m >> (8 * k));
}

// ============================================================================ host side
void rc_state_free(RcRipMap& m) {
    rc_buf_free(m.ring); rc_buf_free(m.avg); rc_buf_free(m.acc); rc_buf_free(m.out);
    rc_fence_free(m.zf);
    m = RcRipMap();
}

static size_t rm_cells(const RcRipMap& m) { return (size_t)m.gx * m.gy; }
// RcRipMap::out: cells [cells] float4 | sums [cells][3] int64 | summary 8 doubles
static float4* rm_out_cells(const RcRipMap& m) { return (float4*)m.out.p; }
static long long* rm_out_sums(const RcRipMap& m) { return (long long*)((char*)m.out.p + rm_cells(m) * 16); }
static double* rm_out_summary(const RcRipMap& m) { return (double*)((char*)m.out.p + rm_cells(m) * 40); }

int rc_state_zero(RcSlot& s, RcRipMap& m) {
    const int rc = rc_fence_zero(m.zf, s.cur, {&m.ring, &m.avg, &m.acc, &m.out});
    if (!rc) m.frames = m.cur = 0;
    return rc;
}

extern "C" int rcflow_ripmap_open(rc_ctx* ctx, int stream, int w, int h, int window, int grid_x, int grid_y, int source,
                                  int flags) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (w <= 0 || h <= 0) { rc_set_error("rcflow_ripmap_open: bad frame size %d x %d", w, h); return RC_EINVAL; }
    if (window < 1 || window > 4096) { rc_set_error("rcflow_ripmap_open: window %d outside 1..4096", window); return RC_EINVAL; }
    if (grid_x < 1 || grid_y < 1 || grid_x > w || grid_y > h || (long long)grid_x * grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("rcflow_ripmap_open: grid %d x %d does not fit a %d x %d frame (at most %d cells)", grid_x, grid_y, w, h,
                     RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    if (source < 0 || source > 1 || (flags & ~RC_RIPMAP_WAIT_FULL)) {
        rc_set_error("rcflow_ripmap_open: bad source %d or flags %d", source, flags);
        return RC_EINVAL;
    }
    int rc = rc_fits_context("rcflow_ripmap_open", ctx, w, h);
    if (rc) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcRipMap n;
    n.w = w; n.h = h; n.window = window; n.gx = grid_x; n.gy = grid_y; n.source = source; n.flags = flags;
    n.pitch = (w + 1) & ~1;
    const size_t plane = (size_t)n.pitch * h * sizeof(float2), nc = rm_cells(n);
    rc = rc_buf_ensure(n.ring, plane * (size_t)window);
    if (!rc) rc = rc_buf_ensure(n.avg, plane);
    if (!rc) rc = rc_buf_ensure(n.acc, sizeof(RmCtl) + nc * 24);
    if (!rc) rc = rc_buf_ensure(n.out, nc * 40 + 64);
    return rc_state_install(*s, s->rm, n, rc);
}

extern "C" int rcflow_ripmap_set(rc_ctx* ctx, int stream, double min_opposition_cos2, double min_cell_mag) {
    RcSlot* s; RcRipMap* m;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rm, "rcflow_ripmap_set", s, m)) return rc;
    if (!(min_opposition_cos2 >= 0. && min_opposition_cos2 < 1.) || !(min_cell_mag >= 0. && min_cell_mag < 1e6)) {
        rc_set_error("rcflow_ripmap_set: min_opposition_cos2 must be in [0, 1), min_cell_mag in [0, 1e6)");
        return RC_EINVAL;
    }
    m->K = min_opposition_cos2;
    m->M = min_cell_mag;
    return RC_OK;
}

extern "C" int rcflow_ripmap_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::rm, "rcflow_ripmap_reset"); }
extern "C" int rcflow_ripmap_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::rm); }

extern "C" int rcflow_ripmap_info(rc_ctx* ctx, int stream, int* w, int* h, int* window, int* grid_x, int* grid_y, int* source,
                                  int* flags, double* min_opposition_cos2, double* min_cell_mag, long long* frames_pushed,
                                  size_t* device_bytes) {
    RcSlot* s; RcRipMap* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rm, "rcflow_ripmap_info", s, mp)) return rc;
    const RcRipMap& m = *mp;
    if (w) *w = m.w;
    if (h) *h = m.h;
    if (window) *window = m.window;
    if (grid_x) *grid_x = m.gx;
    if (grid_y) *grid_y = m.gy;
    if (source) *source = m.source;
    if (flags) *flags = m.flags;
    if (min_opposition_cos2) *min_opposition_cos2 = m.K;
    if (min_cell_mag) *min_cell_mag = m.M;
    if (frames_pushed) *frames_pushed = m.frames;
    if (device_bytes) *device_bytes = m.ring.bytes + m.avg.bytes + m.acc.bytes + m.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_ripmap_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, uint8_t* d_hsv,
                                      size_t hsv_step, uint8_t* d_mask, size_t mask_step, float* d_cells, double* d_summary) {
    static const char* who = "rcflow_ripmap_push_dev";
    RcSlot* s; RcRipMap* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rm, who, s, mp)) return rc;
    RcRipMap& m = *mp;
    if (!d_flow_xy) {                                     // the slot's resident field (rcflow_stream_flow_ptr)
        if (!s->flow_w) { rc_set_error("no flow field is resident on the slot yet"); return RC_ESTATE; }
        if (s->flow_w != m.w || s->flow_h != m.h) {
            rc_set_error("the resident flow field is %d x %d, the map %d x %d", s->flow_w, s->flow_h, m.w, m.h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)m.w * 8;
    } else if (rc_image_check(who, "d_flow_xy", d_flow_xy, flow_step, m.w, m.h, 8, 8, RC_ARG_IN | RC_ARG_ANY_BASE)) {
        return RC_EINVAL;
    }
    if (rc_image_check(who, "d_hsv", d_hsv, hsv_step, m.w, m.h, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL)) return RC_EINVAL;
    if (rc_image_check(who, "d_mask", d_mask, mask_step, m.w, m.h, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL)) return RC_EINVAL;
    if (m.source == 1 && !s->an.thr.p) { rc_set_error("source 1 reads UPPER from the slot's analysis state (rcflow_analysis_reset)"); return RC_ESTATE; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(m.zf, s->cur, true);
    if (rc) return rc;
    RmArgs a;
    a.flow = d_flow_xy; a.flow_step = flow_step;
    a.thr = (const float*)s->an.thr.p;
    const size_t plane = (size_t)m.pitch * m.h;
    a.slot = (float2*)m.ring.p + plane * (size_t)m.cur;
    a.avg = (float2*)m.avg.p;
    a.hsv = d_hsv; a.hsv_step = hsv_step;
    a.ctl = (RmCtl*)m.acc.p;
    a.acc = (long long*)((char*)m.acc.p + sizeof(RmCtl));
    a.sums = rm_out_sums(m); a.cells = rm_out_cells(m); a.summary = rm_out_summary(m);
    a.cells2 = (float4*)d_cells; a.summary2 = d_summary;
    a.w = m.w; a.h = m.h; a.pitch = m.pitch;
    a.rows = rc_rows_per_wave(m.w, m.h, 4);
    a.gx = m.gx; a.gy = m.gy; a.cw = m.w / m.gx; a.ch = m.h / m.gy;
    a.inv = (float)(1. / (float)m.window);                // rcflow_window_mean_dev's
    a.first_scale = m.frames == 0 ? 1e-6f : 0.f;
    a.K = m.K; a.M = m.M;
    m.frames++;
    a.gate = (m.flags & RC_RIPMAP_WAIT_FULL) && m.frames < m.window;
    a.frames = m.frames;
    const dim3 grid((m.w + 127) / 128, (m.h + RM_WAVES * a.rows - 1) / (RM_WAVES * a.rows));
    a.nblocks = grid.x * grid.y;
    {
        // flow 8 + slot 8 in, slot 8 out, mean 8 in / 8 out, colour 3
        RcProfScope ps(ctx, s->cur, RC_K_RIPMAP, 0, (double)m.w * m.h * (40. + (d_hsv ? 3. : 0.)));
        if (m.source == 0) hipLaunchKernelGGL(k_ripmap<0>, grid, dim3(RC_BLOCK), 0, s->cur, a);
        else hipLaunchKernelGGL(k_ripmap<1>, grid, dim3(RC_BLOCK), 0, s->cur, a);
    }
    m.cur = m.cur + 1 >= m.window ? 0 : m.cur + 1;
    if (d_mask) {
        RcProfScope ps(ctx, s->cur, RC_K_RIPMAP, 1, (double)m.w * m.h);
        hipLaunchKernelGGL(k_ripmap_mask, rc_pix3_grid(m.w, m.h, 1), dim3(RC_BLOCK), 0, s->cur,
                           a.cells, m.w, m.h, m.gx, m.gy, a.cw, a.ch, d_mask, mask_step);
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_ripmap_mean_dev(rc_ctx* ctx, int stream, float* d_mean_xy, size_t mean_step) {
    static const char* who = "rcflow_ripmap_mean_dev";
    RcSlot* s; RcRipMap* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rm, who, s, mp)) return rc;
    RcRipMap& m = *mp;
    if (rc_image_check(who, "d_mean_xy", d_mean_xy, mean_step, m.w, m.h, 8, 1, RC_ARG_OUT)) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(m.zf, s->cur, true);
    if (rc) return rc;
    RC_HIP(hipMemcpy2DAsync(d_mean_xy, mean_step, m.avg.p, (size_t)m.pitch * 8, (size_t)m.w * 8, m.h, hipMemcpyDeviceToDevice, s->cur));
    return RC_OK;
}

extern "C" int rcflow_ripmap_read(rc_ctx* ctx, int stream, float* cells, double* summary, long long* sums,
                                  long long* frames_pushed) {
    RcSlot* s; RcRipMap* mp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rm, "rcflow_ripmap_read", s, mp)) return rc;
    RcRipMap& m = *mp;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(m.zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = rm_cells(m);
    if (sums) RC_HIP(hipMemcpyAsync(sums, rm_out_sums(m), nc * 24, hipMemcpyDeviceToHost, s->cur));
    if (cells) RC_HIP(hipMemcpyAsync(cells, rm_out_cells(m), nc * 16, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, rm_out_summary(m), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    if (frames_pushed) *frames_pushed = m.frames;
    return RC_OK;
}
