// shoreline_kernels.hip -- shoreline: where does the water end, and how far does it run up?
//
// A wet/dry indicator of a picture that is already on the device (the time-exposure MEAN, the plan view's picture, a frame, or a
// plane of the caller's), smoothed by a box, split by Otsu's threshold; along lines laid from land to sea the best split of the
// samples into a dry and a wet run, its position to 1/256 sample, the waterline point; along the shore an outlier test; per line a
// ring of the last `window` positions and from it the runup statistics.  include/rcflow.h ("shoreline") is the specification;
// tests/_shoreline_ref.py states it in numpy and the kernels are held to that bit for bit: everything is integer except Otsu's
// score and separability and the records' conversions, which are double, operation by operation.  A push is three launches, four
// when a picture is asked for, and nothing synchronises:
//   shoreline@0  A tile is 64 columns and SH_TH rows; a block walks as many tiles, one below the other, as keep the launch to about
//                SH_MAX_BLOCKS blocks (the shape of kinematics@0).  The indicator with a halo of r, coordinates clamped to the
//                picture, goes into LDS as uint16: a lane takes 4 pixels of the tile's 64 columns at once (12 bytes of an 8UC3 row),
//                a wave 4 rows a pass; the 2 r halo columns pixel by pixel.  Horizontal sums into a second array, vertical sums
//                from it, a wave one LDS row at a time; J to the state plane; the histogram per wave in LDS, met and flushed once
//                per block as one atomic per bin it touched.  The last-arriving block (rc_hand_off_release of rc_reduce.h)
//                takes the histogram out, leaves it zero, and its first wave scans the 511 bins: a lane 8 bins, the prefix sums by
//                a wave scan, the first largest score by a wave reduction;
//   shoreline@1  a wave a line: the samples into LDS, a lane a run of consecutive samples, the dry counts before each run by a wave
//                scan, the best split by a wave reduction (the smallest k of the largest score);
//   shoreline@2  a block a line: the outlier test against the neighbours' points, the ring slot, the held positions sorted in LDS
//                (bitonic) for the rank, the record; the launch's last block writes the summary behind the fenced ticket;
//   shoreline@3  mask, plane and histogram out, a lane 4 pixels;
//   shoreline@4  the primitives, a lane a line.

#include <math.h>
#include <string.h>

#include <vector>

#include "rc_pix3.h"
#include "rc_host.h"
#include "rc_reduce.h"

#define SH_WAVES 4
static_assert(RC_BLOCK == 64 * SH_WAVES, "a block is SH_WAVES waves");
#define SH_TW 64
#define SH_RPW 8               // rows a wave walks
#define SH_TH (SH_WAVES * SH_RPW)
#define SH_MAX_BLOCKS 512      // every block ends in a flush, a release and a ticket on one line (as kinematics@0); at 1080p caps of
                               // 128, 256, 512 and 1024 gave 44, 31, 28 and 37 us (profiles/shoreline_kernel_summary.md)
#define SH_FH (SH_TH + 2 * RC_SHORE_MAX_RADIUS)
#define SH_FW (SH_TW + 2 * RC_SHORE_MAX_RADIUS)
#define SH_LIVE (RC_SHORE_HIST - 1)
static_assert(sizeof(rc_shoreline) == 64 && sizeof(rc_shoreline_params) == 56, "the records of include/rcflow.h have the sizes the Python and numpy mirrors give them");
static_assert(RC_SHORE_MAX_SAMPLES <= 64 * 16 && RC_SHORE_MAX_WINDOW == 4096, "shoreline@1 gives a lane 16 samples at most, shoreline@2 sorts 4096 positions in LDS");

// RcShoreline::ctl.  Each ticket has a 128-byte line of its own: every block adds to it
struct ShCtl {
    RcTicketLine t0;
    unsigned ticket2, cnt[4]; unsigned pad1[27];
    int thr; unsigned pad2; long long N; double eta; unsigned pad3[26];   // of the last shoreline@0
    unsigned hist[RC_SHORE_HIST];                                          // live: zero between launches
};
static_assert(sizeof(ShCtl) == 384 + 4 * RC_SHORE_HIST, "three lines and the histogram");

// what shoreline@1 hands to shoreline@2
struct ShLine { int flags, k, pos, agree, wx, wy, pad[2]; };

__device__ __forceinline__ bool sh_wet(int v, int thr, int high) { return high ? v > thr : v <= thr; }

// ============================================================================ shoreline@0: indicator, box, plane, histogram, Otsu
struct ShArgs0 {
    const uint8_t* img; size_t step;
    const uint8_t* roi; size_t roi_step;         // or null
    uint16_t* plane;                             // the state's, [h][w]
    ShCtl* ctl;
    uint32_t* hist_out;                          // the state's copy of the push's histogram
    int w, h, source, tiles, fixed;              // a block walks `tiles` tiles, one below the other
    unsigned nblocks;
};

__device__ __forceinline__ int sh_ind(uint32_t p, int source) {
    return source == RC_SHORE_RMB ? (int)(p >> 16) - (int)(p & 255u) + 255
                                  : (int)(((p & 255u) * 1868u + ((p >> 8) & 255u) * 9617u + (p >> 16) * 4899u + (1u << 13)) >> 14);
}
// pixel (x, y) of the picture, both inside it
__device__ __forceinline__ int sh_ind_at(const ShArgs0& a, int x, int y) {
    const uint8_t* row = a.img + (size_t)y * a.step;
    if (a.source == RC_SHORE_PLANE) return row[x];
    const uint8_t* p = row + 3 * (size_t)x;
    return sh_ind((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16), a.source);
}

template <int R>
__global__ __launch_bounds__(RC_BLOCK) void k_sh_pixels(const ShArgs0 a) {
    __shared__ uint16_t I[(SH_TH + 2 * R) * (SH_TW + 2 * R)];   // the indicator from (x0 - R, y0 - R), coordinates clamped
    __shared__ uint16_t H[(SH_TH + 2 * R) * SH_TW];             // the horizontal sums from (x0, y0 - R): at most 15 * 510
    __shared__ unsigned hist[SH_WAVES][RC_SHORE_HIST];
    __shared__ int last;
    constexpr int FW = SH_TW + 2 * R, FH = SH_TH + 2 * R, A = (2 * R + 1) * (2 * R + 1);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SH_TW, x = x0 + lane;
    for (int i = threadIdx.x; i < SH_WAVES * RC_SHORE_HIST; i += RC_BLOCK) (&hist[0][0])[i] = 0u;
    for (int t = 0; t < a.tiles; t++) {
        const int y0 = (blockIdx.y * a.tiles + t) * SH_TH;
        if (y0 >= a.h) break;                                 // the whole block leaves
        __syncthreads();                                      // the last tile's reads of I and H; the zeroed histogram
        // the tile's 64 columns: a lane 4 pixels, a wave 4 rows a pass
        for (int rr = wv * 4 + (lane >> 4); rr < FH; rr += 4 * SH_WAVES) {
            const int y = rc_clampi(y0 - R + rr, 0, a.h - 1), cx = x0 + 4 * (lane & 15);
            const uint8_t* row = a.img + (size_t)y * a.step;
            uint16_t* dst = I + rr * FW + R + 4 * (lane & 15);
            if (cx + 4 <= a.w) {
                if (a.source == RC_SHORE_PLANE) {
                    uint32_t q;
                    __builtin_memcpy(&q, row + cx, 4);
#pragma unroll
                    for (int k = 0; k < 4; k++) dst[k] = (uint16_t)((q >> (8 * k)) & 255u);
                } else {
                    uint32_t px[4];
                    rc_pix3_load4(row, cx, 4, px);
#pragma unroll
                    for (int k = 0; k < 4; k++) dst[k] = (uint16_t)sh_ind(px[k], a.source);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) dst[k] = (uint16_t)sh_ind_at(a, min(cx + k, a.w - 1), y);
            }
        }
        // the 2 R halo columns
        if constexpr (R > 0)
            for (int i = threadIdx.x; i < FH * 2 * R; i += RC_BLOCK) {
                const int rr = i / (2 * R), c = i - rr * 2 * R, col = c < R ? c : c + SH_TW;
                I[rr * FW + col] = (uint16_t)sh_ind_at(a, rc_clampi(x0 - R + col, 0, a.w - 1), rc_clampi(y0 - R + rr, 0, a.h - 1));
            }
        __syncthreads();
        for (int rr = wv; rr < FH; rr += SH_WAVES) {
            const uint16_t* p = I + rr * FW + lane;
            int s = 0;
#pragma unroll
            for (int k = 0; k <= 2 * R; k++) s += p[k];
            H[rr * SH_TW + lane] = (uint16_t)s;
        }
        __syncthreads();
        for (int j = 0; j < SH_RPW; j++) {
            const int ly = wv * SH_RPW + j, y = y0 + ly;
            if (y >= a.h) break;                              // the whole wave leaves
            const uint16_t* p = H + ly * SH_TW + lane;
            int s = 0;
#pragma unroll
            for (int k = 0; k <= 2 * R; k++) s += p[k * SH_TW];
            const int J = (2 * s + A) / (2 * A);
            if (x < a.w) {
                a.plane[(size_t)y * a.w + x] = (uint16_t)J;
                if (!a.roi || a.roi[(size_t)y * a.roi_step + x]) atomicAdd(&hist[wv][J], 1u);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SH_LIVE; b += RC_BLOCK) {
        const unsigned v = hist[0][b] + hist[1][b] + hist[2][b] + hist[3][b];
        if (v) rc_acc_add(&a.ctl->hist[b], v);
    }
    if (!rc_hand_off_release(&a.ctl->t0.ticket, a.nblocks, &last)) return;

    // Otsu, by the last-arriving block: the histogram out of the live words, which are left zero for the next push
    unsigned* lh = hist[0];
    for (int b = threadIdx.x; b < RC_SHORE_HIST; b += RC_BLOCK) {
        const unsigned v = b < SH_LIVE ? rc_acc_take(&a.ctl->hist[b]) : 0u;
        lh[b] = v;
        a.hist_out[b] = v;
    }
    __syncthreads();
    if (wv != 0) return;
    long long lw = 0, lm = 0, l2 = 0;                         // a lane 8 bins
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const long long i = 8 * lane + k, v = lh[i];
        lw += v; lm += i * v; l2 += i * i * v;
    }
    long long pw = lw, pm = lm;                               // inclusive over the lanes
    for (int o = 1; o < 64; o <<= 1) {
        const long long tw = __shfl_up(pw, o, 64), tm = __shfl_up(pm, o, 64);
        if (lane >= o) { pw += tw; pm += tm; }
    }
    const long long N = __shfl(pw, 63, 64), S1 = __shfl(pm, 63, 64), S2 = rc_wave_sum_all(l2);
    long long w0 = pw - lw, m0 = pm - lm;
    double best = -1., sfix = 0.;
    int bt = -1;
    for (int k = 0; k < 8; k++) {
        const int t = 8 * lane + k;
        if (t > SH_LIVE - 2) break;                           // t = 0..509
        const long long v = lh[t];
        w0 += v; m0 += t * v;
        const long long w1 = N - w0;
        if (w0 == 0 || w1 == 0) continue;
        const long long d = S1 * w0 - m0 * N;
        const double s = ((double)d * (double)d) / ((double)w0 * (double)w1);
        if (t == a.fixed) sfix = s;
        if (s > best) { best = s; bt = t; }                   // the first largest of the lane's
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(best, o, 64), of = __shfl_xor(sfix, o, 64);
        const int ot = __shfl_xor(bt, o, 64);
        if (ot >= 0 && (bt < 0 || os > best || (os == best && ot < bt))) { best = os; bt = ot; }
        sfix = sfix + of;                                     // one lane's is not zero
    }
    if (lane != 0) return;
    const double tot = (double)N * (double)S2 - (double)S1 * (double)S1;
    int thr = bt;
    double s = best;
    if (a.fixed >= 0) { thr = N > 0 ? a.fixed : -1; s = sfix; }
    a.ctl->thr = thr;                                         // read by the next launches (stream order)
    a.ctl->N = N;
    a.ctl->eta = thr >= 0 && tot > 0. ? s / tot : 0.;
    __hip_atomic_store(&a.ctl->t0.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================================ shoreline@1: samples, best split, position
struct ShArgs1 {
    const rc_transect_sample* table; const rc_transect_geom* geom;
    const uint16_t* plane;
    const ShCtl* ctl;
    ShLine* lin;
    int w, h, L, wet_is_high;
    double min_sep;
};

__global__ __launch_bounds__(RC_BLOCK) void k_sh_lines(const ShArgs1 a) {
    __shared__ uint16_t Vs[SH_WAVES][RC_SHORE_MAX_SAMPLES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int line = blockIdx.x * SH_WAVES + wv;
    const bool active = line < a.L;
    const int thr = a.ctl->thr;
    uint16_t* V = Vs[wv];
    int n = 0, first = 0;
    if (active) {
        const rc_transect_geom gm = a.geom[line];
        n = gm.n; first = gm.first;
        if (thr >= 0)
            for (int j = lane; j < n; j += 64) {
                const rc_transect_sample sm = a.table[(size_t)first + j];
                const int ix = sm.X >> 4, fx = sm.X & 15, iy = sm.Y >> 4, fy = sm.Y & 15;
                const int ix1 = min(ix + 1, a.w - 1), iy1 = min(iy + 1, a.h - 1);
                const uint16_t* r0 = a.plane + (size_t)iy * a.w;
                const uint16_t* r1 = a.plane + (size_t)iy1 * a.w;
                V[j] = (uint16_t)(((16 - fx) * (16 - fy) * r0[ix] + fx * (16 - fy) * r0[ix1] + (16 - fx) * fy * r1[ix] + fx * fy * r1[ix1] + 128) >> 8);
            }
    }
    __syncthreads();                                          // the block's only one: every wave reaches it
    if (!active) return;
    ShLine o;
    memset(&o, 0, sizeof(o));
    o.pos = -1;
    if (thr < 0) {
        o.flags = RC_SHORE_EMPTY;
        if (lane == 0) a.lin[line] = o;
        return;
    }
    // a lane a run of c consecutive samples; D: dry samples before k
    const int c = (n + 63) / 64, j0 = min(lane * c, n), j1 = min(j0 + c, n);
    int ld = 0;
    for (int j = j0; j < j1; j++) ld += !sh_wet(V[j], thr, a.wet_is_high);
    int inc = ld;
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(inc, s, 64);
        if (lane >= s) inc += t;
    }
    const int Dtot = __shfl(inc, 63, 64), Wtot = n - Dtot;
    int D = inc - ld, best = -1, bk = 0x7fffffff;
    for (int k = j0; k < j1; k++) {                           // score(k) = D(k) + (Wtot - (k - D(k)))
        const int sc = 2 * D - k + Wtot;
        if (sc > best) { best = sc; bk = k; }
        D += !sh_wet(V[k], thr, a.wet_is_high);
    }
    if (lane == 0 && Dtot > best) { best = Dtot; bk = n; }    // k = n, the largest k: it wins only when strictly better
    for (int s = 32; s > 0; s >>= 1) {
        const int ob = __shfl_xor(best, s, 64), ok = __shfl_xor(bk, s, 64);
        if (ob > best || (ob == best && ok < bk)) { best = ob; bk = ok; }
    }
    if (lane != 0) return;
    o.k = bk; o.agree = best;
    if (a.ctl->eta < a.min_sep) o.flags |= RC_SHORE_UNSURE;
    if (bk == n) o.flags |= RC_SHORE_DRY;
    else if (bk == 0) o.flags |= RC_SHORE_WET;
    else {
        const int va = V[bk - 1], vb = V[bk], d = abs(vb - va), e = abs(2 * thr + 1 - 2 * va);   // d >= 1: one is dry, one wet
        const int frac = (e * 256 + d) / (2 * d);
        const long long pos = (long long)(bk - 1) * 256 + frac, den = 256ll * (n - 1);
        const rc_transect_sample sa = a.table[first], sb = a.table[(size_t)first + n - 1];
        o.pos = (int)pos;
        o.wx = (int)(16ll * sa.X + rc_floor_div(16ll * (sb.X - sa.X) * pos + 128ll * (n - 1), den));
        o.wy = (int)(16ll * sa.Y + rc_floor_div(16ll * (sb.Y - sa.Y) * pos + 128ll * (n - 1), den));
    }
    a.lin[line] = o;
}

// ============================================================================ shoreline@2: outliers, ring, window, records
struct ShArgs2 {
    const rc_transect_geom* geom;
    const ShLine* lin;
    int* ring;                                   // [L][T]
    rc_shoreline* rec; long long* summary;       // the state's copy
    rc_shoreline* rec2; long long* summary2;     // the caller's, or null
    ShCtl* ctl;
    int L, T, c, held, permille;
    long long lim, pushes;
};

__global__ __launch_bounds__(RC_BLOCK) void k_sh_records(const ShArgs2 a) {
    __shared__ int vals[RC_SHORE_MAX_WINDOW];
    __shared__ unsigned long long sum;
    __shared__ int cur, flags, nvs, last;
    const int line = blockIdx.x;
    if (threadIdx.x == 0) {
        const ShLine me = a.lin[line];
        int fl = me.flags;
        if (me.pos >= 0) {
            int nb = 0, far = 0;
            for (int side = -1; side <= 1; side += 2)
                for (int step = 1; step <= 2; step++) {
                    const int j = line + side * step;
                    if (j < 0 || j >= a.L) continue;
                    const ShLine q = a.lin[j];
                    if (q.pos < 0) continue;
                    const long long dx = llabs((long long)q.wx - me.wx), dy = llabs((long long)q.wy - me.wy);
                    nb++;
                    far += (dx > dy ? dx : dy) > a.lim;
                    break;                                    // the nearest on this side
                }
            if (nb && far == nb) fl |= RC_SHORE_OUTLIER;
        }
        cur = (me.pos >= 0 && !(fl & RC_SHORE_OUTLIER)) ? me.pos : -1;
        a.ring[(size_t)line * a.T + a.c] = cur;
        flags = fl; nvs = 0; sum = 0ull;
    }
    __syncthreads();
    int P = 1;
    while (P < a.held) P <<= 1;
    int ln = 0;
    unsigned long long ls = 0;
    for (int i = threadIdx.x; i < P; i += RC_BLOCK) {
        const int v = i < a.held ? (i == a.c ? cur : a.ring[(size_t)line * a.T + i]) : -1;
        if (v >= 0) { ln++; ls += (unsigned long long)v; }
        vals[i] = v >= 0 ? v : 0x7fffffff;
    }
    if (ln) { atomicAdd(&nvs, ln); atomicAdd(&sum, ls); }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)                          // bitonic, ascending: the positions first, then the empty slots
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += RC_BLOCK) {
                const int p = i ^ j;
                if (p > i) {
                    const int x = vals[i], y = vals[p];
                    if ((x > y) == ((i & k) == 0)) { vals[i] = y; vals[p] = x; }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x != 0) return;
    const ShLine me = a.lin[line];
    const double ds = a.geom[line].ds;
    rc_shoreline r;
    memset(&r, 0, sizeof(r));
    r.flags = flags; r.k = me.k; r.pos = me.pos; r.agree = me.agree; r.wx = me.wx; r.wy = me.wy;
    r.x = (float)((double)me.wx / 256.); r.y = (float)((double)me.wy / 256.);
    if (me.pos >= 0) r.dist_m = (float)(((double)me.pos / 256.) * ds);
    const int nv = nvs;
    if (nv == 0) {
        r.flags |= RC_SHORE_NO_WINDOW;
    } else {
        r.nv = nv; r.pos_min = vals[0]; r.pos_max = vals[nv - 1];
        r.pos_q = vals[(int)(((long long)nv * a.permille + 999) / 1000) - 1];
        r.pos_mean = (float)((double)(long long)sum / (double)nv);
        r.excursion_m = (float)(((double)(r.pos_max - r.pos_min) / 256.) * ds);
    }
    a.rec[line] = r;
    if (a.rec2) a.rec2[line] = r;
    if (cur >= 0) rc_acc_add(&a.ctl->cnt[0], 1u);
    if (r.flags & RC_SHORE_DRY) rc_acc_add(&a.ctl->cnt[1], 1u);
    if (r.flags & RC_SHORE_WET) rc_acc_add(&a.ctl->cnt[2], 1u);
    if (r.flags & RC_SHORE_OUTLIER) rc_acc_add(&a.ctl->cnt[3], 1u);
    last = rc_ticket_fenced(&a.ctl->ticket2, (unsigned)a.L);  // the counts before the ticket
    if (last) {
        long long s[8] = {a.ctl->thr, a.ctl->N, (long long)rint(a.ctl->eta * 4294967296.), 0, 0, 0, 0, a.pushes};
        for (int k = 0; k < 4; k++) s[3 + k] = rc_acc_take(&a.ctl->cnt[k]);      // zero for the next push (stream order)
        rc_acc_take(&a.ctl->ticket2);
        for (int k = 0; k < 8; k++) {
            a.summary[k] = s[k];
            if (a.summary2) a.summary2[k] = s[k];
        }
    }
}

// ============================================================================ shoreline@3: the pictures
struct ShArgs3 {
    const uint16_t* plane; const ShCtl* ctl; const uint32_t* hist_in;
    uint8_t* mask; size_t mask_step;             // or null
    uint16_t* oplane; size_t oplane_step;        // or null; the step in bytes
    uint32_t* hist;                              // or null
    int w, h, wet_is_high, pixels;               // pixels: mask or plane is asked for
};

__global__ __launch_bounds__(RC_BLOCK) void k_sh_pictures(const ShArgs3 a) {
    if (a.hist && blockIdx.x == 0 && blockIdx.y == 0)
        for (int b = threadIdx.x; b < RC_SHORE_HIST; b += RC_BLOCK) a.hist[b] = a.hist_in[b];
    const RcPix3Span t = rc_pix3_span(a.w, 1);
    if (!a.pixels || t.n <= 0 || t.y0 >= a.h) return;
    const int thr = a.ctl->thr;
    const uint16_t* src = a.plane + (size_t)t.y0 * a.w + t.x0;
    uint16_t v[4] = {0, 0, 0, 0};
    if (t.n == 4) __builtin_memcpy(v, src, 8);
    else for (int k = 0; k < t.n; k++) v[k] = src[k];
    if (a.mask) {
        uint8_t m[4];
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = thr >= 0 && sh_wet(v[k], thr, a.wet_is_high) ? 255 : 0;
        uint8_t* dst = a.mask + (size_t)t.y0 * a.mask_step + t.x0;
        if (t.n == 4) __builtin_memcpy(dst, m, 4);
        else for (int k = 0; k < t.n; k++) dst[k] = m[k];
    }
    if (a.oplane) {
        uint16_t* dst = (uint16_t*)((char*)a.oplane + (size_t)t.y0 * a.oplane_step) + t.x0;
        if (t.n == 4) __builtin_memcpy(dst, v, 8);
        else for (int k = 0; k < t.n; k++) dst[k] = v[k];
    }
}

// ============================================================================ shoreline@4: the primitives
__global__ __launch_bounds__(RC_BLOCK) void k_sh_prims(const rc_shoreline* rec, int L, int pushed, uint32_t color, int thickness, int radius,
                                                       rc_draw_prim* out) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= L) return;
    rc_draw_prim p[2];
    memset(p, 0, sizeof(p));
    const rc_shoreline q = rec[i];
    if (pushed && q.pos >= 0 && !(q.flags & RC_SHORE_OUTLIER)) {
        const int px = (q.wx + 128) >> 8, py = (q.wy + 128) >> 8;
        p[0].kind = RC_DRAW_DISC; p[0].x0 = p[0].x1 = px; p[0].y0 = p[0].y1 = py; p[0].size = radius; p[0].color = color;
        for (int j = i + 1; j < L; j++) {
            const rc_shoreline n = rec[j];
            if (n.pos < 0 || (n.flags & RC_SHORE_OUTLIER)) continue;
            p[1].kind = RC_DRAW_LINE; p[1].x0 = px; p[1].y0 = py; p[1].x1 = (n.wx + 128) >> 8; p[1].y1 = (n.wy + 128) >> 8;
            p[1].size = thickness; p[1].color = color;
            break;
        }
    }
    out[2 * (size_t)i] = p[0];
    if (i + 1 < L) out[2 * (size_t)i + 1] = p[1];
}

// ============================================================================ host side
static bool sh_pos(double v) { return v > 0. && rc_finite(v); }
static bool sh_settable(int threshold, double min_sep, double max_jump) {
    return threshold >= -1 && threshold <= SH_LIVE - 2 && min_sep >= 0. && min_sep <= 1. && max_jump > 0. && max_jump <= 16384.;
}

extern "C" int rcflow_shoreline_plan(int w, int h, const rc_transect_line* lines, int n_lines, double metres_per_pixel,
                                     rc_transect_sample* table, rc_transect_geom* geom, int* total) {
    static const char* who = "rcflow_shoreline_plan";
    if (w <= 0 || h <= 0 || !lines || n_lines < 1 || n_lines > RC_SHORE_MAX_LINES || !sh_pos(metres_per_pixel)) {
        rc_set_error("%s: a picture of %d x %d, %d lines (1..%d), metres_per_pixel finite and > 0", who, w, h, n_lines, RC_SHORE_MAX_LINES);
        return RC_EINVAL;
    }
    long long S = 0;
    for (int i = 0; i < n_lines; i++) {
        if (lines[i].n < RC_SHORE_MIN_SAMPLES || lines[i].n > RC_SHORE_MAX_SAMPLES) {
            rc_set_error("%s: line %d has %d samples (%d..%d)", who, i, lines[i].n, RC_SHORE_MIN_SAMPLES, RC_SHORE_MAX_SAMPLES);
            return RC_EINVAL;
        }
        S += lines[i].n;
    }
    if (S > RC_SHORE_MAX_TOTAL) {
        rc_set_error("%s: %lld samples in all (at most %d)", who, S, RC_SHORE_MAX_TOTAL);
        return RC_EINVAL;
    }
    int first = 0;
    for (int i = 0; i < n_lines; i++) {
        if (int rc = rc_line_plan(who, w, h, lines[i], i, first, metres_per_pixel, 1., table, geom)) return rc;
        first += lines[i].n;
    }
    if (total) *total = first;
    return RC_OK;
}

void rc_state_free(RcShoreline& v) {
    rc_buf_free(v.table); rc_buf_free(v.plane); rc_buf_free(v.ring); rc_buf_free(v.lin); rc_buf_free(v.out); rc_buf_free(v.ctl);
    rc_fence_free(v.zf);
    v = RcShoreline();
}

// open and reset: the ring, the last push's outputs, the tickets, the counters and the live histogram; the push count.  The plane
// is written by every push before it is read
int rc_state_zero(RcSlot& s, RcShoreline& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.ring, &v.lin, &v.out, &v.ctl});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

// RcShoreline::table: samples [S] | geometry [L]
static const rc_transect_sample* sh_table(const RcShoreline& v) { return (const rc_transect_sample*)v.table.p; }
static const rc_transect_geom* sh_geom(const RcShoreline& v) { return (const rc_transect_geom*)(sh_table(v) + v.S); }
// RcShoreline::out: records [L] | summary 8 int64 | histogram RC_SHORE_HIST uint32
static rc_shoreline* sh_out_rec(const RcShoreline& v) { return (rc_shoreline*)v.out.p; }
static long long* sh_out_summary(const RcShoreline& v) { return (long long*)(sh_out_rec(v) + v.L); }
static uint32_t* sh_out_hist(const RcShoreline& v) { return (uint32_t*)(sh_out_summary(v) + 8); }

extern "C" int rcflow_shoreline_open(rc_ctx* ctx, int stream, int w, int h, const rc_transect_line* lines, int n_lines,
                                     const rc_shoreline_params* prm) {
    static const char* who = "rcflow_shoreline_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad picture size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    const int T = prm->window;
    if (prm->source < RC_SHORE_RMB || prm->source > RC_SHORE_PLANE || prm->radius < 0 || prm->radius > RC_SHORE_MAX_RADIUS ||
        (prm->wet_is_high != 0 && prm->wet_is_high != 1) || T < 2 || T > RC_SHORE_MAX_WINDOW || prm->permille < 1 || prm->permille > 999 ||
        prm->flags || !sh_pos(prm->metres_per_pixel) || !sh_settable(prm->threshold, prm->min_sep, prm->max_jump)) {
        rc_set_error("%s: source RC_SHORE_RMB, RC_SHORE_GRAY or RC_SHORE_PLANE, radius 0..%d, wet_is_high 0 or 1, threshold -1..%d, window 2..%d, "
                     "permille 1..999, flags 0, min_sep 0..1, max_jump > 0 and <= 16384, metres_per_pixel finite and > 0", who,
                     RC_SHORE_MAX_RADIUS, SH_LIVE - 2, RC_SHORE_MAX_WINDOW);
        return RC_EINVAL;
    }
    int S = 0;
    int rc = rcflow_shoreline_plan(w, h, lines, n_lines, prm->metres_per_pixel, nullptr, nullptr, &S);
    if (rc) {                                                 // the text names the entry point that was called
        const std::string t = rcflow_last_error();
        const size_t at = t.find(": ");
        rc_set_error("%s%s", who, at == std::string::npos ? "" : t.c_str() + at);
        return rc;
    }
    rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    if ((long long)w * h > RC_SHORE_MAX_PIXELS) {
        rc_set_error("%s: %d x %d is more than RC_SHORE_MAX_PIXELS pixels", who, w, h);
        return RC_ESIZE;
    }
    const unsigned long long state = 4ull * T * n_lines;
    if (state > RC_SHORE_MAX_STATE_BYTES) {
        rc_set_error("%s: %d positions of %d lines are %llu bytes of ring, more than RC_SHORE_MAX_STATE_BYTES", who, T, n_lines, state);
        return RC_ESIZE;
    }
    RcShoreline n;
    n.w = w; n.h = h; n.prm = *prm; n.prm.pad = 0; n.L = n_lines; n.S = S;
    std::vector<unsigned char> host((size_t)S * sizeof(rc_transect_sample) + (size_t)n_lines * sizeof(rc_transect_geom));
    (void)rcflow_shoreline_plan(w, h, lines, n_lines, prm->metres_per_pixel, (rc_transect_sample*)host.data(),
                                (rc_transect_geom*)(host.data() + (size_t)S * sizeof(rc_transect_sample)), nullptr);
    RC_HIP(hipSetDevice(ctx->device));
    rc = rc_buf_ensure(n.table, host.size());
    if (!rc) rc = rc_buf_ensure(n.plane, (size_t)w * h * 2);
    if (!rc) rc = rc_buf_ensure(n.ring, (size_t)state);
    if (!rc) rc = rc_buf_ensure(n.lin, (size_t)n_lines * sizeof(ShLine));
    if (!rc) rc = rc_buf_ensure(n.out, (size_t)n_lines * sizeof(rc_shoreline) + 64 + 4 * RC_SHORE_HIST);
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(ShCtl));
    if (!rc && hipMemcpy(n.table.p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        rc_set_error("%s: the upload of the table failed", who);
        rc = RC_EHIP;
    }
    return rc_state_install(*s, s->sh, n, rc);
}

template <int R>
static void sh_launch0(dim3 grid, hipStream_t st, const ShArgs0& a) {
    hipLaunchKernelGGL(k_sh_pixels<R>, grid, dim3(RC_BLOCK), 0, st, a);
}

extern "C" int rcflow_shoreline_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_image, size_t step, int channels, const uint8_t* d_roi,
                                         size_t roi_step, rc_shoreline* d_records, uint8_t* d_mask, size_t mask_step, uint16_t* d_plane,
                                         size_t plane_step, uint32_t* d_hist, long long* d_summary) {
    static const char* who = "rcflow_shoreline_push_dev";
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, who, s, vp)) return rc;
    RcShoreline& v = *vp;
    const int w = v.w, h = v.h, L = v.L, T = v.prm.window, bpp = v.prm.source == RC_SHORE_PLANE ? 1 : 3;
    if (channels != bpp) {
        rc_set_error("%s: the session's source takes a picture of %d channel%s, not %d", who, bpp, bpp == 1 ? "" : "s", channels);
        return RC_EINVAL;
    }
    RcArgsN<8> ar(who, w, h);
    ar.image("d_image", d_image, step, bpp, 1, RC_ARG_IN);
    ar.image("d_roi", d_roi, roi_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.array("d_records", d_records, (size_t)L * sizeof(rc_shoreline), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_plane", d_plane, plane_step, 2, 2, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_hist", d_hist, 4 * RC_SHORE_HIST, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const long long p = v.pushes, pushes = p + 1;
    const double px = (double)w * h;
    {
        ShArgs0 a;
        a.img = d_image; a.step = step; a.roi = d_roi; a.roi_step = roi_step;
        a.plane = (uint16_t*)v.plane.p; a.ctl = (ShCtl*)v.ctl.p; a.hist_out = sh_out_hist(v);
        a.w = w; a.h = h; a.source = v.prm.source; a.fixed = v.prm.threshold;
        const int tx = (w + SH_TW - 1) / SH_TW, ty = (h + SH_TH - 1) / SH_TH;
        a.tiles = (int)(((long long)tx * ty + SH_MAX_BLOCKS - 1) / SH_MAX_BLOCKS);
        const dim3 grid(tx, (ty + a.tiles - 1) / a.tiles);
        a.nblocks = grid.x * grid.y;
        // the picture in, the plane out, the region of interest in
        RcProfScope ps(ctx, s->cur, RC_K_SHORELINE, 0, px * (bpp + 2. + (d_roi ? 1. : 0.)));
        switch (v.prm.radius) {
            case 0: sh_launch0<0>(grid, s->cur, a); break;
            case 1: sh_launch0<1>(grid, s->cur, a); break;
            case 2: sh_launch0<2>(grid, s->cur, a); break;
            case 3: sh_launch0<3>(grid, s->cur, a); break;
            case 4: sh_launch0<4>(grid, s->cur, a); break;
            case 5: sh_launch0<5>(grid, s->cur, a); break;
            case 6: sh_launch0<6>(grid, s->cur, a); break;
            default: sh_launch0<7>(grid, s->cur, a); break;
        }
    }
    {
        ShArgs1 a;
        a.table = sh_table(v); a.geom = sh_geom(v); a.plane = (const uint16_t*)v.plane.p; a.ctl = (const ShCtl*)v.ctl.p;
        a.lin = (ShLine*)v.lin.p;
        a.w = w; a.h = h; a.L = L; a.wet_is_high = v.prm.wet_is_high; a.min_sep = v.prm.min_sep;
        // a sample's record and its four pixels in, a line's hand-over out
        RcProfScope ps(ctx, s->cur, RC_K_SHORELINE, 1, 24. * v.S + (double)L * (sizeof(rc_transect_geom) + sizeof(ShLine)));
        hipLaunchKernelGGL(k_sh_lines, dim3((L + SH_WAVES - 1) / SH_WAVES), dim3(RC_BLOCK), 0, s->cur, a);
    }
    {
        ShArgs2 a;
        a.geom = sh_geom(v); a.lin = (const ShLine*)v.lin.p; a.ring = (int*)v.ring.p;
        a.rec = sh_out_rec(v); a.summary = sh_out_summary(v); a.rec2 = d_records; a.summary2 = d_summary;
        a.ctl = (ShCtl*)v.ctl.p;
        a.L = L; a.T = T; a.c = (int)(p % T); a.held = (int)(pushes < T ? pushes : T); a.permille = v.prm.permille;
        a.lim = (long long)rint(v.prm.max_jump * 256.);
        a.pushes = pushes;
        RcProfScope ps(ctx, s->cur, RC_K_SHORELINE, 2, (double)L * (4. * a.held + 5. * sizeof(ShLine) + sizeof(rc_shoreline) * (d_records ? 2. : 1.)));
        hipLaunchKernelGGL(k_sh_records, dim3(L), dim3(RC_BLOCK), 0, s->cur, a);
    }
    if (d_mask || d_plane || d_hist) {
        ShArgs3 a;
        a.plane = (const uint16_t*)v.plane.p; a.ctl = (const ShCtl*)v.ctl.p; a.hist_in = sh_out_hist(v);
        a.mask = d_mask; a.mask_step = mask_step; a.oplane = d_plane; a.oplane_step = plane_step; a.hist = d_hist;
        a.w = w; a.h = h; a.wet_is_high = v.prm.wet_is_high; a.pixels = d_mask || d_plane;
        RcProfScope ps(ctx, s->cur, RC_K_SHORELINE, 3, a.pixels ? px * (2. + (d_mask ? 1. : 0.) + (d_plane ? 2. : 0.)) : 8. * RC_SHORE_HIST);
        hipLaunchKernelGGL(k_sh_pictures, a.pixels ? rc_pix3_grid(w, h, 1) : dim3(1, 1), dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_shoreline_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, rc_draw_prim* d_prims) {
    static const char* who = "rcflow_shoreline_prims_dev";
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, who, s, vp)) return rc;
    if (rc_prims_check(who, d_prims, thickness, disc_radius)) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    RcProfScope ps(ctx, s->cur, RC_K_SHORELINE, 4, (double)vp->L * (sizeof(rc_shoreline) + 2. * sizeof(rc_draw_prim)));
    hipLaunchKernelGGL(k_sh_prims, dim3((vp->L + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, sh_out_rec(*vp), vp->L,
                       vp->pushes > 0 ? 1 : 0, color, thickness, disc_radius, d_prims);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_shoreline_read(rc_ctx* ctx, int stream, rc_shoreline* records, long long summary[8]) {
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, "rcflow_shoreline_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    if (records) RC_HIP(hipMemcpyAsync(records, sh_out_rec(*vp), (size_t)vp->L * sizeof(rc_shoreline), hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, sh_out_summary(*vp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_shoreline_ring_read(rc_ctx* ctx, int stream, int* ring) {
    static const char* who = "rcflow_shoreline_ring_read";
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, who, s, vp)) return rc;
    if (!ring) { rc_set_error("%s: no buffer", who); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const int T = vp->prm.window, L = vp->L;
    std::vector<int> raw((size_t)L * T);
    RC_HIP(hipMemcpyAsync(raw.data(), vp->ring.p, raw.size() * 4, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    const int held = (int)(vp->pushes < T ? vp->pushes : T), oldest = vp->pushes >= T ? (int)(vp->pushes % T) : 0;
    for (int i = 0; i < L; i++)
        for (int r = 0; r < T; r++) ring[(size_t)i * T + r] = r < held ? raw[(size_t)i * T + (oldest + r) % T] : -1;
    return RC_OK;
}

extern "C" int rcflow_shoreline_table_read(rc_ctx* ctx, int stream, rc_transect_sample* table, rc_transect_geom* geom) {
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, "rcflow_shoreline_table_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    if (table) RC_HIP(hipMemcpyAsync(table, sh_table(*vp), (size_t)vp->S * sizeof(rc_transect_sample), hipMemcpyDeviceToHost, s->cur));
    if (geom) RC_HIP(hipMemcpyAsync(geom, sh_geom(*vp), (size_t)vp->L * sizeof(rc_transect_geom), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_shoreline_set(rc_ctx* ctx, int stream, int threshold, double min_sep, double max_jump) {
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, "rcflow_shoreline_set", s, vp)) return rc;
    if (!sh_settable(threshold, min_sep, max_jump)) {
        rc_set_error("rcflow_shoreline_set: threshold -1..%d, min_sep 0..1, max_jump > 0 and <= 16384", SH_LIVE - 2);
        return RC_EINVAL;
    }
    vp->prm.threshold = threshold; vp->prm.min_sep = min_sep; vp->prm.max_jump = max_jump;
    return RC_OK;
}

extern "C" int rcflow_shoreline_info(rc_ctx* ctx, int stream, rc_shoreline_info* info) {
    RcSlot* s; RcShoreline* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sh, "rcflow_shoreline_info", s, vp)) return rc;
    const RcShoreline& v = *vp;
    if (!info) { rc_set_error("rcflow_shoreline_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->lines = v.L; info->samples = v.S;
    info->launches_per_push = RC_SHORE_LAUNCHES;
    info->held = (int)(v.pushes < v.prm.window ? v.pushes : v.prm.window);
    info->pushes = v.pushes;
    info->device_bytes = v.table.bytes + v.plane.bytes + v.ring.bytes + v.lin.bytes + v.out.bytes + v.ctl.bytes;
    return RC_OK;
}

extern "C" int rcflow_shoreline_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::sh, "rcflow_shoreline_reset"); }
extern "C" int rcflow_shoreline_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::sh); }
