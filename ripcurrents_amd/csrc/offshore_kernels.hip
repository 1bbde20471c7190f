// offshore_kernels.hip -- the offshore frame: the exact distance of every pixel to the shore with the shore point it is nearest to,
// and a flow field projected on the local shore normal.
//
// include/rcflow.h ("offshore frame") is the specification; tests/_offshore_ref.py states it in numpy and the kernels are held to
// that bit for bit: every decision is an integer, the only float arithmetic is (float)v / 64.0f, which is exact, and the records'
// means in double.  Nothing synchronises.  The map is an exact Euclidean distance transform in two passes, three launches:
//   offshore@0  a thread owns a column and sweeps it down and up: per class (dry, wet) and pixel the row of the nearest pixel of
//               the class in the pixel's own column, the upper row on a tie, -1 when the column has none; int16 planes
//   offshore@1  a thread owns a pixel of a row: the least key ((x - x')^2 + (y - g)^2, g * w + x') over the columns x', g the entry
//               of column x' for the OTHER class, by a walk outwards from x that stops once (x - x')^2 exceeds the best so far.  The
//               upper row is the smaller raster index, so the column pass loses nothing the tie rule needs, and a candidate at
//               (x - x')^2 equal to the best can still win on the index, so the walk goes on while it is not larger.  The two
//               planes of the state, every output and the six sums, folded in the wave and the block
//   offshore@2  one wave closes the summary and leaves the accumulators zero
// A push is two launches:
//   offshore@3  a wave owns 64 pixels of a row: classes, cross and along, every output; the table's adds folded over the runs of
//               lanes that share a cell (rc_run of rc_reduce.h), one atomic per run and word
//   offshore@4  one block takes the table, closes a record per station and the summary, and leaves the accumulators zero
// and the band is one launch, offshore@5.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define OF_COLS 64                     // threads of a block of offshore@0: a wave, so that 1920 columns are 30 blocks on 30 CUs
#define OF_ROWS (RC_BLOCK / 64)        // rows of a block of offshore@3
#define OF_NAN 0x7fc00000u
static_assert(RC_BLOCK == 256 && RC_OFFSHORE_MAX_STATIONS <= RC_BLOCK, "offshore@4 is one block with a thread per station");
static_assert(sizeof(rc_offshore_station) == 48 && sizeof(rc_offshore_params) == 48, "the records of include/rcflow.h have the sizes the mirrors give them");
static_assert(RC_OFFSHORE_SUMS == 4 && RC_OFFSHORE_SUMMARY == 8, "the words of a cell and of a summary");
static_assert(2ll * (RC_OFFSHORE_MAX_SIDE - 1) * (RC_OFFSHORE_MAX_SIDE - 1) < 0x7fffffffll, "d2 is int32 and below RC_OFFSHORE_FAR");
static_assert(2ll * 32000 * RC_OFFSHORE_MAX_DIST < 0x7fffffffll, "C and A are int32");

struct OfMapArgs {
    const uint8_t* wet; size_t wet_step;
    short* g[2];                                 // [h][w] each: dry, wet
    int* d2; int* near;                          // the state's planes
    int* dist2; size_t dist2_step;               // each output or null; the steps in bytes
    int* nearo; size_t near_step;
    int* sdist; size_t sdist_step;
    uint8_t* pic; size_t pic_step;
    const uint8_t* jet;
    long long* acc;                              // 8 words
    long long* summary; long long* summary2;     // the state's copy; the caller's, or null
    int w, h, max_dist;
    long long maps;
};

struct OfPushArgs {
    const float* flow; size_t flow_step;
    const int* d2; const int* near;
    float* ca; size_t ca_step;                   // each output or null
    uint8_t* cls; size_t cls_step;
    uint8_t* mask; size_t mask_step;
    uint8_t* pic; size_t pic_step;
    long long* tab;                              // [stations][bins][RC_OFFSHORE_SUMS], zero between pushes
    long long* beyond;                           // [stations]
    long long* cnt;                              // 8: the five classes, the mask pixels
    long long* summary; long long* table; rc_offshore_station* recs;          // the state's copy
    long long* summary2; long long* table2; rc_offshore_station* recs2;       // the caller's, or null
    int w, h, min_d2, max_d2, stations, bins, bin_width, min_count, rip_bins, cmin_q, by_x;
    long long pushes;
};

struct OfBandArgs {
    const int* d2;
    uint8_t* band; size_t band_step;
    int w, h, lo_q, hi_q;
};

// floor(sqrt(4096 d2)), exactly: the double's square root is within one of it
__device__ __forceinline__ int of_r(int d2) {
    const long long v = 4096ll * d2;
    long long r = (long long)sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return (int)r;
}
// floor((2 a + b) / (2 b)), b > 0
__device__ __forceinline__ long long of_rdiv(long long a, long long b) { return rc_floor_div(2 * a + b, 2 * b); }

// ============================================================================ offshore@0: the column pass
// of two rows of a class, one at or above y and one at or below (-1: none), the nearer, the upper on a tie
__device__ __forceinline__ int of_nearer(int up, int dn, int y) { return up < 0 ? dn : dn < 0 ? up : (y - up <= dn - y ? up : dn); }

__global__ __launch_bounds__(OF_COLS) void k_of_cols(const OfMapArgs a) {
    const int x = blockIdx.x * OF_COLS + threadIdx.x;
    if (x >= a.w) return;
    const int w = a.w, h = a.h;
    // the mask and the two planes never share a byte: said so, the loads of the rows ahead do not wait for the stores behind
    const uint8_t* __restrict__ wet = a.wet + x;
    short* __restrict__ g0 = a.g[0] + x;
    short* __restrict__ g1 = a.g[1] + x;
    int last[2] = {-1, -1};
#pragma unroll 8
    for (int y = 0; y < h; y++) {
        const bool c = wet[(size_t)y * a.wet_step] != 0;
        last[c] = y;
        g0[(size_t)y * w] = (short)last[0];
        g1[(size_t)y * w] = (short)last[1];
    }
    int next[2] = {-1, -1};
#pragma unroll 8
    for (int y = h - 1; y >= 0; y--) {
        const bool c = wet[(size_t)y * a.wet_step] != 0;
        next[c] = y;
        const size_t i = (size_t)y * w;
        g0[i] = (short)of_nearer(g0[i], next[0], y);
        g1[i] = (short)of_nearer(g1[i], next[1], y);
    }
}

// ============================================================================ offshore@1: the row pass, the outputs, the sums
__global__ __launch_bounds__(RC_BLOCK) void k_of_rows(const OfMapArgs a) {
    __shared__ uint8_t jet[768];
    __shared__ long long red[RC_BLOCK / 64][6];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = a.w, y = blockIdx.y, x = blockIdx.x * RC_BLOCK + tid;     // y < h by the grid's size
    if (a.pic) {
        rc_stage_jet(jet, a.jet);
        __syncthreads();
    }
    long long s[6] = {0, 0, 0, 0, 0, 0};                      // wet | dry | wet and not FAR | largest d2 of those | their sum | the dry pixels' sum
    if (x < w) {
        const bool c = a.wet[(size_t)y * a.wet_step + x] != 0;
        const short* plane = a.g[c ? 0 : 1] + (size_t)y * w;  // the other class
        unsigned long long best = ((unsigned long long)RC_OFFSHORE_FAR << 32) | 0xffffffffull;
        const auto look = [&](int xc, int dx2) {
            const int g = plane[xc];
            if (g < 0) return;
            const int dy = y - g;
            const unsigned long long k = ((unsigned long long)(unsigned)(dx2 + dy * dy) << 32) | (unsigned)(g * w + xc);
            best = k < best ? k : best;
        };
        look(x, 0);
        const int dmax = max(x, w - 1 - x);
        for (int d = 1; d <= dmax && (unsigned long long)(d * d) <= (best >> 32); d++) {
            if (x - d >= 0) look(x - d, d * d);
            if (x + d < w) look(x + d, d * d);
        }
        const int d2 = (int)(best >> 32);
        const bool far = d2 == RC_OFFSHORE_FAR;
        const int near = far ? -1 : (int)(unsigned)best;
        const int r = far ? RC_OFFSHORE_FAR : of_r(d2);
        const size_t i = (size_t)y * w + x;
        a.d2[i] = c ? d2 : -d2;
        a.near[i] = near;
        if (a.dist2) *(int*)((char*)a.dist2 + (size_t)y * a.dist2_step + 4 * (size_t)x) = c ? d2 : -d2;
        if (a.nearo) *(int*)((char*)a.nearo + (size_t)y * a.near_step + 4 * (size_t)x) = near;
        if (a.sdist) *(int*)((char*)a.sdist + (size_t)y * a.sdist_step + 4 * (size_t)x) = c ? r : -r;
        if (a.pic) {
            uint8_t* d = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x;
            if (far) { d[0] = 0; d[1] = 0; d[2] = 0; }
            else if (!c) { d[0] = 64; d[1] = 64; d[2] = 64; }
            else {
                const uint8_t* e = jet + 3 * (min(r / 64, a.max_dist) * 255 / a.max_dist);
                d[0] = e[0]; d[1] = e[1]; d[2] = e[2];
            }
        }
        s[0] = c; s[1] = !c;
        if (!far) {
            if (c) { s[2] = 1; s[3] = d2; s[4] = d2; }
            else s[5] = d2;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const long long t = k == 3 ? (long long)rc_wave_max_all((int)s[3]) : rc_wave_sum_lane0(s[k]);
        if (lane == 0) red[wv][k] = t;
    }
    __syncthreads();
    if (tid < 6) {
        long long t = red[0][tid];
        for (int k = 1; k < RC_BLOCK / 64; k++) t = tid == 3 ? max(t, red[k][tid]) : t + red[k][tid];
        if (!t) return;
        if (tid == 3) __hip_atomic_fetch_max(a.acc + 3, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else rc_acc_add(a.acc + tid, t);
    }
}

// ============================================================================ offshore@2: the map's summary
__global__ __launch_bounds__(64) void k_of_mapsum(const OfMapArgs a) {
    const int tid = threadIdx.x;
    if (tid >= RC_OFFSHORE_SUMMARY) return;
    const long long v = tid < 6 ? rc_acc_take(a.acc + tid) : tid == 7 ? a.maps : 0;
    a.summary[tid] = v;
    if (a.summary2) a.summary2[tid] = v;
}

// ============================================================================ offshore@3: classes, components, outputs, the table
__global__ __launch_bounds__(RC_BLOCK) void k_of_push(const OfPushArgs a) {
    __shared__ int cnt[8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int w = a.w, h = a.h;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * OF_ROWS + wv;
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    int cell = -1, far_station = -1, cls = -1;
    bool in_mask = false;                                     // also of a pixel beyond the last bin
    long long v[RC_OFFSHORE_SUMS] = {0, 0, 0, 0};
    if (x < w && y < h) {                                     // uniform in y over the wave
        const size_t i = (size_t)y * w + x;
        const int sd2 = a.d2[i];
        int cross = 0, along = 0;
        if (sd2 <= 0) cls = RC_OFFSHORE_C_DRY;                // a dry pixel's d2 is at least 1, negated
        else if (sd2 > a.max_d2) cls = RC_OFFSHORE_C_FAR;     // FAR is above every max_dist^2
        else if (sd2 < a.min_d2) cls = RC_OFFSHORE_C_NEAR;
        else {
            const float2 f = *(const float2*)((const char*)a.flow + (size_t)y * a.flow_step + 8 * (size_t)x);
            if (!(fabsf(f.x) < 500.0f && fabsf(f.y) < 500.0f)) cls = RC_OFFSHORE_C_BAD;       // NaN and the infinities fail the comparison
            else {
                cls = RC_OFFSHORE_C_OK;
                const int qx = (int)rintf(f.x * 64.0f), qy = (int)rintf(f.y * 64.0f);
                const int near = a.near[i];
                const int ny = y - near / w, nx = x - near % w;
                const int C = qx * nx + qy * ny, A = -qx * ny + qy * nx;
                const int r = of_r(sd2);
                cross = (int)of_rdiv(64ll * C, r);
                along = (int)of_rdiv(64ll * A, r);
                in_mask = cross >= a.cmin_q;
                const int bin = r / (64 * a.bin_width);
                const int st = a.by_x ? x * a.stations / w : y * a.stations / h;
                if (bin < a.bins) {
                    cell = st * a.bins + bin;
                    v[0] = 1; v[1] = cross; v[2] = along; v[3] = in_mask;
                } else {
                    far_station = st;
                }
            }
        }
        const bool ok = cls == RC_OFFSHORE_C_OK;
        if (a.ca) {
            const float2 o = ok ? make_float2((float)cross / 64.0f, (float)along / 64.0f) : make_float2(__uint_as_float(OF_NAN), __uint_as_float(OF_NAN));
            *(float2*)((char*)a.ca + (size_t)y * a.ca_step + 8 * (size_t)x) = o;
        }
        if (a.cls) a.cls[(size_t)y * a.cls_step + x] = (uint8_t)cls;
        if (a.mask) a.mask[(size_t)y * a.mask_step + x] = in_mask ? 255 : 0;
        if (a.pic) {
            unsigned c3;                                      // B | G << 8 | R << 16
            if (ok) {
                const int S = max(4 * a.cmin_q, 1), c = min(max(cross, -S), S);
                const unsigned m = 255u - (unsigned)((long long)abs(c) * 255 / S);
                c3 = c >= 0 ? (m | (m << 8) | 0xff0000u) : (0xffu | (m << 8) | (m << 16));
            } else {
                c3 = cls == RC_OFFSHORE_C_DRY ? 0x404040u : cls == RC_OFFSHORE_C_FAR ? 0u : cls == RC_OFFSHORE_C_NEAR ? 0x808080u : 0xff00ffu;
            }
            uint8_t* d = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x;
            d[0] = (uint8_t)c3; d[1] = (uint8_t)(c3 >> 8); d[2] = (uint8_t)(c3 >> 16);
        }
    }
    // the table: one atomic per run of lanes with one cell and per word
    if (__any(cell >= 0)) {
        bool head;
        const int end = rc_run(cell, lane, head);
#pragma unroll
        for (int k = 0; k < RC_OFFSHORE_SUMS; k++) {
            if (!__any(v[k] != 0)) continue;
            const long long s = rc_run_sum(v[k], lane, end);
            if (head && cell >= 0 && s) rc_acc_add(a.tab + (size_t)RC_OFFSHORE_SUMS * cell + k, s);
        }
    }
    if (__any(far_station >= 0)) {
        bool head;
        const int end = rc_run(far_station, lane, head);
        if (head && far_station >= 0) rc_acc_add(a.beyond + far_station, (long long)(end - lane + 1));
    }
    // the counts: by the wave's ballots into the block's, then one atomic per word
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int n = __popcll(__ballot(cls == k));
        if (lane == 0 && n) __hip_atomic_fetch_add(&cnt[k], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    {
        const int n = __popcll(__ballot(in_mask));
        if (lane == 0 && n) __hip_atomic_fetch_add(&cnt[5], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (tid < 6 && cnt[tid]) rc_acc_add(a.cnt + tid, (long long)cnt[tid]);
}

// ============================================================================ offshore@4: the table out, records, summary
// One block behind offshore@3 on the stream: it takes the accumulators, which leaves every one zero for the next push.  The table
// goes through the state's copy: what the block's threads stored there before the barrier, the station's thread reads after it
__global__ __launch_bounds__(RC_BLOCK) void k_of_close(const OfPushArgs a) {
    __shared__ int rips[RC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nt = a.stations * a.bins * RC_OFFSHORE_SUMS;
    for (int i = tid; i < nt; i += RC_BLOCK) {
        const long long t = rc_acc_take(a.tab + i);
        a.table[i] = t;
        if (a.table2) a.table2[i] = t;
    }
    __syncthreads();
    int rip = 0;
    if (tid < a.stations) {
        const long long* t = a.table + (size_t)tid * a.bins * RC_OFFSHORE_SUMS;
        rc_offshore_station rec;
        memset(&rec, 0, sizeof(rec));
        rec.beyond = (int)rc_acc_take(a.beyond + tid);
        const auto passes = [&](int b) { return t[4 * b] >= a.min_count && t[4 * b + 1] >= (long long)a.cmin_q * t[4 * b]; };
        int first = 0;
        while (first < a.bins && t[4 * first] < a.min_count) first++;
        if (first == a.bins) {
            rec.flags = RC_OFFSHORE_EMPTY;
        } else {
            int b = first;
            while (b < a.bins && passes(b)) b++;
            rec.first = first;
            rec.reach_end = b == first ? 0 : b;
            rec.peak_bin = -1;
            for (int k = first; k < a.bins; k++) {
                if (!passes(k)) continue;
                const int m = (int)of_rdiv(t[4 * k + 1], t[4 * k]);
                if (rec.peak_bin < 0 || m > rec.peak_cross) { rec.peak_bin = k; rec.peak_cross = m; }
            }
            long long n = 0, sc = 0, sa = 0;
            for (int k = first; k < rec.reach_end; k++) { n += t[4 * k]; sc += t[4 * k + 1]; sa += t[4 * k + 2]; }
            rec.count = (int)n;
            if (n) {
                rec.mean_cross = (float)(((double)sc / 64.0) / (double)n);
                rec.mean_along = (float)(((double)sa / 64.0) / (double)n);
            }
            if (rec.reach_end - first >= a.rip_bins) { rec.flags |= RC_OFFSHORE_RIP; rip = 1; }
        }
        a.recs[tid] = rec;
        if (a.recs2) a.recs2[tid] = rec;
    }
    rip = rc_wave_sum_lane0(rip);
    if (lane == 0) rips[wv] = rip;
    __syncthreads();
    if (tid >= RC_OFFSHORE_SUMMARY) return;
    long long v = 0;
    if (tid < 6) v = rc_acc_take(a.cnt + tid);
    else if (tid == 6) v = rips[0] + rips[1] + rips[2] + rips[3];
    else v = a.pushes;
    a.summary[tid] = v;
    if (a.summary2) a.summary2[tid] = v;
}

// ============================================================================ offshore@5: the band
__global__ __launch_bounds__(RC_BLOCK) void k_of_band(const OfBandArgs a) {
    const int x = blockIdx.x * RC_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const int sd2 = a.d2[(size_t)y * a.w + x];
    bool in = false;
    if (sd2 > 0 && sd2 != RC_OFFSHORE_FAR) {
        const int r = of_r(sd2);
        in = r >= a.lo_q && r < a.hi_q;
    }
    a.band[(size_t)y * a.band_step + x] = in ? 255 : 0;
}

// ============================================================================ host side
void rc_state_free(RcOffshore& v) {
    rc_buf_free(v.col); rc_buf_free(v.d2); rc_buf_free(v.near); rc_buf_free(v.jet); rc_buf_free(v.acc); rc_buf_free(v.out);
    rc_fence_free(v.zf);
    v = RcOffshore();
}

// open and reset: no map is held; the accumulators, the last calls' outputs and the counts
int rc_state_zero(RcSlot& s, RcOffshore& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.acc, &v.out});
    if (rc) return rc;
    v.have_map = false;
    v.maps = 0; v.pushes = 0;
    return RC_OK;
}

static size_t of_cells(const RcOffshore& v) { return (size_t)v.prm.stations * v.prm.bins; }
// RcOffshore::acc: 8 of a map | the table | beyond [stations] | 8 of a push
static long long* of_acc_tab(const RcOffshore& v) { return (long long*)v.acc.p + 8; }
static long long* of_acc_beyond(const RcOffshore& v) { return of_acc_tab(v) + of_cells(v) * RC_OFFSHORE_SUMS; }
static long long* of_acc_cnt(const RcOffshore& v) { return of_acc_beyond(v) + v.prm.stations; }
// RcOffshore::out: map summary 8 | push summary 8 | the table | records [stations]
static long long* of_out_map(const RcOffshore& v) { return (long long*)v.out.p; }
static long long* of_out_push(const RcOffshore& v) { return (long long*)v.out.p + RC_OFFSHORE_SUMMARY; }
static long long* of_out_table(const RcOffshore& v) { return (long long*)v.out.p + 2 * RC_OFFSHORE_SUMMARY; }
static rc_offshore_station* of_out_recs(const RcOffshore& v) { return (rc_offshore_station*)(of_out_table(v) + of_cells(v) * RC_OFFSHORE_SUMS); }

static const char* of_prm_text = "min_dist 0..max_dist, max_dist 1..4095, stations, bins and bin_width 1..256, min_count >= 1, rip_bins 1..bins, cross_min "
                                 "finite and 0..400, flags RC_OFFSHORE_STATION_X or RC_OFFSHORE_STATION_Y (exactly one), the pad words zero";
static bool of_prm_ok(const rc_offshore_params& p) {
    return p.max_dist >= 1 && p.max_dist <= RC_OFFSHORE_MAX_DIST && p.min_dist >= 0 && p.min_dist <= p.max_dist && p.stations >= 1 &&
           p.stations <= RC_OFFSHORE_MAX_STATIONS && p.bins >= 1 && p.bins <= RC_OFFSHORE_MAX_BINS && p.bin_width >= 1 &&
           p.bin_width <= RC_OFFSHORE_MAX_BIN_WIDTH && p.min_count >= 1 && p.rip_bins >= 1 && p.rip_bins <= p.bins && p.cross_min >= 0.f &&
           p.cross_min <= 400.f && (p.flags == RC_OFFSHORE_STATION_X || p.flags == RC_OFFSHORE_STATION_Y) && !p.pad[0] && !p.pad[1] && !p.pad[2];
}
static int of_ceil64(float v) { return (int)ceil((double)v * 64.0); }

extern "C" int rcflow_offshore_open(rc_ctx* ctx, int stream, int w, int h, const rc_offshore_params* prm) {
    static const char* who = "rcflow_offshore_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad picture size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (!of_prm_ok(*prm)) { rc_set_error("%s: %s", who, of_prm_text); return RC_EINVAL; }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    if (w > RC_OFFSHORE_MAX_SIDE || h > RC_OFFSHORE_MAX_SIDE) {
        rc_set_error("%s: %d x %d is beyond %d a side", who, w, h, RC_OFFSHORE_MAX_SIDE);
        return RC_ESIZE;
    }
    RcOffshore n;
    n.w = w; n.h = h; n.prm = *prm;
    RC_HIP(hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, nc = of_cells(n);
    rc = rc_buf_ensure(n.col, px * 2 * sizeof(short));
    if (!rc) rc = rc_buf_ensure(n.d2, px * 4);
    if (!rc) rc = rc_buf_ensure(n.near, px * 4);
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    if (!rc) rc = rc_buf_ensure(n.acc, (8 + nc * RC_OFFSHORE_SUMS + prm->stations + 8) * 8);
    if (!rc) rc = rc_buf_ensure(n.out, (2 * RC_OFFSHORE_SUMMARY + nc * RC_OFFSHORE_SUMS) * 8 + prm->stations * sizeof(rc_offshore_station));
    return rc_state_install(*s, s->off, n, rc);
}

extern "C" int rcflow_offshore_map_dev(rc_ctx* ctx, int stream, const uint8_t* d_wet, size_t wet_step, int* d_dist2, size_t dist2_step, int* d_near,
                                       size_t near_step, int* d_sdist, size_t sdist_step, uint8_t* d_picture, size_t picture_step,
                                       long long* d_summary) {
    static const char* who = "rcflow_offshore_map_dev";
    RcSlot* s; RcOffshore* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::off, who, s, vp)) return rc;
    RcOffshore& v = *vp;
    const int w = v.w, h = v.h;
    RcArgs ar(who, w, h);
    ar.image("d_wet", d_wet, wet_step, 1, 1, RC_ARG_IN);
    ar.image("d_dist2", d_dist2, dist2_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_near", d_near, near_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_sdist", d_sdist, sdist_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, RC_OFFSHORE_SUMMARY * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    OfMapArgs a;
    memset(&a, 0, sizeof(a));
    a.wet = d_wet; a.wet_step = wet_step;
    a.g[0] = (short*)v.col.p; a.g[1] = (short*)v.col.p + (size_t)w * h;
    a.d2 = (int*)v.d2.p; a.near = (int*)v.near.p;
    a.dist2 = d_dist2; a.dist2_step = dist2_step; a.nearo = d_near; a.near_step = near_step; a.sdist = d_sdist; a.sdist_step = sdist_step;
    a.pic = d_picture; a.pic_step = picture_step; a.jet = (const uint8_t*)v.jet.p;
    a.acc = (long long*)v.acc.p; a.summary = of_out_map(v); a.summary2 = d_summary;
    a.w = w; a.h = h; a.max_dist = v.prm.max_dist; a.maps = v.maps + 1;
    const double px = (double)w * h;
    {   // the mask in twice, the two planes out and in and out again
        RcProfScope ps(ctx, s->cur, RC_K_OFFSHORE, 0, px * (2. + 3. * 4.));
        hipLaunchKernelGGL(k_of_cols, dim3((w + OF_COLS - 1) / OF_COLS), dim3(OF_COLS), 0, s->cur, a);
    }
    {   // the mask and a row of one plane in (the walk's reads are the cache's), the state's planes and the outputs asked for out
        RcProfScope ps(ctx, s->cur, RC_K_OFFSHORE, 1, px * (1. + 2. + 8. + (d_dist2 ? 4. : 0.) + (d_near ? 4. : 0.) + (d_sdist ? 4. : 0.) + (d_picture ? 3. : 0.)));
        hipLaunchKernelGGL(k_of_rows, dim3((w + RC_BLOCK - 1) / RC_BLOCK, h), dim3(RC_BLOCK), 0, s->cur, a);
    }
    {
        RcProfScope ps(ctx, s->cur, RC_K_OFFSHORE, 2, 8. * 8. * (2. + (d_summary ? 1. : 0.)));
        hipLaunchKernelGGL(k_of_mapsum, dim3(1), dim3(64), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    v.maps++;                                                 // a launch that failed is not a map
    v.have_map = true;
    return RC_OK;
}

extern "C" int rcflow_offshore_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, float* d_cross_along, size_t cross_along_step,
                                        uint8_t* d_class, size_t class_step, uint8_t* d_mask, size_t mask_step, uint8_t* d_picture,
                                        size_t picture_step, rc_offshore_station* d_stations, long long* d_table, long long* d_summary) {
    static const char* who = "rcflow_offshore_push_dev";
    RcSlot* s; RcOffshore* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::off, who, s, vp)) return rc;
    RcOffshore& v = *vp;
    const int w = v.w, h = v.h;
    const size_t nc = of_cells(v);
    if (!v.have_map) { rc_set_error("%s: the slot holds no map (rcflow_offshore_map_dev comes first, and again after a reset)", who); return RC_ESTATE; }
    if (!d_flow_xy) {                                         // the slot's resident field (rcflow_stream_flow_ptr), as rcflow_meanflow_push_dev
        if (!s->flow_w) { rc_set_error("%s: no flow field is resident on the slot yet", who); return RC_ESTATE; }
        if (s->flow_w != w || s->flow_h != h) {
            rc_set_error("%s: the resident flow field is %d x %d, the session %d x %d", who, s->flow_w, s->flow_h, w, h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)w * 8;
    }
    RcArgsN<8> ar(who, w, h);
    ar.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    ar.image("d_cross_along", d_cross_along, cross_along_step, 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_class", d_class, class_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_stations", d_stations, v.prm.stations * sizeof(rc_offshore_station), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_table", d_table, nc * RC_OFFSHORE_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, RC_OFFSHORE_SUMMARY * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const rc_offshore_params& q = v.prm;
    OfPushArgs a;
    memset(&a, 0, sizeof(a));
    a.flow = d_flow_xy; a.flow_step = flow_step; a.d2 = (const int*)v.d2.p; a.near = (const int*)v.near.p;
    a.ca = d_cross_along; a.ca_step = cross_along_step; a.cls = d_class; a.cls_step = class_step; a.mask = d_mask; a.mask_step = mask_step;
    a.pic = d_picture; a.pic_step = picture_step;
    a.tab = of_acc_tab(v); a.beyond = of_acc_beyond(v); a.cnt = of_acc_cnt(v);
    a.summary = of_out_push(v); a.table = of_out_table(v); a.recs = of_out_recs(v);
    a.summary2 = d_summary; a.table2 = d_table; a.recs2 = d_stations;
    a.w = w; a.h = h; a.min_d2 = q.min_dist * q.min_dist; a.max_d2 = q.max_dist * q.max_dist;
    a.stations = q.stations; a.bins = q.bins; a.bin_width = q.bin_width; a.min_count = q.min_count; a.rip_bins = q.rip_bins;
    a.cmin_q = of_ceil64(q.cross_min); a.by_x = q.flags == RC_OFFSHORE_STATION_X;
    a.pushes = v.pushes + 1;
    const double px = (double)w * h;
    {   // the map's planes and the field in, the outputs asked for out
        RcProfScope ps(ctx, s->cur, RC_K_OFFSHORE, 3, px * (8. + 8. + (d_cross_along ? 8. : 0.) + (d_class ? 1. : 0.) + (d_mask ? 1. : 0.) + (d_picture ? 3. : 0.)));
        hipLaunchKernelGGL(k_of_push, dim3((w + 63) / 64, (h + OF_ROWS - 1) / OF_ROWS), dim3(RC_BLOCK), 0, s->cur, a);
    }
    {   // the accumulators in and zero out, the table and the records out, once or twice
        const double tb = (double)nc * RC_OFFSHORE_SUMS * 8.;
        RcProfScope ps(ctx, s->cur, RC_K_OFFSHORE, 4, 2. * tb + (tb + q.stations * 48.) * (1. + (d_table || d_stations ? 1. : 0.)) + tb);
        hipLaunchKernelGGL(k_of_close, dim3(1), dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    v.pushes++;                                               // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_offshore_band_dev(rc_ctx* ctx, int stream, float lo, float hi, uint8_t* d_band, size_t band_step) {
    static const char* who = "rcflow_offshore_band_dev";
    RcSlot* s; RcOffshore* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::off, who, s, vp)) return rc;
    RcOffshore& v = *vp;
    if (!v.have_map) { rc_set_error("%s: the slot holds no map (rcflow_offshore_map_dev comes first, and again after a reset)", who); return RC_ESTATE; }
    if (!(lo >= 0.f && lo <= hi && hi <= 65536.f)) { rc_set_error("%s: lo and hi finite, 0 <= lo <= hi <= 65536", who); return RC_EINVAL; }
    if (rc_image_check(who, "d_band", d_band, band_step, v.w, v.h, 1, 1, RC_ARG_OUT)) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    OfBandArgs a;
    memset(&a, 0, sizeof(a));
    a.d2 = (const int*)v.d2.p; a.band = d_band; a.band_step = band_step; a.w = v.w; a.h = v.h; a.lo_q = of_ceil64(lo); a.hi_q = of_ceil64(hi);
    {
        RcProfScope ps(ctx, s->cur, RC_K_OFFSHORE, 5, (double)v.w * v.h * 5.);
        hipLaunchKernelGGL(k_of_band, dim3((v.w + RC_BLOCK - 1) / RC_BLOCK, v.h), dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_offshore_read(rc_ctx* ctx, int stream, rc_offshore_station* stations, long long* table, long long push_summary[RC_OFFSHORE_SUMMARY],
                                    long long map_summary[RC_OFFSHORE_SUMMARY]) {
    RcSlot* s; RcOffshore* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::off, "rcflow_offshore_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = of_cells(*vp);
    if (stations) RC_HIP(hipMemcpyAsync(stations, of_out_recs(*vp), vp->prm.stations * sizeof(rc_offshore_station), hipMemcpyDeviceToHost, s->cur));
    if (table) RC_HIP(hipMemcpyAsync(table, of_out_table(*vp), nc * RC_OFFSHORE_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (push_summary) RC_HIP(hipMemcpyAsync(push_summary, of_out_push(*vp), RC_OFFSHORE_SUMMARY * 8, hipMemcpyDeviceToHost, s->cur));
    if (map_summary) RC_HIP(hipMemcpyAsync(map_summary, of_out_map(*vp), RC_OFFSHORE_SUMMARY * 8, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_offshore_set(rc_ctx* ctx, int stream, const rc_offshore_params* prm) {
    static const char* who = "rcflow_offshore_set";
    RcSlot* s; RcOffshore* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::off, who, s, vp)) return rc;
    if (!prm || !of_prm_ok(*prm)) { rc_set_error("%s: %s", who, prm ? of_prm_text : "no parameters"); return RC_EINVAL; }
    if (prm->stations != vp->prm.stations || prm->bins != vp->prm.bins) {
        rc_set_error("%s: stations and bins are fixed at open (%d and %d)", who, vp->prm.stations, vp->prm.bins);
        return RC_EINVAL;
    }
    vp->prm = *prm;
    return RC_OK;
}

extern "C" int rcflow_offshore_info(rc_ctx* ctx, int stream, rc_offshore_info* info) {
    RcSlot* s; RcOffshore* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::off, "rcflow_offshore_info", s, vp)) return rc;
    const RcOffshore& v = *vp;
    if (!info) { rc_set_error("rcflow_offshore_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->launches_per_map = RC_OFFSHORE_MAP_LAUNCHES; info->launches_per_push = RC_OFFSHORE_PUSH_LAUNCHES;
    info->have_map = v.have_map ? 1 : 0;
    info->maps = v.maps; info->pushes = v.pushes;
    info->device_bytes = v.col.bytes + v.d2.bytes + v.near.bytes + v.jet.bytes + v.acc.bytes + v.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_offshore_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::off, "rcflow_offshore_reset"); }
extern "C" int rcflow_offshore_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::off); }
