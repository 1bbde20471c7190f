// region_kernels.hip -- rip regions (rcflow_regions_*): the connected components of a mask numbered in raster order, filtered
// by area and measured, on the device.  The contract is the header comment of include/rcflow.h; DESIGN 7g has the reasons.
//
// A push is seven launches whatever the mask holds:
//   @0 runs     a wave owns a row segment of 64 pixels; __ballot gives the segment's 64-bit mask and every foreground pixel
//               takes the start of its run in the segment as parent (index y * w + x).  Background: -1.  Area scratch: 0.
//   @1 merge    union-find in global memory over what the runs do not say: the segment border in the row, and the row above
//               (only where a new contact starts).  atomicMin on parent words; a parent is always the smaller index, so a
//               root is the smallest index of its set: first(C), for free.
//   @2 flatten  every pixel takes its root; areas are counted per wave over 8 rows, then per block, then added to the root's word.
//   @3 rows     a block per row: kept roots, roots, foreground pixels, largest kept area, kept pixels of the row.
//   @4 number   a block per row: the kept roots of the rows above (a sum over at most h words) plus the rank inside the row is
//               the root's number; the root's word in the area scratch takes it, its record's accumulator is set up.
//   @5 outputs  labels, the opened mask, and the sums: two pixels per lane (the flow is read 16 bytes per lane where it is
//               aligned), pre-aggregated per wave over 8 rows and per block before any atomic.
//   @6 records  a thread per record: the integer part from the accumulator, the derived doubles, zero bytes beyond K; the summary.
// Nothing is read back and no launch depends on what an earlier one found.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <string.h>

#include "rc_device.h"
#include "rc_host.h"

#define RG_ROWS 8                       // rows a wave walks
#define RG_WAVES 4                      // waves of a block
#define RG_TILE_H (RG_ROWS * RG_WAVES)
#define RG_QMAX 1099511627776.0f        // 2^40: the bound of rcflow_ripmap_*'s fixed point
static_assert(RC_BLOCK == 64 * RG_WAVES, "a block is RG_WAVES waves");

struct RgCtl {                          // zeroed by @0
    unsigned long long bad;             // flow pixels of kept components left out (@5)
    int K;                              // kept components (@4)
    int pad;
};
struct RgAcc {                          // 88 bytes; set up by @4, added into by @5
    int x0, y0, x1, y1, bad, area, first, pad;
    long long sx, sy, sxx, syy, sxy, fx, fy;
};
static_assert(sizeof(RgAcc) == 88 && sizeof(rc_region) == 144 && sizeof(RgCtl) == 16, "layouts");

struct RgRows {                         // views into RcRegions::rows
    int* kept; int* roots; int* fg; int* maxa; long long* keptpx;
};

__device__ __forceinline__ int rg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int rg_find(const int* par, int a) {
    int p;
    while ((p = rg_load(par + a)) != a) a = p;             // a parent is smaller than its child: this ends
    return a;
}
// Playne & Hawick / Komura: hook the larger root under the smaller one; when the word was not a root any more, go on with what it held
__device__ __forceinline__ void rg_union(int* par, int a, int b) {
    a = rg_find(par, a);
    b = rg_find(par, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) break;
        a = old;
    }
}
__device__ __forceinline__ long long rg_wsum(long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------- @0
__global__ __launch_bounds__(RC_BLOCK) void k_rg_runs(const uint8_t* mask, size_t step, int w, int h, int* par, int* area, RgCtl* ctl) {
    const int lane = threadIdx.x, x = blockIdx.x * 64 + lane;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.y == 0 && lane == 0) { ctl->bad = 0; ctl->K = 0; ctl->pad = 0; }
    const int yb = (blockIdx.y * RG_WAVES + threadIdx.y) * RG_ROWS;
    for (int r = 0; r < RG_ROWS; r++) {
        const int y = yb + r;
        if (y >= h) break;
        const bool fg = x < w && mask[(size_t)y * step + x] != 0;
        const unsigned long long m = __ballot(fg);
        if (x < w) {
            const unsigned long long z = ~m & ((1ull << lane) - 1);      // background below this lane
            const int start = z ? 64 - __clzll(z) : 0;
            const int idx = y * w + x;
            par[idx] = fg ? idx - lane + start : -1;
            area[idx] = 0;
        }
    }
}

// ---------------------------------------------------------------------------- @1
template <int CONN>
__global__ __launch_bounds__(RC_BLOCK) void k_rg_merge(int* par, int w, int h) {
    const int lane = threadIdx.x, x = blockIdx.x * 64 + lane;
    const int yb = (blockIdx.y * RG_WAVES + threadIdx.y) * RG_ROWS;
    for (int r = 0; r < RG_ROWS; r++) {
        const int y = yb + r;
        if (y >= h) break;
        const int idx = y * w + x;
        // whether a word is foreground never changes (only its value does): plain sign tests
        const bool fg = x < w && rg_load(par + idx) >= 0;
        const bool up = x < w && y > 0 && rg_load(par + idx - w) >= 0;
        const unsigned long long m = __ballot(fg), mu = __ballot(up);
        if (!fg) continue;
        const bool L = lane ? (m >> (lane - 1)) & 1 : (x > 0 && rg_load(par + idx - 1) >= 0);
        const bool UL = lane ? (mu >> (lane - 1)) & 1 : (x > 0 && y > 0 && rg_load(par + idx - w - 1) >= 0);
        if (lane == 0 && L) rg_union(par, idx, idx - 1);                 // the runs stop at the segment border
        if (CONN == 4) {
            // L and UL both set: L is joined to UL (its own contact), UL to U by the row
            if (up && !(L && UL)) rg_union(par, idx, idx - w);
        } else {
            const bool UR = lane < 63 ? (mu >> (lane + 1)) & 1 : (x + 1 < w && y > 0 && rg_load(par + idx - w + 1) >= 0);
            // Claim: every pixel ends joined to each of UL, U, UR that is set.  Induction over x along the WHOLE row, not
            // the wave: the rule below is the same for every pixel, and lane 0 takes L and UL from memory, so a segment
            // border changes nothing.  Base, x == 0: L and UL are clear, every contact that is set is joined directly.
            // Step: U set and L clear: joined directly; U set and L set: L is joined to its own UR, which is U (the claim
            // at x - 1), and this pixel to L by the row; UL and UR hang on U by the row.  U clear: UL is L's U (the claim
            // at x - 1) or joined directly; UR is no neighbour of L (L's UR is U, clear), so it is always joined directly:
            // that union is needed also when L is set.
            if (up) { if (!L) rg_union(par, idx, idx - w); }
            else {
                if (UL && !L) rg_union(par, idx, idx - w - 1);           // L set: UL is L's U
                if (UR) rg_union(par, idx, idx - w + 1);
            }
        }
    }
}

// ---------------------------------------------------------------------------- @2
__global__ __launch_bounds__(RC_BLOCK) void k_rg_flatten(int* par, int* area, int w, int h) {
    __shared__ int s_root[RG_WAVES], s_cnt[RG_WAVES];
    const int lane = threadIdx.x, wv = threadIdx.y, x = blockIdx.x * 64 + lane;
    const int yb = (blockIdx.y * RG_WAVES + wv) * RG_ROWS;
    int cur = -1, cnt = 0;                                               // the wave's running root and its pixels (uniform)
    for (int r = 0; r < RG_ROWS; r++) {
        const int y = yb + r;
        if (y >= h) break;
        const int idx = y * w + x;
        int root = -1;
        if (x < w && par[idx] >= 0) {
            root = rg_find(par, idx);
            // other waves walk this word meanwhile: the old parent and the root are both ancestors with a smaller index, either is right
            __hip_atomic_store(par + idx, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned long long todo = __ballot(root >= 0);
        while (todo) {
            const int rl = __shfl(root, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(root == rl);
            todo &= ~same;
            if (rl != cur) {
                if (cnt && lane == 0) atomicAdd(area + cur, cnt);
                cur = rl; cnt = 0;
            }
            cnt += __popcll(same);
        }
    }
    if (lane == 0) { s_root[wv] = cur; s_cnt[wv] = cnt; }
    __syncthreads();
    if (wv == 0 && lane == 0) {
        for (int i = 0; i < RG_WAVES; i++) {
            if (!s_cnt[i]) continue;
            int c = s_cnt[i];
            for (int j = i + 1; j < RG_WAVES; j++)
                if (s_cnt[j] && s_root[j] == s_root[i]) { c += s_cnt[j]; s_cnt[j] = 0; }
            atomicAdd(area + s_root[i], c);
        }
    }
}

// ---------------------------------------------------------------------------- @3, @4
__device__ __forceinline__ long long rg_block_sum(long long v, long long* s_red) {
    v = rg_wsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int i = 0; i < RG_WAVES; i++) t += s_red[i];
    return t;
}

__global__ __launch_bounds__(RC_BLOCK) void k_rg_rows(const int* par, const int* area, int w, int min_area, RgRows rows) {
    __shared__ long long s_red[RG_WAVES];
    const int y = blockIdx.x;
    int kept = 0, roots = 0, fg = 0, maxa = 0;
    long long keptpx = 0;
    for (int x = threadIdx.x; x < w; x += RC_BLOCK) {
        const int idx = y * w + x, p = par[idx];
        fg += p >= 0;
        if (p == idx) {
            const int a = area[idx];
            roots++;
            if (a >= min_area) { kept++; keptpx += a; maxa = a > maxa ? a : maxa; }
        }
    }
    const long long k = rg_block_sum(kept, s_red), ro = rg_block_sum(roots, s_red), f = rg_block_sum(fg, s_red);
    const long long kp = rg_block_sum(keptpx, s_red);
#pragma unroll
    for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(maxa, o); maxa = t > maxa ? t : maxa; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = maxa;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long m = 0;
        for (int i = 0; i < RG_WAVES; i++) m = s_red[i] > m ? s_red[i] : m;
        rows.kept[y] = (int)k; rows.roots[y] = (int)ro; rows.fg[y] = (int)f; rows.maxa[y] = (int)m; rows.keptpx[y] = kp;
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_rg_number(const int* par, int* area, int w, int h, int min_area, int max_regions, RgRows rows,
                                                        RgAcc* acc, RgCtl* ctl) {
    __shared__ long long s_red[RG_WAVES];
    __shared__ int s_cnt[RG_WAVES];
    const int y = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long part = 0;
    for (int i = threadIdx.x; i < y; i += RC_BLOCK) part += rows.kept[i];
    int base = (int)rg_block_sum(part, s_red);                           // kept roots of the rows above
    if (y == h - 1 && threadIdx.x == 0) ctl->K = base + rows.kept[y];
    for (int xb = 0; xb < w; xb += RC_BLOCK) {                           // uniform trip count: the barriers below are met by all
        const int x = xb + threadIdx.x, idx = y * w + x;
        bool root = false, keep = false;
        int a = 0;
        if (x < w && par[idx] == idx) { root = true; a = area[idx]; keep = a >= min_area; }
        const unsigned long long m = __ballot(keep);
        __syncthreads();
        if (lane == 0) s_cnt[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < RG_WAVES; i++) { before += i < wv ? s_cnt[i] : 0; total += s_cnt[i]; }
        if (root) {
            const int k = keep ? base + before + __popcll(m & ((1ull << lane) - 1)) + 1 : 0;
            area[idx] = k;                                               // the root's word now holds its number
            if (k && k <= max_regions) {
                RgAcc q;
                q.x0 = INT_MAX; q.y0 = INT_MAX; q.x1 = -1; q.y1 = -1; q.bad = 0; q.area = a; q.first = idx; q.pad = 0;
                q.sx = q.sy = q.sxx = q.syy = q.sxy = q.fx = q.fy = 0;
                acc[k - 1] = q;
            }
        }
        base += total;
    }
}

// ---------------------------------------------------------------------------- @5
struct RgStatArgs {
    const int* par; const int* area; int w, h, max_regions;
    const float* flow; size_t flow_step;
    int32_t* labels; size_t labels_step;
    uint8_t* mask_out; size_t mask_out_step;
    RgAcc* acc; RgCtl* ctl;
};
struct RgPart {                          // the sums of one component over part of a tile (uniform over the wave)
    int k, x0, y0, x1, y1, bad;
    long long sx, sy, sxx, syy, sxy, fx, fy;
};
__device__ __forceinline__ void rg_part_clear(RgPart& p) {
    p.k = 0; p.x0 = INT_MAX; p.y0 = INT_MAX; p.x1 = -1; p.y1 = -1; p.bad = 0;
    p.sx = p.sy = p.sxx = p.syy = p.sxy = p.fx = p.fy = 0;
}
// one thread.  The box words only move one way, so a word that already holds as much needs no atomic
__device__ __forceinline__ void rg_flush(RgAcc* acc, const RgPart& p) {
    if (!p.k) return;
    RgAcc* q = acc + (p.k - 1);
    if (rg_load(&q->x0) > p.x0) atomicMin(&q->x0, p.x0);
    if (rg_load(&q->y0) > p.y0) atomicMin(&q->y0, p.y0);
    if (rg_load(&q->x1) < p.x1) atomicMax(&q->x1, p.x1);
    if (rg_load(&q->y1) < p.y1) atomicMax(&q->y1, p.y1);
    if (p.bad) atomicAdd(&q->bad, p.bad);
    atomicAdd((unsigned long long*)&q->sx, (unsigned long long)p.sx);
    atomicAdd((unsigned long long*)&q->sy, (unsigned long long)p.sy);
    atomicAdd((unsigned long long*)&q->sxx, (unsigned long long)p.sxx);
    atomicAdd((unsigned long long*)&q->syy, (unsigned long long)p.syy);
    atomicAdd((unsigned long long*)&q->sxy, (unsigned long long)p.sxy);
    if (p.fx) atomicAdd((unsigned long long*)&q->fx, (unsigned long long)p.fx);
    if (p.fy) atomicAdd((unsigned long long*)&q->fy, (unsigned long long)p.fy);
}

template <bool FLOW>
__global__ __launch_bounds__(RC_BLOCK) void k_rg_stats(const RgStatArgs a) {
    __shared__ RgPart s_part[RG_WAVES];
    __shared__ unsigned s_bad[RG_WAVES];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const int xb = blockIdx.x * 128, x = xb + 2 * lane;
    const int yb = (blockIdx.y * RG_WAVES + wv) * RG_ROWS;
    const bool in0 = x < a.w, in1 = x + 1 < a.w;
    RgPart cur;
    rg_part_clear(cur);
    unsigned nbad = 0;                                                   // bad pixels of kept components (uniform)
    for (int r = 0; r < RG_ROWS; r++) {
        const int y = yb + r;
        if (y >= a.h) break;
        const int idx = y * a.w + x;
        const int p0 = in0 ? a.par[idx] : -1, p1 = in1 ? a.par[idx + 1] : -1;
        const int k0 = p0 >= 0 ? a.area[p0] : 0, k1 = p1 >= 0 ? a.area[p1] : 0;
        if (a.labels) {
            int32_t* row = (int32_t*)((char*)a.labels + (size_t)y * a.labels_step) + x;
            if (in1 && ((uintptr_t)row & 7) == 0) *(int2*)row = make_int2(k0, k1);
            else { if (in0) row[0] = k0; if (in1) row[1] = k1; }
        }
        if (a.mask_out) {
            uint8_t* row = a.mask_out + (size_t)y * a.mask_out_step + x;
            const uint8_t b0 = k0 ? 255 : 0, b1 = k1 ? 255 : 0;
            if (in1 && ((uintptr_t)row & 1) == 0) *(uchar2*)row = make_uchar2(b0, b1);
            else { if (in0) row[0] = b0; if (in1) row[1] = b1; }
        }
        long long qx0 = 0, qy0 = 0, qx1 = 0, qy1 = 0;
        bool bad0 = false, bad1 = false;
        if (FLOW) {
            const float* row = (const float*)((const char*)a.flow + (size_t)y * a.flow_step) + 2 * x;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in1 && ((uintptr_t)row & 15) == 0) v = *(const float4*)row;
            else {
                if (in0) { const float2 t = *(const float2*)row; v.x = t.x; v.y = t.y; }
                if (in1) { const float2 t = *(const float2*)(row + 2); v.z = t.x; v.w = t.y; }
            }
            // the fixed point of rcflow_ripmap_*: a scaling by 2^16 is exact; NaN fails the comparison
            const float ax = v.x * 65536.0f, ay = v.y * 65536.0f, bx = v.z * 65536.0f, by = v.w * 65536.0f;
            bad0 = k0 && !(fabsf(ax) <= RG_QMAX && fabsf(ay) <= RG_QMAX);
            bad1 = k1 && !(fabsf(bx) <= RG_QMAX && fabsf(by) <= RG_QMAX);
            if (k0 && !bad0) { qx0 = (long long)rintf(ax); qy0 = (long long)rintf(ay); }
            if (k1 && !bad1) { qx1 = (long long)rintf(bx); qy1 = (long long)rintf(by); }
            nbad += __popcll(__ballot(bad0)) + __popcll(__ballot(bad1));
        }
        bool a0 = k0 > 0 && k0 <= a.max_regions, a1 = k1 > 0 && k1 <= a.max_regions;
        for (;;) {
            const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
            if (!(m0 | m1)) break;
            // the component of the leftmost pixel not yet taken
            const int l0 = m0 ? __ffsll((long long)m0) - 1 : 64, l1 = m1 ? __ffsll((long long)m1) - 1 : 64;
            const int kl = l0 <= l1 ? __shfl(k0, l0) : __shfl(k1, l1);
            const bool s0 = a0 && k0 == kl, s1 = a1 && k1 == kl;
            a0 = a0 && !s0; a1 = a1 && !s1;
            const unsigned long long b0 = __ballot(s0), b1 = __ballot(s1);
            const int cnt = __popcll(b0) + __popcll(b1);
            int lo = INT_MAX, hi = -1;
            if (b0) { lo = xb + 2 * (__ffsll((long long)b0) - 1); hi = xb + 2 * (63 - __clzll(b0)); }
            if (b1) {
                const int l = xb + 2 * (__ffsll((long long)b1) - 1) + 1, u = xb + 2 * (63 - __clzll(b1)) + 1;
                lo = l < lo ? l : lo; hi = u > hi ? u : hi;
            }
            const long long X = x;
            const long long sx = rg_wsum((s0 ? X : 0) + (s1 ? X + 1 : 0));
            const long long sxx = rg_wsum((s0 ? X * X : 0) + (s1 ? (X + 1) * (X + 1) : 0));
            long long fx = 0, fy = 0;
            int bad = 0;
            if (FLOW) {
                fx = rg_wsum((s0 ? qx0 : 0) + (s1 ? qx1 : 0));
                fy = rg_wsum((s0 ? qy0 : 0) + (s1 ? qy1 : 0));
                bad = __popcll(__ballot(s0 && bad0)) + __popcll(__ballot(s1 && bad1));
            }
            if (kl != cur.k) {
                if (lane == 0) rg_flush(a.acc, cur);
                rg_part_clear(cur);
                cur.k = kl;
            }
            cur.x0 = lo < cur.x0 ? lo : cur.x0; cur.x1 = hi > cur.x1 ? hi : cur.x1;
            cur.y0 = y < cur.y0 ? y : cur.y0; cur.y1 = y > cur.y1 ? y : cur.y1;
            cur.bad += bad;
            cur.sx += sx; cur.sy += (long long)y * cnt; cur.sxx += sxx; cur.syy += (long long)y * y * cnt; cur.sxy += (long long)y * sx;
            cur.fx += fx; cur.fy += fy;
        }
    }
    if (lane == 0) { s_part[wv] = cur; s_bad[wv] = nbad; }
    __syncthreads();
    if (wv == 0 && lane == 0) {
        unsigned nb = 0;
        for (int i = 0; i < RG_WAVES; i++) {
            nb += s_bad[i];
            RgPart& p = s_part[i];
            if (!p.k) continue;
            for (int j = i + 1; j < RG_WAVES; j++) {
                RgPart& q = s_part[j];
                if (q.k != p.k) continue;
                p.x0 = q.x0 < p.x0 ? q.x0 : p.x0; p.y0 = q.y0 < p.y0 ? q.y0 : p.y0;
                p.x1 = q.x1 > p.x1 ? q.x1 : p.x1; p.y1 = q.y1 > p.y1 ? q.y1 : p.y1;
                p.bad += q.bad;
                p.sx += q.sx; p.sy += q.sy; p.sxx += q.sxx; p.syy += q.syy; p.sxy += q.sxy; p.fx += q.fx; p.fy += q.fy;
                q.k = 0;
            }
            rg_flush(a.acc, p);
        }
        if (nb) atomicAdd(&a.ctl->bad, (unsigned long long)nb);
    }
}

// ---------------------------------------------------------------------------- @6, @7
__device__ __forceinline__ void rg_record(const RgAcc& q, int label, int w, int h, rc_region& o) {
    o.label = label; o.area = q.area;
    o.x0 = q.x0; o.y0 = q.y0; o.x1 = q.x1; o.y1 = q.y1;
    o.first_x = q.first % w; o.first_y = q.first / w;
    o.edges = (q.x0 == 0 ? 1 : 0) | (q.y0 == 0 ? 2 : 0) | (q.x1 == w - 1 ? 4 : 0) | (q.y1 == h - 1 ? 8 : 0);
    o.bad = q.bad;
    o.sx = q.sx; o.sy = q.sy; o.sxx = q.sxx; o.syy = q.syy; o.sxy = q.sxy; o.fx = q.fx; o.fy = q.fy;
    // the derived part: the header's order, every operation rounded on its own (the library is built without contraction)
    const double n = (double)q.area;
    const int m = q.area - q.bad;
    o.cx = (double)q.sx / n; o.cy = (double)q.sy / n;
    o.mean_fx = m ? (float)((double)q.fx / 65536.0 / (double)m) : 0.f;
    o.mean_fy = m ? (float)((double)q.fy / 65536.0 / (double)m) : 0.f;
    const double mxx = (double)q.sxx / n - o.cx * o.cx, myy = (double)q.syy / n - o.cy * o.cy, mxy = (double)q.sxy / n - o.cx * o.cy;
    const double t = (mxx + myy) * 0.5, d = (mxx - myy) * 0.5, r = sqrt(d * d + mxy * mxy);
    o.var_major = t + r; o.var_minor = t - r;
    double ang = atan2(mxy, d) * 0.5 * (180.0 / 3.14159265358979323846);
    if (ang < 0.) ang += 180.;
    if (ang >= 180.) ang = 0.;
    o.angle = ang;
}

__global__ __launch_bounds__(RC_BLOCK) void k_rg_records(const RgAcc* acc, const RgCtl* ctl, RgRows rows, int w, int h, int max_regions,
                                                         long long pushes, rc_region* keep, rc_region* user, long long* keep_sum,
                                                         long long* user_sum) {
    __shared__ long long s_red[RG_WAVES];
    const int K = ctl->K, nrec = K < max_regions ? K : max_regions;
    if (blockIdx.x == 0) {
        long long roots = 0, fg = 0, kp = 0;
        int maxa = 0;
        for (int y = threadIdx.x; y < h; y += RC_BLOCK) {
            roots += rows.roots[y]; fg += rows.fg[y]; kp += rows.keptpx[y];
            maxa = rows.maxa[y] > maxa ? rows.maxa[y] : maxa;
        }
        roots = rg_block_sum(roots, s_red); fg = rg_block_sum(fg, s_red); kp = rg_block_sum(kp, s_red);
#pragma unroll
        for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(maxa, o); maxa = t > maxa ? t : maxa; }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = maxa;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long m = 0;
            for (int i = 0; i < RG_WAVES; i++) m = s_red[i] > m ? s_red[i] : m;
            const long long s[8] = {roots, (long long)K, (long long)nrec, fg, kp, (long long)ctl->bad, pushes, m};
            for (int i = 0; i < 8; i++) { keep_sum[i] = s[i]; if (user_sum) user_sum[i] = s[i]; }
        }
    }
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= max_regions) return;
    rc_region o;
    memset(&o, 0, sizeof(o));
    if (i < nrec) rg_record(acc[i], i + 1, w, h, o);
    keep[i] = o;
    if (user) user[i] = o;
}

__device__ __forceinline__ rc_draw_prim rg_line(int x0, int y0, int x1, int y1, int t, uint32_t color) {
    rc_draw_prim p;
    p.kind = RC_DRAW_LINE; p.x0 = x0; p.y0 = y0; p.x1 = x1; p.y1 = y1; p.size = t; p.color = color; p.flags = 0;
    return p;
}
__device__ __forceinline__ int rg_step(double mean, double scale) {
    const double v = rint(mean * scale);
    return fabs(v) <= 1073741824.0 ? (int)v : INT_MIN;                   // NaN fails the comparison
}

__global__ __launch_bounds__(RC_BLOCK) void k_rg_prims(const rc_region* rec, int max_regions, uint32_t color, int thickness, int radius,
                                                       double flow_scale, rc_draw_prim* out) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= max_regions) return;
    const rc_region q = rec[i];
    rc_draw_prim p[6];
    memset(p, 0, sizeof(p));
    if (q.label) {
        p[0] = rg_line(q.x0, q.y0, q.x1, q.y0, thickness, color);
        p[1] = rg_line(q.x1, q.y0, q.x1, q.y1, thickness, color);
        p[2] = rg_line(q.x1, q.y1, q.x0, q.y1, thickness, color);
        p[3] = rg_line(q.x0, q.y1, q.x0, q.y0, thickness, color);
        const long long n = q.area;
        const int px = (int)((2 * q.sx + n) / (2 * n)), py = (int)((2 * q.sy + n) / (2 * n));
        p[4].kind = RC_DRAW_DISC; p[4].x0 = p[4].x1 = px; p[4].y0 = p[4].y1 = py; p[4].size = radius; p[4].color = color;
        const int m = q.area - q.bad;
        if (flow_scale != 0. && m > 0) {
            const int dx = rg_step((double)q.fx / 65536.0 / (double)m, flow_scale), dy = rg_step((double)q.fy / 65536.0 / (double)m, flow_scale);
            p[5] = rg_line(px, py, dx == INT_MIN ? INT_MIN : px + dx, dy == INT_MIN ? INT_MIN : py + dy, thickness, color);
        }
    }
    for (int j = 0; j < 6; j++) out[(size_t)6 * i + j] = p[j];
}

// ============================================================================ host side
void rc_state_free(RcRegions& g) {
    rc_buf_free(g.par); rc_buf_free(g.area); rc_buf_free(g.rows); rc_buf_free(g.acc); rc_buf_free(g.out);
    rc_fence_free(g.zf);
    g = RcRegions();
}

// open and reset: the kept records and summary, the push count
int rc_state_zero(RcSlot& s, RcRegions& g) {
    const int rc = rc_fence_zero(g.zf, s.cur, {&g.out});
    if (rc) return rc;
    g.pushes = 0;
    return RC_OK;
}

static long long* rg_summary(const RcRegions& g) { return (long long*)g.out.p; }
static rc_region* rg_records(const RcRegions& g) { return (rc_region*)((char*)g.out.p + 64); }
static RgRows rg_rows(const RcRegions& g) {
    RgRows r;
    const size_t h = (size_t)g.h;
    r.keptpx = (long long*)g.rows.p;
    r.kept = (int*)(r.keptpx + h); r.roots = r.kept + h; r.fg = r.roots + h; r.maxa = r.fg + h;
    return r;
}

extern "C" int rcflow_regions_open(rc_ctx* ctx, int stream, int w, int h, const rc_regions_params* prm) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0 || (long long)w * h >= (1ll << 31)) {
        rc_set_error("rcflow_regions_open: bad frame size %d x %d (below 2^31 pixels) or no parameters", w, h);
        return RC_EINVAL;
    }
    if ((prm->connectivity != 4 && prm->connectivity != 8) || prm->min_area < 1 || prm->max_regions < 1 || prm->max_regions > RC_REGIONS_MAX ||
        prm->flags) {
        rc_set_error("rcflow_regions_open: connectivity 4 | 8, min_area >= 1, max_regions 1..%d, flags 0", RC_REGIONS_MAX);
        return RC_EINVAL;
    }
    int rc = rc_fits_context("rcflow_regions_open", ctx, w, h);
    if (rc) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcRegions n;
    n.w = w; n.h = h; n.prm = *prm;
    const size_t px = (size_t)w * h;
    rc = rc_buf_ensure(n.par, px * 4);
    if (!rc) rc = rc_buf_ensure(n.area, px * 4);
    if (!rc) rc = rc_buf_ensure(n.rows, (size_t)h * 24);
    if (!rc) rc = rc_buf_ensure(n.acc, sizeof(RgCtl) + (size_t)prm->max_regions * sizeof(RgAcc));
    if (!rc) rc = rc_buf_ensure(n.out, 64 + (size_t)prm->max_regions * sizeof(rc_region));
    return rc_state_install(*s, s->rg, n, rc);
}

extern "C" int rcflow_regions_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_mask, size_t mask_step, const float* d_flow_xy,
                                       size_t flow_step, int32_t* d_labels, size_t labels_step, uint8_t* d_mask_out, size_t mask_out_step,
                                       rc_region* d_regions, long long* d_summary) {
    static const char* who = "rcflow_regions_push_dev";
    RcSlot* s; RcRegions* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rg, who, s, gp)) return rc;
    RcRegions& g = *gp;
    const int w = g.w, h = g.h;
    RcArgs a(who, w, h);
    const int im = a.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_IN);
    a.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN | RC_ARG_OPTIONAL);
    a.image("d_labels", d_labels, labels_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.in_place(a.image("d_mask_out", d_mask_out, mask_out_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL), im);
    a.array("d_regions", d_regions, (size_t)g.prm.max_regions * sizeof(rc_region), 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(g.zf, s->cur, true);
    if (rc) return rc;
    const double px = (double)w * h;
    int* par = (int*)g.par.p;
    int* area = (int*)g.area.p;
    RgCtl* ctl = (RgCtl*)g.acc.p;
    RgAcc* acc = (RgAcc*)(ctl + 1);
    const RgRows rows = rg_rows(g);
    const dim3 blk(64, RG_WAVES), grid((w + 63) / 64, (h + RG_TILE_H - 1) / RG_TILE_H), grid2((w + 127) / 128, (h + RG_TILE_H - 1) / RG_TILE_H);
    { RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 0, 9. * px);
      hipLaunchKernelGGL(k_rg_runs, grid, blk, 0, s->cur, d_mask, mask_step, w, h, par, area, ctl); }
    { RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 1, 8. * px);
      if (g.prm.connectivity == 4) hipLaunchKernelGGL(k_rg_merge<4>, grid, blk, 0, s->cur, par, w, h);
      else hipLaunchKernelGGL(k_rg_merge<8>, grid, blk, 0, s->cur, par, w, h); }
    { RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 2, 8. * px);
      hipLaunchKernelGGL(k_rg_flatten, grid, blk, 0, s->cur, par, area, w, h); }
    { RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 3, 4. * px);
      hipLaunchKernelGGL(k_rg_rows, dim3(h), dim3(RC_BLOCK), 0, s->cur, par, area, w, g.prm.min_area, rows); }
    { RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 4, 4. * px);
      hipLaunchKernelGGL(k_rg_number, dim3(h), dim3(RC_BLOCK), 0, s->cur, par, area, w, h, g.prm.min_area, g.prm.max_regions, rows, acc, ctl); }
    {
        RgStatArgs a;
        a.par = par; a.area = area; a.w = w; a.h = h; a.max_regions = g.prm.max_regions;
        a.flow = d_flow_xy; a.flow_step = flow_step;
        a.labels = d_labels; a.labels_step = labels_step;
        a.mask_out = d_mask_out; a.mask_out_step = mask_out_step;
        a.acc = acc; a.ctl = ctl;
        RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 5, (4. + (d_flow_xy ? 8. : 0.) + (d_labels ? 4. : 0.) + (d_mask_out ? 1. : 0.)) * px);
        if (d_flow_xy) hipLaunchKernelGGL(k_rg_stats<true>, grid2, blk, 0, s->cur, a);
        else hipLaunchKernelGGL(k_rg_stats<false>, grid2, blk, 0, s->cur, a);
    }
    { RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 6, (double)g.prm.max_regions * (sizeof(RgAcc) + (d_regions ? 2. : 1.) * sizeof(rc_region)));
      hipLaunchKernelGGL(k_rg_records, dim3((g.prm.max_regions + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, acc, ctl, rows, w, h,
                         g.prm.max_regions, g.pushes + 1, rg_records(g), d_regions, rg_summary(g), d_summary); }
    RC_HIP(hipGetLastError());
    g.pushes++;                                           // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_regions_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, double flow_scale,
                                        rc_draw_prim* d_prims) {
    static const char* who = "rcflow_regions_prims_dev";
    RcSlot* s; RcRegions* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rg, who, s, gp)) return rc;
    RcRegions& g = *gp;
    if (rc_prims_check(who, d_prims, thickness, disc_radius)) return RC_EINVAL;
    if (!(fabs(flow_scale) <= 1.7976931348623157e308)) { rc_set_error("%s: flow_scale is not finite", who); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(g.zf, s->cur, true);
    if (rc) return rc;
    RcProfScope ps(ctx, s->cur, RC_K_REGIONS, 7, (double)g.prm.max_regions * (sizeof(rc_region) + 6. * sizeof(rc_draw_prim)));
    hipLaunchKernelGGL(k_rg_prims, dim3((g.prm.max_regions + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, rg_records(g),
                       g.prm.max_regions, color, thickness, disc_radius, flow_scale, d_prims);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_regions_read(rc_ctx* ctx, int stream, rc_region* regions, int cap, int* n, long long summary[8]) {
    RcSlot* s; RcRegions* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rg, "rcflow_regions_read", s, gp)) return rc;
    RcRegions& g = *gp;
    if (cap < 0 || (cap && !regions)) { rc_set_error("rcflow_regions_read: a bad buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(g.zf, s->cur, true);
    if (rc) return rc;
    // summary and records lie together: one copy of the prefix the caller can take
    const int room = cap < g.prm.max_regions ? cap : g.prm.max_regions;
    std::vector<char> host(64 + (size_t)room * sizeof(rc_region));
    RC_HIP(hipMemcpyAsync(host.data(), g.out.p, host.size(), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    long long sum[8];
    memcpy(sum, host.data(), 64);
    const int written = (int)sum[2], take = written < room ? written : room;
    if (regions && take) memcpy(regions, host.data() + 64, (size_t)take * sizeof(rc_region));
    if (n) *n = written;
    if (summary) memcpy(summary, sum, 64);
    return RC_OK;
}

extern "C" int rcflow_regions_set(rc_ctx* ctx, int stream, int min_area) {
    RcSlot* s; RcRegions* g;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rg, "rcflow_regions_set", s, g)) return rc;
    if (min_area < 1) { rc_set_error("rcflow_regions_set: min_area >= 1"); return RC_EINVAL; }
    g->prm.min_area = min_area;
    return RC_OK;
}

extern "C" int rcflow_regions_info(rc_ctx* ctx, int stream, rc_regions_info* info) {
    RcSlot* s; RcRegions* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::rg, "rcflow_regions_info", s, gp)) return rc;
    const RcRegions& g = *gp;
    if (!info) return RC_OK;
    memset(info, 0, sizeof(*info));
    info->w = g.w; info->h = g.h; info->connectivity = g.prm.connectivity; info->min_area = g.prm.min_area;
    info->max_regions = g.prm.max_regions; info->flags = g.prm.flags;
    info->launches_per_push = RC_REGIONS_LAUNCHES;
    info->pushes = g.pushes;
    info->device_bytes = g.par.bytes + g.area.bytes + g.rows.bytes + g.acc.bytes + g.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_regions_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::rg, "rcflow_regions_reset"); }
extern "C" int rcflow_regions_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::rg); }
