// outline_kernels.hip -- region outlines (rcflow_outlines_*): the boundaries of a label plane or a mask traced into ordered polygons.
//
// include/rcflow.h ("region outlines") is the specification; tests/_outlines_ref.py states it by a sequential walk and the kernels are
// held to that bit for bit: everything is an integer.  Nothing synchronises.  Boundary following is a linked list, and the lists are
// ranked by pointer jumping.  A push is RC_OUTLINES_FIXED_LAUNCHES + 2 * rounds launches under eleven profile names (a name's
// level is below RC_MAX_LEVELS, so launches that belong together share one):
//   outlines@0   two launches.  A block owns 256 pixels of a row; the labels with a one-pixel halo go into LDS; the four side bits of
//                every pixel, and the block's count of cracks by the waves' ballots and population counts.  Then one block scans the
//                block counts: the crack count, the overflow word, and the rounds' hand-over words
//   outlines@1   the same blocks: a scan inside the block gives every pixel the number of cracks before it (the base plane), every
//                crack its place in key order, its key, its turn bit and the KEY of its successor
//   outlines@2   a thread per crack: the successor's key to its place, through the base plane and the bits below its side
//   outlines@3   x rounds: pointer doubling, (pointer, smallest place of the window), from one buffer pair into the other
//   outlines@4   every loop cut before its leader; the leader's place kept per crack
//   outlines@5   x rounds: Wyllie's list ranking, (pointer, distance to the end), from one buffer pair into the other
//   outlines@6   three launches: per block of 1024 cracks the leaders, the kept leaders and the kept cracks; one block scans them;
//                every leader gets its number after the filter and its offset in loop order, the kept loops their table entry
//   outlines@7   every crack of a loop with a record goes to offset + rank
//   outlines@8   over that list: the turns per block of 1024, and per loop the turns, area2 and the box, folded over the runs of lanes
//                that share a loop (rc_run of rc_reduce.h), one atomic per run and word
//   outlines@9   two launches: one block scans the turns and the loops' vertex counts (vertex offsets, what is written); then every
//                turn crack of a loop that is stored whole writes its vertex and the place of the loop's next one
//   outlines@10  records, the zero tails and the summary
// and the primitives are one more, outlines@11.  Since places are in key order the smallest place is the smallest key.  A round that
// finds that the round before it changed nothing returns at once (option "outlines_early"): no smaller key arrived anywhere means
// every window already holds its loop's smallest, no pointer left means every rank is final.

#include <limits.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define OL_SEG RC_BLOCK                 // pixels of a row a block of the two launches over pixels owns
#define OL_PASSES 4                     // passes of RC_BLOCK a block of the scans over cracks makes
#define OL_CHUNK (RC_BLOCK * OL_PASSES)
#define OL_ROUNDS_MAX 25
#define OL_KEY 0x7fffffffu
enum { OL_P_SIDES, OL_P_COMPACT, OL_P_LINK, OL_P_LEADER, OL_P_CUT, OL_P_RANK, OL_P_NUMBER, OL_P_SCATTER, OL_P_MEASURE, OL_P_VERTS, OL_P_CLOSE, OL_P_PRIMS };
static_assert(OL_P_PRIMS < RC_MAX_LEVELS, "a profile id is kind * RC_MAX_LEVELS + level: a level beyond it is another kind's, or no one's");
static_assert(RC_BLOCK == 256, "a block is four waves");
static_assert((1ll << OL_ROUNDS_MAX) >= RC_OUTLINES_MAX_CRACKS, "rounds = ceil(log2(max_cracks)) fits the hand-over words");
static_assert(4ll * RC_OUTLINES_MAX_SIDE * RC_OUTLINES_MAX_SIDE < (1ll << 30), "a key leaves bit 31 to the turn and fits int32");
static_assert(RC_OUTLINES_MAX_SIDE <= RC_DRAW_COORD_MAX && RC_OUTLINES_MAX_VERTICES <= RC_DRAW_MAX_PRIMS, "the primitives can be drawn");
static_assert(sizeof(rc_outline_loop) == 56 && sizeof(rc_outlines_params) == 32, "the records of include/rcflow.h have the sizes the mirrors give them");
static_assert(RC_OUTLINES_SUMMARY == 8, "the words of a summary");

struct OlCtl {                          // written by the launches in this order: the block scan, the loop scan and numbers, the scatter, the vertex scan
    int ncracks, overflow;
    int loops, kept, kept_cracks;       // the loop scan
    int cut;                            // the cracks of the loops that get a record: the length of the list in loop order
    int verts_kept;                     // the scatter
    int nrec, verts_written;            // the vertex scan
    int pad[7];
    int lact[32], lpar[32];             // leader round r works when lact[r]; it reads pair[lpar[r]]
    int ract[32], rpar[32];             // the same of the rank rounds
};
struct OlLoop {                         // 48 bytes; set up by the loop numbers, added into by the measures, voff by the vertex scan
    int key, off, len, verts;
    int x0, y0, x1, y1;
    long long area2;
    int voff, pad;
};
static_assert(sizeof(OlLoop) == 48 && sizeof(OlCtl) == 64 + 4 * 128, "layouts");

struct OlArgs {
    const int32_t* lab; size_t lab_step;           // one of the two
    const uint8_t* mask; size_t mask_step;
    int w, h, segs, conn, min_cracks, max_cracks, max_loops, max_vertices, rounds, early;
    uint8_t* bits; int* base;
    int* blkcnt; int* blkbase; int* part;          // part: 3 ints a block of OL_CHUNK cracks (the loops), then 1 (the turns)
    unsigned* kt; int* succ; int* lead;
    int2* pair[2];
    unsigned* okt; int* ok;
    OlLoop* loops; OlCtl* ctl; int* vnext;
    long long* summary; rc_outline_loop* recs; int* verts;       // the state's copy
    long long* summary2; rc_outline_loop* recs2; int* verts2;    // the caller's, or null
    long long pushes;
};

__device__ __forceinline__ int ol_label(const OlArgs& a, int x, int y) {    // 0 outside the picture
    if ((unsigned)x >= (unsigned)a.w || (unsigned)y >= (unsigned)a.h) return 0;
    return a.lab ? *(const int32_t*)((const char*)a.lab + (size_t)y * a.lab_step + 4 * (size_t)x) : (a.mask[(size_t)y * a.mask_step + x] != 0);
}
// the cracks of the push: none when they overflowed
__device__ __forceinline__ int ol_count(const OlArgs& a) { return a.ctl->overflow ? 0 : a.ctl->ncracks; }

// exclusive scan over the block's threads; every thread calls it.  s_w: RC_BLOCK / 64 ints of LDS
__device__ __forceinline__ int ol_block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                          // whoever still reads s_w from the call before
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < RC_BLOCK / 64; i++) { before += i < wv ? s_w[i] : 0; total += s_w[i]; }
    return before + inc - v;
}
__device__ __forceinline__ int ol_block_sum(int v, int* s_w) {
    v = rc_wave_sum_lane0(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < RC_BLOCK / 64; i++) t += s_w[i];
    return t;
}
// the least / largest v over the lane's run from the lane on (rc_run_sum's shape)
__device__ __forceinline__ int ol_run_min(int v, int lane, int end) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(v, o, 64);
        if (lane + o <= end) v = min(v, t);
    }
    return v;
}
__device__ __forceinline__ int ol_run_max(int v, int lane, int end) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(v, o, 64);
        if (lane + o <= end) v = max(v, t);
    }
    return v;
}

// the labels of the block's 256 pixels of row y with a one-pixel halo, 0 outside the picture: t[3][OL_SEG + 2]
__device__ __forceinline__ void ol_stage(const OlArgs& a, int xb, int y, int (*t)[OL_SEG + 2]) {
    for (int i = threadIdx.x; i < 3 * (OL_SEG + 2); i += RC_BLOCK) {
        const int r = i / (OL_SEG + 2), c = i - r * (OL_SEG + 2);
        t[r][c] = ol_label(a, xb + c - 1, y + r - 1);
    }
    __syncthreads();
}
// bit s: side s of the pixel at column c of the tile's middle row is a crack
__device__ __forceinline__ int ol_sides(const int (*t)[OL_SEG + 2], int c) {
    const int L = t[1][c];
    if (!L) return 0;
    return (t[0][c] != L ? 1 : 0) | (t[1][c + 1] != L ? 2 : 0) | (t[2][c] != L ? 4 : 0) | (t[1][c - 1] != L ? 8 : 0);
}

// ============================================================================ outlines@0: sides, block counts
__global__ __launch_bounds__(RC_BLOCK) void k_ol_flag(const OlArgs a) {
    __shared__ int t[3][OL_SEG + 2];
    __shared__ int s_w[RC_BLOCK / 64];
    const int tid = threadIdx.x, xb = blockIdx.x * OL_SEG, x = xb + tid, y = blockIdx.y;
    ol_stage(a, xb, y, t);
    const int b = x < a.w ? ol_sides(t, tid + 1) : 0;
    if (x < a.w) a.bits[(size_t)y * a.w + x] = (uint8_t)b;
    // the wave's cracks: four ballots, four population counts
    const int n = __popcll(__ballot(b & 1)) + __popcll(__ballot(b & 2)) + __popcll(__ballot(b & 4)) + __popcll(__ballot(b & 8));
    if ((tid & 63) == 0) s_w[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) a.blkcnt[blockIdx.y * a.segs + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one block: exclusive scan of v[0..n) into o[0..n) (o may be v), -> the total in every thread
__device__ __forceinline__ int ol_scan_array(const int* v, int* o, int n, int* s_w) {
    int carry = 0;
    for (int b = 0; b < n; b += RC_BLOCK) {                   // uniform trip count
        const int i = b + threadIdx.x;
        const int x = i < n ? v[i] : 0;
        int total;
        const int e = ol_block_scan(x, s_w, total);
        if (i < n) o[i] = carry + e;
        carry += total;
    }
    return carry;
}

// ============================================================================ outlines@0: the scan of the block counts
__global__ __launch_bounds__(RC_BLOCK) void k_ol_blockscan(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    const int total = ol_scan_array(a.blkcnt, a.blkbase, a.segs * a.h, s_w);
    const int tid = threadIdx.x;
    OlCtl* c = a.ctl;
    if (tid < 32) {
        c->lact[tid] = tid == 0; c->lpar[tid] = 0;
        c->ract[tid] = tid == 0; c->rpar[tid] = 0;
    }
    if (tid == 0) {
        c->ncracks = total; c->overflow = total > a.max_cracks;
        c->loops = c->kept = c->kept_cracks = c->cut = c->verts_kept = c->nrec = c->verts_written = 0;
    }
}

// ============================================================================ outlines@1: the cracks in key order
__global__ __launch_bounds__(RC_BLOCK) void k_ol_compact(const OlArgs a) {
    __shared__ int t[3][OL_SEG + 2];
    __shared__ int s_w[RC_BLOCK / 64];
    if (a.ctl->overflow) return;
    const int tid = threadIdx.x, xb = blockIdx.x * OL_SEG, x = xb + tid, y = blockIdx.y, w = a.w, c = tid + 1;
    ol_stage(a, xb, y, t);
    const int b = x < w ? ol_sides(t, c) : 0;
    int total;
    const int base = a.blkbase[blockIdx.y * a.segs + blockIdx.x] + ol_block_scan(__popc(b), s_w, total);
    if (x >= w) return;
    const int pix = y * w + x;
    a.base[pix] = base;
    if (!b) return;
    const int L = t[1][c];
    // side s: d = (DX[s], DY[s]) the crack's direction, the step across it is d of side s + 3
    const int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        if (!(b & (1 << s))) continue;
        const int dx = DX[s], dy = DY[s], ax = DX[(s + 3) & 3], ay = DY[(s + 3) & 3];
        const bool sr = t[1 + dy][c + dx] == L, sl = t[1 + dy + ay][c + dx + ax] == L;      // same(R), same(Lp); L != 0, outside is 0
        int turn;                                             // -1 left, 0 straight, 1 right
        if (a.conn == 8) turn = sl ? -1 : sr ? 0 : 1;
        else turn = !sr ? 1 : sl ? -1 : 0;
        int sk;
        if (turn < 0) sk = ((y + dy + ay) * w + x + dx + ax) * 4 + ((s + 3) & 3);
        else if (turn == 0) sk = ((y + dy) * w + x + dx) * 4 + s;
        else sk = pix * 4 + ((s + 1) & 3);
        const int i = base + __popc(b & ((1 << s) - 1));
        a.kt[i] = (unsigned)(pix * 4 + s) | (turn ? 0x80000000u : 0u);
        a.succ[i] = sk;
    }
}

// ============================================================================ outlines@2: the successor's place
__global__ __launch_bounds__(RC_BLOCK) void k_ol_link(const OlArgs a) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= ol_count(a)) return;
    const int sk = a.succ[i], q = sk >> 2, s = sk & 3;
    const int j = a.base[q] + __popc(a.bits[q] & ((1 << s) - 1));
    a.succ[i] = j;
    a.pair[0][i] = make_int2(j, i);
}

// Sets the word when any thread of the block says so; every thread calls it.  One thread a block looks first and stores only while the
// word is still clear: with a store per wave, the 32 K waves of 2 M cracks queued at the one word's L2 channel and a round took 460 us
// instead of 26 (profiles/outlines_kernel_summary.md)
__device__ __forceinline__ void ol_raise(int* word, bool any) {
    if (__syncthreads_or(any) && threadIdx.x == 0 && !__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_store(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================================ outlines@3: a leader round
__global__ __launch_bounds__(RC_BLOCK) void k_ol_leader(const OlArgs a, int r) {
    OlCtl* c = a.ctl;
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x, par = c->lpar[r];
    if (a.early && !c->lact[r]) {                             // the round before changed nothing: the result stays where it is
        if (i == 0) c->lpar[r + 1] = par;
        return;
    }
    if (i == 0) c->lpar[r + 1] = par ^ 1;
    bool changed = false;
    if (i < ol_count(a)) {
        const int2* src = a.pair[par];
        const int2 p = src[i], q = src[p.x];
        const int m = min(p.y, q.y);
        a.pair[par ^ 1][i] = make_int2(q.x, m);
        changed = m != p.y;
    }
    ol_raise(&c->lact[r + 1], changed);
}

// ============================================================================ outlines@4: the cut before the leader
__global__ __launch_bounds__(RC_BLOCK) void k_ol_cut(const OlArgs a) {
    OlCtl* c = a.ctl;
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x, par = c->lpar[a.rounds];
    if (i == 0) c->rpar[0] = par ^ 1;
    if (i >= ol_count(a)) return;
    const int m = a.pair[par][i].y, j = a.succ[i];
    a.lead[i] = m;
    a.pair[par ^ 1][i] = j == m ? make_int2(-1, 0) : make_int2(j, 1);
}

// ============================================================================ outlines@5: a rank round
__global__ __launch_bounds__(RC_BLOCK) void k_ol_rank(const OlArgs a, int r) {
    OlCtl* c = a.ctl;
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x, par = c->rpar[r];
    if (a.early && !c->ract[r]) {
        if (i == 0) c->rpar[r + 1] = par;
        return;
    }
    if (i == 0) c->rpar[r + 1] = par ^ 1;
    bool more = false;
    if (i < ol_count(a)) {
        const int2* src = a.pair[par];
        int2 p = src[i];
        if (p.x >= 0) {
            const int2 q = src[p.x];
            p = make_int2(q.x, p.y + q.y);
        }
        a.pair[par ^ 1][i] = p;
        more = p.x >= 0;
    }
    ol_raise(&c->ract[r + 1], more);
}

// ============================================================================ outlines@6: the loops numbered
// of crack i: whether it leads a loop, whether that loop is kept, and the loop's length when it is
__device__ __forceinline__ void ol_leader_of(const OlArgs& a, const int2* rank, int i, int n, int& lead, int& keep, int& len) {
    lead = keep = len = 0;
    if (i >= n || a.lead[i] != i) return;
    lead = 1;
    len = rank[i].y + 1;                                      // the leader is the farthest from the end
    keep = len >= a.min_cracks;
}

__global__ __launch_bounds__(RC_BLOCK) void k_ol_loop_part(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    const int n = ol_count(a), b0 = blockIdx.x * OL_CHUNK;
    if (b0 >= n) return;
    const int2* rank = a.pair[a.ctl->rpar[a.rounds]];
    int s0 = 0, s1 = 0, s2 = 0;
    for (int p = 0; p < OL_PASSES; p++) {
        int lead, keep, len;
        ol_leader_of(a, rank, b0 + p * RC_BLOCK + threadIdx.x, n, lead, keep, len);
        s0 += lead; s1 += keep; s2 += keep ? len : 0;
    }
    s0 = ol_block_sum(s0, s_w); s1 = ol_block_sum(s1, s_w); s2 = ol_block_sum(s2, s_w);
    if (threadIdx.x == 0) { int* o = a.part + 3 * blockIdx.x; o[0] = s0; o[1] = s1; o[2] = s2; }
}

__global__ __launch_bounds__(RC_BLOCK) void k_ol_loop_scan(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    const int n = ol_count(a), nb = (n + OL_CHUNK - 1) / OL_CHUNK;
    int carry[3] = {0, 0, 0};
    for (int b = 0; b < nb; b += RC_BLOCK) {
        const int i = b + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int x = i < nb ? a.part[3 * i + k] : 0;
            int total;
            const int e = ol_block_scan(x, s_w, total);
            if (i < nb) a.part[3 * i + k] = carry[k] + e;
            carry[k] += total;
        }
    }
    if (threadIdx.x == 0) {
        OlCtl* c = a.ctl;
        c->loops = carry[0]; c->kept = carry[1]; c->kept_cracks = carry[2];
        c->cut = carry[2];                                    // the numbering makes it less when more loops are kept than get a record
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_ol_loop_number(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    const int n = ol_count(a), b0 = blockIdx.x * OL_CHUNK;
    if (b0 >= n) return;
    const int par = a.ctl->rpar[a.rounds];
    const int2* rank = a.pair[par];
    int2* num = a.pair[par ^ 1];                              // per leader: (number after the filter or -1, offset in loop order)
    int ck = a.part[3 * blockIdx.x + 1], co = a.part[3 * blockIdx.x + 2];
    for (int p = 0; p < OL_PASSES; p++) {
        const int i = b0 + p * RC_BLOCK + threadIdx.x;
        int lead, keep, len, tk, to;
        ol_leader_of(a, rank, i, n, lead, keep, len);
        const int k = ck + ol_block_scan(keep, s_w, tk), off = co + ol_block_scan(keep ? len : 0, s_w, to);
        ck += tk; co += to;
        if (!lead) continue;
        num[i] = keep ? make_int2(k, off) : make_int2(-1, 0);
        if (!keep) continue;
        if (k < a.max_loops) {
            OlLoop q;
            q.key = (int)(a.kt[i] & OL_KEY); q.off = off; q.len = len; q.verts = 0;
            q.x0 = INT_MAX; q.y0 = INT_MAX; q.x1 = -1; q.y1 = -1; q.area2 = 0; q.voff = 0; q.pad = 0;
            a.loops[k] = q;
        } else if (k == a.max_loops) {
            a.ctl->cut = off;
        }
    }
}

// ============================================================================ outlines@7: the cracks in loop order
__global__ __launch_bounds__(RC_BLOCK) void k_ol_scatter(const OlArgs a) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x, n = ol_count(a);
    if (blockIdx.x * RC_BLOCK >= n) return;
    const int par = a.ctl->rpar[a.rounds];
    const int2* rank = a.pair[par];
    const int2* num = a.pair[par ^ 1];
    bool turn = false;
    if (i < n) {
        const int L = a.lead[i];
        const int2 q = num[L];
        if (q.x >= 0) {
            const unsigned v = a.kt[i];
            turn = v >> 31;
            if (q.x < a.max_loops) {
                const int pos = q.y + rank[L].y - rank[i].y;  // offset + length - 1 - distance to the end
                a.okt[pos] = v;
                a.ok[pos] = q.x;
            }
        }
    }
    const int nt = __syncthreads_count(turn);                 // the vertices of every kept loop, with or without a record: one add a block
    if (nt && threadIdx.x == 0) atomicAdd(&a.ctl->verts_kept, nt);
}

// the second corner of the crack with key `key`
__device__ __forceinline__ void ol_corner(int key, int w, int& bx, int& by, int& ax, int& ay) {
    const int s = key & 3, p = key >> 2, x = p % w, y = p / w;
    ax = x + (s == 1 || s == 2); ay = y + (s >= 2);
    bx = x + (s <= 1); by = y + (s == 1 || s == 2);
}

// ============================================================================ outlines@8: turns per block; turns, area and box per loop
__global__ __launch_bounds__(RC_BLOCK) void k_ol_measure(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    const int cut = a.ctl->overflow ? 0 : a.ctl->cut, b0 = blockIdx.x * OL_CHUNK, lane = threadIdx.x & 63;
    if (b0 >= cut) return;
    int turns = 0;
    for (int p = 0; p < OL_PASSES; p++) {
        const int pos = b0 + p * RC_BLOCK + threadIdx.x;
        if (b0 + p * RC_BLOCK >= cut) break;                  // uniform over the block
        int k = -1, t = 0, bx = 0, by = 0;
        long long a2 = 0;
        if (pos < cut) {
            const unsigned v = a.okt[pos];
            int ax, ay;
            k = a.ok[pos];
            t = v >> 31;
            ol_corner((int)(v & OL_KEY), a.w, bx, by, ax, ay);
            a2 = (long long)ax * by - (long long)bx * ay;
        }
        turns += t;
        bool head;
        const int end = rc_run(k, lane, head);
        const long long sa = rc_run_sum(a2, lane, end);
        const int st = (int)rc_run_sum((long long)t, lane, end);
        const int x0 = ol_run_min(bx, lane, end), y0 = ol_run_min(by, lane, end), x1 = ol_run_max(bx, lane, end), y1 = ol_run_max(by, lane, end);
        if (head && k >= 0) {                                 // every corner of a loop is the second corner of one of its cracks
            OlLoop* q = a.loops + k;
            if (sa) atomicAdd((unsigned long long*)&q->area2, (unsigned long long)sa);
            if (st) atomicAdd(&q->verts, st);
            atomicMin(&q->x0, x0); atomicMin(&q->y0, y0); atomicMax(&q->x1, x1); atomicMax(&q->y1, y1);
        }
    }
    turns = ol_block_sum(turns, s_w);
    if (threadIdx.x == 0) a.part[blockIdx.x] = turns;
}

// ============================================================================ outlines@9: the scan of turns, vertex offsets
__global__ __launch_bounds__(RC_BLOCK) void k_ol_vert_scan(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    OlCtl* c = a.ctl;
    if (c->overflow) return;
    (void)ol_scan_array(a.part, a.part, (c->cut + OL_CHUNK - 1) / OL_CHUNK, s_w);
    const int nrec = min(c->kept, a.max_loops);
    int carry = 0, written = 0;
    for (int b = 0; b < nrec; b += RC_BLOCK) {
        const int k = b + threadIdx.x;
        const int v = k < nrec ? a.loops[k].verts : 0;
        int total;
        const int off = carry + ol_block_scan(v, s_w, total);
        if (k < nrec) {
            a.loops[k].voff = off;
            if (off + v <= a.max_vertices) written = off + v;  // offsets only grow: the stored loops are the first ones
        }
        carry += total;
    }
    written = rc_wave_max_all(written);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = written;
    __syncthreads();
    if (threadIdx.x == 0) { c->nrec = nrec; c->verts_written = max(max(s_w[0], s_w[1]), max(s_w[2], s_w[3])); }
}

// ============================================================================ outlines@9: the vertices
__global__ __launch_bounds__(RC_BLOCK) void k_ol_vertices(const OlArgs a) {
    __shared__ int s_w[RC_BLOCK / 64];
    const int cut = a.ctl->overflow ? 0 : a.ctl->cut, b0 = blockIdx.x * OL_CHUNK;
    if (b0 >= cut) return;
    int carry = a.part[blockIdx.x];
    for (int p = 0; p < OL_PASSES; p++) {
        const int pos = b0 + p * RC_BLOCK + threadIdx.x;
        if (b0 + p * RC_BLOCK >= cut) break;                  // uniform over the block
        const unsigned v = pos < cut ? a.okt[pos] : 0u;
        const int t = v >> 31;
        int total;
        const int at = carry + ol_block_scan(t, s_w, total); // the turns before this crack in loop order: the vertex's place
        carry += total;
        if (!t) continue;
        const OlLoop& q = a.loops[a.ok[pos]];
        if (q.voff + q.verts > a.max_vertices) continue;
        int bx, by, ax, ay;
        ol_corner((int)(v & OL_KEY), a.w, bx, by, ax, ay);
        *(int2*)(a.verts + 2 * (size_t)at) = make_int2(bx, by);
        if (a.verts2) { a.verts2[2 * (size_t)at] = bx; a.verts2[2 * (size_t)at + 1] = by; }
        a.vnext[at] = at + 1 == q.voff + q.verts ? q.voff : at + 1;
    }
}

// ============================================================================ outlines@10: records, zero tails, summary
__global__ __launch_bounds__(RC_BLOCK) void k_ol_close(const OlArgs a) {
    const OlCtl* c = a.ctl;
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool over = c->overflow != 0;
    const int nrec = over ? 0 : c->nrec, written = over ? 0 : c->verts_written;
    if (i < a.max_loops) {
        rc_outline_loop o;
        memset(&o, 0, sizeof(o));
        if (i < nrec) {
            const OlLoop q = a.loops[i];
            const int p = q.key >> 2;
            o.x = p % a.w; o.y = p / a.w;
            o.label = ol_label(a, o.x, o.y);
            o.cracks = q.len; o.verts = q.verts;
            o.x0 = q.x0; o.y0 = q.y0; o.x1 = q.x1; o.y1 = q.y1; o.area2 = q.area2;
            const bool stored = q.voff + q.verts <= a.max_vertices;
            o.offset = stored ? q.voff : -1;
            o.flags = (q.area2 < 0 ? RC_OUTLINE_HOLE : 0) | (stored ? 0 : RC_OUTLINE_NOVERTS);
        }
        a.recs[i] = o;
        if (a.recs2) a.recs2[i] = o;
    }
    if (i >= written && i < a.max_vertices) {
        *(int2*)(a.verts + 2 * (size_t)i) = make_int2(0, 0);
        if (a.verts2) { a.verts2[2 * (size_t)i] = 0; a.verts2[2 * (size_t)i + 1] = 0; }
    }
    if (i < RC_OUTLINES_SUMMARY) {
        const long long s[RC_OUTLINES_SUMMARY] = {c->ncracks, over ? 0 : c->loops, over ? 0 : c->kept, nrec, over ? 0 : c->verts_kept, written, over, a.pushes};
        a.summary[i] = s[i];
        if (a.summary2) a.summary2[i] = s[i];
    }
}

// ============================================================================ outlines@11: the primitives
__global__ __launch_bounds__(RC_BLOCK) void k_ol_prims(const long long* summary, const int* verts, const int* vnext, int max_vertices, int w, int h,
                                                        uint32_t color, int thickness, rc_draw_prim* out) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= max_vertices) return;
    rc_draw_prim p;
    memset(&p, 0, sizeof(p));
    if (i < summary[5]) {
        const int j = vnext[i];
        p.kind = RC_DRAW_LINE; p.size = thickness; p.color = color;
        p.x0 = min(verts[2 * i], w - 1); p.y0 = min(verts[2 * i + 1], h - 1);
        p.x1 = min(verts[2 * j], w - 1); p.y1 = min(verts[2 * j + 1], h - 1);
    }
    out[i] = p;
}

// ============================================================================ host side
void rc_state_free(RcOutlines& v) {
    for (RcBuf* b : {&v.bits, &v.base, &v.blk, &v.kt, &v.succ, &v.lead, &v.pair[0], &v.pair[1], &v.okt, &v.ok, &v.loops, &v.ctl, &v.vnext, &v.out})
        rc_buf_free(*b);
    rc_fence_free(v.zf);
    v = RcOutlines();
}

// open and reset: the kept records, vertices and summary, the push count.  Every other buffer is written by a push before it is read
int rc_state_zero(RcSlot& s, RcOutlines& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.out});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static long long* ol_summary(const RcOutlines& v) { return (long long*)v.out.p; }
static rc_outline_loop* ol_records(const RcOutlines& v) { return (rc_outline_loop*)((char*)v.out.p + 8 * RC_OUTLINES_SUMMARY); }
static int* ol_verts(const RcOutlines& v) { return (int*)(ol_records(v) + v.prm.max_loops); }
static int ol_segs(int w) { return (w + OL_SEG - 1) / OL_SEG; }
static int ol_rounds(int max_cracks) {
    int r = 0;
    while ((1ll << r) < max_cracks) r++;
    return r;
}

static const char* ol_prm_text = "connectivity 4 | 8, min_cracks >= 1, max_cracks 4..2^25, max_loops 1..2^20, max_vertices 4..2^24, flags 0, the pad words zero";
static bool ol_prm_ok(const rc_outlines_params& p) {
    return (p.connectivity == 4 || p.connectivity == 8) && p.min_cracks >= 1 && p.max_cracks >= 4 && p.max_cracks <= RC_OUTLINES_MAX_CRACKS &&
           p.max_loops >= 1 && p.max_loops <= RC_OUTLINES_MAX_LOOPS && p.max_vertices >= 4 && p.max_vertices <= RC_OUTLINES_MAX_VERTICES && !p.flags &&
           !p.pad[0] && !p.pad[1];
}

extern "C" int rcflow_outlines_open(rc_ctx* ctx, int stream, int w, int h, const rc_outlines_params* prm) {
    static const char* who = "rcflow_outlines_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad picture size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (!ol_prm_ok(*prm)) { rc_set_error("%s: %s", who, ol_prm_text); return RC_EINVAL; }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    if (w > RC_OUTLINES_MAX_SIDE || h > RC_OUTLINES_MAX_SIDE) {
        rc_set_error("%s: %d x %d is beyond %d a side", who, w, h, RC_OUTLINES_MAX_SIDE);
        return RC_ESIZE;
    }
    RcOutlines n;
    n.w = w; n.h = h; n.prm = *prm; n.rounds = ol_rounds(prm->max_cracks);
    RC_HIP(hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, nb = (size_t)ol_segs(w) * h, mc = (size_t)prm->max_cracks, np = (mc + OL_CHUNK - 1) / OL_CHUNK;
    rc = rc_buf_ensure(n.bits, px);
    if (!rc) rc = rc_buf_ensure(n.base, px * 4);
    if (!rc) rc = rc_buf_ensure(n.blk, (2 * nb + 3 * np) * 4);
    for (RcBuf* b : {&n.kt, &n.succ, &n.lead, &n.okt, &n.ok})
        if (!rc) rc = rc_buf_ensure(*b, mc * 4);
    for (RcBuf* b : {&n.pair[0], &n.pair[1]})
        if (!rc) rc = rc_buf_ensure(*b, mc * 8);
    if (!rc) rc = rc_buf_ensure(n.loops, (size_t)prm->max_loops * sizeof(OlLoop));
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(OlCtl));
    if (!rc) rc = rc_buf_ensure(n.vnext, (size_t)prm->max_vertices * 4);
    if (!rc) rc = rc_buf_ensure(n.out, 8 * RC_OUTLINES_SUMMARY + (size_t)prm->max_loops * sizeof(rc_outline_loop) + (size_t)prm->max_vertices * 8);
    return rc_state_install(*s, s->ol, n, rc);
}

extern "C" int rcflow_outlines_push_dev(rc_ctx* ctx, int stream, const int32_t* d_labels, size_t labels_step, const uint8_t* d_mask, size_t mask_step,
                                        rc_outline_loop* d_loops, int32_t* d_verts, long long* d_summary) {
    static const char* who = "rcflow_outlines_push_dev";
    RcSlot* s; RcOutlines* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ol, who, s, vp)) return rc;
    RcOutlines& v = *vp;
    const int w = v.w, h = v.h;
    const rc_outlines_params& q = v.prm;
    if (!d_labels == !d_mask) { rc_set_error("%s: exactly one of d_labels and d_mask", who); return RC_EINVAL; }
    RcArgs ar(who, w, h);
    ar.image("d_labels", d_labels, labels_step, 4, 4, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_mask", d_mask, mask_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.array("d_loops", d_loops, (size_t)q.max_loops * sizeof(rc_outline_loop), 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_verts", d_verts, (size_t)q.max_vertices * 8, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, RC_OUTLINES_SUMMARY * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    OlArgs a;
    memset(&a, 0, sizeof(a));
    a.lab = d_labels; a.lab_step = labels_step; a.mask = d_mask; a.mask_step = mask_step;
    a.w = w; a.h = h; a.segs = ol_segs(w); a.conn = q.connectivity; a.min_cracks = q.min_cracks; a.max_cracks = q.max_cracks;
    a.max_loops = q.max_loops; a.max_vertices = q.max_vertices; a.rounds = v.rounds; a.early = ctx->outlines_early;
    const size_t nb = (size_t)a.segs * h;
    a.bits = (uint8_t*)v.bits.p; a.base = (int*)v.base.p;
    a.blkcnt = (int*)v.blk.p; a.blkbase = a.blkcnt + nb; a.part = a.blkbase + nb;
    a.kt = (unsigned*)v.kt.p; a.succ = (int*)v.succ.p; a.lead = (int*)v.lead.p;
    a.pair[0] = (int2*)v.pair[0].p; a.pair[1] = (int2*)v.pair[1].p;
    a.okt = (unsigned*)v.okt.p; a.ok = (int*)v.ok.p;
    a.loops = (OlLoop*)v.loops.p; a.ctl = (OlCtl*)v.ctl.p; a.vnext = (int*)v.vnext.p;
    a.summary = ol_summary(v); a.recs = ol_records(v); a.verts = ol_verts(v);
    a.summary2 = d_summary; a.recs2 = d_loops; a.verts2 = d_verts;
    a.pushes = v.pushes + 1;
    const double px = (double)w * h, mc = (double)q.max_cracks, in_px = d_labels ? 4. : 1.;
    const dim3 blk(RC_BLOCK), tiles(a.segs, h), per_crack((q.max_cracks + RC_BLOCK - 1) / RC_BLOCK), per_chunk((q.max_cracks + OL_CHUNK - 1) / OL_CHUNK);
    const int tail = q.max_loops > q.max_vertices ? q.max_loops : q.max_vertices;
    // the bytes are those of a picture whose cracks fill max_cracks: what the slot was opened for
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_SIDES, px * (in_px + 1.));
      hipLaunchKernelGGL(k_ol_flag, tiles, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_SIDES, 8. * nb);
      hipLaunchKernelGGL(k_ol_blockscan, dim3(1), blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_COMPACT, px * (in_px + 4.) + 8. * mc);
      hipLaunchKernelGGL(k_ol_compact, tiles, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_LINK, 21. * mc);
      hipLaunchKernelGGL(k_ol_link, per_crack, blk, 0, s->cur, a); }
    for (int r = 0; r < v.rounds; r++) {
        RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_LEADER, 24. * mc);
        hipLaunchKernelGGL(k_ol_leader, per_crack, blk, 0, s->cur, a, r);
    }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_CUT, 24. * mc);
      hipLaunchKernelGGL(k_ol_cut, per_crack, blk, 0, s->cur, a); }
    for (int r = 0; r < v.rounds; r++) {
        RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_RANK, 24. * mc);
        hipLaunchKernelGGL(k_ol_rank, per_crack, blk, 0, s->cur, a, r);
    }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_NUMBER, 12. * mc);
      hipLaunchKernelGGL(k_ol_loop_part, per_chunk, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_NUMBER, 24. * per_chunk.x);
      hipLaunchKernelGGL(k_ol_loop_scan, dim3(1), blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_NUMBER, 20. * mc);
      hipLaunchKernelGGL(k_ol_loop_number, per_chunk, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_SCATTER, 40. * mc);
      hipLaunchKernelGGL(k_ol_scatter, per_crack, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_MEASURE, 8. * mc);
      hipLaunchKernelGGL(k_ol_measure, per_chunk, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_VERTS, 8. * per_chunk.x + 8. * q.max_loops);
      hipLaunchKernelGGL(k_ol_vert_scan, dim3(1), blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_VERTS, 8. * mc + (d_verts ? 20. : 12.) * q.max_vertices);
      hipLaunchKernelGGL(k_ol_vertices, per_chunk, blk, 0, s->cur, a); }
    { RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_CLOSE, (48. + (d_loops ? 112. : 56.)) * q.max_loops);
      hipLaunchKernelGGL(k_ol_close, dim3((tail + RC_BLOCK - 1) / RC_BLOCK), blk, 0, s->cur, a); }
    RC_HIP(hipGetLastError());
    v.pushes++;                                               // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_outlines_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, rc_draw_prim* d_prims) {
    static const char* who = "rcflow_outlines_prims_dev";
    RcSlot* s; RcOutlines* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ol, who, s, vp)) return rc;
    RcOutlines& v = *vp;
    if (rc_prims_check(who, d_prims, thickness, 0)) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    RcProfScope ps(ctx, s->cur, RC_K_OUTLINES, OL_P_PRIMS, (double)v.prm.max_vertices * (12. + sizeof(rc_draw_prim)));
    hipLaunchKernelGGL(k_ol_prims, dim3((v.prm.max_vertices + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, ol_summary(v), ol_verts(v),
                       (const int*)v.vnext.p, v.prm.max_vertices, v.w, v.h, color, thickness, d_prims);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_outlines_read(rc_ctx* ctx, int stream, rc_outline_loop* loops, int cap, int* n, int32_t* verts, int vcap, int* nv,
                                    long long summary[RC_OUTLINES_SUMMARY]) {
    static const char* who = "rcflow_outlines_read";
    RcSlot* s; RcOutlines* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ol, who, s, vp)) return rc;
    RcOutlines& v = *vp;
    if (cap < 0 || vcap < 0 || (cap && !loops) || (vcap && !verts)) { rc_set_error("%s: a bad buffer", who); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    long long sum[RC_OUTLINES_SUMMARY];
    RC_HIP(hipMemcpyAsync(sum, ol_summary(v), sizeof(sum), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    const int take = (int)(sum[3] < cap ? sum[3] : cap), vtake = (int)(sum[5] < vcap ? sum[5] : vcap);
    if (take) RC_HIP(hipMemcpyAsync(loops, ol_records(v), (size_t)take * sizeof(rc_outline_loop), hipMemcpyDeviceToHost, s->cur));
    if (vtake) RC_HIP(hipMemcpyAsync(verts, ol_verts(v), (size_t)vtake * 8, hipMemcpyDeviceToHost, s->cur));
    if (take || vtake) RC_HIP(hipStreamSynchronize(s->cur));
    if (n) *n = (int)sum[3];
    if (nv) *nv = (int)sum[5];
    if (summary) memcpy(summary, sum, sizeof(sum));
    return RC_OK;
}

extern "C" int rcflow_outlines_set(rc_ctx* ctx, int stream, int min_cracks) {
    RcSlot* s; RcOutlines* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ol, "rcflow_outlines_set", s, vp)) return rc;
    if (min_cracks < 1) { rc_set_error("rcflow_outlines_set: min_cracks >= 1"); return RC_EINVAL; }
    vp->prm.min_cracks = min_cracks;
    return RC_OK;
}

extern "C" int rcflow_outlines_info(rc_ctx* ctx, int stream, rc_outlines_info* info) {
    RcSlot* s; RcOutlines* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ol, "rcflow_outlines_info", s, vp)) return rc;
    const RcOutlines& v = *vp;
    if (!info) { rc_set_error("rcflow_outlines_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->rounds = v.rounds; info->launches_per_push = RC_OUTLINES_FIXED_LAUNCHES + 2 * v.rounds;
    info->pushes = v.pushes;
    info->device_bytes = v.bits.bytes + v.base.bytes + v.blk.bytes + v.kt.bytes + v.succ.bytes + v.lead.bytes + v.pair[0].bytes + v.pair[1].bytes +
                         v.okt.bytes + v.ok.bytes + v.loops.bytes + v.ctl.bytes + v.vnext.bytes + v.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_outlines_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::ol, "rcflow_outlines_reset"); }
extern "C" int rcflow_outlines_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::ol); }
