// track_kernels.hip -- rip tracks (rcflow_tracks_*): the regions of rcflow_regions_push_dev followed from push to push on the
// device.  The contract is the header comment of include/rcflow.h; DESIGN 7h has the reasons.
//
// A push is six launches whatever the labels hold:
//   @0 prepare  the slots that ended in the last push become zero bytes; the overlap table and the merged words are zeroed.
//   @1 overlap  ov[c][t] = pixels with label c and footprint t + 1.  A wave walks 8 rows of 64 pixels and keeps one running
//               (c, t) pair: a __ballot per distinct pair of a row, one atomic when the pair changes, the four waves of a
//               block joined before the last ones.  A full frame on one track is one atomic per block.
//   @2 claim    a block per label: best(c), its overlap; the merged word of every track the label covers enough of.
//   @3 update   a block per slot: the winner among the labels that claimed it, then the record (one thread).
//   @4 births   one block of 1024 threads: ranks of the unclaimed labels and of the free slots by prefix sums, the new
//               records, the two small tables the paint reads, the summary, next_id and the push count.
//   @5 paint    the footprint, the confirmed mask, and the copies of the table and of track_of_label.
// Numbers come from ranks, never from arrival; the only atomics are integer additions into the overlap table.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <string.h>

#include "rc_device.h"
#include "rc_host.h"

#define TK_ROWS 8                       // rows a wave walks
#define TK_WAVES 4                      // waves of a block
#define TK_TILE_H (TK_ROWS * TK_WAVES)
#define TK_BIRTH_BLOCK 1024
#define TK_CONF (1 << 30)               // in the paint's label table: the label's track is confirmed
static_assert(RC_BLOCK == 64 * TK_WAVES, "a block is TK_WAVES waves");
static_assert(RC_TRACKS_MAX <= TK_BIRTH_BLOCK && RC_TRACKS_MAX_REGIONS <= TK_BIRTH_BLOCK, "the births are one block, a thread per label and slot");
static_assert(sizeof(rc_track) == 128, "layout");

struct TkCtl {                          // zeroed by open / reset
    long long issued;                   // next_id - 1
    long long pushes;
};
struct TkTabs {                         // views into RcTracks::aux
    TkCtl* ctl;
    int* best;                          // [max_regions + 1] slot of best(c), or -1
    int* bestov;                        // [max_regions + 1] ov[c][best(c)]
    int* tol;                           // [max_regions + 1] slot + 1 of the label's track (track_of_label)
    int* paint;                         // [max_regions + 1] tol, | TK_CONF when that track is confirmed; 0 beyond R
    int* merged;                        // [max_tracks] some label covers min_overlap pixels of the slot's footprint
    int* keep;                          // [max_tracks] the slot's old footprint stays (used and not ended)
};

__device__ __forceinline__ int tk_R(const long long* regions_summary, int max_regions) {
    const long long v = regions_summary[2];
    return v < 0 ? 0 : v > max_regions ? max_regions : (int)v;
}
__device__ __forceinline__ void tk_means(rc_track& q) {
    q.mean_fx = q.m_sum ? (float)((double)q.fx_sum / 65536.0 / (double)q.m_sum) : 0.f;
    q.mean_fy = q.m_sum ? (float)((double)q.fy_sum / 65536.0 / (double)q.m_sum) : 0.f;
}
// what a track takes from the record of the region it was seen as
__device__ __forceinline__ void tk_geometry(rc_track& q, const rc_region& r) {
    const long long n = r.area;                                          // >= 1 in a record of rcflow_regions_push_dev
    q.area = r.area; q.x0 = r.x0; q.y0 = r.y0; q.x1 = r.x1; q.y1 = r.y1;
    q.px = n > 0 ? (int)((2 * r.sx + n) / (2 * n)) : 0; q.py = n > 0 ? (int)((2 * r.sy + n) / (2 * n)) : 0;
}

// ---------------------------------------------------------------------------- @0
__global__ __launch_bounds__(RC_BLOCK) void k_tk_prepare(rc_track* tab, int max_tracks, int* ov, size_t nov, int* merged) {
    const size_t i0 = (size_t)blockIdx.x * RC_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RC_BLOCK;
    for (size_t i = i0; i < nov; i += stride) ov[i] = 0;
    for (size_t t = i0; t < (size_t)max_tracks; t += stride) {
        merged[t] = 0;
        if (tab[t].flags & RC_TRACK_ENDED) memset(&tab[t], 0, sizeof(rc_track));
    }
}

// ---------------------------------------------------------------------------- @1
__global__ __launch_bounds__(RC_BLOCK) void k_tk_overlap(const int32_t* labels, size_t labels_step, const int* P, int w, int h,
                                                         const long long* regions_summary, int max_regions, int max_tracks, int* ov) {
    __shared__ int s_key[TK_WAVES], s_cnt[TK_WAVES];
    const int lane = threadIdx.x, wv = threadIdx.y, x = blockIdx.x * 64 + lane;
    const int yb = (blockIdx.y * TK_WAVES + wv) * TK_ROWS;
    const int R = tk_R(regions_summary, max_regions);
    int cur = -1, cnt = 0;                                               // the wave's running pair and its pixels (uniform)
    for (int r = 0; r < TK_ROWS; r++) {
        const int y = yb + r;
        if (y >= h) break;
        int key = -1;
        if (x < w) {
            const int c = *(const int32_t*)((const char*)labels + (size_t)y * labels_step + (size_t)x * 4);
            const int p = P[(size_t)y * w + x];
            if (c >= 1 && c <= R && p >= 1 && p <= max_tracks) key = c * max_tracks + (p - 1);
        }
        unsigned long long todo = __ballot(key >= 0);
        while (todo) {
            const int kl = __shfl(key, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(key == kl);
            todo &= ~same;
            if (kl != cur) {
                if (cnt && lane == 0) atomicAdd(ov + cur, cnt);
                cur = kl; cnt = 0;
            }
            cnt += __popcll(same);
        }
    }
    if (lane == 0) { s_key[wv] = cur; s_cnt[wv] = cnt; }
    __syncthreads();
    if (wv == 0 && lane == 0) {
        for (int i = 0; i < TK_WAVES; i++) {
            if (!s_cnt[i]) continue;
            int c = s_cnt[i];
            for (int j = i + 1; j < TK_WAVES; j++)
                if (s_cnt[j] && s_key[j] == s_key[i]) { c += s_cnt[j]; s_cnt[j] = 0; }
            atomicAdd(ov + s_key[i], c);
        }
    }
}

// ---------------------------------------------------------------------------- @2
// the larger overlap, then the smaller id; the slot decides between records that are the same (they never are)
__device__ __forceinline__ bool tk_claim_better(int ov, long long id, int ov2, long long id2) { return ov > ov2 || (ov == ov2 && id < id2); }

__global__ __launch_bounds__(RC_BLOCK) void k_tk_claim(const int* ov, const rc_track* tab, const long long* regions_summary, int max_regions,
                                                       int max_tracks, int min_overlap, TkTabs q) {
    __shared__ int s_ov[TK_WAVES], s_t[TK_WAVES];
    __shared__ long long s_id[TK_WAVES];
    const int c = blockIdx.x, R = tk_R(regions_summary, max_regions);
    if (c < 1 || c > R) {
        if (threadIdx.x == 0) { q.best[c] = -1; q.bestov[c] = 0; q.tol[c] = 0; }
        return;
    }
    int bo = 0, bt = -1;
    long long bid = LLONG_MAX;
    for (int t = threadIdx.x; t < max_tracks; t += RC_BLOCK) {
        const int o = ov[(size_t)c * max_tracks + t];
        if (o < min_overlap) continue;
        const long long id = tab[t].id;
        if (!id) continue;                                               // the footprint never names a free slot
        q.merged[t] = 1;                                                 // every writer stores the same word
        if (bt < 0 || tk_claim_better(o, id, bo, bid)) { bo = o; bid = id; bt = t; }
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        const int o2 = __shfl_xor(bo, s), t2 = __shfl_xor(bt, s);
        const long long id2 = __shfl_xor(bid, s);
        if (t2 >= 0 && (bt < 0 || tk_claim_better(o2, id2, bo, bid))) { bo = o2; bid = id2; bt = t2; }
    }
    if ((threadIdx.x & 63) == 0) { s_ov[threadIdx.x >> 6] = bo; s_id[threadIdx.x >> 6] = bid; s_t[threadIdx.x >> 6] = bt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < TK_WAVES; i++)
            if (s_t[i] >= 0 && (bt < 0 || tk_claim_better(s_ov[i], s_id[i], bo, bid))) { bo = s_ov[i]; bid = s_id[i]; bt = s_t[i]; }
        q.best[c] = bt; q.bestov[c] = bt >= 0 ? bo : 0; q.tol[c] = 0;
    }
}

// ---------------------------------------------------------------------------- @3
__global__ __launch_bounds__(RC_BLOCK) void k_tk_update(rc_track* tab, const rc_region* regions, const long long* regions_summary, int max_regions,
                                                        rc_tracks_params prm, TkTabs q) {
    __shared__ int s_ov[TK_WAVES], s_c[TK_WAVES], s_n[TK_WAVES];
    const int t = blockIdx.x, R = tk_R(regions_summary, max_regions);
    if (!tab[t].id) return;                                              // uniform over the block
    int bo = 0, bc = 0, n = 0;                                           // the winner so far (bc = 0: none), the claims
    for (int c = 1 + threadIdx.x; c <= R; c += RC_BLOCK) {
        if (q.best[c] != t) continue;
        const int o = q.bestov[c];
        n++;
        if (!bc || o > bo) { bo = o; bc = c; }                           // ascending c: the lowest of equals stays
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        const int o2 = __shfl_xor(bo, s), c2 = __shfl_xor(bc, s);
        n += __shfl_xor(n, s);
        if (c2 && (!bc || o2 > bo || (o2 == bo && c2 < bc))) { bo = o2; bc = c2; }
    }
    if ((threadIdx.x & 63) == 0) { s_ov[threadIdx.x >> 6] = bo; s_c[threadIdx.x >> 6] = bc; s_n[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x) return;
    for (int i = 1; i < TK_WAVES; i++) {
        n += s_n[i];
        if (s_c[i] && (!bc || s_ov[i] > bo || (s_ov[i] == bo && s_c[i] < bc))) { bo = s_ov[i]; bc = s_c[i]; }
    }
    rc_track k = tab[t];
    k.age += 1;
    if (bc) {
        const rc_region r = regions[bc - 1];
        k.flags = RC_TRACK_SEEN | (n > 1 ? RC_TRACK_SPLIT : 0);
        k.hits += 1; k.misses = 0; k.label = bc; k.overlap = bo;
        tk_geometry(k, r);
        k.area_sum += r.area; k.fx_sum += r.fx; k.fy_sum += r.fy; k.m_sum += r.area - r.bad;
        q.tol[bc] = t + 1;
    } else {
        k.flags = RC_TRACK_COASTING | (q.merged[t] ? RC_TRACK_MERGED : 0);
        k.misses += 1; k.label = 0; k.overlap = 0;
        if (k.misses > prm.max_misses) k.flags |= RC_TRACK_ENDED;
    }
    if (k.hits >= prm.min_hits) k.flags |= RC_TRACK_CONFIRMED;
    tk_means(k);
    tab[t] = k;
}

// ---------------------------------------------------------------------------- @4
// exclusive rank of a flag over the block's 1024 threads, and the total
__device__ __forceinline__ int tk_rank(bool flag, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int i = 0; i < TK_BIRTH_BLOCK / 64; i++) { before += i < wv ? s_wave[i] : 0; total += s_wave[i]; }
    return before + __popcll(m & ((1ull << lane) - 1));
}
// the five counts of the summary in one word: 12 bits each, a count is at most 1024
#define TK_PACK_BITS 12
static_assert(TK_BIRTH_BLOCK < (1 << TK_PACK_BITS), "a count fits its field");

__global__ __launch_bounds__(TK_BIRTH_BLOCK) void k_tk_births(rc_track* tab, const rc_region* regions, const long long* regions_summary,
                                                              int max_regions, int max_tracks, rc_tracks_params prm, TkTabs q,
                                                              long long* keep_sum, long long* user_sum) {
    __shared__ int s_wave[TK_BIRTH_BLOCK / 64], s_free[TK_BIRTH_BLOCK];
    __shared__ unsigned long long s_pack[TK_BIRTH_BLOCK / 64];
    __shared__ long long s_ctl[2];
    const int i = threadIdx.x, c = i + 1, R = tk_R(regions_summary, max_regions);
    // next_id and the push count as the last push left them: thread 0 alone reads the two words, and alone writes them at
    // the end; everybody else takes them from LDS behind the barriers of the ranks
    if (i == 0) { s_ctl[0] = q.ctl->issued; s_ctl[1] = q.ctl->pushes + 1; }
    // the slot i as the update left it, the label c
    long long id = 0;
    int flags = 0;
    if (i < max_tracks) { id = tab[i].id; flags = tab[i].flags; }
    const bool used = id != 0, ended = used && (flags & RC_TRACK_ENDED), is_free = i < max_tracks && !used;
    int slot1 = c <= R ? q.tol[c] : 0;                                   // slot + 1 of the track that took the label
    const bool orphan = c <= R && !slot1;
    {                                                                    // alive, confirmed, ended, seen, coasting: per wave
        const bool f[5] = {used && !ended, used && !ended && (flags & RC_TRACK_CONFIRMED), ended, used && (flags & RC_TRACK_SEEN),
                           used && (flags & RC_TRACK_COASTING)};
        unsigned long long pack = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) pack |= (unsigned long long)__popcll(__ballot(f[j])) << (TK_PACK_BITS * j);
        if ((i & 63) == 0) s_pack[i >> 6] = pack;
    }
    int nfree, norphan;
    const int frank = tk_rank(is_free, s_wave, nfree);
    const int k = tk_rank(orphan, s_wave, norphan);
    if (is_free) s_free[frank] = i;
    __syncthreads();                                                     // s_free, s_pack and s_ctl are whole
    const int born = norphan < nfree ? norphan : nfree;
    const long long issued = s_ctl[0], push = s_ctl[1];
    bool conf = false;
    if (orphan && k < born) {
        const int slot = s_free[k], b = q.best[c];
        const rc_region* r = regions + (c - 1);
        rc_track* t = tab + slot;                                        // a free slot, all zero bytes: nobody in this launch reads it
        const long long n = r->area, fx = r->fx, fy = r->fy, m = n - r->bad;
        conf = prm.min_hits <= 1;
        t->id = issued + 1 + k; t->parent = b >= 0 ? tab[b].id : 0; t->first_push = push;
        t->area_sum = n; t->fx_sum = fx; t->fy_sum = fy; t->m_sum = m;
        t->slot = slot; t->label = c; t->flags = RC_TRACK_BORN | RC_TRACK_SEEN | (conf ? RC_TRACK_CONFIRMED : 0);
        t->age = 1; t->hits = 1; t->misses = 0; t->overlap = 0;
        tk_geometry(*t, *r);
        t->px0 = t->px; t->py0 = t->py;
        t->mean_fx = m ? (float)((double)fx / 65536.0 / (double)m) : 0.f;
        t->mean_fy = m ? (float)((double)fy / 65536.0 / (double)m) : 0.f;
        slot1 = slot + 1;
        q.tol[c] = slot1;
    } else if (slot1) {
        conf = tab[slot1 - 1].flags & RC_TRACK_CONFIRMED;                // a track the update has seen: not a slot born here
    }
    if (c <= max_regions) q.paint[c] = c > R ? 0 : slot1 ? (slot1 | (conf ? TK_CONF : 0)) : -1;
    if (i < max_tracks) q.keep[i] = used && !ended;
    if (i == 0) {
        unsigned long long pack = 0;
        for (int j = 0; j < TK_BIRTH_BLOCK / 64; j++) pack += s_pack[j];
        long long cnt[5];
        for (int j = 0; j < 5; j++) cnt[j] = (long long)((pack >> (TK_PACK_BITS * j)) & ((1u << TK_PACK_BITS) - 1));
        q.paint[0] = 0;
        q.ctl->issued = issued + born;
        q.ctl->pushes = push;
        const long long s[8] = {cnt[0] + born, cnt[1] + (prm.min_hits <= 1 ? born : 0), (long long)born, cnt[2],
                                cnt[3] + born, cnt[4], (long long)(norphan - born), push};
        for (int j = 0; j < 8; j++) { keep_sum[j] = s[j]; if (user_sum) user_sum[j] = s[j]; }
    }
}

// ---------------------------------------------------------------------------- @5
__global__ __launch_bounds__(RC_BLOCK) void k_tk_paint(const int32_t* labels, size_t labels_step, int* P, int w, int h, int max_regions,
                                                       int max_tracks, TkTabs q, uint8_t* mask_out, size_t mask_out_step, const rc_track* tab,
                                                       rc_track* user_tab, int32_t* user_tol) {
    const int lane = threadIdx.x, wv = threadIdx.y, x = blockIdx.x * 64 + lane;
    const int yb = (blockIdx.y * TK_WAVES + wv) * TK_ROWS;
    for (int r = 0; r < TK_ROWS; r++) {
        const int y = yb + r;
        if (y >= h || x >= w) break;
        const int c = *(const int32_t*)((const char*)labels + (size_t)y * labels_step + (size_t)x * 4);
        int* pp = P + (size_t)y * w + x;
        // the table: slot + 1 (| TK_CONF) for a tracked label, -1 for an untracked one, 0 beyond R: background like every
        // label outside 1..max_regions, which is never looked up
        const int e = (c >= 1 && c <= max_regions) ? q.paint[c] : 0;
        int v = 0;
        if (e > 0) v = e & ~TK_CONF;
        else if (e == 0) {                                               // a track that goes on keeps what nobody has taken
            const int p = *pp;
            v = (p >= 1 && p <= max_tracks && q.keep[p - 1]) ? p : 0;
        }
        *pp = v;
        if (mask_out) mask_out[(size_t)y * mask_out_step + x] = (e > 0 && (e & TK_CONF)) ? 255 : 0;
    }
    const size_t tid = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * RC_BLOCK + wv * 64 + lane, nthr = (size_t)gridDim.x * gridDim.y * RC_BLOCK;
    if (user_tab) {
        const long long* src = (const long long*)tab;
        long long* dst = (long long*)user_tab;
        for (size_t i = tid; i < (size_t)max_tracks * (sizeof(rc_track) / 8); i += nthr) dst[i] = src[i];
    }
    if (user_tol)
        for (size_t i = tid; i <= (size_t)max_regions; i += nthr) user_tol[i] = q.tol[i];
}

// ---------------------------------------------------------------------------- @6
__global__ __launch_bounds__(RC_BLOCK) void k_tk_prims(const rc_track* tab, int max_tracks, uint32_t color, int thickness, int radius, rc_draw_prim* out) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= max_tracks) return;
    const rc_track q = tab[i];
    rc_draw_prim p[5];
    memset(p, 0, sizeof(p));
    if ((q.flags & RC_TRACK_CONFIRMED) && !(q.flags & RC_TRACK_ENDED)) {
        const int bx[5] = {q.x0, q.x1, q.x1, q.x0, q.x0}, by[5] = {q.y0, q.y0, q.y1, q.y1, q.y0};
        for (int j = 0; j < 4; j++) {
            p[j].kind = RC_DRAW_LINE; p[j].x0 = bx[j]; p[j].y0 = by[j]; p[j].x1 = bx[j + 1]; p[j].y1 = by[j + 1];
            p[j].size = thickness; p[j].color = color;
        }
        p[4].kind = RC_DRAW_DISC; p[4].x0 = p[4].x1 = q.px; p[4].y0 = p[4].y1 = q.py; p[4].size = radius; p[4].color = color;
    }
    for (int j = 0; j < 5; j++) out[(size_t)5 * i + j] = p[j];
}

// ============================================================================ host side
void rc_state_free(RcTracks& g) {
    rc_buf_free(g.foot); rc_buf_free(g.ov); rc_buf_free(g.aux); rc_buf_free(g.out);
    rc_fence_free(g.zf);
    g = RcTracks();
}

// open and reset: no track, an empty footprint, next_id 1, no push; the overlap table is zeroed by every push
int rc_state_zero(RcSlot& s, RcTracks& g) {
    const int rc = rc_fence_zero(g.zf, s.cur, {&g.foot, &g.aux, &g.out});
    if (rc) return rc;
    g.pushes = 0;
    return RC_OK;
}

static long long* tk_summary(const RcTracks& g) { return (long long*)g.out.p; }
static rc_track* tk_table(const RcTracks& g) { return (rc_track*)((char*)g.out.p + 64); }
static size_t tk_aux_bytes(const rc_tracks_params& p) { return sizeof(TkCtl) + ((size_t)4 * (p.max_regions + 1) + (size_t)2 * p.max_tracks) * 4; }
static TkTabs tk_tabs(const RcTracks& g) {
    TkTabs q;
    const size_t nl = (size_t)g.prm.max_regions + 1;
    q.ctl = (TkCtl*)g.aux.p;
    q.best = (int*)(q.ctl + 1); q.bestov = q.best + nl; q.tol = q.bestov + nl; q.paint = q.tol + nl;
    q.merged = q.paint + nl; q.keep = q.merged + g.prm.max_tracks;
    return q;
}

extern "C" int rcflow_tracks_open(rc_ctx* ctx, int stream, int w, int h, const rc_tracks_params* prm) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0 || (long long)w * h >= (1ll << 31)) {
        rc_set_error("rcflow_tracks_open: bad frame size %d x %d (below 2^31 pixels) or no parameters", w, h);
        return RC_EINVAL;
    }
    if (prm->max_regions < 1 || prm->max_regions > RC_TRACKS_MAX_REGIONS || prm->max_tracks < 1 || prm->max_tracks > RC_TRACKS_MAX ||
        prm->min_overlap < 1 || prm->max_misses < 0 || prm->max_misses > 65535 || prm->min_hits < 1 || prm->flags) {
        rc_set_error("rcflow_tracks_open: max_regions 1..%d, max_tracks 1..%d, min_overlap >= 1, max_misses 0..65535, min_hits >= 1, flags 0",
                     RC_TRACKS_MAX_REGIONS, RC_TRACKS_MAX);
        return RC_EINVAL;
    }
    int rc = rc_fits_context("rcflow_tracks_open", ctx, w, h);
    if (rc) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcTracks n;
    n.w = w; n.h = h; n.prm = *prm;
    rc = rc_buf_ensure(n.foot, (size_t)w * h * 4);
    if (!rc) rc = rc_buf_ensure(n.ov, ((size_t)prm->max_regions + 1) * prm->max_tracks * 4);
    if (!rc) rc = rc_buf_ensure(n.aux, tk_aux_bytes(*prm));
    if (!rc) rc = rc_buf_ensure(n.out, 64 + (size_t)prm->max_tracks * sizeof(rc_track));
    return rc_state_install(*s, s->tk, n, rc);
}

extern "C" int rcflow_tracks_push_dev(rc_ctx* ctx, int stream, const int32_t* d_labels, size_t labels_step, const rc_region* d_regions,
                                      const long long* d_regions_summary, rc_track* d_tracks, int32_t* d_track_of_label, uint8_t* d_mask_out,
                                      size_t mask_out_step, long long* d_summary) {
    static const char* who = "rcflow_tracks_push_dev";
    RcSlot* s; RcTracks* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tk, who, s, gp)) return rc;
    RcTracks& g = *gp;
    const int w = g.w, h = g.h, NR = g.prm.max_regions, NT = g.prm.max_tracks;
    if (!d_labels || !d_regions || !d_regions_summary) { rc_set_error("%s: d_labels, d_regions and d_regions_summary are needed", who); return RC_EINVAL; }
    RcArgs a(who, w, h);
    a.image("d_labels", d_labels, labels_step, 4, 4, RC_ARG_IN);
    a.array("d_regions", d_regions, (size_t)NR * sizeof(rc_region), 8, RC_ARG_IN);
    a.array("d_regions_summary", d_regions_summary, 64, 8, RC_ARG_IN);
    a.array("d_tracks", d_tracks, (size_t)NT * sizeof(rc_track), 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_track_of_label", d_track_of_label, ((size_t)NR + 1) * 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_mask_out", d_mask_out, mask_out_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(g.zf, s->cur, true);
    if (rc) return rc;
    const double px = (double)w * h;
    int* P = (int*)g.foot.p;
    int* ov = (int*)g.ov.p;
    rc_track* tab = tk_table(g);
    const TkTabs q = tk_tabs(g);
    const size_t nov = ((size_t)NR + 1) * NT;
    const dim3 blk(64, TK_WAVES), grid((w + 63) / 64, (h + TK_TILE_H - 1) / TK_TILE_H);
    { RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 0, 4. * nov + (double)NT * sizeof(rc_track));
      const size_t nb = (nov + RC_BLOCK - 1) / RC_BLOCK;
      hipLaunchKernelGGL(k_tk_prepare, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(RC_BLOCK), 0, s->cur, tab, NT, ov, nov, q.merged); }
    { RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 1, 8. * px);
      hipLaunchKernelGGL(k_tk_overlap, grid, blk, 0, s->cur, d_labels, labels_step, P, w, h, d_regions_summary, NR, NT, ov); }
    { RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 2, 4. * nov);
      hipLaunchKernelGGL(k_tk_claim, dim3(NR + 1), dim3(RC_BLOCK), 0, s->cur, ov, tab, d_regions_summary, NR, NT, g.prm.min_overlap, q); }
    { RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 3, (double)NT * (8. * NR + 2. * sizeof(rc_track)));
      hipLaunchKernelGGL(k_tk_update, dim3(NT), dim3(RC_BLOCK), 0, s->cur, tab, d_regions, d_regions_summary, NR, g.prm, q); }
    { RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 4, (double)NT * sizeof(rc_track) + (double)NR * sizeof(rc_region));
      hipLaunchKernelGGL(k_tk_births, dim3(1), dim3(TK_BIRTH_BLOCK), 0, s->cur, tab, d_regions, d_regions_summary, NR, NT, g.prm, q, tk_summary(g),
                         d_summary); }
    { RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 5, (12. + (d_mask_out ? 1. : 0.)) * px + (d_tracks ? 2. : 0.) * NT * sizeof(rc_track));
      hipLaunchKernelGGL(k_tk_paint, grid, blk, 0, s->cur, d_labels, labels_step, P, w, h, NR, NT, q, d_mask_out, mask_out_step, tab, d_tracks,
                         d_track_of_label); }
    RC_HIP(hipGetLastError());
    g.pushes++;                                           // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_tracks_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, rc_draw_prim* d_prims) {
    static const char* who = "rcflow_tracks_prims_dev";
    RcSlot* s; RcTracks* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tk, who, s, gp)) return rc;
    RcTracks& g = *gp;
    if (rc_prims_check(who, d_prims, thickness, disc_radius)) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(g.zf, s->cur, true);
    if (rc) return rc;
    RcProfScope ps(ctx, s->cur, RC_K_TRACKS, 6, (double)g.prm.max_tracks * (sizeof(rc_track) + 5. * sizeof(rc_draw_prim)));
    hipLaunchKernelGGL(k_tk_prims, dim3((g.prm.max_tracks + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, tk_table(g), g.prm.max_tracks,
                       color, thickness, disc_radius, d_prims);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_tracks_read(rc_ctx* ctx, int stream, rc_track* tracks, int cap, int32_t* footprint, long long summary[8]) {
    RcSlot* s; RcTracks* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tk, "rcflow_tracks_read", s, gp)) return rc;
    RcTracks& g = *gp;
    if (cap < 0 || (cap && !tracks)) { rc_set_error("rcflow_tracks_read: a bad buffer"); return RC_EINVAL; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(g.zf, s->cur, true);
    if (rc) return rc;
    // summary and table lie together: one copy of the prefix the caller can take
    const int room = cap < g.prm.max_tracks ? cap : g.prm.max_tracks;
    std::vector<char> host(64 + (size_t)room * sizeof(rc_track));
    RC_HIP(hipMemcpyAsync(host.data(), g.out.p, host.size(), hipMemcpyDeviceToHost, s->cur));
    if (footprint) RC_HIP(hipMemcpyAsync(footprint, g.foot.p, (size_t)g.w * g.h * 4, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    if (tracks && room) memcpy(tracks, host.data() + 64, (size_t)room * sizeof(rc_track));
    if (summary) memcpy(summary, host.data(), 64);
    return RC_OK;
}

extern "C" int rcflow_tracks_info(rc_ctx* ctx, int stream, rc_tracks_info* info) {
    RcSlot* s; RcTracks* gp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tk, "rcflow_tracks_info", s, gp)) return rc;
    const RcTracks& g = *gp;
    if (!info) return RC_OK;
    memset(info, 0, sizeof(*info));
    info->w = g.w; info->h = g.h; info->prm = g.prm;
    info->launches_per_push = RC_TRACKS_LAUNCHES;
    info->pushes = g.pushes;
    info->device_bytes = g.foot.bytes + g.ov.bytes + g.aux.bytes + g.out.bytes;
    return RC_OK;
}

extern "C" int rcflow_tracks_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::tk, "rcflow_tracks_reset"); }
extern "C" int rcflow_tracks_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::tk); }
