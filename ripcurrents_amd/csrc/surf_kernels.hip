// surf_kernels.hip -- surf zone: where do the waves break, how often, and where does the band of breaking have a hole?
//
// Per pixel a ring of the last `window` grey frames, its sums S1 and S2, and a flag per held frame: bright now and above the
// pixel's own window mean.  Q counts the flags: the fraction of time breaking.  From the same state the variance image (twice the
// standard deviation) and the window mean.  Along lines laid from land to sea the runs of surf samples, the band's inner and outer
// edge, the line's load; along the shore the lower median of the neighbours' loads and the lines that fall below a share of it:
// the rip channels, found without any flow.  include/rcflow.h ("surf") is the specification; tests/_surf_ref.py states it in numpy
// and the kernels are held to that bit for bit: everything is integer except the records' conversions, which are double, operation
// by operation.  A push is one launch, three with lines, and nothing synchronises:
//   surf@0  a pure streaming update.  The state planes have a row pitch of w rounded up to 4 and are walked as one run of pixels:
//           a lane takes 4 consecutive pixels (the frame and the ring slot a dword each, S1 and S2 a dwordx4 each, Q a dwordx2,
//           every byte output a dword), a wave 256, a block SF_WAVES of those a pass, and as many passes as keep the launch to
//           SF_MAX_BLOCKS blocks.  The flag ring is bit planes packed across pixels by the wave's ballot: per held frame and per
//           256 pixels four uint64, word k holding pixel 4 lane + k in bit `lane`; the outgoing flags are read the same way and
//           picked out by lane.  The picture's index depends on Q alone: a table per block in LDS.  The three counts by a wave
//           reduction and LDS to a place per block, then the ticket and the last-arriving block's hand-over
//           (rc_hand_off_release of rc_reduce.h), which adds the places up;
//   surf@1  a wave a line: the samples of the Q plane, four a lane in flight; the in-samples as a bit mask across the lanes by the
//           wave's ballot, the runs of min_run and more by shifting and masking it;
//   surf@2  one block: a thread a line takes the rank among at most 65 loads by counting, thread 0 walks the lines for the
//           channels, every thread closes its lines' records, thread 0 the summary;
//   surf@3  the primitives, a lane a record.

#include <math.h>
#include <string.h>

#include <vector>

#include "rc_host.h"
#include "rc_reduce.h"

#define SF_WAVES 4
static_assert(RC_BLOCK == 64 * SF_WAVES, "a block is SF_WAVES waves");
#define SF_TILE 256            // pixels a wave takes at a time
#define SF_MAX_BLOCKS 256      // every block ends in a release and a ticket on one line (as kinematics@0), and the launch pays for each:
                               // at 1080p caps of 128, 256, 512 and 1024 gave 30, 22, 26 and 36 us without outputs and 48, 33, 33 and 43 us
                               // with all six (profiles/surf_kernel_summary.md)
#define SF_DIV_BITS 22         // the numerators of sf_div are below 2^22
static_assert(sizeof(rc_surf_line) == 64 && sizeof(rc_surf_channel) == 32 && sizeof(rc_surf_params) == 56,
              "the records of include/rcflow.h have the sizes the Python and numpy mirrors give them");
static_assert(RC_SURF_MAX_WINDOW == 4096 && RC_SURF_MAX_SAMPLES == 1024 && RC_SURF_MAX_LINES == 1024 && RC_SURF_MAX_SPAN == 32,
              "Q is uint16 and S2 uint32 (4096 * 255^2 < 2^32); surf@1 holds 1024 samples as 16 ballots, surf@2 1024 lines in LDS");

// RcSurf::ctl.  The ticket has a 128-byte line of its own: every block adds to it.  A block's counts go to a place of their own
// by plain stores, so the ticket is the launch's only atomic on a shared line
struct SfPart { unsigned now, surf; unsigned long long sumq; };
struct SfCtl {
    RcTicketLine t0;
    long long res[3]; unsigned pad1[26];                                 // of the last surf@0: now | surf | sum Q
    SfPart part[SF_MAX_BLOCKS];                                            // written by every block of every launch
};
static_assert(sizeof(SfCtl) == 256 + 16 * SF_MAX_BLOCKS, "two lines and the blocks' counts");

// floor(v / d) for v < 2^SF_DIV_BITS by a multiplication: m = ceil(2^s / d) with s = SF_DIV_BITS + ceil(log2 d) is exact there
// (Granlund and Montgomery); d is the same for every pixel of a push, so the host finds m and s
struct SfDiv { unsigned m; int s; };
static SfDiv sf_div_of(unsigned d) {
    int l = 0;
    while ((1u << l) < d) l++;
    SfDiv r;
    r.s = SF_DIV_BITS + l;
    r.m = (unsigned)(((1ull << r.s) + d - 1) / d);
    return r;
}
__device__ __forceinline__ unsigned sf_div(unsigned v, SfDiv d) { return (unsigned)(((unsigned long long)v * d.m) >> d.s); }

// ============================================================================ surf@0: ring, sums, flags, pictures, counts
struct SfArgs0 {
    const uint8_t* g; size_t step;
    uint8_t* ring;                               // the slot pushes mod W of the ring, [h][P]
    unsigned long long* bits;                    // the same slot of the flag ring, [tiles][4]
    uint32_t* S1; uint32_t* S2; uint16_t* Q;     // [h][P]
    uint8_t* now; size_t now_step;               // each output or null
    uint8_t* surf; size_t surf_step;
    uint16_t* q; size_t q_step;                  // the step in bytes
    uint8_t* mean; size_t mean_step;
    uint8_t* sd; size_t sd_step;
    uint8_t* pic; size_t pic_step;
    const uint8_t* jet;                          // 768 bytes
    SfCtl* ctl;
    long long* summary; long long* summary2;     // written here only by a session without lines; the caller's or null
    int w, h, P, total, tiles;                   // total = P h; tiles of SF_TILE pixels
    int n, bright, delta_n, qthr;                // held frames; delta n; the least Q of a surf pixel
    unsigned vis_n;                              // vis_permille n
    SfDiv d2n, dn;
    unsigned nblocks;
    int lines;
    long long pushes;
};

__device__ __forceinline__ void sf_store4(uint8_t* base, size_t step, int x, int y, int nv, const unsigned v[4]) {
    uint8_t* dst = base + (size_t)y * step + x;
    if (nv == 4) {
        const uint32_t wd = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        __builtin_memcpy(dst, &wd, 4);
    } else {
        for (int k = 0; k < nv; k++) dst[k] = (uint8_t)v[k];
    }
}

template <int SD>
__global__ __launch_bounds__(RC_BLOCK) void k_sf_pixels(const SfArgs0 a) {
    __shared__ uint8_t qi[RC_SURF_MAX_WINDOW + 1];            // the picture's index of Q = 0..n
    __shared__ uint8_t jet[768];
    __shared__ unsigned cnt[2];
    __shared__ unsigned long long sq;
    __shared__ int last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) { cnt[0] = cnt[1] = 0u; sq = 0ull; }
    if (a.pic) {
        for (int i = threadIdx.x; i <= a.n; i += RC_BLOCK) qi[i] = (uint8_t)min(255u, (unsigned)i * 255000u / a.vis_n);
        rc_stage_jet(jet, a.jet);
    }
    __syncthreads();
    unsigned c_now = 0, c_surf = 0, c_q = 0;                  // a lane's: at most 2^25 / (64 SF_WAVES SF_MAX_BLOCKS) * 4 pixels of Q <= 4096
    const unsigned n = (unsigned)a.n;
    for (int tv = blockIdx.x * SF_WAVES + wv; tv < a.tiles; tv += gridDim.x * SF_WAVES) {
        const int t = __builtin_amdgcn_readfirstlane(tv);     // the wave's tile, in a scalar register
        const int idx = t * SF_TILE + 4 * lane;
        const bool act = idx < a.total;                       // total is a multiple of 4
        const int y = act ? idx / a.P : 0, x = idx - y * a.P;
        const int nv = act ? min(4, a.w - x) : 0;             // 1..4 when active: P - w < 4
        uint32_t gw = 0, ow = 0;
        uint4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
        uint2 qw = {0, 0};
        if (act) {
            const uint8_t* src = a.g + (size_t)y * a.step + x;
            if (nv == 4) __builtin_memcpy(&gw, src, 4);
            else for (int k = 0; k < nv; k++) gw |= (uint32_t)src[k] << (8 * k);
            ow = *(const uint32_t*)(a.ring + idx);
            s1 = *(const uint4*)(a.S1 + idx);
            s2 = *(const uint4*)(a.S2 + idx);
            qw = *(const uint2*)(a.Q + idx);
        }
        unsigned long long* bp = a.bits + (size_t)t * 4;      // the tile's four words: the same address in every lane
        const unsigned long long ob[4] = {bp[0], bp[1], bp[2], bp[3]};
        unsigned S1v[4] = {s1.x, s1.y, s1.z, s1.w}, S2v[4] = {s2.x, s2.y, s2.z, s2.w};
        unsigned Qv[4] = {qw.x & 0xffffu, qw.x >> 16, qw.y & 0xffffu, qw.y >> 16};
        unsigned bv[4];
        unsigned long long nb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned g = (gw >> (8 * k)) & 255u, o = (ow >> (8 * k)) & 255u;
            S1v[k] += g - o;
            S2v[k] += g * g - o * o;
            const bool b = k < nv && g >= (unsigned)a.bright && g * n >= S1v[k] + (unsigned)a.delta_n;
            nb[k] = __ballot(b);                              // every lane of the wave is here: the padding and the tail vote 0
            bv[k] = b ? 1u : 0u;
            Qv[k] += bv[k] - (unsigned)((ob[k] >> lane) & 1ull);
        }
        if (lane == 0) {
            bp[0] = nb[0]; bp[1] = nb[1]; bp[2] = nb[2]; bp[3] = nb[3];
        }
        if (!act) continue;                                   // no ballot and no barrier below
        *(uint32_t*)(a.ring + idx) = gw;
        *(uint4*)(a.S1 + idx) = make_uint4(S1v[0], S1v[1], S1v[2], S1v[3]);
        *(uint4*)(a.S2 + idx) = make_uint4(S2v[0], S2v[1], S2v[2], S2v[3]);
        *(uint2*)(a.Q + idx) = make_uint2(Qv[0] | (Qv[1] << 16), Qv[2] | (Qv[3] << 16));
        unsigned sv[4], o4[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            sv[k] = k < nv && Qv[k] >= (unsigned)a.qthr ? 1u : 0u;
            c_now += bv[k]; c_surf += sv[k]; c_q += Qv[k];    // Q of the padding stays 0
        }
        if (a.now) {
#pragma unroll
            for (int k = 0; k < 4; k++) o4[k] = bv[k] ? 255u : 0u;
            sf_store4(a.now, a.now_step, x, y, nv, o4);
        }
        if (a.surf) {
#pragma unroll
            for (int k = 0; k < 4; k++) o4[k] = sv[k] ? 255u : 0u;
            sf_store4(a.surf, a.surf_step, x, y, nv, o4);
        }
        if (a.q) {
            uint16_t* dst = (uint16_t*)((char*)a.q + (size_t)y * a.q_step) + x;
            if (nv == 4) {
                const uint2 v = make_uint2(Qv[0] | (Qv[1] << 16), Qv[2] | (Qv[3] << 16));
                __builtin_memcpy(dst, &v, 8);
            } else {
                for (int k = 0; k < nv; k++) dst[k] = (uint16_t)Qv[k];
            }
        }
        if (a.mean) {
#pragma unroll
            for (int k = 0; k < 4; k++) o4[k] = sf_div(2u * S1v[k] + n, a.d2n);
            sf_store4(a.mean, a.mean_step, x, y, nv, o4);
        }
        if (SD) {
            // isqrt(floor(4 D / n^2)) = floor(isqrt(4 D) / n): r^2 n^2 <= 4 D exactly when r n <= isqrt(4 D).  D = n S2 - S1^2 < 2^44;
            // the root from the double one, put right by one step either way; it is at most 255 n + n < 2^21
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const long long D4 = 4ll * ((long long)n * S2v[k] - (long long)S1v[k] * S1v[k]);
                long long r = (long long)sqrt((double)D4);
                if (r * r > D4) r--;
                else if ((r + 1) * (r + 1) <= D4) r++;
                o4[k] = min(255u, sf_div((unsigned)r, a.dn));
            }
            sf_store4(a.sd, a.sd_step, x, y, nv, o4);
        }
        if (a.pic) {
            uint8_t* dst = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x;
            uint32_t px[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint8_t* e = jet + 3 * qi[Qv[k]];
                px[k] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
            }
            if (nv == 4) {
                uint32_t wd[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
                __builtin_memcpy(dst, wd, 12);
            } else {
                for (int k = 0; k < nv; k++) { dst[3 * k] = (uint8_t)px[k]; dst[3 * k + 1] = (uint8_t)(px[k] >> 8); dst[3 * k + 2] = (uint8_t)(px[k] >> 16); }
            }
        }
    }
    c_now = rc_wave_sum_all(c_now); c_surf = rc_wave_sum_all(c_surf);
    unsigned long long wq = c_q;
    wq = rc_wave_sum_all(wq);
    if (lane == 0) { atomicAdd(&cnt[0], c_now); atomicAdd(&cnt[1], c_surf); atomicAdd(&sq, wq); }
    __syncthreads();
    if (threadIdx.x == 0) {
        SfPart p;
        p.now = cnt[0]; p.surf = cnt[1]; p.sumq = sq;
        a.ctl->part[blockIdx.x] = p;
    }
    if (!rc_hand_off_release(&a.ctl->t0.ticket, a.nblocks, &last)) return;
    // the last-arriving block adds up the blocks' counts
    if (threadIdx.x == 0) { cnt[0] = cnt[1] = 0u; sq = 0ull; }
    __syncthreads();
    unsigned p_now = 0, p_surf = 0;
    unsigned long long p_q = 0;
    for (unsigned b = threadIdx.x; b < a.nblocks; b += RC_BLOCK) {
        p_now += rc_acc_load(&a.ctl->part[b].now);
        p_surf += rc_acc_load(&a.ctl->part[b].surf);
        p_q += rc_acc_load(&a.ctl->part[b].sumq);
    }
    p_now = rc_wave_sum_all(p_now); p_surf = rc_wave_sum_all(p_surf);
    p_q = rc_wave_sum_all(p_q);
    if (lane == 0) { atomicAdd(&cnt[0], p_now); atomicAdd(&cnt[1], p_surf); atomicAdd(&sq, p_q); }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long r0 = cnt[0], r1 = cnt[1], r2 = (long long)sq;
    a.ctl->res[0] = r0; a.ctl->res[1] = r1; a.ctl->res[2] = r2;          // read by surf@2 (stream order)
    __hip_atomic_store(&a.ctl->t0.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.lines == 0) {
        const long long s[8] = {a.n, r0, r1, r2, 0, 0, 0, a.pushes};
        for (int k = 0; k < 8; k++) {
            a.summary[k] = s[k];
            if (a.summary2) a.summary2[k] = s[k];
        }
    }
}

// ============================================================================ surf@1: samples, runs, band, load
struct SfArgs1 {
    const rc_transect_sample* table; const rc_transect_geom* geom;
    const uint16_t* Q;
    rc_surf_line* rec;                           // the state's: surf@2 closes it
    int w, h, P, L, qthr, min_run;
};

// the point at pos (1/256 sample) of a line of n samples from Xa to Xb (1/16 pixel), in 1/256 pixel: the shoreline's formula
__device__ __forceinline__ int sf_point(int Xa, int Xb, long long pos, int n) {
    return (int)(16ll * Xa + rc_floor_div(16ll * (Xb - Xa) * pos + 128ll * (n - 1), 256ll * (n - 1)));
}

// the in-samples of a line as a bit mask: lane u < 16 holds samples 64 u .. 64 u + 63, the others 0.  The mask shifted down by s
// samples, 0 < s < 64, across the lanes
__device__ __forceinline__ unsigned long long sf_mask_shr(unsigned long long m, int s) {
    const unsigned long long next = __shfl_down(m, 1, 64);
    return (m >> s) | (next << (64 - s));
}

__global__ __launch_bounds__(RC_BLOCK) void k_sf_lines(const SfArgs1 a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int line = blockIdx.x * SF_WAVES + wv;
    if (line >= a.L) return;                                  // no barrier and no LDS below: a wave works alone
    const rc_transect_geom gm = a.geom[line];
    const int n = gm.n, first = gm.first;
    int B = 0, peak = -1, kpeak = 0x7fffffff;
    unsigned long long M = 0;
    // four samples a lane at a time, their loads in flight together: indices past the line's end are clamped and not counted
    for (int u0 = 0; u0 * 64 < n; u0 += 4) {
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = min((u0 + k) * 64 + lane, n - 1);
            const rc_transect_sample sm = a.table[(size_t)first + j];
            const int ix = sm.X >> 4, fx = sm.X & 15, iy = sm.Y >> 4, fy = sm.Y & 15;
            const int ix1 = min(ix + 1, a.w - 1), iy1 = min(iy + 1, a.h - 1);
            const uint16_t* r0 = a.Q + (size_t)iy * a.P;
            const uint16_t* r1 = a.Q + (size_t)iy1 * a.P;
            v[k] = ((16 - fx) * (16 - fy) * r0[ix] + fx * (16 - fy) * r0[ix1] + (16 - fx) * fy * r1[ix] + fx * fy * r1[ix1] + 128) >> 8;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = (u0 + k) * 64 + lane;
            const bool live = j < n;
            const unsigned long long word = __ballot(live && v[k] >= a.qthr);       // samples 64 (u0 + k) .. + 63 in bit order
            if (lane == u0 + k) M = word;
            if (live) {
                B += v[k];
                if (v[k] > peak) { peak = v[k]; kpeak = j; }  // j ascends: the first of the lane's largest
            }
        }
    }
    // bit j stays set when samples j .. j + min_run - 1 are all in: the windows double, the rest in one step
    int win = 1;
    while (2 * win <= a.min_run) { M &= sf_mask_shr(M, win); win *= 2; }
    if (a.min_run > win) M &= sf_mask_shr(M, a.min_run - win);
    int k0 = M ? 64 * lane + __builtin_ctzll(M) : 0x7fffffff;
    int k1 = M ? 64 * lane + 63 - __builtin_clzll(M) + a.min_run - 1 : -1;
    for (int o = 32; o > 0; o >>= 1) {
        B += __shfl_xor(B, o, 64);
        k0 = min(k0, __shfl_xor(k0, o, 64));
        k1 = max(k1, __shfl_xor(k1, o, 64));
        const int op = __shfl_xor(peak, o, 64), ok = __shfl_xor(kpeak, o, 64);
        if (op > peak || (op == peak && ok < kpeak)) { peak = op; kpeak = ok; }
    }
    if (lane != 0) return;
    rc_surf_line r;
    memset(&r, 0, sizeof(r));
    r.load = B; r.peak = peak; r.kpeak = kpeak;
    if (k1 < 0) {
        r.flags = RC_SURF_NOBAND; r.k0 = r.k1 = -1;
    } else {
        const rc_transect_sample sa = a.table[first], sb = a.table[(size_t)first + n - 1];
        r.k0 = k0; r.k1 = k1;
        r.ix = sf_point(sa.X, sb.X, 256ll * k0, n); r.iy = sf_point(sa.Y, sb.Y, 256ll * k0, n);
        r.ox = sf_point(sa.X, sb.X, 256ll * k1, n); r.oy = sf_point(sa.Y, sb.Y, 256ll * k1, n);
        r.width_m = (float)((double)(k1 - k0 + 1) * gm.ds);
    }
    a.rec[line] = r;
}

// ============================================================================ surf@2: reference, channels, records, summary
struct SfArgs2 {
    const rc_transect_sample* table; const rc_transect_geom* geom;
    rc_surf_line* rec; rc_surf_channel* chan; long long* summary;        // the state's copy
    rc_surf_line* rec2; rc_surf_channel* chan2; long long* summary2;     // the caller's, or null
    const SfCtl* ctl;
    int L, n, span, ratio, min_load, min_lines;
    double mpp;
    long long pushes;
};

__global__ __launch_bounds__(RC_BLOCK) void k_sf_shore(const SfArgs2 a) {
    __shared__ int B[RC_SURF_MAX_LINES], ref[RC_SURF_MAX_LINES], share[RC_SURF_MAX_LINES], fl[RC_SURF_MAX_LINES];
    __shared__ int nband, nchan_lines;
    __shared__ long long nchan;
    if (threadIdx.x == 0) { nband = 0; nchan_lines = 0; }
    for (int i = threadIdx.x; i < a.L; i += RC_BLOCK) { B[i] = a.rec[i].load; fl[i] = a.rec[i].flags; }
    __syncthreads();
    int lb = 0, lc = 0;
    for (int i = threadIdx.x; i < a.L; i += RC_BLOCK) {
        const int lo = max(0, i - a.span), hi = min(a.L - 1, i + a.span), rank = (hi - lo) / 2;
        int rv = 0;
        for (int p = lo; p <= hi; p++) {                      // the value with `less` <= rank < `less` + `equal`
            const int v = B[p];
            int less = 0, eq = 0;
            for (int q = lo; q <= hi; q++) { less += B[q] < v; eq += B[q] == v; }
            if (less <= rank && rank < less + eq) { rv = v; break; }
        }
        int f = fl[i];
        if (rv < max(a.min_load, 1)) f |= RC_SURF_NOREF;
        else if ((long long)B[i] * 1000 < (long long)a.ratio * rv) f |= RC_SURF_CHANNEL;
        ref[i] = rv;
        share[i] = rv > 0 ? (int)min((long long)B[i] * 1000 / rv, (long long)RC_SURF_MAX_SHARE) : 1000;
        fl[i] = f;
        lb += !(f & RC_SURF_NOBAND); lc += (f & RC_SURF_CHANNEL) != 0;
    }
    if (lb) atomicAdd(&nband, lb);
    if (lc) atomicAdd(&nchan_lines, lc);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long nc = 0;
        rc_surf_channel zero;
        memset(&zero, 0, sizeof(zero));
        for (int i = 0; i < a.L;) {
            if (!(fl[i] & RC_SURF_CHANNEL)) { i++; continue; }
            int e = i;
            while (e < a.L && (fl[e] & RC_SURF_CHANNEL)) e++;
            const int first = i, count = e - i;
            i = e;
            if (count < a.min_lines) continue;
            int c = first;
            for (int j = first; j < e; j++) {
                fl[j] |= RC_SURF_IN_CHANNEL;
                if (share[j] < share[c]) c = j;
            }
            if (nc < RC_SURF_MAX_CHANNELS) {
                const rc_transect_geom gc = a.geom[c];
                long long sum = 0;
                int ne = 0;
                const int flank[2] = {first - 1, e};
                for (int s = 0; s < 2; s++) {
                    const int j = flank[s];
                    if (j < 0 || j >= a.L || (fl[j] & RC_SURF_NOBAND)) continue;
                    const rc_surf_line q = a.rec[j];
                    sum += 128ll * (q.k0 + q.k1);
                    ne++;
                }
                long long pos = ne ? sum / ne : 128ll * (gc.n - 1);
                if (pos > 256ll * (gc.n - 1)) pos = 256ll * (gc.n - 1);
                const rc_transect_sample sa = a.table[gc.first], sb = a.table[(size_t)gc.first + gc.n - 1];
                const rc_transect_sample la = a.table[a.geom[max(first - 1, 0)].first], lz = a.table[a.geom[min(e, a.L - 1)].first];
                const long long dx = (long long)la.X - lz.X, dy = (long long)la.Y - lz.Y;
                rc_surf_channel r = zero;
                r.first = first; r.count = count; r.centre = c; r.share = share[c];
                r.cx = sf_point(sa.X, sb.X, pos, gc.n); r.cy = sf_point(sa.Y, sb.Y, pos, gc.n);
                r.width_m = (float)((sqrt((double)(dx * dx + dy * dy)) / 16.) * a.mpp);
                a.chan[nc] = r;
                if (a.chan2) a.chan2[nc] = r;
            }
            nc++;
        }
        for (long long k = nc; k < RC_SURF_MAX_CHANNELS; k++) {
            a.chan[k] = zero;
            if (a.chan2) a.chan2[k] = zero;
        }
        nchan = nc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.L; i += RC_BLOCK) {
        rc_surf_line r = a.rec[i];
        r.flags = fl[i]; r.ref = ref[i]; r.share = share[i];
        a.rec[i] = r;
        if (a.rec2) a.rec2[i] = r;
    }
    if (threadIdx.x == 0) {
        const long long s[8] = {a.n, a.ctl->res[0], a.ctl->res[1], a.ctl->res[2], nband, nchan_lines, nchan, a.pushes};
        for (int k = 0; k < 8; k++) {
            a.summary[k] = s[k];
            if (a.summary2) a.summary2[k] = s[k];
        }
    }
}

// ============================================================================ surf@3: the primitives
__global__ __launch_bounds__(RC_BLOCK) void k_sf_prims(const rc_surf_line* rec, const rc_surf_channel* chan, int L, int pushed, uint32_t color,
                                                       int thickness, int radius, rc_draw_prim* out) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= L - 1 + RC_SURF_MAX_CHANNELS) return;
    rc_draw_prim p;
    memset(&p, 0, sizeof(p));
    if (pushed && i < L - 1) {
        const rc_surf_line q = rec[i];
        if (!(q.flags & RC_SURF_NOBAND))
            for (int j = i + 1; j < L; j++) {
                const rc_surf_line nx = rec[j];
                if (nx.flags & RC_SURF_NOBAND) continue;
                p.kind = RC_DRAW_LINE; p.x0 = (q.ox + 128) >> 8; p.y0 = (q.oy + 128) >> 8; p.x1 = (nx.ox + 128) >> 8; p.y1 = (nx.oy + 128) >> 8;
                p.size = thickness; p.color = color;
                break;
            }
    } else if (pushed) {
        const rc_surf_channel c = chan[i - (L - 1)];
        if (c.count > 0) {
            p.kind = RC_DRAW_DISC; p.x0 = p.x1 = (c.cx + 128) >> 8; p.y0 = p.y1 = (c.cy + 128) >> 8; p.size = radius; p.color = color;
        }
    }
    out[i] = p;
}

// ============================================================================ host side
static bool sf_pos(double v) { return v > 0. && v <= 1.7976931348623157e308; }       // finite and > 0; NaN fails
static bool sf_settable(int bright, int delta, int q_min, int ratio, int min_load, int vis) {
    return bright >= 0 && bright <= 255 && delta >= 0 && delta <= 255 && q_min >= 1 && q_min <= 1000 && ratio >= 1 && ratio <= 999 && min_load >= 0 &&
           vis >= 1 && vis <= 1000;
}

extern "C" int rcflow_surf_plan(int w, int h, const rc_transect_line* lines, int n_lines, double metres_per_pixel, rc_transect_sample* table,
                                rc_transect_geom* geom, int* total) {
    static const char* who = "rcflow_surf_plan";
    if (w <= 0 || h <= 0 || n_lines < 0 || n_lines > RC_SURF_MAX_LINES || (n_lines > 0 && !lines) || !sf_pos(metres_per_pixel)) {
        rc_set_error("%s: a picture of %d x %d, %d lines (0..%d), metres_per_pixel finite and > 0", who, w, h, n_lines, RC_SURF_MAX_LINES);
        return RC_EINVAL;
    }
    long long S = 0;
    for (int i = 0; i < n_lines; i++) {
        if (lines[i].n < RC_SURF_MIN_SAMPLES || lines[i].n > RC_SURF_MAX_SAMPLES) {
            rc_set_error("%s: line %d has %d samples (%d..%d)", who, i, lines[i].n, RC_SURF_MIN_SAMPLES, RC_SURF_MAX_SAMPLES);
            return RC_EINVAL;
        }
        S += lines[i].n;
    }
    if (S > RC_SURF_MAX_TOTAL) {
        rc_set_error("%s: %lld samples in all (at most %d)", who, S, RC_SURF_MAX_TOTAL);
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

void rc_state_free(RcSurf& v) {
    rc_buf_free(v.table); rc_buf_free(v.ring); rc_buf_free(v.bits); rc_buf_free(v.sums); rc_buf_free(v.out); rc_buf_free(v.ctl); rc_buf_free(v.jet);
    rc_fence_free(v.zf);
    v = RcSurf();
}

// open and reset: the ring, the flag ring, S1, S2 and Q, the last push's outputs, the ticket and the counters; the push count
int rc_state_zero(RcSlot& s, RcSurf& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.ring, &v.bits, &v.sums, &v.out, &v.ctl});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

// RcSurf::table: samples [S] | geometry [L]
static const rc_transect_sample* sf_table(const RcSurf& v) { return (const rc_transect_sample*)v.table.p; }
static const rc_transect_geom* sf_geom(const RcSurf& v) { return (const rc_transect_geom*)(sf_table(v) + v.S); }
// RcSurf::sums: S1 [h][P] uint32 | S2 [h][P] uint32 | Q [h][P] uint16
static uint32_t* sf_S1(const RcSurf& v) { return (uint32_t*)v.sums.p; }
static uint32_t* sf_S2(const RcSurf& v) { return sf_S1(v) + (size_t)v.P * v.h; }
static uint16_t* sf_Q(const RcSurf& v) { return (uint16_t*)(sf_S2(v) + (size_t)v.P * v.h); }
// RcSurf::out: summary 8 int64 | channels [RC_SURF_MAX_CHANNELS] | lines [L]
static long long* sf_out_summary(const RcSurf& v) { return (long long*)v.out.p; }
static rc_surf_channel* sf_out_chan(const RcSurf& v) { return (rc_surf_channel*)(sf_out_summary(v) + 8); }
static rc_surf_line* sf_out_rec(const RcSurf& v) { return (rc_surf_line*)(sf_out_chan(v) + RC_SURF_MAX_CHANNELS); }

extern "C" int rcflow_surf_open(rc_ctx* ctx, int stream, int w, int h, const rc_transect_line* lines, int n_lines, const rc_surf_params* prm) {
    static const char* who = "rcflow_surf_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad picture size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    const int W = prm->window;
    if (W < 2 || W > RC_SURF_MAX_WINDOW || prm->min_run < 1 || prm->min_run > 64 || prm->span < 0 || prm->span > RC_SURF_MAX_SPAN ||
        prm->min_lines < 1 || prm->min_lines > 64 || prm->flags || !sf_pos(prm->metres_per_pixel) ||
        !sf_settable(prm->bright, prm->delta, prm->q_min, prm->ratio, prm->min_load, prm->vis_permille)) {
        rc_set_error("%s: window 2..%d, bright and delta 0..255, q_min 1..1000, min_run 1..64, span 0..%d, ratio 1..999, min_load >= 0, min_lines 1..64, "
                     "vis_permille 1..1000, flags 0, metres_per_pixel finite and > 0", who, RC_SURF_MAX_WINDOW, RC_SURF_MAX_SPAN);
        return RC_EINVAL;
    }
    int S = 0;
    int rc = rcflow_surf_plan(w, h, lines, n_lines, prm->metres_per_pixel, nullptr, nullptr, &S);
    if (rc) {                                                 // the text names the entry point that was called
        const std::string t = rcflow_last_error();
        const size_t at = t.find(": ");
        rc_set_error("%s%s", who, at == std::string::npos ? "" : t.c_str() + at);
        return rc;
    }
    rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    if ((long long)w * h > RC_SURF_MAX_PIXELS) {
        rc_set_error("%s: %d x %d is more than RC_SURF_MAX_PIXELS pixels", who, w, h);
        return RC_ESIZE;
    }
    RcSurf n;
    n.w = w; n.h = h; n.prm = *prm; n.prm.pad = 0; n.L = n_lines; n.S = S;
    n.P = (w + 3) & ~3;
    const unsigned long long px = (unsigned long long)n.P * h;
    n.tiles = (int)((px + SF_TILE - 1) / SF_TILE);
    const unsigned long long ring = px * W, bits = 32ull * n.tiles * W, sums = px * 10, state = ring + bits + sums;
    if (state > RC_SURF_MAX_STATE_BYTES) {
        rc_set_error("%s: %d frames of %d x %d are %llu bytes of ring, flags and sums, more than RC_SURF_MAX_STATE_BYTES", who, W, w, h, state);
        return RC_ESIZE;
    }
    std::vector<unsigned char> host((size_t)S * sizeof(rc_transect_sample) + (size_t)n_lines * sizeof(rc_transect_geom));
    if (n_lines)
        (void)rcflow_surf_plan(w, h, lines, n_lines, prm->metres_per_pixel, (rc_transect_sample*)host.data(),
                               (rc_transect_geom*)(host.data() + (size_t)S * sizeof(rc_transect_sample)), nullptr);
    RC_HIP(hipSetDevice(ctx->device));
    rc = rc_buf_ensure(n.table, host.size());
    if (!rc) rc = rc_buf_ensure(n.ring, (size_t)ring);
    if (!rc) rc = rc_buf_ensure(n.bits, (size_t)bits);
    if (!rc) rc = rc_buf_ensure(n.sums, (size_t)sums);
    if (!rc) rc = rc_buf_ensure(n.out, 64 + RC_SURF_MAX_CHANNELS * sizeof(rc_surf_channel) + (size_t)n_lines * sizeof(rc_surf_line));
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(SfCtl));
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    if (!rc && host.size() && hipMemcpy(n.table.p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        rc_set_error("%s: the upload of the table failed", who);
        rc = RC_EHIP;
    }
    return rc_state_install(*s, s->sf, n, rc);
}

extern "C" int rcflow_surf_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, int channels, uint8_t* d_now, size_t now_step,
                                    uint8_t* d_surf, size_t surf_step, uint16_t* d_q, size_t q_step, uint8_t* d_mean, size_t mean_step,
                                    uint8_t* d_sd, size_t sd_step, uint8_t* d_picture, size_t picture_step, rc_surf_line* d_lines,
                                    rc_surf_channel* d_channels, long long* d_summary) {
    static const char* who = "rcflow_surf_push_dev";
    RcSlot* s; RcSurf* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sf, who, s, vp)) return rc;
    RcSurf& v = *vp;
    const int w = v.w, h = v.h, L = v.L, W = v.prm.window;
    if (channels != 1) {
        rc_set_error("%s: the session takes a grey frame of 1 channel, not %d", who, channels);
        return RC_EINVAL;
    }
    if (L == 0 && (d_lines || d_channels)) {
        rc_set_error("%s: a session without lines has no line records and no channels (d_lines and d_channels must be NULL)", who);
        return RC_EINVAL;
    }
    RcArgsN<10> ar(who, w, h);
    ar.image("d_gray", d_gray, step, 1, 1, RC_ARG_IN);
    ar.image("d_now", d_now, now_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_surf", d_surf, surf_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_q", d_q, q_step, 2, 2, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_mean", d_mean, mean_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_sd", d_sd, sd_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_lines", d_lines, (size_t)L * sizeof(rc_surf_line), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_channels", d_channels, RC_SURF_MAX_CHANNELS * sizeof(rc_surf_channel), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const long long p = v.pushes, pushes = p + 1;
    const int c = (int)(p % W), n = (int)(pushes < W ? pushes : W);
    const int qthr = (int)(((long long)v.prm.q_min * n + 999) / 1000);      // Q 1000 >= q_min n exactly when Q >= ceil(q_min n / 1000)
    const double px = (double)v.P * h;
    {
        SfArgs0 a;
        a.g = d_gray; a.step = step;
        a.ring = (uint8_t*)v.ring.p + (size_t)c * v.P * h;
        a.bits = (unsigned long long*)v.bits.p + (size_t)c * v.tiles * 4;
        a.S1 = sf_S1(v); a.S2 = sf_S2(v); a.Q = sf_Q(v);
        a.now = d_now; a.now_step = now_step; a.surf = d_surf; a.surf_step = surf_step; a.q = d_q; a.q_step = q_step;
        a.mean = d_mean; a.mean_step = mean_step; a.sd = d_sd; a.sd_step = sd_step; a.pic = d_picture; a.pic_step = picture_step;
        a.jet = (const uint8_t*)v.jet.p; a.ctl = (SfCtl*)v.ctl.p;
        a.summary = sf_out_summary(v); a.summary2 = d_summary;
        a.w = w; a.h = h; a.P = v.P; a.total = v.P * h; a.tiles = v.tiles;
        a.n = n; a.bright = v.prm.bright; a.delta_n = v.prm.delta * n; a.qthr = qthr; a.vis_n = (unsigned)v.prm.vis_permille * (unsigned)n;
        a.d2n = sf_div_of(2u * (unsigned)n); a.dn = sf_div_of((unsigned)n);
        const int bt = (v.tiles + SF_WAVES - 1) / SF_WAVES;
        a.nblocks = (unsigned)(bt < SF_MAX_BLOCKS ? bt : SF_MAX_BLOCKS);
        a.lines = L; a.pushes = pushes;
        // the frame in; the ring slot, S1, S2 and Q in and out; a quarter of a byte of flags; the outputs
        RcProfScope ps(ctx, s->cur, RC_K_SURF, 0, px * (1. + 2. + 8. + 8. + 4. + 0.25 + (d_now ? 1. : 0.) + (d_surf ? 1. : 0.) + (d_q ? 2. : 0.) +
                                                        (d_mean ? 1. : 0.) + (d_sd ? 1. : 0.) + (d_picture ? 3. : 0.)));
        if (d_sd) hipLaunchKernelGGL(k_sf_pixels<1>, dim3(a.nblocks), dim3(RC_BLOCK), 0, s->cur, a);
        else hipLaunchKernelGGL(k_sf_pixels<0>, dim3(a.nblocks), dim3(RC_BLOCK), 0, s->cur, a);
    }
    if (L > 0) {
        {
            SfArgs1 a;
            a.table = sf_table(v); a.geom = sf_geom(v); a.Q = sf_Q(v); a.rec = sf_out_rec(v);
            a.w = w; a.h = h; a.P = v.P; a.L = L; a.qthr = qthr; a.min_run = v.prm.min_run;
            // a sample's record and its four pixels in, a line's record out
            RcProfScope ps(ctx, s->cur, RC_K_SURF, 1, 24. * v.S + (double)L * (sizeof(rc_transect_geom) + sizeof(rc_surf_line)));
            hipLaunchKernelGGL(k_sf_lines, dim3((L + SF_WAVES - 1) / SF_WAVES), dim3(RC_BLOCK), 0, s->cur, a);
        }
        {
            SfArgs2 a;
            a.table = sf_table(v); a.geom = sf_geom(v);
            a.rec = sf_out_rec(v); a.chan = sf_out_chan(v); a.summary = sf_out_summary(v);
            a.rec2 = d_lines; a.chan2 = d_channels; a.summary2 = d_summary;
            a.ctl = (const SfCtl*)v.ctl.p;
            a.L = L; a.n = n; a.span = v.prm.span; a.ratio = v.prm.ratio; a.min_load = v.prm.min_load; a.min_lines = v.prm.min_lines;
            a.mpp = v.prm.metres_per_pixel; a.pushes = pushes;
            RcProfScope ps(ctx, s->cur, RC_K_SURF, 2, (double)L * sizeof(rc_surf_line) * (d_lines ? 3. : 2.) + 64. + RC_SURF_MAX_CHANNELS * sizeof(rc_surf_channel));
            hipLaunchKernelGGL(k_sf_shore, dim3(1), dim3(RC_BLOCK), 0, s->cur, a);
        }
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_surf_prims_dev(rc_ctx* ctx, int stream, uint32_t color, int thickness, int disc_radius, rc_draw_prim* d_prims) {
    static const char* who = "rcflow_surf_prims_dev";
    RcSlot* s; RcSurf* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sf, who, s, vp)) return rc;
    if (vp->L == 0) { rc_set_error("%s: a session without lines has no primitives", who); return RC_EINVAL; }
    if (rc_prims_check(who, d_prims, thickness, disc_radius)) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const int np = vp->L - 1 + RC_SURF_MAX_CHANNELS;
    RcProfScope ps(ctx, s->cur, RC_K_SURF, 3, (double)vp->L * sizeof(rc_surf_line) + RC_SURF_MAX_CHANNELS * sizeof(rc_surf_channel) + (double)np * sizeof(rc_draw_prim));
    hipLaunchKernelGGL(k_sf_prims, dim3((np + RC_BLOCK - 1) / RC_BLOCK), dim3(RC_BLOCK), 0, s->cur, sf_out_rec(*vp), sf_out_chan(*vp), vp->L,
                       vp->pushes > 0 ? 1 : 0, color, thickness, disc_radius, d_prims);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_surf_read(rc_ctx* ctx, int stream, rc_surf_line* lines, rc_surf_channel* channels, long long summary[8]) {
    RcSlot* s; RcSurf* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sf, "rcflow_surf_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    if (lines && vp->L) RC_HIP(hipMemcpyAsync(lines, sf_out_rec(*vp), (size_t)vp->L * sizeof(rc_surf_line), hipMemcpyDeviceToHost, s->cur));
    if (channels) RC_HIP(hipMemcpyAsync(channels, sf_out_chan(*vp), RC_SURF_MAX_CHANNELS * sizeof(rc_surf_channel), hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, sf_out_summary(*vp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_surf_table_read(rc_ctx* ctx, int stream, rc_transect_sample* table, rc_transect_geom* geom) {
    RcSlot* s; RcSurf* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sf, "rcflow_surf_table_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    if (table && vp->S) RC_HIP(hipMemcpyAsync(table, sf_table(*vp), (size_t)vp->S * sizeof(rc_transect_sample), hipMemcpyDeviceToHost, s->cur));
    if (geom && vp->L) RC_HIP(hipMemcpyAsync(geom, sf_geom(*vp), (size_t)vp->L * sizeof(rc_transect_geom), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_surf_set(rc_ctx* ctx, int stream, int bright, int delta, int q_min, int ratio, int min_load, int vis_permille) {
    RcSlot* s; RcSurf* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sf, "rcflow_surf_set", s, vp)) return rc;
    if (!sf_settable(bright, delta, q_min, ratio, min_load, vis_permille)) {
        rc_set_error("rcflow_surf_set: bright and delta 0..255, q_min 1..1000, ratio 1..999, min_load >= 0, vis_permille 1..1000");
        return RC_EINVAL;
    }
    vp->prm.bright = bright; vp->prm.delta = delta; vp->prm.q_min = q_min; vp->prm.ratio = ratio; vp->prm.min_load = min_load;
    vp->prm.vis_permille = vis_permille;
    return RC_OK;
}

extern "C" int rcflow_surf_info(rc_ctx* ctx, int stream, rc_surf_info* info) {
    RcSlot* s; RcSurf* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::sf, "rcflow_surf_info", s, vp)) return rc;
    const RcSurf& v = *vp;
    if (!info) { rc_set_error("rcflow_surf_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->lines = v.L; info->samples = v.S;
    info->launches_per_push = v.L ? RC_SURF_LAUNCHES : 1;
    info->held = (int)(v.pushes < v.prm.window ? v.pushes : v.prm.window);
    info->pushes = v.pushes;
    info->device_bytes = v.table.bytes + v.ring.bytes + v.bits.bytes + v.sums.bytes + v.out.bytes + v.ctl.bytes + v.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_surf_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::sf, "rcflow_surf_reset"); }
extern "C" int rcflow_surf_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::sf); }
