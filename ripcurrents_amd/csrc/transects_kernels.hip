// transects_kernels.hip -- transects: how strong is the rip, how wide is its neck, how does it pulse?
//
// Straight lines laid across the picture, sampled at every push: the grey values along a line, one row per frame, are a time
// stack; the field's component across the line against time is the Hovmoeller picture, its integral along the line the
// transport, the stretches above a threshold the jets; the correlation of each grey row with the one `lag` pushes later gives
// the drift along the line.  include/rcflow.h ("transects") is the specification; tests/_transects_ref.py states it in numpy.
// Everything up to the accumulators and the Q sums is integer and held to that bit for bit; the score, the peak and the
// velocity are double, the samples and means float (a stored float within one unit in the last place).  A push is one launch
// when no output is asked for, else up to three, and nothing synchronises:
//   transects@0  sample     a block a line.  The lanes take the line's samples from the frame and the field (bilinear on the
//                           1/16-pixel positions of the table) into the rings' slot of this push.  With a correlation range
//                           the block first brings the four grey rows it needs into LDS as packed bytes: the pushed row and
//                           the one `lag` pushes before it (the pair that comes in), the row the push overwrites and the
//                           one `lag` pushes after that (the pair that goes out, computed again instead of kept).  The older
//                           row of a pair lies in LDS shifted by D, so the interior begins at dword 0 and a zero tail ends it.
//                           A task is (four neighbouring shifts, eight dwords of the interior): per dword of A it reads ONE
//                           new dword of B, builds the byte-shifted ones with v_alignbyte_b32 and does v_dot4_u32_u8 for Tab,
//                           Tb (against ones under the interior) and Tbb, for both pairs; the difference goes to 32-bit words
//                           in LDS by integer atomics (exact in any order), and from there once into the int64 accumulators.
//                           A block owns its line's columns of the ring: no block overwrites what another reads;
//   transects@1  records    a block a line: a lane a shift for the scores in double; a lane a sample for the window mean
//                           (sequential float sum over the held rows, oldest first) and its Q; the exact sums by integer
//                           atomics in LDS; the first lane scans the line's Q for the jets and writes the record; the launch's
//                           last block writes the summary behind the fenced ticket;
//   transects@2  pictures   a lane a pixel of the time stack and of the Hovmoeller picture, rows oldest first.

#include <math.h>
#include <string.h>

#include <vector>

#include "rc_host.h"
#include "rc_reduce.h"

#define TS_ROW (RC_TRANSECTS_MAX_SAMPLES / 4 + 16)   // dwords of a grey row in LDS: the samples and a zero tail the last tasks read
#define TS_CH 8                                      // transects@0: dwords of the interior a task covers
#define TS_MAXNW (3 * (2 * RC_TRANSECTS_MAX_RANGE + 1) + 2)
#define TS_BADQ ((long long)0x8000000000000000ull)   // transects@1: the Q of a bad sample
static_assert(sizeof(rc_transect) == 64 && sizeof(rc_transect_sample) == 16 && sizeof(rc_transect_geom) == 48 && sizeof(rc_transect_line) == 20,
              "the records of include/rcflow.h have the sizes the Python and numpy mirrors give them");
static_assert(RC_TRANSECTS_MAX_TOTAL == RC_TRANSECTS_MAX_LINES * RC_TRANSECTS_MAX_SAMPLES, "the bounds fit each other");

struct TsCtl { unsigned ticket, cnt[4], pad[3]; };   // zero between launches

// ============================================================================ transects@0: sampling, rings, accumulators
struct TsSampleArgs {
    const rc_transect_sample* table; const rc_transect_geom* geom;
    const uint8_t* gray; size_t step;            // or null
    const float* flow; size_t flow_step;         // or null
    uint8_t* ring_g; float2* ring_f;             // [T][S]
    long long* acc;                              // [L][nw], or null (no correlation)
    int w, h, S, T, D, nw;
    int c;                                       // the slot of this push
    int slot_a;                                  // the pair that comes in: its older row's slot, or -1 (fewer than lag pushes so far)
    int slot_ob;                                 // the pair that goes out: its newer row's slot (the older one is c), or -1 (the ring is not full)
};

__device__ __forceinline__ uint32_t ts_ones(int valid) {         // 0x01 in the first `valid` bytes of a dword
    return valid >= 4 ? 0x01010101u : (valid <= 0 ? 0u : (0x01010101u & ((1u << (8 * valid)) - 1u)));
}

// one pair's share of a task: four shifts' Tab, Tb, Tbb over dwords [k0, k1) of the interior.  A: the older row shifted by D,
// B: the newer one from its dword g on
__device__ __forceinline__ void ts_pair(const uint32_t* A, const uint32_t* B, int k0, int k1, int ni, int sign, int* out) {
    uint32_t ab[4] = {0, 0, 0, 0}, b1[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
    uint32_t lo = B[k0];
    for (int k = k0; k < k1; k++) {
        const uint32_t hi = B[k + 1], av = A[k], one = ts_ones(ni - 4 * k), full = one * 255u;
        const uint32_t v0 = lo, v1 = __builtin_amdgcn_alignbyte(hi, lo, 1), v2 = __builtin_amdgcn_alignbyte(hi, lo, 2),
                       v3 = __builtin_amdgcn_alignbyte(hi, lo, 3);
        ab[0] = __builtin_amdgcn_udot4(av, v0, ab[0], false); b1[0] = __builtin_amdgcn_udot4(v0, one, b1[0], false); bb[0] = __builtin_amdgcn_udot4(v0, v0 & full, bb[0], false);
        ab[1] = __builtin_amdgcn_udot4(av, v1, ab[1], false); b1[1] = __builtin_amdgcn_udot4(v1, one, b1[1], false); bb[1] = __builtin_amdgcn_udot4(v1, v1 & full, bb[1], false);
        ab[2] = __builtin_amdgcn_udot4(av, v2, ab[2], false); b1[2] = __builtin_amdgcn_udot4(v2, one, b1[2], false); bb[2] = __builtin_amdgcn_udot4(v2, v2 & full, bb[2], false);
        ab[3] = __builtin_amdgcn_udot4(av, v3, ab[3], false); b1[3] = __builtin_amdgcn_udot4(v3, one, b1[3], false); bb[3] = __builtin_amdgcn_udot4(v3, v3 & full, bb[3], false);
        lo = hi;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) { out[3 * u] += sign * (int)ab[u]; out[3 * u + 1] += sign * (int)b1[u]; out[3 * u + 2] += sign * (int)bb[u]; }
}

__global__ __launch_bounds__(RC_BLOCK) void k_ts_sample(const TsSampleArgs a) {
    // the rows as packed bytes: 0 A of the pair that comes in, 1 its B (the pushed row), 2 A of the pair that goes out, 3 its B
    __shared__ uint32_t rows[4][TS_ROW];
    __shared__ int part[TS_MAXNW];
    const rc_transect_geom gm = a.geom[blockIdx.x];
    const int n = gm.n, first = gm.first, D = a.D, ni = n - 2 * D;
    const bool corr = a.acc != nullptr, in = corr && a.slot_a >= 0, out = corr && a.slot_ob >= 0;
    if (corr) {
        for (int i = threadIdx.x; i < 4 * TS_ROW; i += RC_BLOCK) (&rows[0][0])[i] = 0u;
        if (threadIdx.x < TS_MAXNW) part[threadIdx.x] = 0;
        __syncthreads();
    }
    uint8_t* const r8 = (uint8_t*)&rows[0][0];
    for (int j = threadIdx.x; j < n; j += RC_BLOCK) {
        const size_t s = (size_t)first + j;
        const rc_transect_sample sm = a.table[s];
        const int ix = sm.X >> 4, fx = sm.X & 15, iy = sm.Y >> 4, fy = sm.Y & 15;
        const int ix1 = min(ix + 1, a.w - 1), iy1 = min(iy + 1, a.h - 1);
        if (a.gray) {
            const uint8_t* r0 = a.gray + (size_t)iy * a.step;
            const uint8_t* r1 = a.gray + (size_t)iy1 * a.step;
            const int g = ((16 - fx) * (16 - fy) * r0[ix] + fx * (16 - fy) * r0[ix1] + (16 - fx) * fy * r1[ix] + fx * fy * r1[ix1] + 128) >> 8;
            uint8_t* slot = a.ring_g + (size_t)a.c * a.S + s;
            if (corr) {
                const bool inner = j >= D && j < n - D;
                if (in) {
                    if (inner) r8[j - D] = a.ring_g[(size_t)a.slot_a * a.S + s];
                    r8[4 * TS_ROW + j] = (uint8_t)g;
                }
                if (out) {                                        // this lane reads the old row's sample before it writes the new one
                    if (inner) r8[8 * TS_ROW + j - D] = *slot;
                    r8[12 * TS_ROW + j] = a.ring_g[(size_t)a.slot_ob * a.S + s];
                }
            }
            *slot = (uint8_t)g;
        }
        if (a.flow) {
            const float2* f0 = (const float2*)((const char*)a.flow + (size_t)iy * a.flow_step);
            const float2* f1 = (const float2*)((const char*)a.flow + (size_t)iy1 * a.flow_step);
            const float2 p00 = f0[ix], p10 = f0[ix1], p01 = f1[ix], p11 = f1[ix1];
            const float fa = fx / 16.f, fb = fy / 16.f;
            const float tu = p00.x + fa * (p10.x - p00.x), bu = p01.x + fa * (p11.x - p01.x), u = tu + fb * (bu - tu);
            const float tv = p00.y + fa * (p10.y - p00.y), bv = p01.y + fa * (p11.y - p01.y), v = tv + fb * (bv - tv);
            float2 o;
            o.x = (u * gm.ex + v * gm.ey) * gm.scale;
            o.y = (u * gm.nx + v * gm.ny) * gm.scale;
            a.ring_f[(size_t)a.c * a.S + s] = o;
        }
    }
    if (!in && !out) return;
    __syncthreads();
    // ---- the correlation: a task is (a group of four shifts, TS_CH dwords of the interior), both pairs
    const int ND = 2 * D + 1, ng = (ND + 3) / 4, n4 = (ni + 3) / 4, nch = (n4 + TS_CH - 1) / TS_CH;
    for (int t = threadIdx.x; t < ng * nch; t += RC_BLOCK) {
        const int ch = t / ng, g = t - ch * ng, k0 = ch * TS_CH, k1 = min(k0 + TS_CH, n4);
        int d[12];
#pragma unroll
        for (int e = 0; e < 12; e++) d[e] = 0;
        if (in) ts_pair(rows[0], rows[1] + g, k0, k1, ni, 1, d);
        if (out) ts_pair(rows[2], rows[3] + g, k0, k1, ni, -1, d);
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (4 * g + u < ND) {
#pragma unroll
                for (int e = 0; e < 3; e++)
                    if (d[3 * u + e]) atomicAdd(&part[3 * (4 * g + u) + e], d[3 * u + e]);
            }
        if (g == 0) {                                             // Ta, Taa: the zero tail of A adds nothing
            int ta = 0, taa = 0;
            for (int k = k0; k < k1; k++) {
                if (in) {
                    const uint32_t v = rows[0][k];
                    ta += (int)__builtin_amdgcn_udot4(v, 0x01010101u, 0u, false); taa += (int)__builtin_amdgcn_udot4(v, v, 0u, false);
                }
                if (out) {
                    const uint32_t v = rows[2][k];
                    ta -= (int)__builtin_amdgcn_udot4(v, 0x01010101u, 0u, false); taa -= (int)__builtin_amdgcn_udot4(v, v, 0u, false);
                }
            }
            if (ta) atomicAdd(&part[3 * ND], ta);
            if (taa) atomicAdd(&part[3 * ND + 1], taa);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.nw) a.acc[(size_t)blockIdx.x * a.nw + threadIdx.x] += (long long)part[threadIdx.x];
}

// ============================================================================ transects@1: velocity, transport, jets, records
struct TsRecArgs {
    const rc_transect_geom* geom;
    const float2* ring_f;                        // or null (no FLOW)
    const long long* acc;                        // or null (no correlation)
    rc_transect* rec; long long* sums; long long* summary;       // the state's copy
    rc_transect* rec2; long long* sums2; long long* summary2;    // the caller's, or null
    float2* profile;                             // or null
    TsCtl* ctl;
    int L, S, T, D, nw, lag, held, oldest, pairs;
    double fps;
    long long qmin, pushes;
};

// doubles round operation by operation (-ffp-contract=off) in the order of tests/_transects_ref.py
__device__ __forceinline__ double ts_root(double s) { return copysign(sqrt(fabs(s)), s); }

__global__ __launch_bounds__(RC_BLOCK) void k_ts_records(const TsRecArgs a) {
    __shared__ long long q[RC_TRANSECTS_MAX_SAMPLES];
    __shared__ double sc[2 * RC_TRANSECTS_MAX_RANGE + 1];
    __shared__ unsigned long long red[5];        // Fpos, Fneg, Ft, n_valid, bad
    __shared__ int last;
    const int line = blockIdx.x;
    const rc_transect_geom gm = a.geom[line];
    const int n = gm.n, D = a.D, ND = 2 * D + 1;
    const long long N = (long long)a.pairs * (n - 2 * D);
    if (threadIdx.x < 5) red[threadIdx.x] = 0ull;
    const long long* t = a.acc ? a.acc + (size_t)line * a.nw : nullptr;
    if (a.pairs > 0 && (int)threadIdx.x < ND) {                   // a lane a shift
        const long long Ta = t[3 * ND], Taa = t[3 * ND + 1], Tab = t[3 * threadIdx.x], Tb = t[3 * threadIdx.x + 1], Tbb = t[3 * threadIdx.x + 2];
        const long long num = N * Tab - Ta * Tb, va = N * Taa - Ta * Ta, vb = N * Tbb - Tb * Tb;
        double s = 0.;
        if (va > 0 && vb > 0) {
            const double nd = (double)num;
            s = (nd * fabs(nd)) / ((double)va * (double)vb);
        }
        sc[threadIdx.x] = s;
    }
    __syncthreads();
    // ---- a lane a sample: the window mean, its Q, the line's exact sums
    for (int j = threadIdx.x; j < n; j += RC_BLOCK) {
        long long qn = TS_BADQ;
        if (a.ring_f) {
            const float2* p = a.ring_f + (size_t)gm.first + j;
            float sx = 0.f, sy = 0.f;
            // oldest first: the slots from `oldest` to the ring's end, then those from its start; the loads of a run do not
            // depend on the sums, so several are in flight while the additions keep their order
            const int run = min(a.held, a.T - a.oldest);
            const float2* p0 = p + (size_t)a.oldest * a.S;
#pragma unroll 8
            for (int r = 0; r < run; r++) {
                const float2 f = p0[(size_t)r * a.S];
                sx += f.x; sy += f.y;
            }
#pragma unroll 8
            for (int r = 0; r < a.held - run; r++) {
                const float2 f = p[(size_t)r * a.S];
                sx += f.x; sy += f.y;
            }
            const float hf = (float)a.held, mt = sx / hf, mn = sy / hf;
            if (a.profile) { float2 o; o.x = mt; o.y = mn; a.profile[(size_t)gm.first + j] = o; }
            if (fabsf(mt) < 1048576.f && fabsf(mn) < 1048576.f) {     // NaN and infinity fail
                qn = (long long)rint((double)mn * 65536.);
                const long long qt = (long long)rint((double)mt * 65536.);
                atomicAdd(&red[qn > 0 ? 0 : 1], (unsigned long long)qn);
                atomicAdd(&red[2], (unsigned long long)qt);
                atomicAdd(&red[3], 1ull);
            } else {
                atomicAdd(&red[4], 1ull);
            }
        } else if (a.profile) {
            float2 o; o.x = 0.f; o.y = 0.f;
            a.profile[(size_t)gm.first + j] = o;
        }
        q[j] = qn;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long sm[RC_TRANSECTS_SUMS];
    for (int k = 0; k < RC_TRANSECTS_SUMS; k++) sm[k] = 0;
    rc_transect r;
    memset(&r, 0, sizeof(r));
    r.pairs = a.pairs;
    // ---- the velocity along the line
    if (a.pairs == 0) {
        r.flags = RC_TRANSECTS_EMPTY;
    } else {
        int best = 0;
        bool any = false;
        for (int d = 0; d < ND; d++) {
            if (sc[d] != 0.) any = true;
            if (sc[d] > sc[best]) best = d;                       // the first largest
        }
        if (!any) {
            r.flags = RC_TRANSECTS_FLAT;
        } else {
            const double rq = ts_root(sc[best]);
            double delta = 0.;
            if (best > 0 && best < 2 * D) {
                const double rl = ts_root(sc[best - 1]), rr = ts_root(sc[best + 1]);
                const double den = (rl - 2. * rq) + rr;
                if (den < 0.) delta = (0.5 * (rl - rr)) / den;
            } else {
                r.flags = RC_TRANSECTS_EDGE;
            }
            r.peak_shift = best - D;
            r.v_along = (float)(((((double)(best - D) + delta) * gm.ds) * a.fps) / (double)a.lag);
            r.corr_peak = (float)rq;
            const long long Ta = t[3 * ND], Taa = t[3 * ND + 1], Tab = t[3 * best], Tb = t[3 * best + 1], Tbb = t[3 * best + 2];
            sm[12] = N * Tab - Ta * Tb; sm[13] = N * Taa - Ta * Ta; sm[14] = N * Tbb - Tb * Tb; sm[15] = best;
        }
    }
    sm[11] = N;
    // ---- the transport across it and the jets
    const long long Fpos = (long long)red[0], Fneg = (long long)red[1], Ft = (long long)red[2], nv = (long long)red[3], bad = (long long)red[4];
    int jets = 0, jstart = 0, jlen = 0, jat = 0;
    long long jsum = 0, jpeak = 0;
    if (a.ring_f) {
        int run0 = -1, pat = 0;
        long long rsum = 0, rpeak = 0;
        for (int j = 0; j <= n; j++) {
            const bool inside = j < n && q[j] != TS_BADQ && q[j] >= a.qmin;
            if (inside) {
                if (run0 < 0) { run0 = j; rsum = 0; rpeak = q[j]; pat = j; }
                rsum += q[j];
                if (q[j] > rpeak) { rpeak = q[j]; pat = j; }
            } else if (run0 >= 0) {
                if (jets == 0 || rsum > jsum) { jstart = run0; jlen = j - run0; jsum = rsum; jpeak = rpeak; jat = pat; }
                jets++;
                run0 = -1;
            }
        }
    }
    sm[0] = Fpos; sm[1] = Fneg; sm[2] = Ft; sm[3] = nv; sm[4] = bad; sm[5] = jets; sm[6] = jstart; sm[7] = jlen; sm[8] = jsum; sm[9] = jpeak;
    sm[10] = jat;
    if (nv > 0) {
        r.mean_along = (float)(((double)Ft / 65536.) / (double)nv);
        r.mean_cross = (float)(((double)(Fpos + Fneg) / 65536.) / (double)nv);
    }
    r.flux_out = (float)(((double)Fpos / 65536.) * gm.ds);
    r.flux_in = (float)(((double)Fneg / 65536.) * gm.ds);
    r.jets = jets; r.jet_start = jstart; r.jet_len = jlen; r.jet_peak_at = jat;
    r.jet_flux = (float)(((double)jsum / 65536.) * gm.ds);
    r.jet_peak = (float)((double)jpeak / 65536.);
    r.bad = (int)bad;
    a.rec[line] = r;
    if (a.rec2) a.rec2[line] = r;
    for (int k = 0; k < RC_TRANSECTS_SUMS; k++) {
        a.sums[(size_t)line * RC_TRANSECTS_SUMS + k] = sm[k];
        if (a.sums2) a.sums2[(size_t)line * RC_TRANSECTS_SUMS + k] = sm[k];
    }
    if (!(r.flags & (RC_TRANSECTS_EMPTY | RC_TRANSECTS_FLAT))) rc_acc_add(&a.ctl->cnt[0], 1u);
    if (jets) { rc_acc_add(&a.ctl->cnt[1], 1u); rc_acc_add(&a.ctl->cnt[2], (unsigned)jets); }
    if (bad) rc_acc_add(&a.ctl->cnt[3], (unsigned)bad);
    last = rc_ticket_fenced(&a.ctl->ticket, (unsigned)a.L);       // the counts before the ticket
    if (last) {
        long long s[8] = {a.held, a.pairs, 0, 0, 0, 0, a.pushes, 0};
        for (int k = 0; k < 4; k++) s[2 + k] = rc_acc_take(&a.ctl->cnt[k]);     // zero for the next push (stream order)
        rc_acc_take(&a.ctl->ticket);
        for (int k = 0; k < 8; k++) {
            a.summary[k] = s[k];
            if (a.summary2) a.summary2[k] = s[k];
        }
    }
}

// ============================================================================ transects@2: the pictures
struct TsPicArgs {
    const uint8_t* ring_g; const float2* ring_f;
    uint8_t* stack; size_t stack_step;           // or null
    uint8_t* hov; size_t hov_step;               // or null
    const uint8_t* jet;
    int S, T, held, oldest;
    float vis_max;
};

__global__ __launch_bounds__(RC_BLOCK) void k_ts_pictures(const TsPicArgs a) {
    const int s = blockIdx.x * RC_BLOCK + threadIdx.x, r = blockIdx.y;
    if (s >= a.S) return;
    int slot = a.oldest + r;
    if (slot >= a.T) slot -= a.T;
    const bool have = r < a.held;
    if (a.stack) a.stack[(size_t)r * a.stack_step + s] = have ? a.ring_g[(size_t)slot * a.S + s] : (uint8_t)0;
    if (a.hov) {
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (have) {
            const float un = a.ring_f[(size_t)slot * a.S + s].y;
            if (fabsf(un) <= FLT_MAX) {                           // finite
                const float f = rintf(un / a.vis_max * 127.5f + 127.5f);
                const int i = !(f > 0.f) ? 0 : (f > 255.f ? 255 : (int)f);
                c0 = a.jet[3 * i]; c1 = a.jet[3 * i + 1]; c2 = a.jet[3 * i + 2];
            }
        }
        uint8_t* o = a.hov + (size_t)r * a.hov_step + 3 * (size_t)s;
        o[0] = c0; o[1] = c1; o[2] = c2;
    }
}

// ============================================================================ host side
static bool ts_pos(double v) { return v > 0. && v <= 1.7976931348623157e308; }      // finite and > 0; NaN fails
static bool ts_jet(double v) { return v > 0. && v < 1048576.; }                      // a mean of 2^20 or more is bad and in no jet: such a threshold says nothing
static bool ts_fin(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

int rc_line_plan(const char* who, int w, int h, const rc_transect_line& l, int i, int first, double metres_per_pixel, double fps,
                 rc_transect_sample* table, rc_transect_geom* geom) {
    const double x0 = l.x0, y0 = l.y0, x1 = l.x1, y1 = l.y1;
    if (!ts_fin(x0) || !ts_fin(y0) || !ts_fin(x1) || !ts_fin(y1)) { rc_set_error("%s: line %d has an endpoint that is not finite", who, i); return RC_EINVAL; }
    const double dx = x1 - x0, dy = y1 - y0, len = hypot(dx, dy);
    if (!(len > 0.) || !ts_fin(len)) { rc_set_error("%s: line %d has no length", who, i); return RC_EINVAL; }
    for (int j = 0; j < l.n; j++) {
        const double t = (double)j / (double)(l.n - 1), x = x0 + dx * t, y = y0 + dy * t;
        const double X = rint(16. * x), Y = rint(16. * y);
        if (!(X >= 0. && X <= 16. * (w - 1) && Y >= 0. && Y <= 16. * (h - 1))) {
            rc_set_error("%s: sample %d of line %d lies at (%g, %g), outside the %d x %d picture", who, j, i, x, y, w, h);
            return RC_EINVAL;
        }
        if (table) {
            rc_transect_sample& s = table[first + j];
            s.X = (int)X; s.Y = (int)Y; s.line = i; s.offset = j;
        }
    }
    if (geom) {
        rc_transect_geom& g = geom[i];
        g.first = first; g.n = l.n;
        g.ex = (float)(dx / len); g.ey = (float)(dy / len);
        g.nx = (float)(dy / len); g.ny = (float)(-dx / len);
        g.scale = (float)(metres_per_pixel * fps);
        g.pad = 0;
        g.len = len;
        g.ds = (len * metres_per_pixel) / (double)(l.n - 1);
    }
    return RC_OK;
}

extern "C" int rcflow_transects_plan(int w, int h, const rc_transect_line* lines, int n_lines, double metres_per_pixel, double fps,
                                     rc_transect_sample* table, rc_transect_geom* geom, int* total) {
    static const char* who = "rcflow_transects_plan";
    if (w <= 0 || h <= 0 || !lines || n_lines < 1 || n_lines > RC_TRANSECTS_MAX_LINES || !ts_pos(metres_per_pixel) || !ts_pos(fps)) {
        rc_set_error("%s: a picture of %d x %d, %d lines (1..%d), fps and metres_per_pixel finite and > 0", who, w, h, n_lines, RC_TRANSECTS_MAX_LINES);
        return RC_EINVAL;
    }
    long long S = 0;
    for (int i = 0; i < n_lines; i++) {
        const rc_transect_line& l = lines[i];
        if (l.n < 2 || l.n > RC_TRANSECTS_MAX_SAMPLES) {
            rc_set_error("%s: line %d has %d samples (2..%d)", who, i, l.n, RC_TRANSECTS_MAX_SAMPLES);
            return RC_EINVAL;
        }
        S += l.n;
    }
    if (S > RC_TRANSECTS_MAX_TOTAL) {
        rc_set_error("%s: %lld samples in all (at most %d)", who, S, RC_TRANSECTS_MAX_TOTAL);
        return RC_EINVAL;
    }
    int first = 0;
    for (int i = 0; i < n_lines; i++) {
        if (int rc = rc_line_plan(who, w, h, lines[i], i, first, metres_per_pixel, fps, table, geom)) return rc;
        first += lines[i].n;
    }
    if (total) *total = first;
    return RC_OK;
}

void rc_state_free(RcTransects& v) {
    rc_buf_free(v.table); rc_buf_free(v.ring_g); rc_buf_free(v.ring_f); rc_buf_free(v.acc); rc_buf_free(v.out); rc_buf_free(v.ctl);
    rc_buf_free(v.jet);
    rc_fence_free(v.zf);
    v = RcTransects();
}

// open and reset: the rings, the accumulators, the last push's outputs, the counters; the push count
int rc_state_zero(RcSlot& s, RcTransects& v) {
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.ring_g, &v.ring_f, &v.acc, &v.out, &v.ctl});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

// RcTransects::table: samples [S] | geometry [L]
static const rc_transect_sample* ts_table(const RcTransects& v) { return (const rc_transect_sample*)v.table.p; }
static const rc_transect_geom* ts_geom(const RcTransects& v) { return (const rc_transect_geom*)(ts_table(v) + v.S); }
// RcTransects::out: records [L] | sums [L][RC_TRANSECTS_SUMS] | summary 8 int64
static rc_transect* ts_out_rec(const RcTransects& v) { return (rc_transect*)v.out.p; }
static long long* ts_out_sums(const RcTransects& v) { return (long long*)(ts_out_rec(v) + v.L); }
static long long* ts_out_summary(const RcTransects& v) { return ts_out_sums(v) + (size_t)v.L * RC_TRANSECTS_SUMS; }
static int ts_pairs(const RcTransects& v, long long pushes) {
    if (v.prm.range < 1) return 0;
    const long long held = pushes < v.prm.window ? pushes : v.prm.window;
    return held > v.prm.lag ? (int)(held - v.prm.lag) : 0;
}

extern "C" int rcflow_transects_open(rc_ctx* ctx, int stream, int w, int h, const rc_transect_line* lines, int n_lines,
                                     const rc_transects_params* prm) {
    static const char* who = "rcflow_transects_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad frame size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    const int T = prm->window, D = prm->range, src = prm->sources;
    if (T < 2 || T > RC_TRANSECTS_MAX_WINDOW || src < 1 || src > (RC_TRANSECTS_GRAY | RC_TRANSECTS_FLOW) || prm->lag < 1 ||
        prm->lag > RC_TRANSECTS_MAX_LAG || D < 0 || D > RC_TRANSECTS_MAX_RANGE || prm->flags || !ts_pos(prm->fps) || !ts_pos(prm->metres_per_pixel) ||
        !ts_jet(prm->jet_min) || !ts_pos(prm->vis_max) || (D >= 1 && (!(src & RC_TRANSECTS_GRAY) || T <= prm->lag))) {
        rc_set_error("%s: window 2..%d, sources RC_TRANSECTS_GRAY, RC_TRANSECTS_FLOW or both, lag 1..%d, range 0..%d (a range needs GRAY and "
                     "window > lag), flags 0, fps, metres_per_pixel and vis_max finite and > 0, jet_min > 0 and below 2^20", who, RC_TRANSECTS_MAX_WINDOW,
                     RC_TRANSECTS_MAX_LAG, RC_TRANSECTS_MAX_RANGE);
        return RC_EINVAL;
    }
    int S = 0;
    int rc = rcflow_transects_plan(w, h, lines, n_lines, prm->metres_per_pixel, prm->fps, nullptr, nullptr, &S);
    if (rc) return rc;
    if (D >= 1)
        for (int i = 0; i < n_lines; i++)
            if (lines[i].n < 2 * D + 8) {
                rc_set_error("%s: line %d has %d samples, a range of %d needs %d", who, i, lines[i].n, D, 2 * D + 8);
                return RC_EINVAL;
            }
    rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    const unsigned long long per = ((src & RC_TRANSECTS_GRAY) ? 1ull : 0ull) + ((src & RC_TRANSECTS_FLOW) ? 8ull : 0ull), state = per * T * S;
    if (state > RC_TRANSECTS_MAX_STATE_BYTES) {
        rc_set_error("%s: %d rows of %d samples are %llu bytes of ring, more than RC_TRANSECTS_MAX_STATE_BYTES", who, T, S, state);
        return RC_ESIZE;
    }
    RcTransects n;
    n.w = w; n.h = h; n.prm = *prm; n.L = n_lines; n.S = S;
    n.nw = 3 * (2 * D + 1) + 2;
    std::vector<unsigned char> host((size_t)S * sizeof(rc_transect_sample) + (size_t)n_lines * sizeof(rc_transect_geom));
    (void)rcflow_transects_plan(w, h, lines, n_lines, prm->metres_per_pixel, prm->fps, (rc_transect_sample*)host.data(),
                                (rc_transect_geom*)(host.data() + (size_t)S * sizeof(rc_transect_sample)), nullptr);
    RC_HIP(hipSetDevice(ctx->device));
    rc = rc_buf_ensure(n.table, host.size());
    if (!rc && (src & RC_TRANSECTS_GRAY)) rc = rc_buf_ensure(n.ring_g, (size_t)T * S);
    if (!rc && (src & RC_TRANSECTS_FLOW)) rc = rc_buf_ensure(n.ring_f, (size_t)T * S * 8);
    if (!rc && D >= 1) rc = rc_buf_ensure(n.acc, (size_t)n_lines * n.nw * 8);
    if (!rc) rc = rc_buf_ensure(n.out, (size_t)n_lines * (sizeof(rc_transect) + RC_TRANSECTS_SUMS * 8) + 64);
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(TsCtl));
    if (!rc) rc = rc_buf_ensure(n.jet, 768);
    if (!rc) {
        uint8_t lut[768];
        rcflow_jet_lut(lut);
        if (hipMemcpy(n.jet.p, lut, 768, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(n.table.p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            rc_set_error("%s: the upload of the tables failed", who);
            rc = RC_EHIP;
        }
    }
    return rc_state_install(*s, s->ts, n, rc);
}

extern "C" int rcflow_transects_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, const float* d_flow_xy, size_t flow_step,
                                         rc_transect* d_records, long long* d_sums, float* d_profile, uint8_t* d_stack, size_t stack_step,
                                         uint8_t* d_hov, size_t hov_step, long long* d_summary) {
    static const char* who = "rcflow_transects_push_dev";
    RcSlot* s; RcTransects* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ts, who, s, vp)) return rc;
    RcTransects& v = *vp;
    const int w = v.w, h = v.h, T = v.prm.window, D = v.prm.range, lag = v.prm.lag, S = v.S, L = v.L;
    const bool gray = (v.prm.sources & RC_TRANSECTS_GRAY) != 0, flow = (v.prm.sources & RC_TRANSECTS_FLOW) != 0;
    if ((d_gray != nullptr) != gray || (d_flow_xy != nullptr) != flow) {
        rc_set_error("%s: the session was opened for %s%s%s: a push supplies exactly those inputs", who, gray ? "d_gray" : "", gray && flow ? " and " : "",
                     flow ? "d_flow_xy" : "");
        return RC_EINVAL;
    }
    if ((d_stack && !gray) || (d_hov && !flow)) {
        rc_set_error("%s: d_stack needs RC_TRANSECTS_GRAY, d_hov needs RC_TRANSECTS_FLOW", who);
        return RC_EINVAL;
    }
    RcArgsN<8> a(who, w, h);
    a.image("d_gray", d_gray, step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    a.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN | RC_ARG_OPTIONAL);
    a.array("d_records", d_records, (size_t)L * sizeof(rc_transect), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_sums", d_sums, (size_t)L * RC_TRANSECTS_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.array("d_profile", d_profile, (size_t)S * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    a.image("d_stack", d_stack, stack_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL, S, T);
    a.image("d_hov", d_hov, hov_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL, S, T);
    a.array("d_summary", d_summary, 64, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const long long p = v.pushes, pushes = p + 1;
    const int c = (int)(p % T);
    {
        TsSampleArgs q;
        q.table = ts_table(v); q.geom = ts_geom(v);
        q.gray = d_gray; q.step = step; q.flow = d_flow_xy; q.flow_step = flow_step;
        q.ring_g = (uint8_t*)v.ring_g.p; q.ring_f = (float2*)v.ring_f.p;
        q.acc = D >= 1 ? (long long*)v.acc.p : nullptr;
        q.w = w; q.h = h; q.S = S; q.T = T; q.D = D; q.nw = v.nw; q.c = c;
        q.slot_a = p >= lag ? (int)((p - lag) % T) : -1;
        q.slot_ob = p >= T ? (c + lag) % T : -1;
        // the four pixels of a sample in, its ring entries out; the rows of the two pairs in, the accumulators in and out
        RcProfScope ps(ctx, s->cur, RC_K_TRANSECTS, 0, (double)S * ((gray ? 5. : 0.) + (flow ? 40. : 0.) + (D >= 1 ? 3. : 0.)) + (D >= 1 ? 16. * L * v.nw : 0.));
        hipLaunchKernelGGL(k_ts_sample, dim3(L), dim3(RC_BLOCK), 0, s->cur, q);
    }
    const long long held = pushes < T ? pushes : T;
    const int oldest = pushes >= T ? (int)(pushes % T) : 0;
    if (d_records || d_sums || d_profile || d_summary) {
        TsRecArgs q;
        q.geom = ts_geom(v); q.ring_f = flow ? (const float2*)v.ring_f.p : nullptr; q.acc = D >= 1 ? (const long long*)v.acc.p : nullptr;
        q.rec = ts_out_rec(v); q.sums = ts_out_sums(v); q.summary = ts_out_summary(v);
        q.rec2 = d_records; q.sums2 = d_sums; q.summary2 = d_summary; q.profile = (float2*)d_profile;
        q.ctl = (TsCtl*)v.ctl.p;
        q.L = L; q.S = S; q.T = T; q.D = D; q.nw = v.nw; q.lag = lag; q.held = (int)held; q.oldest = oldest; q.pairs = ts_pairs(v, pushes);
        q.fps = v.prm.fps;
        q.qmin = (long long)rint(v.prm.jet_min * 65536.);         // below 2^36: jet_min is below 2^20
        q.pushes = pushes;
        RcProfScope ps(ctx, s->cur, RC_K_TRANSECTS, 1, (flow ? 8. * S * held : 0.) + (D >= 1 ? 8. * L * v.nw : 0.) + L * (64. + 8. * RC_TRANSECTS_SUMS) + (d_profile ? 8. * S : 0.));
        hipLaunchKernelGGL(k_ts_records, dim3(L), dim3(RC_BLOCK), 0, s->cur, q);
    }
    if (d_stack || d_hov) {
        TsPicArgs q;
        q.ring_g = (const uint8_t*)v.ring_g.p; q.ring_f = (const float2*)v.ring_f.p;
        q.stack = d_stack; q.stack_step = stack_step; q.hov = d_hov; q.hov_step = hov_step;
        q.jet = (const uint8_t*)v.jet.p;
        q.S = S; q.T = T; q.held = (int)held; q.oldest = oldest; q.vis_max = (float)v.prm.vis_max;
        RcProfScope ps(ctx, s->cur, RC_K_TRANSECTS, 2, (double)S * ((d_stack ? held + (double)T : 0.) + (d_hov ? 8. * held + 3. * T : 0.)));
        hipLaunchKernelGGL(k_ts_pictures, dim3((S + RC_BLOCK - 1) / RC_BLOCK, T), dim3(RC_BLOCK), 0, s->cur, q);
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                            // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_transects_read(rc_ctx* ctx, int stream, rc_transect* records, long long summary[8]) {
    RcSlot* s; RcTransects* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ts, "rcflow_transects_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    if (records) RC_HIP(hipMemcpyAsync(records, ts_out_rec(*vp), (size_t)vp->L * sizeof(rc_transect), hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, ts_out_summary(*vp), 64, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_transects_sums_read(rc_ctx* ctx, int stream, long long* sums, long long* line_sums) {
    RcSlot* s; RcTransects* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ts, "rcflow_transects_sums_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t row = (size_t)vp->nw * 8, head = row - 16;
    if (vp->prm.range < 1) {                                      // no correlation, no accumulators: the one shift's sums are zero
        if (sums) memset(sums, 0, (size_t)vp->L * head);
        if (line_sums) memset(line_sums, 0, (size_t)vp->L * 16);
        RC_HIP(hipStreamSynchronize(s->cur));
        return RC_OK;
    }
    if (sums) RC_HIP(hipMemcpy2DAsync(sums, head, vp->acc.p, row, head, vp->L, hipMemcpyDeviceToHost, s->cur));
    if (line_sums) RC_HIP(hipMemcpy2DAsync(line_sums, 16, (const char*)vp->acc.p + head, row, 16, vp->L, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_transects_table_read(rc_ctx* ctx, int stream, rc_transect_sample* table, rc_transect_geom* geom) {
    RcSlot* s; RcTransects* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ts, "rcflow_transects_table_read", s, vp)) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    if (table) RC_HIP(hipMemcpyAsync(table, ts_table(*vp), (size_t)vp->S * sizeof(rc_transect_sample), hipMemcpyDeviceToHost, s->cur));
    if (geom) RC_HIP(hipMemcpyAsync(geom, ts_geom(*vp), (size_t)vp->L * sizeof(rc_transect_geom), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_transects_set(rc_ctx* ctx, int stream, double jet_min, double vis_max) {
    RcSlot* s; RcTransects* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ts, "rcflow_transects_set", s, vp)) return rc;
    if (!ts_jet(jet_min) || !ts_pos(vis_max)) {
        rc_set_error("rcflow_transects_set: jet_min > 0 and below 2^20, vis_max finite and > 0");
        return RC_EINVAL;
    }
    vp->prm.jet_min = jet_min; vp->prm.vis_max = vis_max;
    return RC_OK;
}

extern "C" int rcflow_transects_info(rc_ctx* ctx, int stream, rc_transects_info* info) {
    RcSlot* s; RcTransects* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::ts, "rcflow_transects_info", s, vp)) return rc;
    const RcTransects& v = *vp;
    if (!info) { rc_set_error("rcflow_transects_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->lines = v.L; info->samples = v.S;
    info->launches_per_push = RC_TRANSECTS_LAUNCHES;
    info->held = (int)(v.pushes < v.prm.window ? v.pushes : v.prm.window);
    info->pairs = ts_pairs(v, v.pushes);
    info->pushes = v.pushes;
    info->device_bytes = v.table.bytes + v.ring_g.bytes + v.ring_f.bytes + v.acc.bytes + v.out.bytes + v.ctl.bytes + v.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_transects_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::ts, "rcflow_transects_reset"); }
extern "C" int rcflow_transects_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::ts); }
