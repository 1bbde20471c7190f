// drifters_kernels.hip -- virtual drifters: from where on this beach is a swimmer carried out, where does the rest end, and how fast?
//
// A population of up to RC_DRIFTERS_MAX points kept on the device, 24 bytes each as six int32 planes: home and position in 1/64
// pixel, age, state.  A push releases the waiting (and, with RC_DRIFTERS_RESPAWN, the dead) at their homes, moves the living through
// the field by the four-vector gather in exact integers, and lets them die by a named fate: an edge, a bad vector, old age, a zone
// of the caller's byte map (shore, offshore, ...).  What it keeps: the visit density per pixel, two tables of RC_DRIFTERS_SUMS int64
// per cell of the opposing-flow map's grid (by the place a thing happened, by the home of the drifter it happened to), residence-time
// histograms and a summary.  include/rcflow.h ("drifters") is the specification; tests/_drifters_ref.py states it in numpy and the
// kernels are held to that bit for bit: every sum is an integer atomic, so no result depends on the order of addition.  A push is
// two launches and nothing synchronises:
//   drifters@0  a thread a drifter.  The scattered adds: what shares a destination is summed in the wave first.  Neighbouring
//               drifters start as neighbours and end in a few pixels, so a wave's lanes fall into a few runs of consecutive lanes
//               that share a cell (or a pixel): each run is folded towards its first lane, which issues one atomic per word that
//               is not zero.  The summary and the histograms (152 words) meet in LDS and leave as one atomic per word the block
//               touched.  The tables are cumulative since open / reset, so nothing is taken back between pushes but the count of
//               the living;
//   drifters@1  a thread four pixels of a row: the push's occupancy into the density, and zero again (only where something was);
//               the four pictures.  The same launch closes the records, the tables' copies and the summary, grid-strided over its
//               threads: all of it reads what drifters@0 left, which stream order puts before this launch, so no block waits for another
//               and there is no ticket;
//   drifters@2  rcflow_drifters_zones_dev, stateless: the shoreline's wet mask and the surf zone's mask into the push's byte map.

#include <math.h>
#include <string.h>

#include <vector>

#include "rc_host.h"
#include "rc_reduce.h"

static_assert(sizeof(rc_drifters_cell) == 32 && sizeof(rc_drifters_params) == 40, "the records of include/rcflow.h have the sizes the mirrors give them");
static_assert(RC_DRIFTERS_SUMS == 8 && RC_DRIFTERS_SUMMARY == 24 && RC_DRIFTERS_HIST_BINS == 32, "the words of a cell, the summary, a histogram");
#define DR_PLANES 6            // HX | HY | X | Y | age | st, [max_drifters] int32 each
#define DR_HIST (4 * RC_DRIFTERS_HIST_BINS)
#define DR_LT (RC_DRIFTERS_SUMMARY + DR_HIST)     // a block's words in LDS: the summary's, then the histograms'

// RcDrifters::ctl: the living of the push under way, added by drifters@0 and taken by drifters@1
struct DrCtl { unsigned long long alive; unsigned pad[30]; };
static_assert(sizeof(DrCtl) == 128, "a line");

typedef __attribute__((address_space(3))) unsigned long long dr_lds_u64;   // said to be in LDS: no flat atomic
typedef unsigned dr_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dr_lds_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add((dr_lds_u64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// 0 SHORE, 1 OFFSHORE, 2 EDGE, 3 other
__device__ __forceinline__ int dr_class(int fate) {
    return fate == RC_DRIFTERS_SHORE ? 0 : fate == RC_DRIFTERS_OFFSHORE ? 1 : fate <= RC_DRIFTERS_EDGE_BOTTOM ? 2 : 3;
}

// the runs of consecutive lanes with one key: rc_run and rc_run_sum of rc_reduce.h
// key: the lane's cell, -1 for none (its v is zero then).  One atomic per run and word that is not zero
__device__ __forceinline__ void dr_cell_add(long long* tab, int key, const long long (&v)[RC_DRIFTERS_SUMS], int lane) {
    if (!__any(key >= 0)) return;
    bool head;
    const int end = rc_run(key, lane, head);
#pragma unroll
    for (int k = 0; k < RC_DRIFTERS_SUMS; k++) {
        if (!__any(v[k] != 0)) continue;
        const long long s = rc_run_sum(v[k], lane, end);
        if (head && key >= 0 && s) rc_acc_add(tab + (size_t)RC_DRIFTERS_SUMS * key + k, s);
    }
}

// ============================================================================ drifters@0: release, move, fates, the scattered adds
struct DrArgs0 {
    const float* flow; size_t flow_step;
    const uint8_t* zone; size_t zone_step;       // or null: every byte 0
    int32_t* S;                                  // the six planes, `cap` apart
    int cap, n;
    unsigned* occ; int P;                        // [h][P]: this push's occupancy, zero between pushes
    long long* place; long long* origin;         // [cells][RC_DRIFTERS_SUMS] each, cumulative
    unsigned long long* hist;                    // [4][RC_DRIFTERS_HIST_BINS], cumulative
    long long* tot;                              // the summary's cumulative words, in the summary's places
    DrCtl* ctl;
    float* xy; int32_t* age_out; uint8_t* state_out;          // each output or null
    int w, h, gx, gy, cw, ch;
    int dt_q, max_age, age_bin, respawn;
};

__global__ __launch_bounds__(RC_BLOCK) void k_dr_move(const DrArgs0 a) {
    __shared__ unsigned long long lt[DR_LT];
    for (int i = threadIdx.x; i < DR_LT; i += RC_BLOCK) lt[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    int pkey = -1, okey = -1, opx = -1;
    long long pv[RC_DRIFTERS_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0}, ov[RC_DRIFTERS_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool alive = false, rel = false;
    if (i < a.n) {
        int32_t* const S = a.S + i;
        const size_t cap = (size_t)a.cap;
        const int HX = S[0], HY = S[cap];
        int X = S[2 * cap], Y = S[3 * cap], age = S[4 * cap], st = S[5 * cap];
        rel = st == -1 || (st > 0 && a.respawn);
        const bool mov = st == 0;
        if (rel || mov) {
            int fate = 0, su = 0, sv = 0;
            if (rel) {
                X = HX; Y = HY; age = 0;
            } else {
                // the four-vector gather: positions are inside 0..64 (w-1) x 0..64 (h-1), so ix <= w - 1 and iy <= h - 1
                const int ix = X >> 6, fx = X & 63, iy = Y >> 6, fy = Y & 63;
                const int x1 = min(ix + 1, a.w - 1), y1 = min(iy + 1, a.h - 1);
                const int wt[4] = {(64 - fx) * (64 - fy), fx * (64 - fy), (64 - fx) * fy, fx * fy};
                const int cx[4] = {ix, x1, ix, x1}, cy[4] = {iy, iy, y1, y1};
                int Du = 0, Dv = 0;
                bool bad = false;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (wt[k] == 0) continue;             // a corner of weight 0 is not looked at
                    const float2 f = *(const float2*)((const char*)a.flow + (size_t)cy[k] * a.flow_step + 8 * (size_t)cx[k]);
                    if (!(fabsf(f.x) < 500.0f && fabsf(f.y) < 500.0f)) { bad = true; continue; }     // NaN and the infinities fail the comparison
                    Du += wt[k] * (int)rintf(f.x * 64.0f);        // 4096 * 32000 in all
                    Dv += wt[k] * (int)rintf(f.y * 64.0f);
                }
                if (bad) {
                    fate = RC_DRIFTERS_BAD;
                } else {
                    su = (int)(((long long)Du * a.dt_q + (1ll << 19)) >> 20);     // floor; at most 2^27 * 2^16 / 2^20
                    sv = (int)(((long long)Dv * a.dt_q + (1ll << 19)) >> 20);
                }
            }
            const long long Tx = (long long)X + su, Ty = (long long)Y + sv;
            if (fate == 0) {
                if (Tx < 0) fate = RC_DRIFTERS_EDGE_LEFT;
                else if (Tx > 64ll * (a.w - 1)) fate = RC_DRIFTERS_EDGE_RIGHT;
                else if (Ty < 0) fate = RC_DRIFTERS_EDGE_TOP;
                else if (Ty > 64ll * (a.h - 1)) fate = RC_DRIFTERS_EDGE_BOTTOM;
            }
            bool takeT = false;
            if (fate == 0 && a.zone) {                            // T is inside the picture here, its pixel too
                const int z = min((int)a.zone[(size_t)((Ty + 32) >> 6) * a.zone_step + (size_t)((Tx + 32) >> 6)], 7);
                if (z > 0) { fate = RC_DRIFTERS_ZONE + z; takeT = true; }
            }
            if (mov) age++;
            if (mov && fate == 0 && a.max_age > 0 && age >= a.max_age) { fate = RC_DRIFTERS_AGED; takeT = true; }
            alive = fate == 0;
            if (alive || takeT) { X = (int)Tx; Y = (int)Ty; }
            st = fate;
            S[2 * cap] = X; S[3 * cap] = Y; S[4 * cap] = age; S[5 * cap] = st;
            // what is booked, and where
            const int px = (X + 32) >> 6, py = (Y + 32) >> 6;
            const int pc = min(py / a.ch, a.gy - 1) * a.gx + min(px / a.cw, a.gx - 1);
            const int oc = min(((HY + 32) >> 6) / a.ch, a.gy - 1) * a.gx + min(((HX + 32) >> 6) / a.cw, a.gx - 1);
            pkey = pc;
            if (rel) { okey = oc; ov[0] = 1; }
            if (alive) {
                opx = py * a.P + px;
                pv[0] = 1; pv[1] = su; pv[2] = sv;
            } else {
                const int c = dr_class(fate);
                okey = oc;
                pv[3 + c] = 1; ov[1 + c] = 1;
                if (c == 0) { ov[5] = age; dr_lds_add(lt + 4, (unsigned long long)age); }
                if (c == 1) { pv[7] = age; ov[6] = age; dr_lds_add(lt + 5, (unsigned long long)age); }
                dr_lds_add(lt + 8 + fate, 1ull);
                dr_lds_add(lt + RC_DRIFTERS_SUMMARY + c * RC_DRIFTERS_HIST_BINS + min(RC_DRIFTERS_HIST_BINS - 1, age / a.age_bin), 1ull);
            }
        }
        if (a.xy) ((float2*)a.xy)[i] = make_float2((float)X / 64.0f, (float)Y / 64.0f);
        if (a.age_out) a.age_out[i] = age;
        if (a.state_out) a.state_out[i] = (uint8_t)(st < 0 ? 255 : st);
    }
    // the wave's counts and its scattered adds; every lane is here
    const unsigned long long am = __ballot(alive), rm = __ballot(rel);
    if (lane == 0) {
        if (am) dr_lds_add(lt + 1, (unsigned long long)__popcll(am));
        if (rm) dr_lds_add(lt + 2, (unsigned long long)__popcll(rm));
    }
    if (am) {                                                     // the occupancy: a run of lanes on one pixel adds its length
        bool head;
        const int end = rc_run(opx, lane, head);
        if (head && opx >= 0) rc_acc_add(a.occ + opx, (unsigned)(end - lane + 1));
    }
    dr_cell_add(a.place, pkey, pv, lane);
    dr_cell_add(a.origin, okey, ov, lane);
    __syncthreads();
    for (int k = threadIdx.x; k < DR_LT; k += RC_BLOCK) {
        const unsigned long long v = lt[k];
        if (!v) continue;
        if (k == 1) rc_acc_add(&a.ctl->alive, v);
        else if (k < RC_DRIFTERS_SUMMARY) rc_acc_add(a.tot + k, (long long)v);
        else rc_acc_add(a.hist + (k - RC_DRIFTERS_SUMMARY), v);
    }
}

// ============================================================================ drifters@1: density, pictures, records, summary
struct DrArgs1 {
    unsigned* occ; unsigned* dens; int P;
    uint16_t* now; size_t now_step;              // each output or null; the steps in bytes
    uint32_t* density; size_t density_step;
    uint8_t* live; size_t live_step;
    uint8_t* pic; size_t pic_step;
    const uint8_t* jet;                          // 768 bytes
    const long long* place; const long long* origin; const unsigned long long* hist; const long long* tot;
    DrCtl* ctl;
    long long* summary; rc_drifters_cell* cells;                          // the state's copy
    long long* summary2; rc_drifters_cell* cells2; long long* place2; long long* origin2; unsigned long long* hist2;      // the caller's, or null
    int w, h, ncells;
    unsigned live_min; unsigned long long density_full;
    long long n, pushes;
};

__global__ __launch_bounds__(RC_BLOCK) void k_dr_pixels(const DrArgs1 a) {
    __shared__ uint8_t jet[768];
    if (a.pic) {
        rc_stage_jet(jet, a.jet);
        __syncthreads();
    }
    const int G = a.P / 4;
    const long long g = (long long)blockIdx.x * RC_BLOCK + threadIdx.x, groups = (long long)G * a.h;
    if (g < groups) {
        const int y = (int)(g / G), x0 = 4 * (int)(g % G);
        const int nv = min(4, a.w - x0);                          // >= 1: P - w < 4
        const size_t o = (size_t)y * a.P + x0;
        const dr_u4 oc = *(const dr_u4*)(a.occ + o);
        const bool any = (oc[0] | oc[1] | oc[2] | oc[3]) != 0u;
        dr_u4 d = {0u, 0u, 0u, 0u};
        if (any || a.density || a.pic) d = *(const dr_u4*)(a.dens + o);
        if (any) {
            d += oc;
            *(dr_u4*)(a.dens + o) = d;
            *(dr_u4*)(a.occ + o) = (dr_u4){0u, 0u, 0u, 0u};
        }
        if (a.now) {
            uint16_t* q = (uint16_t*)((char*)a.now + (size_t)y * a.now_step) + x0;
            const unsigned m[4] = {min(oc[0], 65535u), min(oc[1], 65535u), min(oc[2], 65535u), min(oc[3], 65535u)};
            if (nv == 4) {
                const uint2 v = make_uint2(m[0] | (m[1] << 16), m[2] | (m[3] << 16));
                __builtin_memcpy(q, &v, 8);
            } else {
                for (int j = 0; j < nv; j++) q[j] = (uint16_t)m[j];
            }
        }
        if (a.density) {
            uint32_t* q = (uint32_t*)((char*)a.density + (size_t)y * a.density_step) + x0;
            if (nv == 4) __builtin_memcpy(q, &d, 16);
            else
                for (int j = 0; j < nv; j++) q[j] = d[j];
        }
        if (a.live) {
            uint8_t* q = a.live + (size_t)y * a.live_step + x0;
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) m |= (oc[j] >= a.live_min ? 255u : 0u) << (8 * j);
            if (nv == 4) __builtin_memcpy(q, &m, 4);
            else
                for (int j = 0; j < nv; j++) q[j] = (uint8_t)(m >> (8 * j));
        }
        if (a.pic) {
            uint8_t* q = a.pic + (size_t)y * a.pic_step + 3 * (size_t)x0;
            uint32_t px[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned long long e = (unsigned long long)d[j] * 255ull / a.density_full;
                const uint8_t* c = jet + 3 * (e > 255ull ? 255u : (unsigned)e);
                px[j] = d[j] ? (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) : 0u;
            }
            if (nv == 4) {
                const uint32_t wd[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
                __builtin_memcpy(q, wd, 12);
            } else {
                for (int j = 0; j < nv; j++) { q[3 * j] = (uint8_t)px[j]; q[3 * j + 1] = (uint8_t)(px[j] >> 8); q[3 * j + 2] = (uint8_t)(px[j] >> 16); }
            }
        }
    }
    // the records, the tables' copies and the summary: over the launch's threads, from what drifters@0 left
    const long long T = (long long)gridDim.x * RC_BLOCK;
    for (long long c = g; c < a.ncells; c += T) {
        long long pl[RC_DRIFTERS_SUMS], og[RC_DRIFTERS_SUMS];
#pragma unroll
        for (int k = 0; k < RC_DRIFTERS_SUMS; k++) { pl[k] = a.place[RC_DRIFTERS_SUMS * c + k]; og[k] = a.origin[RC_DRIFTERS_SUMS * c + k]; }
        if (a.place2)
#pragma unroll
            for (int k = 0; k < RC_DRIFTERS_SUMS; k++) a.place2[RC_DRIFTERS_SUMS * c + k] = pl[k];
        if (a.origin2)
#pragma unroll
            for (int k = 0; k < RC_DRIFTERS_SUMS; k++) a.origin2[RC_DRIFTERS_SUMS * c + k] = og[k];
        rc_drifters_cell r;
        memset(&r, 0, sizeof(r));
        if (pl[0] == 0 && og[0] == 0) r.flags = RC_DRIFTERS_EMPTY;
        if (pl[0] > 0) {
            r.mean_u = (float)(((double)pl[1] / 64.0) / (double)pl[0]);
            r.mean_v = (float)(((double)pl[2] / 64.0) / (double)pl[0]);
        }
        const long long deaths = og[1] + og[2] + og[3] + og[4];
        if (deaths > 0) {
            r.escape = (float)((double)og[2] / (double)deaths);
            r.beached = (float)((double)og[1] / (double)deaths);
        }
        if (og[2] > 0) r.mean_exit_age = (float)((double)og[6] / (double)og[2]);
        a.cells[c] = r;
        if (a.cells2) a.cells2[c] = r;
    }
    if (a.hist2)
        for (long long k = g; k < DR_HIST; k += T) a.hist2[k] = a.hist[k];
    if (g != 0) return;
    long long s[RC_DRIFTERS_SUMMARY];
    for (int k = 0; k < RC_DRIFTERS_SUMMARY; k++) s[k] = a.tot[k];
    s[0] = a.n; s[1] = (long long)rc_acc_take(&a.ctl->alive); s[3] = a.pushes; s[6] = s[7] = 0;
    for (int k = 0; k < RC_DRIFTERS_SUMMARY; k++) {
        a.summary[k] = s[k];
        if (a.summary2) a.summary2[k] = s[k];
    }
}

// ============================================================================ drifters@2: the zones helper
__global__ __launch_bounds__(RC_BLOCK) void k_dr_zones(const uint8_t* wet, size_t wet_step, const uint8_t* inside, size_t inside_step, int w, int h,
                                                       uint8_t* zone, size_t zone_step) {
    const int x = blockIdx.x * RC_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    uint8_t z = 0;
    if (inside && inside[(size_t)y * inside_step + x] == 0) z = 2;
    if (wet && wet[(size_t)y * wet_step + x] == 0) z = 1;
    zone[(size_t)y * zone_step + x] = z;
}

// ============================================================================ host side
void rc_state_free(RcDrifters& v) {
    rc_buf_free(v.st); rc_buf_free(v.occ); rc_buf_free(v.dens); rc_buf_free(v.tab); rc_buf_free(v.stat); rc_buf_free(v.out); rc_buf_free(v.ctl);
    rc_buf_free(v.jet);
    rc_fence_free(v.zf);
    v = RcDrifters();
}

static int32_t* dr_plane(const RcDrifters& v, int k) { return (int32_t*)v.st.p + (size_t)k * v.prm.max_drifters; }
static size_t dr_cells(const RcDrifters& v) { return (size_t)v.prm.grid_x * v.prm.grid_y; }
// RcDrifters::tab: by place | by origin, [cells][RC_DRIFTERS_SUMS] int64 each.  ::stat: the summary's cumulative words | the histograms.
// ::out: summary RC_DRIFTERS_SUMMARY int64 | records [cells]
static long long* dr_place(const RcDrifters& v) { return (long long*)v.tab.p; }
static long long* dr_origin(const RcDrifters& v) { return dr_place(v) + dr_cells(v) * RC_DRIFTERS_SUMS; }
static long long* dr_tot(const RcDrifters& v) { return (long long*)v.stat.p; }
static unsigned long long* dr_hist(const RcDrifters& v) { return (unsigned long long*)v.stat.p + RC_DRIFTERS_SUMMARY; }
static long long* dr_out_summary(const RcDrifters& v) { return (long long*)v.out.p; }
static rc_drifters_cell* dr_out_cells(const RcDrifters& v) { return (rc_drifters_cell*)((long long*)v.out.p + RC_DRIFTERS_SUMMARY); }

// open and reset: every drifter waits at its home; the occupancy, the density, the tables, the histograms, the last push's outputs
// and the count of the living go to zero; the push count.  All on the slot's stream, before the fence's event
int rc_state_zero(RcSlot& s, RcDrifters& v) {
    if (v.n) {
        const size_t bytes = (size_t)v.n * 4;
        RC_HIP(hipMemcpyAsync(dr_plane(v, 2), dr_plane(v, 0), bytes, hipMemcpyDeviceToDevice, s.cur));
        RC_HIP(hipMemcpyAsync(dr_plane(v, 3), dr_plane(v, 1), bytes, hipMemcpyDeviceToDevice, s.cur));
        RC_HIP(hipMemsetAsync(dr_plane(v, 4), 0, bytes, s.cur));
        RC_HIP(hipMemsetAsync(dr_plane(v, 5), 0xff, bytes, s.cur));       // -1: waiting
    }
    const int rc = rc_fence_zero(v.zf, s.cur, {&v.occ, &v.dens, &v.tab, &v.stat, &v.out, &v.ctl});
    if (rc) return rc;
    v.pushes = 0;
    return RC_OK;
}

static int dr_dt_q(double dt) {                                   // rint(dt * 256) in 1..65536, or 0
    if (!(dt > 0. && dt <= 256.)) return 0;                       // NaN fails
    const double q = rint(dt * 256.0);
    return q >= 1. && q <= 65536. ? (int)q : 0;
}
static bool dr_settable(const rc_drifters_params& p) {
    return dr_dt_q(p.dt) && p.max_age >= 0 && p.density_full >= 1 && p.live_min >= 1 && !(p.flags & ~RC_DRIFTERS_RESPAWN);
}
static const char* dr_settable_text = "dt with rint(dt * 256) in 1..65536, max_age >= 0, density_full >= 1, live_min >= 1, flags 0 or RC_DRIFTERS_RESPAWN";

extern "C" int rcflow_drifters_open(rc_ctx* ctx, int stream, int w, int h, const rc_drifters_params* prm) {
    static const char* who = "rcflow_drifters_open";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!prm || w <= 0 || h <= 0) { rc_set_error("%s: bad field size %d x %d or no parameters", who, w, h); return RC_EINVAL; }
    if (prm->max_drifters < 1 || prm->max_drifters > RC_DRIFTERS_MAX || prm->age_bin < 1 || !dr_settable(*prm)) {
        rc_set_error("%s: max_drifters 1..%d, age_bin >= 1, %s", who, RC_DRIFTERS_MAX, dr_settable_text);
        return RC_EINVAL;
    }
    if (prm->grid_x < 1 || prm->grid_y < 1 || prm->grid_x > w || prm->grid_y > h || (long long)prm->grid_x * prm->grid_y > RC_RIPMAP_MAX_CELLS) {
        rc_set_error("%s: grid %d x %d does not fit a %d x %d field (at most %d cells)", who, prm->grid_x, prm->grid_y, w, h, RC_RIPMAP_MAX_CELLS);
        return RC_EINVAL;
    }
    int rc = rc_fits_context(who, ctx, w, h);
    if (rc) return rc;
    RcDrifters n;
    n.w = w; n.h = h; n.prm = *prm;
    n.P = (w + 3) & ~3;
    RC_HIP(hipSetDevice(ctx->device));
    const size_t nc = dr_cells(n), px = (size_t)n.P * h;
    rc = rc_buf_ensure(n.st, (size_t)DR_PLANES * prm->max_drifters * 4);
    if (!rc) rc = rc_buf_ensure(n.occ, px * 4);
    if (!rc) rc = rc_buf_ensure(n.dens, px * 4);
    if (!rc) rc = rc_buf_ensure(n.tab, 2 * nc * RC_DRIFTERS_SUMS * 8);
    if (!rc) rc = rc_buf_ensure(n.stat, (size_t)DR_LT * 8);
    if (!rc) rc = rc_buf_ensure(n.out, RC_DRIFTERS_SUMMARY * 8 + nc * sizeof(rc_drifters_cell));
    if (!rc) rc = rc_buf_ensure(n.ctl, sizeof(DrCtl));
    if (!rc) rc = rc_jet_ensure(n.jet, who);
    return rc_state_install(*s, s->dr, n, rc);
}

extern "C" int rcflow_drifters_seed(rc_ctx* ctx, int stream, const double* xy, int n) {
    static const char* who = "rcflow_drifters_seed";
    RcSlot* s; RcDrifters* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::dr, who, s, vp)) return rc;
    RcDrifters& v = *vp;
    if (!xy || n < 1) { rc_set_error("%s: no points", who); return RC_EINVAL; }
    if (n > v.prm.max_drifters - v.n) {
        rc_set_error("%s: the session holds %d of %d drifters, %d more do not fit", who, v.n, v.prm.max_drifters, n);
        return RC_ESIZE;
    }
    std::vector<int32_t> q(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        if (!(x >= 0. && x <= (double)(v.w - 1) && y >= 0. && y <= (double)(v.h - 1))) {          // NaN fails
            rc_set_error("%s: point %d (%g, %g) is not finite or lies outside the %d x %d picture", who, i, x, y, v.w, v.h);
            return RC_EINVAL;
        }
        q[i] = (int32_t)llrint(x * 64.0);
        q[(size_t)n + i] = (int32_t)llrint(y * 64.0);
    }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const size_t bytes = (size_t)n * 4;
    RC_HIP(hipMemcpyAsync(dr_plane(v, 0) + v.n, q.data(), bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemcpyAsync(dr_plane(v, 1) + v.n, q.data() + n, bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemcpyAsync(dr_plane(v, 2) + v.n, q.data(), bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemcpyAsync(dr_plane(v, 3) + v.n, q.data() + n, bytes, hipMemcpyHostToDevice, s->cur));
    RC_HIP(hipMemsetAsync(dr_plane(v, 4) + v.n, 0, bytes, s->cur));
    RC_HIP(hipMemsetAsync(dr_plane(v, 5) + v.n, 0xff, bytes, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));                     // q is this call's
    v.n += n;
    return RC_OK;
}

extern "C" int rcflow_drifters_push_dev(rc_ctx* ctx, int stream, const float* d_flow_xy, size_t flow_step, const uint8_t* d_zone, size_t zone_step,
                                        uint16_t* d_now, size_t now_step, uint32_t* d_density, size_t density_step, uint8_t* d_live,
                                        size_t live_step, uint8_t* d_picture, size_t picture_step, float* d_xy, int32_t* d_age, uint8_t* d_state,
                                        rc_drifters_cell* d_cells, long long* d_place, long long* d_origin, unsigned long long* d_hist,
                                        long long* d_summary) {
    static const char* who = "rcflow_drifters_push_dev";
    RcSlot* s; RcDrifters* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::dr, who, s, vp)) return rc;
    RcDrifters& v = *vp;
    const int w = v.w, h = v.h;
    const size_t nc = dr_cells(v), n = (size_t)v.n;
    if (!v.n) { rc_set_error("%s: no drifter has been seeded (rcflow_drifters_seed comes first)", who); return RC_ESTATE; }
    if (!d_flow_xy) {                                         // the slot's resident field (rcflow_stream_flow_ptr), as rcflow_meanflow_push_dev
        if (!s->flow_w) { rc_set_error("%s: no flow field is resident on the slot yet", who); return RC_ESTATE; }
        if (s->flow_w != w || s->flow_h != h) {
            rc_set_error("%s: the resident flow field is %d x %d, the session %d x %d", who, s->flow_w, s->flow_h, w, h);
            return RC_ESIZE;
        }
        d_flow_xy = (const float*)s->stage_flow.p;
        flow_step = (size_t)w * 8;
    }
    RcArgsN<14> ar(who, w, h);
    ar.image("d_flow_xy", d_flow_xy, flow_step, 8, 8, RC_ARG_IN);
    ar.image("d_zone", d_zone, zone_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_now", d_now, now_step, 2, 2, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_density", d_density, density_step, 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_live", d_live, live_step, 1, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.image("d_picture", d_picture, picture_step, 3, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_xy", d_xy, n * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_age", d_age, n * 4, 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_state", d_state, n, 1, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_cells", d_cells, nc * sizeof(rc_drifters_cell), 4, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_place", d_place, nc * RC_DRIFTERS_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_origin", d_origin, nc * RC_DRIFTERS_SUMS * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_hist", d_hist, DR_HIST * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    ar.array("d_summary", d_summary, RC_DRIFTERS_SUMMARY * 8, 8, RC_ARG_OUT | RC_ARG_OPTIONAL);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(v.zf, s->cur, true);
    if (rc) return rc;
    const rc_drifters_params& q = v.prm;
    const long long pushes = v.pushes + 1;
    {
        DrArgs0 a;
        a.flow = d_flow_xy; a.flow_step = flow_step; a.zone = d_zone; a.zone_step = zone_step;
        a.S = (int32_t*)v.st.p; a.cap = q.max_drifters; a.n = v.n;
        a.occ = (unsigned*)v.occ.p; a.P = v.P;
        a.place = dr_place(v); a.origin = dr_origin(v); a.hist = dr_hist(v); a.tot = dr_tot(v); a.ctl = (DrCtl*)v.ctl.p;
        a.xy = d_xy; a.age_out = d_age; a.state_out = d_state;
        a.w = w; a.h = h; a.gx = q.grid_x; a.gy = q.grid_y; a.cw = w / q.grid_x; a.ch = h / q.grid_y;
        a.dt_q = dr_dt_q(q.dt); a.max_age = q.max_age; a.age_bin = q.age_bin; a.respawn = (q.flags & RC_DRIFTERS_RESPAWN) != 0;
        // the state 24 in and 16 out; the four vectors; the occupancy word and three cell words in and out; the outputs
        RcProfScope ps(ctx, s->cur, RC_K_DRIFTERS, 0, (double)n * (40. + 32. + 8. + 48. + (d_xy ? 8. : 0.) + (d_age ? 4. : 0.) + (d_state ? 1. : 0.)));
        hipLaunchKernelGGL(k_dr_move, dim3((unsigned)((n + RC_BLOCK - 1) / RC_BLOCK)), dim3(RC_BLOCK), 0, s->cur, a);
    }
    {
        DrArgs1 a;
        a.occ = (unsigned*)v.occ.p; a.dens = (unsigned*)v.dens.p; a.P = v.P;
        a.now = d_now; a.now_step = now_step; a.density = d_density; a.density_step = density_step; a.live = d_live; a.live_step = live_step;
        a.pic = d_picture; a.pic_step = picture_step; a.jet = (const uint8_t*)v.jet.p;
        a.place = dr_place(v); a.origin = dr_origin(v); a.hist = dr_hist(v); a.tot = dr_tot(v); a.ctl = (DrCtl*)v.ctl.p;
        a.summary = dr_out_summary(v); a.cells = dr_out_cells(v);
        a.summary2 = d_summary; a.cells2 = d_cells; a.place2 = d_place; a.origin2 = d_origin; a.hist2 = d_hist;
        a.w = w; a.h = h; a.ncells = (int)nc;
        a.live_min = (unsigned)q.live_min; a.density_full = (unsigned long long)q.density_full;
        a.n = v.n; a.pushes = pushes;
        const size_t groups = (size_t)(v.P / 4) * h;
        const double px = (double)v.P * h;
        // the occupancy in; where a drifter is, occupancy out and density in and out; the outputs (the density in for two of them)
        RcProfScope ps(ctx, s->cur, RC_K_DRIFTERS, 1, px * (4. + (d_density || d_picture ? 4. : 0.) + (d_now ? 2. : 0.) + (d_density ? 4. : 0.) +
                                                            (d_live ? 1. : 0.) + (d_picture ? 3. : 0.)) + (double)(n < (size_t)px ? n : (size_t)px) * 12. +
                                                           (double)nc * (128. + 32.));
        hipLaunchKernelGGL(k_dr_pixels, dim3((unsigned)((groups + RC_BLOCK - 1) / RC_BLOCK)), dim3(RC_BLOCK), 0, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    v.pushes = pushes;                                        // a launch that failed is not a push
    return RC_OK;
}

extern "C" int rcflow_drifters_read(rc_ctx* ctx, int stream, rc_drifters_cell* cells, long long* place, long long* origin, unsigned long long* hist,
                                    long long summary[RC_DRIFTERS_SUMMARY]) {
    RcSlot* s; RcDrifters* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::dr, "rcflow_drifters_read", s, vp)) return rc;
    const RcDrifters& v = *vp;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(vp->zf, s->cur, true);
    if (rc) return rc;
    const size_t nc = dr_cells(v);
    if (cells) RC_HIP(hipMemcpyAsync(cells, dr_out_cells(v), nc * sizeof(rc_drifters_cell), hipMemcpyDeviceToHost, s->cur));
    if (place) RC_HIP(hipMemcpyAsync(place, dr_place(v), nc * RC_DRIFTERS_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (origin) RC_HIP(hipMemcpyAsync(origin, dr_origin(v), nc * RC_DRIFTERS_SUMS * 8, hipMemcpyDeviceToHost, s->cur));
    if (hist) RC_HIP(hipMemcpyAsync(hist, dr_hist(v), DR_HIST * 8, hipMemcpyDeviceToHost, s->cur));
    if (summary) RC_HIP(hipMemcpyAsync(summary, dr_out_summary(v), RC_DRIFTERS_SUMMARY * 8, hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    return RC_OK;
}

extern "C" int rcflow_drifters_set(rc_ctx* ctx, int stream, double dt, int max_age, int density_full, int live_min, int flags) {
    RcSlot* s; RcDrifters* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::dr, "rcflow_drifters_set", s, vp)) return rc;
    rc_drifters_params p = vp->prm;
    p.dt = dt; p.max_age = max_age; p.density_full = density_full; p.live_min = live_min; p.flags = flags;
    if (!dr_settable(p)) {
        rc_set_error("rcflow_drifters_set: %s", dr_settable_text);
        return RC_EINVAL;
    }
    vp->prm = p;
    return RC_OK;
}

extern "C" int rcflow_drifters_info(rc_ctx* ctx, int stream, rc_drifters_info* info) {
    RcSlot* s; RcDrifters* vp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::dr, "rcflow_drifters_info", s, vp)) return rc;
    const RcDrifters& v = *vp;
    if (!info) { rc_set_error("rcflow_drifters_info: no buffer"); return RC_EINVAL; }
    memset(info, 0, sizeof(*info));
    info->w = v.w; info->h = v.h; info->prm = v.prm;
    info->launches_per_push = RC_DRIFTERS_LAUNCHES;
    info->drifters = v.n;
    info->pushes = v.pushes;
    info->device_bytes = v.st.bytes + v.occ.bytes + v.dens.bytes + v.tab.bytes + v.stat.bytes + v.out.bytes + v.ctl.bytes + v.jet.bytes;
    return RC_OK;
}

extern "C" int rcflow_drifters_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::dr, "rcflow_drifters_reset"); }
extern "C" int rcflow_drifters_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::dr); }

extern "C" int rcflow_drifters_zones_dev(rc_ctx* ctx, int stream, const uint8_t* d_wet, size_t wet_step, const uint8_t* d_inside, size_t inside_step,
                                         int w, int h, uint8_t* d_zone, size_t zone_step) {
    static const char* who = "rcflow_drifters_zones_dev";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (w <= 0 || h <= 0 || h > 65535) { rc_set_error("%s: bad picture size %d x %d", who, w, h); return RC_EINVAL; }
    if (!d_wet && !d_inside) { rc_set_error("%s: d_wet and d_inside are both null", who); return RC_EINVAL; }
    RcArgs ar(who, w, h);
    ar.image("d_wet", d_wet, wet_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_inside", d_inside, inside_step, 1, 1, RC_ARG_IN | RC_ARG_OPTIONAL);
    ar.image("d_zone", d_zone, zone_step, 1, 1, RC_ARG_OUT);
    if (ar.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    {
        RcProfScope ps(ctx, s->cur, RC_K_DRIFTERS, 2, (double)w * h * (1. + (d_wet ? 1. : 0.) + (d_inside ? 1. : 0.)));
        hipLaunchKernelGGL(k_dr_zones, dim3((w + RC_BLOCK - 1) / RC_BLOCK, h), dim3(RC_BLOCK), 0, s->cur, d_wet, wet_step, d_inside, inside_step, w, h,
                           d_zone, zone_step);
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}
