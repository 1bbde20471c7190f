// fit_kernels.hip -- what the tracks say: a motion fitted to point pairs by RANSAC with a counter-based sampler
// (rcflow_fit_motion_dev; the fit of the tracking stabiliser, stab_kernels.hip).  include/rcflow.h states every formula,
// constant and operation order; tests/_trackstab_ref.py restates them in numpy and the device is held to it bit for bit
// in everything that is an integer (samples, winner, counts, inlier bytes, the rung of the ladder).
//
// One launch.  Every workgroup compacts the valid pairs into LDS in input order (the prefix sum is redone per workgroup:
// at most 4096 entries), then each of its four waves takes one hypothesis: lane 0 draws the sample and solves it in fp64
// (the 8 x 8 elimination of a homography works on a matrix in LDS, so nothing is indexed in registers and the kernel has
// no scratch), the 64 lanes stride the points and the wave reduces the count.  The workgroup's best goes into one packed
// 64-bit maximum (count << 32 | ~index: most inliers, lowest index) and the workgroup that arrives LAST refits on the
// winner's inliers, recounts, refits again and walks the ladder.  The hand-off is rc_ticket_release (rc_reduce.h): agent-scope
// atomics, one release fence, the ticket, one acquire fence (DESIGN.md section 7c says why a plain flag is not enough).
//
// Sums of the refits run over the valid list in a fixed order, so they are a function of the input alone: thread t adds
// the terms of points t, t + 256, ... (0.0 for a point that is no inlier), a wave folds its 64 partial sums by the xor
// butterfly 32, 16, ... 1, and the four wave sums are added as ((w0 + w1) + w2) + w3.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_reduce.h"

#define FT_BLOCK 256
#define FT_WAVES (FT_BLOCK / 64)
#define FT_WAVE_DOUBLES 104              // per wave: the 8 x 9 system, z[8], E[9], T[9], ok, then 4 ints of the sample

struct RcFitArgs {
    const float2* p; const float2* q; const uint8_t* status; const int* scores;
    int n, ncap, chunk, model, hyp, min_score;
    unsigned seed;
    double quality, max_shift2, thr2, S, cx, cy, fcx, fcy;
    rc_fit_result* out; uint8_t* inlier; int* samples;
    unsigned long long* ws;              // [0] the packed best of the running launch, [1] its ticket; zero between launches
    double* res; double* res2;           // the stabiliser: centre displacement and inlier fraction (either may be null)
};

__device__ __forceinline__ unsigned ft_mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned ft_draw(unsigned seed, unsigned j, unsigned d) {
    return ft_mix32(ft_mix32(seed + 0x9E3779B9U * (j + 1u)) + 0x85EBCA6BU * (d + 1u));
}
__device__ __forceinline__ int ft_sample_size(int model) { return model; }                       // 1, 2, 3, 4 pairs
__device__ __forceinline__ int ft_need(int model) { return model == 1 ? 3 : 2 * model; }         // max(2 k, k + 2)

// sample of hypothesis j as indices into the valid list; false: void
__device__ bool ft_sample(unsigned seed, int j, int k, int nv, int* smp) {
    for (int i = 0; i < 4; i++) smp[i] = -1;
    if (nv < k) return false;
    int got = 0;
    for (unsigned d = 0; d < 16u && got < k; d++) {
        const int idx = (int)(((unsigned long long)ft_draw(seed, (unsigned)j, d) * (unsigned long long)(unsigned)nv) >> 32);
        bool dup = false;
        for (int i = 0; i < got; i++) dup |= smp[i] == idx;
        if (!dup) smp[got++] = idx;
    }
    if (got == k) return true;
    for (int i = 0; i < 4; i++) smp[i] = -1;
    return false;
}

struct FtPt { double Px, Py, Qx, Qy, Dx, Dy; };
__device__ __forceinline__ FtPt ft_norm(const RcFitArgs& a, const float4 v) {
    FtPt o;
    o.Px = ((double)v.x - a.cx) / a.S; o.Py = ((double)v.y - a.cy) / a.S;
    o.Qx = ((double)v.z - a.cx) / a.S; o.Qy = ((double)v.w - a.cy) / a.S;
    o.Dx = ((double)v.z - (double)v.x) / a.S; o.Dy = ((double)v.w - (double)v.y) / a.S;
    return o;
}

// E (normalised displacement matrix, T_norm - I) -> T in pixels, T = I + N^-1 E N; a homography is scaled to T[8] = 1
__device__ bool ft_to_pixels(const RcFitArgs& a, const double* E, double* T, bool persp) {
    double F[9], G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        F[3 * i] = E[3 * i] / a.S; F[3 * i + 1] = E[3 * i + 1] / a.S;
        F[3 * i + 2] = E[3 * i + 2] - (E[3 * i] * a.cx + E[3 * i + 1] * a.cy) / a.S;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        G[j] = a.S * F[j] + a.cx * F[6 + j];
        G[3 + j] = a.S * F[3 + j] + a.cy * F[6 + j];
        G[6 + j] = F[6 + j];
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; i++) { G[i] = ((i & 3) == 0 ? 1.0 : 0.0) + G[i]; ok = ok && isfinite(G[i]); }
    if (persp) {
        const double d = G[8];
        ok = ok && d > 0.1;
#pragma unroll
        for (int i = 0; i < 9; i++) G[i] = G[i] / d;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) T[i] = G[i];
    return ok;
}

// translation, similarity, affine from the means and the centred sums (the closed forms of st_fit, stab_kernels.hip)
__device__ bool ft_finish_lin(int model, double n, double mpx, double mpy, double mdx, double mdy, double sxx, double sxy, double syy,
                              double xdx, double ydx, double xdy, double ydy, double* E) {
    double b00 = 0., b01 = 0., b10 = 0., b11 = 0.;
    if (model == RC_STAB_AFFINE) {
        const double det = sxx * syy - sxy * sxy;
        if (!(n >= 3.) || !(det > 1e-12 * (sxx * syy))) return false;
        b00 = (xdx * syy - ydx * sxy) / det; b01 = (ydx * sxx - xdx * sxy) / det;
        b10 = (xdy * syy - ydy * sxy) / det; b11 = (ydy * sxx - xdy * sxy) / det;
    } else if (model == RC_STAB_SIMILARITY) {
        if (!(n >= 2.) || !(sxx + syy > 0.)) return false;
        const double sa = (xdx + ydy) / (sxx + syy), sb = (xdy - ydx) / (sxx + syy);
        b00 = sa; b01 = -sb; b10 = sb; b11 = sa;
    } else if (!(n >= 1.)) {
        return false;
    }
    E[0] = b00; E[1] = b01; E[2] = mdx - (b00 * mpx + b01 * mpy);
    E[3] = b10; E[4] = b11; E[5] = mdy - (b10 * mpx + b11 * mpy);
    E[6] = 0.; E[7] = 0.; E[8] = 0.;
    return true;
}

// Gaussian elimination with partial pivoting on M[8][9] (in LDS), first largest |pivot| on ties; false below tol
__device__ bool ft_ge8(double* M, double tol, double* z) {
    for (int c = 0; c < 8; c++) {
        int pr = c;
        double pv = fabs(M[c * 9 + c]);
        for (int r = c + 1; r < 8; r++) {
            const double v = fabs(M[r * 9 + c]);
            if (v > pv) { pv = v; pr = r; }
        }
        if (!(pv >= tol)) return false;
        if (pr != c)
            for (int k = 0; k < 9; k++) { const double t = M[c * 9 + k]; M[c * 9 + k] = M[pr * 9 + k]; M[pr * 9 + k] = t; }
        for (int r = c + 1; r < 8; r++) {
            const double f = M[r * 9 + c] / M[c * 9 + c];
            for (int k = c; k < 9; k++) M[r * 9 + k] = M[r * 9 + k] - f * M[c * 9 + k];
        }
    }
    for (int c = 7; c >= 0; c--) {
        double s = M[c * 9 + 8];
        for (int k = c + 1; k < 8; k++) s = s - M[c * 9 + k] * z[k];
        z[c] = s / M[c * 9 + c];
    }
    return true;
}
__device__ __forceinline__ void ft_z_to_E(const double* z, double* E) {
    for (int i = 0; i < 8; i++) E[i] = z[i];
    E[8] = 0.;
}

// one thread: sample, minimal solve, T in pixels.  wv: the wave's LDS (FT_WAVE_DOUBLES)
__device__ bool ft_hypothesis(const RcFitArgs& a, const float4* pts, int nv, int j, double* wv) {
    double* M = wv; double* z = wv + 72; double* E = wv + 80; double* T = wv + 89;
    int* smp = (int*)(wv + 100);
    const int k = ft_sample_size(a.model);
    if (!ft_sample(a.seed, j, k, nv, smp)) return false;
    if (a.model == RC_STAB_HOMOGRAPHY) {
        for (int i = 0; i < 4; i++) {
            const FtPt t = ft_norm(a, pts[smp[i]]);
            double* r1 = M + 18 * i; double* r2 = r1 + 9;
            r1[0] = t.Px; r1[1] = t.Py; r1[2] = 1.; r1[3] = 0.; r1[4] = 0.; r1[5] = 0.; r1[6] = -t.Qx * t.Px; r1[7] = -t.Qx * t.Py; r1[8] = t.Dx;
            r2[0] = 0.; r2[1] = 0.; r2[2] = 0.; r2[3] = t.Px; r2[4] = t.Py; r2[5] = 1.; r2[6] = -t.Qy * t.Px; r2[7] = -t.Qy * t.Py; r2[8] = t.Dy;
        }
        if (!ft_ge8(M, 1e-9, z)) return false;
        ft_z_to_E(z, E);
        return ft_to_pixels(a, E, T, true);
    }
    double spx = 0., spy = 0., sdx = 0., sdy = 0.;
    for (int i = 0; i < k; i++) {
        const FtPt t = ft_norm(a, pts[smp[i]]);
        spx += t.Px; spy += t.Py; sdx += t.Dx; sdy += t.Dy;
    }
    const double n = (double)k, mpx = spx / n, mpy = spy / n, mdx = sdx / n, mdy = sdy / n;
    double sxx = 0., sxy = 0., syy = 0., xdx = 0., ydx = 0., xdy = 0., ydy = 0.;
    for (int i = 0; i < k; i++) {
        const FtPt t = ft_norm(a, pts[smp[i]]);
        const double ux = t.Px - mpx, uy = t.Py - mpy, ex = t.Dx - mdx, ey = t.Dy - mdy;
        sxx += ux * ux; sxy += ux * uy; syy += uy * uy;
        xdx += ux * ex; ydx += uy * ex; xdy += ux * ey; ydy += uy * ey;
    }
    if (!ft_finish_lin(a.model, n, mpx, mpy, mdx, mdy, sxx, sxy, syy, xdx, ydx, xdy, ydy, E)) return false;
    return ft_to_pixels(a, E, T, false);
}

__device__ __forceinline__ bool ft_inlier(const double* T, const float4 v, double thr2) {
    const double px = (double)v.x, py = (double)v.y;
    const double X = (T[0] * px + T[1] * py) + T[2], Y = (T[3] * px + T[4] * py) + T[5], W = (T[6] * px + T[7] * py) + T[8];
    const double ex = X / W - (double)v.z, ey = Y / W - (double)v.w;
    const double e2 = ex * ex + ey * ey;
    return W > 0. && e2 <= thr2;
}

// every thread returns the workgroup's sum, in the fixed order of the file comment
__device__ __forceinline__ double ft_blk_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// marks the inliers of T (in wv) over the valid list; !ok: none
__device__ __forceinline__ void ft_mark(const RcFitArgs& a, const float4* pts, uint8_t* inl, int nv, const double* Tl, bool ok) {
    double T[9];
#pragma unroll
    for (int i = 0; i < 9; i++) T[i] = Tl[i];
    for (int i = threadIdx.x; i < nv; i += FT_BLOCK) inl[i] = ok && ft_inlier(T, pts[i], a.thr2) ? 1 : 0;
    __syncthreads();
}

// least squares of `model` on the marked points -> T (wave 0's area); the same answer in every thread
__device__ bool ft_block_fit(const RcFitArgs& a, int model, const float4* pts, const uint8_t* inl, int nv, double* wv, double* red) {
    double* M = wv; double* z = wv + 72; double* E = wv + 80; double* T = wv + 89; double* flag = wv + 98;
    const int tid = threadIdx.x;
    bool ok = false;
    if (model == RC_STAB_HOMOGRAPHY) {
        double acc[44], c = 0.;
#pragma unroll
        for (int i = 0; i < 44; i++) acc[i] = 0.;
        for (int i = tid; i < nv; i += FT_BLOCK) {
            const FtPt t = ft_norm(a, pts[i]);
            const bool in = inl[i] != 0;
            const double r1[9] = {t.Px, t.Py, 1., 0., 0., 0., -t.Qx * t.Px, -t.Qx * t.Py, t.Dx};
            const double r2[9] = {0., 0., 0., t.Px, t.Py, 1., -t.Qy * t.Px, -t.Qy * t.Py, t.Dy};
            c += in ? 1. : 0.;
            int e = 0;
#pragma unroll
            for (int r = 0; r < 8; r++)
#pragma unroll
                for (int k = r; k < 9; k++, e++) {
                    const double term = r1[r] * r1[k] + r2[r] * r2[k];
                    acc[e] += in ? term : 0.;
                }
        }
        const double n = ft_blk_sum(c, red);
        int e = 0;
#pragma unroll
        for (int r = 0; r < 8; r++)
#pragma unroll
            for (int k = r; k < 9; k++, e++) {
                const double s = ft_blk_sum(acc[e], red);
                if (tid == 0) { M[r * 9 + k] = s; if (k < 8) M[k * 9 + r] = s; }
            }
        if (tid == 0) {
            bool o = n >= 4. && ft_ge8(M, 1e-12, z);
            if (o) { ft_z_to_E(z, E); o = ft_to_pixels(a, E, T, true); }
            *flag = o ? 1. : 0.;
        }
    } else {
        double c = 0., spx = 0., spy = 0., sdx = 0., sdy = 0.;
        for (int i = tid; i < nv; i += FT_BLOCK) {
            const FtPt t = ft_norm(a, pts[i]);
            const bool in = inl[i] != 0;
            c += in ? 1. : 0.; spx += in ? t.Px : 0.; spy += in ? t.Py : 0.; sdx += in ? t.Dx : 0.; sdy += in ? t.Dy : 0.;
        }
        const double n = ft_blk_sum(c, red);
        spx = ft_blk_sum(spx, red); spy = ft_blk_sum(spy, red); sdx = ft_blk_sum(sdx, red); sdy = ft_blk_sum(sdy, red);
        const double nn = n > 0. ? n : 1.;
        const double mpx = spx / nn, mpy = spy / nn, mdx = sdx / nn, mdy = sdy / nn;
        double sxx = 0., sxy = 0., syy = 0., xdx = 0., ydx = 0., xdy = 0., ydy = 0.;
        if (model >= RC_STAB_SIMILARITY) {
            for (int i = tid; i < nv; i += FT_BLOCK) {
                const FtPt t = ft_norm(a, pts[i]);
                const bool in = inl[i] != 0;
                const double ux = t.Px - mpx, uy = t.Py - mpy, ex = t.Dx - mdx, ey = t.Dy - mdy;
                sxx += in ? ux * ux : 0.; sxy += in ? ux * uy : 0.; syy += in ? uy * uy : 0.;
                xdx += in ? ux * ex : 0.; ydx += in ? uy * ex : 0.; xdy += in ? ux * ey : 0.; ydy += in ? uy * ey : 0.;
            }
            sxx = ft_blk_sum(sxx, red); sxy = ft_blk_sum(sxy, red); syy = ft_blk_sum(syy, red);
            xdx = ft_blk_sum(xdx, red); ydx = ft_blk_sum(ydx, red); xdy = ft_blk_sum(xdy, red); ydy = ft_blk_sum(ydy, red);
        }
        if (tid == 0) {
            bool o = ft_finish_lin(model, n, mpx, mpy, mdx, mdy, sxx, sxy, syy, xdx, ydx, xdy, ydy, E);
            if (o) o = ft_to_pixels(a, E, T, false);
            *flag = o ? 1. : 0.;
        }
    }
    __syncthreads();
    ok = *flag != 0.;
    __syncthreads();
    return ok;
}

extern __shared__ __attribute__((aligned(16))) char ft_smem[];

__global__ __launch_bounds__(FT_BLOCK) void k_robust_fit(const RcFitArgs a) {
    float4* pts = (float4*)ft_smem;                                  // [ncap] (px, py, qx, qy) of the valid pairs
    unsigned short* vidx = (unsigned short*)(pts + a.ncap);          // [ncap] their input indices
    uint8_t* inl = (uint8_t*)(vidx + a.ncap);                        // [ncap]
    double* wvs = (double*)(ft_smem + (size_t)19 * a.ncap);          // [FT_WAVES][FT_WAVE_DOUBLES]
    double* red = wvs + FT_WAVES * FT_WAVE_DOUBLES;                  // [FT_WAVES]
    int* scan = (int*)(red + FT_WAVES);                              // [FT_BLOCK]
    unsigned long long* keys = (unsigned long long*)(scan + FT_BLOCK);   // [FT_WAVES]
    int* ib = (int*)(keys + FT_WAVES);                               // [4]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i0 = tid * a.chunk, i1 = min(a.n, i0 + a.chunk);

    // the gate's maximum over all n scores, then validity, the prefix sum and the compaction
    int smax = 0;
    if (a.scores) {
        for (int i = i0; i < i1; i++) smax = max(smax, a.scores[i]);
        smax = rc_wave_max_all(smax);
        if (lane == 0) scan[wave] = smax;
        __syncthreads();
        smax = max(max(scan[0], scan[1]), max(scan[2], scan[3]));
        __syncthreads();
    }
    const double gate = a.quality * (double)smax;
    unsigned valid = 0;                                              // chunk <= 16 entries
    int cnt = 0;
    for (int i = i0; i < i1; i++) {
        const float2 p = a.p[i], q = a.q[i];
        const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y;
        bool v = a.status[i] == 1 && dx * dx + dy * dy <= a.max_shift2;
        if (a.scores) { const int sc = a.scores[i]; v = v && sc > 0 && sc >= a.min_score && (double)sc >= gate; }
        if (v) { valid |= 1u << (i - i0); cnt++; }
    }
    scan[tid] = cnt;
    __syncthreads();
    int base = 0, nv = 0;
    for (int k = 0; k < FT_BLOCK; k++) { const int c = scan[k]; base += k < tid ? c : 0; nv += c; }
    for (int i = i0; i < i1; i++)
        if (valid >> (i - i0) & 1u) {
            const float2 p = a.p[i], q = a.q[i];
            pts[base] = make_float4(p.x, p.y, q.x, q.y);
            vidx[base] = (unsigned short)i;
            base++;
        }
    __syncthreads();

    // one hypothesis per wave
    const int j = blockIdx.x * FT_WAVES + wave;
    double* wv = wvs + wave * FT_WAVE_DOUBLES;
    if (lane == 0) {
        const bool ok = j < a.hyp && ft_hypothesis(a, pts, nv, j, wv);
        wv[98] = ok ? 1. : 0.;
        if (a.samples && j < a.hyp) {
            const int* smp = (const int*)(wv + 100);
#pragma unroll
            for (int i = 0; i < 4; i++) a.samples[4 * j + i] = ok && smp[i] >= 0 ? (int)vidx[smp[i]] : -1;
        }
    }
    __syncthreads();
    int count = 0;
    if (wv[98] != 0.) {
        double T[9];
#pragma unroll
        for (int i = 0; i < 9; i++) T[i] = wv[89 + i];
        for (int i = lane; i < nv; i += 64) count += ft_inlier(T, pts[i], a.thr2) ? 1 : 0;
        count = rc_wave_sum_all(count);
    }
    if (lane == 0) keys[wave] = j < a.hyp ? ((unsigned long long)(unsigned)count << 32) | (0xffffffffu - (unsigned)j) : 0ull;
    __syncthreads();
    if (tid == 0) {
        unsigned long long key = keys[0];
        for (int k = 1; k < FT_WAVES; k++) key = keys[k] > key ? keys[k] : key;
        (void)__hip_atomic_fetch_max(a.ws, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned* ticket = (unsigned*)(a.ws + 1);
        int last = 0;
        if (rc_ticket_release(ticket, gridDim.x)) {
            const unsigned long long best = rc_acc_load(a.ws);
            __hip_atomic_store(a.ws, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = 1;
            ib[1] = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
        }
        ib[0] = last;
    }
    __syncthreads();
    if (!ib[0]) return;

    // ------------------------------------------------------------------------ the last workgroup: refits and the ladder
    const int winner = ib[1];
    double* w0 = wvs;                                                // T at w0 + 89
    __syncthreads();
    if (tid == 0) w0[99] = ft_hypothesis(a, pts, nv, winner, w0) ? 1. : 0.;
    __syncthreads();
    ft_mark(a, pts, inl, nv, w0 + 89, w0[99] != 0.);
    int model = a.model;
    double ninl = 0.;
    for (;;) {
        if (model == 0) {
            if (tid == 0)
                for (int i = 0; i < 9; i++) w0[89 + i] = (i & 3) == 0 ? 1. : 0.;
            __syncthreads();
            ft_mark(a, pts, inl, nv, w0 + 89, true);
        } else {
            const int rounds = model == a.model ? 2 : 1;
            bool ok = true;
            for (int r = 0; r < rounds && ok; r++) {
                ok = ft_block_fit(a, model, pts, inl, nv, w0, red);
                if (ok) ft_mark(a, pts, inl, nv, w0 + 89, true);
            }
            if (!ok) { model--; continue; }
        }
        double c = 0.;
        for (int i = tid; i < nv; i += FT_BLOCK) c += inl[i] ? 1. : 0.;
        ninl = ft_blk_sum(c, red);
        if (model == 0 || ninl >= (double)ft_need(model)) break;
        model--;
    }
    for (int i = tid; i < a.n; i += FT_BLOCK) a.inlier[i] = 0;
    __syncthreads();
    for (int i = tid; i < nv; i += FT_BLOCK) a.inlier[vidx[i]] = inl[i];
    if (tid == 0) {
        const double* T = w0 + 89;
        for (int i = 0; i < 9; i++) a.out->T[i] = T[i];
        a.out->model_used = model; a.out->n_valid = nv; a.out->n_inliers = (int)ninl; a.out->winner = winner;
        const double X = (T[0] * a.fcx + T[1] * a.fcy) + T[2], Y = (T[3] * a.fcx + T[4] * a.fcy) + T[5], W = (T[6] * a.fcx + T[7] * a.fcy) + T[8];
        const double r0 = X / W - a.fcx, r1 = Y / W - a.fcy, r2 = nv ? ninl / (double)nv : 0.;
        if (a.res) { a.res[0] = r0; a.res[1] = r1; a.res[2] = r2; }
        if (a.res2) { a.res2[0] = r0; a.res2[1] = r1; a.res2[2] = r2; }
    }
}

// ============================================================================ host side
int rc_fit_check(const char* who, int n, int w, int h, const rc_fit_params* prm) {
    if (n < 0 || n > RC_FIT_MAX_POINTS || w <= 0 || h <= 0) { rc_set_error("%s: %d pairs (0..%d) or a bad frame size %d x %d", who, n, RC_FIT_MAX_POINTS, w, h); return RC_EINVAL; }
    if (!prm || prm->model < RC_STAB_TRANSLATION || prm->model > RC_STAB_HOMOGRAPHY || prm->hypotheses < 0 || prm->hypotheses > RC_FIT_MAX_HYPOTHESES ||
        prm->min_score < 0 || !(prm->quality >= 0. && prm->quality <= 1.) || !(prm->max_shift >= 0.) || !(prm->inlier_px >= 0.) ||
        !isfinite(prm->max_shift) || !isfinite(prm->inlier_px)) {
        rc_set_error("%s: unknown model, hypotheses outside 0..%d (0: %d), or a gate that is negative or not finite", who, RC_FIT_MAX_HYPOTHESES,
                     RC_FIT_DEFAULT_HYPOTHESES);
        return RC_EINVAL;
    }
    return RC_OK;
}

// "trackstab@4".  ws: two zeroed 64-bit words that stay with the caller's state.  max_shift 0: 0.1 max(w, h); inlier_px 0: 1
void rc_fit_launch(rc_ctx* ctx, hipStream_t cur, const float* d_p, const float* d_q, const uint8_t* d_status, const int* d_scores, int n, int w,
                   int h, const rc_fit_params& prm, rc_fit_result* d_result, uint8_t* d_inlier, int* d_samples, void* d_ws, double* d_res,
                   double* d_res2) {
    RcFitArgs a;
    memset(&a, 0, sizeof(a));
    a.p = (const float2*)d_p; a.q = (const float2*)d_q; a.status = d_status; a.scores = d_scores;
    a.n = n; a.ncap = ((n + FT_BLOCK - 1) / FT_BLOCK) * FT_BLOCK; a.chunk = a.ncap / FT_BLOCK;
    if (a.ncap == 0) a.ncap = FT_BLOCK;
    a.model = prm.model; a.hyp = prm.hypotheses ? prm.hypotheses : RC_FIT_DEFAULT_HYPOTHESES; a.min_score = prm.min_score; a.seed = prm.seed;
    a.quality = prm.quality;
    const double ms = prm.max_shift > 0. ? prm.max_shift : 0.1 * (double)(w > h ? w : h), thr = prm.inlier_px > 0. ? prm.inlier_px : 1.0;
    a.max_shift2 = ms * ms; a.thr2 = thr * thr;
    a.S = (double)(w > h ? w : h); a.cx = (double)w * 0.5; a.cy = (double)h * 0.5;
    a.fcx = ((double)w - 1.0) / 2.0; a.fcy = ((double)h - 1.0) / 2.0;
    a.out = d_result; a.inlier = d_inlier; a.samples = d_samples; a.ws = (unsigned long long*)d_ws; a.res = d_res; a.res2 = d_res2;
    const size_t lds = (size_t)19 * a.ncap + sizeof(double) * (FT_WAVES * FT_WAVE_DOUBLES + FT_WAVES) + sizeof(int) * FT_BLOCK +
                       sizeof(unsigned long long) * FT_WAVES + 4 * sizeof(int);
    RC_ALLOW_LDS((k_robust_fit), lds);
    RcProfScope ps(ctx, cur, RC_K_TRACKSTAB, 4, 21. * n + sizeof(rc_fit_result) + n);
    hipLaunchKernelGGL(k_robust_fit, dim3((a.hyp + FT_WAVES - 1) / FT_WAVES), dim3(FT_BLOCK), lds, cur, a);
}

extern "C" int rcflow_fit_motion_dev(rc_ctx* ctx, int stream, const float* d_p, const float* d_q, const uint8_t* d_status, const int* d_scores,
                                     int n, int w, int h, const rc_fit_params* prm, rc_fit_result* d_result, uint8_t* d_inlier, int* d_samples) {
    static const char* who = "rcflow_fit_motion_dev";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    int rc = rc_fit_check(who, n, w, h, prm);
    if (rc) return rc;
    if (!d_result || (n > 0 && (!d_p || !d_q || !d_status || !d_inlier))) {
        rc_set_error("%s: a null pointer among d_result and, for n > 0, d_p, d_q, d_status, d_inlier", who);
        return RC_EINVAL;
    }
    RC_HIP(hipSetDevice(ctx->device));
    if (!s->fit_ws.p) {
        if ((rc = rc_buf_ensure(s->fit_ws, 16))) return rc;
        RC_HIP(hipMemsetAsync(s->fit_ws.p, 0, 16, s->cur));
    }
    rc_fit_launch(ctx, s->cur, d_p, d_q, d_status, d_scores, n, w, h, *prm, d_result, d_inlier, d_samples, s->fit_ws.p, nullptr, nullptr);
    RC_HIP(hipGetLastError());
    return RC_OK;
}
