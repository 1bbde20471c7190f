// stab_kernels.hip -- frame stabilisation on the device: the reference's compute_phaseCorrelate (main.cpp:1684-1775),
// and the same estimator on several patches with a motion fitted to them (rcflow_framestab_open_multi; the correcting
// warp of that form is warp_kernels.hip's).
// Per frame: phaseCorrelate(prev_roi, curr_roi, hann) on a patch of beach that does not move, then
// warpAffine(curr, [1 0 -shift.x; 0 1 -shift.y]) and the corrected frame becomes `prev`.  phaseCorrelate,
// createHanningWindow, getOptimalDFTSize and warpAffine are OpenCV's (4.1.0 phasecorr.cpp, imgwarp.cpp), restated
// here from knowledge of upstream: parity-unpinned.
//
// Correlate.  Patches w x h, zero-padded to the optimal DFT sizes N x M (N/2 + 1 = Nh bins kept per row):
//   load      a, b = patch * window (float), zeros in the padding                       ab: 2 x [M][N] float
//   rows      A, B = row DFT of a, b, bins 0..Nh-1                                      AB: 2 x [M][Nh] float2
//   columns   FA, FB = column DFT of A, B; P = FA conj(FB); C = P m / (m m + eps)       C:  [M][Nh] float2 over ab
//   icolumns  D = inverse column DFT of C (no scale)                                    D:  [M][Nh] float2 over AB
//   irows     r = inverse row DFT of D through D(y, N - v) = conj D(y, v)               r:  [M][N] float over ab
//   peak      first maximum of fftShift(r) in row-major order, 5 x 5 centroid in fp64, three doubles out
// Every DFT is a direct sum against a twiddle table indexed by j k mod n (made on the host in double): no size
// restriction, no radix error growth, and at these sizes a launch is bound by the latency of the dependent passes, not
// by flops.  When ab + AB + tables fit the LDS (ST_LDS_MAX) the passes run in ONE workgroup with barriers between
// them; beyond that each pass is a launch of its own over the same device functions, ab and AB in a scratch buffer.
//
// Warp.  dst(x, y) = src(x + shift.x, y + shift.y) in warpAffine's 8-bit fixed point: 1/32 px fractions, weights of
// 2^15, taps outside the frame count 0.  A thread owns 4 consecutive pixels of a row, stored as one dwordx3; a wave
// owns a row, so the row's Y0, fraction and weights are wave-uniform.  The shift is read from device memory (the
// correlate launch before it wrote it) or passed as an argument.  Lanes inside the ROI also write the gray float patch
// of the corrected frame: the `prev` of the next push.

#include <float.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "rc_host.h"
#include "rc_pix3.h"
#include "rc_reduce.h"

#define ST_BLOCK 1024                    // the correlate workgroup: 16 waves
#define ST_RED_BYTES 256                 // per-wave (value, index) of the arg-max
#define ST_LDS_MAX (160 * 1024)
#define FT_TRK_BYTES 34                  // per cell of RcFrameStab::trk (the tracking form)

struct StArgs {
    const float* a; size_t a_step;       // prev patch, byte step
    const float* b; size_t b_step;       // curr patch; or, when bgr is set, the ROI of an 8UC3 frame (gray on the fly)
    const uint8_t* bgr; size_t bgr_step;
    const float* win;                    // [h][w] Hann window of the unpadded size, or null
    const float2* twN; const float2* twM;   // (cos, sin)(2 pi j / n), j < n
    float* ab; float2* AB;               // scratch of the launch-per-pass form (the LDS form carves its own)
    double* res; double* res2;           // shift_x, shift_y, response (res2: the caller's copy, may be null)
    int w, h, N, M, Nh;
};

// ---------------------------------------------------------------------------- pass bodies
// (t0, nt): this thread's index and the number of threads sharing the pass
__device__ __forceinline__ float st_gray(const uint8_t* p) {
    return (float)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14);
}

__device__ __forceinline__ void st_load(const StArgs& p, float* a, float* b, int t0, int nt) {
    for (int i = t0; i < p.M * p.N; i += nt) {
        const int y = i / p.N, x = i - y * p.N;
        float va = 0.f, vb = 0.f;
        if (x < p.w && y < p.h) {
            va = ((const float*)((const char*)p.a + (size_t)y * p.a_step))[x];
            vb = p.bgr ? st_gray(p.bgr + (size_t)y * p.bgr_step + 3 * x)
                       : ((const float*)((const char*)p.b + (size_t)y * p.b_step))[x];
            if (p.win) { const float wv = p.win[y * p.w + x]; va *= wv; vb *= wv; }
        }
        a[i] = va; b[i] = vb;
    }
}

// A[y][k] = sum_x a[y][x] e^(-2 pi i x k / N), both patches against the same twiddles
__device__ __forceinline__ void st_rows(const StArgs& p, const float* a, const float* b, const float2* tw, float2* A, float2* B,
                                        int t0, int nt) {
    for (int i = t0; i < p.M * p.Nh; i += nt) {
        const int y = i / p.Nh, k = i - y * p.Nh;
        float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
        if (y < p.h) {
            const float* ra = a + y * p.N;
            const float* rb = b + y * p.N;
            int j = 0;
            for (int x = 0; x < p.w; x++) {
                const float2 t = tw[j];
                ar += ra[x] * t.x; ai -= ra[x] * t.y;
                br += rb[x] * t.x; bi -= rb[x] * t.y;
                j += k; if (j >= p.N) j -= p.N;
            }
        }
        A[i] = make_float2(ar, ai); B[i] = make_float2(br, bi);
    }
}

// FA, FB = column DFTs; cross power spectrum, normalised as magSpectrums + divSpectrums do
__device__ __forceinline__ void st_cols(const StArgs& p, const float2* A, const float2* B, const float2* tw, float2* C, int t0, int nt) {
    for (int i = t0; i < p.M * p.Nh; i += nt) {
        const int u = i / p.Nh, v = i - u * p.Nh;
        float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
        int j = 0;
        for (int y = 0; y < p.h; y++) {
            const float2 t = tw[j], za = A[y * p.Nh + v], zb = B[y * p.Nh + v];
            ar += za.x * t.x + za.y * t.y; ai += za.y * t.x - za.x * t.y;
            br += zb.x * t.x + zb.y * t.y; bi += zb.y * t.x - zb.x * t.y;
            j += u; if (j >= p.M) j -= p.M;
        }
        const float pr = ar * br + ai * bi, pi = ai * br - ar * bi;
        const float m = (float)sqrt((double)pr * pr + (double)pi * pi);
        const double den = (double)(m * m + FLT_EPSILON);
        C[i] = make_float2((float)((double)(pr * m) / den), (float)((double)(pi * m) / den));
    }
}

// D[y][v] = sum_u C[u][v] e^(+2 pi i u y / M)
__device__ __forceinline__ void st_icols(const StArgs& p, const float2* C, const float2* tw, float2* D, int t0, int nt) {
    for (int i = t0; i < p.M * p.Nh; i += nt) {
        const int y = i / p.Nh, v = i - y * p.Nh;
        float dr = 0.f, di = 0.f;
        int j = 0;
        for (int u = 0; u < p.M; u++) {
            const float2 t = tw[j], z = C[u * p.Nh + v];
            dr += z.x * t.x - z.y * t.y; di += z.x * t.y + z.y * t.x;
            j += y; if (j >= p.M) j -= p.M;
        }
        D[i] = make_float2(dr, di);
    }
}

// r[y][x] = Re sum_{v < N} D[y][v] e^(+2 pi i v x / N) with D[y][N - v] = conj D[y][v]
__device__ __forceinline__ void st_irows(const StArgs& p, const float2* D, const float2* tw, float* r, int t0, int nt) {
    const int vmax = (p.N - 1) / 2;
    for (int i = t0; i < p.M * p.N; i += nt) {
        const int y = i / p.N, x = i - y * p.N;
        const float2* d = D + y * p.Nh;
        float s = 0.f;
        int j = x;
        for (int v = 1; v <= vmax; v++) {
            const float2 t = tw[j];
            s += d[v].x * t.x - d[v].y * t.y;
            j += x; if (j >= p.N) j -= p.N;
        }
        float e = d[0].x;
        if (!(p.N & 1)) e += (x & 1) ? -d[p.N / 2].x : d[p.N / 2].x;
        r[i] = e + 2.f * s;
    }
}

// fftShift (phasecorr.cpp): index i goes to (i + floor(n / 2)) mod n, for odd n too
__device__ __forceinline__ float st_shifted(const StArgs& p, const float* r, int Y, int X) {
    int y = Y - p.M / 2, x = X - p.N / 2;
    if (y < 0) y += p.M;
    if (x < 0) x += p.N;
    return r[y * p.N + x];
}

// minMaxLoc over the shifted surface (lowest row-major index on ties), weightedCentroid in a 5 x 5 box clipped to the
// surface (fp64, values as they are), response = sum / (M N), shift = (N / 2.0, M / 2.0) - centroid.  One workgroup.
__device__ __forceinline__ void st_peak(const StArgs& p, const float* r, char* red) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < p.M * p.N; i += blockDim.x) {
        const int Y = i / p.N, X = i - Y * p.N;
        const float v = st_shifted(p, r, Y, X);
        if (v > bv || bi == 0x7fffffff) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    float* rv = (float*)red;
    int* ri = (int*)(red + ST_RED_BYTES / 2);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < nw; k++)
            if (ri[k] != 0x7fffffff && (bi == 0x7fffffff || rv[k] > bv || (rv[k] == bv && ri[k] < bi))) { bv = rv[k]; bi = ri[k]; }
        const int PY = bi / p.N, PX = bi - PY * p.N;
        const int minr = max(PY - 2, 0), maxr = min(PY + 2, p.M - 1), minc = max(PX - 2, 0), maxc = min(PX + 2, p.N - 1);
        double cx = 0., cy = 0., sum = 0.;
        for (int Y = minr; Y <= maxr; Y++)
            for (int X = minc; X <= maxc; X++) {
                const double v = (double)st_shifted(p, r, Y, X);
                cx += (double)X * v; cy += (double)Y * v; sum += v;
            }
        const double response = sum / (double)(p.M * p.N);
        sum += DBL_EPSILON;
        const double sx = (double)p.N / 2.0 - cx / sum, sy = (double)p.M / 2.0 - cy / sum;
        p.res[0] = sx; p.res[1] = sy; p.res[2] = response;
        if (p.res2) { p.res2[0] = sx; p.res2[1] = sy; p.res2[2] = response; }
    }
}

// ---------------------------------------------------------------------------- correlate kernels
// One workgroup, everything in LDS: 8 M N (ab) + 16 M Nh (AB) + 8 (N + M) (twiddles) + ST_RED_BYTES bytes
extern __shared__ __attribute__((aligned(16))) char st_smem[];
__device__ __forceinline__ void st_correlate_wg(const StArgs& p) {
    float* a = (float*)st_smem;
    float* b = a + p.M * p.N;
    float2* A = (float2*)(b + p.M * p.N);
    float2* B = A + p.M * p.Nh;
    float2* twN = B + p.M * p.Nh;
    float2* twM = twN + p.N;
    char* red = (char*)(twM + p.M);
    const int t0 = threadIdx.x, nt = ST_BLOCK;
    for (int i = t0; i < p.N; i += nt) twN[i] = p.twN[i];
    for (int i = t0; i < p.M; i += nt) twM[i] = p.twM[i];
    st_load(p, a, b, t0, nt);
    __syncthreads();
    st_rows(p, a, b, twN, A, B, t0, nt);
    __syncthreads();
    st_cols(p, A, B, twM, (float2*)a, t0, nt);
    __syncthreads();
    st_icols(p, (const float2*)a, twM, A, t0, nt);
    __syncthreads();
    st_irows(p, A, twN, a, t0, nt);
    __syncthreads();
    st_peak(p, a, red);
}
__global__ __launch_bounds__(ST_BLOCK) void k_stab_correlate(const StArgs p) { st_correlate_wg(p); }

// ---------------------------------------------------------------------------- several patches, a fitted motion
// Workgroup k correlates patch k (the body above, unchanged) and thread 0 of the workgroup that finishes LAST fits the
// motion to the gated shifts, so a push stays at two launches.  Hand-off between workgroups (they run on different CUs
// and XCDs, whose L1 / L2 do not see each other's plain stores): thread 0 stores its three doubles again with
// agent-scope atomic stores, then rc_ticket_release (rc_reduce.h): drain, ONE agent-scope release fence, drain, the
// ticket; the thread that draws n - 1 does ONE agent-scope acquire fence, and reads all the shifts with
// agent-scope atomic loads.  Nothing waits for anything: no spinning, any dispatch order works.  The last arriver zeroes
// the ticket for the next push (stream order), and open / reset zero it with the rest of the state.
struct StMultiArgs {
    StArgs p;                            // sizes and tables; a = the prev patch 0; b, bgr, res are set per workgroup
    const uint8_t* frame; size_t step;   // the incoming frame
    double* state;                       // RcFrameStab::res (RC_FS_*)
    double* res2;                        // the caller's copy of the result, or null
    double min_response;
    int n, model, fw, fh;
    int rx[RC_STAB_MAX_PATCHES], ry[RC_STAB_MAX_PATCHES];
};


// One lane, fp64; products and sums round one by one (-ffp-contract=off), in the order of tests/_framewarp_ref.py
__device__ void st_fit(const StMultiArgs& m) {
    const double* sh = m.state + RC_FS_SHIFTS;
    const double hx = ((double)m.p.w - 1.0) / 2.0, hy = ((double)m.p.h - 1.0) / 2.0;
    double px = 0., py = 0., tx = 0., ty = 0., rmin = INFINITY;
    unsigned mask = 0;
    int cnt = 0;
    for (int k = 0; k < m.n; k++) {
        const double r = rc_acc_load(sh + 3 * k + 2);
        if (!(r >= m.min_response)) continue;
        mask |= 1u << k; cnt++;
        px += (double)m.rx[k] + hx; py += (double)m.ry[k] + hy;
        tx += rc_acc_load(sh + 3 * k); ty += rc_acc_load(sh + 3 * k + 1);
        rmin = r < rmin ? r : rmin;
    }
    double b00 = 0., b01 = 0., b10 = 0., b11 = 0.;
    int used = 0;
    if (cnt) {
        const double dn = (double)cnt;
        px /= dn; py /= dn; tx /= dn; ty /= dn;
        double sxx = 0., sxy = 0., syy = 0., xdx = 0., ydx = 0., xdy = 0., ydy = 0.;
        for (int k = 0; k < m.n; k++) {
            if (!(mask >> k & 1u)) continue;
            const double ux = ((double)m.rx[k] + hx) - px, uy = ((double)m.ry[k] + hy) - py;
            const double ex = rc_acc_load(sh + 3 * k) - tx, ey = rc_acc_load(sh + 3 * k + 1) - ty;
            sxx += ux * ux; sxy += ux * uy; syy += uy * uy;
            xdx += ux * ex; ydx += uy * ex; xdy += ux * ey; ydy += uy * ey;
        }
        used = RC_STAB_TRANSLATION;
        const double det = sxx * syy - sxy * sxy;
        if (m.model >= RC_STAB_AFFINE && cnt >= 3 && det > 1e-12 * (sxx * syy)) {
            used = RC_STAB_AFFINE;
            b00 = (xdx * syy - ydx * sxy) / det; b01 = (ydx * sxx - xdx * sxy) / det;
            b10 = (xdy * syy - ydy * sxy) / det; b11 = (ydy * sxx - xdy * sxy) / det;
        } else if (m.model >= RC_STAB_SIMILARITY && cnt >= 2 && sxx + syy > 0.) {
            used = RC_STAB_SIMILARITY;
            const double a = (xdx + ydy) / (sxx + syy), b = (xdy - ydx) / (sxx + syy);
            b00 = a; b01 = -b; b10 = b; b11 = a;
        }
    } else {
        rmin = 0.;
    }
    double* mo = m.state + RC_FS_MOTION;
    mo[0] = 1.0 + b00; mo[1] = b01; mo[2] = tx - (b00 * px + b01 * py);
    mo[3] = b10; mo[4] = 1.0 + b11; mo[5] = ty - (b10 * px + b11 * py);
    const double cx = ((double)m.fw - 1.0) / 2.0 - px, cy = ((double)m.fh - 1.0) / 2.0 - py;
    const double r0 = cnt ? (b00 * cx + b01 * cy) + tx : 0., r1 = cnt ? (b10 * cx + b11 * cy) + ty : 0.;
    double* res = m.state + RC_FS_RESULT;
    res[0] = r0; res[1] = r1; res[2] = rmin;
    if (m.res2) { m.res2[0] = r0; m.res2[1] = r1; m.res2[2] = rmin; }
    int* u = (int*)(m.state + RC_FS_USED);
    u[0] = used; u[1] = cnt;
}

__global__ __launch_bounds__(ST_BLOCK) void k_stab_correlate_multi(const StMultiArgs m) {
    const int k = blockIdx.x;
    StArgs p = m.p;
    p.a = m.p.a + (size_t)k * p.w * p.h;
    p.bgr = m.frame + (size_t)m.ry[k] * m.step + 3 * (size_t)m.rx[k];
    p.res = m.state + RC_FS_SHIFTS + 3 * k;
    p.res2 = nullptr;
    st_correlate_wg(p);
    if (threadIdx.x != 0) return;
    // this thread wrote p.res (st_peak); again as write-through stores, then release, then the ticket
#pragma unroll
    for (int i = 0; i < 3; i++) __hip_atomic_store(p.res + i, p.res[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned* ticket = (unsigned*)(m.state + RC_FS_TICKET);
    if (!rc_ticket_release(ticket, (unsigned)m.n)) return;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    st_fit(m);
}

// The same passes as launches of their own, ab and AB in device memory (p.ab, p.AB)
#define ST_GRID_T0 (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x)
__global__ __launch_bounds__(RC_BLOCK) void k_stab_rows(const StArgs p) {
    // load and row pass in one launch: a thread's row-pass sums read whole rows, which other threads would have to
    // have loaded; so every output reads its row straight from the patches instead (the load pass folded in)
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    for (int i = t0; i < p.M * p.Nh; i += nt) {
        const int y = i / p.Nh, k = i - y * p.Nh;
        float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
        if (y < p.h) {
            const float* ra = (const float*)((const char*)p.a + (size_t)y * p.a_step);
            const float* rb = (const float*)((const char*)p.b + (size_t)y * p.b_step);
            const uint8_t* rg = p.bgr ? p.bgr + (size_t)y * p.bgr_step : nullptr;
            int j = 0;
            for (int x = 0; x < p.w; x++) {
                const float2 t = p.twN[j];
                float va = ra[x], vb = rg ? st_gray(rg + 3 * x) : rb[x];
                if (p.win) { const float wv = p.win[y * p.w + x]; va *= wv; vb *= wv; }
                ar += va * t.x; ai -= va * t.y;
                br += vb * t.x; bi -= vb * t.y;
                j += k; if (j >= p.N) j -= p.N;
            }
        }
        p.AB[i] = make_float2(ar, ai); p.AB[p.M * p.Nh + i] = make_float2(br, bi);
    }
}
__global__ __launch_bounds__(RC_BLOCK) void k_stab_cols(const StArgs p) {
    st_cols(p, p.AB, p.AB + p.M * p.Nh, p.twM, (float2*)p.ab, ST_GRID_T0);
}
__global__ __launch_bounds__(RC_BLOCK) void k_stab_icols(const StArgs p) {
    st_icols(p, (const float2*)p.ab, p.twM, p.AB, ST_GRID_T0);
}
__global__ __launch_bounds__(RC_BLOCK) void k_stab_irows(const StArgs p) {
    st_irows(p, p.AB, p.twN, p.ab, ST_GRID_T0);
}
__global__ __launch_bounds__(ST_BLOCK) void k_stab_peak(const StArgs p) {
    __shared__ __attribute__((aligned(16))) char red[ST_RED_BYTES];
    st_peak(p, p.ab, red);
}

// ---------------------------------------------------------------------------- warp
struct StWarpArgs {
    const uint8_t* src; size_t step;
    uint8_t* dst; size_t dst_step;
    const double* d_shift;               // shift_x, shift_y on the device; null: sx, sy below
    double sx, sy;
    float* patch;                        // [rh][rw] gray float of the corrected frame's ROI, or null
    int w, h, rows, rx, ry, rw, rh;
};

__global__ __launch_bounds__(RC_BLOCK) void k_stab_warp(const StWarpArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int x0 = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), n = min(4, a.w - x0);
    double sx = a.sx, sy = a.sy;
    if (a.d_shift) { sx = a.d_shift[0]; sy = a.d_shift[1]; }
    // X0 = cvRound(shift.x * 1024) + 16; X = (X0 + 1024 x) >> 5: the same fraction for every pixel
    const int X0 = __double2int_rn(sx * 1024.0) + 16;
    const int fx = (X0 >> 5) & 31, xs = x0 + (X0 >> 10);
    if (n <= 0) return;
    const int yb = (blockIdx.y * RC_PIX3_WAVES + wave) * a.rows;
    for (int y = yb; y < min(yb + a.rows, a.h); y++) {
        // y is inside the rounding: (1.0 * y + shift.y) * 1024 in double, per row
        const int Y0 = __double2int_rn(((double)y + sy) * 1024.0) + 16;
        const int fy = (Y0 >> 5) & 31, ys = Y0 >> 10;
        uint32_t p0[5], p1[5];
        if (n == 4 && xs >= 0 && xs + 5 < a.w && ys >= 0 && ys + 1 < a.h) {
            const uint8_t* s0 = a.src + (size_t)ys * a.step + 3 * (size_t)xs;
            rc_pix3_unpack5(s0, p0);
            rc_pix3_unpack5(s0 + a.step, p1);
        } else {
#pragma unroll
            for (int k = 0; k < 5; k++) {
                p0[k] = rc_pix3_tap(a.src, a.step, a.w, a.h, xs + k, ys);
                p1[k] = rc_pix3_tap(a.src, a.step, a.w, a.h, xs + k, ys + 1);
            }
        }
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = rc_pix3_bilinear(p0[k], p0[k + 1], p1[k], p1[k + 1], fx, fy);
        rc_pix3_store4(a.dst + (size_t)y * a.dst_step, x0, n, o);
        if (a.patch && (unsigned)(y - a.ry) < (unsigned)a.rh) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int px = x0 + k - a.rx;
                if (k < n && (unsigned)px < (unsigned)a.rw) a.patch[(y - a.ry) * a.rw + px] = rc_pix3_gray(o[k]);
            }
        }
    }
}

// ============================================================================ host side
// getOptimalDFTSize: the smallest 2^a 3^b 5^c >= n
static int st_optimal(int n) {
    for (int m = n;; m++) {
        int k = m;
        while (k % 2 == 0) k /= 2;
        while (k % 3 == 0) k /= 3;
        while (k % 5 == 0) k /= 5;
        if (k == 1) return m;
    }
}

struct StPlan {
    int w = 0, h = 0, N = 0, M = 0, Nh = 0;
    size_t lds = 0;                      // bytes of the one-workgroup form
    size_t scratch = 0;                  // bytes of ab + AB
    bool fits = false;
};
static StPlan st_plan(int w, int h) {
    StPlan q;
    q.w = w; q.h = h; q.N = st_optimal(w); q.M = st_optimal(h); q.Nh = q.N / 2 + 1;
    q.scratch = (size_t)8 * q.M * q.N + (size_t)16 * q.M * q.Nh;
    q.lds = q.scratch + (size_t)8 * (q.N + q.M) + ST_RED_BYTES;
    q.fits = q.lds <= ST_LDS_MAX;
    return q;
}

// tab: window [h][w] | twN [N] float2 | twM [M] float2, made in double.  createHanningWindow: the product of the two
// raised-cosine factors (double) rounded to float, then a float square root.
static int st_tables(RcBuf& tab, const StPlan& q, hipStream_t cur) {
    std::vector<float> t((size_t)q.w * q.h + 2 * (size_t)(q.N + q.M));
    const double c0 = 2.0 * M_PI / (double)(q.w - 1), c1 = 2.0 * M_PI / (double)(q.h - 1);
    for (int i = 0; i < q.h; i++) {
        const double wr = 0.5 * (1.0 - cos(c1 * i));
        for (int j = 0; j < q.w; j++) t[(size_t)i * q.w + j] = sqrtf((float)(wr * (0.5 * (1.0 - cos(c0 * j)))));
    }
    float* tw = t.data() + (size_t)q.w * q.h;
    for (int j = 0; j < q.N; j++) { tw[2 * j] = (float)cos(2.0 * M_PI * j / q.N); tw[2 * j + 1] = (float)sin(2.0 * M_PI * j / q.N); }
    tw += 2 * q.N;
    for (int j = 0; j < q.M; j++) { tw[2 * j] = (float)cos(2.0 * M_PI * j / q.M); tw[2 * j + 1] = (float)sin(2.0 * M_PI * j / q.M); }
    int rc = rc_buf_ensure(tab, t.size() * sizeof(float));
    if (rc) return rc;
    RC_HIP(hipStreamSynchronize(cur));          // a previous launch may still read the old tables
    RC_HIP(hipMemcpy(tab.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    return RC_OK;
}

static void st_fill(StArgs& p, const StPlan& q, const RcBuf& tab, const RcBuf& scratch, bool hann) {
    p.w = q.w; p.h = q.h; p.N = q.N; p.M = q.M; p.Nh = q.Nh;
    const float* t = (const float*)tab.p;
    p.win = hann ? t : nullptr;
    p.twN = (const float2*)(t + (size_t)q.w * q.h);
    p.twM = p.twN + q.N;
    p.ab = (float*)scratch.p;
    p.AB = scratch.p ? (float2*)((char*)scratch.p + (size_t)8 * q.M * q.N) : nullptr;
}

// launches: "framestab@0" the one-workgroup form; "framestab@2..6" the passes of the large form
static int st_correlate(rc_ctx* ctx, hipStream_t cur, const StArgs& p, const StPlan& q) {
    const double in_bytes = (p.bgr ? 7. : 8.) * q.w * q.h + (p.win ? 4. * q.w * q.h : 0.) + 8. * (q.N + q.M);
    if (q.fits) {
        if (q.lds > 64 * 1024) {
            (void)hipFuncSetAttribute((const void*)k_stab_correlate, hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_MAX);
            (void)hipGetLastError();
        }
        RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 0, in_bytes + 24. + (p.res2 ? 24. : 0.));
        hipLaunchKernelGGL(k_stab_correlate, dim3(1), dim3(ST_BLOCK), q.lds, cur, p);
    } else {
        const double half = 8. * q.M * q.Nh, full = 4. * q.M * q.N;
        const dim3 gh((q.M * q.Nh + RC_BLOCK - 1) / RC_BLOCK), gf((q.M * q.N + RC_BLOCK - 1) / RC_BLOCK);
        { RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 2, in_bytes + 2. * half); hipLaunchKernelGGL(k_stab_rows, gh, dim3(RC_BLOCK), 0, cur, p); }
        { RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 3, 3. * half); hipLaunchKernelGGL(k_stab_cols, gh, dim3(RC_BLOCK), 0, cur, p); }
        { RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 4, 2. * half); hipLaunchKernelGGL(k_stab_icols, gh, dim3(RC_BLOCK), 0, cur, p); }
        { RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 5, half + full); hipLaunchKernelGGL(k_stab_irows, gf, dim3(RC_BLOCK), 0, cur, p); }
        { RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 6, full + 24. + (p.res2 ? 24. : 0.)); hipLaunchKernelGGL(k_stab_peak, dim3(1), dim3(ST_BLOCK), 0, cur, p); }
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

static int st_check_patch(const char* who, int w, int h, StPlan& q) {
    if (w < 8 || h < 8) { rc_set_error("%s: patch %d x %d is below 8 x 8", who, w, h); return RC_EINVAL; }
    if (w > 256 || h > 256) { rc_set_error("%s: patch %d x %d: the optimal DFT size exceeds 256 x 256", who, w, h); return RC_ESIZE; }
    q = st_plan(w, h);
    if (q.N > 256 || q.M > 256) {
        rc_set_error("%s: patch %d x %d has the optimal DFT size %d x %d, above 256 x 256", who, w, h, q.N, q.M);
        return RC_ESIZE;
    }
    return RC_OK;
}

extern "C" int rcflow_phase_correlate_dev(rc_ctx* ctx, int stream, const float* d_a, size_t a_step, const float* d_b, size_t b_step,
                                          int w, int h, int use_hann, double* d_result) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (!d_a || !d_b || !d_result || w <= 0 || h <= 0 || a_step < (size_t)w * 4 || b_step < (size_t)w * 4 || (a_step & 3) || (b_step & 3)) {
        rc_set_error("rcflow_phase_correlate_dev: bad patch arguments");
        return RC_EINVAL;
    }
    StPlan q;
    int rc = st_check_patch("rcflow_phase_correlate_dev", w, h, q);
    if (rc) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcPhaseCorr& pc = s->pc;
    if (pc.w != w || pc.h != h) {
        pc.w = pc.h = 0;
        if ((rc = st_tables(pc.tab, q, s->cur))) return rc;
        if (!q.fits && (rc = rc_buf_ensure(pc.scratch, q.scratch))) return rc;
        pc.w = w; pc.h = h;
    }
    StArgs p;
    memset(&p, 0, sizeof(p));
    st_fill(p, q, pc.tab, pc.scratch, use_hann != 0);
    p.a = d_a; p.a_step = a_step; p.b = d_b; p.b_step = b_step;
    p.res = d_result;
    return st_correlate(ctx, s->cur, p, q);
}

static void st_warp_launch(rc_ctx* ctx, hipStream_t cur, StWarpArgs& a) {
    a.rows = rc_rows_per_wave(a.w, a.h, 2);
    RcProfScope ps(ctx, cur, RC_K_FRAMESTAB, 1, 6. * a.w * a.h + (a.patch ? 4. * a.rw * a.rh : 0.) + (a.d_shift ? 16. : 0.));
    hipLaunchKernelGGL(k_stab_warp, rc_pix3_grid(a.w, a.h, a.rows), dim3(RC_BLOCK), 0, cur, a);
}

extern "C" int rcflow_warp_translate_bgr_dev(rc_ctx* ctx, int stream, const uint8_t* d_bgr, size_t step, int w, int h, uint8_t* d_out,
                                             size_t out_step, double shift_x, double shift_y) {
    static const char* who = "rcflow_warp_translate_bgr_dev";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (rc_img3_check(who, "d_bgr", d_bgr, step, w, h) || rc_img3_check(who, "d_out", d_out, out_step, w, h)) return RC_EINVAL;
    // the fixed-point coordinates are 32-bit with 10 fraction bits
    if (!(fabs(shift_x) <= 1048576.) || !(fabs(shift_y) <= 1048576.)) {
        rc_set_error("%s: shift (%g, %g) is not finite or beyond 2^20 px", who, shift_x, shift_y);
        return RC_EINVAL;
    }
    if (rc_fits_context(who, ctx, w, h)) return RC_ESIZE;
    if (rc_img3_pair(who, "d_bgr", d_bgr, step, w, h, "d_out", d_out, out_step, w, h)) return RC_EINVAL;   // the warp is not in place
    RC_HIP(hipSetDevice(ctx->device));
    StWarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_bgr; a.step = step; a.dst = d_out; a.dst_step = out_step; a.w = w; a.h = h;
    a.sx = shift_x; a.sy = shift_y;
    st_warp_launch(ctx, s->cur, a);
    RC_HIP(hipGetLastError());
    return RC_OK;
}

// ---------------------------------------------------------------------------- the pipeline (main.cpp:1707-1759)
void rc_state_free(RcFrameStab& f) {
    rc_buf_free(f.tab); rc_buf_free(f.prev); rc_buf_free(f.res); rc_buf_free(f.scratch);
    rc_buf_free(f.lkref); rc_buf_free(f.lkcur); rc_buf_free(f.trk);
    rc_fence_free(f.zf);
    f = RcFrameStab();
}

// nothing to register against yet: frame count, result and prev patch to zero
int rc_state_zero(RcSlot& s, RcFrameStab& f) {
    const int rc = rc_fence_zero(f.zf, s.cur, {&f.prev, &f.res, &f.trk});
    if (!rc) { f.frames = 0; f.pcur = 0; f.pflip = false; }
    return rc;
}

// Both opens behind their own argument checks: n patches of one size at rois (n = 0: the single-patch slot, one ROI)
static int fs_open(const char* who, rc_ctx* ctx, RcSlot& s, int w, int h, const int* rois, int n, int model, double min_response, int flags) {
    const int np = n ? n : 1, rw = rois[2], rh = rois[3];
    for (int k = 0; k < np; k++) {
        const int* r = rois + 4 * k;
        if (r[0] < 0 || r[1] < 0 || r[2] <= 0 || r[3] <= 0 || r[0] > w - r[2] || r[1] > h - r[3]) {
            rc_set_error("%s: patch %d (%d, %d, %d x %d) is not inside the %d x %d frame", who, k, r[0], r[1], r[2], r[3], w, h);
            return RC_EINVAL;
        }
        if (r[2] != rw || r[3] != rh) { rc_set_error("%s: patch %d is %d x %d, patch 0 is %d x %d (one size for all)", who, k, r[2], r[3], rw, rh); return RC_EINVAL; }
    }
    StPlan q;
    int rc = st_check_patch(who, rw, rh, q);
    if (rc) return rc;
    if (n && !q.fits) {
        rc_set_error("%s: patch %d x %d (DFT %d x %d) is beyond the one-workgroup correlation; larger patches are single-patch (rcflow_framestab_open)",
                     who, rw, rh, q.N, q.M);
        return RC_ESIZE;
    }
    if ((rc = rc_fits_context(who, ctx, w, h))) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcFrameStab f;
    f.w = w; f.h = h; f.rx = rois[0]; f.ry = rois[1]; f.rw = rw; f.rh = rh;
    f.N = q.N; f.M = q.M; f.lds = q.fits ? q.lds : 0;
    f.n = n; f.model = model; f.flags = flags; f.min_response = min_response;
    for (int k = 0; k < n; k++) { f.px[k] = rois[4 * k]; f.py[k] = rois[4 * k + 1]; }
    rc = st_tables(f.tab, q, s.cur);
    if (!rc) rc = rc_buf_ensure(f.prev, (size_t)np * rw * rh * sizeof(float));
    if (!rc) rc = rc_buf_ensure(f.res, (size_t)(n ? RC_FS_SHIFTS + 3 * RC_STAB_MAX_PATCHES : 3) * sizeof(double));
    if (!rc && !q.fits) rc = rc_buf_ensure(f.scratch, q.scratch);
    return rc_state_install(s, s.fs, f, rc);
}

extern "C" int rcflow_framestab_open(rc_ctx* ctx, int stream, int w, int h, int roi_x, int roi_y, int roi_w, int roi_h) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (w <= 0 || h <= 0) { rc_set_error("rcflow_framestab_open: bad frame size %d x %d", w, h); return RC_EINVAL; }
    const int roi[4] = {roi_x, roi_y, roi_w, roi_h};
    return fs_open("rcflow_framestab_open", ctx, *s, w, h, roi, 0, 0, 0., 0);
}

extern "C" int rcflow_framestab_open_multi(rc_ctx* ctx, int stream, int w, int h, const int* rois, int n, int model, double min_response,
                                           int flags) {
    static const char* who = "rcflow_framestab_open_multi";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (w <= 0 || h <= 0) { rc_set_error("%s: bad frame size %d x %d", who, w, h); return RC_EINVAL; }
    if (!rois || n < 1 || n > RC_STAB_MAX_PATCHES) { rc_set_error("%s: %d patches (1..%d)", who, n, RC_STAB_MAX_PATCHES); return RC_EINVAL; }
    if (model < RC_STAB_TRANSLATION || model > RC_STAB_AFFINE || (flags & ~RC_STAB_ANCHOR_FIRST) || min_response != min_response) {
        rc_set_error("%s: unknown model %d or flag bits 0x%x, or min_response is NaN", who, model, flags);
        return RC_EINVAL;
    }
    return fs_open(who, ctx, *s, w, h, rois, n, model, min_response, flags);
}


// ---------------------------------------------------------------------------- the tracking form
static int ft_cells_default(int w, int h, int& cx, int& cy) {
    int side = 40;
    for (;; side += 8) {
        cx = (w + side / 2) / side; cy = (h + side / 2) / side;
        cx = cx < 1 ? 1 : cx; cy = cy < 1 ? 1 : cy;
        if ((long long)cx * cy <= RC_CORNER_MAX_CELLS) return side;
    }
}

extern "C" int rcflow_framestab_open_tracks(rc_ctx* ctx, int stream, int w, int h, const rc_stab_tracks* prm) {
    static const char* who = "rcflow_framestab_open_tracks";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    if (w <= 0 || h <= 0) { rc_set_error("%s: bad frame size %d x %d", who, w, h); return RC_EINVAL; }
    if (!prm) { rc_set_error("%s: no parameters", who); return RC_EINVAL; }
    rc_stab_tracks t = *prm;
    if (t.win == 0) t.win = 21;
    if (t.max_level < 0) t.max_level = 3;
    if (t.max_count == 0) t.max_count = 30;
    if (t.epsilon == 0.) t.epsilon = 0.01;
    if (t.min_score == 0) t.min_score = 1;
    if (t.hypotheses == 0) t.hypotheses = RC_FIT_DEFAULT_HYPOTHESES;
    if (t.win < 3 || t.win > 63 || !(t.win & 1) || t.max_level > 7 || t.max_count < 1 || t.max_count > 100 || !(t.epsilon > 0. && t.epsilon <= 10.) ||
        (t.flags & ~RC_STAB_ANCHOR_FIRST)) {
        rc_set_error("%s: win %d (odd, 3..63), max_level %d (<= 7), max_count %d (1..100), epsilon %g (0..10] or flag bits 0x%x", who, t.win,
                     t.max_level, t.max_count, t.epsilon, t.flags);
        return RC_EINVAL;
    }
    const int margin = t.win / 2 + 2;
    if (t.cells_x == 0 && t.cells_y == 0) ft_cells_default(w, h, t.cells_x, t.cells_y);
    int rc = rc_corner_check(who, w, h, t.cells_x, t.cells_y, margin, t.min_score);
    if (rc) return rc;
    const int nc = t.cells_x * t.cells_y;
    const rc_fit_params fp = {t.model, t.hypotheses, t.seed, t.min_score, t.quality, t.max_shift, t.inlier_px};
    if ((rc = rc_fit_check(who, nc, w, h, &fp))) return rc;
    if ((rc = rc_fits_context(who, ctx, w, h))) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcFrameStab f;
    f.w = w; f.h = h; f.rx = margin; f.ry = margin; f.rw = w - 2 * margin; f.rh = h - 2 * margin;
    f.flags = t.flags; f.model = t.model;
    f.tracks = true; f.tp = t; f.ncells = nc; f.margin = margin;
    f.ref = rc_lk_plan(w, h, t.win, t.win, t.max_level, true);
    f.cur = rc_lk_plan(w, h, t.win, t.win, t.max_level, false);
    rc = rc_buf_ensure(f.lkref, f.ref.bytes);
    if (!rc) rc = rc_buf_ensure(f.lkcur, f.cur.bytes);
    if (!rc) rc = rc_buf_ensure(f.trk, (size_t)nc * FT_TRK_BYTES);
    if (!rc) rc = rc_buf_ensure(f.res, RC_FT_DOUBLES * sizeof(double));
    return rc_state_install(*s, s->fs, f, rc);
}

// trk: corners [2][ncells] float2 | tracks [ncells] float2 | scores [2][ncells] int | status [ncells] | inlier [ncells].  Slot
// pcur holds the corners the last push tracked; a chained push writes the corrected frame's corners into the other slot
// and the next push takes them over (a flip on the host), so that a read in between still pairs corner and track.
struct FtBufs { float* p; float* pn; float* q; int* scores; int* scores_n; uint8_t* status; uint8_t* inlier; };
static FtBufs ft_bufs(const RcFrameStab& f) {
    FtBufs b;
    float* base = (float*)f.trk.p;
    const int nc = f.ncells;
    b.p = base + 2 * nc * f.pcur; b.pn = base + 2 * nc * (1 - f.pcur); b.q = base + 4 * nc;
    int* sc = (int*)(base + 6 * nc);
    b.scores = sc + nc * f.pcur; b.scores_n = sc + nc * (1 - f.pcur);
    b.status = (uint8_t*)(sc + 2 * nc); b.inlier = b.status + nc;
    return b;
}

// One push of a tracks slot: gray, pyramid, track, fit (not on the first push); the warp reading T; then, chained or
// first, gray + pyramid + derivatives + corners of the corrected frame
static int fs_push_tracks(rc_ctx* ctx, RcSlot& s, const uint8_t* d_frame, size_t step, uint8_t* d_out, size_t out_step, double* d_result, bool first) {
    RcFrameStab& f = s.fs;
    const rc_stab_tracks& t = f.tp;
    if (f.pflip) { f.pcur = 1 - f.pcur; f.pflip = false; }
    const FtBufs b = ft_bufs(f);
    double* res = (double*)f.res.p;
    unsigned char* rb = (unsigned char*)f.lkref.p;
    if (!first) {
        unsigned char* cb = (unsigned char*)f.lkcur.p;
        rc_gray_launch(ctx, s.cur, d_frame, step, f.w, f.h, cb + f.cur.offI[0]);
        rc_lk_build(ctx, s.cur, f.cur, cb);
        rc_lk_track(ctx, s.cur, f.ref, rb, cb, f.cur, b.p, b.q, f.ncells, b.status, nullptr, t.win, t.win, t.max_count, t.epsilon, 0, 1e-4);
        const rc_fit_params fp = {t.model, t.hypotheses, t.seed, t.min_score, t.quality, t.max_shift, t.inlier_px};
        rc_fit_launch(ctx, s.cur, b.p, b.q, b.status, b.scores, f.ncells, f.w, f.h, fp, (rc_fit_result*)(res + RC_FT_FIT), b.inlier, nullptr,
                      res + RC_FT_WS, res + RC_FT_RESULT, d_result);
    }
    RcWarpArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_frame; a.step = step; a.sw = f.w; a.sh = f.h; a.dst = d_out; a.dst_step = out_step; a.dw = f.w; a.dh = f.h;
    a.M[0] = a.M[4] = a.M[8] = 1.;
    if (!first) a.d_M = res + RC_FT_FIT;
    rc_warp_launch(ctx, s.cur, a, t.model == RC_STAB_HOMOGRAPHY);
    if (first || !(t.flags & RC_STAB_ANCHOR_FIRST)) {
        rc_gray_launch(ctx, s.cur, d_out, out_step, f.w, f.h, rb + f.ref.offI[0]);
        rc_lk_build(ctx, s.cur, f.ref, rb);
        rc_corner_launch(ctx, s.cur, rb + f.ref.offI[0], (size_t)f.w, f.w, f.h, t.cells_x, t.cells_y, f.margin, t.min_score,
                         first ? b.p : b.pn, first ? b.scores : b.scores_n);
        f.pflip = !first;
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_framestab_read_tracks(rc_ctx* ctx, int stream, double T[9], int* model_used, int* n_valid, int* n_inliers, float* pts,
                                            uint8_t* inlier, int* scores, int cap, int* cells, long long* frames_pushed) {
    static const char* who = "rcflow_framestab_read_tracks";
    RcSlot* s; RcFrameStab* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fs, who, s, fp)) return rc;
    RcFrameStab& f = *fp;
    if (!f.tracks) { rc_set_error("%s: the slot's state was not opened by rcflow_framestab_open_tracks", who); return RC_ESTATE; }
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(f.zf, s->cur, false);
    if (rc) return rc;
    double st[RC_FT_DOUBLES] = {};
    std::vector<unsigned char> host((size_t)f.ncells * FT_TRK_BYTES);
    RC_HIP(hipMemcpyAsync(st, f.res.p, sizeof(st), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipMemcpyAsync(host.data(), f.trk.p, host.size(), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    const bool fitted = f.frames > 1;
    rc_fit_result r;
    memcpy(&r, st + RC_FT_FIT, sizeof(r));
    if (!fitted) {
        memset(&r, 0, sizeof(r));
        r.T[0] = r.T[4] = r.T[8] = 1.;
    }
    if (T) memcpy(T, r.T, sizeof(r.T));
    if (model_used) *model_used = r.model_used;
    if (n_valid) *n_valid = r.n_valid;
    if (n_inliers) *n_inliers = r.n_inliers;
    const int nc = f.ncells, m = cap < nc ? (cap < 0 ? 0 : cap) : nc;
    const float* hp = (const float*)host.data() + 2 * nc * f.pcur;
    const float* hq = (const float*)host.data() + 4 * nc;
    const int* hs = (const int*)((const float*)host.data() + 6 * nc) + nc * f.pcur;
    const unsigned char* hi = (const unsigned char*)((const float*)host.data() + 8 * nc) + nc;
    for (int k = 0; k < m; k++) {
        if (pts) { pts[4 * k] = hp[2 * k]; pts[4 * k + 1] = hp[2 * k + 1]; pts[4 * k + 2] = fitted ? hq[2 * k] : hp[2 * k]; pts[4 * k + 3] = fitted ? hq[2 * k + 1] : hp[2 * k + 1]; }
        if (inlier) inlier[k] = fitted ? hi[k] : 0;
        if (scores) scores[k] = hs[k];
    }
    if (cells) *cells = nc;
    if (frames_pushed) *frames_pushed = f.frames;
    return RC_OK;
}

extern "C" int rcflow_framestab_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::fs, "rcflow_framestab_reset"); }
extern "C" int rcflow_framestab_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::fs); }

extern "C" int rcflow_framestab_info(rc_ctx* ctx, int stream, int* w, int* h, int roi[4], int dft_size[2], int* launches_per_push,
                                     long long* frames_pushed, size_t* device_bytes) {
    RcSlot* s; RcFrameStab* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fs, "rcflow_framestab_info", s, fp)) return rc;
    const RcFrameStab& f = *fp;
    if (w) *w = f.w;
    if (h) *h = f.h;
    if (roi) { roi[0] = f.rx; roi[1] = f.ry; roi[2] = f.rw; roi[3] = f.rh; }
    if (dft_size) { dft_size[0] = f.N; dft_size[1] = f.M; }
    if (launches_per_push) {
        *launches_per_push = f.lds ? 2 : 6;
        // gray + pyramid + track + fit + warp, and chained: gray + pyramid + derivatives + corners
        if (f.tracks) *launches_per_push = 4 + f.cur.top + ((f.flags & RC_STAB_ANCHOR_FIRST) ? 0 : 3 + 2 * f.ref.top);
    }
    if (frames_pushed) *frames_pushed = f.frames;
    if (device_bytes) *device_bytes = f.tab.bytes + f.prev.bytes + f.res.bytes + f.scratch.bytes + f.lkref.bytes + f.lkcur.bytes + f.trk.bytes;
    return RC_OK;
}

extern "C" int rcflow_framestab_info_multi(rc_ctx* ctx, int stream, int* n, int* rois, int cap, int* model, double* min_response, int* flags) {
    RcSlot* s; RcFrameStab* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fs, "rcflow_framestab_info_multi", s, fp)) return rc;
    const RcFrameStab& f = *fp;
    const int np = f.tracks ? 0 : (f.n ? f.n : 1);
    if (n) *n = np;
    if (rois)
        for (int k = 0; k < np && k < cap; k++) {
            rois[4 * k] = f.n ? f.px[k] : f.rx; rois[4 * k + 1] = f.n ? f.py[k] : f.ry; rois[4 * k + 2] = f.rw; rois[4 * k + 3] = f.rh;
        }
    if (model) *model = f.n || f.tracks ? f.model : RC_STAB_TRANSLATION;
    if (min_response) *min_response = f.n ? f.min_response : -INFINITY;
    if (flags) *flags = f.flags;
    return RC_OK;
}

// Registers the frame against prev.  The single-patch slot: "framestab@0" (or "@2..6"), the shift into res.  A slot of
// rcflow_framestab_open_multi: "framestab@7" (n workgroups + the fit), the motion into res + RC_FS_MOTION.
static int fs_correlate(rc_ctx* ctx, RcSlot& s, const uint8_t* d_frame, size_t step, double* d_result) {
    const RcFrameStab& f = s.fs;
    const StPlan q = st_plan(f.rw, f.rh);
    StMultiArgs m;
    memset(&m, 0, sizeof(m));
    StArgs& p = m.p;                                     // the single-patch launch takes this part alone
    st_fill(p, q, f.tab, f.scratch, true);
    p.a = (const float*)f.prev.p; p.a_step = (size_t)f.rw * sizeof(float); p.bgr_step = step;
    if (!f.n) {
        p.bgr = d_frame + (size_t)f.ry * step + (size_t)3 * f.rx;
        p.res = (double*)f.res.p; p.res2 = d_result;
        return st_correlate(ctx, s.cur, p, q);
    }
    m.frame = d_frame; m.step = step;
    m.state = (double*)f.res.p; m.res2 = d_result;
    m.min_response = f.min_response; m.n = f.n; m.model = f.model; m.fw = f.w; m.fh = f.h;
    memcpy(m.rx, f.px, sizeof(m.rx)); memcpy(m.ry, f.py, sizeof(m.ry));
    if (q.lds > 64 * 1024) {
        (void)hipFuncSetAttribute((const void*)k_stab_correlate_multi, hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_MAX);
        (void)hipGetLastError();
    }
    {
        const double in_bytes = 7. * q.w * q.h + 4. * q.w * q.h + 8. * (q.N + q.M);
        RcProfScope ps(ctx, s.cur, RC_K_FRAMESTAB, 7, f.n * (in_bytes + 24.) + 72. + (d_result ? 24. : 0.));
        hipLaunchKernelGGL(k_stab_correlate_multi, dim3(f.n), dim3(ST_BLOCK), q.lds, s.cur, m);
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_framestab_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_frame, size_t step, uint8_t* d_out, size_t out_step,
                                         double* d_result) {
    static const char* who = "rcflow_framestab_push_dev";
    RcSlot* s; RcFrameStab* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fs, who, s, fp)) return rc;
    RcFrameStab& f = *fp;
    if (rc_img3_pair(who, "d_frame", d_frame, step, f.w, f.h, "d_out", d_out, out_step, f.w, f.h)) return RC_EINVAL;   // the warp is not in place
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(f.zf, s->cur, true);
    if (rc) return rc;
    const bool first = f.frames == 0;
    if (first) {
        // the first frame is copied (shift 0, the identity: every pixel is its own source) and becomes prev; result (0, 0, 0)
        RC_HIP(hipMemsetAsync(f.res.p, 0, f.res.bytes, s->cur));
        if (d_result) RC_HIP(hipMemsetAsync(d_result, 0, 3 * sizeof(double), s->cur));
    } else if (!f.tracks && (rc = fs_correlate(ctx, *s, d_frame, step, d_result))) {
        return rc;
    }
    if (f.tracks) {
        if ((rc = fs_push_tracks(ctx, *s, d_frame, step, d_out, out_step, d_result, first))) return rc;
    } else if (f.n) {                                    // "framestab@8": the fitted motion, read from device memory
        RcWarpArgs a;
        memset(&a, 0, sizeof(a));
        a.src = d_frame; a.step = step; a.sw = f.w; a.sh = f.h; a.dst = d_out; a.dst_step = out_step; a.dw = f.w; a.dh = f.h;
        a.M[0] = a.M[4] = 1.;
        if (first || !(f.flags & RC_STAB_ANCHOR_FIRST)) {
            a.patch = (float*)f.prev.p; a.npatch = f.n; a.rw = f.rw; a.rh = f.rh;
            memcpy(a.rx, f.px, sizeof(a.rx)); memcpy(a.ry, f.py, sizeof(a.ry));
        }
        if (!first) a.d_M = (const double*)f.res.p + RC_FS_MOTION;
        rc_warp_launch(ctx, s->cur, a, false);
    } else {                                             // "framestab@1": the shift, read from device memory
        StWarpArgs a;
        memset(&a, 0, sizeof(a));
        a.src = d_frame; a.step = step; a.dst = d_out; a.dst_step = out_step; a.w = f.w; a.h = f.h;
        a.patch = (float*)f.prev.p; a.rx = f.rx; a.ry = f.ry; a.rw = f.rw; a.rh = f.rh;
        if (!first) a.d_shift = (const double*)f.res.p;
        st_warp_launch(ctx, s->cur, a);
    }
    RC_HIP(hipGetLastError());
    f.frames++;
    return RC_OK;
}

extern "C" int rcflow_framestab_read_motion(rc_ctx* ctx, int stream, double motion[6], int* model_used, int* patches_used, double* shifts,
                                            long long* frames_pushed) {
    RcSlot* s; RcFrameStab* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fs, "rcflow_framestab_read_motion", s, fp)) return rc;
    RcFrameStab& f = *fp;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(f.zf, s->cur, false);
    if (rc) return rc;
    double st[RC_FS_SHIFTS + 3 * RC_STAB_MAX_PATCHES] = {};
    RC_HIP(hipMemcpyAsync(st, f.res.p, f.tracks ? RC_FT_DOUBLES * sizeof(double) : f.n ? sizeof(st) : 3 * sizeof(double), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    const bool fitted = f.frames > 1;                        // the first push registers against nothing
    double mo[6] = {1., 0., 0., 0., 1., 0.};
    int used[2] = {0, 0};
    const int np = f.tracks ? 0 : (f.n ? f.n : 1);
    if (fitted && f.tracks) {
        rc_fit_result r;
        memcpy(&r, st + RC_FT_FIT, sizeof(r));
        if (r.model_used == RC_STAB_HOMOGRAPHY) {
            rc_set_error("rcflow_framestab_read_motion: the motion of the last push is a homography (rcflow_framestab_read_tracks returns it)");
            return RC_EINVAL;
        }
        memcpy(mo, r.T, sizeof(mo));
        used[0] = r.model_used; used[1] = r.n_inliers;
    } else if (fitted && f.n) {
        memcpy(mo, st + RC_FS_MOTION, sizeof(mo));
        memcpy(used, st + RC_FS_USED, sizeof(used));
    } else if (fitted) {
        mo[2] = st[0]; mo[5] = st[1];
        used[0] = RC_STAB_TRANSLATION; used[1] = 1;
    }
    if (motion) memcpy(motion, mo, sizeof(mo));
    if (model_used) *model_used = used[0];
    if (patches_used) *patches_used = used[1];
    if (shifts)
        for (int i = 0; i < 3 * np; i++) shifts[i] = fitted ? (f.n ? st[RC_FS_SHIFTS + i] : st[i]) : 0.;
    if (frames_pushed) *frames_pushed = f.frames;
    return RC_OK;
}

extern "C" int rcflow_framestab_read(rc_ctx* ctx, int stream, double result[3], long long* frames_pushed) {
    RcSlot* s; RcFrameStab* fp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::fs, "rcflow_framestab_read", s, fp)) return rc;
    RcFrameStab& f = *fp;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(f.zf, s->cur, false);
    if (rc) return rc;
    double r[3] = {0., 0., 0.};
    RC_HIP(hipMemcpyAsync(r, f.res.p, sizeof(r), hipMemcpyDeviceToHost, s->cur));
    RC_HIP(hipStreamSynchronize(s->cur));
    if (result) { result[0] = r[0]; result[1] = r[1]; result[2] = r[2]; }
    if (frames_pushed) *frames_pushed = f.frames;
    return RC_OK;
}
