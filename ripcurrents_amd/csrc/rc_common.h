// rc_common.h -- shared declarations of the HIP implementation (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/rcflow.h"
#include "rc_plan.h"   // RcLevel, RcPolyK, RcWindow and the RC_MAX_* bounds

// Built with -ffp-contract=off: a*b+c rounds twice unless written as fmaf().
#define RC_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

// `(int)float` as the reference's x86 build compiles it (cvttss2si): NaN and values outside int range give
// INT_MIN ("integer indefinite"), where v_cvt_i32_f32 gives 0 and saturates.  Bounds checks written
// for the x86 result (x < 1 || x + 2 > w) then reject such positions instead of letting them through.
__device__ __forceinline__ int rc_cvt_i32_x86(float v) {
    return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000;
}

// finite: neither an infinity nor a NaN (NaN fails the comparison)
__host__ __device__ __forceinline__ bool rc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// helpers the analysis kernels share (analysis_kernels.hip, ripmap_kernels.hip)
__device__ __forceinline__ const float2* rc_row2(const float* base, size_t step, int y) {
    return (const float2*)((const char*)base + (size_t)y * step);
}

// Bilinear sampler shared by every streamline variant (ripcurrents_module.cpp:494-508).
__device__ __forceinline__ bool rc_sample_flow(const float* flow, size_t step, int w, int h, float x, float y,
                                               float& dx, float& dy) {
    int xind = rc_cvt_i32_x86(floorf(x)), yind = rc_cvt_i32_x86(floorf(y));
    float xrem = x - xind, yrem = y - yind;
    if (xind < 1 || yind < 1 || xind + 2 > w || yind + 2 > h) return false;
    const float2* r0 = rc_row2(flow, step, yind) + xind;
    const float2* r1 = rc_row2(flow, step, yind + 1) + xind;
    float2 p00 = r0[0], p01 = r0[1], p10 = r1[0], p11 = r1[1];
    float wa = 1 - xrem, wb = 1 - yrem;
    dx = p00.x * wa * wb + p01.x * xrem * wb + p10.x * wa * yrem + p11.x * xrem * yrem;
    dy = p00.y * wa * wb + p01.y * xrem * wb + p10.y * wa * yrem + p11.y * xrem * yrem;
    return true;
}

// `uchar = float` as x86 compiles it: cvttss2si then the low byte (NaN/overflow -> INT_MIN).
__device__ __forceinline__ uint8_t rc_f2u8(float v) {
    int iv;
    if (!(v > -2147483904.f && v < 2147483648.f)) iv = INT_MIN;
    else iv = (int)v;
    return (uint8_t)(iv & 0xFF);
}

struct RcPyrArgs {
    const uint8_t* src;       // frame 0
    size_t src_step;          // bytes per row
    size_t src_frame_stride;  // bytes per frame
    int W0, H0;
    float* dst;               // I_k slot base
    size_t dst_slot_stride;   // floats per slot
    int dslot0, nslots, zstep; // destination slot of frame z is (dslot0 + z*zstep) % nslots
    int w, h;
    double scale_x, scale_y;
    int ksize;
    const float* kern;        // device, ksize floats
    int tw, th, reg_wp, reg_hmax;
    int direct;               // diagnostic (RC_ABL_PYR_STAGED): the earlier per-pixel / LDS-staged kernels
    int fixed3;               // scale 0: the fixed (1/4, 1/2, 1/4) taps of sigma <= 0 and an identity resize
};

// A pyramid scale written by the scale-0 expansion itself (k_polyexp<..., PYR = 1>)
struct RcPyrFused {
    float* dst;               // I_k slot base
    size_t dst_slot_stride;   // floats per slot
    int w, h;
    const float* kern;        // device: 3 taps (scale 1) / 9 taps (scale 2)
};

struct RcPolyArgs {
    const float* I;           // I_k slot base (scales >= 1, and the stage entry point)
    size_t I_slot_stride;
    const uint8_t* src8;      // scale 0: the 8-bit frames themselves (pyramid fused); else NULL
    size_t src8_step, src8_frame_stride;
    float4* RA;               // (y, x, yy, xx) coefficients
    float* RB;                // xy coefficient
    size_t R_slot_stride;     // elements per slot (pixels)
    int slot0, nslots, zstep;
    int w, h;
    int tile_h;               // rows per block: 32 or 48 (option "poly_tile_h")
    int valu_vertical;        // option "poly_mfma" = 0: vertical pass on the VALU instead of the matrix cores
    RcPolyK pk;
    int npyr;                 // scale 0 only: pyramid scales 1..npyr come out of this launch too
    RcPyrFused py[2];
};

// Option "ablate" (0 in production): every bit selects a bit-identical alternative form of a kernel, or forces a
// production kernel at launch sizes that would not pick it; the bit-identity tests compare the forms.
enum RcAblate : int {
    RC_ABL_EXACT_PLAIN_SCANS = 2,    // option exact, box windows of winsize 3 / 5: the plain scans (V and G row-major in HBM, separate solve)
    RC_ABL_EXACT_FUSED_M = 16,       // option exact, box windows of winsize 3 / 5: FarnebackUpdateMatrices inside the column scan (measured slower)
    RC_ABL_PYR_STAGED = 4096,        // pyramid: per-pixel / LDS-staged kernels
    RC_ABL_TILE_WINDOW = 65536,      // Gaussian winsize 10 / 20: tile kernel even for large launches
    RC_ABL_FORCE_SWEEP = 8388608,    // strip-sweep kernel even for small launches
    RC_ABL_FORCE_CHAIN = 33554432,   // fused winsize-3 kernel: tile chains (option "chain") even for launches too small to want them
};

struct RcIterArgs {
    const float4* RA;         // R slot base of this level
    const float* RB;
    size_t R_slot_stride;
    int slot0, slot1, nslots, zstep; // pair z uses slots (slot0 + z*zstep) % n and (slot1 + z*zstep) % n
    int w, h;
    // flow in: mode 0 zeros, 1 same-resolution, 2 coarser level (resize * mul)
    int in_mode;
    const float2* fin;
    size_t fin_pair_stride;   // elements
    int fin_w, fin_h;
    double up_scale_x, up_scale_y;
    float up_mul;
    int up_exact2;            // the coarse scale is exactly half-size (integer source coordinates, see k_flow_iter2_rr)
    // flow out
    char* fout;
    size_t fout_step;         // bytes per row
    size_t fout_pair_stride;  // bytes per pair
    int tw, th;               // tile (filled by the launcher)
    int tiles_x, tiles_y;
    int solve;                // 0: write flow_in (iterations == 0), 1: normal
    int xcd_remap;            // XCD-aware tile order (speed only)
    int ablate;               // option "ablate" (RcAblate; 0 in production)
    int addr32;               // every offset inside one frame's R planes and one pair's flow field fits 32 bits (set by the level driver)
    int chain_min_blocks;     // option "chain_min_blocks": a launch keeps at least this many blocks when its chains are shortened (0 = 4096)
    int chain;                // option "chain": consecutive pairs a block of the fused winsize-3 kernel walks on its tile (<= 1: none)
    RcWindow win;
};

// Pair groups of a chained launch (k_flow_iter2_rrc): block row g walks pairs start[g] .. start[g + 1] - 1.
#define RC_MAX_CHAIN_GROUPS 64
struct RcChainPlan {
    int ngroups;
    int start[RC_MAX_CHAIN_GROUPS + 1];
};

// Which kernel a flow-iteration launch runs, on which tile (rc_flow_form: host logic only).  rc_launch_flow_iter and
// rc_launch_flow_iter2 switch on this answer, and rcflow_debug_flow_form reports it to the tests, which assert the form
// they claim to test before they run it.
enum RcFlowKernel : int {
    RC_FK_W3 = 1,        // k_flow_iter_w3<in_mode, gauss>: winsize 3, one iteration, 64 x 16 tile
    RC_FK_TILE = 2,      // k_flow_iter<TW, TH, M, G>: compile-time tile (iterations == 0, or a window without a faster form)
    RC_FK_BIG = 3,       // k_flow_iter_big<M, G, NT, TW>: m = 2 / 5 / 10, 32 or 64 x 32 tile
    RC_FK_SWEEP = 4,     // k_flow_iter_sweep<M>: Gaussian m = 5 / 10, strips of 64 columns, th = rows per segment
    RC_FK_RUNTIME = 5,   // k_flow_iter<0, 0, 0, 0>: any other window, runtime tile
    RC_FK_RRC = 6,       // k_flow_iter2_rrc<in_mode, gauss, NIT, D>: winsize 3, two iterations, 28 x (8 NIT - 4) tile
};
struct RcFlowForm {
    int kernel;               // RcFlowKernel
    int tw, th;               // output tile
    int nt;                   // threads per block
    int nit, d;               // RC_FK_RRC: rows per thread and the R1 window's margin; 0 otherwise
    int groups;               // RC_FK_RRC: chain groups (0 = independent pairs)
    int tiles_x, tiles_y;
    int grid_y;               // block rows of the launch: pairs, or chain groups
    int interior;             // RC_FK_RRC: tiles whose M grid lies at least 5 px inside the image (the straight-line path)
};
#define RC_FLOW_FORM_INTS 11

// Option "exact" (exact_kernels.hip): one scale of the upstream CPU operation order, staged through HBM.
struct RcExactArgs {
    const float4* RA;         // R slot base of this scale
    const float* RB;
    size_t n;                 // pixels of the scale (= R slot stride, plane stride of M / V)
    int slot0, slot1, nslots, zstep;
    int w, h;
    const float2* fin;        // flow of the coarser scale (null at the coarsest)
    size_t fin_pair_stride;
    int fin_w, fin_h;
    double up_scale_x, up_scale_y;
    float up_mul;
    float2* flow;             // [pairs][h][w]
    float* M;                 // [pairs][5][h][w]
    void* V;                  // [pairs][5][h][w]: float (Gaussian window) / double (box window)
    void* G;                  // box window: [pairs][5][h][w] double running row sums
    char* out;                // last iteration of scale 0: the caller's buffer (else null -> flow)
    size_t out_step, out_pair_stride;
    int plain_scans;          // RC_ABL_EXACT_PLAIN_SCANS
    int fused_matrices;       // RC_ABL_EXACT_FUSED_M
    RcWindow win;
};
void rc_launch_exact_polyexp(const RcPolyArgs& a, int frames, hipStream_t s);
void rc_launch_exact_flow_init(const RcExactArgs& a, int pairs, hipStream_t s);
void rc_launch_exact_matrices(const RcExactArgs& a, int pairs, hipStream_t s);
void rc_launch_exact_window_solve(const RcExactArgs& a, int pairs, hipStream_t s);
// box windows of winsize 3 / 5: matrices + window + solve of one iteration without M in HBM (reads a.flow, writes a.flow / a.out)
int rc_exact_iteration_fused_ok(const RcExactArgs& a);
void rc_launch_exact_iteration_fused(const RcExactArgs& a, int pairs, hipStream_t s);

// Raises a kernel's dynamic-LDS limit once per (call site, device): the attribute is per device, and a
// process may hold contexts on several devices.
#define RC_MAX_DEVICES 64
#define RC_ALLOW_LDS(fn, lds)                                                                             \
    do {                                                                                                  \
        static size_t rc_seen_[RC_MAX_DEVICES] = {0};                                                     \
        int rc_dev_ = 0;                                                                                  \
        (void)hipGetDevice(&rc_dev_);                                                                     \
        if (rc_dev_ >= 0 && rc_dev_ < RC_MAX_DEVICES && (size_t)(lds) > rc_seen_[rc_dev_]) {             \
            (void)hipFuncSetAttribute((const void*)(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
            rc_seen_[rc_dev_] = (size_t)(lds);                                                            \
        }                                                                                                 \
    } while (0)

void rc_launch_pyr(const RcPyrArgs& a, int frames, size_t lds, hipStream_t s);
void rc_launch_polyexp(const RcPolyArgs& a, int frames, hipStream_t s);
int rc_polyexp_pyr_ok(const RcPolyArgs& a);
// merged launches for a frame or two (see pyr_polyexp_kernels.hip)
int rc_pyr_pair_ok(const RcPyrArgs& a1, const RcPyrArgs& a2);
void rc_launch_pyr_pair(const RcPyrArgs& a1, const RcPyrArgs& a2, int frames, hipStream_t s);
int rc_polyexp_multi_ok(const RcPolyArgs* a, int nlev);
void rc_launch_polyexp_multi(const RcPolyArgs* a, int nlev, int frames, hipStream_t s);
// flow_iter_kernels.hip is built twice: fast arithmetic, and upstream's operation order (Gaussian windows)
#define RC_FLOW_DECLS                                                         \
    void rc_launch_flow_iter(const RcIterArgs& a, int pairs, hipStream_t s);  \
    /* two iterations in one launch (only where rc_flow_iter_can_fuse2 says so) */ \
    int rc_flow_iter_can_fuse2(const RcIterArgs& a);                          \
    int rc_flow_iter2_r0_reads(const RcIterArgs& a, int pairs);               \
    int rc_flow_chain_groups(const RcIterArgs& a, int pairs, int* starts, int cap); \
    /* the form a launch of `fuse` (1 or 2) iterations takes: what the two launchers switch on */ \
    void rc_flow_form(const RcIterArgs& a, int pairs, int fuse, RcFlowForm& f); \
    void rc_launch_flow_iter2(const RcIterArgs& a, int pairs, hipStream_t s);
namespace rc_flow_fast { RC_FLOW_DECLS }
namespace rc_flow_exact { RC_FLOW_DECLS }

// OPTFLOW_USE_INITIAL_FLOW (initial_flow_kernels.hip): `pairs` caller fields of W x H float2 reduced with INTER_AREA to
// the coarsest scale w x h and multiplied by mul = (float)pyr_scale^levels.
struct RcFlowAreaArgs {
    const char* src;          // field of pair 0
    size_t src_step;          // bytes per row
    size_t src_pair_stride;   // bytes per pair
    int W, H;
    float2* dst;              // [pairs][h][w] dense
    size_t dst_pair_stride;   // elements
    int w, h;
    float mul;
    int fast, ix, iy;         // both ratios integers (resizeAreaFast_): W == ix * w, H == iy * h
    // fractional ratios (resizeArea_): DecimateAlpha tables grouped by destination index; xstart has w + 1 entries
    const int* xstart; const int* xsi; const float* xalpha;
    const int* ystart; const int* ysi; const float* yalpha;
    int lds_tab;              // the column-table entries of every 64-column block fit the kernel's LDS staging
};
void rc_launch_flow_area_init(const RcFlowAreaArgs& a, int pairs, hipStream_t s);

// interleave helpers for the stage-level test entry points
void rc_launch_pack_R5(const float* R5, float4* RA, float* RB, int n, int fast_scale, hipStream_t s);
void rc_launch_unpack_R5(const float4* RA, const float* RB, float* R5, int n, int fast_scale, hipStream_t s);
