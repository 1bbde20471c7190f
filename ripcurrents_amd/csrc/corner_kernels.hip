// corner_kernels.hip -- where to track: one best Shi-Tomasi corner per grid cell of an 8UC1 image (rcflow_corners_dev),
// and the gray image of an 8UC3 frame for the tracking stabiliser (stab_kernels.hip, rcflow_framestab_open_tracks).
//
// Response, all integers (include/rcflow.h states it; tests/_trackstab_ref.py restates it in numpy):
//   dx, dy   the 3 x 3 Sobel pair on the bytes                                                       |dx|, |dy| <= 1020
//   a, b, c  sums of dx dx, dx dy, dy dy over the 3 x 3 block around the pixel                       < 2^24
//   R        (a + c) - ceil(sqrt((a - c)^2 + 4 b^2)): twice the smaller eigenvalue of [a b; b c], rounded down; >= 0
// The root is a double estimate corrected by comparison in int64 (D < 2^49 is exact in a double).
//
// One workgroup per cell.  The cell is walked in tiles of CN_TW x CN_TH pixels: the gray tile with its 2-pixel halo and
// the derivative tile with its 1-pixel halo live in LDS (6 KB), so a pixel's nine derivative pairs are computed once
// per tile, not once per neighbour.  A lane keeps its running best as a packed key, R << 32 | ~(y w + x): the largest
// key is the largest R and, among equals, the lowest (y, x).  Wave reduction by shuffles, four waves through LDS, one
// store per cell.  No atomics.  Candidates are at least `margin` >= 2 pixels from every border, so no tile reads outside
// the image and no border rule exists.

#include <math.h>
#include <string.h>

#include "rc_host.h"
#include "rc_pix3.h"

#define CN_TW 64
#define CN_TH 16

struct RcCornerArgs {
    const uint8_t* img; size_t step;
    int w, h, margin, cells_x, cells_y, cw, ch, min_score;   // cw x ch: the cell size (the last column / row takes the remainder)
    float2* pts; int* scores;
};

__device__ __forceinline__ long long cn_ceil_sqrt(long long D) {
    long long s = (long long)sqrt((double)D);
    while (s * s < D) s++;
    while (s > 0 && (s - 1) * (s - 1) >= D) s--;
    return s;
}

__global__ __launch_bounds__(RC_BLOCK) void k_corner_cells(const RcCornerArgs a) {
    __shared__ uint8_t g[CN_TH + 4][CN_TW + 4];
    __shared__ short2 d[CN_TH + 2][CN_TW + 2];
    __shared__ unsigned long long wbest[RC_BLOCK / 64];
    const int tid = threadIdx.x;
    const int cyi = blockIdx.x / a.cells_x, cxi = blockIdx.x - cyi * a.cells_x;
    const int x0 = a.margin + cxi * a.cw, x1 = cxi == a.cells_x - 1 ? a.w - a.margin : x0 + a.cw;
    const int y0 = a.margin + cyi * a.ch, y1 = cyi == a.cells_y - 1 ? a.h - a.margin : y0 + a.ch;
    unsigned long long best = 0ull;
    for (int ty = y0; ty < y1; ty += CN_TH)
        for (int tx = x0; tx < x1; tx += CN_TW) {
            const int tw = min(CN_TW, x1 - tx), th = min(CN_TH, y1 - ty);
            __syncthreads();                               // the previous tile has been read
            for (int i = tid; i < (CN_TH + 4) * (CN_TW + 4); i += RC_BLOCK) {
                const int r = i / (CN_TW + 4), c = i - r * (CN_TW + 4);
                if (r < th + 4 && c < tw + 4) g[r][c] = a.img[(size_t)(ty - 2 + r) * a.step + (size_t)(tx - 2 + c)];
            }
            __syncthreads();
            for (int i = tid; i < (CN_TH + 2) * (CN_TW + 2); i += RC_BLOCK) {
                const int r = i / (CN_TW + 2), c = i - r * (CN_TW + 2);
                if (r < th + 2 && c < tw + 2) {
                    const int dx = (g[r][c + 2] + 2 * g[r + 1][c + 2] + g[r + 2][c + 2]) - (g[r][c] + 2 * g[r + 1][c] + g[r + 2][c]);
                    const int dy = (g[r + 2][c] + 2 * g[r + 2][c + 1] + g[r + 2][c + 2]) - (g[r][c] + 2 * g[r][c + 1] + g[r][c + 2]);
                    d[r][c] = make_short2((short)dx, (short)dy);
                }
            }
            __syncthreads();
            for (int i = tid; i < CN_TH * CN_TW; i += RC_BLOCK) {
                const int r = i / CN_TW, c = i - r * CN_TW;
                if (r >= th || c >= tw) continue;
                int sa = 0, sb = 0, sc = 0;
#pragma unroll
                for (int v = 0; v < 3; v++)
#pragma unroll
                    for (int u = 0; u < 3; u++) {
                        const short2 e = d[r + v][c + u];
                        sa += e.x * e.x; sb += e.x * e.y; sc += e.y * e.y;
                    }
                const long long da = (long long)sa - sc;
                const long long D = da * da + 4ll * sb * sb;
                const long long R = (long long)sa + sc - cn_ceil_sqrt(D);
                const unsigned idx = (unsigned)(ty + r) * (unsigned)a.w + (unsigned)(tx + c);
                const unsigned long long key = ((unsigned long long)R << 32) | (0xffffffffu - idx);
                best = key > best ? key : best;
            }
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long ob = __shfl_xor(best, o, 64);
        best = ob > best ? ob : best;
    }
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < RC_BLOCK / 64; k++) best = wbest[k] > best ? wbest[k] : best;
    const int R = (int)(best >> 32);
    if (R == 0 || R < a.min_score) {
        a.pts[blockIdx.x] = make_float2((float)(x0 + x1 - 1) * 0.5f, (float)(y0 + y1 - 1) * 0.5f);
        a.scores[blockIdx.x] = 0;
    } else {
        const unsigned idx = 0xffffffffu - (unsigned)(best & 0xffffffffull);
        const unsigned y = idx / (unsigned)a.w;
        a.pts[blockIdx.x] = make_float2((float)(idx - y * (unsigned)a.w), (float)y);
        a.scores[blockIdx.x] = R;
    }
}

// COLOR_BGR2GRAY of rc_pix3.h as bytes, rows packed (pitch w): level 0 of a PyrLK pyramid
__global__ __launch_bounds__(RC_BLOCK) void k_bgr_to_gray(const uint8_t* __restrict__ src, size_t step, int w, int h, uint8_t* __restrict__ dst) {
    const RcPix3Span t = rc_pix3_span(w, 1);
    if (t.n <= 0 || t.y0 >= h) return;
    uint32_t px[4];
    rc_pix3_load4(src + (size_t)t.y0 * step, t.x0, t.n, px);
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t p = px[k];
        packed |= (((p & 255u) * 1868u + ((p >> 8) & 255u) * 9617u + (p >> 16) * 4899u + (1u << 13)) >> 14) << (8 * k);
    }
    uint8_t* o = dst + (size_t)t.y0 * w + t.x0;
    if (t.n == 4) {
        __builtin_memcpy(o, &packed, 4);
    } else {
        for (int k = 0; k < t.n; k++) o[k] = (uint8_t)(packed >> (8 * k));
    }
}

// ============================================================================ host side
// "trackstab@0": the gray image of a frame
void rc_gray_launch(rc_ctx* ctx, hipStream_t cur, const uint8_t* d_bgr, size_t step, int w, int h, uint8_t* d_gray) {
    RcProfScope ps(ctx, cur, RC_K_TRACKSTAB, 0, 4. * w * h);
    hipLaunchKernelGGL(k_bgr_to_gray, rc_pix3_grid(w, h, 1), dim3(RC_BLOCK), 0, cur, d_bgr, step, w, h, d_gray);
}

int rc_corner_check(const char* who, int w, int h, int cells_x, int cells_y, int margin, int min_score) {
    if (margin < 2 || min_score < 0 || cells_x < 1 || cells_y < 1 || (long long)cells_x * cells_y > RC_CORNER_MAX_CELLS) {
        rc_set_error("%s: margin %d (>= 2), min_score %d (>= 0) or %d x %d cells (1..%d)", who, margin, min_score, cells_x, cells_y,
                     RC_CORNER_MAX_CELLS);
        return RC_EINVAL;
    }
    if ((w - 2 * margin) / cells_x < 8 || (h - 2 * margin) / cells_y < 8) {
        rc_set_error("%s: %d x %d cells over the %d x %d candidates of a %d x %d image are below 8 px a side", who, cells_x, cells_y,
                     w - 2 * margin, h - 2 * margin, w, h);
        return RC_EINVAL;
    }
    return RC_OK;
}

// "trackstab@5": the corner cells
void rc_corner_launch(rc_ctx* ctx, hipStream_t cur, const uint8_t* d_gray, size_t step, int w, int h, int cells_x, int cells_y, int margin,
                      int min_score, float* d_pts, int* d_scores) {
    RcCornerArgs a;
    memset(&a, 0, sizeof(a));
    a.img = d_gray; a.step = step; a.w = w; a.h = h; a.margin = margin; a.cells_x = cells_x; a.cells_y = cells_y;
    a.cw = (w - 2 * margin) / cells_x; a.ch = (h - 2 * margin) / cells_y; a.min_score = min_score;
    a.pts = (float2*)d_pts; a.scores = d_scores;
    RcProfScope ps(ctx, cur, RC_K_TRACKSTAB, 5, 1. * w * h + 12. * cells_x * cells_y);
    hipLaunchKernelGGL(k_corner_cells, dim3(cells_x * cells_y), dim3(RC_BLOCK), 0, cur, a);
}

extern "C" int rcflow_corners_dev(rc_ctx* ctx, int stream, const uint8_t* d_gray, size_t step, int w, int h, int cells_x, int cells_y,
                                  int margin, int min_score, float* d_pts, int* d_scores) {
    static const char* who = "rcflow_corners_dev";
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    int rc;
    if ((rc = rc_image_check(who, "d_gray", d_gray, step, w, h, 1, 1, RC_ARG_IN))) return rc;
    if (!d_pts || !d_scores) { rc_set_error("%s: a null pointer among d_pts, d_scores", who); return RC_EINVAL; }
    if ((rc = rc_corner_check(who, w, h, cells_x, cells_y, margin, min_score))) return rc;
    if ((rc = rc_fits_context(who, ctx, w, h))) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    rc_corner_launch(ctx, s->cur, d_gray, step, w, h, cells_x, cells_y, margin, min_score, d_pts, d_scores);
    RC_HIP(hipGetLastError());
    return RC_OK;
}
