// rc_pix3.h -- 8UC3 images on the device, shared by the time-exposure, stabiliser, warp and opposing-flow kernels.
//
// A pixel travels as byte0 | byte1 << 8 | byte2 << 16.  A lane owns 4 consecutive pixels of a row: 12 bytes as one
// dwordx3 access (the images are only byte aligned; global memory takes unaligned dwords on this target and the
// compiler emits them for a byte-aligned 12-byte copy), the w % 4 tail pixel by pixel.  A wave owns 256 pixels of a row
// (or of a run of rows), a block RC_PIX3_WAVES waves stacked vertically.
#pragma once

#include "rc_device.h"

#define RC_PIX3_WAVES 4
static_assert(RC_BLOCK == 64 * RC_PIX3_WAVES, "a block is RC_PIX3_WAVES waves, one row (or run of rows) each");

// ---------------------------------------------------------------------------- packed pixels from and to bytes
typedef uint32_t rc_u32x3 __attribute__((ext_vector_type(3)));   // copied as a whole: one dwordx3
__device__ __forceinline__ void rc_pix3_load4(const uint8_t* row, int x0, int n, uint32_t px[4]) {
    const uint8_t* p = row + 3 * (size_t)x0;
    if (n == 4) {
        rc_u32x3 w;
        __builtin_memcpy(&w, p, 12);
        px[0] = w[0] & 0xffffffu;
        px[1] = (w[0] >> 24) | ((w[1] & 0xffffu) << 8);
        px[2] = (w[1] >> 16) | ((w[2] & 0xffu) << 16);
        px[3] = w[2] >> 8;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            px[k] = k < n ? (uint32_t)p[3 * k] | ((uint32_t)p[3 * k + 1] << 8) | ((uint32_t)p[3 * k + 2] << 16) : 0u;
    }
}
__device__ __forceinline__ void rc_pix3_store4(uint8_t* row, int x0, int n, const uint32_t px[4]) {
    uint8_t* p = row + 3 * (size_t)x0;
    if (n == 4) {
        rc_u32x3 w;
        w[0] = px[0] | (px[1] << 24);
        w[1] = (px[1] >> 8) | (px[2] << 16);
        w[2] = (px[2] >> 16) | (px[3] << 8);
        __builtin_memcpy(p, &w, 12);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) {
                p[3 * k] = (uint8_t)px[k];
                p[3 * k + 1] = (uint8_t)(px[k] >> 8);
                p[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
    }
}
// 2 consecutive pixels from 8 bytes, 5 from 16: the caller knows the bytes behind the last pixel are inside the row
__device__ __forceinline__ void rc_pix3_unpack2(const uint8_t* p, uint32_t& p0, uint32_t& p1) {
    uint2 q;
    __builtin_memcpy(&q, p, 8);
    p0 = q.x & 0xffffffu;
    p1 = (q.x >> 24) | ((q.y & 0xffffu) << 8);
}
__device__ __forceinline__ void rc_pix3_unpack5(const uint8_t* p, uint32_t px[5]) {
    uint4 q;
    __builtin_memcpy(&q, p, 16);
    px[0] = q.x & 0xffffffu;
    px[1] = (q.x >> 24) | ((q.y & 0xffffu) << 8);
    px[2] = (q.y >> 16) | ((q.z & 0xffu) << 16);
    px[3] = q.z >> 8;
    px[4] = q.w & 0xffffffu;
}
// pixel (x, y) of a w x h image; 0 outside it (BORDER_CONSTANT, value 0)
__device__ __forceinline__ uint32_t rc_pix3_tap(const uint8_t* src, size_t step, int w, int h, int x, int y) {
    if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return 0u;
    const uint8_t* p = src + (size_t)y * step + 3 * (size_t)x;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// ---------------------------------------------------------------------------- arithmetic on packed pixels
// remap's 8-bit INTER_LINEAR sample (imgwarp.cpp): fractions of 1/32 px, weights of 2^15, rounded per channel
__device__ __forceinline__ uint32_t rc_pix3_bilinear(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int fx, int fy) {
    const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int sh = 8 * c;
        const int v = (int)((p00 >> sh) & 255u) * w00 + (int)((p01 >> sh) & 255u) * w01 +
                      (int)((p10 >> sh) & 255u) * w10 + (int)((p11 >> sh) & 255u) * w11;
        o |= (uint32_t)((v + (1 << 14)) >> 15) << sh;
    }
    return o;
}
// COLOR_BGR2GRAY in 14-bit fixed point, as a float
__device__ __forceinline__ float rc_pix3_gray(uint32_t p) {
    return (float)(int)(((p & 255u) * 1868u + ((p >> 8) & 255u) * 9617u + (p >> 16) * 4899u + (1u << 13)) >> 14);
}

// ---------------------------------------------------------------------------- thread -> pixels, and the grid for it
// columns x0 .. x0 + n - 1 (n <= 0: none) of the rows y0 .. y0 + rows - 1
struct RcPix3Span { int x0, n, y0; };
__device__ __forceinline__ RcPix3Span rc_pix3_span(int w, int rows) {
    RcPix3Span t;
    t.x0 = 4 * (blockIdx.x * 64 + (threadIdx.x & 63));
    t.n = min(4, w - t.x0);
    t.y0 = (blockIdx.y * RC_PIX3_WAVES + (threadIdx.x >> 6)) * rows;
    return t;
}
// host: `large_rows` rows per wave once the image has waves enough to fill the device, one below that
static inline int rc_rows_per_wave(int w, int h, int large_rows) { return (long long)w * h >= (1 << 20) ? large_rows : 1; }
static inline dim3 rc_pix3_grid(int w, int h, int rows) {
    return dim3(((w + 3) / 4 + 63) / 64, (h + RC_PIX3_WAVES * rows - 1) / (RC_PIX3_WAVES * rows));
}
