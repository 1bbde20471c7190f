// timex_kernels.hip -- time-exposure images on the device: the reference's compute_timex (main.cpp:1195-1263,
// running mean of the colour frames) and compute_brightColor (main.cpp:1265-1383: a ring of the last `window`
// frames in HSV, reduced per pixel to its average, its brightest or its darkest sample), plus the 8-bit colour
// conversions they use (OpenCV 4.1.0 color_hsv.cpp, hue range 180) as stage kernels.
//
// The reference recomputes every ring product from the whole ring on every frame.  Here each product is kept
// incrementally, with the same bits:
//   AVERAGE  the reference adds the `window` quotients q(buf[i]) with saturating 8-bit adds; every term is >= 0, so
//            the result is min(255, sum).  The sum is a per-pixel, per-channel uint16 updated by q(new) - q(old).
//   BRIGHT / DARK  the reference seeds with slot 0 DIVIDED (q of all three channels) and walks the slots 1..window-1,
//            replacing on a strictly better V: the arg-max (arg-min) with the lowest slot index winning ties.  The
//            state is the winner's slot index and output triple.  A push into slot c that is not the winner wins
//            iff it is strictly better, or equal with c below the winner's index.  A push into the winner's own slot
//            keeps it the winner when the new value is not worse (everything below it was strictly worse, everything
//            above it not better); otherwise that pixel walks the V plane of the ring again as the reference does.
//
// Layout: rc_pix3.h's (a thread owns 4 consecutive pixels of a row).  The state is planar with a row pitch of a multiple
// of 4 pixels, so that every state access of a thread is one aligned dword / dwordx2 / dwordx4.

#include "rc_host.h"
#include "rc_pix3.h"

__device__ __forceinline__ uint32_t tx_byte(uint32_t v, int k) { return (v >> (8 * k)) & 255u; }

// ---------------------------------------------------------------------------- colour conversions
// cvRound(num / (double)i) for integers: the quotient is exact in double wherever it is a tie
__device__ __forceinline__ int tx_div_rne(int num, int i) {
    const int q = num / i, r = num - q * i;
    return q + ((2 * r > i || (2 * r == i && (q & 1))) ? 1 : 0);
}
// RGB2HSV_b's tables: sdiv[i] = cvRound((255 << 12) / (1.0 * i)), hdiv[i] = cvRound((180 << 12) / (6.0 * i))
__device__ __forceinline__ void tx_hsv_tables(int* sdiv, int* hdiv) {
    for (int i = threadIdx.x; i < 256; i += RC_BLOCK) {
        sdiv[i] = i ? tx_div_rne(255 << 12, i) : 0;
        hdiv[i] = i ? tx_div_rne((180 << 12) / 6, i) : 0;
    }
}
__device__ __forceinline__ uint32_t tx_rgb_to_hsv(uint32_t p, const int* sdiv, const int* hdiv) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    const int v = max(r, max(g, b)), diff = v - min(r, min(g, b));
    const int s = (diff * sdiv[v] + 2048) >> 12;
    int h = (v == r) ? g - b : (v == g) ? b - r + 2 * diff : r - g + 4 * diff;
    h = (h * hdiv[diff] + 2048) >> 12;
    if (h < 0) h += 180;
    h = min(max(h, 0), 255);
    return (uint32_t)h | ((uint32_t)s << 8) | ((uint32_t)v << 16);
}
__device__ __forceinline__ uint32_t tx_sat_u8(float x) {
    const int i = __float2int_rn(x);
    return (uint32_t)min(max(i, 0), 255);
}
// HSV2RGB_b: through HSV2RGB_f with hscale = 6 / 180; byte 0 of the result is "R" (COLOR_HSV2RGB)
__device__ __forceinline__ uint32_t tx_hsv_to_rgb(uint32_t p) {
    float hh = (float)(p & 255);
    const float ss = (float)((p >> 8) & 255) * (1.f / 255.f), vv = (float)((p >> 16) & 255) * (1.f / 255.f);
    float b, g, r;
    if (ss == 0) b = g = r = vv;
    else {
        hh *= 6.f / 180.f;
        if (hh >= 6.f) hh -= 6.f;             // upstream loops; a hue byte is at most 255 = 8.5 sectors: one step
        int sector = (int)floorf(hh);
        hh -= sector;
        if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
        const float t0 = vv, t1 = vv * (1.f - ss), t2 = vv * (1.f - ss * hh), t3 = vv * (1.f - ss * (1.f - hh));
        switch (sector) {
            case 0: b = t1; g = t3; r = t0; break;
            case 1: b = t1; g = t0; r = t2; break;
            case 2: b = t3; g = t0; r = t1; break;
            case 3: b = t0; g = t2; r = t1; break;
            case 4: b = t0; g = t1; r = t3; break;
            default: b = t2; g = t1; r = t0; break;
        }
    }
    return tx_sat_u8(r * 255.f) | (tx_sat_u8(g * 255.f) << 8) | (tx_sat_u8(b * 255.f) << 16);
}

__global__ __launch_bounds__(RC_BLOCK) void k_rgb_to_hsv_u8(const uint8_t* rgb, size_t step, int w, int h, uint8_t* hsv,
                                                            size_t hsv_step, int rows) {
    __shared__ int sdiv[256], hdiv[256];
    tx_hsv_tables(sdiv, hdiv);
    __syncthreads();
    const RcPix3Span t = rc_pix3_span(w, rows);
    const int x0 = t.x0, n = t.n;
    if (n <= 0) return;
    for (int y = t.y0; y < min(t.y0 + rows, h); y++) {
        uint32_t px[4];
        rc_pix3_load4(rgb + (size_t)y * step, x0, n, px);
#pragma unroll
        for (int k = 0; k < 4; k++) px[k] = tx_rgb_to_hsv(px[k], sdiv, hdiv);
        rc_pix3_store4(hsv + (size_t)y * hsv_step, x0, n, px);
    }
}

__global__ __launch_bounds__(RC_BLOCK) void k_hsv_to_rgb_u8(const uint8_t* hsv, size_t hsv_step, int w, int h, uint8_t* rgb,
                                                            size_t step, int rows) {
    const RcPix3Span t = rc_pix3_span(w, rows);
    const int x0 = t.x0, n = t.n;
    if (n <= 0) return;
    for (int y = t.y0; y < min(t.y0 + rows, h); y++) {
        uint32_t px[4];
        rc_pix3_load4(hsv + (size_t)y * hsv_step, x0, n, px);
#pragma unroll
        for (int k = 0; k < 4; k++) px[k] = tx_hsv_to_rgb(px[k]);
        rc_pix3_store4(rgb + (size_t)y * step, x0, n, px);
    }
}

// ---------------------------------------------------------------------------- MEAN (main.cpp:1231-1241)
// sum: [h][pitch][3] fp32.  sum += frame; out = convertTo(8U) of sum * (float)(1.0 / n)
__global__ __launch_bounds__(RC_BLOCK) void k_timex_mean(const uint8_t* frame, size_t step, int w, int h, float* sum, int pitch,
                                                         float rn, uint8_t* out, size_t out_step, int rows) {
    const RcPix3Span t = rc_pix3_span(w, rows);
    const int x0 = t.x0, n = t.n;
    if (n <= 0) return;
    for (int y = t.y0; y < min(t.y0 + rows, h); y++) {
        uint32_t px[4];
        rc_pix3_load4(frame + (size_t)y * step, x0, n, px);
        float4* sp = (float4*)(sum + ((size_t)y * pitch + x0) * 3);
        float4 q[3] = {sp[0], sp[1], sp[2]};
        float* s = (float*)q;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t o = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                s[3 * k + c] += (float)tx_byte(px[k], c);
                o |= tx_sat_u8(s[3 * k + c] * rn) << (8 * c);
            }
            px[k] = o;
        }
        sp[0] = q[0]; sp[1] = q[1]; sp[2] = q[2];
        if (out) rc_pix3_store4(out + (size_t)y * out_step, x0, n, px);
    }
}

// ---------------------------------------------------------------------------- ring products (main.cpp:1305-1363)
struct TxRingArgs {
    const uint8_t* frame; size_t step;
    uint8_t* out[3]; size_t out_step[3];   // AVERAGE, BRIGHT, DARK images (null: state only)
    uint8_t* ring;                         // [window][H, S, V][plane] bytes
    uint16_t* avg;                         // AVERAGE: [H, S, V][plane] sums of q()
    uint16_t* bd_idx[2];                   // BRIGHT, DARK: the winner's slot [plane]
    uint32_t* bd_hsv[2];                   //   and its output triple H | S << 8 | V << 16 [plane]
    size_t plane;                          // pixels per plane (pitch * h, rounded up)
    int w, h, pitch, window, c, products, rows;
    float rw;                              // (float)(1.0 / window)
};

// The reference's walk for one pixel column of the ring: seed with slot 0 divided, then slots 1..window-1, replacing
// on a strictly better V.  vnew is the V dword being written to slot c by this launch (the store may not have landed).
template <bool DARK>
__device__ __forceinline__ void tx_rescan(const TxRingArgs& a, size_t off, uint32_t need, uint32_t hnew, uint32_t snew,
                                          uint32_t vnew, const uint8_t* qt, uint32_t idx[4], uint32_t hsv[4]) {
    const size_t slot = 3 * a.plane;
    const uint8_t* vplane = a.ring + 2 * a.plane + off;
    uint32_t best[4];
    const uint32_t v0 = a.c == 0 ? vnew : *(const uint32_t*)vplane;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (need >> k & 1) { best[k] = qt[tx_byte(v0, k)]; idx[k] = 0; }
    for (int i = 1; i < a.window; i++) {
        const uint32_t vi = i == a.c ? vnew : *(const uint32_t*)(vplane + i * slot);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (need >> k & 1) {
                const uint32_t v = tx_byte(vi, k);
                if (DARK ? v < best[k] : v > best[k]) { best[k] = v; idx[k] = i; }
            }
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (need >> k & 1) {
            const int i = (int)idx[k];
            const uint8_t* t = a.ring + i * slot + off + k;
            uint32_t hh = i == a.c ? tx_byte(hnew, k) : t[0], ss = i == a.c ? tx_byte(snew, k) : t[a.plane];
            if (i == 0) { hh = qt[hh]; ss = qt[ss]; }
            hsv[k] = hh | (ss << 8) | (best[k] << 16);
        }
}

template <bool DARK>
__device__ __forceinline__ void tx_extreme(const TxRingArgs& a, int which, size_t off, const uint32_t px[4], uint32_t hnew,
                                           uint32_t snew, uint32_t vnew, const uint8_t* qt, uint32_t res[4]) {
    uint2* ip = (uint2*)(a.bd_idx[which] + off);
    uint4* tp = (uint4*)(a.bd_hsv[which] + off);
    const uint2 iw = *ip;
    const uint4 tw = *tp;
    uint32_t idx[4] = {iw.x & 0xffffu, iw.x >> 16, iw.y & 0xffffu, iw.y >> 16};
    uint32_t hsv[4] = {tw.x, tw.y, tw.z, tw.w};
    uint32_t need = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // the candidate this push puts into slot c: slot 0 counts divided, all three channels
        uint32_t cand = px[k];
        if (a.c == 0) cand = qt[cand & 255] | ((uint32_t)qt[(cand >> 8) & 255] << 8) | ((uint32_t)qt[cand >> 16] << 16);
        const uint32_t cv = cand >> 16, wv = hsv[k] >> 16;
        const bool better = DARK ? cv < wv : cv > wv;
        if (idx[k] == (uint32_t)a.c) {
            if (better || cv == wv) hsv[k] = cand;      // the winner's slot, not worse than before: still the winner
            else need |= 1u << k;                       // the winner expired
        } else if (better || (cv == wv && (uint32_t)a.c < idx[k])) {
            idx[k] = a.c;
            hsv[k] = cand;
        }
    }
    if (need) tx_rescan<DARK>(a, off, need, hnew, snew, vnew, qt, idx, hsv);
    *ip = make_uint2(idx[0] | (idx[1] << 16), idx[2] | (idx[3] << 16));
    *tp = make_uint4(hsv[0], hsv[1], hsv[2], hsv[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) res[k] = hsv[k];
}

// a product's HSV triples -> its image (COLOR_HSV2RGB, main.cpp:1361), when the caller wants it
__device__ __forceinline__ void tx_emit(uint8_t* out, size_t out_step, int y, int x0, int n, uint32_t hsv[4]) {
    if (!out) return;
#pragma unroll
    for (int k = 0; k < 4; k++) hsv[k] = tx_hsv_to_rgb(hsv[k]);
    rc_pix3_store4(out + (size_t)y * out_step, x0, n, hsv);
}

__global__ __launch_bounds__(RC_BLOCK) void k_timex_ring(const TxRingArgs a) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ uint8_t qt[256];          // q(v) = convertTo(8U) of v * (float)(1.0 / window)
    tx_hsv_tables(sdiv, hdiv);
    for (int i = threadIdx.x; i < 256; i += RC_BLOCK) qt[i] = (uint8_t)tx_sat_u8((float)i * a.rw);
    __syncthreads();
    const RcPix3Span t = rc_pix3_span(a.w, a.rows);
    const int x0 = t.x0, n = t.n;
    if (n <= 0) return;
    for (int y = t.y0; y < min(t.y0 + a.rows, a.h); y++) {
        uint32_t px[4], res[4];
        rc_pix3_load4(a.frame + (size_t)y * a.step, x0, n, px);
        uint32_t hn = 0, sn = 0, vn = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            px[k] = tx_rgb_to_hsv(px[k], sdiv, hdiv);     // columns past w hold the conversion of zeros: zeros
            hn |= tx_byte(px[k], 0) << (8 * k);
            sn |= tx_byte(px[k], 1) << (8 * k);
            vn |= tx_byte(px[k], 2) << (8 * k);
        }
        const size_t off = (size_t)y * a.pitch + x0;
        uint32_t* slot = (uint32_t*)(a.ring + (size_t)a.c * 3 * a.plane + off);
        const size_t pw = a.plane / 4;                    // plane stride in dwords
        if (a.products & RC_TIMEX_AVERAGE) {
            const uint32_t old[3] = {slot[0], slot[pw], slot[2 * pw]}, cur[3] = {hn, sn, vn};
#pragma unroll
            for (int k = 0; k < 4; k++) res[k] = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                uint2* sp = (uint2*)(a.avg + c * a.plane + off);
                const uint2 sw = *sp;
                uint32_t s[4] = {sw.x & 0xffffu, sw.x >> 16, sw.y & 0xffffu, sw.y >> 16};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    s[k] = s[k] + qt[tx_byte(cur[c], k)] - qt[tx_byte(old[c], k)];
                    res[k] |= min(s[k], 255u) << (8 * c);
                }
                *sp = make_uint2(s[0] | (s[1] << 16), s[2] | (s[3] << 16));
            }
            tx_emit(a.out[0], a.out_step[0], y, x0, n, res);
        }
        slot[0] = hn; slot[pw] = sn; slot[2 * pw] = vn;
        if (a.products & RC_TIMEX_BRIGHT) {
            tx_extreme<false>(a, 0, off, px, hn, sn, vn, qt, res);
            tx_emit(a.out[1], a.out_step[1], y, x0, n, res);
        }
        if (a.products & RC_TIMEX_DARK) {
            tx_extreme<true>(a, 1, off, px, hn, sn, vn, qt, res);
            tx_emit(a.out[2], a.out_step[2], y, x0, n, res);
        }
    }
}

// ============================================================================ host side
void rc_state_free(RcTimex& t) {
    rc_buf_free(t.sum); rc_buf_free(t.ring); rc_buf_free(t.avg);
    for (int i = 0; i < 2; i++) { rc_buf_free(t.bd_idx[i]); rc_buf_free(t.bd_hsv[i]); }
    rc_fence_free(t.zf);
    t = RcTimex();
}

static size_t tx_bytes(const RcTimex& t) {
    return t.sum.bytes + t.ring.bytes + t.avg.bytes + t.bd_idx[0].bytes + t.bd_idx[1].bytes + t.bd_hsv[0].bytes + t.bd_hsv[1].bytes;
}

int rc_state_zero(RcSlot& s, RcTimex& t) {
    const int rc = rc_fence_zero(t.zf, s.cur, {&t.sum, &t.ring, &t.avg, &t.bd_idx[0], &t.bd_idx[1], &t.bd_hsv[0], &t.bd_hsv[1]});
    if (!rc) t.frames = t.cur = 0;
    return rc;
}

extern "C" int rcflow_timex_open(rc_ctx* ctx, int stream, int w, int h, int window, int products) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    const int ring_products = products & (RC_TIMEX_AVERAGE | RC_TIMEX_BRIGHT | RC_TIMEX_DARK);
    if (w <= 0 || h <= 0) { rc_set_error("rcflow_timex_open: bad frame size %d x %d", w, h); return RC_EINVAL; }
    if (products <= 0 || products > 15) { rc_set_error("rcflow_timex_open: bad product mask %d", products); return RC_EINVAL; }
    if (ring_products && (window < 1 || window > 4096)) {
        rc_set_error("rcflow_timex_open: window %d outside 1..4096", window);
        return RC_EINVAL;
    }
    int rc = rc_fits_context("rcflow_timex_open", ctx, w, h);
    if (rc) return rc;
    RC_HIP(hipSetDevice(ctx->device));
    RcTimex t;
    t.w = w; t.h = h; t.products = products;
    t.window = ring_products ? window : 0;
    t.pitch = (w + 3) & ~3;
    t.plane = ((size_t)t.pitch * h + 255) & ~(size_t)255;
    if (products & RC_TIMEX_MEAN) rc = rc_buf_ensure(t.sum, t.plane * 3 * sizeof(float));
    if (!rc && ring_products) rc = rc_buf_ensure(t.ring, t.plane * 3 * (size_t)window);
    if (!rc && (products & RC_TIMEX_AVERAGE)) rc = rc_buf_ensure(t.avg, t.plane * 3 * sizeof(uint16_t));
    for (int i = 0; i < 2 && !rc; i++)
        if (products & (i ? RC_TIMEX_DARK : RC_TIMEX_BRIGHT)) {
            rc = rc_buf_ensure(t.bd_idx[i], t.plane * sizeof(uint16_t));
            if (!rc) rc = rc_buf_ensure(t.bd_hsv[i], t.plane * sizeof(uint32_t));
        }
    return rc_state_install(*s, s->tx, t, rc);
}

extern "C" int rcflow_timex_reset(rc_ctx* ctx, int stream) { return rc_state_reset(ctx, stream, &RcSlot::tx, "rcflow_timex_reset"); }
extern "C" int rcflow_timex_close(rc_ctx* ctx, int stream) { return rc_state_close(ctx, stream, &RcSlot::tx); }

extern "C" int rcflow_timex_info(rc_ctx* ctx, int stream, int* w, int* h, int* window, int* products,
                                 long long* frames_pushed, size_t* device_bytes) {
    RcSlot* s; RcTimex* tp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tx, "rcflow_timex_info", s, tp)) return rc;
    const RcTimex& t = *tp;
    if (w) *w = t.w;
    if (h) *h = t.h;
    if (window) *window = t.window;
    if (products) *products = t.products;
    if (frames_pushed) *frames_pushed = t.frames;
    if (device_bytes) *device_bytes = tx_bytes(t);
    return RC_OK;
}

extern "C" int rcflow_timex_push_dev(rc_ctx* ctx, int stream, const uint8_t* d_frame, size_t step, uint8_t* const d_out[4],
                                     const size_t out_step[4]) {
    static const char* who = "rcflow_timex_push_dev";
    static const char* const names[4] = {"d_out[0]", "d_out[1]", "d_out[2]", "d_out[3]"};
    RcSlot* s; RcTimex* tp;
    if (int rc = rc_state_get(ctx, stream, &RcSlot::tx, who, s, tp)) return rc;
    RcTimex& t = *tp;
    uint8_t* out[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t ostep[4] = {0, 0, 0, 0};
    // rows are converted in place in registers, but another product's launch still has to read the frame: an output is apart from it
    RcArgs a(who, t.w, t.h);
    a.image("d_frame", d_frame, step, 3, 1, RC_ARG_IN);
    for (int k = 0; k < 4; k++) {
        if (!d_out || !d_out[k]) continue;
        if (!(t.products & (1 << k))) { rc_set_error("%s: d_out[%d] given for a product that is not open", who, k); return RC_EINVAL; }
        out[k] = d_out[k]; ostep[k] = out_step ? out_step[k] : 0;
        a.image(names[k], out[k], ostep[k], 3, 1, RC_ARG_OUT);
    }
    if (a.check()) return RC_EINVAL;
    RC_HIP(hipSetDevice(ctx->device));
    int rc = rc_fence_wait(t.zf, s->cur, true);
    if (rc) return rc;
    const int rows = rc_rows_per_wave(t.w, t.h, 2);
    const dim3 grid = rc_pix3_grid(t.w, t.h, rows);
    const double npx = (double)t.w * t.h;
    t.frames++;
    if (t.products & RC_TIMEX_MEAN) {
        RcProfScope ps(ctx, s->cur, RC_K_TIMEX, 0, npx * (27. + (out[0] ? 3. : 0.)));
        hipLaunchKernelGGL(k_timex_mean, grid, dim3(RC_BLOCK), 0, s->cur, d_frame, step, t.w, t.h, (float*)t.sum.p, t.pitch,
                           (float)(1.0 / (double)t.frames), out[0], ostep[0], rows);
    }
    if (t.window) {
        TxRingArgs a;
        a.frame = d_frame; a.step = step;
        for (int k = 0; k < 3; k++) { a.out[k] = out[k + 1]; a.out_step[k] = ostep[k + 1]; }
        a.ring = (uint8_t*)t.ring.p;
        a.avg = (uint16_t*)t.avg.p;
        for (int i = 0; i < 2; i++) { a.bd_idx[i] = (uint16_t*)t.bd_idx[i].p; a.bd_hsv[i] = (uint32_t*)t.bd_hsv[i].p; }
        a.plane = t.plane;
        a.w = t.w; a.h = t.h; a.pitch = t.pitch; a.window = t.window; a.c = t.cur; a.products = t.products; a.rows = rows;
        a.rw = (float)(1.0 / (double)t.window);
        // compulsory bytes: frame, the slot's new triple, per product its state both ways and its image;
        // the walks of expired BRIGHT / DARK winners are data dependent and not counted
        double b = 6.;
        if (t.products & RC_TIMEX_AVERAGE) b += 15. + (out[1] ? 3. : 0.);
        if (t.products & RC_TIMEX_BRIGHT) b += 12. + (out[2] ? 3. : 0.);
        if (t.products & RC_TIMEX_DARK) b += 12. + (out[3] ? 3. : 0.);
        RcProfScope ps(ctx, s->cur, RC_K_TIMEX, 1, npx * b);
        hipLaunchKernelGGL(k_timex_ring, grid, dim3(RC_BLOCK), 0, s->cur, a);
        t.cur = t.cur + 1 >= t.window ? 0 : t.cur + 1;
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

static int tx_convert(rc_ctx* ctx, int stream, const uint8_t* d_in, size_t in_step, int w, int h, uint8_t* d_out, size_t out_step,
                      bool to_hsv) {
    RcSlot* s = rc_slot(ctx, stream);
    if (!s) return RC_EINVAL;
    const char* who = to_hsv ? "rcflow_rgb_to_hsv_u8_dev" : "rcflow_hsv_to_rgb_u8_dev";
    if (rc_img3_check(who, "input", d_in, in_step, w, h) || rc_img3_check(who, "output", d_out, out_step, w, h)) return RC_EINVAL;
    if (rc_fits_context(who, ctx, w, h)) return RC_ESIZE;
    RC_HIP(hipSetDevice(ctx->device));
    const int rows = rc_rows_per_wave(w, h, 2);
    const dim3 grid = rc_pix3_grid(w, h, rows);
    {
        RcProfScope ps(ctx, s->cur, RC_K_COLOR_U8, to_hsv ? 0 : 1, 6. * w * h);
        if (to_hsv) hipLaunchKernelGGL(k_rgb_to_hsv_u8, grid, dim3(RC_BLOCK), 0, s->cur, d_in, in_step, w, h, d_out, out_step, rows);
        else hipLaunchKernelGGL(k_hsv_to_rgb_u8, grid, dim3(RC_BLOCK), 0, s->cur, d_in, in_step, w, h, d_out, out_step, rows);
    }
    RC_HIP(hipGetLastError());
    return RC_OK;
}

extern "C" int rcflow_rgb_to_hsv_u8_dev(rc_ctx* ctx, int stream, const uint8_t* d_rgb, size_t step, int w, int h, uint8_t* d_hsv,
                                        size_t hsv_step) {
    return tx_convert(ctx, stream, d_rgb, step, w, h, d_hsv, hsv_step, true);
}
extern "C" int rcflow_hsv_to_rgb_u8_dev(rc_ctx* ctx, int stream, const uint8_t* d_hsv, size_t hsv_step, int w, int h, uint8_t* d_rgb,
                                        size_t step) {
    return tx_convert(ctx, stream, d_hsv, hsv_step, w, h, d_rgb, step, false);
}
