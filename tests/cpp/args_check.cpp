// args_check.cpp -- the argument rules of the device entry points (ripcurrents_amd/csrc/rc_args.cpp) swept against their
// plainest statement: interval intersection on explicit integers plus modulo tests.  Built from that file alone under
// AddressSanitizer + UBSan (tests/test_args_host.py).  Host code only; exits 0 and prints "args_check: ok" when the
// collector and the statement agree everywhere.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../ripcurrents_amd/csrc/rc_args.h"

static char g_text[512];
void rc_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof(g_text), fmt, ap);
    va_end(ap);
}

static long g_checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        g_checks++;                                       \
        if (!(cond)) {                                    \
            fprintf(stderr, "args_check: %s: ", #cond);   \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

// every pointer handed to the collector lies in this buffer; the statement works on the offsets (the base is 64-byte aligned)
alignas(64) static unsigned char g_buf[1 << 14];

// one declared argument, as integers.  off < 0: a null pointer
struct Item { bool img; long off; long step; int w, h, bpp, align; bool out, optional, any_base; };

static long lo(const Item& a) { return a.off; }
static long hi(const Item& a) { return a.img ? a.off + (long)(a.h - 1) * a.step + (long)a.w * a.bpp : a.off + a.w; }   // an array: w bytes

// the rules a second time
static bool form_ok(const Item& a) {
    if (a.off < 0) return a.optional;
    if (a.img && a.step < (long)a.w * a.bpp) return false;
    if (a.img && a.step % a.align) return false;
    return a.any_base || a.off % a.align == 0;
}
static bool intersects(const Item& a, const Item& b) { return (lo(a) > lo(b) ? lo(a) : lo(b)) < (hi(a) < hi(b) ? hi(a) : hi(b)); }
static bool statement(const Item* it, int n, int ip_out, int ip_in) {
    for (int i = 0; i < n; i++)
        if (!form_ok(it[i])) return false;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            if (i == j || it[i].off < 0 || it[j].off < 0 || !it[i].out) continue;      // an output against everything else
            if (!intersects(it[i], it[j])) continue;
            const bool pair = (i == ip_out && j == ip_in) || (j == ip_out && i == ip_in);
            if (pair && it[i].off == it[j].off && it[i].step == it[j].step) continue;
            return false;
        }
    return true;
}

static const char* const NAMES[8] = {"a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7"};
static int collector(const Item* it, int n, int W, int H, int ip_out, int ip_in) {
    RcArgs a("args_check", W, H);
    for (int i = 0; i < n; i++) {
        const Item& x = it[i];
        const void* p = x.off < 0 ? nullptr : g_buf + x.off;
        const int flags = (x.out ? RC_ARG_OUT : RC_ARG_IN) | (x.optional ? RC_ARG_OPTIONAL : 0) | (x.any_base ? RC_ARG_ANY_BASE : 0);
        int idx;
        if (!x.img) idx = a.array(NAMES[i], p, (size_t)x.w, x.align, flags);
        else if (x.w == W && x.h == H) idx = a.image(NAMES[i], p, (size_t)x.step, x.bpp, x.align, flags);
        else idx = a.image(NAMES[i], p, (size_t)x.step, x.bpp, x.align, flags, x.w, x.h);
        CHECK(idx == i, "declaration %d got index %d", i, idx);
    }
    if (ip_out >= 0) a.in_place(ip_out, ip_in);
    g_text[0] = 0;
    const int rc = a.check();
    CHECK(rc == RC_OK || rc == RC_EINVAL, "check() returned %d", rc);
    CHECK(rc == RC_OK ? !g_text[0] : (strncmp(g_text, "args_check: ", 12) == 0 && g_text[12]), "rc %d with the text \"%s\"", rc, g_text);
    return rc;
}

static long g_seen[8];
enum { TOUCH_OK, ONE_BYTE_REFUSED, IN_OVER_IN_OK, IN_PLACE_OK, IN_PLACE_STEP_REFUSED, NULL_SKIPPED, NULL_REFUSED, FULL };

static void agree(const Item* it, int n, int W, int H, int ip_out = -1, int ip_in = -1) {
    const bool want = statement(it, n, ip_out, ip_in);
    const int rc = collector(it, n, W, H, ip_out, ip_in);
    if ((rc == RC_OK) != want) {
        fprintf(stderr, "args_check: the collector %s what the statement %s (\"%s\"):\n", rc ? "refuses" : "accepts", want ? "accepts" : "refuses", g_text);
        for (int i = 0; i < n; i++)
            fprintf(stderr, "  %s %s off %ld step %ld %dx%d bpp %d align %d%s%s%s\n", NAMES[i], it[i].img ? "image" : "array", it[i].off, it[i].step,
                    it[i].w, it[i].h, it[i].bpp, it[i].align, it[i].out ? " out" : " in", it[i].optional ? " optional" : "", it[i].any_base ? " any_base" : "");
        fprintf(stderr, "  in place: %d over %d\n", ip_out, ip_in);
        exit(1);
    }
    g_checks++;
}

static unsigned g_rng = 12345;
static int rnd(int n) { g_rng = g_rng * 1664525u + 1013904223u; return (int)((g_rng >> 8) % (unsigned)n); }

int main() {
    const int BPP[4] = {1, 3, 4, 8}, ALIGN[3] = {1, 4, 8};
    // 1. the form of one image: every size, pixel size, step, base offset and alignment, with and without the base exempt
    for (int w = 1; w <= 5; w++)
        for (int h = 1; h <= 5; h++)
            for (int bpp : BPP)
                for (long step = (long)w * bpp - 1; step <= (long)w * bpp + 9; step++)
                    for (long off = 0; off <= 16; off++)
                        for (int align : ALIGN)
                            for (int any = 0; any < 2; any++) {
                                const Item x = {true, 64 + off, step, w, h, bpp, align, (w + h) % 2 == 1, false, any == 1};
                                agree(&x, 1, w, h);
                            }
    // null: skipped when optional, refused when required; an empty size is refused
    for (int img = 0; img < 2; img++)
        for (int out = 0; out < 2; out++) {
            Item x[2] = {{true, 64, 8, 2, 2, 4, 4, false, false, false}, {img == 1, -1, 8, 2, 2, 4, 4, out == 1, true, false}};
            agree(x, 2, 2, 2);
            CHECK(collector(x, 2, 2, 2, -1, -1) == RC_OK, "an optional null argument was not skipped");
            g_seen[NULL_SKIPPED]++;
            x[1].optional = false;
            agree(x, 2, 2, 2);
            CHECK(collector(x, 2, 2, 2, -1, -1) == RC_EINVAL, "a required null argument was accepted");
            g_seen[NULL_REFUSED]++;
        }
    for (int k = 0; k < 2; k++) {
        const Item x = {true, 64, 64, k ? 0 : 4, k ? 4 : 0, 3, 1, false, false, false};
        CHECK(collector(&x, 1, 4, 4, -1, -1) == RC_EINVAL, "an empty size was accepted");
    }

    // 2. pairs: an image and an array at every position from before its first byte to after its last, in the four roles
    for (int w = 1; w <= 5; w++)
        for (int h = 1; h <= 5; h++)
            for (int bpp : BPP)
                for (long pad : {0L, 1L, 9L})
                    for (int nb : {1, 4, 9}) {
                        const long step = (long)w * bpp + pad;
                        Item x[2] = {{true, 128, step, w, h, bpp, 1, false, false, false}, {false, 0, 0, nb, 1, 1, 1, false, false, false}};
                        for (long off = lo(x[0]) - nb - 1; off <= hi(x[0]) + 1; off++)
                            for (int roles = 0; roles < 4; roles++) {
                                x[1].off = off;
                                x[0].out = roles & 1; x[1].out = (roles & 2) != 0;
                                agree(x, 2, w, h);
                                const bool touch = off + nb == lo(x[0]) || off == hi(x[0]), one = off + nb == lo(x[0]) + 1 || off == hi(x[0]) - 1;
                                if (roles && touch) { CHECK(collector(x, 2, w, h, -1, -1) == RC_OK, "ranges that touch end to start were refused"); g_seen[TOUCH_OK]++; }
                                if (roles && one) { CHECK(collector(x, 2, w, h, -1, -1) == RC_EINVAL, "ranges that share one byte were accepted"); g_seen[ONE_BYTE_REFUSED]++; }
                                if (!roles && one) { CHECK(collector(x, 2, w, h, -1, -1) == RC_OK, "an input over an input was refused"); g_seen[IN_OVER_IN_OK]++; }
                            }
                    }

    // 3. up to three images and two arrays in every role assignment, placed so that they often meet; the in-place pair
    for (int ni = 0; ni <= 3; ni++)
        for (int na = 0; na <= 2; na++)
            for (int roles = 0; roles < 1 << (ni + na); roles++)
                for (int trial = 0; trial < 600; trial++) {
                    const int n = ni + na, W = 1 + rnd(5), H = 1 + rnd(5);
                    if (!n) continue;
                    Item x[5];
                    long next = 64 + rnd(17);
                    for (int i = 0; i < n; i++) {
                        Item& a = x[i];
                        a.img = i < ni;
                        a.bpp = a.img ? BPP[rnd(4)] : 1;
                        a.align = ALIGN[rnd(3)];
                        a.w = a.img ? (rnd(4) ? W : 1 + rnd(5)) : 1 + rnd(40);
                        a.h = a.img ? (a.w == W ? H : 1 + rnd(5)) : 1;
                        a.step = a.img ? (long)a.w * a.bpp + (rnd(8) ? rnd(10) : -1) : 0;
                        if (a.img && rnd(2)) a.step += (a.align - a.step % a.align) % a.align;   // half of them: an aligned step
                        a.out = (roles >> i) & 1;
                        a.optional = rnd(4) == 0;
                        a.any_base = rnd(8) == 0;
                        a.off = rnd(16) == 0 ? -1 : next + (rnd(3) ? 0 : rnd(9) - 6);
                        if (a.off >= 0 && rnd(2)) a.off += (a.align - a.off % a.align) % a.align;
                        if (a.off >= 0) next = hi(a) > next ? hi(a) : next;
                    }
                    int ip_out = -1, ip_in = -1;
                    if (ni >= 2 && rnd(2)) {                  // image 1 over image 0: the same pointer, the same step or another
                        ip_out = 1; ip_in = 0;
                        if (rnd(2) && x[0].off >= 0) {
                            x[1].off = x[0].off; x[1].w = x[0].w; x[1].h = x[0].h; x[1].bpp = x[0].bpp;
                            x[1].step = rnd(2) ? x[0].step : x[0].step + x[1].align;
                        }
                    }
                    agree(x, n, W, H, ip_out, ip_in);
                }
    // the in-place pair by itself, as rcflow_regions_push_dev declares it
    for (long pad : {0L, 3L})
        for (int d = 0; d < 3; d++) {
            const long step = 5 + pad;
            Item x[2] = {{true, 64, step, 5, 4, 1, 1, false, false, false}, {true, 64 + (d == 2), step + (d == 1), 5, 4, 1, 1, true, true, false}};
            agree(x, 2, 5, 4, 1, 0);
            const int rc = collector(x, 2, 5, 4, 1, 0);
            CHECK((rc == RC_OK) == (d == 0), "in place with d = %d gave %d", d, rc);
            g_seen[d == 0 ? IN_PLACE_OK : IN_PLACE_STEP_REFUSED] += d < 2;
            CHECK(collector(x, 2, 5, 4, -1, -1) == RC_EINVAL, "an output over an input was accepted without the declaration");
        }

    // 4. the collector at its capacity: RC_ARGS_MAX arguments side by side, then the last one moved onto the first; one too many
    {
        Item x[8];
        for (int i = 0; i < 8; i++) x[i] = {i < 3, 64 + 32L * i, 8, i < 3 ? 2 : 32, i < 3 ? 4 : 1, i < 3 ? 4 : 1, 4, i >= 2, false, false};
        CHECK(RC_ARGS_MAX == 7, "the capacity is %d: this case wants another count", (int)RC_ARGS_MAX);
        agree(x, 7, 2, 4);
        CHECK(collector(x, 7, 2, 4, -1, -1) == RC_OK, "seven arguments side by side were refused");
        x[6].off = x[0].off + 28;
        agree(x, 7, 2, 4);
        CHECK(collector(x, 7, 2, 4, -1, -1) == RC_EINVAL, "the seventh argument over the first was accepted");
        g_seen[FULL]++;
        x[6].off = 64 + 32 * 6;
        CHECK(collector(x, 8, 2, 4, -1, -1) == RC_EINVAL, "eight arguments were accepted");
    }

    // rc_prims_check
    CHECK(rc_prims_check("p", g_buf + 4, 1, 0) == RC_OK && rc_prims_check("p", g_buf + 4, RC_DRAW_MAX_THICKNESS, RC_DRAW_COORD_MAX) == RC_OK, "prims");
    CHECK(rc_prims_check("p", nullptr, 1, 0) == RC_EINVAL && rc_prims_check("p", g_buf + 2, 1, 0) == RC_EINVAL, "prims pointer");
    CHECK(rc_prims_check("p", g_buf, 0, 0) == RC_EINVAL && rc_prims_check("p", g_buf, RC_DRAW_MAX_THICKNESS + 1, 0) == RC_EINVAL, "prims thickness");
    CHECK(rc_prims_check("p", g_buf, 1, -1) == RC_EINVAL && rc_prims_check("p", g_buf, 1, RC_DRAW_COORD_MAX + 1) == RC_EINVAL, "prims radius");

    // 5. the named forms against the predicates the entry points spelt out before they had them, as plain integer arithmetic.
    // rc_flow_check: p && w > 0 && h > 0 && step >= 8 * w && !(step & 7); nothing asked of the base
    long flow_odd_base_ok = 0, clip_cases = 0;
    for (int w = -1; w <= 5; w++)
        for (int h = -1; h <= 4; h++)
            for (long step = 0; step <= 8L * 5 + 9; step++)
                for (long off = -1; off <= 15; off++) {
                    const bool want = off >= 0 && w > 0 && h > 0 && step >= 8L * w && !(step & 7);
                    g_text[0] = 0;
                    const int rc = rc_flow_check("flow_form", "d_flow", off < 0 ? nullptr : g_buf + 64 + off, (size_t)step, w, h, (w + h) & 1 ? RC_ARG_OUT : RC_ARG_IN);
                    CHECK((rc == RC_OK) == want && (rc == RC_OK || rc == RC_EINVAL), "rc_flow_check gave %d at w %d h %d step %ld off %ld", rc, w, h, step, off);
                    CHECK(rc == RC_OK || (!strncmp(g_text, "flow_form: ", 11) && strstr(g_text, "d_flow")), "rc_flow_check's text \"%s\"", g_text);
                    if (rc == RC_OK && (off & 7)) flow_odd_base_ok++;
                }
    CHECK(flow_odd_base_ok > 0, "no flow field at a base off 8 bytes was accepted");
    // rc_clip_check: the image form of the first frame, and for n > 1 frame_stride >= step * (h - 1) + w * bpp
    for (int bpp : {1, 8})
        for (int w = 1; w <= 4; w++)
            for (int h = 1; h <= 4; h++)
                for (long pad = -1; pad <= 2; pad++)
                    for (int n = -1; n <= 3; n++)
                        for (long d = -2; d <= 2; d++)
                            for (int null = 0; null < 2; null++) {
                                const long step = (long)w * bpp + pad * (pad > 0 ? bpp : 1), bound = step * (h - 1) + (long)w * bpp, stride = bound + d;
                                if (stride < 0) continue;
                                const bool want = !null && step >= (long)w * bpp && (n <= 1 || stride >= bound);
                                g_text[0] = 0;
                                const int rc = rc_clip_check("clip_form", "d_frames", null ? nullptr : g_buf + 3, (size_t)stride, (size_t)step, n, w, h, bpp, 1, RC_ARG_IN);
                                CHECK((rc == RC_OK) == want && (rc == RC_OK || rc == RC_EINVAL), "rc_clip_check gave %d at bpp %d w %d h %d step %ld n %d stride %ld", rc, bpp, w, h, step, n, stride);
                                CHECK(rc == RC_OK || (!strncmp(g_text, "clip_form: ", 11) && strstr(g_text, "d_frames")), "rc_clip_check's text \"%s\"", g_text);
                                clip_cases++;
                            }
    // the frame stride against the alignment, as rcflow_histogram_clip_dev declares its float2 clip (align 8, any base): for n > 1 a
    // stride that is no multiple of it would start the rows of frame 1 off the alignment and is refused; for n <= 1 the stride is
    // not looked at; with align 1 (8-bit frames, and the flow outputs of the Farneback clips) every stride of a frame or more passes
    long clip_stride_refused = 0, clip_stride_ignored = 0;
    for (int w = 1; w <= 3; w++)
        for (int h = 1; h <= 3; h++)
            for (long pad = 0; pad <= 16; pad += 8)
                for (int n = 0; n <= 3; n++)
                    for (long d = 0; d <= 17; d++)
                        for (int align : {1, 8}) {
                            const long step = 8L * w + pad, bound = step * (h - 1) + 8L * w, stride = bound + d;
                            const bool want = n <= 1 || stride % align == 0;
                            g_text[0] = 0;
                            const int rc = rc_clip_check("clip_form", "d_flows", g_buf + 4, (size_t)stride, (size_t)step, n, w, h, 8, align, RC_ARG_IN | RC_ARG_ANY_BASE);
                            CHECK((rc == RC_OK) == want && (rc == RC_OK || rc == RC_EINVAL), "rc_clip_check gave %d at align %d w %d h %d step %ld n %d stride %ld", rc, align, w, h, step, n, stride);
                            CHECK(rc == RC_OK || (!strncmp(g_text, "clip_form: ", 11) && strstr(g_text, "d_flows")), "rc_clip_check's text \"%s\"", g_text);
                            if (!want) clip_stride_refused++;
                            if (n <= 1 && stride % align) clip_stride_ignored++;
                            clip_cases++;
                        }
    CHECK(clip_stride_refused > 0 && clip_stride_ignored > 0, "no clip with a frame stride off the alignment was refused (%ld) or, with one frame, accepted (%ld)",
          clip_stride_refused, clip_stride_ignored);
    // rc_ptr_check: null, and the base against the alignment
    CHECK(rc_ptr_check("p", "x", nullptr) == RC_EINVAL && rc_ptr_check("p", "x", nullptr, 16, RC_ARG_OPTIONAL) == RC_OK, "a null pointer");
    for (int off = 0; off < 32; off++)
        for (int align : {1, 8, 16}) CHECK((rc_ptr_check("p", "x", g_buf + off, align) == RC_OK) == (off % align == 0), "a pointer at %d, alignment %d", off, align);

    for (int k = 0; k < 8; k++) CHECK(g_seen[k] > 0, "case kind %d never occurred", k);
    printf("args_check: ok (%ld checks; touching %ld, one byte %ld, input over input %ld; flow fields at an odd base %ld, clips %ld)\n", g_checks,
           g_seen[TOUCH_OK], g_seen[ONE_BYTE_REFUSED], g_seen[IN_OVER_IN_OK], flow_odd_base_ok, clip_cases);
    return 0;
}
