// rc::Infill (include/rcflow_module.hpp) against the C ABI it wraps and against figures that tests/_infill_ref.py printed for the
// same case: 70 x 50 pixels, a field made from integers in 1/16 pixel, one vector that is not a number, the hole pattern p900 of the
// statement (KNOWN iff (7919 x + 104729 y + 31 x y + 17 (x x + y)) mod 1000 >= 900), 7 levels, a grid of 3 x 2 cells.
//   test_infill
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)
#define HIP(call) do { if ((call) != hipSuccess) FAIL("%s failed", #call); } while (0)

static const int W = 70, H = 50;
// what the statement gives: the summary with 7 levels and min_known 1; the sums of the six cells; the summary with 2 levels,
// min_known 2 and zero left where nothing is known
static const long long SUMMARY7[RC_INFILL_SUMMARY] = {354, 0, 3146, 0, 0, 1, 0, 0, 0, 64, 1309, 1716, 57, 0, 0, 0};
static const long long SUMS7[6][RC_INFILL_SUMS] = {{72, 0, 503, 0, 0, 427, 1581, 1198},    {54, 0, 521, 0, 0, 5241, 767, 1270},
                                                   {61, 0, 539, 0, 0, -591, -23884, 1395}, {56, 0, 519, 0, 0, 634, 7199, 1391},
                                                   {58, 0, 517, 0, 0, 219, -6627, 1316},   {53, 0, 547, 0, 0, 8667, -6330, 1488}};
static const float MEANS7[6][3] = {{0.01160326f, 0.04296196f, 2.3817098f},  {0.14241847f, 0.02084239f, 2.43762f},   {-0.01539063f, -0.6219792f, 2.5881262f},
                                   {0.01722826f, 0.195625f, 2.680154f},     {0.00595109f, -0.18008152f, 2.5454545f}, {0.22570312f, -0.16484375f, 2.7202926f}};
static const long long SUMMARY2[RC_INFILL_SUMMARY] = {354, 0, 3070, 76, 0, 2, 0, 0, 0, 0, 3070, 0, 0, 0, 0, 0};

int main() {
    try {
        rc::Pipeline pipe(W, H);
        rc_infill_params p;
        std::memset(&p, 0, sizeof(p));
        p.levels = 7; p.min_known = 1; p.hold = 0; p.grid_x = 3; p.grid_y = 2; p.flags = RC_INFILL_LEAVE_NAN;
        const size_t N = (size_t)W * H;
        std::vector<float> flow(2 * N);
        std::vector<unsigned char> valid(N);
        for (long long y = 0; y < H; y++)
            for (long long x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                flow[2 * i] = (float)((x * 7 + y * 13) % 97 - 48) / 16.0f;
                flow[2 * i + 1] = (float)((x * 5 + y * 11 + x * y) % 89 - 44) / 16.0f;
                valid[i] = (7919 * x + 104729 * y + 31 * x * y + 17 * (x * x + y)) % 1000 >= 900 ? 255 : 0;
            }
        flow[2 * ((size_t)5 * W + 7)] = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> filled(2 * N);
        std::vector<unsigned char> source(N), mask(N), pic(3 * N);
        std::vector<long long> sa, sums_a;
        std::vector<rc_infill_cell> cells_a;
        {
            rc::Infill fi(pipe, p);
            rc::Mat mflow(H, W, 2, 4, flow.data()), mvalid(H, W, 1, 1, valid.data());
            rc::Mat mfilled(H, W, 2, 4, filled.data()), msource(H, W, 1, 1, source.data()), mmask(H, W, 1, 1, mask.data()), mpic(H, W, 3, 1, pic.data());
            rc::Infill::Pictures all;
            all.filled = &mfilled; all.source = &msource; all.mask = &mmask; all.picture = &mpic;
            if (fi.info().launches_per_push != RC_INFILL_LAUNCHES || fi.info().pushes != 0) FAIL("info");
            fi.push(mflow, &mvalid, nullptr, all);
            sa = fi.read(); cells_a = fi.cells(); sums_a = fi.sums();
            for (int k = 0; k < RC_INFILL_SUMMARY; k++)
                if (sa[k] != SUMMARY7[k]) FAIL("summary word %d: %lld, the statement %lld", k, sa[k], SUMMARY7[k]);
            if (cells_a.size() != 6) FAIL("cells");
            for (int c = 0; c < 6; c++) {
                for (int k = 0; k < RC_INFILL_SUMS; k++)
                    if (sums_a[(size_t)RC_INFILL_SUMS * c + k] != SUMS7[c][k]) FAIL("sum %d of cell %d: %lld", k, c, sums_a[(size_t)RC_INFILL_SUMS * c + k]);
                const rc_infill_cell& r = cells_a[c];
                if (r.flags != 0 || r.valued_pm != 1000 || r.known_pm != (int)(SUMS7[c][0] * 1000 / r.pixels)) FAIL("record %d", c);
                if (std::fabs(r.mean_x - MEANS7[c][0]) > 1e-7f || std::fabs(r.mean_y - MEANS7[c][1]) > 1e-7f || std::fabs(r.mean_level - MEANS7[c][2]) > 1e-6f)
                    FAIL("means of cell %d: %.9g %.9g %.9g", c, r.mean_x, r.mean_y, r.mean_level);
            }
            // what must hold of the pictures
            long long cnt[3] = {0, 0, 0};
            for (size_t i = 0; i < N; i++) {
                const int s = source[i];
                const bool known = valid[i] != 0 && i != (size_t)5 * W + 7;
                if (known != (s == 0)) FAIL("source %zu: %d", i, s);
                if (known && std::memcmp(&filled[2 * i], &flow[2 * i], 8)) FAIL("a known vector changed at %zu", i);
                if (!known && (s < 1 || s > 7)) FAIL("a hole without a level at %zu: %d", i, s);
                if (mask[i] != 255 || std::isnan(filled[2 * i]) || std::isnan(filled[2 * i + 1])) FAIL("pixel %zu has no value", i);
                if (std::fabs(filled[2 * i] * 64.f - std::rint(filled[2 * i] * 64.f)) != 0.f) FAIL("pixel %zu is no 64th", i);
                if (known && (pic[3 * i] != 64 || pic[3 * i + 1] != 64 || pic[3 * i + 2] != 64)) FAIL("picture %zu", i);
                cnt[s == 0 ? 0 : 1]++;
            }
            if (cnt[0] != SUMMARY7[0] || cnt[1] != SUMMARY7[2]) FAIL("counted %lld known, %lld filled", cnt[0], cnt[1]);
            fi.set(2, 2, RC_INFILL_LEAVE_ZERO);                   // from the next push on
            if (fi.info().launches_per_push != RC_INFILL_LAUNCHES - 1) FAIL("launches with two levels");
            fi.push(mflow, &mvalid, nullptr, all);
            sa = fi.read(); cells_a = fi.cells(); sums_a = fi.sums();
            for (int k = 0; k < RC_INFILL_SUMMARY; k++)
                if (sa[k] != SUMMARY2[k]) FAIL("two levels, summary word %d: %lld, the statement %lld", k, sa[k], SUMMARY2[k]);
            long long unfilled = 0;
            for (size_t i = 0; i < N; i++)
                if (source[i] == RC_INFILL_UNFILLED) {
                    unfilled++;
                    if (filled[2 * i] != 0.f || filled[2 * i + 1] != 0.f || mask[i] != 0 || pic[3 * i] != 255 || pic[3 * i + 1] != 0 || pic[3 * i + 2] != 255) FAIL("unfilled %zu", i);
                }
            if (unfilled != SUMMARY2[3]) FAIL("unfilled %lld", unfilled);
            bool threw = false;
            try { fi.push(mmask, &mvalid); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw) FAIL("a grey picture was accepted as a field");
            threw = false;
            rc_infill_params q = p;
            q.flags = RC_INFILL_LEAVE_NAN | RC_INFILL_LEAVE_ZERO;
            try { rc::Infill two(pipe, q); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw || fi.info().w != W || fi.info().pushes != 2) FAIL("both patterns were accepted");
        }
        // the second push through the entry points themselves
        rc_ctx* ctx = pipe.context();
        p.levels = 2; p.min_known = 2; p.flags = RC_INFILL_LEAVE_ZERO;
        if (rcflow_infill_open(ctx, 0, W, H, &p) != RC_OK) FAIL("open: %s", rcflow_last_error());
        unsigned char *dvalid = nullptr, *dsource = nullptr;
        float *dflow = nullptr, *dfilled = nullptr;
        HIP(hipMalloc((void**)&dvalid, N)); HIP(hipMalloc((void**)&dsource, N)); HIP(hipMalloc((void**)&dflow, 8 * N)); HIP(hipMalloc((void**)&dfilled, 8 * N));
        HIP(hipMemcpy(dvalid, valid.data(), N, hipMemcpyHostToDevice)); HIP(hipMemcpy(dflow, flow.data(), 8 * N, hipMemcpyHostToDevice));
        for (int t = 0; t < 2; t++)                               // the push count of the class's session
            if (rcflow_infill_push_dev(ctx, 0, dflow, 8 * W, dvalid, W, nullptr, 0, dfilled, 8 * W, dsource, W, nullptr, 0, nullptr, 0, nullptr, nullptr,
                                       nullptr) != RC_OK)
                FAIL("push: %s", rcflow_last_error());
        long long sb[RC_INFILL_SUMMARY];
        std::vector<long long> sums_b(sums_a.size());
        std::vector<rc_infill_cell> cells_b(cells_a.size());
        if (rcflow_infill_read(ctx, 0, cells_b.data(), sums_b.data(), sb) != RC_OK) FAIL("read: %s", rcflow_last_error());
        std::vector<unsigned char> source_b(N);
        std::vector<float> filled_b(2 * N);
        HIP(hipMemcpy(source_b.data(), dsource, N, hipMemcpyDeviceToHost)); HIP(hipMemcpy(filled_b.data(), dfilled, 8 * N, hipMemcpyDeviceToHost));
        for (int k = 0; k < RC_INFILL_SUMMARY; k++)
            if (sb[k] != sa[k]) FAIL("summary word %d: the class %lld, the entry points %lld", k, sa[k], sb[k]);
        if (sums_b != sums_a || std::memcmp(cells_b.data(), cells_a.data(), cells_a.size() * sizeof(rc_infill_cell))) FAIL("sums or records differ");
        if (source_b != source || std::memcmp(filled_b.data(), filled.data(), 8 * N)) FAIL("source or filled field differ");
        if (rcflow_infill_close(ctx, 0) != RC_OK) FAIL("close");
        (void)hipFree(dvalid); (void)hipFree(dsource); (void)hipFree(dflow); (void)hipFree(dfilled);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_infill: ok\n");
    return 0;
}
