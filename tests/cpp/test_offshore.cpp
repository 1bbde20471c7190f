// rc::Offshore (include/rcflow_module.hpp) against the C ABI it wraps and against the figures of the prototype the product was
// specified with (tests/test_offshore_ref.py holds the numpy statement to the same figures): 96 x 64 pixels, wet where
// y >= rint(20 + 4 sin(2 pi x / 48)), the flow (1, -0.25) with (1, 2) in columns 48..59 and one vector that is not a number;
// min_dist 3, max_dist 40, 8 stations by x, 8 bins of 5 pixels, min_count 8, cross_min 1.
//   test_offshore
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)
#define HIP(call) do { if ((call) != hipSuccess) FAIL("%s failed", #call); } while (0)

static const int W = 96, H = 64;
static const long long MAP_SUMMARY[RC_OFFSHORE_SUMMARY] = {4224, 1920, 4224, 2074, 2517482, 245999, 0, 1};
static const long long PUSH_SUMMARY[RC_OFFSHORE_SUMMARY] = {3745, 253, 225, 1920, 1, 458, 1, 1};
static const long long SUM_NEAR = 12299798, SUM_R = 6927040, SUM_CROSS = 15240, SUM_ALONG = -241909, BEYOND = 16, BAND_10_25 = 1507;
static const long long COUNTS4[8] = {24, 65, 62, 62, 60, 61, 61, 60};
static const long long MEANS4[8] = {108, 108, 112, 113, 116, 117, 119, 120};

static long long rdiv(long long a, long long b) {
    const long long n = 2 * a + b, d = 2 * b, q = n / d;
    return q - (n % d != 0 && n < 0);
}

int main() {
    try {
        rc::Pipeline pipe(W, H);
        rc_offshore_params p;
        std::memset(&p, 0, sizeof(p));
        p.min_dist = 3; p.max_dist = 40; p.stations = 8; p.bins = 8; p.bin_width = 5; p.min_count = 8; p.rip_bins = 3; p.cross_min = 1.0f;
        p.flags = RC_OFFSHORE_STATION_X;
        const size_t N = (size_t)W * H;
        const double pi = 3.14159265358979323846;
        std::vector<unsigned char> wet(N);
        std::vector<float> flow(2 * N);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                wet[i] = y >= (int)std::rint(20.0 + 4.0 * std::sin(2.0 * pi * x / 48.0)) ? 255 : 0;
                const bool jet = x >= 48 && x < 60;
                flow[2 * i] = 1.0f;
                flow[2 * i + 1] = jet ? 2.0f : -0.25f;
            }
        flow[2 * ((size_t)30 * W + 10)] = std::numeric_limits<float>::quiet_NaN();
        std::vector<int> dist2(N), near(N), sdist(N);
        std::vector<float> ca(2 * N);
        std::vector<unsigned char> cls(N), mask(N), pic(3 * N), band(N);
        std::vector<long long> sa, table_a;
        std::vector<rc_offshore_station> st_a;
        {
            rc::Offshore off(pipe, p);
            rc::Mat mwet(H, W, 1, 1, wet.data()), mflow(H, W, 2, 4, flow.data());
            rc::Mat mdist2(H, W, 1, 4, dist2.data()), mnear(H, W, 1, 4, near.data()), msdist(H, W, 1, 4, sdist.data());
            rc::Mat mca(H, W, 2, 4, ca.data()), mcls(H, W, 1, 1, cls.data()), mmask(H, W, 1, 1, mask.data()), mpic(H, W, 3, 1, pic.data());
            rc::Mat mband(H, W, 1, 1, band.data());
            if (off.info().launches_per_map != RC_OFFSHORE_MAP_LAUNCHES || off.info().launches_per_push != RC_OFFSHORE_PUSH_LAUNCHES || off.info().have_map)
                FAIL("info");
            bool threw = false;
            try { off.push(mflow); } catch (const rc::Error& e) { threw = e.code == RC_ESTATE; }
            if (!threw) FAIL("a push before any map was accepted");
            rc::Offshore::MapPictures mp;
            mp.dist2 = &mdist2; mp.near = &mnear; mp.sdist = &msdist;
            off.map(mwet, mp);
            const std::vector<long long> ms = off.map_summary();
            for (int k = 0; k < RC_OFFSHORE_SUMMARY; k++)
                if (ms[k] != MAP_SUMMARY[k]) FAIL("map summary word %d: %lld, the statement %lld", k, ms[k], MAP_SUMMARY[k]);
            long long sum_near = 0, sum_r = 0;
            for (size_t i = 0; i < N; i++) {
                sum_near += near[i]; sum_r += std::abs(sdist[i]);
                if ((dist2[i] > 0) != (wet[i] != 0) || (sdist[i] > 0) != (wet[i] != 0)) FAIL("the sign at %zu", i);
                const int ny = (int)(i / W) - near[i] / W, nx = (int)(i % W) - near[i] % W;
                if (nx * nx + ny * ny != std::abs(dist2[i]) || (wet[near[i]] != 0) == (wet[i] != 0)) FAIL("near of %zu", i);
            }
            if (sum_near != SUM_NEAR || sum_r != SUM_R) FAIL("sum of near %lld, of r %lld", sum_near, sum_r);
            rc::Offshore::PushPictures pp;
            pp.cross_along = &mca; pp.cls = &mcls; pp.mask = &mmask; pp.picture = &mpic;
            off.push(mflow, pp);
            sa = off.read(); st_a = off.stations(); table_a = off.table();
            for (int k = 0; k < RC_OFFSHORE_SUMMARY; k++)
                if (sa[k] != PUSH_SUMMARY[k]) FAIL("push summary word %d: %lld, the statement %lld", k, sa[k], PUSH_SUMMARY[k]);
            long long sc = 0, sl = 0, nmask = 0, beyond = 0, biggest = 0;
            for (size_t i = 0; i < N; i++) {
                if (cls[i] != RC_OFFSHORE_C_OK) {
                    if (!std::isnan(ca[2 * i]) || !std::isnan(ca[2 * i + 1]) || mask[i]) FAIL("pixel %zu takes no part but has a value", i);
                    continue;
                }
                const float c = ca[2 * i] * 64.f, a = ca[2 * i + 1] * 64.f;
                if (c != std::rint(c) || a != std::rint(a)) FAIL("pixel %zu is no 64th", i);
                sc += (long long)c; sl += (long long)a; nmask += mask[i] == 255;
                if ((mask[i] == 255) != (c >= 64.f)) FAIL("mask at %zu", i);
                biggest = std::max(biggest, std::max((long long)std::fabs(c), (long long)std::fabs(a)));
            }
            if (cls[(size_t)30 * W + 10] != RC_OFFSHORE_C_BAD || cls[0] != RC_OFFSHORE_C_DRY) FAIL("classes");
            if (sc != SUM_CROSS || sl != SUM_ALONG || nmask != PUSH_SUMMARY[5] || biggest != 128) FAIL("cross %lld, along %lld, mask %lld, largest %lld", sc, sl, nmask, biggest);
            if (st_a.size() != 8 || table_a.size() != 8 * 8 * RC_OFFSHORE_SUMS) FAIL("sizes");
            for (int s = 0; s < 8; s++) {
                beyond += st_a[s].beyond;
                if (st_a[s].reach_end != (s == 4 ? 8 : 0) || st_a[s].flags != (s == 4 ? RC_OFFSHORE_RIP : 0)) FAIL("station %d: reach_end %d flags %d", s, st_a[s].reach_end, st_a[s].flags);
            }
            if (beyond != BEYOND) FAIL("beyond %lld", beyond);
            for (int b = 0; b < 8; b++) {
                const long long* t = &table_a[(size_t)(4 * 8 + b) * RC_OFFSHORE_SUMS];
                if (t[0] != COUNTS4[b] || rdiv(t[1], t[0]) != MEANS4[b]) FAIL("station 4 bin %d: count %lld mean %lld", b, t[0], rdiv(t[1], t[0]));
            }
            if (st_a[4].first != 0 || st_a[4].peak_bin != 7 || st_a[4].peak_cross != 120 || st_a[4].count != 455) FAIL("station 4's record");
            off.band(10.f, 25.f, mband);
            long long nb = 0;
            for (size_t i = 0; i < N; i++) nb += band[i] == 255;
            if (nb != BAND_10_25) FAIL("band %lld", nb);
            threw = false;
            try { off.push(mmask); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw) FAIL("a grey picture was accepted as a field");
            threw = false;
            rc_offshore_params q = p;
            q.flags = RC_OFFSHORE_STATION_X | RC_OFFSHORE_STATION_Y;
            try { rc::Offshore two(pipe, q); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw || off.info().w != W || off.info().pushes != 1 || off.info().maps != 1) FAIL("both station rules were accepted");
        }
        // the same through the entry points themselves
        rc_ctx* ctx = pipe.context();
        if (rcflow_offshore_open(ctx, 0, W, H, &p) != RC_OK) FAIL("open: %s", rcflow_last_error());
        unsigned char* dwet = nullptr; float *dflow = nullptr, *dca = nullptr; int* dnear = nullptr;
        HIP(hipMalloc((void**)&dwet, N)); HIP(hipMalloc((void**)&dflow, 8 * N)); HIP(hipMalloc((void**)&dca, 8 * N)); HIP(hipMalloc((void**)&dnear, 4 * N));
        HIP(hipMemcpy(dwet, wet.data(), N, hipMemcpyHostToDevice)); HIP(hipMemcpy(dflow, flow.data(), 8 * N, hipMemcpyHostToDevice));
        if (rcflow_offshore_map_dev(ctx, 0, dwet, W, nullptr, 0, dnear, 4 * W, nullptr, 0, nullptr, 0, nullptr) != RC_OK) FAIL("map: %s", rcflow_last_error());
        if (rcflow_offshore_push_dev(ctx, 0, dflow, 8 * W, dca, 8 * W, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) != RC_OK)
            FAIL("push: %s", rcflow_last_error());
        long long sb[RC_OFFSHORE_SUMMARY], mb[RC_OFFSHORE_SUMMARY];
        std::vector<long long> table_b(table_a.size());
        std::vector<rc_offshore_station> st_b(st_a.size());
        if (rcflow_offshore_read(ctx, 0, st_b.data(), table_b.data(), sb, mb) != RC_OK) FAIL("read: %s", rcflow_last_error());
        std::vector<int> near_b(N);
        std::vector<float> ca_b(2 * N);
        HIP(hipMemcpy(near_b.data(), dnear, 4 * N, hipMemcpyDeviceToHost)); HIP(hipMemcpy(ca_b.data(), dca, 8 * N, hipMemcpyDeviceToHost));
        for (int k = 0; k < RC_OFFSHORE_SUMMARY; k++)
            if (sb[k] != sa[k] || mb[k] != MAP_SUMMARY[k]) FAIL("summary word %d: the class %lld, the entry points %lld (map %lld)", k, sa[k], sb[k], mb[k]);
        if (table_b != table_a || std::memcmp(st_b.data(), st_a.data(), st_a.size() * sizeof(rc_offshore_station))) FAIL("table or records differ");
        if (near_b != near || std::memcmp(ca_b.data(), ca.data(), 8 * N)) FAIL("near or the cross / along field differ");
        if (rcflow_offshore_close(ctx, 0) != RC_OK) FAIL("close");
        (void)hipFree(dwet); (void)hipFree(dflow); (void)hipFree(dca); (void)hipFree(dnear);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_offshore: ok\n");
    return 0;
}
