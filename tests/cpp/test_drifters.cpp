// rc::Drifters (include/rcflow_module.hpp) against the C ABI it wraps, on one case of 60 x 40 pixels: a field of columns that flow up
// the picture at 1.5 pixels a push in columns 20..39 and down it at 1 pixel elsewhere, with no lateral motion; rows 0..3 are zone
// OFFSHORE and rows 36..39 zone SHORE; a 28 x 6 lattice of homes on whole pixels.  Exactly the drifters homed in columns 20..39 end
// OFFSHORE, every other one SHORE, and what the census must then say is computed here.  The class and the entry points called
// directly give the same tables, records, histograms, summary and pictures.
//   test_drifters
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)
#define HIP(call) do { if ((call) != hipSuccess) FAIL("%s failed", #call); } while (0)

static const int W = 60, H = 40, A = 20, B = 40, PUSHES = 40;

int main() {
    try {
        rc::Pipeline pipe(W, H);
        rc_drifters_params p;
        std::memset(&p, 0, sizeof(p));
        p.max_drifters = 256; p.grid_x = 3; p.grid_y = 2; p.max_age = 0; p.age_bin = 4; p.density_full = 8; p.live_min = 1; p.flags = 0; p.dt = 1.0;
        const size_t N = (size_t)W * H;
        std::vector<float> flow(2 * N);
        std::vector<unsigned char> zone(N, 0);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                flow[2 * ((size_t)y * W + x)] = 0.f;
                flow[2 * ((size_t)y * W + x) + 1] = x >= A && x < B ? -1.5f : 1.f;
                zone[(size_t)y * W + x] = y < 4 ? 2 : y >= H - 4 ? 1 : 0;
            }
        std::vector<double> homes;
        long long n_out = 0;
        for (int j = 0; j < 6; j++)
            for (int i = 0; i < 28; i++) {
                homes.push_back(2.0 + 2.0 * i); homes.push_back(8.0 + 4.0 * j);
                n_out += 2 + 2 * i >= A && 2 + 2 * i < B;
            }
        const long long n = (long long)homes.size() / 2;
        std::vector<unsigned short> now(N);
        std::vector<unsigned> dens(N);
        std::vector<unsigned char> live(N), pic(3 * N);
        std::vector<long long> sa, place_a, origin_a;
        std::vector<unsigned long long> hist_a;
        std::vector<rc_drifters_cell> cells_a;
        {
            rc::Drifters dr(pipe, p);
            rc::Mat mflow(H, W, 2, 4, flow.data()), mzone(H, W, 1, 1, zone.data());
            rc::Mat mnow(H, W, 1, 2, now.data()), mdens(H, W, 1, 4, dens.data()), mlive(H, W, 1, 1, live.data()), mpic(H, W, 3, 1, pic.data());
            rc::Drifters::Pictures all;
            all.now = &mnow; all.density = &mdens; all.live = &mlive; all.picture = &mpic;
            bool threw = false;
            try { dr.push(mflow, &mzone); } catch (const rc::Error& e) { threw = e.code == RC_ESTATE; }
            if (!threw) FAIL("a push with no drifter seeded was accepted");
            dr.seed(homes);
            if (dr.info().drifters != n) FAIL("seeded %d", dr.info().drifters);
            dr.push(mflow, &mzone, all);                          // the release: everyone at home
            long long occ = 0;
            for (size_t i = 0; i < N; i++) {
                occ += now[i];
                if (dens[i] != now[i] || (live[i] == 255) != (now[i] > 0) || (now[i] == 0 && (pic[3 * i] | pic[3 * i + 1] | pic[3 * i + 2]))) FAIL("pixel %zu after the release", i);
            }
            if (occ != n || now[(size_t)8 * W + 2] != 1 || dr.read()[1] != n || dr.read()[2] != n) FAIL("the release: %lld on the picture", occ);
            for (int t = 1; t < PUSHES; t++) dr.push(mflow, &mzone, t == PUSHES - 1 ? all : rc::Drifters::Pictures());
            sa = dr.read(); cells_a = dr.cells(); place_a = dr.place(); origin_a = dr.origin(); hist_a = dr.hist();
            if (sa[0] != n || sa[1] != 0 || sa[2] != n || sa[3] != PUSHES || sa[8 + RC_DRIFTERS_OFFSHORE] != n_out || sa[8 + RC_DRIFTERS_SHORE] != n - n_out)
                FAIL("summary: %lld drifters, %lld alive, %lld released, %lld pushes, %lld offshore, %lld shore", sa[0], sa[1], sa[2], sa[3],
                     sa[8 + RC_DRIFTERS_OFFSHORE], sa[8 + RC_DRIFTERS_SHORE]);
            // columns 20..39 are origin cells 1 and 4 (cells of 20 x 20 pixels), and nobody else's
            long long visits = 0, released = 0, hs = 0, dsum = 0;
            for (size_t k = 0; k < cells_a.size(); k++) {
                const bool jet = k % 3 == 1;
                if (cells_a[k].escape != (jet ? 1.f : 0.f) || cells_a[k].beached != (jet ? 0.f : 1.f) || cells_a[k].flags) FAIL("cell %zu: escape %g", k, cells_a[k].escape);
                if (jet && cells_a[k].mean_exit_age != (float)((double)origin_a[8 * k + 6] / (double)origin_a[8 * k + 2])) FAIL("cell %zu: exit age", k);
                if (place_a[8 * k] && cells_a[k].mean_v != (float)(((double)place_a[8 * k + 2] / 64.0) / (double)place_a[8 * k])) FAIL("cell %zu: mean_v", k);
                if (cells_a[k].mean_u != 0.f) FAIL("cell %zu: mean_u", k);
                visits += place_a[8 * k]; released += origin_a[8 * k];
            }
            for (size_t i = 0; i < hist_a.size(); i++) hs += (long long)hist_a[i];
            for (size_t i = 0; i < N; i++) dsum += dens[i];
            if (cells_a.size() != 6 || released != n || hs != n || visits != dsum || visits == 0) FAIL("census: %lld released, %lld in the histograms, %lld visits, density %lld", released, hs, visits, dsum);
            // the first to leave: home row 8 at 1.5 a push is in rows 0..3 (y < 3.5) after 4 moves, age 4, bin 1 of class OFFSHORE
            if (hist_a[RC_DRIFTERS_HIST_BINS + 1] == 0 || hist_a[RC_DRIFTERS_HIST_BINS] != 0) FAIL("the first exits: bins %llu %llu", hist_a[32], hist_a[33]);
            dr.set(1.0, 0, 8, 1, RC_DRIFTERS_RESPAWN);            // from the next push on: everyone is released again
            dr.push(mflow, &mzone);
            if (dr.read()[1] != n || dr.read()[2] != 2 * n) FAIL("after set: %lld alive, %lld released", dr.read()[1], dr.read()[2]);
            dr.reset();
            if (dr.info().pushes != 0 || dr.info().drifters != n || dr.read()[2] != 0 || dr.info().prm.flags != RC_DRIFTERS_RESPAWN) FAIL("reset");
            threw = false;
            try { dr.push(mzone); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw) FAIL("a grey picture was accepted as a field");
            threw = false;
            try { dr.seed({1.0, 2.0, (double)W, 3.0}); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw || dr.info().drifters != n) FAIL("a home outside the picture was accepted");
            threw = false;
            rc_drifters_params q = p;
            q.age_bin = 0;
            try { rc::Drifters two(pipe, q); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
            if (!threw || dr.info().w != W) FAIL("age_bin 0 was accepted");
        }
        // the same session through the entry points themselves
        rc_ctx* ctx = pipe.context();
        if (rcflow_drifters_open(ctx, 0, W, H, &p) != RC_OK) FAIL("open: %s", rcflow_last_error());
        if (rcflow_drifters_seed(ctx, 0, homes.data(), (int)n) != RC_OK) FAIL("seed: %s", rcflow_last_error());
        float* dflow = nullptr;
        unsigned char *dzone = nullptr, *dlive = nullptr;
        unsigned* ddens = nullptr;
        HIP(hipMalloc((void**)&dflow, 8 * N)); HIP(hipMalloc((void**)&dzone, N)); HIP(hipMalloc((void**)&dlive, N)); HIP(hipMalloc((void**)&ddens, 4 * N));
        HIP(hipMemcpy(dflow, flow.data(), 8 * N, hipMemcpyHostToDevice)); HIP(hipMemcpy(dzone, zone.data(), N, hipMemcpyHostToDevice));
        for (int t = 0; t < PUSHES; t++)
            if (rcflow_drifters_push_dev(ctx, 0, dflow, 8 * W, dzone, W, nullptr, 0, ddens, 4 * W, dlive, W, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr) != RC_OK)
                FAIL("push: %s", rcflow_last_error());
        long long sb[RC_DRIFTERS_SUMMARY];
        std::vector<long long> place_b(place_a.size()), origin_b(origin_a.size());
        std::vector<unsigned long long> hist_b(hist_a.size());
        std::vector<rc_drifters_cell> cells_b(cells_a.size());
        if (rcflow_drifters_read(ctx, 0, cells_b.data(), place_b.data(), origin_b.data(), hist_b.data(), sb) != RC_OK) FAIL("read: %s", rcflow_last_error());
        std::vector<unsigned> dens_b(N);
        std::vector<unsigned char> live_b(N);
        HIP(hipMemcpy(dens_b.data(), ddens, 4 * N, hipMemcpyDeviceToHost)); HIP(hipMemcpy(live_b.data(), dlive, N, hipMemcpyDeviceToHost));
        for (int k = 0; k < RC_DRIFTERS_SUMMARY; k++)
            if (sb[k] != sa[k]) FAIL("summary word %d: the class %lld, the entry points %lld", k, sa[k], sb[k]);
        if (place_b != place_a || origin_b != origin_a || hist_b != hist_a || std::memcmp(cells_b.data(), cells_a.data(), cells_a.size() * sizeof(rc_drifters_cell)))
            FAIL("tables, histograms or records differ");
        if (dens_b != dens || live_b != live) FAIL("density or live mask differ");
        if (rcflow_drifters_close(ctx, 0) != RC_OK) FAIL("close");
        (void)hipFree(dflow); (void)hipFree(dzone); (void)hipFree(dlive); (void)hipFree(ddens);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_drifters: ok\n");
    return 0;
}
