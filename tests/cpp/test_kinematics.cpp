// rc::Kinematics (include/rcflow_module.hpp) on the analytic rotation field of 64 x 48 pixels, u = -(y - h/2) / h * 100,
// v = (x - w/2) / w * 100: the field is linear, so the smoothing changes nothing, omega = 100 / w + 100 / h and
// ow = -4 (100 / w)(100 / h) at every valid pixel (within a few ulp of values up to 50, divided by 2 s), the divergence is 0, every
// valid pixel turns clockwise and is a core.  The numbers are computed here.
//   test_kinematics
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rcflow_module.hpp"

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

int main() {
    const int w = 64, h = 48, R = 3, s = 2, m = R + s, gx = 2, gy = 2;
    const double om = 100.0 / w + 100.0 / h, okw = -4.0 * (100.0 / w) * (100.0 / h);
    try {
        rc::Pipeline pipe(w, h);
        rc_kinematics_params p;
        std::memset(&p, 0, sizeof(p));
        p.radius = R; p.sigma = 2.0; p.spacing = s; p.grid_x = gx; p.grid_y = gy; p.min_core = 1; p.flags = RC_KINEMATICS_RELATIVE;
        p.scale = 1.0; p.pixel_area = 0.25; p.ow_k = 0.2; p.vis_max = 4.0;
        rc::Kinematics kn(pipe, p);
        const std::vector<float> g = rc::Kinematics::taps(R, 2.0);
        double z = g[0];
        for (int k = 1; k <= R; k++) z += 2.0 * g[k];
        if (g.size() != (size_t)R + 1 || std::fabs(z - 1.0) > 1e-6) FAIL("the taps do not sum to one: %.9g", z);
        std::vector<float> f((size_t)w * h * 2), o((size_t)w * h), d((size_t)w * h), k((size_t)w * h);
        std::vector<unsigned char> mk((size_t)w * h), pic((size_t)w * h * 3);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                f[2 * ((size_t)y * w + x)] = (float)(-(y - h / 2.0) / h * 100);
                f[2 * ((size_t)y * w + x) + 1] = (float)((x - w / 2.0) / w * 100);
            }
        rc::Mat flow(h, w, 2, 4, f.data()), omega(h, w, 1, 4, o.data()), div(h, w, 1, 4, d.data()), ow(h, w, 1, 4, k.data());
        rc::Mat mask(h, w, 1, 1, mk.data()), picture(h, w, 3, 1, pic.data());
        kn.push(flow, &omega, &div, &ow, &mask, &picture);
        const long long interior = (long long)(w - 2 * m) * (h - 2 * m);
        long long seen = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const bool in = x >= m && x < w - m && y >= m && y < h - m;
                const bool lit = (pic[3 * i] | pic[3 * i + 1] | pic[3 * i + 2]) != 0;
                if (in) {
                    if (std::fabs(o[i] - om) > 2e-5 || std::fabs(k[i] - okw) > 2e-4 || std::fabs(d[i]) > 1e-5 || mk[i] != 255 || !lit)
                        FAIL("pixel (%d, %d): omega %.9g, ow %.9g, div %.9g, mask %d", x, y, o[i], k[i], d[i], mk[i]);
                    seen++;
                } else if (o[i] != 0.f || k[i] != 0.f || d[i] != 0.f || mk[i] != 0 || lit) {
                    FAIL("pixel (%d, %d) outside the interior is not zero", x, y);
                }
            }
        std::vector<long long> sm = kn.read();
        // T2 is ow_k^2 times the variance of a constant: the fixed point of 2^-16 on ow and ow^2, with means of 13 and 174, leaves
        // at most 0.04 * 2.1e-4
        double t2;
        std::memcpy(&t2, &sm[4], 8);
        if (sm[0] != interior || seen != interior || sm[1] != 0 || sm[2] != interior || sm[3] != 0 || sm[5] != 0 || sm[6] != 1 || !(t2 >= 0. && t2 < 1e-4))
            FAIL("summary %lld %lld %lld %lld (T2 %.9g) %lld %lld", sm[0], sm[1], sm[2], sm[3], t2, sm[5], sm[6]);
        float mx;
        const unsigned mb = (unsigned)sm[7];
        std::memcpy(&mx, &mb, 4);
        if (std::fabs(mx - om) > 2e-5) FAIL("the largest |omega| is %.9g", mx);
        const std::vector<rc_kinematics_cell> c = kn.cells();
        const std::vector<long long> q = kn.sums();
        long long n = 0;
        for (int i = 0; i < gx * gy; i++) {
            if (c[i].flags != RC_KINEMATICS_CW || c[i].n != q[(size_t)RC_KINEMATICS_SUMS * i] || c[i].bad != 0 || c[i].cores_cw != c[i].n || c[i].cores_ccw != 0)
                FAIL("cell %d: flags %d, n %d, cores %d / %d", i, c[i].flags, c[i].n, c[i].cores_cw, c[i].cores_ccw);
            if (std::fabs(c[i].mean_vorticity - om) > 2e-5 || std::fabs(c[i].mean_ow - okw) > 2e-4 || std::fabs(c[i].mean_divergence) > 1e-5 ||
                std::fabs(c[i].circulation - om * c[i].n * 0.25) > 1e-4 * om * c[i].n || c[i].circulation != c[i].circulation_cw || c[i].circulation_ccw != 0.f)
                FAIL("cell %d: vorticity %.9g, ow %.9g, circulation %.9g", i, c[i].mean_vorticity, c[i].mean_ow, c[i].circulation);
            n += c[i].n;
        }
        if (n != interior) FAIL("the cells hold %lld pixels of %lld", n, interior);
        // a push without outputs is only counted; the summary stays
        kn.push(flow);
        if (kn.read() != sm || kn.info().pushes != 2 || kn.info().margin != m) FAIL("a push without outputs changed the summary");
        // the summary alone; set acts from the next push: no pixel reaches an |omega| of 10
        kn.set(0.2, 0.0, 10.0, 4.0);
        kn.push(flow, nullptr, nullptr, nullptr, nullptr, nullptr, true);
        sm = kn.read();
        if (sm[0] != interior || sm[2] != 0 || sm[3] != 0 || sm[6] != 3) FAIL("after set: %lld %lld %lld %lld", sm[0], sm[2], sm[3], sm[6]);
        kn.reset();
        if (kn.info().pushes != 0 || kn.info().prm.omega_min != 10.0 || kn.read()[0] != 0) FAIL("reset");
        // wrong shapes are refused before anything is copied; a refused open throws and leaves the session working
        bool threw = false;
        rc::Mat small(h - 1, w, 1, 4, o.data());
        try { kn.push(flow, &small); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw) FAIL("an omega of another size was accepted");
        threw = false;
        p.radius = 9;
        try { rc::Kinematics bad(pipe, p); } catch (const rc::Error& e) { threw = e.code == RC_EINVAL; }
        if (!threw || kn.info().w != w) FAIL("radius 9 was accepted");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("test_kinematics: ok\n");
    return 0;
}
