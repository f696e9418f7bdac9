// Stand-alone host check of the box overlaps of the KITTI evaluation: csrc/pcr_kitti_eval_dev.h is the one source of the overlap kernel
// and of pcr_kitti_box_overlap, and plain C++, so this program exercises the clip without a GPU and without the HIP runtime.  Build it
// with a sanitizer and run it:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I point-cloud-process_amd/csrc scripts/kitti_overlap_host_check.cpp -o kitti_overlap_host_check && ./kitti_overlap_host_check
// It feeds the pairs whose answer is known in closed form (tests/kitti_eval_checks.py: special_pairs) and 20 000 generated pairs, and
// checks what must hold for any pair: 0 <= overlap <= 1 (+ rounding), the union overlap symmetric in its arguments, ry and ry + pi alike,
// a rectangle against itself 1.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "pcr_kitti_eval_dev.h"

static int failures = 0;

static void expect(bool ok, const char* what, double got, double want) {
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAILED %s: got %.17g, want %.17g\n", what, got, want);
}

static ke_box make(double cx, double cz, double l, double w, double ry, double h, double cy, double left, double top, double right, double bottom) {
    const double row[16] = {0, 0, 0, -10, left, top, right, bottom, h, w, l, cx, cy, cz, ry, 0};
    return ke_box_from_row(row, std::cos(ry), std::sin(ry));
}

static void exact(const char* name, const ke_box& a, const ke_box& b, int criterion, double image, double ground, double volume) {
    double o[3];
    ke_overlaps(a, b, criterion, o);
    expect(o[0] == image, name, o[0], image);
    expect(o[1] == ground, name, o[1], ground);
    expect(o[2] == volume, name, o[2], volume);
}

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uniform(double lo, double hi) {   // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return lo + (hi - lo) * ((double)(z >> 11) * (1.0 / 9007199254740992.0));
}

int main() {
    const ke_box a = make(0, 0, 4, 2, 0, 2, 1, 0, 0, 8, 4);
    exact("identical", a, a, -1, 1.0, 1.0, 1.0);
    exact("shifted, union", a, make(1, 0.5, 4, 2, 0, 2, 2, 2, 1, 10, 5), -1, 18.0 / 46.0, 4.5 / 11.5, 4.5 / 27.5);
    exact("shifted, first", a, make(1, 0.5, 4, 2, 0, 2, 2, 2, 1, 10, 5), 0, 18.0 / 32.0, 4.5 / 8.0, 4.5 / 16.0);
    exact("shared edge", a, make(4, 0, 4, 2, 0, 2, 1, 8, 0, 16, 4), -1, 0.0, 0.0, 0.0);
    exact("shared corner", a, make(4, 2, 4, 2, 0, 2, 1, 8, 4, 16, 8), -1, 0.0, 0.0, 0.0);
    exact("inside, union", a, make(0.5, 0.25, 2, 1, 0, 1, 0.5, 2, 1, 6, 3), -1, 0.25, 0.25, 0.125);
    exact("inside, second", a, make(0.5, 0.25, 2, 1, 0, 1, 0.5, 2, 1, 6, 3), 1, 1.0, 1.0, 1.0);
    exact("heights touch", a, make(0, 0, 4, 2, 0, 2, 3, 0, 0, 8, 4), -1, 1.0, 1.0, 0.0);
    exact("zero width", a, make(0, 0, 4, 0, 0, 2, 1, 0, 0, 8, 4), -1, 1.0, 0.0, 0.0);
    exact("negative length", a, make(0, 0, -4, 2, 0, 2, 1, 0, 0, 8, 0), -1, 0.0, 0.0, 0.0);
    exact("dontcare", a, make(-1000, -1000, -1, -1, -10, -1, -1000, 0, 0, 16, 4), 0, 1.0, 0.0, 0.0);
    exact("not finite", a, make(NAN, 0, 4, 2, 0, 2, 1, 0, 0, INFINITY, 4), -1, 0.0, 0.0, 0.0);
    {
        double o[3];
        const double area = 2.0 * (std::sqrt(2.0) - 1.0);
        ke_overlaps(make(3, 7, 1, 1, 0, 1, 0, 0, 0, 1, 1), make(3, 7, 1, 1, std::atan(1.0), 1, 0, 0, 0, 1, 1), 0, o);
        expect(std::fabs(o[1] - area) < 1e-14, "octagon", o[1], area);
    }
    const double slack = 1e-12;
    long long overlapping = 0;
    for (int i = 0; i < 20000; ++i) {
        const bool near = i % 4 != 0;
        const double cx = uniform(-40, 40), cz = uniform(0, 80);
        const ke_box p = make(cx, cz, uniform(0.3, 9), uniform(0.3, 3), uniform(-7, 7), uniform(0.5, 3), uniform(0, 3), uniform(0, 600), uniform(0, 200),
                              uniform(600, 1200), uniform(200, 370));
        ke_box q = make(near ? cx + uniform(-3, 3) : uniform(-40, 40), near ? cz + uniform(-3, 3) : uniform(0, 80), uniform(0.3, 9), uniform(0.3, 3), uniform(-7, 7),
                        uniform(0.5, 3), uniform(0, 3), uniform(0, 900), uniform(0, 300), uniform(300, 1200), uniform(100, 370));
        if (i % 97 == 0) q.w = 0.0;
        if (i % 101 == 0) q.cx = NAN;
        double u[3], v[3], f[3], s[3], self[3];
        ke_overlaps(p, q, -1, u);
        ke_overlaps(q, p, -1, v);
        ke_overlaps(p, q, 0, f);
        ke_overlaps(p, q, 1, s);
        ke_overlaps(p, p, -1, self);
        overlapping += u[1] > 0.0;
        for (int m = 0; m < 3; ++m) {
            expect(u[m] >= 0.0 && u[m] <= 1.0 + slack, "union in [0, 1]", u[m], 1.0);
            expect(f[m] >= 0.0 && f[m] <= 1.0 + slack && s[m] >= 0.0 && s[m] <= 1.0 + slack, "criteria 0, 1 in [0, 1]", f[m], s[m]);
            expect(std::fabs(u[m] - v[m]) < slack, "union symmetric", u[m], v[m]);
            expect(u[m] <= f[m] + slack && u[m] <= s[m] + slack, "union <= either", u[m], f[m]);
            expect(std::fabs(self[m] - 1.0) < slack, "a box against itself", self[m], 1.0);
        }
        ke_box r = q;
        r.cs = -q.cs;
        r.sn = -q.sn;   // ry + pi
        double w[3];
        ke_overlaps(p, r, -1, w);
        expect(std::fabs(u[1] - w[1]) < slack, "ry + pi", w[1], u[1]);
    }
    if (overlapping < 5000) { ++failures; std::fprintf(stderr, "FAILED: only %lld generated pairs overlap\n", overlapping); }
    if (failures) return 1;
    std::printf("ok: %lld of 20000 generated pairs overlap on the ground\n", overlapping);
    return 0;
}
