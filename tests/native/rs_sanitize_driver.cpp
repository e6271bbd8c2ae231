// rs_sanitize_driver.cpp -- csrc/fcpp_rsfn.h (the function behind fcpp_debug_rs and the Reeds-Shepp kernels) under ASan + UBSan on the
// CPU: random, degenerate and hostile pairs through rs_solve, rs_runs, rs_pose_in_run and rs_pose_at.  Any sanitizer report aborts; the
// driver itself checks that every finite pair closes on its goal.  usage: rs_sanitize_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_rsfn.h"

using namespace fcpp;

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? strtol(argv[2], nullptr, 10) : 100000;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> pos(0.0, 5000.0), ang(-3.14159265358979, 3.14159265358979), unit(0.0, 1.0);
    const double radii[3] = { 2.0, 8.0, 25.0 };
    const double hostile[] = { 0.0, -0.0, 1e-300, -1e-300, 1e300, -1e300, INFINITY, -INFINITY, NAN, 1e5, -1e5, 4.9e-324 };
    const int n_hostile = (int)(sizeof hostile / sizeof hostile[0]);
    long solved = 0, nan_pairs = 0, samples = 0, cusps = 0;
    double worst = 0.0;
    for (long i = 0; i < n; ++i) {
        const double R = radii[i % 3];
        double p[6] = { pos(rng), pos(rng), ang(rng), 0.0, 0.0, ang(rng) };
        const double reach = (i & 1) ? 4.0 * R * unit(rng) : 5000.0 * unit(rng), dir = ang(rng);
        p[3] = p[0] + reach * cos(dir); p[4] = p[1] + reach * sin(dir);
        if (i % 7 == 0) for (int k = 0; k < 6; ++k) if (unit(rng) < 0.3) p[k] = hostile[rng() % n_hostile];
        if (i % 11 == 0) { p[3] = p[0]; p[4] = p[1]; p[5] = p[2]; }
        int w;
        double s[5], tot;
        rs_solve(p[0], p[1], p[2], p[3], p[4], p[5], R, w, s, tot);
        if (w < 0) { ++nan_pairs; if (tot == tot) { printf("word -1 with a total\n"); return 1; } }
        else {
            ++solved;
            if (w >= RS_WORDS || tot != (((fabs(s[0]) + fabs(s[1])) + fabs(s[2])) + fabs(s[3])) + fabs(s[4])) { printf("bad result at %ld\n", i); return 1; }
            for (int k = 0; k < 5; ++k)
                if (s[k] != 0.0 && (s[k] > 0.0 ? 1 : -1) != rs_gear(w, k)) { printf("gear of segment %d of word %d at %ld\n", k, w, i); return 1; }
            // the runs, and the pose at a few places of each, their ends and beyond them
            const RsRuns runs = rs_runs(w, s);
            if (runs.n < 1 || runs.n > 3) { printf("runs at %ld\n", i); return 1; }
            cusps += runs.n - 1;
            double x = 0, y = 0, h = 0, k = 0;
            int g = 0;
            for (int r = 0; r < runs.n; ++r) {
                const double at[] = { 0.0, runs.len[r] * unit(rng), runs.len[r], runs.len[r] + 1.0, -1.0, NAN, INFINITY };
                for (double e : at) { rs_pose_in_run(p[0], p[1], p[2], R, w, s, runs, r, e, x, y, h, k, g); ++samples; }
            }
            rs_pose_in_run(p[0], p[1], p[2], R, w, s, runs, runs.n - 1, runs.len[runs.n - 1], x, y, h, k, g);
            if (fabs(p[0]) <= 5000.0 && fabs(p[3]) <= 1e4 && fabs(p[1]) <= 5000.0 && fabs(p[4]) <= 1e4 && fabs(p[2]) <= 4.0 && fabs(p[5]) <= 4.0) {
                const double e = fmax(fabs(x - p[3]), fabs(y - p[4]));
                if (e > worst) worst = e;
            }
        }
        // words / segments / positions the solver never returns
        double hs[5], x, y, h, k;
        int g;
        for (int j = 0; j < 5; ++j) hs[j] = unit(rng) < 0.5 ? hostile[rng() % n_hostile] : (unit(rng) - 0.5) * 50.0;
        const int hw = (int)(rng() % 60) - 6;
        rs_pose_at(p[0], p[1], p[2], R, hw, hs, (int)(rng() % 9) - 2, hostile[rng() % n_hostile], x, y, h, k, g);
        const RsRuns hr = rs_runs(hw, hs);
        if (hw >= 0 && hw < RS_WORDS)
            for (int r = 0; r < hr.n; ++r) rs_pose_in_run(p[0], p[1], p[2], R, hw, hs, hr, r, unit(rng) * 100.0, x, y, h, k, g);
        (void)rs_turn(hw, (int)(rng() % 9) - 2);
        (void)rs_gear(hw, (int)(rng() % 9) - 2);
    }
    if (!(worst <= 1e-9)) { printf("closure %g\n", worst); return 1; }
    printf("solved %ld nan %ld samples %ld cusps %ld closure %.3g\n", solved, nan_pairs, samples, cusps, worst);
    return 0;
}
