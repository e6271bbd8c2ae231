// path_speeds_sanitize_driver.cpp -- csrc/fcpp_speedfn.h (the rule behind fcpp_debug_path_speeds and the path-speed kernels) under
// ASan + UBSan on the CPU: the parameter check, the sample check, the caps, the stops and the twin's order of work (speed_path_host: caps,
// forward sweep, backward sweep) over fixed shapes -- empty, one-sample and two-equal-sample paths, doubled junctions and cusps, zero
// steps in runs -- and random paths of random pieces, now and then with a sample that fails.  Any sanitizer report aborts; the driver
// itself checks every path against a brute-force O(n^2) minimum over all (j, i) pairs, summed in long double:
//     u_i = min over j of  c_j + 2 a_acc (d_(j+1) + .. + d_i)  (j <= i),   c_j + 2 a_dec (d_(i+1) + .. + d_j)  (j >= i)
// to (n + 4) 2^-52 on v, stops exactly 0, v <= cap, NaN over a failing path.  It prints how often every kind of result occurred.
// usage: path_speeds_sanitize_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_speedfn.h"

using namespace fcpp;

struct Path {
    std::vector<double> x, y, kappa;
    std::vector<int8_t> part, gear;
    double px = 0.0, py = 0.0, h = 0.3;
    // n samples at `step` along the heading, the first ON the last sample so far (a doubled junction), the last step short
    void piece(int n, double step, double k, int p, int g)
    {
        for (int i = 0; i < n; ++i) {
            if (i > 0) {
                const double ds = (i == n - 1 ? 0.37 : 1.0) * step * g;
                px += ds * cos(h); py += ds * sin(h); h += k * ds;
            }
            x.push_back(px); y.push_back(py); kappa.push_back(k); part.push_back((int8_t)p); gear.push_back((int8_t)g);
        }
    }
};

static long n_paths = 0, n_samples = 0, n_failed = 0, n_stops = 0, n_at_cap = 0, n_zero_steps = 0;

static void die(const char *what, long path, long i)
{
    printf("FAILED %s path %ld sample %ld\n", what, path, i);
    exit(1);
}

static void check(const fcpp_speed_params &prm, const Path &P)
{
    SpeedRule r;
    if (!speed_rule(prm, r)) die("rule", n_paths, -1);
    const int64_t n = (int64_t)P.x.size();
    // exactly sized buffers: a store past the end is ASan's to find
    std::vector<double> u((size_t)n), v((size_t)n), cap((size_t)n);
    const int st = speed_path_host(r, n, P.x.data(), P.y.data(), P.kappa.data(), P.part.data(), P.gear.data(), u.data(), v.data(), cap.data());
    ++n_paths; n_samples += n;
    bool ok = true;
    for (int64_t i = 0; i < n; ++i) ok = ok && speed_sample_ok(P.x[i], P.y[i], P.kappa[i], P.part[i], P.gear[i]);
    if ((st == SPEED_OK) != ok) die("status", n_paths, -1);
    if (!ok) {
        ++n_failed;
        for (int64_t i = 0; i < n; ++i)
            if (!isnan(v[i]) || !isnan(cap[i])) die("nan", n_paths, i);
        return;
    }
    // with either output NULL the other is what it was
    std::vector<double> v2((size_t)n), cap2((size_t)n);
    speed_path_host(r, n, P.x.data(), P.y.data(), P.kappa.data(), P.part.data(), P.gear.data(), u.data(), v2.data(), nullptr);
    speed_path_host(r, n, P.x.data(), P.y.data(), P.kappa.data(), P.part.data(), P.gear.data(), u.data(), nullptr, cap2.data());
    std::vector<long double> c((size_t)n), S((size_t)n, 0.0L);
    for (int64_t i = 0; i < n; ++i) {
        const bool stop = speed_stop(r.flags, i, n, i > 0 ? P.gear[i - 1] : 0, P.gear[i], i < n - 1 ? P.gear[i + 1] : 0);
        c[i] = stop ? 0.0 : speed_cap_u(r, P.kappa[i], P.part[i], P.gear[i]);
        if (i > 0) {
            const double d = speed_step(P.x[i - 1], P.y[i - 1], P.x[i], P.y[i]);
            S[i] = S[i - 1] + (long double)d;
            n_zero_steps += d == 0.0;
        }
        n_stops += stop;
        if (v[i] != v2[i] || cap[i] != cap2[i]) die("null outputs", n_paths, i);
        if (cap[i] != speed_out((double)c[i])) die("cap", n_paths, i);
    }
    for (int64_t i = 0; i < n; ++i) {
        long double best = INFINITY;
        for (int64_t j = 0; j < n; ++j) {
            const long double cand = j <= i ? c[j] + (long double)r.two_acc * (S[i] - S[j]) : c[j] + (long double)r.two_dec * (S[j] - S[i]);
            if (cand < best) best = cand;
        }
        const double want = speed_out((double)best);
        if (!(v[i] <= cap[i])) die("above the cap", n_paths, i);
        if (best == 0.0L ? v[i] != 0.0 : !(fabs(v[i] - want) <= (double)(n + 4) * 0x1p-52 * want) && !(isinf(want) && v[i] == want))
            die("profile", n_paths, i);
        n_at_cap += v[i] == cap[i];
    }
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int N = argc > 2 ? atoi(argv[2]) : 100;
    fcpp_speed_params prm = {};
    const double nominal[8] = { 9.0, 15.0, 15.0, 15.0, 9.0, 15.0, 15.0, 15.0 };
    for (int k = 0; k < 8; ++k) prm.nominal_kmh[k] = nominal[k];
    prm.reverse_kmh = 2.5; prm.turn_kmh = 4.0; prm.a_lat = 2.0; prm.a_acc = 1.5; prm.a_dec = 1.5; prm.safety_factor = 0.85; prm.kappa_eps = 1e-6;
    prm.flags = FCPP_SPEED_REST_START | FCPP_SPEED_REST_END | FCPP_SPEED_STOP_AT_CUSPS;
    SpeedRule r;
    // the parameter check: every member out of range in turn
    {
        fcpp_speed_params b = prm; b.a_acc = 0.0; if (speed_rule(b, r)) die("a_acc", 0, 0);
        b = prm; b.a_dec = INFINITY; if (speed_rule(b, r)) die("a_dec", 0, 0);
        b = prm; b.reverse_kmh = NAN; if (speed_rule(b, r)) die("reverse", 0, 0);
        b = prm; b.nominal_kmh[7] = -1.0; if (speed_rule(b, r)) die("nominal", 0, 0);
        b = prm; b.flags = 8u; if (speed_rule(b, r)) die("flags", 0, 0);
        b = prm; b.turn_kmh = INFINITY; b.nominal_kmh[0] = INFINITY; b.nominal_kmh[1] = 0.0; if (!speed_rule(b, r)) die("inf allowed", 0, 0);
    }
    // the fixed shapes, under every flag word and asymmetric limits
    for (uint32_t flags = 0; flags < 8; ++flags) {
        fcpp_speed_params q = prm;
        q.flags = flags; q.a_acc = 0.3 + 0.1 * flags; q.a_dec = 0.9;
        Path e; check(q, e);
        Path one; one.piece(1, 0.1, 0.2, 4, 1); check(q, one);
        Path two; two.piece(1, 0.1, 0.0, 0, 1); two.piece(1, 0.1, 0.0, 0, -1); check(q, two);
        Path zeros; zeros.piece(5, 0.0, 0.0, 0, 1); zeros.piece(4, 0.1, 0.5, 1, -1); zeros.piece(3, 0.0, 0.0, 2, 1); check(q, zeros);
        Path sas; sas.piece(120, 0.1, 0.0, 0, 1); sas.piece(40, 0.1, 1.0 / 6.0, 1, 1); sas.piece(77, 0.1, 0.0, 0, 1); check(q, sas);
        Path rs; rs.piece(30, 0.1, 0.2, 1, 1); rs.piece(21, 0.1, -0.2, 1, -1); rs.piece(60, 0.1, 0.0, 0, 1); check(q, rs);
        Path bad = sas; bad.kappa[50] = NAN; check(q, bad);
        bad = sas; bad.part[0] = 8; check(q, bad);
        bad = rs; bad.gear[(size_t)bad.gear.size() - 1] = 0; check(q, bad);
        bad = rs; bad.x[3] = INFINITY; check(q, bad);
    }
    std::mt19937_64 rng(seed);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto pick = [&](int n) { return (int)(rng() % (uint64_t)n); };
    const double kappas[6] = { 0.0, 0.0, 0.1, -0.3, 1.5, 1e-7 };
    for (int t = 0; t < N; ++t) {
        fcpp_speed_params q = prm;
        q.flags = (uint32_t)pick(8); q.a_acc = uni(0.05, 2.0); q.a_dec = uni(0.05, 2.0); q.turn_kmh = pick(4) ? uni(1.0, 9.0) : INFINITY;
        q.nominal_kmh[pick(8)] = pick(3) ? uni(1.0, 20.0) : 0.0;
        Path P;
        for (int k = pick(7); k > 0; --k) P.piece(pick(60), pick(5) ? uni(0.02, 0.6) : 0.0, kappas[pick(6)], pick(8), pick(3) ? 1 : -1);
        if (!pick(8) && !P.x.empty()) {
            const size_t at = (size_t)pick((int)P.x.size());
            switch (pick(4)) {
                case 0: P.x[at] = NAN; break;
                case 1: P.kappa[at] = -INFINITY; break;
                case 2: P.part[at] = (int8_t)(pick(2) ? 8 : -1); break;
                default: P.gear[at] = (int8_t)(pick(2) ? 0 : 2);
            }
        }
        check(q, P);
    }
    printf("paths %ld samples %ld failed %ld stops %ld at_cap %ld zero_steps %ld\n", n_paths, n_samples, n_failed, n_stops, n_at_cap, n_zero_steps);
    return 0;
}
