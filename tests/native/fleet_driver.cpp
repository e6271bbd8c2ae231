// fleet_driver.cpp -- csrc/fcpp_fleetfn.h (the rule behind fcpp_debug_fleet_solve and the vehicle shares' kernel) under ASan + UBSan on the
// CPU: random fields of 0 .. 10 swaths against every composition into at most K shares, fields of 17 .. 513 swaths (both sides of the cap),
// 1 .. 64 candidates, both directions and one, K from 0 to 17 (both sides of both bounds), rows of the per-share outputs shorter than K,
// omega 0, 1 and 2.5, and every way a field can be invalid.  Any sanitizer report aborts; the driver itself checks what every field must
// give: the tour is the winner's variant, the shares partition it, their costs are share_cost, their largest is the makespan and their
// rounded sum the total, nothing beats the winner -- and, where a field is small, (M, sum) of every variant over all compositions, bit
// for bit.
// usage: fleet_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_fleetfn.h"

using namespace fcpp;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? strtol(argv[2], nullptr, 10) : 60;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    const int big[] = { 17, 63, 64, 65, 66, 130, 512, 513 };
    const double omegas[] = { 0.0, 1.0, 2.5 };
    long ok = 0, invalid = 0, unsupported = 0, empty = 0, brute = 0, backwards = 0, fewer = 0;
    for (long it = 0; it < n; ++it) {
        const int64_t m = it < 8 ? big[it] : (int64_t)(rng() % 11);
        const bool has_block = m <= ROUTE_MAX_SWATHS;
        const int N = (int)(2 * m), C = it % 9 == 0 && it >= 8 ? TRIP_MAX_CANDIDATES : 1 + (int)(rng() % 4), both = it % 4 != 3;
        const int poison = it >= 8 && it % 7 == 6 ? 1 + (int)(rng() % 6) : 0;
        int K = it < 8 ? (it % 2 ? 16 : 3) : 1 + (int)(rng() % 6), k_stride = it % 3 == 0 ? std::max(K, 1) : FLEET_MAX_VEHICLES;
        const double omega = omegas[it % 3];
        // the field sits behind three swaths of another field: a stride beyond m
        const int64_t s0 = 3, stride = s0 + m;
        std::vector<double> T(has_block ? (size_t)N * (size_t)N : 0), In((size_t)N), Out((size_t)N), len((size_t)m);
        const bool whole = it % 5 == 2;          // whole numbers: ties
        for (double &v : T) v = whole ? (double)(3 + rng() % 27) : 3.0 + 27.0 * unit(rng);
        for (int s = 0; has_block && s < m; ++s)
            for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) T[(size_t)((2 * s + a) * N + 2 * s + b)] = INFINITY;
        for (int p = 0; p < N; ++p) { In[(size_t)p] = whole ? (double)(rng() % 80) : 80.0 * unit(rng); Out[(size_t)p] = whole ? (double)(rng() % 80) : 80.0 * unit(rng); }
        for (double &w : len) w = whole ? (double)(5 + rng() % 55) : 5.0 + 55.0 * unit(rng);
        std::vector<int32_t> tours((size_t)(C * stride), -9);
        for (int c = 0; c < C; ++c) {
            std::vector<int32_t> perm((size_t)m);
            std::iota(perm.begin(), perm.end(), 0);
            std::shuffle(perm.begin(), perm.end(), rng);
            for (int64_t k = 0; k < m; ++k) tours[(size_t)(c * stride + s0 + k)] = 2 * perm[(size_t)k] + (int32_t)(rng() & 1);
        }
        bool poisoned = false, beyond = false;
        if (poison == 4) { K = rng() & 1 ? 0 : -3; poisoned = true; }                  // (these two hold for a field without swaths too)
        if (poison == 5) { K = FLEET_MAX_VEHICLES + 1; beyond = true; }
        if (poison == 6) { K = 5; k_stride = 4; poisoned = true; }
        if (m > 0 && has_block) {
            if (poison == 1) { tours[(size_t)((C - 1) * stride + s0 + (int64_t)(rng() % (uint64_t)m))] = (int32_t)(rng() % 3 == 0 ? N : -1); poisoned = true; }
            if (poison == 2 && m > 1) { tours[(size_t)(s0 + 1)] = tours[(size_t)s0] ^ 1; poisoned = true; }
            if (poison == 3) { len[(size_t)(rng() % (uint64_t)m)] = rng() & 1 ? -1.0 : NAN; poisoned = true; }
            if (poison == 0 && it % 11 == 10 && m > 1) {                               // candidate 0's S not finite
                T[(size_t)(tours[(size_t)s0] * N + tours[(size_t)(s0 + 1)])] = INFINITY;
                poisoned = true;
            }
        }
        const FleetField F = { T.data(), In.data(), Out.data(), len.data(), tours.data() + s0, stride, has_block ? (int)m : 0, C, both, K, k_stride, omega };
        std::vector<int32_t> tour((size_t)m, -7), share((size_t)m, -7), first((size_t)k_stride, -7);
        std::vector<double> Ms((size_t)(2 * C), -7.0), sums((size_t)(2 * C), -7.0), cost((size_t)k_stride, -7.0);
        const FleetResult r = fleet_field_host(F, m, tour.data(), share.data(), Ms.data(), sums.data(), first.data(), cost.data());
        if (!has_block || poisoned || beyond) {
            const int want = !has_block || beyond ? FLEET_EUNSUPPORTED : FLEET_EINVAL;
            if (r.status != want || r.n_used != (m > 0) || r.winner != 0 || r.makespan == r.makespan || r.total == r.total) { printf("status at %ld\n", it); return 1; }
            for (int64_t k = 0; k < m; ++k)
                if (tour[(size_t)k] != tours[(size_t)(s0 + k)] || share[(size_t)k] != 0) { printf("a failed field's tour at %ld\n", it); return 1; }
            for (int v = 0; v < 2 * C; ++v) if (Ms[(size_t)v] == Ms[(size_t)v] || sums[(size_t)v] == sums[(size_t)v]) { printf("a failed field's rows at %ld\n", it); return 1; }
            for (int k = 0; k < k_stride; ++k)
                if (first[(size_t)k] != (k == 0 && m > 0 ? 0 : -1) || cost[(size_t)k] == cost[(size_t)k]) { printf("a failed field's shares at %ld\n", it); return 1; }
            ++(want == FLEET_EINVAL ? invalid : unsupported);
            continue;
        }
        if (r.status != FLEET_OK || r.winner < 0 || r.winner >= 2 * C || !trip_exists(r.winner, both)) { printf("winner at %ld\n", it); return 1; }
        for (int v = 0; v < 2 * C; ++v) {
            const bool is = trip_exists(v, both);
            if (is != (Ms[(size_t)v] == Ms[(size_t)v]) || is != (sums[(size_t)v] == sums[(size_t)v])) { printf("the rows' slots at %ld\n", it); return 1; }
            if (is && v != r.winner && fleet_better(Ms[(size_t)v], sums[(size_t)v], v, r.makespan, r.total, r.winner)) { printf("not the best at %ld\n", it); return 1; }
        }
        if (!same_bits(Ms[(size_t)r.winner], r.makespan) || !same_bits(sums[(size_t)r.winner], r.total)) { printf("values at %ld\n", it); return 1; }
        for (int k = r.n_used; k < k_stride; ++k)
            if (first[(size_t)k] != -1 || cost[(size_t)k] == cost[(size_t)k]) { printf("beyond n_used at %ld\n", it); return 1; }
        if (m == 0) { if (r.n_used != 0 || r.makespan != 0.0 || r.total != 0.0) { printf("empty field at %ld\n", it); return 1; } ++empty; ++ok; continue; }
        if (r.n_used < 1 || r.n_used > std::min<int64_t>(K, m)) { printf("n_used at %ld\n", it); return 1; }
        // the winner's tables, restated
        std::vector<double> P((size_t)m + 1, 0.0), S((size_t)m, 0.0);
        const int32_t *cand = F.tours + (r.winner >> 1) * stride;
        for (int64_t k = 0; k < m; ++k) {
            if (tour[(size_t)k] != trip_at(cand, (int)m, r.winner & 1, (int)k)) { printf("tour at %ld\n", it); return 1; }
            P[(size_t)k + 1] = P[(size_t)k] + len[(size_t)(tour[(size_t)k] >> 1)];
            if (k > 0) S[(size_t)k] = S[(size_t)k - 1] + T[(size_t)(tour[(size_t)k - 1] * N + tour[(size_t)k])];
        }
        auto c_of = [&](const int32_t *t, const double *Pp, const double *Sp, int i, int j) {
            return fleet_cost(In[(size_t)t[i]], Sp[i], Pp[i], Sp[j - 1], Out[(size_t)t[j - 1]], Pp[j], omega);
        };
        double chain = 0.0, top = -INFINITY;
        if (share[0] != 0 || first[0] != 0) { printf("the first share at %ld\n", it); return 1; }
        for (int s = 0; s < r.n_used; ++s) {
            const int i = first[(size_t)s], j = s + 1 < r.n_used ? first[(size_t)s + 1] : (int)m;
            if (i < 0 || j <= i || j > m) { printf("share bounds at %ld\n", it); return 1; }
            for (int k = i; k < j; ++k) if (share[(size_t)k] != s) { printf("share indices at %ld\n", it); return 1; }
            const double c = c_of(tour.data(), P.data(), S.data(), i, j);
            if (!same_bits(c, cost[(size_t)s])) { printf("share cost at %ld\n", it); return 1; }
            chain = tour_plus(c, chain);
            top = fleet_max(top, c);
        }
        if (!same_bits(chain, r.total) || !same_bits(top, r.makespan)) { printf("the shares do not give the values at %ld\n", it); return 1; }
        ++ok;
        backwards += r.winner & 1; fewer += r.n_used < std::min<int64_t>(K, m);
        // every composition of every variant of a small field
        if (m <= 10) {
            FleetTables *W = new FleetTables;
            for (int v = 0; v < 2 * C; ++v) {
                if (!trip_exists(v, both)) continue;
                fleet_tables_host(F, v, *W);          // (its tables; the programme's result is what is being checked)
                std::vector<int32_t> t((size_t)m);
                for (int k = 0; k < m; ++k) t[(size_t)k] = W->t[k];
                double bestM = INFINITY, bestS = INFINITY;
                for (int pass = 0; pass < 2; ++pass)
                    for (uint32_t mask = 0; mask < (1u << (m - 1)); ++mask) {
                        if (__builtin_popcount(mask) > K - 1) continue;
                        double sum = 0.0, mx = -INFINITY;
                        int i = 0;
                        for (int j = 1; j <= m; ++j) {
                            if (j < m && !(mask >> (j - 1) & 1u)) continue;
                            const double c = c_of(t.data(), W->P, W->S, i, j);
                            sum = tour_plus(c, sum); mx = fleet_max(mx, c);
                            i = j;
                        }
                        if (pass == 0 && mx < bestM) bestM = mx;
                        if (pass == 1 && mx <= bestM && sum < bestS) bestS = sum;
                    }
                if (!same_bits(bestM, Ms[(size_t)v]) || !same_bits(bestS, sums[(size_t)v])) { printf("not the optimum at %ld variant %d\n", it, v); delete W; return 1; }
            }
            delete W;
            ++brute;
        }
    }
    printf("ok %ld invalid %ld unsupported %ld empty %ld brute %ld backwards %ld fewer %ld\n", ok, invalid, unsupported, empty, brute, backwards, fewer);
    return 0;
}
