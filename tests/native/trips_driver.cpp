// trips_driver.cpp -- csrc/fcpp_tripfn.h (the rule behind fcpp_debug_trip_solve and the service trips' kernel) under ASan + UBSan on the
// CPU: random fields of 0 .. 10 swaths against every stop set, fields of 17 .. 513 swaths (both sides of the cap), 1 .. 64 candidates,
// both directions and one, with and without E / X and a first capacity, capacities from below every swath to +inf, and every way a field
// can be invalid.  Any sanitizer report aborts; the driver itself checks what every field must give: the tour is the winner's variant,
// the trips partition it and are feasible, the stops chain to `extra`, nothing beats the winner -- and, where a field is small, the
// optimum over all 2^(m - 1) stop sets of every variant, bit for bit.
// usage: trips_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_tripfn.h"

using namespace fcpp;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? strtol(argv[2], nullptr, 10) : 60;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    const int big[] = { 17, 63, 64, 65, 66, 130, 512, 513 };
    long ok = 0, invalid = 0, unsupported = 0, empty = 0, split = 0, overfull = 0, brute = 0, backwards = 0;
    for (long it = 0; it < n; ++it) {
        const int64_t m = it < 8 ? big[it] : (int64_t)(rng() % 11);
        const bool has_block = m <= ROUTE_MAX_SWATHS;
        const int N = (int)(2 * m), C = it % 9 == 0 ? TRIP_MAX_CANDIDATES : 1 + (int)(rng() % 4), both = it % 4 != 3;
        const bool ends = it % 2 == 1, first = it % 3 == 1;
        const int poison = it >= 8 && it % 7 == 6 ? 1 + (int)(rng() % 5) : 0;
        // the field sits behind three swaths of another field: a stride beyond m
        const int64_t s0 = 3, stride = s0 + m;
        std::vector<double> T(has_block ? (size_t)N * (size_t)N : 0), E((size_t)N), X((size_t)N), In((size_t)N), Out((size_t)N), len((size_t)m);
        for (double &v : T) v = 3.0 + 27.0 * unit(rng);
        for (int s = 0; has_block && s < m; ++s)
            for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) T[(size_t)((2 * s + a) * N + 2 * s + b)] = INFINITY;
        for (int p = 0; p < N; ++p) { E[(size_t)p] = 80.0 * unit(rng); X[(size_t)p] = 80.0 * unit(rng); In[(size_t)p] = 80.0 * unit(rng); Out[(size_t)p] = 80.0 * unit(rng); }
        double mean = m > 0 ? 0.0 : 1.0;          // (a field without swaths still needs a capacity above 0)
        for (double &w : len) { w = 5.0 + 55.0 * unit(rng); mean += w / (double)m; }
        std::vector<int32_t> tours((size_t)(C * stride), -9);
        for (int c = 0; c < C; ++c) {
            std::vector<int32_t> perm((size_t)m);
            std::iota(perm.begin(), perm.end(), 0);
            std::shuffle(perm.begin(), perm.end(), rng);
            for (int64_t k = 0; k < m; ++k) tours[(size_t)(c * stride + s0 + k)] = 2 * perm[(size_t)k] + (int32_t)(rng() & 1);
        }
        double Q = it % 5 == 0 ? INFINITY : (it % 5 == 1 ? 4.0 : (it < 8 ? 65.5 * mean : (1.0 + 3.0 * unit(rng)) * mean));
        double Q0 = first ? Q * (0.3 + 0.7 * unit(rng)) : Q;
        if (m > 0 && has_block) {
            if (poison == 1) tours[(size_t)((C - 1) * stride + s0 + (int64_t)(rng() % (uint64_t)m))] = (int32_t)(rng() % 3 == 0 ? N : -1);
            if (poison == 2 && m > 1) tours[(size_t)(s0 + 1)] = tours[(size_t)s0] ^ 1;
            if (poison == 3) len[(size_t)(rng() % (uint64_t)m)] = rng() & 1 ? -1.0 : NAN;
            if (poison == 4) (rng() & 1 ? Q : Q0) = rng() & 1 ? NAN : 0.0;
            if (poison == 5) E[(size_t)tours[(size_t)s0]] = INFINITY;
        }
        const bool poisoned = m > 0 && has_block && (poison == 1 || (poison == 2 && m > 1) || poison == 3 || poison == 4 || (poison == 5 && ends));
        const TripField F = { T.data(), ends ? E.data() : nullptr, ends ? X.data() : nullptr, In.data(), Out.data(), len.data(), tours.data() + s0, stride,
                              has_block ? (int)m : 0, C, both, Q, Q0, it % 2 ? 7.5 : 0.0 };
        std::vector<int32_t> tour((size_t)m, -7), trip((size_t)m, -7);
        std::vector<double> costs((size_t)(2 * C), -7.0);
        const TripResult r = trip_field_host(F, m, tour.data(), trip.data(), costs.data());
        if (!has_block || poisoned) {
            if (r.status != (has_block ? TRIP_EINVAL : TRIP_EUNSUPPORTED) || r.n_trips != (m > 0) || r.overfull != 0 || r.winner != 0 || r.cost == r.cost ||
                r.base == r.base || r.extra == r.extra) { printf("status at %ld\n", it); return 1; }
            for (int64_t k = 0; k < m; ++k)
                if (tour[(size_t)k] != tours[(size_t)(s0 + k)] || trip[(size_t)k] != 0) { printf("a failed field's tour at %ld\n", it); return 1; }
            for (double v : costs) if (v == v) { printf("a failed field's costs at %ld\n", it); return 1; }
            ++(has_block ? invalid : unsupported);
            continue;
        }
        if (r.status != TRIP_OK || r.winner < 0 || r.winner >= 2 * C || !trip_exists(r.winner, both)) { printf("winner at %ld\n", it); return 1; }
        for (int v = 0; v < 2 * C; ++v) {
            const bool is = trip_exists(v, both);
            if (is != (costs[(size_t)v] == costs[(size_t)v])) { printf("the cost row's slots at %ld\n", it); return 1; }
            if (is && (costs[(size_t)v] < r.cost || (costs[(size_t)v] == r.cost && v < r.winner))) { printf("not the cheapest at %ld\n", it); return 1; }
        }
        if (!same_bits(costs[(size_t)r.winner], r.cost) || !same_bits(tour_plus(r.base, r.extra), r.cost)) { printf("cost at %ld\n", it); return 1; }
        if (m == 0) { if (r.n_trips != 0 || r.cost != 0.0) { printf("empty field at %ld\n", it); return 1; } ++empty; ++ok; continue; }
        // the winner's tables, restated
        std::vector<double> P((size_t)m + 1, 0.0), d((size_t)m, 0.0);
        const int32_t *cand = F.tours + (r.winner >> 1) * stride;
        for (int64_t k = 0; k < m; ++k) {
            if (tour[(size_t)k] != trip_at(cand, (int)m, r.winner & 1, (int)k)) { printf("tour at %ld\n", it); return 1; }
            P[(size_t)k + 1] = P[(size_t)k] + len[(size_t)(tour[(size_t)k] >> 1)];
            if (k > 0) d[(size_t)k] = trip_stop(F, tour[(size_t)k - 1], tour[(size_t)k], T[(size_t)(tour[(size_t)k - 1] * N + tour[(size_t)k])]);
        }
        double chain = 0.0;
        int trips = 1, over = 0;
        int64_t start = 0;
        if (trip[0] != 0) { printf("the first trip at %ld\n", it); return 1; }
        for (int64_t k = 1; k <= m; ++k) {
            if (k < m && trip[(size_t)k] == trip[(size_t)k - 1]) continue;
            if (k < m && trip[(size_t)k] != trip[(size_t)k - 1] + 1) { printf("trip indices at %ld\n", it); return 1; }
            const double cap = start == 0 ? Q0 : Q;
            if (!trip_feasible(P[(size_t)start], P[(size_t)k], (int)start, (int)k, cap)) { printf("an infeasible trip at %ld\n", it); return 1; }
            over += trip_over(P[(size_t)start], P[(size_t)k], cap);
            if (k < m) { chain = tour_plus(d[(size_t)k], chain); ++trips; start = k; }
        }
        if (trips != r.n_trips || over != r.overfull || !same_bits(chain, r.extra)) { printf("the stops do not chain to extra at %ld\n", it); return 1; }
        if (Q == INFINITY && r.extra > 0.0) { printf("a paid stop without need at %ld\n", it); return 1; }
        if (Q == 4.0 && Q0 <= 4.0 && (r.n_trips != m || r.overfull != m)) { printf("a capacity below every swath at %ld\n", it); return 1; }
        ++ok;
        split += r.n_trips > 1; overfull += r.overfull; backwards += r.winner & 1;
        // every stop set of every variant of a small field
        if (m <= 10) {
            TripTables W;
            for (int v = 0; v < 2 * C; ++v) {
                if (!trip_exists(v, both)) continue;
                const TripVariant tv = trip_variant_host(F, v, W);          // (its tables; the programme's result is what is being checked)
                double best = INFINITY;
                for (uint32_t mask = 0; mask < (1u << (m - 1)); ++mask) {
                    double c = 0.0;
                    bool fits = true;
                    int i = 0;
                    for (int j = 1; j <= m && fits; ++j) {
                        if (j < m && !(mask >> (j - 1) & 1u)) continue;
                        fits = trip_feasible(W.P[i], W.P[j], i, j, trip_cap(F, i));
                        if (j < m) { c = tour_plus(trip_stop(F, W.t[j - 1], W.t[j], T[(size_t)(W.t[j - 1] * N + W.t[j])]), c); i = j; }
                    }
                    if (fits && c < best) best = c;
                }
                if (!same_bits(best, tv.extra) || !same_bits(tour_plus(tv.base, best), costs[(size_t)v])) { printf("not the optimum at %ld variant %d\n", it, v); return 1; }
            }
            ++brute;
        }
    }
    printf("ok %ld invalid %ld unsupported %ld empty %ld split %ld overfull %ld brute %ld backwards %ld\n", ok, invalid, unsupported, empty, split, overfull,
           brute, backwards);
    return 0;
}
