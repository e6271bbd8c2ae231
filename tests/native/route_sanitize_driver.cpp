// route_sanitize_driver.cpp -- csrc/fcpp_routefn.h (the rule behind fcpp_debug_route and the swath router's kernels) under ASan + UBSan on the
// CPU: random transit blocks made bit-symmetric under (p, q) <-> (q ^ 1, p ^ 1) with an infinite same-swath diagonal, m = 0 .. 40 and the
// cap's two sides (512, 513), 1 .. 64 candidates, with and without E / X, some with NaN or infinite entries.  Any sanitizer report aborts;
// the driver itself checks what every field must give: tours that are permutations, costs that are the tours' costs, a winner no dearer
// than the stored order, the statuses.  usage: route_sanitize_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_routefn.h"

using namespace fcpp;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? strtol(argv[2], nullptr, 10) : 60;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    long ok = 0, invalid = 0, unsupported = 0, improved = 0, poisoned = 0, moves = 0;
    for (long it = 0; it < n; ++it) {
        // the cap's two sides once each, else 0 .. 40
        const int64_t m = it == 3 ? ROUTE_MAX_SWATHS : (it == 4 ? ROUTE_MAX_SWATHS + 1 : (it < 3 ? it : (int64_t)(rng() % 41)));
        const bool big = m >= ROUTE_MAX_SWATHS;
        int S = big ? 3 : (it % 7 == 0 ? ROUTE_MAX_STARTS : 1 + (int)(rng() % ROUTE_MAX_STARTS));
        if (m > 24 && !big && S > 8) S = 1 + S % 8;
        const int max_sweeps = big ? 2 : (it % 5 == 0 ? (int)(rng() % 3) : 8 * (int)m + 8);
        const double min_gain = it % 4 == 0 ? 0.0 : 1e-9;
        const int poison = it % 6 == 5 ? 1 + (int)(rng() % 3) : 0;         // 1: NaN entries, 2: +inf entries, 3: NaN in E
        const bool ends = it % 2 == 1 || poison == 3;
        const int64_t N = 2 * m, blk = route_block(m);
        std::vector<double> T((size_t)blk), E((size_t)N), X((size_t)N);
        for (int64_t p = 0; blk && p < N; ++p)
            for (int64_t q = 0; q < N; ++q) {
                if (!route_canonical((int)p, (int)q, (int)N)) continue;
                double v = (p >> 1) == (q >> 1) ? INFINITY : 5.0 + 95.0 * unit(rng);
                if (poison == 1 && v < INFINITY && rng() % 16 == 0) v = NAN;
                if (poison == 2 && rng() % 8 == 0) v = INFINITY;
                T[(size_t)(p * N + q)] = v;
                T[(size_t)((q ^ 1) * N + (p ^ 1))] = v;
            }
        for (double &v : E) v = 50.0 * unit(rng);
        for (double &v : X) v = 50.0 * unit(rng);
        if (poison == 3 && N) E[(size_t)(rng() % (uint64_t)N)] = NAN;
        std::vector<int32_t> tours((size_t)(S * m), -1), route((size_t)m, -1);
        std::vector<double> costs((size_t)S, -1.0);
        const RouteField f = route_field_host(blk ? T.data() : nullptr, ends ? E.data() : nullptr, ends ? X.data() : nullptr, m, S, min_gain, max_sweeps,
                                              tours.data(), m, costs.data(), route.data());
        if (m > ROUTE_MAX_SWATHS) {
            if (f.status != ROUTE_EUNSUPPORTED || f.winner != 0 || f.sweeps != 0 || f.cost == f.cost) { printf("over the cap at %ld\n", it); return 1; }
            for (int64_t k = 0; k < m; ++k)
                if (route[(size_t)k] != 2 * k + (k & 1) || tours[(size_t)((S - 1) * m + k)] != route[(size_t)k]) { printf("stored order at %ld\n", it); return 1; }
            ++unsupported;
            continue;
        }
        const RouteCosts rc = { T.data(), ends ? E.data() : nullptr, ends ? X.data() : nullptr, (int)N };
        std::vector<int16_t> t((size_t)m);
        for (int c = 0; c <= S; ++c) {          // every candidate's tour, then the route
            const int32_t *src = c < S ? tours.data() + (size_t)c * (size_t)m : route.data();
            std::vector<char> seen((size_t)m, 0);
            for (int64_t k = 0; k < m; ++k) {
                const int32_t p = src[k];
                if (p < 0 || p >= N || seen[(size_t)(p >> 1)]) { printf("not a permutation at %ld candidate %d\n", it, c); return 1; }
                seen[(size_t)(p >> 1)] = 1;
                t[(size_t)k] = (int16_t)p;
            }
            const double cost = route_cost(rc, t.data(), (int)m);
            if (!same_bits(cost, c < S ? costs[(size_t)c] : f.cost)) { printf("cost at %ld candidate %d\n", it, c); return 1; }
        }
        if (f.winner < 0 || f.winner >= S || f.sweeps < 0 || f.sweeps > max_sweeps) { printf("winner / sweeps at %ld\n", it); return 1; }
        if (f.status == ROUTE_OK) {
            if (!route_finite(f.stored) || f.cost > f.stored) { printf("dearer than the stored order at %ld\n", it); return 1; }
            for (int c = 0; c < S; ++c) if (costs[(size_t)c] < f.cost) { printf("not the cheapest at %ld\n", it); return 1; }
            ++ok;
            if (f.cost < f.stored) ++improved;
        } else {
            if (f.status != ROUTE_EINVAL || route_finite(f.stored) || f.winner != 0 || f.sweeps != 0) { printf("status at %ld\n", it); return 1; }
            for (int64_t k = 0; k < m; ++k) if (route[(size_t)k] != route_stored(0, (int)k)) { printf("invalid field's order at %ld\n", it); return 1; }
            ++invalid;
        }
        if (poison) ++poisoned;
        moves += f.sweeps;
    }
    printf("ok %ld invalid %ld unsupported %ld improved %ld poisoned %ld moves %ld\n", ok, invalid, unsupported, improved, poisoned, moves);
    return 0;
}
