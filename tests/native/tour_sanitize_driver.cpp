// tour_sanitize_driver.cpp -- csrc/fcpp_tourfn.h (the rule behind fcpp_debug_cell_tour and the cell tour's kernels) under ASan + UBSan on
// the CPU: random fields of 0 .. 7 cells of 0 .. 4 variants whose joint blocks come from tour_transit on random poses (both modes), the
// caps' two sides (32 / 33 cells, 32 / 33 variants in a cell, 1024 / 1026 nodes) on random blocks, 1 .. 64 candidates, with and without
// E / X and stored nodes, some with NaN poses or a stored node outside its cell.  Any sanitizer report aborts; the driver itself checks
// what every field must give: orders that are permutations with the skipped cells last, nodes inside their cells, the chosen nodes
// chaining to the cost, cost <= stored, the statuses -- and, where a field is small, the optimum over every order and node combination.
// usage: tour_sanitize_driver SEED N
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../field_coverage_path_planning_amd/csrc/fcpp_tourfn.h"

using namespace fcpp;

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// the chained cost of the nodes nd (local to the field) in driving order
static double chain(const TourField &F, const std::vector<int> &nd)
{
    if (nd.empty()) return 0.0;
    double s = tour_first(F, nd[0]);
    for (size_t j = 1; j < nd.size(); ++j) s = tour_close(F, tour_step(F, s, nd[j - 1], nd[j]), nd[j]);
    return tour_last(F, s, nd.back());
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? strtol(argv[2], nullptr, 10) : 60;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    long ok = 0, invalid = 0, unsupported = 0, empty = 0, improved = 0, brute = 0, optimal = 0, moves = 0, solved = 0;
    for (long it = 0; it < n; ++it) {
        // the caps' two sides once each, else small fields
        std::vector<int64_t> V;          // variants per cell
        if (it == 3) V.assign(32, 1);
        else if (it == 4) V.assign(33, 1);
        else if (it == 5) { V.assign(3, 1); V[1] = 32; }
        else if (it == 6) { V.assign(3, 1); V[1] = 33; }
        else if (it == 7) V.assign(16, 32);
        else if (it == 8) V.assign(27, 19);
        else { V.resize((size_t)(it < 3 ? it : rng() % 8)); for (int64_t &v : V) v = (int64_t)(rng() % 5); }
        const bool big = it >= 3 && it <= 8;
        const int64_t m = (int64_t)V.size();
        // the field sits behind a first field of two cells: offsets that do not start at 0
        std::vector<int64_t> voff = { 0, 1, 3 };
        for (int64_t v : V) voff.push_back(voff.back() + v);
        const int64_t c0 = 2, c1 = c0 + m, v0 = voff[(size_t)c0], nv = voff.back(), Nf = 2 * (nv - v0), blk = tour_block(voff.data(), c0, c1);
        const int mode = (int)(it & 1);
        int S = big ? 1 + (int)(it % 3) : (it % 7 == 0 ? TOUR_MAX_STARTS : 1 + (int)(rng() % 12));
        const int max_sweeps = big ? 1 : (it % 5 == 0 ? (int)(rng() % 3) : 8 * (int)m + 8);
        const double min_gain = it % 4 == 0 ? 0.0 : 1e-9;
        const int poison = !big && it % 6 == 5 ? 1 + (int)(rng() % 2) : 0;          // 1: a NaN pose, 2: a stored node outside its cell
        const bool ends = it % 2 == 1, with_sn = it % 3 != 0 || poison == 2;
        std::vector<double> ix((size_t)nv), iy((size_t)nv), ih((size_t)nv), ox((size_t)nv), oy((size_t)nv), oh((size_t)nv), w((size_t)nv);
        for (int64_t v = 0; v < nv; ++v) {
            ix[(size_t)v] = 200.0 * unit(rng); iy[(size_t)v] = 200.0 * unit(rng); ih[(size_t)v] = 6.28 * unit(rng) - 3.14;
            ox[(size_t)v] = 200.0 * unit(rng); oy[(size_t)v] = 200.0 * unit(rng); oh[(size_t)v] = 6.28 * unit(rng) - 3.14;
            w[(size_t)v] = 300.0 * unit(rng);
        }
        if (poison == 1 && nv > v0) ix[(size_t)(v0 + (int64_t)(rng() % (uint64_t)(nv - v0)))] = NAN;
        std::vector<double> D((size_t)blk), E((size_t)(2 * nv)), X((size_t)(2 * nv));
        for (int64_t a = 0; blk && a < Nf; ++a)
            for (int64_t b = 0; b < Nf; ++b) {
                double v = INFINITY;
                if (tour_cell_of(voff.data(), c0, c1, a) != tour_cell_of(voff.data(), c0, c1, b)) {
                    if (big) v = 5.0 + 95.0 * unit(rng);
                    else {
                        v = mode == 0 ? tour_transit<0>(ix.data(), iy.data(), ih.data(), ox.data(), oy.data(), oh.data(), 6.0, v0 + (a >> 1), (int)(a & 1),
                                                        v0 + (b >> 1), (int)(b & 1))
                                      : tour_transit<1>(ix.data(), iy.data(), ih.data(), ox.data(), oy.data(), oh.data(), 6.0, v0 + (a >> 1), (int)(a & 1),
                                                        v0 + (b >> 1), (int)(b & 1));
                        ++solved;
                    }
                }
                D[(size_t)(a * Nf + b)] = v;
            }
        for (double &v : E) v = 50.0 * unit(rng);
        for (double &v : X) v = 50.0 * unit(rng);
        std::vector<int32_t> sn((size_t)(c0 + m), 0);
        for (int64_t c = c0; c < c1; ++c) sn[(size_t)c] = V[(size_t)(c - c0)] ? (int32_t)(rng() % (uint64_t)(2 * V[(size_t)(c - c0)])) : 0;
        int k = 0;
        for (int64_t v : V) k += v > 0;
        if (poison == 2 && k > 0) {
            int64_t c = c0 + (int64_t)(rng() % (uint64_t)m);
            while (V[(size_t)(c - c0)] == 0) c = c0 + (c - c0 + 1) % m;
            sn[(size_t)c] = (int32_t)(2 * V[(size_t)(c - c0)]);
        }
        std::vector<int32_t> order((size_t)m, -7), node((size_t)m, -7), tours((size_t)(S * m), -7);
        std::vector<double> costs((size_t)S, -7.0);
        const TourResult r = tour_field_host(voff.data(), c0, c1, w.data(), with_sn ? sn.data() : nullptr, blk ? D.data() : nullptr,
                                             ends ? E.data() : nullptr, ends ? X.data() : nullptr, S, min_gain, max_sweeps, order.data(), node.data(),
                                             tours.data(), m, costs.data());
        if (!tour_supported(voff.data(), c0, c1)) {
            if (r.status != TOUR_EUNSUPPORTED || r.winner != 0 || r.sweeps != 0 || r.cost == r.cost || r.stored == r.stored || r.joint == r.joint) {
                printf("over a cap at %ld\n", it); return 1;
            }
            for (int64_t q = 0; q < m; ++q)
                if (order[(size_t)q] != q || node[(size_t)q] != -1 || tours[(size_t)((S - 1) * m + q)] != q) { printf("stored order at %ld\n", it); return 1; }
            ++unsupported;
            continue;
        }
        std::vector<int> noff((size_t)m + 1);
        for (int64_t j = 0; j <= m; ++j) noff[(size_t)j] = (int)(2 * (voff[(size_t)(c0 + j)] - v0));
        const TourField F = { D.data(), ends ? E.data() + 2 * v0 : nullptr, ends ? X.data() + 2 * v0 : nullptr, w.data() + v0, noff.data(), (int)Nf };
        // every candidate's order, then the winner's: the kept cells once each, the skipped ones behind them in stored order
        for (int c = 0; c <= S; ++c) {
            const int32_t *src = c < S ? tours.data() + (size_t)c * (size_t)m : order.data();
            std::vector<char> seen((size_t)m, 0);
            int last_rest = -1;
            for (int64_t q = 0; q < m; ++q) {
                const int32_t cell = src[q];
                if (cell < 0 || cell >= m || seen[(size_t)cell]) { printf("not a permutation at %ld candidate %d\n", it, c); return 1; }
                seen[(size_t)cell] = 1;
                const bool is_kept = V[(size_t)cell] > 0;
                if (is_kept != (q < k) || (!is_kept && cell < last_rest)) { printf("skipped cells at %ld candidate %d\n", it, c); return 1; }
                if (!is_kept) last_rest = cell;
            }
        }
        if (r.skipped != m - k || r.winner < 0 || r.winner >= S || r.sweeps < 0 || r.sweeps > max_sweeps) { printf("winner / sweeps at %ld\n", it); return 1; }
        std::vector<int> nd;
        for (int q = 0; q < k; ++q) {
            const int cell = order[(size_t)q], u = node[(size_t)cell];
            if (u < 0 || u >= 2 * V[(size_t)cell]) { printf("node outside its cell at %ld\n", it); return 1; }
            nd.push_back(noff[(size_t)cell] + u);
        }
        for (int64_t j = 0; j < m; ++j) if (V[(size_t)j] == 0 && node[(size_t)j] != -1) { printf("a skipped cell's node at %ld\n", it); return 1; }
        if (r.status == TOUR_OK) {
            if (!tour_finite(r.stored) || r.cost > r.stored) { printf("dearer than the stored order at %ld\n", it); return 1; }
            if (!same_bits(chain(F, nd), r.cost) || !same_bits(costs[(size_t)r.winner], r.cost)) { printf("the nodes do not chain to the cost at %ld\n", it); return 1; }
            for (int c = 0; c < S; ++c) if (costs[(size_t)c] < r.cost) { printf("not the cheapest at %ld\n", it); return 1; }
            if (k == 0) { if (r.cost != 0.0 || r.joint != 0.0) { printf("empty tour at %ld\n", it); return 1; } ++empty; }
            ++ok;
            if (r.cost < r.stored) ++improved;
            // every order and every node combination of a small field
            double combos = 1.0;
            for (int64_t v : V) if (v > 0) combos *= 2.0 * (double)v;
            if (k >= 1 && k <= 5 && combos <= 4096.0) {
                std::vector<int> perm;
                for (int64_t j = 0; j < m; ++j) if (V[(size_t)j] > 0) perm.push_back((int)j);
                double best = INFINITY;
                do {
                    std::vector<int> pick((size_t)k, 0), cur((size_t)k);
                    for (;;) {
                        for (int q = 0; q < k; ++q) cur[(size_t)q] = noff[(size_t)perm[(size_t)q]] + pick[(size_t)q];
                        const double v = chain(F, cur);
                        if (v < best) best = v;
                        int q = 0;
                        while (q < k && ++pick[(size_t)q] == 2 * V[(size_t)perm[(size_t)q]]) pick[(size_t)q++] = 0;
                        if (q == k) break;
                    }
                } while (std::next_permutation(perm.begin(), perm.end()));
                if (r.cost < best) { printf("below the optimum at %ld\n", it); return 1; }
                if (k <= 3 && max_sweeps >= 1 && S >= 2 && r.cost > best + min_gain) { printf("k <= 3 misses the optimum at %ld\n", it); return 1; }
                ++brute;
                if (r.cost == best) ++optimal;
            }
        } else {
            if (r.status != TOUR_EINVAL || tour_finite(r.stored) || r.winner != 0 || r.sweeps != 0 || !same_bits(r.cost, r.stored) || r.joint == r.joint) {
                printf("status at %ld\n", it); return 1;
            }
            int q = 0;
            for (int64_t j = 0; j < m; ++j) if (V[(size_t)j] > 0 && order[(size_t)q++] != j) { printf("invalid field's order at %ld\n", it); return 1; }
            ++invalid;
        }
        moves += r.sweeps;
    }
    printf("ok %ld invalid %ld unsupported %ld empty %ld improved %ld brute %ld optimal %ld moves %ld solved %ld\n", ok, invalid, unsupported, empty,
           improved, brute, optimal, moves, solved);
    return 0;
}
