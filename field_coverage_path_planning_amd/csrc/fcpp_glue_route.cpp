// fcpp_glue_route.cpp -- C-ABI glue of the swath router, the clear-aware transit block and the priced transit block (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_clear.h"
#include "fcpp_clearfn.h"
#include "fcpp_parallel.h"
#include "fcpp_route.h"
#include "fcpp_routefn.h"
#include "fcpp_solveclear.h"

using namespace fcpp;

namespace {
// ---- swath router: what fcpp_route_transit / _solve and their host twins check alike ---------------------------------------------------
int route_search(int S, double min_gain, int max_sweeps)
{
    if (S < 1 || S > ROUTE_MAX_STARTS) return fail(FCPP_EINVAL, "n_starts must lie in 1 .. 64");
    if (!(min_gain >= 0.0) || !isfinite(min_gain)) return fail(FCPP_EINVAL, "min_gain must be non-negative and finite");
    if (max_sweeps < 0 || max_sweeps > ROUTE_MAX_SWEEPS) return fail(FCPP_EINVAL, "max_sweeps must lie in 0 .. 2^20");
    return FCPP_OK;
}

int clear_penalty(double penalty)
{
    if (!(penalty >= 0.0) || !isfinite(penalty)) return fail(FCPP_EINVAL, "penalty must be non-negative and finite");
    return FCPP_OK;
}

// the workgroups of k_clear_transit: CLEAR_TILE entries of one field's block each
int clear_tiles(int64_t n, const std::vector<int64_t> &toff, std::vector<int64_t> &tile_off)
{
    try { tile_off.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n; ++i)
        tile_off[(size_t)i + 1] = tile_off[(size_t)i] + (toff[(size_t)i + 1] - toff[(size_t)i] + CLEAR_TILE - 1) / CLEAR_TILE;
    if (tile_off[(size_t)n] > CLEAR_MAX_GROUPS) return fail(FCPP_ESIZE, "2^39 transit entries or more");
    return FCPP_OK;
}

// What the three transit twins walk, fields to the library's host threads: fn(i, s0, p, q, e, e2) for every canonical entry (p, q) of field
// i's block (none for a field beyond the cap) -- s0 the field's first swath, e the entry's place in T, e2 its mirror's.
template <class Fn>
void transit_twin(int64_t n, const std::vector<int64_t> &soff, const std::vector<int64_t> &toff, Fn fn)
{
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i], t0 = toff[(size_t)i];
        const int N = (int)(toff[(size_t)i + 1] == t0 ? 0 : 2 * (soff[(size_t)i + 1] - s0));
        for (int p = 0; p < N; ++p)
            for (int q = 0; q < N; ++q)
                if (route_canonical(p, q, N)) fn(i, s0, p, q, t0 + p * N + q, t0 + (q ^ 1) * N + (p ^ 1));
    });
}

// ---- the priced transit block (fcpp_clear.hip, fcpp_solveclear.hip; the rule: priced_transit of fcpp_solveclearfn.h) ---------------------
// what the clear-aware and the priced transit entries and their host twins check alike before the offsets (out: T, or NULL if an output is missing)
int transit_clear_args(const void *swath_offsets, const void *t_offsets, const void *ring_offsets, const void *vert_offsets, int64_t n, int64_t n_total,
                       const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                       int64_t t_total, int64_t n_rings, int64_t n_verts, const double *x, const double *y, double penalty, const void *out)
{
    if (!swath_offsets || !t_offsets || !ring_offsets || !vert_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) ||
        (t_total > 0 && !out) || (n_verts > 0 && (!x || !y)))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc == FCPP_OK) rc = clear_penalty(penalty);
    if (rc == FCPP_OK && (n_rings < 0 || n_verts < 0)) rc = fail(FCPP_ESIZE, "bad sizes");
    return rc;
}
}  // namespace

extern "C" {

// ---- swath router (fcpp_route.hip; the rule: fcpp_routefn.h) ------------------------------------------------------------------------
int fcpp_route_transit(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                       const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                       const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, double *T)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!swath_offsets || !t_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) || (t_total > 0 && !T))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK && (t_total + 255) / 256 > ROUTE_MAX_GROUPS) rc = fail(FCPP_ESIZE, "2^39 transit entries or more");
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    if (rc) return rc;
    LAUNCHCHK(launch_route_transit(c->stream, n, swath_offsets, ax, ay, bx, by, angle, radius, mode, t_offsets, t_total, T));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_route_solve(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                     const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const double *T, const double *E, const double *X,
                     int n_starts, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *route, double *cost, int32_t *winner,
                     int32_t *sweeps, int32_t *status, double *stored)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!swath_offsets || !t_offsets || (t_total > 0 && !T)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_search(n_starts, min_gain, max_sweeps);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK && n > ROUTE_MAX_GROUPS / n_starts) rc = fail(FCPP_ESIZE, "2^31 (field, candidate) pairs or more");
    if (rc) return rc;
    // what the pick reads is the solve's own when the caller does not want it
    DevBuf<int32_t> own_tours, applied;
    DevBuf<double> own_costs, own_stored;
    if (!tours) { HIPCHK(own_tours.alloc((size_t)n_starts * (size_t)n_total)); tours = own_tours.p; }
    if (!costs) { HIPCHK(own_costs.alloc((size_t)n * (size_t)n_starts)); costs = own_costs.p; }
    if (!stored) { HIPCHK(own_stored.alloc((size_t)n)); stored = own_stored.p; }
    HIPCHK(applied.alloc((size_t)n * (size_t)n_starts));
    LAUNCHCHK(launch_route_solve(c->stream, n, n_starts, swath_offsets, n_total, t_offsets, T, E, X, min_gain, max_sweeps, tours, costs, applied.p,
                                 stored));
    LAUNCHCHK(launch_route_pick(c->stream, n, n_starts, swath_offsets, n_total, tours, costs, applied.p, stored, route, cost, winner, sweeps, status));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the temporaries die here)
    return FCPP_OK;
}

int fcpp_debug_route_transit(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                             const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total, double *T)
{
    if (!swath_offsets || !t_offsets || (n_total > 0 && (!ax || !ay || !bx || !by)) || (n > 0 && !angle) || (t_total > 0 && !T))
        return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_radius(radius, mode);
    if (rc) return rc;
    std::vector<int64_t> soff, toff;
    rc = route_offsets(nullptr, n, swath_offsets, nullptr, n_total, t_offsets, nullptr, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, angle, nullptr);
    if (rc) return rc;
    transit_twin(n, soff, toff, [&](int64_t i, int64_t s0, int p, int q, int64_t e, int64_t e2) {
        T[e] = T[e2] = mode == 0 ? route_transit<0>(ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q)
                                 : route_transit<1>(ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q);
    });
    return FCPP_OK;
}

int fcpp_debug_route(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                     const double *E, const double *X, int n_starts, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *route,
                     double *cost, int32_t *winner, int32_t *sweeps, int32_t *status, double *stored)
{
    if (!swath_offsets || !t_offsets || (t_total > 0 && !T)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = route_search(n_starts, min_gain, max_sweeps);
    if (rc) return rc;
    std::vector<int64_t> soff, toff;
    rc = route_offsets(nullptr, n, swath_offsets, nullptr, n_total, t_offsets, nullptr, t_total, soff, toff);
    if (rc == FCPP_OK && n > ROUTE_MAX_GROUPS / n_starts) rc = fail(FCPP_ESIZE, "2^31 (field, candidate) pairs or more");
    if (rc) return rc;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i];
        const RouteField f = route_field_host(T + toff[(size_t)i], E ? E + 2 * s0 : nullptr, X ? X + 2 * s0 : nullptr, soff[(size_t)i + 1] - s0, n_starts,
                                              min_gain, max_sweeps, tours ? tours + s0 : nullptr, n_total, costs ? costs + i * n_starts : nullptr,
                                              route ? route + s0 : nullptr);
        store(cost, i, f.cost); store(winner, i, f.winner); store(sweeps, i, f.sweeps); store(status, i, f.status); store(stored, i, f.stored);
    });
    return FCPP_OK;
}

int fcpp_route_transit_clear(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                             const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                             const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const int64_t *ring_offsets,
                             int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, double penalty,
                             double *T, uint8_t *B)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = transit_clear_args(swath_offsets, t_offsets, ring_offsets, vert_offsets, n, n_total, ax, ay, bx, by, angle, radius, mode, t_total, n_rings,
                                n_verts, x, y, penalty, T && B ? T : nullptr);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff, rings, verts, tile_off;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = clear_tiles(n, toff, tile_off);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    if (rc) return rc;
    DevBuf<int64_t> tiles;
    HIPCHK(tiles.alloc((size_t)n + 1));
    HIPCHK(hipMemcpyAsync(tiles.p, tile_off.data(), tile_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    LAUNCHCHK(launch_clear_transit(c->stream, n, swath_offsets, ax, ay, bx, by, angle, radius, mode, t_offsets, tiles.p, tile_off[(size_t)n], F, penalty,
                                   T, B));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the tile offsets die here)
    return FCPP_OK;
}

int fcpp_debug_route_transit_clear(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                   const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total,
                                   const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                   const double *y, double penalty, double *T, uint8_t *B)
{
    int rc = transit_clear_args(swath_offsets, t_offsets, ring_offsets, vert_offsets, n, n_total, ax, ay, bx, by, angle, radius, mode, t_total, n_rings,
                                n_verts, x, y, penalty, T && B ? T : nullptr);
    if (rc) return rc;
    std::vector<int64_t> soff, toff, rings, verts;
    rc = route_offsets(nullptr, n, swath_offsets, nullptr, n_total, t_offsets, nullptr, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, angle, nullptr);
    if (rc) return rc;
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    transit_twin(n, soff, toff, [&](int64_t i, int64_t s0, int p, int q, int64_t e, int64_t e2) {
        bool blocked = false;
        if ((p >> 1) != (q >> 1))
            blocked = mode == 0 ? clear_transit_blocked<0>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q)
                                : clear_transit_blocked<1>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, p, q);
        B[e] = B[e2] = blocked ? 1 : 0;
        if (blocked) { const double v = T[e] + penalty; T[e] = v; T[e2] = v; }
    });
    return FCPP_OK;
}

int fcpp_route_transit_priced(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                              const double *ax, const double *ay, const double *bx, const double *by, const double *angle, double radius, int mode,
                              const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const int64_t *ring_offsets,
                              int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, double penalty,
                              double *T, int8_t *K)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = transit_clear_args(swath_offsets, t_offsets, ring_offsets, vert_offsets, n, n_total, ax, ay, bx, by, angle, radius, mode, t_total, n_rings,
                                n_verts, x, y, penalty, T);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff, rings, verts, tile_off;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = clear_tiles(n, toff, tile_off);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle, nullptr);
    // (the second pass's grid: at most a workgroup per 4 listed entries, t_total / 2 of them)
    if (rc == FCPP_OK && t_total / 8 >= CLEAR_MAX_GROUPS) rc = fail(FCPP_ESIZE, "2^34 transit entries or more");
    if (rc) return rc;
    c->route_priced_listed = 0;
    if (n <= 0 || t_total <= 0) return FCPP_OK;
    DevBuf<int64_t> tiles, list;
    DevBuf<unsigned long long> count;
    const int64_t room = t_total / 2;                     // the canonical pairs of different swaths: half of a block less its 2 N own-swath entries
    HIPCHK(tiles.alloc((size_t)n + 1));
    HIPCHK(list.alloc((size_t)(room > 0 ? room : 1)));
    HIPCHK(count.alloc(1));
    HIPCHK(hipMemcpyAsync(tiles.p, tile_off.data(), tile_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), c->stream));
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    LAUNCHCHK(launch_route_priced_first(c->stream, n, swath_offsets, ax, ay, bx, by, angle, radius, mode, t_offsets, tiles.p, tile_off[(size_t)n], F,
                                        penalty, T, K, list.p, count.p));
    unsigned long long listed = 0;
    HIPCHK(hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (listed > (unsigned long long)room) return fail(FCPP_EHIP, "the first pass listed more entries than there are canonical pairs");
    c->route_priced_listed = (int64_t)listed;
    if (listed > 0) {
        LAUNCHCHK(launch_route_priced_words(c->stream, mode, (int64_t)listed, list.p, n, swath_offsets, ax, ay, bx, by, angle, radius, t_offsets, t_total,
                                            F, T, K));
        ++c->route_priced_word_launches;
    }
    HIPCHK(hipStreamSynchronize(c->stream));              // (the tile offsets and the list die here)
    return FCPP_OK;
}

int fcpp_ctx_route_priced_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->route_priced_listed;
    if (word_launches) *word_launches = c->route_priced_word_launches;
    return FCPP_OK;
}

int fcpp_debug_route_transit_priced(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                    const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total,
                                    const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                    const double *y, double penalty, double *T, int8_t *K)
{
    int rc = transit_clear_args(swath_offsets, t_offsets, ring_offsets, vert_offsets, n, n_total, ax, ay, bx, by, angle, radius, mode, t_total, n_rings,
                                n_verts, x, y, penalty, T);
    if (rc) return rc;
    std::vector<int64_t> soff, toff, rings, verts;
    rc = route_offsets(nullptr, n, swath_offsets, nullptr, n_total, t_offsets, nullptr, t_total, soff, toff);
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = swath_angles(nullptr, n, angle, nullptr);
    if (rc) return rc;
    const ClearFields F = { n, ring_offsets, vert_offsets, x, y };
    transit_twin(n, soff, toff, [&](int64_t i, int64_t s0, int p, int q, int64_t e, int64_t e2) {
        PricedTransit r = { INFINITY, 0, false };
        if ((p >> 1) != (q >> 1))
            r = mode == 0 ? priced_transit<0>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, penalty, p, q)
                          : priced_transit<1>(F, i, ax + s0, ay + s0, bx + s0, by + s0, angle[i], radius, penalty, p, q);
        T[e] = T[e2] = r.t;
        if (K) K[e] = K[e2] = (int8_t)r.rank;
    });
    return FCPP_OK;
}

}  // extern "C"
