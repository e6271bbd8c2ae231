// fcpp_glue_trips.cpp -- C-ABI glue of the service trips and their host twin (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_parallel.h"
#include "fcpp_tripfn.h"
#include "fcpp_trips.h"

using namespace fcpp;

namespace {
// ---- what fcpp_trip_solve and its host twin check alike before the offsets ----------------------------------------------------------------
int trip_args(int64_t n, const void *swath_offsets, int64_t n_total, const void *t_offsets, int64_t t_total, const void *T, const void *length,
              const void *In, const void *Out, int n_cand, const void *tours, int both_ways, const void *capacity, double stop_cost)
{
    if (!swath_offsets || !t_offsets || (t_total > 0 && !T) || (n_total > 0 && (!length || !In || !Out || !tours)) || (n > 0 && !capacity))
        return fail(FCPP_EINVAL, "bad arguments");
    if (n_cand < 1 || n_cand > TRIP_MAX_CANDIDATES) return fail(FCPP_EINVAL, "n_cand must lie in 1 .. 64");
    if (!(stop_cost >= 0.0) || !isfinite(stop_cost)) return fail(FCPP_EINVAL, "stop_cost must be non-negative and finite");
    if (both_ways != 0 && both_ways != 1) return fail(FCPP_EINVAL, "both_ways must be 0 or 1");
    return FCPP_OK;
}
}  // namespace

extern "C" {

// ---- service trips (fcpp_trips.hip; the rule: fcpp_tripfn.h) ----------------------------------------------------------------------------
int fcpp_trip_solve(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                    const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const double *T, const double *length, const double *E,
                    const double *X, const double *In, const double *Out, int n_cand, const int32_t *tours, int both_ways, const double *capacity,
                    const double *first_capacity, double stop_cost, int32_t *tour, int32_t *trip, int32_t *n_trips, int32_t *overfull,
                    int32_t *winner, int32_t *status, double *cost, double *base, double *extra, double *costs)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = trip_args(n, swath_offsets, n_total, t_offsets, t_total, T, length, In, Out, n_cand, tours, both_ways, capacity, stop_cost);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc) return rc;
    const TripArgs a = { swath_offsets, t_offsets, T, length, E, X, In, Out, tours, capacity, first_capacity, n_total, n_cand, both_ways, stop_cost,
                         tour, trip, n_trips, overfull, winner, status, cost, base, extra, costs };
    LAUNCHCHK(launch_trip_solve(c->stream, n, a));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_trip_solve(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                          const double *length, const double *E, const double *X, const double *In, const double *Out, int n_cand,
                          const int32_t *tours, int both_ways, const double *capacity, const double *first_capacity, double stop_cost, int32_t *tour,
                          int32_t *trip, int32_t *n_trips, int32_t *overfull, int32_t *winner, int32_t *status, double *cost, double *base,
                          double *extra, double *costs)
{
    int rc = trip_args(n, swath_offsets, n_total, t_offsets, t_total, T, length, In, Out, n_cand, tours, both_ways, capacity, stop_cost);
    if (rc) return rc;
    std::vector<int64_t> soff, toff;
    rc = route_offsets(nullptr, n, swath_offsets, nullptr, n_total, t_offsets, nullptr, t_total, soff, toff);
    if (rc) return rc;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i], m64 = soff[(size_t)i + 1] - s0;
        const TripField F = { T + toff[(size_t)i], E ? E + 2 * s0 : nullptr, X ? X + 2 * s0 : nullptr, In + 2 * s0, Out + 2 * s0, length + s0, tours + s0,
                              n_total, m64 > ROUTE_MAX_SWATHS ? 0 : (int)m64, n_cand, both_ways, capacity[i], first_capacity ? first_capacity[i] : capacity[i],
                              stop_cost };
        const TripResult r = trip_field_host(F, m64, tour ? tour + s0 : nullptr, trip ? trip + s0 : nullptr, costs ? costs + i * 2 * n_cand : nullptr);
        store(cost, i, r.cost); store(base, i, r.base); store(extra, i, r.extra); store(n_trips, i, r.n_trips); store(overfull, i, r.overfull);
        store(winner, i, r.winner); store(status, i, r.status);
    });
    return FCPP_OK;
}

}  // extern "C"
