// fcpp_glue_fleet.cpp -- C-ABI glue of the vehicle shares and their host twin (what the glue files do and share: fcpp_glue.h).
#include "fcpp_fleet.h"
#include "fcpp_fleetfn.h"
#include "fcpp_glue.h"
#include "fcpp_parallel.h"

using namespace fcpp;

namespace {
// ---- what fcpp_fleet_solve and its host twin check alike before the offsets ---------------------------------------------------------------
int fleet_args(int64_t n, const void *swath_offsets, int64_t n_total, const void *t_offsets, int64_t t_total, const void *T, const void *length,
               const void *In, const void *Out, int n_cand, const void *tours, int both_ways, const void *vehicles, int k_stride, double work_weight)
{
    if (!swath_offsets || !t_offsets || (t_total > 0 && !T) || (n_total > 0 && (!length || !In || !Out || !tours)) || (n > 0 && !vehicles))
        return fail(FCPP_EINVAL, "bad arguments");
    if (n_cand < 1 || n_cand > TRIP_MAX_CANDIDATES) return fail(FCPP_EINVAL, "n_cand must lie in 1 .. 64");
    if (k_stride < 1 || k_stride > FLEET_MAX_VEHICLES) return fail(FCPP_EINVAL, "k_stride must lie in 1 .. 16");
    if (!(work_weight >= 0.0) || !isfinite(work_weight)) return fail(FCPP_EINVAL, "work_weight must be non-negative and finite");
    if (both_ways != 0 && both_ways != 1) return fail(FCPP_EINVAL, "both_ways must be 0 or 1");
    return FCPP_OK;
}
}  // namespace

extern "C" {

// ---- vehicle shares (fcpp_fleet.hip; the rule: fcpp_fleetfn.h) --------------------------------------------------------------------------
int fcpp_fleet_solve(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                     const int64_t *t_offsets, const int64_t *t_offsets_host, int64_t t_total, const double *T, const double *length, const double *In,
                     const double *Out, int n_cand, const int32_t *tours, int both_ways, const int32_t *vehicles, int k_stride, double work_weight,
                     int32_t *tour, int32_t *share, int32_t *n_used, int32_t *winner, int32_t *status, double *makespan, double *total,
                     double *makespans, double *totals, int32_t *share_first, double *share_cost)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = fleet_args(n, swath_offsets, n_total, t_offsets, t_total, T, length, In, Out, n_cand, tours, both_ways, vehicles, k_stride, work_weight);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, toff;
    rc = route_offsets(c, n, swath_offsets, swath_offsets_host, n_total, t_offsets, t_offsets_host, t_total, soff, toff);
    if (rc) return rc;
    const FleetArgs a = { swath_offsets, t_offsets, T, length, In, Out, tours, vehicles, n_total, n_cand, both_ways, k_stride, work_weight,
                          tour, share, n_used, winner, status, makespan, total, makespans, totals, share_first, share_cost };
    int64_t max_m = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t m = soff[(size_t)i + 1] - soff[(size_t)i];
        if (m <= ROUTE_MAX_SWATHS && m > max_m) max_m = m;
    }
    LAUNCHCHK(launch_fleet_solve(c->stream, n, max_m, a));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_fleet_solve(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                           const double *length, const double *In, const double *Out, int n_cand, const int32_t *tours, int both_ways,
                           const int32_t *vehicles, int k_stride, double work_weight, int32_t *tour, int32_t *share, int32_t *n_used,
                           int32_t *winner, int32_t *status, double *makespan, double *total, double *makespans, double *totals,
                           int32_t *share_first, double *share_cost)
{
    int rc = fleet_args(n, swath_offsets, n_total, t_offsets, t_total, T, length, In, Out, n_cand, tours, both_ways, vehicles, k_stride, work_weight);
    if (rc) return rc;
    std::vector<int64_t> soff, toff;
    rc = route_offsets(nullptr, n, swath_offsets, nullptr, n_total, t_offsets, nullptr, t_total, soff, toff);
    if (rc) return rc;
    WorkerPool::parallel_for(n, [&](int64_t i) {
        const int64_t s0 = soff[(size_t)i], m64 = soff[(size_t)i + 1] - s0;
        const FleetField F = { T + toff[(size_t)i], In + 2 * s0, Out + 2 * s0, length + s0, tours + s0, n_total, m64 > ROUTE_MAX_SWATHS ? 0 : (int)m64,
                               n_cand, both_ways, vehicles[i], k_stride, work_weight };
        const FleetResult r = fleet_field_host(F, m64, tour ? tour + s0 : nullptr, share ? share + s0 : nullptr,
                                               makespans ? makespans + i * 2 * n_cand : nullptr, totals ? totals + i * 2 * n_cand : nullptr,
                                               share_first ? share_first + i * k_stride : nullptr, share_cost ? share_cost + i * k_stride : nullptr);
        store(makespan, i, r.makespan); store(total, i, r.total); store(n_used, i, r.n_used); store(winner, i, r.winner); store(status, i, r.status);
    });
    return FCPP_OK;
}

}  // extern "C"
