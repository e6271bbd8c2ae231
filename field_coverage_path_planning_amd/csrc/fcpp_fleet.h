// fcpp_fleet.h -- interface between the C-ABI glue (fcpp_glue_fleet.cpp) and the vehicle shares' kernel (fcpp_fleet.hip): every field's routed
// tour split among at most K vehicles so that the last one finishes as early as possible.  The rule is fcpp_fleetfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

// what fcpp_fleet_solve hands the kernel, every pointer the device's.  soff, toff: n + 1 each; T: the router's transit blocks; length: n_total;
// In, Out: 2 n_total each, field i's at 2 soff[i]; tours: C x n_total, candidate-major; K: n.
// Outputs, any may be NULL: tour, share (n_total); n_used, winner, status, makespan, total (n); makespans, totals (n x 2 C); share_first,
// share_cost (n x k_stride).
struct FleetArgs {
    const int64_t *soff, *toff;
    const double *T, *length, *In, *Out;
    const int32_t *tours;
    const int32_t *K;
    int64_t n_total;
    int C, both_ways, k_stride;
    double omega;
    int32_t *tour, *share, *n_used, *winner, *status;
    double *makespan, *total, *makespans, *totals;
    int32_t *share_first;
    double *share_cost;
};

// max_m: the most swaths of a field of the batch that has a block (m <= ROUTE_MAX_SWATHS); returns 0 or a hipError_t value
int launch_fleet_solve(hipStream_t st, int64_t n, int64_t max_m, const FleetArgs &a);

}  // namespace fcpp
