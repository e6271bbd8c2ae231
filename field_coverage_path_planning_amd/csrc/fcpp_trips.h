// fcpp_trips.h -- interface between the C-ABI glue (fcpp_glue_trips.cpp) and the service trips' kernel (fcpp_trips.hip): every field's routed
// tour split into capacity-limited round trips to a service point.  The rule is fcpp_tripfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

// what fcpp_trip_solve hands the kernel, every pointer the device's.  soff, toff: n + 1 each; T: the router's transit blocks; length: n_total;
// E, X (or NULL), In, Out: 2 n_total each, field i's at 2 soff[i]; tours: C x n_total, candidate-major; Q: n; Q0: n or NULL.
// Outputs, any may be NULL: tour, trip (n_total); n_trips, overfull, winner, status, cost, base, extra (n); costs (n x 2 C).
struct TripArgs {
    const int64_t *soff, *toff;
    const double *T, *length, *E, *X, *In, *Out;
    const int32_t *tours;
    const double *Q, *Q0;
    int64_t n_total;
    int C, both_ways;
    double stop;
    int32_t *tour, *trip, *n_trips, *overfull, *winner, *status;
    double *cost, *base, *extra, *costs;
};

// returns 0 or a hipError_t value
int launch_trip_solve(hipStream_t st, int64_t n, const TripArgs &a);

}  // namespace fcpp
