// fcpp_route.h -- interface between the C-ABI glue (fcpp_glue_route.cpp) and the swath router's kernels (fcpp_route.hip): the transit blocks
// of the fields' oriented swaths, the candidate tours and the winner per field.  The rule is fcpp_routefn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

constexpr int64_t ROUTE_MAX_GROUPS = 0x7fffffffLL;       // the grids: a workgroup per (field, candidate), per 256 entries of T

// every launcher returns 0 or a hipError_t value.
// T[toff[i] ..): field i's block of (2 m_i)^2 entries, m_i = soff[i + 1] - soff[i]; t_total = toff[n]; mode 0 Dubins, 1 Reeds-Shepp
int launch_route_transit(hipStream_t st, int64_t n, const int64_t *soff, const double *ax, const double *ay, const double *bx, const double *by,
                         const double *angle, double R, int mode, const int64_t *toff, int64_t t_total, double *T);
// n x S candidates: tours (S x n_total, candidate-major), costs, applied (n x S) and stored (n: candidate 0's cost as constructed), none NULL;
// E, X: 2 n_total each (field i's at 2 soff[i]) or NULL
int launch_route_solve(hipStream_t st, int64_t n, int S, const int64_t *soff, int64_t n_total, const int64_t *toff, const double *T,
                       const double *E, const double *X, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *applied,
                       double *stored);
// route (n_total), cost, winner, sweeps, status (n): any may be NULL
int launch_route_pick(hipStream_t st, int64_t n, int S, const int64_t *soff, int64_t n_total, const int32_t *tours, const double *costs,
                      const int32_t *applied, const double *stored, int32_t *route, double *cost, int32_t *winner, int32_t *sweeps,
                      int32_t *status);

}  // namespace fcpp
