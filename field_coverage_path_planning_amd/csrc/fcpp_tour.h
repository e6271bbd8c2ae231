// fcpp_tour.h -- interface between the C-ABI glue (fcpp_glue_tour.cpp) and the cell tour's kernels (fcpp_tour.hip): the joint blocks of
// the fields' nodes, the candidate orders and the winner per field with its nodes.  The rule is fcpp_tourfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

constexpr int64_t TOUR_MAX_GROUPS = 0x7fffffffLL;        // the grids: a workgroup per (field, candidate), per 256 entries of D

// every launcher returns 0 or a hipError_t value.
// D[doff[f] ..): field f's block of N_f^2 entries; coff: the fields' cells (n + 1), voff: the cells' variants; ix .. oh: the variants' poses;
// d_total = doff[n]; mode 0 Dubins, 1 Reeds-Shepp
int launch_tour_transit(hipStream_t st, int64_t n, const int64_t *coff, const int64_t *voff, const double *ix, const double *iy, const double *ih,
                        const double *ox, const double *oy, const double *oh, double R, int mode, const int64_t *doff, int64_t d_total, double *D);
// n x S candidates: tours (S x n_cells, candidate-major), costs, applied (n x S) and stored (n), none NULL; w: per variant; stored_node: per
// cell or NULL; E, X: per node (field f's at 2 voff[coff[f]]) or NULL
int launch_tour_solve(hipStream_t st, int64_t n, int S, const int64_t *coff, int64_t n_cells, const int64_t *voff, const double *w,
                      const int32_t *stored_node, const int64_t *doff, const double *D, const double *E, const double *X, double min_gain,
                      int max_sweeps, int32_t *tours, double *costs, int32_t *applied, double *stored);
// order, node (n_cells), cost, stored, joint, winner, sweeps, skipped, status (n): any may be NULL; stored_in: launch_tour_solve's
int launch_tour_pick(hipStream_t st, int64_t n, int S, const int64_t *coff, int64_t n_cells, const int64_t *voff, const double *w,
                     const int32_t *stored_node, const int64_t *doff, const double *D, const double *E, const double *X, const int32_t *tours,
                     const double *costs, const int32_t *applied, const double *stored_in, int32_t *order, int32_t *node, double *cost,
                     double *stored, double *joint, int32_t *winner, int32_t *sweeps, int32_t *skipped, int32_t *status);

}  // namespace fcpp
