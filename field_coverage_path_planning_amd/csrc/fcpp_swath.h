// fcpp_swath.h -- interface between the C-ABI glue (fcpp_glue_polygon.cpp) and the polygon swath kernels (fcpp_swath.hip): the counts and length
// sums of (field, angle) pairs, the CSR offsets of the fields' swaths, and the swath records at those offsets.  The rule is fcpp_swathfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

constexpr int64_t SWATH_MAX_PAIRS = 0x7fffffffLL;        // the grid: a workgroup per (field, angle)

// every launcher returns 0 or a hipError_t value.
// n x A pairs; the angle of pair (i, j) is angles[i] when per_field (A = 1), else angles[j].  n_swaths, n_lines, length, status: n x A, any
// may be NULL.
int launch_swath_count(hipStream_t st, int64_t n, int64_t A, int per_field, const int64_t *ring_offsets, const int64_t *vert_offsets,
                       const double *x, const double *y, const double *angles, double W, double first, double min_length, int32_t *n_swaths,
                       int32_t *n_lines, double *length, int32_t *status);
// out_offsets (n + 1) = the exclusive scan of n_swaths (the workgroup scan of fcpp_samplefn.h); err[0] stays 0
int launch_swath_offsets(hipStream_t st, int64_t n, const int32_t *n_swaths, int64_t *out_offsets, int64_t *err);
// the records of field i at offsets[i] .. offsets[i + 1] (never beyond); any output may be NULL
int launch_swath_fill(hipStream_t st, int64_t n, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x, const double *y,
                      const double *angles, double W, double first, double min_length, const int64_t *offsets, double *ax, double *ay, double *bx,
                      double *by, int32_t *line, double *length);

}  // namespace fcpp
