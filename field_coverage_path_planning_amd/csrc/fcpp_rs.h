// fcpp_rs.h -- interface between the C-ABI glue (fcpp_paths.cpp) and the Reeds-Shepp kernels (fcpp_rs.hip): the batched shortest-path
// solve, the all-pairs transit matrix, and the sampler of solved paths at a fixed spacing, run by run of one gear.  The mathematics is
// fcpp_rsfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

// tile of the matrix kernel: a workgroup solves RS_ROWS "from" poses against RS_COLS "to" poses
constexpr int RS_COLS = 256, RS_ROWS = 32;
constexpr int64_t RS_MAX_POSES = (int64_t)1 << 20;       // per side of the matrix (the grid's second dimension)

// every launcher returns 0 or a hipError_t value; every output may be NULL.  seg: five signed lengths per pair.
int launch_rs_solve(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                    const double *th, double R, int32_t *word, double *seg, double *len);
int launch_rs_matrix(hipStream_t st, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                     const double *ty, const double *th, double R, double *D, int8_t *word);
// out_offsets (n + 1) from the paths' words and segments; err[0] = paths with a segment that is infinite or with 2^31 samples or more
int launch_rs_counts(hipStream_t st, int64_t n, const int32_t *word, const double *seg, double spacing, int64_t *out_offsets, int64_t *err);
int launch_rs_sample(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                     const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                     double *kappas, int8_t *gears);

}  // namespace fcpp
