// fcpp_dubins.h -- interface between the C-ABI glue (fcpp_paths.cpp) and the Dubins kernels (fcpp_dubins.hip): the batched shortest-path
// solve, the all-pairs transit matrix, and the sampler of solved paths at a fixed spacing.  The mathematics is fcpp_dubinsfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

// tile of the matrix kernel: a workgroup solves DUB_ROWS "from" poses against DUB_COLS "to" poses
constexpr int DUB_COLS = 256, DUB_ROWS = 32;
constexpr int64_t DUB_MAX_POSES = (int64_t)1 << 20;      // per side of the matrix (the grid's second dimension)

// every launcher returns 0 or a hipError_t value; every output may be NULL
int launch_dubins_solve(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty,
                        const double *th, double R, int32_t *word, double *seg, double *len);
int launch_dubins_matrix(hipStream_t st, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to, const double *tx,
                         const double *ty, const double *th, double R, double *D, int8_t *word);
// out_offsets (n + 1) from the paths' lengths; err[0] = paths whose length is negative or infinite or whose sample count is out of range
int launch_dubins_counts(hipStream_t st, int64_t n, const double *len, double spacing, int64_t *out_offsets, int64_t *err);
int launch_dubins_sample(hipStream_t st, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                         const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                         double *kappas);

}  // namespace fcpp
