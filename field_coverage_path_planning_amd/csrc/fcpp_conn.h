// fcpp_conn.h -- interface between the C-ABI glue (fcpp_glue_conn.cpp) and the connector kernels (fcpp_conn.hip): the batched shortest-path
// solve, the all-pairs transit matrix, and the sampler of solved paths at a fixed spacing (Reeds-Shepp: run by run of one gear).
// mode 0 Dubins, 1 Reeds-Shepp; the interface of both is fcpp_connfn.h, the mathematics fcpp_dubinsfn.h / fcpp_rsfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

// tile of the matrix kernel: a workgroup solves CONN_ROWS "from" poses against CONN_COLS "to" poses
constexpr int CONN_COLS = 256, CONN_ROWS = 32;
constexpr int64_t CONN_MAX_POSES = (int64_t)1 << 20;     // per side of the matrix (the grid's second dimension)

// every launcher returns 0 or a hipError_t value; every output may be NULL.  seg: three (Dubins) or five signed (Reeds-Shepp) lengths per pair.
int launch_conn_solve(hipStream_t st, int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx,
                      const double *ty, const double *th, double R, int32_t *word, double *seg, double *len);
int launch_conn_matrix(hipStream_t st, int mode, int64_t n_from, const double *fx, const double *fy, const double *fh, int64_t n_to,
                       const double *tx, const double *ty, const double *th, double R, double *D, int8_t *word);
// out_offsets (n + 1) from the paths' lengths; err[0] = paths whose length is negative or infinite or whose sample count is out of range
int launch_dubins_counts(hipStream_t st, int64_t n, const double *len, double spacing, int64_t *out_offsets, int64_t *err);
// out_offsets (n + 1) from the paths' words and segments; err[0] = paths with a segment that is infinite or with 2^31 samples or more
int launch_rs_counts(hipStream_t st, int64_t n, const int32_t *word, const double *seg, double spacing, int64_t *out_offsets, int64_t *err);
// gears: the gear of every sample (fcpp_rs_sample; fcpp_dubins_sample has none and passes NULL)
int launch_conn_sample(hipStream_t st, int mode, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                       const double *seg, double spacing, const int64_t *out_offsets, int64_t total_samples, double *xs, double *ys, double *hs,
                       double *kappas, int8_t *gears);

}  // namespace fcpp
