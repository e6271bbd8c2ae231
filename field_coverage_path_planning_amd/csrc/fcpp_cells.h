// fcpp_cells.h -- interface between the C-ABI glue (fcpp_glue_cells.cpp) and the field cell kernels (fcpp_cells.hip): the cell and vertex
// counts of every field, their CSR offsets, and the cells at those offsets.  The rule is fcpp_cellfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

constexpr int CELL_SMALL_EDGES = 64;                     // up to here a field is one wavefront; beyond, four

// every launcher returns 0 or a hipError_t value.  max_edges: the most edges of any field of at most CELL_MAX_EDGES.  A workgroup per
// field, every table in LDS: a launch takes the whole batch.
// n_cells, n_verts, status, n_cuts, dropped (int32), dropped_area (float64): n each; any but n_cells and n_verts may be NULL.
int launch_cells_count(hipStream_t st, int64_t n, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x,
                       const double *y, const double *angle, int events, double min_area, int32_t *n_cells, int32_t *n_verts, int32_t *status,
                       int32_t *n_cuts, int32_t *dropped, double *dropped_area);
// out_offsets (n + 1) = the exclusive scan of counts (the workgroup scan of fcpp_samplefn.h); err[0] stays 0
int launch_cells_offsets(hipStream_t st, int64_t n, const int32_t *counts, int64_t *out_offsets, int64_t *err);
// the cells of field i at cell_offsets[i] .. [i + 1] and their vertices at fvert_offsets[i] .. [i + 1] (never beyond); any output may be NULL
int launch_cells_fill(hipStream_t st, int64_t n, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x,
                      const double *y, const double *angle, int events, double min_area, const int64_t *cell_offsets,
                      const int64_t *fvert_offsets, int64_t total_cells, int64_t total_verts, int64_t *out_vert_offsets, double *out_x,
                      double *out_y, int32_t *out_src, int32_t *cell_field, double *area);

}  // namespace fcpp
