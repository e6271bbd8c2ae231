// fcpp_inset.h -- interface between the C-ABI glue (fcpp_glue_polygon.cpp) and the polygon inset kernels (fcpp_inset.hip): the ring and vertex
// counts of (field, distance) pairs, their CSR offsets, and the rings at those offsets.  The rule is fcpp_insetfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fcpp {

constexpr int64_t INSET_MAX_PAIRS = 0x7fffffffLL;        // a workgroup per (field, distance)
constexpr int INSET_SMALL_EDGES = 64;                    // up to here a pair is one wavefront with its pieces in LDS
constexpr int64_t INSET_LAUNCH_PAIRS = 1024;             // beyond: pairs per launch, each with a slab of piece records in device memory

// the device memory the piece records of one launch need: `doubles` float64 and `ints` int32 (0, 0 when every field is small)
void inset_scratch_size(int max_edges, int64_t n_pairs, size_t &doubles, size_t &ints);

// every launcher returns 0 or a hipError_t value.  max_edges: the most edges of any field of at most INSET_MAX_EDGES.
// n x D pairs, row-major; the distance of pair (i, j) is dist[j].  n_rings, n_verts (int32), status (int32), gap (float64): n x D; status
// and gap may be NULL.
int launch_inset_count(hipStream_t st, int64_t n, int64_t D, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets,
                       const double *x, const double *y, const double *dist, double arc_step, double *scratch_d, int32_t *scratch_i,
                       int32_t *n_rings, int32_t *n_verts, int32_t *status, double *gap);
// out_offsets (m + 1) = the exclusive scan of counts (the workgroup scan of fcpp_samplefn.h); err[0] stays 0
int launch_inset_offsets(hipStream_t st, int64_t m, const int32_t *counts, int64_t *out_offsets, int64_t *err);
// the rings of pair p at pair_ring_offsets[p] .. [p + 1] and its vertices at pair_vert_offsets[p] .. [p + 1] (never beyond); any output
// may be NULL
int launch_inset_fill(hipStream_t st, int64_t n, int64_t D, int max_edges, const int64_t *ring_offsets, const int64_t *vert_offsets,
                      const double *x, const double *y, const double *dist, double arc_step, double *scratch_d, int32_t *scratch_i,
                      const int64_t *pair_ring_offsets, const int64_t *pair_vert_offsets, int64_t total_rings, int64_t total_verts,
                      int64_t *out_vert_offsets, double *out_x, double *out_y, int32_t *out_src);

}  // namespace fcpp
