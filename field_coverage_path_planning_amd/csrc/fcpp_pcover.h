// fcpp_pcover.h -- interface between the C-ABI glue (fcpp_glue_cover.cpp) and the polygon-coverage kernels (fcpp_pcover.hip): the fields' grids and
// status, the offsets of their cells and tiles, the bounding boxes of the paths' chunks, and the tiles' rasterisation.  The rule is
// fcpp_pcoverfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_pcoverfn.h"

namespace fcpp {

// a chunk of a path: at most PCOVER_CHUNK consecutive segments (first, first + 1) .. of the path that owns the samples [p0, p1)
struct PcoverChunk {
    int64_t first, p0, p1;
    int32_t count, path;
};

struct PcoverBox {         // of a chunk's working segments; inverted (never hit) when it has none
    double x0, y0, x1, y1;
};

// the fields of a call, device pointers: the caller's CSR and what the sizes pass made of it
struct PcoverFields {
    const int64_t *ring_offsets, *vert_offsets;
    const double *x, *y;
    const PcoverDims *dims;
    const int64_t *cell_first, *tile_first;      // n + 1 each
    const int64_t *chunk_first;                  // n + 1: field i tests the chunks chunk_first[i] .. chunk_first[i + 1]
};

// every launcher returns 0 or a hipError_t value
// a wavefront per field: dims, status (n each)
int launch_pcover_sizes(hipStream_t st, int64_t n, const int64_t *ring_offsets, const int64_t *vert_offsets, const double *x, const double *y,
                        double W, double res, PcoverDims *dims, int32_t *status);
// cell_first, tile_first (n + 1 each; either may be NULL): the scans of the fields' cells and 64 x 64 tiles; err: one word of scratch
int launch_pcover_offsets(hipStream_t st, int64_t n, const PcoverDims *dims, int64_t *cell_first, int64_t *tile_first, int64_t *err);
// a workgroup per chunk
int launch_pcover_boxes(hipStream_t st, int64_t n_chunks, const PcoverChunk *chunks, const PcoverPaths &paths, PcoverBox *boxes);
// a workgroup per tile; grid may be NULL; counts (4 n, zeroed by the caller)
int launch_pcover_tiles(hipStream_t st, int64_t n, int64_t n_tiles, const PcoverFields &f, double W, double res, int caps, const PcoverChunk *chunks,
                        const PcoverBox *boxes, const PcoverPaths &paths, uint8_t *grid, unsigned long long *counts);

}  // namespace fcpp
