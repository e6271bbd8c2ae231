// fcpp_regions.h -- interface between the C-ABI glue (fcpp_glue_cover.cpp) and the coverage-region kernels (fcpp_regions.hip): the labelling of
// the fields' tiles, the merge over the tile seams, the numbering of the regions and their records.  The rule is fcpp_regionfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_regionfn.h"

namespace fcpp {

// the fields of a call, device pointers: the caller's grids and where the glue's checked tables place their tiles and numbering blocks
struct RegionFields {
    const RegionDims *dims;                      // n
    const int64_t *cell_first;                   // n + 1: the caller's cell_offsets
    const int64_t *tile_first;                   // n + 1: 64 x 64 tiles, row-major per field
    const int64_t *block_first;                  // n + 1: numbering blocks of REGION_BLOCK_CELLS cells, cut at the fields
};

// every launcher returns 0 or a hipError_t value
// a workgroup per tile: labels = every member's tile root (its field-local index), -1 for a non-member
int launch_region_tiles(hipStream_t st, int64_t n, int64_t n_tiles, const RegionFields &f, const uint8_t *grid, int mask, int value,
                        int connectivity, int32_t *labels);
// the unions over the tiles' first columns and rows; at most max_blocks workgroups stride over them (the context's compute units decide)
int launch_region_seams(hipStream_t st, int64_t n, int64_t n_tiles, const RegionFields &f, int connectivity, int32_t *labels, int max_blocks);
// a workgroup per numbering block: flatten != 0: every member's label becomes its root; block_count (one per block) = the block's roots
int launch_region_count(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, int flatten, int32_t *labels, int64_t *block_count);
// block_prefix (n_blocks + 1) = the exclusive scan of block_count (the samplers' scan; err: one word of scratch); region_offsets (n + 1, or
// NULL) = the roots before every field's first block
int launch_region_offsets(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, const int64_t *block_count, int64_t *block_prefix,
                          int64_t *err, int64_t *region_offsets);
// the roots write their records' keys and seed the boxes (records zeroed before); then every member joins its record and takes its index
int launch_region_first(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, const int32_t *labels, const int64_t *block_prefix,
                        const int64_t *region_offsets, RegionRecord *records);
int launch_region_fill(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, int32_t *labels, const int64_t *region_offsets,
                       RegionRecord *records);

}  // namespace fcpp
