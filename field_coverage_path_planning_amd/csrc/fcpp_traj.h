// fcpp_traj.h -- interface between the C-ABI glue (fcpp_paths.cpp) and the trajectory kernels (fcpp_traj.hip):
// per-point arc length, time stamp and heading of caller-supplied paths (fcpp_trajectory) and their sampling at a fixed time step
// (fcpp_trajectory_counts / fcpp_trajectory_sample).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_device.h"

namespace fcpp {

// what one tile (block, path) contributes to the scan: the sums of its step lengths and step times, and the batch-global point index at
// which its last / first non-zero step starts (the heading's "nearest earlier direction" is the running maximum of those indices --
// an integer scan, exact in any order; the direction itself is taken from x, y at that index when a point needs it)
struct TrajAgg {
    double s, t;
    int64_t last;    // -1: the tile has no non-zero step
    int64_t first;   // INT64_MAX: likewise
};

// The spine is anchored at the path: a BLOCK is up to TRAJ_BLOCK_TILES consecutive tiles of ONE path, counted from the path's first
// tile, so the order in which a path's terms are added depends on the path alone -- not on where it lies in the batch.
constexpr int TRAJ_BLOCK_TILES = 256;
struct TrajBlock {
    int64_t tile0;   // first tile of the block in the tile table
    int32_t path;
    int32_t count;   // tiles, <= TRAJ_BLOCK_TILES
};

// every launcher returns 0 or a hipError_t value
// tiles: agg[tile] = the tile's own sums (relative to its first point) and first / last non-zero step
int launch_traj_tiles(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const double *x, const double *y,
                      const double *v, TrajAgg *agg);
// blocks: pre[tile] = what enters the tile, relative to its block's first tile; blk[block] = the block's own sums
int launch_traj_blocks(hipStream_t st, int64_t n_blocks, const TrajBlock *blocks, const TrajAgg *agg, TrajAgg *pre, TrajAgg *blk);
// paths: cin[block] = what enters the block, relative to the path's first point; path_first[path] = index of the path's first non-zero
// step; totals (may be NULL) = (length, time) per path
int launch_traj_paths(hipStream_t st, int64_t n_paths, const int64_t *block_first, const TrajAgg *blk, TrajAgg *cin, int64_t *path_first,
                      double *totals);
// apply: the tile-local scan again, with what enters the tile; s, t, heading may each be NULL; fs may be NULL
int launch_traj_apply(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const int64_t *tile_first,
                      const int64_t *block_first, const double *x, const double *y, const double *v, const uint32_t *fs, const TrajAgg *pre,
                      const TrajAgg *cin, const int64_t *path_first, double *s, double *t, double *heading);
// out_offsets (n_paths + 1) from the paths' total times; err[0] = paths whose time or sample count is out of range
int launch_traj_counts(hipStream_t st, int64_t n_paths, const double *totals, double dt, int include_end, int64_t *out_offsets, int64_t *err);
int launch_traj_sample(hipStream_t st, int64_t n_paths, const int64_t *offsets, const int64_t *out_offsets, int64_t total_samples, const double *x,
                       const double *y, const double *v, const double *s, const double *t, const double *heading, const uint32_t *fs, double dt,
                       int include_end, double *xs, double *ys, double *vs, double *ss, double *hs, uint32_t *fss, int64_t *src);

}  // namespace fcpp
