// fcpp_speed.h -- interface between the C-ABI glue (fcpp_glue_speed.cpp) and the path-speed kernels (fcpp_speed.hip): the speed profile
// of sampled paths from their kappa, part and gear (fcpp_path_speeds; the rule: fcpp_speedfn.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_device.h"
#include "fcpp_speedfn.h"

namespace fcpp {

// the five columns of a path set the rule reads
struct SpeedIn {
    const double *x, *y, *kappa;
    const int8_t *part, *gear;
};

// every launcher returns 0 or a hipError_t value
// tiles: agg_f / agg_b[tile] = the tile's composed map forwards / backwards (Agg of fcpp_devfn.h); status[path] = SPEED_EINVAL where a
// sample of the path fails (status is zeroed by the caller)
int launch_speed_tiles(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const SpeedRule &rule, const SpeedIn &in,
                       void *agg_f, void *agg_b, int32_t *status);
// (the spine between the two: launch_scan_spine, fcpp_device.h -- the maps are the speed planner's, whatever the steps weigh)
// apply: the tile-local scan again with what enters the tile from both sides; v, cap may each be NULL
int launch_speed_apply(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const SpeedRule &rule, const SpeedIn &in,
                       const double *carry_f, const double *carry_b, const int32_t *status, double *v, double *cap);

}  // namespace fcpp
