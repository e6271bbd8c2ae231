// fcpp_hpath.h -- interface between the C-ABI glue (fcpp_paths.cpp) and the headland-path kernels (fcpp_hpath.hip): the leg records of every
// ring's slots, the rings' status, the sample offsets per slot and per ring with the rings' totals, and the samples.  The rule is
// fcpp_hpathfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_hpathfn.h"

namespace fcpp {

// every launcher returns 0 or a hipError_t value.  n_slots = 2 n_verts; `in` holds device pointers.
// legs, cnt (n_slots): every slot's record and sample count; status, drivable (n_rings int32, zeroed): the rings' status and whether a ring
// has a drivable element -- cnt, status and drivable all NULL: records only (the fill's pass)
int launch_hpath_legs(hipStream_t st, int64_t n_rings, int64_t n_verts, const HpathIn &in, int mode, HpathLeg *legs, int64_t *cnt, int32_t *status,
                      int32_t *drivable);
// the rings' final status (a ring of fewer than two vertices, a ring without a drivable element), the counts of failed rings set to 0;
// leg_off (n_slots + 1): the scan of the counts; err[0]: the legs and rings of 2^31 samples or more.  path_off (n_rings + 1), work, transit,
// skipped (n_rings; each may be NULL)
int launch_hpath_offsets(hipStream_t st, int64_t n_rings, int64_t n_verts, const int64_t *roff, const HpathLeg *legs, int64_t *cnt, int32_t *status,
                         const int32_t *drivable, int64_t *leg_off, int64_t *path_off, double *work, double *transit, double *skipped, int64_t *err);
// a lane per sample; every output may be NULL
int launch_hpath_fill(hipStream_t st, int64_t n_slots, const HpathLeg *legs, const int64_t *leg_off, int64_t total_samples, double R, double spacing,
                      double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg);

}  // namespace fcpp
