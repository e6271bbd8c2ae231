// fcpp_fpath.h -- interface between the C-ABI glue (fcpp_paths.cpp) and the field-path kernels (fcpp_fpath.hip): the leg records of every
// field's slots, the sample offsets per slot and per field with the fields' totals, and the samples.  The rule is fcpp_fpathfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_fpathfn.h"

namespace fcpp {

// every launcher returns 0 or a hipError_t value.  n_slots = 2 n_total + n; `in` holds device pointers.
// legs, cnt (n_slots): every slot's record and sample count; seen (n_total int32, zeroed) and status (n int32, zeroed): the order's
// validation and the fields' status -- both NULL: records only (the fill's pass)
int launch_fpath_legs(hipStream_t st, int64_t n, int64_t n_total, const FpathIn &in, int mode, FpathLeg *legs, int64_t *cnt, int32_t *seen,
                      int32_t *status);
// leg_off (n_slots + 1): the scan of the counts, a failed field's as 0; err[0]: the legs and fields of 2^31 samples or more.  path_off
// (n + 1), work, transit (n; either may be NULL)
int launch_fpath_offsets(hipStream_t st, int64_t n, int64_t n_total, const int64_t *soff, const FpathLeg *legs, const int64_t *cnt,
                         const int32_t *status, int has_entry, int has_exit, int64_t *leg_off, int64_t *path_off, double *work, double *transit,
                         int64_t *err);
// a lane per sample; every output may be NULL
int launch_fpath_fill(hipStream_t st, int64_t n_slots, const FpathLeg *legs, const int64_t *leg_off, int64_t total_samples, double R,
                      double spacing, double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg);

}  // namespace fcpp
