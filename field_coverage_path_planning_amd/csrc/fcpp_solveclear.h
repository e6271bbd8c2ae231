// fcpp_solveclear.h -- interface between the C-ABI glue (fcpp_paths.cpp) and the clear-connector kernels (fcpp_solveclear.hip).  The rule is
// fcpp_solveclearfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_solveclearfn.h"

namespace fcpp {

constexpr int SOLVECLEAR_BLOCK = 256;                    // threads of a workgroup of both kernels

// the poses of the pairs and what is written per pair; any output may be NULL
struct SolveClearIo {
    const double *fx, *fy, *fh, *tx, *ty, *th;
    const int64_t *pair_field;
    int32_t *word;
    double *seg, *len;
    int32_t *rank, *crossings;
};

// every launcher returns 0 or a hipError_t value.  F: the fields' CSR on the device, checked by the caller.
// First pass, a lane per pair: every pair's result, and the pairs whose other words have to be looked at appended to list (room for n),
// their number added to *count (zeroed by the caller).
int launch_solve_clear_pairs(hipStream_t st, int mode, int64_t n, const SolveClearIo &io, double R, const ClearFields &F, int64_t *list,
                             unsigned long long *count);
// Second pass, a group of lanes per listed pair (8 for mode 0, 64 for mode 1), a lane per word.
int launch_solve_clear_words(hipStream_t st, int mode, int64_t count, const int64_t *list, const SolveClearIo &io, double R, const ClearFields &F);

}  // namespace fcpp
