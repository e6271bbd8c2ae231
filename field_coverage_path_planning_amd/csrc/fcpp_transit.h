// fcpp_transit.h -- interface between the C-ABI glue (fcpp_glue_legs.cpp) and the loop-transit kernels (fcpp_transit.hip).  The rule is
// fcpp_transitfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_transitfn.h"

namespace fcpp {

constexpr int TRANSIT_BLOCK = 256;                       // threads of a workgroup of every kernel; the pick pass's tile of stations

// the pairs and what is written per pair; any output may be NULL.  seg: NSEG per pair
struct TransitIo {
    const double *fx, *fy, *fh, *tx, *ty, *th;
    const int64_t *pair_field;
    int32_t *found;
    int64_t *loop, *i, *j;
    int32_t *in_word;
    double *in_seg, *in_len;
    int32_t *in_rank, *out_word;
    double *out_seg, *out_len;
    int32_t *out_rank;
    double *ride, *total;
    int32_t *status;
};

// the call's temporaries, on the device.  st_idx, st_loop: room for every sample (a field's stations at the place of its first sample);
// n_st, loops_ok, region_status: per field; val: n x 2 x per doubles (in then out of every pair); pick_*: per pair
struct TransitTemp {
    int64_t *st_idx, *st_loop, *n_st;
    int32_t *loops_ok;
    const int32_t *region_status;
    double *val;
    int64_t *pick_l, *pick_i, *pick_j;
};

// every launcher returns 0 or a hipError_t value.  L, F hold device pointers whose offsets the caller has checked.
// a wavefront per field: its stations in order, their number, whether its loops are valid
int launch_transit_stations(hipStream_t st, const TransitLoops &L, const TransitTemp &T);
// Stations pass, first launch: a lane per (pair, side, station slot below per): solve_clear_first; val gets the len (+inf unless rank 0),
// the lanes whose other words have to be looked at are appended to list (room for n x 2 x per), their number added to *count (zeroed).
int launch_transit_sides(hipStream_t st, int mode, int64_t n, int64_t per, const TransitIo &io, double R, const ClearFields &F, const TransitLoops &L,
                         const TransitTemp &T, int64_t *list, unsigned long long *count);
// second launch, a group of lanes per listed entry (8 for mode 0, 64 for mode 1), a lane per word: a clear winner's total into val
int launch_transit_words(hipStream_t st, int mode, int64_t count, const int64_t *list, int64_t n, int64_t per, const TransitIo &io, double R,
                         const ClearFields &F, const TransitLoops &L, const TransitTemp &T);
// Pick pass, a workgroup per pair; then a lane per pair: the result (transit_finish)
int launch_transit_pick(hipStream_t st, int64_t n, int64_t per, const TransitIo &io, const TransitLoops &L, const TransitTemp &T);
int launch_transit_finish(hipStream_t st, int mode, int64_t n, const TransitIo &io, double R, const ClearFields &F, const TransitLoops &L,
                          const TransitTemp &T);
// the scan of the pairs' sample counts (fcpp_samplefn.h); err[0]: the pairs of 2^31 samples or more
int launch_transit_counts(hipStream_t st, int mode, int64_t n, const TransitRec &rec, int64_t n_loops, const int64_t *loop_off, double spacing,
                          int64_t *out_offsets, int64_t *err);
// a lane per output sample; every output may be NULL
int launch_transit_fill(hipStream_t st, int mode, int64_t n, const TransitRec &rec, const TransitLoops &L, const double *fx, const double *fy,
                        const double *fh, double R, double spacing, const int64_t *out_offsets, int64_t total_samples, double *x, double *y,
                        double *heading, double *kappa, int8_t *part, int8_t *gear);

}  // namespace fcpp
