// fcpp_legs.h -- interface between the C-ABI glue (fcpp_glue_legs.cpp) and the kernels of the leg-path operators (fcpp_legs.hip): the field paths
// (rule and leg set: fcpp_fpathfn.h, FieldLegs) and the headland paths (fcpp_hpathfn.h, RingLegs).  Both are records -> scan -> groups ->
// samples: a group (a field, a ring) owns a run of leg slots, a rule kernel writes a record and a sample count per slot, the counts are
// scanned into slot offsets, a lane per group writes its path offset and totals, a lane per sample evaluates its slot's record.  Only the
// rule kernels (launch_legs) and what precedes the scan (launch_leg_offsets) are an operator's own.  The clear field paths put one stage
// between the fields' records and the scan (fcpp_solveclear.h: launch_fpath_clear_*); nothing here changes for it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_fpathfn.h"
#include "fcpp_hpathfn.h"

namespace fcpp {

// a group's totals, one array per total of the leg set (P::N_TOTALS of them; each may be NULL)
struct LegTotals {
    double *p[3];
};

// every launcher returns 0 or a hipError_t value; `in` holds device pointers.  n_slots = 2 n_total + n (fields) / 2 n_verts (rings).
// legs, cnt (n_slots): every slot's record and sample count.  status (n_groups int32, zeroed): the groups' status.  scratch (int32, zeroed):
// the order's validation, a counter per swath (fields: n_total) / whether a ring has a drivable element (rings: n_rings).  cnt, scratch
// and status all NULL: records only (the fill's pass).
int launch_legs(hipStream_t st, int64_t n, int64_t n_slots, const FpathIn &in, int mode, FpathLeg *legs, int64_t *cnt, int32_t *scratch, int32_t *status);
int launch_legs(hipStream_t st, int64_t n_rings, int64_t n_slots, const HpathIn &in, int mode, HpathLeg *legs, int64_t *cnt, int32_t *scratch,
                int32_t *status);
// leg_off (n_slots + 1): the scan of the counts, a failed group's as 0; err[0]: the legs and groups of 2^31 samples or more; path_off
// (n_groups + 1) and the totals.  The rings' status becomes final here (a ring of fewer than two vertices, a ring without a drivable
// element) and the counts of failed rings are set to 0; the fields' are left as they are.
int launch_leg_offsets(hipStream_t st, int64_t n, int64_t n_slots, const FpathIn &in, const FpathLeg *legs, int64_t *cnt, int32_t *status,
                       const int32_t *scratch, int64_t *leg_off, int64_t *path_off, const LegTotals &totals, int64_t *err);
int launch_leg_offsets(hipStream_t st, int64_t n_rings, int64_t n_slots, const HpathIn &in, const HpathLeg *legs, int64_t *cnt, int32_t *status,
                       const int32_t *scratch, int64_t *leg_off, int64_t *path_off, const LegTotals &totals, int64_t *err);
// a lane per sample; every output may be NULL.  P: FieldLegs or RingLegs
template <class P>
int launch_leg_fill(hipStream_t st, int64_t n_slots, const typename P::Leg *legs, const int64_t *leg_off, int64_t total_samples, double R, double spacing,
                    double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg);

}  // namespace fcpp
