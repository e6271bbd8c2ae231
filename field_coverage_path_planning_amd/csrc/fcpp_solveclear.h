// fcpp_solveclear.h -- interface between the C-ABI glue (fcpp_glue_conn.cpp, fcpp_glue_route.cpp, fcpp_glue_legs.cpp) and the clear-connector kernels (fcpp_solveclear.hip).  The rule is
// fcpp_solveclearfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_fpathfn.h"
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

// The second pass of the priced transit block (fcpp_route_transit_priced; the first one is launch_route_priced_first of fcpp_clear.h): a
// group of lanes per listed entry of T (global indices below t_total, canonical pairs, each once; count at most 2^31 - 1 groups' worth:
// checked by the caller).  A winner of rank >= 0 writes its total to both mirrored entries of T and its rank to K (int8, may be NULL).
int launch_route_priced_words(hipStream_t st, int mode, int64_t count, const int64_t *list, int64_t n, const int64_t *soff, const double *ax,
                              const double *ay, const double *bx, const double *by, const double *angle, double R, const int64_t *toff,
                              int64_t t_total, const ClearFields &F, double *T, int8_t *K);

// The clear field paths (the rule: fcpp_fpathfn.h): the same two passes over the connector slots of the leg records launch_legs wrote
// (legs, cnt: 2 n_total + n slots; F: the region CSR, field i of the swaths is field i of it; n_conn = n_total + n connector slots).
// rank, crossings (per slot, zeroed by the caller), status (the fields' path status) and cnt may be NULL: records only (the fill's pass).
// First pass, a lane per connector slot: the record's word tested, rank and crossings written, the slots to look at appended to list
// (room for n_conn), their number added to *count (zeroed by the caller).
int launch_fpath_clear_slots(hipStream_t st, int mode, int64_t n, int64_t n_conn, const int64_t *soff, double R, const FpathLeg *legs,
                             const int32_t *status, const ClearFields &F, int32_t *rank, int32_t *crossings, int64_t *list,
                             unsigned long long *count);
// Second pass, a group of lanes per listed slot: the winner's word into the record, its count, rank and crossings.
int launch_fpath_clear_words(hipStream_t st, int mode, int64_t count, const int64_t *list, const FpathIn &in, const ClearFields &F, FpathLeg *legs,
                             int64_t *cnt, int32_t *rank, int32_t *crossings);
// A lane per slot: the records' word, seg (5 each) and total; a lane per field: blocked and reshaped from rank.  Any output may be NULL
// (rank NULL: no blocked / reshaped).
int launch_fpath_clear_report(hipStream_t st, int64_t n, int64_t n_slots, const int64_t *soff, const FpathLeg *legs, const int32_t *rank,
                              int32_t *leg_word, double *leg_seg, double *leg_total, int32_t *blocked, int32_t *reshaped);

}  // namespace fcpp
