// fcpp_clear.h -- interface between the C-ABI glue (fcpp_glue_conn.cpp, fcpp_glue_route.cpp) and the connector clearance kernels (fcpp_clear.hip): solved
// connectors against the rings of their field, elementwise and over every field's transit block.  The rule is fcpp_clearfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_clearfn.h"

namespace fcpp {

constexpr int CLEAR_TILE = 256;                          // entries of a field's block that one workgroup of k_clear_transit owns
constexpr int64_t CLEAR_MAX_GROUPS = 0x7fffffffLL;       // the grids

// every launcher returns 0 or a hipError_t value.  F: the fields' CSR on the device, checked by the caller.
// status[f] for f < F.n
int launch_clear_field_status(hipStream_t st, const ClearFields &F, int32_t *status);
// path i = (fx, fy, fh)[i], word[i], seg[NSEG i ..) against field pair_field[i]; crossings, inside, first_s: any may be NULL
int launch_clear_conn(hipStream_t st, int mode, int64_t n, const double *fx, const double *fy, const double *fh, double R, const int32_t *word,
                      const double *seg, const int64_t *pair_field, const ClearFields &F, int32_t *crossings, int8_t *inside, double *first_s);
// tile_off (n + 1): field i's block is owned by the workgroups tile_off[i] .. tile_off[i + 1], CLEAR_TILE entries each; n_tiles = tile_off[n].
// T (in / out) and B as fcpp_route_transit_clear documents them.
int launch_clear_transit(hipStream_t st, int64_t n, const int64_t *soff, const double *ax, const double *ay, const double *bx, const double *by,
                         const double *angle, double R, int mode, const int64_t *toff, const int64_t *tile_off, int64_t n_tiles,
                         const ClearFields &F, double penalty, double *T, uint8_t *B);
// The first pass of the priced transit block (fcpp_route_transit_priced): the same walk with T out only -- every canonical pair's complete
// answer to both mirrored entries of T and K (int8, may be NULL) -- and the global indices of the entries whose other words have to be
// looked at appended to list (room for every canonical pair: t_total / 2), their number added to *count (zeroed by the caller).  The
// second pass is launch_route_priced_words of fcpp_solveclear.h.
int launch_route_priced_first(hipStream_t st, int64_t n, const int64_t *soff, const double *ax, const double *ay, const double *bx,
                              const double *by, const double *angle, double R, int mode, const int64_t *toff, const int64_t *tile_off,
                              int64_t n_tiles, const ClearFields &F, double penalty, double *T, int8_t *K, int64_t *list, unsigned long long *count);

}  // namespace fcpp
