// fcpp_fpath.hip -- gfx950 (MI355X) kernels of the field paths: k_fpath_legs (a lane per leg slot of every field: the order's validation,
// the connector solves, the slot's record and sample count), the slot offsets through k_path_counts (fcpp_samplefn.h: the samplers' scan),
// k_fpath_fields (a lane per field: its path offset, its totals, the 2^31 check) and k_fpath_fill (a lane per output sample).  The rule is
// ONE set of host+device expressions, fcpp_fpathfn.h; float64, -ffp-contract=off like every other translation unit, so the kernels give
// the bits fcpp_debug_field_paths gives on the host.  Plain C++: no inline assembly, no float atomics, no per-thread arrays beyond a
// record's five segments, every loop bounded.
//
// k_fpath_legs: the field of a slot by bisection of the fields' first slots 2 soff[i] + i (no table of its own).  The order is validated
// with an int32 counter per swath, bumped by the lane of the swath slot that names it (an integer atomic): the lane that sees a second
// visit, or an entry out of range, writes the field's status.  Every such lane writes the same value, and whether a swath is named twice
// does not depend on who arrives first.  Odd slots (swaths) and even slots (connectors) alternate, so every wavefront runs both branches:
// the swath branch is a few loads, the connector branch a solve of several hundred (Dubins) to several thousand (Reeds-Shepp)
// instructions -- half the lanes idle through it.  Accepted: a batch of 4096 fields of 30 swaths is 250 000 slots, one solve each per two
// lanes, tens of microseconds beside the samples.
//
// k_fpath_fill: a lane per sample.  Its slot by bisection of the slot offsets (sample_path), its record (96 B, read by every lane of the
// leg: L1 / L2 hits), then fpath_eval.  STATIC FIGURES.  Written per sample: 4 x 8 B (x, y, heading, kappa) + 1 B (part) + 1 B (gear) + 4 B
// (leg) = 38 B, each array with consecutive addresses per lane: a wavefront writes 512 consecutive bytes of every float64 array.  fp64
// operations per sample: a swath sample 7 (one division); a Dubins connector sample at most 4 fc_sincos (40 each: the start heading and
// one per segment up to the sample's) + 3 divisions + about 30 more = about 190; a Reeds-Shepp sample at most 6 fc_sincos + the runs
// = about 290.  The data sheet's fp64 vector rate (78.6 Tflop/s) counts an fma as two; most of these are not fused, so a Dubins
// connector sample's 190 operations take about as long as its 38 B take on the 8 TB/s write stream: connector samples sit near the
// balance point, swath samples are pure streaming.  Not measured here: DESIGN.md holds what was.
// DIVERGENCE.  Lanes of one wavefront that straddle a swath and a connector (a leg of 30 m at 0.5 m spacing is 61 samples: most wavefronts
// straddle) run both branches one after the other, and within a connector the lanes on different segments run dubins_pose_at's loop to
// the longest count.  Accepted and not worked around: sorting samples by kind would cost a pass over them, which is what the kernel
// is bound by.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_fpath.h"
#include "fcpp_fpathfn.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int FBLOCK = 256;

#define FPATH_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

template <int MODE>
__global__ __launch_bounds__(FBLOCK) void k_fpath_legs(int64_t n, int64_t n_slots, FpathIn in, FpathLeg *__restrict__ legs,
                                                       int64_t *__restrict__ cnt, int32_t *__restrict__ seen, int32_t *__restrict__ status)
{
    const int64_t g = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (g >= n_slots) return;
    int64_t lo = 0, hi = n;                    // the last field whose first slot lies at or before g: the one that holds it
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (fpath_first_slot(in.soff, mid) <= g) lo = mid; else hi = mid;
    }
    const int64_t i = lo, j = g - fpath_first_slot(in.soff, i);
    FpathLeg leg;
    bool invalid;
    const int64_t K = fpath_leg<MODE>(in, i, j, leg, invalid);
    if (seen && in.order && (j & 1) && !invalid && leg.kind == FPATH_SWATH) {
        const int64_t s0 = in.soff[i];
        const int32_t o = in.order[s0 + (j - 1) / 2];          // (in range: the leg exists)
        if (atomicAdd(&seen[s0 + (o >> 1)], 1) != 0) invalid = true;
    }
    if (invalid && status) status[i] = FPATH_EINVAL;
    legs[g] = leg;
    if (cnt) cnt[g] = K;
}

// the count of a slot as the scan takes it: 0 in a failed field, bad for a leg of 2^31 samples or more
struct FpathCount {
    const FpathLeg *legs;
    const int64_t *cnt;
    const int32_t *status;
    __device__ int64_t operator()(int64_t p, int64_t &bad) const
    {
        if (status[legs[p].field] != FPATH_OK) return 0;
        const int64_t c = cnt[p];
        if (c < 0) { ++bad; return 0; }
        return c;
    }
};

// lane i < n: field i's path offset and totals; lane n: the closing offset.  (after the scan: err[0] holds the bad legs)
__global__ __launch_bounds__(FBLOCK) void k_fpath_fields(int64_t n, int64_t n_slots, const int64_t *__restrict__ soff,
                                                         const FpathLeg *__restrict__ legs, const int32_t *__restrict__ status, int has_entry,
                                                         int has_exit, const int64_t *__restrict__ leg_off, int64_t *__restrict__ path_off,
                                                         double *__restrict__ work, double *__restrict__ transit, int64_t *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (i > n) return;
    if (i == n) { path_off[n] = leg_off[n_slots]; return; }
    const int64_t first = fpath_first_slot(soff, i), next = fpath_first_slot(soff, i + 1), m = soff[i + 1] - soff[i];
    path_off[i] = leg_off[first];
    if (leg_off[next] - leg_off[first] > FPATH_MAX_SAMPLES) atomicAdd((unsigned long long *)err, 1ull);
    double w = __builtin_nan(""), t = __builtin_nan("");
    if (status[i] == FPATH_OK) fpath_totals(legs + first, m, has_entry != 0, has_exit != 0, w, t);
    if (work) work[i] = w;
    if (transit) transit[i] = t;
}

__global__ __launch_bounds__(FBLOCK) void k_fpath_fill(int64_t n_slots, const FpathLeg *__restrict__ legs, const int64_t *__restrict__ leg_off,
                                                       int64_t total_samples, double R, double spacing, double *__restrict__ xs,
                                                       double *__restrict__ ys, double *__restrict__ hs, double *__restrict__ kappas,
                                                       int8_t *__restrict__ parts, int8_t *__restrict__ gears, int32_t *__restrict__ slots)
{
    const int64_t q = (int64_t)blockIdx.x * FBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(leg_off, n_slots, q, p, k, K);
    const FpathLeg &leg = legs[p];            // (read where it lies: a copy with its indexed segments would live in scratch)
    double x, y, h, kap;
    int gear;
    fpath_eval(leg, R, spacing, k, K, x, y, h, kap, gear);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (parts) parts[q] = (int8_t)leg.part;
    if (gears) gears[q] = (int8_t)gear;
    if (slots) slots[q] = leg.slot;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_fpath_legs(hipStream_t st, int64_t n, int64_t n_total, const FpathIn &in, int mode, FpathLeg *legs, int64_t *cnt, int32_t *seen,
                      int32_t *status)
{
    if (n <= 0) return 0;
    const int64_t n_slots = 2 * n_total + n;
    const dim3 grid((unsigned)((n_slots + FBLOCK - 1) / FBLOCK));
    if (mode == 0) hipLaunchKernelGGL(k_fpath_legs<0>, grid, dim3(FBLOCK), 0, st, n, n_slots, in, legs, cnt, seen, status);
    else hipLaunchKernelGGL(k_fpath_legs<1>, grid, dim3(FBLOCK), 0, st, n, n_slots, in, legs, cnt, seen, status);
    FPATH_LAUNCH_CHECK();
    return 0;
}

int launch_fpath_offsets(hipStream_t st, int64_t n, int64_t n_total, const int64_t *soff, const FpathLeg *legs, const int64_t *cnt,
                         const int32_t *status, int has_entry, int has_exit, int64_t *leg_off, int64_t *path_off, double *work, double *transit,
                         int64_t *err)
{
    const int64_t n_slots = n > 0 ? 2 * n_total + n : 0;
    hipLaunchKernelGGL((k_path_counts<FBLOCK, FpathCount>), dim3(1), dim3(FBLOCK), 0, st, n_slots, FpathCount{ legs, cnt, status }, leg_off, err);
    FPATH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fpath_fields, dim3((unsigned)((n + 1 + FBLOCK - 1) / FBLOCK)), dim3(FBLOCK), 0, st, n, n_slots, soff, legs, status, has_entry,
                       has_exit, leg_off, path_off, work, transit, err);
    FPATH_LAUNCH_CHECK();
    return 0;
}

int launch_fpath_fill(hipStream_t st, int64_t n_slots, const FpathLeg *legs, const int64_t *leg_off, int64_t total_samples, double R,
                      double spacing, double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (total_samples <= 0 || n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_fpath_fill, dim3((unsigned)((total_samples + FBLOCK - 1) / FBLOCK)), dim3(FBLOCK), 0, st, n_slots, legs, leg_off,
                       total_samples, R, spacing, x, y, heading, kappa, part, gear, leg);
    FPATH_LAUNCH_CHECK();
    return 0;
}

}  // namespace fcpp
