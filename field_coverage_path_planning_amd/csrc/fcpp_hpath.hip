// fcpp_hpath.hip -- gfx950 (MI355X) kernels of the headland paths: k_hpath_legs (a lane per driven vertex of every ring: its element, the
// joint behind it, the two slots' records and sample counts), k_hpath_mark (a lane per ring: the status of a ring of fewer than two
// vertices or without a drivable element), k_hpath_settle (a lane per slot: a failed ring's counts become 0), the slot offsets through
// k_path_counts (fcpp_samplefn.h: the samplers' scan, as it is), k_hpath_rings (a lane per ring: its path offset, its totals, the 2^31
// check) and k_hpath_fill (a lane per output sample).  The rule is ONE set of host+device expressions, fcpp_hpathfn.h; float64,
// -ffp-contract=off like every other translation unit, so the kernels give the bits fcpp_debug_headland_paths gives on the host.  Plain
// C++: no inline assembly, no float atomics, no per-thread arrays beyond a record's five segments, every loop bounded.
//
// k_hpath_legs: the ring of a vertex by bisection of ring_offsets (no table of its own).  A lane whose vertex starts no element writes two
// empty records.  A lane that starts one scans forward to the end of its src run (an arc of 16 chords: 16 loads of src), forms the
// element (one fc_hypot, one atan2_fd; an arc a square root, a second atan2_fd, two divisions and two wraps more), and, when the element
// is drivable, walks over the skipped elements to the next drivable one and solves the connector unless the joint is smooth.  Both scans
// stay inside the ring and end after at most m steps; only drivable elements walk, so a ring's walks together visit each element at most
// twice.  Status: a lane that finds a cause of EINVAL writes it with an integer atomic exchange (every writer the same value), a lane
// with a drivable element sets the ring's flag with an integer atomic or; k_hpath_mark turns "status 0 and no flag" into EUNSUPPORTED in
// a later launch, so arrival order changes no output bit.  Written per vertex: two records of 128 B and two counts -- 272 B, each
// lane's 256 B of records contiguous, the wavefront's 16 KiB too.
// DIVERGENCE, accepted.  Element starts and the arc vertices between them alternate irregularly, sharp joints (a solve of several hundred
// instructions for Dubins, several thousand for Reeds-Shepp) and smooth ones (none) too: on a ring of straight pieces and 16-chord arcs
// about one lane in eight starts an element and fewer solve, so most of a wavefront idles through a solve.  The benchmark's batch (4096
// stars, three passes) is 12 473 rings, 2.9 M lanes and 714 415 legs (elements and connectors); not worked around: compacting the
// element starts would cost a scan over the vertices, which is what the call already spends most on (below).
//
// k_hpath_fill: a lane per sample.  Its slot by bisection of the slot offsets (sample_path), its record (128 B, read by every lane of the
// leg: L1 / L2 hits), then hpath_eval.  STATIC FIGURES, not measured.  Written per sample: 4 x 8 B (x, y, heading, kappa) + 1 B (part) + 1 B
// (gear) + 4 B (leg) = 38 B, each array with consecutive addresses per lane: a wavefront writes 512 consecutive bytes of every float64
// array.  fp64 operations per sample: a straight sample 7 (one division); a followed-arc sample one fc_sincos (40), one division, the wrap
// (6) and 8 more = about 55; a Dubins connector sample about 190, a Reeds-Shepp sample about 290 (fcpp_fpath.hip's count: the same
// functions).  Straight and arc samples are streaming (55 unfused operations per 38 B stay below the balance point of 78.6 Tflop/s --
// an fma counted as two -- against 8 TB/s); connector samples sit near it.  DESIGN.md holds what was measured.
// Lanes of one wavefront that straddle an element and a connector run both branches one after the other, as in k_fpath_fill.
//
// THE SCAN is one workgroup over 2 n_verts slots (fcpp_samplefn.h), the field paths' largest cost and this call's too; a scan over several
// workgroups belongs to all samplers at once.  k_hpath_settle keeps the scan's loads to one coalesced count per slot.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_hpath.h"
#include "fcpp_hpathfn.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int HBLOCK = 256;

#define HPATH_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

template <int MODE>
__global__ __launch_bounds__(HBLOCK) void k_hpath_legs(int64_t n_rings, int64_t n_verts, HpathIn in, HpathLeg *__restrict__ legs,
                                                       int64_t *__restrict__ cnt, int32_t *__restrict__ status, int32_t *__restrict__ drivable)
{
    const int64_t g = (int64_t)blockIdx.x * HBLOCK + threadIdx.x;
    if (g >= n_verts) return;
    int64_t lo = 0, hi = n_rings;              // the last ring whose first vertex lies at or before g: the one that holds it
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (in.roff[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t r = lo, k = g - in.roff[r];
    int64_t c_el, c_jt;
    bool invalid, drives;
    // (built where they lie: two records of 128 B in registers would spill)
    hpath_legs<MODE>(in, r, k, legs[2 * g], legs[2 * g + 1], c_el, c_jt, invalid, drives);
    if (invalid && status) atomicExch(&status[r], HPATH_EINVAL);
    if (drives && drivable) atomicOr(&drivable[r], 1);
    if (cnt) { cnt[2 * g] = c_el; cnt[2 * g + 1] = c_jt; }
}

// a lane per ring: fewer than two vertices (a ring of none has no lane above) is EINVAL; status 0 and no drivable element EUNSUPPORTED
__global__ __launch_bounds__(HBLOCK) void k_hpath_mark(int64_t n_rings, const int64_t *__restrict__ roff, const int32_t *__restrict__ drivable,
                                                       int32_t *__restrict__ status)
{
    const int64_t r = (int64_t)blockIdx.x * HBLOCK + threadIdx.x;
    if (r >= n_rings) return;
    if (roff[r + 1] - roff[r] < 2) status[r] = HPATH_EINVAL;
    else if (status[r] == HPATH_OK && drivable[r] == 0) status[r] = HPATH_EUNSUPPORTED;
}

// a lane per slot: the count of a slot of a failed ring is 0
__global__ __launch_bounds__(HBLOCK) void k_hpath_settle(int64_t n_slots, const HpathLeg *__restrict__ legs, const int32_t *__restrict__ status,
                                                         int64_t *__restrict__ cnt)
{
    const int64_t p = (int64_t)blockIdx.x * HBLOCK + threadIdx.x;
    if (p >= n_slots) return;
    if (cnt[p] != 0 && status[legs[p].leg.field] != HPATH_OK) cnt[p] = 0;
}

// the count of a slot as the scan takes it: bad for a leg of 2^31 samples or more
struct HpathCount {
    const int64_t *cnt;
    __device__ int64_t operator()(int64_t p, int64_t &bad) const
    {
        const int64_t c = cnt[p];
        if (c < 0) { ++bad; return 0; }
        return c;
    }
};

// lane r < n_rings: ring r's path offset and totals; lane n_rings: the closing offset.  (after the scan: err[0] holds the bad legs)
__global__ __launch_bounds__(HBLOCK) void k_hpath_rings(int64_t n_rings, int64_t n_slots, const int64_t *__restrict__ roff,
                                                        const HpathLeg *__restrict__ legs, const int32_t *__restrict__ status,
                                                        const int64_t *__restrict__ leg_off, int64_t *__restrict__ path_off,
                                                        double *__restrict__ work, double *__restrict__ transit, double *__restrict__ skipped,
                                                        int64_t *__restrict__ err)
{
    const int64_t r = (int64_t)blockIdx.x * HBLOCK + threadIdx.x;
    if (r > n_rings) return;
    if (r == n_rings) { path_off[n_rings] = leg_off[n_slots]; return; }
    const int64_t first = 2 * roff[r], next = 2 * roff[r + 1];
    path_off[r] = leg_off[first];
    if (leg_off[next] - leg_off[first] > FPATH_MAX_SAMPLES) atomicAdd((unsigned long long *)err, 1ull);
    double w = __builtin_nan(""), t = __builtin_nan(""), s = __builtin_nan("");
    if (status[r] != HPATH_EINVAL) hpath_totals(legs + first, (next - first) / 2, w, t, s);
    if (work) work[r] = w;
    if (transit) transit[r] = t;
    if (skipped) skipped[r] = s;
}

__global__ __launch_bounds__(HBLOCK) void k_hpath_fill(int64_t n_slots, const HpathLeg *__restrict__ legs, const int64_t *__restrict__ leg_off,
                                                       int64_t total_samples, double R, double spacing, double *__restrict__ xs,
                                                       double *__restrict__ ys, double *__restrict__ hs, double *__restrict__ kappas,
                                                       int8_t *__restrict__ parts, int8_t *__restrict__ gears, int32_t *__restrict__ slots)
{
    const int64_t q = (int64_t)blockIdx.x * HBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(leg_off, n_slots, q, p, k, K);
    const HpathLeg &lg = legs[p];             // (read where it lies: a copy with its indexed segments would live in scratch)
    double x, y, h, kap;
    int gear;
    hpath_eval(lg, R, spacing, k, K, x, y, h, kap, gear);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (parts) parts[q] = (int8_t)lg.leg.part;
    if (gears) gears[q] = (int8_t)gear;
    if (slots) slots[q] = lg.leg.slot;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
static unsigned hpath_grid(int64_t lanes) { return (unsigned)((lanes + HBLOCK - 1) / HBLOCK); }

int launch_hpath_legs(hipStream_t st, int64_t n_rings, int64_t n_verts, const HpathIn &in, int mode, HpathLeg *legs, int64_t *cnt, int32_t *status,
                      int32_t *drivable)
{
    if (n_rings <= 0 || n_verts <= 0) return 0;
    if (mode == 0) hipLaunchKernelGGL(k_hpath_legs<0>, dim3(hpath_grid(n_verts)), dim3(HBLOCK), 0, st, n_rings, n_verts, in, legs, cnt, status, drivable);
    else hipLaunchKernelGGL(k_hpath_legs<1>, dim3(hpath_grid(n_verts)), dim3(HBLOCK), 0, st, n_rings, n_verts, in, legs, cnt, status, drivable);
    HPATH_LAUNCH_CHECK();
    return 0;
}

int launch_hpath_offsets(hipStream_t st, int64_t n_rings, int64_t n_verts, const int64_t *roff, const HpathLeg *legs, int64_t *cnt, int32_t *status,
                         const int32_t *drivable, int64_t *leg_off, int64_t *path_off, double *work, double *transit, double *skipped, int64_t *err)
{
    const int64_t n_slots = n_rings > 0 ? 2 * n_verts : 0;
    if (n_rings > 0) {
        hipLaunchKernelGGL(k_hpath_mark, dim3(hpath_grid(n_rings)), dim3(HBLOCK), 0, st, n_rings, roff, drivable, status);
        HPATH_LAUNCH_CHECK();
    }
    if (n_slots > 0) {
        hipLaunchKernelGGL(k_hpath_settle, dim3(hpath_grid(n_slots)), dim3(HBLOCK), 0, st, n_slots, legs, status, cnt);
        HPATH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((k_path_counts<HBLOCK, HpathCount>), dim3(1), dim3(HBLOCK), 0, st, n_slots, HpathCount{ cnt }, leg_off, err);
    HPATH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hpath_rings, dim3(hpath_grid(n_rings + 1)), dim3(HBLOCK), 0, st, n_rings, n_slots, roff, legs, status, leg_off, path_off, work,
                       transit, skipped, err);
    HPATH_LAUNCH_CHECK();
    return 0;
}

int launch_hpath_fill(hipStream_t st, int64_t n_slots, const HpathLeg *legs, const int64_t *leg_off, int64_t total_samples, double R, double spacing,
                      double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (total_samples <= 0 || n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_hpath_fill, dim3(hpath_grid(total_samples)), dim3(HBLOCK), 0, st, n_slots, legs, leg_off, total_samples, R, spacing, x, y,
                       heading, kappa, part, gear, leg);
    HPATH_LAUNCH_CHECK();
    return 0;
}

}  // namespace fcpp
