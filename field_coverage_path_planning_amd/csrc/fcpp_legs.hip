// fcpp_legs.hip -- gfx950 (MI355X) kernels of the leg-path operators: the field paths (a group is a field; rule and leg set: fcpp_fpathfn.h)
// and the headland paths (a group is a ring; fcpp_hpathfn.h).  Per operator a RULE kernel: k_fpath_legs (a lane per leg slot of every
// field: the order's validation, the connector solves, the slot's record and sample count) / k_hpath_legs (a lane per driven vertex of
// every ring: its element, the joint behind it, the two slots' records and counts), the latter with k_hpath_mark (a lane per ring: the
// status of a ring of fewer than two vertices or without a drivable element) and k_hpath_settle (a lane per slot: a failed ring's counts
// become 0).  For both alike, on the leg set P: the slot offsets through k_path_counts (fcpp_samplefn.h: the samplers' scan, as it is),
// k_leg_groups<P> (a lane per group: its path offset, its totals, the 2^31 check) and k_leg_fill<P> (a lane per output sample).  Each rule
// is ONE set of host+device expressions; float64, -ffp-contract=off like every other translation unit, so the kernels give the bits
// fcpp_debug_field_paths / fcpp_debug_headland_paths give on the host.  Plain C++: no inline assembly, no float atomics, no per-thread
// arrays beyond a record's five segments and a group's totals, every loop bounded.
//
// k_fpath_legs: the field of a slot by bisection of the fields' first slots 2 soff[i] + i (no table of its own).  The order is validated
// with an int32 counter per swath, bumped by the lane of the swath slot that names it (an integer atomic): the lane that sees a second
// visit, or an entry out of range, writes the field's status.  Every such lane writes the same value, and whether a swath is named twice
// does not depend on who arrives first.  Odd slots (swaths) and even slots (connectors) alternate, so every wavefront runs both branches:
// the swath branch is a few loads, the connector branch a solve of several hundred (Dubins) to several thousand (Reeds-Shepp)
// instructions -- half the lanes idle through it.  Accepted: a batch of 4096 fields of 30 swaths is 250 000 slots, one solve each per two
// lanes, tens of microseconds beside the samples.
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
// DIVERGENCE of the rule kernels, accepted.  Fields: see above.  Rings: element starts and the arc vertices between them alternate
// irregularly, sharp joints (a solve) and smooth ones (none) too: on a ring of straight pieces and 16-chord arcs about one lane in eight
// starts an element and fewer solve, so most of a wavefront idles through a solve.  The benchmark's batch (4096 stars, three passes) is
// 12 473 rings, 2.9 M lanes and 714 415 legs (elements and connectors); not worked around: compacting the element starts would cost a
// scan over the vertices, which is what the call already spends most on (below).
//
// k_leg_fill: a lane per sample.  Its slot by bisection of the slot offsets (sample_path), its record (fields 96 B, rings 128 B, read by
// every lane of the leg: L1 / L2 hits), then P::eval.  STATIC FIGURES, not measured here: DESIGN.md holds what was.  Written per sample:
// 4 x 8 B (x, y, heading, kappa) + 1 B (part) + 1 B (gear) + 4 B (leg) = 38 B, each array with consecutive addresses per lane: a wavefront
// writes 512 consecutive bytes of every float64 array.  fp64 operations per sample: a swath or straight sample 7 (one division); a
// followed-arc sample (rings only) one fc_sincos (40), one division, the wrap (6) and 8 more = about 55; a Dubins connector sample at most
// 4 fc_sincos (40 each: the start heading and one per segment up to the sample's) + 3 divisions + about 30 more = about 190; a
// Reeds-Shepp sample at most 6 fc_sincos + the runs = about 290.  The data sheet's fp64 vector rate (78.6 Tflop/s) counts an fma as two;
// most of these are not fused, so a Dubins connector sample's 190 operations take about as long as its 38 B take on the 8 TB/s write
// stream: connector samples sit near the balance point, swath, straight and arc samples are streaming.
// DIVERGENCE of the fill.  Lanes of one wavefront that straddle an element and a connector (a leg of 30 m at 0.5 m spacing is 61 samples:
// most wavefronts straddle) run both branches one after the other, and within a connector the lanes on different segments run
// dubins_pose_at's loop to the longest count.  Accepted and not worked around: sorting samples by kind would cost a pass over them, which
// is what the kernel is bound by.
//
// THE SCAN is one workgroup over all slots (fcpp_samplefn.h), either operator's largest cost; a scan over several workgroups belongs to
// all samplers at once.  What it takes as a slot's count is the one difference between the operators downstream of
// the records: the fields' functor reads status[legs[p].field] per slot, the rings' counts were zeroed beforehand by k_hpath_settle, which
// keeps the scan's loads to one coalesced count per slot.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_legs.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int LBLOCK = 256;

// ---- the rule kernels -------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(LBLOCK) void k_fpath_legs(int64_t n, int64_t n_slots, FpathIn in, FpathLeg *__restrict__ legs,
                                                       int64_t *__restrict__ cnt, int32_t *__restrict__ seen, int32_t *__restrict__ status)
{
    const int64_t g = (int64_t)blockIdx.x * LBLOCK + threadIdx.x;
    if (g >= n_slots) return;
    const int64_t i = last_at_or_before(n, g, [&](int64_t f) { return fpath_first_slot(in.soff, f); });      // the field that holds slot g
    const int64_t j = g - fpath_first_slot(in.soff, i);
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

template <int MODE>
__global__ __launch_bounds__(LBLOCK) void k_hpath_legs(int64_t n_rings, int64_t n_verts, HpathIn in, HpathLeg *__restrict__ legs,
                                                       int64_t *__restrict__ cnt, int32_t *__restrict__ status, int32_t *__restrict__ drivable)
{
    const int64_t g = (int64_t)blockIdx.x * LBLOCK + threadIdx.x;
    if (g >= n_verts) return;
    const int64_t r = last_at_or_before(n_rings, g, [&](int64_t f) { return in.roff[f]; });                  // the ring that holds vertex g
    const int64_t k = g - in.roff[r];
    int64_t c_el, c_jt;
    bool invalid, drives;
    // (built where they lie: two records of 128 B in registers would spill)
    hpath_legs<MODE>(in, r, k, legs[2 * g], legs[2 * g + 1], c_el, c_jt, invalid, drives);
    if (invalid && status) atomicExch(&status[r], HPATH_EINVAL);
    if (drives && drivable) atomicOr(&drivable[r], 1);
    if (cnt) { cnt[2 * g] = c_el; cnt[2 * g + 1] = c_jt; }
}

// a lane per ring: fewer than two vertices (a ring of none has no lane above) is EINVAL; status 0 and no drivable element EUNSUPPORTED
__global__ __launch_bounds__(LBLOCK) void k_hpath_mark(int64_t n_rings, const int64_t *__restrict__ roff, const int32_t *__restrict__ drivable,
                                                       int32_t *__restrict__ status)
{
    const int64_t r = (int64_t)blockIdx.x * LBLOCK + threadIdx.x;
    if (r >= n_rings) return;
    if (roff[r + 1] - roff[r] < 2) status[r] = HPATH_EINVAL;
    else if (status[r] == HPATH_OK && drivable[r] == 0) status[r] = HPATH_EUNSUPPORTED;
}

// a lane per slot: the count of a slot of a failed ring is 0
__global__ __launch_bounds__(LBLOCK) void k_hpath_settle(int64_t n_slots, const HpathLeg *__restrict__ legs, const int32_t *__restrict__ status,
                                                         int64_t *__restrict__ cnt)
{
    const int64_t p = (int64_t)blockIdx.x * LBLOCK + threadIdx.x;
    if (p >= n_slots) return;
    if (cnt[p] != 0 && status[legs[p].leg.field] != HPATH_OK) cnt[p] = 0;
}

// the count of a slot as the scan takes it: bad for a leg of 2^31 samples or more.  Fields: 0 in a failed field; rings: settled before
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

struct HpathCount {
    const int64_t *cnt;
    __device__ int64_t operator()(int64_t p, int64_t &bad) const
    {
        const int64_t c = cnt[p];
        if (c < 0) { ++bad; return 0; }
        return c;
    }
};

// ---- downstream of the records: the same for every leg set P ------------------------------------------------------------------------
// lane g < n_groups: group g's path offset and totals; lane n_groups: the closing offset.  (after the scan: err[0] holds the bad legs)
template <class P>
__global__ __launch_bounds__(LBLOCK) void k_leg_groups(int64_t n_groups, int64_t n_slots, typename P::In in, const typename P::Leg *__restrict__ legs,
                                                       const int32_t *__restrict__ status, const int64_t *__restrict__ leg_off,
                                                       int64_t *__restrict__ path_off, LegTotals totals, int64_t *__restrict__ err)
{
    const int64_t g = (int64_t)blockIdx.x * LBLOCK + threadIdx.x;
    if (g > n_groups) return;
    if (g == n_groups) { path_off[n_groups] = leg_off[n_slots]; return; }
    const int64_t first = P::first_slot(in, g), next = P::first_slot(in, g + 1);
    path_off[g] = leg_off[first];
    if (leg_off[next] - leg_off[first] > FPATH_MAX_SAMPLES) atomicAdd((unsigned long long *)err, 1ull);
    double t[P::N_TOTALS];
    P::totals(in, legs + first, g, status[g], t);
#pragma unroll
    for (int k = 0; k < P::N_TOTALS; ++k)
        if (totals.p[k]) totals.p[k][g] = t[k];
}

template <class P>
__global__ __launch_bounds__(LBLOCK) void k_leg_fill(int64_t n_slots, const typename P::Leg *__restrict__ legs, const int64_t *__restrict__ leg_off,
                                                     int64_t total_samples, double R, double spacing, double *__restrict__ xs,
                                                     double *__restrict__ ys, double *__restrict__ hs, double *__restrict__ kappas,
                                                     int8_t *__restrict__ parts, int8_t *__restrict__ gears, int32_t *__restrict__ slots)
{
    const int64_t q = (int64_t)blockIdx.x * LBLOCK + threadIdx.x;
    if (q >= total_samples) return;
    int64_t p, k, K;
    sample_path(leg_off, n_slots, q, p, k, K);
    const typename P::Leg &lg = legs[p];      // (read where it lies: a copy with its indexed segments would live in scratch)
    double x, y, h, kap;
    int gear;
    P::eval(lg, R, spacing, k, K, x, y, h, kap, gear);
    if (xs) xs[q] = x;
    if (ys) ys[q] = y;
    if (hs) hs[q] = h;
    if (kappas) kappas[q] = kap;
    if (parts) parts[q] = (int8_t)P::base(lg).part;
    if (gears) gears[q] = (int8_t)gear;
    if (slots) slots[q] = P::base(lg).slot;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_legs(hipStream_t st, int64_t n, int64_t n_slots, const FpathIn &in, int mode, FpathLeg *legs, int64_t *cnt, int32_t *scratch, int32_t *status)
{
    if (n <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_fpath_legs<M()>, blocks_for(n_slots, LBLOCK), LBLOCK, n, n_slots, in, legs, cnt, scratch, status);
    });
}

int launch_legs(hipStream_t st, int64_t n_rings, int64_t n_slots, const HpathIn &in, int mode, HpathLeg *legs, int64_t *cnt, int32_t *scratch,
                int32_t *status)
{
    const int64_t n_verts = n_slots / 2;
    if (n_rings <= 0 || n_verts <= 0) return 0;
    return by_mode(mode, [&](auto M) {
        return launch(st, k_hpath_legs<M()>, blocks_for(n_verts, LBLOCK), LBLOCK, n_rings, n_verts, in, legs, cnt, status, scratch);
    });
}

// the scan of the slots' counts as count_of takes them, then the groups
template <class P, class CountOf>
static int leg_offsets(hipStream_t st, int64_t n_groups, int64_t n_slots, const typename P::In &in, const typename P::Leg *legs, CountOf count_of,
                       const int32_t *status, int64_t *leg_off, int64_t *path_off, const LegTotals &totals, int64_t *err)
{
    if (int e = launch_path_counts<LBLOCK>(st, n_slots, count_of, leg_off, err)) return e;
    return launch(st, k_leg_groups<P>, blocks_for(n_groups + 1, LBLOCK), LBLOCK, n_groups, n_slots, in, legs, status, leg_off, path_off, totals, err);
}

int launch_leg_offsets(hipStream_t st, int64_t n, int64_t n_slots, const FpathIn &in, const FpathLeg *legs, int64_t *cnt, int32_t *status,
                       const int32_t *, int64_t *leg_off, int64_t *path_off, const LegTotals &totals, int64_t *err)
{
    return leg_offsets<FieldLegs>(st, n, n_slots, in, legs, FpathCount{ legs, cnt, status }, status, leg_off, path_off, totals, err);
}

int launch_leg_offsets(hipStream_t st, int64_t n_rings, int64_t n_slots, const HpathIn &in, const HpathLeg *legs, int64_t *cnt, int32_t *status,
                       const int32_t *scratch, int64_t *leg_off, int64_t *path_off, const LegTotals &totals, int64_t *err)
{
    if (n_rings > 0) {
        if (int e = launch(st, k_hpath_mark, blocks_for(n_rings, LBLOCK), LBLOCK, n_rings, in.roff, scratch, status)) return e;
    }
    if (n_slots > 0) {
        if (int e = launch(st, k_hpath_settle, blocks_for(n_slots, LBLOCK), LBLOCK, n_slots, legs, status, cnt)) return e;
    }
    return leg_offsets<RingLegs>(st, n_rings, n_slots, in, legs, HpathCount{ cnt }, status, leg_off, path_off, totals, err);
}

template <class P>
int launch_leg_fill(hipStream_t st, int64_t n_slots, const typename P::Leg *legs, const int64_t *leg_off, int64_t total_samples, double R, double spacing,
                    double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (total_samples <= 0 || n_slots <= 0) return 0;
    return launch(st, k_leg_fill<P>, blocks_for(total_samples, LBLOCK), LBLOCK, n_slots, legs, leg_off, total_samples, R, spacing, x, y, heading,
                  kappa, part, gear, leg);
}

template int launch_leg_fill<FieldLegs>(hipStream_t, int64_t, const FpathLeg *, const int64_t *, int64_t, double, double, double *, double *, double *,
                                        double *, int8_t *, int8_t *, int32_t *);
template int launch_leg_fill<RingLegs>(hipStream_t, int64_t, const HpathLeg *, const int64_t *, int64_t, double, double, double *, double *, double *,
                                       double *, int8_t *, int8_t *, int32_t *);

}  // namespace fcpp
