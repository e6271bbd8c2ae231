// fcpp_speed.hip -- gfx950 (MI355X) kernels of the path speeds (fcpp_path_speeds): the greatest speed profile of every sampled path under
// its caps and separate acceleration and braking limits.  The rule: fcpp_speedfn.h.
//
// The two sweeps as ONE segmented (min, +) scan each way.  Sample i is the map u -> min(c_i, u + w_i); maps compose associatively as
// (c, w) o (c', w') = (min(c, c' + w), w' + w) (combine_after, fcpp_devfn.h).  Forwards w_i = 2 a_acc d_i, backwards the map of sample i
// carries the step that LEAVES it, w_i = 2 a_dec d_(i+1): two scans over the same caps with different weights.  A path's first sample
// forwards and its last backwards have w = +inf: the map is constant, which is the segment boundary -- nothing else resets, a zero step
// is w = 0.  "Forward then backward" equals min(forward(c), backward(c)) (for k <= i <= j the detour over j costs at least the direct
// term of k, for i < k <= j at least the direct term of k backwards), so the two scans are independent and run side by side.
//
// Shape: tiles -> spine -> apply on the path set's tile table (tiles of at most 512 samples that never straddle a path), two consecutive
// samples per thread, everything in registers: a thread composes its two maps, the wavefront scans by shuffles, the four wavefronts meet
// in 128 B of LDS.  The spine between the two passes is the speed planner's (launch_scan_spine: blocks of 2048 tiles, three levels above
// that) -- it composes (c, w) pairs and does not care what the weights mean.  The spine counts tiles from the batch's first, so a path's
// sums are grouped by where it lies in the batch: the same path alone and inside a batch agrees to the rule's bound, not bit for bit.
//
// A failing sample (non-finite x, y, kappa, a part outside 0 .. 7, a gear other than +-1) marks its path in status by one integer atomic
// per tile; its map is made harmless (c = +inf, a NaN weight becomes 0) so that nothing crosses into the neighbouring paths, and the
// apply pass writes NaN over the whole path.
//
// Traffic per sample: both passes read x, y, kappa, part, gear (26 B), the apply pass writes v and cap (16 B); the spine moves 48 B per
// TILE.  No atomics on values; float64; -ffp-contract=off like every other translation unit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_devfn.h"
#include "fcpp_launch.h"
#include "fcpp_speed.h"

namespace fcpp {

static constexpr int SBLOCK = 256, SNWAVE = SBLOCK / 64;
static_assert(TILE_POINTS == 2 * SBLOCK, "two consecutive samples per thread");

// one thread's two consecutive samples j0 = 2 * tid, j0 + 1 of a tile: their caps and the weights of their maps both ways.  A slot
// beyond the tile is the identity map (c = +inf, w = 0).
struct SpeedLane {
    double c0, c1;          // caps [m^2/s^2], 0 at a stop
    double wf0, wf1;        // forwards: 2 a_acc x the step INTO the sample (+inf at a path's first sample)
    double wb0, wb1;        // backwards: 2 a_dec x the step that LEAVES it (+inf at a path's last sample)
    bool in0, in1;          // the sample belongs to the tile
    bool bad;               // one of the two fails the rule's sample check
};
struct SpeedShared { Agg wf[SNWAVE], wb[SNWAVE]; };

__device__ __forceinline__ double speed_weight(double two_a, double d)
{
    const double w = two_a * d;
    return w >= 0.0 ? w : 0.0;          // (NaN: a failing sample next to it; its path is NaN in the end)
}

// Neighbouring samples come from the neighbouring lanes; only a wavefront's first and last lane (and the tile's last sample) load their
// halo themselves.
__device__ __forceinline__ void speed_tile_load(const DevTile &t, const DevPath &p, const SpeedRule &r, const SpeedIn &in, SpeedLane &s)
{
    const int tid = threadIdx.x, lane = tid & 63, j0 = 2 * tid;
    const int64_t i0 = t.start + j0, g0 = p.off + i0;
    s.in0 = j0 < t.count; s.in1 = j0 + 1 < t.count;
    const bool have1 = s.in0 && i0 + 1 < p.n;                   // the sample after j0 exists (in this tile or as its halo)
    double x0 = 0, y0 = 0, k0 = 0, x1 = 0, y1 = 0, k1 = 0;
    int p0 = 0, q0 = 0, p1 = 0, q1 = 0;                         // part, gear
    if (s.in0) { x0 = in.x[g0]; y0 = in.y[g0]; k0 = in.kappa[g0]; p0 = in.part[g0]; q0 = in.gear[g0]; }
    if (have1) { x1 = in.x[g0 + 1]; y1 = in.y[g0 + 1]; q1 = in.gear[g0 + 1]; }
    if (s.in1) { k1 = in.kappa[g0 + 1]; p1 = in.part[g0 + 1]; }
    // the sample before j0: the neighbouring lane's second
    double xp = __shfl_up(x1, 1), yp = __shfl_up(y1, 1);
    int qp = __shfl_up(q1, 1);
    const bool havep = s.in0 && i0 > 0;
    if (lane == 0 && havep) { xp = in.x[g0 - 1]; yp = in.y[g0 - 1]; qp = in.gear[g0 - 1]; }
    // the sample after j0 + 1: the neighbouring lane's first
    double xn = __shfl_down(x0, 1), yn = __shfl_down(y0, 1);
    int qn = __shfl_down(q0, 1);
    const bool have2 = s.in1 && i0 + 2 < p.n;
    if (have2 && (lane == 63 || j0 + 2 >= t.count)) { xn = in.x[g0 + 2]; yn = in.y[g0 + 2]; qn = in.gear[g0 + 2]; }

    const double d0 = havep ? speed_step(xp, yp, x0, y0) : 0.0;
    const double d1 = have1 ? speed_step(x0, y0, x1, y1) : 0.0;
    const double d2 = have2 ? speed_step(x1, y1, xn, yn) : 0.0;
    const bool ok0 = !s.in0 || speed_sample_ok(x0, y0, k0, p0, q0), ok1 = !s.in1 || speed_sample_ok(x1, y1, k1, p1, q1);
    s.bad = !(ok0 && ok1);
    s.c0 = FCPP_INF; s.c1 = FCPP_INF; s.wf0 = 0.0; s.wf1 = 0.0; s.wb0 = 0.0; s.wb1 = 0.0;
    if (s.in0) {
        if (ok0) s.c0 = speed_stop(r.flags, i0, p.n, qp, q0, q1) ? 0.0 : speed_cap_u(r, k0, p0, q0);
        s.wf0 = havep ? speed_weight(r.two_acc, d0) : FCPP_INF;
        s.wb0 = have1 ? speed_weight(r.two_dec, d1) : FCPP_INF;
    }
    if (s.in1) {
        if (ok1) s.c1 = speed_stop(r.flags, i0 + 1, p.n, q0, q1, qn) ? 0.0 : speed_cap_u(r, k1, p1, q1);
        s.wf1 = speed_weight(r.two_acc, d1);
        s.wb1 = have2 ? speed_weight(r.two_dec, d2) : FCPP_INF;
    }
}

// The tile-local scan: ef / eb = the composed maps of everything in the tile before / behind this thread's two samples, tf / tb = the
// whole tile's, forwards and backwards.
__device__ __forceinline__ void speed_tile_scan(SpeedShared &S, const SpeedLane &s, Agg &ef, Agg &eb, Agg &tf, Agg &tb)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Agg fi = combine_after({ s.c0, s.wf0 }, { s.c1, s.wf1 });          // sample 0, then sample 1
    Agg bi = combine_after({ s.c1, s.wb1 }, { s.c0, s.wb0 });          // sample 1, then sample 0
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Agg pf = { __shfl_up(fi.c, o), __shfl_up(fi.w, o) };
        const Agg pb = { __shfl_down(bi.c, o), __shfl_down(bi.w, o) };
        if (lane >= o) fi = combine_after(pf, fi);
        if (lane + o < 64) bi = combine_after(pb, bi);
    }
    if (lane == 63) S.wf[wave] = fi;
    if (lane == 0) S.wb[wave] = bi;
    __syncthreads();
    ef = { __shfl_up(fi.c, 1), __shfl_up(fi.w, 1) };
    if (lane == 0) ef = { FCPP_INF, 0.0 };
    eb = { __shfl_down(bi.c, 1), __shfl_down(bi.w, 1) };
    if (lane == 63) eb = { FCPP_INF, 0.0 };
    Agg pre = { FCPP_INF, 0.0 }, suf = { FCPP_INF, 0.0 };
    tf = { FCPP_INF, 0.0 }; tb = { FCPP_INF, 0.0 };
#pragma unroll
    for (int q = 0; q < SNWAVE; ++q) {
        if (q == wave) pre = tf;
        tf = combine_after(tf, S.wf[q]);
    }
#pragma unroll
    for (int q = SNWAVE - 1; q >= 0; --q) {
        if (q == wave) suf = tb;
        tb = combine_after(tb, S.wb[q]);
    }
    ef = combine_after(pre, ef);
    eb = combine_after(suf, eb);
}

__global__ __launch_bounds__(SBLOCK) void k_speed_tiles(const DevTile *__restrict__ tiles, const DevPath *__restrict__ paths, SpeedRule rule,
                                                        SpeedIn in, Agg *__restrict__ agg_f, Agg *__restrict__ agg_b,
                                                        int32_t *__restrict__ status)
{
    __shared__ SpeedShared S;
    const DevTile t = tiles[blockIdx.x];
    const DevPath p = paths[t.field];
    SpeedLane s;
    speed_tile_load(t, p, rule, in, s);
    Agg ef, eb, tf, tb;
    speed_tile_scan(S, s, ef, eb, tf, tb);
    const int any_bad = __syncthreads_or(s.bad ? 1 : 0);
    if (threadIdx.x == 0) {
        agg_f[blockIdx.x] = tf; agg_b[blockIdx.x] = tb;
        if (any_bad) atomicMin(&status[t.field], SPEED_EINVAL);          // (integer, order independent)
    }
}

__global__ __launch_bounds__(SBLOCK) void k_speed_apply(const DevTile *__restrict__ tiles, const DevPath *__restrict__ paths, SpeedRule rule,
                                                        SpeedIn in, const double *__restrict__ carry_f, const double *__restrict__ carry_b,
                                                        const int32_t *__restrict__ status, double *__restrict__ v, double *__restrict__ cap)
{
    __shared__ SpeedShared S;
    const DevTile t = tiles[blockIdx.x];
    const DevPath p = paths[t.field];
    const int64_t g0 = p.off + t.start + 2 * threadIdx.x;
    if (status[t.field] != SPEED_OK) {          // (uniform over the workgroup)
        const double nan = __builtin_nan("");
        const bool in0 = 2 * (int)threadIdx.x < t.count, in1 = 2 * (int)threadIdx.x + 1 < t.count;
        if (v) { if (in0) v[g0] = nan; if (in1) v[g0 + 1] = nan; }
        if (cap) { if (in0) cap[g0] = nan; if (in1) cap[g0 + 1] = nan; }
        return;
    }
    SpeedLane s;
    speed_tile_load(t, p, rule, in, s);
    Agg ef, eb, tf, tb;
    speed_tile_scan(S, s, ef, eb, tf, tb);
    // what enters this thread's samples from the left and from the right, then the two samples each way
    const double uf = fmin(ef.c, carry_f[blockIdx.x] + ef.w), ub = fmin(eb.c, carry_b[blockIdx.x] + eb.w);
    const double f0 = fmin(s.c0, uf + s.wf0), f1 = fmin(s.c1, f0 + s.wf1);
    const double b1 = fmin(s.c1, ub + s.wb1), b0 = fmin(s.c0, b1 + s.wb0);
    if (v) {
        if (s.in0) v[g0] = speed_out(fmin(f0, b0));
        if (s.in1) v[g0 + 1] = speed_out(fmin(f1, b1));
    }
    if (cap) {
        if (s.in0) cap[g0] = speed_out(s.c0);
        if (s.in1) cap[g0 + 1] = speed_out(s.c1);
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_speed_tiles(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const SpeedRule &rule, const SpeedIn &in,
                       void *agg_f, void *agg_b, int32_t *status)
{
    if (n_tiles <= 0) return 0;
    return launch(st, k_speed_tiles, (unsigned)n_tiles, SBLOCK, tiles, paths, rule, in, (Agg *)agg_f, (Agg *)agg_b, status);
}

int launch_speed_apply(hipStream_t st, int64_t n_tiles, const DevTile *tiles, const DevPath *paths, const SpeedRule &rule, const SpeedIn &in,
                       const double *carry_f, const double *carry_b, const int32_t *status, double *v, double *cap)
{
    if (n_tiles <= 0) return 0;
    return launch(st, k_speed_apply, (unsigned)n_tiles, SBLOCK, tiles, paths, rule, in, carry_f, carry_b, status, v, cap);
}

}  // namespace fcpp
