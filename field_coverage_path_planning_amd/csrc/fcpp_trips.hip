// fcpp_trips.hip -- gfx950 (MI355X) kernel of the service trips: k_trip_solve splits every field's candidate tours, in both driving
// directions, into capacity-limited round trips to the service point and keeps the cheapest.  The rule is ONE set of host+device
// expressions, fcpp_tripfn.h; float64, -ffp-contract=off like every other translation unit, so the kernel gives the bits
// fcpp_debug_trip_solve gives.
//
// One workgroup of 256 threads per field.  Wavefront w takes the variants v = w, w + 4, .. (with both_ways = 0, where only the even
// variants exist, 2 w, 2 w + 8, ..: none of the four idles): each wavefront keeps the tables of its
// variant (t, P, d, g, pred) and the trip starts of its best variant so far in LDS of its own, 14.5 KiB, so the four share nothing
// until the end.  A variant in three phases:
//   tables     a lane per position: the oriented swath, its length, the transit behind it (one global load per position, all in flight
//              together) and the stop price d.
//   chains     P and base are left-to-right rounded sums, sequential by rule: lane 0 walks both from LDS.
//   programme  j ascending; the lanes take the starts i of j's window in rounds of 64, the pair (g[i], i) is reduced by xor-shuffles
//              (lexicographic and total: no g is NaN, so the tree does not matter); lane 0 stores g[j] and pred[j].  The window's first
//              start only moves forward (fcpp_tripfn.h: the windows), so a field costs about m rounds, not m^2 / 64.
// A wavefront whose variant beats its best so far backtracks at once (lane 0, at most m steps) into its mark bytes, so no variant is
// solved twice.  Behind one barrier the block picks the best of the four, writes the winner's tour, and the first wavefront turns the
// marks into trip indices by ballots.  The candidates are validated before anything is indexed by them (a bit per swath in LDS, set by
// LDS atomics): a bad tour never reaches T.  No float atomics, no per-thread arrays (no scratch), every loop bounded by m or C.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_tripfn.h"
#include "fcpp_trips.h"

namespace fcpp {

static constexpr int TRBLOCK = 256;
static constexpr int TRWAVES = TRBLOCK / 64;

struct TripWave {            // a wavefront's LDS
    double P[ROUTE_MAX_SWATHS + 1], d[ROUTE_MAX_SWATHS], g[ROUTE_MAX_SWATHS];
    int16_t t[ROUTE_MAX_SWATHS], pred[ROUTE_MAX_SWATHS];
    uint8_t mark[ROUTE_MAX_SWATHS];          // 1 where a trip of the wavefront's best variant starts
};

// what one lane of a wavefront wrote to LDS, for the others to read
__device__ __forceinline__ void trip_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the wavefront's least (g, i) under trip_better, in every lane.  g is never NaN.
__device__ __forceinline__ void trip_wave_min(double &g, int &i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double og = __shfl_xor(g, o);
        const int oi = __shfl_xor(i, o);
        if (trip_better(og, oi, g, i)) { g = og; i = oi; }
    }
}

// the least (g[i], i) over the feasible starts i < j of a trip that ends before position j (1 <= j <= m), in every lane; lo: the first
// start >= 1 that may be feasible, moved forward for j and kept for the next one
__device__ __forceinline__ void trip_pick_wave(const TripField &F, const TripWave &W, int j, int &lo, double &bg, int &bi)
{
    const int lane = threadIdx.x & 63;
    const double Pj = W.P[j];
    while (lo < j - 1 && !trip_feasible(W.P[lo], Pj, lo, j, F.Q)) ++lo;          // (uniform)
    bg = INFINITY; bi = INT32_MAX;
    if (lane == 0 && trip_feasible(W.P[0], Pj, 0, j, F.Q0)) { bg = W.g[0]; bi = 0; }
    for (int i = lo + lane; i < j; i += 64)
        if (trip_feasible(W.P[i], Pj, i, j, F.Q) && trip_better(W.g[i], i, bg, bi)) { bg = W.g[i]; bi = i; }
    trip_wave_min(bg, bi);
}

// trip_variant_host by ONE wavefront, every lane of which calls it with the same arguments; the result is the same in every lane and
// the variant's tables stay in W
__device__ __forceinline__ TripVariant trip_variant_wave(const TripField &F, int v, TripWave &W)
{
    const int lane = threadIdx.x & 63, m = F.m, N = 2 * m, r = v & 1;
    const int32_t *cand = F.tours + (v >> 1) * F.stride;
    if (m == 0) return { 0.0, 0.0, tour_plus(0.0, 0.0), -1 };
    // tables: W.P[k + 1] holds w_k and W.g[k] the transit into position k until the chains have walked them
    for (int k = lane; k < m; k += 64) {
        const int b = trip_at(cand, m, r, k);
        W.t[k] = (int16_t)b;
        W.P[k + 1] = F.length[b >> 1];
        if (k > 0) {
            const int a = trip_at(cand, m, r, k - 1);
            const double e = F.T[a * N + b];
            W.g[k] = e;
            W.d[k] = trip_stop(F, a, b, e);
        }
    }
    trip_wave_sync();
    double base = 0.0;
    if (lane == 0) {
        double s = 0.0;
        W.P[0] = 0.0;
        for (int k = 0; k < m; ++k) { s = s + W.P[k + 1]; W.P[k + 1] = s; }
        base = trip_gate(F.E, W.t[0]);                   // route_cost's chain
        for (int k = 1; k < m; ++k) base += W.g[k];
        base = base + trip_gate(F.X, W.t[m - 1]);
        W.g[0] = 0.0;
    }
    base = __shfl(base, 0);
    trip_wave_sync();
    int lo = 1, bi;
    double bg;
    for (int j = 1; j < m; ++j) {
        trip_pick_wave(F, W, j, lo, bg, bi);
        if (lane == 0) { W.g[j] = tour_plus(W.d[j], bg); W.pred[j] = (int16_t)bi; }
        trip_wave_sync();
    }
    trip_pick_wave(F, W, m, lo, bg, bi);
    return { base, bg, tour_plus(base, bg), bi };
}

__global__ __launch_bounds__(TRBLOCK) void k_trip_solve(TripArgs a)
{
    __shared__ TripWave sh[TRWAVES];
    __shared__ double sh_costs[2 * TRIP_MAX_CANDIDATES];
    __shared__ uint32_t sh_seen[TRWAVES][ROUTE_MAX_SWATHS / 32];
    __shared__ double sh_total[TRWAVES], sh_base[TRWAVES], sh_extra[TRWAVES];
    __shared__ int sh_v[TRWAVES], sh_trips[TRWAVES], sh_over[TRWAVES];
    __shared__ int sh_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.x, s0 = a.soff[f], m64 = a.soff[f + 1] - s0;
    const int n_var = trip_n_variants(a.C);
    const double nan = __builtin_nan("");
    const int32_t *cand0 = a.tours + s0;
    int status = m64 > ROUTE_MAX_SWATHS ? TRIP_EUNSUPPORTED : TRIP_OK;
    const int m = status == TRIP_OK ? (int)m64 : 0, N = 2 * m;
    const double Q = a.Q[f];
    const TripField F = { a.T + a.toff[f], a.E ? a.E + 2 * s0 : nullptr, a.X ? a.X + 2 * s0 : nullptr, a.In + 2 * s0, a.Out + 2 * s0, a.length + s0, cand0,
                          a.n_total, m, a.C, a.both_ways, Q, a.Q0 ? a.Q0[f] : Q, a.stop };
    if (status == TRIP_OK) {                   // (uniform: the whole workgroup is one field's)
        if (tid == 0) sh_bad = 0;
        __syncthreads();
        // the field's status before anything is indexed by a candidate: capacities, lengths, every candidate a permutation
        bool bad = !trip_capacity_ok(F.Q) || !trip_capacity_ok(F.Q0);
        for (int k = tid; k < m; k += TRBLOCK) bad |= !trip_length_ok(F.length[k]);
        for (int c0 = 0; c0 < a.C; c0 += TRWAVES) {
            const int c = c0 + wave;
            if (lane < ROUTE_MAX_SWATHS / 32) sh_seen[wave][lane] = 0;
            trip_wave_sync();
            if (c < a.C) {
                const int32_t *cand = F.tours + c * F.stride;
                for (int k = lane; k < m; k += 64) {
                    const int32_t p = cand[k];
                    if (p < 0 || p >= N) { bad = true; continue; }
                    const uint32_t bit = 1u << ((p >> 1) & 31);
                    if (atomicOr(&sh_seen[wave][p >> 6], bit) & bit) bad = true;
                }
            }
            trip_wave_sync();
        }
        if (bad) atomicOr(&sh_bad, 1);
        __syncthreads();
        if (!sh_bad) {
            TripWave &W = sh[wave];
            double best_total = INFINITY;
            int best_v = INT32_MAX;
            // (one direction: the even variants alone, dealt to all four wavefronts; the odd slots of the cost row are NaN)
            const int step = a.both_ways ? 1 : 2;
            if (!a.both_ways && tid < a.C) sh_costs[2 * tid + 1] = nan;
            for (int v = wave * step; v < n_var; v += TRWAVES * step) {           // (uniform within a wavefront)
                const TripVariant r = trip_variant_wave(F, v, W);
                if (lane == 0) sh_costs[v] = r.total;
                if (v == 0 && !tour_finite(r.base) && lane == 0) atomicOr(&sh_bad, 1);
                if (!trip_better(r.total, v, best_total, best_v)) continue;
                best_total = r.total; best_v = v;
                for (int k = lane; k < m; k += 64) W.mark[k] = 0;
                trip_wave_sync();
                if (lane == 0) {
                    int n_trips = 0, over = 0;
                    for (int i = r.last, j = m; i >= 0; j = i, i = W.pred[i]) {
                        W.mark[i] = 1;
                        ++n_trips;
                        if (trip_over(W.P[i], W.P[j], trip_cap(F, i))) ++over;
                        if (i == 0) break;
                    }
                    sh_base[wave] = r.base; sh_extra[wave] = r.extra; sh_trips[wave] = n_trips; sh_over[wave] = over;
                }
                trip_wave_sync();
            }
            if (lane == 0) { sh_total[wave] = best_total; sh_v[wave] = best_v; }
        }
        __syncthreads();
        if (sh_bad) status = TRIP_EINVAL;
    }
    double *costs = a.costs ? a.costs + f * n_var : nullptr;
    if (status != TRIP_OK) {                   // candidate 0 as given, one trip
        for (int64_t k = tid; k < m64; k += TRBLOCK) {
            if (a.tour) a.tour[s0 + k] = cand0[k];
            if (a.trip) a.trip[s0 + k] = 0;
        }
        if (costs && tid < n_var) costs[tid] = nan;
        if (tid != 0) return;
        if (a.cost) a.cost[f] = nan;
        if (a.base) a.base[f] = nan;
        if (a.extra) a.extra[f] = nan;
        if (a.n_trips) a.n_trips[f] = m64 > 0 ? 1 : 0;
        if (a.overfull) a.overfull[f] = 0;
        if (a.winner) a.winner[f] = 0;
        if (a.status) a.status[f] = status;
        return;
    }
    int ww = 0;                                // the wavefront that holds the winner: the least (total, v) of the four
#pragma unroll
    for (int x = 1; x < TRWAVES; ++x)
        if (trip_better(sh_total[x], sh_v[x], sh_total[ww], sh_v[ww])) ww = x;
    const int win = sh_v[ww];
    const int32_t *cand = F.tours + (win >> 1) * F.stride;
    if (a.tour)
        for (int k = tid; k < m; k += TRBLOCK) a.tour[s0 + k] = trip_at(cand, m, win & 1, k);
    if (a.trip && wave == 0) {
        int before = 0;                        // the trip starts before this round of 64 positions
        for (int k0 = 0; k0 < m; k0 += 64) {
            const int k = k0 + lane;
            const unsigned long long starts = __ballot(k < m && sh[ww].mark[k] != 0);
            if (k < m) a.trip[s0 + k] = before + __popcll(starts & ((2ull << lane) - 1ull)) - 1;
            before += __popcll(starts);
        }
    }
    if (costs && tid < n_var) costs[tid] = sh_costs[tid];
    if (tid != 0) return;
    if (a.cost) a.cost[f] = sh_total[ww];
    if (a.base) a.base[f] = sh_base[ww];
    if (a.extra) a.extra[f] = sh_extra[ww];
    if (a.n_trips) a.n_trips[f] = sh_trips[ww];
    if (a.overfull) a.overfull[f] = sh_over[ww];
    if (a.winner) a.winner[f] = win;
    if (a.status) a.status[f] = TRIP_OK;
}

// ---- launcher ---------------------------------------------------------------------------------------------------------------------------
int launch_trip_solve(hipStream_t st, int64_t n, const TripArgs &a)
{
    if (n <= 0) return 0;
    return launch(st, k_trip_solve, (unsigned)n, TRBLOCK, a);
}

}  // namespace fcpp
