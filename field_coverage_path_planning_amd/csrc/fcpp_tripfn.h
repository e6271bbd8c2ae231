// fcpp_tripfn.h -- service trips: after which swaths of a routed field to leave for the service point (a tank, a trailer at the gate), so
// that no trip works more than the vehicle's capacity and the added driving is least.  The split of a "giant tour": an exact dynamic
// programme over the positions of a tour, run on every candidate tour of the router in both driving directions; the cheapest total wins.
// ONE set of expressions for the host (fcpp_debug_trip_solve, the tests' checker) and the device (fcpp_trips.hip), in plain IEEE-754
// double operations compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the reference knows
// no capacity.  Path planning inside ONE field: nothing here orders fields or vehicles.
//
// THE RULE (include/fcpp.h states it for callers).
//   field     m swaths, N = 2 m oriented swaths p = 2 s + d as in the router's rule (fcpp_routefn.h); T its N x N transit block; E, X, In,
//             Out: N values each.  In[q]: from the service pose to the start of q; Out[p]: from the end of p to the service pose; E, X: the
//             first trip's way in and the last trip's way out (NULL = zeros).  length[s]: the work of swath s.  Q: the capacity in metres
//             of work, Q0 the first trip's (NULL = Q); stop: a price per stop in metres.
//   variant   v = 2 c + r of candidate tour c (1 <= C <= 64): r = 0 the tour t = tours[c] as given, r = 1 the same tour driven backwards,
//             t[k] = tours[c][m - 1 - k] ^ 1.  both_ways = 0: only r = 0.
//   tables    w_k = length[t[k] >> 1]; P[0] = 0, P[k + 1] = fl(P[k] + w_k); base = E[t[0]] + T[t[0]][t[1]] + .. + X[t[m - 1]], the router's
//             cost expression (route_cost) in its order; a stop between positions j - 1 and j, 1 <= j <= m - 1, costs
//             d_j = plus(fl(fl(Out[t[j - 1]] + In[t[j]]) - T[t[j - 1]][t[j]]), stop), plus = tour_plus of fcpp_tourfn.h: never NaN.
//   feasible  a trip over the positions i .. j - 1 iff j == i + 1 or fl(P[j] - P[i]) <= cap_i, cap_0 = Q0, cap_i = Q otherwise.  A swath
//             longer than the capacity is a trip of its own and counts in `overfull`; no field is infeasible.
//   programme g[0] = 0; g[j] = plus(d_j, min over feasible i < j of g[i]), the minimum over the pair (g[i], i) in lexicographic order
//             (ties to the lowest i), pred[j] that i; extra = min over i with (i, m) feasible of g[i], the same order; total =
//             plus(base, extra).  The order is total (no g is NaN), so any reduction tree gives the same pick.
//   result    the variant of least total, ties to the lowest v; its trip starts by backtracking pred from the final pick.  m = 0: no
//             trip, cost 0.
//   status    TRIP_EUNSUPPORTED for m > ROUTE_MAX_SWATHS (no block in T); TRIP_EINVAL for a candidate that is no permutation of the field's
//             swaths, a length that is negative or not finite, a capacity that is NaN or <= 0, candidate 0's base not finite.  For both:
//             tour = candidate 0 as given, trip all 0, n_trips = min(m, 1), overfull 0, winner 0, the costs NaN.
// The windows: P does not decrease, and rounded subtraction is monotone, so for i >= 1 a start that is infeasible for j stays infeasible
// for every later j: the device skips the starts below the first feasible one; the host walks every i.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_routefn.h"
#include "fcpp_tourfn.h"

namespace fcpp {

constexpr int TRIP_MAX_CANDIDATES = 64;
constexpr int TRIP_OK = 0, TRIP_EINVAL = -1, TRIP_EUNSUPPORTED = -3;         // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED

// a field: its block, its E, X (NULL: zeros), In, Out (N each), its swaths' lengths, candidate c's tour at tours[c * stride + k]
struct TripField {
    const double *T, *E, *X, *In, *Out, *length;
    const int32_t *tours;
    int64_t stride;
    int m, C, both_ways;
    double Q, Q0, stop;
};

// ---- variants ---------------------------------------------------------------------------------------------------------------------------
FCPP_HD int trip_n_variants(int C) { return 2 * C; }
FCPP_HD bool trip_exists(int v, int both_ways) { return both_ways || (v & 1) == 0; }
// position k of variant r of the candidate tour `cand` (m entries)
FCPP_HD int trip_at(const int32_t *cand, int m, int r, int k) { return r ? (cand[m - 1 - k] ^ 1) : cand[k]; }

// ---- the tables -------------------------------------------------------------------------------------------------------------------------
FCPP_HD bool trip_capacity_ok(double q) { return q > 0.0; }          // false for NaN; +inf is one trip
FCPP_HD bool trip_length_ok(double w) { return w >= 0.0 && tour_finite(w); }
FCPP_HD double trip_cap(const TripField &F, int i) { return i == 0 ? F.Q0 : F.Q; }
FCPP_HD bool trip_feasible(double Pi, double Pj, int i, int j, double cap) { return j == i + 1 || Pj - Pi <= cap; }
FCPP_HD bool trip_over(double Pi, double Pj, double cap) { return Pj - Pi > cap; }
// the price of a stop between the oriented swaths a and b, whose transit is e = T[a][b]
FCPP_HD double trip_stop(const TripField &F, int a, int b, double e) { return tour_plus((F.Out[a] + F.In[b]) - e, F.stop); }
FCPP_HD double trip_gate(const double *G, int p) { return G ? G[p] : 0.0; }
// is (g, i) before (bg, bi)?  (g is never NaN)
FCPP_HD bool trip_better(double g, int i, double bg, int bi) { return g < bg || (g == bg && i < bi); }

// is candidate c's tour a permutation of the field's swaths?  seen: m bytes of scratch
inline bool trip_permutation_host(const TripField &F, int c, uint8_t *seen)
{
    const int32_t *cand = F.tours + c * F.stride;
    for (int s = 0; s < F.m; ++s) seen[s] = 0;
    for (int k = 0; k < F.m; ++k) {
        const int32_t p = cand[k];
        if (p < 0 || p >= 2 * F.m || seen[p >> 1]) return false;
        seen[p >> 1] = 1;
    }
    return true;
}

// ---- the host twin: one field -----------------------------------------------------------------------------------------------------------
struct TripTables {          // of one variant; m <= ROUTE_MAX_SWATHS
    int16_t t[ROUTE_MAX_SWATHS], pred[ROUTE_MAX_SWATHS];
    double P[ROUTE_MAX_SWATHS + 1], g[ROUTE_MAX_SWATHS];
};
struct TripVariant { double base, extra, total; int last; };

// variant v of the field: its tables, its programme -> base, extra, total and the final pick (the start of the last trip; -1 for m = 0)
inline TripVariant trip_variant_host(const TripField &F, int v, TripTables &W)
{
    const int m = F.m, N = 2 * m, r = v & 1;
    const int32_t *cand = F.tours + (v >> 1) * F.stride;
    W.P[0] = 0.0;
    for (int k = 0; k < m; ++k) {
        W.t[k] = (int16_t)trip_at(cand, m, r, k);
        W.P[k + 1] = W.P[k] + F.length[W.t[k] >> 1];
    }
    const RouteCosts rc = { F.T, F.E, F.X, N };
    TripVariant out = { route_cost(rc, W.t, m), 0.0, 0.0, -1 };
    if (m > 0) {
        W.g[0] = 0.0;
        for (int j = 1; j <= m; ++j) {
            double bg = INFINITY;
            int bi = INT32_MAX;
            for (int i = 0; i < j; ++i)
                if (trip_feasible(W.P[i], W.P[j], i, j, trip_cap(F, i)) && trip_better(W.g[i], i, bg, bi)) { bg = W.g[i]; bi = i; }
            if (j == m) { out.extra = bg; out.last = bi; break; }
            const int a = W.t[j - 1], b = W.t[j];
            W.g[j] = tour_plus(trip_stop(F, a, b, F.T[a * N + b]), bg);
            W.pred[j] = (int16_t)bi;
        }
    }
    out.total = tour_plus(out.base, out.extra);
    return out;
}

struct TripResult { double cost, base, extra; int n_trips, overfull, winner, status; };

// the field's status before any variant is solved, candidate 0's base aside; seen: m bytes of scratch
inline int trip_status_host(const TripField &F, int64_t m64, uint8_t *seen)
{
    if (m64 > ROUTE_MAX_SWATHS) return TRIP_EUNSUPPORTED;
    if (!trip_capacity_ok(F.Q) || !trip_capacity_ok(F.Q0)) return TRIP_EINVAL;
    for (int s = 0; s < F.m; ++s)
        if (!trip_length_ok(F.length[s])) return TRIP_EINVAL;
    for (int c = 0; c < F.C; ++c)
        if (!trip_permutation_host(F, c, seen)) return TRIP_EINVAL;
    return TRIP_OK;
}

// One field of m64 swaths (F.m = m64 where that is within the cap).  tour, trip: the field's m entries or NULL; costs: 2 C or NULL.
inline TripResult trip_field_host(const TripField &F, int64_t m64, int32_t *tour, int32_t *trip, double *costs)
{
    const double nan = __builtin_nan("");
    const int n_var = trip_n_variants(F.C);
    uint8_t mark[ROUTE_MAX_SWATHS];
    TripTables W, best;
    TripVariant bv = { nan, nan, nan, -1 };
    int win = 0;
    int status = trip_status_host(F, m64, mark);
    if (status == TRIP_OK) {
        for (int v = 0; v < n_var; ++v) {
            if (!trip_exists(v, F.both_ways)) { if (costs) costs[v] = nan; continue; }
            const TripVariant r = trip_variant_host(F, v, W);
            if (v == 0 && !tour_finite(r.base)) { status = TRIP_EINVAL; break; }
            if (costs) costs[v] = r.total;
            if (v == 0 || r.total < bv.total) { bv = r; win = v; best = W; }
        }
    }
    if (status != TRIP_OK) {
        for (int64_t k = 0; k < m64; ++k) {
            if (tour) tour[k] = F.tours[k];
            if (trip) trip[k] = 0;
        }
        if (costs) for (int v = 0; v < n_var; ++v) costs[v] = nan;
        return { nan, nan, nan, m64 > 0 ? 1 : 0, 0, 0, status };
    }
    const int m = F.m;
    TripResult out = { bv.total, bv.base, bv.extra, 0, 0, win, TRIP_OK };
    for (int k = 0; k < m; ++k) mark[k] = 0;
    for (int i = bv.last, j = m; i >= 0; j = i, i = best.pred[i]) {
        mark[i] = 1;
        ++out.n_trips;
        if (trip_over(best.P[i], best.P[j], trip_cap(F, i))) ++out.overfull;
        if (i == 0) break;
    }
    for (int k = 0, at = -1; k < m; ++k) {
        at += mark[k];
        if (tour) tour[k] = best.t[k];
        if (trip) trip[k] = at;
    }
    return out;
}

}  // namespace fcpp
