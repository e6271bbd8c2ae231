// fcpp_fleetfn.h -- vehicle shares: which contiguous stretch of a routed field's tour each of K vehicles drives from a common depot and
// back, so that the vehicle that finishes last finishes as early as possible -- and, among the splits that are as balanced as that, the
// one of least summed cost.  Two exact dynamic programmes over the positions of a tour (a min-max one, then a min-sum one under its
// bound), run on every candidate tour of the router in both driving directions; the least (makespan, sum) wins.
// ONE set of expressions for the host (fcpp_debug_fleet_solve, the tests' checker) and the device (fcpp_fleet.hip), in plain IEEE-754
// double operations compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined.  Path planning inside
// ONE field: the vehicles share one depot, one speed and one width; nothing here orders fields.
//
// THE RULE (include/fcpp.h states it for callers).
//   field     m swaths, N = 2 m oriented swaths p = 2 s + d as in the router's rule (fcpp_routefn.h); T its N x N transit block; In[q]: from
//             the depot pose to the start of q; Out[p]: from the end of p to the depot (N values each); length[s]: the work of swath s;
//             K: the number of vehicles, 1 <= K <= FLEET_MAX_VEHICLES; omega >= 0: the weight of a metre of work against a metre of
//             driving (transit speed / working speed), so a share's cost is proportional to its time.
//   variant   the trips' (fcpp_tripfn.h): v = 2 c + r of candidate tour c (1 <= C <= 64), r = 1 the tour driven backwards, t[k] =
//             tours[c][m - 1 - k] ^ 1; both_ways = 0: only r = 0.
//   tables    P[0] = 0, P[k + 1] = fl(P[k] + length[t[k] >> 1]); S[0] = 0, S[k] = fl(S[k - 1] + T[t[k - 1]][t[k]]) for k = 1 .. m - 1.
//   share     the positions i .. j - 1 (0 <= i < j <= m) driven by one vehicle from the depot and back cost
//             c(i, j) = plus(fl(fl(In[t[i]] + fl(S[j - 1] - S[i])) + Out[t[j - 1]]), fl(omega * fl(P[j] - P[i]))), plus = tour_plus of
//             fcpp_tourfn.h: never NaN, every sum that is not below +inf is +inf.
//   stage 1   G_1[j] = c(0, j); G_k[j] = min over k - 1 <= i < j of max(G_(k-1)[i], c(i, j)) for k <= j; M = min over 1 <= k <= min(K, m) of
//             G_k[m].  max and min do not round: M is the exact least, over every split of the tour into AT MOST K non-empty contiguous
//             shares, of the largest share cost.  (A further vehicle adds its own In and Out and can make things worse.)
//   stage 2   H_0[0] = 0; H_k[j] = min over the starts i for which H_(k-1)[i] exists and c(i, j) <= M of plus(c(i, j), H_(k-1)[i]), the
//             pair (value, i) in lexicographic order (i ascending, strict "less than"), pred_k[j] that i; H_k[j] exists iff such an i
//             does.  sum = the least (H_k[m], k) over the k <= min(K, m) for which it exists; one does, since M is attained.  Rounded
//             addition is monotone, so sum is the least left-to-right rounded sum of share costs over all splits with every share <= M.
//   result    the variant of least (M, sum, v), lexicographically; its shares by backtracking pred from (k, m).  m = 0: no share,
//             makespan 0, sum 0.
//   status    FLEET_EUNSUPPORTED for m > ROUTE_MAX_SWATHS (no block in T) or K > FLEET_MAX_VEHICLES; FLEET_EINVAL for K < 1 or K beyond the
//             row length of the per-share outputs, a candidate that is no permutation of the field's swaths, a length that is negative or
//             not finite, candidate 0's S[m - 1] not finite.  For both: tour = candidate 0 as given, share all 0, n_used = min(m, 1),
//             winner 0, share_first = 0 for that one share, every cost NaN.
// The windows are NOT monotone in floating point (S[j - 1] - S[i] is a difference of rounded prefix sums): no start is skipped.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_routefn.h"
#include "fcpp_tourfn.h"
#include "fcpp_tripfn.h"

namespace fcpp {

constexpr int FLEET_MAX_VEHICLES = 16;                   // FCPP_FLEET_MAX_VEHICLES of include/fcpp.h
constexpr int FLEET_OK = 0, FLEET_EINVAL = -1, FLEET_EUNSUPPORTED = -3;      // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED

// a field: its block, its In, Out (N each), its swaths' lengths, candidate c's tour at tours[c * stride + k]
struct FleetField {
    const double *T, *In, *Out, *length;
    const int32_t *tours;
    int64_t stride;
    int m, C, both_ways, K, k_stride;
    double omega;
};

// ---- the expressions --------------------------------------------------------------------------------------------------------------------
FCPP_HD double fleet_max(double a, double b) { return a < b ? b : a; }          // (neither is NaN)
FCPP_HD bool fleet_is(double h) { return h == h; }                               // a stage-2 value that exists (NaN: it does not)
FCPP_HD int fleet_layers(int K, int m) { return K < m ? K : m; }
// c(i, j) from In[t[i]], S[i], P[i] and S[j - 1], Out[t[j - 1]], P[j]
FCPP_HD double fleet_cost(double in_i, double Si, double Pi, double Sj1, double out_j, double Pj, double omega)
{
    return tour_plus((in_i + (Sj1 - Si)) + out_j, omega * (Pj - Pi));
}
// is the variant (M, sum, v) before (bM, bsum, bv)?
FCPP_HD bool fleet_better(double M, double sum, int v, double bM, double bsum, int bv)
{
    return M < bM || (M == bM && (sum < bsum || (sum == bsum && v < bv)));
}
// the field's status from its sizes alone
FCPP_HD int fleet_size_status(int64_t m64, int K, int k_stride)
{
    if (m64 > ROUTE_MAX_SWATHS || K > FLEET_MAX_VEHICLES) return FLEET_EUNSUPPORTED;
    if (K < 1 || K > k_stride) return FLEET_EINVAL;
    return FLEET_OK;
}

// ---- the host twin: one field -----------------------------------------------------------------------------------------------------------
struct FleetTables {         // of one variant; m <= ROUTE_MAX_SWATHS
    int16_t t[ROUTE_MAX_SWATHS], pred[FLEET_MAX_VEHICLES][ROUTE_MAX_SWATHS + 1];
    double P[ROUTE_MAX_SWATHS + 1], S[ROUTE_MAX_SWATHS], A[ROUTE_MAX_SWATHS], B[ROUTE_MAX_SWATHS], row[2][ROUTE_MAX_SWATHS + 1];
};
struct FleetVariant { double M, sum; int k; };          // k: the shares used

inline double fleet_cost_host(const FleetField &F, const FleetTables &W, int i, int j)
{
    return fleet_cost(W.A[i], W.S[i], W.P[i], W.S[j - 1], W.B[j - 1], W.P[j], F.omega);
}

// the tables of variant v: t, P, S and the ways in and out per position (A[k] = In[t[k]], B[k] = Out[t[k]])
inline void fleet_tables_host(const FleetField &F, int v, FleetTables &W)
{
    const int m = F.m, N = 2 * m, r = v & 1;
    const int32_t *cand = F.tours + (v >> 1) * F.stride;
    W.P[0] = 0.0;
    for (int k = 0; k < m; ++k) {
        W.t[k] = (int16_t)trip_at(cand, m, r, k);
        W.P[k + 1] = W.P[k] + F.length[W.t[k] >> 1];
        W.A[k] = F.In[W.t[k]];
        W.B[k] = F.Out[W.t[k]];
        W.S[k] = k == 0 ? 0.0 : W.S[k - 1] + F.T[W.t[k - 1] * N + W.t[k]];
    }
}

// variant v of the field (m > 0, its tables in W): both stages -> M, sum, the shares used; pred stays in W
inline FleetVariant fleet_variant_host(const FleetField &F, FleetTables &W)
{
    const int m = F.m, Kc = fleet_layers(F.K, m);
    const double nan = __builtin_nan("");
    if (m == 0) return { 0.0, 0.0, 0 };
    // stage 1: layer 0 is the empty split, below every cost
    double M = INFINITY;
    int cur = 1;
    W.row[0][0] = -INFINITY;
    for (int k = 1; k <= Kc; ++k, cur ^= 1) {
        const double *prev = W.row[cur ^ 1];
        for (int j = k; j <= m; ++j) {
            double bg = INFINITY;
            for (int i = k - 1, end = k == 1 ? 1 : j; i < end; ++i) {
                const double g = fleet_max(prev[i], fleet_cost_host(F, W, i, j));
                if (g < bg) bg = g;
            }
            W.row[cur][j] = bg;
        }
        if (W.row[cur][m] < M) M = W.row[cur][m];
    }
    // stage 2
    FleetVariant out = { M, nan, 0 };
    cur = 1;
    W.row[0][0] = 0.0;
    for (int k = 1; k <= Kc; ++k, cur ^= 1) {
        const double *prev = W.row[cur ^ 1];
        for (int j = k; j <= m; ++j) {
            double bh = 0.0;
            int bi = -1;
            for (int i = k - 1, end = k == 1 ? 1 : j; i < end; ++i) {
                const double c = fleet_cost_host(F, W, i, j);
                if (!fleet_is(prev[i]) || !(c <= M)) continue;
                const double h = tour_plus(c, prev[i]);
                if (bi < 0 || h < bh) { bh = h; bi = i; }
            }
            W.row[cur][j] = bi < 0 ? nan : bh;
            W.pred[k - 1][j] = (int16_t)bi;
        }
        const double h = W.row[cur][m];
        if (fleet_is(h) && (out.k == 0 || h < out.sum)) { out.sum = h; out.k = k; }
    }
    return out;
}

// is candidate c's tour a permutation of the field's swaths?  seen: m bytes of scratch
inline bool fleet_permutation_host(const FleetField &F, int c, uint8_t *seen)
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

// the field's status before any variant is solved, candidate 0's S aside; seen: m bytes of scratch
inline int fleet_status_host(const FleetField &F, int64_t m64, uint8_t *seen)
{
    const int status = fleet_size_status(m64, F.K, F.k_stride);
    if (status != FLEET_OK) return status;
    for (int s = 0; s < F.m; ++s)
        if (!trip_length_ok(F.length[s])) return FLEET_EINVAL;
    for (int c = 0; c < F.C; ++c)
        if (!fleet_permutation_host(F, c, seen)) return FLEET_EINVAL;
    return FLEET_OK;
}

struct FleetResult { double makespan, total; int n_used, winner, status; };

// One field of m64 swaths (F.m = m64 where that is within the cap).  tour, share: the field's m entries or NULL; makespans, totals: 2 C or
// NULL; share_first, share_cost: k_stride or NULL.
inline FleetResult fleet_field_host(const FleetField &F, int64_t m64, int32_t *tour, int32_t *share, double *makespans, double *totals,
                                    int32_t *share_first, double *share_cost)
{
    const double nan = __builtin_nan("");
    const int n_var = trip_n_variants(F.C);
    uint8_t mark[ROUTE_MAX_SWATHS];
    FleetTables *W = new FleetTables, *best = new FleetTables;
    FleetVariant bv = { nan, nan, 0 };
    int win = 0;
    int status = fleet_status_host(F, m64, mark);
    if (status == FLEET_OK) {
        for (int v = 0; v < n_var; ++v) {
            if (!trip_exists(v, F.both_ways)) {
                if (makespans) makespans[v] = nan;
                if (totals) totals[v] = nan;
                continue;
            }
            fleet_tables_host(F, v, *W);
            if (v == 0 && F.m > 0 && !tour_finite(W->S[F.m - 1])) { status = FLEET_EINVAL; break; }
            const FleetVariant r = fleet_variant_host(F, *W);
            if (makespans) makespans[v] = r.M;
            if (totals) totals[v] = r.sum;
            if (v == 0 || fleet_better(r.M, r.sum, v, bv.M, bv.sum, win)) { bv = r; win = v; *best = *W; }
        }
    }
    for (int k = 0; share_first && k < F.k_stride; ++k) share_first[k] = -1;
    for (int k = 0; share_cost && k < F.k_stride; ++k) share_cost[k] = nan;
    if (status != FLEET_OK) {
        for (int64_t k = 0; k < m64; ++k) {
            if (tour) tour[k] = F.tours[k];
            if (share) share[k] = 0;
        }
        for (int v = 0; v < n_var; ++v) {
            if (makespans) makespans[v] = nan;
            if (totals) totals[v] = nan;
        }
        if (share_first && m64 > 0 && F.k_stride > 0) share_first[0] = 0;
        delete W; delete best;
        return { nan, nan, m64 > 0 ? 1 : 0, 0, status };
    }
    const int m = F.m;
    for (int k = bv.k, j = m; k > 0; --k) {
        const int i = best->pred[k - 1][j];
        if (share_first) share_first[k - 1] = i;
        if (share_cost) share_cost[k - 1] = fleet_cost_host(F, *best, i, j);
        for (int q = i; q < j; ++q) {
            if (share) share[q] = k - 1;
        }
        j = i;
    }
    for (int k = 0; tour && k < m; ++k) tour[k] = best->t[k];
    const FleetResult out = { bv.M, bv.sum, bv.k, win, FLEET_OK };
    delete W; delete best;
    return out;
}

}  // namespace fcpp
