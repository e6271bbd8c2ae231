// fcpp_routefn.h -- the swath router: in which ORDER and DIRECTION to drive the swaths of one field (fcpp_swath_fill's records), with the
// transits priced by the Dubins or Reeds-Shepp connectors.  ONE set of expressions for the host (fcpp_debug_route_transit,
// fcpp_debug_route, the tests' checker) and the device (fcpp_route.hip), written like fcpp_swathfn.h in plain IEEE-754 double operations and
// compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the reference drives the stored order.
// Path planning inside ONE field: nothing here orders fields or vehicles.
//
// THE RULE (include/fcpp.h states it for callers).
//   oriented  a field has m swath records s = 0 .. m - 1 in the stored order.  Oriented swath p = 2 s + d: d = 0 drives a -> b with heading
//             theta, d = 1 drives b -> a with heading fl(theta + pi).  p ^ 1 is the same swath the other way ("p-bar").  N = 2 m.
//   transit   T, N x N row-major: T[p][q] = the shortest connector length from the exit pose of p to the entry pose of q at radius R, mode 0
//             Dubins (dubins_solve), mode 1 Reeds-Shepp (rs_solve); +inf where p and q are the same swath.  A path driven backwards with
//             the headings flipped is again a path, so T[p][q] = T[q-bar][p-bar] mathematically; to make that hold in BITS every entry is
//             evaluated on its canonical pair -- of (p, q) and (q-bar, p-bar) the one with the smaller key p N + q -- and both entries get
//             that value.  The reversal moves below rely on it: the edges inside a reversed segment keep their value.
//   cost      a tour t[0 .. m - 1] holds one oriented swath of every swath.  cost = E[t[0]] + T[t[0]][t[1]] + .. + X[t[m - 1]], added left to
//             right; E, X (N each, NULL = zeros): from the field's entry pose to each oriented swath, from each to the field's exit pose.
//             e(u, v) below: e(START, q) = E[q], e(p, END) = X[p], else T[u][v].
//   candidate c = 0 .. S - 1 (1 <= S <= 64): c = 0 the stored boustrophedon t[k] = 2 k + (k & 1); c = 1 its mirror t[k] = 2 k + 1 - (k & 1);
//             c >= 2 nearest neighbour from the oriented swath floor((c - 2) N / (S - 2)): repeatedly the orientation q of an unvisited
//             swath with the least T[cur][q], ties to the lowest q (an entry that is not below +inf -- NaN included -- counts as +inf).
//   sweeps    a sweep evaluates EVERY move of the set below on the current tour, takes the one with the least delta, ties to the lowest
//             code, and applies it iff delta < -min_gain; otherwise the candidate is finished; it also stops after max_sweeps sweeps.
//             removed and added are each summed left to right, delta = added - removed.  A NaN delta compares false: never taken.
//     move A  reverse(i, j), 0 <= i <= j < m, code i m + j: t[i .. j] reversed and every member flipped (i = j turns one swath round).
//             u = the node at i - 1 or START, v = the node at j + 1 or END.
//             removed = e(u, t[i]) + e(t[j], v);  added = e(u, t[j]-bar) + e(t[i]-bar, v).
//     move B  or-opt, needs m > l: the segment t[i .. i + l - 1], l in {1, 2, 3}, moved to between positions k and k + 1 of the tour,
//             k in [-1, m - 1] with k < i - 1 or k >= i + l; r = 0 as it is, r = 1 reversed and flipped.
//             code m m + (((l - 1) 2 + r) m + i) (m + 1) + (k + 1).  f = t[i], g = t[i + l - 1]; (in, out) = (f, g) for r = 0, (g-bar, f-bar)
//             for r = 1; u, v the segment's neighbours, a, b the nodes at k and k + 1 (START / END at the ends).
//             removed = (e(u, f) + e(g, v)) + e(a, b);  added = (e(u, v) + e(a, in)) + e(out, b).
//   result    every candidate's final cost is recomputed from its final tour.  The winner: the least cost, ties to the lowest c (a NaN cost
//             never wins over candidate 0).  sweeps: the largest number of moves any candidate applied (below max_sweeps: none stopped on it).
//   status    ROUTE_EUNSUPPORTED for m > ROUTE_MAX_SWATHS (the field has no block in T; every candidate's tour is the stored order, the
//             costs are NaN); ROUTE_EINVAL when candidate 0's cost as constructed is not finite (nothing is improved: every candidate stays
//             as constructed).  For either the route is candidate 0 as constructed, the winner 0.
// min_gain >= 0 far above the rounding of a delta makes the true cost fall with every applied move, so the loop ends; max_sweeps bounds it
// regardless.  The minimum over (delta, code) pairs does not depend on the order in which the moves are looked at, and every delta comes
// from one expression: the device may hand the codes to its threads in any way.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_connfn.h"

namespace fcpp {

constexpr int ROUTE_MAX_SWATHS = 512;                    // FCPP_ROUTE_MAX_SWATHS of include/fcpp.h
constexpr int ROUTE_MAX_STARTS = 64;
constexpr int ROUTE_MAX_SWEEPS = 1 << 20;
constexpr int ROUTE_OK = 0, ROUTE_EINVAL = -1, ROUTE_EUNSUPPORTED = -3;      // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr int ROUTE_START = -1, ROUTE_END = -2;          // the nodes before position 0 and behind position m - 1

// the size of a field's block of T: (2 m)^2, none beyond the cap
FCPP_HD int64_t route_block(int64_t m) { return m > ROUTE_MAX_SWATHS ? 0 : 4 * m * m; }

// ---- transit ----------------------------------------------------------------------------------------------------------------------
// the pose at which oriented swath p is left (exit) or entered; ax .. by: the field's records
FCPP_HD void route_pose(const double *ax, const double *ay, const double *bx, const double *by, double theta, int p, bool exit, double &x,
                        double &y, double &h)
{
    const int s = p >> 1, d = p & 1;
    const bool at_b = (d == 0) == exit;                  // d = 0 enters at a and leaves at b, d = 1 the other way
    x = at_b ? bx[s] : ax[s];
    y = at_b ? by[s] : ay[s];
    h = d ? theta + kPi : theta;
}

// is (p, q) the pair its entry is evaluated on?  (the other one: (q ^ 1, p ^ 1))
FCPP_HD bool route_canonical(int p, int q, int N) { return p * N + q <= (q ^ 1) * N + (p ^ 1); }

// the connector length of the pair AS GIVEN (the caller passes the canonical one); MODE 0 Dubins, 1 Reeds-Shepp
template <int MODE>
FCPP_HD double route_transit(const double *ax, const double *ay, const double *bx, const double *by, double theta, double R, int p, int q)
{
    if ((p >> 1) == (q >> 1)) return INFINITY;
    double x0, y0, h0, x1, y1, h1, total;
    route_pose(ax, ay, bx, by, theta, p, true, x0, y0, h0);
    route_pose(ax, ay, bx, by, theta, q, false, x1, y1, h1);
    int word;
    double seg[Conn<MODE>::NSEG];
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, R, word, seg, total);
    return total;
}

// ---- tours ------------------------------------------------------------------------------------------------------------------------
struct RouteCosts { const double *T, *E, *X; int N; };          // a field's block and its E, X (NULL: zeros)

FCPP_HD double route_edge(const RouteCosts &c, int u, int v)
{
    if (u < 0) return (v < 0 || !c.E) ? 0.0 : c.E[v];
    if (v < 0) return c.X ? c.X[u] : 0.0;
    return c.T[u * c.N + v];
}

FCPP_HD int route_node(const int16_t *t, int m, int k) { return k < 0 ? ROUTE_START : (k >= m ? ROUTE_END : (int)t[k]); }

FCPP_HD bool route_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }          // false for NaN

FCPP_HD double route_cost(const RouteCosts &c, const int16_t *t, int m)
{
    if (m <= 0) return 0.0;
    double sum = route_edge(c, ROUTE_START, t[0]);
    for (int k = 0; k + 1 < m; ++k) sum += route_edge(c, t[k], t[k + 1]);
    return sum + route_edge(c, t[m - 1], ROUTE_END);
}

// candidates 0 and 1 at position k; where a nearest-neighbour candidate starts; what it compares
FCPP_HD int route_stored(int c, int k) { return 2 * k + (c == 0 ? (k & 1) : 1 - (k & 1)); }
FCPP_HD int route_nn_start(int c, int S, int N) { return (int)((int64_t)(c - 2) * N / (S - 2)); }
FCPP_HD double route_nn_key(double v) { return v < INFINITY ? v : INFINITY; }

// ---- moves ------------------------------------------------------------------------------------------------------------------------
struct RouteMove { int kind, i, j, l, r, k; };          // kind 0: A (i, j); 1: B (i, l, r, k)

FCPP_HD int route_n_codes(int m) { return m * m + 6 * m * (m + 1); }          // 1 837 056 at the cap

// the move of a code in [0, route_n_codes(m)); false for a code that names no move
FCPP_HD bool route_decode(int m, int code, RouteMove &mv)
{
    if (code < m * m) {
        mv.kind = 0; mv.i = code / m; mv.j = code - mv.i * m; mv.l = 0; mv.r = 0; mv.k = 0;
        return mv.i <= mv.j;
    }
    int c = code - m * m;
    const int kk = c % (m + 1);
    c /= m + 1;
    mv.kind = 1; mv.i = c % m; mv.j = 0;
    c /= m;
    mv.r = c & 1; mv.l = (c >> 1) + 1; mv.k = kk - 1;
    return m > mv.l && mv.i + mv.l <= m && (mv.k < mv.i - 1 || mv.k >= mv.i + mv.l);
}

FCPP_HD double route_delta(const RouteCosts &c, const int16_t *t, int m, const RouteMove &mv)
{
    if (mv.kind == 0) {
        const int u = route_node(t, m, mv.i - 1), v = route_node(t, m, mv.j + 1), f = t[mv.i], g = t[mv.j];
        const double removed = route_edge(c, u, f) + route_edge(c, g, v);
        const double added = route_edge(c, u, g ^ 1) + route_edge(c, f ^ 1, v);
        return added - removed;
    }
    const int f = t[mv.i], g = t[mv.i + mv.l - 1], in = mv.r ? g ^ 1 : f, out = mv.r ? f ^ 1 : g;
    const int u = route_node(t, m, mv.i - 1), v = route_node(t, m, mv.i + mv.l), a = route_node(t, m, mv.k), b = route_node(t, m, mv.k + 1);
    const double removed = (route_edge(c, u, f) + route_edge(c, g, v)) + route_edge(c, a, b);
    const double added = (route_edge(c, u, v) + route_edge(c, a, in)) + route_edge(c, out, b);
    return added - removed;
}

// position p of the tour AFTER the move, read from the tour before it
FCPP_HD int route_moved(const int16_t *t, const RouteMove &mv, int p)
{
    if (mv.kind == 0) return (p < mv.i || p > mv.j) ? (int)t[p] : (t[mv.i + mv.j - p] ^ 1);
    const int i = mv.i, l = mv.l, at = mv.k < i ? mv.k + 1 : mv.k + 1 - l;          // where the segment starts afterwards
    if (p >= at && p < at + l) return mv.r ? (t[i + l - 1 - (p - at)] ^ 1) : (int)t[i + (p - at)];
    const int q = p < at ? p : p - l;                                              // p's rank among the others
    return t[q < i ? q : q + l];
}

// is (d, code) better than (bd, bc)?  (never for a NaN d)
FCPP_HD bool route_better(double d, int code, double bd, int bc) { return d < bd || (d == bd && code < bc); }

// ---- the host twin: one candidate, one field ------------------------------------------------------------------------------------------
// candidate c of S as constructed, in t[0 .. m - 1] (m <= ROUTE_MAX_SWATHS); seen: m bytes of scratch
inline void route_construct_host(const RouteCosts &rc, int m, int c, int S, int16_t *t, uint8_t *seen)
{
    if (c < 2) { for (int k = 0; k < m; ++k) t[k] = (int16_t)route_stored(c, k); return; }
    if (m == 0) return;
    for (int k = 0; k < m; ++k) seen[k] = 0;
    int cur = route_nn_start(c, S, rc.N);
    t[0] = (int16_t)cur; seen[cur >> 1] = 1;
    for (int k = 1; k < m; ++k) {
        double bv = INFINITY;
        int bq = INT32_MAX;
        for (int q = 0; q < rc.N; ++q) {
            if (seen[q >> 1]) continue;
            const double v = route_nn_key(rc.T[cur * rc.N + q]);
            if (route_better(v, q, bv, bq)) { bv = v; bq = q; }
        }
        cur = bq;
        t[k] = (int16_t)cur; seen[cur >> 1] = 1;
    }
}

// the sweeps on t (tmp: m entries of scratch) -> the number of moves applied
inline int route_improve_host(const RouteCosts &rc, int m, double min_gain, int max_sweeps, int16_t *t, int16_t *tmp)
{
    const int n_codes = route_n_codes(m);
    int applied = 0;
    while (applied < max_sweeps) {
        double bd = INFINITY;
        int bc = INT32_MAX;
        RouteMove mv;
        for (int code = 0; code < n_codes; ++code) {
            if (!route_decode(m, code, mv)) continue;
            const double d = route_delta(rc, t, m, mv);
            if (route_better(d, code, bd, bc)) { bd = d; bc = code; }
        }
        if (!(bd < -min_gain)) break;
        (void)route_decode(m, bc, mv);
        for (int p = 0; p < m; ++p) tmp[p] = (int16_t)route_moved(t, mv, p);
        for (int p = 0; p < m; ++p) t[p] = tmp[p];
        ++applied;
    }
    return applied;
}

// One field: T its block (unused for m > ROUTE_MAX_SWATHS), E, X its N entries or NULL.  tours: candidate c's at tours[c * stride + k] (int32)
// or NULL; costs: S or NULL; route: m or NULL.  The winner's cost, the winner, the sweeps, the status and candidate 0's cost as constructed.
struct RouteField { double cost, stored; int winner, sweeps, status; };
inline RouteField route_field_host(const double *T, const double *E, const double *X, int64_t m64, int S, double min_gain, int max_sweeps,
                                   int32_t *tours, int64_t stride, double *costs, int32_t *route)
{
    const double nan = __builtin_nan("");
    if (m64 > ROUTE_MAX_SWATHS) {
        for (int c = 0; c < S; ++c) {
            if (tours) for (int64_t k = 0; k < m64; ++k) tours[c * stride + k] = (int32_t)(2 * k + (k & 1));
            if (costs) costs[c] = nan;
        }
        if (route) for (int64_t k = 0; k < m64; ++k) route[k] = (int32_t)(2 * k + (k & 1));
        return { nan, nan, 0, 0, ROUTE_EUNSUPPORTED };
    }
    const int m = (int)m64;
    const RouteCosts rc = { T, E, X, 2 * m };
    int16_t t[ROUTE_MAX_SWATHS], tmp[ROUTE_MAX_SWATHS], best_t[ROUTE_MAX_SWATHS];
    uint8_t seen[ROUTE_MAX_SWATHS];
    route_construct_host(rc, m, 0, S, t, seen);
    const double stored = route_cost(rc, t, m);
    const bool improve = route_finite(stored);
    RouteField out = { stored, stored, 0, 0, improve ? ROUTE_OK : ROUTE_EINVAL };
    for (int c = 0; c < S; ++c) {
        route_construct_host(rc, m, c, S, t, seen);
        const int applied = improve ? route_improve_host(rc, m, min_gain, max_sweeps, t, tmp) : 0;
        const double cost = route_cost(rc, t, m);
        if (tours) for (int k = 0; k < m; ++k) tours[c * stride + k] = t[k];
        if (costs) costs[c] = cost;
        if (applied > out.sweeps) out.sweeps = applied;
        if (c == 0 || (improve && cost < out.cost)) {
            out.cost = cost; out.winner = c;
            for (int k = 0; k < m; ++k) best_t[k] = t[k];
        }
    }
    if (route) for (int k = 0; k < m; ++k) route[k] = best_t[k];
    return out;
}

}  // namespace fcpp
