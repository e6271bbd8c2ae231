// fcpp_transitfn.h -- loop transits: a pair of poses P -> Q joined by a clear connector to a station of a headland loop, a ride along the
// loop's own samples and a clear connector from a second station of that loop.  ONE set of expressions for the host
// (fcpp_debug_loop_transits, the tests' driver) and the device (fcpp_transit.hip), in plain IEEE-754 double operations and compiled with
// -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the reference has no obstacles to ride round.
//
// Nothing geometric is written here.  A connector is what the clear-connector rule (solve_clear of fcpp_solveclearfn.h: candidates, order
// (total, word), test, rank) gives; a ride is a run of samples somebody else made, copied.
//
// THE RULE (include/fcpp.h states it for callers).
//   loops     a path set in the samplers' CSR form: loop l owns the samples loop_off[l] .. loop_off[l + 1]; per sample x, y, heading,
//             kappa, part, gear and s, the arc length from the loop's first sample (fcpp_trajectory's s: never decreasing).  S_l is the s of
//             the loop's last sample.  Field f is served by the loops field_loops[f] .. field_loops[f + 1].  A loop is closed and driven
//             forwards only, so a ride may wrap over its end; the caller offers the other direction as a second loop.
//   station   a sample of local index k with k mod stride == 0, part 0 or 4 (a straight element, a followed arc) and gear +1; its pose is
//             the sample's (x, y, heading).
//   in, out   in_i = the len solve_clear gives for P -> station i against region field f, out_j the same for station j -> Q; +inf unless
//             rank >= 0.
//   ride      i, j stations of ONE loop: fl(s_j - s_i) for j >= i, fl(fl(S_l - s_i) + s_j) for j < i (the wrap); i == j is a via point.
//   cost      C = fl(fl(in_i + ride) + out_j); the transit of a pair is the least C below +inf over (l, i, j), ties by (C, l, i, j)
//             ascending.  i and j are reported as GLOBAL sample indices, which order as (l, local index) does.
//   status    TRANSIT_EINVAL for a pose that is not finite, a field index outside 0 .. n_fields - 1, a region field of status CLEAR_EINVAL,
//             a field with a loop whose first or last s is not finite; TRANSIT_EUNSUPPORTED for a field of more than
//             TRANSIT_MAX_STATIONS stations; else 0.  A pair of status 0 whose field has no loop, no station or no finite C is not found.
//   not found found 0, loop / i / j -1, both words -1 with NaN seg and len and rank -1, ride NaN, total +inf.
//   path      K_in samples of the in-connector (Conn<MODE>::count / ::eval, part 1), then the loop's samples i .. j copied bit for bit,
//             through the loop's end when j < i (part TRANSIT_PART_RIDE, their own gear and kappa), then K_out samples of the out-connector
//             from station j's pose (part 1).  Junctions stay doubled.  A pair that is not found has no samples.
// The ride is NOT tested against the region: a headland pass lies inside its field by construction, its corner connectors may not.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_fpathfn.h"
#include "fcpp_solveclearfn.h"

namespace fcpp {

constexpr int TRANSIT_MAX_STATIONS = 2048;              // FCPP_TRANSIT_MAX_STATIONS of include/fcpp.h
constexpr int TRANSIT_OK = 0, TRANSIT_EINVAL = -1, TRANSIT_EUNSUPPORTED = -3;          // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr int TRANSIT_PART_CONN = 1, TRANSIT_PART_RIDE = 5;                            // FCPP_PART_LOOP_RIDE

// the loop set (host pointers on the host, device pointers on the device); kappa is read by the fill only, s / part by the choice only
struct TransitLoops {
    int64_t n_fields, n_loops;
    const int64_t *field_loops, *loop_off;
    const double *x, *y, *h, *kappa, *s;
    const int8_t *part, *gear;
    int64_t stride;
};

// is global sample g of loop l a station?
FCPP_HD bool transit_is_station(const TransitLoops &L, int64_t l, int64_t g)
{
    const int p = L.part[g];
    return (g - L.loop_off[l]) % L.stride == 0 && (p == 0 || p == 4) && L.gear[g] == 1;
}

// a loop that has samples must have a finite first and last s
FCPP_HD bool transit_loop_ok(const TransitLoops &L, int64_t l)
{
    const int64_t g0 = L.loop_off[l], g1 = L.loop_off[l + 1];
    return g1 <= g0 || (clear_finite(L.s[g0]) && clear_finite(L.s[g1 - 1]));
}

FCPP_HD bool transit_pose_finite(double x, double y, double h) { return clear_finite(x) && clear_finite(y) && clear_finite(h); }

// the pair's status.  region_status, loops_ok, n_stations: per field
FCPP_HD int transit_pair_status(double x0, double y0, double h0, double x1, double y1, double h1, int64_t f, int64_t n_fields,
                                const int32_t *region_status, const int32_t *loops_ok, const int64_t *n_stations)
{
    if (!transit_pose_finite(x0, y0, h0) || !transit_pose_finite(x1, y1, h1)) return TRANSIT_EINVAL;
    if (f < 0 || f >= n_fields) return TRANSIT_EINVAL;
    if (region_status[f] != CLEAR_OK || !loops_ok[f]) return TRANSIT_EINVAL;
    if (n_stations[f] > TRANSIT_MAX_STATIONS) return TRANSIT_EUNSUPPORTED;
    return TRANSIT_OK;
}

// the len of a side's connector as the cost takes it
FCPP_HD double transit_side_len(const SolveClearResult &r) { return r.rank >= 0 ? r.len : INFINITY; }

// the connector of one side: 0 the pair's pose (px, py, ph) -> the station (sx, sy, sh), 1 the station -> the pair's pose
template <int MODE>
FCPP_HD SolveClearResult transit_side(const ClearFields &F, int64_t f, int side, double px, double py, double ph, double sx, double sy, double sh,
                                      double R)
{
    return side == 0 ? solve_clear<MODE>(F, f, px, py, ph, sx, sy, sh, R) : solve_clear<MODE>(F, f, sx, sy, sh, px, py, ph, R);
}

// the ride from s_i to s_j on a loop whose last sample has s = S; forward: j >= i, else the ride wraps over the loop's end
FCPP_HD double transit_ride_s(double si, double sj, double S, bool forward) { return forward ? sj - si : (S - si) + sj; }
// stations gi, gj (global sample indices) of loop l
FCPP_HD double transit_ride(const TransitLoops &L, int64_t l, int64_t gi, int64_t gj)
{
    return transit_ride_s(L.s[gi], L.s[gj], L.s[L.loop_off[l + 1] - 1], gj >= gi);
}

FCPP_HD double transit_cost(double in, double ride, double out) { return (in + ride) + out; }

// is candidate a ordered before candidate b?  (global sample indices: (i, j) orders as (l, i, j) does)
FCPP_HD bool transit_before(double Ca, int64_t ia, int64_t ja, double Cb, int64_t ib, int64_t jb)
{
    return Ca < Cb || (Ca == Cb && (ia < ib || (ia == ib && ja < jb)));
}

// the least candidate so far; none: C +inf, which no candidate is ordered behind unless its C is below +inf
struct TransitPick { double C; int64_t l, i, j; };
FCPP_HD TransitPick transit_pick_none() { return { INFINITY, -1, -1, -1 }; }
FCPP_HD void transit_pick_take(TransitPick &p, double C, int64_t l, int64_t i, int64_t j)
{
    if (transit_before(C, i, j, p.C, p.i, p.j)) { p.C = C; p.l = l; p.i = i; p.j = j; }
}

// ---- the result of a pair -----------------------------------------------------------------------------------------------------------
struct TransitResult {
    int32_t found, status;
    int64_t loop, i, j;
    SolveClearResult in, out;
    double ride, total;
};

FCPP_HD void transit_no_conn(SolveClearResult &r)
{
    r.word = -1; r.rank = -1; r.crossings = 0; r.len = __builtin_nan("");
    for (int k = 0; k < 5; ++k) r.seg[k] = __builtin_nan("");
}

// from the pick (stations of loop l, or none) to the result: both connectors by the rule, as they were priced
template <int MODE>
FCPP_HD TransitResult transit_finish(const ClearFields &F, const TransitLoops &L, int64_t f, double x0, double y0, double h0, double x1, double y1,
                                     double h1, double R, int status, const TransitPick &p)
{
    TransitResult r;
    r.found = 0; r.status = status; r.loop = r.i = r.j = -1;
    transit_no_conn(r.in); transit_no_conn(r.out);
    r.ride = __builtin_nan(""); r.total = INFINITY;
    if (status != TRANSIT_OK || p.i < 0 || p.j < 0 || p.l < 0) return r;
    r.in = transit_side<MODE>(F, f, 0, x0, y0, h0, L.x[p.i], L.y[p.i], L.h[p.i], R);
    r.out = transit_side<MODE>(F, f, 1, x1, y1, h1, L.x[p.j], L.y[p.j], L.h[p.j], R);
    r.found = 1; r.loop = p.l; r.i = p.i; r.j = p.j;
    r.ride = transit_ride(L, p.l, p.i, p.j);
    r.total = transit_cost(transit_side_len(r.in), r.ride, transit_side_len(r.out));
    return r;
}

// ---- the sampled path of a pair --------------------------------------------------------------------------------------------------------
// what a pair's samples are evaluated from (the solve's outputs, as the caller hands them back); seg: NSEG per pair
struct TransitRec {
    const int32_t *found;
    const int64_t *loop, *i, *j;
    const int32_t *in_word;
    const double *in_seg;
    const int32_t *out_word;
    const double *out_seg;
};

// the three counts of pair p; all 0 for a pair that is not found or whose record names no two samples of one loop.  bad: 2^31 or more
template <int MODE>
FCPP_HD void transit_counts(const TransitRec &rec, int64_t n_loops, const int64_t *loop_off, double spacing, int64_t p, int64_t &K_in,
                            int64_t &N_ride, int64_t &K_out, int64_t &bad)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    K_in = N_ride = K_out = 0;
    if (rec.found[p] == 0) return;
    const int64_t l = rec.loop[p], gi = rec.i[p], gj = rec.j[p];
    if (l < 0 || l >= n_loops) return;
    const int64_t g0 = loop_off[l], g1 = loop_off[l + 1];
    if (gi < g0 || gi >= g1 || gj < g0 || gj >= g1) return;
    int64_t b = 0;
    const int64_t a = Conn<MODE>::count(rec.in_word[p], rec.in_seg + p * NSEG, spacing, b);
    const int64_t c = Conn<MODE>::count(rec.out_word[p], rec.out_seg + p * NSEG, spacing, b);
    const int64_t ride = gj >= gi ? gj - gi + 1 : (g1 - gi) + (gj - g0) + 1;
    if (b || a + ride + c > FPATH_MAX_SAMPLES) { ++bad; return; }
    K_in = a; N_ride = ride; K_out = c;
}

// sample k of the K samples of pair p (K = K_in + N_ride + K_out by transit_counts; a K that is not is cut or padded by the out-connector)
template <int MODE>
FCPP_HD void transit_eval(const TransitRec &rec, const TransitLoops &L, const double *fx, const double *fy, const double *fh, double R,
                          double spacing, int64_t p, int64_t k, int64_t K, double &x, double &y, double &h, double &kappa, int &part, int &gear)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    int64_t K_in, N_ride, K_out, bad = 0;
    transit_counts<MODE>(rec, L.n_loops, L.loop_off, spacing, p, K_in, N_ride, K_out, bad);
    x = y = h = kappa = __builtin_nan("");
    part = TRANSIT_PART_CONN; gear = 0;
    if (K_in + N_ride + K_out == 0) return;
    if (k < K_in) {
        Conn<MODE>::eval(fx[p], fy[p], fh[p], R, rec.in_word[p], rec.in_seg + p * NSEG, spacing, k, K_in, x, y, h, kappa, gear);
        return;
    }
    const int64_t gi = rec.i[p], gj = rec.j[p];
    if (k < K_in + N_ride) {
        const int64_t l = rec.loop[p], g0 = L.loop_off[l], n = L.loop_off[l + 1] - g0;
        const int64_t g = g0 + ((gi - g0) + (k - K_in)) % n;
        x = L.x[g]; y = L.y[g]; h = L.h[g]; kappa = L.kappa[g]; gear = L.gear[g];
        part = TRANSIT_PART_RIDE;
        return;
    }
    Conn<MODE>::eval(L.x[gj], L.y[gj], L.h[gj], R, rec.out_word[p], rec.out_seg + p * NSEG, spacing, k - K_in - N_ride, K - K_in - N_ride, x, y, h,
                     kappa, gear);
}

// ---- the host twin: one field's stations, one pair ---------------------------------------------------------------------------------------
// the stations of field f in order -> their number; idx / loop (room for the field's samples) may be NULL
inline int64_t transit_field_stations(const TransitLoops &L, int64_t f, int64_t *idx, int64_t *loop)
{
    int64_t c = 0;
    for (int64_t l = L.field_loops[f]; l < L.field_loops[f + 1]; ++l)
        for (int64_t g = L.loop_off[l]; g < L.loop_off[l + 1]; ++g)
            if (transit_is_station(L, l, g)) {
                if (idx) idx[c] = g;
                if (loop) loop[c] = l;
                ++c;
            }
    return c;
}
inline bool transit_field_loops_ok(const TransitLoops &L, int64_t f)
{
    for (int64_t l = L.field_loops[f]; l < L.field_loops[f + 1]; ++l)
        if (!transit_loop_ok(L, l)) return false;
    return true;
}

// the pick of a pair of status 0 by brute force.  idx, loop: the field's n_st stations; in, out: n_st doubles of scratch each
template <int MODE>
inline TransitPick transit_pick_host(const ClearFields &F, const TransitLoops &L, int64_t f, double x0, double y0, double h0, double x1, double y1,
                                     double h1, double R, int64_t n_st, const int64_t *idx, const int64_t *loop, double *in, double *out)
{
    for (int64_t a = 0; a < n_st; ++a) {
        const int64_t g = idx[a];
        in[a] = transit_side_len(transit_side<MODE>(F, f, 0, x0, y0, h0, L.x[g], L.y[g], L.h[g], R));
        out[a] = transit_side_len(transit_side<MODE>(F, f, 1, x1, y1, h1, L.x[g], L.y[g], L.h[g], R));
    }
    TransitPick p = transit_pick_none();
    for (int64_t a = 0; a < n_st; ++a) {
        if (!(in[a] < INFINITY)) continue;
        for (int64_t b = 0; b < n_st; ++b) {
            if (loop[b] != loop[a]) continue;
            transit_pick_take(p, transit_cost(in[a], transit_ride(L, loop[a], idx[a], idx[b]), out[b]), loop[a], idx[a], idx[b]);
        }
    }
    return p;
}

}  // namespace fcpp
