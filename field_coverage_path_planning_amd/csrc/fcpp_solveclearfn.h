// fcpp_solveclearfn.h -- clear connectors: per pair of poses the SHORTEST feasible Dubins or Reeds-Shepp word whose pieces stay inside the
// pair's polygon field.  ONE set of expressions for the host (fcpp_debug_conn_words, fcpp_debug_conn_solve_clear, the tests' driver) and
// the device (fcpp_solveclear.hip), in plain IEEE-754 double operations and compiled with -ffp-contract=off on both sides, so that both
// give the same bits.  Build-defined: the reference's connectors are straight lines that nothing tests.
//
// Nothing geometric is written here.  The candidates are what the solvers' own word enumerations (dubins_words, rs_words) hand to an
// accumulator -- the solvers keep the best one, the accumulators below keep all of them or one named word -- and a candidate is tested by
// the clearance rule's own steps (clear_pieces, clear_walk, clear_finish of fcpp_clearfn.h), which is what clear_path does.
//
// THE RULE (include/fcpp.h states it for callers).
//   candidates  the words the solver finds feasible with a finite total, 6 (mode 0) or 48 (mode 1), each with the seg and total bits
//               fcpp_dubins_solve / fcpp_rs_solve would write had it won (Reeds-Shepp: seg + 0.0).  None for a pair the solver leaves
//               unsolved (an input that is not finite).
//   order       (total, word) ascending: the solvers' tie rule.  Position 0 is the solvers' answer.
//   result      word, seg, len, rank, crossings.
//               unsolved pair: word -1, NaN, rank -1, crossings 0 -- whatever the field, field -1 included: there is no word to give.
//               field -1 (no region): the shortest word, rank 0, crossings 0.
//               field outside -1 .. n - 1 or of status CLEAR_EINVAL: the shortest word, rank -1, crossings 0.
//               else the first candidate of the order that is clear: rank = its position, crossings 0;  if none is clear the shortest word
//               with rank -1 and ITS crossings.  `inside` is a property of the start point alone, so a start that is not inside decides
//               rank -1 from the shortest word's test and no other word is looked at.
// solve_clear_first is the part a lane per pair does (the solve, the shortest word's test); it says whether the other words have to be
// looked at.  solve_clear_rest is the sequential form of that look (host); the device does it with a lane per word (SolveClearOne).
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_clearfn.h"
#include "fcpp_connfn.h"

namespace fcpp {

template <int MODE> struct SolveClearWords;
template <> struct SolveClearWords<0> { static constexpr int NW = 6; };
template <> struct SolveClearWords<1> { static constexpr int NW = RS_WORDS; };

// a candidate is one the solvers could have kept: feasible and of a total below +inf (their `tt < best`; a NaN total never wins)
FCPP_HD bool solve_clear_candidate(bool ok, double total) { return ok && total < INFINITY; }

// ---- accumulators for dubins_words / rs_words ------------------------------------------------------------------------------------------
// every candidate of a pair
template <int MODE> struct SolveClearAll {
    static constexpr int NW = SolveClearWords<MODE>::NW, NSEG = Conn<MODE>::NSEG;
    bool ok[NW];
    double total[NW], seg[NW][NSEG];
    FCPP_HD SolveClearAll()
    {
        for (int w = 0; w < NW; ++w) {
            ok[w] = false;
            total[w] = __builtin_nan("");
            for (int k = 0; k < NSEG; ++k) seg[w][k] = __builtin_nan("");
        }
    }
    FCPP_HD void take(int w, bool feasible, double c0, double c1, double c2)          // (Dubins)
    {
        const double tt = (c0 + c1) + c2;
        if (!solve_clear_candidate(feasible, tt)) return;
        ok[w] = true; total[w] = tt; seg[w][0] = c0; seg[w][1] = c1; seg[w][2] = c2;
    }
};
FCPP_HD void rs_keep(SolveClearAll<1> &a, int w, bool feasible, double tt, double l0, double l1, double l2, double l3, double l4)
{
    if (!solve_clear_candidate(feasible, tt)) return;
    a.ok[w] = true; a.total[w] = tt;
    a.seg[w][0] = l0 + 0.0; a.seg[w][1] = l1 + 0.0; a.seg[w][2] = l2 + 0.0; a.seg[w][3] = l3 + 0.0; a.seg[w][4] = l4 + 0.0;
}

// the candidate of ONE word: what a lane of the word kernel keeps
template <int MODE> struct SolveClearOne {
    static constexpr int NSEG = Conn<MODE>::NSEG;
    int want;
    bool ok;
    double total, seg[NSEG];
    FCPP_HD explicit SolveClearOne(int w) : want(w), ok(false), total(INFINITY)
    {
        for (int k = 0; k < NSEG; ++k) seg[k] = 0.0;
    }
    FCPP_HD void take(int w, bool feasible, double c0, double c1, double c2)          // (Dubins)
    {
        const double tt = (c0 + c1) + c2;
        if (w != want || !solve_clear_candidate(feasible, tt)) return;
        ok = true; total = tt; seg[0] = c0; seg[1] = c1; seg[2] = c2;
    }
};
FCPP_HD void rs_keep(SolveClearOne<1> &a, int w, bool feasible, double tt, double l0, double l1, double l2, double l3, double l4)
{
    if (w != a.want || !solve_clear_candidate(feasible, tt)) return;
    a.ok = true; a.total = tt;
    a.seg[0] = l0 + 0.0; a.seg[1] = l1 + 0.0; a.seg[2] = l2 + 0.0; a.seg[3] = l3 + 0.0; a.seg[4] = l4 + 0.0;
}

// the pair's words into acc; false for a pair the solvers leave unsolved (then acc means nothing)
template <int MODE, class ACC>
FCPP_HD bool solve_clear_words(double x0, double y0, double h0, double x1, double y1, double h1, double R, ACC &acc);
template <class ACC>
FCPP_HD bool solve_clear_words_dubins(double x0, double y0, double h0, double x1, double y1, double h1, double R, ACC &acc)
{
    const DubinsPose f = dubins_prep(x0, y0, h0, R), t = dubins_prep(x1, y1, h1, R);
    dubins_words(f, t, R, acc);
    return dubins_inputs_finite(f, t);
}
template <class ACC>
FCPP_HD bool solve_clear_words_rs(double x0, double y0, double h0, double x1, double y1, double h1, double R, ACC &acc)
{
    const RsPose f = rs_prep(x0, y0, h0), t = rs_prep(x1, y1, h1);
    rs_words(f, t, R, acc);
    return rs_inputs_finite(f, t);
}
template <int MODE, class ACC>
FCPP_HD bool solve_clear_words(double x0, double y0, double h0, double x1, double y1, double h1, double R, ACC &acc)
{
    if constexpr (MODE == 0) return solve_clear_words_dubins(x0, y0, h0, x1, y1, h1, R, acc);
    else return solve_clear_words_rs(x0, y0, h0, x1, y1, h1, R, acc);
}

// ---- the test of one candidate: clear_path's steps, with the field's validity kept apart ------------------------------------------------
// f in 0 .. F.n - 1.  valid: the field has status 0 (else the result is the unsolved path's)
template <int MODE>
FCPP_HD ClearResult solve_clear_test(const ClearFields &F, int64_t f, double x0, double y0, double h0, double R, int word, const double *seg,
                                     bool &valid)
{
    ClearPiece pc[Conn<MODE>::NSEG];
    ClearBox box;
    const bool solved = clear_pieces<MODE>(x0, y0, h0, R, word, seg, pc, box);
    ClearAcc a = clear_begin();
    valid = clear_walk<Conn<MODE>::NSEG>(F, f, pc, x0, y0, R, a);
    return clear_finish(solved, valid, a);
}

// ---- the result ----------------------------------------------------------------------------------------------------------------------
struct SolveClearResult { int32_t word; double seg[5], len; int32_t rank, crossings; };

// is candidate (ta, wa) ordered before (tb, wb)?
FCPP_HD bool solve_clear_before(double ta, int wa, double tb, int wb) { return ta < tb || (ta == tb && wa < wb); }

// The solve and the shortest word's test.  r is complete on return; true: the shortest word starts inside a valid field and crosses its
// boundary -- r holds the rank -1 answer, and the other words have to be looked at (solve_clear_rest, or the word kernel).
template <int MODE>
FCPP_HD bool solve_clear_first(const ClearFields &F, int64_t f, double x0, double y0, double h0, double x1, double y1, double h1, double R,
                               SolveClearResult &r)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    int word;
    double seg[NSEG], total;
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, R, word, seg, total);
    r.word = word;
    for (int k = 0; k < 5; ++k) r.seg[k] = k < NSEG ? seg[k] : 0.0;
    r.len = total;
    r.rank = -1;
    r.crossings = 0;
    if (word < 0) return false;
    if (f == -1) { r.rank = 0; return false; }
    if (f < 0 || f >= F.n) return false;
    bool valid;
    const ClearResult c = solve_clear_test<MODE>(F, f, x0, y0, h0, R, word, seg, valid);
    if (!valid) return false;
    if (c.clear) { r.rank = 0; return false; }
    r.crossings = c.crossings;
    return c.inside != 0;
}

// The other words, one after the other in the order, until one is clear.  Only after solve_clear_first returned true.
template <int MODE>
FCPP_HD void solve_clear_rest(const ClearFields &F, int64_t f, double x0, double y0, double h0, double x1, double y1, double h1, double R,
                              SolveClearResult &r)
{
    constexpr int NSEG = Conn<MODE>::NSEG, NW = SolveClearWords<MODE>::NW;
    SolveClearAll<MODE> all;
    if (!solve_clear_words<MODE>(x0, y0, h0, x1, y1, h1, R, all)) return;
    double pt = -INFINITY;              // the candidate looked at last
    int pw = -1;
    for (int rank = 0; rank < NW; ++rank) {
        int w = -1;
        for (int j = 0; j < NW; ++j)
            if (all.ok[j] && solve_clear_before(pt, pw, all.total[j], j) && (w < 0 || solve_clear_before(all.total[j], j, all.total[w], w))) w = j;
        if (w < 0) return;
        pt = all.total[w]; pw = w;
        if (rank == 0) continue;        // (the shortest word: solve_clear_first has tested it)
        bool valid;
        if (!solve_clear_test<MODE>(F, f, x0, y0, h0, R, w, all.seg[w], valid).clear) continue;
        r.word = w;
        for (int k = 0; k < NSEG; ++k) r.seg[k] = all.seg[w][k];
        r.len = all.total[w];
        r.rank = rank;
        r.crossings = 0;
        return;
    }
}

template <int MODE>
FCPP_HD SolveClearResult solve_clear(const ClearFields &F, int64_t f, double x0, double y0, double h0, double x1, double y1, double h1, double R)
{
    SolveClearResult r;
    if (solve_clear_first<MODE>(F, f, x0, y0, h0, x1, y1, h1, R, r)) solve_clear_rest<MODE>(F, f, x0, y0, h0, x1, y1, h1, R, r);
    return r;
}

// ---- the priced transit block (include/fcpp.h: fcpp_route_transit_priced) ------------------------------------------------------------------
// the canonical pair (p, q) of field i's block, p and q of different swaths: the rule above on the poses route_transit solves, against
// field i -> what both mirrored entries of T and K hold.  The clear word's own total; with no clear word (rank -1) the shortest word's
// total + penalty, one sum.  listed: the first pass hands the pair to the second.
struct PricedTransit { double t; int32_t rank; bool listed; };

template <int MODE>
FCPP_HD PricedTransit priced_transit(const ClearFields &F, int64_t i, const double *ax, const double *ay, const double *bx, const double *by,
                                     double theta, double R, double penalty, int p, int q)
{
    double x0, y0, h0, x1, y1, h1;
    route_pose(ax, ay, bx, by, theta, p, true, x0, y0, h0);
    route_pose(ax, ay, bx, by, theta, q, false, x1, y1, h1);
    SolveClearResult r;
    const bool listed = solve_clear_first<MODE>(F, i, x0, y0, h0, x1, y1, h1, R, r);
    if (listed) solve_clear_rest<MODE>(F, i, x0, y0, h0, x1, y1, h1, R, r);
    return { r.rank >= 0 ? r.len : r.len + penalty, r.rank, listed };
}

}  // namespace fcpp
