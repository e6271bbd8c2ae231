// fcpp_dubinsfn.h -- the shortest forward-only Dubins path between two poses, and the pose at an arc length along it: ONE function for the
// host (fcpp_debug_dubins, the tests' checker) and the device (fcpp_conn.hip), written like fcpp_planfn.h in plain IEEE-754 double
// operations with the transcendentals of fcpp_math.h / fcpp_geom.h (fc_sincos, atan2_fd) and compiled with -ffp-contract=off on both
// sides, so that both give the same bits.  Build-defined: the reference has no code for it (its roadmap asks for it: doc/两层路径规划器 -
// 深度优化和改进路线图.md section 1.2; its connectors are straight lines, MLP:1313-1355).
//
// A pose is (x, y, h): metres and the heading in radians, any finite value with |h| <= 1e5 (fc_sincos' range).  R > 0 is the turning radius.
// Words in this order: 0 LSL, 1 LSR, 2 RSL, 3 RSR, 4 RLR, 5 LRL (L: left turn, counter-clockwise; R: right turn; S: straight).
//
// Method (L. E. Dubins 1957; the closed forms as in Shkel & LaValle 2001, here WITHOUT the normalising rotation and scaling: everything is
// formed in metres from differences of the two positions, so a pair far from the origin loses nothing).  With s_k = R sin h_k, c_k = R cos h_k
// the centres of the turning circles are  left_k = (x_k - s_k, y_k + c_k),  right_k = (x_k + s_k, y_k - c_k),  and with dx = x_1 - x_0,
// dy = y_1 - y_0 (taken FIRST) the four centre-to-centre vectors are
//     LL = (dx + (s_0 - s_1), dy - (c_0 - c_1))      RR = (dx - (s_0 - s_1), dy + (c_0 - c_1))
//     LR = (dx + (s_0 + s_1), dy - (c_0 + c_1))      RL = (dx - (s_0 + s_1), dy + (c_0 + c_1))            (left_0 -> right_1, right_0 -> left_1)
//   LSL: straight of length |LL| in direction phi = atan2(LL);             arcs  arc(phi - h_0),  arc(h_1 - phi)
//   RSR: the same with RR;                                                  arcs  arc(h_0 - phi),  arc(phi - h_1)
//   LSR: p = sqrt(|LR|^2 - 4 R^2), psi = atan2(2R LR.x + p LR.y, p LR.x - 2R LR.y);      arcs  arc(psi - h_0),  arc(psi - h_1)
//   RSL: p = sqrt(|RL|^2 - 4 R^2), psi = atan2(p RL.y - 2R RL.x, p RL.x + 2R RL.y);      arcs  arc(h_0 - psi),  arc(h_1 - psi)
//   RLR: g = atan2(sqrt(16 R^2 - |RR|^2), |RR|)  (= acos(|RR| / 4R));  t = arc(h_0 - phi_RR + g + pi/2),  middle arc(pi + 2 g),
//        q = arc((h_0 - h_1) - t + middle)
//   LRL: g likewise from |LL|;  t = arc(phi_LL + g + pi/2 - h_0),  middle arc(pi + 2 g),  q = arc((h_1 - h_0) - t + middle)
// A segment's length is R x its angle (arcs) or p (straights), each >= 0; total = (seg[0] + seg[1]) + seg[2].  The shortest feasible word
// wins; among equal totals the LOWEST word index.
//
// The rules at the edges (include/fcpp.h states them for callers):
//   * arc(a): a reduced into [0, 2 pi); a result above 2 pi - 2^-43 (128 ulp of 2 pi) is 0.  An arc that is mathematically 0 but comes out
//     as -1 ulp would otherwise be a full circle -- where a start heading points at the goal, or two swaths are exactly parallel.  What the
//     rule can cost: a true arc that close to a full circle is not driven, the end pose is off by < 2^-43 (R + straight) metres.
//   * feasibility: LSR / RSL need |c|^2 >= 4 R^2 (1 - 2^-48), RLR / LRL |c|^2 <= 16 R^2 (1 + 2^-48) -- |c|^2 the computed squared centre
//     distance; inside that band of 16 ulp the root's argument is clamped to 0 (the circles touch), beyond it the word is infeasible.
//   * centres closer than R 2^-40 (LL for LSL / LRL, RR for RSR / RLR) count as coincident: the direction between them is noise, the
//     straight's direction is taken as h_0 (no first arc).  Start == goal therefore gives word 0 and lengths 0, 0, 0.
//   * a pair whose dx, dy, h_0 or h_1 is not finite (or so large that no word's length is finite): word -1, lengths and total NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_math.h"

namespace fcpp {

constexpr double kDubTwoPiHi = 6.28318530717958623200e+00, kDubTwoPiLo = 2.44929359829470635445e-16;
constexpr double kDubInvTwoPi = 1.59154943091895345554e-01;
constexpr double kDubAngTol = 0x1p-43;      // an arc within this of a full circle is no arc
constexpr double kDubEdge = 0x1p-48;        // relative band around a word's feasibility edge that is clamped
constexpr double kDubCoincide = 0x1p-40;    // centres closer than this x R are one centre

FCPP_HD bool dubins_finite(double v) { return v - v == 0.0; }

// a reduced into [0, 2 pi), and 0 when it comes out within kDubAngTol below 2 pi
FCPP_HD double dubins_arc(double a)
{
    const double k = floor(a * kDubInvTwoPi);
    double r = fma(-k, kDubTwoPiHi, a);
    r = fma(-k, kDubTwoPiLo, r);
    if (r < 0.0) r += kDubTwoPiHi;              // (the product's rounding put k one too high / too low)
    if (r >= kDubTwoPiHi) r -= kDubTwoPiHi;
    return r > kDubTwoPiHi - kDubAngTol ? 0.0 : r;
}

// a heading brought into (-pi, pi] as fcpp_trajectory writes it; a value already there is returned as it is
FCPP_HD double dubins_wrap_pi(double a)
{
    const double k = rint(a * kDubInvTwoPi);
    double r = fma(-k, kDubTwoPiHi, a);
    r = fma(-k, kDubTwoPiLo, r);
    if (r <= -3.14159265358979311600e+00) r += kDubTwoPiHi;
    if (r > 3.14159265358979311600e+00) r -= kDubTwoPiHi;
    return r;
}

// what depends on ONE pose only: hoisted out of the pair loop of the matrix kernel
struct DubinsPose { double x, y, h, s, c; };        // s = R sin h, c = R cos h
FCPP_HD DubinsPose dubins_prep(double x, double y, double h, double R)
{
    double sn, cs;
    fc_sincos(h, sn, cs);
    return { x, y, h, R * sn, R * cs };
}

// What the word enumeration hands every candidate to.  DubinsBest is the solver's own: the shortest feasible word, among equal totals the
// lowest index (the candidates come in word order).  fcpp_solveclearfn.h brings accumulators that keep more than one.
struct DubinsBest {
    double best = INFINITY, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    int bw = 0;
    FCPP_HD void take(int w, bool ok, double c0, double c1, double c2)
    {
        const double tt = (c0 + c1) + c2;
        if (ok && tt < best) { best = tt; bw = w; b0 = c0; b1 = c1; b2 = c2; }
    }
};

// all six words evaluated (no branch by word), each handed to acc.take(word, feasible, seg0, seg1, seg2)
template <class ACC>
FCPP_HD void dubins_words(const DubinsPose &f, const DubinsPose &t, double R, ACC &acc)
{
    const double dx = t.x - f.x, dy = t.y - f.y;
    const double sm = f.s - t.s, sp = f.s + t.s, cm = f.c - t.c, cp = f.c + t.c;
    const double R2 = R * R, twoR = 2.0 * R, near = R * kDubCoincide;
    const double h0 = f.h, h1 = t.h;
    // left centre -> left centre, right centre -> right centre
    const double lx = dx + sm, ly = dy - cm, rx = dx - sm, ry = dy + cm;
    const double Dl2 = lx * lx + ly * ly, Dr2 = rx * rx + ry * ry;
    const double Dl = sqrt(Dl2), Dr = sqrt(Dr2);
    const double phl = Dl >= near ? atan2_fd(ly, lx) : h0, phr = Dr >= near ? atan2_fd(ry, rx) : h0;
    acc.take(0, true, R * dubins_arc(phl - h0), Dl, R * dubins_arc(h1 - phl));
    {   // LSR: left centre -> right centre
        const double ux = dx + sp, uy = dy - cp, e = (ux * ux + uy * uy) - 4.0 * R2;
        const double p = sqrt(fmax(e, 0.0)), psi = atan2_fd(twoR * ux + p * uy, p * ux - twoR * uy);
        acc.take(1, e >= -4.0 * R2 * kDubEdge, R * dubins_arc(psi - h0), p, R * dubins_arc(psi - h1));
    }
    {   // RSL: right centre -> left centre
        const double wx = dx - sp, wy = dy + cp, e = (wx * wx + wy * wy) - 4.0 * R2;
        const double p = sqrt(fmax(e, 0.0)), psi = atan2_fd(p * wy - twoR * wx, p * wx + twoR * wy);
        acc.take(2, e >= -4.0 * R2 * kDubEdge, R * dubins_arc(h0 - psi), p, R * dubins_arc(h1 - psi));
    }
    acc.take(3, true, R * dubins_arc(h0 - phr), Dr, R * dubins_arc(phr - h1));
    {   // RLR
        const double e = 16.0 * R2 - Dr2, g = atan2_fd(sqrt(fmax(e, 0.0)), Dr);
        const double a0 = dubins_arc(((h0 - phr) + g) + kHalfPi), am = dubins_arc(kPi + 2.0 * g), a2 = dubins_arc(((h0 - h1) - a0) + am);
        acc.take(4, e >= -16.0 * R2 * kDubEdge, R * a0, R * am, R * a2);
    }
    {   // LRL
        const double e = 16.0 * R2 - Dl2, g = atan2_fd(sqrt(fmax(e, 0.0)), Dl);
        const double a0 = dubins_arc(((phl - h0) + g) + kHalfPi), am = dubins_arc(kPi + 2.0 * g), a2 = dubins_arc(((h1 - h0) - a0) + am);
        acc.take(5, e >= -16.0 * R2 * kDubEdge, R * a0, R * am, R * a2);
    }
}

// are the pair's inputs such that a word can be had at all?  (the solvers' "word -1" rule, the totals aside)
FCPP_HD bool dubins_inputs_finite(const DubinsPose &f, const DubinsPose &t)
{
    return dubins_finite(t.x - f.x) && dubins_finite(t.y - f.y) && dubins_finite(f.h) && dubins_finite(t.h);
}

// the shortest word selected
FCPP_HD void dubins_solve_prepped(const DubinsPose &f, const DubinsPose &t, double R, int &word, double &seg0, double &seg1, double &seg2, double &total)
{
    DubinsBest b;
    dubins_words(f, t, R, b);
    const bool ok = dubins_inputs_finite(f, t) && dubins_finite(b.best);
    const double nan = __builtin_nan("");
    word = ok ? b.bw : -1;
    seg0 = ok ? b.b0 : nan; seg1 = ok ? b.b1 : nan; seg2 = ok ? b.b2 : nan;
    total = ok ? b.best : nan;
}

FCPP_HD void dubins_solve(double x0, double y0, double h0, double x1, double y1, double h1, double R, int &word, double &seg0, double &seg1,
                          double &seg2, double &total)
{
    dubins_solve_prepped(dubins_prep(x0, y0, h0, R), dubins_prep(x1, y1, h1, R), R, word, seg0, seg1, seg2, total);
}

// turn direction of segment k of a word: +1 left, -1 right, 0 straight
FCPP_HD int dubins_turn(int word, int k)
{
    const int first = (word == 0 || word == 1 || word == 5) ? 1 : -1, last = (word == 0 || word == 2 || word == 5) ? 1 : -1;
    return k == 0 ? first : (k == 2 ? last : (word < 4 ? 0 : -first));
}

// The pose at arc length s in [0, total] of the path (word, seg) that starts at (x0, y0, h0), and the signed curvature there (+1/R left,
// -1/R right, 0 straight).  Evaluated from the START OF THE SEGMENT that contains s -- the segment start poses are closed forms of the
// start pose -- never from a previous sample.  s at a junction belongs to the segment that starts there; s >= total is the end of the last
// segment.  The heading comes back in (-pi, pi].  word outside 0 .. 5 or s NaN: NaN.
FCPP_HD void dubins_pose_at(double x0, double y0, double h0, double R, int word, double seg0, double seg1, double seg2, double s, double &x,
                            double &y, double &h, double &kappa)
{
    if (word < 0 || word > 5 || !(s == s)) { x = y = h = kappa = __builtin_nan(""); return; }
    int k = 0;
    double u = s;
    if (!(s < seg0)) {
        const double u1 = s - seg0;
        if (u1 < seg1) { k = 1; u = u1; }
        else { k = 2; u = fmin(u1 - seg1, seg2); }
    }
    if (s >= (seg0 + seg1) + seg2) { k = 2; u = seg2; }
    if (u < 0.0) u = 0.0;                                   // (s < 0)
    double px = x0, py = y0, ph = h0, sn, cs;
    fc_sincos(ph, sn, cs);
    for (int j = 0; j <= k; ++j) {
        const double len = j < k ? (j == 0 ? seg0 : seg1) : u;
        const int sg = dubins_turn(word, j);
        if (sg == 0) { px += len * cs; py += len * sn; continue; }
        const double nh = sg > 0 ? ph + len / R : ph - len / R;
        double s2, c2;
        fc_sincos(nh, s2, c2);
        if (sg > 0) { px += R * (s2 - sn); py -= R * (c2 - cs); }
        else        { px -= R * (s2 - sn); py += R * (c2 - cs); }
        ph = nh; sn = s2; cs = c2;
    }
    const int sgk = dubins_turn(word, k);
    x = px; y = py; h = dubins_wrap_pi(ph);
    kappa = sgk == 0 ? 0.0 : (sgk > 0 ? 1.0 / R : -(1.0 / R));
}

}  // namespace fcpp
