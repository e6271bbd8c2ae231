// fcpp_rsfn.h -- the shortest Reeds-Shepp path (forward AND reverse motion) between two poses, and the pose at a position along it: ONE
// function for the host (fcpp_debug_rs, the tests' checker) and the device (fcpp_conn.hip), written like fcpp_dubinsfn.h in plain IEEE-754
// double operations with the transcendentals of fcpp_math.h / fcpp_geom.h (fc_sincos, atan2_fd) and compiled with -ffp-contract=off on both
// sides, so that both give the same bits.  Build-defined: the reference has no code for it (its roadmap asks for it: doc/两层路径规划器 -
// 深度优化和改进路线图.md section 1.2), but its vehicle reverses at every outer headland corner (MLP:1024-1082).
//
// A pose is (x, y, h): metres and the heading in radians, any finite value with |h| <= 1e5 (fc_sincos' range).  R > 0 is the turning radius.
// fc_sincos is also taken of phi = h_1 - h_0, so the two headings of a PAIR must not differ by more than ~1e5 either: |h| <= 5e4 for both is
// always safe (beyond it the reduction by pi/2 loses bits gradually; nothing faults).
//
// THE WORD TABLE.  word = 4 * base + flip + 2 * mirror.  A base word has up to five segments; its letters (L: left / counter-clockwise turn,
// R: right turn, S: straight) and gears (+ forward, - reverse) are
//     base  0  L+ S+ L+            (Reeds & Shepp 1990, formula 8.1)        base  6  L+ R- L- R+         (8.8, both middle arcs u)
//     base  1  L+ S+ R+            (8.2)                                    base  7  L+ R- S- L-         (8.9,  the R arc is pi/2)
//     base  2  L+ R- L+            (8.3)                                    base  8  L+ R- S- R-         (8.10, the first R arc is pi/2)
//     base  3  L+ R- L-            (8.4)                                    base  9  L- S- R- L+         (8.9 backwards,  the R arc is pi/2)
//     base  4  L- R- L+            (8.4 backwards)                          base 10  R- S- R- L+         (8.10 backwards, the last R arc is pi/2)
//     base  5  L+ R+ L- R-         (8.7, both middle arcs u)                base 11  L+ R- S- L- R+      (8.11, both inner arcs pi/2)
// flip (bit 0, the paper's time-flip) reverses every gear; mirror (bit 1, the paper's reflect) swaps L and R.  So the word of the mirror
// image of a path is word ^ 2 and the word of the path driven with every gear reversed is word ^ 1: 12 x 4 = the 48 words of the paper.
// rs_turn(word, k) / rs_gear(word, k) read the table.
//
// Method.  dx = x_1 - x_0, dy = y_1 - y_0 are taken FIRST (a pair 5000 m from the origin loses nothing), rotated into the start frame and
// divided by R:  x = (dx cos h_0 + dy sin h_0) / R,  y = (dy cos h_0 - dx sin h_0) / R,  phi = h_1 - h_0, s = sin phi, c = cos phi (of the
// difference itself: equal headings give s = 0, c = 1 exactly; the sine and cosine of h_0 are hoisted by the matrix kernel).  The four symmetry transforms
// (identity, flip: x -> -x, phi -> -phi; mirror: y -> -y, phi -> -phi; both) meet the base formulas only through two vectors each:
//     "minus" vector (8.1, 8.3, 8.4, 8.9):    identity / flip  (+-(x - s),  y - 1 + c)        mirror / both  (+-(x + s), -y - 1 + c)
//     "plus"  vector (8.2, 8.7, 8.8, 8.10, 8.11):              (+-(x + s),  y - 1 - c)                       (+-(x - s), -y - 1 - c)
// A flip only negates the vector's first component: its length rho is shared and its polar angle is pi - theta.  So FOUR polar forms (one
// atan2 and one root each) serve all four transforms, and everything that depends on rho alone -- the roots, asin(rho / 4), the acos of 8.7 and
// 8.8, atan2(2, sqrt(rho^2 - 4)) -- is computed once per vector, not once per word.  The "backwards" words (bases 4, 9, 10) are the same
// formulas on the pose (x c + y s, x s - y c, phi) with the segments in reverse order: four more vectors.  22 atan2 per pair in all.
// With theta' the vector's angle under the transform, phi' = +-phi, r = sqrt(rho^2 - 4), beta = atan2(2, r), in units of R:
//     8.1   t = pos(theta'),                    u = rho,                  v = pos(phi' - t)        (u R: the same vector's length formed in metres)
//     8.2   t = pos(theta' + beta),             u = r,                    v = pos(t - phi')                       rho^2 >= 4    (u R formed in metres)
//           (rho^2 - 4 of the forward plus vectors as X^2 + (Y - 2)(Y + 2), Y + 2 = +-y + (1 - c) formed directly: rs_polar_plus)
//     8.3/4 t = pos(theta' + pi - a),           u = -2a, a = asin(rho/4), v = wrap(phi' - t + u): base 2 if v >= 0, else base 3      rho <= 4
//     8.7   t = pos(theta' + pi/2 + u),         u = acos((2 + rho) / 4),  v = neg(t - 2u - phi')    segments t, u, -u, v      rho <= 2
//     8.8   t = pos(theta' + pi/2 + atan2(sin u, 2 - cos u)),  u = acos((20 - rho^2) / 16),  v = pos(t - phi')   segments t, -u, -u, v   4 <= rho^2 <= 20
//     (8.7, 8.8 from the chain of the four circle centres, each 2 from the next: the vector from the first to the last is
//      2 (2 cos u - 1) e(t - u - pi/2) in 8.7 and 2 e(t - pi/2) (2 - e(u)) in 8.8, e(a) = (cos a, sin a))
//     8.9   t = pos(theta' + pi/2 + beta),      u = 2 - r <= 0,           v = neg(phi' - pi/2 - t)  segments t, -pi/2, u, v   rho^2 >= 8
//     8.10  t = pos(theta' + pi/2),             u = 2 - rho <= 0,         v = neg(t + pi/2 - phi')  segments t, -pi/2, u, v   rho >= 2
//     8.11  t = pos(theta' + pi/2 + beta),      u = 4 - r <= 0,           v = pos(t - phi')   segments t, -pi/2, u, -pi/2, v  rho^2 >= 20
// (the atan2 of products of the paper's tau / omega and of 8.9 - 8.11 are written as theta' + an angle of rho alone: the same angle mod 2 pi).
// A flip negates all segments.  A segment's signed length is R x its value: positive is driven forward, negative in reverse.
// total = (((|seg0| + |seg1|) + |seg2|) + |seg3|) + |seg4|.  The shortest feasible word wins; among equal totals the LOWEST word index.
//
// The rules at the edges (include/fcpp.h states them for callers):
//   * every arc is an angle reduced into (-pi, pi].  pos(a): a reduced into [0, 2 pi) by dubins_arc -- a value within 2^-43 below 2 pi is 0, so
//     an arc that is mathematically 0 but comes out as -1 ulp is no arc and not a word lost -- and the word is feasible iff the result is
//     <= pi + 2^-43 (clamped to pi).  neg(a) = -pos(-a).  What it can cost: the end pose off by < 2^-43 (R + straight) metres.
//   * feasibility in rho^2, the computed squared length of the word's vector: each bound above holds with a relative band of 2^-48; inside
//     the band the root's / acos' argument is clamped to its edge and u to 0, beyond it the word is infeasible.
//   * a vector shorter than 2^-40 (in units of R) has no direction and no length: theta' = 0, rho = 0.
//     Start == goal therefore gives word 0 and five zeros.  The price: < 2^-40 R metres at the end pose.
//   * a pair whose dx, dy, h_0 or h_1 is not finite (or so large that no word's length is finite): word -1, segments and total NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_dubinsfn.h"
#include "fcpp_math.h"

namespace fcpp {

constexpr double kRsAngTol = 0x1p-43;       // an arc within this below 0 (or above pi) is 0 (is pi)
constexpr double kRsEdge = 0x1p-48;         // relative band around a word's feasibility edge that is clamped
constexpr double kRsCoincide = 0x1p-40;     // a vector shorter than this (units of R) has no direction and no length
constexpr int RS_WORDS = 48;

// the table: per base five 2-bit turn codes (0 none / straight, 1 L, 2 R) and five gear bits (1 = reverse), segment 0 lowest
//                                   base:   0      1      2      3      4      5      6      7      8      9      10     11
//                                turns:    L.L    L.R    LRL    LRL    LRL    LRLR   LRLR   LR.L   LR.R   L.RL   R.RL   LR.LR
constexpr uint64_t kRsTurnLo = 0x011ull | (0x021ull << 10) | (0x019ull << 20) | (0x019ull << 30) | (0x019ull << 40) | (0x099ull << 50);
constexpr uint64_t kRsTurnHi = 0x099ull | (0x049ull << 10) | (0x089ull << 20) | (0x061ull << 30) | (0x062ull << 40) | (0x249ull << 50);
//                                gears:    +++    +++    +-+    +--    --+    ++--   +--+   +---   +---   ---+   ---+   +---+
constexpr uint64_t kRsGear = 0x00ull | (0x00ull << 5) | (0x02ull << 10) | (0x06ull << 15) | (0x03ull << 20) | (0x0cull << 25) | (0x06ull << 30) |
                             (0x0eull << 35) | (0x0eull << 40) | (0x07ull << 45) | (0x07ull << 50) | (0x0eull << 55);

// turn direction of segment k of a word: +1 left, -1 right, 0 straight (or no such segment)
FCPP_HD int rs_turn(int word, int k)
{
    if (word < 0 || word >= RS_WORDS || k < 0 || k > 4) return 0;
    const int base = word >> 2;
    const uint64_t tab = base < 6 ? kRsTurnLo : kRsTurnHi;
    const int code = (int)((tab >> (10 * (base % 6) + 2 * k)) & 3);
    const int t = code == 1 ? 1 : (code == 2 ? -1 : 0);
    return (word & 2) ? -t : t;
}

// gear of segment k of a word: +1 forward, -1 reverse (a segment the word does not have: the gear the table's zero bit gives)
FCPP_HD int rs_gear(int word, int k)
{
    if (word < 0 || word >= RS_WORDS || k < 0 || k > 4) return 0;
    const int g = ((kRsGear >> (5 * (word >> 2) + k)) & 1) ? -1 : 1;
    return (word & 1) ? -g : g;
}

// a in [0, pi] or infeasible (ok cleared); neg: a in [-pi, 0]
FCPP_HD double rs_pos(double a, bool &ok)
{
    const double r = dubins_arc(a);
    ok = ok && r <= kPi + kRsAngTol;
    return fmin(r, kPi);
}
FCPP_HD double rs_neg(double a, bool &ok) { return 0.0 - rs_pos(-a, ok); }

struct RsBest { double total; int word; double s0, s1, s2, s3, s4; };

// What the word enumeration hands every candidate to: rs_keep(acc, word, feasible, total, five signed lengths).  This overload is the
// solver's own -- the shortest feasible word, among equal totals the lowest index; fcpp_solveclearfn.h brings accumulators that keep more.
FCPP_HD void rs_keep(RsBest &b, int w, bool ok, double tt, double l0, double l1, double l2, double l3, double l4)
{
    if (ok && (tt < b.total || (tt == b.total && w < b.word))) { b.total = tt; b.word = w; b.s0 = l0; b.s1 = l1; b.s2 = l2; b.s3 = l3; b.s4 = l4; }
}
// candidates of 3, 4, 5 segments in units of R; sg = -1 under a flip
// (straight_m: the straight of 8.1 and 8.2 comes in metres, formed without the division by R: an axis-aligned straight is exact)
template <class ACC>
FCPP_HD void rs_take3(ACC &b, double R, double sg, int w, bool ok, double a0, double a1, double a2, bool straight_m = false)
{
    const double l0 = (R * a0) * sg, l1 = (straight_m ? a1 : R * a1) * sg, l2 = (R * a2) * sg;
    rs_keep(b, w, ok, (fabs(l0) + fabs(l1)) + fabs(l2), l0, l1, l2, 0.0, 0.0);
}
template <class ACC>
FCPP_HD void rs_take4(ACC &b, double R, double sg, int w, bool ok, double a0, double a1, double a2, double a3)
{
    const double l0 = (R * a0) * sg, l1 = (R * a1) * sg, l2 = (R * a2) * sg, l3 = (R * a3) * sg;
    rs_keep(b, w, ok, ((fabs(l0) + fabs(l1)) + fabs(l2)) + fabs(l3), l0, l1, l2, l3, 0.0);
}
template <class ACC>
FCPP_HD void rs_take5(ACC &b, double R, double sg, int w, bool ok, double a0, double a1, double a2, double a3, double a4)
{
    const double l0 = (R * a0) * sg, l1 = (R * a1) * sg, l2 = (R * a2) * sg, l3 = (R * a3) * sg, l4 = (R * a4) * sg;
    rs_keep(b, w, ok, (((fabs(l0) + fabs(l1)) + fabs(l2)) + fabs(l3)) + fabs(l4), l0, l1, l2, l3, l4);
}

// a vector in polar form: its squared length, its length, its angle and its angle under a flip (first component negated)
struct RsVec { double rho2, rho, th, thf, e4; };       // e4 = rho^2 - 4
FCPP_HD RsVec rs_polar(double X, double Y)
{
    RsVec v;
    v.rho2 = X * X + Y * Y;
    const double rho = sqrt(v.rho2);
    const bool far = rho >= kRsCoincide;
    v.rho = far ? rho : 0.0;
    v.th = far ? atan2_fd(Y, X) : 0.0;
    v.thf = far ? kPi - v.th : 0.0;
    v.e4 = v.rho2 - 4.0;
    return v;
}
// The "plus" vector (X, Y) with Y = y' - 1 - c given together with Yp2 = Y + 2 = y' + (1 - c) formed WITHOUT the cancellation: rho^2 - 4 =
// X^2 + (Y - 2)(Y + 2).  Where the goal lies nearly straight ahead (y', phi ~ 0) rho^2 = 4 + X^2 rounds to ulp(4), and r = sqrt(rho^2 - 4)
// taken from it is off by 2^-51 / X^2 relatively: for a goal a few millimetres ahead the arcs of 8.2 (true size: rounding of the goal's own
// coordinates, 1e-11 rad) would come out beyond the 2^-43 snap with either sign and the straight word would be lost.
FCPP_HD RsVec rs_polar_plus(double X, double Y, double Yp2)
{
    RsVec v = rs_polar(X, Y);
    v.e4 = X * X + (Y - 2.0) * Yp2;
    return v;
}

// The words of a "minus" vector under identity and flip (mirror: the caller passes the mirrored vector and -phi).  back: the vector is
// that of the backwards pose, the segments come in reverse order (bases 4 and 9 instead of 0, 2, 3, 7).
template <class ACC>
FCPP_HD void rs_minus_words(ACC &b, double R, const RsVec &V, double phi, int mirror, bool back, double rho_m = 0.0)
{
    const double e4 = V.rho2 - 4.0, r = sqrt(fmax(e4, 0.0));
    const double e16 = 16.0 - V.rho2, as = atan2_fd(V.rho, sqrt(fmax(e16, 0.0)));      // asin(rho / 4)
    const double beta = atan2_fd(2.0, r);
    const bool ok_ccc = e16 >= -16.0 * kRsEdge, ok_ccsc = V.rho2 - 8.0 >= -8.0 * kRsEdge;
    const double u3 = -2.0 * as, u7 = fmin(2.0 - r, 0.0);
#pragma unroll
    for (int flip = 0; flip < 2; ++flip) {
        const double th = flip ? V.thf : V.th, ph = flip ? -phi : phi, sg = flip ? -1.0 : 1.0;
        const int tr = flip + 2 * mirror;
        if (!back) {
            bool ok = true;
            const double t = rs_pos(th, ok), v = rs_pos(ph - t, ok);
            rs_take3(b, R, sg, 0 + tr, ok, t, V.rho > 0.0 ? rho_m : 0.0, v, true);
        }
        {
            bool ok = ok_ccc;
            const double t = rs_pos(th + (kPi - as), ok);
            if (!back) {
                const double v = dubins_wrap_pi((ph - t) + u3);
                rs_take3(b, R, sg, (v >= 0.0 ? 8 : 12) + tr, ok, t, u3, v);
            } else {
                const double v = rs_neg((ph - t) + u3, ok);
                rs_take3(b, R, sg, 16 + tr, ok, v, u3, t);
            }
        }
        {
            bool ok = ok_ccsc;
            const double t = rs_pos(th + (kHalfPi + beta), ok), v = rs_neg((ph - kHalfPi) - t, ok);
            if (!back) rs_take4(b, R, sg, 28 + tr, ok, t, -kHalfPi, u7, v);
            else rs_take4(b, R, sg, 36 + tr, ok, v, u7, -kHalfPi, t);
        }
    }
}

// The words of a "plus" vector: bases 1, 5, 6, 8, 11; backwards only base 10.
template <class ACC>
FCPP_HD void rs_plus_words(ACC &b, double R, const RsVec &V, double phi, int mirror, bool back, double r_m = 0.0)
{
    // (the backwards plus vectors come through rs_polar, e4 = rho^2 - 4 as it is: there it only decides base 10's edge rho >= 2, where the word's
    //  straight is 0 and a word of nearly the same length competes -- no root is taken of it)
    const double e4 = V.e4;
    const bool ok2 = e4 >= -4.0 * kRsEdge;                     // rho >= 2
    const double u8 = fmin(2.0 - V.rho, 0.0);
    if (back) {
#pragma unroll
        for (int flip = 0; flip < 2; ++flip) {
            const double th = flip ? V.thf : V.th, ph = flip ? -phi : phi, sg = flip ? -1.0 : 1.0;
            bool ok = ok2;
            const double t = rs_pos(th + kHalfPi, ok), v = rs_neg((t + kHalfPi) - ph, ok);
            rs_take4(b, R, sg, 40 + flip + 2 * mirror, ok, v, u8, -kHalfPi, t);
        }
        return;
    }
    const double r = sqrt(fmax(e4, 0.0)), beta = atan2_fd(2.0, r);
    // 8.7: cos u = (2 + rho) / 4
    const bool ok5 = -e4 >= -4.0 * kRsEdge;                    // rho <= 2
    const double cu = fmin((2.0 + V.rho) * 0.25, 1.0), su = sqrt(fmax(1.0 - cu * cu, 0.0));
    const double u5 = atan2_fd(su, cu);
    // 8.8: cos u = (20 - rho^2) / 16, u <= 0
    const double e20 = 20.0 - V.rho2;
    const bool ok6 = ok2 && e20 >= -20.0 * kRsEdge, ok11 = -e20 >= -20.0 * kRsEdge;
    const double c6 = fmin(fmax(e20 * 0.0625, 0.0), 1.0), s6 = sqrt(fmax(1.0 - c6 * c6, 0.0));
    const double u6 = -atan2_fd(s6, c6), g6 = atan2_fd(s6, 2.0 - c6);
    const double u11 = fmin(4.0 - r, 0.0);
#pragma unroll
    for (int flip = 0; flip < 2; ++flip) {
        const double th = flip ? V.thf : V.th, ph = flip ? -phi : phi, sg = flip ? -1.0 : 1.0;
        const int tr = flip + 2 * mirror;
        {
            bool ok = ok2;
            const double t = rs_pos(th + beta, ok), v = rs_pos(t - ph, ok);
            rs_take3(b, R, sg, 4 + tr, ok, t, r_m, v, true);
        }
        {
            bool ok = ok5;
            const double t = rs_pos(th + (kHalfPi + u5), ok), v = rs_neg((t - 2.0 * u5) - ph, ok);
            rs_take4(b, R, sg, 20 + tr, ok, t, u5, -u5, v);
        }
        {
            bool ok = ok6;
            const double t = rs_pos(th + (kHalfPi + g6), ok), v = rs_pos(t - ph, ok);
            rs_take4(b, R, sg, 24 + tr, ok, t, u6, u6, v);
        }
        {
            bool ok = ok2;
            const double t = rs_pos(th + kHalfPi, ok), v = rs_neg((t + kHalfPi) - ph, ok);
            rs_take4(b, R, sg, 32 + tr, ok, t, -kHalfPi, u8, v);
        }
        {
            bool ok = ok11;
            const double t = rs_pos(th + (kHalfPi + beta), ok), v = rs_pos(t - ph, ok);
            rs_take5(b, R, sg, 44 + tr, ok, t, -kHalfPi, u11, -kHalfPi, v);
        }
    }
}

// what depends on ONE pose only: hoisted out of the pair loop of the matrix kernel
struct RsPose { double x, y, h, sn, cs; };          // sn = sin h, cs = cos h
FCPP_HD RsPose rs_prep(double x, double y, double h)
{
    double sn, cs;
    fc_sincos(h, sn, cs);
    return { x, y, h, sn, cs };
}

// all 48 words evaluated (no branch by word), each handed to rs_keep(acc, ...)
template <class ACC>
FCPP_HD void rs_words(const RsPose &f, const RsPose &t, double R, ACC &b)
{
    const double dx = t.x - f.x, dy = t.y - f.y, inv = 1.0 / R;
    const double xm = dx * f.cs + dy * f.sn, ym = dy * f.cs - dx * f.sn, x = xm * inv, y = ym * inv;
    const double phi = t.h - f.h;
    double s, c;
    fc_sincos(phi, s, c);
    const double xb = x * c + y * s, yb = x * s - y * c;
    const double Rs = R * s, Rc = R * c, ax = xm - Rs, ay = (ym - R) + Rc, bx = xm + Rs, by = (-ym - R) + Rc;      // the 8.1 vectors in metres
    rs_minus_words(b, R, rs_polar(x - s, (y - 1.0) + c), phi, 0, false, sqrt(ax * ax + ay * ay));
    rs_minus_words(b, R, rs_polar(x + s, (-y - 1.0) + c), -phi, 1, false, sqrt(bx * bx + by * by));
    const double omc = c > 0.0 ? (s * s) / (1.0 + c) : 1.0 - c;          // 1 - cos phi without the cancellation (exactly 0 for equal headings)
    // (the straight of 8.2 in metres, like that of 8.1: sqrt(X^2 + (Y - 2R)(Y + 2R)) of the same vector times R)
    const double Ro = R * omc, twoR = 2.0 * R;
    const double rc = sqrt(fmax(bx * bx + (((ym - R) - Rc) - twoR) * (ym + Ro), 0.0)), rd = sqrt(fmax(ax * ax + (((-ym - R) - Rc) - twoR) * (Ro - ym), 0.0));
    rs_plus_words(b, R, rs_polar_plus(x + s, (y - 1.0) - c, y + omc), phi, 0, false, rc);
    rs_plus_words(b, R, rs_polar_plus(x - s, (-y - 1.0) - c, omc - y), -phi, 1, false, rd);
    rs_minus_words(b, R, rs_polar(xb - s, (yb - 1.0) + c), phi, 0, true);
    rs_minus_words(b, R, rs_polar(xb + s, (-yb - 1.0) + c), -phi, 1, true);
    rs_plus_words(b, R, rs_polar(xb + s, (yb - 1.0) - c), phi, 0, true);
    rs_plus_words(b, R, rs_polar(xb - s, (-yb - 1.0) - c), -phi, 1, true);
}

// are the pair's inputs such that a word can be had at all?  (the solvers' "word -1" rule, the totals aside)
FCPP_HD bool rs_inputs_finite(const RsPose &f, const RsPose &t)
{
    return dubins_finite(t.x - f.x) && dubins_finite(t.y - f.y) && dubins_finite(f.h) && dubins_finite(t.h);
}

// the shortest word selected.  seg: five signed lengths.
FCPP_HD void rs_solve_prepped(const RsPose &f, const RsPose &t, double R, int &word, double *seg, double &total)
{
    RsBest b = { INFINITY, 0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    rs_words(f, t, R, b);
    const bool ok = rs_inputs_finite(f, t) && dubins_finite(b.total);
    const double nan = __builtin_nan("");
    word = ok ? b.word : -1;
    // (+ 0.0: a segment of length 0 under a flip is +0, not -0)
    seg[0] = ok ? b.s0 + 0.0 : nan; seg[1] = ok ? b.s1 + 0.0 : nan; seg[2] = ok ? b.s2 + 0.0 : nan; seg[3] = ok ? b.s3 + 0.0 : nan; seg[4] = ok ? b.s4 + 0.0 : nan;
    total = ok ? b.total : nan;
}

FCPP_HD void rs_solve(double x0, double y0, double h0, double x1, double y1, double h1, double R, int &word, double *seg, double &total)
{
    rs_solve_prepped(rs_prep(x0, y0, h0), rs_prep(x1, y1, h1), R, word, seg, total);
}

// ---- gear runs: what the sampler walks ------------------------------------------------------------------------------------------------
// A run is a maximal stretch of segments driven in one gear; segments of length 0 belong to the run around them.  A word has at most two
// cusps, so at most three runs.  first[r] .. last[r]: the run's first and last segment of non-zero length, len[r] the sum of |seg| over
// them in order, gear[r] = +1 / -1.  A path of total 0 is one run of length 0 in the gear of the word's first segment.  -> number of runs
struct RsRuns { int n; int first[3], last[3], gear[3]; double len[3]; };
FCPP_HD RsRuns rs_runs(int word, const double *seg)
{
    RsRuns r;
    r.n = 0;
    for (int j = 0; j < 3; ++j) { r.first[j] = r.last[j] = 0; r.gear[j] = 1; r.len[j] = 0.0; }
    for (int k = 0; k < 5; ++k) {
        const double v = seg[k];
        if (!(v != 0.0) || !(v == v)) continue;
        const int g = v > 0.0 ? 1 : -1;
        if (r.n == 0 || (g != r.gear[r.n - 1] && r.n < 3)) { r.first[r.n] = k; r.gear[r.n] = g; r.len[r.n] = 0.0; ++r.n; }
        r.last[r.n - 1] = k;
        r.len[r.n - 1] += fabs(v);
    }
    if (r.n == 0) { r.n = 1; r.gear[0] = rs_gear(word, 0) < 0 ? -1 : 1; }
    return r;
}

// The pose on segment k of the path (word, seg) that starts at (x0, y0, h0), at the SIGNED position u from that segment's start (u has the
// sign of seg[k] and is clamped to it), with the signed curvature there (+1/R left, -1/R right, 0 straight) and the gear (+1 / -1).
// Evaluated from the START OF THE SEGMENT -- the segment start poses are closed forms of the start pose -- never from a previous sample.
// The heading is the VEHICLE's (on a reverse segment it points against the motion), in (-pi, pi].  word outside 0 .. 47, k outside 0 .. 4
// or u NaN: NaN and gear 0.
FCPP_HD void rs_pose_at(double x0, double y0, double h0, double R, int word, const double *seg, int k, double u, double &x, double &y,
                        double &h, double &kappa, int &gear)
{
    if (word < 0 || word >= RS_WORDS || k < 0 || k > 4 || !(u == u)) { x = y = h = kappa = __builtin_nan(""); gear = 0; return; }
    const double sk = seg[k];
    if (sk >= 0.0) u = fmin(fmax(u, 0.0), sk); else u = fmax(fmin(u, 0.0), sk);
    double px = x0, py = y0, ph = h0, sn, cs;
    fc_sincos(ph, sn, cs);
    for (int j = 0; j <= k; ++j) {
        const double len = j < k ? seg[j] : u;
        const int sg = rs_turn(word, j);
        if (sg == 0) { px += len * cs; py += len * sn; continue; }
        const double nh = sg > 0 ? ph + len / R : ph - len / R;
        double s2, c2;
        fc_sincos(nh, s2, c2);
        if (sg > 0) { px += R * (s2 - sn); py -= R * (c2 - cs); }
        else        { px -= R * (s2 - sn); py += R * (c2 - cs); }
        ph = nh; sn = s2; cs = c2;
    }
    const int sgk = rs_turn(word, k);
    x = px; y = py; h = dubins_wrap_pi(ph);
    kappa = sgk == 0 ? 0.0 : (sgk > 0 ? 1.0 / R : -(1.0 / R));
    gear = sk > 0.0 ? 1 : (sk < 0.0 ? -1 : rs_gear(word, k));
}

// The pose at distance e >= 0 from the start of run r: the segment that holds it (a junction belongs to the segment that starts there;
// e >= the run's length is the end of its last segment), then rs_pose_at.
FCPP_HD void rs_pose_in_run(double x0, double y0, double h0, double R, int word, const double *seg, const RsRuns &runs, int r, double e,
                            double &x, double &y, double &h, double &kappa, int &gear)
{
    int k = runs.first[r];
    double left = e;
    if (e >= runs.len[r]) { k = runs.last[r]; left = fabs(seg[k]); }
    else
        while (k < runs.last[r] && left >= fabs(seg[k])) { left -= fabs(seg[k]); ++k; }
    rs_pose_at(x0, y0, h0, R, word, seg, k, runs.gear[r] > 0 ? left : -left, x, y, h, kappa, gear);
    if (gear != 0 && seg[k] == 0.0) gear = runs.gear[r];
}

}  // namespace fcpp
