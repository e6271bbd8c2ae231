// fcpp_clearfn.h -- connector clearance: does a SOLVED Dubins or Reeds-Shepp connector stay inside a polygon field?  ONE set of expressions
// for the host (fcpp_debug_conn_clear, fcpp_debug_route_transit_clear, the tests' driver) and the device (fcpp_clear.hip), written like
// fcpp_routefn.h in plain IEEE-754 double operations and compiled with -ffp-contract=off on both sides, so that both give the same bits.
// Build-defined: the reference's connectors are straight lines that are never tested.  A test, not a planner: no path is re-shaped here.
//
// THE RULE (include/fcpp.h states it for callers).
//   region    a field of the two-level CSR of the swath entries: rings, closed implicitly, either orientation, even-odd interior.  Edge g of
//             a ring runs from vertex g to vertex g + 1 (the last one back to the first): A = (x0, y0), B = (x1, y1), e = fl(B - A), the
//             points A + t e with t in [0, 1).  A margin is no parameter: inset the field first.
//   path      start pose, R, word, seg as Conn<MODE>::solve wrote them (3 segments, or 5 signed ones).  Piece k is segment k if seg[k] != 0:
//             from P_k to Q_k, where Q_k is the pose at the END of segment k by the samplers' closed form (dubins_pose_at at the prefix sum
//             seg[0] + .. + seg[k] added left to right, rs_pose_at at u = seg[k]) and P_k = Q_j of the piece before (the start pose for the
//             first): neighbours share their junction's bits.  A straight is the segment P Q.  An arc has the centre
//             c = P +- R (-sin h, cos h) (+ left, - right; h the heading at P), runs from u = P - c to v = Q - c counter-clockwise when
//             turn x gear > 0, else clockwise, and is WIDE when |seg[k]| / R > pi.  s_k = |seg[0]| + .. + |seg[k - 1]|, left to right.
//   straight x edge   o1 = e_p x (A - P), o2 = e_p x (B - P), o3 = e x (P - A), o4 = e x (Q - A), e_p = Q - P:  a crossing iff
//             (o1 >= 0) != (o2 >= 0) and (o3 >= 0) != (o4 >= 0) -- half-open on both, so a path through a vertex is counted on one of the
//             two edges there, and collinear overlap is none.  At s = s_k + fmin(o3 / (o3 - o4), 1) |seg[k]|.
//   arc x edge        f = A - c, a = e.e, b = f.e, q = f.f - R^2, D = b b - a q:  for D > 0 (a tangent edge does not cross) the roots
//             t = (-b -+ sqrt D) / a with 0 <= t < 1 give d = f + t e; d lies on the arc iff, with c1 = +-(u x d), c2 = +-(d x v) (- for
//             a clockwise arc):  narrow: c1 >= 0 and c2 >= 0 and (u.d >= 0 or v.d >= 0);  wide: not (c1 < 0 and c2 < 0).  Every root kept
//             is a crossing (an arc may cross one edge twice), at s = s_k + fmin(R atan2(+-(u x d), u.d) [+ 2 pi if negative], |seg[k]|).
//   crossings the (straight piece, edge) pairs that cross plus the kept roots of the (arc piece, edge) pairs;  first_s the least s over
//             them, +inf if none;
//   inside    even-odd membership of the START point S: edge counted iff (y0 > S.y) != (y1 > S.y) and S lies left of it there,
//             (S.x - x0) e.y < (S.y - y0) e.x for e.y > 0 and > for e.y < 0 -- no division;   clear = inside and crossings == 0.
//   unsolved  word outside the mode's table or a NaN segment: crossings 0, inside 0, first_s NaN, not clear.
//   field     status CLEAR_EINVAL for a field with no ring, a ring of fewer than 3 vertices or a vertex that is not finite: every path
//             tested against it gets the unsolved path's result.  A path with field -1 ("no region") is clear: 0, inside 1, +inf.
// There is no cap on the edges of a field: the device walks them in LDS chunks of CLEAR_EDGE_CHUNK, and skips a chunk whose bounding box
// neither meets the path's (arcs: the box of their whole circle) nor the ray S + (t, 0); a skipped edge could not have counted.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_connfn.h"
#include "fcpp_routefn.h"

namespace fcpp {

constexpr int CLEAR_EDGE_CHUNK = 256;                    // FCPP_CLEAR_EDGE_CHUNK of include/fcpp.h
constexpr int CLEAR_OK = 0, CLEAR_EINVAL = -1;          // FCPP_OK / FCPP_EINVAL
constexpr int CLEAR_NONE = 0, CLEAR_LINE = 1, CLEAR_CCW = 2, CLEAR_CW = 3;

// kind: CLEAR_NONE for a segment of length 0.  (cx, cy): the arc's centre.  s0: the path length before the piece, len = |seg[k]|.
struct ClearPiece { double px, py, qx, qy, cx, cy, s0, len; int kind; bool wide; };

struct ClearBox { double x0, y0, x1, y1; };             // min and max corner

// what the edge loop accumulates for one path
struct ClearAcc { int crossings, parity; double first_s; };

struct ClearResult { int32_t crossings; int8_t inside; double first_s; bool clear; };

FCPP_HD bool clear_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }          // false for NaN
FCPP_HD bool clear_vertex_ok(double x, double y) { return clear_finite(x) && clear_finite(y); }

// ---- the path's pieces ------------------------------------------------------------------------------------------------------------
template <int MODE> FCPP_HD bool clear_solved(int word, const double *seg);
template <> FCPP_HD bool clear_solved<0>(int word, const double *seg)
{
    return word >= 0 && word <= 5 && seg[0] == seg[0] && seg[1] == seg[1] && seg[2] == seg[2];
}
template <> FCPP_HD bool clear_solved<1>(int word, const double *seg) { return Conn<1>::solved(word, seg); }

// turn of segment k (+1 left, -1 right, 0 straight) and the position at its END: the samplers' closed forms, nothing chained here
template <int MODE> FCPP_HD int clear_turn(int word, int k);
template <> FCPP_HD int clear_turn<0>(int word, int k) { return dubins_turn(word, k); }
template <> FCPP_HD int clear_turn<1>(int word, int k) { return rs_turn(word, k); }

template <int MODE>
FCPP_HD void clear_segment_end(double x0, double y0, double h0, double R, int word, const double *seg, int k, double &x, double &y, double &h);
template <>
FCPP_HD void clear_segment_end<0>(double x0, double y0, double h0, double R, int word, const double *seg, int k, double &x, double &y, double &h)
{
    const double s = k == 0 ? seg[0] : (k == 1 ? seg[0] + seg[1] : (seg[0] + seg[1]) + seg[2]);
    double kappa;
    dubins_pose_at(x0, y0, h0, R, word, seg[0], seg[1], seg[2], s, x, y, h, kappa);
}
template <>
FCPP_HD void clear_segment_end<1>(double x0, double y0, double h0, double R, int word, const double *seg, int k, double &x, double &y, double &h)
{
    double kappa;
    int gear;
    rs_pose_at(x0, y0, h0, R, word, seg, k, seg[k], x, y, h, kappa, gear);
}

// pc[0 .. NSEG - 1] and the box of the whole path; false (every piece CLEAR_NONE) for an unsolved path
template <int MODE>
FCPP_HD bool clear_pieces(double x0, double y0, double h0, double R, int word, const double *seg, ClearPiece *pc, ClearBox &box)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    box.x0 = box.x1 = x0;
    box.y0 = box.y1 = y0;
    const bool ok = clear_solved<MODE>(word, seg) && clear_finite(x0) && clear_finite(y0) && clear_finite(h0);
    double px = x0, py = y0, ph = h0, s0 = 0.0;
#pragma unroll
    for (int k = 0; k < NSEG; ++k) {
        ClearPiece &p = pc[k];
        p.px = p.py = p.qx = p.qy = p.cx = p.cy = p.s0 = p.len = 0.0;
        p.kind = CLEAR_NONE;
        p.wide = false;
        if (!ok || !(seg[k] != 0.0)) continue;
        const double len = fabs(seg[k]);
        const int turn = clear_turn<MODE>(word, k);
        double qx, qy, qh;
        clear_segment_end<MODE>(x0, y0, h0, R, word, seg, k, qx, qy, qh);
        p.px = px; p.py = py; p.qx = qx; p.qy = qy; p.s0 = s0; p.len = len;
        if (turn == 0) {
            p.kind = CLEAR_LINE;
            box.x0 = fmin(box.x0, qx); box.x1 = fmax(box.x1, qx);
            box.y0 = fmin(box.y0, qy); box.y1 = fmax(box.y1, qy);
        } else {
            double sn, cs;
            fc_sincos(ph, sn, cs);
            p.cx = turn > 0 ? px - R * sn : px + R * sn;
            p.cy = turn > 0 ? py + R * cs : py - R * cs;
            p.kind = ((turn > 0) == (seg[k] > 0.0)) ? CLEAR_CCW : CLEAR_CW;
            p.wide = len / R > kPi;
            box.x0 = fmin(box.x0, p.cx - R); box.x1 = fmax(box.x1, p.cx + R);
            box.y0 = fmin(box.y0, p.cy - R); box.y1 = fmax(box.y1, p.cy + R);
        }
        px = qx; py = qy; ph = qh;
        s0 += len;
    }
    return ok;
}

// ---- one edge against the pieces -------------------------------------------------------------------------------------------------------
FCPP_HD void clear_hit(ClearAcc &a, double s) { if (s < a.first_s) a.first_s = s; }

// is d = (hit - centre) on the arc, and at which length from the piece's start?  (false leaves s alone)
FCPP_HD bool clear_on_arc(const ClearPiece &p, double R, double ux, double uy, double vx, double vy, double dx, double dy, double &s)
{
    const double sg = p.kind == CLEAR_CCW ? 1.0 : -1.0;
    const double cr1 = sg * (ux * dy - uy * dx), c2 = sg * (dx * vy - dy * vx);
    const double dt1 = ux * dx + uy * dy;
    const bool on = p.wide ? !(cr1 < 0.0 && c2 < 0.0) : (cr1 >= 0.0 && c2 >= 0.0 && (dt1 >= 0.0 || vx * dx + vy * dy >= 0.0));
    if (!on) return false;
    double ang = atan2_fd(cr1, dt1);
    if (ang < 0.0) ang += kDubTwoPiHi;
    s = fmin(R * ang, p.len);
    return true;
}

// edge A = (x0, y0), B = (x1, y1), e = (ex, ey) = fl(B - A) against the NSEG pieces of a path that starts at (sx, sy)
template <int NSEG>
FCPP_HD void clear_edge(const ClearPiece *pc, double sx, double sy, double R, double x0, double y0, double x1, double y1, double ex, double ey,
                        ClearAcc &a)
{
    if ((y0 > sy) != (y1 > sy)) {
        const double l = (sx - x0) * ey, r = (sy - y0) * ex;
        if (ey > 0.0 ? l < r : l > r) a.parity ^= 1;
    }
    const double ee = ex * ex + ey * ey, R2 = R * R;
#pragma unroll
    for (int k = 0; k < NSEG; ++k) {
        const ClearPiece &p = pc[k];
        if (p.kind == CLEAR_NONE) continue;
        if (p.kind == CLEAR_LINE) {
            const double wx = p.qx - p.px, wy = p.qy - p.py;
            const double ax = x0 - p.px, ay = y0 - p.py, bx = x1 - p.px, by = y1 - p.py;
            const double o1 = wx * ay - wy * ax, o2 = wx * by - wy * bx;
            if ((o1 >= 0.0) == (o2 >= 0.0)) continue;
            const double o3 = ey * ax - ex * ay, o4 = ex * (p.qy - y0) - ey * (p.qx - x0);      // o3 = e x (P - A)
            if ((o3 >= 0.0) == (o4 >= 0.0)) continue;
            ++a.crossings;
            clear_hit(a, p.s0 + fmin(o3 / (o3 - o4), 1.0) * p.len);
            continue;
        }
        const double fx = x0 - p.cx, fy = y0 - p.cy;
        const double b = fx * ex + fy * ey, q = (fx * fx + fy * fy) - R2, D = b * b - ee * q;
        if (!(D > 0.0)) continue;
        const double rt = sqrt(D), t1 = (-b - rt) / ee, t2 = (-b + rt) / ee;
        const bool in1 = t1 >= 0.0 && t1 < 1.0, in2 = t2 >= 0.0 && t2 < 1.0;
        if (!in1 && !in2) continue;
        const double ux = p.px - p.cx, uy = p.py - p.cy, vx = p.qx - p.cx, vy = p.qy - p.cy;
        double s1 = INFINITY, s2 = INFINITY;
        const bool h1 = in1 && clear_on_arc(p, R, ux, uy, vx, vy, fx + t1 * ex, fy + t1 * ey, s1);
        const bool h2 = in2 && clear_on_arc(p, R, ux, uy, vx, vy, fx + t2 * ex, fy + t2 * ey, s2);
        if (!h1 && !h2) continue;
        a.crossings += (h1 ? 1 : 0) + (h2 ? 1 : 0);
        clear_hit(a, p.s0 + fmin(s1, s2));
    }
}

// ---- results ------------------------------------------------------------------------------------------------------------------------
FCPP_HD ClearAcc clear_begin() { return { 0, 0, INFINITY }; }

// solved: the path has pieces; valid: its field has status 0
FCPP_HD ClearResult clear_finish(bool solved, bool valid, const ClearAcc &a)
{
    if (!solved || !valid) return { 0, 0, __builtin_nan(""), false };
    const bool in = a.parity != 0;
    return { a.crossings, (int8_t)(in ? 1 : 0), a.first_s, in && a.crossings == 0 };
}
FCPP_HD ClearResult clear_no_region() { return { 0, 1, INFINITY, true }; }

// ---- a field of the CSR, walked edge by edge -----------------------------------------------------------------------------------------
struct ClearFields { int64_t n; const int64_t *ring_off, *vert_off; const double *x, *y; };

// the field's status: CLEAR_EINVAL for no ring, a ring of fewer than 3 vertices, a vertex that is not finite
FCPP_HD int clear_field_status(const ClearFields &F, int64_t f)
{
    const int64_t r0 = F.ring_off[f], r1 = F.ring_off[f + 1];
    if (r1 <= r0) return CLEAR_EINVAL;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t v0 = F.vert_off[r], v1 = F.vert_off[r + 1];
        if (v1 - v0 < 3) return CLEAR_EINVAL;
        for (int64_t v = v0; v < v1; ++v)
            if (!clear_vertex_ok(F.x[v], F.y[v])) return CLEAR_EINVAL;
    }
    return CLEAR_OK;
}

// every edge of field f against the pieces; false for a field whose status is CLEAR_EINVAL (then `a` means nothing)
template <int NSEG>
FCPP_HD bool clear_walk(const ClearFields &F, int64_t f, const ClearPiece *pc, double sx, double sy, double R, ClearAcc &a)
{
    const int64_t r0 = F.ring_off[f], r1 = F.ring_off[f + 1];
    bool ok = r1 > r0;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t v0 = F.vert_off[r], v1 = F.vert_off[r + 1];
        if (v1 - v0 < 3) { ok = false; continue; }
        double x0 = F.x[v1 - 1], y0 = F.y[v1 - 1];          // the closing edge first: one load per vertex
        ok = ok && clear_vertex_ok(x0, y0);
        for (int64_t v = v0; v < v1; ++v) {
            const double x1 = F.x[v], y1 = F.y[v];
            ok = ok && clear_vertex_ok(x1, y1);
            clear_edge<NSEG>(pc, sx, sy, R, x0, y0, x1, y1, x1 - x0, y1 - y0, a);
            x0 = x1; y0 = y1;
        }
    }
    return ok;
}

// a path against field f: f = -1 no region; f outside [-1, n) counts as a field of status CLEAR_EINVAL
template <int MODE>
FCPP_HD ClearResult clear_path(const ClearFields &F, int64_t f, double x0, double y0, double h0, double R, int word, const double *seg)
{
    if (f == -1) return clear_no_region();
    ClearPiece pc[Conn<MODE>::NSEG];
    ClearBox box;
    const bool solved = clear_pieces<MODE>(x0, y0, h0, R, word, seg, pc, box);
    if (!solved || f < 0 || f >= F.n) return clear_finish(false, false, clear_begin());
    ClearAcc a = clear_begin();
    const bool valid = clear_walk<Conn<MODE>::NSEG>(F, f, pc, x0, y0, R, a);
    return clear_finish(true, valid, a);
}

// ---- the transit block ------------------------------------------------------------------------------------------------------------------
// the canonical pair (p, q) of field i's block, p and q of different swaths: its connector solved as route_transit solves it and tested
// against field i -> blocked?
template <int MODE>
FCPP_HD bool clear_transit_blocked(const ClearFields &F, int64_t i, const double *ax, const double *ay, const double *bx, const double *by,
                                   double theta, double R, int p, int q)
{
    double x0, y0, h0, x1, y1, h1, total;
    route_pose(ax, ay, bx, by, theta, p, true, x0, y0, h0);
    route_pose(ax, ay, bx, by, theta, q, false, x1, y1, h1);
    int word;
    double seg[Conn<MODE>::NSEG];
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, R, word, seg, total);
    return !clear_path<MODE>(F, i, x0, y0, h0, R, word, seg).clear;
}

}  // namespace fcpp
