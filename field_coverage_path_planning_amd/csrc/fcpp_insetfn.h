// fcpp_insetfn.h -- the inset of ANY polygon field: the set of points inside a field (rings: ring 0 the outer boundary, further rings holes)
// that lie at least d from its boundary -- the centre line of a headland pass (its boundary at d = first + (k - 1) W) and the work area
// that m passes leave (d = m W).  ONE set of expressions for the host (fcpp_debug_inset, the tests' subject) and the device
// (fcpp_inset.hip), written like fcpp_swathfn.h in plain IEEE-754 double operations with fc_sincos / atan2_fd and compiled with
// -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the reference insets a convex quadrilateral by mitres.
//
// THE RULE (include/fcpp.h states it for callers).
//   orient    every ring is oriented by the sign of its shoelace area (summed in vertex order about the ring's first vertex) so that the
//             interior lies on the LEFT: ring 0 counter-clockwise, holes clockwise; a ring of the other orientation is traversed backwards.
//             Edge g, in that traversal order, runs from p_g to q_g with the unit direction u_g, the left normal n_g = (-u_y, u_x) and the
//             length L_g; an edge of length 0 has u = 0 (it offsets to nothing and still removes like a point).
//   prims     primitive 2 g: the offset segment  p_g + d n_g + t u_g,  0 <= t <= L_g.  Primitive 2 g + 1 exists iff the turn at q_g is to the
//             right, cross(u_g, u_next) < 0: the arc  q_g + d (n_g cos s + u_g sin s),  0 <= s <= atan2(-cross, dot) < pi, from n_g to n_next.
//   removal   a point of a primitive is removed iff its distance to some OTHER edge (a segment skips its own edge, an arc its two) is below
//             d (1 - 1e-12).  Per (primitive, edge): the parameters at which the primitive meets the two end circles of radius d and the two
//             side lines at distance d of the edge -- at most 8 inside (0, T) -- are sorted; every interval between consecutive ones is
//             judged at its midpoint by the plain point-to-segment distance.  The candidates carry no slack, so corners come out exact.
//   pieces    what survives of a primitive, found by a sweep: advance t past every removed interval that contains it until none does (the
//             piece's start), then the piece ends at the least start of a removed interval beyond t, or at T.  Pieces shorter than 1e-9 m
//             (arcs: d times the angle) are dropped.  Pieces are numbered by (primitive, start).
//   stitch    succ(k) = the piece whose start is nearest to the end of k by squared distance, ties to the lowest number.  From the lowest
//             unused piece follow succ until it returns to that piece: one ring.  Reaching another used piece: INSET_EUNSUPPORTED (the
//             critical distance at which offsets meet in one point).  gap = the largest end-to-start distance over all pieces.
//   vertices  a segment piece emits its start point; an arc piece spanning D rad emits m = ceil(D / arc_step) points at t0 + k (D / m).
//   status    INSET_EINVAL: no ring, a ring with fewer than 3 vertices, a vertex that is not finite.  INSET_EUNSUPPORTED: more than
//             INSET_MAX_EDGES edges, more than 4 x edges pieces, an arc piece of INSET_MAX_ARC_VERTS points or more, the degenerate walk.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "fcpp_math.h"

namespace fcpp {

constexpr int INSET_MAX_EDGES = 1024;                    // FCPP_INSET_MAX_EDGES of include/fcpp.h
constexpr int INSET_PIECES_PER_EDGE = 4;                 // FCPP_INSET_PIECES_PER_EDGE: the piece cap of a field is this times its edges
constexpr int INSET_MAX_ARC_VERTS = 1 << 18;
constexpr int INSET_OK = 0, INSET_EINVAL = -1, INSET_EUNSUPPORTED = -3;      // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr double INSET_SLACK = 1e-12, INSET_MIN_PIECE = 1e-9;
constexpr double INSET_MAX_ARC_STEP = 1.57079632679489661923;

FCPP_HD bool inset_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }          // false for NaN

// a field's oriented edges (the device keeps them in LDS)
struct InsetEdges {
    const double *px, *py, *ux, *uy, *len;
    const uint16_t *nxt;            // the edge that follows g in its ring
    int E;
};

// One ring of m >= 3 vertices at vx, vy (in place): turned so that the interior is on the left, nxt[0 .. m - 1] = base + the next index
FCPP_HD void inset_orient_ring(double *vx, double *vy, uint16_t *nxt, int base, int m, bool outer)
{
    const double x0 = vx[0], y0 = vy[0];
    double a = 0.0;
    for (int t = 1; t + 1 < m; ++t) a += (vx[t] - x0) * (vy[t + 1] - y0) - (vx[t + 1] - x0) * (vy[t] - y0);
    if (outer ? a < 0.0 : a > 0.0)
        for (int t = 0, b = m - 1; t < b; ++t, --b) {
            const double sx = vx[t], sy = vy[t];
            vx[t] = vx[b]; vy[t] = vy[b];
            vx[b] = sx; vy[b] = sy;
        }
    for (int t = 0; t < m; ++t) nxt[t] = (uint16_t)(base + (t + 1 == m ? 0 : t + 1));
}

FCPP_HD void inset_edge(double px, double py, double qx, double qy, double &ux, double &uy, double &len)
{
    const double dx = qx - px, dy = qy - py;
    len = sqrt(dx * dx + dy * dy);
    ux = len > 0.0 ? dx / len : 0.0;
    uy = len > 0.0 ? dy / len : 0.0;
}

struct InsetPrim {
    int arc;                    // 0: offset segment, 1: arc
    double ox, oy;              // the segment's start, or the arc's centre
    double ux, uy, nx, ny;      // direction and left normal of the primitive's edge
    double T;                   // length, or angle
    int skip0, skip1;           // the edges that do not remove from it
};

// primitive q of the field at distance d; false when it does not exist
FCPP_HD bool inset_prim(const InsetEdges &e, int q, double d, InsetPrim &p)
{
    const int g = q >> 1;
    p.ux = e.ux[g]; p.uy = e.uy[g];
    p.nx = -p.uy; p.ny = p.ux;
    p.arc = q & 1;
    if (!p.arc) {
        p.ox = e.px[g] + d * p.nx;
        p.oy = e.py[g] + d * p.ny;
        p.T = e.len[g];
        p.skip0 = p.skip1 = g;
        return p.T > 0.0;
    }
    const int h = e.nxt[g];
    const double cr = p.ux * e.uy[h] - p.uy * e.ux[h], dt = p.ux * e.ux[h] + p.uy * e.uy[h];
    if (!(cr < 0.0)) return false;
    p.ox = e.px[h]; p.oy = e.py[h];
    p.T = atan2_fd(-cr, dt);
    p.skip0 = g; p.skip1 = h;
    return p.T > 0.0;
}

FCPP_HD void inset_point(const InsetPrim &p, double d, double t, double &x, double &y)
{
    if (!p.arc) {
        x = p.ox + t * p.ux;
        y = p.oy + t * p.uy;
    } else {
        double s, c;
        fc_sincos(t, s, c);
        x = p.ox + d * (p.nx * c + p.ux * s);
        y = p.oy + d * (p.ny * c + p.uy * s);
    }
}

// squared distance of (x, y) to edge j
FCPP_HD double inset_dist2(const InsetEdges &e, int j, double x, double y)
{
    const double wx = x - e.px[j], wy = y - e.py[j], ux = e.ux[j], uy = e.uy[j];
    const double tau = fmin(fmax(wx * ux + wy * uy, 0.0), e.len[j]);
    const double rx = wx - tau * ux, ry = wy - tau * uy;
    return rx * rx + ry * ry;
}

// a candidate parameter: itself inside (0, T), else 0 (which opens an empty interval)
FCPP_HD double inset_cand(double t, double T) { return t > 0.0 && t < T ? t : 0.0; }
// the parameter of the arc's point v + (rx, ry)
FCPP_HD double inset_arc_param(const InsetPrim &p, double rx, double ry) { return atan2_fd(rx * p.ux + ry * p.uy, rx * p.nx + ry * p.ny); }

#define FCPP_INSET_CE(a, b) do { const double lo_ = fmin(a, b), hi_ = fmax(a, b); a = lo_; b = hi_; } while (0)

// One edge against one primitive within the sweep: t = the sweep's position, nxt = the least start of a removed interval beyond it so far.
FCPP_HD void inset_sweep_edge(const InsetEdges &e, const InsetPrim &p, double d, double ds2, int j, double &t, double &nxt)
{
    const double T = p.T, pjx = e.px[j], pjy = e.py[j], ujx = e.ux[j], ujy = e.uy[j], Lj = e.len[j];
    const double qjx = pjx + Lj * ujx, qjy = pjy + Lj * ujy, njx = -ujy, njy = ujx;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0, c5 = 0.0, c6 = 0.0, c7 = 0.0;
    if (!p.arc) {
        // (a conservative reject: the capsule of edge j lies wholly before t, beyond nxt, or off to one side of the line)
        const double ax = pjx - p.ox, ay = pjy - p.oy, bx = qjx - p.ox, by = qjy - p.oy;
        const double ta = ax * p.ux + ay * p.uy, tb = bx * p.ux + by * p.uy, ha = p.ux * ay - p.uy * ax, hb = p.ux * by - p.uy * bx;
        const double far = 1.000001 * d;
        if (fmax(ta, tb) + far < t || fmin(ta, tb) - far > nxt || fmin(ha, hb) > far || fmax(ha, hb) < -far) return;
        // the two end circles
        const double da = d * d - ha * ha, db = d * d - hb * hb;
        if (da >= 0.0) { const double s = sqrt(da); c0 = inset_cand(ta - s, T); c1 = inset_cand(ta + s, T); }
        if (db >= 0.0) { const double s = sqrt(db); c2 = inset_cand(tb - s, T); c3 = inset_cand(tb + s, T); }
        // the two side lines  p_j +- d n_j + tau u_j
        const double den = p.ux * ujy - p.uy * ujx;
        if (den != 0.0) {
            const double w1x = ax + d * njx, w1y = ay + d * njy, w2x = ax - d * njx, w2y = ay - d * njy;
            c4 = inset_cand((w1x * ujy - w1y * ujx) / den, T);
            c5 = inset_cand((w2x * ujy - w2y * ujx) / den, T);
        }
    } else {
        const double far = 2.000001 * d;
        if (!(inset_dist2(e, j, p.ox, p.oy) < far * far)) return;
        // the two end circles: equal radii, so the common chord bisects the line of centres
        for (int end = 0; end < 2; ++end) {
            const double cx = (end ? qjx : pjx) - p.ox, cy = (end ? qjy : pjy) - p.oy;
            const double D = sqrt(cx * cx + cy * cy), half = 0.5 * D, h2 = d * d - half * half;
            if (D > 0.0 && h2 >= 0.0) {
                const double ex = cx / D, ey = cy / D, h = sqrt(h2);
                const double s1 = inset_cand(inset_arc_param(p, half * ex - h * ey, half * ey + h * ex), T);
                const double s2 = inset_cand(inset_arc_param(p, half * ex + h * ey, half * ey - h * ex), T);
                if (end) { c2 = s1; c3 = s2; } else { c0 = s1; c1 = s2; }
            }
        }
        // the two side lines
        for (int side = 0; side < 2; ++side) {
            const double sg = side ? -d : d;
            const double wx = pjx + sg * njx - p.ox, wy = pjy + sg * njy - p.oy;
            const double h0 = ujx * wy - ujy * wx, disc = d * d - h0 * h0;
            if (disc >= 0.0) {
                const double tau0 = -(wx * ujx + wy * ujy), r = sqrt(disc);
                const double s1 = inset_cand(inset_arc_param(p, wx + (tau0 - r) * ujx, wy + (tau0 - r) * ujy), T);
                const double s2 = inset_cand(inset_arc_param(p, wx + (tau0 + r) * ujx, wy + (tau0 + r) * ujy), T);
                if (side) { c6 = s1; c7 = s2; } else { c4 = s1; c5 = s2; }
            }
        }
    }
    // sort the eight (a fixed network of compare-exchanges: no run-time indexing)
    FCPP_INSET_CE(c0, c1); FCPP_INSET_CE(c2, c3); FCPP_INSET_CE(c4, c5); FCPP_INSET_CE(c6, c7);
    FCPP_INSET_CE(c0, c2); FCPP_INSET_CE(c1, c3); FCPP_INSET_CE(c4, c6); FCPP_INSET_CE(c5, c7);
    FCPP_INSET_CE(c1, c2); FCPP_INSET_CE(c5, c6); FCPP_INSET_CE(c0, c4); FCPP_INSET_CE(c3, c7);
    FCPP_INSET_CE(c1, c5); FCPP_INSET_CE(c2, c6);
    FCPP_INSET_CE(c1, c4); FCPP_INSET_CE(c3, c6);
    FCPP_INSET_CE(c2, c4); FCPP_INSET_CE(c3, c5);
    FCPP_INSET_CE(c3, c4);
    const double b[10] = { 0.0, c0, c1, c2, c3, c4, c5, c6, c7, T };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 9; ++k) {
        const double lo = b[k], hi = b[k + 1];
        if (!(hi > lo) || !(hi > t) || !(lo < nxt)) continue;
        double x, y;
        inset_point(p, d, 0.5 * (lo + hi), x, y);
        if (!(inset_dist2(e, j, x, y) < ds2)) continue;
        if (lo <= t) t = hi;
        else nxt = lo;              // (lo < nxt was asked above)
    }
}

// The next surviving piece of primitive p at or beyond `from`: [t0, t1]; false when nothing survives there.
FCPP_HD bool inset_next_piece(const InsetEdges &e, const InsetPrim &p, double d, double from, double &t0, double &t1)
{
    const double ds = d * (1.0 - INSET_SLACK), ds2 = ds * ds, T = p.T;
    double t = from;
    for (;;) {
        if (!(t < T)) return false;
        const double told = t;
        double nxt = T;
        for (int j = 0; j < e.E; ++j) {
            if (j == p.skip0 || j == p.skip1) continue;
            inset_sweep_edge(e, p, d, ds2, j, t, nxt);
            if (!(t < T)) return false;
        }
        if (t == told) { t0 = t; t1 = nxt; return true; }
    }
}

FCPP_HD bool inset_piece_kept(const InsetPrim &p, double d, double t0, double t1) { return (p.arc ? d * (t1 - t0) : t1 - t0) >= INSET_MIN_PIECE; }

// the vertices a piece emits (0: an arc piece of INSET_MAX_ARC_VERTS points or more)
FCPP_HD int inset_piece_verts(const InsetPrim &p, double t0, double t1, double arc_step)
{
    if (!p.arc) return 1;
    const double q = ceil((t1 - t0) / arc_step);
    if (!(q < (double)INSET_MAX_ARC_VERTS)) return 0;
    return q < 1.0 ? 1 : (int)q;
}

// vertex k of the m a piece emits
FCPP_HD void inset_piece_vertex(const InsetPrim &p, double d, double t0, double t1, int m, int k, double &x, double &y)
{
    inset_point(p, d, k == 0 ? t0 : t0 + (double)k * ((t1 - t0) / (double)m), x, y);
}

// succ(k): the piece among P whose start is nearest to (ex, ey), ties to the lowest; d2 = that squared distance
FCPP_HD int inset_succ(const double *sx, const double *sy, int P, double ex, double ey, double &d2)
{
    int best = 0;
    d2 = INFINITY;
    for (int j = 0; j < P; ++j) {
        const double dx = sx[j] - ex, dy = sy[j] - ey, v = dx * dx + dy * dy;
        if (v < d2) { d2 = v; best = j; }
    }
    return best;
}

// The walk.  pos[k]: in, minus the vertex count of piece k; out, the offset of its first vertex within the field's output.  ring(r, off) is
// called at the start of ring r.  -> status; n_rings, n_verts.
template <class Ring>
FCPP_HD int inset_walk(int P, const uint16_t *succ, int32_t *pos, int32_t &n_rings, int32_t &n_verts, Ring ring)
{
    int32_t off = 0, R = 0;
    for (int first = 0; first < P; ++first) {
        if (pos[first] >= 0) continue;
        ring(R, off);
        ++R;
        int cur = first;
        do {
            const int32_t m = -pos[cur];
            pos[cur] = off;
            off += m;
            cur = succ[cur];
        } while (pos[cur] < 0);
        if (cur != first) return INSET_EUNSUPPORTED;
    }
    n_rings = R;
    n_verts = off;
    return INSET_OK;
}

struct InsetTotals {
    int32_t status, n_rings, n_verts;
    double gap;
};

// the host's working arrays of one field
struct InsetWork {
    std::vector<double> px, py, ux, uy, len, sx, sy, ex, ey, t0, t1;
    std::vector<uint16_t> nxt, succ;
    std::vector<int32_t> prim, pos;
};

// The rule on the host: one field (rings r0 .. r1 of vert_offsets) at one distance.  ring(r, off): ring r starts at vertex `off` of the
// field's output; vertex(at, x, y, src): vertex `at` of the field's output.  Both are called only for a field of status 0.
template <class Ring, class Vertex>
inline InsetTotals inset_field_host(const int64_t *vert_offsets, int64_t r0, int64_t r1, const double *x, const double *y, double d, double arc_step,
                                    InsetWork &w, Ring ring, Vertex vertex)
{
    const InsetTotals invalid = { INSET_EINVAL, 0, 0, 0.0 }, unsupported = { INSET_EUNSUPPORTED, 0, 0, 0.0 };
    if (r1 <= r0) return invalid;
    for (int64_t r = r0; r < r1; ++r)
        if (vert_offsets[r + 1] - vert_offsets[r] < 3) return invalid;
    const int64_t v0 = vert_offsets[r0], v1 = vert_offsets[r1];
    for (int64_t v = v0; v < v1; ++v)
        if (!inset_finite(x[v]) || !inset_finite(y[v])) return invalid;
    if (v1 - v0 > INSET_MAX_EDGES) return unsupported;
    const int E = (int)(v1 - v0);
    w.px.assign(x + v0, x + v1); w.py.assign(y + v0, y + v1);
    w.ux.resize((size_t)E); w.uy.resize((size_t)E); w.len.resize((size_t)E); w.nxt.resize((size_t)E);
    for (int64_t r = r0; r < r1; ++r) {
        const int base = (int)(vert_offsets[r] - v0), m = (int)(vert_offsets[r + 1] - vert_offsets[r]);
        inset_orient_ring(w.px.data() + base, w.py.data() + base, w.nxt.data() + base, base, m, r == r0);
    }
    for (int g = 0; g < E; ++g) {
        const int h = w.nxt[(size_t)g];
        inset_edge(w.px[(size_t)g], w.py[(size_t)g], w.px[(size_t)h], w.py[(size_t)h], w.ux[(size_t)g], w.uy[(size_t)g], w.len[(size_t)g]);
    }
    const InsetEdges e = { w.px.data(), w.py.data(), w.ux.data(), w.uy.data(), w.len.data(), w.nxt.data(), E };
    const size_t cap = (size_t)INSET_PIECES_PER_EDGE * (size_t)E;
    w.sx.clear(); w.sy.clear(); w.ex.clear(); w.ey.clear(); w.t0.clear(); w.t1.clear(); w.prim.clear(); w.pos.clear();
    for (int q = 0; q < 2 * E; ++q) {
        InsetPrim p;
        if (!inset_prim(e, q, d, p)) continue;
        double from = 0.0, t0, t1;
        while (inset_next_piece(e, p, d, from, t0, t1)) {
            from = t1;
            if (!inset_piece_kept(p, d, t0, t1)) continue;
            const int m = inset_piece_verts(p, t0, t1, arc_step);
            if (m == 0 || w.prim.size() == cap) return unsupported;
            double ax, ay, bx, by;
            inset_point(p, d, t0, ax, ay);
            inset_point(p, d, t1, bx, by);
            w.sx.push_back(ax); w.sy.push_back(ay); w.ex.push_back(bx); w.ey.push_back(by);
            w.t0.push_back(t0); w.t1.push_back(t1); w.prim.push_back(q); w.pos.push_back(-m);
        }
    }
    const int P = (int)w.prim.size();
    w.succ.resize((size_t)P);
    double gap2 = 0.0;
    for (int k = 0; k < P; ++k) {
        double d2;
        w.succ[(size_t)k] = (uint16_t)inset_succ(w.sx.data(), w.sy.data(), P, w.ex[(size_t)k], w.ey[(size_t)k], d2);
        gap2 = fmax(gap2, d2);
    }
    InsetTotals out = { INSET_OK, 0, 0, sqrt(gap2) };
    std::vector<int32_t> ring_at;
    out.status = inset_walk(P, w.succ.data(), w.pos.data(), out.n_rings, out.n_verts, [&](int32_t, int32_t off) { ring_at.push_back(off); });
    if (out.status != INSET_OK) return unsupported;
    for (size_t r = 0; r < ring_at.size(); ++r) ring((int32_t)r, ring_at[r]);
    for (int k = 0; k < P; ++k) {
        InsetPrim p;
        (void)inset_prim(e, w.prim[(size_t)k], d, p);
        const int m = inset_piece_verts(p, w.t0[(size_t)k], w.t1[(size_t)k], arc_step);
        for (int a = 0; a < m; ++a) {
            double vx, vy;
            inset_piece_vertex(p, d, w.t0[(size_t)k], w.t1[(size_t)k], m, a, vx, vy);
            vertex(w.pos[(size_t)k] + a, vx, vy, w.prim[(size_t)k]);
        }
    }
    return out;
}

}  // namespace fcpp
