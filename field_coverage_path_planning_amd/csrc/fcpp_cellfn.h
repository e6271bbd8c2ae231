// fcpp_cellfn.h -- the cells of ANY polygon field: a field (rings of either orientation, even-odd interior) split along a cut direction phi into
// cells that are ordinary one-ring fields, so that every cell can be given its own track angle.  Cuts leave reflex vertices along +-u of the
// frame of phi and end at the first boundary they meet (the vertical decomposition; with events = extrema only at the vertices where the
// boundary turns back across the cut direction: the boustrophedon decomposition, whose cells are monotone across the cuts).  ONE set of
// expressions for the host (fcpp_debug_cells, the tests' subject) and the device (fcpp_cells.hip), written like fcpp_insetfn.h in plain
// IEEE-754 double operations with fc_sincos and compiled with -ffp-contract=off on both sides, so that both give the same bits.
// Build-defined: the reference plans one quadrilateral at one angle.
//
// THE RULE (include/fcpp.h states it for callers).
//   frame     (s, c) = fc_sincos(phi); every vertex gets u = x c + y s and w = -x s + y c once (swath_uw).  Cuts are segments of constant w.
//   orient    depth of a ring = the number of the field's OTHER rings that contain its first vertex (the swath rule's half-open crossing
//             test on a ray along +u).  Even depth is driven counter-clockwise, odd depth clockwise, by the sign of the shoelace sum in x, y
//             about the ring's first vertex: the interior is on the left of every oriented edge.  Vertices keep their field-local input
//             index v; oriented edge g runs from vertex g to nxt[g].
//   rays      e1 = v - prv, e2 = nxt - v in (u, w).  v is reflex iff cross(e1, e2) < 0; with events = extrema it must also be extremal: the
//             first vertices backwards and forwards whose w differs from w_v lie on the same side of it.  A +u ray leaves a qualifying v
//             iff w_prv > w_v or w_nxt < w_v, a -u ray iff w_prv < w_v or w_nxt > w_v.
//   ray end   over the edges (a, b) not incident to v with w_a != w_b, in edge order: the edge meets the level at u_a if w_a = w_v, at u_b if
//             w_b = w_v (a VERTEX hit), at u_a + (w_v - w_a) / (w_b - w_a) (u_b - u_a) if (w_a < w_v) != (w_b < w_v) (an EDGE hit).  A ray
//             runs inside the field, so only an edge that has the interior towards it can end it: w_b > w_a for a +u ray, w_b < w_a for a
//             -u ray (of the two edges at a vertex an ulp off the level, whose hits round to the same u, this takes the one in front).  The
//             ray ends at the nearest hit strictly ahead; ties go to a vertex hit, then to the lowest edge.  An edge hit is a new node at
//             (u_hit, w_v), x = u c - w s, y = u s + w c; input vertices keep their input bits.  A ray that meets nothing: CELL_EUNSUPPORTED.
//   cuts      ray (v, dir), dir 0 = +u, 1 = -u, numbered 2 v + dir.  A ray that hits vertex t while ray (t, 1 - dir) hits v is dropped when
//             t < v: the cut of two facing vertices is kept once.  Kept rays are the cuts, new nodes are numbered E + j, both in ray order.
//   half-     every oriented edge is split at its new nodes, ordered along the edge by w (equal w: by node number), into boundary pieces:
//   edges     numbered by (edge, position).  Cut k adds half-edges B + 2 k (from v) and B + 2 k + 1 (back to v), B the number of pieces.
//             A node has one boundary piece and at most one cut leaving along +u and one along -u; a second one: CELL_EUNSUPPORTED.
//   succ      arriving at a node by half-edge h, leave by the outgoing half-edge met first when turning clockwise from the direction back
//             along h, never by h's twin: classes by the signs of cross and dot with the back direction, order within a class by the sign of
//             the cross product of the two.  A boundary piece has the direction of its whole edge, a cut (+-1, 0).
//   cells     from the lowest unused half-edge follow succ until it returns: one cell, its vertices the origins of its half-edges.  Reaching a
//             used half-edge other than the start: CELL_EUNSUPPORTED (touching or crossing rings).  src = the field-local INPUT edge of the
//             boundary piece that leaves the vertex, -1 for a cut; area = half the shoelace sum in x, y about the cell's first vertex, in
//             vertex order.  Cells with area <= min_area are not emitted: counted in `dropped`, their areas summed in cell order.
//   status    CELL_EINVAL: no ring, a ring with fewer than 3 vertices, a vertex that is not finite (or whose u or w is not), an edge of
//             length 0.  CELL_EUNSUPPORTED: more than CELL_MAX_EDGES edges, or one of the cases above.  EINVAL wins.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "fcpp_math.h"
#include "fcpp_swathfn.h"

namespace fcpp {

constexpr int CELL_MAX_EDGES = 1024;                     // FCPP_CELLS_MAX_EDGES of include/fcpp.h
constexpr int CELL_OK = 0, CELL_EINVAL = -1, CELL_EUNSUPPORTED = -3;         // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr int CELL_REFLEX = 0, CELL_EXTREMA = 1;
constexpr int CELL_NODES_PER_EDGE = 3, CELL_HALF_PER_EDGE = 7;      // E vertices + 2 E new nodes; 3 E boundary pieces + 2 x 2 E cut half-edges
constexpr uint16_t CELL_NONE = 0xffff;
constexpr int32_t CELL_NO_RAY = -1, CELL_NO_HIT = -2;

// a field's working arrays (the device keeps them in LDS); x, y: the field's input vertices
struct CellView {
    const double *x, *y;
    double *u, *w;                      // E: the frame
    uint16_t *nxt, *prv;                // E: the oriented ring
    int32_t *ray;                       // 2 E: CELL_NO_RAY, CELL_NO_HIT, the vertex hit (< E), or E + the edge hit
    uint16_t *org, *succ, *pos;         // 7 E per half-edge: origin node, successor, position within its cell (CELL_NONE: unused)
    uint16_t *bout, *cutp, *cutm;       // 3 E per node: the boundary piece and the cuts along +u / -u that leave it
    uint16_t *nray;                     // 2 E per new node: its ray
    uint16_t *ebase;                    // E + 1: the first piece of every edge
    uint16_t *cfirst, *clen, *cout, *cvoff;     // 2 E + 1 per cell: first half-edge, vertices, emitted index (CELL_NONE: dropped), vertex offset
    double *area;                       // 2 E + 1 per cell
    int E;
    double c, s;
};

struct CellCounts {
    int32_t J, K, B, H;                 // new nodes, cuts, boundary pieces, half-edges
};

struct CellTotals {
    int32_t status, n_cells, n_verts, n_cuts, dropped;
    double dropped_area;
};

// has the ring of m vertices at vx, vy an edge of length 0
FCPP_HD bool cell_ring_zero_edge(const double *vx, const double *vy, int64_t m)
{
    bool zero = false;
    for (int64_t t = 0; t < m; ++t) {
        const int64_t n = t + 1 == m ? 0 : t + 1;
        zero |= vx[t] == vx[n] && vy[t] == vy[n];
    }
    return zero;
}

// ring r of the field (rings r0 .. r1 of vert_offsets; u, w set): -> nxt, prv of its vertices
FCPP_HD void cell_orient_ring(const CellView &f, const int64_t *vert_offsets, int64_t r0, int64_t r1, int64_t r)
{
    const int64_t v0 = vert_offsets[r0];
    const int base = (int)(vert_offsets[r] - v0), m = (int)(vert_offsets[r + 1] - vert_offsets[r]);
    const double *vx = f.x + base, *vy = f.y + base;
    const double x0 = vx[0], y0 = vy[0];
    double a = 0.0;
    for (int t = 1; t + 1 < m; ++t) a += (vx[t] - x0) * (vy[t + 1] - y0) - (vx[t + 1] - x0) * (vy[t] - y0);
    const double u0 = f.u[base], w0 = f.w[base];
    int depth = 0;
    for (int64_t q = r0; q < r1; ++q) {
        if (q == r) continue;
        const int b2 = (int)(vert_offsets[q] - v0), m2 = (int)(vert_offsets[q + 1] - vert_offsets[q]);
        int in = 0;
        for (int e = 0; e < m2; ++e) {
            const int p = b2 + e, n = b2 + (e + 1 == m2 ? 0 : e + 1);
            if (swath_crosses(f.w[p], f.w[n], w0) && swath_cross_u(f.u[p], f.w[p], f.u[n], f.w[n], w0) > u0) in ^= 1;
        }
        depth += in;
    }
    const bool rev = (depth & 1) ? a > 0.0 : a < 0.0;
    for (int t = 0; t < m; ++t) {
        const int fwd = base + (t + 1 == m ? 0 : t + 1), bwd = base + (t == 0 ? m - 1 : t - 1);
        f.nxt[base + t] = (uint16_t)(rev ? bwd : fwd);
        f.prv[base + t] = (uint16_t)(rev ? fwd : bwd);
    }
}

// where edge g (w_a != w_b, the level strictly between) meets the level wv
FCPP_HD double cell_hit_u(const CellView &f, int g, double wv)
{
    const int b = f.nxt[g];
    return f.u[g] + (wv - f.w[g]) / (f.w[b] - f.w[g]) * (f.u[b] - f.u[g]);
}

// the two rays of vertex v -> ray[2 v], ray[2 v + 1]
FCPP_HD void cell_rays(const CellView &f, int v, int events)
{
    const int E = f.E, p = f.prv[v], n = f.nxt[v];
    const double uv = f.u[v], wv = f.w[v], wp = f.w[p], wn = f.w[n];
    const double e1u = uv - f.u[p], e1w = wv - wp, e2u = f.u[n] - uv, e2w = wn - wv;
    bool q = e1u * e2w - e1w * e2u < 0.0;
    if (q && events == CELL_EXTREMA) {
        int P = v, N = v;
        for (int i = 0, k = p; i < E && k != v; ++i, k = f.prv[k])
            if (f.w[k] != wv) { P = k; break; }
        for (int i = 0, k = n; i < E && k != v; ++i, k = f.nxt[k])
            if (f.w[k] != wv) { N = k; break; }
        q = P != v && N != v && (f.w[P] < wv) == (f.w[N] < wv);
    }
    const bool plus = q && (wp > wv || wn < wv), minus = q && (wp < wv || wn > wv);
    int32_t tp = plus ? CELL_NO_HIT : CELL_NO_RAY, tm = minus ? CELL_NO_HIT : CELL_NO_RAY;
    if (plus || minus) {
        double bp = INFINITY, bm = -INFINITY;
        for (int g = 0; g < E; ++g) {
            if (g == v || g == p) continue;
            const int b = f.nxt[g];
            const double wa = f.w[g], wb = f.w[b];
            if (wa == wb) continue;
            double hu;
            int32_t t;
            if (wa == wv) { hu = f.u[g]; t = g; }
            else if (wb == wv) { hu = f.u[b]; t = b; }
            else if ((wa < wv) != (wb < wv)) { hu = cell_hit_u(f, g, wv); t = E + g; }
            else continue;
            if (plus && wb > wa && hu > uv && (hu < bp || (hu == bp && t < E && tp >= E))) { bp = hu; tp = t; }
            if (minus && wb < wa && hu < uv && (hu > bm || (hu == bm && t < E && tm >= E))) { bm = hu; tm = t; }
        }
    }
    f.ray[2 * v] = tp;
    f.ray[2 * v + 1] = tm;
}

// is ray q a cut (not the second of two facing vertices' rays)
FCPP_HD bool cell_ray_kept(const CellView &f, int q)
{
    const int32_t t = f.ray[q];
    if (t < 0) return false;
    const int v = q >> 1, dir = q & 1;
    return !(t < f.E && t < v && f.ray[2 * t + (1 - dir)] == v);
}

// the edge whose piece leaves node X
FCPP_HD int cell_node_edge(const CellView &f, int X) { return X < f.E ? X : f.ray[f.nray[X - f.E]] - f.E; }
// the level of new node j
FCPP_HD double cell_node_w(const CellView &f, int j) { return f.w[f.nray[j] >> 1]; }

// Numbering, by ONE thread: the pieces of every edge, the new nodes and the cuts with their four table entries; cutp, cutm hold CELL_NONE
// on entry.  -> CELL_OK, or CELL_EUNSUPPORTED: a ray without a hit, a node with two cuts along one direction.
FCPP_HD int cell_number(const CellView &f, CellCounts &n)
{
    const int E = f.E;
    int st = CELL_OK;
    for (int g = 0; g <= E; ++g) f.ebase[g] = 0;
    for (int q = 0; q < 2 * E; ++q) {
        if (f.ray[q] == CELL_NO_HIT) st = CELL_EUNSUPPORTED;
        if (f.ray[q] >= E) ++f.ebase[f.ray[q] - E + 1];
    }
    if (st != CELL_OK) return st;
    int at = 0;
    for (int g = 0; g < E; ++g) {           // ebase[g + 1] = new nodes of edge g  ->  ebase[g] = its first piece
        const int cnt = f.ebase[g + 1];
        f.ebase[g] = (uint16_t)at;
        at += 1 + cnt;
    }
    f.ebase[E] = (uint16_t)at;
    const int B = at;
    int J = 0, K = 0;
    for (int q = 0; q < 2 * E; ++q) {
        if (!cell_ray_kept(f, q)) continue;
        const int v = q >> 1, dir = q & 1, t = f.ray[q];
        int X = t;
        if (t >= E) { f.nray[J] = (uint16_t)q; X = E + J; ++J; }
        const int h0 = B + 2 * K, h1 = h0 + 1;
        f.org[h0] = (uint16_t)v;
        f.org[h1] = (uint16_t)X;
        uint16_t &a = dir == 0 ? f.cutp[v] : f.cutm[v], &b = dir == 0 ? f.cutm[X] : f.cutp[X];
        if (a != CELL_NONE || b != CELL_NONE) st = CELL_EUNSUPPORTED;
        a = (uint16_t)h0;
        b = (uint16_t)h1;
        ++K;
    }
    n.J = J; n.K = K; n.B = B; n.H = B + 2 * K;
    return st;
}

// the boundary piece that leaves node X (vertices: X < E; new nodes: by their rank along the edge) -> bout, org
FCPP_HD void cell_place_node(const CellView &f, int J, int X)
{
    const int E = f.E;
    int piece;
    if (X < E) piece = f.ebase[X];
    else {
        const int j = X - E, g = cell_node_edge(f, X);
        const double wj = cell_node_w(f, j);
        const bool up = f.w[f.nxt[g]] > f.w[g];
        int rank = 0;
        for (int k = 0; k < J; ++k) {
            if (k == j || cell_node_edge(f, E + k) != g) continue;
            const double wk = cell_node_w(f, k);
            if ((up ? wk < wj : wk > wj) || (wk == wj && k < j)) ++rank;
        }
        piece = f.ebase[g] + 1 + rank;
    }
    f.bout[X] = (uint16_t)piece;
    f.org[piece] = (uint16_t)X;
}

// the class of direction d turning clockwise from r: 0 within (0, pi), 1 at pi, 2 within (pi, 2 pi), 3 at 2 pi
FCPP_HD int cell_turn_class(double ru, double rw, double du, double dw)
{
    const double cr = ru * dw - rw * du;
    if (cr < 0.0) return 0;
    if (cr > 0.0) return 2;
    return ru * du + rw * dw < 0.0 ? 1 : 3;
}

// is direction a met before direction b when turning clockwise from r
FCPP_HD bool cell_before(double ru, double rw, double au, double aw, double bu, double bw)
{
    const int ca = cell_turn_class(ru, rw, au, aw), cb = cell_turn_class(ru, rw, bu, bw);
    if (ca != cb) return ca < cb;
    return au * bw - aw * bu < 0.0;
}

FCPP_HD void cell_edge_dir(const CellView &f, int g, double &du, double &dw)
{
    const int b = f.nxt[g];
    du = f.u[b] - f.u[g];
    dw = f.w[b] - f.w[g];
}

// succ(h)
FCPP_HD int cell_succ(const CellView &f, const CellCounts &n, int h)
{
    int X, twin = -1;
    double ru, rw;
    if (h < n.B) {
        const int g = cell_node_edge(f, f.org[h]);
        X = h + 1 < f.ebase[g + 1] ? f.org[h + 1] : f.nxt[g];
        cell_edge_dir(f, g, ru, rw);
        ru = -ru; rw = -rw;
    } else {
        twin = n.B + ((h - n.B) ^ 1);
        X = f.org[twin];
        ru = f.cutp[f.org[h]] == h ? -1.0 : 1.0;
        rw = 0.0;
    }
    int best = f.bout[X];
    double bu, bw;
    cell_edge_dir(f, cell_node_edge(f, X), bu, bw);
    const int cp = f.cutp[X], cm = f.cutm[X];
    if (cp != CELL_NONE && cp != twin && cell_before(ru, rw, 1.0, 0.0, bu, bw)) { best = cp; bu = 1.0; bw = 0.0; }
    if (cm != CELL_NONE && cm != twin && cell_before(ru, rw, -1.0, 0.0, bu, bw)) { best = cm; bu = -1.0; bw = 0.0; }
    return best;
}

// The walk, by ONE thread; pos holds CELL_NONE on entry.  -> status; C cells with cfirst, clen; pos = the position of a half-edge in its cell
FCPP_HD int cell_walk(const CellView &f, int H, int &C)
{
    int c = 0;
    for (int first = 0; first < H; ++first) {
        if (f.pos[first] != CELL_NONE) continue;
        int cur = first, m = 0;
        do {
            f.pos[cur] = (uint16_t)m++;
            cur = f.succ[cur];
        } while (f.pos[cur] == CELL_NONE);
        if (cur != first || c == 2 * f.E + 1) return CELL_EUNSUPPORTED;         // (1 + cuts - holes cells at most: the tables' size)
        f.cfirst[c] = (uint16_t)first;
        f.clen[c] = (uint16_t)m;
        ++c;
    }
    C = c;
    return CELL_OK;
}

FCPP_HD void cell_node_xy(const CellView &f, int X, double &x, double &y)
{
    if (X < f.E) { x = f.x[X]; y = f.y[X]; return; }
    const int q = f.nray[X - f.E];
    const double wv = f.w[q >> 1];
    swath_point(cell_hit_u(f, f.ray[q] - f.E, wv), wv, f.c, f.s, x, y);
}

// the input edge of oriented edge g: g itself in a ring driven in input order, else the edge that ends at g
FCPP_HD int cell_input_edge(const CellView &f, int g) { return f.nxt[g] == g + 1 || f.prv[g] + 1 == g ? g : f.nxt[g]; }

FCPP_HD int cell_vertex_src(const CellView &f, const CellCounts &n, int h) { return h < n.B ? cell_input_edge(f, cell_node_edge(f, f.org[h])) : -1; }

// the area of cell c
FCPP_HD double cell_area(const CellView &f, int c)
{
    int h = f.cfirst[c];
    const int m = f.clen[c];
    double x0, y0, px, py, a = 0.0;
    cell_node_xy(f, f.org[h], x0, y0);
    h = f.succ[h];
    cell_node_xy(f, f.org[h], px, py);
    for (int t = 2; t < m; ++t) {
        double qx, qy;
        h = f.succ[h];
        cell_node_xy(f, f.org[h], qx, qy);
        a += (px - x0) * (qy - y0) - (qx - x0) * (py - y0);
        px = qx; py = qy;
    }
    return 0.5 * a;
}

// The totals, by ONE thread (area set): cout, cvoff of every cell
FCPP_HD void cell_totals(const CellView &f, int C, double min_area, CellTotals &t)
{
    t.n_cells = t.n_verts = t.dropped = 0;
    t.dropped_area = 0.0;
    for (int c = 0; c < C; ++c) {
        f.cvoff[c] = (uint16_t)t.n_verts;
        if (f.area[c] <= min_area) {
            f.cout[c] = CELL_NONE;
            ++t.dropped;
            t.dropped_area += f.area[c];
        } else {
            f.cout[c] = (uint16_t)t.n_cells++;
            t.n_verts += f.clen[c];
        }
    }
}

// the host's working arrays of one field: every table a vector of its exact size
struct CellWork {
    std::vector<double> u, w, area;
    std::vector<int32_t> ray;
    std::vector<uint16_t> nxt, prv, org, succ, pos, bout, cutp, cutm, nray, ebase, cfirst, clen, cout, cvoff;
    CellView view(const double *x, const double *y, int E, double c, double s)
    {
        const size_t e = (size_t)E, cells = 2 * e + 1, half = (size_t)CELL_HALF_PER_EDGE * e, nodes = (size_t)CELL_NODES_PER_EDGE * e;
        u.assign(e, 0.0); w.assign(e, 0.0); area.assign(cells, 0.0);
        ray.assign(2 * e, CELL_NO_RAY);
        nxt.assign(e, 0); prv.assign(e, 0);
        org.assign(half, 0); succ.assign(half, 0); pos.assign(half, CELL_NONE);
        bout.assign(nodes, 0); cutp.assign(nodes, CELL_NONE); cutm.assign(nodes, CELL_NONE);
        nray.assign(2 * e, 0); ebase.assign(e + 1, 0);
        cfirst.assign(cells, 0); clen.assign(cells, 0); cout.assign(cells, CELL_NONE); cvoff.assign(cells, 0);
        CellView f;
        f.x = x; f.y = y; f.u = u.data(); f.w = w.data(); f.ray = ray.data(); f.area = area.data();
        f.nxt = nxt.data(); f.prv = prv.data(); f.org = org.data(); f.succ = succ.data(); f.pos = pos.data();
        f.bout = bout.data(); f.cutp = cutp.data(); f.cutm = cutm.data(); f.nray = nray.data(); f.ebase = ebase.data();
        f.cfirst = cfirst.data(); f.clen = clen.data(); f.cout = cout.data(); f.cvoff = cvoff.data();
        f.E = E; f.c = c; f.s = s;
        return f;
    }
};

// The rule on the host: one field (rings r0 .. r1 of vert_offsets).  cell(k, off, area): emitted cell k of the field starts at vertex `off` of
// the field's output; vertex(at, x, y, src): vertex `at` of the field's output.  Both are called only for a field of status 0.
template <class Cell, class Vertex>
inline CellTotals cell_field_host(const int64_t *vert_offsets, int64_t r0, int64_t r1, const double *x, const double *y, double phi, int events,
                                  double min_area, CellWork &work, Cell cell, Vertex vertex)
{
    const CellTotals invalid = { CELL_EINVAL, 0, 0, 0, 0, 0.0 }, unsupported = { CELL_EUNSUPPORTED, 0, 0, 0, 0, 0.0 };
    if (r1 <= r0) return invalid;
    for (int64_t r = r0; r < r1; ++r)
        if (vert_offsets[r + 1] - vert_offsets[r] < 3) return invalid;
    double s, c;
    fc_sincos(phi, s, c);
    const int64_t v0 = vert_offsets[r0], v1 = vert_offsets[r1];
    for (int64_t v = v0; v < v1; ++v) {
        double u, w;
        swath_uw(x[v], y[v], c, s, u, w);
        if (!swath_finite(x[v]) || !swath_finite(y[v]) || !swath_finite(u) || !swath_finite(w)) return invalid;
    }
    for (int64_t r = r0; r < r1; ++r)
        if (cell_ring_zero_edge(x + vert_offsets[r], y + vert_offsets[r], vert_offsets[r + 1] - vert_offsets[r])) return invalid;
    if (v1 - v0 > CELL_MAX_EDGES) return unsupported;
    const int E = (int)(v1 - v0);
    const CellView f = work.view(x + v0, y + v0, E, c, s);
    for (int v = 0; v < E; ++v) swath_uw(f.x[v], f.y[v], c, s, f.u[v], f.w[v]);
    for (int64_t r = r0; r < r1; ++r) cell_orient_ring(f, vert_offsets, r0, r1, r);
    for (int v = 0; v < E; ++v) cell_rays(f, v, events);
    CellCounts n;
    if (cell_number(f, n) != CELL_OK) return unsupported;
    for (int X = 0; X < E + n.J; ++X) cell_place_node(f, n.J, X);
    for (int h = 0; h < n.H; ++h) f.succ[h] = (uint16_t)cell_succ(f, n, h);
    int C = 0;
    if (cell_walk(f, n.H, C) != CELL_OK) return unsupported;
    for (int k = 0; k < C; ++k) f.area[k] = cell_area(f, k);
    CellTotals t = { CELL_OK, 0, 0, n.K, 0, 0.0 };
    cell_totals(f, C, min_area, t);
    for (int k = 0; k < C; ++k) {
        if (f.cout[k] == CELL_NONE) continue;
        cell(f.cout[k], f.cvoff[k], f.area[k]);
        int h = f.cfirst[k];
        for (int a = 0; a < f.clen[k]; ++a, h = f.succ[h]) {
            double vx, vy;
            cell_node_xy(f, f.org[h], vx, vy);
            vertex(f.cvoff[k] + a, vx, vy, cell_vertex_src(f, n, h));
        }
    }
    return t;
}

}  // namespace fcpp
