// fcpp_tourfn.h -- the cell tour: in which ORDER to drive the cells of one field (field_cells' cells) and which of its candidate routes, in
// which direction, every cell takes, with the joints between cells priced by the Dubins or Reeds-Shepp connectors.  A generalised
// travelling-salesman problem: the order is a local search like the swath router's (fcpp_routefn.h), the node choice for a given order is
// exact, a layered shortest path like the mission's (fcpp_missionfn.h).  ONE set of expressions for the host (fcpp_debug_cell_tour, the
// tests' checker) and the device (fcpp_tour.hip), in plain IEEE-754 double operations compiled with -ffp-contract=off on both sides, so
// that both give the same bits.  Build-defined: the reference knows no cells.
//
// THE RULE (include/fcpp.h states it for callers).
//   cells     field f owns the cells coff[f] .. coff[f + 1], m of them; cell c owns the variants voff[c] .. voff[c + 1], V_c of them.  A variant
//             has an in-pose (ix, iy, ih), an out-pose (ox, oy, oh) and an inner cost w, the caller's price of driving it.
//   nodes     cell c has N_c = 2 V_c nodes u = 2 v + d: d = 0 the variant as given, d = 1 the same drive backwards -- in-pose (ox, oy,
//             fl(oh + pi)), out-pose (ix, iy, fl(ih + pi)) -- at the same w.  A field's nodes are numbered cell by cell, N_f of them.
//   transit   D, N_f x N_f row-major: D[a][b] = the shortest connector length from out(a) to in(b) at radius R, mode 0 Dubins, 1 Reeds-
//             Shepp; +inf where a and b belong to one cell.  Every entry is evaluated on its own pair (no mirrored pairs: in and out
//             poses of a variant are unrelated).
//   sums      plus(a, b) = fl(a + b) if that is below +inf, else +inf (NaN included): no layer value is ever NaN.
//   cost      of an order c_1 .. c_k of the KEPT cells (V_c > 0): g_1[b] = plus(E[b], w(b)); g_j[b] = plus(min over a in c_(j-1) of
//             plus(g_(j-1)[a], D[a][b]), w(b)), the minimiser the lowest a that attains the minimum (a ascending, strict "less than");
//             cost = min over b in c_k of plus(g_k[b], X[b]), the lowest b.  E, X (N_f each, NULL = zeros): from the field's entry pose to
//             in(b), from out(b) to the field's exit pose.  The backtrack gives one node per kept cell; joint_length = the chosen D
//             entries, with E and X where given, added in driving order from 0.  k = 0: cost 0, no joints.
//   candidate c = 0 .. S - 1 (1 <= S <= 64): c = 0 the stored order of the kept cells; c = 1 that order reversed; c >= 2 nearest neighbour
//             from the kept cell floor((c - 2) k / (S - 2)): repeatedly the unvisited kept cell j with the least C[cur][j], ties to the
//             lowest j; C[i][j] = min over a in i, b in j of D[a][b] (an entry not below +inf counts as +inf).
//   sweeps    a sweep evaluates EVERY move below on the current order -- by the cost of the moved order, the full rule above -- takes the
//             one with the least cost, ties to the lowest code, and applies it iff cost < fl(current cost - min_gain); otherwise the
//             candidate is finished; it also stops after max_sweeps sweeps.
//     move A  reverse(i, j), 0 <= i < j < k, code i k + j: the order of positions i .. j reversed (a cell's direction is the node choice's).
//     move B  or-opt, needs k > l: the segment of l in {1, 2, 3} cells at position i moved to between positions p and p + 1, p in
//             [-1, k - 1] with p < i - 1 or p >= i + l; r = 0 as it is, r = 1 (l >= 2 only) reversed.
//             code k k + (((l - 1) 2 + r) k + i) (k + 1) + (p + 1).
//   result    the winner: the candidate with the least final cost, ties to the lowest c.  sweeps: the most moves any candidate applied.
//             stored: the stored order with node stored_node[c] of every kept cell (NULL: node 0), chained as the rule chains:
//             s = plus(E, w), s = plus(plus(s, D), w) per cell, plus(s, X); cost <= stored by the monotonicity of rounded addition.
//             order: the winner's cells in driving order, the skipped cells (V_c = 0) behind them in stored order; node: the chosen
//             local node of every cell in cell order, -1 for a skipped cell.
//   status    TOUR_EUNSUPPORTED for m > TOUR_MAX_CELLS, a cell of more than TOUR_MAX_CELL_NODES nodes or N_f > TOUR_MAX_NODES: the field
//             has no block in D, its order is the stored one (every cell), every node -1, the costs NaN.  TOUR_EINVAL when `stored` is
//             not finite (a stored_node outside its cell makes it NaN): nothing is improved, the order is the stored one, the nodes the
//             stored ones (0 for one outside its cell), cost = stored, joint_length NaN.
// The minimum over (cost, code) pairs does not depend on the order in which the moves are looked at, and every cost is the one
// expression chain above, a ascending: the device may hand the codes to its wavefronts in any way.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_connfn.h"

namespace fcpp {

constexpr int TOUR_MAX_CELLS = 32;                       // FCPP_TOUR_MAX_CELLS of include/fcpp.h
constexpr int TOUR_MAX_CELL_NODES = 64;                  // FCPP_TOUR_MAX_CELL_NODES: a lane per target node
constexpr int TOUR_MAX_NODES = 1024;                     // FCPP_TOUR_MAX_NODES: a block of at most 8 MiB
constexpr int TOUR_MAX_STARTS = 64;
constexpr int TOUR_MAX_SWEEPS = 1 << 20;
constexpr int TOUR_OK = 0, TOUR_EINVAL = -1, TOUR_EUNSUPPORTED = -3;         // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// does the field of the cells c0 .. c1 fit the caps?  (voff: the variant offsets of ALL cells)
FCPP_HD bool tour_supported(const int64_t *voff, int64_t c0, int64_t c1)
{
    if (c1 - c0 > TOUR_MAX_CELLS || 2 * (voff[c1] - voff[c0]) > TOUR_MAX_NODES) return false;
    for (int64_t c = c0; c < c1; ++c)
        if (2 * (voff[c + 1] - voff[c]) > TOUR_MAX_CELL_NODES) return false;
    return true;
}

// the size of the field's block of D: N_f^2, none beyond a cap
FCPP_HD int64_t tour_block(const int64_t *voff, int64_t c0, int64_t c1)
{
    const int64_t Nf = 2 * (voff[c1] - voff[c0]);
    return tour_supported(voff, c0, c1) ? Nf * Nf : 0;
}

// the cell of the field (c0 .. c1, not empty) that owns its local node u: the last one whose nodes start at or before u
FCPP_HD int64_t tour_cell_of(const int64_t *voff, int64_t c0, int64_t c1, int64_t u)
{
    const int64_t v0 = voff[c0];
    int64_t lo = c0, hi = c1;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (2 * (voff[mid] - v0) <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- transit ----------------------------------------------------------------------------------------------------------------------
// the pose at which direction d of variant v is left (exit) or entered; the flipped heading as route_pose forms it
FCPP_HD void tour_pose(const double *ix, const double *iy, const double *ih, const double *ox, const double *oy, const double *oh, int64_t v, int d,
                       bool exit, double &x, double &y, double &h)
{
    const bool at_out = (d == 0) == exit;                // d = 0 enters at the in-pose and leaves at the out-pose, d = 1 the other way
    x = at_out ? ox[v] : ix[v];
    y = at_out ? oy[v] : iy[v];
    const double h0 = at_out ? oh[v] : ih[v];
    h = d ? h0 + kPi : h0;
}

// the connector length from out(variant va, direction da) to in(vb, db); MODE 0 Dubins, 1 Reeds-Shepp
template <int MODE>
FCPP_HD double tour_transit(const double *ix, const double *iy, const double *ih, const double *ox, const double *oy, const double *oh, double R,
                            int64_t va, int da, int64_t vb, int db)
{
    double x0, y0, h0, x1, y1, h1, total;
    tour_pose(ix, iy, ih, ox, oy, oh, va, da, true, x0, y0, h0);
    tour_pose(ix, iy, ih, ox, oy, oh, vb, db, false, x1, y1, h1);
    int word;
    double seg[Conn<MODE>::NSEG];
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, R, word, seg, total);
    return total;
}

// ---- the layers -------------------------------------------------------------------------------------------------------------------
// a field: its block, its E, X (N_f each or NULL), its variants' w and the first local node of each of its m cells (m + 1 values)
struct TourField { const double *D, *E, *X, *w; const int *noff; int Nf; };

FCPP_HD bool tour_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }          // false for NaN
FCPP_HD double tour_plus(double a, double b) { const double s = a + b; return s < INFINITY ? s : INFINITY; }
FCPP_HD double tour_key(double v) { return v < INFINITY ? v : INFINITY; }
FCPP_HD double tour_first(const TourField &F, int b) { return tour_plus(F.E ? F.E[b] : 0.0, F.w[b >> 1]); }
FCPP_HD double tour_step(const TourField &F, double g, int a, int b) { return tour_plus(g, F.D[a * F.Nf + b]); }
FCPP_HD double tour_close(const TourField &F, double best, int b) { return tour_plus(best, F.w[b >> 1]); }
FCPP_HD double tour_last(const TourField &F, double g, int b) { return tour_plus(g, F.X ? F.X[b] : 0.0); }

// ---- moves ------------------------------------------------------------------------------------------------------------------------
struct TourMove { int kind, i, j, l, r, p; };          // kind -1: none; 0: A (i, j); 1: B (i, l, r, p)

FCPP_HD int tour_n_codes(int k) { return k * k + 6 * k * (k + 1); }          // 7360 at the cap

// the move of a code in [0, tour_n_codes(k)); false for a code that names no move
FCPP_HD bool tour_decode(int k, int code, TourMove &mv)
{
    if (code < k * k) {
        mv.kind = 0; mv.i = code / k; mv.j = code - mv.i * k; mv.l = 0; mv.r = 0; mv.p = 0;
        return mv.i < mv.j;
    }
    int c = code - k * k;
    const int pp = c % (k + 1);
    c /= k + 1;
    mv.kind = 1; mv.i = c % k; mv.j = 0;
    c /= k;
    mv.r = c & 1; mv.l = (c >> 1) + 1; mv.p = pp - 1;
    return k > mv.l && mv.i + mv.l <= k && (mv.r == 0 || mv.l >= 2) && (mv.p < mv.i - 1 || mv.p >= mv.i + mv.l);
}

// position q of the order AFTER the move, read from the order before it
FCPP_HD int tour_moved(const uint8_t *t, const TourMove &mv, int q)
{
    if (mv.kind < 0) return t[q];
    if (mv.kind == 0) return (q < mv.i || q > mv.j) ? t[q] : t[mv.i + mv.j - q];
    const int i = mv.i, l = mv.l, at = mv.p < i ? mv.p + 1 : mv.p + 1 - l;          // where the segment starts afterwards
    if (q >= at && q < at + l) return mv.r ? t[i + l - 1 - (q - at)] : t[i + (q - at)];
    const int o = q < at ? q : q - l;                                              // q's rank among the others
    return t[o < i ? o : o + l];
}

// is (v, code) better than (bv, bc)?  (v is never NaN)
FCPP_HD bool tour_better(double v, int code, double bv, int bc) { return v < bv || (v == bv && code < bc); }

FCPP_HD int tour_nn_start(int c, int S, int k) { return (int)((int64_t)(c - 2) * k / (S - 2)); }

// the stored cost: the kept cells in stored order, node sn[j] of kept cell j (a node outside its cell: NaN)
FCPP_HD double tour_stored(const TourField &F, const uint8_t *kept, int k, const int32_t *sn)
{
    double s = 0.0;
    int prev = 0;
    for (int j = 0; j < k; ++j) {
        const int cell = kept[j], n0 = F.noff[cell], nc = F.noff[cell + 1] - n0, u = sn ? sn[cell] : 0;
        if (u < 0 || u >= nc) return __builtin_nan("");
        const int b = n0 + u;
        s = j == 0 ? tour_first(F, b) : tour_close(F, tour_step(F, s, prev, b), b);
        prev = b;
    }
    return k > 0 ? tour_last(F, s, prev) : 0.0;
}

// the joints of nodes nd[cell] (local to the cell) in the order t, added in driving order from 0
FCPP_HD double tour_joints(const TourField &F, const uint8_t *t, int k, const int32_t *nd)
{
    double s = 0.0;
    int prev = 0;
    for (int j = 0; j < k; ++j) {
        const int b = F.noff[t[j]] + nd[t[j]];
        if (j == 0) { if (F.E) s += F.E[b]; }
        else s += F.D[prev * F.Nf + b];
        prev = b;
    }
    if (k > 0 && F.X) s += F.X[prev];
    return s;
}

// ---- the host twin: one field -----------------------------------------------------------------------------------------------------------
// the cost of the order t AFTER the move mv (kind -1: as it is); pred (N_f, or NULL): the minimiser of every node of positions 1 .. k - 1,
// local to the cell before; last: the node of the last cell that attains the cost, local to the field
inline double tour_eval_host(const TourField &F, const uint8_t *t, int k, const TourMove &mv, int16_t *pred, int *last)
{
    if (last) *last = -1;
    if (k <= 0) return 0.0;
    double g[TOUR_MAX_CELL_NODES], ng[TOUR_MAX_CELL_NODES];
    int nprev = 0, n0prev = 0;
    for (int j = 0; j < k; ++j) {
        const int cell = tour_moved(t, mv, j), n0 = F.noff[cell], nc = F.noff[cell + 1] - n0;
        for (int b = 0; b < nc; ++b) {
            if (j == 0) { ng[b] = tour_first(F, n0 + b); continue; }
            double best = tour_step(F, g[0], n0prev, n0 + b);
            int arg = 0;
            for (int a = 1; a < nprev; ++a) {
                const double v = tour_step(F, g[a], n0prev + a, n0 + b);
                if (v < best) { best = v; arg = a; }
            }
            ng[b] = tour_close(F, best, n0 + b);
            if (pred) pred[n0 + b] = (int16_t)arg;
        }
        for (int b = 0; b < nc; ++b) g[b] = ng[b];
        nprev = nc; n0prev = n0;
    }
    double best = tour_last(F, g[0], n0prev);
    int arg = 0;
    for (int b = 1; b < nprev; ++b) {
        const double v = tour_last(F, g[b], n0prev + b);
        if (v < best) { best = v; arg = b; }
    }
    if (last) *last = n0prev + arg;
    return best;
}

// C[i * TOUR_MAX_CELLS + j] over the field's m cells (+inf for i = j and for a cell without nodes)
inline void tour_cell_matrix_host(const TourField &F, int m, double *C)
{
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            double mn = INFINITY;
            if (i != j)
                for (int a = F.noff[i]; a < F.noff[i + 1]; ++a)
                    for (int b = F.noff[j]; b < F.noff[j + 1]; ++b) {
                        const double v = tour_key(F.D[a * F.Nf + b]);
                        if (v < mn) mn = v;
                    }
            C[i * TOUR_MAX_CELLS + j] = mn;
        }
}

// the nearest-neighbour order from kept cell `start` (an index into kept)
FCPP_HD void tour_nn(const double *C, const uint8_t *kept, int k, int start, uint8_t *t)
{
    uint32_t seen = 0;
    int cur = kept[start];
    t[0] = (uint8_t)cur; seen |= 1u << cur;
    for (int q = 1; q < k; ++q) {
        double bv = INFINITY;
        int bj = INT32_MAX;
        for (int o = 0; o < k; ++o) {
            const int j = kept[o];
            if (seen >> j & 1u) continue;
            const double v = C[cur * TOUR_MAX_CELLS + j];
            if (tour_better(v, j, bv, bj)) { bv = v; bj = j; }
        }
        cur = bj;
        t[q] = (uint8_t)cur; seen |= 1u << cur;
    }
}

// candidate c of S as constructed (k > 0)
FCPP_HD void tour_construct(const double *C, const uint8_t *kept, int k, int c, int S, uint8_t *t)
{
    if (c == 0) for (int q = 0; q < k; ++q) t[q] = kept[q];
    else if (c == 1) for (int q = 0; q < k; ++q) t[q] = kept[k - 1 - q];
    else tour_nn(C, kept, k, tour_nn_start(c, S, k), t);
}

// the sweeps on t (tmp: k entries of scratch), cur its cost going in and coming out -> the number of moves applied
inline int tour_improve_host(const TourField &F, int k, double min_gain, int max_sweeps, uint8_t *t, uint8_t *tmp, double &cur)
{
    const int n_codes = tour_n_codes(k);
    int applied = 0;
    while (applied < max_sweeps) {
        double bd = INFINITY;
        int bc = INT32_MAX;
        TourMove mv;
        for (int code = 0; code < n_codes; ++code) {
            if (!tour_decode(k, code, mv)) continue;
            const double d = tour_eval_host(F, t, k, mv, nullptr, nullptr);
            if (tour_better(d, code, bd, bc)) { bd = d; bc = code; }
        }
        if (!(bd < cur - min_gain)) break;
        (void)tour_decode(k, bc, mv);
        for (int q = 0; q < k; ++q) tmp[q] = (uint8_t)tour_moved(t, mv, q);
        for (int q = 0; q < k; ++q) t[q] = tmp[q];
        cur = bd;
        ++applied;
    }
    return applied;
}

struct TourResult { double cost, stored, joint; int winner, sweeps, skipped, status; };

// One field, the cells c0 .. c1 of voff: w, stored_node (or NULL), E, X (or NULL) are the arrays of ALL fields, D the field's block (unused
// beyond the caps).  order, node: the field's m entries or NULL; tours: candidate c's at tours[c * stride + q] or NULL; costs: S or NULL.
inline TourResult tour_field_host(const int64_t *voff, int64_t c0, int64_t c1, const double *w, const int32_t *stored_node, const double *D,
                                  const double *E, const double *X, int S, double min_gain, int max_sweeps, int32_t *order, int32_t *node,
                                  int32_t *tours, int64_t stride, double *costs)
{
    const double nan = __builtin_nan("");
    const int64_t m64 = c1 - c0;
    int skipped = 0;
    for (int64_t c = c0; c < c1; ++c) skipped += voff[c + 1] == voff[c];
    if (!tour_supported(voff, c0, c1)) {
        for (int64_t q = 0; q < m64; ++q) {
            if (order) order[q] = (int32_t)q;
            if (node) node[q] = -1;
            if (tours) for (int c = 0; c < S; ++c) tours[c * stride + q] = (int32_t)q;
        }
        if (costs) for (int c = 0; c < S; ++c) costs[c] = nan;
        return { nan, nan, nan, 0, 0, skipped, TOUR_EUNSUPPORTED };
    }
    const int m = (int)m64;
    int noff[TOUR_MAX_CELLS + 1];
    uint8_t kept[TOUR_MAX_CELLS], rest[TOUR_MAX_CELLS], t[TOUR_MAX_CELLS], tmp[TOUR_MAX_CELLS], best_t[TOUR_MAX_CELLS];
    int k = 0, n_rest = 0;
    for (int j = 0; j <= m; ++j) noff[j] = (int)(2 * (voff[c0 + j] - voff[c0]));
    for (int j = 0; j < m; ++j)
        if (noff[j + 1] > noff[j]) kept[k++] = (uint8_t)j; else rest[n_rest++] = (uint8_t)j;
    const int64_t n0 = 2 * voff[c0];
    const TourField F = { D, E ? E + n0 : nullptr, X ? X + n0 : nullptr, w + voff[c0], noff, noff[m] };
    const int32_t *sn = stored_node ? stored_node + c0 : nullptr;
    const double stored = tour_stored(F, kept, k, sn);
    const bool improve = tour_finite(stored);
    TourResult out = { stored, stored, nan, 0, 0, skipped, improve ? TOUR_OK : TOUR_EINVAL };
    double C[TOUR_MAX_CELLS * TOUR_MAX_CELLS];
    if (S > 2 && k > 0) tour_cell_matrix_host(F, m, C);
    const TourMove none = { -1, 0, 0, 0, 0, 0 };
    for (int c = 0; c < S; ++c) {
        if (k > 0) tour_construct(C, kept, k, c, S, t);
        double cost = tour_eval_host(F, t, k, none, nullptr, nullptr);
        const int applied = improve ? tour_improve_host(F, k, min_gain, max_sweeps, t, tmp, cost) : 0;
        if (tours) {
            for (int q = 0; q < k; ++q) tours[c * stride + q] = t[q];
            for (int q = 0; q < n_rest; ++q) tours[c * stride + k + q] = rest[q];
        }
        if (costs) costs[c] = cost;
        if (applied > out.sweeps) out.sweeps = applied;
        if (c == 0 || (improve && cost < out.cost)) {
            out.cost = cost; out.winner = c;
            for (int q = 0; q < k; ++q) best_t[q] = t[q];
        }
    }
    int32_t nd[TOUR_MAX_CELLS];
    for (int j = 0; j < m; ++j) nd[j] = -1;
    if (improve) {
        int16_t pred[TOUR_MAX_NODES];
        int b = -1;
        out.cost = tour_eval_host(F, best_t, k, none, pred, &b);
        for (int q = k - 1; q >= 0; --q) {
            const int cell = best_t[q], u = b - noff[cell];
            nd[cell] = u;
            if (q > 0) b = noff[best_t[q - 1]] + pred[b];
        }
        out.joint = tour_joints(F, best_t, k, nd);
    } else {
        out.cost = stored;
        for (int q = 0; q < k; ++q) {
            const int cell = kept[q], u = sn ? sn[cell] : 0;
            nd[cell] = (u < 0 || u >= noff[cell + 1] - noff[cell]) ? 0 : u;
        }
    }
    for (int q = 0; q < m; ++q) {
        if (order) order[q] = q < k ? best_t[q] : rest[q - k];
        if (node) node[q] = nd[q];
    }
    return out;
}

}  // namespace fcpp
