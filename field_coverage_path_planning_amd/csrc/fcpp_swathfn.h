// fcpp_swathfn.h -- the swaths of ANY polygon field: which parallel tracks of working width W at track angle theta cover a field given as
// rings (ring 0 the outer boundary, further rings holes).  ONE set of expressions for the host (fcpp_debug_swaths, the tests' checker) and
// the device (fcpp_swath.hip), written like fcpp_dubinsfn.h / fcpp_rsfn.h in plain IEEE-754 double operations with fc_sincos of
// fcpp_math.h and compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the reference's swath
// generator reads a field's bounding box and four corners only.
//
// THE RULE (include/fcpp.h states it for callers).
//   input     a field is a list of rings, closed implicitly, of either orientation; its interior follows the EVEN-ODD rule, so neither an
//             orientation nor a nesting test is needed.  Two CSR levels: ring_offsets (fields -> rings), vert_offsets (rings -> vertices).
//   frame     (s, c) = fc_sincos(theta); every vertex gets  u = x c + y s  along the tracks and  w = -x s + y c  across them (swath_uw: one
//             expression per vertex, so the two edges that share a vertex see the same w).  w_min, w_max: over all vertices of the field.
//   lines     line k lies at  w_k = fl(fl(w_min + first) + fl(k W))  (swath_line_w), 0 <= first < W the offset of line 0.  The field has K
//             lines: the k >= 0 with w_k < w_max -- floor((w_max - fl(w_min + first)) / W) + 1 corrected by stepping to the first k whose
//             line is not below w_max (swath_n_lines; w_k is non-decreasing in k, the estimate is off by at most a few).
//   crossings an edge (p, q), in ring order, crosses line k iff (w_p <= w_k) != (w_q <= w_k), at
//             u = u_p + (w_k - w_p) / (w_q - w_p) * (u_q - u_p).  Half-open: an edge lying ON a line never crosses it, a line through a vertex
//             is counted consistently, and every line has an even number of crossings with every closed ring.
//   segments  the crossings of a line sorted by u ascending, ties by (ring, edge) -- they are inserted in that order behind their equals; as a
//             record carries only u, the order among equals changes no output -- and paired (0, 1), (2, 3), ...  A segment is a swath iff
//             u_b - u_a > min_length (min_length >= 0: touches of zero length never appear).
//   records   a swath's end points mapped back, (u c - w_k s, u s + w_k c) (swath_point), its line k and its length u_b - u_a; within a field
//             ordered by k, then by u.
//   length    the sum of a field's swath lengths in a FIXED order: 64 partial sums, sum j taking the swaths of the lines k = j mod 64 in the
//             order of the records, then acc[j] += acc[j + o] for o = 32, 16, .. 1 (the device's lanes and its xor butterfly): the same bits.
//   status    FCPP_EINVAL: no ring, a ring with fewer than 3 vertices, a vertex that is not finite (or whose u or w is not).
//             FCPP_EUNSUPPORTED: a line with more than FCPP_SWATH_MAX_CROSSINGS = 64 crossings, or more than 2^22 lines.  Such a field has no
//             swaths, no lines and length 0; EINVAL wins over EUNSUPPORTED.
// theta: finite, |theta| <= 1e5 (fc_sincos' range).  theta = 0 gives s = 0 and c = 1 exactly.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_math.h"

namespace fcpp {

constexpr int SWATH_MAX_CROSSINGS = 64;                  // FCPP_SWATH_MAX_CROSSINGS of include/fcpp.h
constexpr int64_t SWATH_MAX_LINES = (int64_t)1 << 22;
constexpr int SWATH_OK = 0, SWATH_EINVAL = -1, SWATH_EUNSUPPORTED = -3;      // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr double SWATH_MAX_ANGLE = 1e5;

FCPP_HD void swath_uw(double x, double y, double c, double s, double &u, double &w)
{
    u = x * c + y * s;
    w = -x * s + y * c;
}

FCPP_HD bool swath_finite(double v) { return fabs(v) <= 1.79769313486231570815e+308; }          // false for NaN

FCPP_HD double swath_line_w(double base, double W, int64_t k) { return base + (double)k * W; }      // base = fl(w_min + first)

// K, or SWATH_MAX_LINES + 1 for more than that
FCPP_HD int64_t swath_n_lines(double w_min, double w_max, double first, double W)
{
    const double base = w_min + first;
    if (!(base < w_max)) return 0;
    const double q = floor((w_max - base) / W);
    if (!(q < (double)SWATH_MAX_LINES)) return SWATH_MAX_LINES + 1;
    int64_t k = (int64_t)q + 1;
    while (k > 0 && !(swath_line_w(base, W, k - 1) < w_max)) --k;
    while (k <= SWATH_MAX_LINES && swath_line_w(base, W, k) < w_max) ++k;
    return k;
}

FCPP_HD bool swath_crosses(double wp, double wq, double wk) { return (wp <= wk) != (wq <= wk); }
FCPP_HD double swath_cross_u(double up, double wp, double uq, double wq, double wk) { return up + (wk - wp) / (wq - wp) * (uq - up); }

// col[0], col[stride], ..: `cnt` < SWATH_MAX_CROSSINGS values in ascending order; v goes behind its equals
FCPP_HD void swath_insert(double *col, int stride, int cnt, double v)
{
    int j = cnt;
    while (j > 0) {
        const double prev = col[(j - 1) * stride];
        if (!(prev > v)) break;
        col[j * stride] = prev;
        --j;
    }
    col[j * stride] = v;
}

FCPP_HD void swath_point(double u, double wk, double c, double s, double &x, double &y)
{
    x = u * c - wk * s;
    y = u * s + wk * c;
}

struct SwathTotals {
    int32_t status, n_lines, n_swaths;
    double length;
};

// The rule on the host, line by line: one field (rings r0 .. r1 of vert_offsets) at one angle.  emit(k, ua, ub, wk, c, s, len) is called
// for every swath in record order.
template <class Emit>
inline SwathTotals swath_field_host(const int64_t *vert_offsets, int64_t r0, int64_t r1, const double *x, const double *y, double theta, double W,
                                    double first, double min_length, double *u, double *w, Emit emit)
{
    SwathTotals out = { SWATH_OK, 0, 0, 0.0 };
    const SwathTotals invalid = { SWATH_EINVAL, 0, 0, 0.0 }, unsupported = { SWATH_EUNSUPPORTED, 0, 0, 0.0 };
    if (r1 <= r0) return invalid;
    double s, c;
    fc_sincos(theta, s, c);
    const int64_t v0 = vert_offsets[r0], v1 = vert_offsets[r1];
    for (int64_t r = r0; r < r1; ++r)
        if (vert_offsets[r + 1] - vert_offsets[r] < 3) return invalid;
    double w_min = INFINITY, w_max = -INFINITY;
    for (int64_t v = v0; v < v1; ++v) {
        swath_uw(x[v], y[v], c, s, u[v - v0], w[v - v0]);
        if (!swath_finite(x[v]) || !swath_finite(y[v]) || !swath_finite(u[v - v0]) || !swath_finite(w[v - v0])) return invalid;
        if (w[v - v0] < w_min) w_min = w[v - v0];
        if (w[v - v0] > w_max) w_max = w[v - v0];
    }
    const int64_t K = swath_n_lines(w_min, w_max, first, W);
    if (K > SWATH_MAX_LINES) return unsupported;
    const double base = w_min + first;
    double cr[SWATH_MAX_CROSSINGS];
    // first pass: the cap (a field over it emits nothing); second pass: the records
    for (int pass = 0; pass < 2; ++pass) {
        double acc[64];
        for (int j = 0; j < 64; ++j) acc[j] = 0.0;
        int64_t n_sw = 0;
        for (int64_t k = 0; k < K; ++k) {
            const double wk = swath_line_w(base, W, k);
            int cnt = 0;
            for (int64_t r = r0; r < r1; ++r) {
                const int64_t a = vert_offsets[r] - v0, m = vert_offsets[r + 1] - vert_offsets[r];
                for (int64_t e = 0; e < m; ++e) {
                    const int64_t p = a + e, q = a + (e + 1 == m ? 0 : e + 1);
                    if (!swath_crosses(w[p], w[q], wk)) continue;
                    if (cnt == SWATH_MAX_CROSSINGS) return unsupported;
                    swath_insert(cr, 1, cnt, swath_cross_u(u[p], w[p], u[q], w[q], wk));
                    ++cnt;
                }
            }
            if (pass == 0) continue;
            for (int j = 0; j + 1 < cnt; j += 2) {
                const double len = cr[j + 1] - cr[j];
                if (!(len > min_length)) continue;
                acc[k & 63] += len;
                ++n_sw;
                emit(k, cr[j], cr[j + 1], wk, c, s, len);
            }
        }
        if (pass == 0) continue;
        for (int o = 32; o > 0; o >>= 1)
            for (int j = 0; j < o; ++j) acc[j] = acc[j] + acc[j + o];
        out.n_lines = (int32_t)K;
        out.n_swaths = (int32_t)n_sw;
        out.length = acc[0];
    }
    return out;
}

}  // namespace fcpp
