// fcpp_hpathfn.h -- headland paths: every ring of a polygon inset (fcpp_inset_fill's x, y, src: the centre line of one headland pass) as ONE
// sampled, closed, drivable path.  ONE set of expressions for the host (fcpp_debug_headland_paths, the tests' checker) and the device
// (fcpp_legs.hip), written like fcpp_fpathfn.h in plain IEEE-754 double operations with the transcendentals of fcpp_math.h / fcpp_geom.h
// (fc_sincos, atan2_fd, fc_hypot) and compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the
// reference has no polygon fields.  The straight elements are sampled by fpath_eval's swath rule, the connectors solved, counted and
// sampled by Conn<MODE> (fcpp_connfn.h); what is written HERE is the rule that turns a ring into elements and joints, and the followed arc.
//
// THE RULE (include/fcpp.h states it for callers).  A ring has m vertices v_0 .. v_(m-1), closed implicitly, and the inset distance d.
//   driving   direction +1: driven vertex k is v_k, its chord's source s_k = src[k].  direction -1: driven vertex k is v_((m - k) mod m),
//             s_k = src[m - 1 - k] (the stored chord that ends there).  Both start at v_0.  Driven vertex k owns slot 2 k (an element) and
//             slot 2 k + 1 (the joint behind it); ring r's first slot is 2 roff[r].
//   elements  driven vertex k starts an element iff k = 0, or s_k is even, or s_k != s_(k-1).  The element runs from A = its start vertex
//             to B = the next element start, cyclically (the last one ends at v_0); the arc vertices between only mark the run.  With
//             (dx, dy) = B - A, c = fc_hypot(dx, dy), h_c = atan2_fd(dy, dx):
//               s even: a STRAIGHT element of length c and heading h_c.
//               s odd : an ARC element of radius d: h = sqrt(max(d d - c c / 4, 0)), half = atan2_fd(c / 2, h), sweep D = 2 half, length d D.
//                       As stored the arc turns right (sigma = -1), driven backwards left (sigma = +1): kappa = sigma / d, heading
//                       h_c - sigma half at A and h_c + sigma half at B (both wrapped), centre = (A + (dx, dy) / 2) - sigma h (u_y, -u_x),
//                       u = (dx, dy) / c.  DRIVABLE iff d >= R.
//             An element with c = 0 (or c NaN) and an undrivable arc have no leg: they are skipped.
//   element   straight: fpath_eval's swath rule (sample_count(c, spacing, end), t = fmin(k spacing / c, 1), the last sample B itself), kappa 0,
//   legs      gear +1, part 0.  Followed arc: sample_count(d D, spacing, end) samples at s = k spacing: heading hd = h_A + sigma s / d, position
//             centre + sigma d (sin hd, -cos hd) (= centre + d (cos, sin) of hd - sigma pi / 2), heading wrap(hd); the FIRST sample is A
//             itself with h_A, the LAST B itself with h_B.  kappa = sigma / d, gear +1, part 4.
//   joint     only a drivable element e has one.  f = the next drivable element in driving order, cyclically (e itself when it is the
//   legs      only one).  If f directly follows e and |wrap(h_in(f) - h_out(e))| <= smooth_tol there is no leg.  Otherwise a connector:
//             Conn<MODE>::solve at R from (B_e, h_out(e)) to (A_f, h_in(f)), counted and sampled by Conn<MODE>::count / ::eval, part 1.
//   junctions stay doubled, as in the field paths.
//   totals    one pass over the ring's slots in order: work = straight elements + followed arcs, transit = connectors, skipped = d D of
//             the undrivable arcs.
//   status    EINVAL: m < 2, a vertex or d that is not finite, a negative src, an arc with d <= 0, a connector with word -1: no samples,
//             NaN totals.  Else EUNSUPPORTED: no drivable element: no samples (the totals stand: work 0, transit 0, what was skipped).
// A leg with 2^31 samples or more counts FPATH_OVERSIZE (the call's FCPP_ESIZE).  Every sample is evaluated from its leg's record alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_fpathfn.h"
#include "fcpp_geom.h"

namespace fcpp {

constexpr int HPATH_OK = 0, HPATH_EINVAL = -1, HPATH_EUNSUPPORTED = -3;       // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr int HPATH_ARC = 4, HPATH_SKIPPED = 5;                               // a leg's kind, beside FPATH_NONE .. FPATH_RS
constexpr int HPATH_PART_ARC = 4;                                             // beside FPATH_PART_SWATH (0) and FPATH_PART_BETWEEN (1)
constexpr int64_t HPATH_MAX_VERTS = (int64_t)1 << 30;                         // n_verts of one call: slots stay int32

// what a call is given (host pointers on the host, device pointers on the device)
struct HpathIn {
    const int64_t *roff;                 // n_rings + 1: rings -> vertices
    const double *x, *y;                 // n_verts
    const int32_t *src;                  // n_verts
    const double *dist;                  // n_rings
    double R, spacing, smooth_tol;
    int direction;                       // +1 / -1
};

// a leg's record.  leg: a straight element as a swath record, a connector as the field paths hold it (leg.field is the RING).  A followed
// arc (HPATH_ARC): (x0, y0, h0) the pose at A, seg[0], seg[1] = B, seg[2] = total = d D, seg[3] = kappa; centre, radius and h_B beside it.
// A skipped arc (HPATH_SKIPPED): total = d D, no samples.  128 bytes.
struct HpathLeg {
    FpathLeg leg;
    double cx, cy, d, h1;
};

// an element of a ring, from driven vertex k0 to driven vertex k1 (k1 = m: back at v_0)
struct HpathElem {
    int64_t k0, k1;
    int kind;                            // FPATH_NONE (c = 0), FPATH_SWATH, HPATH_ARC, HPATH_SKIPPED
    bool invalid;                        // an arc with a radius that is not positive
    double ax, ay, bx, by, h_in, h_out, len, cx, cy, kappa;
};

FCPP_HD bool hpath_finite(double v) { return v - v == 0.0; }
FCPP_HD bool hpath_drivable(int kind) { return kind == FPATH_SWATH || kind == HPATH_ARC; }
// the stored vertex that is driven k-th (k = m: v_0 again)
FCPP_HD int64_t hpath_vertex(int64_t m, int dir, int64_t k) { return k <= 0 || k >= m ? 0 : (dir > 0 ? k : m - k); }
FCPP_HD int32_t hpath_src(const int32_t *src, int64_t m, int dir, int64_t k) { return dir > 0 ? src[k] : src[m - 1 - k]; }
FCPP_HD bool hpath_starts(const int32_t *src, int64_t m, int dir, int64_t k)
{
    if (k == 0) return true;
    const int32_t s = hpath_src(src, m, dir, k);
    return (s & 1) == 0 || s != hpath_src(src, m, dir, k - 1);
}

// The element that driven vertex k (an element start, 0 <= k < m) of a ring at v0 starts.  The scan to its end is bounded by the ring.
FCPP_HD void hpath_element(const HpathIn &in, int64_t v0, int64_t m, double d, int64_t k, HpathElem &e)
{
    const double *x = in.x + v0, *y = in.y + v0;
    const int32_t *src = in.src + v0;
    const int dir = in.direction;
    int64_t j = k + 1;
    while (j < m && !hpath_starts(src, m, dir, j)) ++j;
    const int64_t ia = hpath_vertex(m, dir, k), ib = hpath_vertex(m, dir, j);
    const int32_t s = hpath_src(src, m, dir, k);
    e.k0 = k; e.k1 = j; e.kind = FPATH_NONE; e.invalid = false;
    e.ax = x[ia]; e.ay = y[ia]; e.bx = x[ib]; e.by = y[ib];
    e.h_in = e.h_out = e.len = e.cx = e.cy = e.kappa = 0.0;
    const double dx = e.bx - e.ax, dy = e.by - e.ay;
    const double c = fc_hypot(dx, dy);
    if ((s & 1) && !(d > 0.0)) { e.invalid = true; return; }
    if (!(c > 0.0) || !hpath_finite(c)) return;
    const double hc = atan2_fd(dy, dx);
    if ((s & 1) == 0) {
        e.kind = FPATH_SWATH; e.h_in = e.h_out = hc; e.len = c;
        return;
    }
    const double sigma = dir > 0 ? -1.0 : 1.0;
    const double h = sqrt(fmax(d * d - 0.25 * (c * c), 0.0));
    const double half = atan2_fd(0.5 * c, h);
    const double ux = dx / c, uy = dy / c;
    e.len = d * (2.0 * half);
    e.h_in = dubins_wrap_pi(hc - sigma * half);
    e.h_out = dubins_wrap_pi(hc + sigma * half);
    e.cx = (e.ax + 0.5 * dx) - sigma * (h * uy);
    e.cy = (e.ay + 0.5 * dy) + sigma * (h * ux);
    e.kappa = sigma / d;
    e.kind = d >= in.R ? HPATH_ARC : HPATH_SKIPPED;
}

FCPP_HD void hpath_clear(HpathLeg &lg, int64_t r, int64_t slot)
{
    lg.leg.field = (int32_t)r; lg.leg.slot = (int32_t)slot; lg.leg.kind = FPATH_NONE; lg.leg.part = FPATH_PART_SWATH; lg.leg.word = -1; lg.leg.pad = 0;
    lg.leg.x0 = lg.leg.y0 = lg.leg.h0 = lg.leg.total = 0.0;
    for (int q = 0; q < 5; ++q) lg.leg.seg[q] = 0.0;
    lg.cx = lg.cy = lg.d = lg.h1 = 0.0;
}

// Driven vertex k of ring r: the records of its two slots and their sample counts (0 without a leg, FPATH_OVERSIZE).  invalid: this vertex
// makes its ring EINVAL; drivable: it starts a drivable element.  Both scans -- to the end of its own element, and over the skipped
// elements to the next drivable one -- stay inside the ring and end after at most m steps.
template <int MODE>
FCPP_HD void hpath_legs(const HpathIn &in, int64_t r, int64_t k, HpathLeg &el, HpathLeg &jt, int64_t &cnt_el, int64_t &cnt_jt, bool &invalid,
                        bool &drivable)
{
    const int64_t v0 = in.roff[r], m = in.roff[r + 1] - v0;
    const double d = in.dist[r];
    hpath_clear(el, r, 2 * k);
    hpath_clear(jt, r, 2 * k + 1);
    cnt_el = cnt_jt = 0;
    drivable = false;
    invalid = m < 2 || !hpath_finite(d) || !hpath_finite(in.x[v0 + k]) || !hpath_finite(in.y[v0 + k]) || in.src[v0 + k] < 0;
    if (m < 2 || !hpath_starts(in.src + v0, m, in.direction, k)) return;
    HpathElem e;
    hpath_element(in, v0, m, d, k, e);
    if (e.invalid) { invalid = true; return; }
    if (e.kind == FPATH_NONE) return;
    int64_t bad = 0;
    el.leg.kind = e.kind;
    el.leg.x0 = e.ax; el.leg.y0 = e.ay; el.leg.h0 = e.h_in;
    el.leg.seg[0] = e.bx; el.leg.seg[1] = e.by; el.leg.seg[2] = e.len; el.leg.total = e.len;
    if (e.kind != FPATH_SWATH) {
        el.leg.part = HPATH_PART_ARC; el.leg.seg[3] = e.kappa;
        el.cx = e.cx; el.cy = e.cy; el.d = d; el.h1 = e.h_out;
    }
    if (e.kind == HPATH_SKIPPED) return;
    drivable = true;
    {
        const int64_t K = sample_count(e.len, in.spacing, true, false, bad);
        cnt_el = bad ? FPATH_OVERSIZE : K;
    }
    // the next drivable element, over the skipped ones: at most one visit per element of the ring
    HpathElem f;
    bool direct = true, found = false;
    int64_t kk = e.k1;
    for (int64_t it = 0; it < m && !found; ++it) {
        if (kk >= m) kk = 0;
        if (kk == k) break;                                  // round the ring: the element itself
        hpath_element(in, v0, m, d, kk, f);
        if (f.invalid) { invalid = true; return; }
        if (hpath_drivable(f.kind)) found = true;
        else { direct = false; kk = f.k1; }
    }
    if (!found) { f = e; direct = false; }
    if (direct && fabs(dubins_wrap_pi(f.h_in - e.h_out)) <= in.smooth_tol) return;
    jt.leg.part = FPATH_PART_BETWEEN;
    jt.leg.x0 = e.bx; jt.leg.y0 = e.by; jt.leg.h0 = e.h_out;
    int word;
    Conn<MODE>::solve(e.bx, e.by, e.h_out, f.ax, f.ay, f.h_in, in.R, word, jt.leg.seg, jt.leg.total);
    jt.leg.kind = MODE == 0 ? FPATH_DUBINS : FPATH_RS; jt.leg.word = word;
    if (word < 0) { invalid = true; return; }
    bad = 0;
    const int64_t K = Conn<MODE>::count(word, jt.leg.seg, in.spacing, bad);
    cnt_jt = bad ? FPATH_OVERSIZE : K;
}

// sample k of the K samples of a leg
FCPP_HD void hpath_eval(const HpathLeg &lg, double R, double spacing, int64_t k, int64_t K, double &x, double &y, double &h, double &kappa, int &gear)
{
    if (lg.leg.kind != HPATH_ARC) { fpath_eval(lg.leg, R, spacing, k, K, x, y, h, kappa, gear); return; }
    const double len = lg.leg.seg[2], s = (double)k * spacing;
    kappa = lg.leg.seg[3]; gear = 1;
    if (k >= K - 1 || s > len) { x = lg.leg.seg[0]; y = lg.leg.seg[1]; h = lg.h1; return; }
    if (k <= 0) { x = lg.leg.x0; y = lg.leg.y0; h = lg.leg.h0; return; }
    const double sigma = kappa > 0.0 ? 1.0 : -1.0;
    const double hd = lg.leg.h0 + sigma * (s / lg.d);
    double sn, cs;
    fc_sincos(hd, sn, cs);
    x = lg.cx + sigma * (lg.d * sn);
    y = lg.cy - sigma * (lg.d * cs);
    h = dubins_wrap_pi(hd);
}

// a ring's totals from its 2 m records, in slot order (a ring that is not EINVAL)
FCPP_HD void hpath_totals(const HpathLeg *legs, int64_t m, double &work, double &transit, double &skipped)
{
    work = transit = skipped = 0.0;
    for (int64_t j = 0; j < 2 * m; ++j) {
        const int kind = legs[j].leg.kind;
        const double t = legs[j].leg.total;
        if (kind == FPATH_SWATH || kind == HPATH_ARC) work += t;
        else if (kind == FPATH_DUBINS || kind == FPATH_RS) transit += t;
        else if (kind == HPATH_SKIPPED) skipped += t;
    }
}

// ---- the host twin: one ring -----------------------------------------------------------------------------------------------------------
// legs, cnt: the ring's 2 m slots.  -> the status; a failed ring's counts are 0, an EINVAL ring's totals NaN.
template <int MODE>
inline int hpath_ring_host(const HpathIn &in, int64_t r, HpathLeg *legs, int64_t *cnt, double &work, double &transit, double &skipped, bool &oversize)
{
    const int64_t m = in.roff[r + 1] - in.roff[r];
    bool any_invalid = m < 2, any_drivable = false;
    for (int64_t k = 0; k < m; ++k) {
        bool invalid, drivable;
        hpath_legs<MODE>(in, r, k, legs[2 * k], legs[2 * k + 1], cnt[2 * k], cnt[2 * k + 1], invalid, drivable);
        any_invalid = any_invalid || invalid;
        any_drivable = any_drivable || drivable;
    }
    const int status = any_invalid ? HPATH_EINVAL : (any_drivable ? HPATH_OK : HPATH_EUNSUPPORTED);
    oversize = leg_counts_host(cnt, 2 * m, status == HPATH_OK);
    if (status != HPATH_EINVAL) hpath_totals(legs, m, work, transit, skipped);
    else work = transit = skipped = __builtin_nan("");
    return status;
}

// ---- the leg set of the headland paths (what FieldLegs of fcpp_fpathfn.h is to the field paths): a group is a ring ----------------------
struct RingLegs {
    typedef HpathIn In;
    typedef HpathLeg Leg;
    static constexpr int N_TOTALS = 3;                                     // work, transit, skipped
    static FCPP_HD int64_t first_slot(const In &in, int64_t g) { return 2 * in.roff[g]; }
    static FCPP_HD const FpathLeg &base(const Leg &lg) { return lg.leg; }
    static FCPP_HD void eval(const Leg &lg, double R, double spacing, int64_t k, int64_t K, double &x, double &y, double &h, double &kappa, int &gear)
    {
        hpath_eval(lg, R, spacing, k, K, x, y, h, kappa, gear);
    }
    // the totals of group g (legs: its first record): NaN only for EINVAL (a ring without a drivable element keeps what was skipped)
    static FCPP_HD void totals(const In &in, const Leg *legs, int64_t g, int status, double *t)
    {
        t[0] = t[1] = t[2] = __builtin_nan("");
        if (status != HPATH_EINVAL) hpath_totals(legs, in.roff[g + 1] - in.roff[g], t[0], t[1], t[2]);
    }
};

}  // namespace fcpp
