// fcpp_fpathfn.h -- field paths: the sampled path of every field of a batch from its cut swaths (fcpp_swath_fill's records), a driving order
// (the stored boustrophedon or fcpp_route_solve's route) and the connectors between them, with optional entry and exit poses.  ONE set of
// expressions for the host (fcpp_debug_field_paths, the tests' checker) and the device (fcpp_legs.hip), written like fcpp_routefn.h in
// plain IEEE-754 double operations and compiled with -ffp-contract=off on both sides, so that both give the same bits.  Build-defined: the
// reference has no polygon fields.  Nothing is restated here: the poses are route_pose's, the connectors dubins_solve's / rs_solve's and
// their samples, like the count rule, the samplers' own (Conn<MODE>::eval / ::count and sample_count of fcpp_connfn.h).
//
// THE RULE (include/fcpp.h states it for callers).
//   slots     a field of m swaths has 2 m + 1 leg slots: slot 0 the entry connector, slot 2 k + 1 the k-th swath in driving order, slot
//             2 k + 2 the connector behind it, the last slot (2 m) the exit connector.  Field i's first slot is 2 soff[i] + i.  A slot without
//             a leg has no samples: entry / exit without a pose, the one slot of a field with m = 0.
//   order     NULL: the stored boustrophedon route_stored(0, k); else m_total int32, field i's m values at soff[i], each an oriented swath
//             2 s + d local to the field (SwathRoute.order).  An entry outside 0 .. 2 m - 1 or a swath named twice: the field is EINVAL.
//   swath     from (sx, sy) to (ex, ey) (route_pose of the oriented swath), len = the record's own length: sample_count(len, spacing, end)
//             samples, sample k at t = fmin((k spacing) / len, 1), x = sx + t (ex - sx), y likewise; the LAST sample is (ex, ey) itself (a swath
//             of length 0 is that one sample); heading dubins_wrap_pi of the oriented heading, curvature 0, gear +1.  A length that is
//             negative, infinite or NaN: the field is EINVAL.
//   connector dubins_solve (mode 0) or rs_solve (mode 1) at R from the exit pose of the leg before (or the field's entry pose) to the entry
//             pose of the leg behind (or the field's exit pose); sampled as fcpp_dubins_sample / fcpp_rs_sample sample a solved path (the
//             last sample AT the path's end; Reeds-Shepp per gear run, a cusp twice).  Word -1: the field is EINVAL.
//   junctions stay doubled: a swath's last sample and the connector's first are two samples (of one position).
//   totals    work = the swath lengths added in driving order; transit = the connector totals added in route_cost's order: the entry
//             connector (or 0), the connectors between swaths left to right, then the exit connector (or 0).  NaN for a failed field.
//   failed    a field that is EINVAL has no samples at all; the other fields are unaffected.
// A leg with 2^31 samples or more counts FPATH_OVERSIZE (the call's FCPP_ESIZE).  Every sample is evaluated from its leg's record alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_routefn.h"
#include "fcpp_solveclearfn.h"

namespace fcpp {

constexpr int FPATH_OK = 0, FPATH_EINVAL = -1;                          // FCPP_OK / FCPP_EINVAL
constexpr int FPATH_NONE = 0, FPATH_SWATH = 1, FPATH_DUBINS = 2, FPATH_RS = 3;          // a leg's kind
constexpr int FPATH_PART_SWATH = 0, FPATH_PART_BETWEEN = 1, FPATH_PART_ENTRY = 2, FPATH_PART_EXIT = 3;
constexpr int64_t FPATH_OVERSIZE = -1;                                   // the count of a leg of 2^31 samples or more
constexpr int64_t FPATH_MAX_SWATHS = (int64_t)1 << 30;                  // n_total of one call: slots and oriented swaths stay int32
constexpr int64_t FPATH_MAX_SAMPLES = 2147483646;

// what a call is given (host pointers on the host, device pointers on the device); order, e* and x* may be NULL
struct FpathIn {
    const int64_t *soff;                                   // n + 1
    const double *ax, *ay, *bx, *by, *length;              // n_total each: the swath records
    const double *angle;                                   // n
    const int32_t *order;                                  // n_total or NULL
    double R, spacing;
    const double *ex, *ey, *eh, *xx, *xy, *xh;             // n each or NULL: the fields' entry and exit poses
};

// a leg's record: all a sample of it is evaluated from.  swath: (x0, y0) its start, h0 the wrapped heading, seg[0], seg[1] its end,
// total = seg[2] its length; connector: the start pose, the word and its segments (three for Dubins, five for Reeds-Shepp), total.
struct FpathLeg {
    int32_t field, slot, kind, part, word, pad;
    double x0, y0, h0, seg[5], total;
};

FCPP_HD int64_t fpath_first_slot(const int64_t *soff, int64_t i) { return 2 * soff[i] + i; }

// the oriented swath at position k of a field's driving order; false when the entry names none
FCPP_HD bool fpath_oriented(const int32_t *order, int64_t s0, int64_t m, int64_t k, int &p)
{
    if (!order) { p = route_stored(0, (int)k); return true; }
    p = order[s0 + k];
    return p >= 0 && (int64_t)p < 2 * m;
}

// The poses of the connector in (even) slot j of field i, 0 <= j <= 2 m, m > 0: from the exit pose of the leg before (or the field's entry
// pose) to the entry pose of the leg behind (or the field's exit pose), route_pose's UNWRAPPED headings -- what fpath_leg hands to the solver
// and the clear stage (below) to solve_clear.  false: the slot has no leg (no entry / exit pose) or, with invalid set, no poses (an order
// entry out of range).
FCPP_HD bool fpath_conn_poses(const FpathIn &in, int64_t i, int64_t j, double &x0, double &y0, double &h0, double &x1, double &y1, double &h1,
                              bool &invalid)
{
    const int64_t s0 = in.soff[i], m = in.soff[i + 1] - s0;
    const double *ax = in.ax + s0, *ay = in.ay + s0, *bx = in.bx + s0, *by = in.by + s0;
    const double theta = in.angle[i];
    const bool entry = j == 0, exit = j == 2 * m;
    if ((entry && !in.ex) || (exit && !in.xx)) return false;
    int p;
    if (entry) { x0 = in.ex[i]; y0 = in.ey[i]; h0 = in.eh[i]; }
    else {
        if (!fpath_oriented(in.order, s0, m, j / 2 - 1, p)) { invalid = true; return false; }
        route_pose(ax, ay, bx, by, theta, p, true, x0, y0, h0);
    }
    if (exit) { x1 = in.xx[i]; y1 = in.xy[i]; h1 = in.xh[i]; }
    else {
        if (!fpath_oriented(in.order, s0, m, j / 2, p)) { invalid = true; return false; }
        route_pose(ax, ay, bx, by, theta, p, false, x1, y1, h1);
    }
    return true;
}

// Slot j of field i: its record, and -> its sample count (0 without a leg, FPATH_OVERSIZE).  invalid: the slot makes its field EINVAL
// (an order entry out of range, a bad length, an unsolvable connector); a swath named twice is the caller's to find (it needs all slots).
template <int MODE>
FCPP_HD int64_t fpath_leg(const FpathIn &in, int64_t i, int64_t j, FpathLeg &leg, bool &invalid)
{
    const int64_t s0 = in.soff[i], m = in.soff[i + 1] - s0;
    leg.field = (int32_t)i; leg.slot = (int32_t)j; leg.kind = FPATH_NONE; leg.part = FPATH_PART_SWATH; leg.word = -1; leg.pad = 0;
    leg.x0 = leg.y0 = leg.h0 = leg.total = 0.0;
    for (int k = 0; k < 5; ++k) leg.seg[k] = 0.0;
    invalid = false;
    if (m <= 0 || j < 0 || j > 2 * m) return 0;
    int64_t bad = 0;
    if (j & 1) {
        const double *ax = in.ax + s0, *ay = in.ay + s0, *bx = in.bx + s0, *by = in.by + s0;
        const double theta = in.angle[i];
        int p;
        if (!fpath_oriented(in.order, s0, m, (j - 1) / 2, p)) { invalid = true; return 0; }
        const double len = in.length[s0 + (p >> 1)];
        double sx, sy, sh, ex, ey, eh;
        route_pose(ax, ay, bx, by, theta, p, false, sx, sy, sh);
        route_pose(ax, ay, bx, by, theta, p, true, ex, ey, eh);
        leg.kind = FPATH_SWATH;
        leg.x0 = sx; leg.y0 = sy; leg.h0 = dubins_wrap_pi(sh);
        leg.seg[0] = ex; leg.seg[1] = ey; leg.seg[2] = len; leg.total = len;
        if (!(len >= 0.0) || !(len < INFINITY)) { invalid = true; return 0; }
        const int64_t K = sample_count(len, in.spacing, true, false, bad);
        return bad ? FPATH_OVERSIZE : K;
    }
    double x0, y0, h0, x1, y1, h1;
    if (!fpath_conn_poses(in, i, j, x0, y0, h0, x1, y1, h1, invalid)) return 0;
    const bool entry = j == 0, exit = j == 2 * m;
    leg.part = entry ? FPATH_PART_ENTRY : (exit ? FPATH_PART_EXIT : FPATH_PART_BETWEEN);
    leg.x0 = x0; leg.y0 = y0; leg.h0 = h0;
    int word;
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, in.R, word, leg.seg, leg.total);
    leg.kind = MODE == 0 ? FPATH_DUBINS : FPATH_RS; leg.word = word;
    if (word < 0) { invalid = true; return 0; }
    const int64_t K = Conn<MODE>::count(word, leg.seg, in.spacing, bad);
    return bad ? FPATH_OVERSIZE : K;
}

// sample k of the K samples of a leg
FCPP_HD void fpath_eval(const FpathLeg &leg, double R, double spacing, int64_t k, int64_t K, double &x, double &y, double &h, double &kappa,
                        int &gear)
{
    if (leg.kind == FPATH_SWATH) {
        const double ex = leg.seg[0], ey = leg.seg[1], len = leg.seg[2];
        const double t = fmin(((double)k * spacing) / len, 1.0);
        x = leg.x0 + t * (ex - leg.x0);
        y = leg.y0 + t * (ey - leg.y0);
        if (k >= K - 1) { x = ex; y = ey; }
        h = leg.h0; kappa = 0.0; gear = 1;
        return;
    }
    x = y = h = kappa = __builtin_nan("");
    gear = 0;
    if (leg.kind == FPATH_DUBINS) Conn<0>::eval(leg.x0, leg.y0, leg.h0, R, leg.word, leg.seg, spacing, k, K, x, y, h, kappa, gear);
    else if (leg.kind == FPATH_RS) Conn<1>::eval(leg.x0, leg.y0, leg.h0, R, leg.word, leg.seg, spacing, k, K, x, y, h, kappa, gear);
}

// a field's totals from its 2 m + 1 records (a field that is not EINVAL)
FCPP_HD void fpath_totals(const FpathLeg *legs, int64_t m, bool has_entry, bool has_exit, double &work, double &transit)
{
    work = 0.0; transit = 0.0;
    if (m <= 0) return;
    for (int64_t k = 0; k < m; ++k) work += legs[2 * k + 1].total;
    double sum = has_entry ? legs[0].total : 0.0;
    for (int64_t k = 0; k + 1 < m; ++k) sum += legs[2 * k + 2].total;
    transit = sum + (has_exit ? legs[2 * m].total : 0.0);
}

// ---- the host twins' count rule, for every leg rule: a failed group's counts are 0; -> a leg or the group has 2^31 samples or more -------
inline bool leg_counts_host(int64_t *cnt, int64_t n_slots, bool ok)
{
    bool oversize = false;
    int64_t sum = 0;
    for (int64_t j = 0; j < n_slots; ++j) {
        if (!ok) cnt[j] = 0;
        else if (cnt[j] < 0) { oversize = true; cnt[j] = 0; }
        sum += cnt[j];
    }
    return oversize || sum > FPATH_MAX_SAMPLES;
}

// ---- the host twin: one field ---------------------------------------------------------------------------------------------------------
// legs, cnt: the field's 2 m + 1 slots; seen: m entries of scratch.  -> the status; a failed field's counts are 0, its totals NaN.
inline int64_t fpath_field_slots(const FpathIn &in, int64_t i)
{
    const int64_t m = in.soff[i + 1] - in.soff[i];
    return 2 * (m > 0 ? m : 0) + 1;
}

// the records and raw counts of the field's slots -> the status
template <int MODE>
inline int fpath_field_records(const FpathIn &in, int64_t i, FpathLeg *legs, int64_t *cnt, int32_t *seen)
{
    const int64_t s0 = in.soff[i], m = in.soff[i + 1] - s0, n_slots = fpath_field_slots(in, i);
    int status = FPATH_OK;
    for (int64_t k = 0; k < m; ++k) seen[k] = 0;
    for (int64_t j = 0; j < n_slots; ++j) {
        bool invalid;
        cnt[j] = fpath_leg<MODE>(in, i, j, legs[j], invalid);
        if (!invalid && in.order && (j & 1) && m > 0 && seen[in.order[s0 + (j - 1) / 2] >> 1]++ != 0) invalid = true;
        if (invalid) status = FPATH_EINVAL;
    }
    return status;
}

// the counts as the scan takes them and the totals, from the records
inline void fpath_field_finish(const FpathIn &in, int64_t i, int status, const FpathLeg *legs, int64_t *cnt, double &work, double &transit,
                               bool &oversize)
{
    oversize = leg_counts_host(cnt, fpath_field_slots(in, i), status == FPATH_OK);
    if (status == FPATH_OK) fpath_totals(legs, in.soff[i + 1] - in.soff[i], in.ex != nullptr, in.xx != nullptr, work, transit);
    else work = transit = __builtin_nan("");
}

template <int MODE>
inline int fpath_field_host(const FpathIn &in, int64_t i, FpathLeg *legs, int64_t *cnt, int32_t *seen, double &work, double &transit,
                            bool &oversize)
{
    const int status = fpath_field_records<MODE>(in, i, legs, cnt, seen);
    fpath_field_finish(in, i, status, legs, cnt, work, transit, oversize);
    return status;
}

// ---- the CLEAR field paths: drive, per connector, the shortest word that stays off the field's region ---------------------------------
// THE CLEAR RULE (include/fcpp.h states it for callers).  The field paths above with ONE difference: in a field of status OK the record of
// every connector slot -- word, seg, total -- is what solve_clear<MODE> (fcpp_solveclearfn.h) gives for the slot's poses
// (fpath_conn_poses), R and field i of a region CSR (field i of the swaths is field i of the CSR).  rank >= 0: that candidate of the pair,
// rank 0 the record as it was.  rank -1 (no candidate clear, a start outside the region, a region field of status CLEAR_EINVAL): the
// shortest word, as it was, with its crossings -- the leg is still driven.  Counts, samples, junctions, part / gear / leg and the totals
// follow from the records as above.  Per slot rank and crossings: 0 on a swath slot, a slot without a leg and in a field that is EINVAL
// (whose records stay what the rule above made them).  Per field blocked = its legs of rank -1, reshaped = its legs of rank > 0.
// The device (fcpp_solveclear.hip) does not solve again: it tests the record's word (solve_clear_test, as solve_clear_first does) and
// looks at the other words with a lane per word; the bits are solve_clear's.
FCPP_HD bool fpath_is_conn(const FpathLeg &leg) { return (leg.kind == FPATH_DUBINS || leg.kind == FPATH_RS) && leg.word >= 0; }

// a chosen word into a connector's record -> its sample count
template <int MODE>
FCPP_HD int64_t fpath_set_word(FpathLeg &leg, int word, const double *seg, double total, double spacing)
{
    leg.word = word;
    for (int k = 0; k < Conn<MODE>::NSEG; ++k) leg.seg[k] = seg[k];
    leg.total = total;
    int64_t bad = 0;
    const int64_t K = Conn<MODE>::count(word, leg.seg, spacing, bad);
    return bad ? FPATH_OVERSIZE : K;
}

// rank, crossings: the field's 2 m + 1 slots; the rest as fpath_field_host
template <int MODE>
inline int fpath_field_clear_host(const FpathIn &in, const ClearFields &F, int64_t i, FpathLeg *legs, int64_t *cnt, int32_t *seen, int32_t *rank,
                                  int32_t *crossings, int32_t &blocked, int32_t &reshaped, double &work, double &transit, bool &oversize)
{
    const int64_t n_slots = fpath_field_slots(in, i);
    const int status = fpath_field_records<MODE>(in, i, legs, cnt, seen);
    blocked = reshaped = 0;
    for (int64_t j = 0; j < n_slots; ++j) rank[j] = crossings[j] = 0;
    for (int64_t j = 0; status == FPATH_OK && j < n_slots; j += 2) {
        if (!fpath_is_conn(legs[j])) continue;
        double x0, y0, h0, x1, y1, h1;
        bool invalid = false;
        if (!fpath_conn_poses(in, i, j, x0, y0, h0, x1, y1, h1, invalid)) continue;      // (the record exists: so do the poses)
        const SolveClearResult r = solve_clear<MODE>(F, i, x0, y0, h0, x1, y1, h1, in.R);
        if (r.word < 0) continue;                                                        // (the record is solved: so is r)
        cnt[j] = fpath_set_word<MODE>(legs[j], r.word, r.seg, r.len, in.spacing);
        rank[j] = r.rank; crossings[j] = r.crossings;
        blocked += r.rank < 0; reshaped += r.rank > 0;
    }
    fpath_field_finish(in, i, status, legs, cnt, work, transit, oversize);
    return status;
}

// ---- the leg set of the field paths: all that the kernels, launchers and entries shared by the leg-path operators (fcpp_legs.hip, -------
// fcpp_paths.cpp) ask of one.  A GROUP (here a field) owns a contiguous run of leg slots, first_slot(g) .. first_slot(g + 1).
struct FieldLegs {
    typedef FpathIn In;
    typedef FpathLeg Leg;
    static constexpr int N_TOTALS = 2;                                     // work, transit
    static FCPP_HD int64_t first_slot(const In &in, int64_t g) { return fpath_first_slot(in.soff, g); }
    static FCPP_HD const FpathLeg &base(const Leg &lg) { return lg; }
    static FCPP_HD void eval(const Leg &lg, double R, double spacing, int64_t k, int64_t K, double &x, double &y, double &h, double &kappa, int &gear)
    {
        fpath_eval(lg, R, spacing, k, K, x, y, h, kappa, gear);
    }
    // the totals of group g (legs: its first record): NaN unless the field is OK
    static FCPP_HD void totals(const In &in, const Leg *legs, int64_t g, int status, double *t)
    {
        t[0] = t[1] = __builtin_nan("");
        if (status == FPATH_OK) fpath_totals(legs, in.soff[g + 1] - in.soff[g], in.ex != nullptr, in.xx != nullptr, t[0], t[1]);
    }
};

}  // namespace fcpp
