// fcpp_missionfn.h -- mission paths: the path sets of a field (headland loops, the field path, the patch passes) joined into ONE drivable
// path per field.  An item is a path of a path set, open (driven from its first sample to its last) or a closed loop (entered at one of its
// stations and left there again after one lap); WHERE every loop is entered is chosen so that the joints between the items are shortest in
// all: a shortest path through the layered graph of the items' nodes.  ONE set of expressions for the host (fcpp_debug_mission_paths, the
// tests' driver) and the device (fcpp_mission.hip), in plain IEEE-754 double operations and compiled with -ffp-contract=off on both sides,
// so that both give the same bits.  Build-defined: the reference joins nothing.
//
// Nothing geometric is written here.  A joint is what dubins_solve / rs_solve give and Conn<MODE>::count / ::eval sample; an item's samples
// are somebody else's, copied.
//
// THE RULE (include/fcpp.h states it for callers).
//   paths     a path set in the samplers' CSR form: path p owns the samples path_off[p] .. path_off[p + 1] (n_p of them) of x, y, heading,
//             kappa, part, gear.
//   items     field f owns the items item_off[f] .. item_off[f + 1], in DRIVING ORDER; item i drives path item_path[i], open
//             (item_closed[i] == 0) or as a closed loop.
//   nodes     an open item has one node: in-pose its path's first sample, out-pose its last.  A closed item's nodes are its STATIONS, the
//             loop transits' rule: local sample index k with k mod stride == 0, part 0 or 4, gear +1 -- and k < n_p - 1, the last sample
//             repeats the first pose; in-pose = out-pose = the sample's pose.  The entry and the exit pose of a field are one-node layers.
//   skipped   an item whose path has no samples, a closed item without a station: it drives nothing and is counted; the others are unaffected.
//   cost      d(a, b): the total the solver gives at R from out(a) to in(b).  c_0 = 0, or fl(0 + d(entry, .)) with an entry;
//             c_j[b] = min over a of fl(c_(j-1)[a] + d(a, b)), a sum that is not below +inf (a NaN: no path) counting as +inf; the predecessor
//             is the LOWEST a that attains the minimum.  The end: the lowest b of the last layer that attains the minimum, after the exit's
//             edge when there is an exit.  (cost, a) is ordered lexicographically: a total order, so any reduction tree gives the same pick.
//   transit   the chosen joints' totals added in driving order, from 0: the chain of additions of the optimum, hence its bits.
//   slots     a field of m items has 2 m + 1 slots, the first 2 item_off[f] + f.  KEPT item j (the j-th that is not skipped) owns slot 2 j, the
//             joint INTO it (empty for the first without an entry) and slot 2 j + 1, itself; slot 2 k behind the k kept items is the exit
//             joint (empty without an exit, or without an entry when k = 0).  The slots behind it are empty.
//   samples   a joint: Conn<MODE>::count / ::eval from the out-pose before it, part MISSION_PART_JOIN, its own gear and kappa, src -1.  An open
//             item: its samples as they are.  A closed item entered at local index k: the samples k, k + 1 .. n_p - 1, 0, 1 .. k: n_p + 1, the
//             seam a doubled junction like every other.  Copied samples keep all six columns; src is the source sample's global index.
//   status    MISSION_EUNSUPPORTED: a closed item of more than MISSION_MAX_STATIONS stations; MISSION_EINVAL: a chosen joint without a word (a
//             chosen pose that is not finite).  Such a field has no samples, transit NaN, and its per-item and per-slot rows are NOT written.
// Every sample is evaluated from its slot alone (mission_eval), every slot's count from its record (mission_slot_count).
#pragma once
#include <math.h>
#include <stdint.h>

#include "fcpp_connfn.h"
#include "fcpp_fpathfn.h"

namespace fcpp {

constexpr int MISSION_MAX_STATIONS = 1024;              // FCPP_MISSION_MAX_STATIONS of include/fcpp.h
constexpr int MISSION_OK = 0, MISSION_EINVAL = -1, MISSION_EUNSUPPORTED = -3;          // FCPP_OK / FCPP_EINVAL / FCPP_EUNSUPPORTED
constexpr int MISSION_PART_JOIN = 6;                    // FCPP_PART_JOIN

// what a call is given (host pointers on the host, device pointers on the device); kappa is read by the fill only, part by the stations only;
// e*, x*: the fields' entry and exit poses or NULL
struct MissionIn {
    int64_t n_fields, n_items, n_paths;
    const int64_t *item_off, *item_path;
    const int32_t *item_closed;
    const int64_t *path_off;
    const double *x, *y, *h, *kappa;
    const int8_t *part, *gear;
    const double *ex, *ey, *eh, *xx, *xy, *xh;
    double R;
    int64_t stride;
};

// the solve's temporaries.  st_base (n_items + 1): item i's nodes have room at st_base[i] .. st_base[i + 1] of st_idx (the node's global
// sample index; an open item's one entry is not used) and pred (the predecessor of every node in the kept item before, 0 in the first
// layer); n_nodes: per item; end_node: per field, the last kept item's chosen node (-1 without a kept item); choice: per item, scratch of
// the backtrack
struct MissionTemp {
    const int64_t *st_base;
    int64_t *st_idx, *n_nodes;
    int32_t *pred, *end_node, *choice;
};

// what the solve writes; any may be NULL.  Per field status, transit_length, skipped; per item item_station; per slot the rest, seg 5 per slot
struct MissionOut {
    int32_t *status;
    double *transit_length;
    int32_t *skipped;
    int64_t *item_station, *slot_item;
    int32_t *slot_word;
    double *slot_seg, *slot_total;
};

// what the counts and the fill are handed back
struct MissionRec {
    const int32_t *status;
    const int64_t *item_station, *slot_item;
    const int32_t *slot_word;
    const double *slot_seg;
};

FCPP_HD int64_t mission_first_slot(const int64_t *item_off, int64_t f) { return 2 * item_off[f] + f; }

// room for the nodes of an item of n_p samples: the local indices k < n_p - 1 with k mod stride == 0; 1 for an open item
FCPP_HD int64_t mission_node_room(int64_t n_p, bool closed, int64_t stride) { return !closed ? 1 : (n_p > 1 ? (n_p - 2) / stride + 1 : 0); }

// is local sample k of the n_p samples from p0 a station?
FCPP_HD bool mission_is_station(const MissionIn &in, int64_t p0, int64_t n_p, int64_t k)
{
    if (k < 0 || k >= n_p - 1 || k % in.stride != 0) return false;
    const int p = in.part[p0 + k];
    return (p == 0 || p == 4) && in.gear[p0 + k] == 1;
}

// the global sample whose pose is node a's in-pose (out false) or out-pose (out true)
FCPP_HD int64_t mission_node_sample(const MissionIn &in, const MissionTemp &T, int64_t item, int64_t a, bool out)
{
    const int64_t p = in.item_path[item];
    if (in.item_closed[item]) return T.st_idx[T.st_base[item] + a];
    return out ? in.path_off[p + 1] - 1 : in.path_off[p];
}

// the order of (cost, a): a sum that is not below +inf counts as +inf
struct MissionPick { double c; int64_t a; };
FCPP_HD MissionPick mission_pick_none() { return { INFINITY, INT64_MAX }; }
FCPP_HD void mission_pick_take(MissionPick &p, double c, int64_t a)
{
    const double cc = c < INFINITY ? c : INFINITY;
    if (cc < p.c || (cc == p.c && a < p.a)) { p.c = cc; p.a = a; }
}

// the field's status before anything is chosen, and its skipped items
FCPP_HD int mission_field_status(const MissionIn &in, const int64_t *n_nodes, int64_t f, int32_t &skipped)
{
    int st = MISSION_OK;
    skipped = 0;
    for (int64_t i = in.item_off[f]; i < in.item_off[f + 1]; ++i) {
        if (n_nodes[i] <= 0) ++skipped;
        if (in.item_closed[i] && n_nodes[i] > MISSION_MAX_STATIONS) st = MISSION_EUNSUPPORTED;
    }
    return st;
}

// ---- finish: backtrack, the chosen joints by the sequential form of the solve, the records ------------------------------------------------
struct MissionJoint { int word; double seg[5], total; };

template <int MODE>
FCPP_HD MissionJoint mission_joint(double x0, double y0, double h0, double x1, double y1, double h1, double R)
{
    MissionJoint j;
    for (int k = 0; k < 5; ++k) j.seg[k] = 0.0;
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, R, j.word, j.seg, j.total);
    return j;
}

FCPP_HD void mission_store_slot(const MissionOut &o, int64_t s, int64_t item, int word, const double *seg, double total)
{
    if (o.slot_item) o.slot_item[s] = item;
    if (o.slot_word) o.slot_word[s] = word;
    if (o.slot_seg) for (int k = 0; k < 5; ++k) o.slot_seg[5 * s + k] = seg ? seg[k] : __builtin_nan("");
    if (o.slot_total) o.slot_total[s] = total;
}

// the chosen chain of field f (T.choice holds the kept items' nodes) walked in driving order: WRITE false -> is every joint solved?;
// WRITE true: the per-item and per-slot rows.  transit: the joints' totals added in order.
template <int MODE, bool WRITE>
FCPP_HD bool mission_walk(const MissionIn &in, const MissionTemp &T, int64_t f, const MissionOut &o, double &transit)
{
    const int64_t i0 = in.item_off[f], i1 = in.item_off[f + 1], s0 = mission_first_slot(in.item_off, f);
    const double nan = __builtin_nan("");
    bool have = in.ex != nullptr, ok = true;
    double px = have ? in.ex[f] : 0.0, py = have ? in.ey[f] : 0.0, ph = have ? in.eh[f] : 0.0;
    int64_t j = 0;
    transit = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        if (T.n_nodes[i] <= 0) {
            if (WRITE && o.item_station) o.item_station[i] = -1;
            continue;
        }
        const int64_t gin = mission_node_sample(in, T, i, T.choice[i], false), gout = mission_node_sample(in, T, i, T.choice[i], true);
        if (have) {
            const MissionJoint jt = mission_joint<MODE>(px, py, ph, in.x[gin], in.y[gin], in.h[gin], in.R);
            if (jt.word < 0) ok = false;
            transit = transit + jt.total;
            if (WRITE) mission_store_slot(o, s0 + 2 * j, -1, jt.word, jt.seg, jt.total);
        } else if (WRITE) mission_store_slot(o, s0 + 2 * j, -1, -1, nullptr, nan);
        if (WRITE) {
            mission_store_slot(o, s0 + 2 * j + 1, i, -1, nullptr, nan);
            if (o.item_station) o.item_station[i] = in.item_closed[i] ? gin : -1;
        }
        px = in.x[gout]; py = in.y[gout]; ph = in.h[gout];
        have = true;
        ++j;
    }
    int64_t s = s0 + 2 * j;
    if (have && in.xx && (j > 0 || in.ex)) {
        const MissionJoint jt = mission_joint<MODE>(px, py, ph, in.xx[f], in.xy[f], in.xh[f], in.R);
        if (jt.word < 0) ok = false;
        transit = transit + jt.total;
        if (WRITE) mission_store_slot(o, s, -1, jt.word, jt.seg, jt.total);
    } else if (WRITE) mission_store_slot(o, s, -1, -1, nullptr, nan);
    if (WRITE)
        for (++s; s < s0 + 2 * (i1 - i0) + 1; ++s) mission_store_slot(o, s, -1, -1, nullptr, nan);
    return ok;
}

// field f from the solve's temporaries (n_nodes, st_idx, pred, end_node) to its outputs
template <int MODE>
FCPP_HD void mission_finish(const MissionIn &in, const MissionTemp &T, int64_t f, const MissionOut &o)
{
    const int64_t i0 = in.item_off[f], i1 = in.item_off[f + 1];
    int32_t skipped;
    int status = mission_field_status(in, T.n_nodes, f, skipped);
    double transit = __builtin_nan("");
    if (status == MISSION_OK) {
        int64_t cur = T.end_node[f];
        for (int64_t i = i1 - 1; i >= i0; --i) {
            T.choice[i] = -1;
            if (T.n_nodes[i] <= 0) continue;
            if (cur < 0 || cur >= T.n_nodes[i]) cur = 0;           // (never: the solve's picks are nodes; keeps every read inside the arrays)
            T.choice[i] = (int32_t)cur;
            cur = T.pred[T.st_base[i] + cur];
        }
        if (!mission_walk<MODE, false>(in, T, f, o, transit)) { status = MISSION_EINVAL; transit = __builtin_nan(""); }
        else mission_walk<MODE, true>(in, T, f, o, transit);
    }
    if (o.status) o.status[f] = status;
    if (o.transit_length) o.transit_length[f] = transit;
    if (o.skipped) o.skipped[f] = skipped;
}

// ---- counts and samples, from the records as the caller hands them back -------------------------------------------------------------------
// what slot s of field f holds: 0 nothing, 1 a joint, 2 an item (item, its path's first sample p0 and its n_p > 0 samples, k0 the local
// index it is entered at -- 0 for an open item).  A record that names no item of the field or no sample of the item's path holds nothing.
FCPP_HD int mission_slot_kind(const MissionIn &in, const MissionRec &rec, int64_t f, int64_t s, int64_t &item, int64_t &p0, int64_t &n_p, int64_t &k0)
{
    item = -1; p0 = n_p = k0 = 0;
    if (rec.status[f] != MISSION_OK) return 0;
    const int64_t it = rec.slot_item[s];
    if (it < 0) return rec.slot_word[s] >= 0 ? 1 : 0;
    if (it < in.item_off[f] || it >= in.item_off[f + 1]) return 0;
    const int64_t p = in.item_path[it];
    if (p < 0 || p >= in.n_paths) return 0;
    p0 = in.path_off[p]; n_p = in.path_off[p + 1] - p0;
    if (n_p <= 0) return 0;
    if (in.item_closed[it]) {
        k0 = rec.item_station[it] - p0;
        if (k0 < 0 || k0 >= n_p) return 0;
    }
    item = it;
    return 2;
}

// the samples of slot s of field f; bad: 2^31 - 1 or more
template <int MODE>
FCPP_HD int64_t mission_slot_count(const MissionIn &in, const MissionRec &rec, double spacing, int64_t f, int64_t s, int64_t &bad)
{
    int64_t item, p0, n_p, k0, b = 0;
    const int kind = mission_slot_kind(in, rec, f, s, item, p0, n_p, k0);
    if (kind == 0) return 0;
    const int64_t K = kind == 1 ? Conn<MODE>::count(rec.slot_word[s], rec.slot_seg + 5 * s, spacing, b) : n_p + (in.item_closed[item] ? 1 : 0);
    if (b || K > FPATH_MAX_SAMPLES) { ++bad; return 0; }
    return K;
}

// the pose a joint in slot s of field f starts at: the entry pose in the field's first slot, else the out-pose of the item in slot s - 1
FCPP_HD bool mission_joint_start(const MissionIn &in, const MissionRec &rec, int64_t f, int64_t s, double &x, double &y, double &h)
{
    if (s == mission_first_slot(in.item_off, f)) {
        if (!in.ex) return false;
        x = in.ex[f]; y = in.ey[f]; h = in.eh[f];
        return true;
    }
    int64_t item, p0, n_p, k0;
    if (mission_slot_kind(in, rec, f, s - 1, item, p0, n_p, k0) != 2) return false;
    const int64_t g = in.item_closed[item] ? p0 + k0 : p0 + n_p - 1;
    x = in.x[g]; y = in.y[g]; h = in.h[g];
    return true;
}

// sample k of the K samples of slot s of field f (K by mission_slot_count; a K that is not repeats the slot's last sample)
template <int MODE>
FCPP_HD void mission_eval(const MissionIn &in, const MissionRec &rec, double spacing, int64_t f, int64_t s, int64_t k, int64_t K, double &x, double &y,
                          double &h, double &kappa, int &part, int &gear, int64_t &src)
{
    int64_t item, p0, n_p, k0;
    const int kind = mission_slot_kind(in, rec, f, s, item, p0, n_p, k0);
    x = y = h = kappa = __builtin_nan("");
    part = MISSION_PART_JOIN; gear = 0; src = -1;
    if (kind == 2) {
        const int64_t last = in.item_closed[item] ? n_p : n_p - 1;
        src = p0 + (k0 + (k < last ? k : last)) % n_p;
        x = in.x[src]; y = in.y[src]; h = in.h[src]; kappa = in.kappa[src]; part = in.part[src]; gear = in.gear[src];
        return;
    }
    double sx, sy, sh;
    if (kind != 1 || !mission_joint_start(in, rec, f, s, sx, sy, sh)) return;
    Conn<MODE>::eval(sx, sy, sh, in.R, rec.slot_word[s], rec.slot_seg + 5 * s, spacing, k, K, x, y, h, kappa, gear);
}

// ---- the host twin: one field's stations and its layers -----------------------------------------------------------------------------------
// the nodes of item i -> their number; idx: room for mission_node_room of them
inline int64_t mission_item_nodes(const MissionIn &in, int64_t i, int64_t *idx)
{
    const int64_t p = in.item_path[i], p0 = in.path_off[p], n_p = in.path_off[p + 1] - p0;
    if (!in.item_closed[i]) return n_p > 0 ? 1 : 0;
    int64_t c = 0;
    for (int64_t k = 0; k < n_p - 1; k += in.stride)
        if (mission_is_station(in, p0, n_p, k)) idx[c++] = p0 + k;
    return c;
}

template <int MODE>
inline double mission_len(double x0, double y0, double h0, double x1, double y1, double h1, double R)
{
    int word;
    double seg[5], total;
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, R, word, seg, total);
    return total;
}

// the layers of field f (status MISSION_OK, T.n_nodes and T.st_idx made): T.pred and T.end_node.  cost: 2 x MISSION_MAX_STATIONS doubles
template <int MODE>
inline void mission_layers_host(const MissionIn &in, const MissionTemp &T, int64_t f, double *cost)
{
    double *cur = cost, *nxt = cost + MISSION_MAX_STATIONS;
    int64_t prev = -1, m = 0;
    if (in.ex) { cur[0] = 0.0; m = 1; }
    for (int64_t i = in.item_off[f]; i < in.item_off[f + 1]; ++i) {
        const int64_t n = T.n_nodes[i];
        if (n <= 0) continue;
        for (int64_t b = 0; b < n; ++b) {
            MissionPick best = mission_pick_none();
            if (m == 0) best = { 0.0, 0 };
            const int64_t gb = mission_node_sample(in, T, i, b, false);
            for (int64_t a = 0; a < m; ++a) {
                const int64_t ga = prev >= 0 ? mission_node_sample(in, T, prev, a, true) : -1;
                const double d = prev >= 0 ? mission_len<MODE>(in.x[ga], in.y[ga], in.h[ga], in.x[gb], in.y[gb], in.h[gb], in.R)
                                           : mission_len<MODE>(in.ex[f], in.ey[f], in.eh[f], in.x[gb], in.y[gb], in.h[gb], in.R);
                mission_pick_take(best, cur[a] + d, a);
            }
            nxt[b] = best.c;
            T.pred[T.st_base[i] + b] = (int32_t)best.a;
        }
        double *t = cur; cur = nxt; nxt = t;
        prev = i; m = n;
    }
    MissionPick end = mission_pick_none();
    for (int64_t a = 0; prev >= 0 && a < m; ++a) {
        const int64_t ga = mission_node_sample(in, T, prev, a, true);
        const double d = in.xx ? mission_len<MODE>(in.x[ga], in.y[ga], in.h[ga], in.xx[f], in.xy[f], in.xh[f], in.R) : 0.0;
        mission_pick_take(end, cur[a] + d, a);
    }
    T.end_node[f] = prev >= 0 ? (int32_t)end.a : -1;
}

}  // namespace fcpp
