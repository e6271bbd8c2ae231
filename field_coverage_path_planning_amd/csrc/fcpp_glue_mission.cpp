// fcpp_glue_mission.cpp -- C-ABI glue of the mission paths: a field's path sets joined into one drivable path (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_mission.h"
#include "fcpp_missionfn.h"
#include "fcpp_parallel.h"

using namespace fcpp;

namespace {
// what the three entries and the host twin check alike before any offsets are read.  sample_arrays: the path set's columns the entry reads
int mission_args(int mode, int64_t n_fields, const void *item_offsets, int64_t n_items, const void *item_path, const void *item_closed, int64_t n_paths,
                 const void *path_offsets, int64_t n_samples, bool sample_arrays, const double *ex, const double *ey, const double *eh, const double *xx,
                 const double *xy, const double *xh, double radius)
{
    if (!item_offsets || !path_offsets || (n_items > 0 && (!item_path || !item_closed)) || (n_samples > 0 && !sample_arrays))
        return fail(FCPP_EINVAL, "bad arguments");
    if (((ex || ey || eh) && !(ex && ey && eh)) || ((xx || xy || xh) && !(xx && xy && xh)))
        return fail(FCPP_EINVAL, "an entry or exit pose takes all three of x, y and heading");
    const int rc = route_radius(radius, mode);
    if (rc) return rc;
    if (n_fields < 0 || n_items < 0 || n_paths < 0 || n_samples < 0 || n_fields > INT32_MAX || n_items > ((int64_t)1 << 30) || n_paths > INT32_MAX
        || n_samples > ((int64_t)1 << 38))
        return fail(FCPP_ESIZE, "bad sizes (at most 2^30 items)");
    return FCPP_OK;
}

// the three host tables every entry reads and checks: the items of the fields, the samples of the paths, the path of every item
struct MissionTables {
    std::vector<int64_t> ioff, poff, ipath;
    int get(fcpp_ctx *c, int64_t n_fields, const int64_t *item_offsets, const int64_t *item_offsets_host, int64_t n_items, const int64_t *item_path,
            const int64_t *item_path_host, int64_t n_paths, const int64_t *path_offsets, const int64_t *path_offsets_host, int64_t n_samples)
    {
        int rc = host_offsets(c, n_fields, item_offsets, item_offsets_host, n_items, "item_offsets", ioff);
        if (rc == FCPP_OK) rc = host_offsets(c, n_paths, path_offsets, path_offsets_host, n_samples, "path_offsets", poff);
        if (rc == FCPP_OK) rc = host_table(c, n_items, item_path, item_path_host, ipath);
        if (rc) return rc;
        for (int64_t i = 0; i < n_items; ++i)
            if (ipath[(size_t)i] < 0 || ipath[(size_t)i] >= n_paths) return fail(FCPP_ESIZE, "item_path must name a path of the set");
        return FCPP_OK;
    }
};

// where every item's nodes have room (n_items + 1)
int mission_node_bases(const MissionTables &t, const std::vector<int32_t> &closed, int64_t stride, std::vector<int64_t> &base)
{
    const int64_t n_items = (int64_t)t.ipath.size();
    try { base.assign((size_t)n_items + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t p = t.ipath[(size_t)i];
        base[(size_t)i + 1] = base[(size_t)i] + mission_node_room(t.poff[(size_t)p + 1] - t.poff[(size_t)p], closed[(size_t)i] != 0, stride);
    }
    return FCPP_OK;
}

bool mission_rec_args(int64_t n_fields, int64_t n_items, const MissionRec &rec)
{
    return (n_fields <= 0 || (rec.status && rec.slot_item && rec.slot_word && rec.slot_seg)) && (n_items <= 0 || rec.item_station);
}

const char *const MISSION_ESIZE = "a slot or a field has 2^31 - 1 samples or more";
}  // namespace

extern "C" {

int fcpp_mission_solve(fcpp_ctx *c, int mode, int64_t n_fields, const int64_t *item_offsets, const int64_t *item_offsets_host, int64_t n_items,
                       const int64_t *item_path, const int64_t *item_path_host, const int32_t *item_closed, int64_t n_paths,
                       const int64_t *path_offsets, const int64_t *path_offsets_host, int64_t n_samples, const double *x, const double *y,
                       const double *heading, const int8_t *part, const int8_t *gear, const double *entry_x, const double *entry_y,
                       const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h, double radius, int64_t stride,
                       int32_t *status, double *transit_length, int32_t *skipped, int64_t *item_station, int64_t *slot_item, int32_t *slot_word,
                       double *slot_seg, double *slot_total)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = mission_args(mode, n_fields, item_offsets, n_items, item_path, item_closed, n_paths, path_offsets, n_samples, x && y && heading && part && gear,
                          entry_x, entry_y, entry_h, exit_x, exit_y, exit_h, radius);
    if (rc) return rc;
    if (stride < 1) return fail(FCPP_EINVAL, "stride must be at least 1");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    MissionTables t;
    std::vector<int32_t> closed;
    std::vector<int64_t> base;
    rc = t.get(c, n_fields, item_offsets, item_offsets_host, n_items, item_path, item_path_host, n_paths, path_offsets, path_offsets_host, n_samples);
    if (rc == FCPP_OK) rc = host_table(c, n_items, item_closed, (const int32_t *)nullptr, closed);
    if (rc == FCPP_OK) rc = mission_node_bases(t, closed, stride, base);
    if (rc) return rc;
    if (n_fields <= 0) return FCPP_OK;
    const int64_t room = base.back();
    DevBuf<int64_t> st_base, st_idx, n_nodes;
    DevBuf<int32_t> pred, end_node, choice;
    HIPCHK(st_base.upload(base, st));
    HIPCHK(st_idx.alloc((size_t)room));
    HIPCHK(n_nodes.alloc((size_t)n_items));
    HIPCHK(pred.alloc((size_t)room));
    HIPCHK(end_node.alloc((size_t)n_fields));
    HIPCHK(choice.alloc((size_t)n_items));
    const MissionIn in = { n_fields, n_items, n_paths, item_offsets, item_path, item_closed, path_offsets, x, y, heading, nullptr, part, gear,
                           entry_x, entry_y, entry_h, exit_x, exit_y, exit_h, radius, stride };
    const MissionTemp T = { st_base.p, st_idx.p, n_nodes.p, pred.p, end_node.p, choice.p };
    const MissionOut out = { status, transit_length, skipped, item_station, slot_item, slot_word, slot_seg, slot_total };
    LAUNCHCHK(launch_mission_stations(st, in, T));
    LAUNCHCHK(launch_mission_layers(st, mode, in, T));
    LAUNCHCHK(launch_mission_finish(st, mode, in, T, out));
    HIPCHK(hipStreamSynchronize(st));          // (the temporaries and the staged bases die here)
    return FCPP_OK;
}

int fcpp_mission_counts(fcpp_ctx *c, int mode, int64_t n_fields, const int64_t *item_offsets, const int64_t *item_offsets_host, int64_t n_items,
                        const int64_t *item_path, const int64_t *item_path_host, const int32_t *item_closed, int64_t n_paths,
                        const int64_t *path_offsets, const int64_t *path_offsets_host, int64_t n_samples, const int32_t *status,
                        const int64_t *item_station, const int64_t *slot_item, const int32_t *slot_word, const double *slot_seg, double spacing,
                        int64_t *out_path_offsets, int64_t *out_path_offsets_host, int64_t *slot_offsets)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = mission_args(mode, n_fields, item_offsets, n_items, item_path, item_closed, n_paths, path_offsets, n_samples, true, nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr, 1.0);
    if (rc == FCPP_OK) rc = positive_finite(spacing, "spacing");
    if (rc) return rc;
    const MissionRec rec = { status, item_station, slot_item, slot_word, slot_seg };
    if (!mission_rec_args(n_fields, n_items, rec) || !out_path_offsets || !slot_offsets) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    MissionTables t;
    rc = t.get(c, n_fields, item_offsets, item_offsets_host, n_items, item_path, item_path_host, n_paths, path_offsets, path_offsets_host, n_samples);
    if (rc) return rc;
    std::vector<int64_t> own;
    if (!out_path_offsets_host) {
        try { own.assign((size_t)n_fields + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
        out_path_offsets_host = own.data();
    }
    const MissionIn in = { n_fields, n_items, n_paths, item_offsets, item_path, item_closed, path_offsets, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 1 };
    rc = sample_counts(c, n_fields, out_path_offsets, out_path_offsets_host, MISSION_ESIZE, [&](hipStream_t st, int64_t *err) {
        return launch_mission_counts(st, mode, in, rec, spacing, slot_offsets, out_path_offsets, err);
    });
    if (rc) return rc;
    for (int64_t f = 0; f < n_fields; ++f)
        if (out_path_offsets_host[f + 1] - out_path_offsets_host[f] > FPATH_MAX_SAMPLES) return fail(FCPP_ESIZE, MISSION_ESIZE);
    return FCPP_OK;
}

int fcpp_mission_fill(fcpp_ctx *c, int mode, int64_t n_fields, const int64_t *item_offsets, const int64_t *item_offsets_host, int64_t n_items,
                      const int64_t *item_path, const int64_t *item_path_host, const int32_t *item_closed, int64_t n_paths,
                      const int64_t *path_offsets, const int64_t *path_offsets_host, int64_t n_samples, const double *x, const double *y,
                      const double *heading, const double *kappa, const int8_t *part, const int8_t *gear, const double *entry_x,
                      const double *entry_y, const double *entry_h, double radius, double spacing, const int32_t *status,
                      const int64_t *item_station, const int64_t *slot_item, const int32_t *slot_word, const double *slot_seg,
                      const int64_t *slot_offsets, int64_t total_samples, double *out_x, double *out_y, double *out_heading, double *out_kappa,
                      int8_t *out_part, int8_t *out_gear, int32_t *out_slot, int64_t *out_src)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = mission_args(mode, n_fields, item_offsets, n_items, item_path, item_closed, n_paths, path_offsets, n_samples,
                          x && y && heading && kappa && part && gear, entry_x, entry_y, entry_h, nullptr, nullptr, nullptr, radius);
    if (rc == FCPP_OK) rc = positive_finite(spacing, "spacing");
    if (rc) return rc;
    const MissionRec rec = { status, item_station, slot_item, slot_word, slot_seg };
    if (!mission_rec_args(n_fields, n_items, rec) || !slot_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (total_samples < 0 || total_samples > ((int64_t)1 << 38)) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    MissionTables t;
    rc = t.get(c, n_fields, item_offsets, item_offsets_host, n_items, item_path, item_path_host, n_paths, path_offsets, path_offsets_host, n_samples);
    if (rc) return rc;
    int64_t first = 0, last = 0;
    rc = table_ends(c, slot_offsets, 2 * n_items + n_fields, &first, &last);
    if (rc) return rc;
    if (first != 0 || last != total_samples) return fail(FCPP_ESIZE, "slot_offsets do not span [0, total_samples]");
    const MissionIn in = { n_fields, n_items, n_paths, item_offsets, item_path, item_closed, path_offsets, x, y, heading, kappa, part, gear,
                           entry_x, entry_y, entry_h, nullptr, nullptr, nullptr, radius, 1 };
    LAUNCHCHK(launch_mission_fill(c->stream, mode, in, rec, spacing, slot_offsets, total_samples, out_x, out_y, out_heading, out_kappa, out_part,
                                  out_gear, out_slot, out_src));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_mission_paths(int mode, int64_t n_fields, const int64_t *item_offsets, int64_t n_items, const int64_t *item_path,
                             const int32_t *item_closed, int64_t n_paths, const int64_t *path_offsets, int64_t n_samples, const double *x,
                             const double *y, const double *heading, const double *kappa, const int8_t *part, const int8_t *gear,
                             const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x, const double *exit_y,
                             const double *exit_h, double radius, int64_t stride, double spacing, int32_t *status, double *transit_length,
                             int32_t *skipped, int64_t *item_station, int64_t *slot_item, int32_t *slot_word, double *slot_seg, double *slot_total,
                             int64_t *out_path_offsets, int64_t *slot_offsets, int64_t cap, double *out_x, double *out_y, double *out_heading,
                             double *out_kappa, int8_t *out_part, int8_t *out_gear, int32_t *out_slot, int64_t *out_src)
{
    int rc = mission_args(mode, n_fields, item_offsets, n_items, item_path, item_closed, n_paths, path_offsets, n_samples,
                          x && y && heading && kappa && part && gear, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h, radius);
    if (rc == FCPP_OK) rc = positive_finite(spacing, "spacing");
    if (rc) return rc;
    if (stride < 1) return fail(FCPP_EINVAL, "stride must be at least 1");
    if (cap < 0) return fail(FCPP_ESIZE, "bad sizes");
    MissionTables t;
    rc = t.get(nullptr, n_fields, item_offsets, nullptr, n_items, item_path, nullptr, n_paths, path_offsets, nullptr, n_samples);
    if (rc) return rc;
    const int64_t n_slots = n_fields > 0 ? 2 * n_items + n_fields : 0;
    const double nan = __builtin_nan("");
    std::vector<int32_t> closed, st, sk, pred, end_node, choice, word;
    std::vector<int64_t> base, st_idx, n_nodes, station, sitem, off;
    std::vector<double> tl, seg, tot;
    try {
        closed.assign(item_closed, item_closed + n_items);
        rc = mission_node_bases(t, closed, stride, base);
        if (rc) return rc;
        st.assign((size_t)n_fields, 0); sk.assign((size_t)n_fields, 0); tl.assign((size_t)n_fields, nan);
        st_idx.assign((size_t)base.back(), 0); pred.assign((size_t)base.back(), 0); n_nodes.assign((size_t)n_items, 0);
        end_node.assign((size_t)n_fields, -1); choice.assign((size_t)n_items, -1); station.assign((size_t)n_items, -1);
        sitem.assign((size_t)n_slots, -1); word.assign((size_t)n_slots, -1); seg.assign((size_t)n_slots * 5, nan); tot.assign((size_t)n_slots, nan);
        off.assign((size_t)n_slots + 1, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    const MissionIn in = { n_fields, n_items, n_paths, item_offsets, item_path, item_closed, path_offsets, x, y, heading, kappa, part, gear,
                           entry_x, entry_y, entry_h, exit_x, exit_y, exit_h, radius, stride };
    const MissionTemp T = { base.data(), st_idx.data(), n_nodes.data(), pred.data(), end_node.data(), choice.data() };
    const MissionOut own = { st.data(), tl.data(), sk.data(), station.data(), sitem.data(), word.data(), seg.data(), tot.data() };
    const MissionRec rec = { st.data(), station.data(), sitem.data(), word.data(), seg.data() };
    std::vector<char> big((size_t)n_fields, 0), nomem((size_t)n_fields, 0);
    WorkerPool::parallel_for(n_fields, [&](int64_t f) {
        std::vector<double> cost;
        try { cost.assign(2 * (size_t)MISSION_MAX_STATIONS, 0.0); } catch (const std::bad_alloc &) { nomem[(size_t)f] = 1; return; }
        for (int64_t i = item_offsets[f]; i < item_offsets[f + 1]; ++i) n_nodes[(size_t)i] = mission_item_nodes(in, i, st_idx.data() + base[(size_t)i]);
        int32_t s;
        if (mission_field_status(in, n_nodes.data(), f, s) == MISSION_OK) {
            if (mode == 0) mission_layers_host<0>(in, T, f, cost.data());
            else mission_layers_host<1>(in, T, f, cost.data());
        }
        if (mode == 0) mission_finish<0>(in, T, f, own);
        else mission_finish<1>(in, T, f, own);
        // the counts of the field's slots (in off, one slot ahead: scanned below)
        int64_t bad = 0, sum = 0;
        for (int64_t q = mission_first_slot(item_offsets, f); q < mission_first_slot(item_offsets, f + 1); ++q) {
            off[(size_t)q + 1] = mode == 0 ? mission_slot_count<0>(in, rec, spacing, f, q, bad) : mission_slot_count<1>(in, rec, spacing, f, q, bad);
            sum += off[(size_t)q + 1];
        }
        big[(size_t)f] = bad != 0 || sum > FPATH_MAX_SAMPLES;
        // the caller's rows: a failed field's per-item and per-slot rows are left alone
        store(status, f, st[(size_t)f]); store(transit_length, f, tl[(size_t)f]); store(skipped, f, sk[(size_t)f]);
        if (st[(size_t)f] != MISSION_OK) return;
        for (int64_t i = item_offsets[f]; i < item_offsets[f + 1]; ++i) store(item_station, i, station[(size_t)i]);
        for (int64_t q = mission_first_slot(item_offsets, f); q < mission_first_slot(item_offsets, f + 1); ++q) {
            store(slot_item, q, sitem[(size_t)q]); store(slot_word, q, word[(size_t)q]); store(slot_total, q, tot[(size_t)q]);
            if (slot_seg) for (int k = 0; k < 5; ++k) slot_seg[5 * q + k] = seg[(size_t)(5 * q + k)];
        }
    });
    for (int64_t f = 0; f < n_fields; ++f) {
        if (nomem[(size_t)f]) return fail(FCPP_ENOMEM, "out of host memory");
        if (big[(size_t)f]) return fail(FCPP_ESIZE, MISSION_ESIZE);
    }
    for (int64_t q = 0; q < n_slots; ++q) off[(size_t)q + 1] += off[(size_t)q];
    if (slot_offsets) memcpy(slot_offsets, off.data(), off.size() * sizeof(int64_t));
    if (out_path_offsets) {
        for (int64_t f = 0; f < n_fields; ++f) out_path_offsets[f] = off[(size_t)mission_first_slot(item_offsets, f)];
        out_path_offsets[n_fields] = off[(size_t)n_slots];
    }
    if (cap == 0 || !(out_x || out_y || out_heading || out_kappa || out_part || out_gear || out_slot || out_src)) return FCPP_OK;
    WorkerPool::parallel_for(n_fields, [&](int64_t f) {
        const int64_t s0 = mission_first_slot(item_offsets, f);
        for (int64_t q = s0; q < mission_first_slot(item_offsets, f + 1); ++q) {
            const int64_t at = off[(size_t)q], K = off[(size_t)q + 1] - at;
            for (int64_t k = 0; k < K && at + k < cap; ++k) {
                double px, py, ph, pk;
                int pp, pg;
                int64_t src;
                if (mode == 0) mission_eval<0>(in, rec, spacing, f, q, k, K, px, py, ph, pk, pp, pg, src);
                else mission_eval<1>(in, rec, spacing, f, q, k, K, px, py, ph, pk, pp, pg, src);
                store(out_x, at + k, px); store(out_y, at + k, py); store(out_heading, at + k, ph); store(out_kappa, at + k, pk);
                store(out_part, at + k, (int8_t)pp); store(out_gear, at + k, (int8_t)pg); store(out_slot, at + k, (int32_t)(q - s0)); store(out_src, at + k, src);
            }
        }
    });
    return FCPP_OK;
}

}  // extern "C"
