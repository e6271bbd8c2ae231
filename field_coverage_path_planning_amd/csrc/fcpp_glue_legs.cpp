// fcpp_glue_legs.cpp -- C-ABI glue of the leg paths: field paths, headland paths, clear field paths, loop transits (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_clear.h"
#include "fcpp_clearfn.h"
#include "fcpp_fpathfn.h"
#include "fcpp_hpathfn.h"
#include "fcpp_legs.h"
#include "fcpp_parallel.h"
#include "fcpp_solveclear.h"
#include "fcpp_transit.h"
#include "fcpp_transitfn.h"

using namespace fcpp;

namespace {
// the connectors' radius and mode, the samples' spacing: what every leg operator checks of them
int leg_spacing(double radius, int mode, double spacing)
{
    const int rc = route_radius(radius, mode);
    return rc ? rc : positive_finite(spacing, "spacing");
}

// ---- field paths: what fcpp_field_path_counts / _fill and fcpp_debug_field_paths check alike ------------------------------------------------
// the arguments that need no offsets: NULLs, the poses' triples, radius, mode, spacing, the sizes
int fpath_args(int64_t n, const void *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx, const double *by,
               const double *length, const double *angle, double radius, int mode, double spacing, const double *ex, const double *ey,
               const double *eh, const double *xx, const double *xy, const double *xh)
{
    if (!swath_offsets || (n_total > 0 && (!ax || !ay || !bx || !by || !length)) || (n > 0 && !angle)) return fail(FCPP_EINVAL, "bad arguments");
    if (((ex || ey || eh) && !(ex && ey && eh)) || ((xx || xy || xh) && !(xx && xy && xh)))
        return fail(FCPP_EINVAL, "an entry or exit pose takes all three of x, y and heading");
    const int rc = leg_spacing(radius, mode, spacing);
    if (rc) return rc;
    if (n < 0 || n_total < 0 || n > INT32_MAX || n_total > FPATH_MAX_SWATHS) return fail(FCPP_ESIZE, "bad sizes (at most 2^30 swaths)");
    return FCPP_OK;
}

// the swath offsets on the host and the angles, checked (read back from the device where the caller has no host copy)
int fpath_offsets(fcpp_ctx *c, int64_t n, const int64_t *soff_ptr, const int64_t *soff_host, int64_t n_total, const double *angle_ptr,
                  const double *angle_host, std::vector<int64_t> &soff)
{
    int rc = host_offsets(c, n, soff_ptr, soff_host, n_total, "swath_offsets", soff);
    if (rc == FCPP_OK) rc = swath_angles(c, n, angle_ptr, angle_host);
    return rc;
}

// ---- headland paths: what fcpp_headland_path_counts / _fill and fcpp_debug_headland_paths check alike --------------------------------------
int hpath_args(int64_t n_rings, const void *ring_offsets, int64_t n_verts, const double *x, const double *y, const int32_t *src,
               const double *ring_dist, double radius, int mode, double spacing, int direction, double smooth_tol)
{
    if (!ring_offsets || (n_verts > 0 && (!x || !y || !src)) || (n_rings > 0 && !ring_dist)) return fail(FCPP_EINVAL, "bad arguments");
    const int rc = leg_spacing(radius, mode, spacing);
    if (rc) return rc;
    if (direction != 1 && direction != -1) return fail(FCPP_EINVAL, "direction must be +1 (as stored) or -1");
    if (!(smooth_tol >= 0.0)) return fail(FCPP_EINVAL, "smooth_tol must not be negative");
    if (n_rings < 0 || n_verts < 0 || n_rings > INT32_MAX || n_verts > HPATH_MAX_VERTS) return fail(FCPP_ESIZE, "bad sizes (at most 2^30 vertices)");
    return FCPP_OK;
}
// ---- leg paths: what the field paths' and the headland paths' three entries are behind their argument checks, on the leg set P ------------
// (FieldLegs / RingLegs of the rule headers; the kernels: fcpp_legs.hip).  A fill RECOMPUTES the leg records from its inputs (one more
// launch of the rule kernel) instead of keeping the counts call's in the context: the entries stay stateless, and the solves are a small
// part of the samples' cost.
// *_counts: the temporaries (n_scratch: the int32 scratch of the rule kernel), the call's own status buffer when the caller passes none
// stage(stream, legs, cnt, status) -> 0 or a hipError_t value: what an entry does to the records between the rule kernel and the scan
struct NoLegStage {
    template <class Leg> int operator()(hipStream_t, Leg *, int64_t *, const int32_t *) const { return 0; }
};

template <class P, class Stage = NoLegStage>
int legs_counts(fcpp_ctx *c, int64_t n_groups, int64_t n_slots, int64_t n_scratch, const typename P::In &in, int mode, const char *esize,
                int64_t *path_offsets, int64_t *path_offsets_host, int64_t *leg_offsets, const LegTotals &totals, int32_t *status,
                Stage &&stage = Stage())
{
    DevBuf<typename P::Leg> legs;
    DevBuf<int64_t> cnt;
    DevBuf<int32_t> scratch, own_status;
    HIPCHK(legs.alloc((size_t)n_slots));
    HIPCHK(cnt.alloc((size_t)n_slots));
    HIPCHK(scratch.alloc((size_t)n_scratch));
    if (!status) { HIPCHK(own_status.alloc((size_t)n_groups)); status = own_status.p; }
    return sample_counts(c, n_groups, path_offsets, path_offsets_host, esize, [&](hipStream_t st, int64_t *err) {
        if (n_scratch > 0) { const hipError_t e = hipMemsetAsync(scratch.p, 0, (size_t)n_scratch * sizeof(int32_t), st); if (e != hipSuccess) return (int)e; }
        if (n_groups > 0) { const hipError_t e = hipMemsetAsync(status, 0, (size_t)n_groups * sizeof(int32_t), st); if (e != hipSuccess) return (int)e; }
        int e = launch_legs(st, n_groups, n_slots, in, mode, legs.p, cnt.p, scratch.p, status);
        if (e == 0) e = stage(st, legs.p, cnt.p, status);
        return e ? e : launch_leg_offsets(st, n_groups, n_slots, in, legs.p, cnt.p, status, scratch.p, leg_offsets, path_offsets, totals, err);
    });      // (sample_counts has drained the stream: the temporaries die here)
}

// *_fill.  The ends of the slot offsets must match the output arrays.  (The fill writes sample q < total_samples of every array and reads
// the record of a slot below n_slots whatever lies between the ends: offsets that are not the counts call's give wrong samples, never an
// access outside the arrays.)
template <class P, class Stage = NoLegStage>
int legs_fill(fcpp_ctx *c, int64_t n_groups, int64_t n_slots, const typename P::In &in, int mode, const int64_t *leg_offsets, int64_t total_samples,
              double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg, Stage &&stage = Stage())
{
    int64_t first = 0, last = 0;
    const int rc = table_ends(c, leg_offsets, n_slots, &first, &last);
    if (rc) return rc;
    if (first != 0 || last != total_samples) return fail(FCPP_ESIZE, "leg_offsets do not span [0, total_samples]");
    DevBuf<typename P::Leg> legs;
    HIPCHK(legs.alloc((size_t)n_slots));
    LAUNCHCHK(launch_legs(c->stream, n_groups, n_slots, in, mode, legs.p, nullptr, nullptr, nullptr));
    LAUNCHCHK(stage(c->stream, legs.p, (int64_t *)nullptr, (const int32_t *)nullptr));
    LAUNCHCHK(launch_leg_fill<P>(c->stream, n_slots, legs.p, leg_offsets, total_samples, in.R, in.spacing, x, y, heading, kappa, part, gear, leg));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the records die here)
    return FCPP_OK;
}

// fcpp_debug_*: group(g, legs, cnt, t, oversize) -> status is the rule's host twin of one group (its records, its counts -- in off, one
// slot ahead: scanned below -- and its totals); groups go to the library's host threads.  `in` holds host pointers.
template <class P, class Group>
int legs_host(int64_t n_groups, int64_t n_slots, const typename P::In &in, const char *esize, Group group, int64_t *path_offsets, int64_t *leg_offsets,
              const LegTotals &totals, int32_t *status, int32_t *leg_kind, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap, double *x,
              double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    std::vector<typename P::Leg> legs;
    std::vector<int64_t> off;
    std::vector<char> big;
    try {
        legs.resize((size_t)n_slots); off.assign((size_t)n_slots + 1, 0); big.assign((size_t)n_groups, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    WorkerPool::parallel_for(n_groups, [&](int64_t g) {
        const int64_t first = P::first_slot(in, g);
        double t[P::N_TOTALS];
        bool oversize;
        const int st = group(g, legs.data() + first, off.data() + first + 1, t, oversize);
        big[(size_t)g] = oversize;
        store(status, g, st);
        for (int k = 0; k < P::N_TOTALS; ++k)
            if (totals.p[k]) totals.p[k][g] = t[k];
    });
    for (int64_t g = 0; g < n_groups; ++g)
        if (big[(size_t)g]) return fail(FCPP_ESIZE, esize);
    for (int64_t p = 0; p < n_slots; ++p) {
        off[(size_t)p + 1] += off[(size_t)p];
        const FpathLeg &lg = P::base(legs[(size_t)p]);
        store(leg_kind, p, lg.kind); store(leg_word, p, lg.kind == FPATH_DUBINS || lg.kind == FPATH_RS ? lg.word : -1);
        if (leg_seg) for (int k = 0; k < 5; ++k) leg_seg[5 * p + k] = lg.seg[k];
        store(leg_total, p, lg.total);
    }
    if (leg_offsets) memcpy(leg_offsets, off.data(), off.size() * sizeof(int64_t));
    if (path_offsets) {
        for (int64_t g = 0; g < n_groups; ++g) path_offsets[g] = off[(size_t)P::first_slot(in, g)];
        path_offsets[n_groups] = off[(size_t)n_slots];
    }
    if (cap == 0 || !(x || y || heading || kappa || part || gear || leg)) return FCPP_OK;
    WorkerPool::parallel_for(n_groups, [&](int64_t g) {
        for (int64_t p = P::first_slot(in, g); p < P::first_slot(in, g + 1); ++p) {
            const typename P::Leg &lg = legs[(size_t)p];
            const int64_t at = off[(size_t)p], K = off[(size_t)p + 1] - at;
            for (int64_t k = 0; k < K && at + k < cap; ++k) {
                double px, py, ph, pk;
                int pg;
                P::eval(lg, in.R, in.spacing, k, K, px, py, ph, pk, pg);
                store(x, at + k, px); store(y, at + k, py); store(heading, at + k, ph); store(kappa, at + k, pk);
                store(part, at + k, (int8_t)P::base(lg).part); store(gear, at + k, (int8_t)pg); store(leg, at + k, P::base(lg).slot);
            }
        }
    });
    return FCPP_OK;
}

// ---- the clear field paths: what the records go through between the rule kernel and the scan (kernels: fcpp_solveclear.hip) -----------------
// First pass, the list's length read back, the second pass unless it is 0, then (a counts call) the per-slot and per-field reports.  The
// fill passes no outputs: records only.  The buffers live in the stage, which outlives the entry's last synchronisation.
struct FpathClearStage {
    fcpp_ctx *c;
    int mode;
    int64_t n, n_total;
    FpathIn in;
    ClearFields F;
    int32_t *rank = nullptr, *crossings = nullptr, *leg_word = nullptr;
    double *leg_seg = nullptr, *leg_total = nullptr;
    int32_t *blocked = nullptr, *reshaped = nullptr, *region_status = nullptr;
    DevBuf<int64_t> list;
    DevBuf<unsigned long long> count;
    DevBuf<int32_t> own_rank;

    int operator()(hipStream_t st, FpathLeg *legs, int64_t *cnt, const int32_t *status)
    {
        const int64_t n_conn = n_total + n, n_slots = 2 * n_total + n;
        c->fpath_clear_listed = 0;
        if (n <= 0) return 0;
        hipError_t e = (hipError_t)launch_clear_field_status(st, F, region_status);
        if (e == hipSuccess) e = list.alloc((size_t)n_conn);
        if (e == hipSuccess) e = count.alloc(1);
        if (e == hipSuccess && !rank && (blocked || reshaped)) { e = own_rank.alloc((size_t)n_slots); rank = own_rank.p; }
        if (e == hipSuccess) e = hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st);
        if (e == hipSuccess && rank) e = hipMemsetAsync(rank, 0, (size_t)n_slots * sizeof(int32_t), st);
        if (e == hipSuccess && crossings) e = hipMemsetAsync(crossings, 0, (size_t)n_slots * sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
        int rc = launch_fpath_clear_slots(st, mode, n, n_conn, in.soff, in.R, legs, status, F, rank, crossings, list.p, count.p);
        if (rc) return rc;
        unsigned long long listed = 0;
        e = hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        if (listed > (unsigned long long)n_conn) return (int)hipErrorUnknown;      // (more slots listed than there are)
        c->fpath_clear_listed = (int64_t)listed;
        if (listed > 0) {
            rc = launch_fpath_clear_words(st, mode, (int64_t)listed, list.p, in, F, legs, cnt, rank, crossings);
            if (rc) return rc;
            ++c->fpath_clear_word_launches;
        }
        return launch_fpath_clear_report(st, n, n_slots, in.soff, legs, rank, leg_word, leg_seg, leg_total, blocked, reshaped);
    }
};

// the region CSR of the clear field paths: what fcpp_conn_clear checks of its fields, for n fields
int fpath_region_args(int64_t n, const void *ring_offsets, int64_t n_rings, const void *vert_offsets, int64_t n_verts, const double *x, const double *y)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y))) return fail(FCPP_EINVAL, "bad arguments");
    if (n < 0 || n_rings < 0 || n_verts < 0) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

// ---- loop transits (fcpp_transit.hip; the rule: fcpp_transitfn.h) -------------------------------------------------------------------------
// what the loop-transit entries and the host twin check alike of their loop set, before the offsets
int transit_loop_args(int64_t n_loops, const void *loop_offsets, int64_t n_samples, bool arrays)
{
    if (!loop_offsets || (n_samples > 0 && !arrays)) return fail(FCPP_EINVAL, "bad arguments");
    if (n_loops < 0 || n_samples < 0 || n_loops > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

int transit_solve_args(int mode, int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty, const double *th,
                       double radius, const int64_t *pair_field, int64_t n_fields, const void *ring_offsets, int64_t n_rings, const void *vert_offsets,
                       int64_t n_verts, const double *x, const double *y, int64_t n_loops, const void *loop_offsets, int64_t n_samples, bool arrays,
                       const void *field_loops, int64_t stride)
{
    int rc = solve_clear_args(mode, n, fx, fy, fh, tx, ty, th, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc == FCPP_OK) rc = transit_loop_args(n_loops, loop_offsets, n_samples, arrays);
    if (rc) return rc;
    if (!field_loops) return fail(FCPP_EINVAL, "bad arguments");
    if (stride < 1) return fail(FCPP_EINVAL, "stride must be at least 1");
    return FCPP_OK;
}

bool transit_rec_args(int64_t n, const TransitRec &rec)
{
    return n <= 0 || (rec.found && rec.loop && rec.i && rec.j && rec.in_word && rec.in_seg && rec.out_word && rec.out_seg);
}
}  // namespace

extern "C" {

// ---- field paths and headland paths (fcpp_legs.hip; the rules: fcpp_fpathfn.h, fcpp_hpathfn.h): argument checks, then the leg paths' skeleton ----
int fcpp_field_path_counts(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                           const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                           const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                           const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h, int64_t *path_offsets,
                           int64_t *path_offsets_host, int64_t *leg_offsets, double *work_length, double *transit_length, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!path_offsets || !leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    return legs_counts<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, n_total, in, mode, "a leg or a field has 2^31 samples or more", path_offsets,
                                  path_offsets_host, leg_offsets, { { work_length, transit_length, nullptr } }, status);
}

int fcpp_field_path_fill(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                         const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                         const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                         const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h, const int64_t *leg_offsets,
                         int64_t total_samples, double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK && (total_samples < 0 || total_samples > ((int64_t)1 << 38))) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    return legs_fill<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, in, mode, leg_offsets, total_samples, x, y, heading, kappa, part, gear, leg);
}

int fcpp_debug_field_paths(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                           const double *by, const double *length, const double *angle, const int32_t *order, double radius, int mode,
                           double spacing, const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x,
                           const double *exit_y, const double *exit_h, int64_t *path_offsets, int64_t *leg_offsets, double *work_length,
                           double *transit_length, int32_t *status, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap,
                           double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> soff;
    rc = fpath_offsets(nullptr, n, swath_offsets, nullptr, n_total, angle, nullptr, soff);
    if (rc) return rc;
    const FpathIn in = { soff.data(), ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    std::vector<int32_t> seen;
    try { seen.assign((size_t)n_total, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    return legs_host<FieldLegs>(n, n > 0 ? 2 * n_total + n : 0, in, "a leg or a field has 2^31 samples or more",
                                [&](int64_t i, FpathLeg *legs, int64_t *cnt, double *t, bool &oversize) {
                                    int32_t *sn = seen.data() + soff[(size_t)i];
                                    return mode == 0 ? fpath_field_host<0>(in, i, legs, cnt, sn, t[0], t[1], oversize)
                                                     : fpath_field_host<1>(in, i, legs, cnt, sn, t[0], t[1], oversize);
                                },
                                path_offsets, leg_offsets, { { work_length, transit_length, nullptr } }, status, nullptr, leg_word, leg_seg, leg_total, cap,
                                x, y, heading, kappa, part, gear, leg);
}

// ---- the clear field paths: the entries above with the region CSR and the stage between the records and the scan ----------------------------
int fcpp_field_path_counts_clear(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                                 const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                                 const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                                 const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h,
                                 const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                 const double *y, int64_t *path_offsets, int64_t *path_offsets_host, int64_t *leg_offsets, double *work_length,
                                 double *transit_length, int32_t *status, int32_t *leg_rank, int32_t *leg_crossings, int32_t *leg_word,
                                 double *leg_seg, double *leg_total, int32_t *blocked, int32_t *reshaped, int32_t *region_status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!path_offsets || !leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK) rc = fpath_region_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, rings, verts;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    FpathClearStage stage = { c, mode, n, n_total, in, { n, ring_offsets, vert_offsets, x, y } };
    stage.rank = leg_rank; stage.crossings = leg_crossings; stage.leg_word = leg_word; stage.leg_seg = leg_seg; stage.leg_total = leg_total;
    stage.blocked = blocked; stage.reshaped = reshaped; stage.region_status = region_status;
    return legs_counts<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, n_total, in, mode, "a leg or a field has 2^31 samples or more", path_offsets,
                                  path_offsets_host, leg_offsets, { { work_length, transit_length, nullptr } }, status, stage);
}

int fcpp_field_path_fill_clear(fcpp_ctx *c, int64_t n, const int64_t *swath_offsets, const int64_t *swath_offsets_host, int64_t n_total,
                               const double *ax, const double *ay, const double *bx, const double *by, const double *length, const double *angle,
                               const int32_t *order, double radius, int mode, double spacing, const double *entry_x, const double *entry_y,
                               const double *entry_h, const double *exit_x, const double *exit_y, const double *exit_h,
                               const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *rx,
                               const double *ry, const int64_t *leg_offsets, int64_t total_samples, double *x, double *y, double *heading,
                               double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK) rc = fpath_region_args(n, ring_offsets, n_rings, vert_offsets, n_verts, rx, ry);
    if (rc == FCPP_OK && (total_samples < 0 || total_samples > ((int64_t)1 << 38))) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> soff, rings, verts;
    rc = fpath_offsets(c, n, swath_offsets, swath_offsets_host, n_total, angle, nullptr, soff);
    if (rc == FCPP_OK) rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const FpathIn in = { swath_offsets, ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    FpathClearStage stage = { c, mode, n, n_total, in, { n, ring_offsets, vert_offsets, rx, ry } };
    return legs_fill<FieldLegs>(c, n, n > 0 ? 2 * n_total + n : 0, in, mode, leg_offsets, total_samples, x, y, heading, kappa, part, gear, leg, stage);
}

int fcpp_ctx_field_path_clear_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->fpath_clear_listed;
    if (word_launches) *word_launches = c->fpath_clear_word_launches;
    return FCPP_OK;
}

int fcpp_debug_field_paths_clear(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                 const double *by, const double *length, const double *angle, const int32_t *order, double radius, int mode,
                                 double spacing, const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x,
                                 const double *exit_y, const double *exit_h, const int64_t *ring_offsets, int64_t n_rings,
                                 const int64_t *vert_offsets, int64_t n_verts, const double *rx, const double *ry, int64_t *path_offsets,
                                 int64_t *leg_offsets, double *work_length, double *transit_length, int32_t *status, int32_t *leg_rank,
                                 int32_t *leg_crossings, int32_t *leg_word, double *leg_seg, double *leg_total, int32_t *blocked,
                                 int32_t *reshaped, int32_t *region_status, int64_t cap, double *x, double *y, double *heading, double *kappa,
                                 int8_t *part, int8_t *gear, int32_t *leg)
{
    int rc = fpath_args(n, swath_offsets, n_total, ax, ay, bx, by, length, angle, radius, mode, spacing, entry_x, entry_y, entry_h, exit_x, exit_y,
                        exit_h);
    if (rc == FCPP_OK) rc = fpath_region_args(n, ring_offsets, n_rings, vert_offsets, n_verts, rx, ry);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> soff, rings, verts;
    rc = fpath_offsets(nullptr, n, swath_offsets, nullptr, n_total, angle, nullptr, soff);
    if (rc == FCPP_OK) rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    const FpathIn in = { soff.data(), ax, ay, bx, by, length, angle, order, radius, spacing, entry_x, entry_y, entry_h, exit_x, exit_y, exit_h };
    const ClearFields F = { n, ring_offsets, vert_offsets, rx, ry };
    const int64_t n_slots = n > 0 ? 2 * n_total + n : 0;
    std::vector<int32_t> seen, rank, cross;
    try {
        seen.assign((size_t)n_total, 0); rank.assign((size_t)n_slots, 0); cross.assign((size_t)n_slots, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (region_status) WorkerPool::parallel_for(n, [&](int64_t f) { region_status[f] = clear_field_status(F, f); });
    rc = legs_host<FieldLegs>(n, n_slots, in, "a leg or a field has 2^31 samples or more",
                              [&](int64_t i, FpathLeg *legs, int64_t *cnt, double *t, bool &oversize) {
                                  int32_t *sn = seen.data() + soff[(size_t)i];
                                  int32_t *rk = rank.data() + fpath_first_slot(soff.data(), i), *cr = cross.data() + fpath_first_slot(soff.data(), i);
                                  int32_t b, r;
                                  const int st = mode == 0 ? fpath_field_clear_host<0>(in, F, i, legs, cnt, sn, rk, cr, b, r, t[0], t[1], oversize)
                                                           : fpath_field_clear_host<1>(in, F, i, legs, cnt, sn, rk, cr, b, r, t[0], t[1], oversize);
                                  store(blocked, i, b); store(reshaped, i, r);
                                  return st;
                              },
                              path_offsets, leg_offsets, { { work_length, transit_length, nullptr } }, status, nullptr, leg_word, leg_seg, leg_total, cap,
                              x, y, heading, kappa, part, gear, leg);
    if (rc) return rc;
    if (leg_rank && n_slots > 0) memcpy(leg_rank, rank.data(), rank.size() * sizeof(int32_t));
    if (leg_crossings && n_slots > 0) memcpy(leg_crossings, cross.data(), cross.size() * sizeof(int32_t));
    return FCPP_OK;
}

int fcpp_headland_path_counts(fcpp_ctx *c, int64_t n_rings, const int64_t *ring_offsets, const int64_t *ring_offsets_host, int64_t n_verts,
                              const double *x, const double *y, const int32_t *src, const double *ring_dist, double radius, int mode,
                              double spacing, int direction, double smooth_tol, int64_t *path_offsets, int64_t *path_offsets_host,
                              int64_t *leg_offsets, double *work_length, double *transit_length, double *skipped_length, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!path_offsets || !leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = hpath_args(n_rings, ring_offsets, n_verts, x, y, src, ring_dist, radius, mode, spacing, direction, smooth_tol);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> roff;
    rc = host_offsets(c, n_rings, ring_offsets, ring_offsets_host, n_verts, "ring_offsets", roff);
    if (rc) return rc;
    const HpathIn in = { ring_offsets, x, y, src, ring_dist, radius, spacing, smooth_tol, direction };
    return legs_counts<RingLegs>(c, n_rings, n_rings > 0 ? 2 * n_verts : 0, n_rings, in, mode, "a leg or a ring has 2^31 samples or more", path_offsets,
                                 path_offsets_host, leg_offsets, { { work_length, transit_length, skipped_length } }, status);
}

int fcpp_headland_path_fill(fcpp_ctx *c, int64_t n_rings, const int64_t *ring_offsets, const int64_t *ring_offsets_host, int64_t n_verts,
                            const double *x, const double *y, const int32_t *src, const double *ring_dist, double radius, int mode, double spacing,
                            int direction, double smooth_tol, const int64_t *leg_offsets, int64_t total_samples, double *out_x, double *out_y,
                            double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!leg_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = hpath_args(n_rings, ring_offsets, n_verts, x, y, src, ring_dist, radius, mode, spacing, direction, smooth_tol);
    if (rc == FCPP_OK && (total_samples < 0 || total_samples > ((int64_t)1 << 38))) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> roff;
    rc = host_offsets(c, n_rings, ring_offsets, ring_offsets_host, n_verts, "ring_offsets", roff);
    if (rc) return rc;
    const HpathIn in = { ring_offsets, x, y, src, ring_dist, radius, spacing, smooth_tol, direction };
    return legs_fill<RingLegs>(c, n_rings, n_rings > 0 ? 2 * n_verts : 0, in, mode, leg_offsets, total_samples, out_x, out_y, heading, kappa, part, gear,
                               leg);
}

int fcpp_debug_headland_paths(int64_t n_rings, const int64_t *ring_offsets, int64_t n_verts, const double *x, const double *y, const int32_t *src,
                              const double *ring_dist, double radius, int mode, double spacing, int direction, double smooth_tol,
                              int64_t *path_offsets, int64_t *leg_offsets, double *work_length, double *transit_length, double *skipped_length,
                              int32_t *status, int32_t *leg_kind, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap, double *out_x,
                              double *out_y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg)
{
    int rc = hpath_args(n_rings, ring_offsets, n_verts, x, y, src, ring_dist, radius, mode, spacing, direction, smooth_tol);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> roff;
    rc = host_offsets(nullptr, n_rings, ring_offsets, nullptr, n_verts, "ring_offsets", roff);
    if (rc) return rc;
    const HpathIn in = { roff.data(), x, y, src, ring_dist, radius, spacing, smooth_tol, direction };
    return legs_host<RingLegs>(n_rings, n_rings > 0 ? 2 * n_verts : 0, in, "a leg or a ring has 2^31 samples or more",
                               [&](int64_t r, HpathLeg *legs, int64_t *cnt, double *t, bool &oversize) {
                                   return mode == 0 ? hpath_ring_host<0>(in, r, legs, cnt, t[0], t[1], t[2], oversize)
                                                    : hpath_ring_host<1>(in, r, legs, cnt, t[0], t[1], t[2], oversize);
                               },
                               path_offsets, leg_offsets, { { work_length, transit_length, skipped_length } }, status, leg_kind, leg_word, leg_seg, leg_total,
                               cap, out_x, out_y, heading, kappa, part, gear, leg);
}

int fcpp_loop_transit_solve(fcpp_ctx *c, int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                            const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                            const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y,
                            int64_t n_loops, const int64_t *loop_offsets, const int64_t *loop_offsets_host, int64_t n_samples, const double *loop_x,
                            const double *loop_y, const double *loop_h, const double *loop_s, const int8_t *loop_part, const int8_t *loop_gear,
                            const int64_t *field_loops, const int64_t *field_loops_host, int64_t stride, int32_t *found, int64_t *loop, int64_t *st_i,
                            int64_t *st_j, int32_t *in_word, double *in_seg, double *in_len, int32_t *in_rank, int32_t *out_word, double *out_seg,
                            double *out_len, int32_t *out_rank, double *ride, double *total, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    int rc = transit_solve_args(mode, n, from_x, from_y, from_h, to_x, to_y, to_h, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets,
                                n_verts, x, y, n_loops, loop_offsets ? (const void *)loop_offsets : (const void *)loop_offsets_host, n_samples,
                                loop_x && loop_y && loop_h && loop_s && loop_part && loop_gear,
                                field_loops ? (const void *)field_loops : (const void *)field_loops_host, stride);
    if (rc) return rc;
    if (!loop_offsets || !field_loops) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<int64_t> rings, verts, loff, floops;
    rc = swath_fields(c, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(c, n_loops, loop_offsets, loop_offsets_host, n_samples, "loop_offsets", loff);
    if (rc == FCPP_OK) rc = host_offsets(c, n_fields, field_loops, field_loops_host, n_loops, "field_loops", floops);
    if (rc) return rc;
    c->transit_listed = 0;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    const TransitLoops L = { n_fields, n_loops, field_loops, loop_offsets, loop_x, loop_y, loop_h, nullptr, loop_s, loop_part, loop_gear, stride };
    const TransitIo io = { from_x, from_y, from_h, to_x, to_y, to_h, pair_field, found, loop, st_i, st_j, in_word, in_seg, in_len, in_rank,
                           out_word, out_seg, out_len, out_rank, ride, total, status };
    if (n <= 0) return FCPP_OK;
    DevBuf<int64_t> st_idx, st_loop, n_st, pick_l, pick_i, pick_j, list;
    DevBuf<int32_t> loops_ok, region_status;
    DevBuf<double> val;
    DevBuf<unsigned long long> count;
    HIPCHK(st_idx.alloc((size_t)n_samples));
    HIPCHK(st_loop.alloc((size_t)n_samples));
    HIPCHK(n_st.alloc((size_t)n_fields));
    HIPCHK(loops_ok.alloc((size_t)n_fields));
    HIPCHK(region_status.alloc((size_t)n_fields));
    HIPCHK(pick_l.alloc((size_t)n));
    HIPCHK(pick_i.alloc((size_t)n));
    HIPCHK(pick_j.alloc((size_t)n));
    HIPCHK(count.alloc(1));
    TransitTemp T = { st_idx.p, st_loop.p, n_st.p, loops_ok.p, region_status.p, nullptr, pick_l.p, pick_i.p, pick_j.p };
    LAUNCHCHK(launch_clear_field_status(st, F, region_status.p));
    LAUNCHCHK(launch_transit_stations(st, L, T));
    // the station counts come back: the stations pass's grid is sized by the largest a pair can use
    std::vector<int64_t> nst;
    try { nst.assign((size_t)n_fields, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    if (n_fields > 0) HIPCHK(hipMemcpyAsync(nst.data(), n_st.p, (size_t)n_fields * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t most = 0;
    for (int64_t f = 0; f < n_fields; ++f) most = std::max(most, std::min<int64_t>(nst[(size_t)f], TRANSIT_MAX_STATIONS));
    const int64_t per = (most + TRANSIT_BLOCK - 1) / TRANSIT_BLOCK * TRANSIT_BLOCK;
    if (per > 0 && n > (((int64_t)1 << 36) / (2 * per))) return fail(FCPP_ESIZE, "2^36 (pair, side, station) items or more");
    const int64_t items = n * 2 * per;
    if (items > 0) {
        HIPCHK(val.alloc((size_t)items));
        HIPCHK(list.alloc((size_t)items));
        T.val = val.p;
        HIPCHK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st));
        LAUNCHCHK(launch_transit_sides(st, mode, n, per, io, radius, F, L, T, list.p, count.p));
        unsigned long long listed = 0;
        HIPCHK(hipMemcpyAsync(&listed, count.p, sizeof listed, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (listed > (unsigned long long)items) return fail(FCPP_EHIP, "the first pass listed more items than there are");
        c->transit_listed = (int64_t)listed;
        if (listed > 0) {
            LAUNCHCHK(launch_transit_words(st, mode, (int64_t)listed, list.p, n, per, io, radius, F, L, T));
            ++c->transit_word_launches;
        }
    }
    LAUNCHCHK(launch_transit_pick(st, n, per, io, L, T));
    LAUNCHCHK(launch_transit_finish(st, mode, n, io, radius, F, L, T));
    HIPCHK(hipStreamSynchronize(st));          // (the temporaries die here)
    return FCPP_OK;
}

int fcpp_ctx_loop_transit_passes(const fcpp_ctx *c, int64_t *listed, int64_t *word_launches)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (listed) *listed = c->transit_listed;
    if (word_launches) *word_launches = c->transit_word_launches;
    return FCPP_OK;
}

int fcpp_loop_transit_counts(fcpp_ctx *c, int mode, int64_t n, const int32_t *found, const int64_t *loop, const int64_t *st_i, const int64_t *st_j,
                             const int32_t *in_word, const double *in_seg, const int32_t *out_word, const double *out_seg, int64_t n_loops,
                             const int64_t *loop_offsets, const int64_t *loop_offsets_host, int64_t n_samples, double spacing,
                             int64_t *path_offsets, int64_t *path_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    const TransitRec rec = { found, loop, st_i, st_j, in_word, in_seg, out_word, out_seg };
    int rc = leg_spacing(1.0, mode, spacing);
    if (rc == FCPP_OK) rc = transit_loop_args(n_loops, loop_offsets, n_samples, true);
    if (rc) return rc;
    if (!transit_rec_args(n, rec) || !path_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> loff;
    rc = host_offsets(c, n_loops, loop_offsets, loop_offsets_host, n_samples, "loop_offsets", loff);
    if (rc) return rc;
    return sample_counts(c, n, path_offsets, path_offsets_host, "a transit has 2^31 samples or more", [&](hipStream_t st, int64_t *err) {
        return launch_transit_counts(st, mode, n, rec, n_loops, loop_offsets, spacing, path_offsets, err);
    });
}

int fcpp_loop_transit_fill(fcpp_ctx *c, int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, double radius,
                           const int32_t *found, const int64_t *loop, const int64_t *st_i, const int64_t *st_j, const int32_t *in_word,
                           const double *in_seg, const int32_t *out_word, const double *out_seg, int64_t n_loops, const int64_t *loop_offsets,
                           const int64_t *loop_offsets_host, int64_t n_samples, const double *loop_x, const double *loop_y, const double *loop_h,
                           const double *loop_kappa, const int8_t *loop_gear, double spacing, const int64_t *path_offsets,
                           const int64_t *path_offsets_host, int64_t total_samples, double *out_x, double *out_y, double *heading, double *kappa,
                           int8_t *part, int8_t *gear)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    const TransitRec rec = { found, loop, st_i, st_j, in_word, in_seg, out_word, out_seg };
    int rc = leg_spacing(radius, mode, spacing);
    if (rc == FCPP_OK) rc = transit_loop_args(n_loops, loop_offsets, n_samples, loop_x && loop_y && loop_h && loop_kappa && loop_gear);
    if (rc) return rc;
    if (!transit_rec_args(n, rec) || !path_offsets || (n > 0 && (!from_x || !from_y || !from_h))) return fail(FCPP_EINVAL, "bad arguments");
    if (n < 0 || n > INT32_MAX || total_samples < 0 || total_samples > ((int64_t)1 << 38)) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> loff;
    rc = host_offsets(c, n_loops, loop_offsets, loop_offsets_host, n_samples, "loop_offsets", loff);
    if (rc) return rc;
    SampleOffsets outs;
    rc = outs.get(c, n, path_offsets, path_offsets_host, total_samples, "path_offsets", true);
    if (rc) return rc;
    const TransitLoops L = { 0, n_loops, nullptr, loop_offsets, loop_x, loop_y, loop_h, loop_kappa, nullptr, nullptr, loop_gear, 1 };
    LAUNCHCHK(launch_transit_fill(c->stream, mode, n, rec, L, from_x, from_y, from_h, radius, spacing, outs.dev, total_samples, out_x, out_y, heading,
                                  kappa, part, gear));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_loop_transits(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                             const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                             const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y,
                             int64_t n_loops, const int64_t *loop_offsets, int64_t n_samples, const double *loop_x, const double *loop_y,
                             const double *loop_h, const double *loop_kappa, const double *loop_s, const int8_t *loop_part, const int8_t *loop_gear,
                             const int64_t *field_loops, int64_t stride, double spacing, int32_t *found, int64_t *loop, int64_t *st_i, int64_t *st_j,
                             int32_t *in_word, double *in_seg, double *in_len, int32_t *in_rank, int32_t *out_word, double *out_seg, double *out_len,
                             int32_t *out_rank, double *ride, double *total, int32_t *status, int64_t *path_offsets, int64_t cap, double *out_x,
                             double *out_y, double *heading, double *kappa, int8_t *part, int8_t *gear)
{
    int rc = transit_solve_args(mode, n, from_x, from_y, from_h, to_x, to_y, to_h, radius, pair_field, n_fields, ring_offsets, n_rings, vert_offsets,
                                n_verts, x, y, n_loops, loop_offsets, n_samples, loop_x && loop_y && loop_h && loop_kappa && loop_s && loop_part && loop_gear,
                                field_loops, stride);
    if (rc == FCPP_OK) rc = leg_spacing(radius, mode, spacing);
    if (rc == FCPP_OK && cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> rings, verts, loff, floops;
    rc = swath_fields(nullptr, n_fields, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(nullptr, n_loops, loop_offsets, nullptr, n_samples, "loop_offsets", loff);
    if (rc == FCPP_OK) rc = host_offsets(nullptr, n_fields, field_loops, nullptr, n_loops, "field_loops", floops);
    if (rc) return rc;
    const ClearFields F = { n_fields, ring_offsets, vert_offsets, x, y };
    const TransitLoops L = { n_fields, n_loops, field_loops, loop_offsets, loop_x, loop_y, loop_h, loop_kappa, loop_s, loop_part, loop_gear, stride };
    const int nseg = mode == 0 ? 3 : 5;
    // per field: the region's status, the loops' validity, the stations (at the place of the field's first sample)
    std::vector<int32_t> region_status, loops_ok;
    std::vector<int64_t> n_st, st_idx, st_loop, cnt;
    std::vector<TransitResult> res;
    try {
        region_status.assign((size_t)n_fields, 0); loops_ok.assign((size_t)n_fields, 0); n_st.assign((size_t)n_fields, 0);
        st_idx.assign((size_t)n_samples, 0); st_loop.assign((size_t)n_samples, 0); cnt.assign((size_t)n + 1, 0); res.resize((size_t)n);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    WorkerPool::parallel_for(n_fields, [&](int64_t f) {
        region_status[(size_t)f] = clear_field_status(F, f);
        loops_ok[(size_t)f] = transit_field_loops_ok(L, f) ? 1 : 0;
        const int64_t base = field_loops[f + 1] > field_loops[f] ? loop_offsets[field_loops[f]] : 0;
        n_st[(size_t)f] = transit_field_stations(L, f, st_idx.data() + base, st_loop.data() + base);
    });
    std::vector<char> big((size_t)n, 0), nomem((size_t)n, 0);
    WorkerPool::parallel_for(n, [&](int64_t p) {
        const int64_t f = pair_field[p];
        const double x0 = from_x[p], y0 = from_y[p], h0 = from_h[p], x1 = to_x[p], y1 = to_y[p], h1 = to_h[p];
        const int stt = transit_pair_status(x0, y0, h0, x1, y1, h1, f, n_fields, region_status.data(), loops_ok.data(), n_st.data());
        TransitPick pick = transit_pick_none();
        if (stt == TRANSIT_OK && n_st[(size_t)f] > 0) {
            const int64_t base = loop_offsets[field_loops[f]], m = n_st[(size_t)f];
            std::vector<double> in, out;
            try { in.assign((size_t)m, 0.0); out.assign((size_t)m, 0.0); } catch (const std::bad_alloc &) { nomem[(size_t)p] = 1; return; }
            pick = mode == 0 ? transit_pick_host<0>(F, L, f, x0, y0, h0, x1, y1, h1, radius, m, st_idx.data() + base, st_loop.data() + base, in.data(), out.data())
                             : transit_pick_host<1>(F, L, f, x0, y0, h0, x1, y1, h1, radius, m, st_idx.data() + base, st_loop.data() + base, in.data(), out.data());
        }
        const TransitResult r = mode == 0 ? transit_finish<0>(F, L, f, x0, y0, h0, x1, y1, h1, radius, stt, pick)
                                          : transit_finish<1>(F, L, f, x0, y0, h0, x1, y1, h1, radius, stt, pick);
        res[(size_t)p] = r;
        store(found, p, r.found); store(loop, p, r.loop); store(st_i, p, r.i); store(st_j, p, r.j); store(in_word, p, r.in.word);
        store(out_word, p, r.out.word);
        for (int k = 0; k < nseg; ++k) {
            store(in_seg, p * nseg + k, r.in.seg[k]); store(out_seg, p * nseg + k, r.out.seg[k]);
        }
        store(in_len, p, r.in.len); store(out_len, p, r.out.len); store(in_rank, p, r.in.rank); store(out_rank, p, r.out.rank);
        store(ride, p, r.ride); store(total, p, r.total); store(status, p, r.status);
    });
    for (int64_t p = 0; p < n; ++p)
        if (nomem[(size_t)p]) return fail(FCPP_ENOMEM, "out of host memory");
    if (!path_offsets && (cap == 0 || !(out_x || out_y || heading || kappa || part || gear))) return FCPP_OK;
    // the sampled paths, from the results as a caller would hand them back (one pair at a time: NSEG segments in place)
    auto rec_of = [&](const TransitResult &r, int32_t &fnd, int64_t *ids, int32_t *words) {
        fnd = r.found; ids[0] = r.loop; ids[1] = r.i; ids[2] = r.j; words[0] = r.in.word; words[1] = r.out.word;
        return TransitRec{ &fnd, ids, ids + 1, ids + 2, words, r.in.seg, words + 1, r.out.seg };
    };
    WorkerPool::parallel_for(n, [&](int64_t p) {
        int32_t fnd, words[2];
        int64_t ids[3], a, b, c2, bad = 0;
        const TransitRec rec = rec_of(res[(size_t)p], fnd, ids, words);
        if (mode == 0) transit_counts<0>(rec, n_loops, loop_offsets, spacing, 0, a, b, c2, bad);
        else transit_counts<1>(rec, n_loops, loop_offsets, spacing, 0, a, b, c2, bad);
        cnt[(size_t)p + 1] = a + b + c2;
        big[(size_t)p] = bad != 0;
    });
    for (int64_t p = 0; p < n; ++p) {
        if (big[(size_t)p]) return fail(FCPP_ESIZE, "a transit has 2^31 samples or more");
        cnt[(size_t)p + 1] += cnt[(size_t)p];
    }
    if (path_offsets) memcpy(path_offsets, cnt.data(), cnt.size() * sizeof(int64_t));
    if (cap == 0 || !(out_x || out_y || heading || kappa || part || gear)) return FCPP_OK;
    WorkerPool::parallel_for(n, [&](int64_t p) {
        int32_t fnd, words[2];
        int64_t ids[3];
        const TransitRec rec = rec_of(res[(size_t)p], fnd, ids, words);
        const int64_t at = cnt[(size_t)p], K = cnt[(size_t)p + 1] - at;
        for (int64_t k = 0; k < K && at + k < cap; ++k) {
            double px, py, ph, pk;
            int pp, pg;
            if (mode == 0) transit_eval<0>(rec, L, from_x + p, from_y + p, from_h + p, radius, spacing, 0, k, K, px, py, ph, pk, pp, pg);
            else transit_eval<1>(rec, L, from_x + p, from_y + p, from_h + p, radius, spacing, 0, k, K, px, py, ph, pk, pp, pg);
            store(out_x, at + k, px); store(out_y, at + k, py); store(heading, at + k, ph); store(kappa, at + k, pk); store(part, at + k, (int8_t)pp);
            store(gear, at + k, (int8_t)pg);
        }
    });
    return FCPP_OK;
}

}  // extern "C"
