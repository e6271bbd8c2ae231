// fcpp_setup.cpp -- the setup of a batch, fcpp_batch_create's and fcpp_batch_plan's work behind the C entries of fcpp_api.cpp: the turn templates,
// the setup on the DEVICE as a sequence of named phases over one record (DeviceSetup; its decisions: fcpp_setuprule.h), the host path (host plan,
// tiler, image, one copy), and the fill pass a direct setup left for later (flush_tables / ensure_tables).
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>

#include "fcpp_batch.h"
#include "fcpp_parallel.h"

using namespace fcpp;

namespace fcpp { thread_local double g_trace_totals_ms = 0.0; }

// Are the U-turns of this batch closed form?  A turn is a translate / mirror of the template t[0..nu); its neighbours are the
// swath line it leaves (whose last point is the turn's first: a skipped step, nothing propagates across it) and the next
// line, reached by a jump J from the turn's last sample.  If every sample keeps the nominal turn speed under the curvature
// clamp, the next line's first point keeps the work speed, and 2a|J| is too long for the sweeps to bind across the jump, then
// turn points are template + translation, curvature and segment lengths are the shape's own (dk), speeds are nominal.
// Fills the per-batch constants the quiet kernel and the run statistics need.  Index 0 / 1: passes ascending / descending in y.
static bool closed_form_turns(const fcpp_vehicle &veh, const TurnTemplates &tt, const std::vector<double2> &t,
                              const std::vector<double2> &dk, DevConst &c)
{
    const int nu = tt.nu;
    const double W = veh.working_width, R = veh.min_turn_radius;
    // the turn's first sample must be the line's last point: template offset 0 (clothoid: x = (max_x - R) + t.x) or R (arcs: x = max_x - t.x)
    if (nu < 3 || fabs(t[0].x - (tt.turn_model == FCPP_TURN_ARC ? R : 0.0)) > 1e-9 || fabs(t[0].y) > 1e-9) return false;
    const double q_t = c.v_turn * c.inv_sf36, q_w = c.v_work * c.inv_sf36, lim = c.a_lat * 0.999;
    double len = 0.0, maxk = 0.0, maxj = 0.0;
    for (int k = 1; k < nu; ++k) len += dk[(size_t)k].x;
    for (int k = 1; k + 1 < nu; ++k) {
        maxk = std::max(maxk, dk[(size_t)k].y);
        maxj = std::max(maxj, fabs(dk[(size_t)k].y - dk[(size_t)k - 1].y));
    }
    if (maxk * q_t * q_t >= lim) return false;
    // the turn's last chord in the frame of a right turn (world x grows to the right)
    const bool arc = tt.turn_model == FCPP_TURN_ARC;
    const double sx = arc ? -1.0 : 1.0;                    // arcs: px = max_x - t.x; clothoid: px = (max_x - R) + t.x
    const double c1x = sx * (t[(size_t)nu - 1].x - t[(size_t)nu - 2].x), c1y = t[(size_t)nu - 1].y - t[(size_t)nu - 2].y;
    const double d1 = sqrt(c1x * c1x + c1y * c1y);
    const double u_t = c.ms_turn * c.ms_turn, u_w = c.ms_work * c.ms_work;
    for (int v = 0; v < 2; ++v) {
        // jump to the first point of the next line: x back to max_x - R, y to the next pass (+W, or -W in top-down order)
        const double jx = arc ? (-R + t[(size_t)nu - 1].x) : -t[(size_t)nu - 1].x;
        const double jy = (v == 0 ? W : -W) - t[(size_t)nu - 1].y;
        const double dj = sqrt(jx * jx + jy * jy);
        if (!(dj >= 1e-3) || d1 < 1e-6) return false;
        if (u_t + 2 * c.a_lon * dj < u_w * (1.0 + 1e-9)) return false;          // the sweeps must not bind across the jump
        const double k_last = fabs(2 * atan2_fd(c1x * jy - c1y * jx, c1x * jx + c1y * jy) / (d1 + dj));
        // first point of the next line: chords J and the line heading (-x after a right turn); its curvature is largest for step -> 0
        const double k_first_max = fabs(2 * atan2_fd(jx * 0.0 - jy * -1.0, jx * -1.0 + jy * 0.0) / dj);
        if (k_last * q_t * q_t >= lim || k_first_max * q_w * q_w >= lim) return false;
        c.turn_kappa_last[v] = k_last;
        c.turn_jump[v] = dj;
        c.turn_max_kappa[v] = std::max(maxk, k_last);
        c.turn_max_jump[v] = std::max(std::max(maxj, fabs(dk[(size_t)nu - 2].y - (nu >= 3 ? dk[(size_t)nu - 3].y : 0.0))), fabs(k_last - dk[(size_t)nu - 2].y));
    }
    c.turn_len = len;
    c.turn_time = len / std::max(c.ms_turn, 0.1);
    return true;
}
// the constants of the closed-form cut (fcpp_cutfn.h) for a batch: the templates and their chord tables as the HOST copies or as the device
// arrays (the same values), the rest from the batch's constants (closed_form_turns has run)
static CutConsts make_cut_consts(TemplateSet &ts, bool device, const BatchTileConsts &k, const DevConst &cst)
{
    CutConsts cc;
    memset(&cc, 0, sizeof cc);
    ts.template_box();
    if (device) {
        cc.tu = reinterpret_cast<const Pt2 *>(ts.tmpl_u.p); cc.tc = reinterpret_cast<const Pt2 *>(ts.tmpl_c.p);
        cc.dk_u = reinterpret_cast<const Pt2 *>(ts.tmpl_u_dk.p); cc.dk_c = reinterpret_cast<const Pt2 *>(ts.tmpl_c_dk.p);
    } else {
        cc.tu = reinterpret_cast<const Pt2 *>(ts.h_tu.data()); cc.tc = reinterpret_cast<const Pt2 *>(ts.h_tc.data());
        cc.dk_u = reinterpret_cast<const Pt2 *>(ts.h_dk.data()); cc.dk_c = reinterpret_cast<const Pt2 *>(ts.h_dkc.data());
    }
    cc.nu = k.nu; cc.nc = k.nc; cc.turn_quiet = k.turn_quiet ? 1 : 0; cc.wave_factor = k.wave_factor;
    cc.two_a = k.two_a; cc.u_cap = k.u_cap; cc.c_line = k.c_line; cc.fence_margin = k.fence_margin;
    cc.jump[0] = cst.turn_jump[0]; cc.jump[1] = cst.turn_jump[1];
    for (int d = 0; d < 2; ++d) { cc.tc_lo[d] = ts.tc_lo[d]; cc.tc_hi[d] = ts.tc_hi[d]; }
    // the shortest chord of either template (host copies of the device's chord tables: the same values whichever side cuts)
    cc.u_step_min = cc.c_step_min = HUGE_VAL;
    for (size_t k = 1; k < ts.h_dk.size(); ++k) cc.u_step_min = std::min(cc.u_step_min, ts.h_dk[k].x);
    for (size_t k = 1; k < ts.h_dkc.size(); ++k) cc.c_step_min = std::min(cc.c_step_min, ts.h_dkc[k].x);
    if (ts.h_dk.size() < 2) cc.u_step_min = 0.0;
    if (ts.h_dkc.size() < 2) cc.c_step_min = 0.0;
    return cc;
}

namespace fcpp {
// Field records that live in DEVICE memory (round 5: a table kept on the GPU -- engine.FieldTable.to_device(), a caller whose fields are
// made there -- is read by the device-side setup where it lies, like pinned records, without crossing PCIe): the HOST paths (host plan,
// fcpp_plan_count, a batch the device planner hands back) read a copy.  -> `host` = fields, or copy.data()
int host_fields(const fcpp_field *fields, int64_t n_fields, std::vector<fcpp_field> &copy, const fcpp_field *&host)
{
    host = fields;
    if (n_fields <= 0 || !fields) return FCPP_OK;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, fields) != hipSuccess) { (void)hipGetLastError(); return FCPP_OK; }      // (pageable memory, or no GPU at all)
    if (at.type != hipMemoryTypeDevice) return FCPP_OK;
    try { copy.resize((size_t)n_fields); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    HIPCHK(hipMemcpy(copy.data(), fields, (size_t)n_fields * sizeof(fcpp_field), hipMemcpyDeviceToHost));
    host = copy.data();
    return FCPP_OK;
}
}  // namespace fcpp

// the context's turn templates for (tt, clothoid_frac): the kept set, or a new one sampled on the device (asynchronous: the caller
// synchronises the stream before it reads the host copies; `fresh` tells it to)
static int get_templates(fcpp_ctx *c, const TurnTemplates &tt, const fcpp_options &opt, hipStream_t st, std::shared_ptr<TemplateSet> &out, bool &fresh)
{
    fresh = false;
    if (c->templates && c->templates->same(tt, opt.clothoid_frac)) { out = c->templates; return FCPP_OK; }
    std::shared_ptr<TemplateSet> ts(new (std::nothrow) TemplateSet());
    if (!ts) return fail(FCPP_ENOMEM, "out of host memory");
    ts->tt = tt; ts->clothoid_frac = opt.clothoid_frac;
    const int nu = tt.nu, nc = tt.nc;
    std::vector<CacShape> shp = { make_cac_shape(kPi, opt.clothoid_frac), make_cac_shape(kHalfPi, opt.clothoid_frac) };
    HIPCHK(ts->shapes.upload(shp, st));
    HIPCHK(hipStreamSynchronize(st));             // (shp dies with this scope)
    HIPCHK(ts->tmpl_u.alloc((size_t)nu));
    HIPCHK(ts->tmpl_c.alloc((size_t)nc));
    HIPCHK(ts->tmpl_u_dk.alloc((size_t)nu));
    HIPCHK(ts->tmpl_c_dk.alloc((size_t)nc));
    LAUNCHCHK(launch_build_templates(st, tt, ts->shapes.p, ts->tmpl_u.p, ts->tmpl_c.p));
    LAUNCHCHK(launch_build_template_metrics(st, nu, ts->tmpl_u.p, ts->tmpl_u_dk.p));
    LAUNCHCHK(launch_build_template_metrics(st, nc, ts->tmpl_c.p, ts->tmpl_c_dk.p));
    ts->h_tu.resize((size_t)nu); ts->h_tc.resize((size_t)nc); ts->h_dk.resize((size_t)nu); ts->h_dkc.resize((size_t)nc);
    if (nu > 0) {
        HIPCHK(hipMemcpyAsync(ts->h_tu.data(), ts->tmpl_u.p, (size_t)nu * sizeof(double2), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ts->h_dk.data(), ts->tmpl_u_dk.p, (size_t)nu * sizeof(double2), hipMemcpyDeviceToHost, st));
    }
    if (nc > 0) {
        HIPCHK(hipMemcpyAsync(ts->h_tc.data(), ts->tmpl_c.p, (size_t)nc * sizeof(double2), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ts->h_dkc.data(), ts->tmpl_c_dk.p, (size_t)nc * sizeof(double2), hipMemcpyDeviceToHost, st));
    }
    out = ts;
    fresh = true;
    return FCPP_OK;
}

fcpp::SetupSwitches fcpp::SetupSwitches::read()
{
    SetupSwitches sw;
    const char *e_small = getenv("FCPP_SMALL_BATCH"), *e_direct = getenv("FCPP_DIRECT"), *e_fw = getenv("FCPP_FIELD_WORK"), *e_span = getenv("FCPP_DENSE_SPAN"),
               *e_chunks = getenv("FCPP_HOST_CHUNKS"), *e_rows = getenv("FCPP_CUT_ROWS");
    if (e_small) sw.small_batch = atoll(e_small);
    sw.exact_only = getenv("FCPP_SETUP_EXACT") != nullptr;
    sw.direct = !(e_direct && atoi(e_direct) == 0);
    sw.cut_rows = !(e_rows && atoi(e_rows) == 0);
    sw.field_work = !(e_fw && atoi(e_fw) == 0);
    sw.span_line_max = e_span && atoll(e_span) <= 0 ? 64 : INT64_MAX;
    sw.device_chunks = !(e_chunks && atoi(e_chunks) != 0);
    return sw;
}

namespace fcpp {
namespace {
// the batch's device allocation: the context's spare if it is large enough
int take_slab(fcpp_ctx *c, fcpp_batch *b, std::string &err)
{
    const ImageLayout &lay = b->lay;
    if (c->spare && c->spare_cap >= lay.total_bytes) { b->slab = c->spare; b->slab_bytes = c->spare_cap; c->spare = nullptr; c->spare_cap = 0; return FCPP_OK; }
    hipError_t e = hipMalloc(&b->slab, std::max<size_t>(lay.total_bytes, 256));
    if (e != hipSuccess) { b->slab = nullptr; err = std::string("batch tables: ") + hipGetErrorString(e); return FCPP_ENOMEM; }
    b->slab_bytes = std::max<size_t>(lay.total_bytes, 256);
    return FCPP_OK;
}

#define DEVCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return FCPP_EHIP; } \
    } while (0)

// Host memory for an upload of nb bytes: the context's pinned staging memory, reallocated with `want` bytes when it holds fewer than nb
// (whatever was being copied out of it drained first), or `pageable` when the upload is larger than kStageMax or pinned memory cannot be had
int upload_buffer(fcpp_ctx *c, size_t nb, size_t want, std::vector<unsigned char> &pageable, unsigned char *&img, std::string &err)
{
    img = nullptr;
    if (nb <= kStageMax) {
        DEVCHK(c->stage_wait());
        if (c->stage_cap < nb) {
            if (c->stage) { (void)hipHostFree(c->stage); c->stage = nullptr; c->stage_cap = 0; }
            if (hipHostMalloc(&c->stage, want, hipHostMallocDefault) == hipSuccess) c->stage_cap = want;
            else { c->stage = nullptr; (void)hipGetLastError(); }
        }
        if (c->stage_cap >= nb) img = static_cast<unsigned char *>(c->stage);
    }
    if (!img) {
        try { pageable.resize(nb); } catch (const std::bad_alloc &) { err = "out of host memory"; return FCPP_ENOMEM; }
        img = pageable.data();
    }
    return FCPP_OK;
}

// the batch's kernel constants, with its template set (on the host by now); true: its U-turns are closed form
bool set_batch_consts(fcpp_batch *b, const TemplateSet &ts)
{
    b->cst = make_const(b->veh, b->opt);
    b->cst.shapes = ts.shapes.p;
    b->cst.tmpl_u = ts.tmpl_u.p; b->cst.tmpl_c = ts.tmpl_c.p; b->cst.tmpl_u_dk = ts.tmpl_u_dk.p;
    b->cst.tmpl_n = (int)ts.tt.nu; b->cst.tmpl_nc = std::max(1, (int)ts.tt.nc);
    return ts.tt.nu >= 3 && closed_form_turns(b->veh, ts.tt, ts.h_tu, ts.h_dk, b->cst);
}
}  // namespace

// The fill pass a direct setup left out, on the setup's stream (behind the step): from the plan slot's scratch, which nobody has touched
// since -- counts, kept rows and the setup's buffer of aggregates are as the counting pass left them.  Does nothing for any other batch.
// `now`: the stream of the call that asks.  A setup stream the caller has destroyed since (as ev_plan and wait_setup allow for): whatever ran
// there is drained with the device, and the fill pass goes to `now`, which becomes the batch's setup stream.
int flush_tables(fcpp_batch *b, hipStream_t now, std::string &err)
{
    if (!b->tables_pending) return FCPP_OK;
    fcpp_ctx *c = b->ctx;
    b->tables_pending = false;
    fcpp_ctx::PlanSlot *sl = b->tables_slot >= 0 ? &c->plan_slots[b->tables_slot] : nullptr;
    if (sl && sl->tables_batch == b) sl->tables_batch = nullptr;
    b->cst.field_junc = b->t.field_junc;
    ++c->direct_fills;
    int frc = launch_devplan_fill(b->setup_stream, b->n_fields, b->tables_tc, b->cst, b->tables_scratch, b->t, nullptr);
    if (frc && now != b->setup_stream) {
        (void)hipGetLastError();
        if (hipDeviceSynchronize() != hipSuccess) { err = "the device after a batch's setup stream was destroyed"; return FCPP_EHIP; }
        if (sl && sl->stream == b->setup_stream) sl->stream = now;
        b->setup_stream = now; b->setup_seen.clear();
        b->note_stream(now);
        frc = launch_devplan_fill(now, b->n_fields, b->tables_tc, b->cst, b->tables_scratch, b->t, nullptr);
    }
    if (frc) { err = std::string("launch_devplan_fill: ") + hipGetErrorString((hipError_t)frc); return FCPP_EHIP; }
    return FCPP_OK;
}

// the context's planner scratch for n fields (grow-only), ordered behind the last fill pass that read it
int plan_scratch(fcpp_ctx *c, int64_t n_fields, int max_prims, hipStream_t st, DevPlanScratch &s, std::string &err)
{
    // the slot: this stream's, else an unused one, else the one used longest ago -- ordered behind whatever another stream left in it
    int k = -1;
    for (int i = 0; i < fcpp_ctx::kPlanSlots; ++i) if (c->plan_slots[i].p && c->plan_slots[i].stream == st) k = i;
    if (k < 0) for (int i = 0; i < fcpp_ctx::kPlanSlots; ++i) if (!c->plan_slots[i].p) { k = i; break; }
    if (k < 0) { k = 0; for (int i = 1; i < fcpp_ctx::kPlanSlots; ++i) if (c->plan_slots[i].tick < c->plan_slots[k].tick) k = i; }
    fcpp_ctx::PlanSlot &sl = c->plan_slots[k];
    // (a batch whose tables are still to be filled from this slot's scratch: its fill pass goes first, on the stream of its setup)
    if (sl.tables_batch) { const int frc = flush_tables(sl.tables_batch, st, err); if (frc != FCPP_OK) return frc; }
    if (sl.pending && sl.stream != st) {       // (that batch's fill pass, on another stream, may still read the scratch)
        if (!c->ev_plan) DEVCHK(hipEventCreateWithFlags(&c->ev_plan, hipEventDisableTiming));
        if (hipEventRecord(c->ev_plan, sl.stream) == hipSuccess) DEVCHK(hipStreamWaitEvent(st, c->ev_plan, 0));
        else { (void)hipGetLastError(); DEVCHK(hipDeviceSynchronize()); }        // (that stream is gone)
        sl.pending = false;
    }
    sl.stream = st; sl.tick = ++c->plan_tick;
    c->plan_cur = k;
    const size_t need = devplan_scratch_layout(n_fields, max_prims, nullptr, s);
    if (sl.cap < need) {
        if (sl.p) { DEVCHK(hipDeviceSynchronize()); (void)hipFree(sl.p); sl.p = nullptr; sl.cap = 0; }
        const size_t want = need + need / 4;
        if (hipMalloc(&sl.p, want) != hipSuccess) { (void)hipGetLastError(); sl.p = nullptr; err = "out of device memory for the planner's scratch"; return FCPP_ENOMEM; }
        sl.cap = want;
        // (the flags live at the start of the allocation and are never cleared again: they hold generation numbers; behind them the two
        // buffers of aggregates, zero from here on whenever a setup begins: SlotAggregates, fcpp_setuprule.h)
        DevPlanScratch head;
        devplan_scratch_layout(1, 1, sl.p, head);
        DEVCHK(hipMemsetAsync(sl.p, 0, (size_t)(reinterpret_cast<unsigned char *>(head.agg + 2 * (size_t)OFF_WORDS) - static_cast<unsigned char *>(sl.p)), st));
        static_cast<SlotAggregates &>(sl) = SlotAggregates();
    }
    if (!c->plan_totals_host)
        { DEVCHK(hipHostMalloc((void **)&c->plan_totals_host, PLAN_TOTALS * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent)); memset(c->plan_totals_host, 0, PLAN_TOTALS * sizeof(int64_t)); }
    devplan_scratch_layout(n_fields, max_prims, sl.p, s);
    return FCPP_OK;
}

// The field records as the device reaches them.  Records in pinned host memory (hipHostMalloc / hipHostRegister: a torch tensor with
// pin_memory, engine.FieldTable) are read by k_plan_fields where they lie -- the kernel's first load is the transfer, 128 bytes per
// thread, and no copy command goes before it; anything else is copied to the scratch first.  The callers drain the stream before they return, so
// the caller's memory is not touched afterwards either way.
int device_fields(const fcpp_field *fields, int64_t n_fields, hipStream_t st, const DevPlanScratch &s, const fcpp_field *&dev, std::string &err)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    void *dp = nullptr;
    if (hipPointerGetAttributes(&at, fields) == hipSuccess && at.type == hipMemoryTypeHost &&
        hipHostGetDevicePointer(&dp, const_cast<fcpp_field *>(fields), 0) == hipSuccess && dp) {
        dev = static_cast<const fcpp_field *>(dp);
        return FCPP_OK;
    }
    // (records in DEVICE memory: read where they lie when they are this context's device's, copied from the peer otherwise)
    int cur = -1;
    if (at.type == hipMemoryTypeDevice && hipGetDevice(&cur) == hipSuccess && at.device == cur) { dev = fields; return FCPP_OK; }
    (void)hipGetLastError();          // (pageable memory: "invalid value" on some runtimes, hipMemoryTypeUnregistered on others)
    DEVCHK(hipMemcpyAsync(s.fields_in, fields, (size_t)n_fields * sizeof(fcpp_field), at.type == hipMemoryTypeDevice ? hipMemcpyDefault : hipMemcpyHostToDevice, st));
    dev = s.fields_in;
    return FCPP_OK;
}

namespace {
// What the host tiler and the device tiler both derive from the batch (set_batch_consts has run), computed once.
void batch_tile_consts(const fcpp_batch &b, bool turn_quiet, bool field_work, int64_t span_line_max, BatchTileConsts &k)
{
    k.nu = b.templates->tt.nu; k.nc = b.templates->tt.nc;
    k.turn_quiet = turn_quiet;
    k.two_a = 2 * b.cst.a_lon; k.u_cap = b.cst.u_cap; k.c_line = b.cst.ms_work * b.cst.ms_work;
    // (the device flags a point whose edge function is below -geofence_tol; host and device evaluate a point by the same formulas and
    // differ by roundings of ~1e-12 m: 1e-7 m of slack is five orders of magnitude of safety -- and lets the points that lie ON the boundary,
    // the ends of the reverse fills, three per field of the metric's size, pass with the default tolerance of 1e-6 m: with the millimetre of margin
    // of rounds 2-3a those three points sent half of the headline's wave tiles through the geofence test)
    k.fence_margin = 1e-7 - b.opt.geofence_tol;
    k.fuse_spans = field_work && k.nu <= TMPL_LDS_SAMPLES;
    k.span_line_max = span_line_max;
}

// the device tiler's constants: the shared ones, the templates on the device, the kernels' fixed parameters
DevTileConsts dev_tile_consts(const BatchTileConsts &k, const fcpp_batch &b, int max_prims, bool dense, int64_t n_fields, int64_t gen)
{
    DevTileConsts tc;
    tc.tu = reinterpret_cast<const Pt2 *>(b.templates->tmpl_u.p); tc.tc = reinterpret_cast<const Pt2 *>(b.templates->tmpl_c.p);
    tc.nu = k.nu; tc.nc = k.nc; tc.turn_quiet = k.turn_quiet; tc.fuse_spans = k.fuse_spans; tc.span_line_max = k.span_line_max;
    tc.two_a = k.two_a; tc.u_cap = k.u_cap; tc.c_line = k.c_line; tc.fence_margin = k.fence_margin;
    tc.wave_factor = k.wave_factor; tc.field_work_tiles = FIELD_WORK_TILES; tc.reduce_wg_max = TileConsts::reduce_wg_max; tc.max_prims = max_prims;
    tc.no_bases = 0; tc.speculative = 0; tc.closed_cut = dense ? 0 : 1; tc.dense = dense ? 1 : 0; tc.direct = 0;
    tc.gen = gen;
    tc.cut = make_cut_consts(*b.templates, true, k, b.cst);
    return tc;
}

// a device-built slab's layout before its counts: the fields, the obstacle table, fcpp_field_info in the slab
void device_layout(ImageLayout &l, int64_t n_fields, const fcpp_polys *obstacles)
{
    l = ImageLayout();
    l.n_fields = n_fields; l.info_on_device = true;
    l.n_polys = obstacles ? obstacles->n_polys : 0; l.n_poly_verts = l.n_polys > 0 ? obstacles->offsets[l.n_polys] : 0;
}

// SPECULATIVE layout, for small batches (at most 8192 fields: the counting phase's one-scan form): by per-field CAPACITIES, before anything
// has run, so that the fill pass can be enqueued right behind the last scan -- the host then waits for the totals (they size the output
// arrays and the steps' launches) while the fill pass already runs, instead of the device waiting for the host's round trip in between.
// A field beyond the capacities (PF_OVER_CAPACITY: more than eight wave tiles, a span of more than sixteen chunks: big fields, many
// headland loops) makes the fill pass a no-op; the tables are then laid out from the totals and filled again, as for large batches.
// Within a table the records lie packed either way: only where each table begins differs.
void capacity_layout(ImageLayout &l, int64_t n_fields, const fcpp_polys *obstacles, int max_prims)
{
    device_layout(l, n_fields, obstacles);
    const int64_t K = DEVPLAN_KEEP_TILES;
    l.n_prims = n_fields * max_prims;
    l.n_tiles = l.n_stat = n_fields * (1 + K); l.n_wave = l.n_general = l.n_open_wave = n_fields * K;
    l.n_span_chunks = n_fields * SPEC_SPAN_CHUNKS; l.n_runs = n_fields;
    l.n_red[0] = n_fields; l.n_work[0] = l.n_field_work = n_fields;
    layout_image(l);
}

// what the tables hold, from the counting phase's totals (fuse: the spans of fields of field work are their workgroups')
void counts_from_totals(ImageLayout &l, const int64_t *tot, bool fuse)
{
    l.n_prims = tot[PC_PRIMS];
    l.n_tiles = tot[PC_TILES]; l.n_wave = tot[PC_WAVE]; l.n_general = tot[PC_GENERAL]; l.n_stat = tot[PC_STAT];
    l.n_span_chunks = fuse ? tot[PC_SPAN_F] : tot[PC_SPAN]; l.n_runs = tot[PC_RUNS];
    for (int k = 0; k < 4; ++k) l.n_red[k] = tot[PC_CLS0 + k];
    l.n_work[0] = tot[PC_WORK]; l.n_field_work = tot[PC_WORK]; l.n_open_wave = tot[PC_OPEN];
    l.quiet_points = tot[PC_SPAN_PTS] + tot[PC_CHUNK_PTS]; l.span_points = tot[PC_SPAN_PTS] - (fuse ? tot[PC_WORK_SPAN_PTS] : 0); l.work_span_points = fuse ? tot[PC_WORK_SPAN_PTS] : 0;
    l.n_chunks = tot[PC_CHUNKS]; l.chunk_points = tot[PC_CHUNK_PTS]; l.wave_points = tot[PC_WAVE_PTS];
    l.work_wave_points = tot[PC_WORK_WAVE_PTS]; l.wave_inside = tot[PC_WAVE_INSIDE];
}

// the batch's layout is decided and its slab is there: the tables' pointers, and the obstacle table into the slab
int bind_and_upload_obstacles(fcpp_ctx *c, fcpp_batch *b, const fcpp_polys *obstacles, hipStream_t st, std::string &err)
{
    const ImageLayout &lay = b->lay;
    b->t = bind_tables(lay, b->slab);
    if (lay.n_polys <= 0) return FCPP_OK;
    // (the obstacle region of the image -- it alone, offsets rebased -- through the context's pinned staging memory, pageable when that
    // cannot be had; the copy out of the staging memory is asynchronous: the next writer of that memory drains this stream first)
    const size_t o0 = lay.obs_off, o1 = lay.seg, nb = o1 - o0;
    std::vector<unsigned char> tmp;
    unsigned char *img = nullptr;
    if (const int urc = upload_buffer(c, nb, nb + nb / 4, tmp, img, err); urc != FCPP_OK) return urc;
    fill_obstacles(obstacles, lay, img, o0);
    DEVCHK(hipMemcpyAsync(static_cast<unsigned char *>(b->slab) + o0, img, nb, hipMemcpyHostToDevice, st));
    if (!tmp.empty()) DEVCHK(hipStreamSynchronize(st));
    else { c->stage_stream = st; c->stage_busy = true; }
    return FCPP_OK;
}

// A setup that failed gives its slab back: the device path's failure, the host path's (FailedBatch) and the speculative slab that turns out too
// small for the exact layout (DeviceSetup::settle) -- whatever was enqueued on `st` may still write it: drained first.  (A batch that succeeds
// hands its slab to the context's spare in fcpp_batch_destroy.)
hipError_t release_slab(fcpp_batch *b, hipStream_t st)
{
    if (!b->slab) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(st);
    (void)hipFree(b->slab); b->slab = nullptr; b->slab_bytes = 0;
    return e;
}
struct FailedBatch {      // batch_create's owner of a batch that is not handed out
    void operator()(fcpp_batch *b) const { (void)release_slab(b, b->ctx->stream); delete b; }
};

// A word of the host's own pinned memory that a kernel sets to the phase's generation number -- there a microsecond after the kernel wrote it --
// polled, with the drained stream as the fallback: 1024 spins between two looks at the clock, 2 ms at most.  No event behind the kernel: a
// record between two kernels holds the second one back by 5 us.
int poll_word(const volatile int64_t *w, int64_t gen, hipStream_t st, std::string &err)
{
    const auto t_poll = std::chrono::steady_clock::now();
    bool seen = false;
    for (int spin = 0; !seen; ++spin) {
        seen = *w == gen;
        if (!seen && (spin & 1023) == 1023 && ms_since(t_poll) > 2.0) break;
    }
    if (!seen) DEVCHK(hipStreamSynchronize(st));
    std::atomic_thread_fence(std::memory_order_acquire);
    return FCPP_OK;
}

// The device setup of one batch: what its phases share, on the stack of try_device_setup.  Every decision is read from fcpp_setuprule.h
// (setup_accept, setup_begin, setup_end, the slot's begin_aggregates / aggregates_settled); the phases enqueue and wait.
struct DeviceSetup {
    fcpp_ctx *c;
    fcpp_batch *b;
    const int64_t n_fields;
    const fcpp_field *fields;
    const fcpp_polys *obstacles;
    bool &fresh_templates;            // the batch's template set is still on its way back from the device (cleared once this path has waited for it)
    const SetupSwitches &sw;
    std::string &err;
    PlanOutputs *po;                  // fcpp_batch_plan: outputs are wanted
    hipStream_t st;
    // constants, scratch, the plan slot and the totals' mirror (prepare)
    PlanConsts pc;
    TurnTemplates tt;
    BatchTileConsts k;
    DevTileConsts tc;
    DevPlanScratch s;
    const fcpp_field *dev_fields;
    fcpp_ctx::PlanSlot *slot;
    const int64_t *tot;
    // the decisions
    bool dense, no_polys;
    SetupBegin begin;                 // spec, direct
    bool stepped;                     // the direct step is in the stream
    bool totals_seen;                 // the counting pass is through: nothing in the stream reads the caller's records any more
    SetupEnd end;                     // fuse, within, qualifies, taken, refill
    std::chrono::steady_clock::time_point t0, t_call;

    // a launcher returned an error.  Until the totals are seen the stream is drained first: whatever was launched may still be reading the
    // caller's pinned records.  Afterwards (the refill, the rescan, the exact fill) the planner is long through and the failed batch's slab
    // is drained where it is given back (release_slab).
    int launch_failed(int lrc, const char *launcher)
    {
        if (!totals_seen) (void)hipStreamSynchronize(st);
        err = std::string(launcher) + ": " + hipGetErrorString((hipError_t)lrc);
        return FCPP_EHIP;
    }
    int decline(SetupDecline d) { err = setup_decline_text(d); return kNotOnDevice; }
    // the fill pass (it also computes what the host path launches k_field_junctions, k_run_consts and k_work_totals for, field by field)
    int fill()
    {
        b->cst.field_junc = b->t.field_junc;
        const int frc = launch_devplan_fill(st, n_fields, tc, b->cst, s, b->t, c->plan_totals_host);
        return frc ? launch_failed(frc, "launch_devplan_fill") : FCPP_OK;
    }

    // ---- 1. decline or accept (fcpp_setuprule.h: setup_accept); the plan constants and the polygon table's checks
    int accept()
    {
        const fcpp_options &opt = b->opt;
        SetupAcceptIn in = { c->setup_mode, n_fields, sw.small_batch, opt.obstacle_mode, sw.field_work, 0, DEVPLAN_PRIMS_CAP };
        if (const SetupDecline d = setup_accept(in)) return decline(d);
        dense = opt.sample_spacing != 0.0;          // (round 5: span + quiet runs of the straights + general tiles, k_tile_fields' dense block)
        int rc = plan_prepare(b->veh, opt, pc, tt, err);
        if (rc != FCPP_OK) return rc;
        if ((rc = validate_polys(obstacles, err)) != FCPP_OK) return rc;
        in.max_prims = pc.max_prims;
        if (const SetupDecline d = setup_accept(in)) return decline(d);
        t0 = std::chrono::steady_clock::now();
        t_call = t0;
        return FCPP_OK;
    }

    // ---- 2. constants and scratch.  Templates on the host (closed-form test); a fresh set is on its way back
    int prepare()
    {
        if (fresh_templates) { DEVCHK(hipStreamSynchronize(st)); fresh_templates = false; }
        c->templates = b->templates;
        const bool turn_quiet = set_batch_consts(b, *b->templates);
        b->setup.templates_ms += ms_since(t0);

        t0 = std::chrono::steady_clock::now();
        int rc;
        if ((rc = plan_scratch(c, n_fields, pc.max_prims, st, s, err)) != FCPP_OK) return rc;
        if ((rc = device_fields(fields, n_fields, st, s, dev_fields, err)) != FCPP_OK) return rc;
        batch_tile_consts(*b, turn_quiet, sw.field_work, sw.span_line_max, k);
        tc = dev_tile_consts(k, *b, pc.max_prims, dense, n_fields, ++c->plan_gen);
        tot = c->plan_totals_host;
        slot = &c->plan_slots[c->plan_cur];
        return FCPP_OK;
    }

    // ---- 3. how the setup begins (setup_begin): the speculative layout (capacity_layout), its slab and obstacle table, the slot's aggregates;
    // the direct step (fcpp_batch_plan, no obstacle polygons) -- attempted while the context's last speculative setup qualified for it
    int begin_speculative()
    {
        no_polys = !obstacles || obstacles->n_polys == 0;
        SetupBeginIn in = { n_fields, devplan_small_blocks(), sw.exact_only, dense, 0, po != nullptr, no_polys, tc.fuse_spans != 0, c->direct_ok, sw.direct };
        if (setup_wants_capacities(in)) {
            capacity_layout(b->lay, n_fields, obstacles, pc.max_prims);
            in.capacity_bytes = b->lay.total_bytes;
        }
        begin = setup_begin(in);
        tc.speculative = begin.spec ? 1 : 0;
        if (begin.direct) tc.direct = DIRECT_COUNT;
        if (!begin.spec) return FCPP_OK;
        int rc;
        if ((rc = take_slab(c, b, err)) != FCPP_OK) return rc;
        if ((rc = bind_and_upload_obstacles(c, b, obstacles, st, err)) != FCPP_OK) return rc;
        const AggBegin ab = slot->begin_aggregates();      // (no command in the stream clears them: SlotAggregates, fcpp_setuprule.h)
        if (ab.clear_both) DEVCHK(hipMemsetAsync(s.agg, 0, 2 * (size_t)OFF_WORDS * sizeof(int64_t), st));
        if (ab.use_second) std::swap(s.agg, s.agg_next);
        return FCPP_OK;
    }

    // ---- 4. plan and count
    int count()
    {
        const int lrc = launch_devplan_count(st, n_fields, pc, tc, s, dev_fields, obstacles ? obstacles->n_polys : 0, obstacles != nullptr, c->plan_totals_host,
                                             begin.direct ? &b->cst : nullptr, sw.cut_rows);
        if (!lrc && devplan_count_in_rows(tc, n_fields, sw.cut_rows)) ++c->cut_rows_passes;
        return lrc ? launch_failed(lrc, "launch_devplan_count") : FCPP_OK;
    }

    // ---- 5. direct: the point total is final once the planner has run -- the counting launch's first workgroup writes it; the output arrays are
    // allocated and the step enqueued while the counting pass runs.  The step applies the batch rule itself and publishes the totals.
    int direct_step()
    {
        if (!begin.direct) return FCPP_OK;
        const volatile int64_t *early = tot + PX_EARLY_GEN;
        if (const int rc = poll_word(early, tc.gen, st, err); rc != FCPP_OK) return rc;
        const int64_t points = tot[PX_EARLY_POINTS];
        // (a total beyond the limits, or no room for the arrays: the setup goes on as without the direct step and reports what it finds)
        if (*early == tc.gen && points >= 0 && points <= kCountCap &&
            fcpp_outputs_alloc(c, points, 0, &po->x, &po->y, &po->kappa, &po->v, &po->fs) == FCPP_OK) {
            po->allocated = true; po->points = points;
            const int drc = launch_plan_sparse_direct(st, n_fields, tc.gen, s, b->cst, po->x, po->y, po->kappa, po->v, po->fs,
                                                      po->stats ? po->stats : b->t.own_stats, c->plan_totals_host);
            if (drc) return launch_failed(drc, "launch_plan_sparse_direct");
            stepped = true;
            ++c->direct_steps;
        }
        tc.direct = stepped ? DIRECT_FILL : 0;      // (a fill pass behind the step has no publisher)
        return FCPP_OK;
    }

    // ---- 6. the speculative fill pass right behind the counting pass (it publishes the totals: no scan in between) -- unless the step is there
    int speculative_fill()
    {
        if (!begin.spec) return FCPP_OK;
        if (!stepped) { const int rc = fill(); if (rc != FCPP_OK) return rc; }
        slot->aggregates_settled();
        return FCPP_OK;
    }

    // ---- 7. wait for the totals, checks.
    // The last scan -- or the speculative setup's publisher -- has written the totals and the flags to `tot`, then the phase's generation number
    // to tot[PX_DONE]: polled (poll_word); a speculative fill pass runs on.  Batches laid out from their totals poll as well: nothing else is
    // in the stream, and the poll sees the word ~10 us before a drained stream reports.
    int await()
    {
        int rc = poll_word(tot + PX_DONE, tc.gen, st, err);
        if (rc == FCPP_OK) {
            totals_seen = true;
            g_trace_totals_ms = ms_since(t_call);
            // what the counting phase found: an error, a batch for the host after all, or FCPP_OK
            if (tot[PC_COLS + PF_BAD_OBSTACLES] == tc.gen) { err = "field obstacle range outside the polygon table"; rc = FCPP_ESIZE; }
            else if (tot[PC_COLS + PF_FALLBACK] == tc.gen) { err = "a field beyond the device planner's limits (general stretch, primitives)"; rc = kNotOnDevice; }
            else if (tot[PC_POINTS] > kCountCap) { err = "batch too large"; rc = FCPP_ESIZE; }
            else if (tot[PC_PRIMS] > ((int64_t)1 << 26)) { err = "too many path primitives in one batch: split the batch"; rc = FCPP_ESIZE; }
            else if (tot[PC_TILES] > INT32_MAX) { err = "too many tiles in one batch: split the batch"; rc = FCPP_ESIZE; }
        }
        b->setup.host_plan_ms = ms_since(t0);          // (the plan and the counting pass, on the device)
        return rc;
    }

    // ---- 8. how the setup ends (setup_end): within its capacities -- the tables begin where the capacities put them; what they hold is what the
    // totals say -- or the exact layout: from the totals, the allocation, the obstacle table, the scan, the fill pass
    int settle()
    {
        fcpp_setup_times &tm = b->setup;
        ImageLayout &lay = b->lay;
        t0 = std::chrono::steady_clock::now();
        const SetupEndIn in = { begin.spec, stepped, po ? po->points : 0, tot[PC_UNFUSABLE], tot[PC_WORK_SPAN_PTS], tot[PC_WORK], tot[PC_POINTS],
                                tot[PC_COLS + PF_OVER_CAPACITY], tc.gen, n_fields, tc.fuse_spans != 0, no_polys };
        end = setup_end(in);
        if (begin.spec) c->direct_ok = end.qualifies;
        int rc;
        if (end.refill && (rc = fill()) != FCPP_OK) return rc;      // declined: the fill pass, its publisher off
        if (end.within) {
            counts_from_totals(lay, tot, end.fuse);
            tm.image_ms = ms_since(t0);
            return FCPP_OK;
        }
        ImageLayout ex;
        device_layout(ex, n_fields, obstacles);
        counts_from_totals(ex, tot, end.fuse);
        layout_image(ex);
        if (b->slab && b->slab_bytes < ex.total_bytes) {       // (a speculative slab that is too small: its fill pass was a no-op, but it is in the stream)
            const hipError_t e = release_slab(b, st);
            if (e != hipSuccess) { err = std::string("hipStreamSynchronize(st): ") + hipGetErrorString(e); return FCPP_EHIP; }
        }
        lay = ex;
        if (!b->slab && (rc = take_slab(c, b, err)) != FCPP_OK) return rc;
        if ((rc = bind_and_upload_obstacles(c, b, obstacles, st, err)) != FCPP_OK) return rc;
        tm.image_ms = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        // (after a speculative counting phase no scan has run: the pass wrote every column, the scan makes the positions of the exact layout)
        if (begin.spec) { const int src = launch_devplan_rescan(st, n_fields, s); if (src) return launch_failed(src, "launch_devplan_rescan"); }
        tc.speculative = 0; tc.direct = 0;
        tc.fuse_spans = end.fuse;
        return fill();
    }

    // ---- 9. the batch is set up: the slot and the batch remember the stream, a taken batch its fill pass for later.
    // fcpp_field_info stays on the device until somebody asks (fcpp_batch_info); the stream is NOT drained: a step enqueued next runs
    // right behind the setup
    void commit()
    {
        fcpp_setup_times &tm = b->setup;
        const ImageLayout &lay = b->lay;
        tm.image_bytes = (int64_t)((size_t)n_fields * sizeof(fcpp_field) + (lay.n_polys > 0 ? lay.seg - lay.obs_off : 0));
        slot->pending = true;
        b->setup_stream = st; b->setup_pending = true;
        if (end.taken) {
            b->tables_pending = true; b->tables_slot = c->plan_cur; b->tables_tc = tc; b->tables_scratch = s;
            slot->tables_batch = b;
            po->stepped = true;
            ++c->direct_taken;
        }
        b->info_dev = b->t.info;
        b->hp.info.clear();
        b->hp.tt = tt;
        b->hp.total_points = tot[PC_POINTS]; b->hp.total_prims = tot[PC_PRIMS];
        b->hp.fields.clear(); b->hp.blocks.clear(); b->hp.same_as.clear();
        tm.tiler_ms = ms_since(t0);              // (the fill pass, the setup kernels and the copy back of the field records)
        tm.h2d_ms = 0.0;
        tm.device_setup = 1;
    }

    int run()
    {
        int rc;      // (FCPP_OK is 0: the first phase that does not return it ends the setup)
        if ((rc = accept()) || (rc = prepare()) || (rc = begin_speculative()) || (rc = count()) || (rc = direct_step()) || (rc = speculative_fill()) ||
            (rc = await()) || (rc = settle())) return rc;
        commit();
        return FCPP_OK;
    }
};

// FCPP_OK: the batch is set up (tables on the device, info on the host); kNotOnDevice: not this path's batch; else the error -- either way the
// batch holds no slab then.
int try_device_setup(fcpp_ctx *c, fcpp_batch *b, int64_t n_fields, const fcpp_field *fields, const fcpp_polys *obstacles, bool &fresh_templates,
                     const SetupSwitches &sw, std::string &err, PlanOutputs *po)
{
    DeviceSetup d = { c, b, n_fields, fields, obstacles, fresh_templates, sw, err, po, c->stream };
    const int rc = d.run();
    if (rc != FCPP_OK) (void)release_slab(b, c->stream);
    return rc;
}
#undef DEVCHK
}  // namespace

int batch_create(fcpp_ctx *c, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields,
                 const fcpp_field *fields, const fcpp_polys *obstacles, fcpp_batch **out, PlanOutputs *po)
{
    if (!c || !veh || !opt || !out || n_fields < 0 || (n_fields > 0 && !fields))
        return fail(FCPP_EINVAL, "bad arguments");
    if (n_fields > INT32_MAX) return fail(FCPP_ESIZE, "too many fields");
    *out = nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<fcpp_batch, FailedBatch> b(new (std::nothrow) fcpp_batch());
    if (!b) return fail(FCPP_ENOMEM, "out of host memory");
    b->ctx = c; b->veh = *veh; b->opt = *opt; b->n_fields = n_fields;
    const SetupSwitches sw = SetupSwitches::read();
    fcpp_setup_times &tm = b->setup;
    tm.threads = WorkerPool::width();
    std::string err;
    hipStream_t st = c->stream;
    b->note_stream(st);

    // ---- 1. the turn templates go first: their two launches and the copy back run on the device while the host plans the fields
    auto t0 = std::chrono::steady_clock::now();
    bool fresh = false;
    {
        TurnTemplates tt;
        int rc = plan_templates(*veh, *opt, tt, err);
        if (rc != FCPP_OK) return fail(rc, err);
        rc = get_templates(c, tt, *opt, st, b->templates, fresh);
        if (rc != FCPP_OK) return rc;
    }
    tm.templates_ms = ms_since(t0);

    // ---- 2a. the setup on the DEVICE (fcpp_devplan.h) for batches at the reference's own sampling: the field records go up, the plan
    // function the host would run (fcpp_planfn.h) runs one thread per field, the tiler's cut one wavefront per field, the totals come
    // back once (they size the tables and the output arrays), the tables are written in place.  The host plans nothing per field.
    {
        int rc = try_device_setup(c, b.get(), n_fields, fields, obstacles, fresh, sw, err, po);
        if (rc == FCPP_OK) {
            tm.total_ms = ms_since(t_begin);
            c->last_setup = tm;
            *out = b.release();
            return FCPP_OK;
        }
        if (rc != kNotOnDevice) return fail(rc, err);
        if (c->setup_mode == FCPP_SETUP_DEVICE) return fail(FCPP_EUNSUPPORTED, "FCPP_SETUP_DEVICE: " + err);
        err.clear();
    }

    // ---- 2. host plan: __init__ + the O(1) decisions of every field, blocks of fields side by side (fcpp_host.cpp)
    t0 = std::chrono::steady_clock::now();
    std::vector<fcpp_field> fcopy;             // (records in device memory: the host plans a copy)
    int rc = host_fields(fields, n_fields, fcopy, fields);
    if (rc != FCPP_OK) { if (fresh) (void)hipStreamSynchronize(st); return rc; }
    rc = build_host_plan(*veh, *opt, n_fields, fields, obstacles, true, b->hp, err);
    if (rc != FCPP_OK) { if (fresh) (void)hipStreamSynchronize(st); return fail(rc, err); }
    tm.host_plan_ms = ms_since(t0);

    // ---- 3. templates on the host; are the U-turns of this batch closed form?
    t0 = std::chrono::steady_clock::now();
    if (fresh) HIPCHK(hipStreamSynchronize(st));
    c->templates = b->templates;
    const TemplateSet &ts = *b->templates;
    const bool turn_quiet = set_batch_consts(b.get(), ts);
    tm.templates_ms += ms_since(t0);

    // ---- 4. tiler: every field's path cut into work for the four kernels, blocks side by side (fcpp_tiler.cpp)
    t0 = std::chrono::steady_clock::now();
    TileConsts tc;
    batch_tile_consts(*b, turn_quiet, sw.field_work, sw.span_line_max, tc);
    tc.tu = reinterpret_cast<const Pt2 *>(ts.h_tu.data()); tc.tc = reinterpret_cast<const Pt2 *>(ts.h_tc.data());
    tc.templates_ok = true;
    tc.field_work = sw.field_work;
    // the chunk lists are expanded on the device from the host's chunk groups; FCPP_HOST_CHUNKS=1 (the checker, tests/test_gpu_devplan.py)
    // keeps the host's own lists
    tc.device_chunks = sw.device_chunks;
    // the reference's sampling: the general stretch of every field with a closed-form span is cut in closed form (fcpp_cutfn.h), as the device
    // planner cuts it -- host-built and device-built tables stay equal byte for byte
    tc.closed_cut = opt->sample_spacing == 0.0 && opt->obstacle_mode == FCPP_OBSTACLES_FLAG;
    tc.cut = make_cut_consts(*b->templates, false, tc, b->cst);
    BatchTiler tiler;
    ImageLayout &lay = b->lay;
    rc = tiler.plan(b->hp, tc, obstacles, lay, err);
    if (rc != FCPP_OK) return fail(rc, err);
    if (tc.fuse_spans && lay.unfusable_work > 0) {       // all spans of fields of field work are fused, or none (as on the device path)
        tc.fuse_spans = false;
        rc = tiler.plan(b->hp, tc, obstacles, lay, err);
        if (rc != FCPP_OK) return fail(rc, err);
    }
    tm.tiler_ms = ms_since(t0);

    // ---- 5. the image: one device allocation (the context's spare if it is large enough), the tables written into pinned memory
    t0 = std::chrono::steady_clock::now();
    if ((rc = take_slab(c, b.get(), err)) != FCPP_OK) return fail(rc, err);      // (an error below gives it back: FailedBatch)
    unsigned char *img = nullptr;
    std::vector<unsigned char> pageable;
    rc = upload_buffer(c, lay.upload_bytes, std::min(kStageMax, std::max<size_t>(lay.upload_bytes + lay.upload_bytes / 4, (size_t)1 << 20)), pageable, img, err);
    if (rc != FCPP_OK) return fail(rc, err);
    tiler.fill(b->hp, obstacles, lay, img);
    b->t = bind_tables(lay, b->slab);
    // (the primitives live in the image now; the host keeps the per-field records for fcpp_batch_info and the staged pipeline's tiling)
    for (PlanBlock &blk : b->hp.blocks) std::vector<DevPrim>().swap(blk.prims);
    std::vector<int32_t>().swap(b->hp.same_as);
    tm.image_ms = ms_since(t0);
    tm.image_bytes = (int64_t)lay.upload_bytes;

    // ---- 6. one copy, the per-field junction constants, and the stream drained (the staging memory is the context's)
    t0 = std::chrono::steady_clock::now();
    if (lay.upload_bytes > 0) HIPCHK(hipMemcpyAsync(b->slab, img, lay.upload_bytes, hipMemcpyHostToDevice, st));
    if (n_fields > 0) {
        b->cst.field_junc = b->t.field_junc;
        LAUNCHCHK(launch_field_junctions(st, n_fields, b->t.fields, b->cst, b->t.field_junc));
        LAUNCHCHK(launch_expand_chunks(st, lay.n_chunk_groups, b->t.chunk_groups,
                                       b->t.tiles, b->t.fields, b->t.chunks, b->t.span_chunks));
        // the statistics slots: closed-form statistics of the quiet runs (the same at every step), zeros elsewhere
        LAUNCHCHK(launch_run_consts(st, lay.n_stat, b->t.stat_ids, b->t.stat_run, b->t.tiles, b->t.fields, b->t.prims, b->cst, b->t.partial));
        LAUNCHCHK(launch_work_totals(st, lay.n_field_work, b->t.field_work, b->t.stat_run, b->t.partial, b->t.work_totals));
    }
    // The stream is NOT drained when the image went through the context's pinned staging memory (round 5; as the device-side setup leaves it):
    // a step enqueued next runs right behind the copy and the setup kernels, a consumer on another stream is ordered behind them (wait_setup),
    // the staging memory's next writer drains this stream first (stage_wait).  A pageable image is freed on return: drained.
    if (!pageable.empty() || lay.upload_bytes == 0) HIPCHK(hipStreamSynchronize(st));
    else { c->stage_stream = st; c->stage_busy = true; b->setup_stream = st; b->setup_pending = true; }
    tm.h2d_ms = ms_since(t0);
    tm.total_ms = ms_since(t_begin);
    c->last_setup = tm;
    *out = b.release();
    return FCPP_OK;
}

int ensure_tables(fcpp_batch *b)
{
    if (!b->tables_pending) return FCPP_OK;
    HIPCHK(hipSetDevice(b->ctx->device));
    std::string err;
    const int rc = flush_tables(b, b->ctx->stream, err);
    return rc == FCPP_OK ? FCPP_OK : fail(rc, err);
}

}  // namespace fcpp
