// fcpp_api.cpp -- the C ABI declared in include/fcpp.h: the context and its output arena, a batch's entries and step, GA, cover, gather and the
// debug entries: argument checking, device buffers, launches.  (A batch's setup: fcpp_setup.cpp; the standalone path operators: fcpp_paths.cpp, fcpp_glue_*.cpp.)
// No CPU compute path exists here: every operator ends in a HIP kernel launch or fails with FCPP_EHIP.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <vector>

#include "fcpp_batch.h"
#include "fcpp_cover.h"
#include "fcpp_ga.h"
#include "fcpp_connfn.h"

using namespace fcpp;

namespace fcpp { thread_local LaunchProf g_launch_prof; }

namespace { thread_local std::string g_err; }

int fcpp::fail(int code, const std::string &msg) { g_err = msg; return code; }

DevConst fcpp::make_const(const fcpp_vehicle &veh, const fcpp_options &opt)
{
    DevConst c;
    c.a_lat = veh.max_lateral_accel; c.a_lon = veh.max_longitudinal_accel; c.sf = veh.safety_factor;
    c.geofence_tol = opt.geofence_tol;
    c.v_work = veh.max_work_speed_kmh; c.v_turn = veh.headland_turn_speed_kmh; c.v_head = veh.max_headland_speed_kmh;
    const double vm = std::max(std::max(veh.max_work_speed_kmh, veh.max_headland_speed_kmh),
                               std::max(veh.headland_turn_speed_kmh, 2.5)) / 3.6;
    c.u_cap = vm * vm;
    c.inv_sf36 = 1.0 / (c.sf * 3.6);
    c.ms_work = c.v_work / 3.6; c.ms_turn = c.v_turn / 3.6; c.ms_head = c.v_head / 3.6; c.ms_rev = 2.5 / 3.6;
    c.shapes = nullptr; c.tmpl_u = nullptr; c.tmpl_c = nullptr; c.tmpl_u_dk = nullptr; c.field_junc = nullptr;
    c.tmpl_n = 0; c.tmpl_nc = 1;
    c.turn_kappa_last[0] = c.turn_kappa_last[1] = c.turn_len = c.turn_time = 0.0;
    c.turn_max_kappa[0] = c.turn_max_kappa[1] = c.turn_max_jump[0] = c.turn_max_jump[1] = 0.0;
    c.turn_jump[0] = c.turn_jump[1] = 0.0;
    return c;
}

namespace {
constexpr int kStages = 7;
constexpr int kProfRuns = 256;
const char *const kStageNames[2][kStages] = {
    { "k_generate", "k_curv_clamp", "k_scan_tiles", "k_scan_spine", "k_scan_apply", "k_validate", "k_reduce_stats" },
    { "k_plan_quiet_spans", "k_plan_quiet", "k_plan_sparse", "k_plan_fused", "k_reduce_stats", "k_plan_sparse_fields", "" } };
const int kStageCount[2] = { 7, 6 };
}

namespace {
// fcpp_debug_dubins (MODE 0) / fcpp_debug_rs (MODE 1): the host side of the connectors' one function, a pair at a time
// (one pair, kept out of line: with the 48 words inlined into the loop below the host compiler's loop passes take minutes to hours over
//  them; a call changes no bit)
template <int MODE>
__attribute__((noinline)) void debug_conn_pair(double x0, double y0, double h0, double x1, double y1, double h1, double radius, int &w, double *s,
                                               double &tot)
{
    Conn<MODE>::solve(x0, y0, h0, x1, y1, h1, radius, w, s, tot);
}

template <int MODE>
int debug_conn(int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty, const double *th,
               double radius, int32_t *word, double *seg, double *len)
{
    constexpr int NSEG = Conn<MODE>::NSEG;
    if (!(radius > 0.0) || !isfinite(radius)) return fail(FCPP_EINVAL, "radius must be positive and finite");
    if (n < 0) return fail(FCPP_ESIZE, "bad sizes");
    if (n > 0 && (!fx || !fy || !fh || !tx || !ty || !th)) return fail(FCPP_EINVAL, "bad arguments");
    for (int64_t i = 0; i < n; ++i) {
        int w;
        double s[NSEG], tot;
        debug_conn_pair<MODE>(fx[i], fy[i], fh[i], tx[i], ty[i], th[i], radius, w, s, tot);
        if (word) word[i] = w;
        if (seg) for (int k = 0; k < NSEG; ++k) seg[NSEG * i + k] = s[k];
        if (len) len[i] = tot;
    }
    return FCPP_OK;
}
}  // namespace

extern "C" {

const char *fcpp_last_error(void) { return g_err.c_str(); }
int fcpp_abi_version(void) { return FCPP_ABI_VERSION; }

void fcpp_vehicle_default(fcpp_vehicle *v)
{
    v->working_width = 3.2; v->min_turn_radius = 8.0; v->max_work_speed_kmh = 9.0;
    v->max_headland_speed_kmh = 15.0; v->headland_turn_speed_kmh = 4.0; v->max_lateral_accel = 2.0;
    v->max_longitudinal_accel = 1.5; v->safety_factor = 0.85;
}

void fcpp_options_default(fcpp_options *o)
{
    o->turn_model = FCPP_TURN_ARC; o->clothoid_fit = 1; o->sample_spacing = 0.0; o->clothoid_frac = 0.5;
    o->geofence_tol = 1e-6; o->obstacle_mode = FCPP_OBSTACLES_FLAG; o->ring_order = FCPP_RING_AS_VERTICES;
}

int fcpp_ctx_create(int device_id, fcpp_ctx **out)
{
    if (!out) return fail(FCPP_EINVAL, "ctx out pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(FCPP_EHIP, "no HIP device available: libfcpp has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(FCPP_EINVAL, "device_id out of range");
    HIPCHK(hipSetDevice(device_id));
    fcpp_ctx *c = new (std::nothrow) fcpp_ctx();
    if (!c) return fail(FCPP_ENOMEM, "out of host memory");
    c->device = device_id;
    e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (c->own) (void)hipStreamDestroy(c->own);
        if (c->side) (void)hipStreamDestroy(c->side);
        if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
        delete c;
        return fail(FCPP_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    c->stream = c->own;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess) { (void)hipGetLastError(); c->n_cu = 0; }
    if (const char *e = getenv("FCPP_SETUP")) c->setup_mode = !strcmp(e, "host") ? FCPP_SETUP_HOST : (!strcmp(e, "device") ? FCPP_SETUP_DEVICE : FCPP_SETUP_AUTO);
    *out = c;
    return FCPP_OK;
}

int fcpp_ctx_set_setup(fcpp_ctx *c, int mode)
{
    if (!c || mode < FCPP_SETUP_AUTO || mode > FCPP_SETUP_DEVICE) return fail(FCPP_EINVAL, "bad arguments");
    c->setup_mode = mode;
    return FCPP_OK;
}

int fcpp_ctx_destroy(fcpp_ctx *c)
{
    if (!c) return FCPP_OK;
    (void)hipSetDevice(c->device);
    if (c->own) { (void)hipStreamSynchronize(c->own); (void)hipStreamDestroy(c->own); }
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    free_paths_cache(c);
    (void)c->stage_wait();
    if (c->stage) (void)hipHostFree(c->stage);
    if (c->spare) (void)hipFree(c->spare);
    for (auto &sl : c->plan_slots) if (sl.p) { (void)hipDeviceSynchronize(); (void)hipFree(sl.p); sl.p = nullptr; }
    if (c->arena) { (void)hipDeviceSynchronize(); (void)hipFree(c->arena); }
    if (c->ev_plan) (void)hipEventDestroy(c->ev_plan);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->plan_totals_host) (void)hipHostFree(c->plan_totals_host);
    if (c->ga_mirror) (void)hipHostFree(c->ga_mirror);
    if (c->verify_scratch) (void)hipFree(c->verify_scratch);
    c->templates.reset();
    delete c;
    return FCPP_OK;
}

int fcpp_ctx_set_stream(fcpp_ctx *c, void *s)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    c->stream = (hipStream_t)s;   // NULL = HIP's default stream
    return FCPP_OK;
}

int fcpp_ctx_synchronize(fcpp_ctx *c)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_malloc(fcpp_ctx *c, int64_t bytes, void **p)
{
    if (!c || !p || bytes < 0) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    *p = nullptr;
    if (bytes == 0) return FCPP_OK;
    HIPCHK(hipMalloc(p, (size_t)bytes));
    return FCPP_OK;
}

int fcpp_free(fcpp_ctx *c, void *p)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (p) HIPCHK(hipFree(p));
    return FCPP_OK;
}

// ---- output arrays with the placement rule of DESIGN.md section 2 (HISTORY.md "Where the five arrays lie").  Measured on MI355X: the streaming kernels
// write x, y, kappa, v and flagseg side by side, and five write streams that lie within a few GiB of each other in (physical) device
// memory run at 4.6 TB/s, the same streams >= 12-24 GiB apart at 6.3-6.6 TB/s (tools/placement_pitch.py: the class follows the pitch
// and nothing else).  The context's ARENA is the remedy that several live batches can share: one allocation made once
// (fcpp_ctx_reserve_outputs: five lanes `pitch` apart), array k of every fcpp_outputs_alloc in lane k.
int fcpp_ctx_reserve_outputs(fcpp_ctx *c, int64_t lane_bytes, int64_t pitch_bytes)
{
    if (!c || lane_bytes < 0 || pitch_bytes < 0) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (c->arena) {
        if (!c->arena_live.empty()) return fail(FCPP_EINVAL, "the output arena has live allocations");
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipFree(c->arena));
        c->arena = nullptr; c->arena_pitch = c->arena_lane = 0;
    }
    size_t pitch = pitch_bytes > 0 ? (size_t)pitch_bytes : (size_t)FCPP_OUTPUT_PITCH;
    size_t lane = lane_bytes > 0 ? (size_t)lane_bytes : pitch;
    pitch = (pitch + 4095) / 4096 * 4096; lane = (lane + 4095) / 4096 * 4096;
    if (lane > pitch) pitch = lane;                      // lanes must not overlap
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t reserve = (size_t)8 << 30;
    if (free_b < 4 * pitch + lane + reserve) return fail(FCPP_ENOMEM, "not enough free device memory for the output arena (4 x pitch + lane + 8 GiB)");
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, 4 * pitch + lane);
    if (e != hipSuccess) return fail(FCPP_ENOMEM, std::string("output arena: ") + hipGetErrorString(e));
    c->arena = p; c->arena_pitch = pitch; c->arena_lane = lane;
    c->arena_live.clear();
    return FCPP_OK;
}

int fcpp_ctx_outputs_info(const fcpp_ctx *c, int64_t *lane_bytes, int64_t *pitch_bytes, int64_t *live_bytes)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (lane_bytes) *lane_bytes = (int64_t)c->arena_lane;
    if (pitch_bytes) *pitch_bytes = (int64_t)c->arena_pitch;
    if (live_bytes) { size_t s = 0; for (const auto &blk : c->arena_live) s += blk.len; *live_bytes = (int64_t)s; }
    return FCPP_OK;
}

int fcpp_outputs_alloc(fcpp_ctx *c, int64_t n_points, int64_t pitch_bytes, double **x, double **y, double **kappa, double **v, uint32_t **flagseg)
{
    if (!c || n_points < 0 || !x || !y || !kappa || !v || !flagseg) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    const size_t S = (((size_t)n_points * 8 + 4095) / 4096) * 4096;
    char *b = nullptr;
    size_t P = 0;
    if (pitch_bytes == 0 && c->arena && S <= c->arena_lane) {
        // first fit in the lanes (the same offset in all five): the lowest gap between live allocations that holds the array
        const size_t need = std::max<size_t>(S, 4096);
        size_t off = 0;
        size_t at = 0;
        for (; at < c->arena_live.size(); ++at) {
            if (c->arena_live[at].off - off >= need) break;
            off = c->arena_live[at].off + c->arena_live[at].len;
        }
        if (off + need <= c->arena_lane) {
            c->arena_live.insert(c->arena_live.begin() + (long)at, fcpp_ctx::ArenaBlock{ off, need, nullptr, false });
            b = static_cast<char *>(c->arena) + off;
            P = c->arena_pitch;
        }
    }
    if (!b) {
        // without an arena (or beyond it): ONE allocation of its own, the arrays pitch_bytes apart -- back to back when no pitch is asked
        // for (the slow placement class for arrays of GBs, but nothing is taken from the device that the arrays do not need)
        P = pitch_bytes > 0 ? (size_t)pitch_bytes : S;
        if (P < S) P = S;
        P = (P + 4095) / 4096 * 4096;
        void *slab = nullptr;
        hipError_t e = hipMalloc(&slab, std::max<size_t>(4 * P + S, 4096));
        if (e != hipSuccess) return fail(FCPP_ENOMEM, std::string("output arrays: ") + hipGetErrorString(e));
        b = static_cast<char *>(slab);
    }
    *x = reinterpret_cast<double *>(b); *y = reinterpret_cast<double *>(b + P); *kappa = reinterpret_cast<double *>(b + 2 * P);
    *v = reinterpret_cast<double *>(b + 3 * P); *flagseg = reinterpret_cast<uint32_t *>(b + 4 * P);
    return FCPP_OK;
}

int fcpp_outputs_free(fcpp_ctx *c, double *x)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (!x) return FCPP_OK;
    char *p = reinterpret_cast<char *>(x);
    if (c->arena && p >= static_cast<char *>(c->arena) && p < static_cast<char *>(c->arena) + c->arena_lane) {
        const size_t off = (size_t)(p - static_cast<char *>(c->arena));
        for (size_t k = 0; k < c->arena_live.size(); ++k)
            if (c->arena_live[k].off == off) {
                // (steps that write the block may still be queued on the stream they ran on, and first fit may hand the same offset to a
                // batch on another stream at once: the block goes back only when that stream has finished with it -- a query when it is idle)
                const fcpp_ctx::ArenaBlock blk = c->arena_live[k];
                if (blk.used && hipStreamQuery(blk.last) != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipStreamSynchronize(blk.last)); }
                c->arena_live.erase(c->arena_live.begin() + (long)k);
                return FCPP_OK;
            }
        return fail(FCPP_EINVAL, "not an allocation of the output arena");
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(x));
    return FCPP_OK;
}

int fcpp_memcpy_h2d(fcpp_ctx *c, void *dst, const void *src, int64_t bytes)
{
    if (!c || bytes < 0) return fail(FCPP_EINVAL, "bad arguments");
    if (bytes == 0) return FCPP_OK;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_memcpy_d2h(fcpp_ctx *c, void *dst, const void *src, int64_t bytes)
{
    if (!c || bytes < 0) return fail(FCPP_EINVAL, "bad arguments");
    if (bytes == 0) return FCPP_OK;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_plan_count(const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields, const fcpp_field *fields,
                    const fcpp_polys *obstacles, fcpp_field_info *info_out)
{
    if (!veh || !opt || n_fields < 0 || (n_fields > 0 && (!fields || !info_out)))
        return fail(FCPP_EINVAL, "bad arguments");
    HostPlan hp;
    std::string err;
    std::vector<fcpp_field> fcopy;
    int rc = host_fields(fields, n_fields, fcopy, fields);
    if (rc != FCPP_OK) return rc;
    rc = build_host_plan(*veh, *opt, n_fields, fields, obstacles, false, hp, err);
    if (rc != FCPP_OK) return fail(rc, err);
    if (n_fields) memcpy(info_out, hp.info.data(), (size_t)n_fields * sizeof(fcpp_field_info));
    return FCPP_OK;
}

// Sizing for a sharded job: points per field.  On the device for the batches the device planner takes (k_plan_fields without primitives,
// the counts copied back), else on the host's cores.
int fcpp_plan_points(fcpp_ctx *c, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields, const fcpp_field *fields,
                     const fcpp_polys *obstacles, int64_t *points_out)
{
    if (!c || !veh || !opt || n_fields < 0 || (n_fields > 0 && (!fields || !points_out))) return fail(FCPP_EINVAL, "bad arguments");
    if (n_fields == 0) return FCPP_OK;
    std::string err;
    PlanConsts pc;
    TurnTemplates tt;
    int rc = plan_prepare(*veh, *opt, pc, tt, err);
    if (rc != FCPP_OK) return fail(rc, err);
    const bool on_device = c->setup_mode != FCPP_SETUP_HOST && opt->sample_spacing == 0.0 && opt->obstacle_mode == FCPP_OBSTACLES_FLAG &&
                           pc.max_prims <= DEVPLAN_PRIMS_CAP;
    if (!on_device) {
        HostPlan hp;
        std::vector<fcpp_field> fcopy;
        if ((rc = host_fields(fields, n_fields, fcopy, fields)) != FCPP_OK) return rc;
        rc = build_host_plan(*veh, *opt, n_fields, fields, obstacles, false, hp, err);
        if (rc != FCPP_OK) return fail(rc, err);
        for (int64_t i = 0; i < n_fields; ++i) points_out[i] = hp.info[(size_t)i].n_main + hp.info[(size_t)i].n_head;
        return FCPP_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevPlanScratch s;
    if ((rc = plan_scratch(c, n_fields, pc.max_prims, st, s, err)) != FCPP_OK) return fail(rc, err);
    const fcpp_field *dev_fields = nullptr;
    if ((rc = device_fields(fields, n_fields, st, s, dev_fields, err)) != FCPP_OK) return fail(rc, err);
    {   // (whatever was launched may still be reading the caller's pinned records: drained before an error goes back)
        const int lrc = launch_devplan_points(st, n_fields, pc, s, dev_fields);
        if (lrc) { (void)hipStreamSynchronize(st); return fail(FCPP_EHIP, std::string("launch_devplan_points: ") + hipGetErrorString((hipError_t)lrc)); }
    }
    HIPCHK(hipMemcpyAsync(points_out, s.counts + (int64_t)PC_POINTS * n_fields, (size_t)n_fields * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FCPP_OK;
}

int fcpp_batch_create(fcpp_ctx *c, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields,
                      const fcpp_field *fields, const fcpp_polys *obstacles, fcpp_batch **out)
{
    return batch_create(c, veh, opt, n_fields, fields, obstacles, out, nullptr);
}

// fcpp_field_info of a batch set up on the device: copied back when first needed
static int ensure_info(fcpp_batch *b)
{
    if (!b->info_dev || !b->hp.info.empty() || b->n_fields == 0) return FCPP_OK;
    HIPCHK(hipSetDevice(b->ctx->device));
    { const int rc = ensure_tables(b); if (rc) return rc; }
    try { b->hp.info.resize((size_t)b->n_fields); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (hipStream_t s : b->used_streams) HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(b->hp.info.data(), b->info_dev, (size_t)b->n_fields * sizeof(fcpp_field_info), hipMemcpyDeviceToHost));
    return FCPP_OK;
}

// output arrays from the context's arena: their block remembers the stream that writes it (fcpp_outputs_free)
static void note_arena_writer(fcpp_ctx *c, const double *x, hipStream_t st)
{
    if (!c->arena || !x) return;
    const char *p = reinterpret_cast<const char *>(x), *a0 = static_cast<const char *>(c->arena);
    if (p >= a0 && p < a0 + c->arena_lane) {
        const size_t off = (size_t)(p - a0);
        for (auto &blk : c->arena_live) if (off >= blk.off && off < blk.off + blk.len) { blk.last = st; blk.used = true; break; }
    }
}

int fcpp_batch_setup_times(const fcpp_batch *b, fcpp_setup_times *out)
{
    if (!b || !out) return fail(FCPP_EINVAL, "bad arguments");
    *out = b->setup;
    return FCPP_OK;
}

int fcpp_batch_info(const fcpp_batch *b, fcpp_field_info *info_out, int64_t *total_points)
{
    if (!b) return fail(FCPP_EINVAL, "batch is NULL");
    if (info_out && b->n_fields) { const int rc = ensure_info(const_cast<fcpp_batch *>(b)); if (rc) return rc; }
    if (info_out && b->n_fields) memcpy(info_out, b->hp.info.data(), (size_t)b->n_fields * sizeof(fcpp_field_info));
    if (total_points) *total_points = b->hp.total_points;
    return FCPP_OK;
}

int fcpp_batch_run(fcpp_batch *b, double *x, double *y, double *kappa, double *v, uint32_t *fs,
                   fcpp_field_stats *stats, int mode)
{
    if (!b) return fail(FCPP_EINVAL, "batch is NULL");
    // mode 1 (default): quiet tiles (k_plan_quiet, streaming) and general tiles (k_plan_fused) as two launches.
    // (Measured and dropped: both tile kinds in one grid, and the two kernels on two streams -- the HBM-bound and the
    // ALU-bound kernel do not overlap usefully, the sum of the two launches is the faster schedule.)
    if (mode != 0 && mode != 1) return fail(FCPP_EINVAL, "unknown pipeline mode");
    if (mode != b->last_mode) { b->prof_runs = 0; b->last_mode = mode; }
    if (b->n_fields == 0) return FCPP_OK;
    if (b->hp.total_points > 0 && (!x || !y || !kappa || !v || !fs)) return fail(FCPP_EINVAL, "output pointer is NULL");
    if (!stats) return fail(FCPP_EINVAL, "stats pointer is NULL");
    HIPCHK(hipSetDevice(b->ctx->device));
    hipStream_t st = b->ctx->stream;
    b->note_stream(st);
    { const int rc = ensure_tables(b); if (rc) return rc; }
    HIPCHK(b->wait_setup(st));
    note_arena_writer(b->ctx, x, st);
    if (mode == 0 && !b->til0_built) {      // the staged pipeline's own tiling: plain tiles of at most TILE_POINTS points
        { const int rc = ensure_info(b); if (rc) return rc; }
        Tiling t0;
        std::vector<int64_t> offs((size_t)b->n_fields + 1, 0);
        for (int64_t i = 0; i < b->n_fields; ++i) offs[(size_t)i + 1] = offs[(size_t)i] + b->hp.info[(size_t)i].n_main + b->hp.info[(size_t)i].n_head;
        t0.build(b->n_fields, offs.data());
        HIPCHK(b->til0.upload(t0, st));
        b->til0_built = true;
    }
    DevObstacles obs = { b->t.obs_off, b->t.obs_x, b->t.obs_y, b->t.obs_bbox };
    hipEvent_t *ev = nullptr;
    unsigned char *evs = nullptr;
    if (b->profiling > 0 && b->prof_runs < kProfRuns && (b->run_counter++ % b->profiling) == 0) {
        ev = &b->events[(size_t)b->prof_runs * kStages * 2];
        evs = &b->ev_set[(size_t)b->prof_runs * kStages];
    }
    // a stage = one kernel; profiled, its dispatch carries a start and a stop event (fcpp_device.h: LaunchProf)
#define STAGE(k, call)                                                                  \
    do {                                                                                \
        if (ev) { g_launch_prof.start = ev[2 * (k)]; g_launch_prof.stop = ev[2 * (k) + 1]; } \
        const int e_ = (call);                                                          \
        if (ev) { evs[k] = g_launch_prof.start == nullptr; g_launch_prof = LaunchProf(); }   \
        if (e_ != 0) return fail(FCPP_EHIP, std::string(#call) + ": " + hipGetErrorString((hipError_t)e_)); \
    } while (0)
    if (mode == 1) {
        const SlabTables &t = b->t;
        const ImageLayout &lay = b->lay;
        // Two streams inside the step where the general tiles are FEW and long-lived (dense sampling of a single large field: a dozen
        // tiles that walk long halos, cfg3: 5873 points in 0.37 ms): beside the HBM-bound streaming kernel they cost nothing (cfg3
        // 0.87 -> 0.51 ms).  Not when the general kernel can fill the chip itself -- side by side it takes compute units from the
        // streaming kernel (cfg2 at 0.1 m, 5950 general tiles: 6.5 vs 5.6 ms) -- and not at sparse sampling: k_plan_sparse and the
        // span kernel get in each other's way (cfg5 2.41 vs 2.29 ms, cfg1 x 4096 0.114 vs 0.098 ms; measured again with the final kernels: 2.46 vs 2.40
        // and 0.091 vs 0.085 ms, k_plan_sparse 1.07 instead of 0.69 ms; also with the span kernel held to four or five
        // waves per SIMD).
        hipStream_t sd = st;
        const bool two = lay.span_points + lay.chunk_points > 0 && lay.n_general > 0 && lay.n_general <= 512 && lay.n_wave == 0;
        if (two) {
            sd = b->ctx->side;
            HIPCHK(hipEventRecord(b->ctx->ev_fork, st));
            HIPCHK(hipStreamWaitEvent(sd, b->ctx->ev_fork, 0));
        }
        // the wave tiles of fields that k_plan_sparse_fields does not take (all of them when there are none of those)
        const bool fw = lay.n_field_work > 0;
        if (!fw) STAGE(2, launch_plan_sparse(sd, lay.n_wave, t.wtiles, t.fields, t.prims, b->cst, obs, x, y, kappa, v, fs, t.partial));
        else STAGE(2, launch_plan_sparse(sd, lay.n_open_wave, t.wtiles, t.fields, t.prims, b->cst, obs, x, y, kappa, v, fs, t.partial, t.open_wave_ids));
        STAGE(3, launch_plan_fused(sd, lay.n_general, t.general_ids, t.tiles, t.fields, t.prims, b->cst, obs, x,
                                   y, kappa, v, fs, t.partial));
        if (two) HIPCHK(hipEventRecord(b->ctx->ev_join, sd));
        STAGE(0, launch_plan_quiet(st, lay.n_span_chunks, t.span_chunks, 16, t.fields, t.prims, b->cst, obs, x, y, kappa, v, fs, t.partial));
        // (straights and U-turns in ONE launch: measured 4 % faster on identical memory than an instance each)
        STAGE(1, launch_plan_quiet(st, lay.n_chunks, t.chunks, 14, t.fields, t.prims, b->cst, obs, x, y, kappa, v, fs, t.partial));
        // fields planned and reduced by one workgroup each: after the streaming kernels, whose flag counts their reduction reads
        if (fw) {       // (one launch per class of fields; normally one class holds them all: the stage's events time the first launch)
            int64_t off = 0;
            bool first = true;
            for (int c = 0; c < 4; ++c) {
                if (lay.n_work[c] == 0) continue;
                if (first) STAGE(5, launch_plan_sparse_fields(st, lay.n_work[c], t.field_packs + off, b->cst, obs, x, y, kappa, v, fs, t.partial,
                                                              FIELD_WORK_WAVES[c], t.work_totals + off, stats, lay.work_span_points > 0));
                else LAUNCHCHK(launch_plan_sparse_fields(st, lay.n_work[c], t.field_packs + off, b->cst, obs, x, y, kappa, v, fs, t.partial,
                                                         FIELD_WORK_WAVES[c], t.work_totals + off, stats, lay.work_span_points > 0));
                first = false;
                off += lay.n_work[c];
            }
        }
        if (two) HIPCHK(hipStreamWaitEvent(st, b->ctx->ev_join, 0));
        // (four classes of paths by their number of entries; normally one of them holds every path of a batch: the stage's events
        // time the first launch)
        {
            const int groups[4] = { 8, 64, 256, 256 };     // (16 or 32 lanes for the first class: 49 -> 53 / 79 us on cfg5)
            const int32_t *pl = t.red_paths;
            bool first = true;
            for (int c = 0; c < 4; ++c) {
                if (lay.n_red[c] == 0) continue;
                // (a class that holds every path lists them in order: no list, one dependent load less in a latency-bound kernel)
                const int32_t *list = lay.n_red[c] == lay.n_fields ? nullptr : pl;
                if (first)
                    STAGE(4, launch_reduce_stats(st, lay.n_red[c], t.partial, t.stat_first, nullptr, stats, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, &b->cst, list, groups[c], c == 3 ? t.red_scratch : nullptr, 1));
                else
                    LAUNCHCHK(launch_reduce_stats(st, lay.n_red[c], t.partial, t.stat_first, nullptr, stats, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr, &b->cst, list, groups[c], c == 3 ? t.red_scratch : nullptr, 1));
                first = false;
                pl += lay.n_red[c];
            }
        }
        if (ev) ++b->prof_runs;
        return FCPP_OK;
    }
    DevTiling &t = b->til0;
    HIPCHK(hipMemsetAsync(t.n_adj.p, 0, (size_t)t.n_paths * sizeof(unsigned long long), st));
    STAGE(0, launch_generate(st, t.n_tiles, t.tiles.p, b->t.fields, b->t.prims, b->cst, x, y, v, fs));
    STAGE(1, launch_curv_clamp(st, t.n_tiles, t.tiles.p, t.paths.p, b->cst, 1, x, y, v, v, kappa, t.n_adj.p));
    STAGE(2, launch_scan_tiles(st, t.n_tiles, t.tiles.p, t.paths.p, b->cst, x, y, v, t.agg_f.p, t.agg_b.p));
    STAGE(3, launch_scan_spine(st, t.n_tiles, t.agg_f.p, t.agg_b.p, t.carry_f.p, t.carry_b.p, t.spine.p));
    STAGE(4, launch_scan_apply(st, t.n_tiles, t.tiles.p, t.paths.p, b->cst, 3, x, y, v, v, t.carry_f.p, t.carry_b.p));
    STAGE(5, launch_validate(st, t.n_tiles, t.tiles.p, t.paths.p, b->t.fields, b->cst, obs, x, y, kappa, v, fs, t.partial.p));
    STAGE(6, launch_reduce_stats(st, t.n_paths, t.partial.p, t.tile_first.p, t.n_adj.p, stats));
#undef STAGE
    if (ev) ++b->prof_runs;
    return FCPP_OK;
}

int fcpp_batch_plan(fcpp_ctx *c, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields, const fcpp_field *fields,
                    const fcpp_polys *obstacles, fcpp_field_stats *stats, fcpp_batch **batch, double **x, double **y, double **kappa, double **v,
                    uint32_t **fs, int64_t *total_points)
{
    if (!batch || !x || !y || !kappa || !v || !fs) return fail(FCPP_EINVAL, "bad arguments");
    *batch = nullptr; *x = *y = *kappa = *v = nullptr; *fs = nullptr;
    fcpp_batch *b = nullptr;
    static const bool trace = getenv("FCPP_TRACE_PLAN") != nullptr;      // (diagnostic: the host's side of a plan call, microseconds since its start, to stderr)
    const auto t_begin = std::chrono::steady_clock::now();
    // (outputs are wanted: a speculative device setup may allocate the arrays itself, from the early point total, and run the step directly
    // behind its counting pass -- fcpp_setup.cpp: DeviceSetup)
    PlanOutputs po;
    po.stats = stats;
    int rc = batch_create(c, veh, opt, n_fields, fields, obstacles, &b, &po);
    if (rc != FCPP_OK || (po.allocated && po.points != b->hp.total_points)) {       // (the arrays of a setup that did not end as it began)
        if (po.allocated) { const std::string keep = g_err; (void)hipStreamSynchronize(c->stream); (void)fcpp_outputs_free(c, po.x); g_err = keep; }
        po.allocated = false;
    }
    if (rc != FCPP_OK) return rc;
    const double t_create = trace ? ms_since(t_begin) : 0.0;
    const int64_t total = b->hp.total_points;
    if (po.allocated) { *x = po.x; *y = po.y; *kappa = po.kappa; *v = po.v; *fs = po.fs; }
    else rc = fcpp_outputs_alloc(c, total, 0, x, y, kappa, v, fs);
    const double t_alloc = trace ? ms_since(t_begin) : 0.0;
    if (rc == FCPP_OK && po.stepped) {
        // the step has run: what fcpp_batch_run notes besides its launches (the batch's stream was noted at creation)
        b->last_mode = 1;
        note_arena_writer(c, *x, c->stream);
        if (trace) fprintf(stderr, "[fcpp] plan call, direct step: totals seen %.1f us, create returns %.1f\n", g_trace_totals_ms * 1e3, t_create * 1e3);
    } else if (rc == FCPP_OK) {
        if (!stats) stats = b->t.own_stats;
        rc = fcpp_batch_run(b, *x, *y, *kappa, *v, *fs, stats, 1);
        if (trace) fprintf(stderr, "[fcpp] plan call: entered at %.1f us (CLOCK_MONOTONIC mod 1 s), totals seen %.1f us, create returns %.1f, arrays %.1f, step enqueued %.1f\n",
                           (double)(std::chrono::duration_cast<std::chrono::nanoseconds>(t_begin.time_since_epoch()).count() % 1000000000ll) / 1e3,
                           g_trace_totals_ms * 1e3, t_create * 1e3, t_alloc * 1e3, ms_since(t_begin) * 1e3);
        if (rc != FCPP_OK) { const std::string keep = g_err; (void)hipStreamSynchronize(c->stream); (void)fcpp_outputs_free(c, *x); g_err = keep; }
    }
    if (rc != FCPP_OK) {
        const std::string keep = g_err;
        (void)fcpp_batch_destroy(b);
        *x = *y = *kappa = *v = nullptr; *fs = nullptr;
        g_err = keep;
        return rc;
    }
    *batch = b;
    if (total_points) *total_points = total;
    return FCPP_OK;
}

int fcpp_batch_own_stats(const fcpp_batch *b, fcpp_field_stats **stats)
{
    if (!b || !stats) return fail(FCPP_EINVAL, "bad arguments");
    *stats = b->t.own_stats;
    return FCPP_OK;
}

int fcpp_batch_set_profiling(fcpp_batch *b, int enable)
{
    if (!b) return fail(FCPP_EINVAL, "batch is NULL");
    HIPCHK(hipSetDevice(b->ctx->device));
    if (enable && b->events.empty()) {
        b->events.resize((size_t)kProfRuns * kStages * 2);
        b->ev_set.assign((size_t)kProfRuns * kStages, 0);
        for (hipEvent_t &e : b->events) HIPCHK(hipEventCreate(&e));
    }
    b->profiling = enable > 0 ? enable : 0;
    b->prof_runs = 0; b->run_counter = 0;
    return FCPP_OK;
}

int fcpp_batch_stage_times(fcpp_batch *b, int max_stages, double *ms_sum, int *n_stages, int *n_runs)
{
    if (!b || !ms_sum || max_stages < kStages) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    const int ns = kStageCount[b->last_mode];
    for (int k = 0; k < kStages; ++k) ms_sum[k] = 0.0;
    for (int r = 0; r < b->prof_runs; ++r) {
        hipEvent_t *ev = &b->events[(size_t)r * kStages * 2];
        for (int k = 0; k < ns; ++k) {
            if (!b->ev_set[(size_t)r * kStages + k]) continue;      // the stage had nothing to launch
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
            ms_sum[k] += ms;
        }
    }
    if (n_stages) *n_stages = ns;
    if (n_runs) *n_runs = b->prof_runs;
    b->prof_runs = 0;
    return FCPP_OK;
}

int fcpp_batch_stage_points(const fcpp_batch *b, int mode, int stage, int64_t *points)
{
    if (!b || !points || mode < 0 || mode > 1 || stage < 0 || stage >= kStageCount[mode]) return fail(FCPP_EINVAL, "bad arguments");
    const ImageLayout &t = b->lay;
    const int64_t all = b->hp.total_points;
    if (mode == 0) { *points = all; return FCPP_OK; }         // every staged kernel sees every point
    const int64_t per_stage[6] = { t.span_points, t.chunk_points, t.wave_points - t.work_wave_points, all - t.quiet_points - t.wave_points, all,
                                   t.work_wave_points + t.work_span_points };
    *points = per_stage[stage];
    return FCPP_OK;
}

int fcpp_batch_point_split(const fcpp_batch *b, int64_t *quiet_points, int64_t *general_points)
{
    if (!b) return fail(FCPP_EINVAL, "batch is NULL");
    const int64_t q = b->lay.quiet_points;
    if (quiet_points) *quiet_points = q;
    if (general_points) *general_points = b->hp.total_points - q;
    return FCPP_OK;
}

int fcpp_batch_reduce_classes(const fcpp_batch *b, int64_t *classes_out)
{
    if (!b || !classes_out) return fail(FCPP_EINVAL, "bad arguments");
    for (int c = 0; c < 4; ++c) classes_out[c] = b->lay.n_red[c];
    return FCPP_OK;
}

const char *fcpp_batch_stage_name(int mode, int stage)
{
    return (mode >= 0 && mode < 2 && stage >= 0 && stage < kStages) ? kStageNames[mode][stage] : "";
}

int fcpp_batch_connectors(fcpp_batch *b, double *approach_xy, double *departure_xy)
{
    if (!b) return fail(FCPP_EINVAL, "batch is NULL");
    if (b->n_fields == 0) return FCPP_OK;
    HIPCHK(hipSetDevice(b->ctx->device));
    hipStream_t st = b->ctx->stream;
    b->note_stream(st);
    { const int rc = ensure_tables(b); if (rc) return rc; }
    HIPCHK(b->wait_setup(st));
    if (approach_xy) LAUNCHCHK(launch_straight(st, b->n_fields, b->t.seg, 50, b->t.seg_mask, approach_xy));
    if (departure_xy)
        LAUNCHCHK(launch_straight(st, b->n_fields, b->t.seg + 4 * b->n_fields, 50, b->t.seg_mask + b->n_fields, departure_xy));
    return FCPP_OK;
}

int fcpp_batch_destroy(fcpp_batch *b)
{
    if (!b) return FCPP_OK;
    fcpp_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    if (b->tables_pending) {      // (a fill pass nobody asked for is dropped, not run)
        b->tables_pending = false;
        if (b->tables_slot >= 0 && c->plan_slots[b->tables_slot].tables_batch == b) c->plan_slots[b->tables_slot].tables_batch = nullptr;
    }
    // (the tables may become the next batch's: nothing that reads them may still be running -- on whichever streams this batch ran)
    // (every stream the batch was created, stepped or read on is noted in used_streams; the context's CURRENT stream is not drained for its own
    // sake: it may be another batch's -- a caller with two plan calls in flight on two streams would wait for the other call's step here)
    for (hipStream_t s : b->used_streams) (void)hipStreamSynchronize(s);
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (b->slab) {      // the larger of this allocation and the context's spare stays for the next batch
        if (b->slab_bytes <= kSpareMax && b->slab_bytes > c->spare_cap) {
            if (c->spare) (void)hipFree(c->spare);
            c->spare = b->slab; c->spare_cap = b->slab_bytes;
        } else (void)hipFree(b->slab);
        b->slab = nullptr;
    }
    if (b->ev_setup && c->ev_pool.size() < 64) { c->ev_pool.push_back(b->ev_setup); b->ev_setup = nullptr; }
    delete b;
    return FCPP_OK;
}

int fcpp_batch_trajectory(fcpp_batch *b, const double *x, const double *y, const double *v, const uint32_t *flagseg, double *s, double *t,
                          double *heading, double *totals)
{
    if (!b) return fail(FCPP_EINVAL, "batch is NULL");
    if (b->n_fields == 0) return FCPP_OK;
    if (b->hp.total_points > 0 && (!x || !y || !v)) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(b->ctx->device));
    { const int rc = ensure_info(b); if (rc) return rc; }
    // two paths per field: main work, then headland (a field that raised: two empty paths)
    std::vector<int64_t> offs;
    try { offs.assign(2 * (size_t)b->n_fields + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < b->n_fields; ++i) {
        const fcpp_field_info &fi = b->hp.info[(size_t)i];
        offs[2 * (size_t)i + 1] = offs[2 * (size_t)i] + fi.n_main;
        offs[2 * (size_t)i + 2] = offs[2 * (size_t)i + 1] + fi.n_head;
    }
    hipStream_t st = b->ctx->stream;
    b->note_stream(st);
    HIPCHK(b->wait_setup(st));
    return trajectory_paths(b->ctx, 2 * b->n_fields, nullptr, offs.data(), b->hp.total_points, x, y, v, flagseg, s, t, heading, totals);
}

namespace {
// One fcpp_ga_evolve call, step by step: setup, check_permutations, one of the two loops (loop_one_launch / loop_two_streams), read_back.
struct GaRun {
    fcpp_ctx *const c; const int n, pop; const fcpp_ga_config &cfg;
    const double *const D; int32_t *const routes, *const best_route; double *const hist;      // the call's arguments
    hipStream_t st = nullptr;
    DevBuf<int32_t> scratch;
    DevBuf<double> fd;             // fitness / distance of both buffers
    DevBuf<GaState> state;
    int32_t *buf[2] = { nullptr, nullptr };
    double *fit[2] = { nullptr, nullptr }, *dist[2] = { nullptr, nullptr };
    volatile unsigned long long *mir = nullptr;     // the mirror word, or null: no such word
    GaState h = {};

    // argument checks, the buffers, and the run's progress in a word of pinned memory the bookkeeping role writes (GaState::mirror):
    // followed without draining the stream
    int setup()
    {
        if (n < 2 || n > GA_MAX_NODES) return fail(FCPP_EUNSUPPORTED, "n_nodes must be in [2, 2048]");
        if (pop < 2 || (pop & 1) || cfg.elite_size < 0 || cfg.elite_size >= pop || cfg.tournament_size < 1 ||
            cfg.tournament_size > 64 || cfg.tournament_size > pop || cfg.max_generations < 0)
            return fail(FCPP_EINVAL, "population_size must be even and > elite_size; 1 <= tournament_size <= min(64, population_size)");
        HIPCHK(hipSetDevice(c->device));
        st = c->stream;
        HIPCHK(scratch.alloc((size_t)pop * n));
        HIPCHK(fd.alloc((size_t)pop * 4));
        HIPCHK(state.alloc(1));
        HIPCHK(hipMemsetAsync(state.p, 0, sizeof(GaState), st));
        buf[0] = routes; buf[1] = scratch.p;
        fit[0] = fd.p; fit[1] = fd.p + 2 * (size_t)pop; dist[0] = fd.p + pop; dist[1] = fd.p + 3 * (size_t)pop;
        if (!c->ga_mirror && hipHostMalloc((void **)&c->ga_mirror, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { c->ga_mirror = nullptr; (void)hipGetLastError(); }
        mir = c->ga_mirror;
        void *mirror_dp = nullptr;                      // (the word as the device addresses it; lives until the copy below has read it)
        if (mir) {
            *mir = 0ull;
            if (hipHostGetDevicePointer(&mirror_dp, c->ga_mirror, 0) == hipSuccess && mirror_dp) {
                HIPCHK(hipMemcpyAsync(reinterpret_cast<unsigned char *>(state.p) + offsetof(GaState, mirror), &mirror_dp, sizeof mirror_dp, hipMemcpyHostToDevice, st));
                HIPCHK(hipStreamSynchronize(st));       // (once per run, in front of its first launch)
            } else { mir = nullptr; (void)hipGetLastError(); }
        }
        return FCPP_OK;
    }

    // the initial population must consist of permutations: the kernels index D and their LDS marks by gene
    int check_permutations()
    {
        DevBuf<int32_t> bad;
        int32_t hb = 0;
        HIPCHK(bad.alloc(1));
        HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(int32_t), st));
        LAUNCHCHK(launch_ga_check_perm(st, n, pop, routes, bad.p));
        HIPCHK(hipMemcpyAsync(&hb, bad.p, sizeof hb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (hb) return fail(FCPP_EINVAL, "routes must hold permutations of 0 .. n_nodes-1");
        return FCPP_OK;
    }

    // the pipelined convergence check (round 5b): has the bookkeeping of generation g - 63 been done (mirror word: generations >= g - 63)?
    // -> 1: the run has converged, 0: go on, -1: no mirror word / not seen within 2 s (progress() falls back to a copy back + drained stream)
    int follow(int g) const
    {
        if (!mir) return -1;
        const auto t_wait = std::chrono::steady_clock::now();
        for (int spin = 0;; ++spin) {
            const unsigned long long w = *mir;
            if ((w >> 32) != 0) return 1;
            if ((long long)(w & 0xffffffffull) >= (long long)g - 63) return 0;
            if ((spin & 4095) == 4095 && ms_since(t_wait) > 2000.0) return -1;
        }
    }

    // Both loops' look at the run after every 32nd generation's launches (the kernels are no-ops once converged; stop launching them) -> stop.
    // Round 5b: the check is PIPELINED.  The bookkeeping role of launch L leaves `generations` = L in the mirror word, so the
    // host waits -- on that word, not on the stream -- only until launch g - 63 is through: two blocks of 32 launches are in
    // flight at most, the device never runs dry at a check (it used to: a copy back and a drained stream every 32 generations,
    // ~20 us of idle device each = 0.5 us of a generation's 10), and a converged run is noticed within 64 launches (no-ops by then).
    // drain: the stream the bookkeeping runs on, for the fallback.  -> 1: stop, 0: go on, < 0: an error code
    int progress(int g, hipStream_t drain)
    {
        const int f = follow(g);
        if (f >= 0) return f;
        HIPCHK(hipMemcpyAsync(&h, state.p, sizeof h, hipMemcpyDeviceToHost, drain));
        HIPCHK(hipStreamSynchronize(drain));
        return h.converged ? 1 : 0;
    }

    // One launch per generation (k_ga_generation): the population in buffer a -> its statistics and elites (the bookkeeping of
    // generation g - 1) and its children (generation g) at once; the launch after the last generation only evaluates the final
    // population.  cfg4: 77 -> 55 us per generation (45 us with the DPP arg-max of the elite selection).
    int loop_one_launch()
    {
        for (int g = 0; g <= cfg.max_generations; ++g) {
            const int a = g & 1, b = a ^ 1;
            LAUNCHCHK(launch_ga_generation(st, c->n_cu, n, pop, D, buf[a], fit[a], dist[a], buf[b], fit[b], dist[b], cfg, g, state.p, best_route, hist));
            if ((g & 31) == 31) {
                const int p = progress(g, st);
                if (p < 0) return p;
                if (p) break;
            }
        }
        return FCPP_OK;
    }

    // Larger tours: two launches per generation on two streams.  Population g + 1 (buffer b) = the children k_ga_pairs(g) makes of population g (buffer a) + the elites of population
    // g, which k_ga_stats_elite(g - 1) copied into b's last rows while it evaluated population g.  So k_ga_stats_elite(g) -- statistics
    // of population g + 1, its elites into a's last rows -- and k_ga_pairs(g + 1) -- children of population g + 1 into a's other rows --
    // need the same two predecessors (k_ga_pairs(g), k_ga_stats_elite(g - 1)) and write disjoint rows: they run side by side, the pairs on the context's stream, the
    // single-workgroup bookkeeping (the longer of the two) on its side stream, a generation costs the longer kernel instead of the sum
    // (measured on cfg4, which normally takes the one-launch path: 77 -> 72 us, the cross-stream waits cost ~13 us a generation).  The pairs of the generation that follows convergence may still run (they read the flag at their start):
    // they write the buffer that is NOT the final population.
    int loop_two_streams()
    {
        LAUNCHCHK(launch_ga_stats_elite(st, n, pop, buf[0], fit[0], dist[0], buf[1], fit[1], dist[1], cfg, -1, state.p, best_route, hist));
        struct Events {
            hipEvent_t p[2] = { nullptr, nullptr }, s[2] = { nullptr, nullptr };
            ~Events() { for (int k = 0; k < 2; ++k) { if (p[k]) (void)hipEventDestroy(p[k]); if (s[k]) (void)hipEventDestroy(s[k]); } }
        } ev;
        for (int k = 0; k < 2; ++k) {
            HIPCHK(hipEventCreateWithFlags(&ev.p[k], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&ev.s[k], hipEventDisableTiming));
        }
        hipStream_t sd = c->side;
        HIPCHK(hipEventRecord(ev.s[1], st));              // k_ga_stats_elite(-1) ran on the main stream
        HIPCHK(hipStreamWaitEvent(sd, ev.s[1], 0));
        HIPCHK(hipEventRecord(ev.s[0], st));              // (so that every event a stream waits on has been recorded)
        for (int g = 0; g < cfg.max_generations; ++g) {
            const int a = g & 1, b = a ^ 1;               // generation g: buffer a -> buffer b
            HIPCHK(hipStreamWaitEvent(st, ev.s[g & 1], 0));                // the elites of population g are in a: k_ga_stats_elite(g - 2)
            LAUNCHCHK(launch_ga_pairs(st, n, pop, D, buf[a], fit[a], buf[b], fit[b], dist[b], cfg, g, state.p));
            HIPCHK(hipEventRecord(ev.p[g & 1], st));
            HIPCHK(hipStreamWaitEvent(sd, ev.p[g & 1], 0));                 // the children of population g are in b
            LAUNCHCHK(launch_ga_stats_elite(sd, n, pop, buf[b], fit[b], dist[b], buf[a], fit[a], dist[a], cfg, g, state.p, best_route, hist));
            HIPCHK(hipEventRecord(ev.s[g & 1], sd));
            if ((g & 31) == 31) {
                const int p = progress(g, sd);
                if (p < 0) return p;
                if (p) break;
            }
        }
        HIPCHK(hipStreamSynchronize(sd));
        return FCPP_OK;
    }

    // the state comes back; the final population goes to `routes` if the last completed generation left it in the scratch buffer
    int read_back(fcpp_ga_result *result)
    {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpyAsync(&h, state.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h.generations & 1)                             // the last completed generation wrote the scratch buffer
            HIPCHK(hipMemcpyAsync(routes, scratch.p, (size_t)pop * n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        result->generations = h.generations;                               // GA:122-127 (generation + 1)
        result->convergence_gen = h.generations - 1 - h.gwi;
        result->best_distance = h.best_dist;
        result->best_fitness = h.best_fit;
        return FCPP_OK;
    }
};
}  // namespace

int fcpp_ga_evolve(fcpp_ctx *c, int32_t n, const fcpp_ga_config *cfg, const double *D, int32_t *routes, int32_t *best_route,
                   double *hist, fcpp_ga_result *result)
{
    if (!c || !cfg || !D || !routes || !best_route || !result) return fail(FCPP_EINVAL, "bad arguments");
    GaRun r{ c, n, cfg->population_size, *cfg, D, routes, best_route, hist };
    int rc;
    if ((rc = r.setup()) != FCPP_OK) return rc;
    if ((rc = r.check_permutations()) != FCPP_OK) return rc;
    LAUNCHCHK(launch_ga_fitness(r.st, n, r.pop, D, routes, r.dist[0], r.fit[0], 0));                       // GA:64
    rc = ga_launch_plan(n, r.pop, c->n_cu).one_launch ? r.loop_one_launch() : r.loop_two_streams();
    if (rc != FCPP_OK) return rc;
    return r.read_back(result);
}

int fcpp_cover_grid(fcpp_ctx *c, int64_t n_jobs, const fcpp_cover_job *jobs, int64_t n_pts, const double *px, const double *py,
                    uint8_t *grid, int64_t *counts)
{
    if (!c || n_jobs < 0 || (n_jobs > 0 && (!jobs || !counts))) return fail(FCPP_EINVAL, "bad arguments");
    if (n_jobs == 0) return FCPP_OK;
    std::vector<DevCoverJob> dj((size_t)n_jobs);
    int64_t tiles = 0;
    for (int64_t k = 0; k < n_jobs; ++k) {
        const fcpp_cover_job &j = jobs[k];
        if (j.nx < 0 || j.ny < 0 || j.n_a < 0 || j.n_b < 0 || !(j.res > 0) || !(j.radius >= 0) || j.pts_first < 0 ||
            j.pts_first + j.n_a + j.n_b > n_pts || ((j.n_a > 0 || j.n_b > 0) && (!px || !py)) || (j.grid_first >= 0 && !grid))
            return fail(FCPP_EINVAL, "bad coverage job");
        DevCoverJob &d = dj[(size_t)k];
        d.ox = j.ox; d.oy = j.oy; d.res = j.res; d.shift = j.shift; d.radius = j.radius;
        d.nx = j.nx; d.ny = j.ny; d.n_a = j.n_a; d.n_b = j.n_b; d.pts_first = j.pts_first; d.grid_first = j.grid_first;
        d.strict = j.strict; d.region = j.region;
        memcpy(d.outer, j.outer, sizeof d.outer); memcpy(d.inner, j.inner, sizeof d.inner);
        d.tiles_x = (j.nx + 63) / 64; d.tiles_y = (j.ny + 63) / 64;
        d.tile_first = tiles;
        tiles += (int64_t)d.tiles_x * d.tiles_y;
    }
    if (tiles > 0x7fffffffLL) return fail(FCPP_ESIZE, "coverage grids too large for one call");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf<DevCoverJob> dev;
    HIPCHK(dev.upload(dj, st));
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)n_jobs * 3 * sizeof(int64_t), st));
    LAUNCHCHK(launch_cover(st, n_jobs, tiles, dev.p, px, py, grid, reinterpret_cast<unsigned long long *>(counts)));
    HIPCHK(hipStreamSynchronize(st));      // the job table dies here
    return FCPP_OK;
}

int fcpp_ga_fitness(fcpp_ctx *c, int32_t n_nodes, int64_t pop, const double *D, const int32_t *routes, double *dist,
                    double *fit, int order_mode)
{
    if (!c || n_nodes < 1 || pop < 0 || (pop > 0 && (!D || !routes)) || (order_mode != 0 && order_mode != 1))
        return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_ga_fitness(c->stream, n_nodes, pop, D, routes, dist, fit, order_mode));
    return FCPP_OK;
}

// ---- the final gather of a sharded job over RCCL -------------------------------------------------------------------------
// RCCL is not linked: its four entry points are looked up in the process (a caller that holds an ncclComm_t has the library loaded;
// PyTorch's ROCm wheels bundle their own copy), then by name.
extern "C++" {
namespace {
struct Rccl {
    int (*group_start)() = nullptr;
    int (*group_end)() = nullptr;
    int (*send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    bool ok() const { return group_start && group_end && send && recv; }
};
const Rccl &rccl()
{
    static const Rccl r = [] {
        Rccl q;
        auto look = [&](void *h) {
            q.group_start = reinterpret_cast<int (*)()>(dlsym(h, "ncclGroupStart"));
            q.group_end = reinterpret_cast<int (*)()>(dlsym(h, "ncclGroupEnd"));
            q.send = reinterpret_cast<int (*)(const void *, size_t, int, int, void *, hipStream_t)>(dlsym(h, "ncclSend"));
            q.recv = reinterpret_cast<int (*)(void *, size_t, int, int, void *, hipStream_t)>(dlsym(h, "ncclRecv"));
        };
        look(RTLD_DEFAULT);
        for (const char *name : { "librccl.so.1", "librccl.so" }) {
            if (q.ok()) break;
            if (void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) look(h);
        }
        return q;
    }();
    return r;
}
}  // namespace
}  // extern "C++"

int fcpp_gather(fcpp_ctx *c, void *nccl_comm, int rank, int world, int root, int n_arrays, const void *const *send_dev, const int32_t *elem_bytes,
                const int64_t *counts_per_rank, void *const *recv_dev, int flags)
{
    if (!c || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || n_arrays < 0 || !counts_per_rank ||
        (n_arrays > 0 && (!send_dev || !elem_bytes)) || (rank == root && n_arrays > 0 && !recv_dev))
        return fail(FCPP_EINVAL, "bad arguments");
    for (int r = 0; r < world; ++r) if (counts_per_rank[r] < 0) return fail(FCPP_ESIZE, "negative count");
    for (int a = 0; a < n_arrays; ++a) if (elem_bytes[a] <= 0) return fail(FCPP_ESIZE, "element size must be positive");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool self_through_comm = (flags & 1) != 0;
    const bool need_comm = world > 1 || (self_through_comm && counts_per_rank[rank] > 0);
    if (need_comm && (!nccl_comm || !rccl().ok())) return fail(FCPP_EUNSUPPORTED, nccl_comm ? "RCCL (ncclSend / ncclRecv) is not available in this process" : "nccl_comm is NULL");
    std::vector<int64_t> first((size_t)world + 1, 0);
    for (int r = 0; r < world; ++r) first[(size_t)r + 1] = first[(size_t)r] + counts_per_rank[r];
    // one group: the root posts a receive per peer and array straight into the slice of its full array, every peer one send per array --
    // point to point, each peer over its own xGMI link to the root (no ring, no staging, no concatenation)
    bool grouped = false;
#define NCCLCHK(expr) do { const int e_ = (expr); if (e_ != 0) { if (grouped) (void)rccl().group_end(); return fail(FCPP_EHIP, std::string(#expr) + ": RCCL error " + std::to_string(e_)); } } while (0)
    // (the root's own block: a plain copy, enqueued BEFORE the group opens -- an error return inside an open group would leave the communicator in group mode)
    if (rank == root && !self_through_comm && counts_per_rank[rank] > 0)
        for (int a = 0; a < n_arrays; ++a) {
            const size_t eb = (size_t)elem_bytes[a];
            char *dst = static_cast<char *>(recv_dev[a]) + (size_t)first[(size_t)rank] * eb;
            if (dst != send_dev[a]) HIPCHK(hipMemcpyAsync(dst, send_dev[a], (size_t)counts_per_rank[rank] * eb, hipMemcpyDeviceToDevice, st));
        }
    if (need_comm) { NCCLCHK(rccl().group_start()); grouped = true; }
    for (int a = 0; a < n_arrays; ++a) {
        const size_t eb = (size_t)elem_bytes[a];
        if (rank == root) {
            char *full = static_cast<char *>(recv_dev[a]);
            for (int r = 0; r < world; ++r) {
                const size_t bytes = (size_t)counts_per_rank[r] * eb;
                if (bytes == 0) continue;
                char *dst = full + (size_t)first[(size_t)r] * eb;
                if (r == rank && !self_through_comm) continue;
                else NCCLCHK(rccl().recv(dst, bytes, /* ncclInt8 */ 0, r, nccl_comm, st));
            }
            if (self_through_comm && counts_per_rank[rank] > 0)
                NCCLCHK(rccl().send(send_dev[a], (size_t)counts_per_rank[rank] * eb, 0, rank, nccl_comm, st));
        } else if (counts_per_rank[rank] > 0) {
            NCCLCHK(rccl().send(send_dev[a], (size_t)counts_per_rank[rank] * eb, 0, root, nccl_comm, st));
        }
    }
    if (grouped) { grouped = false; NCCLCHK(rccl().group_end()); }
#undef NCCLCHK
    return FCPP_OK;
}

// ---- diagnostics (tests) -------------------------------------------------------------------------------------------------------------
int fcpp_debug_math(int fn, int64_t n, const double *a, const double *b, double *out0, double *out1)
{
    if (fn < 0 || fn > 5 || n < 0 || (n > 0 && (!a || !out0)) || ((fn == 1 || fn == 3 || fn == 5) && n > 0 && !b) || ((fn == 0 || fn == 4) && n > 0 && !out1))
        return fail(FCPP_EINVAL, "bad arguments");
    for (int64_t i = 0; i < n; ++i) {
        if (fn == 0) fc_sincos(a[i], out0[i], out1[i]);
        else if (fn == 4) fc_sincos_cr(a[i], out0[i], out1[i]);
        else if (fn == 5) out0[i] = fc_atan2_cr(a[i], b[i]);
        else if (fn == 1) out0[i] = atan2_fd(a[i], b[i]);
        else if (fn == 2) out0[i] = fc_acos(a[i]);
        else out0[i] = fc_hypot(a[i], b[i]);
    }
    return FCPP_OK;
}

int fcpp_debug_offsets(int64_t n, int n_cols, const int64_t *counts, int64_t *prefix, int64_t *totals)
{
    if (n < 1 || n > OFF_FIELDS_MAX || n_cols < 1 || n_cols > PC_COLS || !counts || !prefix || !totals) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<int64_t> agg((size_t)OFF_WORDS);
    for (int col = 0; col < n_cols; ++col) {
        offset_aggregate(counts, n, col, agg.data());
        for (int64_t i = 0; i < n; ++i) prefix[(int64_t)col * n + i] = offset_prefix(agg.data(), counts, n, col, i);
        totals[col] = offset_total(agg.data(), n, col);
    }
    return FCPP_OK;
}

int fcpp_debug_setup_rule(int what, const int64_t *in, int64_t *out)
{
    if (what < 0 || what > 3 || !in || !out) return fail(FCPP_EINVAL, "bad arguments");
    if (what == 0) {
        const SetupAcceptIn a = { (int)in[0], in[1], in[2], (int)in[3], in[4] != 0, (int)in[5], DEVPLAN_PRIMS_CAP };
        out[0] = setup_accept(a);
    } else if (what == 1) {
        const SetupBeginIn a = { in[0], devplan_small_blocks(), in[1] != 0, in[2] != 0, (uint64_t)in[3], in[4] != 0, in[5] != 0, in[6] != 0, in[7] != 0, in[8] != 0 };
        const SetupBegin r = setup_begin(a);
        out[0] = r.spec; out[1] = r.direct; out[2] = setup_wants_capacities(a);
    } else if (what == 2) {
        const SetupEndIn a = { in[0] != 0, in[1] != 0, in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10] != 0, in[11] != 0 };
        const SetupEnd r = setup_end(a);
        out[0] = r.fuse; out[1] = r.within; out[2] = r.qualifies; out[3] = r.taken; out[4] = r.refill;
    } else {
        if (in[0] < 0 || in[0] > 4096) return fail(FCPP_EINVAL, "bad arguments");
        fcpp_ctx::PlanSlot slot;
        for (int64_t k = 0; k < in[0]; ++k) {
            const int64_t ev = in[1 + k];
            if (ev < 0 || ev > 2) return fail(FCPP_EINVAL, "bad arguments");
            if (ev == 2) { static_cast<SlotAggregates &>(slot) = SlotAggregates(); out[2 * k] = out[2 * k + 1] = -1; continue; }
            const AggBegin r = slot.begin_aggregates();
            if (ev == 0) slot.aggregates_settled();
            out[2 * k] = r.clear_both; out[2 * k + 1] = r.use_second;
        }
    }
    return FCPP_OK;
}

int fcpp_debug_ga_launch_plan(fcpp_ctx *c, int32_t n, int32_t pop, int32_t *out)
{
    if (!c || !out || n < 2 || n > GA_MAX_NODES || pop < 2 || (pop & 1)) return fail(FCPP_EINVAL, "bad arguments");
    const GaLaunchPlan p = ga_launch_plan(n, pop, c->n_cu);
    out[0] = p.one_launch ? 1 : 0; out[1] = (int32_t)p.groups; out[2] = p.base; out[3] = p.extra; out[4] = p.per_wg; out[5] = (int32_t)p.lds;
    return FCPP_OK;
}

int fcpp_debug_math_dev(fcpp_ctx *c, int fn, int64_t n, const double *a, const double *b, double *out0, double *out1)
{
    if (!c || fn < 0 || fn > 5 || n < 0) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    LAUNCHCHK(launch_debug_math(c->stream, fn, n, a, b, out0, out1));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPP_OK;
}

int fcpp_debug_dubins(int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty, const double *th,
                      double radius, int32_t *word, double *seg, double *len)
{
    return debug_conn<0>(n, fx, fy, fh, tx, ty, th, radius, word, seg, len);
}

int fcpp_debug_rs(int64_t n, const double *fx, const double *fy, const double *fh, const double *tx, const double *ty, const double *th,
                  double radius, int32_t *word, double *seg, double *len)
{
    return debug_conn<1>(n, fx, fy, fh, tx, ty, th, radius, word, seg, len);
}

int fcpp_ctx_direct_steps(const fcpp_ctx *c, int64_t *launched, int64_t *taken, int64_t *fills)
{
    if (!c) return fail(FCPP_EINVAL, "ctx is NULL");
    if (launched) *launched = c->direct_steps;
    if (taken) *taken = c->direct_taken;
    if (fills) *fills = c->direct_fills;
    return FCPP_OK;
}

int fcpp_ctx_cut_rows_passes(const fcpp_ctx *c, int64_t *passes)
{
    if (!c || !passes) return fail(FCPP_EINVAL, "bad arguments");
    *passes = c->cut_rows_passes;
    return FCPP_OK;
}

int fcpp_batch_debug_table(const fcpp_batch *b, int table, void *dst, int64_t cap, int64_t *bytes_out)
{
    if (!b || !bytes_out) return fail(FCPP_EINVAL, "bad arguments");
    // (the numbers are the ABI's: tests/test_gpu_devplan.py lists them in this order)
    static const SlabTable kTables[] = { ST_fields, ST_prims, ST_tiles, ST_wtiles, ST_general_ids, ST_chunks, ST_span_chunks, ST_stat_ids, ST_stat_first, ST_stat_run,
                                         ST_red_paths, ST_field_work, ST_open_wave_ids, ST_seg, ST_seg_mask, ST_partial, ST_field_junc, ST_work_totals,
                                         ST_obs_off, ST_obs_x, ST_obs_y, ST_obs_bbox, ST_field_packs };
    if (table < 0 || table >= (int)(sizeof(kTables) / sizeof(kTables[0]))) return fail(FCPP_EINVAL, "no such table");
    const SlabSpan sp = slab_table(b->lay, kTables[table]);
    *bytes_out = (int64_t)sp.bytes;
    if (!dst) return FCPP_OK;
    if (cap < (int64_t)sp.bytes) return fail(FCPP_ESIZE, "buffer too small");
    if (sp.bytes == 0 || b->lay.n_fields == 0) return FCPP_OK;
    HIPCHK(hipSetDevice(b->ctx->device));
    { const int rc = ensure_tables(const_cast<fcpp_batch *>(b)); if (rc) return rc; }
    for (hipStream_t s : b->used_streams) HIPCHK(hipStreamSynchronize(s));          // (the setup's stream is one of them)
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    HIPCHK(hipMemcpy(dst, static_cast<const unsigned char *>(b->slab) + sp.off, sp.bytes, hipMemcpyDeviceToHost));
    return FCPP_OK;
}

}  // extern "C"
