// fcpp_batch.h -- a batch and its setup: what fcpp_setup.cpp (fcpp_batch_create's work: templates, the device setup in phases, the host path)
// and fcpp_api.cpp (the C entries that step and read a batch) share.  Private to csrc/, host code only.
#pragma once
#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "fcpp_api_internal.h"
#include "fcpp_devplan.h"

namespace fcpp {
// The turn templates of a batch (every field shares the vehicle and the sampling options, hence the shape and the sample count of
// its U-turns and corner turns): sampled once on the device (k_build_templates), copied back for the tiler's halo sizing and the
// closed-form test.  A context keeps the last set: a caller that creates batch after batch with one vehicle (the planner mirror does,
// one per plan_complete_coverage) pays for the two launches and the copy once.
struct TemplateSet {
    TurnTemplates tt;
    double clothoid_frac = 0.0;
    DevBuf<CacShape> shapes;                       // [0] 180-degree, [1] 90-degree clothoid-arc-clothoid unit shapes
    DevBuf<double2> tmpl_u, tmpl_c, tmpl_u_dk;     // sampled turn templates (fcpp_fused.hip), (segment length, curvature) per U-turn sample
    DevBuf<double2> tmpl_c_dk;                     // the same per corner-turn sample (the closed-form cut's chord table, fcpp_cutfn.h)
    std::vector<double2> h_tu, h_tc, h_dk, h_dkc;  // host copies
    double tc_lo[2] = { 0.0, 0.0 }, tc_hi[2] = { 0.0, 0.0 };      // the corner template's box (from h_tc; template_box())
    bool box_done = false;
    void template_box()                            // (needs the host copies: after the stream that fetched them has been drained)
    {
        if (box_done) return;
        for (int d = 0; d < 2; ++d) { tc_lo[d] = 0.0; tc_hi[d] = 0.0; }
        for (size_t k = 0; k < h_tc.size(); ++k) {
            tc_lo[0] = std::min(tc_lo[0], h_tc[k].x); tc_hi[0] = std::max(tc_hi[0], h_tc[k].x);
            tc_lo[1] = std::min(tc_lo[1], h_tc[k].y); tc_hi[1] = std::max(tc_hi[1], h_tc[k].y);
        }
        box_done = true;
    }
    bool same(const TurnTemplates &o, double frac) const { return memcmp(&tt, &o, sizeof tt) == 0 && clothoid_frac == frac; }
};
}  // namespace fcpp

struct fcpp_batch {
    fcpp_ctx *ctx = nullptr;
    fcpp_vehicle veh;
    fcpp_options opt;
    int64_t n_fields = 0;
    fcpp::HostPlan hp;               // info + field descriptors (the blocks' primitive lists are dropped once the image is built)
    fcpp::DevConst cst;
    void *slab = nullptr; size_t slab_bytes = 0;
    fcpp::ImageLayout lay;           // counts and offsets of the tables in the slab (fcpp_slab.h)
    fcpp::SlabTables t;              // ... and pointers to them: bind_tables(lay, slab)
    fcpp::DevTiling til0;            // staged pipeline (mode 0): plain near-equal tiles, built on its first run
    bool til0_built = false;
    std::shared_ptr<fcpp::TemplateSet> templates;
    // optional per-stage HIP-event timing (fcpp_batch_set_profiling)
    int profiling = 0;           // 0: off; k > 0: every k-th run carries the per-kernel events
    int64_t run_counter = 0;
    std::vector<hipEvent_t> events;   // kProfRuns x kStages x (start, stop)
    std::vector<unsigned char> ev_set; // kProfRuns x kStages: the stage launched a kernel in that run
    int prof_runs = 0;
    int last_mode = 0;
    fcpp_setup_times setup = {};
    const fcpp_field_info *info_dev = nullptr;     // device-side setup: the records in the slab; hp.info is filled from them on demand
    // every stream this batch's kernels were enqueued on (callers re-bind the context's stream between calls: engine.py binds torch's
    // current stream): fcpp_batch_destroy drains them all before the tables go back to the context as the next batch's allocation
    std::vector<hipStream_t> used_streams;
    void note_stream(hipStream_t s) { if (std::find(used_streams.begin(), used_streams.end(), s) == used_streams.end()) used_streams.push_back(s); }
    // the device-side setup returns with its last kernels still in the stream it was enqueued on: whoever reads the tables on ANOTHER stream
    // (a caller that re-binds the context's stream between create and run) waits for this event first
    // (the event is recorded on the setup's stream when such a stream first shows up -- everything enqueued there so far, the setup included,
    // lies before it -- not by the setup itself: see fcpp_ctx::ev_plan)
    hipStream_t setup_stream = nullptr;
    bool setup_pending = false;
    hipEvent_t ev_setup = nullptr;
    std::vector<hipStream_t> setup_seen;           // streams already ordered behind the setup
    hipError_t wait_setup(hipStream_t s)
    {
        if (!setup_pending || s == setup_stream || std::find(setup_seen.begin(), setup_seen.end(), s) != setup_seen.end()) return hipSuccess;
        if (!ev_setup) {
            if (!ctx->ev_pool.empty()) { ev_setup = ctx->ev_pool.back(); ctx->ev_pool.pop_back(); }
            else { const hipError_t e = hipEventCreateWithFlags(&ev_setup, hipEventDisableTiming); if (e != hipSuccess) return e; }
        }
        hipError_t e = hipEventRecord(ev_setup, setup_stream);
        if (e != hipSuccess) {          // (the setup's stream is gone: whatever ran there has been drained or is drained now)
            (void)hipGetLastError();
            e = hipDeviceSynchronize();
            if (e == hipSuccess) setup_pending = false;
            return e;
        }
        e = hipStreamWaitEvent(s, ev_setup, 0);
        if (e == hipSuccess) setup_seen.push_back(s);
        return e;
    }
    // fcpp_batch_plan ran this batch's step directly off the counting pass of its setup (fcpp_devplan.h: DevTileConsts.direct) and enqueued no
    // fill pass: the tables are filled when somebody asks for them (ensure_tables) or when another setup takes the plan slot whose scratch
    // they are filled from (plan_scratch) -- the unchanged fill pass with its publisher off, on the setup's stream
    bool tables_pending = false;
    int tables_slot = -1;
    fcpp::DevTileConsts tables_tc;
    fcpp::DevPlanScratch tables_scratch;
    ~fcpp_batch() { for (hipEvent_t e : events) (void)hipEventDestroy(e); if (ev_setup) (void)hipEventDestroy(ev_setup); }
};

namespace fcpp {

constexpr size_t kStageMax = (size_t)2 << 30;      // pinned setup memory a context keeps at most
constexpr size_t kSpareMax = (size_t)1 << 30;      // device allocation of a destroyed batch kept for the next one at most
inline double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// What fcpp_batch_plan hands down to the device setup: outputs are wanted.  A speculative setup without obstacle polygons then sizes the output
// arrays from the early point total, while the counting pass runs, and enqueues the step right behind that pass (DevTileConsts.direct).
struct PlanOutputs {
    fcpp_field_stats *stats = nullptr;      // the caller's records; null: the batch's own
    double *x = nullptr, *y = nullptr, *kappa = nullptr, *v = nullptr;
    uint32_t *fs = nullptr;
    int64_t points = 0;                     // what the arrays were sized for
    bool allocated = false;                 // the arrays are there
    bool stepped = false;                   // ... and the direct step has written them and the statistics: no fcpp_batch_run
};
extern thread_local double g_trace_totals_ms;     // (FCPP_TRACE_PLAN: when the last device setup saw its totals, ms since try_device_setup began)
constexpr int kNotOnDevice = 1;      // try_device_setup: this batch is the host's (reason in err)

// The reference and checker switches of a batch's setup, read from the environment once per batch_create (tests set them between batches) and
// handed down:
//   FCPP_SMALL_BATCH   fields below which `auto` takes the host: 0 sends every batch it can take to the device (tools/fuzz_parity.py)
//   FCPP_SETUP_EXACT   set: no speculative layout (the checker of it: tests/test_gpu_devplan.py)
//   FCPP_DIRECT        0: no direct step (the checker of tests/test_gpu_direct_step.py)
//   FCPP_CUT_ROWS      0: the direct setup's counting pass keeps a wavefront per field, never the row form (k_tile_rows_direct).  A checker
//                      like FCPP_DIRECT=0, not a tuning knob (tests/test_gpu_cut_rows.py)
//   FCPP_FIELD_WORK    0: every wave tile planned with k_plan_sparse, every field reduced with k_reduce_stats (the reference of
//                      k_plan_sparse_fields; the host tiler's path)
//   FCPP_DENSE_SPAN    0: round 4's per-line runs for fields without obstacles too (TileConsts::span_line_max)
//   FCPP_HOST_CHUNKS   1: the host path keeps the host's own chunk lists (the checker, tests/test_gpu_devplan.py)
struct SetupSwitches {
    int64_t small_batch = 16;
    bool exact_only = false, direct = true, cut_rows = true, field_work = true, device_chunks = true;
    int64_t span_line_max = INT64_MAX;
    static SetupSwitches read();
};

// fcpp_batch_create; po: fcpp_batch_plan wants outputs (PlanOutputs), else null
int batch_create(fcpp_ctx *c, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields, const fcpp_field *fields,
                 const fcpp_polys *obstacles, fcpp_batch **out, PlanOutputs *po);
// the tables of a batch whose step ran directly (fcpp_batch::tables_pending): every entry that reads b->t beyond own_stats calls this first
int ensure_tables(fcpp_batch *b);
int flush_tables(fcpp_batch *b, hipStream_t now, std::string &err);
// what fcpp_plan_count and fcpp_plan_points share with the setup: the records on the host, the planner's scratch, the records as the device reaches them
int host_fields(const fcpp_field *fields, int64_t n_fields, std::vector<fcpp_field> &copy, const fcpp_field *&host);
int plan_scratch(fcpp_ctx *c, int64_t n_fields, int max_prims, hipStream_t st, DevPlanScratch &s, std::string &err);
int device_fields(const fcpp_field *fields, int64_t n_fields, hipStream_t st, const DevPlanScratch &s, const fcpp_field *&dev, std::string &err);

}  // namespace fcpp
