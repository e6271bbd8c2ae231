// fcpp_api_internal.h -- what the host translation units behind include/fcpp.h share: fcpp_api.cpp (context, output arena, a batch's step), fcpp_setup.cpp
// (batch setup), fcpp_paths.cpp and fcpp_glue_*.cpp (the standalone path operators, one glue file per family).  Private to csrc/.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "fcpp_device.h"
#include "fcpp_internal.h"
#include "fcpp_setuprule.h"
#include "fcpp_tiler.h"

namespace fcpp {

// sets the calling thread's message (fcpp_last_error) and returns the code; the message itself lives in fcpp_api.cpp
int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(FCPP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)
#define LAUNCHCHK(expr) HIPCHK((hipError_t)(expr))      // the kernels' launchers return 0 or a hipError_t value

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count)
    {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc((void **)&p, count * sizeof(T));
    }
    hipError_t upload(const std::vector<T> &h, hipStream_t st)
    {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    }
};

DevConst make_const(const fcpp_vehicle &veh, const fcpp_options &opt);

// plain tile table of a set of paths (the staged pipeline and the standalone operators): tiles never straddle paths, hold at most
// TILE_POINTS points, a path is cut into near-equal tiles.  (The fused pipeline's tiler lives in fcpp_tiler.cpp.)
struct Tiling {
    std::vector<DevPath> paths;
    std::vector<DevTile> tiles;
    std::vector<int64_t> tile_first;
    void build(int64_t n_paths, const int64_t *offsets)
    {
        paths.resize((size_t)n_paths);
        tile_first.assign((size_t)n_paths + 1, 0);
        tiles.clear();
        for (int64_t p = 0; p < n_paths; ++p) {
            const int64_t n = offsets[p + 1] - offsets[p];
            paths[(size_t)p] = { offsets[p], n };
            tile_first[(size_t)p] = (int64_t)tiles.size();
            if (n <= 0) continue;
            const int64_t k = (n + TILE_POINTS - 1) / TILE_POINTS;
            const TilerSplit<int64_t> sp(n, k);
            for (int64_t i = 0; i < k; ++i) {
                DevTile t;
                t.field = (int32_t)p; t.start = sp.start(i); t.count = (int32_t)sp.count(i); t.quiet = 0; t.stat_tile = 0; t.idx0 = 0; t.off0 = 0;
                tiles.push_back(t);
            }
        }
        tile_first[(size_t)n_paths] = (int64_t)tiles.size();
    }
};

struct DevTiling {
    DevBuf<DevPath> paths;
    DevBuf<DevTile> tiles;
    DevBuf<int64_t> tile_first;
    DevBuf<char> agg_f, agg_b;   // Agg = 2 doubles
    DevBuf<double> carry_f, carry_b;
    DevBuf<char> spine;          // scratch of the three-level spine (large batches)
    DevBuf<TilePartial> partial;
    DevBuf<unsigned long long> n_adj;
    int64_t n_tiles = 0, n_paths = 0;
    hipError_t upload(const Tiling &t, hipStream_t st)
    {
        n_tiles = (int64_t)t.tiles.size(); n_paths = (int64_t)t.paths.size();
        hipError_t e;
        if ((e = paths.upload(t.paths, st)) != hipSuccess) return e;
        if ((e = tiles.upload(t.tiles, st)) != hipSuccess) return e;
        if ((e = tile_first.upload(t.tile_first, st)) != hipSuccess) return e;
        if ((e = agg_f.alloc((size_t)n_tiles * 16)) != hipSuccess) return e;
        if ((e = agg_b.alloc((size_t)n_tiles * 16)) != hipSuccess) return e;
        if ((e = carry_f.alloc((size_t)n_tiles)) != hipSuccess) return e;
        if ((e = carry_b.alloc((size_t)n_tiles)) != hipSuccess) return e;
        if ((e = spine.alloc((size_t)spine_scratch_bytes(n_tiles))) != hipSuccess) return e;
        if ((e = partial.alloc((size_t)n_tiles)) != hipSuccess) return e;
        if ((e = n_adj.alloc((size_t)n_paths)) != hipSuccess) return e;
        return hipStreamSynchronize(st);   // the staging vectors die here
    }
};

struct TemplateSet;     // a batch's turn templates (fcpp_batch.h)
struct PathTiling;      // the standalone operators' last path set (fcpp_paths.cpp)
void free_paths_cache(fcpp_ctx *c);

// fcpp_trajectory on a checked context and device (fcpp_paths.cpp); fcpp_batch_trajectory calls it with the batch's two paths per field
int trajectory_paths(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, const int64_t *offsets_host, int64_t total, const double *x,
                     const double *y, const double *v, const uint32_t *fs, double *s, double *t, double *heading, double *totals);

// the tile table of a path set on a checked context (fcpp_paths.cpp: path_set, the context's cache), for the path operators of other glue files
int path_tiling(fcpp_ctx *c, int64_t n_paths, const int64_t *offsets, const int64_t *offsets_host, int64_t total, DevTiling **out);

}  // namespace fcpp

struct fcpp_ctx {
    int device = 0;
    fcpp::PathTiling *paths_cache = nullptr;     // tile table of the standalone operators' last path set (path_set)
    hipStream_t own = nullptr, stream = nullptr;
    // side stream of the fused pipeline: the ALU-bound kernels (wave tiles, general tiles) run beside the HBM-bound streaming
    // kernels of the same step; ev_fork / ev_join order the two streams inside a step
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // batch setup (fcpp_batch_create): the image of a batch's tables is built in pinned host memory that the context keeps (grow-only,
    // up to kStageMax; larger images go through a pageable buffer), and the last destroyed batch's device allocation is kept for the
    // next one (up to kSpareMax): a caller that plans batch after batch allocates nothing after the first
    void *stage = nullptr; size_t stage_cap = 0;
    // the stream of the last asynchronous copy out of `stage`: whoever writes that memory next drains it first (a caller that plans batch
    // after batch has drained it long before: a query; no event -- a record between two kernels holds the second back by 5 us)
    hipStream_t stage_stream = nullptr; bool stage_busy = false;
    hipError_t stage_wait()
    {
        if (!stage_busy) return hipSuccess;
        stage_busy = false;
        hipError_t e = hipStreamSynchronize(stage_stream);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipDeviceSynchronize(); }      // (that stream is gone)
        return e;
    }
    void *spare = nullptr; size_t spare_cap = 0;
    std::shared_ptr<fcpp::TemplateSet> templates;   // the last batch's turn templates
    fcpp_setup_times last_setup = {};
    // device-side setup (fcpp_devplan.h): FCPP_SETUP_AUTO / _HOST / _DEVICE; its scratch (grow-only) and a small pinned block for the
    // totals that come back in the middle of it
    int setup_mode = FCPP_SETUP_AUTO;
    // (up to FOUR scratch allocations, one per stream that sets batches up: a caller that plans batch k + 1 on a second stream while batch k's step
    // still runs on the first -- the sustained rate of bench.py -- must not wait for that step because its fill pass shared the scratch)
    // (SlotAggregates, fcpp_setuprule.h: which of the slot's two buffers of aggregates the next speculative setup accumulates into --
    // DevPlanScratch.agg -- and whether both are to be cleared first: begin_aggregates() / aggregates_settled())
    // (tables_batch: the batch whose step ran directly off the slot's counting pass and whose tables are still to be filled from the slot's scratch
    // -- fcpp_batch::tables_pending; whoever takes the slot next enqueues that fill pass first: plan_scratch)
    struct PlanSlot : fcpp::SlotAggregates { void *p = nullptr; size_t cap = 0; hipStream_t stream = nullptr; bool pending = false; uint64_t tick = 0;
                                             fcpp_batch *tables_batch = nullptr; };
    static constexpr int kPlanSlots = 4;
    PlanSlot plan_slots[kPlanSlots];
    uint64_t plan_tick = 0;
    int plan_cur = 0;                               // the slot of the setup in progress / of the last one
    void *verify_scratch = nullptr;                 // sliced reduction of the standalone operators' long paths (reduce_paths)
    size_t verify_scratch_cap = 0;
    int64_t *plan_totals_host = nullptr;            // pinned, PC_COLS + PF_COUNT values: the scans of the counting phase write them here
    unsigned long long *ga_mirror = nullptr;        // pinned, one word: (converged << 32) | generations of the running fcpp_ga_evolve (GaState::mirror)
    int n_cu = 0;                                   // compute units of `device`, read at creation (0: the query failed); ga_launch_plan spreads the GA's pairs over them
    int64_t plan_gen = 0;                           // generation number of the last counting phase (PlanFlag, fcpp_devplan.h)
    // fcpp_batch_plan's direct step (fcpp_devplan.h: DevTileConsts.direct) is attempted while the last speculative setup's batch qualified for it
    // (or there was none): a caller of batches that do not -- mixed classes, unfusable spans -- pays the empty launch once, not per call
    bool direct_ok = true;
    int64_t cut_rows_passes = 0;         // direct setups whose counting pass took the row form (fcpp_ctx_cut_rows_passes: tests)
    int64_t direct_steps = 0, direct_taken = 0, direct_fills = 0;      // launched / batches taken / their fill passes enqueued later (fcpp_ctx_direct_steps: tests)
    // fcpp_conn_solve_clear: the pairs its first pass listed in the last call, and the second-pass launches so far (fcpp_ctx_solve_clear_passes: tests)
    int64_t solve_clear_listed = 0, solve_clear_word_launches = 0;
    // fcpp_field_path_counts_clear / _fill_clear: the same two figures of the clear field paths (fcpp_ctx_field_path_clear_passes: tests)
    int64_t fpath_clear_listed = 0, fpath_clear_word_launches = 0;
    // fcpp_route_transit_priced: the same two figures of the priced transit block (fcpp_ctx_route_priced_passes: tests)
    int64_t route_priced_listed = 0, route_priced_word_launches = 0;
    // fcpp_loop_transit_solve: the same two figures of the loop transits' stations pass (fcpp_ctx_loop_transit_passes: tests)
    int64_t transit_listed = 0, transit_word_launches = 0;
    // the stream the last device-side setup was enqueued on (its fill pass may still read the scratch): a setup on ANOTHER stream records
    // ev_plan there and waits for it -- lazily, when that other stream shows up: an event recorded between two kernels of the plan call
    // costs 5 us of device time between them (round 5: the three records of a plan call were 16 of its 158 us)
    hipEvent_t ev_plan = nullptr;
    // the output arena (fcpp_ctx_reserve_outputs): ONE allocation of 4 x pitch + lane bytes; array k of every batch's outputs lies in lane k
    // (lanes `pitch` apart), placed first-fit among the live allocations of the lane -- all five arrays of an allocation at the same offset
    void *arena = nullptr; size_t arena_pitch = 0, arena_lane = 0;
    struct ArenaBlock { size_t off, len; hipStream_t last = nullptr; bool used = false; };      // last: the stream of the last fcpp_batch_run that wrote the block
    std::vector<ArenaBlock> arena_live;             // sorted by off
    std::vector<hipEvent_t> ev_pool;                // setup events of destroyed batches (fcpp_batch::ev_setup), reused: no event is created per plan call
};
