// fcpp_devplan.h -- the setup of a batch ON THE DEVICE (fcpp_devplan.hip): what fcpp_host.cpp (one field's plan) and fcpp_tiler.cpp (its
// path cut into kernel work) do on the host's cores, done by the GPU -- the plan call of the reference, plan_complete_coverage
// (MLP:387-465), plans a NEW field every time, so the setup belongs on the clock and off the host.  Batches with obstacle_mode = FLAG: at the
// reference's own sampling (rounds 4-5) and at dense sampling when no field has obstacles (round 5).
//
//   k_plan_fields16    sixteen lanes per field, four fields per wavefront: fcpp_planfn.h's plan function restated lane-parallel, the same
//                      float64 operations in the same order -> fcpp_field_info, DevField, its primitives (k_plan_fields: the one-thread
//                      original, FCPP_PLAN_SERIAL=1 and fcpp_plan_points)
//   k_tile_fields<0>   one wavefront per field, the tiler's cut, counting its records.  Sparse sampling: span of whole passes + the general
//                      stretch cut in closed form (fcpp_cutfn.h) or by the window cut; dense sampling (the DENSE instance): span + a lane per
//                      quiet zone (last line, headland straights) + a lane per stretch between them (general tiles, or wave tiles by the
//                      window cut, a stretch after the other)
//   k_scan_*           exclusive scans over the fields of the per-field counts; the totals go to the host's pinned memory (polled)
//                      (not launched by the speculative setup of a small batch: there every kernel adds its counts into per-block aggregates
//                      and the next kernel takes a field's offsets from them -- fcpp_offsetfn.h, "two levels" below)
//   k_tile_fields<1>   the records written at their scanned positions: the tables of ImageLayout, equal byte for byte to what BatchTiler::fill
//                      writes on the host (tests/test_gpu_devplan.py)
// Only the 128-byte fcpp_field records go to the device and the totals (one small copy) and fcpp_field_info come back.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_device.h"
#include "fcpp_internal.h"
#include "fcpp_slab.h"
#include "fcpp_planfn.h"
#include "fcpp_tilefn.h"
#include "fcpp_cutfn.h"
#include "fcpp_offsetfn.h"

namespace fcpp {

// columns of the per-field count table (counts[col][field]) and of its exclusive scan (bases[col][field]); totals[col] = sum
enum PlanCol : int {
    PC_POINTS = 0, PC_PRIMS, PC_TILES, PC_WAVE, PC_GENERAL, PC_STAT, PC_SPAN, PC_WORK, PC_OPEN, PC_CLS0, PC_CLS1, PC_CLS2, PC_CLS3,
    PC_RUNS, PC_SPAN_PTS, PC_WAVE_PTS, PC_WORK_WAVE_PTS, PC_WAVE_INSIDE, PC_WORK_SPAN_PTS, PC_SPAN_F, PC_UNFUSABLE,
    PC_CHUNKS, PC_CHUNK_PTS,      // dense sampling: chunk records / points of the quiet runs of straights (the last swath line, headland straights)
    PC_COLS
};
// (PC_SPAN: span chunks when no span is fused; PC_SPAN_F: when every fusable span is; PC_UNFUSABLE: fields of field work whose span has too
// many chunks to be fused -- the host fuses all or none, k_tile_fields<true> is told which: DevTileConsts.fuse_spans)
// totals[PC_COLS + k]: flags the kernels raise -- a flag holds the generation number (DevTileConsts.gen, counted up by the context) of the
// last counting phase that raised it, so nothing has to be cleared between batches: raised in this phase <=> flag == gen
enum PlanFlag : int { PF_FALLBACK = 0, PF_BAD_OBSTACLES = 1, PF_OVER_CAPACITY = 2, PF_COUNT = 3 };
// behind the flags: [PX_ARRIVED] the columns of the counting phase's last scan that have published their totals (device only), [PX_DONE] the
// generation number of the phase whose totals are complete -- written to the host's copy by the last column to arrive: the host polls it
// (a word in its own pinned memory) instead of waiting for an event
static_assert(PC_COLS <= OFF_ROW, "a block's row of aggregates holds every column");
constexpr int PX_ARRIVED = PC_COLS + PF_COUNT, PX_DONE = PC_COLS + PF_COUNT + 1;
// behind PX_DONE, the host's copy only: a direct setup's counting launch (DevTileConsts.direct) writes the batch's point total -- the planner's
// aggregates, complete before the pass begins -- and then its generation number: the host sizes the output arrays while the pass runs
constexpr int PX_EARLY_POINTS = PC_COLS + PF_COUNT + 2, PX_EARLY_GEN = PC_COLS + PF_COUNT + 3, PLAN_TOTALS = PC_COLS + PF_COUNT + 4;
// (PF_OVER_CAPACITY: a speculative setup -- tables laid out by per-field capacities, the fill pass enqueued before the host has the totals
// -- met a field beyond them: SPEC_* below; the host then lays the tables out from the totals and fills them again)
constexpr int SPEC_SPAN_CHUNKS = 16;         // span chunks per field a speculative layout has room for (tiles: 1 + DEVPLAN_KEEP_TILES, wave / general tiles: DEVPLAN_KEEP_TILES)

// what the device tiler needs to know about the batch (TileConsts of fcpp_tiler.h with the templates on the device)
struct DevTileConsts {
    const Pt2 *tu, *tc;           // the batch's U-turn / corner templates (device)
    int32_t nu, nc;
    int32_t turn_quiet, wave_factor, field_work_tiles, max_prims, fuse_spans;
    int32_t no_bases;             // counting pass of a small batch: the fields' point offsets are not known yet (ONE scan, after the pass)
    int32_t speculative;          // the tables are laid out by capacities: the counting pass watches them, the fill pass decides the fusing of
                                  // spans itself and does nothing when a flag of this generation is up.  No scan is launched: both passes take
                                  // their offsets from the two levels of fcpp_offsetfn.h (DevPlanScratch.agg), the fill pass publishes the totals
    int32_t closed_cut;           // the general stretches of fields with a closed-form span are cut in closed form (fcpp_cutfn.h); 0: by the window cut of round 4
    int32_t dense;                // sample_spacing > 0: span of all complete passes + quiet runs of the straights + general tiles between them (k_tile_fields, "dense")
    int32_t direct;               // speculative setups of fcpp_batch_plan.  DIRECT_COUNT, counting pass: every field of field work with a fusable span gets
                                  // its pack and its run totals in the scratch (DevPlanScratch.direct_packs / direct_totals), the step is launched
                                  // from them (launch_plan_sparse_direct) and publishes the totals; one workgroup more writes PX_EARLY_POINTS.
                                  // DIRECT_FILL, fill pass: the totals were published by that step -- no publisher workgroup
    int64_t span_line_max;        // TileConsts.span_line_max
    double two_a, u_cap, c_line, fence_margin;
    int64_t reduce_wg_max;
    int64_t gen;                  // this counting phase's generation number (> 0)
    CutConsts cut;                // the closed-form cut (fcpp_cutfn.h), templates and chord tables on the device
};

enum : int32_t { DIRECT_COUNT = 1, DIRECT_FILL = 2 };

// the device planner's scratch: one allocation the context keeps (grow-only); all pointers device
struct DevPlanScratch {
    fcpp_field *fields_in;        // n (copied from the host, unless the device reads the caller's pinned records where they lie)
    fcpp_field_info *info;        // n (copied back)
    DevField *fields_tmp;         // n: pt_off / prim_first still relative to the field
    DevPrim *prims_tmp;           // n x max_prims
    int64_t *counts, *bases;      // PC_COLS x n
    int64_t *blk_sums;            // PC_COLS x blocks of 1024 fields
    int64_t *totals;              // PLAN_TOTALS
    // two levels (fcpp_offsetfn.h), speculative setups: agg[col][block of OFF_B fields] = the block's sum of the column, added up with atomics by
    // the planner (PC_POINTS) and the counting pass (every other column), read by the NEXT kernel only.  Two buffers per plan slot, zero when
    // the slot is allocated: a setup accumulates into `agg`, its fill pass zeroes `agg_next`, the next setup of the slot swaps them -- no
    // clearing command in the stream (fcpp_setuprule.h: SlotAggregates, which also says what happens after a setup that ended in between)
    int64_t *agg, *agg_next;      // OFF_WORDS each: OFF_NB rows of OFF_ROW words, PC_COLS of them used
    // the counting pass keeps the first DEVPLAN_KEEP_TILES wave tiles of every field (records with field-relative indices): the fill pass
    // copies and rebases them instead of cutting the field again (fields with more are cut again)
    DevTile *keep_tiles;          // n x DEVPLAN_KEEP_ROWS
    DevWaveTile *keep_wtiles;     // n x DEVPLAN_KEEP_WROWS
    // direct setups (DevTileConsts.direct), indexed by field: the pack of a field of field work with a fusable span as the fill pass would lay it
    // out (positions the step never reads stay relative to the field; work.n_tiles = -1: not such a field) and its work_totals record
    DevFieldPack *direct_packs;   // n (batches of at most OFF_FIELDS_MAX fields)
    TilePartial *direct_totals;   // n
    double2 *direct_junc;         // n: the field's junction after a U-turn (the step's DevConst.field_junc: the batch's own table is the fill pass's)
};
int64_t devplan_small_blocks();
// the scratch for n fields laid out at `base` (null: sizing only); returns its size in bytes
size_t devplan_scratch_layout(int64_t n, int max_prims, void *base, DevPlanScratch &s);

// the device tiler's LDS window over a field's general stretch (it slides), and the most primitives a field may have (8-bit indices in
// that window); a batch whose vehicle needs more (31+ headland loops) is set up on the host
constexpr int DEVPLAN_WINDOW = 576;
constexpr int DEVPLAN_PRIMS_CAP = 255;
constexpr int DEVPLAN_KEEP_TILES = 8;
constexpr int DEVPLAN_KEEP_ROWS = CUT_TILES_MAX;      // rows per field of the kept-tile arrays: every tile of a closed-form cut is kept (the fill pass never cuts such a field again)
static_assert(DEVPLAN_KEEP_ROWS >= DEVPLAN_KEEP_TILES, "the window cut keeps its first DEVPLAN_KEEP_TILES tiles in the same rows");
// rows per field of the kept WAVE-tile array: one more, whose 64 bytes hold a dense field's wave tiles per stretch (byte j: stretch j; 255: the
// stretch is the general kernel's) -- the counting pass's verdicts, read by the fill pass
constexpr int DEVPLAN_KEEP_WROWS = DEVPLAN_KEEP_ROWS + 1;
static_assert(sizeof(DevWaveTile) == 64, "a row of the kept wave tiles holds the 64 stretches' bytes");

// Small batches (at most 8192 fields) are counted WITHOUT the fields' point offsets: what depends on a span's alignment in the batch arrays
// -- its chunk count, hence whether its field's workgroup can write it (PC_SPAN, PC_SPAN_F, PC_WORK_SPAN_PTS, PC_UNFUSABLE) -- is derived by the
// one scan that follows the pass, from the offsets it has just computed (span_counts): one launch and one scan fewer in front of the pass.
// phase 1: plan + count.  Enqueues k_plan_fields, the scans and the counting pass; afterwards totals[] holds the sums and the flags, and so
// does totals_host (pinned host memory the device can write, or null) once the stream has got there: the scans write it themselves.
// tc.speculative (at most OFF_FIELDS_MAX fields, reference sampling): planner and counting pass only -- the pass has the point offsets from
// the planner's aggregates, writes every column and adds it to the aggregates; the totals are published by the speculative fill pass.
// fields: the records as the device reaches them (s.fields_in after a copy, or the caller's pinned memory).
// tc.direct (speculative, no obstacle polygons): cst = the batch's kernel constants (the span's closed-form statistics), see DevTileConsts.direct
int launch_devplan_count(hipStream_t st, int64_t n, const PlanConsts &pc, const DevTileConsts &tc, const DevPlanScratch &s, const fcpp_field *fields,
                         int64_t n_polys, int check_obstacles, int64_t *totals_host, const DevConst *cst = nullptr, bool cut_rows = true);
// The counting pass of a direct setup has two forms with the same outputs: a wavefront per field (k_tile_fields_direct) and, from
// ROWS_MIN_FIELDS fields on, a row of 32 lanes per field, two fields per wavefront (k_tile_rows_direct).  The threshold is the smallest device batch: measured at 64, 256, 1024,
// 2048 and 4096 fields the row form was nowhere slower than the wave form (DESIGN section 3 has the figures); it stays a named constant
// because that is a measurement, not a property.  true: launch_devplan_count takes the row form for this setup.
constexpr int64_t ROWS_MIN_FIELDS = 16;
// cut_rows: false keeps the wave form (FCPP_CUT_ROWS=0, the checker: SetupSwitches)
bool devplan_count_in_rows(const DevTileConsts &tc, int64_t n, bool cut_rows);
// (tc.dense: the counting pass needs the fields' point offsets -- the chunks of every quiet run lie on 512-point boundaries of the batch arrays --:
// planner, scan of the points, pass, scan of the other columns)
// sizing only (fcpp_plan_points): k_plan_fields without primitives; counts[PC_POINTS][field] = points of the field
int launch_devplan_points(hipStream_t st, int64_t n, const PlanConsts &pc, const DevPlanScratch &s, const fcpp_field *fields);
// phase 2: the tables (pointers into the batch's slab, laid out by the host).  `bases` / `totals` as phase 1 left them.
// tc.speculative: positions from the two levels; one more workgroup publishes the totals, the flags and tc.gen to totals_host (the host
// polls it: DeviceSetup::await, fcpp_setup.cpp) and zeroes s.agg_next -- also when the flags make the pass a no-op.
int launch_devplan_fill(hipStream_t st, int64_t n, const DevTileConsts &tc, const DevConst &cst, const DevPlanScratch &s, const SlabTables &t, int64_t *totals_host);
// the exact layout after a speculative counting phase (over capacity): the scan of all columns as the pass wrote them -> bases, totals
int launch_devplan_rescan(hipStream_t st, int64_t n, const DevPlanScratch &s);
// fcpp_math.h on the device (tests): fn 0 sincos, 1 atan2(a, b), 2 acos(a), 3 hypot(a, b)
int launch_debug_math(hipStream_t st, int fn, int64_t n, const double *a, const double *b, double *out0, double *out1);
// the step of a direct setup (fcpp_sparse.hip): one workgroup per FIELD from s.direct_packs / s.direct_totals, enqueued right behind the counting
// pass; every workgroup applies the batch rule to the aggregates' totals itself (no flag of generation `gen` up, every field a field of field
// work, every span fusable) and returns when it fails; one workgroup more publishes the totals as the fill pass's publisher does
int launch_plan_sparse_direct(hipStream_t st, int64_t n, int64_t gen, const DevPlanScratch &s, const DevConst &cst, double *x, double *y, double *kappa,
                              double *v, uint32_t *fs, fcpp_field_stats *stats, int64_t *totals_host);

#if defined(__HIPCC__)
// a column's total to the host's copy; the flags (generation numbers, see PlanFlag) with the first column of the last scan
__device__ __forceinline__ void publish_total(const int64_t *totals, int64_t *mirror, int col, int64_t value, bool flags)
{
    if (!mirror) return;
    mirror[col] = value;
    if (flags) for (int k = 0; k < PF_COUNT; ++k) mirror[PC_COLS + k] = totals[PC_COLS + k];
}

// The publisher of a speculative setup -- the first workgroup of its fill pass, or of its direct step: what the last scan of a counting phase
// does for the host, without a scan.
// Wavefront 0 sums every column's aggregates (total(col), fcpp_offsetfn.h) and writes the totals, the flags and then the phase's generation
// number to the host's copy (DeviceSetup::await polls that word) -- whatever the flags say: a pass they make a no-op is waited for as well.
// Wavefront 1 zeroes the OTHER buffer of aggregates, the one the slot's next setup accumulates into (nothing of this setup reads or writes it).
__device__ __forceinline__ void publish_two_level(int64_t n, int64_t gen, int64_t *__restrict__ totals, const int64_t *__restrict__ agg, int64_t *__restrict__ agg_next,
                                                  int64_t *__restrict__ mirror, int wave, int lane)
{
    if (wave == 1) {
        for (int k = lane; k < OFF_WORDS; k += 64) agg_next[k] = 0;
        return;
    }
    if (wave != 0) return;
    int64_t flag[PF_COUNT];
#pragma unroll
    for (int k = 0; k < PF_COUNT; ++k) flag[k] = totals[PC_COLS + k];
    int64_t p0, p1, t0, t1;
    offset_row_sums(agg, 0, (int)offset_blocks(n), lane, p0, p1, t0, t1);
    // lane c: total(c) -- lane l holds the totals of columns 2 (l & 15) and 2 (l & 15) + 1; lanes PC_COLS + k: flag k
    const int64_t other = __shfl(t1, lane >> 1), even = __shfl(t0, lane >> 1);
    int64_t mine = (lane & 1) ? other : even;
#pragma unroll
    for (int k = 0; k < PF_COUNT; ++k) if (lane == PC_COLS + k) mine = flag[k];
    if (lane < PC_COLS) { totals[lane] = mine; publish_total(totals, mirror, lane, mine, false); }
    if (!mirror) return;
    if (lane >= PC_COLS && lane < PC_COLS + PF_COUNT) mirror[lane] = mine;      // (the flags as loaded above, a lane each)
    __threadfence_system();
    if (lane == 0) reinterpret_cast<volatile int64_t *>(mirror)[PX_DONE] = gen;
}
#endif

}  // namespace fcpp
