/*
 * fcpp.h -- C ABI of libfcpp.so, the MI355X (gfx950) coverage-path geometry engine.
 *
 * The reference (qwagrox/field-coverage-path-planning @ 2025-10-24) is pure Python and has no
 * FFI: its boundary is the class surface of multi_layer_planner_v3.py ("MLP") and
 * genetic_algorithm_solver.py ("GA").  Each entry point below names the reference
 * method(s) it replaces; the Python mirror of that surface
 * (field_coverage_path_planning_amd/multi_layer_planner_v3.py) binds them through ctypes, and
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every function returns FCPP_OK (0) or a negative FCPP_E* code and
 *     records a message retrievable with fcpp_last_error() (thread-local).
 *   - pointers named *_dev are DEVICE pointers (hipMalloc / torch CUDA tensors); all others
 *     are host pointers.  Path arrays are SoA float64: x[], y[], kappa[], v[] (km/h) plus
 *     one uint32 flag/segment word per point.
 *   - work is enqueued on the context's HIP stream (fcpp_ctx_set_stream); calls that return
 *     host data synchronise that stream themselves, the others are asynchronous.
 *   - a context is not thread-safe; distinct contexts are independent.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry fails with
 *     FCPP_EHIP.
 */
#ifndef FCPP_H
#define FCPP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCPP_ABI_VERSION 5

enum {
    FCPP_OK = 0,
    FCPP_EINVAL = -1,       /* the reference's ValueError: no field given / headland wider than field (MLP:135,597-598) */
    FCPP_EHEADLAND = -2,    /* a headland loop's inset polygon is empty (MLP:967-969 followed by the vstack at :939) */
    FCPP_EUNSUPPORTED = -3, /* not a convex quadrilateral, or a decision only GEOS could take: the corner-gap test `gap.area > 0.1` (MLP:1070) where
                               0.1 m^2 lies between the areas for the exact and for GEOS' polygonal buffer -- a band of ~0.04 m of working width */
    FCPP_EHIP = -4,         /* HIP runtime failure / no device */
    FCPP_ENOMEM = -5,
    FCPP_ESIZE = -6         /* negative / inconsistent sizes */
};

/* ---- VehicleParams (MLP:29-39), same field order and defaults ------------------------ */
typedef struct fcpp_vehicle {
    double working_width;          /* 3.2  */
    double min_turn_radius;        /* 8.0  */
    double max_work_speed_kmh;     /* 9.0  */
    double max_headland_speed_kmh; /* 15.0 */
    double headland_turn_speed_kmh;/* 4.0  */
    double max_lateral_accel;      /* 2.0  */
    double max_longitudinal_accel; /* 1.5  */
    double safety_factor;          /* 0.85 */
} fcpp_vehicle;

/* ---- sampling / validation options (build-defined; all-zero + geofence_tol = reference) -- */
enum { FCPP_TURN_ARC = 0, FCPP_TURN_CLOTHOID = 1 };
typedef struct fcpp_options {
    int32_t turn_model;     /* FCPP_TURN_ARC: circular arcs as MLP:807-825,1046-1062; _CLOTHOID: line->clothoid->arc->clothoid->line */
    int32_t clothoid_fit;   /* 0: kappa_max = 1/R ; 1: scale so the turn ends where the reference arc ends */
    double sample_spacing;  /* 0: the reference's fixed counts (2/20/15/20, reverse 0.5 m); >0: uniform arc-length spacing [m] */
    double clothoid_frac;   /* share of a turn's heading change spent in its two clothoids, in [0,1] */
    double geofence_tol;    /* a point further than this outside the field polygon is flagged [m] */
    int32_t obstacle_mode;  /* FCPP_OBSTACLES_FLAG: obstacles only set the validity flag of the points inside them (the reference: its
                               swath generator ignores the differenced work area, MLP:731-732); FCPP_OBSTACLES_AVOID: the swaths
                               of layer 1 are clipped against the obstacles and re-routed around them (below) */
    int32_t ring_order;     /* the order in which Shapely's `buffer(-offset).exterior.coords[:-1]` lists the four inset corners of a headland
                               loop (MLP:964-972) -- a GEOS fact the reference neither documents nor tests, and its corner formulas index
                               the list (MLP:1049-1060): FCPP_RING_AS_VERTICES = in the order of the field vertices (the documented
                               intent 0=LL, 1=LR, 2=UR, 3=UL of MLP:957; reproduces every number the reference publishes);
                               FCPP_RING_REVERSED = the other way round from the same first vertex (0, 3, 2, 1: LL, UL, UR, LR -- what a
                               clockwise shell starting at the first vertex lists).  INTEGRATION.md shows how a user with Shapely
                               checks which one their GEOS produces.  Host-side permutation only. */
} fcpp_options;
enum { FCPP_RING_AS_VERTICES = 0, FCPP_RING_REVERSED = 1 };

/* Obstacle-aware swaths (what README_en.md:156-178 promises and MLP:601-609 prepares: obstacles expanded by
 * working_width / 2 and taken out of the work area).  Build-defined -- the reference has no code for it.  In the frame of layer 1
 * (MLP:686-687) every obstacle is represented by the bounding box of its vertices grown by W/2 on every side; grown boxes that overlap
 * or touch are merged into their common bounding box until no two do, so the boxes are disjoint.  A swath line whose y lies strictly
 * inside a box is CLIPPED there and led around the obstacle (segment kind FCPP_KIND_DETOUR, nominal speed headland_turn_speed_kmh; legs
 * sampled like the reverse fills at the reference's sampling: 0.5 m, at least 2 points per leg):
 *   - an obstacle whose box was not merged: along its W/2-grown POLYGON (round 4) -- the convex hull of its vertices, every edge moved
 *     W/2 outwards, neighbours joined at their mitre point (a corner sharper than 60 degrees: a square cap W/2 beyond it), clipped to the
 *     grown box; it contains every point within W/2 of the hull.
 *     The swath is worked up to where its line meets the polygon, the way around is the shorter of the polygon's upper and lower chain
 *     between the two meeting points that stays inside the y-range of the main work area (never longer than the box's three legs), and a
 *     line that passes clear of the polygon is not interrupted;
 *   - merged boxes: three straight legs along the box -- up or down its near side, along its top or bottom (the closer one unless it lies
 *     outside the y-range of the main work area), back along its far side.
 * The legs stay inside their own box and the boxes are disjoint: no leg enters another obstacle.  A box (or polygon) with room on neither
 * side is refused.  Sub-swaths and legs are numpy.linspace runs between their end points in field coordinates.
 * End zones (round 4): the turn after a pass starts where its line ends and occupies a zone beyond that end -- the reference's half
 * circle about (max_x, y): 2 R along the line and R above it; the clothoid turn: the extents of its shape.  A box that meets that zone,
 * or either of the two lines within it, moves the turn inwards until the zone is free (again if the moved zone meets another box): both
 * passes end / start there, the U-turn is the same shape translated, and the strip beyond stays unworked.  Only the free ends -- the
 * start of the first pass, the end of the last -- are not moved: a box there, or one that leaves no side to pass, refuses the field
 * with FCPP_EUNSUPPORTED (its status; the other fields of the batch are planned).
 * Headland (round 4): a headland straight that crosses a grown box is cut at the box and led around it along the box's boundary -- from
 * where it enters to where it leaves, the shorter way whose box corners stay at least W/2 inside the field -- as FCPP_KIND_DETOUR legs
 * carrying the loop's FCPP_FLAG_HEADLAND; the pieces of the straight keep its sample density (length / 19 per step at the reference's
 * sampling).  A box over an end of a straight or within 2 R of a loop corner (where the corner turns are), across a reverse fill, or
 * with no way around inside the field refuses the field. */
enum { FCPP_OBSTACLES_FLAG = 0, FCPP_OBSTACLES_AVOID = 1 };

/* ---- one field = one planner instance (ctor arguments, MLP:63-72) ---------------------- */
typedef struct fcpp_field {
    double vx[4], vy[4];        /* field_vertices; for field_length/field_width: (0,0),(L,0),(L,H),(0,H) (MLP:127-132) */
    int32_t from_vertices;      /* 1 = field_vertices=..., 0 = field_length/field_width */
    int32_t has_start, has_end; /* start_point / end_point given */
    double start_x, start_y, end_x, end_y;
    int32_t n_obstacles;        /* obstacles=[...] : polygons obstacle_first .. +n_obstacles of the batch polygon table */
    int32_t _pad;
    int64_t obstacle_first;
} fcpp_field;

/* obstacle polygons of a whole batch, CSR layout, host pointers */
typedef struct fcpp_polys {
    int64_t n_polys;
    const int64_t *offsets;     /* n_polys + 1 */
    const double *x, *y;        /* offsets[n_polys] vertices */
} fcpp_polys;

/* ---- what the host-side setup decides per field (integers: bit-exact parity) ------------ */
typedef struct fcpp_field_info {
    int64_t point_offset;       /* first point of this field in the batch arrays */
    int64_t n_main, n_head;     /* len(main_work['path']), len(headland['path']) */
    int32_t n_swaths;           /* num_passes, MLP:739 */
    int32_t n_loops;            /* ceil(R / W), MLP:916 */
    int32_t start_corner;       /* MLP:360-385 */
    int32_t reverse_order, start_from_right; /* MLP:631-668 */
    int32_t rotated;            /* |rotation_angle| > 0.01, MLP:686 */
    int32_t start_kept, end_kept; /* after _validate_point, MLP:322-343 */
    int32_t shape;              /* 0 rectangle, 1 parallelogram, 2 other (MLP:137-163) */
    int32_t n_reverse[4];       /* reverse-fill points appended at corner c of the outer loop */
    int32_t status;             /* FCPP_OK or the error this field raises (its n_main = n_head = 0) */
    double corner_angles[4];    /* degrees, MLP:165-192 */
    double field_length, field_width, headland_width, rotation_angle;
    double approach_from[2], approach_to[2];    /* MLP:437-441 (valid if start_kept) */
    double departure_from[2], departure_to[2];  /* MLP:443-447 (valid if end_kept) */
} fcpp_field_info;

/* ---- per-field results reduced on the device ---------------------------------------- */
typedef struct fcpp_field_stats {
    double main_len_m, main_time_pre_s, main_time_s;   /* MLP:616-628 and :423-426 */
    double head_len_m, head_time_pre_s, head_time_s;   /* MLP:882-895 and :428-431 */
    double max_kappa, max_alat, max_jump;              /* verify_curvature_constraints over main||headland, MLP:1396-1408 */
    int64_t n_viol;          /* a_lat > max_lateral_accel, MLP:1401 */
    int64_t n_outside;       /* geofence: points outside the field polygon */
    int64_t n_in_obstacle;   /* points inside an obstacle polygon */
    int64_t n_adjusted;      /* points slowed by the curvature clamp, MLP:502-504 */
} fcpp_field_stats;

/* ---- flag / segment word -------------------------------------------------------------- */
enum {
    FCPP_KIND_SWATH = 0, FCPP_KIND_UTURN = 1, FCPP_KIND_HEAD_START = 2, FCPP_KIND_HEAD_STRAIGHT = 3,
    FCPP_KIND_CORNER = 4, FCPP_KIND_REVERSE = 5, FCPP_KIND_DETOUR = 6
};
#define FCPP_KIND_MASK 7u
#define FCPP_FLAG_HEADLAND 8u     /* layer 2 */
#define FCPP_FLAG_ALAT 16u        /* lateral acceleration above max_lateral_accel at this point */
#define FCPP_FLAG_OUTSIDE 32u     /* outside the field polygon (geofence) */
#define FCPP_FLAG_OBSTACLE 64u    /* inside an obstacle polygon */
#define FCPP_INDEX_SHIFT 8        /* bits 8..31: swath index i (layer 1) or loop*8 + corner/side (layer 2) */

typedef struct fcpp_ctx fcpp_ctx;
typedef struct fcpp_batch fcpp_batch;

/* ---- library / context ---------------------------------------------------------------- */
const char *fcpp_last_error(void);
int fcpp_abi_version(void);
void fcpp_vehicle_default(fcpp_vehicle *v);   /* VehicleParams() defaults, MLP:31-38 */
void fcpp_options_default(fcpp_options *o);   /* reference behaviour, geofence_tol = 1e-6 */
int fcpp_ctx_create(int device_id, fcpp_ctx **ctx);
int fcpp_ctx_destroy(fcpp_ctx *ctx);
int fcpp_ctx_set_stream(fcpp_ctx *ctx, void *hip_stream); /* a hipStream_t; NULL = HIP's default stream.  A new context starts on a private non-blocking stream */
int fcpp_ctx_synchronize(fcpp_ctx *ctx);
/* Where the setup of a batch runs (fcpp_batch_create: every field's __init__ and O(1) decisions, MLP:63-107, 591-668, 898-1084, and the
 * cut of its path into kernel work).  FCPP_SETUP_AUTO: on the DEVICE for batches of 16 fields and more with obstacle_mode = FLAG -- at the
 * reference's own sampling (sample_spacing = 0) and, since round 5, at any uniform sampling when no field of the batch has obstacles;
 * only the fcpp_field records go up, fcpp_field_info comes back -- and on the host's cores otherwise (obstacle-aware swaths, dense
 * sampling of fields with obstacles, fields beyond the device planner's limits, a handful of fields).  _HOST: always on the host (the checker of the device
 * path: both build the same tables, byte for byte).  _DEVICE: batches the device planner does not take fail with FCPP_EUNSUPPORTED.
 * The environment variable FCPP_SETUP=host|device sets the initial mode of new contexts. */
enum { FCPP_SETUP_AUTO = 0, FCPP_SETUP_HOST = 1, FCPP_SETUP_DEVICE = 2 };
int fcpp_ctx_set_setup(fcpp_ctx *ctx, int mode);
/* device memory for hosts without their own allocator (torch users pass tensor pointers instead) */
int fcpp_malloc(fcpp_ctx *ctx, int64_t bytes, void **dev_ptr);
int fcpp_free(fcpp_ctx *ctx, void *dev_ptr);
/* Output arrays for fcpp_batch_run, and the placement rule measured on MI355X: the hot kernels write x, y, kappa, v
 * and flagseg side by side, and five write streams within a few GiB of each other in device memory reach 4.6 TB/s where the same streams
 * >= 12-24 GiB apart reach 6.3-6.6 TB/s (small batches -- a few hundred MB of output -- live in the caches and do not care).
 *
 * fcpp_ctx_reserve_outputs gives the context an ARENA for that: ONE device allocation of 4 x pitch + lane bytes, made once (an allocation
 * of this size takes the driver seconds: it belongs to context creation, not to a plan call), five lanes `pitch_bytes` apart (0:
 * FCPP_OUTPUT_PITCH) of `lane_bytes` each (0: one pitch).  fcpp_outputs_alloc(pitch_bytes = 0) then places array k in lane k, first fit
 * among the live allocations -- any number of live batches share the arena, each with its arrays a pitch apart.  Nothing is reserved
 * unless the caller asks: without an arena (or for arrays larger than a lane) pitch_bytes = 0 gives one allocation with the arrays back to
 * back, pitch_bytes > 0 one allocation of 4 x pitch + array bytes of the caller's own.  Free all five with fcpp_outputs_free(ctx, x).
 * fcpp_ctx_reserve_outputs again re-sizes the arena (no live allocations allowed); fcpp_ctx_destroy releases it. */
#define FCPP_OUTPUT_PITCH ((int64_t)24 << 30)
int fcpp_ctx_reserve_outputs(fcpp_ctx *ctx, int64_t lane_bytes, int64_t pitch_bytes);
int fcpp_ctx_outputs_info(const fcpp_ctx *ctx, int64_t *lane_bytes, int64_t *pitch_bytes, int64_t *live_bytes);   /* 0, 0, 0 without an arena */
int fcpp_outputs_alloc(fcpp_ctx *ctx, int64_t n_points, int64_t pitch_bytes, double **x_dev, double **y_dev, double **kappa_dev,
                       double **v_dev, uint32_t **flagseg_dev);
int fcpp_outputs_free(fcpp_ctx *ctx, double *x_dev);
int fcpp_memcpy_h2d(fcpp_ctx *ctx, void *dst_dev, const void *src, int64_t bytes);
int fcpp_memcpy_d2h(fcpp_ctx *ctx, void *dst, const void *src_dev, int64_t bytes);

/* ---- planner: TwoLayerPathPlannerV37.__init__ + plan_complete_coverage (MLP:63-107, 387-465) ---- */
/* Host-only sizing and decisions for n_fields planners (no GPU needed): __init__ (MLP:63-107),
 * _select_best_start_corner (:360-385), _determine_optimal_pass_order (:631-668), num_passes (:739),
 * num_loops (:916), reverse-fill lengths (:1154-1288).  Fields that raise get info[i].status < 0. */
int fcpp_plan_count(const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields,
                    const fcpp_field *fields, const fcpp_polys *obstacles /* may be NULL unless obstacle_mode = AVOID */,
                    fcpp_field_info *info_out);
/* Sizing alone, for a job sharded over several GPUs (contiguous blocks of fields cut on the point counts): points_out[i] =
 * n_main + n_head of field i, 0 for a field that raises.  Runs on the device where the device-side setup takes the batch (fcpp_ctx_set_setup;
 * only the field records go up, 8 bytes per field come back), else on the host's cores like fcpp_plan_count.  Synchronises. */
int fcpp_plan_points(fcpp_ctx *ctx, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields, const fcpp_field *fields,
                     const fcpp_polys *obstacles, int64_t *points_out);
/* Same setup, plus the per-field descriptors and the kernels' work lists on the device.  `fields` is read only during the call; it may be
 *   - DEVICE memory (round 5; engine.FieldTable.to_device(), a caller whose field table lives on the GPU): the device-side setup reads the
 *     records where they lie, nothing crosses PCIe in front of its first kernel (the headline's plan call 0.145 -> 0.138 ms); the writes that
 *     made the records must be ordered before the context's stream.  Records on another device are copied over.  The library's host paths
 *     (fewer than 16 fields, AVOID mode, FCPP_SETUP_HOST, fcpp_plan_count) copy them back first;
 *   - PINNED host memory (hipHostMalloc / hipHostRegister, a torch tensor with pin_memory): read by the device-side setup across PCIe where
 *     they lie -- no copy goes before its first kernel (fcpp_plan_points likewise);
 *   - pageable host memory: copied to the device first. */
int fcpp_batch_create(fcpp_ctx *ctx, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields,
                      const fcpp_field *fields, const fcpp_polys *obstacles, fcpp_batch **batch);
int fcpp_batch_info(const fcpp_batch *batch, fcpp_field_info *info_out /* n_fields, may be NULL */,
                    int64_t *total_points);
/* Where the time of fcpp_batch_create went (wall-clock milliseconds on the host): the plan call of the reference,
 * plan_complete_coverage (MLP:387-465), times its field setup together with the generation -- fcpp_batch_create + one fcpp_batch_run is
 * that call for a whole batch, and bench.py reports it as such (end to end) beside the time of the step alone. */
typedef struct fcpp_setup_times {
    double host_plan_ms;    /* __init__ + the O(1) decisions of every field (MLP:63-107, 591-668, 898-1084), blocks of fields on the host's cores */
    double templates_ms;    /* turn templates sampled on the device and copied back (close to 0 when the context already had them) */
    double tiler_ms;        /* the paths cut into kernel work (quiet runs, spans, wave tiles with their halos, general tiles) */
    double image_ms;        /* device allocation + the tables written into the context's pinned staging memory */
    double h2d_ms;          /* the one host-to-device copy, the per-field junction kernel, and the stream drained */
    double total_ms;        /* the whole call */
    int64_t image_bytes;    /* bytes copied to the device */
    int32_t threads;        /* host threads that took part (FCPP_THREADS; default: the machine's, at most 16) */
    int32_t device_setup;   /* 1: the setup ran on the device (fcpp_ctx_set_setup): host_plan_ms = field records up + plan + counting pass + totals
                               back, image_ms = layout + allocation + obstacle table, tiler_ms = tables written + per-batch constants +
                               fcpp_field_info back, h2d_ms = 0, image_bytes = bytes copied to the device */
} fcpp_setup_times;
int fcpp_batch_setup_times(const fcpp_batch *batch, fcpp_setup_times *out);
/* The hot path: sample every path point (MLP:720-830, 898-1084, 1154-1218, 1580-1608), curvature
 * (MLP:513-536), curvature clamp (MLP:467-511), forward/backward sweeps (MLP:538-589), validator
 * (MLP:1373-1424 + geofence / obstacle flags) and metrics (MLP:1290-1311).  Outputs are device
 * arrays of total_points elements; stats_dev has n_fields entries.
 * mode 0: staged pipeline (one kernel per operator, 7 launches); mode 1: fused single-pass kernels
 * (each point is written once, nothing is read back: closed-form runs and spans, wave tiles at sparse sampling,
 * general tiles) -- same results.
 * Buffers: the contract of the standalone operators below (natural alignment is enough -- x_dev at 8 (mod 16), flagseg_dev at 4 (mod 8) --,
 * each of the six outputs is written exactly over its extent, every point and every field's statistics record -- zeros for a field that
 * raises -- whatever the buffers held, and nothing beside them), in both modes; tests/test_gpu_step_guarded.py enforces it. */
int fcpp_batch_run(fcpp_batch *batch, double *x_dev, double *y_dev, double *kappa_dev, double *v_dev,
                   uint32_t *flagseg_dev, fcpp_field_stats *stats_dev, int mode);
/* The reference's plan call for a whole batch in ONE entry: plan_complete_coverage (MLP:387-465) sets a NEW field up and generates its path in
 * one call, and so does this -- fcpp_batch_create, output arrays for the batch's points (fcpp_outputs_alloc(pitch_bytes = 0): from the
 * context's arena when it has one, else an allocation of their own; released with fcpp_outputs_free(ctx, *x_dev)) and one fcpp_batch_run
 * (mode 1), with nothing of the caller's between the three: the step is enqueued the moment the setup's totals have sized the arrays.
 * stats_dev: n_fields records of the caller's, or NULL: the batch's own (fcpp_batch_own_stats; they live as long as the batch).
 * Asynchronous like fcpp_batch_run: the arrays are complete when the context's stream is.
 * The batch stays valid for further fcpp_batch_run calls on the same arrays (or others) until fcpp_batch_destroy.  On an error nothing is
 * left allocated.  bench.py's headline step is this call + the stream drained.
 * Buffers: as fcpp_batch_run -- whichever step the call takes (the direct step behind the counting pass, or fcpp_batch_run) writes every one of
 * the total_points elements of the five arrays it returns and nothing behind them, whatever the arena's memory held, and stats_dev needs
 * only the alignment of its 8-byte members (tests/test_gpu_step_guarded.py). */
int fcpp_batch_plan(fcpp_ctx *ctx, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_fields, const fcpp_field *fields,
                    const fcpp_polys *obstacles, fcpp_field_stats *stats_dev, fcpp_batch **batch, double **x_dev, double **y_dev,
                    double **kappa_dev, double **v_dev, uint32_t **flagseg_dev, int64_t *total_points);
/* the statistics records a batch keeps for callers that bring none (n_fields records inside the batch's own device allocation) */
int fcpp_batch_own_stats(const fcpp_batch *batch, fcpp_field_stats **stats_dev);
/* _generate_approach_path / _generate_departure_path (MLP:1313-1355): 50 points each, AoS (x,y) per
 * field at [field*100 .. +100); rows of fields without a kept start/end point, and of fields that raise, are left untouched.
 * Either pointer may be NULL. */
int fcpp_batch_connectors(fcpp_batch *batch, double *approach_xy_dev, double *departure_xy_dev);
/* fcpp_trajectory (below) on the batch's own paths: TWO per field, main work then headland (the reference times them separately,
 * MLP:423-431), so path 2 f starts at point_offset of field f and has n_main points, path 2 f + 1 follows with n_head; a field that raises
 * is two empty paths.  x / y / v / flagseg: the arrays of fcpp_batch_run.  totals_dev: 4 doubles per field (main length, main time,
 * headland length, headland time).  Runs after the batch's step on the same stream and synchronises it. */
int fcpp_batch_trajectory(fcpp_batch *batch, const double *x_dev, const double *y_dev, const double *v_dev, const uint32_t *flagseg_dev,
                          double *s_dev, double *t_dev, double *heading_dev, double *totals_dev);
int fcpp_batch_destroy(fcpp_batch *batch);
/* Per-kernel device timing with HIP events (bench.py's roofline leg).  enable = k > 0: every k-th fcpp_batch_run from now on
 * dispatches each of its kernels with a start and a stop event of its own (hipExtLaunchKernel: the dispatch's time stamps, no
 * marker packets between the kernels; up to 256 runs are kept); such a run costs ~15 us more than a plain one, hence the stride.
 * fcpp_batch_stage_times synchronises, returns the summed milliseconds per stage over the recorded runs, their number, and
 * clears the record. */
int fcpp_batch_set_profiling(fcpp_batch *batch, int enable);
int fcpp_batch_stage_times(fcpp_batch *batch, int max_stages, double *ms_sum_out, int *n_stages_out, int *n_runs_out);
const char *fcpp_batch_stage_name(int mode, int stage);
/* points one launch of stage `stage` of pipeline `mode` processes (the stages of fcpp_batch_stage_name; mode 1: the closed-form spans,
 * the closed-form runs, the wave tiles of the sparse kernel, the general tiles, and all points for the reduction) */
int fcpp_batch_stage_points(const fcpp_batch *batch, int mode, int stage, int64_t *points);
/* how the fused pipeline (mode 1) splits the batch: points in closed-form runs and spans (k_plan_quiet) / all other points */
int fcpp_batch_point_split(const fcpp_batch *batch, int64_t *quiet_points, int64_t *general_points);
/* how the per-field statistics of the fused pipeline are reduced: paths per class of k_reduce_stats, by statistic entries of a path
 * (<= 64: 8 lanes, <= 256: a wavefront, <= 1024: a workgroup, more: 64 workgroups + join); classes_out[4] */
int fcpp_batch_reduce_classes(const fcpp_batch *batch, int64_t *classes_out);

/* ---- standalone operators on caller-supplied paths (CSR offsets, n_paths+1, device) -------
 * Buffers of fcpp_curvature, fcpp_speed_plan, fcpp_trajectory / _counts / _sample, fcpp_dubins_*, fcpp_rs_*, fcpp_swath_*, fcpp_inset_*, fcpp_cells_*, fcpp_route_* and fcpp_field_path_*
 * (tests/test_gpu_guarded.py enforces it for these entries): a device pointer needs only the natural alignment of its element type, an
 * output is written exactly over its stated extent -- every element of it, nothing beside it --, inputs are never written, and an output
 * must not overlap an input or another output except where an entry says so.  The same holds, enforced by
 * tests/test_gpu_step_guarded.py, for fcpp_batch_run, fcpp_batch_plan, fcpp_batch_connectors, fcpp_batch_trajectory (above) and for
 * fcpp_verify, fcpp_validate, fcpp_straight_segments, fcpp_corner_turns, fcpp_fresnel and fcpp_cover_grid; two of them write an output
 * only in part and leave the rest of it untouched: fcpp_batch_connectors the rows of fields that raise or have no kept start / end point,
 * fcpp_corner_turns the points of a corner's row behind its counts_dev[2k] + counts_dev[2k+1].  The other entries keep what their own
 * comments state.
 * The offsets size the launches, so the host needs them: offsets_host (n_paths + 1 values, same content as offsets_dev) spares
 * the call a device-to-host copy and a stream synchronisation; NULL = the library reads offsets_dev back itself.  The tile table
 * built from the offsets is kept in the context and reused while consecutive calls bring the same offsets (compared by
 * content when offsets_host is given). */
/* _calculate_curvature for every interior point (MLP:513-536); end points get 0 */
int fcpp_curvature(fcpp_ctx *ctx, int64_t n_paths, const int64_t *offsets_dev, int64_t total_points,
                   const double *x_dev, const double *y_dev, double *kappa_dev, const int64_t *offsets_host);
/* _apply_curvature_based_speed_limit incl. _smooth_speed_profile (MLP:467-589); paths with fewer
 * than 3 points are returned unchanged (MLP:480-481).  clamp=0 runs _smooth_speed_profile only.
 * v_out_dev may alias v_in_dev; kappa_dev and n_adjusted_dev (int64[n_paths]) may be NULL. */
int fcpp_speed_plan(fcpp_ctx *ctx, const fcpp_vehicle *veh, int clamp, int64_t n_paths,
                    const int64_t *offsets_dev, int64_t total_points, const double *x_dev,
                    const double *y_dev, const double *v_in_dev, double *v_out_dev, double *kappa_dev,
                    int64_t *n_adjusted_dev, const int64_t *offsets_host);
/* verify_curvature_constraints (MLP:1373-1424) + _calculate_path_length/_calculate_work_time
 * (MLP:1290-1311) per path; stats_dev[n_paths] uses the main_* members for the whole path. */
int fcpp_verify(fcpp_ctx *ctx, const fcpp_vehicle *veh, int64_t n_paths, const int64_t *offsets_dev,
                int64_t total_points, const double *x_dev, const double *y_dev, const double *v_dev,
                fcpp_field_stats *stats_dev, const int64_t *offsets_host);
/* The validator on CALLER-SUPPLIED paths (README_en.md:183 "Electronic Fence Boundary Checking" -- the reference has the
 * bounds test of its start / end points only, MLP:322-343): per point the lateral-acceleration flag of verify_curvature_constraints
 * (MLP:1383-1401), the geofence flag against the path's field polygon and the obstacle flag against its obstacle polygons; per path the
 * statistics of fcpp_verify plus n_outside / n_in_obstacle.  Polygons are arbitrary simple polygons (host CSR tables, copied by the call):
 *   field_polys (NULL: no geofence): polygon p is the field of path p (n_polys == n_paths; a polygon of < 3 vertices: no geofence for that path).
 *       A point is FCPP_FLAG_OUTSIDE iff its signed distance to the polygon's boundary (+ inside, - outside; even-odd rule) is below
 *       -opt->geofence_tol -- for a convex field and a tolerance >= 0 the planner's own rule except beyond the corners, where the distance
 *       to the corner decides instead of the distances to the two edge lines.
 *   obstacles (NULL: none) with obstacle_offsets (n_paths + 1 values: path p is tested against the polygons [obstacle_offsets[p],
 *       obstacle_offsets[p + 1]); NULL: every path against all of them).  A point inside one (even-odd) is FCPP_FLAG_OBSTACLE.
 * flags_dev: total_points words, overwritten (FCPP_FLAG_ALAT | _OUTSIDE | _OBSTACLE).  Only veh's limits and opt->geofence_tol are read.
 * offsets_host as for the other standalone operators.  Synchronises. */
int fcpp_validate(fcpp_ctx *ctx, const fcpp_vehicle *veh, const fcpp_options *opt, int64_t n_paths, const int64_t *offsets_dev,
                  int64_t total_points, const double *x_dev, const double *y_dev, const double *v_dev, const fcpp_polys *field_polys,
                  const fcpp_polys *obstacles, const int64_t *obstacle_offsets, uint32_t *flags_dev, fcpp_field_stats *stats_dev,
                  const int64_t *offsets_host);
/* ---- trajectory: what a path-tracking controller follows -------------------------------------------------------------------------
 * Per point of every path its arc length s, its time stamp t and the heading of the VEHICLE: the running values of
 * _calculate_path_length (MLP:1294-1296) and _calculate_work_time (MLP:1303-1310, with its 0.1 m/s floor).  Per path p_0 .. p_(n-1), v in km/h:
 *     d_i = sqrt((x_i - x_(i-1))^2 + (y_i - y_(i-1))^2),  tau_i = d_i / max(((v_(i-1) + v_i) / 2) / 3.6, 0.1)      (the terms fcpp_verify sums)
 *     s_0 = t_0 = 0,  s_i = d_1 + .. + d_i,  t_i = tau_1 + .. + tau_i;  jumps and duplicate points are steps like any other; paths of 0 or 1
 *     points: zeros.  s and t never decrease along a path (exactly).
 *     heading_i = atan2(y_(i+1) - y_i, x_(i+1) - x_i), radians in (-pi, pi]: the chord of the step that LEAVES point i.  A zero step (both
 *     differences 0) takes the direction of the nearest earlier non-zero step of the path, leading zero steps that of the first non-zero step
 *     that follows, the last point that of its incoming step; a path without a non-zero step: 0.  With flagseg_dev, a point of kind
 *     FCPP_KIND_REVERSE is driven backwards: its heading is that direction turned by pi (h > 0: h - pi, else h + pi).
 * The order of the additions is fixed by the path alone (tiles and the blocks of the scan's spine are counted from the path's first point,
 * no atomics): a path gives the same bits alone, as path 4711 of a batch, and under any sharding.  s_dev, t_dev, heading_dev (total_points
 * each) and totals_dev (2 per path: length, time = s and t of its last point) may each be NULL.  offsets_host, the cached tile table and the
 * error codes as for the other standalone operators; synchronises. */
int fcpp_trajectory(fcpp_ctx *ctx, int64_t n_paths, const int64_t *offsets_dev, int64_t total_points, const double *x_dev, const double *y_dev,
                    const double *v_dev, const uint32_t *flagseg_dev /* may be NULL */, double *s_dev, double *t_dev, double *heading_dev,
                    double *totals_dev, const int64_t *offsets_host);
/* The trajectory at a fixed time step dt > 0 [s] (a controller's rate instead of the planner's uneven sample points): sample k of path p lies
 * at time k * dt (one rounding, never accumulated), k = 0 .. K_p - 1, K_p = floor(T_p / dt) + 1, T_p = the path's total time; with
 * include_end != 0 one more sample AT T_p when the last of them lies before T_p, and the last sample of every path IS its last point.
 * fcpp_trajectory_counts makes the samples' CSR offsets (n_paths + 1 values) from totals_dev (2 per path as fcpp_trajectory writes them; only
 * the times are read); out_offsets_host: NULL or room for a copy.  FCPP_EINVAL: dt <= 0; FCPP_ESIZE: a time that is negative or not finite,
 * a path of 2^31 samples or more.  Synchronises.  (A path without points has T_p = 0 like a path of one point: it gets its one sample, which
 * fcpp_trajectory_sample fills with NaN, flag word 0 and src_index -1.) */
int fcpp_trajectory_counts(fcpp_ctx *ctx, int64_t n_paths, const double *totals_dev, double dt, int include_end, int64_t *out_offsets_dev,
                           int64_t *out_offsets_host);
/* For the sample at time T: the step i with t_i <= T < t_(i+1) (the LAST such i where steps of zero duration repeat a time; T >= T_p: the last
 * point), lambda = (T - t_i) / (t_(i+1) - t_i); x, y, s interpolated linearly with lambda, and so is v -- linear IN TIME: the constant
 * acceleration over a step that the speed planner's sweeps assume; heading and flag word are those of point i, src_index = i (index into
 * the batch arrays).  s, t, heading are fcpp_trajectory's outputs for the same paths.  Every output may be NULL.  offsets_host /
 * out_offsets_host spare the read-backs (both tables are checked: FCPP_ESIZE); synchronises. */
int fcpp_trajectory_sample(fcpp_ctx *ctx, int64_t n_paths, const int64_t *offsets_dev, int64_t total_points, const double *x_dev,
                           const double *y_dev, const double *v_dev, const double *s_dev, const double *t_dev, const double *heading_dev,
                           const uint32_t *flagseg_dev /* may be NULL */, double dt, int include_end, const int64_t *out_offsets_dev,
                           int64_t total_samples, double *xs_dev, double *ys_dev, double *vs_dev, double *ss_dev, double *hs_dev,
                           uint32_t *flagseg_s_dev, int64_t *src_index_dev, const int64_t *offsets_host, const int64_t *out_offsets_host);
/* numpy.linspace straight segments (MLP:1013-1022, 1313-1355): seg_dev = n_seg x (x0,y0,x1,y1),
 * out_xy_dev = n_seg x n_points x 2 */
int fcpp_straight_segments(fcpp_ctx *ctx, int64_t n_seg, const double *seg_dev, int32_t n_points,
                           double *out_xy_dev);
/* _generate_corner_turn_arc (MLP:1580-1608) and _generate_corner_turn_with_reverse (MLP:1024-1084 with
 * _generate_optimal_reverse_path, MLP:1154-1218, and _calculate_distance_to_boundary, MLP:1220-1288) for n corners at once:
 * corner k = corners_dev[2k .. 2k+1], quadrant formula corner_index_dev[k] (0 LL, 1 LR, 2 UR, else UL; MLP:1049-1060).
 * The 15-point quarter arc of radius min_turn_radius goes to out_xy_dev[k * stride * 2 ..]; where with_reverse_dev[k] != 0
 * the reverse fill follows it: backwards along the arc's end tangent to the nearest side of the box [0, field_length] x
 * [0, field_width], at most 3R (2R when no side lies ahead), max(10, int(len / 0.5)) points.  counts_dev[2k], [2k+1] = points of
 * the arc and of the reverse fill.  stride (points per corner in out_xy_dev) must be >= 15 + max(10, int(3R / 0.5)).
 * The Shapely-dependent decision `gap.area > 0.1` (MLP:1070) stays with the caller (with_reverse_dev). */
int fcpp_corner_turns(fcpp_ctx *ctx, const fcpp_vehicle *veh, int64_t n, const double *corners_dev,
                      const int32_t *corner_index_dev, const int32_t *with_reverse_dev, double field_length,
                      double field_width, int32_t stride, double *out_xy_dev, int32_t *counts_dev);
/* Fresnel integrals C(t), S(t) = int_0^t cos|sin(pi u^2/2) du (README_en.md:111-120 promises the
 * clothoid; the reference has no code for it) */
int fcpp_fresnel(fcpp_ctx *ctx, int64_t n, const double *t_dev, double *c_dev, double *s_dev);

/* ---- GeneticAlgorithmSolver._calculate_distance / _calculate_fitness (GA:168-181) ---------- */
/* routes_dev: pop x n_nodes int32 permutations; D_dev: n_nodes x n_nodes float64 row-major.
 * order_mode 0 = left-to-right summation (bit-exact with the reference), 1 = tree reduction.
 * Precondition: every gene lies in [0, n_nodes); a chromosome that violates it gets distance = fitness = NaN (no out-of-range
 * read happens). */
int fcpp_ga_fitness(fcpp_ctx *ctx, int32_t n_nodes, int64_t pop, const double *D_dev,
                    const int32_t *routes_dev, double *dist_dev, double *fit_dev, int order_mode);

/* ---- GeneticAlgorithmSolver.solve: the evolution loop on the device (GA:64-115, 183-268) --------------
 * selection (GA:183-196), OX crossover (GA:198-242), swap mutation (GA:244-252), elitism (GA:254-268), fitness
 * (GA:168-181), best tracking and the convergence test (GA:90-113) for up to max_generations, whole generations on the
 * GPU.  The reference draws from the unseeded stdlib `random`; here every decision comes from the counter-based
 * generator Philox4x32-10 with key = seed and counter = (generation, pair, stream, block):
 *   stream 1 + s, word j : tournament candidate j of slot s = word % population_size, duplicates are redrawn
 *   stream 3             : crossover iff unit(w0, w1) < crossover_rate; cut points i = w2 % n, j = w3 % (n-1), j += (j >= i)
 *   stream 4 + c         : mutation of child c iff unit(w0, w1) < mutation_rate; positions as for the cut points
 *   unit(a, b) = ((a >> 5) * 2^26 + (b >> 6)) / 2^53
 * so a run is reproducible and identical to oracle/fcpp_oracle.c: orc_ga_evolve.  Ties in the elitism order go to the
 * larger index.  routes_dev must hold permutations of 0 .. n_nodes-1 (checked on the device before the first generation:
 * FCPP_EINVAL otherwise).  population_size must be even (the reference grows an odd population by one per generation, GA:203),
 * elite_size < population_size, tournament_size <= min(64, population_size), 2 <= n_nodes <= 2048. */
typedef struct fcpp_ga_config {   /* GAConfig, GA:20-29, + seed */
    int32_t population_size, max_generations;
    double crossover_rate, mutation_rate;
    int32_t elite_size, tournament_size, convergence_threshold, _pad;
    uint64_t seed;
} fcpp_ga_config;
typedef struct fcpp_ga_result {   /* the `stats` of GA:122-127 */
    int32_t generations;          /* generation + 1 */
    int32_t convergence_gen;      /* generation - generations_without_improvement */
    double best_distance, best_fitness;
} fcpp_ga_result;
/* routes_dev: pop x n int32, in = the initial population, out = the final one; best_route_dev: n int32 (as found, not yet
 * rotated to start at node 0, GA:118-120); hist_dev: NULL or 2 * max_generations doubles = best_fitness_history then
 * avg_fitness_history (GA:106-107; entries [0, generations) of each half are written).  Synchronises the stream. */
int fcpp_ga_evolve(fcpp_ctx *ctx, int32_t n_nodes, const fcpp_ga_config *cfg, const double *D_dev, int32_t *routes_dev,
                   int32_t *best_route_dev, double *hist_dev, fcpp_ga_result *result);

/* ---- scheduler inputs -----------------------------------------------------------
 * MultiVehiclePlanner._build_distance_matrix (MVP:229-259) / MultiFieldPlanner._calculate_distance_matrix (MFP:263-288):
 * D[i][j] = sqrt((x_i - x_j)^2 + (y_i - y_j)^2), 0 on the diagonal; node 0 is the depot, the others field centroids.
 * D_dev: n x n float64 row-major (the layout fcpp_ga_fitness / fcpp_ga_evolve take). */
int fcpp_distance_matrix(fcpp_ctx *ctx, int32_t n, const double *x_dev, const double *y_dev, double *D_dev);
/* MultiFieldPlanner._find_best_connection (MFP:290-320) for a batch of consecutive node pairs: pair p connects one of the exit
 * candidates [from_off[p], from_off[p+1]) of its first node with one of the entry candidates [to_off[p], to_off[p+1]) of its
 * second node; the shortest pair wins, the FIRST one in (exit-major, entry-minor) order among equals (the reference's
 * `distance < best_distance`).  Outputs per pair: the winning candidate indices (into fx/fy and tx/ty) and the distance
 * (-1, -1, +inf when a candidate list is empty).  All arrays on the device. */
int fcpp_best_connections(fcpp_ctx *ctx, int64_t n_pairs, const int64_t *from_off_dev, const int64_t *to_off_dev,
                          const double *fx_dev, const double *fy_dev, const double *tx_dev, const double *ty_dev,
                          int32_t *best_from_dev, int32_t *best_to_dev, double *best_dist_dev);

/* ---- Dubins connectors: the shortest forward-only path between two POSES for a vehicle with a turning radius --------------------------
 * Build-defined.  What they replace: the reference's straight 50-point approach / departure lines (MLP:1313-1355, "简单的直线连接"), the
 * missing link between main work and headland, and the Euclidean transit cost of the scheduler inputs above; its roadmap asks for them
 * (doc/两层路径规划器 - 深度优化和改进路线图.md section 1.2: shortest path between two poses, sampled at a spacing).  Forward motion only
 * (paths that also reverse: the Reeds-Shepp connectors below).
 * A pose is (x, y, heading): metres, and radians as fcpp_trajectory writes them (any finite value with |heading| <= 1e5).  All arrays are
 * device pointers, SoA float64; `radius` > 0 is ONE scalar per call.  Words: 0 LSL, 1 LSR, 2 RSL, 3 RSR, 4 RLR, 5 LRL (L = left /
 * counter-clockwise arc, R = right arc, S = straight).  For each pair all six closed forms (Dubins 1957; Shkel & LaValle 2001) are evaluated
 * on the turning circles' centres -- formed from the DIFFERENCE of the two positions, in metres, no normalising rotation or scaling -- the
 * feasible ones kept and the shortest taken; among equal totals the LOWEST word index wins, so the choice is a function of the inputs alone.
 * seg: three segment lengths in metres, each >= 0, an arc's length = radius x its angle in [0, 2 pi); total = (seg[0] + seg[1]) + seg[2].
 * The rules at the edges (csrc/fcpp_dubinsfn.h, one function for host and device: the same bits on both):
 *   - every arc angle is a difference reduced into [0, 2 pi); a reduced angle ABOVE 2 pi - 2^-43 (within 128 ulp of a full circle) is 0.
 *     Without it an angle that is mathematically 0 but comes out as -1 ulp would be a full circle of path that is not there -- exactly where
 *     a start heading points at the goal or two swaths are exactly parallel.  The price: the end pose of such a path may be off by up to
 *     2^-43 x (radius + straight) metres;
 *   - with c2 the computed squared distance of the two circle centres a word uses: LSR / RSL are feasible iff c2 >= 4 R^2 (1 - 2^-48), RLR / LRL
 *     iff c2 <= 16 R^2 (1 + 2^-48); inside those bands of 16 ulp the root's argument is clamped to 0 (the circles touch), beyond them the word is
 *     infeasible (the shortest length is discontinuous in the poses there: a last bit may decide which word wins);
 *   - circle centres closer than 2^-40 R count as one centre (no first arc; the straight keeps its tiny length).  Start == goal exactly:
 *     word 0, lengths 0, 0, 0;
 *   - a pair with a non-finite coordinate difference or heading (or differences so large that their squares overflow): word -1, lengths and total NaN -- per pair, the call succeeds (as
 *     fcpp_ga_fitness treats bad genes).
 * Errors, checked before anything touches the GPU: FCPP_EINVAL for a NULL handle or array, a radius or spacing that is <= 0 or not finite;
 * FCPP_ESIZE for negative or inconsistent sizes.  Asynchronous on the context's stream unless stated. */
/* pair i = (from i -> to i), a lane per pair.  word_dev: n int32; seg_dev: 3 per pair; len_dev: n totals.  Any output may be NULL. */
int fcpp_dubins_solve(fcpp_ctx *ctx, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                      const double *to_x_dev, const double *to_y_dev, const double *to_h_dev, double radius, int32_t *word_dev,
                      double *seg_dev, double *len_dev);
/* The transit matrix: D[i][j] = shortest length from exit pose i to entry pose j, row-major n_from x n_to -- the layout fcpp_ga_fitness /
 * fcpp_ga_evolve take when both lists are the same nodes.  NOT symmetric; the diagonal of a list against itself is 0.  Entry (i, j) has the
 * bits fcpp_dubins_solve gives for that pair.  word_dev: NULL or n_from x n_to int8.  At most 2^20 poses per side. */
int fcpp_dubins_matrix(fcpp_ctx *ctx, int64_t n_from, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                       int64_t n_to, const double *to_x_dev, const double *to_y_dev, const double *to_h_dev, double radius, double *D_dev,
                       int8_t *word_dev);
/* Solved paths at a fixed spacing [m] (the pattern of fcpp_trajectory_counts / _sample): path p gets K_p = floor(total_p / spacing) + 1
 * samples at s = k * spacing (one multiplication, never accumulated), plus one more AT total_p when the last of them lies before it: the
 * first sample is the start pose, the last the path's end.  A path of total 0 has its one sample, a NaN path one sample of NaNs.
 * fcpp_dubins_counts: the samples' CSR offsets (n + 1) from len_dev; out_offsets_host: NULL or room for a copy.  FCPP_ESIZE: a length that is
 * negative or infinite, a path of 2^31 samples or more.  Synchronises. */
int fcpp_dubins_counts(fcpp_ctx *ctx, int64_t n, const double *len_dev, double spacing, int64_t *out_offsets_dev, int64_t *out_offsets_host);
/* Per sample x, y, heading in (-pi, pi] and the signed curvature (+1/radius on a left arc, -1/radius on a right arc, 0 on the straight),
 * evaluated from the START OF THE SEGMENT that contains s (the segment start poses are closed forms of the start pose), never from the
 * previous sample: a path gives the same bits alone and as path 4711 of a batch.  s at a junction belongs to the segment that starts there;
 * the last sample is the end of the last segment.  word_dev / seg_dev as fcpp_dubins_solve wrote them for the same start poses and
 * radius.  Every output may be NULL; out_offsets_host spares the read-back (the table is checked: FCPP_ESIZE).  Synchronises. */
int fcpp_dubins_sample(fcpp_ctx *ctx, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev, double radius,
                       const int32_t *word_dev, const double *seg_dev, double spacing, const int64_t *out_offsets_dev, int64_t total_samples,
                       double *xs_dev, double *ys_dev, double *hs_dev, double *kappas_dev, const int64_t *out_offsets_host);

/* ---- Reeds-Shepp connectors: the shortest path between two POSES for a vehicle that turns with a radius AND reverses -------------------
 * Build-defined (the reference's roadmap section 1.2 asks for them beside the Dubins paths; its vehicle already backs up at every outer
 * headland corner, MLP:1024-1082).  Where two swaths lie closer than two turning radii the forward-only link is a loop of R (pi + 4 g);
 * the reversing vehicle makes a three-point turn of little more than pi R.  Poses, arrays, radius and errors as for the Dubins entries;
 * the Dubins range of the headings does NOT carry over: the sine and cosine of the heading DIFFERENCE are taken, so the two headings of a
 * pair must not differ by more than 1e5 rad -- |heading| <= 5e4 for every pose is always safe.
 * For each pair all 48 words of Reeds & Shepp (1990) are evaluated -- the base formulas 8.1 - 8.4, 8.7 - 8.11 of the paper under time-flip,
 * reflection and backwards, on the DIFFERENCE of the two positions rotated into the start frame -- and the shortest feasible one taken; among
 * equal totals the LOWEST word index wins, so the choice is a function of the inputs alone.
 * THE WORD TABLE.  word = 4 * base + flip + 2 * mirror; letters L = left / counter-clockwise arc, R = right arc, S = straight; gears + forward,
 * - reverse:
 *     base 0  L+ S+ L+        base 3  L+ R- L-        base 6  L+ R- L- R+      base  9  L- S- R- L+
 *     base 1  L+ S+ R+        base 4  L- R- L+        base 7  L+ R- S- L-      base 10  R- S- R- L+
 *     base 2  L+ R- L+        base 5  L+ R+ L- R-     base 8  L+ R- S- R-      base 11  L+ R- S- L- R+
 * flip (bit 0) reverses every gear, mirror (bit 1) swaps L and R: the mirror image of a path has word ^ 2, the path with all gears reversed
 * word ^ 1.  In bases 7 - 11 the R arcs next to the straight are a quarter circle; in bases 5 and 6 the two middle arcs are equal.
 * seg: FIVE signed segment lengths in metres per pair, in the order of the word's letters: positive is driven forward, negative in reverse,
 * an arc's length = radius x its angle in [-pi, pi]; segments the word does not have are exactly 0.
 * total = (((|seg[0]| + |seg[1]|) + |seg[2]|) + |seg[3]|) + |seg[4]|.
 * The rules at the edges (csrc/fcpp_rsfn.h, one function for host and device: the same bits on both):
 *   - every arc angle is reduced into (-pi, pi]; where a word asks for an angle in [0, pi], a reduced value within 2^-43 below 0 is 0 and one
 *     within 2^-43 above pi is pi (and likewise for [-pi, 0]): an arc that is mathematically 0 but comes out as -1 ulp neither becomes a reverse
 *     stub nor rules its word out.  The price: the end pose of such a path may be off by up to 2^-43 x (radius + straight) metres;
 *   - a word's feasibility bound on rho^2 (the computed squared length, in radii, of the vector its formula uses: >= 4, <= 16, >= 8, >= 20 ...)
 *     holds with a relative band of 2^-48: inside the band the root's or arc cosine's argument is clamped to the edge, beyond it the word is
 *     infeasible (a last bit may decide which of two words of nearly equal length wins);
 *   - a vector shorter than 2^-40 radii has no direction and no length (its angle and its length count as 0: the end pose may be off by
 *     2^-40 x radius metres).  Start == goal exactly: word 0, five zeros, total 0;
 *   - a pair with a non-finite coordinate difference or heading: word -1, segments and total NaN -- per pair, the call succeeds.
 * The length is a metric on poses: symmetric, and the matrix of a list against itself has a zero diagonal. */
/* pair i = (from i -> to i), a lane per pair.  word_dev: n int32; seg_dev: 5 per pair; len_dev: n totals.  Any output may be NULL. */
int fcpp_rs_solve(fcpp_ctx *ctx, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                  const double *to_x_dev, const double *to_y_dev, const double *to_h_dev, double radius, int32_t *word_dev,
                  double *seg_dev, double *len_dev);
/* The transit matrix of the reversing vehicle: D[i][j] = shortest length from pose i to pose j, row-major n_from x n_to, the layout
 * fcpp_ga_fitness / fcpp_ga_evolve take.  Entry (i, j) has the bits fcpp_rs_solve gives for that pair.  word_dev: NULL or n_from x n_to
 * int8.  At most 2^20 poses per side. */
int fcpp_rs_matrix(fcpp_ctx *ctx, int64_t n_from, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                   int64_t n_to, const double *to_x_dev, const double *to_y_dev, const double *to_h_dev, double radius, double *D_dev,
                   int8_t *word_dev);
/* Solved paths at a fixed spacing [m], sampled PER GEAR RUN: a run is a maximal stretch of segments of one sign (zero segments aside; at
 * most three runs, a path of total 0 is one run).  A run of length T_r gets floor(T_r / spacing) + 1 samples at k * spacing from ITS start
 * (one multiplication, never accumulated), plus one more AT its end when the last of them lies before it.  So every cusp is a sample
 * twice: as the end of one run and as the start of the next, with the same x, y and heading and the opposite gear.
 * fcpp_rs_counts: the samples' CSR offsets (n + 1) from the words and segments; a NaN path has one sample.  FCPP_ESIZE: an infinite
 * segment, a path of 2^31 samples or more.  Synchronises. */
int fcpp_rs_counts(fcpp_ctx *ctx, int64_t n, const int32_t *word_dev, const double *seg_dev, double spacing, int64_t *out_offsets_dev,
                   int64_t *out_offsets_host);
/* Per sample x, y, the VEHICLE's heading in (-pi, pi] (on a reverse run it points against the motion), the signed curvature (+1/radius on
 * an L arc, -1/radius on an R arc, 0 on the straight) and the gear (int8: +1 forward, -1 reverse; 0 on the one sample of a NaN path),
 * evaluated from the START OF THE SEGMENT that contains the sample, never from the previous sample: a path gives the same bits alone and
 * as one path of a batch.  A position at a junction within a run belongs to the segment that starts there.  word_dev / seg_dev as
 * fcpp_rs_solve wrote them for the same start poses and radius.  Every output may be NULL.  Synchronises. */
int fcpp_rs_sample(fcpp_ctx *ctx, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev, double radius,
                   const int32_t *word_dev, const double *seg_dev, double spacing, const int64_t *out_offsets_dev, int64_t total_samples,
                   double *xs_dev, double *ys_dev, double *hs_dev, double *kappas_dev, int8_t *gears_dev, const int64_t *out_offsets_host);

/* ---- swaths of ANY polygon field: the batched cut and the angle search ------------------------------------------------------------------
 * Build-defined (the reference's swath generator reads a field's bounding box and four corners only).  Standalone like the connectors:
 * fcpp_batch_plan still takes convex quadrilaterals only and nothing here feeds it.  The caller passes the WORK AREA: a surveyed boundary goes
 * through the polygon inset below first (fcpp_inset_counts / _fill at the headland's width).  The records come in the stored order (by line, then along it); the order and direction in
 * which to DRIVE them is the swath router's, below.
 * A field is a list of rings: ring 0 the outer boundary, further rings holes (obstacles, keep-out areas).  Rings are closed implicitly and
 * may have either orientation; the interior follows the EVEN-ODD rule.  Two CSR levels: ring_offsets (n + 1: fields -> rings, ending at
 * n_rings), vert_offsets (n_rings + 1: rings -> vertices, ending at n_verts) over x, y.
 * THE RULE (csrc/fcpp_swathfn.h, one set of expressions for host and device: the same bits on both), for the track angle theta [rad],
 * |theta| <= 1e5, the working width W > 0, the offset 0 <= first < W of line 0 and min_length >= 0:
 *   - (s, c) = the library's own sine and cosine of theta (exactly 0 and 1 for theta = 0).  Every vertex gets u = x c + y s along the tracks
 *     and w = -x s + y c across them, once, so the two edges at a vertex see the same w; w_min, w_max over all vertices of the field;
 *   - line k lies at w_k = fl(fl(w_min + first) + fl(k W)); the field has K lines, the k >= 0 with w_k < w_max;
 *   - an edge (p, q), in ring order, crosses line k iff (w_p <= w_k) != (w_q <= w_k), at u = u_p + (w_k - w_p) / (w_q - w_p) * (u_q - u_p):
 *     an edge lying ON a line never crosses it, a line through a vertex is counted consistently, every line has an even number of crossings;
 *   - the crossings of a line sorted by u ascending (ties by ring, then edge) are paired (0, 1), (2, 3), ..; a pair is a swath iff
 *     u_b - u_a > min_length, so touches of zero length never appear;
 *   - a swath record: its end points a, b mapped back, (u c - w_k s, u s + w_k c), its line k, its length u_b - u_a.  Within a field the
 *     records are ordered by k, then by u;
 *   - the length sum of a (field, angle) pair adds the swath lengths in a fixed order (64 partial sums by k mod 64, each in record order,
 *     then folded 32, 16, .. 1): host and device give the same bits.
 * Status per (field, angle), int32: 0; FCPP_EINVAL -- no ring, a ring with fewer than 3 vertices, a vertex that is not finite (or not
 * finite in the track frame); FCPP_EUNSUPPORTED -- a line with more than FCPP_SWATH_MAX_CROSSINGS crossings, or more than 2^22 lines.  Such a
 * pair has 0 swaths, 0 lines and length 0; the other fields of the batch are unaffected (the convention of fcpp_batch_plan).
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or array, W <= 0 or not finite, first outside [0, W),
 * min_length negative or not finite, an angle that is not finite or beyond 1e5 in magnitude; FCPP_ESIZE -- negative sizes, 2^31 (field,
 * angle) pairs or more, offsets that do not start at 0, decrease, or do not end at the length of the array they index.  (The offsets and
 * the angles are read back for these checks.)  All three entries synchronise. */
#define FCPP_SWATH_MAX_CROSSINGS 64
/* The angle search: n fields x A angles (the list is shared by all fields).  n_swaths, n_lines (int32), length (float64), status (int32):
 * n x A row-major, entry (i, j) = field i at angles[j]; any may be NULL. */
int fcpp_swath_scores(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev,
                      int64_t n_verts, const double *x_dev, const double *y_dev, int64_t A, const double *angles_dev, double W, double first,
                      double min_length, int32_t *n_swaths_dev, int32_t *n_lines_dev, double *length_dev, int32_t *status_dev);
/* The cut, count -> scan -> fill like the *_counts / *_sample pairs: field i at angle_dev[i].  fcpp_swath_counts writes the CSR offsets of
 * the fields' swaths (n + 1; out_offsets_host: NULL or room for a copy), n_lines and status (n each, may be NULL). */
int fcpp_swath_counts(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev,
                      int64_t n_verts, const double *x_dev, const double *y_dev, const double *angle_dev, double W, double first,
                      double min_length, int64_t *out_offsets_dev, int64_t *out_offsets_host, int32_t *n_lines_dev, int32_t *status_dev);
/* fcpp_swath_fill writes the records of the same fields, angles and parameters at those offsets (n_total = offsets[n]): ax, ay, bx, by,
 * length (float64) and line (int32), any may be NULL.  A field never writes outside its own range of the offsets. */
int fcpp_swath_fill(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                    const double *x_dev, const double *y_dev, const double *angle_dev, double W, double first, double min_length,
                    const int64_t *offsets_dev, int64_t n_total, double *ax_dev, double *ay_dev, double *bx_dev, double *by_dev, int32_t *line_dev,
                    double *length_dev);

/* ---- the swath router: order and direction of one field's swaths --------------------------------------------------------------------------
 * Build-defined (the reference drives the stored order).  Path planning inside ONE field, batched over fields: nothing here orders fields
 * or vehicles.  Standalone like the swath entries, whose records it reads; nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_routefn.h, one set of expressions for host and device: the same bits on both).
 *   - A field has m swath records s = 0 .. m - 1 (fcpp_swath_fill's order) cut at the track angle theta.  Oriented swath p = 2 s + d: d = 0
 *     drives a -> b with heading theta, d = 1 drives b -> a with heading fl(theta + pi).  p ^ 1 ("p-bar") is the same swath the other way.  N = 2 m.
 *   - The transit block T of a field, N x N float64 row-major: T[p][q] = the shortest connector length from the exit pose of p to the entry
 *     pose of q at `radius`, mode 0 Dubins (fcpp_dubins_solve's function), mode 1 Reeds-Shepp (fcpp_rs_solve's); +inf where p and q are the
 *     same swath.  Every entry is evaluated on its canonical pair -- of (p, q) and (q-bar, p-bar) the one with the smaller p N + q -- and
 *     both entries get that value: T[p][q] and T[q-bar][p-bar] have equal BITS (a path driven backwards with flipped headings is a path).
 *   - Block i starts at t_offsets[i] = sum over j < i of (2 m_j)^2 (int64, n + 1 values).  A field whose swath status was non-zero has m = 0;
 *     a field with m > FCPP_ROUTE_MAX_SWATHS has a block of size 0 and the route status FCPP_EUNSUPPORTED.
 *   - A tour t[0 .. m - 1] holds one oriented swath of every swath; cost = E[t[0]] + T[t[0]][t[1]] + .. + T[t[m - 2]][t[m - 1]] + X[t[m - 1]],
 *     added left to right.  E, X: optional, 2 n_total float64 each, field i's N values at 2 swath_offsets[i]: the cost from the field's
 *     entry pose to each oriented swath and from each oriented swath to the field's exit pose; NULL = zeros.  Below e(u, v) = T[u][v],
 *     e(START, q) = E[q], e(p, END) = X[p].
 *   - Candidates c = 0 .. n_starts - 1, 1 <= n_starts <= 64: c = 0 the stored boustrophedon t[k] = 2 k + (k & 1); c = 1 its mirror
 *     t[k] = 2 k + 1 - (k & 1); c >= 2 nearest neighbour from the oriented swath floor((c - 2) N / (n_starts - 2)): repeatedly the orientation q
 *     of an unvisited swath with the least T[cur][q], ties to the lowest q (an entry not below +inf, NaN included, counts as +inf).
 *   - Improvement in sweeps.  A sweep evaluates EVERY move below on the current tour, takes the one with the least delta, ties to the lowest
 *     code, and applies it iff delta < -min_gain; otherwise the candidate is finished; it also stops after max_sweeps sweeps.  removed and
 *     added are each summed left to right, delta = added - removed; a NaN delta compares false and is never taken.
 *       Move A, reverse(i, j), 0 <= i <= j < m, code i m + j: t[i .. j] reversed and every member flipped (i = j turns one swath round).  u = the
 *         node at i - 1 or START, v = the node at j + 1 or END.  removed = e(u, t[i]) + e(t[j], v); added = e(u, t[j]-bar) + e(t[i]-bar, v).
 *         (The edges inside keep their value by the equality above.)
 *       Move B, or-opt, needs m > l: the segment t[i .. i + l - 1], l in {1, 2, 3}, moved to between positions k and k + 1 of the tour, k in
 *         [-1, m - 1] with k < i - 1 or k >= i + l; r = 0 as it is, r = 1 reversed and flipped.  Code m m + (((l - 1) 2 + r) m + i) (m + 1) + (k + 1).
 *         f = t[i], g = t[i + l - 1]; (in, out) = (f, g) for r = 0, (g-bar, f-bar) for r = 1; u, v the segment's neighbours, a, b the nodes at k
 *         and k + 1 (START / END at the ends).  removed = (e(u, f) + e(g, v)) + e(a, b); added = (e(u, v) + e(a, in)) + e(out, b).
 *     min_gain far above the rounding of a delta (1e-9 m) makes the true cost fall with every applied move; max_sweeps bounds the loop anyway.
 *   - Per field: every candidate's final cost is recomputed from its final tour; the winner has the least cost, ties to the lowest c;
 *     sweeps = the largest number of moves any candidate applied (a value below max_sweeps: no candidate stopped on max_sweeps);
 *     stored = candidate 0's cost AS CONSTRUCTED (what the stored order costs).  Status, int32: 0; FCPP_EUNSUPPORTED for
 *     m > FCPP_ROUTE_MAX_SWATHS (every candidate's tour is the stored order, the costs NaN); FCPP_EINVAL when `stored` is not finite (a
 *     non-finite swath, E or X: nothing is improved, every candidate stays as constructed).  For either the route is candidate 0 as
 *     constructed and the winner 0.  m = 0: an empty tour, cost 0.  m = 1: the cheaper direction under E + X (given a second candidate or a sweep).
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or array, radius <= 0 or not finite, mode not 0 or 1, an
 * angle not finite or beyond 1e5, n_starts outside 1 .. 64, min_gain negative or not finite, max_sweeps < 0 or > 2^20; FCPP_ESIZE -- negative
 * sizes, offsets that do not start at 0, decrease or do not end at their total, t_offsets that are not the blocks of the swath offsets.
 * The offsets are checked on the host: pass the host copies (swath_offsets_host, t_offsets_host) or NULL to have them read back.  Both
 * entries synchronise. */
#define FCPP_ROUTE_MAX_SWATHS 512
/* T_dev (t_total = t_offsets[n] float64): every field's transit block from its records ax .. by (n_total each) and its angle (n). */
int fcpp_route_transit(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                       const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev, const double *angle_dev,
                       double radius, int mode, const int64_t *t_offsets_dev, const int64_t *t_offsets_host, int64_t t_total, double *T_dev);
/* tours_dev: n_starts x n_total int32, candidate-major, each field's tour at its swath offsets; costs_dev: n x n_starts float64; route_dev:
 * n_total int32, the winner's oriented swaths in driving order; cost_dev, stored_dev (float64), winner_dev, sweeps_dev, status_dev (int32):
 * n each.  Any output may be NULL. */
int fcpp_route_solve(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                     const int64_t *t_offsets_dev, const int64_t *t_offsets_host, int64_t t_total, const double *T_dev, const double *E_dev,
                     const double *X_dev, int n_starts, double min_gain, int max_sweeps, int32_t *tours_dev, double *costs_dev,
                     int32_t *route_dev, double *cost_dev, int32_t *winner_dev, int32_t *sweeps_dev, int32_t *status_dev, double *stored_dev);

/* ---- connector clearance: solved connectors against the rings of a field ---------------------------------------------------------------------
 * Build-defined (the reference's connectors are straight lines that nothing tests).  Every connector of this library is the shortest Dubins or
 * Reeds-Shepp path between two poses and knows no boundary.  These entries TEST solved connectors against polygon fields -- exactly, piece
 * against edge, not by samples -- so that the swath router can avoid the blocked ones through its T / E / X arrays and what stays blocked is
 * reported.  No path is re-shaped by THESE entries (fcpp_conn_solve_clear below chooses another word).  Standalone like the router's
 * entries; nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_clearfn.h, one set of expressions for host and device: the same bits on both).
 *   - Region: a field of the two-level CSR of the swath entries above -- rings, closed implicitly, either orientation, even-odd interior.
 *     Edge g of a ring runs from vertex g to the next (the last back to the first): the points A + t e, 0 <= t < 1, e = fl(B - A).  There
 *     is NO margin parameter: pass the field's inset (fcpp_inset_counts / _fill at the margin) for one.
 *   - Path: start pose, radius, word and seg as fcpp_dubins_solve (mode 0: 3 segments) or fcpp_rs_solve (mode 1: 5 signed segments) wrote
 *     them.  Piece k is segment k where seg[k] != 0, from P_k to Q_k: Q_k the position at the END of segment k by the samplers' closed form
 *     (fcpp_dubins_sample / fcpp_rs_sample: from the start of the segment, never chained), P_k the Q of the piece before, the start pose for
 *     the first.  A straight piece is the segment P Q.  An arc has the centre c = P +- radius (-sin h, cos h) (+ for L, - for R; h the
 *     heading at P), runs from P to Q counter-clockwise for L forward or R reverse, else clockwise, and is WIDE when |seg[k]| / radius > pi.
 *     s_k = |seg[0]| + .. + |seg[k - 1]| added left to right.
 *   - Straight piece against edge, with e_p = Q - P:  o1 = e_p x (A - P), o2 = e_p x (B - P), o3 = e x (P - A), o4 = e x (Q - A).  They
 *     cross iff (o1 >= 0) != (o2 >= 0) and (o3 >= 0) != (o4 >= 0): half-open on both, so a path through a vertex is counted on ONE of the
 *     two edges there, never twice for one pair, and collinear overlap is no crossing.  At s = s_k + fmin(o3 / (o3 - o4), 1) |seg[k]|.
 *   - Arc piece against edge: f = A - c, a = e.e, b = f.e, q = f.f - radius^2, D = b b - a q.  For D > 0 (an edge that only touches the circle
 *     does not cross) each root t = (-b -+ sqrt D) / a with 0 <= t < 1 gives d = f + t e, which lies within the arc's sweep iff, with
 *     u = P - c, v = Q - c, c1 = u x d, c2 = d x v (both negated for a clockwise arc):  narrow arc: c1 >= 0 and c2 >= 0 and (u.d >= 0 or
 *     v.d >= 0);  wide arc: not (c1 < 0 and c2 < 0) -- cross and dot products against the arc's end directions, no angle is taken to
 *     decide.  Every root kept is a crossing (an arc may cross one edge twice); it lies at s = s_k + fmin(radius x angle, |seg[k]|),
 *     angle = atan2(c1, u.d) brought into [0, 2 pi).
 *   - Per (path, field): crossings (int32) = the (straight piece, edge) pairs that cross plus the kept roots of the (arc piece, edge)
 *     pairs -- the points where the path crosses the boundary; first_s (float64) = the least s of a crossing,
 *     +inf if there is none; inside (int8) = even-odd membership of the path's START point S from the same loop over the edges -- an
 *     edge counts iff (A.y > S.y) != (B.y > S.y) and (S.x - A.x) e.y < (S.y - A.y) e.x for e.y > 0, > for e.y < 0;
 *     clear = inside and crossings == 0.
 *   - An unsolved path (word outside the mode's table, a NaN segment, a start pose that is not finite): crossings 0, inside 0, first_s NaN,
 *     not clear.  pair_field = -1 means "no region": crossings 0, inside 1, first_s +inf, clear.
 *   - field_status (int32 per field): 0, or FCPP_EINVAL for a field with no ring, a ring of fewer than 3 vertices or a vertex that is not
 *     finite; every path tested against such a field -- or naming a field outside -1 .. n_fields - 1 -- gets the unsolved path's result.
 *     The other fields are unaffected.
 * There is NO cap on the edges of a field: the kernels walk them in LDS chunks of FCPP_CLEAR_EDGE_CHUNK edges (48 B each: 12 KiB of the
 * workgroup's 64 KiB).
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or array (outputs aside), radius <= 0 or not finite, mode not
 * 0 or 1, an angle not finite or beyond 1e5, penalty negative or not finite; FCPP_ESIZE -- negative sizes, offsets that do not start at 0,
 * decrease or do not end at their total, t_offsets that are not the blocks of the swath offsets.  (The CSR offsets are read back for these
 * checks.)  Both entries synchronise. */
#define FCPP_CLEAR_EDGE_CHUNK 256
/* Elementwise, a lane per path: path i starts at (from_x, from_y, from_h)[i] with word_dev[i] and seg_dev[3 i ..) (mode 0) or [5 i ..)
 * (mode 1), and is tested against field pair_field_dev[i] (int64) of the CSR.  Pairs are expected grouped by field; no result depends on
 * it.  crossings_dev (n int32), inside_dev (n int8), first_s_dev (n float64), field_status_dev (n_fields int32): any may be NULL. */
int fcpp_conn_clear(fcpp_ctx *ctx, int mode, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                    double radius, const int32_t *word_dev, const double *seg_dev, const int64_t *pair_field_dev, int64_t n_fields,
                    const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts, const double *x_dev,
                    const double *y_dev, int32_t *crossings_dev, int8_t *inside_dev, double *first_s_dev, int32_t *field_status_dev);
/* The matrix form over every field's transit block: fcpp_route_transit's arguments, then the fields' CSR (field i of the swaths is field i
 * of the CSR: ring_offsets holds n + 1 values), the penalty [m], T_dev (IN / OUT: the blocks as fcpp_route_transit wrote them) and B_dev
 * (uint8, T's layout and offsets).  Every canonical pair's connector is solved again, as fcpp_route_transit picks and solves it, and tested
 * once against its field: B[p][q] = B[q-bar][p-bar] = !clear, and where the pair is blocked T[p][q] = T[q-bar][p-bar] = fl(T[p][q] + penalty)
 * -- one sum, written to both, so the two keep EQUAL BITS (move A of the router relies on it).  Entries within one swath stay +inf with
 * B = 0.  penalty 0 reports without changing T.  A field beyond FCPP_ROUTE_MAX_SWATHS has no block; every pair of a field whose status
 * would be FCPP_EINVAL is blocked. */
int fcpp_route_transit_clear(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                             const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev, const double *angle_dev,
                             double radius, int mode, const int64_t *t_offsets_dev, const int64_t *t_offsets_host, int64_t t_total,
                             const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                             const double *x_dev, const double *y_dev, double penalty, double *T_dev, uint8_t *B_dev);
/* The PRICED transit block: every transit priced by the word that fcpp_conn_solve_clear would drive for it, not by a penalty on the shortest
 * one.  Build-defined.  The arguments of fcpp_route_transit_clear, but T_dev is OUT ONLY -- every entry of every block is written, no
 * fcpp_route_transit call is needed first -- and K_dev (int8, T's layout and offsets; may be NULL) takes the place of B_dev.  Offsets, the
 * canonical-pair rule, equal bits in mirrored entries and +inf within one swath are as for fcpp_route_transit.
 *   - For a canonical pair (p, q) of different swaths the poses are p's exit and q's entry, the field is field i of the CSR, and the rule of
 *     the clear connectors below (fcpp_conn_solve_clear: candidates, order (total, word), test, rank) is applied to that pair.
 *   - rank >= 0: T[p][q] = T[q-bar][p-bar] = that candidate's len -- the word's own total, no penalty -- and K = rank (below 48).
 *   - rank -1 (no word is clear: a start that is not inside the field, a field whose status is FCPP_EINVAL, an unsolved pair):
 *     T = fl(len of the shortest word + penalty), one sum written to both mirrored entries, and K = -1.
 *   - Entries within one swath: T = +inf, K = 0.
 * So where K == 0, T has the bits fcpp_route_transit writes; where K == -1, the bits fcpp_route_transit_clear writes with the same penalty;
 * K != 0 exactly where fcpp_route_transit_clear's B == 1; and elementwise plain <= priced <= penalised.  penalty 0 is allowed.  A field
 * beyond FCPP_ROUTE_MAX_SWATHS has no block and nothing of it is written.
 * Two launches, for the reason fcpp_conn_solve_clear gives: the first is fcpp_route_transit_clear's tiled walk, in which the lane that
 * owns a canonical pair writes the complete answer for the shortest word and lists the entry iff its field is valid, its start is inside
 * and the shortest word crosses; the call reads the list's length back and, unless it is 0, a second kernel looks at a listed entry's
 * words with a lane per word and overwrites T and K where one of them is clear.  Errors of the call as for fcpp_route_transit_clear
 * (FCPP_ESIZE also for 2^34 entries or more).  Synchronises. */
int fcpp_route_transit_priced(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                              const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev, const double *angle_dev,
                              double radius, int mode, const int64_t *t_offsets_dev, const int64_t *t_offsets_host, int64_t t_total,
                              const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                              const double *x_dev, const double *y_dev, double penalty, double *T_dev, int8_t *K_dev);
/* listed: the entries the first pass of this context's LAST fcpp_route_transit_priced handed to the second; word_launches: the second-pass
 * launches of all its calls so far (a call that lists nothing launches none).  Either may be NULL.  For tests. */
int fcpp_ctx_route_priced_passes(const fcpp_ctx *ctx, int64_t *listed, int64_t *word_launches);

/* ---- clear connectors: per pair of poses the shortest word that stays off the field's rings -------------------------------------------------
 * Build-defined.  The entries above test a SOLVED connector; this one chooses: both solvers evaluate every word of a pair (6 Dubins, 48
 * Reeds-Shepp) and keep the shortest -- here the shortest one that is CLEAR of the pair's field is kept.  One word per pair, no margin
 * (pass the inset); via points and detours along the headland are the loop transits' (fcpp_loop_transit_solve, below).  Standalone like the clearance entries; nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_solveclearfn.h, one set of expressions for host and device: the same bits on both).  Nothing geometric is added: the
 * candidates come out of the solvers' own word enumerations and are tested by the clearance rule above.
 *   - Candidates of a pair: the words the solver finds feasible with a finite total, each with exactly the seg and total bits
 *     fcpp_dubins_solve / fcpp_rs_solve would write had that word won -- their rules at the edges unchanged (the 2^-43 angle snap, the 2^-48
 *     feasibility bands, + 0.0 on Reeds-Shepp segments).  A pair the solvers leave unsolved (an input that is not finite) has none.
 *   - Order: (total, word) ascending, the solvers' own tie rule.  The candidate at position 0 is the solvers' answer.
 *   - A candidate is tested as fcpp_conn_clear tests a solved path against field pair_field[i]: clear = inside and crossings == 0.
 *   - Result per pair: word (int32), seg (3 / 5 float64), len (float64, the word's total), rank, crossings (int32).
 *       rank >= 0: the candidate at that position of the order is the first clear one; crossings 0.  rank 0 has the bits of the solvers.
 *       rank -1:   no candidate is clear.  The SHORTEST word is returned -- the caller still has a drivable path -- with ITS crossings.
 *                  `inside` belongs to the start point alone: a start that is not inside decides this for all words at once.
 *       pair_field -1 ("no region"): the shortest word, rank 0, crossings 0.
 *       an unsolved pair (word -1, seg and len NaN; whatever pair_field says, -1 included), a field whose status is FCPP_EINVAL, a field
 *       index outside -1 .. n_fields - 1: rank -1 with the solvers' own output and crossings 0 -- fcpp_conn_clear's "unsolved path".
 *   - word and seg feed fcpp_dubins_counts / _sample, fcpp_rs_counts / _sample and fcpp_conn_clear as they are.
 * Two launches: a lane per pair solves and tests the shortest word and lists the pairs that are inside but cross; the call reads the list's
 * length back and, unless it is 0, a second kernel looks at a listed pair's words with a lane per word.
 * from_* / to_* (n float64 each), pair_field_dev (n int64), the fields' CSR as for fcpp_conn_clear.  word_dev, seg_dev, len_dev, rank_dev,
 * crossings_dev (n each, seg 3 n or 5 n), field_status_dev (n_fields int32): any may be NULL.  Errors of the call as for fcpp_conn_clear;
 * n is at most 2^31 - 1.  Synchronises. */
int fcpp_conn_solve_clear(fcpp_ctx *ctx, int mode, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                          const double *to_x_dev, const double *to_y_dev, const double *to_h_dev, double radius, const int64_t *pair_field_dev,
                          int64_t n_fields, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                          const double *x_dev, const double *y_dev, int32_t *word_dev, double *seg_dev, double *len_dev, int32_t *rank_dev,
                          int32_t *crossings_dev, int32_t *field_status_dev);
/* listed: the pairs the first pass of this context's LAST fcpp_conn_solve_clear handed to the second; word_launches: the second-pass launches
 * of all its calls so far (a call that lists nothing launches none).  Either may be NULL.  For tests. */
int fcpp_ctx_solve_clear_passes(const fcpp_ctx *ctx, int64_t *listed, int64_t *word_launches);

/* ---- field paths: every field's routed swaths and connectors as ONE sampled path per field ------------------------------------------------
 * Build-defined.  The last stage of the polygon-field chain (inset -> angle -> swaths -> route -> PATH), batched like the others: a counts
 * entry and a fill entry over all fields.  The result is a path set in CSR form (path_offsets), which fcpp_curvature, fcpp_speed_plan,
 * fcpp_validate and fcpp_trajectory take as it is.  Standalone: nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_fpathfn.h, one set of expressions for host and device: the same bits on both).
 *   - Leg slots.  A field of m swaths has 2 m + 1 slots: slot 0 the entry connector, slot 2 k + 1 the k-th swath in driving order, slot
 *     2 k + 2 the connector behind it, the last slot the exit connector.  Field i's first slot is 2 swath_offsets[i] + i.  A slot without
 *     a leg has no samples: entry / exit without a pose, the one slot of a field with m = 0.  leg_offsets (2 n_total + n + 1 int64) holds
 *     the first sample of every slot; path_offsets (n + 1) is leg_offsets at the fields' first slots.
 *   - Driving order.  order = NULL: the stored boustrophedon 2 k + (k & 1).  Else n_total int32, field i's m values at swath_offsets[i]:
 *     oriented swaths 2 s + d LOCAL to the field, as fcpp_route_solve's route_dev holds them.  An entry outside 0 .. 2 m - 1 or a swath
 *     named twice gives status[i] = FCPP_EINVAL and no samples for that field -- found on the device; the other fields are unaffected.
 *   - A swath leg from (sx, sy) to (ex, ey) -- the oriented swath's poses as the router forms them -- of length len = length[s], the
 *     record's own: floor(len / spacing) + 1 samples, one more at the end when the last lies before it; sample k at
 *     t = fmin((k spacing) / len, 1), x = sx + t (ex - sx), y likewise; the LAST sample is (ex, ey) itself (a swath of length 0 is that one
 *     sample).  heading = the oriented heading wrapped into (-pi, pi], curvature 0, gear +1.  A length that is negative, infinite or NaN
 *     makes the field FCPP_EINVAL.
 *   - A connector leg: fcpp_dubins_solve's (mode 0) or fcpp_rs_solve's (mode 1) path at `radius` from the exit pose of the leg before (or
 *     the field's entry pose) to the entry pose of the leg behind (or the field's exit pose), sampled exactly as fcpp_dubins_sample /
 *     fcpp_rs_sample sample it: the last sample AT the path's end, Reeds-Shepp per gear run with every cusp twice.  Its end lies within
 *     2^-43 (radius + straight) metres of the next leg's start (the connectors' documented bound).  A pair with no path (word -1: a
 *     non-finite pose) makes the field FCPP_EINVAL.
 *   - Junctions stay doubled: a swath's last sample and the connector's first are two samples of one position.
 *   - part (int8): 0 swath, 1 connector between swaths, 2 entry connector, 3 exit connector.  gear (int8): +1 / -1.  leg (int32): the
 *     sample's slot within its field.  Every sample is evaluated from its leg alone, never from a neighbouring sample.
 *   - work_length[i] = the swath lengths added in driving order; transit_length[i] = the connector totals added in the router's order (entry
 *     first, exit last, left to right): fcpp_route_solve's cost of that order, up to the last bits of the entries the router evaluates
 *     on the mirrored pair.  Both NaN for a field that is FCPP_EINVAL.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, an entry or exit pose given in part,
 * radius or spacing <= 0 or not finite, mode not 0 or 1, an angle not finite or beyond 1e5; FCPP_ESIZE -- negative sizes, more than 2^30
 * swaths, offsets that do not start at 0, decrease or do not end at their total.  FCPP_ESIZE after the count: a leg or a field of 2^31
 * samples or more.  swath_offsets_host: the host copy, or NULL to have it read back.  Both entries synchronise.
 * fcpp_field_path_fill recomputes the leg records from the same inputs (nothing is kept in the context between the two calls); every one
 * of its seven outputs may be NULL. */
int fcpp_field_path_counts(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                           const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev, const double *length_dev,
                           const double *angle_dev, const int32_t *order_dev, double radius, int mode, double spacing,
                           const double *entry_x_dev, const double *entry_y_dev, const double *entry_h_dev, const double *exit_x_dev,
                           const double *exit_y_dev, const double *exit_h_dev, int64_t *path_offsets_dev, int64_t *path_offsets_host,
                           int64_t *leg_offsets_dev, double *work_length_dev, double *transit_length_dev, int32_t *status_dev);
int fcpp_field_path_fill(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                         const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev, const double *length_dev,
                         const double *angle_dev, const int32_t *order_dev, double radius, int mode, double spacing,
                         const double *entry_x_dev, const double *entry_y_dev, const double *entry_h_dev, const double *exit_x_dev,
                         const double *exit_y_dev, const double *exit_h_dev, const int64_t *leg_offsets_dev, int64_t total_samples,
                         double *x_dev, double *y_dev, double *heading_dev, double *kappa_dev, int8_t *part_dev, int8_t *gear_dev,
                         int32_t *leg_dev);

/* ---- clear field paths: the field paths, every connector driven by the shortest word that stays off a region ---------------------------------
 * Build-defined.  fcpp_field_path_counts / _fill drive the shortest word of every connector whatever it crosses; these two drive, per
 * connector, the word fcpp_conn_solve_clear chooses.  One word per connector, no margin (pass the inset); a leg without a clear word can ride a headland loop
 * (fcpp_loop_transit_solve, below: engine.field_paths(loops=...) splices such transits in); fcpp_route_transit_priced gives the router the matrix of the chosen words' lengths.  Standalone: nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_fpathfn.h over csrc/fcpp_solveclearfn.h, one set of expressions for host and device: the same bits on both).  The clear
 * field path of a batch is the field path above with ONE difference: in a field whose path status is FCPP_OK the record of every connector
 * slot -- word, seg, total -- is what fcpp_conn_solve_clear gives for the slot's from-pose and to-pose (the very poses the connector above is
 * solved from: the oriented swaths' poses with the router's unwrapped headings, the field's entry / exit pose), `radius`, and field i of the
 * region CSR (field i of the swaths is field i of the CSR: ring_offsets holds n + 1 values ending at n_rings).
 *   - rank >= 0: the leg drives that candidate of the pair's (total, word) order; rank 0 keeps the bits of the entries above.
 *   - rank -1 (no candidate clear, a start outside the region, a region field of status FCPP_EINVAL): the shortest word, as above, with its
 *     crossings (0 for a region of status FCPP_EINVAL).  The leg is still driven.
 *   - A pair with no path (word -1) makes the path field FCPP_EINVAL, as above.
 *   - Sample counts, sampling, doubled junctions, part / gear / leg follow from the record as above; transit_length is the sum of the
 *     chosen totals in the same order.
 * Per slot (2 n_total + n each): leg_rank, leg_crossings (int32; 0 on a swath slot, on a slot without a leg and in a path field that is
 * FCPP_EINVAL), leg_word (int32; -1 unless the slot is a connector), leg_seg (5 float64), leg_total (float64) -- the last three in
 * fcpp_debug_field_paths' layout (a swath's end point and length in seg[0 .. 2]; a failed field's records as the rule above left them), so
 * that the driven connectors go to fcpp_conn_clear and fcpp_dubins_sample / fcpp_rs_sample as they are.  Per field (n each, int32):
 * blocked = its connector legs of rank -1, reshaped = those of rank > 0, region_status = fcpp_conn_clear's field_status of region field i.
 * Any of the eight may be NULL.
 * Launches: the rule kernel of the entries above, then a lane per connector slot tests the RECORD's word (no second solve) and lists the
 * slots whose word starts inside a valid region but crosses; the call reads the list's length back and, unless it is 0, a second kernel
 * looks at a listed slot's words with a lane per word and overwrites the record; then the scan and the rest as above.
 * fcpp_field_path_fill_clear recomputes the records the same way; leg_offsets_dev is the counts call's.
 * Errors of the CALL, found before any kernel runs: those of fcpp_field_path_counts and those fcpp_conn_clear finds in its fields' CSR (a
 * NULL region array, negative sizes, offsets that do not start at 0, decrease or do not end at their total).  Both entries synchronise. */
int fcpp_field_path_counts_clear(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                                 const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev,
                                 const double *length_dev, const double *angle_dev, const int32_t *order_dev, double radius, int mode,
                                 double spacing, const double *entry_x_dev, const double *entry_y_dev, const double *entry_h_dev,
                                 const double *exit_x_dev, const double *exit_y_dev, const double *exit_h_dev,
                                 const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                                 const double *x_dev, const double *y_dev, int64_t *path_offsets_dev, int64_t *path_offsets_host,
                                 int64_t *leg_offsets_dev, double *work_length_dev, double *transit_length_dev, int32_t *status_dev,
                                 int32_t *leg_rank_dev, int32_t *leg_crossings_dev, int32_t *leg_word_dev, double *leg_seg_dev,
                                 double *leg_total_dev, int32_t *blocked_dev, int32_t *reshaped_dev, int32_t *region_status_dev);
int fcpp_field_path_fill_clear(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                               const double *ax_dev, const double *ay_dev, const double *bx_dev, const double *by_dev, const double *length_dev,
                               const double *angle_dev, const int32_t *order_dev, double radius, int mode, double spacing,
                               const double *entry_x_dev, const double *entry_y_dev, const double *entry_h_dev, const double *exit_x_dev,
                               const double *exit_y_dev, const double *exit_h_dev, const int64_t *ring_offsets_dev, int64_t n_rings,
                               const int64_t *vert_offsets_dev, int64_t n_verts, const double *region_x_dev, const double *region_y_dev,
                               const int64_t *leg_offsets_dev, int64_t total_samples, double *x_dev, double *y_dev, double *heading_dev,
                               double *kappa_dev, int8_t *part_dev, int8_t *gear_dev, int32_t *leg_dev);
/* listed: the connector slots the first pass of this context's LAST clear field-path call (counts or fill) handed to the second;
 * word_launches: the second-pass launches of all such calls so far (a call that lists nothing launches none).  Either may be NULL.  The
 * counts call skips the fields whose path status is FCPP_EINVAL; the fill keeps no status and also looks at their legs, which have no
 * samples, so its `listed` may be larger.  For tests; fcpp_ctx_solve_clear_passes keeps its meaning. */
int fcpp_ctx_field_path_clear_passes(const fcpp_ctx *ctx, int64_t *listed, int64_t *word_launches);

/* ---- loop transits: a blocked leg rides a headland loop round the obstacle ------------------------------------------------------------------
 * Build-defined.  The clear connectors above give ONE word per pair; where no word is clear (rank -1) the leg still crosses the pond.  A
 * LOOP TRANSIT of a pair P -> Q is three pieces: a clear connector from P to a station i of a loop, the loop's own samples from i forward
 * to a station j of the same loop, a clear connector from station j to Q.  fcpp_loop_transit_solve finds, per pair, the cheapest one over
 * all loops of the pair's field and all station pairs; fcpp_loop_transit_counts / _fill sample it.  Standalone: nothing here feeds
 * fcpp_batch_plan.
 * THE RULE (csrc/fcpp_transitfn.h over csrc/fcpp_solveclearfn.h, one set of expressions for host and device: the same bits on both).
 *   - Loops: a path set in the samplers' CSR form as fcpp_headland_path_fill writes it: loop l owns the samples loop_offsets[l] ..
 *     loop_offsets[l + 1] of loop_x, loop_y, loop_h (heading), loop_kappa, loop_part, loop_gear, and loop_s, the arc length of every sample
 *     from its loop's first sample -- fcpp_trajectory's s for that path set, which never decreases.  S_l is the s of the loop's last sample.
 *     field_loops (n_fields + 1, ending at n_loops): field f is served by the loops field_loops[f] .. field_loops[f + 1].  A loop is closed
 *     and driven FORWARDS only, in its sample order; pass the direction = +1 and direction = -1 loops as two loops to offer both.
 *   - Stations: the samples of a loop with local index k mod stride == 0 (stride >= 1), part 0 or 4 (a straight element, a followed arc:
 *     never a corner connector) and gear +1.  The station's pose is the sample's (x, y, heading).
 *   - in_i: the len fcpp_conn_solve_clear gives for P -> station i against region field pair_field[p]; out_j the same for station j -> Q.
 *     +inf unless rank >= 0.  Nothing is added to the geometry of a connector.
 *   - ride(i, j) = fl(s_j - s_i) for j >= i, fl(fl(S_l - s_i) + s_j) for j < i (the ride wraps over the loop's end).  i == j is a via point.
 *   - C = fl(fl(in_i + ride) + out_j).  The transit of a pair is the least C below +inf over (l, i, j), ties by (C, l, i, j) ascending.
 *   - Result per pair: found (int32), loop (int64), st_i, st_j (int64: the stations' GLOBAL sample indices into the loop arrays; -1 if not
 *     found), the two connectors' word (int32), seg (3 / 5 float64), len, rank (int32) as fcpp_conn_solve_clear writes them, ride, total
 *     (float64; C) and status (int32).  Not found: words -1, seg, len and ride NaN, ranks -1, total +inf.
 *   - status: 0 for a pair that is handled; FCPP_EINVAL for a pose that is not finite, a pair_field outside 0 .. n_fields - 1 (there is no
 *     "no region" here), a region field whose status is FCPP_EINVAL, a field with a loop whose first or last s is not finite;
 *     FCPP_EUNSUPPORTED for a field of more than FCPP_TRANSIT_MAX_STATIONS stations (raise the stride).  A pair whose field has no loop or no
 *     station is simply not found, with status 0.
 *   - THE RIDE IS NOT TESTED against the region: a headland pass lies inside its field by construction.  Its corner connectors (part 1)
 *     may not, as everywhere; fcpp_validate flags that.  One loop per transit: no ride on two loops.
 * The sampled path of a found pair (fcpp_loop_transit_counts / _fill), in this order: the in-connector sampled as fcpp_dubins_sample /
 * fcpp_rs_sample sample it (part 1); the loop's samples i .. j copied bit for bit, through the loop's end when j < i, with part
 * FCPP_PART_LOOP_RIDE and their own gear and kappa; the out-connector from station j's pose (part 1).  Junctions stay doubled as in the field
 * paths.  A pair that is not found has no samples.  path_offsets (n + 1) is the CSR fcpp_curvature, fcpp_speed_plan, fcpp_validate and
 * fcpp_trajectory take.  The counts and fill entries take the solve's outputs back as inputs; a record that names no two samples of one
 * loop counts as not found.  Every fill output may be NULL.
 * Launches of the solve: a wavefront per field lists its stations; the station counts are read back; the stations pass is the two passes of
 * fcpp_conn_solve_clear on the (pair, side, station) items -- the second is skipped when the first lists nothing; the pick pass, a
 * workgroup per pair, reduces (C, i, j) lexicographically; a lane per pair writes the result.  Temporaries: 16 B per (pair, side, station
 * slot), the slots the batch's largest station count rounded up to 256.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, radius or spacing <= 0 or not finite,
 * mode not 0 or 1, stride < 1; FCPP_ESIZE -- negative sizes, n or n_loops above 2^31 - 1, offsets that do not start at 0, decrease or do
 * not end at their total, 2^36 (pair, side, station slot) items or more.  FCPP_ESIZE after the count: a transit of 2^31 samples or more.
 * The *_host offsets: the host copy, or NULL to have it read back.  All three entries synchronise. */
#define FCPP_TRANSIT_MAX_STATIONS 2048
#define FCPP_PART_LOOP_RIDE 5
int fcpp_loop_transit_solve(fcpp_ctx *ctx, int mode, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                            const double *to_x_dev, const double *to_y_dev, const double *to_h_dev, double radius, const int64_t *pair_field_dev,
                            int64_t n_fields, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                            const double *x_dev, const double *y_dev, int64_t n_loops, const int64_t *loop_offsets_dev,
                            const int64_t *loop_offsets_host, int64_t n_samples, const double *loop_x_dev, const double *loop_y_dev,
                            const double *loop_h_dev, const double *loop_s_dev, const int8_t *loop_part_dev, const int8_t *loop_gear_dev,
                            const int64_t *field_loops_dev, const int64_t *field_loops_host, int64_t stride, int32_t *found_dev, int64_t *loop_dev,
                            int64_t *st_i_dev, int64_t *st_j_dev, int32_t *in_word_dev, double *in_seg_dev, double *in_len_dev, int32_t *in_rank_dev,
                            int32_t *out_word_dev, double *out_seg_dev, double *out_len_dev, int32_t *out_rank_dev, double *ride_dev,
                            double *total_dev, int32_t *status_dev);
int fcpp_loop_transit_counts(fcpp_ctx *ctx, int mode, int64_t n, const int32_t *found_dev, const int64_t *loop_dev, const int64_t *st_i_dev,
                             const int64_t *st_j_dev, const int32_t *in_word_dev, const double *in_seg_dev, const int32_t *out_word_dev,
                             const double *out_seg_dev, int64_t n_loops, const int64_t *loop_offsets_dev, const int64_t *loop_offsets_host,
                             int64_t n_samples, double spacing, int64_t *path_offsets_dev, int64_t *path_offsets_host);
int fcpp_loop_transit_fill(fcpp_ctx *ctx, int mode, int64_t n, const double *from_x_dev, const double *from_y_dev, const double *from_h_dev,
                           double radius, const int32_t *found_dev, const int64_t *loop_dev, const int64_t *st_i_dev, const int64_t *st_j_dev,
                           const int32_t *in_word_dev, const double *in_seg_dev, const int32_t *out_word_dev, const double *out_seg_dev,
                           int64_t n_loops, const int64_t *loop_offsets_dev, const int64_t *loop_offsets_host, int64_t n_samples,
                           const double *loop_x_dev, const double *loop_y_dev, const double *loop_h_dev, const double *loop_kappa_dev,
                           const int8_t *loop_gear_dev, double spacing, const int64_t *path_offsets_dev, const int64_t *path_offsets_host,
                           int64_t total_samples, double *x_dev, double *y_dev, double *heading_dev, double *kappa_dev, int8_t *part_dev,
                           int8_t *gear_dev);
/* listed: the (pair, side, station) items the first launch of the stations pass of this context's LAST fcpp_loop_transit_solve handed to the
 * second; word_launches: the second launches of all its calls so far (a call that lists nothing launches none).  Either may be NULL.  For
 * tests. */
int fcpp_ctx_loop_transit_passes(const fcpp_ctx *ctx, int64_t *listed, int64_t *word_launches);
/* The host twin, the same bits: fcpp_loop_transit_solve's outputs (any may be NULL), path_offsets (n + 1, may be NULL) and the samples
 * below cap (cap 0 or all six NULL: none).  Host pointers throughout.  Test infrastructure only. */
int fcpp_debug_loop_transits(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                             const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                             const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                             const double *y, int64_t n_loops, const int64_t *loop_offsets, int64_t n_samples, const double *loop_x,
                             const double *loop_y, const double *loop_h, const double *loop_kappa, const double *loop_s, const int8_t *loop_part,
                             const int8_t *loop_gear, const int64_t *field_loops, int64_t stride, double spacing, int32_t *found, int64_t *loop,
                             int64_t *st_i, int64_t *st_j, int32_t *in_word, double *in_seg, double *in_len, int32_t *in_rank, int32_t *out_word,
                             double *out_seg, double *out_len, int32_t *out_rank, double *ride, double *total, int32_t *status,
                             int64_t *path_offsets, int64_t cap, double *out_x, double *out_y, double *heading, double *kappa, int8_t *part,
                             int8_t *gear);

/* ---- mission paths: headland loops, field path and patch passes joined into ONE drive per field ---------------------------------------------
 * Build-defined.  The field paths, the headland paths and the patch passes each give a path set; nothing above joins them.  A MISSION PATH
 * drives, per field, a list of ITEMS in the caller's order -- each a path of ONE path set, open or a closed loop -- with a connector (a
 * JOINT) between consecutive items and from / to an optional entry / exit pose.  A closed loop may be entered at any of its stations and is
 * left there again after one lap; fcpp_mission_solve chooses every loop's station so that the joints are shortest in all,
 * fcpp_mission_counts / _fill sample the result.  Standalone: nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_missionfn.h, one set of expressions for host and device: the same bits on both).
 *   - Paths: a path set in the samplers' CSR form as the *_path_fill entries write it: path p owns the samples path_offsets[p] ..
 *     path_offsets[p + 1] (n_p of them) of x, y, heading, kappa, part, gear.  Concatenate several sets into one.
 *   - Items: field f owns the items item_offsets[f] .. item_offsets[f + 1], in DRIVING ORDER.  item_path (int64): the path the item drives;
 *     item_closed (int32): 0 open -- driven from its first sample to its last -- else a closed loop whose last sample repeats its first pose.
 *   - Nodes: an open item has one node, in-pose its first sample, out-pose its last.  A closed item's nodes are its stations, the loop
 *     transits' rule: the samples of local index k with k mod stride == 0 (stride >= 1), part 0 or 4 and gear +1 -- and k < n_p - 1;
 *     in-pose = out-pose = the sample's (x, y, heading).  The entry and the exit pose of a field (three columns each, NULL: none) are
 *     layers of one node.
 *   - An item whose path has no samples, and a closed item without a station, is SKIPPED: it drives nothing, is counted in `skipped`, and
 *     the items around it are joined to each other.
 *   - Cost: d(a, b) is the total fcpp_dubins_solve (mode 0) / fcpp_rs_solve (mode 1) give at `radius` from out(a) to in(b).  c_0 = 0, or
 *     fl(0 + d(entry, .)) with an entry; c_j[b] = min over a of fl(c_(j-1)[a] + d(a, b)), a sum that is not below +inf (NaN: a pose that is
 *     not finite) counting as +inf; the predecessor of b is the LOWEST a that attains the minimum.  The end is the lowest b of the last
 *     layer that attains the minimum, after the exit's edge fl(c[b] + d(b, exit)) when there is an exit.  The backtrack gives one node per
 *     kept item.  transit_length: the chosen joints' totals added in driving order from 0 -- the chain of additions of the optimum.
 *   - Slots: a field of m items has 2 m + 1 slots, its first 2 item_offsets[f] + f.  KEPT item j (the j-th not skipped) owns slot 2 j, the
 *     joint INTO it (empty for the first without an entry), and slot 2 j + 1, itself; slot 2 k behind the field's k kept items holds the
 *     exit joint (empty without an exit; with k = 0 the joint entry -> exit if both are given).  The slots behind are empty.
 *   - Samples: a joint as fcpp_dubins_sample / fcpp_rs_sample sample it from the out-pose before it, part FCPP_PART_JOIN, its own gear and
 *     kappa.  An open item: its samples as they are.  A closed item entered at local index k: the samples k, k + 1 .. n_p - 1, 0, 1 .. k --
 *     n_p + 1 of them, the seam a doubled junction like every other.  Copied samples keep x, y, heading, kappa, part and gear bit for bit.
 *     Beside the six columns every sample has slot (int32, local to its field) and src (int64: the source sample's index into the path
 *     set, -1 on a joint), by which pass ids, work flags or anything else per source sample can be gathered.  Junctions stay doubled.
 *   - Per field: status (int32), transit_length (float64), skipped (int32).  status FCPP_EUNSUPPORTED: a closed item of more than
 *     FCPP_MISSION_MAX_STATIONS stations (raise the stride); FCPP_EINVAL: a chosen joint without a word, i.e. a chosen in- or out-pose, entry
 *     or exit pose that is not finite.  Such a field has no samples and transit_length NaN, its per-item and per-slot rows are NOT
 *     written, and the other fields are unaffected.
 *   - Per item: item_station (int64), the chosen station's GLOBAL sample index; -1 for an open or a skipped item.
 *   - Per slot: slot_item (int64: the item of an item slot, else -1), slot_word (int32), slot_seg (5 float64, the field paths' record
 *     layout: three used by mode 0, the rest 0), slot_total (float64) of a joint; word -1, seg and total NaN on every other slot.
 * fcpp_mission_counts: slot_offsets (2 n_items + n_fields + 1) and path_offsets (n_fields + 1; the CSR fcpp_curvature, fcpp_speed_plan,
 * fcpp_validate and fcpp_trajectory take) from the solve's outputs handed back; a record that names no item of its field or no sample of
 * the item's path counts as empty.  fcpp_mission_fill: the samples; every output may be NULL.
 * Launches of the solve: a wavefront per item lists its stations; a workgroup per field walks its layers, the two cost vectors in LDS, a
 * wavefront per target node, its lanes over the source nodes, (cost, a) reduced lexicographically; a lane per field backtracks and writes
 * the records.  Temporaries: 12 B per (item, station slot).  Nothing is kept in the context.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, an entry or exit pose with fewer than
 * three columns, radius or spacing <= 0 or not finite, mode not 0 or 1, stride < 1; FCPP_ESIZE -- negative sizes, more than 2^30 items,
 * offsets that do not start at 0, decrease or do not end at their total, an item_path outside 0 .. n_paths - 1, slot_offsets that do not span
 * [0, total_samples].  FCPP_ESIZE after the count: a slot or a field of more than 2^31 - 2 samples.  The *_host tables: the host copy, or
 * NULL to have it read back.  All three entries synchronise. */
#define FCPP_MISSION_MAX_STATIONS 1024
#define FCPP_PART_JOIN 6
int fcpp_mission_solve(fcpp_ctx *ctx, int mode, int64_t n_fields, const int64_t *item_offsets_dev, const int64_t *item_offsets_host, int64_t n_items,
                       const int64_t *item_path_dev, const int64_t *item_path_host, const int32_t *item_closed_dev, int64_t n_paths,
                       const int64_t *path_offsets_dev, const int64_t *path_offsets_host, int64_t n_samples, const double *x_dev,
                       const double *y_dev, const double *heading_dev, const int8_t *part_dev, const int8_t *gear_dev, const double *entry_x_dev,
                       const double *entry_y_dev, const double *entry_h_dev, const double *exit_x_dev, const double *exit_y_dev,
                       const double *exit_h_dev, double radius, int64_t stride, int32_t *status_dev, double *transit_length_dev,
                       int32_t *skipped_dev, int64_t *item_station_dev, int64_t *slot_item_dev, int32_t *slot_word_dev, double *slot_seg_dev,
                       double *slot_total_dev);
int fcpp_mission_counts(fcpp_ctx *ctx, int mode, int64_t n_fields, const int64_t *item_offsets_dev, const int64_t *item_offsets_host, int64_t n_items,
                        const int64_t *item_path_dev, const int64_t *item_path_host, const int32_t *item_closed_dev, int64_t n_paths,
                        const int64_t *path_offsets_dev, const int64_t *path_offsets_host, int64_t n_samples, const int32_t *status_dev,
                        const int64_t *item_station_dev, const int64_t *slot_item_dev, const int32_t *slot_word_dev, const double *slot_seg_dev,
                        double spacing, int64_t *out_path_offsets_dev, int64_t *out_path_offsets_host, int64_t *slot_offsets_dev);
int fcpp_mission_fill(fcpp_ctx *ctx, int mode, int64_t n_fields, const int64_t *item_offsets_dev, const int64_t *item_offsets_host, int64_t n_items,
                      const int64_t *item_path_dev, const int64_t *item_path_host, const int32_t *item_closed_dev, int64_t n_paths,
                      const int64_t *path_offsets_dev, const int64_t *path_offsets_host, int64_t n_samples, const double *x_dev, const double *y_dev,
                      const double *heading_dev, const double *kappa_dev, const int8_t *part_dev, const int8_t *gear_dev,
                      const double *entry_x_dev, const double *entry_y_dev, const double *entry_h_dev, double radius, double spacing,
                      const int32_t *status_dev, const int64_t *item_station_dev, const int64_t *slot_item_dev, const int32_t *slot_word_dev,
                      const double *slot_seg_dev, const int64_t *slot_offsets_dev, int64_t total_samples, double *out_x_dev, double *out_y_dev,
                      double *out_heading_dev, double *out_kappa_dev, int8_t *out_part_dev, int8_t *out_gear_dev, int32_t *out_slot_dev,
                      int64_t *out_src_dev);
/* The host twin, the same bits: solve + counts + fill in one call.  Every output may be NULL; the samples below cap (cap 0 or all eight
 * NULL: none).  Host pointers throughout.  Test infrastructure only. */
int fcpp_debug_mission_paths(int mode, int64_t n_fields, const int64_t *item_offsets, int64_t n_items, const int64_t *item_path,
                             const int32_t *item_closed, int64_t n_paths, const int64_t *path_offsets, int64_t n_samples, const double *x,
                             const double *y, const double *heading, const double *kappa, const int8_t *part, const int8_t *gear,
                             const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x, const double *exit_y,
                             const double *exit_h, double radius, int64_t stride, double spacing, int32_t *status, double *transit_length,
                             int32_t *skipped, int64_t *item_station, int64_t *slot_item, int32_t *slot_word, double *slot_seg, double *slot_total,
                             int64_t *out_path_offsets, int64_t *slot_offsets, int64_t cap, double *out_x, double *out_y, double *out_heading,
                             double *out_kappa, int8_t *out_part, int8_t *out_gear, int32_t *out_slot, int64_t *out_src);

/* ---- path speeds: the accel-limited speed profile of the polygon chain's paths -----------------------------------------------------------------
 * Build-defined.  The sampled paths above (field paths, headland paths, loop transits, mission paths) carry per sample an exact pose, a
 * signed kappa, a part and a gear, but no speed; fcpp_speed_plan cannot supply it: it mirrors the reference's two loops (MLP:467-600), which
 * restart at every step below 1e-6 m -- every doubled junction and cusp of these paths --, take curvature from chords and never stop.
 * fcpp_path_speeds gives v in the units and CSR form fcpp_trajectory, fcpp_validate and fcpp_trajectory_sample take.
 * THE RULE (csrc/fcpp_speedfn.h, one set of expressions for host and device).  Per path p of n samples, speeds in m/s inside, u = v^2:
 *   - Cap: c_i = the smallest of (nominal_kmh[part_i] / 3.6)^2; (reverse_kmh / 3.6)^2 where gear_i = -1; and, where |kappa_i| > kappa_eps,
 *     (turn_kmh / 3.6)^2 and (sqrt(a_lat / |kappa_i|) * safety_factor)^2 -- the reference's formula (MLP:496-499) on the stored kappa.
 *     nominal_kmh is indexed by part: 0 straight working piece, 1 / 2 / 3 connectors, 4 followed arc, FCPP_PART_LOOP_RIDE, FCPP_PART_JOIN.
 *   - Stops: c_i = 0 at sample 0 with FCPP_SPEED_REST_START, at sample n - 1 with FCPP_SPEED_REST_END, and with FCPP_SPEED_STOP_AT_CUSPS at
 *     every sample whose gear differs from its predecessor's or its successor's within the path (both samples of a doubled cusp).
 *   - Steps: d_i = the chord from sample i - 1 to i, fcpp_trajectory's expression.  No threshold: a zero step passes the value on unchanged.
 *   - Profile: u_i = min over j of  c_j + 2 a_acc (d_(j+1) + .. + d_i) for j <= i  and  c_j + 2 a_dec (d_(i+1) + .. + d_j) for j >= i -- the
 *     forward sweep u_i = min(c_i, u_(i-1) + 2 a_acc d_i) followed by the backward sweep with a_dec: the greatest profile under the caps and
 *     both limits.  v_i = sqrt(u_i) * 3.6 [km/h], cap_i = sqrt(c_i) * 3.6.  The device composes the maps in a scan, the host twin walks the
 *     two sweeps: the same non-negative terms in other groupings, |v_dev - v_host| <= (n + 4) 2^-52 v; cap and the stops (exactly 0) are
 *     the same bits.  A path's bits may depend on where its tiles lie in the batch, to the same bound.
 *   - status (int32 per path): 0, or FCPP_EINVAL for a path with a non-finite x, y or kappa, a part outside 0 .. 7 or a gear other than
 *     +-1: NaN in v and cap over the whole path (every element is still written), found on the device; the other paths are unaffected.
 *   - Empty and one-sample paths are legal.  v_out and cap_out may each be NULL.
 * Launches: caps + tile aggregates, the blocked spine of fcpp_speed_plan's scan, apply.  Temporaries: the context's tile table of the path
 * set (shared with the other path operators).  Traffic: 26 B read twice and 16 B written per sample.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle, parameter block or required array, a parameter that is not
 * finite and positive (turn_kmh and the nominals may be +inf; a nominal may be 0, a stop), an unknown flag; FCPP_ESIZE -- negative sizes,
 * offsets that do not span [0, total_points] or decrease.  offsets_host: the host copy, or NULL to have it read back.  Synchronises.
 * Out of scope: dwell time at a gear change, jerk limits, speed-dependent widths. */
#define FCPP_SPEED_REST_START 1u
#define FCPP_SPEED_REST_END 2u
#define FCPP_SPEED_STOP_AT_CUSPS 4u
typedef struct fcpp_speed_params {
    double nominal_kmh[8];      /* by part */
    double reverse_kmh;         /* cap of the gear -1 samples */
    double turn_kmh;            /* cap where |kappa| > kappa_eps */
    double a_lat;               /* [m/s^2] */
    double a_acc, a_dec;        /* [m/s^2] speeding up, braking */
    double safety_factor;
    double kappa_eps;           /* [1/m] */
    uint32_t flags;             /* FCPP_SPEED_* */
    uint32_t _pad;
} fcpp_speed_params;
int fcpp_path_speeds(fcpp_ctx *ctx, const fcpp_speed_params *params, int64_t n_paths, const int64_t *offsets_dev, int64_t total_points,
                     const double *x_dev, const double *y_dev, const double *kappa_dev, const int8_t *part_dev, const int8_t *gear_dev,
                     double *v_out_dev, double *cap_out_dev, int32_t *status_out_dev, const int64_t *offsets_host);
/* The host twin: the plain sequential two-sweep form of the same header.  Host pointers throughout.  Test infrastructure only. */
int fcpp_debug_path_speeds(const fcpp_speed_params *params, int64_t n_paths, const int64_t *offsets, int64_t total_points, const double *x,
                           const double *y, const double *kappa, const int8_t *part, const int8_t *gear, double *v_out, double *cap_out,
                           int32_t *status_out);

/* ---- headland passes of ANY polygon field: the batched inset --------------------------------------------------------------------------
 * Build-defined (the reference insets a convex quadrilateral by mitres, MLP:867-877).  Standalone like the swath entries, whose field layout it
 * shares and whose input it makes: boundary -> headland pass centre lines -> work area -> swaths -> route.  Nothing here feeds fcpp_batch_plan.
 * For a field P (ring 0 the outer boundary, further rings holes, as above) and a distance d > 0 the inset is
 *     I_d(P) = { p inside P : dist(p, boundary of P) >= d }.
 * Headland pass k of working width W has the centre line  boundary of I_d  at d = first + (k - 1) W (usually first = W / 2); the work area
 * after m passes is I_(m W).  The boundary of I_d consists of pieces of the edges' inward offset segments and of arcs of radius d around
 * reflex vertices (the hole side rounds, convex corners stay sharp).  The inset may fall apart into several rings (a narrow neck), a hole
 * may merge with the outer boundary (a pond near the edge), the inset may be empty (0 rings): all three are ordinary results of status 0.
 * Input: simple rings of either orientation, holes inside ring 0 and disjoint from one another.  Self-intersecting rings and islands inside
 * holes give unspecified but bounded output.
 * THE RULE (csrc/fcpp_insetfn.h, one set of expressions for host and device: the same bits on both).
 *   - Every ring is oriented by the sign of its shoelace area (summed in vertex order about its first vertex) so that the interior lies on
 *     the left: ring 0 counter-clockwise, holes clockwise; a ring of the other orientation is traversed backwards.  Edges get the global
 *     index g in that traversal order; u_g the unit direction, n_g = (-u_y, u_x) the left normal, L_g the length of edge g from p_g to q_g.
 *   - Primitive 2 g is the offset segment p_g + d n_g + t u_g, 0 <= t <= L_g.  Primitive 2 g + 1 exists when the turn at q_g is to the right:
 *     the arc q_g + d (n_g cos s + u_g sin s) from n_g (s = 0) to the next edge's normal.
 *   - A point of a primitive is removed iff its distance to some OTHER edge's segment is below d (1 - 1e-12): a segment skips its own edge,
 *     an arc its two.  Per (primitive, edge) the parameters at which the primitive meets the edge's two end circles of radius d and two side
 *     lines at distance d are sorted, and every interval between consecutive ones is judged at its midpoint by the plain point-to-segment
 *     distance.  (The slack keeps a primitive's own joints; the candidates carry none, so sharp corners are exact.)
 *   - What survives of a primitive is a set of pieces (start, end); pieces shorter than 1e-9 m are dropped; pieces are numbered by
 *     (primitive, start parameter).  A field may have at most FCPP_INSET_PIECES_PER_EDGE x its edges pieces.
 *   - The successor of a piece is the piece whose start is nearest to its end by squared distance, ties to the lowest number.  Walking from
 *     the lowest unused piece until the walk returns to it gives one ring; rings come in the order of their lowest piece and start there.
 *     gap = the largest end-to-start distance of the pair's pieces.  A walk that runs into a used piece other than its first is
 *     FCPP_EUNSUPPORTED: the critical distance at which, say, three offsets pass through one point.
 *   - A segment piece emits its start point; an arc piece spanning a rad emits ceil(a / arc_step) points at equal angles from its start point
 *     on, without its end point: all on the circle, so chords are inscribed.  Rings are closed implicitly; the kept area is on the left
 *     (outer boundaries counter-clockwise, grown holes clockwise).
 * Status per (field, distance), int32: 0 (an empty inset included); FCPP_EINVAL -- no ring, a ring with fewer than 3 vertices, a vertex that
 * is not finite; FCPP_EUNSUPPORTED -- more than FCPP_INSET_MAX_EDGES edges, more pieces than the cap, an arc piece of 2^18 points or more,
 * the degenerate walk.  A pair with a non-zero status has 0 rings, 0 vertices and gap 0; the other pairs of the batch are unaffected.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or array, a distance <= 0 or not finite, arc_step not in
 * (0, pi/2]; FCPP_ESIZE -- negative sizes, 2^31 (field, distance) pairs or more, offsets that do not start at 0, decrease, or do not end at
 * the length of the array they index.  (The offsets and the distances are read back for these checks.)  Both entries synchronise.  Fields of
 * more than 64 edges keep their piece records in device memory for the duration of the call: 208 KiB for each of up to 1024 pairs. */
#define FCPP_INSET_MAX_EDGES 1024
#define FCPP_INSET_PIECES_PER_EDGE 4
/* Counting pass: n fields x D distances (the list is shared by all fields), pair (i, j) = i D + j.  Writes the CSR offsets pairs -> rings and
 * pairs -> vertices (n D + 1 int64 each; the host pointers: NULL or room for a copy), status (int32) and gap (float64), n D each, may be NULL. */
int fcpp_inset_counts(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev,
                      int64_t n_verts, const double *x_dev, const double *y_dev, int64_t D, const double *dist_dev, double arc_step,
                      int64_t *pair_ring_offsets_dev, int64_t *pair_ring_offsets_host, int64_t *pair_vert_offsets_dev,
                      int64_t *pair_vert_offsets_host, int32_t *status_dev, double *gap_dev);
/* fcpp_inset_fill writes the rings of the same fields, distances and arc_step at those offsets: out_vert_offsets_dev (total_rings + 1 int64:
 * rings -> vertices), out_x_dev, out_y_dev (total_verts float64) and out_src_dev (int32 per vertex: the primitive, 2 g or 2 g + 1, that emitted
 * it -- odd for arcs, g the source edge).  Any output may be NULL.  A pair never writes outside its own ranges. */
int fcpp_inset_fill(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                    const double *x_dev, const double *y_dev, int64_t D, const double *dist_dev, double arc_step,
                    const int64_t *pair_ring_offsets_dev, const int64_t *pair_vert_offsets_dev, int64_t total_rings, int64_t total_verts,
                    int64_t *out_vert_offsets_dev, double *out_x_dev, double *out_y_dev, int32_t *out_src_dev);

/* ---- field cells: a polygon field split along a cut direction into cells that are ordinary fields ----------------------------------------
 * Build-defined (the reference plans one quadrilateral at one angle).  Standalone like the swath and inset entries, whose field layout it
 * shares: work area -> CELLS -> angle, swaths, route and path per cell.  Nothing here feeds fcpp_batch_plan.
 * Input per field: its rings (simple, pairwise disjoint, closed implicitly, either orientation, EVEN-ODD interior; several outer rings are
 * fine -- an inset can split a field), a cut angle phi (finite, |phi| <= 1e5), events (0 = reflex: a cut at every reflex vertex, the cells
 * are convex; 1 = extrema: only where the boundary turns back across the cuts, the cells are monotone across the cuts) and min_area >= 0.
 * THE RULE (csrc/fcpp_cellfn.h, one set of expressions for host and device: the same bits on both).
 *   - Frame: (s, c) = fc_sincos(phi); every vertex gets u = x c + y s, w = -x s + y c once.  Cuts are segments of constant w.
 *   - Orientation: a ring's depth is the number of the field's other rings that contain its first vertex (the swath rule's half-open
 *     crossing test).  Even depth is driven counter-clockwise, odd depth clockwise (shoelace sum in x, y about the ring's first vertex): the
 *     interior is on the left of every oriented edge.  Vertices keep their field-local input index; oriented edge g leaves vertex g.
 *   - Rays: with e1 = v - pred, e2 = succ - v in (u, w), v is reflex iff cross(e1, e2) < 0.  In mode extrema v must also be extremal: the
 *     first vertices backwards and forwards whose w differs from w_v lie on the same side of it.  A +u ray leaves a qualifying v iff
 *     w_pred > w_v or w_succ < w_v, a -u ray iff w_pred < w_v or w_succ > w_v: the direction lies strictly inside the interior cone.
 *   - Ray end: over the edges (a, b) not incident to v with w_a != w_b: the edge meets the level at u_a if w_a = w_v, at u_b if w_b = w_v,
 *     at u_a + (w_v - w_a) / (w_b - w_a) (u_b - u_a) if (w_a < w_v) != (w_b < w_v).  A ray runs inside the field, so only an edge with the
 *     interior towards it counts: w_b > w_a for a +u ray, w_b < w_a for a -u ray.  The ray ends at the nearest such point strictly ahead;
 *     ties go to a vertex hit, then to the lowest edge.  A hit at an edge end IS that vertex; otherwise a new node on the edge at (u, w_v).
 *   - Cuts are undirected: what two facing vertices shoot at each other is kept once.  An input vertex keeps its input x, y bits; a new node
 *     has x = u c - w s, y = u s + w c.  Rays are numbered 2 v + (0: +u, 1: -u); cuts and new nodes are numbered in ray order.
 *   - Half-edges: every oriented edge is split at its new nodes, ordered along the edge by w, into boundary pieces, numbered by (edge,
 *     position); then cut k gives half-edges B + 2 k (from its vertex) and B + 2 k + 1 (back).
 *   - Successor: arriving at a node, leave by the outgoing half-edge met first when turning clockwise from the direction back along the
 *     arriving one -- the sharpest left turn, never the arriving half-edge's twin -- by the signs of cross and dot products in (u, w); a
 *     boundary piece has the direction of its whole edge, a cut (+-1, 0).
 *   - Cells: from the lowest unused half-edge follow the successor until it returns.  A cell is a simple counter-clockwise ring (flat
 *     vertices kept) of its half-edges' origins, starting at the lowest.  A field of h holes and k cuts has 1 + k - h cells.  src per vertex:
 *     the field-local INPUT edge of the boundary piece leaving it, -1 where a cut leaves it; area: half the shoelace sum in x, y about the
 *     cell's first vertex.  Cells with area <= min_area are not emitted: `dropped` counts them, `dropped_area` sums them in cell order.
 * Status per field, int32: 0; FCPP_EINVAL -- no ring, a ring with fewer than 3 vertices, a vertex that is not finite (also in the frame), an
 * edge of length 0; FCPP_EUNSUPPORTED -- more than FCPP_CELLS_MAX_EDGES edges, a ray that meets nothing, two cuts leaving a node the same
 * way, or a walk that reaches a used half-edge other than its start (touching or crossing rings).  Such a field has no cells, no cuts and
 * nothing dropped; the other fields of the batch are unaffected.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or input array, an angle that is not finite or beyond 1e5 in
 * magnitude, events outside {0, 1}, a negative or non-finite min_area; FCPP_ESIZE -- negative sizes, offsets that do not start at 0, decrease,
 * or do not end at the length of the array they index.  (The offsets and the angles are read back for these checks.)  Both entries
 * synchronise.  Every table of a field lives in the workgroup's LDS: the entries allocate nothing per field. */
#define FCPP_CELLS_MAX_EDGES 1024
#define FCPP_CELLS_REFLEX 0
#define FCPP_CELLS_EXTREMA 1
/* Counting pass: angle_dev holds n cut angles.  Writes the CSR offsets fields -> cells and fields -> cell vertices (n + 1 int64 each; the
 * host pointers: NULL or room for a copy), status, n_cuts, dropped (int32) and dropped_area (float64), n each.  Any output may be NULL. */
int fcpp_cells_counts(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev,
                      int64_t n_verts, const double *x_dev, const double *y_dev, const double *angle_dev, int events, double min_area,
                      int64_t *cell_offsets_dev, int64_t *cell_offsets_host, int64_t *cell_vert_offsets_dev, int64_t *cell_vert_offsets_host,
                      int32_t *status_dev, int32_t *n_cuts_dev, int32_t *dropped_dev, double *dropped_area_dev);
/* fcpp_cells_fill writes the cells of the same fields, angles, events and min_area at those offsets: out_vert_offsets_dev (total_cells + 1
 * int64: cells -> vertices), out_x_dev, out_y_dev (total_verts float64), out_src_dev (int32 per vertex), cell_field_dev (int32 per cell: its
 * field) and area_dev (float64 per cell).  Any output may be NULL.  A field never writes outside its own ranges. */
int fcpp_cells_fill(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                    const double *x_dev, const double *y_dev, const double *angle_dev, int events, double min_area,
                    const int64_t *cell_offsets_dev, const int64_t *cell_vert_offsets_dev, int64_t total_cells, int64_t total_verts,
                    int64_t *out_vert_offsets_dev, double *out_x_dev, double *out_y_dev, int32_t *out_src_dev, int32_t *cell_field_dev,
                    double *area_dev);

/* ---- the cell tour: the order of a field's cells and the route of each ----------------------------------------------------------------------
 * Build-defined (the reference knows no cells).  A generalised travelling-salesman problem per field, batched over fields: each cell offers
 * a set of nodes, the task is the order of the cells and one node per cell so that inner costs plus joints are least.  The order is a local
 * search like the swath router's, the node choice for a given order is exact (a layered shortest path).  Standalone; nothing here feeds
 * fcpp_batch_plan.  Path planning inside ONE field: nothing here orders fields or vehicles.
 * THE RULE (csrc/fcpp_tourfn.h, one set of expressions for host and device: the same bits on both).
 *   - Field f owns the cells cell_offsets[f] .. cell_offsets[f + 1], m of them; cell c owns the variants var_offsets[c] .. var_offsets[c + 1],
 *     V_c of them.  A variant has an in-pose (ix, iy, ih), an out-pose (ox, oy, oh) and an inner cost w (all float64): w is the caller's
 *     price of driving it.
 *   - Cell c has N_c = 2 V_c nodes u = 2 v + d.  d = 0: the poses as given; d = 1: the same drive backwards, in-pose (ox, oy, fl(oh + pi)),
 *     out-pose (ix, iy, fl(ih + pi)); w(u) is the variant's w for both.  A field's nodes are numbered cell by cell, N_f of them.
 *   - The joint block D of a field, N_f x N_f float64 row-major: D[a][b] = the total fcpp_dubins_solve (mode 0) or fcpp_rs_solve (mode 1)
 *     gives at `radius` from out(a) to in(b); +inf where a and b belong to one cell.  Block f starts at d_offsets[f] = sum over earlier
 *     fields of N^2 (int64, n + 1 values).
 *   - E, X: optional, sum of N_f float64 each, field f's at 2 var_offsets[cell_offsets[f]]: the cost from the field's entry pose to in(b) and
 *     from out(b) to its exit pose; NULL = zeros.
 *   - plus(a, b) = fl(a + b) where that is below +inf, else +inf (NaN included).  The cost of an order c_1 .. c_k of the KEPT cells (V_c > 0),
 *     exact over the nodes: g_1[b] = plus(E[b], w(b)); g_j[b] = plus(min over a in c_(j-1) of plus(g_(j-1)[a], D[a][b]), w(b)), the
 *     minimiser the lowest a that attains the minimum; cost = min over b in c_k of plus(g_k[b], X[b]), the lowest b.  The backtrack gives
 *     one node per kept cell.  joint_length: the chosen D entries, with E and X where given, added in driving order from 0.
 *   - Candidates c = 0 .. n_starts - 1, 1 <= n_starts <= 64: c = 0 the stored order of the kept cells; c = 1 that order reversed; c >= 2
 *     nearest neighbour from the kept cell floor((c - 2) k / (n_starts - 2)): repeatedly the unvisited kept cell j with the least C[cur][j],
 *     ties to the lowest j, C[i][j] = min over a in i, b in j of D[a][b] (an entry not below +inf counts as +inf).
 *   - Improvement in sweeps.  A sweep evaluates EVERY move below on the current order, each by the cost of the moved order under the full
 *     rule above, takes the one with the least cost, ties to the lowest code, and applies it iff cost < fl(current cost - min_gain);
 *     otherwise the candidate is finished; it also stops after max_sweeps sweeps.
 *       Move A, reverse(i, j), 0 <= i < j < k, code i k + j: the ORDER of positions i .. j reversed (a cell's direction is the node choice's).
 *       Move B, or-opt, needs k > l: the segment of l in {1, 2, 3} cells at position i moved to between positions p and p + 1, p in
 *         [-1, k - 1] with p < i - 1 or p >= i + l; r = 0 as it is, r = 1 (l >= 2) reversed.  Code k k + (((l - 1) 2 + r) k + i) (k + 1) + (p + 1).
 *   - Per field: the winner is the candidate with the least final cost, ties to the lowest c; sweeps = the most moves any candidate
 *     applied; stored = the stored order with node stored_node[c] of every kept cell (int32, local to the cell; NULL = node 0), chained as
 *     the rule chains: s = plus(E, w), s = plus(plus(s, D), w) per cell, plus(s, X).  cost <= stored always.  order: field-local cell
 *     indices in driving order, the skipped cells (V_c = 0) behind the kept ones in stored order; node: the chosen local node of every cell
 *     in cell order, -1 for a skipped cell; skipped: their number.
 *   - Status, int32: 0; FCPP_EUNSUPPORTED for m > FCPP_TOUR_MAX_CELLS, a cell with N_c > FCPP_TOUR_MAX_CELL_NODES or N_f >
 *     FCPP_TOUR_MAX_NODES (the field has a block of size 0, the stored order of all its cells, every node -1, costs NaN); FCPP_EINVAL when
 *     `stored` is not finite (a non-finite pose, w, E or X, or a stored_node outside its cell, which makes it NaN): nothing is improved,
 *     the order is the stored one, the nodes the stored ones (0 for one outside its cell), cost = stored, joint_length NaN.  The other
 *     fields are unaffected.  k = 0: an empty tour of cost 0.  k = 1: the cheapest node under E + w + X.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, radius <= 0 or not finite, mode not 0
 * or 1, n_starts outside 1 .. 64, min_gain negative or not finite, max_sweeps < 0 or > 2^20; FCPP_ESIZE -- negative sizes, offsets that
 * do not start at 0, decrease or do not end at their total, d_offsets that are not the blocks of the two offset tables.  The offsets are
 * checked on the host: pass the host copies or NULL to have them read back.  Both entries synchronise; nothing is kept in the context. */
#define FCPP_TOUR_MAX_CELLS 32
#define FCPP_TOUR_MAX_CELL_NODES 64
#define FCPP_TOUR_MAX_NODES 1024
/* D_dev (d_total = d_offsets[n] float64): every field's joint block from its variants' poses (n_vars each). */
int fcpp_cell_tour_transit(fcpp_ctx *ctx, int64_t n, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host, int64_t n_cells,
                           const int64_t *var_offsets_dev, const int64_t *var_offsets_host, int64_t n_vars, const double *ix_dev,
                           const double *iy_dev, const double *ih_dev, const double *ox_dev, const double *oy_dev, const double *oh_dev,
                           double radius, int mode, const int64_t *d_offsets_dev, const int64_t *d_offsets_host, int64_t d_total, double *D_dev);
/* w_dev: n_vars float64; stored_node_dev: n_cells int32 or NULL.  order_dev, node_dev: n_cells int32; cost_dev, stored_dev, joint_length_dev
 * (float64), winner_dev, sweeps_dev, skipped_dev, status_dev (int32): n each; tours_dev: n_starts x n_cells int32, candidate-major, every
 * candidate's final order laid out like order_dev; costs_dev: n x n_starts float64.  Any output may be NULL. */
int fcpp_cell_tour_solve(fcpp_ctx *ctx, int64_t n, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host, int64_t n_cells,
                         const int64_t *var_offsets_dev, const int64_t *var_offsets_host, int64_t n_vars, const double *w_dev,
                         const int32_t *stored_node_dev, const int64_t *d_offsets_dev, const int64_t *d_offsets_host, int64_t d_total,
                         const double *D_dev, const double *E_dev, const double *X_dev, int n_starts, double min_gain, int max_sweeps,
                         int32_t *order_dev, int32_t *node_dev, double *cost_dev, double *stored_dev, double *joint_length_dev,
                         int32_t *winner_dev, int32_t *sweeps_dev, int32_t *skipped_dev, int32_t *status_dev, int32_t *tours_dev,
                         double *costs_dev);

/* ---- service trips: a routed field split into capacity-limited round trips to a service point ------------------------------------------------
 * Build-defined (the reference knows no capacity).  A sprayer runs empty, a harvester runs full: after so many metres of work the vehicle
 * drives to a service point and comes back.  Given the router's candidate tours of a field, the operator decides after which swaths to
 * leave so that no trip works more than the capacity and the added driving is least -- the split of a "giant tour", an exact dynamic
 * programme per tour -- over every candidate in both driving directions, and keeps the cheapest.  Standalone; it reads what
 * fcpp_route_transit (or its _clear / _priced forms) and fcpp_route_solve wrote.  Path planning inside ONE field.
 * THE RULE (csrc/fcpp_tripfn.h, one set of expressions for host and device: the same bits on both).
 *   - Field i has m swaths and N = 2 m oriented swaths p = 2 s + d as in the router's rule; T is its N x N transit block, at t_offsets[i].
 *   - E, X, In, Out: 2 n_total float64 each in the layout of the router's E / X, field i's N values at 2 swath_offsets[i].  In[q]: the
 *     connector length from the service pose to the start of q; Out[p]: from the end of p to the service pose; E / X: the first trip's way
 *     in and the last trip's way out, NULL = zeros.  In and Out must not be NULL.
 *   - tours: n_cand candidate tours, 1 <= n_cand <= 64, candidate-major n_cand x n_total int32 as fcpp_route_solve writes tours_dev.
 *   - Per field a capacity Q and an optional first capacity Q0 (first_capacity NULL = Q), in metres of work (summed swath length: length,
 *     n_total float64); stop_cost >= 0: a price per stop, in metres.
 *   - Variants v = 2 c + r: r = 0 the tour t = tours[c]; r = 1 the same tour driven backwards, t[k] = tours[c][m - 1 - k] ^ 1.  With
 *     both_ways = 0 only r = 0 exists; the cost row still has 2 n_cand slots, the odd ones NaN.
 *   - Tables of a variant, all added left to right: w_k = length[t[k] >> 1]; P[0] = 0, P[k + 1] = fl(P[k] + w_k); base = E[t[0]] +
 *     T[t[0]][t[1]] + .. + T[t[m - 2]][t[m - 1]] + X[t[m - 1]], the router's own cost expression; for 1 <= j <= m - 1 a stop between the
 *     positions j - 1 and j costs d_j = plus(fl(fl(Out[t[j - 1]] + In[t[j]]) - T[t[j - 1]][t[j]]), stop_cost), plus(a, b) = fl(a + b) where
 *     that is below +inf, else +inf (NaN included).
 *   - A trip over the positions i .. j - 1 is feasible iff j == i + 1 or fl(P[j] - P[i]) <= cap_i, cap_0 = Q0, cap_i = Q otherwise.  A swath
 *     longer than the capacity is therefore a trip of its own, counted in `overfull`: the vehicle refills mid-swath, which this operator
 *     does not plan.  No field is infeasible.
 *   - The programme: g[0] = 0; g[j] = plus(d_j, min over feasible i < j of g[i]) for j = 1 .. m - 1, the minimum over the pair (g[i], i) in
 *     lexicographic order (ties to the lowest i), pred[j] that i; extra = min over i with (i, m) feasible of g[i], the same order; total =
 *     plus(base, extra).  Rounded addition is monotone, so this is the minimum over all stop sets of the left-to-right rounded sum.
 *   - Per field the winner is the variant of least total, ties to the lowest v; its trip starts come from backtracking pred from the final
 *     pick.  tour: the winner's oriented swaths in driving order; trip: per tour position the trip index within the field, from 0, never
 *     decreasing; n_trips; overfull: the trips whose work exceeds their cap; winner = v; cost = total, base, extra; costs: every variant's
 *     total.  m = 0: no trip, cost 0.  m = 1: one trip.  A capacity of +inf is valid: one trip, as long as no d_j is negative --
 *     connector lengths obey the triangle inequality; a caller's table in which a stop PAYS gets that stop.
 *   - Status, int32: 0; FCPP_EUNSUPPORTED for m > FCPP_ROUTE_MAX_SWATHS (the field has no block); FCPP_EINVAL for a candidate tour that is no
 *     permutation of the field's swaths, a length that is negative or not finite, a capacity that is NaN or <= 0, candidate 0's base not
 *     finite.  For both the field gets tour = candidate 0 as given, trip all 0, n_trips = min(m, 1), overfull 0, winner 0 and NaN costs.
 *     The other fields are unaffected.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or input, n_cand outside 1 .. 64, stop_cost negative or not
 * finite, both_ways not 0 or 1; FCPP_ESIZE -- sizes or offsets inconsistent in the ways fcpp_route_solve checks them.  The entry synchronises
 * like fcpp_route_solve and keeps nothing in the context; it may be called per chunk of fields.
 * tour_dev, trip_dev: n_total int32; n_trips_dev, overfull_dev, winner_dev, status_dev (int32), cost_dev, base_dev, extra_dev (float64): n
 * each; costs_dev: n x 2 n_cand float64.  Any output may be NULL. */
int fcpp_trip_solve(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                    const int64_t *t_offsets_dev, const int64_t *t_offsets_host, int64_t t_total, const double *T_dev, const double *length_dev,
                    const double *E_dev, const double *X_dev, const double *In_dev, const double *Out_dev, int n_cand, const int32_t *tours_dev,
                    int both_ways, const double *capacity_dev, const double *first_capacity_dev, double stop_cost, int32_t *tour_dev,
                    int32_t *trip_dev, int32_t *n_trips_dev, int32_t *overfull_dev, int32_t *winner_dev, int32_t *status_dev, double *cost_dev,
                    double *base_dev, double *extra_dev, double *costs_dev);

/* ---- vehicle shares: a routed field divided among K vehicles of one depot, least makespan ---------------------------------------------------
 * Build-defined.  Given the router's candidate tours of a field, the operator decides which contiguous stretch of which tour each of at
 * most K vehicles drives, from the depot and back, so that the vehicle that finishes last finishes as early as possible -- and, among the
 * splits that are as balanced as that, the one of least summed cost.  Two exact dynamic programmes per tour, over every candidate in both
 * driving directions.  Standalone; it reads what fcpp_route_transit (or its _clear / _priced forms) and fcpp_route_solve wrote.  Path
 * planning inside ONE field: one depot, one speed and one width for all vehicles.
 * THE RULE (csrc/fcpp_fleetfn.h, one set of expressions for host and device: the same bits on both).
 *   - Field i has m swaths and N = 2 m oriented swaths p = 2 s + d as in the router's rule; T is its N x N transit block, at t_offsets[i].
 *   - In, Out: 2 n_total float64 each in the layout of the router's E / X, field i's N values at 2 swath_offsets[i].  In[q]: the connector
 *     length from the depot pose to the start of q; Out[p]: from the end of p to the depot.  Neither may be NULL.
 *   - tours: n_cand candidate tours, 1 <= n_cand <= 64, candidate-major n_cand x n_total int32 as fcpp_route_solve writes tours_dev.
 *   - vehicles: K per field, int32, 1 <= K <= FCPP_FLEET_MAX_VEHICLES; length: n_total float64, the swaths' work in metres; work_weight
 *     (omega) >= 0 and finite: the weight of a metre of work against a metre of driving (transit speed / working speed), so that a
 *     share's cost is proportional to its time.
 *   - Variants v = 2 c + r, the service trips': r = 0 the tour t = tours[c]; r = 1 the same tour driven backwards, t[k] =
 *     tours[c][m - 1 - k] ^ 1.  With both_ways = 0 only r = 0 exists; the value rows still have 2 n_cand slots, the odd ones NaN.
 *   - Tables of a variant: P[0] = 0, P[k + 1] = fl(P[k] + length[t[k] >> 1]); S[0] = 0, S[k] = fl(S[k - 1] + T[t[k - 1]][t[k]]) for k = 1 ..
 *     m - 1.
 *   - A share, the positions i .. j - 1 (0 <= i < j <= m) driven by one vehicle from the depot and back, costs c(i, j) =
 *     plus(fl(fl(In[t[i]] + fl(S[j - 1] - S[i])) + Out[t[j - 1]]), fl(omega * fl(P[j] - P[i]))), plus(a, b) = fl(a + b) where that is below
 *     +inf, else +inf (NaN included): c is never NaN.
 *   - Stage 1, the makespan: G_1[j] = c(0, j); G_k[j] = min over k - 1 <= i < j of max(G_(k-1)[i], c(i, j)) for k <= j; M = min over 1 <= k <=
 *     min(K, m) of G_k[m].  max and min do not round, so M is the exact least, over every split of the tour into AT MOST K non-empty
 *     contiguous shares, of the largest share cost.  A further vehicle adds its own In and Out and can make things worse: it stays home.
 *   - Stage 2, the cheapest among the balanced: H_0[0] = 0; H_k[j] = min over the starts i for which H_(k-1)[i] exists and c(i, j) <= M of
 *     plus(c(i, j), H_(k-1)[i]), the pair (value, i) in lexicographic order (ties to the lowest i), pred_k[j] that i; H_k[j] exists iff such
 *     an i does.  The variant's sum is the least (H_k[m], k) over the k <= min(K, m) for which it exists; one does, since M is attained.
 *     Rounded addition is monotone, so this is the least left-to-right rounded sum of share costs over all splits with every share <= M.
 *   - Per field the winner is the variant of least (M, sum, v), lexicographically; its shares come from backtracking pred.  tour: the
 *     winner's oriented swaths in driving order; share: per tour position the vehicle index, from 0, never decreasing; n_used: the shares
 *     used, <= min(K, m); winner = v; makespan = M, total = sum; makespans, totals: every variant's M and sum; share_first: a share's first
 *     position, -1 beyond n_used; share_cost: c of every share, NaN beyond n_used.  k_stride, max K <= k_stride <= 16, is the row length
 *     of share_first and share_cost.  m = 0: no share, makespan 0, total 0.
 *   - Status, int32: 0; FCPP_EUNSUPPORTED for m > FCPP_ROUTE_MAX_SWATHS (the field has no block) or K > FCPP_FLEET_MAX_VEHICLES;
 *     FCPP_EINVAL for K < 1 or K > k_stride, a candidate tour that is no permutation of the field's swaths, a length that is negative or not
 *     finite, candidate 0's S[m - 1] not finite.  For both the field is written as fcpp_trip_solve writes a failed one: tour = candidate 0
 *     as given, share all 0, n_used = min(m, 1), winner 0, share_first 0 for that one share, and every cost NaN.  The other fields are
 *     unaffected.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or input, n_cand outside 1 .. 64, k_stride outside 1 .. 16,
 * work_weight negative or not finite, both_ways not 0 or 1; FCPP_ESIZE -- sizes or offsets inconsistent in the ways fcpp_route_solve checks
 * them.  The entry synchronises like fcpp_route_solve and keeps nothing in the context; it may be called per chunk of fields.
 * tour_dev, share_dev: n_total int32; n_used_dev, winner_dev, status_dev (int32), makespan_dev, total_dev (float64): n each; makespans_dev,
 * totals_dev: n x 2 n_cand float64; share_first_dev (int32), share_cost_dev (float64): n x k_stride.  Any output may be NULL. */
#define FCPP_FLEET_MAX_VEHICLES 16
int fcpp_fleet_solve(fcpp_ctx *ctx, int64_t n, const int64_t *swath_offsets_dev, const int64_t *swath_offsets_host, int64_t n_total,
                     const int64_t *t_offsets_dev, const int64_t *t_offsets_host, int64_t t_total, const double *T_dev, const double *length_dev,
                     const double *In_dev, const double *Out_dev, int n_cand, const int32_t *tours_dev, int both_ways,
                     const int32_t *vehicles_dev, int k_stride, double work_weight, int32_t *tour_dev, int32_t *share_dev, int32_t *n_used_dev,
                     int32_t *winner_dev, int32_t *status_dev, double *makespan_dev, double *total_dev, double *makespans_dev,
                     double *totals_dev, int32_t *share_first_dev, double *share_cost_dev);

/* ---- headland paths: every ring of an inset as ONE sampled, closed, drivable path ------------------------------------------------------------
 * Build-defined.  The rings fcpp_inset_fill writes are bare polygons: straight offset pieces that meet in sharp convex corners, and chords
 * of arcs of radius d around reflex vertices.  This operator turns every ring of a batch (all fields, all passes) into a loop a vehicle of
 * turning radius `radius` can drive: the straight pieces driven to their very ends, the arcs followed where d >= radius and bridged where
 * not, every sharp joint closed by a Dubins (mode 0) or Reeds-Shepp (mode 1) connector -- at a corner, where both poses share one
 * position, the bulb turn or the three-point turn.  A counts entry and a fill entry over all rings; the result is a path set in CSR form
 * (path_offsets), which fcpp_curvature, fcpp_speed_plan, fcpp_validate and fcpp_trajectory take as it is.  Standalone: nothing here feeds
 * fcpp_batch_plan.  Connectors know no boundary, as everywhere: fcpp_validate flags what leaves the field, and the connector clearance above
 * tests them exactly (fcpp_conn_clear on the legs' poses).
 * Input: n_rings rings, ring r owning the vertices ring_offsets[r] .. ring_offsets[r + 1] of x, y (float64) and src (int32: even for a
 * vertex that starts a straight piece, odd for a vertex on an arc, equal along one arc -- fcpp_inset_fill's out_src), closed implicitly,
 * the kept area on the left; ring_dist (n_rings float64): the inset distance d of the ring's (field, distance) pair.
 * THE RULE (csrc/fcpp_hpathfn.h, one set of expressions for host and device: the same bits on both), per ring of m vertices v_0 .. v_(m-1):
 *   - Driving order.  direction +1: driven vertex k is v_k and its chord's source s_k = src[k].  direction -1: driven vertex k is
 *     v_((m - k) mod m) and s_k = src[m - 1 - k].  Both start at v_0.  Driven vertex k owns slot 2 k (an element) and slot 2 k + 1 (the joint
 *     behind it); ring r's first slot is 2 ring_offsets[r].  leg_offsets (2 n_verts + 1 int64) holds the first sample of every slot;
 *     path_offsets (n_rings + 1) is leg_offsets at the rings' first slots.
 *   - Elements.  Driven vertex k starts an element iff k = 0, or s_k is even, or s_k != s_(k-1); the element runs from A = its start vertex
 *     to B = the next element start, cyclically (the last one ends at v_0).  The arc vertices between only mark the run: they are not
 *     sampled.  With c = |AB| and h_c the chord's heading: s even is a STRAIGHT element of length c and heading h_c; s odd an ARC element of
 *     radius d: h = sqrt(max(d^2 - c^2 / 4, 0)), half = atan2(c / 2, h), sweep D = 2 half, length d D.  As stored the arc turns right, curvature
 *     -1 / d, heading h_c + half at A and h_c - half at B, centre = midpoint + h (u_y, -u_x) with u = (B - A) / c; direction -1 mirrors it: a
 *     left turn, curvature +1 / d.  An arc is DRIVABLE iff d >= radius; a straight element with c > 0 always.  An element with c = 0 and an
 *     undrivable arc have no leg: they are skipped.
 *   - Element leg (slot 2 k).  Straight: sampled as a swath of the field paths -- floor(c / spacing) + 1 samples, one more at the end when
 *     the last lies before it, sample j at t = fmin((j spacing) / c, 1), the LAST sample B itself; curvature 0, gear +1, part 0.  Followed
 *     arc: as many samples by the same count rule on d D, sample j at arc length s = j spacing: centre + d (cos, sin) of the start angle -/+ s / d,
 *     heading likewise; the FIRST sample is A itself, the LAST B itself; curvature -/+ 1 / d, gear +1, part 4.
 *   - Joint leg (slot 2 k + 1), of a drivable element e only.  f = the next drivable element in driving order, cyclically (e itself when
 *     it is the only one).  If f directly follows e and |wrap(heading_in(f) - heading_out(e))| <= smooth_tol there is no leg: the loop
 *     drives straight through.  Otherwise -- a sharp corner, or a joint across skipped elements -- the leg is fcpp_dubins_solve's (mode 0)
 *     or fcpp_rs_solve's (mode 1) path at `radius` from e's exit pose to f's entry pose, sampled exactly as fcpp_dubins_sample /
 *     fcpp_rs_sample sample it; part 1.  Its end lies within 2^-43 (radius + straight) metres of f's start (the connectors' bound).
 *   - Junctions stay doubled, as in the field paths.  The loop is closed: the last sample's pose is the first sample's (to that bound).
 *   - leg (int32): the sample's slot within its ring.  Every sample is evaluated from its leg alone, never from a neighbouring sample.
 *   - Totals per ring, added in slot order: work_length = straight elements + followed arcs; transit_length = connectors; skipped_length =
 *     d D of the undrivable arcs (the centre line that was bridged, not driven).
 * Status per ring, int32: 0; FCPP_EINVAL -- fewer than 2 vertices, a vertex or distance that is not finite, an arc with d <= 0, a negative
 * src, a connector without a path (word -1): no samples, NaN totals; FCPP_EUNSUPPORTED -- no drivable element: no samples (work and
 * transit 0, skipped as summed).  The other rings are unaffected.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, radius or spacing <= 0 or not finite,
 * mode not 0 or 1, direction not +1 or -1, smooth_tol negative (or NaN); FCPP_ESIZE -- negative sizes, more than 2^30 vertices, offsets
 * that do not start at 0, decrease or do not end at n_verts.  FCPP_ESIZE after the count: a leg of 2^31 samples or more, a ring above
 * 2^31 - 2 samples.  ring_offsets_host: the host copy, or NULL to have it read back.  Both entries synchronise.
 * fcpp_headland_path_fill recomputes the leg records from the same inputs (nothing is kept in the context between the two calls); every
 * one of its seven outputs may be NULL, as may work_length, transit_length, skipped_length, status and path_offsets_host of the counts. */
int fcpp_headland_path_counts(fcpp_ctx *ctx, int64_t n_rings, const int64_t *ring_offsets_dev, const int64_t *ring_offsets_host, int64_t n_verts,
                              const double *x_dev, const double *y_dev, const int32_t *src_dev, const double *ring_dist_dev, double radius,
                              int mode, double spacing, int direction, double smooth_tol, int64_t *path_offsets_dev,
                              int64_t *path_offsets_host, int64_t *leg_offsets_dev, double *work_length_dev, double *transit_length_dev,
                              double *skipped_length_dev, int32_t *status_dev);
int fcpp_headland_path_fill(fcpp_ctx *ctx, int64_t n_rings, const int64_t *ring_offsets_dev, const int64_t *ring_offsets_host, int64_t n_verts,
                            const double *x_dev, const double *y_dev, const int32_t *src_dev, const double *ring_dist_dev, double radius,
                            int mode, double spacing, int direction, double smooth_tol, const int64_t *leg_offsets_dev,
                            int64_t total_samples, double *out_x_dev, double *out_y_dev, double *heading_dev, double *kappa_dev,
                            int8_t *part_dev, int8_t *gear_dev, int32_t *leg_dev);

/* ---- polygon coverage: what a sampled path set covers of fields given as rings -------------------------------------------------------------
 * Build-defined.  The last stage of the polygon chain: per field, on a grid of cells, the area inside the SURVEYED boundary, the part of it
 * the working passes cover, the part two different passes cover (double application), and what they cover outside the boundary or inside a
 * hole.  fcpp_cover_grid answers this for quads (four half-planes, one polyline, a host array of jobs, every tile culling every segment);
 * this operator takes rings with holes, a whole path set with a work mask and pass ids, and keeps a tile's work independent of its field's
 * sample count.  Standalone: nothing here feeds fcpp_batch_plan.
 * THE RULE (csrc/fcpp_pcoverfn.h, one set of expressions for host and device: the same bits on both).
 *   - Fields.  The two-level CSR of the swath operators (ring_offsets, vert_offsets, x, y), even-odd interior.
 *   - Grid of field i.  r = width / 2, m = ceil(r / res) margin cells; gx = x_min - m res, gy = y_min - m res;
 *     nx = ceil((x_max - x_min) / res) + 2 m, ny likewise; cell (a, b) is sampled at (gx + ((double)a + 0.5) res, gy + ((double)b + 0.5) res):
 *     fcpp_cover_grid's expression with ox = gx, oy = gy, shift = 0.5.  A failed field has an empty grid and zero counts, its paths are
 *     ignored; the other fields are unaffected.
 *   - Inside.  A cell is inside iff an odd number of edges cross its row at u < X -- the half-open crossing rule of the swaths in the frame
 *     theta = 0: an edge (p, q) crosses row Y iff (y_p <= Y) != (y_q <= Y), at u = x_p + (Y - y_p) / (y_q - y_p) (x_q - x_p).
 *   - Paths.  One sampled path set in the CSR form every path operator emits (path_offsets, x, y).  Field i owns the paths
 *     path_ids[field_path_offsets[i] .. field_path_offsets[i + 1]) (int64; path_ids NULL: the identity).  work (uint8 per sample, NULL: all
 *     samples work), pass (int32 per sample, NULL: the path's index).
 *   - Working segments.  Segment (k, k + 1) of a path works iff both samples work and both are finite; its pass is pass[k].  An end of a
 *     working segment is a JOINT iff the neighbouring segment of the same path on that side also works.
 *   - Covered.  With a -> b the segment, p the cell, dot = (p - a).(b - a), len2 = |b - a|^2, cross = (b - a) x (p - a), strictly:
 *         0 < dot < len2 : cross^2 < r^2 len2
 *         dot <= 0       : a joint: |p - a|^2 < r^2;  a flat end: dot == 0 and cross^2 < r^2 len2
 *         dot >= len2    : a joint: |p - b|^2 < r^2;  a flat end: dot == len2 and cross^2 < r^2 len2
 *     so a run of working segments sweeps a rectangle with rounded interior joints, as an implement does.  caps = 1 makes every end round:
 *     the predicate is then bit for bit fcpp_cover_grid's with strict = 1.
 *   - Overlapped.  A cell is overlapped iff working segments of at least two different pass ids cover it.
 *   - counts (int64, 4 per field, zeroed by the call): cells inside; inside and covered; inside and overlapped; covered and not inside
 *     (spill, within the grid).  grid (optional): one byte per cell, row-major [b][a], field i's at cell_offsets[i]: bit 0 inside, bit 1
 *     covered, bit 2 overlapped.
 * Status per field, int32: 0; FCPP_EINVAL -- no ring, a ring with fewer than 3 vertices, a vertex that is not finite; FCPP_EUNSUPPORTED --
 * more than 2^28 cells.
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, width or res <= 0 or not finite, caps not
 * 0 or 1, a path id outside [0, n_paths); FCPP_ESIZE -- negative sizes, offsets that do not start at 0, decrease or do not end at their
 * total, cell offsets that do not end at these fields' cells, 2^31 tiles or chunks of 256 segments or more.
 * fcpp_polygon_cover_sizes: dims_dev -- n records of 32 bytes (gx, gy as float64; nx, ny as int64); cell_offsets_dev (n + 1 int64), its copy
 * to cell_offsets_host (or NULL); status_dev (or NULL).  fcpp_polygon_cover recomputes the grids from the same inputs (nothing is kept in the
 * context between the two calls); path_offsets_host and cell_offsets_host: the host copies, or NULL to have what is needed read back;
 * work_dev, pass_dev, path_ids_dev, grid_dev and status_dev may be NULL (cell_offsets too when grid_dev is).  Inputs are never written,
 * outputs exactly over their extent, natural alignment suffices.  Both entries synchronise. */
int fcpp_polygon_cover_sizes(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev,
                             int64_t n_verts, const double *x_dev, const double *y_dev, double width, double res, void *dims_dev,
                             int64_t *cell_offsets_dev, int64_t *cell_offsets_host, int32_t *status_dev);
int fcpp_polygon_cover(fcpp_ctx *ctx, int64_t n, const int64_t *ring_offsets_dev, int64_t n_rings, const int64_t *vert_offsets_dev, int64_t n_verts,
                       const double *x_dev, const double *y_dev, double width, double res, int caps, int64_t n_paths,
                       const int64_t *path_offsets_dev, const int64_t *path_offsets_host, int64_t total_points, const double *px_dev,
                       const double *py_dev, const uint8_t *work_dev, const int32_t *pass_dev, const int64_t *field_path_offsets_dev,
                       const int64_t *path_ids_dev, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host, uint8_t *grid_dev,
                       int64_t *counts_dev, int32_t *status_dev);

/* ---- coverage regions: the missed, overlapped, spilled or covered patches of the coverage grids ------------------------------------------------
 * Build-defined.  fcpp_polygon_cover says how much of a field a plan misses; this operator says WHERE that ground lies and in how many
 * patches: connected-component labelling of a batch of byte grids, on the device, where the grids are.  Standalone: nothing here feeds
 * fcpp_batch_plan.
 * THE RULE (csrc/fcpp_regionfn.h, one set of expressions for host and device; all integers: the same values on both, whatever the order).
 *   - Input.  The grids exactly as fcpp_polygon_cover writes them: dims (n records of 32 bytes: gx, gy as float64; nx, ny as int64),
 *     cell_offsets (n + 1 int64), one byte per cell, row-major [b][a].  A field with an empty grid (a failed field) has no regions; its
 *     neighbours are unaffected.
 *   - Members.  Cell c is a member iff (grid[c] & mask) == value, mask and value in 0 .. 255.  The named kinds: missed (mask 3, value 1:
 *     inside and not covered), overlapped (4, 4), spill (3, 2: covered and not inside), covered (3, 3).
 *   - Neighbours.  connectivity 4: W, E, N, S; 8: plus the four diagonals.  Neighbours exist only inside ONE field's nx x ny grid: cell
 *     (nx - 1, b) and cell (0, b + 1) are not neighbours, nor are the last row of field i and the first row of field i + 1.
 *   - Regions.  A region is a maximal connected set of members.  Its KEY is the smallest field-local cell index b nx + a among its cells;
 *     the regions of a field are numbered 0, 1, .. in ascending key.  Numbering, records and labels are a function of the input alone.
 *   - Record, 48 bytes per region, region k of field i at region_offsets[i] + k: first (int64: the key), cells (int64), a_min, a_max,
 *     b_min, b_max (int32: the bounding box in cells), sum_a, sum_b (int64: the sums of the members' column and row indices; a field has
 *     at most 2^28 cells, so every sum stays below 2^56).  The centroid is gx + (sum_a / cells + 0.5) res, likewise in y.  Integer atomics
 *     only (add, min, max): order-independent.  Out of scope: second moments (they can overflow int64 on a thin grid), orientation, the
 *     outline of a region.
 *   - Labels, int32 per cell, the caller's array, which lives across the two calls (nothing is kept in the context): after
 *     fcpp_cover_regions_counts a member holds its region's key, after fcpp_cover_regions_fill its region's index within its field; a
 *     non-member holds -1 after both.
 * fcpp_cover_regions_counts labels every cell, resolves the keys and writes the regions' CSR offsets (region_offsets_dev, n + 1; its copy
 * to region_offsets_host, or NULL).  fcpp_cover_regions_fill writes the records (n_regions = region_offsets[n]; it zeroes them itself) and
 * rewrites labels from keys to indices; it takes the labels and offsets of the counts call on the same grids.  cell_offsets_host,
 * region_offsets_host of the fill: the host copies, or NULL to have them read back (the kernels read the device arrays either way).
 * Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, mask or value outside 0 .. 255,
 * value & ~mask non-zero, connectivity not 4 or 8; FCPP_ESIZE -- negative sizes, cell or region offsets that do not start at 0 or
 * decrease, cell offsets that disagree with dims (nx ny against their differences), a grid of more than 2^28 cells, an n_regions that
 * is not the region offsets' total, 2^31 tiles or more.  Inputs are never written, outputs exactly over their extent, natural alignment
 * suffices.  Both entries synchronise. */
int fcpp_cover_regions_counts(fcpp_ctx *ctx, int64_t n, const void *dims_dev, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host,
                              const uint8_t *grid_dev, int mask, int value, int connectivity, int32_t *labels_dev, int64_t *region_offsets_dev,
                              int64_t *region_offsets_host);
int fcpp_cover_regions_fill(fcpp_ctx *ctx, int64_t n, const void *dims_dev, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host,
                            int32_t *labels_dev, const int64_t *region_offsets_dev, const int64_t *region_offsets_host, int64_t n_regions,
                            void *records_dev);

/* ---- patch passes: swaths over the member cells of coverage regions ------------------------------------------------------------------------------
 * Build-defined.  fcpp_cover_regions_fill says where the missed ground lies; this operator lays straight working passes over it, parallel
 * to the field's tracks, on the device, where the grids and labels are.  The passes come out as swath records (the SoA of fcpp_swath_fill
 * plus the region of every swath), so the router, the field paths and a second fcpp_polygon_cover take them.  Standalone.
 * THE RULE (csrc/fcpp_patchfn.h, one set of expressions for host and device).
 *   - Input.  The grids as fcpp_polygon_cover writes them: dims, cell_offsets and res.  labels, int32 per cell: a value >= 0 is the
 *     cell's region index within its field, any negative value means not a member (-1 / -2 both).  region_offsets (n + 1), one track
 *     angle theta per field (finite, |theta| <= 1e5), width W, margin m (0 <= m, We = W - 2 m > 0), join j >= 0.
 *   - Frame.  (s, c) = fc_sincos(theta), written per field to frame (n x 2 float64: s, c).  Cell (a, b) has the grid-local centre
 *     x = ((double)a + 0.5) res, y = ((double)b + 0.5) res; u = x c + y s runs along the tracks, w = -x s + y c across them.  The grid
 *     origin (gx, gy) is added only at the output.
 *   - Extent, per region: u_min, u_max, w_min, w_max over its members; exact min / max, so the order of work does not show.
 *   - Lines.  K = floor((w_max - w_min) / We) + 1, w_lo = w_min - (fl(K We) - (w_max - w_min)) / 2; line k lies at
 *     w_k = w_lo + ((double)k + 0.5) We; a member belongs to line clamp(floor((w - w_lo) / We), 0, K - 1).
 *   - Bins along a line.  h = res, B = floor((u_max - u_min) / h) + 1; a member falls in bin clamp(floor((u - u_min) / h), 0, B - 1).
 *     Bit (region, k, q) is set iff some member falls there: line k of a region is ceil(B / 64) words of 64 bits at
 *     first_word + k ceil(B / 64), bin q bit q mod 64 of word q / 64.  Everything after the two floors is integer work.
 *   - Runs.  J = floor(j / h).  On a line a set bin q starts a run iff none of the bins q - J - 1 .. q - 1 is set; a run ends at the last
 *     set bin before the next start, or at the line's last set bin.
 *   - Swath of a run q0 .. q1 on line k: u_a = u_min + (double)q0 h - m, u_b = u_min + (double)(q1 + 1) h + m, the end points
 *     (u c - w_k s + gx, u s + w_k c + gy), length u_b - u_a; a is the end with the smaller u.  Within a field the swaths are ordered by
 *     region, then k, then u; `line` is the number of lines of the field's earlier regions plus k, `region` the global region index.
 *   - Record, 64 bytes per region: u_min, w_lo (float64), K, B, first_line, first_word (int64: the lines / words of all earlier regions
 *     of the call), status (int32), 0 (int32), u_max (float64).  status FCPP_EUNSUPPORTED for K > 2^22 or K ceil(B / 64) >= 2^31: K = B = 0,
 *     no swaths.  A region whose label never occurs has no members, no lines and status 0.
 *   - Guarantees: every member lies within We / 2 across its line and at least m inside a swath's ends along it (to 1e-9 m, the rounding
 *     of w_k and u_a); with m = res / 2 the whole cell square is covered at theta = 0.
 * Memory is the caller's, nothing is kept in the context.  fcpp_patch_sizes writes frame, the records and to totals_host[0 .. 1] the
 * lines and 64-bit bitmap words of the call.  fcpp_patch_counts takes the caller's bitmap (n_words) and line_counts (n_lines int64), zeroed
 * or not: it zeroes them, marks, counts the runs of every line and writes line_offsets (n_lines + 1: the swaths before every line) and
 * swath_offsets (n + 1: the swaths before every field; its copy to swath_offsets_host, or NULL).  fcpp_patch_fill writes the n_swaths =
 * line_offsets[n_lines] swath records, every element exactly once.  cell_offsets_host, region_offsets_host: the host copies, or NULL to
 * have them read back.  Errors of the CALL, found before any kernel runs: FCPP_EINVAL -- a NULL handle or required array, res or W not
 * positive, m < 0, W - 2 m <= 0, j < 0, any of them or an angle not finite, |theta| > 1e5; FCPP_ESIZE -- negative sizes, offsets that do
 * not start at 0 or decrease, cell offsets that disagree with dims, a grid of more than 2^28 cells, an n_regions or n_swaths that is not
 * its offsets' total.  Inputs are never written, outputs exactly over their extent, natural alignment suffices.  All three synchronise. */
int fcpp_patch_sizes(fcpp_ctx *ctx, int64_t n, const void *dims_dev, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host, double res,
                     const int32_t *labels_dev, const int64_t *region_offsets_dev, const int64_t *region_offsets_host, int64_t n_regions,
                     const double *angle_dev, double width, double margin, double join, double *frame_dev, void *records_dev,
                     int64_t *totals_host);
int fcpp_patch_counts(fcpp_ctx *ctx, int64_t n, const void *dims_dev, const int64_t *cell_offsets_dev, const int64_t *cell_offsets_host, double res,
                      const int32_t *labels_dev, const int64_t *region_offsets_dev, const int64_t *region_offsets_host, int64_t n_regions,
                      const double *frame_dev, double width, double margin, double join, const void *records_dev, int64_t n_lines,
                      int64_t n_words, uint64_t *bitmap_dev, int64_t *line_counts_dev, int64_t *line_offsets_dev, int64_t *swath_offsets_dev,
                      int64_t *swath_offsets_host);
int fcpp_patch_fill(fcpp_ctx *ctx, int64_t n, const void *dims_dev, double res, const int64_t *region_offsets_dev,
                    const int64_t *region_offsets_host, int64_t n_regions, const double *frame_dev, double width, double margin, double join,
                    const void *records_dev, int64_t n_lines, int64_t n_words, const uint64_t *bitmap_dev, const int64_t *line_offsets_dev,
                    int64_t n_swaths, double *ax_dev, double *ay_dev, double *bx_dev, double *by_dev, int32_t *line_dev, double *length_dev,
                    int64_t *region_dev);

/* ---- coverage rasterisation -------------------------------------------------
 * Replaces the Shapely calls of verify_corner_coverage_grid_based (MLP:1426-1509: `LineString(path).buffer(W/2)
 * .contains(Point)` per 0.1 m grid cell of a 2R x 2R corner square, first for the turn, then for the reverse fill on
 * the cells still open) and of _calculate_coverage_rate (MLP:1357-1371: area(path.buffer(W/2) & area) / area(area)),
 * by one sampled operator: a job is a regular grid of sample points, a polyline A and an optional polyline B (stored
 * right after A in px/py).  A sample is covered by a polyline iff its distance to one of the polyline's segments
 * (consecutive point pairs, jumps included -- as in LineString(path)) is < radius (strict = 1, Shapely's `contains`)
 * or <= radius (strict = 0).  The distance test is division-free and the same in the oracle and on the GPU: with
 * a -> b the segment, p the sample, dot = (p-a).(b-a), len2 = |b-a|^2:
 *     dot <= 0     : |p-a|^2              < radius^2
 *     dot >= len2  : |p-b|^2              < radius^2
 *     otherwise    : ((b-a) x (p-a))^2    < radius^2 * len2
 * B is only evaluated on samples A left open (MLP:1489-1497).  counts (3 per job): samples in the region, of those
 * covered by A, of those covered by A or B.  grid (optional): one byte per sample, row-major [j][i] like the
 * reference's grid[j, i] (MLP:1483), bit 0 = A, bit 1 = B (and not A); samples outside the region stay 0. */
typedef struct fcpp_cover_job {
    double ox, oy;        /* sample (i, j) lies at (ox + (i + shift) * res, oy + (j + shift) * res) */
    double res, shift;    /* MLP:1449, 1477-1478: res = 0.1, shift = 0 (cell corners); 0.5 = cell centres for area estimates */
    double radius;        /* W / 2 (MLP:1471, 1363) */
    int32_t nx, ny;       /* samples per row, rows */
    int32_t n_a, n_b;     /* points of polyline A and of polyline B (0 = none) */
    int64_t pts_first;    /* index of A's first point in px / py */
    int64_t grid_first;   /* offset of this job's nx * ny bytes in `grid`, or -1: counts only */
    int32_t strict;       /* 1: distance < radius, 0: distance <= radius */
    int32_t region;       /* 0: every sample counts; 1: samples inside `outer` and not inside `inner` */
    double outer[12];     /* 4 half-planes (a, b, c): inside <=> a*x + b*y + c >= 0 for all four */
    double inner[12];
} fcpp_cover_job;

/* jobs: host array; px, py: device (n_pts points, e.g. the x / y arrays of fcpp_batch_run); grid_dev may be NULL when no job
 * asks for it; counts_dev: 3 * n_jobs int64 (zeroed by the call).  Runs on the context's stream and synchronises it. */
int fcpp_cover_grid(fcpp_ctx *ctx, int64_t n_jobs, const fcpp_cover_job *jobs, int64_t n_pts, const double *px_dev,
                    const double *py_dev, uint8_t *grid_dev, int64_t *counts_dev);

/* ---- the final gather of a job sharded over the GPUs of a node ----------------------------------
 * Fields are independent: every rank plans a contiguous block of them (cut on fcpp_plan_points) with its own context and batch, and the
 * only exchange is this gather of the blocks' results on one rank.  For each of n_arrays arrays (elem_bytes[a] bytes per element: 8 for
 * x / y / kappa / v, 4 for flagseg, sizeof(fcpp_field_stats) for the statistics with counts in fields) rank r contributes counts_per_rank[r]
 * elements from send_dev[a]; the root receives them in rank order into recv_dev[a] (sum of the counts elements; NULL on the other ranks).
 * One ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the context's stream over the caller's communicator (`nccl_comm`: an
 * ncclComm_t of RCCL) -- point to point, every peer over its own xGMI link to the root, no ring and no staging copy; the root's own block
 * is a device-to-device copy (flags bit 0: it, too, goes through the communicator -- a one-GPU test of the RCCL path).  Asynchronous: the
 * arrays are complete when the stream is.  RCCL is looked up in the process at the first call, not linked: FCPP_EUNSUPPORTED without
 * it.  (The Python mirror gathers through torch.distributed instead -- sharding.py -- whose process group owns the communicator.) */
int fcpp_gather(fcpp_ctx *ctx, void *nccl_comm, int rank, int world, int root, int n_arrays, const void *const *send_dev, const int32_t *elem_bytes,
                const int64_t *counts_per_rank, void *const *recv_dev, int flags);

/* ---- diagnostics (tests/) -----------------------------------------------------------------------
 * The setup's transcendentals (csrc/fcpp_math.h: plain IEEE operations so that host and device agree bit for bit) evaluated on the host /
 * on the device: fn 0 = sin and cos of a -> out0, out1; 1 = atan2(a, b); 2 = acos(a); 3 = hypot(a, b) -> out0.  The _dev variant takes
 * device pointers and synchronises. */
int fcpp_debug_math(int fn, int64_t n, const double *a, const double *b, double *out0, double *out1);
int fcpp_debug_math_dev(fcpp_ctx *ctx, int fn, int64_t n, const double *a_dev, const double *b_dev, double *out0_dev, double *out1_dev);
/* The device setup's rule for a field's table offsets without a scan (csrc/fcpp_offsetfn.h: the exclusive prefix of a count column from the
 * per-block aggregates and the counts of the field's own block), its HOST version on host pointers: counts[col * n + i], n_cols columns of
 * n <= 8192 fields -> prefix[col * n + i] and totals[col].  What the kernels' offsets are checked against; a diagnostic, not a fallback. */
int fcpp_debug_offsets(int64_t n, int n_cols, const int64_t *counts, int64_t *prefix, int64_t *totals);
/* The decisions of a batch's device setup (csrc/fcpp_setuprule.h: the functions the setup itself reads), evaluated on the host, on host
 * pointers; booleans as 0 / 1.
 *   what 0, setup_accept: in = { setup mode, fields, small-batch threshold, obstacle mode, field_work, max_prims } -> out[0] = 0: accepted, or
 *           the decline: 1 host setup requested, 2 empty batch, 3 a handful of fields, 4 obstacle mode, 5 FCPP_FIELD_WORK=0, 6 too many primitives
 *   what 1, setup_begin: in = { fields, exact_only, dense, bytes of the capacity layout, outputs wanted, no polygons, fuse_spans, direct_ok,
 *           FCPP_DIRECT } -> out = { spec, direct, the capacity layout is looked at }
 *   what 2, setup_end: in = { spec, direct_step, early point total, PC_UNFUSABLE, PC_WORK_SPAN_PTS, PC_WORK, PC_POINTS, the flag PF_OVER_CAPACITY,
 *           generation, fields, fuse_spans, no polygons } -> out = { fuse, within, qualifies, taken, refill }
 *   what 3, a plan slot's two buffers of aggregates over a sequence of events: in = { k <= 4096, event 0 .. k-1 }; event 0: a speculative setup
 *           that settles, 1: one that never settles (a launch error), 2: the slot is allocated afresh -> out[2 i], out[2 i + 1] = what setup i
 *           does first: { clear both buffers, add into the second } (-1, -1 for event 2).  A diagnostic, not a fallback. */
int fcpp_debug_setup_rule(int what, const int64_t *in, int64_t *out);
/* What fcpp_ga_evolve will launch per generation for n_nodes and population_size on the context's device -- host code, the function its
 * launchers read; out (a HOST pointer) = { 1: one launch per generation (k_ga_generation), 0: two launches on two streams; pair workgroups;
 * base; extra (workgroup b takes base + (b < extra) pairs); the most pairs of one workgroup; dynamic LDS bytes of the pair launch }.  So
 * that a test which names a path proves it took that path.  n_nodes and population_size as for fcpp_ga_evolve. */
int fcpp_debug_ga_launch_plan(fcpp_ctx *ctx, int32_t n_nodes, int32_t population_size, int32_t *out);
/* fcpp_dubins_solve's function (csrc/fcpp_dubinsfn.h) evaluated on the HOST, on host pointers: what the device results are compared with
 * bit for bit, and what tests the mathematics on a machine without a GPU.  A diagnostic, not a fallback. */
int fcpp_debug_dubins(int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x, const double *to_y,
                      const double *to_h, double radius, int32_t *word, double *seg, double *len);
/* fcpp_rs_solve's function (csrc/fcpp_rsfn.h) evaluated on the HOST, on host pointers (seg: 5 per pair): what the device results are
 * compared with bit for bit, and what tests the mathematics on a machine without a GPU.  A diagnostic, not a fallback. */
int fcpp_debug_rs(int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x, const double *to_y,
                  const double *to_h, double radius, int32_t *word, double *seg, double *len);
/* The polygon swath rule (csrc/fcpp_swathfn.h) evaluated on the HOST, on host pointers, for both the scores and the cut: what the device
 * results are compared with bit for bit.  The angle of pair (i, j) is angles[i] when per_field (then A = 1), else angles[j]; n_swaths,
 * n_lines, length, status: n x A, any may be NULL.  out_offsets: NULL, or (A = 1) n + 1 CSR offsets of the fields' swaths; the records
 * below `cap` are written to ax .. seg_length (any may be NULL), so a first call with cap = 0 sizes the second.  The call's errors as
 * for fcpp_swath_scores.  A diagnostic, not a fallback. */
int fcpp_debug_swaths(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                      const double *y, int64_t A, const double *angles, int per_field, double W, double first, double min_length,
                      int32_t *n_swaths, int32_t *n_lines, double *length, int32_t *status, int64_t *out_offsets, int64_t cap, double *ax,
                      double *ay, double *bx, double *by, int32_t *line, double *seg_length);
/* The polygon inset rule (csrc/fcpp_insetfn.h) evaluated on the HOST, on host pointers, counts and fill in one call: what the device results
 * are compared with bit for bit.  pair_ring_offsets, pair_vert_offsets (n D + 1), status, gap (n D): any may be NULL.  Ring r of all is
 * written to out_vert_offsets while r < ring_cap (and the closing entry when the total fits), vertex v to out_x, out_y, out_src while
 * v < vert_cap: call once with caps of 0 for the sizes, then with them.  A diagnostic, not a fallback. */
int fcpp_debug_inset(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                     const double *y, int64_t D, const double *dist, double arc_step, int64_t *pair_ring_offsets, int64_t *pair_vert_offsets,
                     int32_t *status, double *gap, int64_t ring_cap, int64_t vert_cap, int64_t *out_vert_offsets, double *out_x, double *out_y,
                     int32_t *out_src);
/* The field cell rule (csrc/fcpp_cellfn.h) evaluated on the HOST, on host pointers, counts and fill in one call: what the device results are
 * compared with bit for bit.  cell_offsets, cell_vert_offsets (n + 1), status, n_cuts, dropped, dropped_area (n): any may be NULL.  Cell k of
 * all is written to out_vert_offsets, cell_field, area while k < cell_cap (and the closing offset when the total fits), vertex v to out_x,
 * out_y, out_src while v < vert_cap: call once with caps of 0 for the sizes, then with them.  The call's errors as for fcpp_cells_counts.
 * Fields are handed to the library's host threads; the results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_cells(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                     const double *y, const double *angle, int events, double min_area, int64_t *cell_offsets, int64_t *cell_vert_offsets,
                     int32_t *status, int32_t *n_cuts, int32_t *dropped, double *dropped_area, int64_t cell_cap, int64_t vert_cap,
                     int64_t *out_vert_offsets, double *out_x, double *out_y, int32_t *out_src, int32_t *cell_field, double *area);
/* The swath router's rule (csrc/fcpp_routefn.h) evaluated on the HOST, on host pointers: fcpp_route_transit's blocks and fcpp_route_solve's
 * results, what the device results are compared with bit for bit.  Arguments, outputs and the call's errors as for those two (the offsets
 * are the host's).  Fields are handed to the library's host threads; the results do not depend on their number.  Diagnostics, not fallbacks. */
int fcpp_debug_route_transit(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                             const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total, double *T);
int fcpp_debug_route(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                     const double *E, const double *X, int n_starts, double min_gain, int max_sweeps, int32_t *tours, double *costs, int32_t *route,
                     double *cost, int32_t *winner, int32_t *sweeps, int32_t *status, double *stored);
/* The cell tour's rule (csrc/fcpp_tourfn.h) evaluated on the HOST, on host pointers, transit and solve in one call: what the device
 * results are compared with bit for bit.  Arguments, outputs and the call's errors as for fcpp_cell_tour_transit / _solve (the offsets are
 * the host's); D (d_total float64) is an output too and may be NULL like the others.  Fields are handed to the library's host threads; the
 * results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_cell_tour(int64_t n, const int64_t *cell_offsets, int64_t n_cells, const int64_t *var_offsets, int64_t n_vars, const double *ix,
                         const double *iy, const double *ih, const double *ox, const double *oy, const double *oh, const double *w,
                         const int32_t *stored_node, double radius, int mode, const int64_t *d_offsets, int64_t d_total, double *D, const double *E,
                         const double *X, int n_starts, double min_gain, int max_sweeps, int32_t *order, int32_t *node, double *cost, double *stored,
                         double *joint_length, int32_t *winner, int32_t *sweeps, int32_t *skipped, int32_t *status, int32_t *tours, double *costs);
/* The service trips' rule (csrc/fcpp_tripfn.h) evaluated on the HOST, on host pointers: what fcpp_trip_solve is compared with bit for
 * bit.  Arguments, outputs and the call's errors as for it (the offsets are the host's).  Fields are handed to the library's host
 * threads; the results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_trip_solve(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                          const double *length, const double *E, const double *X, const double *In, const double *Out, int n_cand,
                          const int32_t *tours, int both_ways, const double *capacity, const double *first_capacity, double stop_cost,
                          int32_t *tour, int32_t *trip, int32_t *n_trips, int32_t *overfull, int32_t *winner, int32_t *status, double *cost,
                          double *base, double *extra, double *costs);
/* The vehicle shares' rule (csrc/fcpp_fleetfn.h) evaluated on the HOST, on host pointers: what fcpp_fleet_solve is compared with bit for
 * bit.  Arguments, outputs and the call's errors as for it (the offsets are the host's).  Fields are handed to the library's host
 * threads; the results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_fleet_solve(int64_t n, const int64_t *swath_offsets, int64_t n_total, const int64_t *t_offsets, int64_t t_total, const double *T,
                           const double *length, const double *In, const double *Out, int n_cand, const int32_t *tours, int both_ways,
                           const int32_t *vehicles, int k_stride, double work_weight, int32_t *tour, int32_t *share, int32_t *n_used,
                           int32_t *winner, int32_t *status, double *makespan, double *total, double *makespans, double *totals,
                           int32_t *share_first, double *share_cost);
/* The clearance rule (csrc/fcpp_clearfn.h) evaluated on the HOST, on host pointers: what fcpp_conn_clear and fcpp_route_transit_clear are
 * compared with bit for bit.  Arguments, outputs and the call's errors as for those two (the offsets are the host's).  Paths and fields
 * are handed to the library's host threads; the results do not depend on their number.  Diagnostics, not fallbacks. */
int fcpp_debug_conn_clear(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, double radius,
                          const int32_t *word, const double *seg, const int64_t *pair_field, int64_t n_fields, const int64_t *ring_offsets,
                          int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x, const double *y, int32_t *crossings,
                          int8_t *inside, double *first_s, int32_t *field_status);
int fcpp_debug_route_transit_clear(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                   const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total,
                                   const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                   const double *y, double penalty, double *T, uint8_t *B);
/* The priced transit block evaluated on the HOST, on host pointers: what fcpp_route_transit_priced is compared with bit for bit -- per
 * canonical pair the sequential form of the clear-connector rule (fcpp_debug_conn_solve_clear's) on the poses fcpp_debug_route_transit
 * solves.  Arguments, outputs and the call's errors as for it (the offsets are the host's); K may be NULL.  A diagnostic, not a fallback. */
int fcpp_debug_route_transit_priced(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                    const double *by, const double *angle, double radius, int mode, const int64_t *t_offsets, int64_t t_total,
                                    const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                    const double *y, double penalty, double *T, int8_t *K);
/* The clear-connector rule (csrc/fcpp_solveclearfn.h) evaluated on the HOST, on host pointers.  fcpp_debug_conn_words: ALL candidates of
 * every pair -- ok (uint8), total (float64): n x W, seg: n x W x S float64, W = 6, S = 3 (mode 0) or W = 48, S = 5 (mode 1); a word that is
 * no candidate has ok 0 and NaN.  Any output may be NULL.  Test infrastructure only.  fcpp_debug_conn_solve_clear: what
 * fcpp_conn_solve_clear is compared with bit for bit; arguments, outputs and the call's errors as for it (the offsets are the host's).
 * Pairs are handed to the library's host threads; the results do not depend on their number.  Diagnostics, not fallbacks. */
int fcpp_debug_conn_words(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                          const double *to_y, const double *to_h, double radius, uint8_t *ok, double *seg, double *total);
int fcpp_debug_conn_solve_clear(int mode, int64_t n, const double *from_x, const double *from_y, const double *from_h, const double *to_x,
                                const double *to_y, const double *to_h, double radius, const int64_t *pair_field, int64_t n_fields,
                                const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                                const double *y, int32_t *word, double *seg, double *len, int32_t *rank, int32_t *crossings,
                                int32_t *field_status);
/* The field-path rule (csrc/fcpp_fpathfn.h) evaluated on the HOST, on host pointers, counts and fill in one call: what the device results
 * are compared with bit for bit.  Arguments and the call's errors as for fcpp_field_path_counts / _fill.  path_offsets (n + 1), leg_offsets
 * (2 n_total + n + 1), work_length, transit_length, status (n): any may be NULL.  leg_word, leg_seg (5 each), leg_total (2 n_total + n slots,
 * any may be NULL): every slot's record -- a connector's word, segments and total as fcpp_debug_dubins / fcpp_debug_rs give them; a swath's
 * end point and length in seg[0 .. 2], word -1; zeros and -1 for a slot without a leg.  Sample q of all is written to x .. leg (any may be NULL)
 * while q < cap: call once with cap = 0 for the sizes, then with them.  Fields are handed to the library's host threads; the results do
 * not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_field_paths(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                           const double *by, const double *length, const double *angle, const int32_t *order, double radius, int mode,
                           double spacing, const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x,
                           const double *exit_y, const double *exit_h, int64_t *path_offsets, int64_t *leg_offsets, double *work_length,
                           double *transit_length, int32_t *status, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap,
                           double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg);
/* The clear field-path rule evaluated on the HOST, counts and fill in one call like fcpp_debug_field_paths: what
 * fcpp_field_path_counts_clear / _fill_clear are compared with bit for bit.  Arguments, outputs and the call's errors as for them (the
 * offsets are the host's); it applies the sequential form of the clear-connector rule to every connector slot.  A diagnostic, not a
 * fallback. */
int fcpp_debug_field_paths_clear(int64_t n, const int64_t *swath_offsets, int64_t n_total, const double *ax, const double *ay, const double *bx,
                                 const double *by, const double *length, const double *angle, const int32_t *order, double radius, int mode,
                                 double spacing, const double *entry_x, const double *entry_y, const double *entry_h, const double *exit_x,
                                 const double *exit_y, const double *exit_h, const int64_t *ring_offsets, int64_t n_rings,
                                 const int64_t *vert_offsets, int64_t n_verts, const double *region_x, const double *region_y,
                                 int64_t *path_offsets, int64_t *leg_offsets, double *work_length, double *transit_length, int32_t *status,
                                 int32_t *leg_rank, int32_t *leg_crossings, int32_t *leg_word, double *leg_seg, double *leg_total,
                                 int32_t *blocked, int32_t *reshaped, int32_t *region_status, int64_t cap, double *x, double *y,
                                 double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg);
/* The headland-path rule (csrc/fcpp_hpathfn.h) evaluated on the HOST, on host pointers, counts and fill in one call: what the device
 * results are compared with bit for bit.  Arguments and the call's errors as for fcpp_headland_path_counts / _fill.  path_offsets
 * (n_rings + 1), leg_offsets (2 n_verts + 1), work_length, transit_length, skipped_length, status (n_rings): any may be NULL.  leg_kind,
 * leg_word (int32), leg_seg (5 each), leg_total (2 n_verts slots, any may be NULL): every slot's record -- kind 0 no leg, 1 a straight
 * element (its end point and length in seg[0 .. 2]), 2 / 3 a Dubins / Reeds-Shepp connector (word, segments and total as fcpp_debug_dubins /
 * fcpp_debug_rs give them), 4 a followed arc (end point, length, curvature in seg[0 .. 3]), 5 a skipped arc (total = d D); word -1 for all
 * but connectors.  Sample q of all is written to out_x .. leg (any may be NULL) while q < cap: call once with cap = 0 for the sizes, then
 * with them.  Rings are handed to the library's host threads; the results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_headland_paths(int64_t n_rings, const int64_t *ring_offsets, int64_t n_verts, const double *x, const double *y, const int32_t *src,
                              const double *ring_dist, double radius, int mode, double spacing, int direction, double smooth_tol,
                              int64_t *path_offsets, int64_t *leg_offsets, double *work_length, double *transit_length, double *skipped_length,
                              int32_t *status, int32_t *leg_kind, int32_t *leg_word, double *leg_seg, double *leg_total, int64_t cap,
                              double *out_x, double *out_y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *leg);
/* The polygon-coverage rule (csrc/fcpp_pcoverfn.h) evaluated on the HOST, on host pointers, sizes and cover in one call: what the device
 * results are compared with bit for bit.  Arguments and the call's errors as for fcpp_polygon_cover_sizes / fcpp_polygon_cover.  dims
 * (n records of 32 bytes), cell_offsets (n + 1), status (n): any may be NULL.  counts (4 n) NULL: the sizes only, the paths are not read.
 * grid (may be NULL) is written when all cells fit in cell_cap: call once without it for the sizes, then with it.  Fields are handed to
 * the library's host threads; the results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_polygon_cover(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                             const double *y, double width, double res, int caps, int64_t n_paths, const int64_t *path_offsets,
                             int64_t total_points, const double *px, const double *py, const uint8_t *work, const int32_t *pass,
                             const int64_t *field_path_offsets, const int64_t *path_ids, void *dims, int64_t *cell_offsets, int64_t cell_cap,
                             uint8_t *grid, int64_t *counts, int32_t *status);
/* The coverage-region rule (csrc/fcpp_regionfn.h) evaluated on the HOST, on host pointers, counts and fill in one call: what the device
 * results are compared with exactly -- a sequential two-pass union-find per field over the same member and neighbour functions (the result
 * is unique, so the order of work does not show).  Arguments and the call's errors as for fcpp_cover_regions_counts.  region_offsets
 * (n + 1), labels_counts, labels_fill (one int32 per cell: the labels after the counts call / after the fill call): any may be NULL.
 * records (may be NULL) is written when all regions fit in region_cap: call once with 0 for the sizes, then with them.  Fields are handed
 * to the library's host threads; the results do not depend on their number.  A diagnostic, not a fallback. */
int fcpp_debug_cover_regions(int64_t n, const void *dims, const int64_t *cell_offsets, const uint8_t *grid, int mask, int value, int connectivity,
                             int64_t *region_offsets, int64_t region_cap, void *records, int32_t *labels_counts, int32_t *labels_fill);
/* The patch-pass rule (csrc/fcpp_patchfn.h) evaluated on the HOST, on host pointers, sizes, counts and fill in one call: what the device
 * results are compared with, every value equal.  Arguments and the call's errors as for fcpp_patch_sizes.  frame (2 n), records
 * (64 bytes per region), totals (3: lines, bitmap words, swaths), swath_offsets (n + 1): any may be NULL.  bitmap is written when the
 * words fit in word_cap, line_counts and line_offsets (lines + 1) when the lines fit in line_cap, the swath arrays when the swaths fit in
 * swath_cap: call once with 0 for the totals, then with them.  Fields are handed to the library's host threads; the results do not depend
 * on their number.  A diagnostic, not a fallback. */
int fcpp_debug_patch_swaths(int64_t n, const void *dims, const int64_t *cell_offsets, double res, const int32_t *labels, const int64_t *region_offsets,
                            int64_t n_regions, const double *angle, double width, double margin, double join, double *frame, void *records,
                            int64_t *totals, int64_t word_cap, uint64_t *bitmap, int64_t line_cap, int64_t *line_counts, int64_t *line_offsets,
                            int64_t *swath_offsets, int64_t swath_cap, double *ax, double *ay, double *bx, double *by, int32_t *line,
                            double *length, int64_t *region);
/* One of a batch's device tables copied to the host (dst = NULL: only its size in *bytes_out): 0 field descriptors, 1 primitives, 2 tiles,
 * 3 wave tiles, 4 general tile ids, 5 chunks, 6 span chunks, 7 statistics entry -> tile, 8 first entry per field, 9 run length per entry,
 * 10 reduction lists, 11 field work, 12 open wave tile ids, 13 connector segments, 14 connector masks, 15 statistics slots (after batch
 * creation: the closed-form statistics of the quiet runs), 16 junction constants, 17 run totals per field of field work, 18-21 obstacle
 * offsets / x / y / bounding boxes, 22 the packs of k_plan_sparse_fields.  tests/test_gpu_devplan.py compares the tables of a batch set up on the device with those of the
 * same batch set up on the host. */
int fcpp_batch_debug_table(const fcpp_batch *batch, int table, void *dst, int64_t cap_bytes, int64_t *bytes_out);
/* The direct step of fcpp_batch_plan on this context so far (the step of a speculative device setup enqueued right behind the counting pass,
   before the host has the totals: batches without obstacle polygons; FCPP_DIRECT=0 switches the path off).  launched: steps enqueued;
   taken: of those, the calls whose batch qualified -- no fill pass and no fcpp_batch_run in the call; fills: fill passes of taken batches
   enqueued since, because somebody asked for the tables or another setup took the plan slot.  Any pointer may be NULL.  Tests. */
int fcpp_ctx_direct_steps(const fcpp_ctx *ctx, int64_t *launched, int64_t *taken, int64_t *fills);
/* Direct setups on this context so far whose counting pass took its row form (two fields per wavefront, 32 lanes each; FCPP_CUT_ROWS=0
   keeps the form of a wavefront per field, which is its checker).  Tests. */
int fcpp_ctx_cut_rows_passes(const fcpp_ctx *ctx, int64_t *passes);

#ifdef __cplusplus
}
#endif
#endif /* FCPP_H */
