// fcpp_setuprule.h -- every decision of a batch's device setup (fcpp_setup.cpp: DeviceSetup) as a function of plain values: which batches the
// device takes, how a setup begins (speculative layout, direct step), how it ends once the totals are there, and which of a plan slot's two
// buffers of aggregates it adds into.  Plain C++, no HIP: the setup reads its decisions here and nowhere else, and fcpp_debug_setup_rule
// evaluates the same functions on a machine without a GPU (tests/test_setup_rule_host.py).
#pragma once
#include <stdint.h>

#include "../../include/fcpp.h"

namespace fcpp {

// ---- accept or decline.  The declines in the order they are looked at; the first that holds is the answer.
enum SetupDecline : int {
    SETUP_ACCEPT = 0,
    SETUP_HOST_REQUESTED,     // FCPP_SETUP_HOST
    SETUP_EMPTY,              // no field
    SETUP_HANDFUL,            // FCPP_SETUP_AUTO and fewer fields than the small-batch threshold
    SETUP_OBSTACLE_MODE,      // obstacle-aware swaths
    SETUP_NO_FIELD_WORK,      // FCPP_FIELD_WORK=0
    SETUP_PRIMS               // more primitives per field than the device planner holds
};
struct SetupAcceptIn {
    int setup_mode;           // FCPP_SETUP_AUTO / _HOST / _DEVICE
    int64_t n_fields;
    int64_t small_batch;      // fields below which `auto` takes the host (FCPP_SMALL_BATCH, default 16)
    int obstacle_mode;
    bool field_work;
    int max_prims, prims_cap; // PlanConsts.max_prims (0: not planned yet -- the declines in front of plan_prepare) against DEVPLAN_PRIMS_CAP
};
// (a handful of fields: the device's chain of five dependent launches costs ~110 us whatever the batch, the host's plan + tiler + one copy
// ~65 us + 3 us per field -- a single 500 x 200 m planner's plan call 0.49 -> 0.44 ms)
inline SetupDecline setup_accept(const SetupAcceptIn &in)
{
    if (in.setup_mode == FCPP_SETUP_HOST) return SETUP_HOST_REQUESTED;
    if (in.n_fields <= 0) return SETUP_EMPTY;
    if (in.setup_mode == FCPP_SETUP_AUTO && in.n_fields < in.small_batch) return SETUP_HANDFUL;
    if (in.obstacle_mode != FCPP_OBSTACLES_FLAG) return SETUP_OBSTACLE_MODE;
    if (!in.field_work) return SETUP_NO_FIELD_WORK;
    if (in.max_prims > in.prims_cap) return SETUP_PRIMS;
    return SETUP_ACCEPT;
}
inline const char *setup_decline_text(SetupDecline d)
{
    switch (d) {
    case SETUP_HOST_REQUESTED: return "host setup requested";
    case SETUP_EMPTY: return "empty batch";
    case SETUP_HANDFUL: return "a handful of fields: set up by the host";
    case SETUP_OBSTACLE_MODE: return "obstacle-aware swaths are planned on the host";
    case SETUP_NO_FIELD_WORK: return "FCPP_FIELD_WORK=0: the host tiler's reference path";
    case SETUP_PRIMS: return "too many headland loops for the device planner";
    default: return "";
    }
}

// ---- how a setup begins.  spec: the SPECULATIVE layout (fcpp_setup.cpp: capacity_layout), tables laid out by per-field capacities before
// anything has run, for batches of the counting phase's one-scan form whose capacity layout stays within 1 GiB.  direct: fcpp_batch_plan's
// direct step -- outputs are wanted, no obstacle polygons, fused spans -- attempted while the context's last speculative setup qualified for it
// (direct_ok) and FCPP_DIRECT does not switch it off.
struct SetupBeginIn {
    int64_t n_fields;
    int64_t small_blocks;     // devplan_small_blocks(): blocks of 1024 fields up to which ONE scan serves
    bool exact_only;          // FCPP_SETUP_EXACT
    bool dense;               // sample_spacing != 0
    uint64_t capacity_bytes;  // the capacity layout's size (looked at only when setup_wants_capacities)
    bool outputs, no_polys, fuse_spans, direct_ok, direct_switch;
};
struct SetupBegin { bool spec, direct; };
constexpr uint64_t kSpecBytesMax = (uint64_t)1 << 30;
// is the capacity layout worth computing at all?
inline bool setup_wants_capacities(const SetupBeginIn &in)
{
    return (in.n_fields + 1023) / 1024 <= in.small_blocks && !in.exact_only && !in.dense;
}
inline SetupBegin setup_begin(const SetupBeginIn &in)
{
    SetupBegin r;
    r.spec = setup_wants_capacities(in) && in.capacity_bytes <= kSpecBytesMax;
    r.direct = in.outputs && r.spec && in.no_polys && in.fuse_spans && in.direct_ok && in.direct_switch;
    return r;
}

// ---- how a setup ends: the totals are on the host.
// fuse: the spans of fields of field work are written by the fields' own workgroups (k_plan_sparse_fields) when ALL of them are short enough for
// that -- the span launch of such a batch disappears -- and by k_plan_quiet otherwise (a mix loses: measured on cfg2 at the reference's
// sampling, a third of its spans fusable, 0.0435 instead of 0.0392 ms).
// within: the speculative layout held.  Else the batch gets the exact layout.
// qualifies: the batch rule of the direct step, as its workgroups applied it: every field a field of field work, every span fused, no flag up.
// taken: the direct step has planned the batch (the arrays were sized for the final point total): no fill pass until somebody asks for the tables.
// refill: the direct step declined a batch within its capacities: the fill pass follows, its publisher off.
struct SetupEndIn {
    bool spec, direct_step;
    int64_t early_points;     // what the direct step's arrays were sized for
    int64_t unfusable, work_span_pts, work, points;      // totals: PC_UNFUSABLE, PC_WORK_SPAN_PTS, PC_WORK, PC_POINTS
    int64_t over_capacity;    // the flag PF_OVER_CAPACITY: the generation that raised it last
    int64_t gen, n_fields;
    bool fuse_spans, no_polys;
};
struct SetupEnd { bool fuse, within, qualifies, taken, refill; };
inline SetupEnd setup_end(const SetupEndIn &in)
{
    SetupEnd r;
    r.fuse = in.fuse_spans && in.unfusable == 0 && in.work_span_pts > 0;
    r.within = in.spec && in.over_capacity != in.gen;
    r.qualifies = r.within && r.fuse && in.work == in.n_fields && in.no_polys;
    r.taken = in.direct_step && r.qualifies && in.points == in.early_points;
    r.refill = in.direct_step && !r.taken && r.within;
    return r;
}

// ---- a plan slot's two buffers of aggregates (fcpp_offsetfn.h; DevPlanScratch.agg / agg_next).
// The aggregates of the two levels are cleared by NO command in the stream: the slot has two buffers, a speculative setup adds into one (zero:
// the slot's allocation or the fill pass of its last speculative setup left it so) and its fill pass -- or its direct step's publisher --, which
// runs whatever the flags say, zeroes the other for the next.  Only a setup that ends between its first launch and that pass (a launch error)
// leaves them unknown: the slot stays dirty, and both buffers are cleared in front of its next speculative setup, which starts at the first.
struct AggBegin { bool clear_both, use_second; };
struct SlotAggregates {
    int agg_flip = 0;         // which buffer the next speculative setup adds into
    bool agg_dirty = false;   // a setup began and has not settled
    // a speculative setup begins: clear both buffers first? add into the second (swap agg / agg_next)?  Leaves the slot dirty and flipped.
    AggBegin begin_aggregates()
    {
        AggBegin r;
        r.clear_both = agg_dirty;
        if (agg_dirty) agg_flip = 0;
        r.use_second = agg_flip != 0;
        agg_flip ^= 1;
        agg_dirty = true;
        return r;
    }
    // the pass that zeroes the other buffer is in the stream
    void aggregates_settled() { agg_dirty = false; }
};

}  // namespace fcpp
