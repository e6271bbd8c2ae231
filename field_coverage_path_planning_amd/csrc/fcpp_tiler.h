// fcpp_tiler.h -- the host-side tiler of the fused pipeline: cuts every field's path into work for the four single-pass kernels
// (spans and closed-form runs for k_plan_quiet, wave tiles for k_plan_sparse, general tiles for k_plan_fused) plus the lists
// k_reduce_stats walks, and lays all of it out as ONE image that goes to the device in one copy.
//
// Pure C++ (no HIP): fields are tiled block by block on the host's cores (fcpp_parallel.h), the blocks' records are merged in block
// order, so the image does not depend on the thread count.  A field's cut depends on the field alone, never on its position in the
// batch; only indices (field, tile slot, primitive, output offset) differ between two equal fields.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "fcpp_internal.h"
#include "fcpp_slab.h"
#include "fcpp_tilefn.h"
#include "fcpp_cutfn.h"

namespace fcpp {

// what this tiler and the device's (fcpp_devplan.h: DevTileConsts) both derive from the batch: computed once per batch (fcpp_setup.cpp: batch_tile_consts)
struct BatchTileConsts {
    int nu = 0, nc = 0;                       // samples of the U-turn / corner templates
    bool turn_quiet = false;                  // U-turns of this batch are closed form (closed_form_turns, fcpp_setup.cpp)
    double two_a = 0.0, u_cap = 0.0, c_line = 0.0;     // 2 a_lon, (v_max / 3.6)^2, (v_work / 3.6)^2
    double fence_margin = 1e-7;               // a point whose edge functions are all at least this cannot be flagged by the device's geofence test (1e-7 - geofence_tol)
    static constexpr int wave_factor = 24;    // wave tiles where wave_factor * 2a * line step >= u_cap
    bool fuse_spans = true;                   // a field of field work's workgroup also writes the field's layer-1 span (its chunks are then not in k_plan_quiet's list)
    // a field's complete passes (line + closed-form U-turn) form ONE span -- one run, one statistics entry, chunks decoded by (pass, offset) -- when
    // its lines' quiet zones are shorter than span_line_max; fields with obstacles keep 64 (their lines and turns stay runs of their own: a line's
    // chunks test the obstacles once per line, a span's chunks pair by pair -- cfg3: 0.36 vs 0.43 ms a step).  Round 5: unlimited for fields without
    // obstacles, whatever the sampling -- 2P - 1 runs per field become one (cfg2 at 0.5 m: a 20 MB image -> 6 MB, the plan call 3.1 -> 2.4 ms,
    // the step itself 1.23 -> 1.10 ms); FCPP_DENSE_SPAN=0 keeps round 4's runs (the reference of the sliced reduction's test).
    int64_t span_line_max = INT64_MAX;
};

// what the tiler needs to know about the batch besides the host plan
struct TileConsts : BatchTileConsts {
    const Pt2 *tu = nullptr, *tc = nullptr;   // host copies of the U-turn / corner templates (nu / nc samples)
    bool templates_ok = false;                // the copies are there (wave tiles need them to size their halos)
    bool field_work = true;                   // fields with few wave tiles and nothing else general: planned and reduced by one workgroup (DevFieldWork)
    static constexpr int64_t reduce_wg_max = 1024;     // statistic entries one workgroup reduces; beyond: 64 workgroups + join
    bool closed_cut = false;                  // reference sampling: the general stretch of a field with a closed-form span is cut by fcpp_cutfn.h (as the device planner cuts it)
    CutConsts cut = {};                       // ... with these constants (host copies of the templates and their chord tables)
    bool device_chunks = false;               // the chunk lists of k_plan_quiet are expanded on the device from chunk groups (fcpp_batch_create; false: written by the host, the checker)
};

// the obstacle part of the image (also used by the device-side setup, fcpp_setup.cpp)
// (rebase: dst holds the image from byte `rebase` on -- the obstacle region alone when rebase = lay.obs_off)
void fill_obstacles(const fcpp_polys *polys, const ImageLayout &lay, unsigned char *dst, size_t rebase = 0);

struct BlockTiles;      // a block's records before the merge (fcpp_tiler.cpp)

class BatchTiler {
public:
    BatchTiler();
    ~BatchTiler();
    // phase 1: tile every block of `hp` (side by side), size the image.  `polys` (may be NULL): the batch's obstacle table, copied into
    // the image with one bounding box per polygon.
    int plan(const HostPlan &hp, const TileConsts &tc, const fcpp_polys *polys, ImageLayout &lay, std::string &err);
    // phase 2: write the image into `dst` (lay.upload_bytes bytes; pinned host memory in fcpp_batch_create), side by side
    void fill(const HostPlan &hp, const fcpp_polys *polys, const ImageLayout &lay, unsigned char *dst) const;
private:
    int plan_impl(const HostPlan &hp, const TileConsts &tc, const fcpp_polys *polys, ImageLayout &lay, std::string &err);
    std::vector<BlockTiles> *blocks_;
};

}  // namespace fcpp
